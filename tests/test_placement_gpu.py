"""Placed restarts (phys_batch_place_configure + phys_batch_end_episodes) on the MI355X: the device's kernel against the numpy
restatement of the header's definition (tests/placement_check.py) with the comparison and the near-border condition of the CPU suite,
the height scan of the placed envs, the identity placement against the unplaced kernel, the configure call's refusals, and a bank whose
second terrain is a plateau: restarted onto it, the robots stand on it instead of inside it.  The CPU counterpart -- the same kernel on
the wave emulator -- is tests/test_placement.py, whose cases these tests share."""

import numpy as np
import pytest

import episode_check as ec
import placement_check as pc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd._lib import lib
from test_episodes import RULES
from test_placement import GROUND_REF, check_scan_consistency, copy_place, footprint, make_case, random_poses

pytestmark = pytest.mark.gpu

NENV = 70
RANGES = [(0, 35), (35, 35)]
FIELDS = (("qpos", P.F_QPOS), ("qvel", P.F_QVEL), ("sensordata", P.F_SENSORDATA), ("actuator_velocity", P.F_ACTUATOR_VELOCITY),
          ("qacc", P.F_QACC), ("qacc_warmstart", P.F_QACC_WARMSTART), ("ctrl", P.F_CTRL), ("time", P.F_TIME))
EPISODE = (("done", P.EP_DONE), ("reason", P.EP_REASON), ("steps", P.EP_STEPS), ("count", P.EP_COUNT), ("terminal", P.EP_TERMINAL))


def load(c, placed=True, scan=False):
    """The case on the device: state uploaded, per-env geometry through randomize, the bank of terrains, the episode arrays, the terrain
    index and the three placement arrays bound as torch tensors; end_episodes over two ranges on two streams -> (state, place, scan)."""
    import torch
    model, pod, s, pl = c["model"], c["pod"], c["state"], copy_place(c["place"])
    n = len(s["qpos"])
    b = Batch(model, n)
    try:
        keep = {}
        if pl["grids"] is not None:
            b.set_hfield_bank(pl["grids"])
            keep["index"] = torch.from_numpy(pl["index"].copy()).cuda()
            b.bind_terrain_index(keep["index"].data_ptr())
        if pl["geom_pos"] is not None:
            b.randomize(P.P_GEOM_POS, pl["geom_pos"].reshape(n, -1))
            b.randomize(P.P_GEOM_QUAT, pl["geom_quat"].reshape(n, -1))
        for k, f in FIELDS:
            b.set(f, s[k])
        b.enable_episodes(**RULES)
        for k, which in EPISODE:
            keep[k] = torch.from_numpy(s[k].copy()).cuda()
            b.bind_episode(which, keep[k].data_ptr())
        b.set_reset_bank(c["bank"])
        if placed:
            b.configure_placement(pl["anchor"], pl["footprint"], pl["ground_ref"])
            keep["pose"], keep["ground"] = torch.from_numpy(pl["pose"].copy()).cuda(), torch.from_numpy(pl["ground"].copy()).cuda()
            b.bind_placement(P.PLACE_POSE, keep["pose"].data_ptr())
            b.bind_placement(P.PLACE_GROUND, keep["ground"].data_ptr())
            assert b.placement_ptr(P.PLACE_POSE) == keep["pose"].data_ptr() and not b.placement_ptr(P.PLACE_NEXT_TERRAIN)
            if pl["nxt"] is not None:
                keep["nxt"] = torch.from_numpy(pl["nxt"].copy()).cuda()
                b.bind_placement(P.PLACE_NEXT_TERRAIN, keep["nxt"].data_ptr())
        pick_d, force_d = torch.from_numpy(c["pick"]).cuda(), torch.from_numpy(c["force"]).cuda()
        b.sync()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for (e0, cnt), st in zip(RANGES, streams):
            b.end_episodes(e0, cnt, True, pick_ptr=pick_d.data_ptr() + 4 * e0, force_ptr=force_d.data_ptr() + 4 * e0, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        got = {k: b.get(f).reshape(s[k].shape) for k, f in FIELDS}
        got["warn"] = b.warnings()[0]
        got["meas"] = got["drive"] = None
        for k, _ in EPISODE:
            got[k] = keep[k].cpu().numpy()
        if placed:
            pl["ground"] = keep["ground"].cpu().numpy()
            assert np.array_equal(b.placement_ground(), pl["ground"]) and np.array_equal(keep["pose"].cpu().numpy(), pl["pose"])
        if "index" in keep:
            pl["index"] = keep["index"].cpu().numpy()
        values = None
        if scan:
            b.configure_scan(pl["footprint"], pl["anchor"], 10.0)
            for (e0, cnt), st in zip(RANGES, streams):
                b.height_scan(e0, cnt, stream=st.cuda_stream)
            b.sync()
            values = b.get(P.F_HEIGHT_SCAN)
        return got, pl, values
    finally:
        b.close()


def reference(c):
    s, pl = ec.copy_state(c["state"]), copy_place(c["place"])
    ended, nears = [], []
    for e0, cnt in RANGES:
        _, envs, near = pc.end_episodes(s, c["pod"], RULES, e0, cnt, True, c["bank"], pl, pick=c["pick"][e0:e0 + cnt], force=c["force"][e0:e0 + cnt])
        ended.append(envs); nears.append(near)
    return s, pl, np.concatenate(ended), np.concatenate(nears)


@pytest.mark.parametrize("name,npoints", [("cassie_hfield", 70), ("cassie_tray_box", 5)])
def test_placed_restart_on_the_device_matches_the_definition_and_its_scan(built, name, npoints):
    """70 envs as two ranges on two streams, pose / next-terrain / ground arrays bound as torch tensors: the comparison and the
    near-border condition of tests/test_placement.py (test 2), then the height scan of the placed envs with the footprint as its
    pattern (test 4)."""
    c = make_case(name, npoints, drive=False, nenv=NENV, env0=0, n=NENV)
    if c["place"]["grids"] is None:                              # next terrains bound with no bank set: ignored
        c["place"]["nxt"] = np.full(NENV, 9, dtype=np.int32)
    want, want_place, envs, near = reference(c)
    assert 20 <= len(envs) <= 50
    got, got_place, values = load(c, scan=True)
    pc.compare(got, want, got_place, want_place, c["pod"], envs, near, "%s on the device, %d points" % (name, npoints))
    if name == "cassie_hfield":
        sp = c["special"]
        assert got["warn"][sp["off"]] == P.WARN_PLACE_MISS and got["warn"][sp["tilted"]] == P.WARN_SCAN_TILTED | P.WARN_PLACE_MISS
        assert got["warn"][sp["below"]] & P.WARN_TERRAIN_INDEX and got_place["index"][sp["above"]] == 3
    check_scan_consistency(c, want_place, envs, near, got["qpos"], got["warn"], values)


@pytest.mark.parametrize("name", ["cassie", "cassie_tray_box"])
def test_identity_placement_on_the_device(built, name):
    """The pose (0, 0, 0, 0) with no footprint against a batch that never configured placement: every array equal."""
    c = make_case(name, 1, drive=False, nenv=NENV, env0=0, n=NENV)
    c["place"].update(pose=np.zeros((NENV, 4)), footprint=None, geom_pos=None, geom_quat=None)
    plain, _, _ = load(c, placed=False)
    placed, pl, _ = load(c, placed=True)
    for k in plain:
        if plain[k] is None:
            assert placed[k] is None
        else:
            assert np.array_equal(plain[k], placed[k]), k
    assert plain["done"].sum() > 20
    assert np.all(pl["ground"][plain["done"] != 0] == GROUND_REF[name])


def test_configure_errors(built):
    """Each returns -1 with a message: a body that is not a root, 1025 points, per-env models."""
    model = Model("cassie")
    pod = model.pod
    pelvis = int(pod.root_body[0])
    b = Batch(model, 4)
    try:
        L = lib()
        one = np.zeros((1, 2))
        assert L.phys_batch_place_configure(b._h, pelvis + 1, one.ctypes.data, 1, 0.0) == -1 and b"child of the world" in L.phys_last_error()
        many = np.zeros((1025, 2))
        assert L.phys_batch_place_configure(b._h, pelvis, many.ctypes.data, 1025, 0.0) == -1 and b"1024" in L.phys_last_error()
        with pytest.raises(ValueError, match="child of the world"):
            b.configure_placement(pelvis + 1, one)
        b.configure_placement(pelvis, one)                       # fine; and off again
        b.configure_placement(0)
        b.set_model(pod, env=1)
        assert L.phys_batch_place_configure(b._h, pelvis, one.ctypes.data, 1, 0.0) == -1 and b"per-env models" in L.phys_last_error()
    finally:
        b.close()


def test_restart_onto_a_plateau(built):
    """A bank of two terrains: elevation 0 everywhere, and a plateau -- elevation 1 everywhere, hfield_size's whole height -- whose
    surface lies 0.3 m above the ground the bank's row was recorded on (the init pose, which stands on z = 0, lowered until it stands
    0.3 m below the plateau).  64 envs restart onto the plateau at random spots and headings: PHYS_PLACE_GROUND is the plateau's
    height within 1e-12, and after one policy step of 50 substeps every qpos and qvel is finite and no env has WARN_DIVERGED."""
    import torch
    model = Model("cassie_hfield")
    pod, n = model.pod, 64
    plateau = pod.geom_pos[pod.hfield_geom][2] + pod.hfield_size[2]      # (elevation 1.0 is exact in float32)
    ground_ref = plateau - 0.3
    grids = np.stack([np.zeros((pod.hfield_nrow, pod.hfield_ncol), dtype=np.float32), np.ones((pod.hfield_nrow, pod.hfield_ncol), dtype=np.float32)])
    row_q = model.qpos_init()
    row_q[2] += ground_ref                                         # stands on ground_ref as the init pose stands on 0
    b = Batch(model, n)
    try:
        b.set_hfield_bank(grids)
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        b.enable_episodes()
        b.set_reset_bank(b.make_reset_bank(row_q[None]))
        b.configure_placement(int(pod.root_body[0]), footprint(5), ground_ref)
        pose = random_poses(np.random.default_rng(2), n)
        pose[:, 2] = 0.0
        b.set_placement(pose)
        nxt = torch.ones(n, dtype=torch.int32, device="cuda")
        force = torch.ones(n, dtype=torch.int32, device="cuda")
        b.bind_placement(P.PLACE_NEXT_TERRAIN, nxt.data_ptr())
        torch.cuda.synchronize()
        b.end_episodes(force_ptr=force.data_ptr())
        ground = b.placement_ground()
        assert np.max(np.abs(ground - plateau)) <= 1e-12
        q = b.get(P.F_QPOS)
        assert np.max(np.abs(q[:, 2] - (row_q[2] + 0.3))) <= 1e-12 and not b.warnings()[0].any()
        assert np.max(np.abs(q[:, 0:2] - (row_q[0:2] + pose[:, 0:2]))) <= 1e-12
        b.step(50)
        q, v, w = b.get(P.F_QPOS), b.get(P.F_QVEL), b.warnings()[0]
        assert np.isfinite(q).all() and np.isfinite(v).all() and not (w & P.WARN_DIVERGED).any()
        # (25 ms: free fall is 3 mm; a robot put down INSIDE the plateau would be thrown out of it)
        assert np.max(np.abs(q[:, 2] - (row_q[2] + 0.3))) < 0.05 and abs(50 * pod.timestep - 0.025) < 1e-12
    finally:
        b.close()
