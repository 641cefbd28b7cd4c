"""Probes on the MI355X (phys_batch_probe: a forward pass into the probes' own read-out block, then cassie_probe_kernel): against the
definition restated from the oracle's state (tests/probes_check.py, the cases and tolerances of tests/test_probes.py), against the
drop-in's single-simulator getters, queued into the two-range, two-stream loop in DRIVE_PD_SAFE without disturbing one byte of it,
on env ranges with strided and bound outputs, and the counters and refusals of the entry points."""
import ctypes
import os

import numpy as np
import pytest

import bench
import probes_check as pc
import probes_emu_py as pe
import randomise_check as rc
import terrain_check as tc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd._lib import REPO_DIR, lib
from test_episodes_gpu import bank_states, drive_bytes, make
from test_probes import BODY, ROWS, SITE, cassie_probes, cassie_states, own_masses

pytestmark = pytest.mark.gpu

STATE_FIELDS = (P.F_QPOS, P.F_QVEL, P.F_QACC_WARMSTART, P.F_TIME, P.F_CTRL, P.F_QFRC_APPLIED, P.F_XFRC_APPLIED, P.F_QACC, P.F_SENSORDATA,
                P.F_ACTUATOR_VELOCITY, P.F_XPOS, P.F_XQUAT, P.F_PD_PTARGET, P.F_PD_KP, P.F_PD_KD, P.F_BODY_CFRC, P.F_DRIVE_CMD, P.F_MEAS,
                P.F_PD_DTARGET, P.F_PD_TORQUE)


def _probe_batch(model, q, v, ctrl, probes, quantities, prepare=None):
    """A fresh batch set to the states, probed once on its own stream -> (quantities, contact words, the batch's warning words)."""
    b = Batch(model, len(q))
    try:
        b.set(P.F_QPOS, q)
        b.set(P.F_QVEL, v)
        if ctrl is not None:
            b.set(P.F_CTRL, ctrl)
        if prepare:
            prepare(b)
        b.configure_probes(probes, quantities)
        b.probe()
        b.sync()
        assert b.get(P.F_QPOS).tobytes() == np.ascontiguousarray(q).tobytes() and not b.get(P.F_XPOS).any()     # (a fresh batch's poses: zeros, still)
        return b.probes(), b.probe_contacts() if quantities & P.PQ_CONTACTS else None, b.warnings()[0]
    finally:
        b.close()


# ------------------------------------------------------------------ 1. the device against the definition ----
def test_definition_on_cassie(cassie):
    """Case 1 of tests/test_probes.py: six envs (one with its own masses, through randomize + set_const), eight probes, every quantity."""
    q, v, ctrl = cassie_states(cassie)
    probes, classes = cassie_probes(cassie), pe.geom_classes(cassie)
    _, pods, params = own_masses("cassie", len(q), 5)

    def prepare(b):
        for f in ("body_mass", "body_ipos", "body_inertia"):
            b.randomize(rc.PARAM_IDS[f], params[f])
        b.set_const()

    got, words, warn = _probe_batch(cassie, q, v, ctrl, probes, P.PQ_ALL, prepare)
    assert not warn.any() and set(got) == set(pe.NAMES)
    pc.check_rows(pods, q, v, probes, got, ctrl=ctrl, words=words, classes=classes)
    assert np.all(got["cfrc"][0] == 0) and got["cfrc"][2, 1, 2] > 50 and words[3] == P.PC_SELF | P.PC_GROUP0 << 1
    assert not np.allclose(got["cfrc"][5], got["cfrc"][2], rtol=1e-3)


def test_definition_on_the_tray_model():
    """Case 3: a probe on the cube (its own tree root) and one on the tray; the cube sits on the tray."""
    m = Model("cassie_tray_box")
    pod = m.pod
    tray, cube = m.name2id(1, "tray"), pod.nbody - 1
    rng = np.random.default_rng(9)
    q = np.tile(np.array(pod.qpos0[: pod.nq]), (2, 1))
    o = pc.oracle_forward(pod, q[0], np.zeros(pod.nv))
    top = np.array(o.d.geom_xpos[[g for g in range(pod.ngeom) if pod.geom_bodyid[g] == tray][0]])
    qa = pod.jnt_qposadr[pod.body_jntadr[cube]]
    q[:, qa: qa + 3] = top + [[0, 0, 0.054], [0.01, -0.02, 0.053]]
    v = rng.uniform(-0.3, 0.3, (2, pod.nv))
    probes = [(BODY, cube, [0, 0, 0]), (BODY, cube, [0.05, 0.05, -0.05]), (BODY, tray, [0, 0, 0]), (BODY, tray, [0.1, 0, 0.005])]
    classes = pe.geom_classes(m)
    got, words, warn = _probe_batch(m, q, v, None, probes, P.PQ_ALL)
    assert not warn.any()
    pc.check_rows(pod, q, v, probes, got, words=words, classes=classes)
    for e in range(2):
        assert abs(got["cfrc"][e, 0, 2]) > 50 and np.allclose(got["cfrc"][e, 0], -got["cfrc"][e, 2], **pc.FORCE_TOL) and words[e] & P.PC_OBSTACLE


def test_cfrc_follows_each_envs_own_terrain():
    """cassie_hfield on a bank of terrains: envs 0 and 1 in the SAME state, on the ramp (feet pressed in) and on the low flat grid (in
    the air); env 2 lower, pressed into the raised flat grid.  Every env's forces are those of its own terrain."""
    m = Model("cassie_hfield")
    pod = m.pod
    bank = tc.make_bank(pod.hfield_nrow, pod.hfield_ncol, count=5)[[0, 1, 4]]
    index = np.array([1, 0, 2], dtype=np.int32)
    q = np.tile(m.qpos_init(), (3, 1))
    q[:, 2] -= [0.015, 0.015, 0.095]
    v = np.random.default_rng(4).uniform(-0.2, 0.2, (3, pod.nv))
    feet = [m.name2id(1, "left-foot"), m.name2id(1, "right-foot")]
    probes = [(BODY, feet[0], [0, 0, 0]), (BODY, feet[1], [0, 0, 0]), (BODY, 1, [0, 0, 0]), (SITE, 0, [0.01, 0, 0])]

    def prepare(b):
        b.set_hfield_bank(bank)
        b.set_terrain(index)

    got, _, warn = _probe_batch(m, q, v, None, probes, ROWS, prepare)
    assert not warn.any()
    pc.check_rows(pod, q, v, probes, got, hfields=[bank[t].reshape(-1) for t in index])
    assert got["cfrc"][0, 0, 2] > 50 and np.all(got["cfrc"][1] == 0) and got["cfrc"][2, 1, 2] > 50
    assert np.array_equal(got["pos"][0], got["pos"][1])


# ------------------------------------------------------------------ 2. against the drop-in's getters ----
def test_probe_rows_are_the_drop_ins_getters(cassie):
    """One env's state loaded into a cassie_sim_t: cassie_sim_get_jacobian_full / _full_site, body_velocities, body_acceleration,
    body_contact_force, site_xpos / site_xquat and the three collision checks agree with that env's probe rows."""
    L = lib()
    if hasattr(L, "cassie_agility_blocks_absent"):
        pytest.skip("the drop-in (cassie_sim_t) cannot be loaded: this build was linked without the Agility blocks")
    VP, DP, CP = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_char_p
    L.cassie_sim_init.restype, L.cassie_sim_init.argtypes = VP, [CP, ctypes.c_bool]
    L.cassie_sim_free.argtypes = [VP]
    for f in ("cassie_sim_qpos", "cassie_sim_qvel", "cassie_sim_ctrl"):
        getattr(L, f).restype, getattr(L, f).argtypes = DP, [VP]
    L.cassie_sim_forward.argtypes = [VP]
    L.cassie_sim_get_jacobian_full.argtypes = L.cassie_sim_get_jacobian_full_site.argtypes = [VP, VP, VP, CP]
    for f in ("cassie_sim_body_velocities", "cassie_sim_body_acceleration", "cassie_sim_body_contact_force"):
        getattr(L, f).argtypes, getattr(L, f).restype = [VP, VP, CP], None
    L.cassie_sim_site_xpos.restype, L.cassie_sim_site_xpos.argtypes = DP, [VP, CP]
    L.cassie_sim_site_xquat.argtypes, L.cassie_sim_site_xquat.restype = [VP, CP, VP], None
    for f in ("cassie_sim_check_obstacle_collision", "cassie_sim_check_self_collision"):
        getattr(L, f).restype, getattr(L, f).argtypes = ctypes.c_bool, [VP]
    L.cassie_sim_geom_collision.restype, L.cassie_sim_geom_collision.argtypes = ctypes.c_bool, [VP, ctypes.c_int]
    pod = cassie.pod
    q, v, ctrl = cassie_states(cassie)
    bodies, sites = ["cassie-pelvis", "left-foot", "right-tarsus"], ["left-heel", "right-toe", "imu"]
    probes = [(BODY, cassie.name2id(1, s), [0, 0, 0]) for s in bodies] + [(SITE, cassie.name2id(6, s), [0, 0, 0]) for s in sites]
    got, words, _ = _probe_batch(cassie, q, v, ctrl, probes, P.PQ_ALL)
    c = L.cassie_sim_init(os.path.join(REPO_DIR, "models", "cassie.cmodel").encode(), False)
    assert c
    try:
        for e in (2, 3, 4):                     # pressed into the floor, legs crossed, randomised joints
            np.ctypeslib.as_array(L.cassie_sim_qpos(c), (pod.nq,))[:] = q[e]
            np.ctypeslib.as_array(L.cassie_sim_qvel(c), (pod.nv,))[:] = v[e]
            np.ctypeslib.as_array(L.cassie_sim_ctrl(c), (pod.nu,))[:] = ctrl[e]
            L.cassie_sim_forward(c)
            jp, jr, six, quat = np.zeros((3, pod.nv)), np.zeros((3, pod.nv)), np.zeros(6), np.zeros(4)
            for j, name in enumerate(bodies):
                L.cassie_sim_get_jacobian_full(c, jp.ctypes.data, jr.ctypes.data, name.encode())
                assert np.allclose(got["jacp"][e, j], jp, atol=pc.ATOL, rtol=0) and np.allclose(got["jacr"][e, j], jr, atol=pc.ATOL, rtol=0)
                L.cassie_sim_body_velocities(c, six.ctypes.data, name.encode())
                assert np.allclose(got["cvel"][e, j], six, atol=pc.ATOL, rtol=0)
                L.cassie_sim_body_acceleration(c, six.ctypes.data, name.encode())
                assert np.allclose(got["acc"][e, j], six, **pc.FORCE_TOL)
                L.cassie_sim_body_contact_force(c, six.ctypes.data, name.encode())
                assert np.allclose(got["cfrc"][e, j], six[:3], **pc.FORCE_TOL) and not six[3:].any()
            for j, name in enumerate(sites, start=len(bodies)):
                L.cassie_sim_get_jacobian_full_site(c, jp.ctypes.data, jr.ctypes.data, name.encode())
                assert np.allclose(got["jacp"][e, j], jp, atol=pc.ATOL, rtol=0) and np.allclose(got["jacr"][e, j], jr, atol=pc.ATOL, rtol=0)
                assert np.allclose(got["pos"][e, j], np.ctypeslib.as_array(L.cassie_sim_site_xpos(c, name.encode()), (3,)), atol=pc.ATOL, rtol=0)
                L.cassie_sim_site_xquat(c, name.encode(), quat.ctypes.data)
                assert np.allclose(got["quat"][e, j], quat, atol=pc.ATOL, rtol=0)
            word = (P.PC_OBSTACLE if L.cassie_sim_check_obstacle_collision(c) else 0) | (P.PC_SELF if L.cassie_sim_check_self_collision(c) else 0)
            for g in range(6):
                word |= (P.PC_GROUP0 << g) if L.cassie_sim_geom_collision(c, g) else 0
            assert int(words[e]) == word
        assert np.abs(got["cfrc"][2, 1]).max() > 50 and words[3] & P.PC_SELF
    finally:
        L.cassie_sim_free(c)


# ------------------------------------------------------------------ 3. the loop is not disturbed ----
@pytest.mark.parametrize("extras", ["plain", "step_sums", "episodes"])
def test_the_loop_is_not_disturbed(cassie, extras):
    """Two batches of 8 envs in DRIVE_PD_SAFE run step_range(50 substeps) x 6 on two ranges and two streams; the second with a probe of
    each range behind every step launch, on the range's stream.  At the end every downloadable field, the warning words, the solver
    statistics and the drive-level state are byte-identical -- also with the step sums on, and with episodes ended and restarted in the loop."""
    import torch
    n, npol, k = 8, 6, 4
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * np.arange(n)
    tgd = torch.from_numpy(bench.pd_targets(np.arange(n), npol)).cuda()
    pick_d = torch.from_numpy(np.random.default_rng(7).integers(0, k, (npol, n)).astype(np.int32)).cuda()
    bq, bv = bank_states(cassie, k)
    probes = cassie_probes(cassie)
    ranges = [(0, 4), (4, 4)]

    def run(probing):
        b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
        try:
            if extras == "step_sums":
                b.enable_step_sums()
            if extras == "episodes":
                b.enable_episodes(max_steps=2, min_height=0.6)
                bank_d = torch.from_numpy(b.make_reset_bank(bq, bv)).cuda()
                b.set_reset_bank(device_ptr=bank_d.data_ptr(), n=k)
            if probing:
                b.configure_probes(probes, P.PQ_ALL)
            b.sync()
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for p in range(npol):
                b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
                for (e0, cnt), st in zip(ranges, streams):
                    b.step_range(e0, cnt, 50, st.cuda_stream)
                    if probing:
                        b.probe(e0, cnt, stream=st.cuda_stream)
                    if extras == "episodes":
                        b.end_episodes(e0, cnt, True, pick_ptr=pick_d[p].data_ptr() + 4 * e0, stream=st.cuda_stream)
            b.sync()
            torch.cuda.synchronize()
            out = {f: b.get(f).tobytes() for f in STATE_FIELDS}
            w, info = b.warnings()
            out["warn"], out["info"], out["drive"] = w.tobytes(), info.tobytes(), drive_bytes(b)
            if extras == "step_sums":
                out["sums"] = b.get(P.F_STEP_SUMS).tobytes()
                assert b.get(P.F_STEP_SUMS)[:, P.SUM_COUNT].tolist() == [50.0] * n
            if extras == "episodes":
                done, reason, steps, count, terminal = b.episodes()
                out["episodes"] = b"".join(a.tobytes() for a in (done, reason, steps, count, terminal))
                assert count.min() >= 2
            rows = None
            if probing:
                assert b.probe_launches() == (2 * npol, 2 * npol)
                rows = (b.probes(), b.probe_contacts(), b.get(P.F_QPOS), b.get(P.F_QVEL), b.get(P.F_CTRL), b.get(P.F_QACC_WARMSTART))
            return out, rows
        finally:
            b.close()

    want, _ = run(False)
    got, rows = run(True)
    for key in want:
        assert got[key] == want[key], key
    if extras == "plain":
        # ... and what the last probes saw is the state the loop ended in, under the torques the last step applied
        vals, words, q, v, ctrl, warm = rows
        pc.check_rows(cassie.pod, q, v, probes, vals, ctrl=ctrl, words=words, classes=pe.geom_classes(cassie), warm=warm)
        assert np.abs(ctrl).max() > 1.0


# ------------------------------------------------------------------ 4. ranges and binding ----
def test_ranges_and_bindings(cassie):
    """PROBE_GRID + 3 envs: probe(env0 = 2, n = PROBE_GRID) with the rows bound as a strided column block of a wider tensor and the
    contact words bound to a caller's tensor writes exactly those rows and columns; the env in the middle has a NaN in qpos."""
    import torch
    pod = cassie.pod
    pe.lib()
    G = pe.PROBE_GRID
    nenv, env0, mid = G + 3, 2, 2 + G // 2
    LEFT, RIGHT, FILL = 3, 5, -7.0
    rng = np.random.default_rng(1)
    q = np.tile(cassie.qpos_init(), (nenv, 1))
    q[:, 2] -= 0.0003 * np.arange(nenv)
    v = rng.uniform(-0.2, 0.2, (nenv, pod.nv))
    q[mid, 9] = np.nan
    probes, classes = cassie_probes(cassie)[:4], pe.geom_classes(cassie)
    Q = P.PQ_POS | P.PQ_VEL | P.PQ_JACP | P.PQ_CFRC | P.PQ_CONTACTS
    b = Batch(cassie, nenv)
    try:
        b.set(P.F_QPOS, q)
        b.set(P.F_QVEL, v)
        b.configure_probes(probes, Q)
        row = pe.layout(len(probes), Q, pod.nv)[0]
        assert b.dim(P.F_PROBES) == row == lib().phys_batch_probe_row_dim(b._h)
        assert b.probe_layout() == {"pos": (0, (4, 3)), "vel": (12, (4, 6)), "jacp": (36, (4, 3, 32)), "cfrc": (36 + 384, (4, 3))}
        obs = torch.full((nenv, LEFT + row + RIGHT), FILL, dtype=torch.float64, device="cuda")
        words_d = torch.full((nenv,), -5, dtype=torch.int32, device="cuda")
        b.bind(P.F_PROBES, obs.data_ptr() + 8 * LEFT, row_stride=LEFT + row + RIGHT)
        b.bind_probe_contacts(words_d.data_ptr())
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        b.probe(env0, G, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        o, words = obs.cpu().numpy(), words_d.cpu().numpy()
        out = o[:, LEFT: LEFT + row]
        assert np.all(o[:, :LEFT] == FILL) and np.all(o[:, LEFT + row:] == FILL)
        outside = [0, 1, nenv - 1]
        assert np.all(out[outside] == FILL) and np.all(words[outside] == -5)
        assert np.all(np.isnan(out[mid])) and words[mid] == 0
        inside = [e for e in range(env0, env0 + G) if e != mid]
        assert np.all(np.isfinite(out[inside])) and np.all(words[inside] >= 0)
        assert np.array_equal(b.get(P.F_PROBES)[inside], out[inside]) and np.array_equal(b.probe_contacts(), words)
        got = pe.split(out, len(probes), Q, pod.nv)
        pc.check_rows(pod, q, v, probes, got, words=words, classes=classes, envs=[env0, mid - 1, mid + 1, env0 + G - 1])
        w = b.warnings()[0]
        assert w[mid] == P.WARN_DIVERGED and not w[inside].any()
        # the batch's own words again
        b.bind_probe_contacts(None)
        b.probe(0, 2)
        own = b.probe_contacts()
        assert np.all(own[:2] >= 0) and not own[2:].any() and np.all(words_d.cpu().numpy()[:2] == -5)
    finally:
        b.close()


# ------------------------------------------------------------------ 5. counters and refusals ----
def test_counters_and_refusals(cassie):
    pod = cassie.pod
    n = 8
    err = lambda: (lib().phys_last_error() or b"").decode()
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    twin = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        tg = bench.pd_targets(np.arange(n), 1)[0]
        for x in (b, twin):
            x.set(P.F_PD_PTARGET, tg)
        assert b.probe_launches() == (0, 0) and b.dim(P.F_PROBES) == 0
        assert lib().phys_batch_probe(b._h, 0, n, None) == -1 and err() == "phys_batch_probe: not configured (phys_batch_probes_configure first)"
        with pytest.raises(RuntimeError, match="phys_batch_probes_configure"):
            b.get(P.F_PROBES)
        with pytest.raises(ValueError, match="a body probe's id must lie in"):
            b.configure_probes([(BODY, pod.nbody, [0, 0, 0])], P.PQ_POS)
        with pytest.raises(ValueError, match="quantities is a non-empty OR of PHYS_PQ_"):
            b.configure_probes([(BODY, 1, [0, 0, 0])], 0)
        with pytest.raises(ValueError, match="0 .. 32 probes"):
            b.configure_probes([(BODY, 1, [0, 0, 0])] * 33, P.PQ_POS)
        assert b.probe_launches() == (0, 0) and b.dim(P.F_PROBES) == 0
        probes = cassie_probes(cassie)
        b.configure_probes(probes, P.PQ_ALL)
        assert lib().phys_batch_probe(b._h, 4, 5, None) == -1 and err() == "phys_batch_probe: env range out of bounds"
        assert lib().phys_batch_probe(b._h, -1, 2, None) == -1 and err() == "phys_batch_probe: env range out of bounds"
        forms = b.form_launches()
        for x in (b, twin):
            x.step(50)
        stepped = b.form_launches()
        b.probe()
        b.probe(2, 3)
        b.probe(0, 0)                                   # (nothing to do: nothing launched)
        assert b.probe_launches() == (2, 2) and b.form_launches() == stepped and stepped != forms
        first = b.probes()
        assert np.isfinite(first["jacp"]).all() and np.abs(first["cfrc"][:, 1]).max() > 50
        # another list: the rows take its size, the values are the new probes'
        b.configure_probes(probes[1:3], P.PQ_POS | P.PQ_CFRC)
        assert b.dim(P.F_PROBES) == 2 * 6 and b.probe_layout() == {"pos": (0, (2, 3)), "cfrc": (6, (2, 3))}
        b.probe()
        second = b.probes()
        assert np.array_equal(second["pos"], first["pos"][:, 1:3]) and np.array_equal(second["cfrc"], first["cfrc"][:, 1:3])
        with pytest.raises(RuntimeError, match="PHYS_PQ_CONTACTS"):
            b.probe_contacts()
        # released: as before configuring
        b.configure_probes([], 0)
        assert b.dim(P.F_PROBES) == 0 and lib().phys_batch_probe_row_dim(b._h) == 0 and b.probe_launches() == (3, 3)
        assert lib().phys_batch_probe(b._h, 0, n, None) == -1 and err() == "phys_batch_probe: not configured (phys_batch_probes_configure first)"
        # and a following step is what it is without any of it
        for x in (b, twin):
            x.step(50)
        for f in STATE_FIELDS:
            assert b.get(f).tobytes() == twin.get(f).tobytes(), f
        assert drive_bytes(b) == drive_bytes(twin) and b.warnings()[0].tobytes() == twin.warnings()[0].tobytes()
        # a batch made from a compiled model alone knows no geom classes: the contact word is refused, the rows are not
        c = Batch(pod, 2)
        try:
            with pytest.raises(ValueError, match="phys_batch_probe_geom_classes first"):
                c.configure_probes(probes, P.PQ_ALL)
            c.configure_probes(probes, ROWS)
            c.probe()
            assert np.isfinite(c.probes()["pos"]).all()
        finally:
            c.close()
    finally:
        b.close()
        twin.close()
