"""Placed restarts (phys_batch_place_configure + phys_batch_end_episodes), on the CPU: the device's placed episode kernel
(csrc/episode_kernels.h: cassie_episode_place_kernel) executed by the wave emulator, against the unplaced kernel (the identity placement),
against the numpy restatement of the header's definition (tests/placement_check.py), the restatement against the oracle's forward pass,
and the emulated height scan of the placed envs.  The GPU counterpart is tests/test_placement_gpu.py.

Tolerances (placement_check): entries the definition leaves alone are EQUAL; a transformed entry is at most three products of values
below about 10 and sines / cosines good to a few ulp: within 1e-12 max(1, |v|), about 10^3 ulp of room; the ground height and the z
entries within the scan suite's 1e-12 m.  An env with a footprint point within 1e-9 m of a border between surface pieces is left out of
the ground / z comparison only; fewer than 5 % of the restarted envs may be, which is asserted on the restatement before anything is
compared (the seeds below were chosen for it)."""
import functools

import numpy as np
import pytest

import emu_py
import episode_check as ec
import oracle_py
import placement_check as pc
import placement_emu_py
import terrain_check as tc
from cassie_amd import Model
from cassie_amd import phys as P
from test_episodes import RULES, make_bank, make_state
from test_terrain import _blocks, _quat_mul, _random_quat, _yaw_quat

MODELS = ["cassie", "cassie_hfield", "cassie_tray_box"]
NENV, ENV0, N, GRID, NROWS = 70, 3, 61, 8, 5
GROUND_REF = {"cassie": 0.0, "cassie_hfield": -0.1, "cassie_tray_box": -0.01}
SEEDS = {"cassie": 31, "cassie_hfield": 32, "cassie_tray_box": 33}


def footprint(npoints):
    """1: the anchor's own spot; 5: the spot and a foot-sized rectangle's corners; 70: a 10 x 7 grid 5 cm apart (a loop past 64 lanes)."""
    if npoints == 1:
        return np.zeros((1, 2))
    if npoints == 5:
        return np.array([[0.0, 0.0], [0.15, 0.1], [0.15, -0.1], [-0.15, 0.1], [-0.15, -0.1]])
    assert npoints == 70
    return np.array([[0.05 * (i - 4.5), 0.05 * (j - 3.0)] for i in range(10) for j in range(7)])


def random_poses(rng, nenv):
    """|dx|, |dy| <= 3, |dz| <= 0.2, yaw over (-pi, pi]."""
    return np.ascontiguousarray(np.stack([rng.uniform(-3, 3, nenv), rng.uniform(-3, 3, nenv), rng.uniform(-0.2, 0.2, nenv),
                                          -rng.uniform(-np.pi, np.pi, nenv)], axis=1))


def make_case(name, npoints, drive=True, nenv=NENV, env0=ENV0, n=N, seed=None):
    """A batch somewhere in mid-episode, about half of the range's envs forced to end, random bank rows, random poses -- and per model:
      cassie_hfield    a bank of 4 terrains, next terrains with one id below and one above the bank, the height-field geom moved and
                       yawed per env, TILTED for one restarting env, one restarting env sent wholly off the grid;
      cassie           per-env geometry: stair boxes under some spawn points, the floor tilted;
      cassie_tray_box  the model's own floor; the cube is the second moving root."""
    model = Model(name)
    pod = model.pod
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    state = make_state(model, nenv, seed=7 + len(name), drive=drive)
    force = (rng.random(n) < 0.5).astype(np.int32)
    ended = env0 + np.nonzero(force)[0]
    bank = make_bank(pod, NROWS, seed=13)
    pick = rng.integers(0, NROWS, n).astype(np.int32)
    pose = random_poses(rng, nenv)
    place = dict(anchor=int(pod.root_body[0]), footprint=footprint(npoints), ground_ref=GROUND_REF[name], pose=pose,
                 ground=rng.uniform(5.0, 6.0, nenv), nxt=None, index=None, grids=None, geom_pos=None, geom_quat=None)
    emu = dict(blocks=None, hfield=None, stride=0, nterrain=0)
    row_xy = np.zeros((nenv, 2))
    row_xy[env0:env0 + n] = bank[pick][:, 0:2]                    # the anchor's x, y in the row an env would restart from
    spawn = row_xy + pose[:, 0:2]
    special = {}
    if name == "cassie_hfield":
        grids = tc.make_bank(pod.hfield_nrow, pod.hfield_ncol, seed=3, count=4)
        place["grids"] = grids
        place["index"] = rng.integers(0, 4, nenv).astype(np.int32)
        nxt = rng.integers(0, 4, nenv).astype(np.int32)
        nxt[ended[0]], nxt[ended[1]] = -2, 7
        place["nxt"] = nxt
        gp, gq = tc.model_geom_poses(pod, nenv)
        g = pod.hfield_geom
        gp[:, g] += np.concatenate([rng.uniform(-0.5, 0.5, (nenv, 2)), rng.uniform(-0.2, 0.2, (nenv, 1))], axis=1)
        gq[:, g] = _yaw_quat(rng.uniform(-np.pi, np.pi, nenv))
        a = np.radians(3.0) / 2
        gq[ended[2], g] = _quat_mul(_yaw_quat(np.array([0.7])), np.array([[np.cos(a), 0.0, np.sin(a), 0.0]]))[0]
        pose[ended[3], 0] = 40.0                                  # (beyond |dx| <= 3 on purpose: nothing under it, no floor in this model)
        place["geom_pos"], place["geom_quat"] = gp, gq
        emu.update(hfield=grids.reshape(-1), stride=pod.hfield_nrow * pod.hfield_ncol, nterrain=4)
        special = dict(below=ended[0], above=ended[1], tilted=ended[2], off=ended[3])
    elif name == "cassie":
        gp, gq = tc.model_geom_poses(pod, nenv)
        boxes = [g for g, t in tc.static_geoms(pod) if t == tc.BOX]
        floor = [g for g, t in tc.static_geoms(pod) if t == tc.PLANE][0]
        for k, g in enumerate(boxes[:6]):
            half = np.array(list(pod.geom_size[g]))
            gp[:, g, 0:2] = spawn + rng.uniform(-1.6, 1.6, (nenv, 2))
            gp[:, g, 2] = -half[2] + rng.uniform(0.02, 0.5, nenv)
            gq[:, g] = _random_quat(rng, nenv, 0.5 if k % 2 else 0.0)
        gq[:, floor] = _random_quat(rng, nenv, 0.15)
        place["geom_pos"], place["geom_quat"] = gp, gq
    if place["geom_pos"] is not None:
        emu["blocks"] = _blocks(pod, place["geom_pos"], place["geom_quat"])
    return dict(name=name, model=model, pod=pod, state=state, force=force, ended=ended, bank=bank, pick=pick, place=place, emu=emu,
                env0=env0, n=n, special=special)


def copy_place(place):
    return {k: (v.copy() if isinstance(v, np.ndarray) and k in ("ground", "index") else v) for k, v in place.items()}


def run_reference(c):
    """The restatement on a copy of the case -> (state, place, restarted envs, near)."""
    s, pl = ec.copy_state(c["state"]), copy_place(c["place"])
    done, envs, near = pc.end_episodes(s, c["pod"], RULES, c["env0"], c["n"], True, c["bank"], pl, pick=c["pick"], force=c["force"])
    assert np.array_equal(envs, c["ended"])
    return s, pl, envs, near


def run_emulator(c, strided=True, grid=GRID):
    """The emulated kernel on a copy of the case, qpos / qvel / sensordata as column blocks of one wider array -> (state, place)."""
    pod = c["pod"]
    s, pl = ec.copy_state(c["state"]), copy_place(c["place"])
    block = None
    if strided:
        w = pod.nq + pod.nv + pod.nsensordata
        block = np.full((len(s["qpos"]), w + 3), 12345.678)
        block[:, :w] = np.concatenate([s["qpos"], s["qvel"], s["sensordata"]], axis=1)
        s["qpos"], s["qvel"], s["sensordata"] = block[:, :pod.nq], block[:, pod.nq:pod.nq + pod.nv], block[:, pod.nq + pod.nv:w]
    placement_emu_py.end_episodes(s, pod, RULES, c["env0"], c["n"], True, c["bank"], pl["anchor"], pl["pose"], pl["ground"],
                                  footprint=pl["footprint"], ground_ref=pl["ground_ref"], nxt=pl["nxt"], pick=c["pick"], force=c["force"],
                                  grid=grid, block=block, index=pl["index"], **c["emu"])
    if strided:
        assert np.all(block[:, -3:] == 12345.678)
        s = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in s.items()}
    return s, pl


@functools.lru_cache(maxsize=None)
def solved(name, npoints):
    """(case, reference results, emulator results): computed once, shared by the tests below, which leave them unchanged."""
    c = make_case(name, npoints)
    return c, run_reference(c), run_emulator(c)


# ------------------------------------------------------------------ 1. the identity placement ----
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("drive", [True, False])
def test_identity_placement_leaves_what_an_unplaced_restart_leaves(built, name, drive):
    """The pose (0, 0, 0, 0) with no footprint against emu_py.end_episodes (the unplaced kernel) on the same state: every array equal."""
    c = make_case(name, 1, drive=drive)
    pod = c["pod"]
    a, b = ec.copy_state(c["state"]), ec.copy_state(c["state"])
    emu_py.end_episodes(a, pod, RULES, ENV0, N, True, bank=c["bank"], pick=c["pick"], force=c["force"], grid=GRID)
    ground = np.full(NENV, 5.5)
    placement_emu_py.end_episodes(b, pod, RULES, ENV0, N, True, c["bank"], c["place"]["anchor"], np.zeros((NENV, 4)), ground,
                                  footprint=None, ground_ref=GROUND_REF[name], pick=c["pick"], force=c["force"], grid=GRID)
    assert 20 <= a["done"].sum() <= 45
    for k in a:
        if a[k] is None:
            assert b[k] is None
        else:
            assert np.array_equal(a[k], b[k]), k
    assert np.all(ground[c["ended"]] == GROUND_REF[name]) and np.all(np.delete(ground, c["ended"]) == 5.5)


# ------------------------------------------------------------------ 2. the emulated kernel against the restatement ----
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("npoints", [1, 5, 70])
def test_placed_restart_matches_the_definition(built, name, npoints):
    c, (want, want_place, envs, near), (got, got_place) = solved(name, npoints)
    assert 20 <= len(envs) <= 45
    pc.compare(got, want, got_place, want_place, c["pod"], envs, near, "%s, %d points" % (name, npoints))
    w = want["warn"]
    if name == "cassie_hfield":
        sp = c["special"]
        assert w[sp["below"]] & P.WARN_TERRAIN_INDEX and w[sp["above"]] & P.WARN_TERRAIN_INDEX
        assert want_place["index"][sp["below"]] == 0 and want_place["index"][sp["above"]] == 3
        assert w[sp["tilted"]] == P.WARN_SCAN_TILTED | P.WARN_PLACE_MISS          # (no other static geom in this model)
        assert w[sp["off"]] == P.WARN_PLACE_MISS == placement_emu_py.lib().emu_place_warn_bit() == 128
        assert want_place["ground"][sp["off"]] == GROUND_REF[name]
        assert (w[envs] == 0).sum() > len(envs) // 2
    else:
        assert not w.any()
    if name == "cassie":                                          # some spawn points stand on a stair box, some on the tilted floor
        gp0, _ = tc.model_geom_poses(c["pod"], NENV)
        far = dict(c["place"], geom_pos=gp0, ground=c["place"]["ground"].copy())
        s2 = ec.copy_state(c["state"])
        pc.end_episodes(s2, c["pod"], RULES, ENV0, N, True, c["bank"], far, pick=c["pick"], force=c["force"])
        on_box = want_place["ground"][envs] > far["ground"][envs] + 1e-6
        assert on_box.sum() >= 3 and (~on_box).sum() >= 3
    # the pose does move things: the restatement is not the identity
    assert np.abs(want["qpos"][envs] - c["bank"][c["pick"][envs - ENV0]][:, :c["pod"].nq]).max() > 1.0


def test_result_does_not_depend_on_the_grid_or_the_row_stride(built):
    c, _, (got, got_place) = solved("cassie_tray_box", 5)
    for strided, grid in ((False, 1), (False, 0), (True, 32)):
        s, pl = run_emulator(c, strided=strided, grid=grid)
        ec.assert_states_equal(s, got, "grid %d" % grid)
        assert np.array_equal(pl["ground"], got_place["ground"])


def test_no_next_terrains_leaves_the_index_alone(built):
    c = make_case("cassie_hfield", 5)
    before = c["place"]["index"].copy()
    c["place"]["nxt"] = None
    (want, want_place, envs, near), (got, got_place) = run_reference(c), run_emulator(c)
    pc.compare(got, want, got_place, want_place, c["pod"], envs, near, "no next terrains")
    assert np.array_equal(got_place["index"], before)


def test_next_terrains_without_a_bank_are_ignored(built):
    """A next-terrain array bound while no bank of terrains is set: not read, the index array not written, the result that of a batch
    with none bound."""
    c, _, (got, got_place) = solved("cassie_tray_box", 5)
    d = make_case("cassie_tray_box", 5)
    d["place"]["nxt"] = np.full(NENV, 9, dtype=np.int32)
    d["place"]["index"] = np.full(NENV, -4, dtype=np.int32)
    assert d["emu"]["nterrain"] == 0
    (want, want_place, envs, near), (s, pl) = run_reference(d), run_emulator(d)
    pc.compare(s, want, pl, want_place, d["pod"], envs, near, "next terrains, no bank")
    ec.assert_states_equal(s, got, "next terrains, no bank")
    assert np.all(pl["index"] == -4) and np.array_equal(pl["ground"], got_place["ground"]) and not s["warn"].any()


def test_configure_refuses_what_it_cannot_place(built):
    c = make_case("cassie", 1)
    pod, s = c["pod"], ec.copy_state(c["state"])
    args = (s, pod, RULES, ENV0, N, True, c["bank"])
    pose, ground = np.zeros((NENV, 4)), np.zeros(NENV)
    pelvis = int(pod.root_body[0])
    assert "child of the world" in placement_emu_py.end_episodes(*args, pelvis + 1, pose, ground, expect_error=True)
    assert "1024" in placement_emu_py.end_episodes(*args, pelvis, pose, ground, footprint=np.zeros((1025, 2)), expect_error=True)
    import ctypes
    from cassie_amd._lib import CmModel
    odd = CmModel.from_buffer_copy(pod)
    odd.body_kin[pelvis].slide_axis_p[0][0], odd.body_kin[pelvis].slide_axis_p[0][1] = 0.6, 0.8
    assert "slides" in placement_emu_py.end_episodes(s, odd, *args[2:], pelvis, pose, ground, expect_error=True)
    elsewhere = CmModel.from_buffer_copy(pod)
    framequat = [sn for sn in range(pod.nsensor) if pod.sensor_type[sn] == pc.SENS_FRAMEQUAT][0]
    elsewhere.sensor_body[framequat] = pelvis + 1                 # the framequat's site on a leg body
    assert "sensor" in placement_emu_py.end_episodes(s, elsewhere, *args[2:], pelvis, pose, ground, expect_error=True)
    assert ctypes.sizeof(placement_emu_py.PlaceArgs) == placement_emu_py.lib().emu_place_sizeof()
    ec.assert_states_equal(s, c["state"], "refused calls")


# ------------------------------------------------------------------ 3. the restatement against the oracle ----
ORACLE_MEASURED = {"cassie": 3.95e-3, "cassie_tray_box": 2.68e-3}        # (see the test's docstring)
ORACLE_BOUND = {k: 10 * v for k, v in ORACLE_MEASURED.items()}
ORACLE_EXACT = 1e-12       # the entries that do not pass through the contact solve: a few roundings of values below 10


def oracle_rows(model, k, seed):
    """k rows [qpos | qvel | sensordata | actuator_velocity | qacc] of an oracle forward() at perturbed standing states, feet on the floor,
    with non-zero qvel."""
    pod = model.pod
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(k):
        q = model.qpos_init()
        q[0:2] = rng.uniform(-0.5, 0.5, 2)
        q[2] -= rng.uniform(0.0, 0.012)
        q[3:7] = _random_quat(rng, 1, 0.03)[0]
        q[7:35] += rng.uniform(-0.01, 0.01, 28)
        v = rng.uniform(-0.05, 0.05, pod.nv)
        rows.append(oracle_forward(pod, q, v))
    return np.stack(rows)


def oracle_forward(pod, q, v):
    o = oracle_py.Oracle(pod, q)
    o.qvel[:] = v
    o.forward()
    return np.concatenate([o.qpos, o.qvel, o.sensordata, o.actuator_velocity, o.qacc])


@pytest.mark.parametrize("name", ["cassie", "cassie_tray_box"])
def test_restatement_is_a_symmetry_of_the_oracle_on_the_flat_floor(built, name):
    """A rigid motion about the vertical is a symmetry of a model on a flat floor: the placed row [qpos | qvel | sensordata |
    actuator_velocity | qacc] (dz = 0, no footprint, |dx|, |dy| <= 3: away from the stair boxes at y = 20) against an oracle forward() at
    the placed qpos and qvel.  The cube of cassie_tray_box shows that every moving root is carried along.

    The bound is 10 x the largest difference measured between the numpy restatement and the oracle over this test's cases on the CPU
    (for rounding through the contact solve on other hosts), relative to max(1, |v|):
        cassie           measured 3.95e-3 (qacc; the accelerometer 6.1e-4)   bound 3.95e-2
        cassie_tray_box  measured 2.68e-3 (qacc; the accelerometer 3.9e-4)   bound 2.68e-2
    All of it is qacc and the accelerometer, i.e. the contact solve: its friction pyramids stand on the FLOOR's tangent axes, which do
    not turn with the robot, and 50 PGS sweeps do not converge to the last bits (a pure shift, yaw = 0, differs by 9e-11).  Every other
    entry -- qpos, qvel, the joint and actuator positions, framequat, gyro, magnetometer, actuator_velocity -- measured at most 3.4e-16
    and is held to ORACLE_EXACT = 1e-12 here besides."""
    model = Model(name)
    pod = model.pod
    k = 12
    rows = oracle_rows(model, k, seed=5)
    assert np.abs(rows[:, -pod.nv:]).max() > 1.0 and np.abs(rows[:, pod.nq:pod.nq + pod.nv]).max() > 0.01
    rng = np.random.default_rng(6)
    pose = random_poses(rng, k)
    pose[:, 2] = 0.0
    place = dict(anchor=int(pod.root_body[0]), footprint=None, ground_ref=GROUND_REF[name], pose=pose)
    q, v, s, a, G, bits, near = pc.place_rows(pod, rows, place, np.arange(k))
    nq, nv, nsd, nu = pod.nq, pod.nv, pod.nsensordata, pod.nu
    placed = np.concatenate([q, v, s, rows[:, nq + nv + nsd:nq + nv + nsd + nu], a], axis=1)
    want = np.stack([oracle_forward(pod, q[e], v[e]) for e in range(k)])
    err = float(np.max(np.abs(placed - want) / np.maximum(1.0, np.abs(want))))
    moved = float(np.max(np.abs(placed - rows)))
    print("%s: the placed rows differ from the oracle's forward pass by %.3g (relative), from the rows themselves by %.3g" % (name, err, moved))
    assert moved > 1.0 and not bits.any() and np.all(G == GROUND_REF[name])
    if name == "cassie_tray_box":
        cube = pc.root_layout(pod, pc.moving_roots(pod)[1])
        assert cube["free"] and np.abs(q[:, cube["q"][0]] - rows[:, cube["q"][0]]).max() > 1.0
    assert err <= ORACLE_BOUND[name], (err, ORACLE_BOUND[name])
    solved_cols = np.zeros(placed.shape[1], dtype=bool)         # what the contact solve decides: qacc and the accelerometer
    solved_cols[-nv:] = True
    for sn in range(pod.nsensor):
        if pod.sensor_type[sn] == pc.SENS_ACCELEROMETER:
            solved_cols[nq + nv + pod.sensor_adr[sn]:nq + nv + pod.sensor_adr[sn] + 3] = True
    rel = np.abs(placed - want) / np.maximum(1.0, np.abs(want))
    assert float(rel[:, ~solved_cols].max()) <= ORACLE_EXACT, float(rel[:, ~solved_cols].max())


# ------------------------------------------------------------------ 4. the height scan of a placed env ----
def check_scan_consistency(c, want_place, envs, near, qpos_after, warn_after, values):
    """min_j value == z_anchor(row) - ground_ref + dz within 1e-12 for every restarted env whose footprint met ground (the others read
    +range everywhere), envs with a near-border point left out (fewer than 5 %)."""
    pod, pl = c["pod"], c["place"]
    assert float(np.mean(near)) < pc.MOST_NEAR
    rows = c["bank"][c["pick"][envs - c["env0"]]]
    z_row = pc.root_pose(pod, pl["anchor"], rows[:, :pod.nq])[0][:, 2]
    want = z_row - pl["ground_ref"] + pl["pose"][envs, 2]
    hit = (warn_after[envs] & P.WARN_PLACE_MISS) == 0
    use = hit & ~near
    assert use.sum() > len(envs) // 2
    err = np.abs(values[envs].min(axis=1) - want)
    print("%s: %d placed envs scanned, min of the scan within %.2g m of the row's height above its ground" % (c["name"], use.sum(), err[use].max()))
    assert err[use].max() <= 1e-12
    assert np.all(values[envs][~hit] == 10.0)


@pytest.mark.parametrize("name", MODELS)
def test_scan_of_a_placed_env_reads_the_rows_height_above_ground(built, name):
    c, (want, want_place, envs, near), (got, got_place) = solved(name, 5)
    emu = c["emu"]
    values, _ = emu_py.height_scan(c["pod"], got["qpos"], c["place"]["footprint"], c["place"]["anchor"], 10.0, blocks=emu["blocks"],
                                   hfield=emu["hfield"], stride=emu["stride"], index=got_place["index"], nterrain=emu["nterrain"])
    check_scan_consistency(c, want_place, envs, near, got["qpos"], got["warn"], values)
