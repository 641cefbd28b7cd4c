"""Per-env terrains from a bank and the height scan, on the CPU: the device's scan kernel (csrc/surface_kernels.h: cassie_scan_kernel)
and the step kernel's terrain index (PhysIO::hfield_index), executed by the wave emulator, against the numpy restatement of the
scan's definition in tests/terrain_check.py, hand-computed answers, the oracle's height-field narrow phase, and the step kernel
handed each env's grid as its own.  The GPU counterpart is tests/test_terrain_gpu.py.

Tolerance of the scan: 1e-12 m absolute.  A value is a dozen fp64 roundings on magnitudes under 10 m (below 2e-14); the bound only has
to absorb a different order of operations.  Points within 1e-9 m of a border between surface pieces (a triangle's edge, a cell border,
the footprint's edge, a box's edge) are left out -- either side is right there -- and fewer than 1 % of the points may be."""
import ctypes

import numpy as np
import pytest

import emu_py
import geometry_randomise_check as gc
import oracle_py
import terrain_check as tc
from cassie_amd import Model
from cassie_amd import phys as P
from cassie_amd._lib import CmModel

SETCONST_GEOMETRY = 2
RANGE = 2.5


def _pelvis(pod):
    return pod.root_body[0]


def emu_scan(pod, qpos, offsets, scan_range=RANGE, **kw):
    """The emulated kernel -> (values [nenv][P], warn [nenv]) (emu_py.height_scan), from the pelvis."""
    return emu_py.height_scan(pod, qpos, offsets, _pelvis(pod), scan_range, **kw)


def _yaw_quat(a):
    a = np.asarray(a, dtype=np.float64)
    return np.stack([np.cos(a / 2), np.zeros_like(a), np.zeros_like(a), np.sin(a / 2)], axis=-1)


def _quat_mul(a, b):
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def _random_quat(rng, n, tilt):
    """Unit quaternions: yaw over the full circle, then a tilt of up to `tilt` rad about a random horizontal axis."""
    yaw = _yaw_quat(rng.uniform(-np.pi, np.pi, n))
    t, d = rng.uniform(0, tilt, n), rng.uniform(-np.pi, np.pi, n)
    tq = np.stack([np.cos(t / 2), np.sin(t / 2) * np.cos(d), np.sin(t / 2) * np.sin(d), np.zeros(n)], axis=-1)
    return _quat_mul(yaw, tq)


def _blocks(pod, gp, gq):
    """Per-env parameter blocks with the geom poses gp [nenv][ngeom][3] / gq [nenv][ngeom][4], their matrices derived by the device's
    set_const kernel (what phys_batch_randomize of CM_P_GEOM_POS / QUAT leaves)."""
    nenv = gp.shape[0]
    params = gc.own_params(pod, nenv)
    params["geom_pos"], params["geom_quat"] = gp.reshape(nenv, -1).copy(), gq.reshape(nenv, -1).copy()
    blocks = gc.new_blocks(pod, nenv, params)
    emu_py.set_const(pod, blocks, nenv, SETCONST_GEOMETRY)
    return blocks


def hfield_case(hf, nenv, seed, nbank=6):
    """cassie_hfield: a bank of distinct grids (flat, ramp, steps, noise, ...), a random index, envs spread over the grid, its edge and
    beyond, yaw over the full circle and some tilt of the pelvis, the height-field geom moved and yawed per env."""
    pod = hf.pod
    rng = np.random.default_rng(seed)
    bank = tc.make_bank(pod.hfield_nrow, pod.hfield_ncol, seed=seed, count=nbank)
    index = rng.integers(0, nbank, nenv).astype(np.int32)
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-5.6, 5.6, (nenv, 2))
    qpos[: nenv // 4, 0] = rng.choice([-5.0, 5.0], nenv // 4) + rng.uniform(-0.8, 0.8, nenv // 4)     # the edge, in and out
    qpos[:, 2] = rng.uniform(0.6, 1.3, nenv)
    qpos[:, 3:7] = _random_quat(rng, nenv, 0.4) * rng.uniform(0.98, 1.02, (nenv, 1))                 # (not quite unit: normalised by the scan)
    gp, gq = tc.model_geom_poses(pod, nenv)
    g = pod.hfield_geom
    gp[:, g] += np.concatenate([rng.uniform(-0.5, 0.5, (nenv, 2)), rng.uniform(-0.2, 0.2, (nenv, 1))], axis=1)
    gq[:, g] = _yaw_quat(rng.uniform(-np.pi, np.pi, nenv))
    return dict(pod=pod, bank=bank, index=index, qpos=qpos, gp=gp, gq=gq)


def stairs_case(cassie, nenv, seed):
    """cassie: the stair boxes brought under the robot and rotated per env (any pose), the floor tilted."""
    pod = cassie.pod
    rng = np.random.default_rng(seed)
    qpos = np.tile(cassie.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-3, 3, (nenv, 2))
    qpos[:, 2] = rng.uniform(0.7, 1.4, nenv)
    qpos[:, 3:7] = _random_quat(rng, nenv, 0.4)
    gp, gq = tc.model_geom_poses(pod, nenv)
    boxes = [g for g, t in tc.static_geoms(pod) if t == tc.BOX]
    floor = [g for g, t in tc.static_geoms(pod) if t == tc.PLANE][0]
    for k, g in enumerate(boxes[:6]):
        half = np.array(list(pod.geom_size[g]))
        gp[:, g, 0:2] = qpos[:, 0:2] + rng.uniform(-1.6, 1.6, (nenv, 2))
        gp[:, g, 2] = -half[2] + rng.uniform(0.02, 0.5, nenv)
        gq[:, g] = _random_quat(rng, nenv, 0.5 if k % 2 else 0.0)
    gq[:, floor] = _random_quat(rng, nenv, 0.15)
    return dict(pod=pod, qpos=qpos, gp=gp, gq=gq, boxes=boxes, floor=floor)


# ------------------------------------------------------------------ 1. the emulated kernel against the definition ----
def test_scan_matches_the_definition_on_the_height_field_model(built):
    hf = Model("cassie_hfield")
    c = hfield_case(hf, 96, seed=5)
    pod, offsets = c["pod"], tc.grid_pattern()
    assert offsets.shape[0] == 187                                    # three passes of the wave over the pattern
    assert len({g.tobytes() for g in c["bank"]}) >= 4
    want, near, tilted = tc.scan(pod, c["qpos"], offsets, RANGE, c["gp"], c["gq"], c["bank"][c["index"]])
    assert not tilted.any()
    inside = np.abs(want) < RANGE
    assert 0.3 < inside.mean() < 0.95 and (want == RANGE).any()     # on the grid, over its edge, and beyond it
    blocks = _blocks(pod, c["gp"], c["gq"])
    n = pod.hfield_nrow * pod.hfield_ncol
    got, warn = emu_scan(pod, c["qpos"], offsets, blocks=blocks, hfield=c["bank"].reshape(-1), stride=n, index=c["index"], nterrain=len(c["bank"]))
    tc.compare(got, want, near)
    assert not warn.any()
    # the same grids handed in as every env's own (per-env mode), and a range of the batch through a small grid of workgroups
    own = np.ascontiguousarray(c["bank"][c["index"]]).reshape(-1)
    got2, _ = emu_scan(pod, c["qpos"], offsets, blocks=blocks, hfield=own, stride=n)
    assert np.array_equal(got, got2)
    part = np.full_like(got, -7.0)
    emu_scan(pod, c["qpos"], offsets, blocks=blocks, hfield=own, stride=n, env0=10, n=50, grid=3, out=part)
    assert np.array_equal(part[10:60], got[10:60]) and np.all(part[:10] == -7.0) and np.all(part[60:] == -7.0)


def test_scan_matches_the_definition_on_stairs_and_a_tilted_floor(cassie):
    c = stairs_case(cassie, 64, seed=11)
    pod, offsets = c["pod"], tc.grid_pattern()
    want, near, _ = tc.scan(pod, c["qpos"], offsets, RANGE, c["gp"], c["gq"])
    gp0, _ = tc.model_geom_poses(pod, 64)                               # (the boxes where the model has them, far away: the floor alone)
    on_box = want < tc.scan(pod, c["qpos"], offsets, RANGE, gp0, c["gq"])[0] - 1e-6
    assert on_box.mean() > 0.1 and (~on_box).mean() > 0.1
    got, warn = emu_scan(pod, c["qpos"], offsets, blocks=_blocks(pod, c["gp"], c["gq"]))
    tc.compare(got, want, near)
    assert not warn.any()
    # without per-env blocks the scan reads the model's own poses: the floor alone under a robot near the origin
    got0, _ = emu_scan(pod, c["qpos"], offsets)
    want0, near0, _ = tc.scan(pod, c["qpos"], offsets, RANGE)
    tc.compare(got0, want0, near0)
    assert np.allclose(got0, np.clip(c["qpos"][:, 2:3], -RANGE, RANGE), atol=1e-12)


# ------------------------------------------------------------------ 2. known answers by hand ----
def test_flat_grid_ramp_and_footprint_by_hand(built):
    hf = Model("cassie_hfield")
    pod = hf.pod
    nr, nc, n = pod.hfield_nrow, pod.hfield_ncol, pod.hfield_nrow * pod.hfield_ncol
    sx, sz = pod.hfield_size[0], pod.hfield_size[2]
    gz = pod.geom_pos[pod.hfield_geom][2]
    offsets = tc.grid_pattern()
    rng = np.random.default_rng(2)
    nenv = 8
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-3, 3, (nenv, 2))
    qpos[:, 2] = rng.uniform(0.7, 1.2, nenv)
    qpos[:, 3:7] = _yaw_quat(rng.uniform(-np.pi, np.pi, nenv))
    qpos[7, 0:2] = [30.0, -40.0]                                   # far from the grid: nothing under it, no floor in this model
    h = 0.375
    flat = np.full((nr, nc), h, dtype=np.float32)
    got, _ = emu_scan(pod, qpos, offsets, hfield=flat.reshape(-1))
    want = qpos[:, 2:3] - (gz + sz * h) + np.zeros_like(got)
    assert np.max(np.abs(got[:7] - want[:7])) <= 1e-12
    assert np.all(got[7] == RANGE)
    # a ramp along x: elevation rises linearly from 0 at x = -sx to 1 at x = +sx, so the surface is linear in the world X of the point
    ramp = np.tile(np.linspace(0.0, 1.0, nc), (nr, 1)).astype(np.float32)
    got, _ = emu_scan(pod, qpos, offsets, hfield=ramp.reshape(-1))
    pos, quat = tc.pelvis_pose(qpos)
    X, _ = tc.world_points(pos, quat, offsets)
    want = qpos[:, 2:3] - (gz + sz * (X + sx) / (2 * sx))
    # (float32 samples: linspace's values are rounded to 2^-24 relative, the surface between them is the chord: 1.2e-8 m at most)
    assert np.max(np.abs(got[:7] - want[:7])) <= sz * 2.0 ** -23
    exact = np.tile((np.arange(nc) / 256.0), (nr, 1)).astype(np.float32)       # samples exact in float32: the surface is exactly linear
    got, _ = emu_scan(pod, qpos, offsets, hfield=exact.reshape(-1))
    want = qpos[:, 2:3] - (gz + sz * ((X + sx) / (2 * sx) * (nc - 1)) / 256.0)
    assert np.max(np.abs(got[:7] - want[:7])) <= 1e-12
    # no samples at all: a miss everywhere
    got, _ = emu_scan(pod, qpos, offsets)
    assert np.all(got == RANGE)
    # the clamp: a robot high above the ground reads +range, one far below it -range
    qpos[0, 2], qpos[1, 2] = 9.0, -9.0
    got, _ = emu_scan(pod, qpos, offsets, hfield=flat.reshape(-1))
    assert np.all(got[0] == RANGE) and np.all(got[1] == -RANGE)


def test_one_stair_box_under_the_robot_by_hand(cassie):
    pod = cassie.pod
    box = [g for g, t in tc.static_geoms(pod) if t == tc.BOX][0]
    half = np.array(list(pod.geom_size[box]))
    nenv = 6
    rng = np.random.default_rng(4)
    qpos = np.tile(cassie.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-1, 1, (nenv, 2))
    qpos[:, 3:7] = _yaw_quat(rng.uniform(-np.pi, np.pi, nenv))
    gp, gq = tc.model_geom_poses(pod, nenv)
    a = rng.uniform(-np.pi, np.pi, nenv)
    top = rng.uniform(0.05, 0.4, nenv)
    gp[:, box, 0:2] = qpos[:, 0:2] + rng.uniform(-0.9, 0.9, (nenv, 2))
    gp[:, box, 2] = top - half[2]
    gq[:, box] = _yaw_quat(a)
    offsets = tc.grid_pattern(21, 21, 0.17)
    got, _ = emu_scan(pod, qpos, offsets, blocks=_blocks(pod, gp, gq))
    pos, quat = tc.pelvis_pose(qpos)
    X, Y = tc.world_points(pos, quat, offsets)
    dx, dy = X - gp[:, box, 0:1], Y - gp[:, box, 1:2]
    lx = np.cos(a)[:, None] * dx + np.sin(a)[:, None] * dy        # the point in the box's yawed frame
    ly = -np.sin(a)[:, None] * dx + np.cos(a)[:, None] * dy
    margin = np.minimum(np.abs(np.abs(lx) - half[0]), np.abs(np.abs(ly) - half[1]))
    on = (np.abs(lx) <= half[0]) & (np.abs(ly) <= half[1])
    floor_z = pod.geom_pos[0][2]
    want = np.where(on, qpos[:, 2:3] - top[:, None], qpos[:, 2:3] - floor_z)
    clear = margin > 1e-9
    assert on.any() and (~on).any() and clear.mean() > 0.99
    assert np.max(np.abs(got - want)[clear]) <= 1e-12


# ------------------------------------------------------------------ 3. the scan reads the collision's surface ----
def _probe(pod, ps, r):
    L = oracle_py.lib()
    L.co_test_hfield_sphere.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    out = np.zeros(7)
    p = np.ascontiguousarray(ps, dtype=np.float64)
    n = L.co_test_hfield_sphere(ctypes.byref(pod), p.ctypes.data, r, 0.0, out.ctypes.data)
    return n, out[0]


@pytest.mark.parametrize("kind", ["rough", "flat"])
def test_scanned_surface_is_the_one_the_narrow_phase_collides_with(built, kind):
    """A sphere of radius r whose centre is r - delta above the scanned surface is in contact, at least delta deep (the closest point
    of the surface is no further than the point straight below); on the flat grid exactly delta deep."""
    hf = Model("cassie_hfield")
    pod = hf.pod
    rng = np.random.default_rng(8)
    grid = (rng.random((pod.hfield_nrow, pod.hfield_ncol)) if kind == "rough" else np.full((pod.hfield_nrow, pod.hfield_ncol), 0.25)).astype(np.float32)
    nenv = 6
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-4, 4, (nenv, 2))
    qpos[:, 3:7] = _yaw_quat(rng.uniform(-np.pi, np.pi, nenv))
    offsets = tc.grid_pattern(5, 4, 0.13)
    got, _ = emu_scan(pod, qpos, offsets, hfield=grid.reshape(-1))
    pos, quat = tc.pelvis_pose(qpos)
    X, Y = tc.world_points(pos, quat, offsets)
    S = qpos[:, 2:3] - got
    delta = 1e-3
    oracle_py.set_hfield(grid)
    try:
        for e in range(nenv):
            for j in range(offsets.shape[0]):
                for r in (0.02, 0.08):
                    n, dist = _probe(pod, [X[e, j], Y[e, j], S[e, j] + r - delta], r)
                    assert n == 1 and dist <= -delta + 1e-12, (e, j, r, dist)
                    if kind == "flat":
                        assert abs(dist + delta) <= 1e-12
    finally:
        oracle_py.set_hfield(None)


# ------------------------------------------------------------------ 4. the terrain index in the step kernel ----
def _run_terrain(pod, state, nsub, hfield, stride, index=None, nterrain=0):
    state.hfield, state.hfield_stride, state.nterrain = hfield, stride, nterrain
    state.hfield_index = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    state.step(nsub)


def _fresh(hf, nenv):
    b = emu_py.EmuBatch(hf.pod, nenv)
    b.qpos[:] = hf.qpos_init()
    b.qpos[:, 0] = [0.0, 0.35, -0.6, 0.9][:nenv]               # the flat start patch, its edge, the rough part
    b.qpos[:, 2] -= 0.06                                       # (a shorter drop: the feet land within 200 steps)
    return b


def _same(a, b):
    for f in ("qpos", "qvel", "qacc_warmstart", "qacc", "sensordata", "actuator_velocity", "time", "warn", "info"):
        if not np.array_equal(getattr(a, f), getattr(b, f)):
            return False
    return True


def _step_bank(pod, count):
    """Rough terrains with the flat start patch of config 4's workload (tests/test_hfield.py: terrain)."""
    bank = []
    for k in range(count):
        h = np.random.default_rng(100 + k).random((pod.hfield_nrow, pod.hfield_ncol)).astype(np.float32) * (0.4 + 0.2 * k)
        h[95:105, 95:105] = 0
        bank.append(h)
    return np.stack(bank)


@pytest.mark.parametrize("fast", [False, True])
def test_stepping_on_a_bank_equals_stepping_on_the_same_grid_as_the_envs_own(built, fast):
    hf = Model("cassie_hfield")
    pod, nenv = hf.pod, 4
    n = pod.hfield_nrow * pod.hfield_ncol
    bank = _step_bank(pod, 3)
    index = np.array([2, 0, 1, 2], dtype=np.int32)
    with emu_py.settings(fast_rows=1 if fast else 0, two_waves=1 if fast else 0, chunks=2 if fast else 1):
        a, b = _fresh(hf, nenv), _fresh(hf, nenv)
        own = np.ascontiguousarray(bank[index]).reshape(-1)
        for _ in range(6):
            _run_terrain(pod, a, 25, bank.reshape(-1), n, index, len(bank))
            _run_terrain(pod, b, 25, own, n)
            assert _same(a, b)
        assert a.info[:, 0].max() >= 2 and not a.warn.any()          # the robots have landed
        # an index outside the bank is clamped, never followed: the state is that of the clamped terrain, the new bit is raised
        c, d = _fresh(hf, nenv), _fresh(hf, nenv)
        bad = np.array([-1, len(bank), 1, 7], dtype=np.int32)
        for _ in range(6):
            _run_terrain(pod, c, 50, bank.reshape(-1), n, bad, len(bank))
            _run_terrain(pod, d, 50, bank.reshape(-1), n, np.clip(bad, 0, len(bank) - 1), len(bank))
        bit = emu_py.lib().emu_warn_bit(0)
        assert bit == P.WARN_TERRAIN_INDEX == 32
        assert list(c.warn & bit) == [bit, bit, 0, bit] and not (d.warn & bit).any()
        c.warn &= ~np.int32(bit)
        assert _same(c, d)


def test_no_index_is_todays_entry_point_bit_for_bit(built):
    hf = Model("cassie_hfield")
    pod = hf.pod
    grid = _step_bank(pod, 1)[0]
    a, b = _fresh(hf, 2), _fresh(hf, 2)
    b.hfield = grid.reshape(-1).copy()
    most = 0
    for _ in range(8):
        _run_terrain(pod, a, 50, grid.reshape(-1), 0)
        b.step(50)
        assert _same(a, b)
        most = max(most, int(a.info[:, 0].max()))
    assert most >= 2


# ------------------------------------------------------------------ 5. a tilted height-field geom ----
def test_tilted_height_field_geom_is_left_out_and_flagged(built):
    hf = Model("cassie_hfield")
    pod, nenv = hf.pod, 4
    rng = np.random.default_rng(3)
    grid = rng.random((pod.hfield_nrow, pod.hfield_ncol)).astype(np.float32)
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-2, 2, (nenv, 2))
    gp, gq = tc.model_geom_poses(pod, nenv)
    g = pod.hfield_geom
    a = np.radians(3.0) / 2
    gq[1, g] = [np.cos(a), np.sin(a), 0.0, 0.0]                    # tilted about x
    gq[3, g] = _quat_mul(_yaw_quat(np.array([0.7])), np.array([[np.cos(a), 0.0, np.sin(a), 0.0]]))[0]
    gq[2, g] = _yaw_quat(np.array([2.0]))[0]                        # yawed only: scanned
    offsets = tc.grid_pattern()
    got, warn = emu_scan(pod, qpos, offsets, blocks=_blocks(pod, gp, gq), hfield=grid.reshape(-1))
    want, near, tilted = tc.scan(pod, qpos, offsets, RANGE, gp, gq, np.tile(grid, (nenv, 1, 1)))
    assert list(tilted) == [False, True, False, True]
    bit = emu_py.lib().emu_warn_bit(1)
    assert bit == P.WARN_SCAN_TILTED == 64 and list(warn) == [0, bit, 0, bit]
    tc.compare(got, want, near)
    assert np.all(got[1] == RANGE) and np.all(got[3] == RANGE)      # no other static geom in this model: a miss everywhere
    assert np.all(np.abs(got[0]) < RANGE) and np.all(np.abs(got[2]) < RANGE)
