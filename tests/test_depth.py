"""The egocentric depth image on the CPU: the device's kernel (csrc/depth_kernel.h: cassie_depth_kernel) executed by the wave emulator,
against the numpy restatement of its definition in tests/depth_check.py -- itself pinned by brute force over every triangle of the
grid -- and against hand-computed answers.  The GPU counterpart is tests/test_depth_gpu.py.

Tolerance: 1e-11 m absolute off the mask (depth_check.TOL).  A depth is a few dozen fp64 roundings on magnitudes under 10 m, below
1e-13, times at most 1e3 for the grazing bound the mask keeps.  Rays within 1e-9 of a threshold or grazing are left out, and fewer
than 1 % of the rays of any case may be: asserted from the restatement alone, before a kernel result is looked at."""
import numpy as np
import pytest

import depth_check as dc
import depth_emu_py
import emu_py
import terrain_check as tc
from cassie_amd import Model
from cassie_amd import phys as P
from test_terrain import _blocks, _quat_mul, _random_quat, _yaw_quat, stairs_case

W, H, FOVY, NEAR, FAR = 20, 12, 65.5, 0.05, 5.0
CAM_POS = np.array([0.1, 0.0, 0.25])


def _pelvis(pod):
    return pod.root_body[0]


def emu_depth(pod, qpos, cam_quat, cam_pos=CAM_POS, width=W, height=H, fovy=FOVY, near=NEAR, far=FAR, **kw):
    return depth_emu_py.depth_image(pod, qpos, _pelvis(pod), cam_pos, cam_quat, width, height, fovy, near, far, **kw)


def hfield_depth_case(hf, nenv, seed, nbank):
    """cassie_hfield: a bank of grids without vertical faces, a random index, envs over the grid, its edge and beyond, pelvis yaw over
    the full circle with tilt, the height-field geom moved, yawed and tilted (up to 0.3 rad) per env."""
    pod = hf.pod
    rng = np.random.default_rng(seed)
    bank = dc.ramp_noise_flat_bank(pod.hfield_nrow, pod.hfield_ncol, nbank, seed=seed)
    index = rng.integers(0, nbank, nenv).astype(np.int32)
    sx = pod.hfield_size[0]
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-0.8 * sx, 0.8 * sx, (nenv, 2))
    k = nenv // 3
    qpos[:k, 0] = rng.choice([-sx, sx], k) + rng.uniform(-0.8, 0.8, k)                            # the edge, in and out
    qpos[k:k + max(1, nenv // 12), 0] = 3.0 * sx                                                  # beyond it
    qpos[:, 2] = rng.uniform(0.9, 1.6, nenv)
    qpos[:, 3:7] = _random_quat(rng, nenv, 0.3) * rng.uniform(0.98, 1.02, (nenv, 1))              # (not quite unit: normalised by the kernel)
    gp, gq = tc.model_geom_poses(pod, nenv)
    g = pod.hfield_geom
    gp[:, g] += np.concatenate([rng.uniform(-0.5, 0.5, (nenv, 2)), rng.uniform(-0.2, 0.2, (nenv, 1))], axis=1)
    gq[:, g] = _random_quat(rng, nenv, 0.3)
    return dict(pod=pod, bank=bank, index=index, qpos=qpos, gp=gp, gq=gq, cam_quat=dc.pitched_down(45.0))


def stairs_depth_case(cassie, nenv, seed):
    """cassie: stairs_case's boxes (any pose) and tilted floor, some boxes brought in front of the camera; env 0's camera inside a box,
    env 1's below the floor looking up."""
    c = stairs_case(cassie, nenv, seed)
    pod = c["pod"]
    rng = np.random.default_rng(seed + 1)
    cam_quat = dc.pitched_down(30.0)
    yaw = tc.yaw_of(tc.pelvis_pose(c["qpos"])[1])
    for k, g in enumerate(c["boxes"][:3]):                      # ahead of the robot, 0.6 .. 3 m
        ahead = rng.uniform(0.6, 3.0, nenv)
        c["gp"][:, g, 0] = c["qpos"][:, 0] + ahead * np.cos(yaw) + rng.uniform(-0.5, 0.5, nenv)
        c["gp"][:, g, 1] = c["qpos"][:, 1] + ahead * np.sin(yaw) + rng.uniform(-0.5, 0.5, nenv)
    # env 0: box 0 around the camera (level pelvis, the camera 0.25 above and 0.1 ahead of it)
    g = c["boxes"][0]
    c["qpos"][0, 3:7] = [1, 0, 0, 0]
    c["gp"][0, g] = c["qpos"][0, 0:3] + CAM_POS + [0.05, 0.02, -0.03]
    c["gq"][0, g] = [1, 0, 0, 0]
    # env 1: the floor level again, the robot 0.8 m below it and on its back-ish (the camera looks up through the floor)
    c["gq"][1, c["floor"]] = [1, 0, 0, 0]
    gp0, gq0 = tc.model_geom_poses(pod, 1)
    c["gp"][1, c["boxes"]], c["gq"][1, c["boxes"]] = gp0[0, c["boxes"]], gq0[0, c["boxes"]]     # (its boxes where the model has them, far away)
    c["qpos"][1, 2] = pod.geom_pos[c["floor"]][2] - 0.8
    c["qpos"][1, 3:7] = [np.cos(-0.9), 0, np.sin(-0.9), 0]      # pitched up by 1.8 rad about y
    c["cam_quat"] = cam_quat
    return c


@pytest.fixture(scope="module")
def hfield_result(built):
    """Case 1 and what the restatement and the emulator make of it, computed once."""
    hf = Model("cassie_hfield")
    c = hfield_depth_case(hf, 12, seed=31, nbank=4)
    pod = c["pod"]
    want, mask = dc.depth(pod, c["qpos"], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR, c["gp"], c["gq"], c["bank"][c["index"]])
    dc.check_mask(mask)
    c["blocks"] = _blocks(pod, c["gp"], c["gq"])
    n = pod.hfield_nrow * pod.hfield_ncol
    got, warn = emu_depth(pod, c["qpos"], c["cam_quat"], blocks=c["blocks"], hfield=c["bank"].reshape(-1), stride=n, index=c["index"], nterrain=len(c["bank"]))
    return dict(c=c, want=want, mask=mask, got=got, warn=warn)


# ------------------------------------------------------------------ 1. the emulated kernel against the definition ----
def test_depth_matches_the_definition_on_the_height_field_model(hfield_result):
    r = hfield_result
    c, want, mask, got = r["c"], r["want"], r["mask"], r["got"]
    pod = c["pod"]
    assert W % 8 == 4 and H % 8 == 4 and len({g.tobytes() for g in c["bank"]}) == 4       # half-empty tiles, more than one tile per env
    hit = want < FAR
    assert 0.2 < hit.mean() < 0.95                                    # hits, and rays that end at `far`
    assert (~hit[c["qpos"][:, 0] > 2 * pod.hfield_size[0]]).all()     # beyond the footprint: misses
    # (rays clamped at `far` although the surface lies under them further out: the same rays with ten times the range do hit)
    longer, _ = dc.depth(pod, c["qpos"], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, 10 * FAR, c["gp"], c["gq"], c["bank"][c["index"]])
    assert ((want == FAR) & (longer < 10 * FAR)).any()
    dc.compare(got, want, mask, "height field, emulator")
    assert not r["warn"].any()
    # the same grids handed in as every env's own (per-env mode), and a range of the batch through a small grid of workgroups
    n = pod.hfield_nrow * pod.hfield_ncol
    own = np.ascontiguousarray(c["bank"][c["index"]]).reshape(-1)
    got2, _ = emu_depth(pod, c["qpos"], c["cam_quat"], blocks=c["blocks"], hfield=own, stride=n)
    assert got.tobytes() == got2.tobytes()
    part = np.full_like(got, -7.0)
    emu_depth(pod, c["qpos"], c["cam_quat"], blocks=c["blocks"], hfield=own, stride=n, env0=3, n=6, grid=3, out=part)
    assert np.array_equal(part[3:9], got[3:9]) and np.all(part[:3] == -7.0) and np.all(part[9:] == -7.0)


def test_the_restatement_agrees_with_brute_force_over_every_triangle(hfield_result):
    r = hfield_result
    c, want, mask = r["c"], r["want"], r["mask"]
    picks = dc.sample_rays(np.arange(12), 170, W * H, seed=9)
    t = dc.brute_force(c["pod"], c["qpos"], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR, c["gp"], c["gq"], c["bank"][c["index"]], picks)
    assert dc.compare_brute(t, want, mask, picks, FAR, "case 1") > 300


def test_the_restatement_agrees_with_brute_force_on_the_device_case(built):
    """The case the device is judged on (tests/test_depth_gpu.py: 512 envs, 32 x 24, a bank of 8, seed 41): 2000 of its rays, from 20
    envs that between them stand on every terrain of the bank.  (An env's image depends on nothing but the env, so the restatement is
    made for those envs alone.)"""
    hf = Model("cassie_hfield")
    c = hfield_depth_case(hf, 512, seed=41, nbank=8)
    w, h = 32, 24
    envs = np.concatenate([np.nonzero(c["index"] == k)[0][:2] for k in range(8)] + [np.arange(500, 504)])
    assert len(envs) == 20 and set(c["index"][envs]) == set(range(8))
    qpos, gp, gq, grids = c["qpos"][envs], c["gp"][envs], c["gq"][envs], c["bank"][c["index"][envs]]
    want, mask = dc.depth(hf.pod, qpos, CAM_POS, c["cam_quat"], w, h, FOVY, NEAR, FAR, gp, gq, grids)
    dc.check_mask(mask)
    picks = dc.sample_rays(np.arange(20), 100, w * h, seed=10)
    t = dc.brute_force(hf.pod, qpos, CAM_POS, c["cam_quat"], w, h, FOVY, NEAR, FAR, gp, gq, grids, picks)
    assert dc.compare_brute(t, want, mask, picks, FAR, "the device's case") > 300


def test_depth_matches_the_definition_on_stairs_and_a_tilted_floor(cassie):
    c = stairs_depth_case(cassie, 12, seed=13)
    pod = c["pod"]
    want, mask = dc.depth(pod, c["qpos"], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR, c["gp"], c["gq"])
    dc.check_mask(mask)
    gp0, _ = tc.model_geom_poses(pod, 12)                               # (the boxes where the model has them, far away: the floor alone)
    floor_only, _ = dc.depth(pod, c["qpos"], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR, gp0, c["gq"])
    assert (want < floor_only - 1e-6).mean() > 0.05                     # boxes in front of the floor
    assert np.all(want[0] == NEAR)                                      # the camera inside a box
    assert np.all(want[1] < FAR) and np.all(want[1] > NEAR)             # below the floor, looking up: the plane from its back
    got, warn = emu_depth(pod, c["qpos"], c["cam_quat"], blocks=_blocks(pod, c["gp"], c["gq"]))
    dc.compare(got, want, mask, "stairs, emulator")
    assert not warn.any()


# ------------------------------------------------------------------ 2. known answers by hand ----
DOWN = np.array([1.0, 0.0, 0.0, 0.0])          # the camera's frame = the body's: it looks along the body's -z, straight down


def test_straight_down_over_a_flat_floor_is_the_height_in_every_pixel(cassie):
    pod = cassie.pod
    floor_z = pod.geom_pos[0][2]
    qpos = np.tile(cassie.qpos_init(), (2, 1))
    qpos[:, 0:2] = [[0.3, -0.2], [-1.0, 0.4]]
    qpos[:, 2] = floor_z + 1.0
    qpos[1, 3:7] = _yaw_quat(np.array([0.7]))[0]
    zero = np.zeros(3)
    got, _ = emu_depth(pod, qpos, DOWN, cam_pos=zero, width=9, height=7)
    assert np.all(got[:, (7 // 2) * 9 + 9 // 2] == 1.0)               # the centre pixel: the ray is the axis
    assert np.max(np.abs(got - 1.0)) <= 1e-14                          # every pixel: depth is along the axis, not along the ray
    got1, _ = emu_depth(pod, qpos, DOWN, cam_pos=zero, width=1, height=1)
    assert got1.shape == (2, 1) and np.all(got1 == 1.0)               # a 1 x 1 image
    # the near and the far plane: a floor 1 m away is not seen by a camera whose range ends at 0.9 m or starts at 1.1 m
    assert np.all(emu_depth(pod, qpos, DOWN, cam_pos=zero, width=9, height=7, far=0.9)[0] == 0.9)
    assert np.all(emu_depth(pod, qpos, DOWN, cam_pos=zero, width=9, height=7, near=1.1)[0] == FAR)


def test_looking_ahead_at_a_box_face_at_a_known_distance(cassie):
    pod = cassie.pod
    box = [g for g, t in tc.static_geoms(pod) if t == tc.BOX][0]
    half = np.array(list(pod.geom_size[box]))
    qpos = np.tile(cassie.qpos_init(), (1, 1))
    qpos[0, 0:3] = [0.0, 0.0, 30.0]                                     # high above the floor: out of range for every ray
    gp, gq = tc.model_geom_poses(pod, 1)
    dist = 1.75
    gp[0, box] = [dist + half[0], 0.0, 30.0]                            # its near face is the plane x = dist
    gq[0, box] = [1, 0, 0, 0]
    w, h, fovy = 21, 15, 120.0                                          # wide enough to look past the face on every side
    got, _ = emu_depth(pod, qpos, dc.pitched_down(0.0), cam_pos=np.zeros(3), width=w, height=h, fovy=fovy, blocks=_blocks(pod, gp, gq))
    d = dc.pixel_dirs(w, h, fovy)
    # where the ray meets the plane x = dist: camera x (right) is the body's -y, camera y (up) the body's z
    my, mz = half[1] - np.abs(dist * d[:, 0]), half[2] - np.abs(dist * d[:, 1])
    on, off = (my > 1e-9) & (mz > 1e-9), (my < -1e-9) | (mz < -1e-9)
    assert on[(h // 2) * w + w // 2] and on.sum() > 10 and off.sum() > 10 and (on | off).all()
    assert (my[off] < -1e-9).any() and (mz[off] < -1e-9).any()          # past it sideways, and above / below it
    assert np.max(np.abs(got[0][on] - dist)) <= 1e-14
    # past the face the ray meets nothing: the box's other faces are behind the near one, the floor is out of range
    assert np.all(got[0][off] == FAR)


def test_flat_height_field_equals_the_plane_at_its_height(built):
    hf = Model("cassie_hfield")
    pod = hf.pod
    sz, g = pod.hfield_size[2], pod.hfield_geom
    flat = np.full((pod.hfield_nrow, pod.hfield_ncol), 0.5, dtype=np.float32)
    rng = np.random.default_rng(3)
    nenv = 4
    qpos = np.tile(hf.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-2, 2, (nenv, 2))
    qpos[:, 2] = pod.geom_pos[g][2] + sz * 0.5 + rng.uniform(0.5, 1.2, nenv)
    qpos[:, 3:7] = _random_quat(rng, nenv, 0.3)
    cam_quat = dc.pitched_down(45.0)
    got, _ = emu_depth(pod, qpos, cam_quat, hfield=flat.reshape(-1))
    o, D = dc.rays(qpos, CAM_POS, cam_quat, W, H, FOVY)
    t = ((pod.geom_pos[g][2] + sz * 0.5) - o[:, None, 2]) / D[:, :, 2]           # the plane z = geom z + sz / 2
    assert list(pod.geom_quat[g]) == [1, 0, 0, 0]
    px, py = o[:, None, 0] + t * D[:, :, 0] - pod.geom_pos[g][0], o[:, None, 1] + t * D[:, :, 1] - pod.geom_pos[g][1]
    edge = np.minimum(pod.hfield_size[0] - np.abs(px), pod.hfield_size[1] - np.abs(py))       # (the plane is infinite, the grid is not)
    want = np.where((t >= NEAR) & (t <= FAR) & (edge >= 0), t, FAR)
    clear = np.abs(edge) > 1e-9
    assert (want < FAR).mean() > 0.5 and clear.all() and np.max(np.abs(got - want)) <= 1e-12
    # no samples at all: a miss everywhere
    assert np.all(emu_depth(pod, qpos, cam_quat)[0] == FAR)


# ------------------------------------------------------------------ 3. per-env extrinsics ----
def test_per_env_extrinsics_equal_the_shared_pose_bit_for_bit(hfield_result):
    c = hfield_result["c"]
    pod, nenv = c["pod"], 12
    n = pod.hfield_nrow * pod.hfield_ncol
    rng = np.random.default_rng(17)
    pose = np.zeros((nenv, 7))
    pose[:, 0:3] = CAM_POS + rng.uniform(-0.05, 0.05, (nenv, 3))
    tilt = np.stack([np.cos(0.1 * rng.uniform(-1, 1, nenv)), np.zeros(nenv), np.zeros(nenv), np.zeros(nenv)], axis=-1)
    tilt[:, 1:4] = rng.uniform(-0.1, 0.1, (nenv, 3))
    pose[:, 3:7] = _quat_mul(np.tile(c["cam_quat"], (nenv, 1)), tilt) * rng.uniform(0.5, 2.0, (nenv, 1))       # far from unit
    kw = dict(blocks=c["blocks"], hfield=c["bank"].reshape(-1), stride=n, index=c["index"], nterrain=len(c["bank"]))
    got, _ = emu_depth(pod, c["qpos"], c["cam_quat"], pose=pose, **kw)
    for e in range(nenv):
        one, _ = emu_depth(pod, c["qpos"], pose[e, 3:7], cam_pos=pose[e, 0:3], env0=e, n=1, **kw)
        assert one[e].tobytes() == got[e].tobytes(), e
    assert len({got[e].tobytes() for e in range(nenv)}) == nenv
    # the quaternion is normalised: the restatement on the unit quaternions
    unit = pose.copy()
    unit[:, 3:7] = dc.unit(pose[:, 3:7])
    want, mask = dc.depth(pod, c["qpos"], None, None, W, H, FOVY, NEAR, FAR, c["gp"], c["gq"], c["bank"][c["index"]], pose=unit)
    dc.check_mask(mask)
    dc.compare(got, want, mask, "per-env extrinsics, emulator")
    # ... and that restatement against every triangle of the grid
    picks = dc.sample_rays(np.arange(nenv), 170, W * H, seed=12)
    t = dc.brute_force(pod, c["qpos"], None, None, W, H, FOVY, NEAR, FAR, c["gp"], c["gq"], c["bank"][c["index"]], picks, pose=unit)
    assert dc.compare_brute(t, want, mask, picks, FAR, "per-env extrinsics") > 300


# ------------------------------------------------------------------ 4. an index outside the bank (the emulator only) ----
def test_index_outside_the_bank_is_clamped_and_flagged(hfield_result):
    c = hfield_result["c"]
    pod = c["pod"]
    n, nbank = pod.hfield_nrow * pod.hfield_ncol, len(c["bank"])
    bad = c["index"].copy()
    bad[[0, 5, 7]] = [-1, nbank, 9]
    kw = dict(blocks=c["blocks"], hfield=c["bank"].reshape(-1), stride=n, nterrain=nbank)
    got, warn = emu_depth(pod, c["qpos"], c["cam_quat"], index=bad, **kw)
    want, warn0 = emu_depth(pod, c["qpos"], c["cam_quat"], index=np.clip(bad, 0, nbank - 1), **kw)
    bit = emu_py.lib().emu_warn_bit(0)
    assert bit == P.WARN_TERRAIN_INDEX
    assert list(np.nonzero(warn)[0]) == [0, 5, 7] and np.all(warn[[0, 5, 7]] == bit) and not warn0.any()
    assert got.tobytes() == want.tobytes()
