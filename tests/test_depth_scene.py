"""The depth image of a chosen set of geoms, the moving bodies' included, on the CPU: the device's scene kernel (csrc/depth_kernel.h:
cassie_depth_scene_kernel) executed by the wave emulator, against hand-computed answers and against the numpy restatement of its
definition in tests/depth_scene_check.py -- itself pinned by brute force on the solids' signed distance functions.  The GPU counterpart
is tests/test_depth_scene_gpu.py.

Tolerance: depth_check.TOL (1e-11 m) off the mask, as in tests/test_depth.py, whose reasoning carries over: a root of the quadratic
is a few dozen fp64 roundings on magnitudes under 10 m (the discriminant is formed about the ray's closest approach, from terms of
the size of r^2), times at most 1e3 for the grazing bound the mask keeps.  Fewer than 1 % of the rays of any case may be masked:
asserted from the restatement alone, before a kernel result is looked at.  Ids are compared exactly off the id mask.

Largest differences seen off the mask, emulator against restatement: consistent poses 4.9e-15 m, any pose 5.3e-15 m (cassie and
cassie_tray_box); the restatement against brute force 3.8e-15 m.  No ray of any case is masked."""
import numpy as np
import pytest

import depth_check as dc
import depth_emu_py
import depth_scene_check as sc
import depth_scene_emu_py as se
import emu_py
import terrain_check as tc
from cassie_amd import Model
from test_depth import FAR, FOVY, NEAR, stairs_depth_case
from test_terrain import _blocks, _quat_mul, _random_quat

EGO_POS = np.array([0.2, 0.0, 0.2])                 # the reference's `egocentric` camera: 0.2 m ahead of the pelvis and 0.2 m up
NENV = 12


def _pelvis(pod):
    return pod.root_body[0]


def emu_scene(pod, qpos, cam_quat, mask, xpos, xquat, cam_pos=EGO_POS, width=20, height=12, near=NEAR, far=FAR, **kw):
    return se.depth_image(pod, qpos, _pelvis(pod), cam_pos, cam_quat, width, height, FOVY, near, far, mask, xpos, xquat, **kw)


def _uniform_quat(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _quat_conj(q):
    return np.asarray(q, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def hinge_qpos(pod, qpos, rng):
    """Every limited hinge of every env drawn over its range (the legs swing through the camera's view)."""
    for j in range(pod.njnt):
        if pod.jnt_type[j] == 3 and pod.jnt_limited[j]:
            lo, hi = pod.jnt_range[j]
            qpos[:, pod.jnt_qposadr[j]] = rng.uniform(lo, hi, qpos.shape[0])
    return qpos


def emu_forward(pod, qpos):
    """The project's own forward pass on the CPU (the emulated step kernel, integrate = 0) -> xpos [E][nbody * 3], xquat [E][nbody * 4]."""
    eb = emu_py.EmuBatch(pod, qpos.shape[0])
    eb.qpos[:] = qpos
    eb.forward()
    return eb.xpos.copy(), eb.xquat.copy()


def consistent_case(cassie, nenv, seed):
    """stairs_depth_case with the hinges drawn over their ranges, the egocentric camera pitched 45 degrees down in one half of the envs
    and 80 in the other (per-env extrinsics), body poses from the forward pass on that qpos."""
    c = stairs_depth_case(cassie, nenv, seed)
    rng = np.random.default_rng(seed + 7)
    hinge_qpos(c["pod"], c["qpos"], rng)
    pose = np.zeros((nenv, 7))
    pose[:, 0:3] = EGO_POS
    pose[0::2, 3:7], pose[1::2, 3:7] = dc.pitched_down(45.0), dc.pitched_down(80.0)
    c["pose"] = pose
    return c


def any_pose_case(model, nenv, seed, width, height):
    """Every moving body of every env at an independent random rigid pose in a shell 0.3 .. 3 m around the camera, any orientation;
    per-env geometry blocks, in which env 2's capsules have a pose of their own."""
    pod = model.pod
    rng = np.random.default_rng(seed)
    qpos = np.tile(model.qpos_init(), (nenv, 1))
    qpos[:, 0:2] = rng.uniform(-3, 3, (nenv, 2))
    qpos[:, 2] = rng.uniform(0.8, 1.4, nenv)
    qpos[:, 3:7] = _random_quat(rng, nenv, 0.3)
    cam_quat = dc.pitched_down(45.0)
    o, D = dc.rays(qpos, EGO_POS, cam_quat, width, height, FOVY)
    v = rng.normal(size=(nenv, pod.nbody, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True)
    xpos = o[:, None, :] + v * rng.uniform(0.3, 3.0, (nenv, pod.nbody, 1))
    xquat = _uniform_quat(rng, nenv * pod.nbody).reshape(nenv, pod.nbody, 4)
    gp, gq = tc.model_geom_poses(pod, nenv)
    caps = [g for g in range(pod.ngeom) if pod.geom_type[g] == sc.CAPSULE]
    gp[2, caps] += rng.uniform(-0.2, 0.2, (len(caps), 3))
    gq[2, caps] = _uniform_quat(rng, len(caps))
    for g in caps[:3]:                                                  # (three of them about the optical axis, so that env 2 sees some)
        xpos[2, pod.geom_bodyid[g]] = o[2] + D[2].mean(axis=0) * rng.uniform(0.8, 1.5) + rng.uniform(-0.15, 0.15, 3)
    return dict(pod=pod, qpos=qpos, cam_quat=cam_quat, xpos=xpos.reshape(nenv, -1), xquat=xquat.reshape(nenv, -1), gp=gp, gq=gq, caps=caps)


@pytest.fixture(scope="module")
def consistent_result(cassie):
    """Case 2 and what the restatement and the emulator make of it, computed once."""
    c = consistent_case(cassie, NENV, seed=13)
    pod = c["pod"]
    c["xpos"], c["xquat"] = emu_forward(pod, c["qpos"])
    c["blocks"] = _blocks(pod, c["gp"], c["gq"])
    every = sc.all_mask(pod)
    want, ids, mask, id_mask = sc.depth(pod, c["qpos"], None, None, 20, 12, FOVY, NEAR, FAR, every, c["xpos"], c["xquat"], c["gp"], c["gq"],
                                        pose=c["pose"], with_id_mask=True)
    dc.check_mask(mask)
    dc.check_mask(id_mask)
    got, got_ids, warn = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], every, c["xpos"], c["xquat"], pose=c["pose"], blocks=c["blocks"])
    return dict(c=c, want=want, ids=ids, mask=mask, id_mask=id_mask, got=got, got_ids=got_ids, warn=warn)


# ------------------------------------------------------------------ 0. the restatement against brute force ----
@pytest.mark.parametrize("kind,size", [(sc.SPHERE, (0.15, 0, 0)), (sc.CAPSULE, (0.04, 0.2176, 0)), (sc.CAPSULE, (0.08, 0.06, 0)),
                                        (sc.CAPSULE, (0.02, 0.08, 0)), (sc.BOX, (0.14, 0.14, 0.005)), (sc.BOX, (0.05, 0.05, 0.05))])
def test_the_restatement_agrees_with_brute_force_on_the_signed_distance(kind, size):
    """4000 rays per solid, in the solid's frame: the restatement's value against the first sign change of the signed distance along
    the ray.  Rays the restatement flags are left out; so are none else."""
    rng = np.random.default_rng(100 * kind + int(1000 * size[0]))
    half = {sc.SPHERE: [size[0]] * 3, sc.CAPSULE: [size[0], size[0], size[0] + size[1]], sc.BOX: list(size)}[kind]
    o, d = sc.random_rays(rng, 4000, half)
    if kind == sc.CAPSULE:                                              # some along the axis exactly, some across it exactly
        d[100:140, 0:2] = 0.0
        d[140:180, 2] = 0.0
    t, bad, almost = sc.solid(kind, size, o, d, NEAR, FAR)
    want = np.where(np.isfinite(t), t, FAR)
    mask = bad | (almost < want)
    dc.check_mask(mask, most=0.01)
    hits = 0
    err = 0.0
    for lo in range(0, 4000, 500):
        s = slice(lo, lo + 500)
        brute, _ = sc.brute_force_solid(kind, size, o[s], d[s], NEAR, FAR)
        brute = np.where(np.isfinite(brute) & (brute < FAR), brute, FAR)
        err = max(err, float(np.where(mask[s], 0.0, np.abs(brute - want[s])).max()))
        hits += int((brute < FAR).sum())
    print("solid %d %s: %d of 4000 rays hit, %d at `near`, %.3f %% masked, largest difference %.3g m" % (kind, size, hits, int((want == NEAR).sum()), 100 * mask.mean(), err))
    assert 600 < hits < 3600 and (want == NEAR).sum() >= 10             # hits, misses, and origins inside the solid
    assert err <= 1e-12


# ------------------------------------------------------------------ 1. known answers by hand ----
def _by_hand(cassie, geom, desired_quat, D, cam_shift=(0.0, 0.0, 0.0), near=NEAR, far=FAR):
    """A level pelvis 30 m up, the camera at its origin looking along world +x, 21 x 13 (the centre pixel's ray is the optical axis);
    `geom` alone in the mask, its body's row of xpos / xquat written so that the geom sits at distance D ahead with the world
    orientation desired_quat -> (image, ids, the centre pixel)."""
    pod = cassie.pod
    qpos = np.tile(cassie.qpos_init(), (1, 1))
    qpos[0, 0:3] = [0.3, -0.2, 30.0]
    qpos[0, 3:7] = [1, 0, 0, 0]
    body = pod.geom_bodyid[geom]
    gq = np.array(list(pod.geom_quat[geom]))
    gpos = np.array(list(pod.geom_pos[geom]))
    qB = _quat_mul(np.asarray(desired_quat, dtype=np.float64), _quat_conj(gq))          # R(qB) R(gq) = R(desired)
    xpos, xquat = np.zeros((1, pod.nbody, 3)), np.zeros((1, pod.nbody, 4))
    xquat[0, body] = qB
    xpos[0, body] = qpos[0, 0:3] + np.array([D, 0.0, 0.0]) + np.asarray(cam_shift) - tc.quat2mat(qB) @ gpos
    got, ids, _ = emu_scene(pod, qpos, dc.pitched_down(0.0), 1 << geom, xpos, xquat, cam_pos=np.zeros(3), width=21, height=13, near=near, far=far)
    return got[0], ids[0], 6 * 21 + 10


def test_known_answers_sphere_capsule_inside_behind_and_beyond(cassie):
    pod = cassie.pod
    sphere = [g for g in range(pod.ngeom) if pod.geom_type[g] == sc.SPHERE][0]
    shin = [g for g in range(pod.ngeom) if pod.geom_type[g] == sc.CAPSULE and abs(pod.geom_size[g][1] - 0.2176) < 1e-3][0]
    assert pod.geom_size[sphere][0] == 0.15 and pod.geom_size[shin][0] == 0.04 and sc.is_moving(pod, sphere) and sc.is_moving(pod, shin)
    h = pod.geom_size[shin][1]
    upright, end_on = [1.0, 0.0, 0.0, 0.0], [np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0]           # the geom's z along world z / along world x
    D = 0.75
    # the pelvis sphere D ahead: D - r at the centre, the sphere's id where it is seen and -1 elsewhere
    img, ids, centre = _by_hand(cassie, sphere, upright, D)
    assert abs(img[centre] - (D - 0.15)) <= 1e-14 and ids[centre] == sphere
    assert set(np.unique(ids)) == {-1, sphere} and np.all((ids == -1) == (img == FAR)) and 3 < (ids == sphere).sum() < 60
    assert np.all(img[ids == sphere] >= D - 0.15) and np.all(img[ids == sphere] < D)
    # a shin capsule across the optical axis: D - r; end-on: D - h - r
    img, ids, centre = _by_hand(cassie, shin, upright, D)
    assert abs(img[centre] - (D - 0.04)) <= 1e-14 and ids[centre] == shin
    column = img.reshape(13, 21)[:, 10]
    assert np.max(np.abs(column[np.abs(np.arange(13) - 6) <= 1] - (D - 0.04))) <= 1e-14     # the side is a vertical line: the same depth up and down it
    assert set(np.unique(ids)) == {-1, shin}
    img, ids, centre = _by_hand(cassie, shin, end_on, D)
    assert abs(img[centre] - (D - h - 0.04)) <= 1e-14 and ids[centre] == shin
    assert (ids == shin).sum() < 30
    # the camera inside the pelvis sphere: `near` in every pixel
    img, ids, _ = _by_hand(cassie, sphere, upright, 0.05, cam_shift=(0.0, 0.02, -0.03))
    assert np.all(img == NEAR) and np.all(ids == sphere)
    # wholly behind the camera, and beyond `far`: nothing
    for dist in (-1.0, FAR + 1.0):
        for g in (sphere, shin):
            img, ids, _ = _by_hand(cassie, g, upright, dist)
            assert np.all(img == FAR) and np.all(ids == -1)
    # the near plane cuts the sphere (its front is nearer than `near`, its back is not): `near`; a range that ends inside it: the entry
    img, ids, centre = _by_hand(cassie, sphere, upright, 0.5, near=0.45)
    assert img[centre] == 0.45 and ids[centre] == sphere
    img, ids, centre = _by_hand(cassie, sphere, upright, 0.5, near=0.66)
    assert img[centre] == FAR and ids[centre] == -1
    img, ids, centre = _by_hand(cassie, sphere, upright, D, far=D)
    assert abs(img[centre] - (D - 0.15)) <= 1e-14


# ------------------------------------------------------------------ 2. consistent poses ----
def test_consistent_poses_the_robot_sees_its_own_legs(consistent_result):
    r = consistent_result
    c, want, ids = r["c"], r["want"], r["ids"]
    pod = c["pod"]
    moving = np.isin(ids, [g for g in range(pod.ngeom) if sc.is_moving(pod, g)])
    seen = set(np.unique(ids[moving]))
    print("moving geoms in %.1f %% of the pixels: %s" % (100 * moving.mean(), sorted(seen)))
    assert 0.02 < moving.mean() < 0.60 and len(seen) >= 4
    assert (ids == -1).any() and np.isin(ids, [g for g, _ in tc.static_geoms(pod)]).any()
    dc.compare(r["got"], want, r["mask"], "consistent poses, emulator")
    sc.compare_ids(r["got_ids"], ids, r["id_mask"], "consistent poses, emulator")
    assert not r["warn"].any()


# ------------------------------------------------------------------ 3. any pose ----
@pytest.mark.parametrize("name", ["cassie", "cassie_tray_box"])
def test_any_pose_of_every_moving_body(built, name):
    model = Model(name)
    c = any_pose_case(model, NENV, seed=29, width=20, height=12)
    pod = c["pod"]
    every = sc.all_mask(pod)
    want, ids, mask, id_mask = sc.depth(pod, c["qpos"], EGO_POS, c["cam_quat"], 20, 12, FOVY, NEAR, FAR, every, c["xpos"], c["xquat"], c["gp"], c["gq"],
                                        with_id_mask=True)
    dc.check_mask(mask)
    dc.check_mask(id_mask)
    kinds = {pod.geom_type[g] for g in np.unique(ids) if g >= 0 and sc.is_moving(pod, g)}
    assert kinds == ({sc.SPHERE, sc.CAPSULE, sc.BOX} if name == "cassie_tray_box" else {sc.SPHERE, sc.CAPSULE})
    blocks = _blocks(pod, c["gp"], c["gq"])
    got, got_ids, warn = emu_scene(pod, c["qpos"], c["cam_quat"], every, c["xpos"], c["xquat"], blocks=blocks)
    dc.compare(got, want, mask, "any pose, %s, emulator" % name)
    sc.compare_ids(got_ids, ids, id_mask, "any pose, %s, emulator" % name)
    assert not warn.any()
    # env 2's capsules have a pose of their own in its block: the kernel reads it (the model's poses give another image there, and there only)
    gp0, gq0 = tc.model_geom_poses(pod, NENV)
    plain, _, _ = emu_scene(pod, c["qpos"], c["cam_quat"], every, c["xpos"], c["xquat"], blocks=_blocks(pod, gp0, gq0), want_ids=False)
    assert np.isin(ids[2], c["caps"]).any() and (plain[2] != got[2]).any()
    assert np.array_equal(np.delete(plain, 2, axis=0), np.delete(got, 2, axis=0))


# ------------------------------------------------------------------ 4. the mask ----
def test_the_default_mask_is_the_static_kernel_bit_for_bit(consistent_result):
    c = consistent_result["c"]
    pod = c["pod"]
    static = [g for g, _ in tc.static_geoms(pod)]
    assert sc.default_mask(pod) == sum(1 << g for g in static) and sc.default_mask(pod) != sc.all_mask(pod)
    old, _ = depth_emu_py.depth_image(pod, c["qpos"], _pelvis(pod), EGO_POS, c["pose"][0, 3:7], 20, 12, FOVY, NEAR, FAR, pose=c["pose"], blocks=c["blocks"])
    new, ids, _ = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.default_mask(pod), c["xpos"], c["xquat"], pose=c["pose"], blocks=c["blocks"])
    assert new.tobytes() == old.tobytes()
    assert set(np.unique(ids)) <= set(static) | {-1} and np.all((ids == -1) == (new == FAR))
    # ... and without body poses at all
    none, _, _ = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.default_mask(pod), None, None, pose=c["pose"], blocks=c["blocks"])
    assert none.tobytes() == old.tobytes()


def test_a_mask_hides_exactly_its_geoms(consistent_result):
    r = consistent_result
    c, all_img, all_ids = r["c"], r["got"], r["got_ids"]
    pod = c["pod"]
    kw = dict(pose=c["pose"], blocks=c["blocks"])
    moving_only, ids, _ = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.moving_mask(pod), c["xpos"], c["xquat"], **kw)
    static_won = ~np.isin(all_ids, [g for g in range(pod.ngeom) if sc.is_moving(pod, g)])
    assert static_won.any() and (~static_won).any()
    assert np.array_equal(moving_only[~static_won], all_img[~static_won]) and np.array_equal(ids[~static_won], all_ids[~static_won])
    hidden = static_won & ~np.isin(ids, [g for g in range(pod.ngeom) if sc.is_moving(pod, g)])     # (a leg behind a stair shows once the stair is gone)
    assert np.all(moving_only[hidden] == FAR) and np.all(ids[hidden] == -1) and hidden.sum() > 0.2 * static_won.sum()
    assert np.all(moving_only[static_won] >= all_img[static_won])
    sphere = [g for g in range(pod.ngeom) if pod.geom_type[g] == sc.SPHERE][0]
    no_sphere, ids2, _ = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.all_mask(pod) & ~(1 << sphere), c["xpos"], c["xquat"], **kw)
    was = all_ids == sphere
    assert np.array_equal(no_sphere[~was], all_img[~was]) and np.array_equal(ids2[~was], all_ids[~was])
    assert not (ids2 == sphere).any() and (not was.any() or np.all(no_sphere[was] > all_img[was]))
    # a bit at or above ngeom is refused
    assert se.lib().emu_depth_scene_image is not None
    with pytest.raises(AssertionError):
        emu_scene(pod, c["qpos"], c["pose"][0, 3:7], 1 << pod.ngeom, c["xpos"], c["xquat"], **kw)


# ------------------------------------------------------------------ 5. a range through a small grid ----
def test_a_range_through_a_small_grid_leaves_the_other_rows_alone(consistent_result):
    r = consistent_result
    c = r["c"]
    pod = c["pod"]
    part, part_ids = np.full_like(r["got"], -7.0), np.full_like(r["got_ids"], -7)
    emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.all_mask(pod), c["xpos"], c["xquat"], pose=c["pose"], blocks=c["blocks"], env0=3, n=6, grid=3,
              out=part, ids=part_ids)
    assert np.array_equal(part[3:9], r["got"][3:9]) and np.all(part[:3] == -7.0) and np.all(part[9:] == -7.0)
    assert np.array_equal(part_ids[3:9], r["got_ids"][3:9]) and np.all(part_ids[:3] == -7) and np.all(part_ids[9:] == -7)


# ------------------------------------------------------------------ 6. NaN body poses (the emulator only) ----
def test_nan_body_poses_leave_the_static_image(consistent_result):
    r = consistent_result
    c = r["c"]
    pod = c["pod"]
    kw = dict(pose=c["pose"], blocks=c["blocks"])
    static, _, _ = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.default_mask(pod), c["xpos"], c["xquat"], **kw)
    moving = [g for g in range(pod.ngeom) if sc.is_moving(pod, g)]
    for field in ("xpos", "xquat"):
        bad = {k: c[k].copy() for k in ("xpos", "xquat")}
        e = int(np.argmax(np.isin(r["got_ids"], moving).sum(axis=1)))          # the env that sees most of itself
        bad[field][e] = np.nan
        got, ids, warn = emu_scene(pod, c["qpos"], c["pose"][0, 3:7], sc.all_mask(pod), bad["xpos"], bad["xquat"], **kw)
        assert got[e].tobytes() == static[e].tobytes() and not np.isin(ids[e], moving).any() and (got[e] != r["got"][e]).any()
        assert np.array_equal(np.delete(got, e, axis=0), np.delete(r["got"], e, axis=0))
        want, wids, mask = sc.depth(pod, c["qpos"], None, None, 20, 12, FOVY, NEAR, FAR, sc.all_mask(pod), bad["xpos"], bad["xquat"], c["gp"], c["gq"], pose=c["pose"])
        dc.compare(got, want, mask, "NaN %s, emulator" % field)
        assert not np.isin(wids[e], moving).any()
