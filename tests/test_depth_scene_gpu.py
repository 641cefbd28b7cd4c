"""The depth image of a chosen set of geoms, the moving bodies' included, on the MI355X: cassie_depth_scene_kernel against the numpy
restatement of its definition (tests/depth_scene_check.py, same bound and cap as on the emulator: tests/test_depth_scene.py), against
the wave emulator on the same case, the default image against a batch that never touches the new calls, queued behind stepping
launches with nothing synchronised, and what the Python layer refuses.

Largest differences seen off the mask, device against restatement: consistent poses 6.7e-14 m, any pose 8.0e-15 m (cassie) and
1.1e-14 m (cassie_tray_box), behind three step launches 4.1e-15 m; device against emulator 7.9e-15 m.  No ray of any case is masked."""
import numpy as np
import pytest

import bench
import depth_check as dc
import depth_scene_check as sc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from test_depth import CAM_POS, FAR, FOVY, NEAR, stairs_depth_case
from test_depth_scene import EGO_POS, any_pose_case, consistent_case
from test_depth_scene import consistent_result  # noqa: F401  (the module-scoped fixture: CPU case 2, its restatement and the emulator's image)
from test_episodes_gpu import make

pytestmark = pytest.mark.gpu

NENV, W, H = 256, 32, 24


def _device_scene(model, c, width, height, mask, forward):
    """The case on the device: per-env geometry through randomize; body poses from Batch.forward() on the uploaded qpos (forward=True)
    or uploaded as the case has them; the image on two ranges and two streams, written through a strided binding into the middle
    columns of a wider tensor, the ids into an int32 tensor -> (images, ids, warning words, xpos, xquat as the device holds them)."""
    import torch
    pod, n, npix = model.pod, c["qpos"].shape[0], width * height
    left, right = 3, 6
    b = Batch(model, n)
    try:
        b.set(P.F_QPOS, c["qpos"])
        b.randomize(P.P_GEOM_POS, c["gp"].reshape(n, -1))
        b.randomize(P.P_GEOM_QUAT, c["gq"].reshape(n, -1))
        if forward:
            b.forward()
            b.sync()
            b.clear_warnings()          # (the forward pass's own: hinges drawn over their whole ranges fill its contact and row buffers)
        else:
            b.set(P.F_XPOS, c["xpos"])
            b.set(P.F_XQUAT, c["xquat"])
        cam_quat = c["pose"][0, 3:7] if "pose" in c else c["cam_quat"]
        b.configure_depth(pod.root_body[0], EGO_POS, cam_quat, width, height, FOVY, NEAR, FAR)
        assert b.depth_geoms(mask) == mask
        obs = torch.full((n, left + npix + right), -3.25, dtype=torch.float64, device="cuda")
        b.bind(P.F_DEPTH, obs.data_ptr() + 8 * left, row_stride=left + npix + right)
        ids = torch.full((n, npix), -9, dtype=torch.int32, device="cuda")
        b.bind_depth_ids(ids.data_ptr())
        pose_d = None
        if "pose" in c:
            pose_d = torch.from_numpy(np.ascontiguousarray(c["pose"])).cuda()
            b.bind_depth_pose(pose_d.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        half = n // 2
        for (e0, cnt), st in zip([(0, half), (half, n - half)], streams):
            b.depth_image(e0, cnt, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        assert b.depth_launches() == (0, 2)
        o = obs.cpu().numpy()
        assert np.all(o[:, :left] == -3.25) and np.all(o[:, left + npix:] == -3.25)
        assert np.array_equal(b.get(P.F_DEPTH), o[:, left:left + npix])
        return o[:, left:left + npix].copy(), ids.cpu().numpy(), b.warnings()[0], b.get(P.F_XPOS), b.get(P.F_XQUAT)
    finally:
        b.close()


# ------------------------------------------------------------------ 1. the device against the definition ----
def test_consistent_poses_on_the_device_256_envs(cassie):
    c = consistent_case(cassie, NENV, seed=43)
    pod = c["pod"]
    every = sc.all_mask(pod)
    got, got_ids, warn, xpos, xquat = _device_scene(cassie, c, W, H, every, forward=True)
    assert np.abs(xpos.reshape(NENV, -1, 3)[:, pod.root_body[0]] - c["qpos"][:, 0:3]).max() < 1e-12       # the forward pass ran on this qpos
    want, ids, mask, id_mask = sc.depth(pod, c["qpos"], None, None, W, H, FOVY, NEAR, FAR, every, xpos, xquat, c["gp"], c["gq"], pose=c["pose"],
                                        with_id_mask=True)
    dc.check_mask(mask)
    dc.check_mask(id_mask)
    moving = np.isin(ids, [g for g in range(pod.ngeom) if sc.is_moving(pod, g)])
    assert 0.02 < moving.mean() < 0.60 and len(set(np.unique(ids[moving]))) >= 4
    dc.compare(got, want, mask, "consistent poses, device")
    sc.compare_ids(got_ids, ids, id_mask, "consistent poses, device")
    assert not warn.any()


@pytest.mark.parametrize("name", ["cassie", "cassie_tray_box"])
def test_any_pose_on_the_device_256_envs(built, name):
    model = Model(name)
    c = any_pose_case(model, NENV, seed=47, width=W, height=H)
    pod = c["pod"]
    every = sc.all_mask(pod)
    want, ids, mask, id_mask = sc.depth(pod, c["qpos"], EGO_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR, every, c["xpos"], c["xquat"], c["gp"], c["gq"],
                                        with_id_mask=True)
    dc.check_mask(mask)
    dc.check_mask(id_mask)
    kinds = {pod.geom_type[g] for g in np.unique(ids) if g >= 0 and sc.is_moving(pod, g)}
    assert kinds == ({sc.SPHERE, sc.CAPSULE, sc.BOX} if name == "cassie_tray_box" else {sc.SPHERE, sc.CAPSULE})
    got, got_ids, warn, xpos, xquat = _device_scene(model, c, W, H, every, forward=False)
    assert xpos.tobytes() == c["xpos"].tobytes() and xquat.tobytes() == c["xquat"].tobytes()
    dc.compare(got, want, mask, "any pose, %s, device" % name)
    sc.compare_ids(got_ids, ids, id_mask, "any pose, %s, device" % name)
    assert not warn.any()


# ------------------------------------------------------------------ 2. the device against the emulator ----
def test_the_device_equals_the_emulator(cassie, consistent_result):
    """Case 2 of tests/test_depth_scene.py with the body poses the emulator's forward pass gave it: within the bound, not bit for bit
    (the device contracts FMAs where the emulator's build does not)."""
    r = consistent_result
    c = r["c"]
    got, got_ids, warn, _, _ = _device_scene(cassie, c, 20, 12, sc.all_mask(c["pod"]), forward=False)
    dc.compare(got, r["got"], r["mask"], "device against emulator")
    sc.compare_ids(got_ids, r["got_ids"], r["id_mask"], "device against emulator")
    assert not warn.any()


# ------------------------------------------------------------------ 3. the default is the static kernel's image ----
def test_the_default_mask_is_the_image_of_a_batch_that_never_asks(cassie):
    c = stairs_depth_case(cassie, NENV, seed=42)
    pod, n = cassie.pod, NENV
    images = []
    for ask in (False, True):
        b = Batch(cassie, n)
        try:
            b.set(P.F_QPOS, c["qpos"])
            b.randomize(P.P_GEOM_POS, c["gp"].reshape(n, -1))
            b.randomize(P.P_GEOM_QUAT, c["gq"].reshape(n, -1))
            b.forward()
            b.configure_depth(pod.root_body[0], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR)
            assert b.depth_default_geoms() == sc.default_mask(pod) and b.depth_all_geoms() == sc.all_mask(pod)
            if ask:
                b.depth_geoms(moving=True)
                assert b.depth_geoms(b.depth_default_geoms()) == sc.default_mask(pod)
            b.depth_image()
            b.sync()
            assert b.depth_launches() == (1, 0)                         # the static kernel, whether asked or not
            images.append(b.get(P.F_DEPTH))
        finally:
            b.close()
    assert images[0].tobytes() == images[1].tobytes()
    want, mask = dc.depth(pod, c["qpos"], CAM_POS, c["cam_quat"], W, H, FOVY, NEAR, FAR, c["gp"], c["gq"])
    dc.compare(images[0], want, mask, "the default image, device")


# ------------------------------------------------------------------ 4. nothing synchronised ----
def test_the_image_follows_the_step_launches_with_nothing_synchronised(cassie):
    """Three policy steps of step_range(..., 50), then depth_image with all geoms, on one stream with no synchronisation between them:
    the image is that of the qpos, xpos and xquat the launches in front of it left."""
    import torch
    pod, n, w, h = cassie.pod, NENV, 16, 12
    rng = np.random.default_rng(23)
    qpos = np.tile(cassie.qpos_init(), (n, 1))
    qpos[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    yaw = rng.uniform(-np.pi, np.pi, n)
    qpos[:, 3:7] = np.stack([np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)], axis=-1)
    cam_quat = dc.pitched_down(85.0)                                           # (steep enough to look at its own pelvis and hips)
    tg = bench.pd_targets(np.arange(n), 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE, qpos=qpos)
    try:
        b.configure_depth(pod.root_body[0], EGO_POS, cam_quat, w, h, FOVY, NEAR, FAR)
        every = b.depth_geoms(moving=True)
        ids_d = torch.full((n, w * h), -9, dtype=torch.int32, device="cuda")
        b.bind_depth_ids(ids_d.data_ptr())
        tg_d = torch.from_numpy(tg).cuda()
        ptarget = torch.zeros((n, 10), dtype=torch.float64, device="cuda")
        b.bind(P.F_PD_PTARGET, ptarget.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for p in range(3):
                ptarget.copy_(tg_d[p])
                b.step_range(0, n, 50, st.cuda_stream)
            b.depth_image(0, n, stream=st.cuda_stream)
        torch.cuda.synchronize()
        q, xpos, xquat, got = b.get(P.F_QPOS), b.get(P.F_XPOS), b.get(P.F_XQUAT), b.get(P.F_DEPTH)
        assert np.abs(q - qpos).max() > 1e-3                                   # the envs have moved on
        want, ids, mask, id_mask = sc.depth(pod, q, EGO_POS, cam_quat, w, h, FOVY, NEAR, FAR, every, xpos, xquat, with_id_mask=True)
        dc.check_mask(mask)
        moving = np.isin(ids, [g for g in range(pod.ngeom) if sc.is_moving(pod, g)])
        assert moving.mean() > 0.02                                            # the robot sees its own legs
        dc.compare(got, want, mask, "behind three step launches")
        sc.compare_ids(ids_d.cpu().numpy(), ids, id_mask, "behind three step launches")
        start, _, _ = sc.depth(pod, qpos, EGO_POS, cam_quat, w, h, FOVY, NEAR, FAR, every, xpos, xquat)
        assert (np.abs(got - start) > 1e-6).mean() > 0.05                      # ... and not the image of the start state
    finally:
        b.close()


# ------------------------------------------------------------------ 5. what the Python layer refuses ----
def test_python_layer_refuses(cassie):
    import torch
    pod = cassie.pod
    q = dc.pitched_down(85.0)                                          # (steep enough for the standing robot to see itself)
    b = Batch(cassie, 8)
    try:
        ids = torch.zeros((8, 64), dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError):
            b.depth_geoms(moving=True)                                 # not configured
        with pytest.raises(RuntimeError):
            b.bind_depth_ids(ids.data_ptr())
        b.configure_depth(pod.root_body[0], EGO_POS, q, 8, 8, FOVY, NEAR, FAR)
        with pytest.raises(ValueError):
            b.depth_geoms(1 << pod.ngeom)                              # a bit at ngeom
        with pytest.raises(ValueError):
            b.depth_geoms(-1)
        with pytest.raises(ValueError):
            b.depth_geoms()                                            # neither a mask nor moving=
        with pytest.raises(ValueError):
            b.depth_geoms(3, moving=True)
        assert b.depth_geoms(moving=True) == sc.all_mask(pod)
        b.bind_depth_ids(ids.data_ptr())
        b.forward()
        b.depth_image()
        b.sync()
        assert b.depth_launches() == (0, 1)
        seen = set(np.unique(ids.cpu().numpy()))
        assert seen <= set(range(pod.ngeom)) | {-1} and len(seen) > 1
        # configuring again restores the default mask and drops the ids: the static kernel runs, the ids stay as they were
        b.configure_depth(pod.root_body[0], EGO_POS, q, 8, 8, FOVY, NEAR, FAR)
        ids.fill_(-5)
        b.depth_image()
        b.sync()
        torch.cuda.synchronize()
        assert b.depth_launches() == (1, 1) and bool((ids == -5).all())
        assert b.depth_geoms(moving=False) == sc.default_mask(pod)
        b.bind_depth_ids(None)
    finally:
        b.close()
