"""The egocentric depth image on the MI355X: cassie_depth_kernel against the numpy restatement of its definition
(tests/depth_check.py, same bound and cap as on the emulator: tests/test_depth.py), against the wave emulator on the same case, queued
behind stepping and episode launches with nothing synchronised, and what the Python layer refuses.  No test here hands the device an
index outside the bank."""
import numpy as np
import pytest

import bench
import depth_check as dc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from test_depth import CAM_POS, FAR, FOVY, NEAR, hfield_depth_case, stairs_depth_case
from test_depth import hfield_result  # noqa: F401  (the module-scoped fixture: case 1, its restatement and the emulator's image)
from test_episodes_gpu import bank_states, make

pytestmark = pytest.mark.gpu


def _device_depth(model, c, width, height, bank=None, index=None, pose=None):
    """The case on the device: per-env geometry through randomize, the image on two ranges and two streams, written through a strided
    binding into the middle columns of a wider tensor -> (images, warning words)."""
    import torch
    pod, n, npix = model.pod, c["qpos"].shape[0], width * height
    left, right = 3, 6
    b = Batch(model, n)
    try:
        if bank is not None:
            b.set_hfield_bank(bank)
            b.set_terrain(index)
        b.set(P.F_QPOS, c["qpos"])
        b.randomize(P.P_GEOM_POS, c["gp"].reshape(n, -1))
        b.randomize(P.P_GEOM_QUAT, c["gq"].reshape(n, -1))
        b.configure_depth(pod.root_body[0], CAM_POS, c["cam_quat"], width, height, FOVY, NEAR, FAR)
        assert b.dim(P.F_DEPTH) == npix
        obs = torch.full((n, left + npix + right), -3.25, dtype=torch.float64, device="cuda")
        b.bind(P.F_DEPTH, obs.data_ptr() + 8 * left, row_stride=left + npix + right)
        pose_d = None
        if pose is not None:
            pose_d = torch.from_numpy(np.ascontiguousarray(pose)).cuda()
            b.bind_depth_pose(pose_d.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        half = n // 2
        for (e0, cnt), st in zip([(0, half), (half, n - half)], streams):
            b.depth_image(e0, cnt, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        o = obs.cpu().numpy()
        assert np.all(o[:, :left] == -3.25) and np.all(o[:, left + npix:] == -3.25)
        assert np.array_equal(b.get(P.F_DEPTH), o[:, left:left + npix])
        return o[:, left:left + npix].copy(), b.warnings()[0]
    finally:
        b.close()


def test_depth_on_the_device_512_envs_height_field(built):
    hf = Model("cassie_hfield")
    c = hfield_depth_case(hf, 512, seed=41, nbank=8)
    w, h = 32, 24
    want, mask = dc.depth(hf.pod, c["qpos"], CAM_POS, c["cam_quat"], w, h, FOVY, NEAR, FAR, c["gp"], c["gq"], c["bank"][c["index"]])
    dc.check_mask(mask)
    assert 0.2 < (want < FAR).mean() < 0.95
    got, warn = _device_depth(hf, c, w, h, c["bank"], c["index"])
    dc.compare(got, want, mask, "height field, device")
    assert not warn.any()


def test_depth_on_the_device_512_envs_stairs(cassie):
    c = stairs_depth_case(cassie, 512, seed=42)
    w, h = 32, 24
    want, mask = dc.depth(cassie.pod, c["qpos"], CAM_POS, c["cam_quat"], w, h, FOVY, NEAR, FAR, c["gp"], c["gq"])
    dc.check_mask(mask)
    assert np.all(want[0] == NEAR) and np.all(want[1] < FAR)
    got, warn = _device_depth(cassie, c, w, h)
    dc.compare(got, want, mask, "stairs, device")
    assert not warn.any()


def test_the_device_equals_the_emulator(hfield_result):
    """Case 1 of tests/test_depth.py: within the bound, not bit for bit (the device contracts FMAs where the emulator's build does not)."""
    from test_depth import H, W
    r = hfield_result
    c = r["c"]
    got, warn = _device_depth(Model("cassie_hfield"), c, W, H, c["bank"], c["index"])
    dc.compare(got, r["got"], r["mask"], "device against emulator")
    assert not warn.any()


def test_images_follow_the_state_with_nothing_synchronised(cassie):
    """step_range + end_episodes + depth_image queued on one stream, three policy steps, no synchronisation in between: the image is
    that of the state the launches in front of it left -- of a restarted env, that of its start state."""
    import torch
    pod, n, k, w, h = cassie.pod, 256, 8, 16, 12
    rng = np.random.default_rng(23)
    bq, bv = bank_states(cassie, k)
    bq[:, 0:2] = rng.uniform(-1, 1, (k, 2))
    bq[:, 2] += rng.uniform(0.0, 0.3, k)
    yaw = rng.uniform(-np.pi, np.pi, k)
    bq[:, 3:7] = np.stack([np.cos(yaw / 2), np.zeros(k), np.zeros(k), np.sin(yaw / 2)], axis=-1)
    forced = np.unique(rng.integers(0, n, 40))
    force = np.zeros(n, dtype=np.int32)
    force[forced] = 1
    pick = rng.integers(0, k, n).astype(np.int32)
    cam_quat = dc.pitched_down(45.0)
    tg = bench.pd_targets(np.arange(n), 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.enable_episodes()
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.configure_depth(pod.root_body[0], CAM_POS, cam_quat, w, h, FOVY, NEAR, FAR)
        tg_d = torch.from_numpy(tg).cuda()
        ptarget = torch.zeros((n, 10), dtype=torch.float64, device="cuda")
        b.bind(P.F_PD_PTARGET, ptarget.data_ptr())
        none_d, force_d, pick_d = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.from_numpy(force).cuda(), torch.from_numpy(pick).cuda()
        b.sync()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for p in range(3):
                ptarget.copy_(tg_d[p])
                b.step_range(0, n, 50, st.cuda_stream)
                b.end_episodes(0, n, True, pick_ptr=pick_d.data_ptr(), force_ptr=(force_d if p == 2 else none_d).data_ptr(), stream=st.cuda_stream)
                b.depth_image(0, n, stream=st.cuda_stream)
        torch.cuda.synchronize()
        qpos, got = b.get(P.F_QPOS), b.get(P.F_DEPTH)
        done = b.episodes()[0]
        assert np.array_equal(np.nonzero(done)[0], forced)
        assert qpos[forced].tobytes() == bq[pick[forced]].tobytes()
        others = np.setdiff1d(np.arange(n), forced)
        assert np.abs(qpos[others] - cassie.qpos_init()).max() > 1e-3          # the others have moved on
        want, mask = dc.depth(pod, qpos, CAM_POS, cam_quat, w, h, FOVY, NEAR, FAR)
        dc.check_mask(mask)
        dc.compare(got, want, mask, "behind step + end_episodes")
        start, _ = dc.depth(pod, bq[pick[forced]], CAM_POS, cam_quat, w, h, FOVY, NEAR, FAR)
        assert np.max(np.abs(got[forced] - start)[~mask[forced]]) <= dc.TOL
        assert len({got[e].tobytes() for e in forced}) > 4
    finally:
        b.close()


def test_python_layer_refuses(built):
    import torch
    hf = Model("cassie_hfield")
    pelvis = hf.pod.root_body[0]
    q = dc.pitched_down(45.0)
    b = Batch(hf, 8)
    try:
        buf = torch.zeros((8, 64), dtype=torch.float64, device="cuda")
        with pytest.raises(RuntimeError):
            b.depth_image()                                            # not configured
        with pytest.raises(RuntimeError):
            b.bind(P.F_DEPTH, buf.data_ptr())                          # a bind before configure
        with pytest.raises(RuntimeError):
            b.get(P.F_DEPTH)
        with pytest.raises(ValueError):
            b.configure_depth(pelvis, CAM_POS, q, 129, 128, FOVY, NEAR, FAR)         # W H > 16384
        with pytest.raises(ValueError):
            b.configure_depth(pelvis + 1, CAM_POS, q, 8, 8, FOVY, NEAR, FAR)         # not a child of the world
        with pytest.raises(ValueError):
            b.configure_depth(pelvis, CAM_POS, q, 8, 8, FOVY, 2.0, 2.0)              # near >= far
        with pytest.raises(ValueError):
            b.configure_depth(pelvis, CAM_POS, q, 8, 8, FOVY, 3.0, 2.0)
        with pytest.raises(ValueError):
            b.configure_depth(pelvis, CAM_POS, q, 0, 8, FOVY, NEAR, FAR)
        assert b.dim(P.F_DEPTH) == 0
        b.configure_depth(pelvis, CAM_POS, q, 128, 128, FOVY, NEAR, FAR)             # the largest image
        assert b.dim(P.F_DEPTH) == 16384
        b.configure_depth(pelvis, CAM_POS, q, 8, 8, FOVY, NEAR, FAR)                 # reconfiguring is allowed
        assert b.dim(P.F_DEPTH) == 64
        b.bind(P.F_DEPTH, buf.data_ptr())
        b.depth_image()
        b.sync()
        assert np.all(b.get(P.F_DEPTH) == FAR)                                      # (no height-field samples: nothing to see)
        with pytest.raises(RuntimeError):
            b.depth_image(4, 5)                                                     # outside the batch
    finally:
        b.close()
