"""The launcher's refusals on the MI355X are the shared checks' (csrc/small_launch.h): for every refused scan / depth / mask
configuration of tests/test_small_launch.py the batch's last error ends with the very message the emulator's probe of the same
function returns, nothing is configured and no depth kernel has been launched by then, and the batch goes on to an accepted scan and
an accepted 9 x 7 depth image that agree with the emulator's."""
import numpy as np
import pytest

import depth_check as dc
import depth_emu_py
import emu_py
import terrain_check as tc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd._lib import lib
from test_small_launch import FAR, FOVY, NEAR, emu_message, refusals

pytestmark = pytest.mark.gpu


def _device_refuses(b, kind, args):
    """The C entry point itself (the Python layer has checks of its own in front of it) -> the last error, None where it accepted."""
    L = lib()
    if kind == "scan":
        npoints, body, scan_range = args
        off = np.zeros((max(npoints, 1), 2))
        rc, entry = L.phys_batch_scan_configure(b._h, off.ctypes.data, npoints, body, scan_range), "phys_batch_scan_configure: "
    elif kind == "depth":
        body, width, height, fovy, near, far, quat = args
        pos, quat = np.zeros(3), np.ascontiguousarray(quat, dtype=np.float64)
        rc = L.phys_batch_depth_configure(b._h, body, pos.ctypes.data, quat.ctypes.data, width, height, fovy, near, far)
        entry = "phys_batch_depth_configure: "
    else:
        rc, entry = L.phys_batch_depth_set_geoms(b._h, args[0]), "phys_batch_depth_set_geoms: "
    if rc == 0:
        return None
    assert rc == -1
    text = L.phys_last_error().decode()
    assert text.startswith(entry), text
    return text


def test_the_launcher_refuses_with_the_shared_messages_and_stays_usable(built):
    hf = Model("cassie_hfield")
    pod, n = hf.pod, 2
    pelvis = pod.root_body[0]
    table = refusals(pod)
    b = Batch(hf, n)
    try:
        for what, kind, args, _ in table:
            if kind == "mask":
                continue                      # (a mask is looked at once an image is configured: below)
            message = emu_message(pod, kind, args)
            assert message is not None, what
            assert _device_refuses(b, kind, args).endswith(": " + message), what
        # nothing was configured and nothing launched
        assert b.dim(P.F_HEIGHT_SCAN) == 0 and b.dim(P.F_DEPTH) == 0 and b.depth_launches() == (0, 0)
        with pytest.raises(RuntimeError, match="phys_batch_scan_configure first"):
            b.height_scan()
        with pytest.raises(RuntimeError, match="phys_batch_depth_configure first"):
            b.depth_image()
        # an accepted scan and an accepted 9 x 7 image on the same batch: a flat height field at 0.4 of its full elevation, the robot
        # turned and raised a little, the camera pitched down far enough for every ray to land well inside the grid
        grid = np.full(pod.hfield_nrow * pod.hfield_ncol, 0.4, dtype=np.float32)
        qpos = np.tile(hf.qpos_init(), (n, 1))
        qpos[1, 0:3] += (0.3, -0.2, 0.25)
        qpos[1, 3:7] = (np.cos(0.35), 0.0, 0.0, np.sin(0.35))
        offsets, cam_pos, cam_quat = tc.grid_pattern(3, 3, 0.1), np.array([0.1, 0.0, 0.1]), dc.pitched_down(70.0)
        b.set_hfield(grid)
        b.set(P.F_QPOS, qpos)
        b.configure_scan(offsets, pelvis, 1.5)
        b.configure_depth(pelvis, cam_pos, cam_quat, 9, 7, np.degrees(FOVY), NEAR, FAR)
        for what, kind, args, _ in table:
            if kind == "mask":
                assert _device_refuses(b, kind, args).endswith(": " + emu_message(pod, kind, args)), what
        b.height_scan()
        b.depth_image()
        b.sync()
        assert b.depth_launches() == (1, 0)                   # (the refused mask left the default in force: the static kernel)
        assert not b.warnings()[0].any()
        scan, _ = emu_py.height_scan(pod, qpos, offsets, pelvis, 1.5, hfield=grid)
        image, _ = depth_emu_py.depth_image(pod, qpos, pelvis, cam_pos, cam_quat, 9, 7, np.degrees(FOVY), NEAR, FAR, hfield=grid)
        # (the surface is one plane: no pixel and no scan point sits at a discontinuity, so the bounds of tests/test_terrain_gpu.py and
        # tests/test_depth_gpu.py -- the device contracts FMAs where the emulator's build does not -- hold everywhere)
        assert np.all(np.abs(scan) < 1.5) and np.max(np.abs(b.get(P.F_HEIGHT_SCAN) - scan)) <= 1e-12
        assert np.all(image < FAR) and np.all(image > NEAR) and np.max(np.abs(b.get(P.F_DEPTH) - image)) <= dc.TOL
    finally:
        b.close()
