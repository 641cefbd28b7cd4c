"""ctypes access to the depth-image kernel on the CPU wave emulator (tests/emu/emu_depth.cpp) -- test infrastructure only.  The library
is the one tests/emu_py.py loads; this module declares the one entry point it adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd._lib import CmModel

_vp, _ci, _cd, _ul = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulong
_declared = False


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        L.emu_depth_image.argtypes = [ctypes.POINTER(CmModel), _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _cd, _cd, _cd, _vp, _ci,
                                      _vp, _ci, _vp, _ul, _vp, _ci, _vp]
        _declared = True
    return L


def depth_image(pod, qpos, body, cam_pos, cam_quat, width, height, fovy_deg, near, far, pose=None, blocks=None, hfield=None, stride=0,
                index=None, nterrain=0, env0=0, n=None, grid=0, out=None, warn=None):
    """The emulated depth kernel -> (images [nenv][height * width], warn [nenv]).  hfield: float32, one grid / nenv grids / a bank;
    blocks: per-env parameter blocks whose geometry the kernel reads (the model is then told to, like a batch that has randomised
    geometry); pose: [nenv][7] per-env extrinsics."""
    _ptr = emu_py._ptr
    nenv = qpos.shape[0]
    n = nenv - env0 if n is None else n
    qpos = np.ascontiguousarray(qpos, dtype=np.float64)
    cam_pos, cam_quat = np.ascontiguousarray(cam_pos, dtype=np.float64), np.ascontiguousarray(cam_quat, dtype=np.float64)
    pose = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64)
    out = np.full((nenv, width * height), np.nan) if out is None else out
    warn = np.zeros(nenv, dtype=np.int32) if warn is None else warn
    model = CmModel.from_buffer_copy(pod)
    model.env_geom = 1 if blocks is not None else 0
    index = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc = lib().emu_depth_image(ctypes.byref(model), _ptr(blocks), env0, n, grid, body, _ptr(cam_pos), _ptr(cam_quat), _ptr(pose), width, height,
                               float(np.radians(fovy_deg)), near, far, _ptr(qpos), qpos.shape[1], _ptr(out), out.shape[1], _ptr(hfield), stride,
                               _ptr(index), nterrain, _ptr(warn))
    assert rc == 0
    return out, warn
