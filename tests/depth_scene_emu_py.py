"""ctypes access to the scene depth kernel on the CPU wave emulator (tests/emu/emu_depth_scene.cpp) -- test infrastructure only.  The
library is the one tests/emu_py.py loads; this module declares the one entry point it adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd._lib import CmModel

_vp, _ci, _cd, _ul, _cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulong, ctypes.c_uint
_declared = False


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        L.emu_depth_scene_image.argtypes = [ctypes.POINTER(CmModel), _vp, _ci, _ci, _ci, _ci, _vp, _vp, _vp, _ci, _ci, _cd, _cd, _cd, _vp, _ci,
                                            _vp, _ci, _vp, _ul, _vp, _ci, _vp, _cu, _vp, _vp, _vp]
        _declared = True
    return L


def depth_image(pod, qpos, body, cam_pos, cam_quat, width, height, fovy_deg, near, far, mask, xpos=None, xquat=None, want_ids=True, pose=None,
                blocks=None, hfield=None, stride=0, index=None, nterrain=0, env0=0, n=None, grid=0, out=None, ids=None, warn=None):
    """The emulated scene kernel -> (images [nenv][height * width], ids [nenv][height * width] int32 or None, warn [nenv]).  mask: bit g =
    compiled geom g; xpos / xquat: [nenv][nbody * 3 / 4] body poses (None: moving geoms are unseen); the rest as
    depth_emu_py.depth_image."""
    _ptr = emu_py._ptr
    nenv = qpos.shape[0]
    n = nenv - env0 if n is None else n
    qpos = np.ascontiguousarray(qpos, dtype=np.float64)
    cam_pos, cam_quat = np.ascontiguousarray(cam_pos, dtype=np.float64), np.ascontiguousarray(cam_quat, dtype=np.float64)
    pose = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64)
    xpos = None if xpos is None else np.ascontiguousarray(xpos, dtype=np.float64).reshape(nenv, -1)
    xquat = None if xquat is None else np.ascontiguousarray(xquat, dtype=np.float64).reshape(nenv, -1)
    assert xpos is None or (xpos.shape[1] == 3 * pod.nbody and xquat.shape[1] == 4 * pod.nbody)
    out = np.full((nenv, width * height), np.nan) if out is None else out
    if ids is None and want_ids:
        ids = np.full((nenv, width * height), -9, dtype=np.int32)
    assert ids is None or (ids.dtype == np.int32 and ids.flags.c_contiguous and ids.shape == (nenv, width * height))
    warn = np.zeros(nenv, dtype=np.int32) if warn is None else warn
    model = CmModel.from_buffer_copy(pod)
    model.env_geom = 1 if blocks is not None else 0
    index = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc = lib().emu_depth_scene_image(ctypes.byref(model), _ptr(blocks), env0, n, grid, body, _ptr(cam_pos), _ptr(cam_quat), _ptr(pose), width,
                                     height, float(np.radians(fovy_deg)), near, far, _ptr(qpos), qpos.shape[1], _ptr(out), out.shape[1],
                                     _ptr(hfield), stride, _ptr(index), nterrain, _ptr(warn), int(mask), _ptr(xpos), _ptr(xquat), _ptr(ids))
    assert rc == 0
    return out, ids, warn
