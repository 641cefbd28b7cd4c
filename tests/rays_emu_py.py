"""ctypes access to the ray kernel on the CPU wave emulator (tests/emu/emu_rays.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_rays.cpp adds."""
import ctypes

import numpy as np

import emu_py
import rays_check as rc
from cassie_amd._lib import CmModel

_vp, _ci, _cd, _ul, _cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulong, ctypes.c_uint
_declared = False


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        L.emu_rays_check.argtypes, L.emu_rays_check.restype = [ctypes.POINTER(CmModel), _vp, _ci, _cd, _cd, _ci, _cu, _vp, _vp], ctypes.c_char_p
        L.emu_rays_grid.argtypes = [_ci, _ci]
        L.emu_sizeof_ray.restype = _ul
        L.emu_rays_record.argtypes, L.emu_rays_record.restype = [ctypes.POINTER(CmModel), _ci, _cd, _cd, _cu, _ci, _ci, _ci, _ci, _ci, _ci, _vp, _vp], None
        L.emu_rays_cast.argtypes = [ctypes.POINTER(CmModel), _vp, _ci, _ci, _ci, _vp, _ci, _cd, _cd, _ci, _cu, _vp, _vp, _vp, _ci, _vp, _ul, _vp, _ci,
                                    _vp, _vp, _vp]
        L.emu_rays_last_refusal.restype = ctypes.c_char_p
        assert L.emu_sizeof_ray() == rc.RAY_DTYPE.itemsize
        _declared = True
    return L


def grid(n, nrays):
    """ck::rays_grid."""
    return lib().emu_rays_grid(n, nrays)


def check(pod, table, rmin, rmax, mask=None):
    """ck::rays_configure (and ck::check_ray_geoms for a mask) -> (the refusal's message or None, the normalised table, the mask in force)."""
    table = np.ascontiguousarray(table, dtype=rc.RAY_DTYPE)
    out = np.zeros(max(table.size, 1), dtype=rc.RAY_DTYPE)
    m = _cu(0)
    why = lib().emu_rays_check(ctypes.byref(pod), table.ctypes.data if table.size else None, table.size, rmin, rmax, int(mask is not None), int(mask or 0),
                               out.ctypes.data, ctypes.byref(m))
    return (None if why is None else why.decode()), out[: table.size], m.value


def record(pod, nrays, rmin, rmax, mask, sout, env0, n, ids=False, normals=False, nterrain=0):
    """What ck::make_rays_io makes of a configuration and an env range -> (dict of the record's integer fields, (rmin, rmax))."""
    ints, reals = np.zeros(11, dtype=np.int64), np.zeros(2)
    lib().emu_rays_record(ctypes.byref(pod), nrays, rmin, rmax, mask, sout, env0, n, int(ids), int(normals), nterrain, ints.ctypes.data, reals.ctypes.data)
    names = ("env0", "n", "nrays", "sout", "sxp", "sxq", "geoms", "ids", "normals", "index", "nterrain")
    return dict(zip(names, (int(v) for v in ints))), tuple(reals)


def cast(pod, table, rmin, rmax, xpos, xquat, mask=None, want_ids=True, want_normals=True, blocks=None, hfield=None, stride=0, index=None, nterrain=0,
         env0=0, n=None, grid=0, out=None, ids=None, normals=None, warn=None):
    """The emulated kernel -> (ranges [nenv][nrays], ids [nenv][nrays] int32 or None, normals [nenv][nrays][3] or None, warn [nenv]).
    table: RAY_DTYPE entries as phys_batch_rays_configure takes them; mask None: the default geoms; xpos / xquat: [nenv][nbody * 3 / 4]."""
    _ptr = emu_py._ptr
    table = np.ascontiguousarray(table, dtype=rc.RAY_DTYPE)
    xpos, xquat = np.ascontiguousarray(xpos, dtype=np.float64), np.ascontiguousarray(xquat, dtype=np.float64)
    nenv, N = xpos.shape[0], table.size
    xpos, xquat = xpos.reshape(nenv, -1), xquat.reshape(nenv, -1)
    assert xpos.shape[1] == 3 * pod.nbody and xquat.shape[1] == 4 * pod.nbody
    n = nenv - env0 if n is None else n
    out = np.full((nenv, N), np.nan) if out is None else out
    if ids is None and want_ids:
        ids = np.full((nenv, N), -9, dtype=np.int32)
    if normals is None and want_normals:
        normals = np.full((nenv, N, 3), np.nan)
    warn = np.zeros(nenv, dtype=np.int32) if warn is None else warn
    model = CmModel.from_buffer_copy(pod)
    model.env_geom = 1 if blocks is not None else 0
    index = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc_ = lib().emu_rays_cast(ctypes.byref(model), _ptr(blocks), env0, n, grid, table.ctypes.data, N, rmin, rmax, int(mask is not None), int(mask or 0),
                              _ptr(xpos), _ptr(xquat), _ptr(out), out.shape[1], _ptr(hfield), stride, _ptr(index), nterrain, _ptr(warn), _ptr(ids),
                              _ptr(normals))
    assert rc_ == 0, (lib().emu_rays_last_refusal() or b"").decode()
    return out, ids, normals, warn
