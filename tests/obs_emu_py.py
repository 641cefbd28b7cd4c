"""ctypes access to the observation kernel on the CPU wave emulator (tests/emu/emu_obs.cpp) -- test infrastructure only.  The library
is the one tests/emu_py.py loads; this module declares the entry points emu_obs.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P

_vp, _ci = ctypes.c_void_p, ctypes.c_int
_declared = False
OBS_GRID = MAXSLOTS = None    # ck::OBS_GRID, ck::OBS_MAXSLOTS, once the library is loaded (lib())
NFIELDS = P.F_PROBES + 1      # PHYS_F_COUNT
COL_DTYPE = np.dtype([("slot", np.int32), ("elem", np.int32), ("comp", np.int32), ("qslot", np.int32), ("qelem", np.int32), ("pad", np.int32),
                      ("vec", np.float64, 3), ("offset", np.float64), ("scale", np.float64), ("noise", np.float64), ("lo", np.float64), ("hi", np.float64)])


class ObsField(ctypes.Structure):
    _fields_ = [("base", _vp), ("dim", _ci), ("stride", _ci)]


class ObsArgs(ctypes.Structure):
    _fields_ = [("fields", ctypes.POINTER(ObsField)), ("nfields", _ci), ("depth_field", _ci), ("nenv", _ci),
                ("terms", _vp), ("nterms", _ci), ("history", _ci), ("dtype", _ci), ("seed", ctypes.c_ulonglong), ("env_base", ctypes.c_uint),
                ("input", _vp), ("input_dim", _ci), ("input_stride", ctypes.c_longlong), ("input_dtype", _ci),
                ("rows", _vp), ("srow", ctypes.c_longlong), ("frames", _vp)]


def lib():
    global _declared, OBS_GRID, MAXSLOTS
    L = emu_py.lib()
    if not _declared:
        L.emu_obs_last_refusal.restype = ctypes.c_char_p
        L.emu_obs_constants.argtypes, L.emu_obs_constants.restype = [_vp], None
        L.emu_obs_grid.argtypes = [_ci]
        L.emu_obs_philox.argtypes, L.emu_obs_philox.restype = [_vp, _vp, _vp], None
        L.emu_obs_uniform.argtypes, L.emu_obs_uniform.restype = [ctypes.c_uint], ctypes.c_double
        L.emu_obs_check.argtypes, L.emu_obs_check.restype = [ctypes.POINTER(ObsArgs), _vp, _vp], ctypes.c_char_p
        L.emu_obs_columns.argtypes = [ctypes.POINTER(ObsArgs), _vp]
        L.emu_obs_call_check.argtypes, L.emu_obs_call_check.restype = [ctypes.POINTER(ObsArgs), _ci, _vp, _ci, _ci], ctypes.c_char_p
        L.emu_obs_record.argtypes = [ctypes.POINTER(ObsArgs), _ci, _ci, _vp, _vp]
        L.emu_obs.argtypes = [ctypes.POINTER(ObsArgs), _ci, _ci, _vp, _ci]
        c = np.zeros(8, dtype=np.int64)
        L.emu_obs_constants(c.ctypes.data)
        assert (int(c[1]), int(c[2]), int(c[3])) == (P.OBS_MAXCOLS, P.OBS_MAXHISTORY, P.OBS_MAXROW)
        assert (int(c[5]), int(c[6]), int(c[7])) == (P.OBS_TERM_DTYPE.itemsize, COL_DTYPE.itemsize, ctypes.sizeof(ObsArgs))
        OBS_GRID, MAXSLOTS = int(c[0]), int(c[4])
        _declared = True
    return L


def philox(counter, key):
    """The kernel's own ck::philox4x32_10 -> the four words."""
    c, k, out = np.asarray(counter, dtype=np.uint32), np.asarray(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    lib().emu_obs_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return tuple(int(w) for w in out)


def uniform(w):
    """The kernel's own ck::obs_uniform."""
    return lib().emu_obs_uniform(int(w))


def grid(n):
    """ck::obs_grid."""
    return lib().emu_obs_grid(n)


def _dtype_code(dtype):
    return dtype if isinstance(dtype, int) else P._obs_dtype(dtype)


class Call:
    """What the batch holds and how the observation is configured, as the arguments of the emulator's entry points.  fields: {field id:
    float64 array [nenv][>= dim]} -- a 2-D view with a row stride stands for a strided binding; dims: {field id: row length} where it is
    not the array's width.  inp: the bound input array [nenv][>= input_dim] (float32 / float64) or None.  rows: [nenv][>= history *
    ncols] of the dtype, frames: uint32 [nenv]; both the caller's, written in place."""

    def __init__(self, fields, nenv, terms, history=1, dtype=np.float32, seed=0, env_base=0, inp=None, input_dim=None, rows=None, frames=None, dims=None,
                 nterms=None):
        self.keep = [fields, inp, rows, frames]
        self.table = P.obs_terms(terms)
        self.farr = (ObsField * NFIELDS)()
        for f, a in fields.items():
            assert a.dtype == np.float64 and a.ndim == 2 and a.strides[1] == 8 and a.strides[0] % 8 == 0
            self.farr[f] = ObsField(a.ctypes.data, (dims or {}).get(f, a.shape[1]), a.strides[0] // 8)
        self.a = ObsArgs(fields=self.farr, nfields=NFIELDS, depth_field=P.F_DEPTH, nenv=nenv, terms=self.table.ctypes.data if self.table.size else None,
                         nterms=self.table.size if nterms is None else nterms, history=history, dtype=_dtype_code(dtype), seed=seed, env_base=env_base)
        if inp is not None:
            self.bind_input(inp, input_dim)
        if rows is not None:
            assert rows.ndim == 2 and rows.strides[1] == rows.itemsize
            self.a.rows, self.a.srow = rows.ctypes.data, rows.strides[0] // rows.itemsize
        if frames is not None:
            assert frames.dtype == np.uint32
            self.a.frames = frames.ctypes.data

    def bind_input(self, inp, input_dim=None, dtype=None, stride=None):
        self.keep.append(inp)
        self.a.input, self.a.input_dim = inp.ctypes.data, inp.shape[1] if input_dim is None else input_dim
        self.a.input_stride = inp.strides[0] // inp.itemsize if stride is None else stride
        self.a.input_dtype = _dtype_code(inp.dtype if dtype is None else dtype)

    def check(self):
        """obs_configure and the bind checks -> (refusal or None, the record's numbers, every term's first column)."""
        ints, first = np.zeros(6 + 2 * 16, dtype=np.int64), np.zeros(max(self.table.size, 1), dtype=np.int32)
        why = lib().emu_obs_check(ctypes.byref(self.a), ints.ctypes.data, first.ctypes.data)
        if why is not None:
            return why.decode(), None, None
        names = ("nterms", "ncols", "history", "dtype", "nslots", "input_need")
        rec = dict(zip(names, (int(v) for v in ints[:6])))
        rec["slot_field"], rec["slot_dim"] = [int(v) for v in ints[6:6 + rec["nslots"]]], [int(v) for v in ints[22:22 + rec["nslots"]]]
        return None, rec, [int(v) for v in first[: self.table.size]]

    def columns(self):
        """The column table [ncols] (COL_DTYPE)."""
        cols = np.zeros(P.OBS_MAXCOLS, dtype=COL_DTYPE)
        n = lib().emu_obs_columns(ctypes.byref(self.a), cols.ctypes.data)
        assert n >= 0, (lib().emu_obs_last_refusal() or b"").decode()
        return cols[:n]

    def call_check(self, env0, n, configured=True, now=None):
        """ck::check_obs_call -> refusal or None.  now: {field id: (array or None, dim)} that differ at the call from the configure call."""
        arr = None
        if now is not None:
            arr = (ObsField * NFIELDS)(*self.farr)
            for f, (a, dim) in now.items():
                arr[f] = ObsField(None if a is None else a.ctypes.data, dim, 0 if a is None else a.strides[0] // 8)
        why = lib().emu_obs_call_check(ctypes.byref(self.a), int(configured), arr, env0, n)
        return None if why is None else why.decode()

    def record(self, env0, n, refill=None):
        """What ck::make_obs_io makes of the configuration and an env range -> (dict of the record's numbers, [(base, stride, f32)] per slot)."""
        out = np.zeros(13 + 3 * 16, dtype=np.uint64)
        nslots = lib().emu_obs_record(ctypes.byref(self.a), env0, n, emu_py._ptr(refill), out.ctypes.data)
        assert nslots >= 0, (lib().emu_obs_last_refusal() or b"").decode()
        names = ("env0", "n", "ncols", "history", "f32", "env_base", "key0", "key1", "cols", "rows", "srow", "frames", "refill")
        return dict(zip(names, (int(v) for v in out[:13]))), [tuple(int(v) for v in out[13 + 3 * s: 16 + 3 * s]) for s in range(nslots)]

    def observe(self, env0=0, n=None, refill=None, grid=0):
        """phys_batch_obs on the emulator: the rows and the frame counts of the range, in place."""
        n = self.a.nenv - env0 if n is None else n
        refill = None if refill is None else np.ascontiguousarray(refill, dtype=np.int32)
        rc = lib().emu_obs(ctypes.byref(self.a), env0, n, emu_py._ptr(refill), grid)
        assert rc == 0, (lib().emu_obs_last_refusal() or b"").decode()
