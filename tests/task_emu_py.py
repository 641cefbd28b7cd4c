"""ctypes access to the task kernel on the CPU wave emulator (tests/emu/emu_task.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_task.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P
from obs_emu_py import NFIELDS, ObsField

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_declared = False
TASK_GRID = MAXDST = None    # ck::TASK_GRID, ck::ACT_MAXDST, once the library is loaded (lib())
COL_DTYPE = np.dtype([(k, np.int32) for k in ("kind", "form", "group", "rate_col", "phase_col", "src", "tcol", "dslot", "delem")] +
                     [(k, np.uint32) for k in ("period_lo", "span", "hold")] + [("thr", np.uint64)] +
                     [(k, np.float64) for k in ("center", "half", "rest", "rate", "rate_scale", "phase0", "shift", "duty", "ramp", "offset", "scale")])
CMD_FIELDS = np.array(P.ACT_CMD_FIELDS, dtype=np.int32)


class TaskArgs(ctypes.Structure):
    _fields_ = [("fields", ctypes.POINTER(ObsField)), ("nfields", _ci), ("nenv", _ci),
                ("cmd_fields", _vp), ("ncmd", _ci),
                ("cols", _vp), ("ncols", _ci), ("dtype", _ci), ("seed", ctypes.c_ulonglong), ("env_base", ctypes.c_uint),
                ("table", _vp), ("nframes", _ci), ("tcols", _ci),
                ("rows", _vp), ("srow", _ll), ("state", _vp), ("words", _vp), ("counts", _vp)]


def lib():
    global _declared, TASK_GRID, MAXDST
    L = emu_py.lib()
    if not _declared:
        L.emu_task_last_refusal.restype = ctypes.c_char_p
        L.emu_task_constants.argtypes, L.emu_task_constants.restype = [_vp], None
        L.emu_task_grid.argtypes = [_ci]
        L.emu_task_check.argtypes, L.emu_task_check.restype = [ctypes.POINTER(TaskArgs), _vp], ctypes.c_char_p
        L.emu_task_columns.argtypes = [ctypes.POINTER(TaskArgs), _vp]
        L.emu_task_table_check.argtypes, L.emu_task_table_check.restype = [ctypes.POINTER(TaskArgs), _vp, _ci, _ci], ctypes.c_char_p
        L.emu_task_call_check.argtypes, L.emu_task_call_check.restype = [ctypes.POINTER(TaskArgs), _ci, _vp, _ci, _ci], ctypes.c_char_p
        L.emu_task_record.argtypes = [ctypes.POINTER(TaskArgs), _ci, _ci, _vp, _vp]
        L.emu_task.argtypes = [ctypes.POINTER(TaskArgs), _ci, _ci, _vp, _ci]
        L.emu_task_sincos.argtypes, L.emu_task_sincos.restype = [_vp, _ci, _vp, _vp, _vp], None
        c = np.zeros(8, dtype=np.int64)
        L.emu_task_constants(c.ctypes.data)
        assert (int(c[1]), int(c[2]), int(c[3]), int(c[4])) == (P.TASK_MAXCOLS, P.TASK_MAXFRAMES, P.TASK_MAXTCOLS, 3)
        assert (int(c[5]), int(c[6]), int(c[7])) == (P.TASK_COL_DTYPE.itemsize, COL_DTYPE.itemsize, ctypes.sizeof(TaskArgs))
        TASK_GRID, MAXDST = int(c[0]), len(P.ACT_CMD_FIELDS)
        _declared = True
    return L


def grid(n):
    """ck::task_grid."""
    return lib().emu_task_grid(n)


def sincos(theta):
    """ck::task_sincos2pi and ck::task_wrap of every theta -> (sin2pi, cos2pi, wrap)."""
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    sn, cs, wr = np.empty_like(theta), np.empty_like(theta), np.empty_like(theta)
    lib().emu_task_sincos(theta.ctypes.data, theta.size, sn.ctypes.data, cs.ctypes.data, wr.ctypes.data)
    return sn, cs, wr


def _dtype_code(dtype):
    return dtype if isinstance(dtype, int) else P._obs_dtype(dtype)


class Call:
    """What the batch holds and how the task rows are configured, as the arguments of the emulator's entry points.  fields: {field id:
    float64 array [nenv][>= dim]} -- a 2-D view with a row stride stands for a strided binding, and the destination fields are written in
    place; dims: {field id: row length} where it is not the array's width.  table: float64 [nframes][tcols] or None.  rows: [nenv][>=
    ncols] of the dtype, state: float64 [nenv][ncols], words: uint32 [nenv][3][ncols], counts: uint32 [nenv]; all the caller's, written
    in place."""

    def __init__(self, fields, nenv, cols, dtype=np.float32, seed=0, env_base=0, table=None, rows=None, state=None, words=None, counts=None, dims=None,
                 ncols=None, cmd_fields=CMD_FIELDS, table_shape=None):
        self.keep = [fields, table, rows, state, words, counts, cmd_fields]
        self.table = P.task_cols(cols)
        self.farr = (ObsField * NFIELDS)()
        for f, a in fields.items():
            assert a.dtype == np.float64 and a.ndim == 2 and a.strides[1] == 8 and a.strides[0] % 8 == 0
            self.farr[f] = ObsField(a.ctypes.data, (dims or {}).get(f, a.shape[1]), a.strides[0] // 8)
        self.a = TaskArgs(fields=self.farr, nfields=NFIELDS, nenv=nenv, cmd_fields=cmd_fields.ctypes.data, ncmd=len(cmd_fields),
                          cols=self.table.ctypes.data if self.table.size else None, ncols=self.table.size if ncols is None else ncols,
                          dtype=_dtype_code(dtype), seed=seed, env_base=env_base)
        if table is not None:
            assert table.dtype == np.float64 and table.flags.c_contiguous and table.ndim == 2
            self.a.table = table.ctypes.data
            self.a.nframes, self.a.tcols = table.shape if table_shape is None else table_shape
        if rows is not None:
            assert rows.ndim == 2 and rows.strides[1] == rows.itemsize
            self.a.rows, self.a.srow = rows.ctypes.data, rows.strides[0] // rows.itemsize
        if state is not None:
            assert state.dtype == np.float64 and state.flags.c_contiguous
            self.a.state = state.ctypes.data
        if words is not None:
            assert words.dtype == np.uint32 and words.flags.c_contiguous
            self.a.words = words.ctypes.data
        if counts is not None:
            assert counts.dtype == np.uint32
            self.a.counts = counts.ctypes.data

    def check(self):
        """check_task_table, task_configure and the bind check -> (refusal or None, the record's numbers)."""
        ints = np.zeros(4 + 2 * 9, dtype=np.int64)
        why = lib().emu_task_check(ctypes.byref(self.a), ints.ctypes.data)
        if why is not None:
            return why.decode(), None
        rec = dict(zip(("ncols", "dtype", "ndst", "tcol_need"), (int(v) for v in ints[:4])))
        rec["dst_field"], rec["dst_dim"] = [int(v) for v in ints[4:4 + rec["ndst"]]], [int(v) for v in ints[13:13 + rec["ndst"]]]
        return None, rec

    def columns(self):
        """The column table [ncols] (COL_DTYPE)."""
        cols = np.zeros(P.TASK_MAXCOLS, dtype=COL_DTYPE)
        n = lib().emu_task_columns(ctypes.byref(self.a), cols.ctypes.data)
        assert n >= 0, (lib().emu_task_last_refusal() or b"").decode()
        return cols[:n]

    def table_check(self, table, shape=None):
        """A later set_table against this configuration -> refusal or None."""
        nframes, tcols = table.shape if shape is None else shape
        why = lib().emu_task_table_check(ctypes.byref(self.a), table.ctypes.data, nframes, tcols)
        return None if why is None else why.decode()

    def call_check(self, env0, n, configured=True, now=None):
        """ck::check_task_call -> refusal or None.  now: {field id: (array or None, dim)} that differ at the call from the configure call."""
        arr = None
        if now is not None:
            arr = (ObsField * NFIELDS)(*self.farr)
            for f, (a, dim) in now.items():
                arr[f] = ObsField(None if a is None else a.ctypes.data, dim, 0 if a is None else a.strides[0] // 8)
        why = lib().emu_task_call_check(ctypes.byref(self.a), int(configured), arr, env0, n)
        return None if why is None else why.decode()

    def record(self, env0, n, reset=None):
        """What ck::make_task_io makes of the configuration and an env range -> (dict of the record's numbers, [(base, stride)] per
        destination slot)."""
        out = np.zeros(18 + 2 * 9, dtype=np.uint64)
        rc = lib().emu_task_record(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), out.ctypes.data)
        assert rc == 0, (lib().emu_task_last_refusal() or b"").decode()
        names = ("env0", "n", "ncols", "f32", "nframes", "tcols", "env_base", "key0", "key1", "cols", "table", "rows", "srow", "state", "words", "counts",
                 "reset", "ndst")
        rec = dict(zip(names, (int(v) for v in out[:18])))
        dst = [tuple(int(v) for v in out[18 + 2 * s: 20 + 2 * s]) for s in range(rec["ndst"])]
        return rec, dst

    def task(self, env0=0, n=None, reset=None, grid=0):
        """phys_batch_task on the emulator: the rows, the state, the words, the counts and the destination elements of the range, in place."""
        n = self.a.nenv - env0 if n is None else n
        reset = None if reset is None else np.ascontiguousarray(reset, dtype=np.int32)
        rc = lib().emu_task(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), grid)
        assert rc == 0, (lib().emu_task_last_refusal() or b"").decode()
