"""ctypes access to the action kernel on the CPU wave emulator (tests/emu/emu_actions.cpp) -- test infrastructure only.  The library
is the one tests/emu_py.py loads; this module declares the entry points emu_actions.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P
from obs_emu_py import NFIELDS, ObsField

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_declared = False
ACT_GRID = MAXSLOTS = MAXDST = None    # ck::ACT_GRID, ck::ACT_MAXSLOTS, ck::ACT_MAXDST, once the library is loaded (lib())
COL_DTYPE = np.dtype([("slot", np.int32), ("elem", np.int32), ("dslot", np.int32), ("delem", np.int32), ("lo", np.float64), ("hi", np.float64),
                      ("noise", np.float64), ("smooth", np.float64), ("offset", np.float64), ("scale", np.float64), ("out_lo", np.float64),
                      ("out_hi", np.float64)])
CMD_FIELDS = np.array(P.ACT_CMD_FIELDS, dtype=np.int32)


class ActArgs(ctypes.Structure):
    _fields_ = [("fields", ctypes.POINTER(ObsField)), ("nfields", _ci), ("depth_field", _ci), ("nenv", _ci),
                ("cmd_fields", _vp), ("ncmd", _ci),
                ("cols", _vp), ("ncols", _ci), ("delay_max", _ci), ("dtype", _ci), ("seed", ctypes.c_ulonglong), ("env_base", ctypes.c_uint),
                ("actions", _vp), ("act_stride", _ll), ("act_dtype", _ci),
                ("input", _vp), ("input_dim", _ci), ("input_stride", _ll), ("input_dtype", _ci),
                ("delay", _vp),
                ("rows", _vp), ("srow", _ll), ("state", _vp), ("counts", _vp)]


def lib():
    global _declared, ACT_GRID, MAXSLOTS, MAXDST
    L = emu_py.lib()
    if not _declared:
        L.emu_act_last_refusal.restype = ctypes.c_char_p
        L.emu_act_constants.argtypes, L.emu_act_constants.restype = [_vp], None
        L.emu_act_grid.argtypes = [_ci]
        L.emu_act_check.argtypes, L.emu_act_check.restype = [ctypes.POINTER(ActArgs), _vp], ctypes.c_char_p
        L.emu_act_columns.argtypes = [ctypes.POINTER(ActArgs), _vp]
        L.emu_act_call_check.argtypes, L.emu_act_call_check.restype = [ctypes.POINTER(ActArgs), _ci, _vp, _ci, _ci], ctypes.c_char_p
        L.emu_act_record.argtypes = [ctypes.POINTER(ActArgs), _ci, _ci, _vp, _vp]
        L.emu_act.argtypes = [ctypes.POINTER(ActArgs), _ci, _ci, _vp, _ci]
        c = np.zeros(8, dtype=np.int64)
        L.emu_act_constants(c.ctypes.data)
        assert (int(c[1]), int(c[2]), int(c[4])) == (P.ACT_MAXCOLS, P.ACT_MAXDELAY, len(P.ACT_CMD_FIELDS))
        assert (int(c[5]), int(c[6]), int(c[7])) == (P.ACT_COL_DTYPE.itemsize, COL_DTYPE.itemsize, ctypes.sizeof(ActArgs))
        ACT_GRID, MAXSLOTS, MAXDST = int(c[0]), int(c[3]), int(c[4])
        _declared = True
    return L


def grid(n):
    """ck::act_grid."""
    return lib().emu_act_grid(n)


def _dtype_code(dtype):
    return dtype if isinstance(dtype, int) else P._obs_dtype(dtype)


class Call:
    """What the batch holds and how the actions are configured, as the arguments of the emulator's entry points.  fields: {field id:
    float64 array [nenv][>= dim]} -- a 2-D view with a row stride stands for a strided binding, and the destination fields are written in
    place; dims: {field id: row length} where it is not the array's width.  actions: [nenv][>= ncols] float32 / float64 or None; inp: the
    bound input array or None; delay: int32 [nenv] or None.  rows: [nenv][>= 3 ncols] of the dtype, state: float64 [nenv][(delay_max + 3)
    ncols], counts: uint32 [nenv]; all the caller's, written in place."""

    def __init__(self, fields, nenv, cols, delay_max=0, dtype=np.float32, seed=0, env_base=0, actions=None, inp=None, input_dim=None, delay=None, rows=None,
                 state=None, counts=None, dims=None, ncols=None, cmd_fields=CMD_FIELDS):
        self.keep = [fields, actions, inp, delay, rows, state, counts, cmd_fields]
        self.table = P.act_cols(cols)
        self.farr = (ObsField * NFIELDS)()
        for f, a in fields.items():
            assert a.dtype == np.float64 and a.ndim == 2 and a.strides[1] == 8 and a.strides[0] % 8 == 0
            self.farr[f] = ObsField(a.ctypes.data, (dims or {}).get(f, a.shape[1]), a.strides[0] // 8)
        self.a = ActArgs(fields=self.farr, nfields=NFIELDS, depth_field=P.F_DEPTH, nenv=nenv, cmd_fields=cmd_fields.ctypes.data, ncmd=len(cmd_fields),
                         cols=self.table.ctypes.data if self.table.size else None, ncols=self.table.size if ncols is None else ncols,
                         delay_max=delay_max, dtype=_dtype_code(dtype), seed=seed, env_base=env_base)
        if actions is not None:
            self.bind_actions(actions)
        if inp is not None:
            self.bind_input(inp, input_dim)
        if delay is not None:
            assert delay.dtype == np.int32
            self.a.delay = delay.ctypes.data
        if rows is not None:
            assert rows.ndim == 2 and rows.strides[1] == rows.itemsize
            self.a.rows, self.a.srow = rows.ctypes.data, rows.strides[0] // rows.itemsize
        if state is not None:
            assert state.dtype == np.float64 and state.flags.c_contiguous
            self.a.state = state.ctypes.data
        if counts is not None:
            assert counts.dtype == np.uint32
            self.a.counts = counts.ctypes.data

    def bind_actions(self, actions, dtype=None, stride=None):
        self.keep.append(actions)
        self.a.actions = actions.ctypes.data
        self.a.act_stride = actions.strides[0] // actions.itemsize if stride is None else stride
        self.a.act_dtype = _dtype_code(actions.dtype if dtype is None else dtype)

    def bind_input(self, inp, input_dim=None, dtype=None, stride=None):
        self.keep.append(inp)
        self.a.input, self.a.input_dim = inp.ctypes.data, inp.shape[1] if input_dim is None else input_dim
        self.a.input_stride = inp.strides[0] // inp.itemsize if stride is None else stride
        self.a.input_dtype = _dtype_code(inp.dtype if dtype is None else dtype)

    def check(self):
        """act_configure and the bind checks -> (refusal or None, the record's numbers)."""
        ints = np.zeros(7 + 2 * 16 + 2 * 9, dtype=np.int64)
        why = lib().emu_act_check(ctypes.byref(self.a), ints.ctypes.data)
        if why is not None:
            return why.decode(), None
        names = ("ncols", "delay_max", "dtype", "nslots", "ndst", "input_need", "state_dim")
        rec = dict(zip(names, (int(v) for v in ints[:7])))
        rec["slot_field"], rec["slot_dim"] = [int(v) for v in ints[7:7 + rec["nslots"]]], [int(v) for v in ints[23:23 + rec["nslots"]]]
        rec["dst_field"], rec["dst_dim"] = [int(v) for v in ints[39:39 + rec["ndst"]]], [int(v) for v in ints[48:48 + rec["ndst"]]]
        return None, rec

    def columns(self):
        """The column table [ncols] (COL_DTYPE)."""
        cols = np.zeros(P.ACT_MAXCOLS, dtype=COL_DTYPE)
        n = lib().emu_act_columns(ctypes.byref(self.a), cols.ctypes.data)
        assert n >= 0, (lib().emu_act_last_refusal() or b"").decode()
        return cols[:n]

    def call_check(self, env0, n, configured=True, now=None):
        """ck::check_act_call -> refusal or None.  now: {field id: (array or None, dim)} that differ at the call from the configure call."""
        arr = None
        if now is not None:
            arr = (ObsField * NFIELDS)(*self.farr)
            for f, (a, dim) in now.items():
                arr[f] = ObsField(None if a is None else a.ctypes.data, dim, 0 if a is None else a.strides[0] // 8)
        why = lib().emu_act_call_check(ctypes.byref(self.a), int(configured), arr, env0, n)
        return None if why is None else why.decode()

    def record(self, env0, n, reset=None):
        """What ck::make_act_io makes of the configuration and an env range -> (dict of the record's numbers, [(base, stride, f32)] per
        source slot, [(base, stride)] per destination slot)."""
        out = np.zeros(20 + 3 * 16 + 2 * 9, dtype=np.uint64)
        rc = lib().emu_act_record(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), out.ctypes.data)
        assert rc == 0, (lib().emu_act_last_refusal() or b"").decode()
        names = ("env0", "n", "ncols", "delay_max", "f32", "act_f32", "env_base", "key0", "key1", "cols", "actions", "sact", "rows", "srow", "state", "counts",
                 "delay", "reset", "nslots", "ndst")
        rec = dict(zip(names, (int(v) for v in out[:20])))
        src = [tuple(int(v) for v in out[20 + 3 * s: 23 + 3 * s]) for s in range(rec["nslots"])]
        dst = [tuple(int(v) for v in out[68 + 2 * s: 70 + 2 * s]) for s in range(rec["ndst"])]
        return rec, src, dst

    def act(self, env0=0, n=None, reset=None, grid=0):
        """phys_batch_act on the emulator: the destination elements, the rows, the state and the counts of the range, in place."""
        n = self.a.nenv - env0 if n is None else n
        reset = None if reset is None else np.ascontiguousarray(reset, dtype=np.int32)
        rc = lib().emu_act(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), grid)
        assert rc == 0, (lib().emu_act_last_refusal() or b"").decode()
