"""ctypes access to the event kernel on the CPU wave emulator (tests/emu/emu_events.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_events.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P
from obs_emu_py import NFIELDS, ObsField

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_declared = False
EVENT_GRID = MAXSLOTS = None    # ck::EVENT_GRID, ck::EVENT_MAXSLOTS, once the library is loaded (lib())


class EventsArgs(ctypes.Structure):
    _fields_ = [("fields", ctypes.POINTER(ObsField)), ("nfields", _ci), ("depth_field", _ci), ("nenv", _ci),
                ("cols", _vp), ("ncols", _ci), ("dtype", _ci), ("done_mask", ctypes.c_ulonglong),
                ("input", _vp), ("input_dim", _ci), ("input_stride", _ll), ("input_dtype", _ci),
                ("rows", _vp), ("srow", _ll), ("flags", _vp), ("state", _vp), ("words", _vp), ("counts", _vp)]


def lib():
    global _declared, EVENT_GRID, MAXSLOTS
    L = emu_py.lib()
    if not _declared:
        L.emu_events_last_refusal.restype = ctypes.c_char_p
        L.emu_events_constants.argtypes, L.emu_events_constants.restype = [_vp], None
        L.emu_events_grid.argtypes = [_ci]
        L.emu_events_check.argtypes, L.emu_events_check.restype = [ctypes.POINTER(EventsArgs), _vp, _vp], ctypes.c_char_p
        L.emu_events_call_check.argtypes, L.emu_events_call_check.restype = [ctypes.POINTER(EventsArgs), _ci, _vp, _ci, _ci], ctypes.c_char_p
        L.emu_events.argtypes = [ctypes.POINTER(EventsArgs), _ci, _ci, _vp, _ci]
        c = np.zeros(6, dtype=np.int64)
        L.emu_events_constants(c.ctypes.data)
        assert (int(c[1]), int(c[2]), int(c[3])) == (P.EV_MAXCOLS, P.EV_MAXCOUNT, 16)
        assert (int(c[4]), int(c[5])) == (P.EV_COL_DTYPE.itemsize, ctypes.sizeof(EventsArgs))
        EVENT_GRID, MAXSLOTS = int(c[0]), int(c[3])
        _declared = True
    return L


def grid(n):
    """ck::events_grid."""
    return lib().emu_events_grid(n)


def _dtype_code(dtype):
    return dtype if isinstance(dtype, int) else P._obs_dtype(dtype)


class Call:
    """What the batch holds and how the event rows are configured, as the arguments of the emulator's entry points.  fields: {field id:
    float64 array [nenv][>= dim]} -- a 2-D view with a row stride stands for a strided binding; dims: {field id: row length} where it is
    not the array's width.  inp: float32 / float64 [nenv][>= input_dim] or None.  The outputs are this object's, in the HOST's shape:
    rows [nenv][ncols (+ pad)] of the dtype, flags int32 [nenv], state float64 [nenv][2][ncols], words uint32 [nenv][ncols], counts uint32
    [nenv]; a call moves the state and the words into the device's shape ([2][ncols][nenv], [ncols][nenv]) and back."""

    def __init__(self, fields, nenv, cols, dtype=np.float32, done_mask=0, inp=None, input_dim=None, dims=None, ncols=None, pad=0, fill=0.0, own_rows=True,
                 depth_field=P.F_DEPTH):
        self.table = P.ev_cols(cols)
        nc = self.table.size
        self.nenv, self.nc = nenv, nc
        self.farr = (ObsField * NFIELDS)()
        for f, a in fields.items():
            assert a.dtype == np.float64 and a.ndim == 2 and a.strides[1] == 8 and a.strides[0] % 8 == 0
            self.farr[f] = ObsField(a.ctypes.data, (dims or {}).get(f, a.shape[1]), a.strides[0] // 8)
        self.keep = [fields, inp]
        npdt = np.float64 if _dtype_code(dtype) == 8 else np.float32
        self.rows_raw = np.full((nenv, max(nc, 1) + pad), fill, dtype=npdt)
        self.rows = self.rows_raw[:, :nc]
        self.flags = np.zeros(nenv, dtype=np.int32)
        self.state = np.zeros((nenv, 2, nc), dtype=np.float64)
        self.words = np.zeros((nenv, nc), dtype=np.uint32)
        self.counts = np.zeros(nenv, dtype=np.uint32)
        self.a = EventsArgs(fields=self.farr, nfields=NFIELDS, depth_field=depth_field, nenv=nenv, cols=self.table.ctypes.data if nc else None,
                            ncols=nc if ncols is None else ncols, dtype=_dtype_code(dtype), done_mask=int(done_mask) & 0xFFFFFFFFFFFFFFFF)
        if own_rows:
            self.a.rows, self.a.srow = self.rows_raw.ctypes.data, self.rows_raw.shape[1]
        self.a.flags, self.a.counts = self.flags.ctypes.data, self.counts.ctypes.data
        if inp is not None:
            assert inp.ndim == 2 and inp.strides[1] == inp.itemsize and inp.dtype in (np.float32, np.float64)
            self.a.input, self.a.input_dim = inp.ctypes.data, inp.shape[1] if input_dim is None else input_dim
            self.a.input_stride, self.a.input_dtype = inp.strides[0] // inp.itemsize, inp.itemsize

    def check(self):
        """events_configure and the bind checks -> (refusal or None, the record's numbers, the table a launch reads)."""
        ints = np.zeros(4 + 2 * 16, dtype=np.int64)
        table = np.zeros(max(self.a.ncols, 1), dtype=P.EV_COL_DTYPE)
        why = lib().emu_events_check(ctypes.byref(self.a), ints.ctypes.data, table.ctypes.data if 0 < self.a.ncols <= P.EV_MAXCOLS else None)
        if why is not None:
            return why.decode(), None, None
        rec = dict(zip(("ncols", "dtype", "nslots", "input_need"), (int(v) for v in ints[:4])))
        rec["slot_field"], rec["slot_dim"] = [int(v) for v in ints[4:4 + rec["nslots"]]], [int(v) for v in ints[20:20 + rec["nslots"]]]
        return None, rec, table[:self.a.ncols]

    def call_check(self, env0, n, configured=True, now=None):
        """ck::check_events_call -> refusal or None.  now: {field id: (array or None, dim)} that differ at the call from the configure call."""
        arr = None
        dev = self._to_device()
        if now is not None:
            arr = (ObsField * NFIELDS)(*self.farr)
            for f, (a, dim) in now.items():
                arr[f] = ObsField(None if a is None else a.ctypes.data, dim, 0 if a is None else a.strides[0] // 8)
        why = lib().emu_events_call_check(ctypes.byref(self.a), int(configured), arr, env0, n)
        del dev
        return None if why is None else why.decode()

    def _to_device(self):
        st = np.ascontiguousarray(self.state.transpose(1, 2, 0))
        wd = np.ascontiguousarray(self.words.transpose(1, 0))
        self.a.state, self.a.words = st.ctypes.data, wd.ctypes.data
        return st, wd

    def events(self, env0=0, n=None, reset=None, grid=0):
        """phys_batch_events on the emulator: the rows, the done words, the state, the words and the counts of the range, in place."""
        n = self.nenv - env0 if n is None else n
        reset = None if reset is None else np.ascontiguousarray(reset, dtype=np.int32)
        st, wd = self._to_device()
        rc = lib().emu_events(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), grid)
        assert rc == 0, (lib().emu_events_last_refusal() or b"").decode()
        self.state[:], self.words[:] = st.transpose(2, 0, 1), wd.transpose(1, 0)

    def refusal(self, env0=0, n=None, reset=None):
        """The message with which a call is refused (None: it ran)."""
        n = self.nenv - env0 if n is None else n
        st, wd = self._to_device()
        rc = lib().emu_events(ctypes.byref(self.a), env0, n, None, 0)
        return (lib().emu_events_last_refusal() or b"").decode() if rc != 0 else None
