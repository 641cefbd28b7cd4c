"""ctypes access to the reward kernel on the CPU wave emulator (tests/emu/emu_rewards.cpp) -- test infrastructure only.  The library
is the one tests/emu_py.py loads; this module declares the entry points emu_rewards.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P
from obs_emu_py import NFIELDS, ObsField

_vp, _ci, _cd, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
_declared = False
REWARD_GRID = MAXSLOTS = None    # ck::REWARD_GRID, ck::REWARD_MAXSLOTS, once the library is loaded (lib())


class RewardArgs(ctypes.Structure):
    _fields_ = [("fields", ctypes.POINTER(ObsField)), ("nfields", _ci), ("depth_field", _ci), ("nenv", _ci),
                ("terms", _vp), ("nterms", _ci), ("dtype", _ci), ("lo", _cd), ("hi", _cd),
                ("input", _vp), ("input_dim", _ci), ("input_stride", _ll), ("input_dtype", _ci),
                ("rew", _vp), ("srew", _ll), ("trows", _vp), ("sterm", _ll), ("ret", _vp), ("fin", _vp)]


def lib():
    global _declared, REWARD_GRID, MAXSLOTS
    L = emu_py.lib()
    if not _declared:
        L.emu_reward_last_refusal.restype = ctypes.c_char_p
        L.emu_reward_constants.argtypes, L.emu_reward_constants.restype = [_vp], None
        L.emu_reward_grid.argtypes = [_ci]
        L.emu_reward_expn.argtypes, L.emu_reward_expn.restype = [_vp, _vp, _ll], None
        L.emu_reward_check.argtypes, L.emu_reward_check.restype = [ctypes.POINTER(RewardArgs), _vp, _vp], ctypes.c_char_p
        L.emu_reward_call_check.argtypes, L.emu_reward_call_check.restype = [ctypes.POINTER(RewardArgs), _ci, _vp, _ci, _ci], ctypes.c_char_p
        L.emu_reward_record.argtypes = [ctypes.POINTER(RewardArgs), _ci, _ci, _vp, _vp]
        L.emu_reward.argtypes = [ctypes.POINTER(RewardArgs), _ci, _ci, _vp, _ci]
        c = np.zeros(6, dtype=np.int64)
        L.emu_reward_constants(c.ctypes.data)
        assert (int(c[1]), int(c[2])) == (P.REW_MAXTERMS, P.REW_MAXCOUNT)
        assert (int(c[4]), int(c[5])) == (P.REW_TERM_DTYPE.itemsize, ctypes.sizeof(RewardArgs))
        REWARD_GRID, MAXSLOTS = int(c[0]), int(c[3])
        _declared = True
    return L


def expn(a):
    """The kernel's own ck::reward_expn on an array."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    out = np.empty_like(a)
    lib().emu_reward_expn(a.ctypes.data, out.ctypes.data, a.size)
    return out


def grid(n):
    """ck::reward_grid."""
    return lib().emu_reward_grid(n)


def _dtype_code(dtype):
    return dtype if isinstance(dtype, int) else P._obs_dtype(dtype)


def _strided(a):
    """(address, elements between two envs') of a [nenv] view or of [nenv] rows whose elements are contiguous."""
    assert a.strides[0] % a.itemsize == 0 and (a.ndim == 1 or a.strides[1] == a.itemsize)
    return a.ctypes.data, a.strides[0] // a.itemsize


class Call:
    """What the batch holds and how the reward is configured, as the arguments of the emulator's entry points.  fields: {field id: float64
    array [nenv][>= dim]} -- a 2-D view with a row stride stands for a strided binding; dims: {field id: row length} where it is not the
    array's width.  inp: the bound input array [nenv][>= input_dim] (float32 / float64) or None.  rew: [nenv] of the dtype (a strided
    1-D view stands for a bound column), rows: [nenv][>= nterms] or None, ret / fin: float64 [nenv]; all the caller's, written in place."""

    def __init__(self, fields, nenv, terms, dtype=np.float32, lo=-np.inf, hi=np.inf, inp=None, input_dim=None, rew=None, rows=None, ret=None, fin=None,
                 dims=None, nterms=None):
        self.keep = [fields, inp, rew, rows, ret, fin]
        self.table = P.rew_terms(terms)
        self.farr = (ObsField * NFIELDS)()
        for f, a in fields.items():
            assert a.dtype == np.float64 and a.ndim == 2 and a.strides[1] == 8 and a.strides[0] % 8 == 0
            self.farr[f] = ObsField(a.ctypes.data, (dims or {}).get(f, a.shape[1]), a.strides[0] // 8)
        self.a = RewardArgs(fields=self.farr, nfields=NFIELDS, depth_field=P.F_DEPTH, nenv=nenv, terms=self.table.ctypes.data if self.table.size else None,
                            nterms=self.table.size if nterms is None else nterms, dtype=_dtype_code(dtype), lo=lo, hi=hi)
        if inp is not None:
            self.bind_input(inp, input_dim)
        if rew is not None:
            assert rew.ndim == 1
            self.a.rew, self.a.srew = _strided(rew)
        if rows is not None:
            assert rows.ndim == 2
            self.a.trows, self.a.sterm = _strided(rows)
        for name, arr in (("ret", ret), ("fin", fin)):
            if arr is not None:
                assert arr.dtype == np.float64 and arr.flags.c_contiguous
                setattr(self.a, name, arr.ctypes.data)

    def bind_input(self, inp, input_dim=None, dtype=None, stride=None):
        self.keep.append(inp)
        self.a.input, self.a.input_dim = inp.ctypes.data, inp.shape[1] if input_dim is None else input_dim
        self.a.input_stride = inp.strides[0] // inp.itemsize if stride is None else stride
        self.a.input_dtype = _dtype_code(inp.dtype if dtype is None else dtype)

    def check(self):
        """reward_configure and the bind checks -> (refusal or None, the record's numbers, the term table with the fields as slots)."""
        ints, table = np.zeros(4 + 2 * 16, dtype=np.int64), np.zeros(max(self.table.size, 1), dtype=P.REW_TERM_DTYPE)
        why = lib().emu_reward_check(ctypes.byref(self.a), ints.ctypes.data, table.ctypes.data)
        if why is not None:
            return why.decode(), None, None
        rec = dict(zip(("nterms", "dtype", "nslots", "input_need"), (int(v) for v in ints[:4])))
        rec["slot_field"], rec["slot_dim"] = [int(v) for v in ints[4:4 + rec["nslots"]]], [int(v) for v in ints[20:20 + rec["nslots"]]]
        return None, rec, table[: self.table.size]

    def call_check(self, env0, n, configured=True, now=None):
        """ck::check_reward_call -> refusal or None.  now: {field id: (array or None, dim)} that differ at the call from the configure call."""
        arr = None
        if now is not None:
            arr = (ObsField * NFIELDS)(*self.farr)
            for f, (a, dim) in now.items():
                arr[f] = ObsField(None if a is None else a.ctypes.data, dim, 0 if a is None else a.strides[0] // 8)
        why = lib().emu_reward_call_check(ctypes.byref(self.a), int(configured), arr, env0, n)
        return None if why is None else why.decode()

    def record(self, env0, n, reset=None):
        """What ck::make_reward_io makes of the configuration and an env range -> (dict of the record's numbers, [(base, stride, f32)] per slot)."""
        out = np.zeros(14 + 3 * 16, dtype=np.uint64)
        nslots = lib().emu_reward_record(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), out.ctypes.data)
        assert nslots >= 0, (lib().emu_reward_last_refusal() or b"").decode()
        names = ("env0", "n", "nterms", "f32", "terms", "rew", "srew", "trows", "sterm", "ret", "fin", "reset")
        rec = dict(zip(names, (int(v) for v in out[:12])))
        rec["lo"], rec["hi"] = (float(v) for v in out[12:14].view(np.float64))
        return rec, [tuple(int(v) for v in out[14 + 3 * s: 17 + 3 * s]) for s in range(nslots)]

    def reward(self, env0=0, n=None, reset=None, grid=0):
        """phys_batch_reward on the emulator: the rewards, term rows and returns of the range, in place."""
        n = self.a.nenv - env0 if n is None else n
        reset = None if reset is None else np.ascontiguousarray(reset, dtype=np.int32)
        rc = lib().emu_reward(ctypes.byref(self.a), env0, n, emu_py._ptr(reset), grid)
        assert rc == 0, (lib().emu_reward_last_refusal() or b"").decode()
