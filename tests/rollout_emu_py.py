"""ctypes access to the rollout kernels on the CPU wave emulator (tests/emu/emu_rollout.cpp) -- test infrastructure only.  The library is
the one tests/emu_py.py loads; this module declares the entry points emu_rollout.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P

_vp, _ci, _ll, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
_declared = False
CONSTANTS = None                       # {name: ck::ROLLOUT_*}, once the library is loaded (lib())
N = P.RO_MAXSRC


class Live(ctypes.Structure):
    """ck::RolloutLive: where the batch reads or writes, now, what an unbound source is resolved from."""
    _fields_ = [("obs", _vp), ("obs_dim", _ci), ("obs_stride", _ll),
                ("mu", _vp), ("mu_dim", _ci), ("mu_stride", _ll),
                ("value", _vp), ("value_stride", _ll),
                ("action", _vp), ("action_dim", _ci), ("action_stride", _ll), ("logp", _vp),
                ("rew", _vp), ("rew_stride", _ll), ("rew_dtype", _ci),
                ("done", _vp), ("reason", _vp)]


class RolloutArgs(ctypes.Structure):
    _fields_ = [("srcs", _vp), ("nsrcs", _ci), ("T", _ci), ("nenv", _ci), ("tmask", ctypes.c_uint),
                ("gamma", _d), ("lam", _d),
                ("src", _vp * N), ("ssrc", _ll * N),
                ("store", _vp * N), ("step", _ll * N), ("row", _ll * N),
                ("arr", _vp * 3), ("arr_step", _ll * 3), ("arr_row", _ll * 3),
                ("q", _vp), ("live", Live)]


def lib():
    global _declared, CONSTANTS
    L = emu_py.lib()
    if not _declared:
        A = ctypes.POINTER(RolloutArgs)
        L.emu_rollout_last_refusal.restype = ctypes.c_char_p
        L.emu_rollout_constants.argtypes, L.emu_rollout_constants.restype = [_vp], None
        L.emu_rollout_check.argtypes, L.emu_rollout_check.restype = [A, _ci, _ci, _ci, _ci, _ci, _vp, _ll, _d], ctypes.c_char_p
        L.emu_rollout_record.argtypes = [A, _ci, _ci, _ci, _ci, _vp]
        L.emu_rollout_finish.argtypes = [A, _ci, _ci, _vp, _ll, _ci]
        L.emu_rollout_normalise.argtypes = [A, _d, _ci]
        c = np.zeros(10, dtype=np.int64)
        L.emu_rollout_constants(c.ctypes.data)
        assert tuple(int(v) for v in c[:3]) == (P.RO_MAXT, P.RO_MAXSRC, P.RO_MAXDIM)
        assert (int(c[8]), int(c[9])) == (ctypes.sizeof(RolloutArgs), ctypes.sizeof(Live))
        CONSTANTS = dict(zip(("MAXT", "MAXSRC", "MAXDIM", "JOB", "GRID", "FIN_GRID", "SCALE_GRID", "AHEAD"), (int(v) for v in c[:8])))
        _declared = True
    return L


ARRAYS = {P.RO_ADV: 0, P.RO_RET: 1, P.RO_ADVN: 2, "adv": 0, "ret": 1, "advn": 2}


class Call:
    """A rollout as the arguments of the emulator's entry points.  srcs: (role, dim) pairs, passed as written.  Everything bound is the
    caller's numpy array, written in place."""

    def __init__(self, srcs, steps, nenv, gamma=0.99, lam=0.95, tmask=0, nsrcs=None):
        srcs = list(srcs)
        self.keep = []
        self.table = P.ro_srcs(srcs[: P.RO_MAXSRC]) if len(srcs) <= P.RO_MAXSRC else np.zeros(len(srcs), dtype=P.RO_SRC_DTYPE)
        self.a = RolloutArgs(srcs=self.table.ctypes.data if srcs else None, nsrcs=len(srcs) if nsrcs is None else nsrcs, T=steps, nenv=nenv,
                             tmask=tmask, gamma=gamma, lam=lam)
        self.q = np.zeros(2 * nenv + 4, dtype=np.float64)
        self.a.q = self.q.ctypes.data

    @classmethod
    def of_case(cls, case, stores=None, arrays=None):
        """The call of a rollout_cases.Case with its stores (rollout_cases.Store per source) and ADV / RET / ADVN ({name: Store}) bound;
        the sources are bound per step (bind_step)."""
        c = cls(case.srcs, case.T, case.nenv, case.gamma, case.lam, case.tmask)
        for s, st in enumerate(stores or []):
            c.bind_storage(s, st.buf, st.step, st.row)
        for name, st in (arrays or {}).items():
            c.bind_storage(name, st.buf, st.step, st.row)
        return c

    def bind_source(self, s, a, stride=None):
        """a: a 2-D array of 4-byte elements (its row stride is the source's), or None."""
        self.keep.append(a)
        self.a.src[s] = emu_py._ptr(a)
        self.a.ssrc[s] = (0 if a is None else a.strides[0] // 4) if stride is None else stride

    def bind_step(self, tensors):
        for s, a in enumerate(tensors):
            self.bind_source(s, a)

    def bind_storage(self, s, buf, step, row):
        self.keep.append(buf)
        if s in ARRAYS:
            k = ARRAYS[s]
            self.a.arr[k], self.a.arr_step[k], self.a.arr_row[k] = emu_py._ptr(buf), step, row
        else:
            self.a.store[s], self.a.step[s], self.a.row[s] = emu_py._ptr(buf), step, row

    def check(self, what=0, t=0, env0=0, n=0, last=None, stride=1, eps=1e-8, configured=True):
        """rollout_configure and the bind checks, then (what 1 / 2 / 3) the check of a record / finish / normalise -> refusal or None."""
        why = lib().emu_rollout_check(ctypes.byref(self.a), int(configured), what, t, env0, n, emu_py._ptr(last), stride, eps)
        return None if why is None else why.decode()

    def _ok(self, rc):
        assert rc == 0, (lib().emu_rollout_last_refusal() or b"").decode()

    def record(self, t, env0=0, n=None, grid=0):
        """phys_batch_rollout_record on the emulator -> per source, whether it took the 16-byte path."""
        n = self.a.nenv - env0 if n is None else n
        vec = np.zeros(N, dtype=np.int32)
        self._ok(lib().emu_rollout_record(ctypes.byref(self.a), t, env0, n, grid, vec.ctypes.data))
        return vec[: self.a.nsrcs]

    def finish(self, env0=0, n=None, last=None, stride=None, grid=0):
        """phys_batch_rollout_finish on the emulator; last: a float32 array whose first axis is the envs (None: resolved)."""
        n = self.a.nenv - env0 if n is None else n
        self.keep.append(last)
        self._ok(lib().emu_rollout_finish(ctypes.byref(self.a), env0, n, emu_py._ptr(last), (1 if last is None else last.strides[0] // 4) if stride is None else stride, grid))

    def normalise(self, eps=1e-8, grid=0):
        """phys_batch_rollout_normalise on the emulator -> (mean, std, inv)."""
        self._ok(lib().emu_rollout_normalise(ctypes.byref(self.a), eps, grid))
        return tuple(self.q[2 * self.a.nenv: 2 * self.a.nenv + 3])
