"""ctypes access to the draw kernels on the CPU wave emulator (tests/emu/emu_draw.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_draw.cpp adds.  Every array of a run is a numpy array of this
module's Draw: the library keeps nothing from call to call."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P

_vp, _ci, _ll, _ull, _cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_uint
_declared = False
F32, F64 = np.float32, np.float64


class DrawArgs(ctypes.Structure):
    _fields_ = [("A", _ci), ("nenv", _ci), ("perm_n", _ll), ("seed", _ull), ("env_base", _cu), ("epoch", _cu),
                ("dst", _vp), ("sdst", _ll), ("perm_dst", _vp),
                ("pol_A", _ci), ("pad", _ci), ("pol_eps", _vp), ("pol_seps", _ll),
                ("counts", _vp), ("perm", _vp),
                ("env0", _ci), ("n", _ci), ("grid", _ci), ("pad2", _ci)]


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        A = ctypes.POINTER(DrawArgs)
        L.emu_draw_last_refusal.restype = ctypes.c_char_p
        L.emu_draw_constants.argtypes, L.emu_draw_constants.restype = [_vp], None
        L.emu_draw_configure.argtypes = [A]
        L.emu_draw.argtypes = [A, _vp]
        L.emu_draw_perm.argtypes = [A, _vp]
        L.emu_draw_logn.argtypes, L.emu_draw_logn.restype = [_vp, _vp, _ll], None
        L.emu_draw_pair.argtypes, L.emu_draw_pair.restype = [_vp, _vp, _vp, _vp, _ll], None
        L.emu_draw_philox.argtypes, L.emu_draw_philox.restype = [_vp, _vp, _vp], None
        c = np.zeros(6, dtype=np.int64)
        L.emu_draw_constants(c.ctypes.data)
        assert (int(c[0]), int(c[1])) == (P.DRAW_MAXA, P.DRAW_MAXPERM) and int(c[5]) == ctypes.sizeof(DrawArgs)
        lib.GRID, lib.PERM_GRID, lib.ROUNDS = int(c[2]), int(c[3]), int(c[4])
        _declared = True
    return L


def refusal():
    return (lib().emu_draw_last_refusal() or b"").decode()


def logn(x):
    x = np.ascontiguousarray(x, dtype=F64)
    y = np.empty_like(x)
    lib().emu_draw_logn(x.ctypes.data, y.ctypes.data, x.size)
    return y


def pair(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
    zc, zs = np.empty(a.size, dtype=F64), np.empty(a.size, dtype=F64)
    lib().emu_draw_pair(a.ctypes.data, b.ctypes.data, zc.ctypes.data, zs.ctypes.data, a.size)
    return zc, zs


def philox(counter, key):
    c, k, out = np.array(counter, dtype=np.uint32), np.array(key, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    lib().emu_draw_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return tuple(int(v) for v in out)


class Draw:
    """The draw rows on the emulator: the arrays the batch owns on the device (the counts, the permutation), a destination of this run's
    (rows, `fill` until written; bound unless bind=False) and, for the calls that resolve, what stands for the policy's sample binding."""

    def __init__(self, nenv, A, perm_n=0, seed=0, env_base=0, stride=None, fill=np.nan, bind=True):
        self.a = a = DrawArgs(A=A, nenv=nenv, perm_n=perm_n, seed=seed & 0xFFFFFFFFFFFFFFFF, env_base=env_base)
        self.nenv, self.A = nenv, A
        self.why = None if lib().emu_draw_configure(ctypes.byref(a)) == 0 else refusal()
        self.rows = np.full((nenv, max(A, 1) if stride is None else stride), fill, dtype=F32)
        self.counts = np.zeros(nenv, dtype=np.uint32)
        self.perm = np.full(max(perm_n, 1), -1, dtype=np.int32)
        a.counts, a.perm = self.counts.ctypes.data, self.perm.ctypes.data
        if bind and A > 0:
            a.dst, a.sdst = self.rows.ctypes.data, self.rows.shape[1]
        self.info = None

    def policy(self, A, bound=True):
        """What stands for the batch's policy: an actor of A outputs, and this run's rows as the eps of its sample binding."""
        a = self.a
        a.pol_A = A
        a.pol_eps, a.pol_seps = (self.rows.ctypes.data, self.rows.shape[1]) if bound else (None, 0)

    def try_draw(self, env0=0, n=None, grid=0):
        """-> None, or the message of the refusal."""
        a = self.a
        a.env0, a.n, a.grid = env0, self.nenv - env0 if n is None else n, grid
        info = np.zeros(4, dtype=np.int64)
        if lib().emu_draw(ctypes.byref(a), info.ctypes.data) != 0:
            return refusal()
        self.info = dict(lanes=int(info[0]), per_wave=int(info[1]), vec=int(info[2]), grid=int(info[3]))
        return None

    def draw(self, env0=0, n=None, grid=0):
        why = self.try_draw(env0, n, grid)
        assert why is None, why
        return self.rows

    def try_perm(self, epoch, grid=0):
        a = self.a
        a.epoch, a.grid = epoch & 0xFFFFFFFF, grid
        info = np.zeros(3, dtype=np.int64)
        if lib().emu_draw_perm(ctypes.byref(a), info.ctypes.data) != 0:
            return refusal()
        self.pinfo = dict(h=int(info[0]), walk_max=int(info[1]), grid=int(info[2]))
        return None

    def draw_perm(self, epoch, grid=0):
        why = self.try_perm(epoch, grid)
        assert why is None, why
        return self.perm
