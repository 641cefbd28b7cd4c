"""ctypes access to the normaliser kernels on the CPU wave emulator (tests/emu/emu_norm.cpp) -- test infrastructure only.  The library is
the one tests/emu_py.py loads; this module declares the entry points emu_norm.cpp adds.  Every array of a run is a numpy array of this
module's Norm: the library keeps nothing from call to call."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P

_vp, _ci, _ll, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
_declared = False
F32, F64 = np.float32, np.float64
FILL = 0.5


class NormArgs(ctypes.Structure):
    _fields_ = [("dim", _ci), ("block", _ci), ("max_rows", _ll), ("eps", _cd),
                ("src", _vp), ("steps", _ci), ("rows", _ci), ("step_stride", _ll), ("row_stride", _ll),
                ("out_mean", _vp), ("out_inv", _vp),
                ("nenv", _ci), ("ro_T", _ci), ("ro_dim", _ci), ("pol_in_dim", _ci), ("ro_store", _vp), ("ro_step", _ll), ("ro_row", _ll),
                ("pol_mean", _vp), ("pol_inv", _vp),
                ("state", _vp), ("part", _vp), ("cnt", _vp),
                ("last_R", _ll), ("last_blocks", _ll), ("calls", _ll),
                ("grid", _ci), ("pad", _ci)]


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        A = ctypes.POINTER(NormArgs)
        L.emu_norm_last_refusal.restype = ctypes.c_char_p
        L.emu_norm_constants.argtypes, L.emu_norm_constants.restype = [_vp], None
        L.emu_norm_sizes.argtypes = [A, _vp]
        L.emu_norm_update.argtypes = [A, _vp]
        L.emu_norm_write.argtypes = [A]
        L.emu_norm_stats.argtypes = [A, _vp]
        L.emu_norm_region.argtypes = [A, _ci, _ci, _vp]
        c = np.zeros(8, dtype=np.int64)
        L.emu_norm_constants(c.ctypes.data)
        assert tuple(int(v) for v in c[:4]) == (P.NORM_MINBLOCK, P.NORM_MAXBLOCK, P.NORM_MAXROWS, P.NORM_NSTATS) and int(c[7]) == ctypes.sizeof(NormArgs)
        lib.STATE_ROWS, lib.AHEAD, lib.GRID = int(c[4]), int(c[5]), int(c[6])
        _declared = True
    return L


def refusal():
    return (lib().emu_norm_last_refusal() or b"").decode()


class Norm:
    """The normaliser rows on the emulator: the arrays the batch owns on the device, the two outputs (FILL until a column is written)
    and, for the calls that resolve, what stands for the rollout's OBS store and the policy's bound normalisation."""

    def __init__(self, D, block, max_rows=1 << 20, eps=1e-8, bind_output=True):
        self.a = a = NormArgs(dim=D, block=block, max_rows=max_rows, eps=eps)
        self.D = D
        sizes = np.zeros(4, dtype=np.int64)
        self.ok = lib().emu_norm_sizes(ctypes.byref(a), sizes.ctypes.data) == 0
        if not self.ok:
            return
        self.max_blocks = int(sizes[3])
        self.state, self.part, self.cnt = np.zeros(int(sizes[0]), dtype=F64), np.zeros(int(sizes[1]), dtype=F64), np.zeros(int(sizes[2]), dtype=np.int32)
        self.mean, self.inv = np.full(D, FILL, dtype=F32), np.full(D, FILL, dtype=F32)
        a.state, a.part, a.cnt = self.state.ctypes.data, self.part.ctypes.data, self.cnt.ctypes.data
        if bind_output:
            a.out_mean, a.out_inv = self.mean.ctypes.data, self.inv.ctypes.data
        self.info, self._keep = None, None

    def bind_source(self, ptr, steps, rows, step_stride, row_stride, keep=None):
        a = self.a
        a.src, a.steps, a.rows, a.step_stride, a.row_stride = ptr, steps, rows, step_stride, row_stride
        self._keep = keep

    def rollout(self, T, nenv, dim, store=None, step=0, row=0):
        """What stands for the batch's rollout: T steps of nenv envs with an OBS source of `dim` words (0: none) in `store`."""
        a = self.a
        a.ro_T, a.nenv, a.ro_dim, a.ro_step, a.ro_row = T, nenv, dim, step, row
        a.ro_store = None if store is None else store.ctypes.data
        self._keep = store

    def policy(self, in_dim, bound=True):
        """What stands for the batch's policy: in_dim, and this run's outputs as its bound normalisation."""
        a = self.a
        a.pol_in_dim = in_dim
        a.pol_mean, a.pol_inv = (self.mean.ctypes.data, self.inv.ctypes.data) if bound else (None, None)

    def try_update(self, grid=0):
        """-> None, or the message of the refusal."""
        self.a.grid = grid
        info = np.zeros(4, dtype=np.int64)
        if lib().emu_norm_update(ctypes.byref(self.a), info.ctypes.data) != 0:
            return refusal()
        self.info = dict(R=int(info[0]), blocks=int(info[1]), vec=int(info[2]), grid=int(info[3]))
        self.a.last_R, self.a.last_blocks, self.a.calls = int(info[0]), int(info[1]), self.a.calls + 1
        return None

    def update(self, grid=0):
        why = self.try_update(grid)
        assert why is None, why
        return self.snapshot()

    def try_write(self):
        return None if lib().emu_norm_write(ctypes.byref(self.a)) == 0 else refusal()

    def write(self):
        why = self.try_write()
        assert why is None, why

    def region(self, what, upload=False):
        """What phys_batch_norm_download(what) hands out: a view into this run's arrays (writable: the upload); None: no such thing."""
        r = np.zeros(5, dtype=np.int64)
        if lib().emu_norm_region(ctypes.byref(self.a), what, int(upload), r.ctypes.data) != 0:
            return None
        in_part, off, rows, width, pitch = (int(v) for v in r)
        base = self.part if in_part else self.state
        v = np.lib.stride_tricks.as_strided(base[off:], shape=(rows, width), strides=(pitch * 8, 8))
        return v.reshape(2, -1, self.D) if in_part else v[0]

    def stats(self):
        out = np.zeros(P.NORM_NSTATS, dtype=F64)
        assert lib().emu_norm_stats(ctypes.byref(self.a), out.ctypes.data) == 0, refusal()
        return out

    def snapshot(self):
        """Every word of the run in norm_cases' form."""
        names = ("n", "mean", "m2", "skipped", "excluded", "mb", "counts")
        snap = {k: self.region(i).copy() for i, k in enumerate(names)}
        a12 = self.region(P.NORM_PARTIALS)
        snap.update(a1=a12[0].copy(), a2=a12[1].copy(), out_mean=self.mean.copy(), out_inv=self.inv.copy(), stats=self.stats())
        return snap
