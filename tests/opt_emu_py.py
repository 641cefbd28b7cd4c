"""ctypes access to the optimiser kernels on the CPU wave emulator (tests/emu/emu_opt.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_opt.cpp adds.  Every array of a run is a numpy array of this
module's Opt: the library keeps nothing from call to call."""
import ctypes

import numpy as np

import emu_py
import grad_cases as gcs
from cassie_amd import phys as P

_vp, _ci, _ll, _cd, _cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_uint
_declared = False
F32, F64 = np.float32, np.float64
FILL = gcs.FILL


class OptArgs(ctypes.Structure):
    _fields_ = [("nets", _vp), ("nnets", _ci), ("in_dim", _ci),
                ("w", _vp * 8), ("sw", _ll * 8), ("b", _vp * 8),
                ("loaded", _cu), ("pad", _ci),
                ("log_std", _vp), ("opt_ls", _vp),
                ("dw", _vp * 8), ("sdw", _ll * 8), ("db", _vp * 8), ("dls", _vp),
                ("beta1", _cd), ("beta2", _cd), ("eps", _cd), ("max_norm", _cd), ("lr", _cd),
                ("grad_called", _ci), ("grid", _ci),
                ("packed", _vp), ("packt", _vp), ("mom", _vp), ("part", _vp), ("sc", _vp)]


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        A = ctypes.POINTER(OptArgs)
        L.emu_opt_last_refusal.restype = ctypes.c_char_p
        L.emu_opt_constants.argtypes, L.emu_opt_constants.restype = [_vp], None
        L.emu_opt_sizes.argtypes = [A, _vp]
        L.emu_opt_begin.argtypes = [A]
        L.emu_opt_check.argtypes, L.emu_opt_check.restype = [A], ctypes.c_char_p
        L.emu_opt_step.argtypes = [A]
        L.emu_opt_region.argtypes = [A, _ci, _ci, _ci, _vp]
        c = np.zeros(7, dtype=np.int64)
        L.emu_opt_constants(c.ctypes.data)
        assert (int(c[0]), int(c[3])) == (P.OPT_SEG, P.OPT_NSTATS) and int(c[6]) == ctypes.sizeof(OptArgs)
        lib.SC_COUNT, lib.SC_T = int(c[4]), int(c[5])
        _declared = True
    return L


def refusal():
    return (lib().emu_opt_last_refusal() or b"").decode()


class Opt:
    """The optimiser rows of a grad_cases.Case on the emulator: master tensors with a row stride (FILL between the rows), gradient
    tensors of the same form, and the arrays the batch owns on the device."""

    def __init__(self, case, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=np.inf, bind=True, load=True, bind_ls=True, begin=True):
        p = case.p
        self.case = case
        self.table = P.pol_nets(p.defs, p.in_dim)
        self.a = a = OptArgs(nets=self.table.ctypes.data, nnets=len(p.defs), in_dim=p.in_dim, beta1=beta1, beta2=beta2, eps=eps, max_norm=max_norm,
                             grad_called=1)
        self.shapes = [(w.shape[0], w.shape[1] - p.wpad) for layers in p.weights for w, _ in layers]
        self.slots = [(n, l) for n, layers in enumerate(p.weights) for l in range(len(layers))]
        self.wfull = [w.copy() for layers in p.weights for w, _ in layers]           # [out][in + wpad], FILL in the padding
        self.b = [np.array(b, dtype=F32) for layers in p.weights for _, b in layers]
        self.ls = np.array(case.log_std, dtype=F32)
        dw, db, self.dls = gcs.result_tensors(case)
        self.dwfull, self.db = [t for per in dw for t in per], [t for per in db for t in per]
        for k, (n, l) in enumerate(self.slots):
            s = 4 * n + l
            if bind or load:
                a.w[s], a.sw[s], a.b[s] = self.wfull[k].ctypes.data, self.wfull[k].strides[0] // 4, self.b[k].ctypes.data
            if load:
                a.loaded |= 1 << s
            a.dw[s], a.sdw[s], a.db[s] = self.dwfull[k].ctypes.data, self.dwfull[k].strides[0] // 4, self.db[k].ctypes.data
        a.dls, a.log_std = self.dls.ctypes.data, self.ls.ctypes.data
        if bind_ls:
            a.opt_ls = self.ls.ctypes.data
        sizes = np.zeros(5, dtype=np.int64)
        self.ok = lib().emu_opt_sizes(ctypes.byref(a), sizes.ctypes.data) == 0
        if not self.ok:
            return
        self.Q, self.nseg = int(sizes[2]), int(sizes[3])
        self.packed, self.packt = np.full(int(sizes[0]), FILL, dtype=F32), np.full(int(sizes[1]), FILL, dtype=F32)
        self.mom, self.part, self.sc = np.full(2 * self.Q, FILL, dtype=F32), np.full(self.nseg, FILL, dtype=F64), np.full(int(sizes[4]), FILL, dtype=F64)
        a.packed, a.packt, a.mom, a.part, a.sc = (x.ctypes.data for x in (self.packed, self.packt, self.mom, self.part, self.sc))
        if begin:
            self.begin()
            if not bind:                                   # (loaded from them, not bound)
                for n, l in self.slots:
                    a.w[4 * n + l], a.b[4 * n + l] = None, None

    def begin(self):
        """load_policy of every layer from the master tensors as they are now, and configure_opt's state: moments +0.0, t = 0."""
        assert lib().emu_opt_begin(ctypes.byref(self.a)) == 0, refusal()

    def set_params(self, ws, bs, ls):
        """Other values in the master tensors (a checkpoint's): begin() loads them."""
        for k in range(len(self.slots)):
            self.w(k)[:] = ws[k]
            self.b[k][:] = bs[k]
        self.ls[:] = ls

    def w(self, k):
        return self.wfull[k][:, : self.shapes[k][1]]

    def set_grads(self, dws, dbs, dls):
        """The gradients of a call, per slot dense dW [out][in] and db [out], into the bound gradient tensors."""
        for k in range(len(self.slots)):
            self.dwfull[k][:, : self.shapes[k][1]] = dws[k]
            self.db[k][:] = dbs[k]
        self.dls[:] = dls

    def check(self, lr=1e-3, grad_called=True):
        self.a.lr, self.a.grad_called = lr, int(grad_called)
        why = lib().emu_opt_check(ctypes.byref(self.a))
        return None if why is None else why.decode()

    def step(self, lr, grid=0):
        self.a.lr, self.a.grid, self.a.grad_called = lr, grid, 1
        assert lib().emu_opt_step(ctypes.byref(self.a)) == 0, refusal()
        return self.snapshot()

    def region(self, what, net=0, layer=0):
        """What phys_batch_opt_download(what, net, layer) hands out: a view into this run's arrays (writable: the upload)."""
        r = np.zeros(4, dtype=np.int64)
        assert lib().emu_opt_region(ctypes.byref(self.a), what, net, layer, r.ctypes.data) == 0
        off, rows, width, pitch = (int(v) for v in r)
        base = self.sc if what == P.OPT_SCALARS else self.part if what == P.OPT_PARTIALS else self.mom
        return np.lib.stride_tricks.as_strided(base[off:], shape=(rows, width), strides=(pitch * base.itemsize, base.itemsize))

    def snapshot(self):
        """Every word of the run in opt_cases' form."""
        T = lib.SC_T
        return {"w": [self.w(k).copy() for k in range(len(self.slots))], "wfull": [w.copy() for w in self.wfull], "b": [b.copy() for b in self.b],
                "ls": self.ls.copy(), "packed": self.packed.copy(), "packt": self.packt.copy(), "m": self.mom[: self.Q].copy(),
                "v": self.mom[self.Q:].copy(), "part": self.part.copy(), "scalars": self.sc[T: T + 4].copy(), "stats": self.sc[:8].copy()}
