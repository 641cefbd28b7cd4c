"""ctypes access to the gradient kernels on the CPU wave emulator (tests/emu/emu_grad.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_grad.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P

_vp, _ci, _ll, _cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
_declared = False
F32, F64 = np.float32, np.float64
SRC = ("obs", "action", "logp", "advn", "ret")
NSTATS = 8


class GradArgs(ctypes.Structure):
    _fields_ = [("nets", _vp), ("nnets", _ci), ("in_dim", _ci), ("nenv", _ci), ("T", _ci),
                ("w", _vp * 8), ("sw", _ll * 8), ("b", _vp * 8),
                ("mean", _vp), ("inv", _vp), ("clip", _cd),
                ("log_std", _vp),
                ("src", _vp * 5), ("step", _ll * 5), ("row", _ll * 5),
                ("max_m", _ci), ("chunk", _ci), ("eps", _cd), ("c_v", _cd), ("c_ent", _cd),
                ("idx", _vp), ("m", _ci), ("pad", _ci),
                ("dw", _vp * 8), ("sdw", _ll * 8), ("db", _vp * 8), ("dls", _vp)]


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        A = ctypes.POINTER(GradArgs)
        L.emu_grad_last_refusal.restype = ctypes.c_char_p
        L.emu_grad_constants.argtypes, L.emu_grad_constants.restype = [_vp], None
        L.emu_grad_check.argtypes, L.emu_grad_check.restype = [A], ctypes.c_char_p
        L.emu_grad.argtypes = [A, _ci]
        L.emu_grad_fetch.argtypes, L.emu_grad_fetch.restype = [_ci, _ci, _ci, _vp], _ll
        L.emu_grad_fetch_raw.argtypes, L.emu_grad_fetch_raw.restype = [_ci, _ci, _ci, _vp, ctypes.POINTER(_ci)], _ll
        c = np.zeros(7, dtype=np.int64)
        L.emu_grad_constants(c.ctypes.data)
        assert (int(c[3]), int(c[4]), int(c[5])) == (P.GRAD_MINCHUNK, P.GRAD_MAXCHUNK, P.GRAD_NSTATS) and int(c[6]) == ctypes.sizeof(GradArgs)
        _declared = True
    return L


class Call:
    """A gradient call of a grad_cases.Case as the arguments of the emulator's entry points."""

    def __init__(self, case, chunk, max_m=None, load=True, skip=(), eps=None, c_v=None, c_ent=None):
        p = case.p
        self.case, self.keep = case, []
        self.table = P.pol_nets(p.defs, p.in_dim)
        self.a = GradArgs(nets=self.table.ctypes.data, nnets=len(p.defs), in_dim=p.in_dim, nenv=case.nenv, T=case.T)
        if load:
            for n, layers in enumerate(p.weights):
                for l, (w, b) in enumerate(layers):
                    s = 4 * n + l
                    self.a.w[s], self.a.sw[s], self.a.b[s] = w.ctypes.data, w.strides[0] // 4, b.ctypes.data
        if p.norm is not None:
            mean, inv = (np.ascontiguousarray(v, dtype=F32) for v in p.norm[:2])
            self.keep += [mean, inv]
            self.a.mean, self.a.inv, self.a.clip = mean.ctypes.data, inv.ctypes.data, p.norm[2]
        self.log_std = np.ascontiguousarray(case.log_std, dtype=F32)
        self.a.log_std = self.log_std.ctypes.data
        for k, name in enumerate(SRC):
            if name in skip or (name == "ret" and len(p.defs) < 2):
                continue
            self.a.src[k], self.a.step[k], self.a.row[k] = case.arr[name].ctypes.data, case.step[name], case.row[name]
        self.a.max_m = case.S if max_m is None else max_m
        self.a.chunk = chunk
        self.a.eps, self.a.c_v, self.a.c_ent = (case.eps if eps is None else eps, case.c_v if c_v is None else c_v, case.c_ent if c_ent is None else c_ent)

    def bind(self, dw, db, dls):
        """The caller's gradient tensors: dw[net][layer] 2-D float32 views (their row stride is the tensor's), db[net][layer], dls."""
        self.keep += [dw, db, dls]
        for n in range(len(dw)):
            for l in range(len(dw[n])):
                s = 4 * n + l
                self.a.dw[s], self.a.sdw[s], self.a.db[s] = dw[n][l].ctypes.data, dw[n][l].strides[0] // 4, db[n][l].ctypes.data
        self.a.dls = dls.ctypes.data

    def check(self, idx=None, m=None):
        idx = np.zeros(1, dtype=np.int32) if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
        self.a.idx, self.a.m = idx.ctypes.data, len(idx) if m is None else m
        why = lib().emu_grad_check(ctypes.byref(self.a))
        return None if why is None else why.decode()

    def grad(self, idx, grid=0):
        """phys_batch_grad on the emulator -> the result in grad_check.grad's form."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        self.a.idx, self.a.m = idx.ctypes.data, len(idx)
        rc = lib().emu_grad(ctypes.byref(self.a), grid)
        assert rc == 0, (lib().emu_grad_last_refusal() or b"").decode()
        return fetch_all(self.case, len(idx), self.a.chunk, fetch)


def fetch(what, net=0, layer=0, dtype=F32):
    L = lib()
    n = L.emu_grad_fetch(what, net, layer, None)
    assert n >= 0
    out = np.zeros(n, dtype=dtype)
    L.emu_grad_fetch(what, net, layer, out.ctypes.data)
    return out


def fetch_raw(what, net, layer):
    """The padded rows of a store as they lie: [mcap][row width]."""
    L = lib()
    w = _ci(0)
    n = L.emu_grad_fetch_raw(what, net, layer, None, ctypes.byref(w))
    assert n >= 0
    out = np.zeros(n, dtype=F32)
    L.emu_grad_fetch_raw(what, net, layer, out.ctypes.data, None)
    return out.reshape(-1, w.value)


def fetch_all(case, m, chunk, get):
    """Every download of a call in grad_check.grad's form; get(what, net, layer, dtype) -> flat array."""
    res = {"act": [], "delta": [], "part": [], "dw": [], "db": []}
    nch = (m + chunk - 1) // chunk
    for n, (layers, _) in enumerate(case.p.nets):
        widths = [case.p.in_dim] + [w.shape[0] for w, _ in layers]
        res["act"].append([get(P.GRAD_ACT, n, l, F32).reshape(m, widths[l]) for l in range(len(widths))])
        res["delta"].append([get(P.GRAD_DELTA, n, l, F32).reshape(m, widths[l + 1]) for l in range(len(layers))])
        res["part"].append([get(P.GRAD_PARTIAL, n, l, F64).reshape(nch, widths[l + 1], widths[l] + 1) for l in range(len(layers))])
        res["dw"].append([get(P.GRAD_DW, n, l, F32).reshape(widths[l + 1], widths[l]) for l in range(len(layers))])
        res["db"].append([get(P.GRAD_DB, n, l, F32) for l in range(len(layers))])
    res["dls"] = get(P.GRAD_DLS, 0, 0, F32)
    res["stats"] = get(NSTATS, 0, 0, F64)
    return res
