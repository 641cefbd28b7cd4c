"""ctypes access to the policy kernels on the CPU wave emulator (tests/emu/emu_policy.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_policy.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_declared = False
POLICY_GRID = POLICY_TILE = POLICY_WAVES = None    # ck::POLICY_GRID, _TILE, _WAVES, once the library is loaded (lib())
F32 = np.float32


class PolicyArgs(ctypes.Structure):
    _fields_ = [("nets", _vp), ("nnets", _ci), ("in_dim", _ci), ("nenv", _ci),
                ("w", _vp * 8), ("sw", _ll * 8), ("b", _vp * 8),
                ("x", _vp), ("x_dim", _ci), ("sx", _ll), ("x_dtype", _ci),
                ("mean", _vp), ("inv", _vp), ("clip", ctypes.c_double),
                ("out", _vp * 2), ("sout", _ll * 2),
                ("eps", _vp), ("seps", _ll), ("log_std", _vp), ("action", _vp), ("saction", _ll), ("logp", _vp)]


def lib():
    global _declared, POLICY_GRID, POLICY_TILE, POLICY_WAVES
    L = emu_py.lib()
    if not _declared:
        A = ctypes.POINTER(PolicyArgs)
        L.emu_policy_last_refusal.restype = ctypes.c_char_p
        L.emu_policy_constants.argtypes, L.emu_policy_constants.restype = [_vp], None
        L.emu_policy_grid.argtypes = [_ci, _ci]
        L.emu_policy_check.argtypes, L.emu_policy_check.restype = [A, _ci, _ci, _ci, _ci], ctypes.c_char_p
        L.emu_policy_load_check.argtypes, L.emu_policy_load_check.restype = [A, _ci, _ci, _vp, _ll, _vp], ctypes.c_char_p
        L.emu_policy_packed.argtypes, L.emu_policy_packed.restype = [A, _vp, _vp], _ll
        L.emu_policy.argtypes = [A, _ci, _ci, _ci]
        L.emu_policy_lds_bytes.argtypes, L.emu_policy_lds_bytes.restype = [A], _ll
        c = np.zeros(9, dtype=np.int64)
        L.emu_policy_constants(c.ctypes.data)
        assert tuple(int(v) for v in c[3:7]) == (P.POL_MAXNETS, P.POL_MAXLAYERS, P.POL_MAXDIM, P.POL_MAXOUT)
        assert (int(c[7]), int(c[8])) == (P.POL_NET_DTYPE.itemsize, ctypes.sizeof(PolicyArgs))
        POLICY_GRID, POLICY_TILE, POLICY_WAVES = int(c[0]), int(c[1]), int(c[2])
        _declared = True
    return L


def grid(n, nnets=1):
    """ck::policy_grid."""
    return lib().emu_policy_grid(n, nnets)


def _stride(a):
    assert a.dtype == F32 and a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0
    return a.strides[0] // 4


class Call:
    """A policy as the arguments of the emulator's entry points.  defs: per network a list of pol_layer(...) (or (in, out, act) triples,
    passed as written); nenv: the envs of the batch.  Everything bound is the caller's numpy array, written in place."""

    def __init__(self, defs, in_dim, nenv, nnets=None):
        self.keep = []
        self.table = P.pol_nets(defs, in_dim)
        if len(defs) > P.POL_MAXNETS:                       # (more networks than a table holds: the count alone says so)
            self.table = np.zeros(len(defs), dtype=P.POL_NET_DTYPE)
        self.a = PolicyArgs(nets=self.table.ctypes.data if len(defs) else None, nnets=len(defs) if nnets is None else nnets, in_dim=in_dim, nenv=nenv)

    @classmethod
    def of_case(cls, case, res=None, load=True, bind=True):
        """The call of a policy_cases.Case, its tensors bound; res: the output tensors (case.fresh())."""
        c = cls(case.defs, case.in_dim, case.nenv)
        if load:
            for n, layers in enumerate(case.weights):
                for l, (w, b) in enumerate(layers):
                    c.load(n, l, w[:, : w.shape[1] - case.wpad], b)
        if bind:
            c.bind_input(case.x[:, : case.in_dim])
            if case.norm is not None:
                c.bind_norm(*case.norm)
            if res is not None:
                for n, w in enumerate(case.widths):
                    c.bind_output(n, res["out"][n][:, :w])
                if case.eps is not None:
                    c.bind_sample(case.eps[:, : case.widths[0]], case.log_std, res["action"][:, : case.widths[0]], res["logp"])
        return c

    def load(self, net, layer, w, b, stride=None):
        """w: a 2-D float32 view (its row stride is the weight's); b float32 [out]."""
        self.keep += [w, b]
        s = 4 * net + layer
        self.a.w[s], self.a.sw[s], self.a.b[s] = w.ctypes.data, _stride(w) if stride is None else stride, b.ctypes.data

    def bind_input(self, x, dim=None, stride=None, dtype=4):
        self.keep.append(x)
        self.a.x, self.a.x_dim, self.a.x_dtype = x.ctypes.data, x.shape[1] if dim is None else dim, dtype
        self.a.sx = (x.strides[0] // x.itemsize) if stride is None else stride

    def bind_norm(self, mean, inv, clip):
        mean, inv = (None if v is None else np.ascontiguousarray(v, dtype=F32) for v in (mean, inv))
        self.keep += [mean, inv]
        self.a.mean, self.a.inv, self.a.clip = emu_py._ptr(mean), emu_py._ptr(inv), clip

    def bind_output(self, net, out, stride=None):
        self.keep.append(out)
        self.a.out[net], self.a.sout[net] = out.ctypes.data, _stride(out) if stride is None else stride

    def bind_sample(self, eps, log_std, action, logp, eps_stride=None, action_stride=None):
        self.keep += [eps, log_std, action, logp]
        self.a.eps, self.a.seps = eps.ctypes.data, _stride(eps) if eps_stride is None else eps_stride
        self.a.log_std, self.a.logp = emu_py._ptr(log_std), emu_py._ptr(logp)
        self.a.action = emu_py._ptr(action)
        self.a.saction = (0 if action is None else _stride(action)) if action_stride is None else action_stride

    def check(self, call=False, env0=0, n=0, configured=True):
        """policy_configure, the load and bind checks and (call) check_policy_call -> refusal or None."""
        why = lib().emu_policy_check(ctypes.byref(self.a), int(configured), int(call), env0, n)
        return None if why is None else why.decode()

    def load_check(self, net, layer, w, stride, b):
        why = lib().emu_policy_load_check(ctypes.byref(self.a), net, layer, emu_py._ptr(w), stride, emu_py._ptr(b))
        return None if why is None else why.decode()

    def lds_bytes(self):
        """ck::policy_lds_bytes: the LDS a workgroup of the launch takes."""
        return lib().emu_policy_lds_bytes(ctypes.byref(self.a))

    def packed(self):
        """The packed floats the pack kernel makes of the loaded layers, and per (net, layer) slot (w_off, b_off, k4, out16)."""
        offs = np.zeros((8, 4), dtype=np.int64)
        n = lib().emu_policy_packed(ctypes.byref(self.a), None, offs.ctypes.data)
        assert n >= 0, (lib().emu_policy_last_refusal() or b"").decode()
        out = np.zeros(n, dtype=F32)
        lib().emu_policy_packed(ctypes.byref(self.a), out.ctypes.data, None)
        return out, offs

    def policy(self, env0=0, n=None, grid=0):
        """phys_batch_policy on the emulator: the bound outputs and the sample of the range, in place."""
        n = self.a.nenv - env0 if n is None else n
        rc = lib().emu_policy(ctypes.byref(self.a), env0, n, grid)
        assert rc == 0, (lib().emu_policy_last_refusal() or b"").decode()
