"""The optimiser cases the CPU tests (tests/test_opt.py: the wave emulator) and the GPU tests (tests/test_opt_gpu.py: the device) share, each
against the restatement (tests/opt_check.py) -- test infrastructure only.  Built on grad_cases: a case's parameters are its policy's, its
gradients those a grad call of the case leaves."""
import functools

import numpy as np

import grad_cases as gcs
import grad_emu_py as ge
import opt_check as oc

F32, F64 = np.float32, np.float64
FILL = gcs.FILL
HYPER = dict(beta1=0.9, beta2=0.999, eps=1e-8)
LRS = (3e-3, 1e-3, 2e-3)
# name -> (the grad case, the three minibatches (m, chunk, seed) whose gradients the three steps take, Q)
CASES = {"shared": (gcs.shared_case, ((130, 16, 3), (37, 16, 4), (17, 32, 5)), 914),
         "four layers": (gcs.four_layer_case, ((38, 16, 3), (20, 16, 4), (16, 16, 5)), 1007),
         "one layer": (gcs.one_layer_case, ((20, 32, 3), (17, 32, 4), (20, 16, 5)), 6),
         "actor only": (gcs.actor_only_case, ((37, 32, 3), (16, 16, 4), (20, 16, 5)), None),
         "limits": (gcs.limits_case, ((16, 16, 3), (16, 16, 4), (16, 16, 5)), 820864)}


def slots(res):
    """A gradient call's result (grad_check.grad's form) -> (dws, dbs, dls) in slot order."""
    return ([g for per in res["dw"] for g in per], [g for per in res["db"] for g in per], res["dls"])


@functools.lru_cache(maxsize=None)
def setup(name):
    """-> (the grad case, the three gradient sets): made once, shared by the tests, never changed."""
    make, runs, _ = CASES[name]
    case = make()
    grads = [slots(ge.Call(case, chunk).grad(case.idx(m, seed=seed))) for m, chunk, seed in runs]
    return case, grads


def norms(grads):
    return [float(np.sqrt(oc.sum_squares(oc.flat(*g)))) for g in grads]


class Ref:
    """A run of the restatement in the snapshot form of opt_emu_py.Opt."""

    def __init__(self, case, max_norm=np.inf, **hyper):
        self.shapes = [w.shape for layers, _ in case.p.nets for w, _ in layers]
        self.A = case.A
        self.w = oc.flat([w for layers, _ in case.p.nets for w, _ in layers], [b for layers, _ in case.p.nets for _, b in layers], case.log_std)
        self.st = oc.State(len(self.w))
        self.hyper = dict(HYPER, max_norm=max_norm, **hyper)
        self.stats, self.part = None, None

    def step(self, grads, lr, **kw):
        self.w, self.stats, self.part = oc.step(self.w, oc.flat(*grads), self.st, lr, **self.hyper, **kw)
        return self.snapshot()

    def params(self):
        return oc.unflat(self.w, self.shapes, self.A)

    def snapshot(self):
        ws, bs, ls = self.params()
        packed, packt = oc.packed(self.shapes, ws, bs)
        return {"w": ws, "b": bs, "ls": ls, "packed": packed, "packt": packt, "m": self.st.m.copy(), "v": self.st.v.copy(), "part": self.part,
                "scalars": self.st.scalars(), "stats": self.stats}


KEYS = ("ls", "packed", "packt", "m", "v", "part", "scalars", "stats")


def differing(got, want, keys=KEYS + ("w", "b")):
    """The names of what differs in a bit (a NaN equal to any NaN); empty: bit for bit the same."""
    bad = []
    for key in keys:
        if key in ("w", "b"):
            bad += ["%s[%d]" % (key, k) for k, (g, w) in enumerate(zip(got[key], want[key])) if np.shape(g) != np.shape(w) or not oc.same_bits(g, w)]
        elif np.shape(got[key]) != np.shape(want[key]) or not oc.same_bits(np.asarray(got[key]), np.asarray(want[key])):
            bad.append(key)
    return bad


def padding_kept(snap, shapes):
    """The caller's row-stride padding of the master tensors still holds FILL."""
    return all(np.all(full[:, kin:] == FILL) for full, (_, kin) in zip(snap["wfull"], shapes))
