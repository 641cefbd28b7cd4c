"""The rollout cases the CPU tests (tests/test_rollout.py: the wave emulator) and the GPU tests (tests/test_rollout_gpu.py: the device)
share, each against the restatement (tests/rollout_check.py) -- test infrastructure only."""
import numpy as np

import rollout_check as rc
from cassie_amd import phys as P

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32
SENT = U32(0xDEADBEEF)                 # the sentinel of every word no call may touch (as a float32: -6.26e18, no NaN)
NENV, T = 130, 5                       # two full blocks of 64 envs and a tail of 2
RANGES = ((0, 37), (37, 93))           # (env0, n): the two ranges a batch is cut into
ORDER = (3, 0, 4, 1, 2)                # the slots are recorded out of order
GAMMA, LAMBDA, TMASK, EPS = 0.99, 0.95, 0x4, 1e-8


def aligned_words(count, fill=SENT, align=64):
    """count uint32 words that begin on an `align`-byte boundary, filled."""
    raw = np.empty(count + align // 4, dtype=U32)
    off = (-raw.ctypes.data % align) // 4
    a = raw[off: off + count]
    a[:] = fill
    assert a.ctypes.data % align == 0
    return a


class Store:
    """[T][nenv][dim] words with `row` words between two envs and `step` between two steps, SENT everywhere."""

    def __init__(self, steps, nenv, dim, row, step, fill=SENT):
        assert row >= dim and step >= (nenv - 1) * row + dim
        self.T, self.nenv, self.dim, self.row, self.step = steps, nenv, dim, row, step
        self.buf = aligned_words(steps * step, fill)

    def view(self, buf=None):
        """The rows proper, [T][nenv][dim] (of another buffer of the same layout: of that one)."""
        return np.lib.stride_tricks.as_strided(self.buf if buf is None else buf, (self.T, self.nenv, self.dim), (4 * self.step, 4 * self.row, 4))

    def expected(self, dense, written):
        """The buffer after calls that wrote dense[written]: SENT everywhere else.  dense [T][nenv][dim] words, written bool [T][nenv]."""
        want = np.full(self.buf.shape, SENT, dtype=U32)
        v = self.view(want)
        v[written] = np.asarray(dense).view(U32).reshape(self.T, self.nenv, self.dim)[written]
        return want


class Case:
    """A rollout: the sources (role, dim, row stride of the caller's tensor, row and extra step words of the store), the tensors of every
    step, the value behind the last step.  Every source is bound; tests of the resolution replace pointers as they need."""
    # (role, dim, source row stride, store row stride, extra words of a store's step)
    SOURCES = ((P.RO_VALUE, 1, 2, 1, 5), (P.RO_REWARD, 1, 1, 2, 0), (P.RO_DONE, 1, 1, 1, 1), (P.RO_REASON, 1, 3, 1, 0),
               (P.RO_ACTION, 3, 3, 5, 3), (P.RO_OBS, 68, 72, 72, 8), (P.RO_DATA, 70, 73, 71, 2), (P.RO_LOGP, 1, 1, 1, 0))
    VEC = (0, 0, 0, 0, 0, 1, 0, 0)     # the 16-byte path: pointers, dim and both row strides multiples of 4 words

    def __init__(self, seed=5, nenv=NENV, steps=T, p_done=0.2):
        rng = np.random.default_rng(seed)
        self.nenv, self.T = nenv, steps
        self.gamma, self.lam, self.tmask = GAMMA, LAMBDA, TMASK
        self.srcs = [(role, dim) for role, dim, _, _, _ in self.SOURCES]
        self.dims = [dim for _, dim, _, _, _ in self.SOURCES]
        self.src_stride = [st for _, _, st, _, _ in self.SOURCES]
        # the dense truth: per source [T][nenv][dim]
        self.dense = []
        for role, dim, _, _, _ in self.SOURCES:
            if role == P.RO_DONE:
                a = (rng.random((steps, nenv, 1)) < p_done).astype(I32)
                self.done = a[:, :, 0]
            elif role == P.RO_REASON:
                a = (self.done * rng.choice(np.array([4, 1, 5, 4], dtype=I32), size=(steps, nenv)))[:, :, None].astype(I32)   # a time limit alone, another rule, both
            elif role == P.RO_DATA:
                a = rng.integers(0, 2 ** 32, (steps, nenv, dim), dtype=np.uint64).astype(U32)
            else:
                a = (rng.normal(size=(steps, nenv, dim)) * 2.0 ** rng.integers(-3, 4, (steps, nenv, dim))).astype(F32)
            self.dense.append(np.ascontiguousarray(a))
        self.last = np.full((nenv, 2), F32(-7.25), dtype=F32)
        self.last[:, 0] = rng.normal(size=nenv).astype(F32)
        # the caller's tensors of a step: rows with a stride, SENT between them
        self.steps = []
        for t in range(steps):
            per = []
            for s, (_, dim, st, _, _) in enumerate(self.SOURCES):
                a = aligned_words(nenv * st).reshape(nenv, st)
                a[:, :dim] = self.dense[s][t].view(U32)
                per.append(a)
            self.steps.append(per)

    def role(self, role):
        return [r for r, _ in self.srcs].index(role)

    def stores(self):
        """Fresh padded stores of every source, and of ADV, RET, ADVN."""
        n = self.nenv
        st = [Store(self.T, n, dim, row, n * row + extra) for _, dim, _, row, extra in self.SOURCES]
        arr = {"adv": Store(self.T, n, 1, 2, 2 * n + 3), "ret": Store(self.T, n, 1, 1, n + 1), "advn": Store(self.T, n, 1, 3, 3 * n)}
        return st, arr

    def written(self, calls):
        """calls [(t, env0, n)] -> bool [T][nenv]."""
        w = np.zeros((self.T, self.nenv), dtype=bool)
        for t, env0, n in calls:
            w[t, env0: env0 + n] = True
        return w

    def gae(self, **kw):
        """(adv, ret, q1) of the whole batch by the restatement."""
        f = lambda role: self.dense[self.role(role)][:, :, 0]
        return rc.gae(f(P.RO_VALUE), f(P.RO_REWARD), f(P.RO_DONE), f(P.RO_REASON), self.last[:, 0], self.gamma, self.lam, self.tmask, **kw)

    def normalised(self, eps=EPS):
        adv, _, q1 = self.gae()
        return rc.normalise(adv, q1, eps)
