"""The normaliser rows' definition (include/cassie_phys.h, NORMALISER ROWS) restated in numpy -- test infrastructure only.  Every step is
one rounded float64 operation on arrays over the columns (numpy contracts nothing into an fma); the blocks are walked by loops, a block's
samples one after the other, and a value that is not finite is left out by a select."""
import numpy as np

from obs_check import same_bits  # noqa: F401  (for the tests)

F32, F64 = np.float32, np.float64


class State:
    """What the batch owns per column: n, mean, m2 and the two counts, float64 [D], +0.0 at configuration."""
    NAMES = ("n", "mean", "m2", "skipped", "excluded")

    def __init__(self, D):
        for k in self.NAMES:
            setattr(self, k, np.zeros(D, dtype=F64))

    def copy(self):
        c = State(len(self.n))
        for k in self.NAMES:
            setattr(c, k, getattr(self, k).copy())
        return c

    def arrays(self):
        return [getattr(self, k) for k in self.NAMES]


def chain(x, sel=None):
    """Rows of x [K][D] added in order from +0.0; sel [K][D]: a row's element is added only where it is set."""
    acc = np.zeros(x.shape[1], dtype=F64)
    for k in range(x.shape[0]):
        acc = acc + x[k] if sel is None else np.where(sel[k], acc + x[k], acc)
    return acc


def outputs(n, m2, eps):
    """inv of the columns (those with n = 0 hold rubbish: the caller selects)."""
    return (F64(1.0) / np.sqrt(m2 / n + F64(eps))).astype(F32)


def update(x, st, block, eps, mean, inv):
    """x: the samples, float32 [R][D]; st: a State, changed in place; mean, inv: the float32 [D] outputs, changed in place where a column
    is updated -> {"mb", "counts", "a1", "a2"}."""
    x = np.asarray(x, dtype=F32)
    R, D = x.shape
    xd = x.astype(F64)
    fin = np.abs(xd) < np.inf                                   # (false for a NaN)
    blocks = [(s, min(R, s + block)) for s in range(0, R, block)]
    with np.errstate(all="ignore"):
        a1 = np.array([chain(xd[s:e], fin[s:e]) for s, e in blocks], dtype=F64)
        M = np.array([fin[s:e].sum(axis=0) for s, e in blocks], dtype=np.int64).sum(axis=0)
        Md = M.astype(F64)
        upd = M > 0
        mb = np.where(upd, chain(a1) / Md, F64(0.0))
        d = xd - mb[None, :]
        a2 = np.array([chain(d[s:e] * d[s:e], fin[s:e]) for s, e in blocks], dtype=F64)
        S2 = chain(a2)
        nn = st.n + Md
        delta = mb - st.mean
        w = Md / nn
        mean1 = st.mean + delta * w
        m21 = (st.m2 + S2) + (delta * delta) * (st.n * w)
        st.skipped = np.where(upd, st.skipped, st.skipped + F64(1.0))
        st.excluded = np.where(upd, st.excluded + (F64(R) - Md), st.excluded)
        st.n, st.mean, st.m2 = np.where(upd, nn, st.n), np.where(upd, mean1, st.mean), np.where(upd, m21, st.m2)
        mean[upd] = mean1.astype(F32)[upd]
        inv[upd] = outputs(nn, m21, eps)[upd]
    return {"mb": mb, "counts": Md, "a1": a1, "a2": a2}


def write(st, eps, mean, inv):
    """mean and inv of every column with n > 0 from the state."""
    has = st.n > 0
    with np.errstate(all="ignore"):
        mean[has] = st.mean.astype(F32)[has]
        inv[has] = outputs(st.n, st.m2, eps)[has]


def stats(st, last, R, block, calls):
    """The eight statistics after a call that returned `last`."""
    upd = last["counts"] > 0
    return np.array([R, (R + block - 1) // block, upd.sum(), (~upd).sum(), (R - last["counts"][upd]).sum(), calls, st.n.max(), 0.0], dtype=F64)
