"""The optimiser rows' definition (include/cassie_phys.h, OPTIMISER ROWS) restated in numpy -- test infrastructure only.  Every step is one
rounded float64 operation on arrays; the NORM's chain adds the exact product g * g of a float32 with itself, which is the fma's one
rounding.  `reduce` is rollout_check's, the packings are policy_check.pack and grad_check.pack_t."""
import numpy as np

import grad_check as gc
import policy_check as pc
import rollout_check as roc
from obs_check import same_bits  # noqa: F401  (for the tests)

F32, F64 = np.float32, np.float64
SEG = 256


def flat(ws, bs, ls):
    """Per slot W [out][in] and b [out], then log_std -> the flat order: r = u (in + 1) + k with the bias at k = in, log_std last."""
    parts = [np.concatenate([np.asarray(w, dtype=F32), np.asarray(b, dtype=F32)[:, None]], axis=1).reshape(-1) for w, b in zip(ws, bs)]
    return np.concatenate(parts + [np.asarray(ls, dtype=F32)])


def unflat(x, shapes, A):
    """The inverse of flat: shapes [(out, in)] -> (ws, bs, ls)."""
    ws, bs, at = [], [], 0
    for out, kin in shapes:
        blk = x[at: at + out * (kin + 1)].reshape(out, kin + 1)
        ws.append(np.ascontiguousarray(blk[:, :kin]))
        bs.append(np.ascontiguousarray(blk[:, kin]))
        at += out * (kin + 1)
    assert at + A == len(x)
    return ws, bs, x[at:].copy()


def partials(g):
    """The NORM's segment partials of the flat float32 gradients: float64 [ceil(Q / 256)]."""
    g = np.asarray(g, dtype=F32)
    nseg = (len(g) + SEG - 1) // SEG
    pad = np.zeros(nseg * SEG, dtype=F64)
    pad[: len(g)] = g.astype(F64)
    pad = pad.reshape(nseg, 4, 64)
    with np.errstate(all="ignore"):
        acc = np.zeros((nseg, 64), dtype=F64)
        for i in range(4):
            acc = acc + pad[:, i, :] * pad[:, i, :]
        return np.array([roc.wave_sum_ref(acc[s]) for s in range(nseg)], dtype=F64)


def sum_squares(g, sequential=False):
    """S of the NORM (sequential: the WRONG reading the negative control needs, one chain over the flat order)."""
    if sequential:
        s = F64(0.0)
        with np.errstate(all="ignore"):
            for x in np.asarray(g, dtype=F32).astype(F64):
                s = s + x * x
        return s
    return roc.reduce(partials(g))


class State:
    """What the batch owns: the moments in the flat order, and the scalars."""

    def __init__(self, Q):
        self.m, self.v = np.zeros(Q, dtype=F32), np.zeros(Q, dtype=F32)
        self.t, self.p1, self.p2, self.skipped = F64(0.0), F64(1.0), F64(1.0), F64(0.0)

    def copy(self):
        c = State(len(self.m))
        c.m, c.v = self.m.copy(), self.v.copy()
        c.t, c.p1, c.p2, c.skipped = self.t, self.p1, self.p2, self.skipped
        return c

    def scalars(self):
        return np.array([self.t, self.p1, self.p2, self.skipped], dtype=F64)


def step(w, g, st, lr, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=np.inf, sequential=False):
    """w, g: the flat float32 parameters and gradients; st: a State, changed in place -> (the new flat parameters, the eight statistics,
    the partials).  A skipped call returns w itself."""
    w, g = np.asarray(w, dtype=F32), np.asarray(g, dtype=F32)
    b1, b2, eps, lr, max_norm = F64(beta1), F64(beta2), F64(eps), F64(lr), F64(max_norm)
    omb1, omb2 = F64(1.0) - b1, F64(1.0) - b2
    with np.errstate(all="ignore"):
        part = partials(g)
        norm = np.sqrt(sum_squares(g, sequential))
        finite = bool(norm < np.inf)
        raw = max_norm / (norm + F64(1e-6))
        scale = raw if raw < 1 else F64(1.0)
        if not finite:
            st.skipped = st.skipped + F64(1.0)
            return w, np.array([norm, scale, 1.0, st.t, st.skipped, lr, st.p1, st.p2], dtype=F64), part
        st.t, st.p1, st.p2 = st.t + F64(1.0), st.p1 * b1, st.p2 * b2
        bc1, sbc2 = F64(1.0) - st.p1, np.sqrt(F64(1.0) - st.p2)
        stp = lr / bc1
        gs = g.astype(F64) * scale
        st.m = (b1 * st.m.astype(F64) + omb1 * gs).astype(F32)
        st.v = (b2 * st.v.astype(F64) + omb2 * (gs * gs)).astype(F32)
        den = np.sqrt(st.v.astype(F64)) / sbc2 + eps
        w1 = (w.astype(F64) - (stp * st.m.astype(F64)) / den).astype(F32)
    return w1, np.array([norm, scale, 0.0, st.t, st.skipped, lr, st.p1, st.p2], dtype=F64), part


def packed(nets_shapes, ws, bs):
    """The policy's packed floats of every layer in slot order (policy_check.pack), and the transposed packings (grad_check.pack_t)."""
    return np.concatenate([pc.pack(w, b) for w, b in zip(ws, bs)]), np.concatenate([gc.pack_t(w) for w in ws])
