"""The gradient rows' definition (include/cassie_phys.h, GRADIENT ROWS) restated in numpy -- test infrastructure only.  Every fma chain is a
loop over k / u / p on float64 arrays, acc = acc + a * b: the product of two float32 values is exact in a double, so the device's fma is
this one rounding.  The forward pass is policy_check's, `reduce` is rollout_check's."""
import numpy as np

import policy_check as pc
import rollout_check as roc
from cassie_amd import phys as P
from obs_check import same_bits  # noqa: F401  (for the tests)

F32, F64 = np.float32, np.float64
H = pc.H


def D(kind, g, h):
    """D(act, g, h) on float64 arrays: the activation's derivative in terms of its output, times g."""
    g, h = np.asarray(g, dtype=F64), np.asarray(h, dtype=F64)
    with np.errstate(all="ignore"):
        if kind == P.POL_IDENTITY:
            return g
        if kind == P.POL_RELU:
            return np.where(h > 0, g, F64(0.0))
        if kind == P.POL_TANH:
            return g * (F64(1.0) - h * h)
        if kind == P.POL_ELU:
            return np.where(h > 0, g, g * (h + F64(1.0)))
    raise ValueError(kind)


def chain(acc, a, b, prod32=False):
    """One step of an fma chain on float64 arrays (prod32: the WRONG reading, the product rounded to float32 first)."""
    with np.errstate(all="ignore"):
        prod = a * b
        return acc + (prod.astype(F32).astype(F64) if prod32 else prod)


def pack_t(w):
    """A layer's transposed packing: per block of 16 k and u-step of 4 the 64 words W[4 ustep + (l >> 4)][16 block + (l & 15)] in lane
    order, zero-padded to out rounded up to 4 and `in` rounded up to 16."""
    w = np.asarray(w, dtype=F32)
    out, kin = w.shape
    u4, in16 = (out + 3) & ~3, (kin + 15) & ~15
    wp = np.zeros((u4, in16), dtype=F32)
    wp[:out, :kin] = w
    return wp.reshape(u4 // 4, 4, in16 // 16, 16).transpose(2, 0, 1, 3).reshape(-1)


def tree_sum(parts):
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def grad(nets, stores, idx, chunk, eps, c_v, c_ent, norm=None, log_std=None, p_desc=False, chunk_tree=False, u_desc=False, prod32=False):
    """nets [(layers [(W, b)], acts)]; stores: {"obs" float32 [S][in], "action" [S][A], "logp" [S], "advn" [S], "ret" [S]} over the S = T nenv
    samples; idx int32 [M].  p_desc, chunk_tree, u_desc, prod32: the WRONG readings the negative controls need (positions from the top of
    a chunk; the chunks summed by a tree; u from the top; products rounded to float32).
    -> {"act": [net][l = 0 .. L] float32 [M][width], "delta": [net][l] float32 [M][out], "part": [net][l] float64 [chunks][out][in + 1],
        "dw", "db": [net][l] float32, "dls" float32 [A], "stats" float64 [8], and the head's doubles "ratio", "adv", "lr", "s1", "s2", "z"}"""
    idx = np.asarray(idx, dtype=np.int32)
    M, S = len(idx), len(stores["logp"])
    mcap = (M + chunk - 1) // chunk * chunk
    full = np.full(mcap, -1, dtype=np.int64)
    full[:M] = idx
    live = (full >= 0) & (full < S)
    s = np.where(live, full, 0)
    lv = live[:, None]
    inv_m = F64(1.0) / F64(M)
    lo, hi, eps = F64(1.0) - F64(eps), F64(1.0) + F64(eps), F64(eps)
    res = {"act": [], "delta": [], "part": [], "dw": [], "db": [], "z": []}
    with np.errstate(all="ignore"):
        x = np.where(lv, np.asarray(stores["obs"], dtype=F32).reshape(S, -1)[s], F32(0.0))
        h0 = x if norm is None else np.where(lv, pc.normalise(x, *norm), F32(0.0)).astype(F32)
        ls = np.asarray(log_std, dtype=F32).astype(F64)
        for n, (layers, acts) in enumerate(nets):
            L = len(layers)
            kept, h = [h0], h0
            for (w, b), a in zip(layers, acts):
                h = pc.layer(h, w, b, a)
                kept.append(np.where(lv, h, F32(0.0)).astype(F32))
            out = h.astype(F64)
            if n == 0:
                A = out.shape[1]
                isd = pc.expn(ls)
                a = np.where(lv, np.asarray(stores["action"], dtype=F32).reshape(S, -1)[s], F32(0.0)).astype(F64)
                q, Lsum = np.zeros(mcap, dtype=F64), F64(0.0)
                d = np.zeros((mcap, A), dtype=F64)
                for j in range(A):
                    d[:, j] = (a[:, j] - out[:, j]) * isd[j]
                    q = q + d[:, j] * d[:, j]
                    Lsum = Lsum + ls[j]
                logp = (F64(-0.5) * q - Lsum) - F64(A) * H
                lr = logp - np.where(live, np.asarray(stores["logp"], dtype=F32)[s], F32(0.0)).astype(F64)
                ratio = pc.expn(-lr)
                adv = np.where(live, np.asarray(stores["advn"], dtype=F32)[s], F32(0.0)).astype(F64)
                s1 = ratio * adv
                rc = np.where(ratio < lo, lo, np.where(ratio > hi, hi, ratio))
                s2 = rc * adv
                active = ~(s2 < s1)
                g = np.where(active, -s1, F64(0.0))
                gtop = np.zeros((mcap, A), dtype=F32)
                gls = np.zeros((mcap, A), dtype=F64)
                for j in range(A):
                    gtop[:, j] = (g * (d[:, j] * isd[j])).astype(F32)
                    gls[:, j] = np.where(live, g * (d[:, j] * d[:, j] - F64(1.0)), F64(0.0))
                r1 = ratio - F64(1.0)
                ploss = np.where(live, -np.where(active, s1, s2), F64(0.0))
                kl = np.where(live, r1 - lr, F64(0.0))
                clipped = np.where(live & (np.abs(r1) > eps), F64(1.0), F64(0.0))
                res.update(ratio=ratio[:M], adv=adv[:M], lr=lr[:M], s1=s1[:M], s2=s2[:M])
            else:
                dv = out[:, 0] - np.where(live, np.asarray(stores["ret"], dtype=F32)[s], F32(0.0)).astype(F64)
                gtop = (F64(c_v) * dv).astype(F32)[:, None]
                vloss = np.where(live, (F64(0.5) * dv) * dv, F64(0.0))
            deltas = [None] * L
            deltas[L - 1] = np.where(lv, D(acts[L - 1], gtop.astype(F64), out).astype(F32), F32(0.0)).astype(F32)
            for l in range(L - 1, 0, -1):
                w = np.asarray(layers[l][0], dtype=F32).astype(F64)
                dl = deltas[l].astype(F64)
                acc = np.zeros((mcap, w.shape[1]), dtype=F64)
                for u in (range(w.shape[0] - 1, -1, -1) if u_desc else range(w.shape[0])):
                    acc = chain(acc, dl[:, u, None], w[None, u, :], prod32)
                deltas[l - 1] = np.where(lv, D(acts[l - 1], acc, kept[l].astype(F64)).astype(F32), F32(0.0)).astype(F32)
            parts, dws, dbs = [], [], []
            for l in range(L):
                hb = np.concatenate([kept[l].astype(F64), np.ones((mcap, 1), dtype=F64)], axis=1)
                dl = deltas[l].astype(F64)
                P_ = np.zeros((mcap // chunk, dl.shape[1], hb.shape[1]), dtype=F64)
                for c in range(mcap // chunk):
                    acc = np.zeros(P_.shape[1:], dtype=F64)
                    ps = range(c * chunk, (c + 1) * chunk)
                    for p in (reversed(ps) if p_desc else ps):
                        acc = chain(acc, dl[p, :, None], hb[p, None, :], prod32)
                    P_[c] = acc
                if chunk_tree:
                    tot = tree_sum([P_[c] for c in range(len(P_))])
                else:
                    tot = np.zeros(P_.shape[1:], dtype=F64)
                    for c in range(len(P_)):
                        tot = tot + P_[c]
                gw = (tot * inv_m).astype(F32)
                parts.append(P_)
                dws.append(np.ascontiguousarray(gw[:, :-1]))
                dbs.append(np.ascontiguousarray(gw[:, -1]))
            res["act"].append([k[:M] for k in kept])
            res["delta"].append([dl[:M] for dl in deltas])
            res["part"].append(parts)
            res["dw"].append(dws)
            res["db"].append(dbs)
            res["z"].append(out[:M])
        A = len(ls)
        res["dls"] = np.array([roc.reduce(gls[:M, j]) * inv_m - F64(c_ent) for j in range(A)], dtype=F64).astype(F32)
        ent = Lsum + F64(A) * (F64(0.5) + H)
        void = np.where(live[:M], F64(0.0), F64(1.0))
        res["stats"] = np.array([roc.reduce(ploss[:M]) * inv_m, roc.reduce(vloss[:M]) * inv_m if len(nets) > 1 else 0.0, roc.reduce(kl[:M]) * inv_m,
                                 roc.reduce(clipped[:M]) * inv_m, ent, roc.reduce(void), F64(M), 0.0], dtype=F64)
    return res


def words(res):
    """Every word of a result as one uint64 array (float32 words widened), in a fixed order."""
    out = []
    for n in range(len(res["dw"])):
        for key in ("act", "delta", "dw", "db"):
            out += [np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32).astype(np.uint64) for a in res[key][n]]
        out += [np.ascontiguousarray(a, dtype=F64).reshape(-1).view(np.uint64) for a in res["part"][n]]
    out.append(np.asarray(res["dls"], dtype=F32).view(np.uint32).astype(np.uint64))
    out.append(np.asarray(res["stats"], dtype=F64).view(np.uint64))
    return np.concatenate(out)


def differing(got, want):
    """The names of what differs in a bit (a NaN equal to any NaN); empty: bit for bit the same."""
    bad = []
    for n in range(len(want["dw"])):
        for key in ("act", "delta", "part", "dw", "db"):
            for l, (g, w) in enumerate(zip(got[key][n], want[key][n])):
                if np.shape(g) != np.shape(w) or not same_bits(np.asarray(g), np.asarray(w)):
                    bad.append("%s[%d][%d]" % (key, n, l))
    for key in ("dls", "stats"):
        if not same_bits(np.asarray(got[key]), np.asarray(want[key])):
            bad.append(key)
    return bad
