"""The rollout rows' definition (include/cassie_phys.h, ROLLOUT ROWS) restated in numpy -- test infrastructure only.  A step of the GAE is
a handful of elementwise operations on float64 arrays over the envs, each one rounding; `reduce` stands on the wave's documented tree
(tests/test_wave_primitives.py: wave_sum_ref)."""
import numpy as np

from obs_check import same_bits  # noqa: F401  (for the tests)
from test_wave_primitives import wave_sum_ref

F32, F64 = np.float32, np.float64


def record(store, t, src, env0=0, n=None):
    """store[t][env][:dim] = src[env][:dim] for the envs of the range, as words; store [T][nenv][>= dim], src [nenv][>= dim] (padded
    rows are views of wider arrays).  In place."""
    n = src.shape[0] - env0 if n is None else n
    dim = min(store.shape[2], src.shape[1])
    store.view(np.uint32)[t, env0:env0 + n, :dim] = src.view(np.uint32)[env0:env0 + n, :dim]


def gae(val, rew, done, reason, last, gamma, lam, tmask=0, products=False):
    """val, rew float32 [T][n]; done, reason int32 [T][n] or None; last float32 [n] -> (adv float32 [T][n], ret float32 [T][n], q1
    float64 [n]).  products: the textbook form, (1 - done) as a factor -- the reading the selects exist to avoid."""
    val, rew = np.asarray(val, dtype=F32), np.asarray(rew, dtype=F32)
    T, n = val.shape
    g, gl = F64(gamma), F64(gamma) * F64(lam)
    adv, ret = np.zeros((T, n), dtype=F32), np.zeros((T, n), dtype=F32)
    nv, a = np.asarray(last, dtype=F32).astype(F64), np.zeros(n, dtype=F64)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            v, r = val[t].astype(F64), rew[t].astype(F64)
            d = np.zeros(n, dtype=bool) if done is None else np.asarray(done[t]) != 0
            if tmask and done is not None and reason is not None:
                q = np.asarray(reason[t]).astype(np.int64) & 0xffffffff
                cut = d & ((q & tmask) != 0) & ((q & ~tmask & 0xffffffff) == 0)
                r = np.where(cut, r + g * v, r)
            if products:
                live = F64(1.0) - d.astype(F64)
                delta = (r + g * nv * live) - v
                a = delta + gl * live * a
            else:
                nvs, as_ = np.where(d, F64(0.0), nv), np.where(d, F64(0.0), a)
                delta = (r + g * nvs) - v
                a = delta + gl * as_
            adv[t], ret[t] = a.astype(F32), (a + v).astype(F32)
            nv = v
        q1 = np.zeros(n, dtype=F64)
        for t in range(T):
            q1 = q1 + adv[t].astype(F64)
    return adv, ret, q1


def reduce(x):
    """The envs padded with +0.0 to a multiple of 64, every block of 64 summed by the wave's tree, the block sums added in block order
    from +0.0."""
    x = np.asarray(x, dtype=F64)
    pad = np.zeros((len(x) + 63) // 64 * 64, dtype=F64)
    pad[:len(x)] = x
    s = F64(0.0)
    with np.errstate(all="ignore"):
        for b in range(0, len(pad), 64):
            s = s + F64(wave_sum_ref(pad[b:b + 64]))
    return s


def normalise(adv, q1, eps):
    """adv float32 [T][n], q1 float64 [n] -> (advn float32 [T][n], (mean, std, inv), q2)."""
    adv = np.asarray(adv, dtype=F32)
    T, n = adv.shape
    M = T * n
    with np.errstate(all="ignore"):
        mean = reduce(q1) / F64(M)
        q2 = np.zeros(n, dtype=F64)
        for t in range(T):
            c = adv[t].astype(F64) - mean
            q2 = q2 + c * c
        std = np.sqrt(reduce(q2) / F64(M - 1))
        inv = F64(1.0) / (std + F64(eps))
        advn = ((adv.astype(F64) - mean) * inv).astype(F32)
    return advn, (mean, std, inv), q2


def gae_plain(val, rew, done, reason, last, gamma, lam, tmask=0):
    """The definition as a plain Python loop, env by env: Python floats are individually rounded doubles.  -> (adv, ret) float32 [T][n]."""
    T, n = np.asarray(val).shape
    gamma, gl = float(gamma), float(gamma) * float(lam)
    adv, ret = np.zeros((T, n), dtype=F32), np.zeros((T, n), dtype=F32)
    for e in range(n):
        nv, a = float(last[e]), 0.0
        for t in range(T - 1, -1, -1):
            v, r = float(val[t][e]), float(rew[t][e])
            d = done is not None and int(done[t][e]) != 0
            if tmask and d and reason is not None:
                q = int(reason[t][e]) & 0xffffffff
                if (q & tmask) != 0 and (q & ~tmask & 0xffffffff) == 0:
                    r = r + gamma * v
            nvs, as_ = (0.0, 0.0) if d else (nv, a)
            delta = (r + gamma * nvs) - v
            a = delta + gl * as_
            adv[t][e], ret[t][e] = F32(a), F32(a + v)
            nv = v
    return adv, ret
