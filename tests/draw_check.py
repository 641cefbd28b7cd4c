"""The draw rows (phys_batch_draw, phys_batch_draw_perm; include/cassie_phys.h: DRAW ROWS) restated in numpy and Python integers -- test
infrastructure only.  The definition is the header's: Philox4x32-10 on uint64 arrays (checked against tests/obs_check.py's Python-integer
restatement and the known answer), logn step by step, sincos2pi step by step (tests/task_check.py's coefficients), the Box-Muller pair, the
Feistel walk.  Every arithmetic step is one elementwise float64 operation of numpy's, individually rounded.  Nothing here shares code with
the library: the device and the emulator are compared with it bit for bit."""
import numpy as np

from obs_check import M0, M1, W0, W1, MASK
from task_check import COS_COEF, SIN_COEF, TWO_PI

F64, F32, U64 = np.float64, np.float32, np.uint64
TAG_NORMAL, TAG_PERM, ROUNDS = 4, 5, 6
LN2_HI, LN2_LO = F64(6.93147180369123816490e-01), F64(1.90821492927058770002e-10)
SQRT2 = F64(1.4142135623730951)
LOG_COEF = [F64(1.0) / F64(k) for k in range(23, 1, -2)]       # the doubles nearest 1/23, 1/21, ..., 1/3
TWO_M32 = F64(2.0 ** -32)


def philox(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays (or scalars) of words: the counter's four, the key from the seed -> the four output arrays (uint64 holding words)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(v, dtype=U64) & U64(MASK) for v in (c0, c1, c2, c3)))
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    m = U64(MASK)
    for _ in range(10):
        p0, p1 = U64(M0) * c0, U64(M1) * c2                      # (32 x 32 bits: fits 64)
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ U64(k0), p1 & m, (p0 >> U64(32)) ^ c3 ^ U64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def logn(x):
    """logn of an array of doubles, by the header's steps."""
    x = np.atleast_1d(np.asarray(x, dtype=F64)).copy()
    with np.errstate(all="ignore"):
        nan, neg, zero, inf = x != x, x < 0.0, x == 0.0, x == np.inf
        special = nan | neg | zero | inf
        y = np.where(special, F64(1.0), x)
        tiny = y < F64(2.2250738585072014e-308)
        y = np.where(tiny, y * F64(2.0 ** 54), y)
        bits = y.view(U64)
        e = ((bits >> U64(52)) & U64(0x7FF)).astype(np.int64) - 1023 - np.where(tiny, 54, 0)
        m = ((bits & U64(0x000FFFFFFFFFFFFF)) | U64(0x3FF0000000000000)).view(F64)
        upper = m >= SQRT2
        m = np.where(upper, m * F64(0.5), m)
        e = e + upper
        f = m - F64(1.0)
        s = f / (F64(2.0) + f)
        z = s * s
        p = np.full_like(z, LOG_COEF[0])
        for k in LOG_COEF[1:]:
            p = k + z * p
        t = s + (s * z) * p
        r = F64(2.0) * t
        ed = e.astype(F64)
        out = ed * LN2_HI + (ed * LN2_LO + r)
        out = np.where(inf, np.inf, out)
        out = np.where(zero, -np.inf, out)
        out = np.where(neg, np.nan, out)
        out = np.where(nan, x, out)
    return out


def sincos2pi(theta):
    """(sin2pi, cos2pi) of an array of theta in [0, 1): tests/task_check.py's steps, elementwise."""
    theta = np.asarray(theta, dtype=F64)
    q = np.rint(F64(4.0) * theta)
    r = theta - F64(0.25) * q
    x = r * TWO_PI
    z = x * x
    p = np.full_like(z, SIN_COEF[0])
    for k in SIN_COEF[1:]:
        p = k + z * p
    S = x + (x * z) * p
    c = np.full_like(z, COS_COEF[0])
    for k in COS_COEF[1:]:
        c = k + z * c
    C = F64(1.0) + z * c
    quad = q.astype(np.int64) & 3
    return np.choose(quad, [S, C, -S, -C]), np.choose(quad, [C, -S, -C, S])


def radius(a):
    """u and rad = sqrt(-2 logn(u)) of an array of words a."""
    u = (np.asarray(a, dtype=U64).astype(F64) + F64(0.5)) * TWO_M32
    return u, np.sqrt(F64(-2.0) * logn(u))


def pair(a, b):
    """(rad cos, rad sin) of arrays of words a, b: float64."""
    _, rad = radius(a)
    sn, cs = sincos2pi(np.asarray(b, dtype=U64).astype(F64) * TWO_M32)
    return rad * cs, rad * sn


def normal_rows(seed, env_base, envs, counts, A):
    """The float32 rows [len(envs)][A] of the envs `envs` (batch indices) with the call counts `counts`."""
    envs, counts = np.asarray(envs, dtype=np.int64), np.asarray(counts, dtype=U64)
    nb = (A + 3) // 4
    c0 = ((envs + int(env_base)) & MASK).astype(U64)[:, None]
    w = philox(c0, np.arange(nb, dtype=U64)[None, :], counts[:, None], TAG_NORMAL, seed)
    z = np.empty((len(envs), nb, 4), dtype=F64)
    z[:, :, 0], z[:, :, 1] = pair(w[0], w[1])
    z[:, :, 2], z[:, :, 3] = pair(w[2], w[3])
    return z.reshape(len(envs), 4 * nb)[:, :A].astype(F32)


class Draws:
    """What the batch does: rows [nenv][stride] (sentinel until written), the counts; draw(env0, n) by the definition."""

    def __init__(self, nenv, A, seed=0, env_base=0, stride=None, fill=np.nan):
        self.nenv, self.A, self.seed, self.env_base = nenv, A, seed, env_base
        self.rows = np.full((nenv, A if stride is None else stride), fill, dtype=F32)
        self.counts = np.zeros(nenv, dtype=np.uint32)

    def draw(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        envs = np.arange(env0, env0 + n)
        self.rows[envs, : self.A] = normal_rows(self.seed, self.env_base, envs, self.counts[envs], self.A)
        self.counts[envs] += np.uint32(1)          # (wraps)
        return self.rows


def perm_half(n):
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    return h


def feistel(x, h, epoch, seed):
    """One application of the six rounds to an array of words < 2^(2 h)."""
    mask = U64((1 << h) - 1)
    L, R = x >> U64(h), x & mask
    for r in range(ROUNDS):
        w0 = philox(R, r, int(epoch) & MASK, TAG_PERM, seed)[0]
        L, R = R, L ^ (w0 & mask)
    return (L << U64(h)) | R


def perm(n, epoch, seed, walks=None):
    """perm[0 .. n) keyed by (seed, epoch): int32.  walks: a list that takes the largest number of applications an index needed."""
    h = perm_half(n)
    x = feistel(np.arange(n, dtype=U64), h, epoch, seed)
    most, bound = 1, (1 << (2 * h)) - n + 1
    while True:
        out = np.nonzero(x >= U64(n))[0]
        if out.size == 0:
            break
        assert most < bound, "a walk went past its bound"
        x[out] = feistel(x[out], h, epoch, seed)
        most += 1
    if walks is not None:
        walks.append(most)
    return x.astype(np.int32)
