"""The observation rows (phys_batch_obs, include/cassie_phys.h) restated in numpy and Python integers -- test infrastructure only.  The
definition is the header's: a column's value is a chain of individually rounded fp64 operations (numpy's scalar operations are), the
noise is Philox4x32-10 on (env_base + env, column, frames[env], 0), the history shifts per env.  Nothing here shares code with the
library: the device and the emulator are compared with it bit for bit."""
import numpy as np

from cassie_amd import phys as P

M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
F64 = np.float64


def philox4x32_10(counter, key):
    """Philox4x32-10 in Python integers: counter (4 words), key (2 words) -> the 4 output words."""
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(w):
    """A word -> xi in (-1, 1): (w + 0.5) 2^-31 - 1, exact in fp64."""
    return (F64(w) + F64(0.5)) * F64(2.0 ** -31) - F64(1.0)


def noise_word(seed, env_base, env, column, frames):
    return philox4x32_10(((env_base + env) & MASK, column, int(frames) & MASK, 0), (seed & MASK, (seed >> 32) & MASK))[0]


def columns(terms):
    """The terms (P.obs_terms takes the same) -> one dict per column of the frame, and every term's first column."""
    cols, first = [], []
    for t in P.obs_terms(terms):
        first.append(len(cols))
        rot = int(t["kind"]) == P.OBS_ROT_INV
        for j in range(3 if rot else int(t["count"])):
            cols.append(dict(rot=rot, comp=j, field=int(t["field"]), elem=int(t["index"]) + (0 if rot else j), qfield=int(t["qfield"]), qelem=int(t["qindex"]),
                             vec=[F64(v) for v in t["vec"]], offset=F64(t["offset"]), scale=F64(t["scale"]), noise=F64(t["noise"]), lo=F64(t["lo"]), hi=F64(t["hi"])))
    return cols, first


def rot_inv(q, v, comp):
    """Component comp of R(q)^T v: quat2mat's matrix and mulmatTvec3's sums, every product and sum rounded on its own."""
    q00, q11, q22, q33 = q[0] * q[0], q[1] * q[1], q[2] * q[2], q[3] * q[3]
    q01, q02, q03 = q[0] * q[1], q[0] * q[2], q[0] * q[3]
    q12, q13, q23 = q[1] * q[2], q[1] * q[3], q[2] * q[3]
    two = F64(2.0)
    m = [((q00 + q11) - q22) - q33, two * (q12 - q03), two * (q13 + q02),
         two * (q12 + q03), ((q00 - q11) + q22) - q33, two * (q23 - q01),
         two * (q13 - q02), two * (q23 + q01), ((q00 - q11) - q22) + q33]
    return (m[comp] * v[0] + m[3 + comp] * v[1]) + m[6 + comp] * v[2]


def value(col, fields, env, column, frames, seed, env_base):
    """The fp64 value of a column of an env's new frame (before the cast): fields {field id or P.OBS_INPUT: array [nenv][dim]}."""
    src = lambda f, k: F64(fields[f][env, k])          # (float32 inputs widen exactly)
    if col["rot"]:
        q = [src(col["qfield"], col["qelem"] + k) for k in range(4)]
        v = col["vec"] if col["field"] == P.OBS_CONST else [src(col["field"], col["elem"] + k) for k in range(3)]
        x = rot_inv(q, v, col["comp"])
    else:
        x = src(col["field"], col["elem"])
    e = x - col["offset"]
    if col["noise"] != 0:
        e = e + col["noise"] * uniform(noise_word(seed, env_base, env, column, frames))
    y = e * col["scale"]
    return col["lo"] if y < col["lo"] else (col["hi"] if y > col["hi"] else y)


class Obs:
    """The rows [nenv][history][ncols] and the frame counts [nenv] of a configuration, advanced as phys_batch_obs advances them."""

    def __init__(self, terms, nenv, history=1, dtype=np.float32, seed=0, env_base=0):
        self.cols, self.first = columns(terms)
        self.ncols, self.history, self.seed, self.env_base = len(self.cols), history, int(seed), int(env_base)
        self.rows = np.zeros((nenv, history, self.ncols), dtype=dtype)
        self.frames = np.zeros(nenv, dtype=np.uint32)

    def observe(self, fields, env0=0, n=None, refill=None):
        n = len(self.frames) - env0 if n is None else n
        with np.errstate(all="ignore"):
            for i in range(n):
                env = env0 + i
                new = np.array([value(c, fields, env, k, self.frames[env], self.seed, self.env_base) for k, c in enumerate(self.cols)], dtype=np.float64)
                new = new.astype(self.rows.dtype)     # (round to nearest even)
                if self.frames[env] == 0 or (refill is not None and refill[i] != 0):
                    self.rows[env, :] = new
                else:
                    self.rows[env, 1:] = self.rows[env, :-1].copy()
                    self.rows[env, 0] = new
                self.frames[env] = (int(self.frames[env]) + 1) & MASK
        return self.rows


def same_bits(a, b):
    """IEEE bits equal, a NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))
