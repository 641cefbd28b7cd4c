"""The task rows (phys_batch_task, include/cassie_phys.h) restated in numpy and Python integers -- test infrastructure only.  The
definition is the header's: per env the SAMPLE columns (a schedule from Philox4x32-10 on (env_base + env, group, epoch, 2), a value from
(env_base + env, column, epoch, 3)), the PHASE clocks, the WAVE forms -- sin2pi / cos2pi written out step by step -- and the TABLE columns;
every arithmetic step one individually rounded fp64 operation (numpy's scalar operations are).  Nothing here shares code with the library
but the Philox restatement of tests/obs_check.py: the device and the emulator are compared with it bit for bit."""
import math
from fractions import Fraction

import numpy as np

from cassie_amd import phys as P
from obs_check import MASK, philox4x32_10, uniform

F64 = np.float64
INT_KEYS = ("kind", "form", "group", "rate_col", "phase_col", "src", "tcol", "dfield", "dindex", "period_lo", "period_hi", "hold")
TWO_PI = F64(6.283185307179586)
INV_FACT = {k: F64(float(Fraction(1, math.factorial(k)))) for k in range(2, 21)}      # the doubles nearest 1 / k!
SIN_COEF = [(-1.0 if (k // 2) % 2 else 1.0) * INV_FACT[k] for k in range(19, 1, -2)]  # -1/19!, 1/17!, ..., -1/3!
COS_COEF = [(-1.0 if (k // 2) % 2 else 1.0) * INV_FACT[k] for k in range(20, 0, -2)]  # 1/20!, -1/18!, ..., -1/2!


def wrap(p):
    p = F64(p)
    f = p - np.floor(p)
    return F64(0.0) if f >= 1.0 else f


def sincos2pi(theta):
    """(sin2pi, cos2pi) of theta in [0, 1), by the header's steps."""
    theta = F64(theta)
    if theta != theta:
        return theta, theta
    q = np.rint(F64(4.0) * theta)
    r = theta - F64(0.25) * q
    x = r * TWO_PI
    z = x * x
    p = SIN_COEF[0]
    for k in SIN_COEF[1:]:
        p = k + z * p
    S = x + (x * z) * p
    c = COS_COEF[0]
    for k in COS_COEF[1:]:
        c = k + z * c
    C = F64(1.0) + z * c
    return ((S, C), (C, -S), (-S, -C), (-C, S))[int(q) & 3]


def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def schedule_words(seed, env_base, env, group, epoch):
    return philox4x32_10(((env_base + env) & MASK, group, int(epoch) & MASK, 2), (seed & MASK, (seed >> 32) & MASK))


def value_word(seed, env_base, env, column, epoch):
    return philox4x32_10(((env_base + env) & MASK, column, int(epoch) & MASK, 3), (seed & MASK, (seed >> 32) & MASK))[0]


def period(word, lo, hi):
    """L of a draw: the integer formula."""
    return lo + ((int(word) * (hi - lo + 1)) >> 32)


def threshold(p_rest):
    return int(round(float(p_rest) * 2.0 ** 32))      # (p 2^32 is exact; halves go to even, as llrint's)


class Task:
    """The rows [nenv][ncols], the state [nenv][ncols] (x or phi), the words [nenv][3][ncols] (left | age | epoch) and the counts
    [nenv] of a configuration, advanced as phys_batch_task advances them.  drew / resting [nenv][ncols]: what the last call did."""

    def __init__(self, cols, nenv, dtype=np.float32, seed=0, env_base=0, table=None):
        self.cols = [{k: (int(c[k]) if k in INT_KEYS else F64(c[k])) for k in P.TASK_COL_DTYPE.names} for c in P.task_cols(cols)]
        for k, col in enumerate(self.cols):
            if col["kind"] == P.TASK_SAMPLE and col["group"] < 0:
                col["group"] = k
        self.ncols, self.seed, self.env_base = len(self.cols), int(seed), int(env_base)
        self.table = None if table is None else np.asarray(table, dtype=np.float64)
        self.rows = np.zeros((nenv, self.ncols), dtype=dtype)
        self.state = np.zeros((nenv, self.ncols), dtype=np.float64)
        self.words = np.zeros((nenv, 3, self.ncols), dtype=np.uint32)
        self.counts = np.zeros(nenv, dtype=np.uint32)
        self.drew = np.zeros((nenv, self.ncols), dtype=bool)
        self.resting = np.zeros((nenv, self.ncols), dtype=bool)
        self.wrapped = np.zeros((nenv, self.ncols), dtype=bool)

    def task(self, fields, env0=0, n=None, reset=None):
        """fields {field id: array [nenv][dim]}: the destination elements are written in place."""
        n = len(self.counts) - env0 if n is None else n
        with np.errstate(all="ignore"):
            for i in range(n):
                env = env0 + i
                count = int(self.counts[env])
                fresh = count == 0 or (reset is not None and reset[i] != 0)
                st, wd = self.state[env], self.words[env]
                out = [F64(0.0)] * self.ncols
                self.drew[env] = False
                self.wrapped[env] = False
                for c, col in enumerate(self.cols):
                    if col["kind"] != P.TASK_SAMPLE:
                        continue
                    x, left, age, epoch = F64(st[c]), int(wd[0, c]), int(wd[1, c]), int(wd[2, c])
                    if fresh or left == 0:
                        epoch = 0 if count == 0 else (epoch + 1) & MASK
                        s = schedule_words(self.seed, self.env_base, env, col["group"], epoch)
                        left = period(s[0], col["period_lo"], col["period_hi"])
                        rest = s[1] < threshold(col["p_rest"])
                        x = col["rest"] if rest else col["center"] + col["half"] * uniform(value_word(self.seed, self.env_base, env, c, epoch))
                        age = 0
                        self.drew[env, c], self.resting[env, c] = True, rest
                    out[c] = x if (col["hold"] == 0 or age < col["hold"]) else col["rest"]
                    st[c] = x
                    wd[:, c] = ((left - 1) & MASK, (age + 1) & MASK, epoch)
                for c, col in enumerate(self.cols):
                    if col["kind"] != P.TASK_PHASE:
                        continue
                    if fresh:
                        phi = wrap(col["phase0"] if col["phase_col"] < 0 else out[col["phase_col"]])
                    else:
                        inc = col["rate"] if col["rate_col"] < 0 else col["rate"] + col["rate_scale"] * out[col["rate_col"]]
                        raw = F64(st[c]) + inc
                        phi = wrap(raw)
                        self.wrapped[env, c] = bool(raw >= 1.0 or raw < 0.0)
                    st[c] = out[c] = phi
                for c, col in enumerate(self.cols):
                    if col["kind"] not in (P.TASK_WAVE, P.TASK_TABLE):
                        continue
                    theta = wrap(out[col["src"]] + col["shift"])
                    if col["kind"] == P.TASK_TABLE:
                        T, nf = self.table, self.table.shape[0]
                        s = theta * F64(nf)
                        a = int(np.floor(s)) if s >= 0 else 0
                        a = min(a, nf - 1)
                        fr = s - F64(a)
                        b = 0 if a + 1 == nf else a + 1
                        ta, tb = F64(T[a, col["tcol"]]), F64(T[b, col["tcol"]])
                        g = ta + fr * (tb - ta)
                    elif col["form"] == P.TASK_SAW:
                        g = theta
                    elif col["form"] == P.TASK_TRAPEZOID:
                        g = clamp(theta / col["ramp"], F64(0.0), F64(1.0)) - clamp((theta - col["duty"]) / col["ramp"], F64(0.0), F64(1.0))
                    else:
                        g = sincos2pi(theta)[0 if col["form"] == P.TASK_SIN else 1]
                    out[c] = col["offset"] + col["scale"] * g
                for c, col in enumerate(self.cols):
                    if col["dfield"] != P.TASK_NONE:
                        fields[col["dfield"]][env, col["dindex"]] = out[c]
                self.rows[env] = np.array(out, dtype=np.float64).astype(self.rows.dtype)     # (round to nearest even)
                self.counts[env] = (count + 1) & MASK
        return self.rows
