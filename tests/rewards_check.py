"""The reward rows (phys_batch_reward, include/cassie_phys.h) restated in numpy -- test infrastructure only.  The definition is the header's:
every step of a term is one individually rounded fp64 operation (numpy's scalar operations are), the sums are sequential from +0.0, expn is
the header's six steps.  Nothing here shares code with the library: the device and the emulator are compared with it bit for bit."""
from fractions import Fraction
from math import factorial

import numpy as np

from cassie_amd import phys as P
from obs_check import rot_inv, same_bits  # noqa: F401  (R(q)^T v is the observation's, by definition; same_bits for the tests)

F64 = np.float64
LOG2E, LN2_HI, LN2_LO = F64(1.44269504088896338700e+00), F64(6.93147180369123816490e-01), F64(1.90821492927058770002e-10)
COEF = [F64(float(Fraction(1, factorial(i)))) for i in range(14)]       # (float of a Fraction rounds correctly: the double nearest 1/i!)
ZERO, ONE = F64(0.0), F64(1.0)


def expn(a):
    """The header's expn(a) ~ exp(-a), on a scalar."""
    a = F64(a)
    if np.isnan(a):
        return a
    if a > 708.0:
        return ZERO
    if a < -708.0:
        return F64(np.inf)
    n = np.rint(a * LOG2E)
    rho = (a - n * LN2_HI) - n * LN2_LO
    x = -rho
    p = COEF[13]
    for i in range(12, -1, -1):
        p = p * x + COEF[i]
    return F64(np.ldexp(p, -int(n)))


def expn_array(a):
    """expn on an array of arguments in [-708, 708], vectorised (the same operations in the same order, elementwise)."""
    a = np.asarray(a, dtype=F64)
    assert np.all(np.abs(a) <= 708.0)
    n = np.rint(a * LOG2E)
    x = -((a - n * LN2_HI) - n * LN2_LO)
    p = np.full(a.shape, COEF[13])
    for i in range(12, -1, -1):
        p = p * x + COEF[i]
    return np.ldexp(p, -n.astype(np.int64))


def term_value(t, fields, env):
    """The fp64 contribution c of term t (a REW_TERM_DTYPE entry) for an env: fields {field id or P.REW_INPUT: array [nenv][dim]}."""
    src = lambda f, k: F64(fields[int(f)][env, int(k)])          # (float32 inputs widen exactly)
    kind, const_t = int(t["kind"]), int(t["tfield"]) == P.REW_CONST
    if kind == P.REW_QUAT:
        q = [src(t["field"], t["index"] + k) for k in range(4)]
        tq = [F64(t["vec"][k]) if const_t else src(t["tfield"], t["tindex"] + k) for k in range(4)]
        d = ((q[0] * tq[0] + q[1] * tq[1]) + q[2] * tq[2]) + q[3] * tq[3]
        s = ONE - d * d
    else:
        if kind == P.REW_ROT_INV:
            q = [src(t["qfield"], t["qindex"] + k) for k in range(4)]
            v = [F64(t["vec"][k]) for k in range(3)] if int(t["field"]) == P.REW_CONST else [src(t["field"], t["index"] + k) for k in range(3)]
            x = [rot_inv(q, v, j) for j in range(3)]
        else:
            x = [src(t["field"], t["index"] + j) for j in range(int(t["count"]))]
        dead, norm = F64(t["dead"]), int(t["norm"])
        s = ZERO
        for j, xj in enumerate(x):
            e = xj - (F64(t["target"]) if const_t else src(t["tfield"], t["tindex"] + j))
            if dead > 0:
                m = np.abs(e) - dead
                e = ZERO if m < 0 else m
            if norm == P.REW_SUMSQ:
                s = s + e * e
            elif norm == P.REW_SUMABS:
                s = s + np.abs(e)
            elif np.abs(e) > s:
                s = np.abs(e)
        if int(t["root"]) != 0:
            s = np.sqrt(s)
    shape, k = int(t["shape"]), F64(t["k"])
    v = s if shape == P.REW_LINEAR else expn(k * s) if shape == P.REW_EXP else ONE / (ONE + k * s)
    c = F64(t["weight"]) * v
    if int(t["gfield"]) != P.REW_NONE:
        c = c * src(t["gfield"], t["gindex"])
    return c


class Rewards:
    """The rewards [nenv], the term rows [nenv][nterms], the returns and final returns [nenv] of a configuration, advanced as
    phys_batch_reward advances them."""

    def __init__(self, terms, nenv, dtype=np.float32, lo=-np.inf, hi=np.inf):
        self.terms, self.lo, self.hi = P.rew_terms(terms), F64(lo), F64(hi)
        self.rew = np.zeros(nenv, dtype=dtype)
        self.rows = np.zeros((nenv, len(self.terms)), dtype=dtype)
        self.ret, self.final = np.zeros(nenv), np.zeros(nenv)

    def reward(self, fields, env0=0, n=None, reset=None):
        n = len(self.rew) - env0 if n is None else n
        with np.errstate(all="ignore"):
            for i in range(n):
                env = env0 + i
                r = ZERO
                for k, t in enumerate(self.terms):
                    c = term_value(t, fields, env)
                    self.rows[env, k] = c                  # (round to nearest even)
                    r = r + c
                r = self.lo if r < self.lo else (self.hi if r > self.hi else r)
                self.rew[env] = r
                if reset is not None and reset[i] != 0:
                    self.final[env], self.ret[env] = self.ret[env], 0.0
                self.ret[env] = self.ret[env] + r
        return self.rew
