"""The linear-algebra primitives of csrc/pk_factor_solve.h, one at a time, against exact rational references: the two
L^T D L factorisations in both forms, the triangular solves (through the kernel's own staging of the packed rows) and one
sweep of the guarded and of the speculative projected Gauss-Seidel chain -- on the CPU wave emulator and, with -m gpu, on
the device build of the same bodies (tests/device/wave_bodies.h, product flags).

Every bound is a componentwise rounding-error bound that follows from the number format (u = 2^-53) and the count of
operations, never from what the code returns; the negative controls at the end show that a plain fp64 restatement of each
primitive stays inside its bound and that one dropped term or one missing Newton step leaves it by more than 100 x."""
import ctypes
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from test_wave_primitives import BACKENDS, U, _wave_check, model_pivots, same_bits

RT, CASSIE, TRAY = 0, 1, 2
TREE_MODEL = {CASSIE: "cassie", TRAY: "cassie_tray_box"}
FACTOR_BODY = {RT: "factor_rt", CASSIE: "factor_cassie", TRAY: "factor_tray"}
SOLVE_BODY = {RT: "solve_rt", CASSIE: "solve_cassie", TRAY: "solve_tray"}
MASS_SCALE = (0.2, 5.0)  # per-body log-uniform factors on masses and inertias


@pytest.fixture(params=BACKENDS)
def wc(request):
    return _wave_check(request.param)


def report(wc, what, ratio):
    print("%s on the %s: largest error / bound = %.3g" % (what, wc.backend, ratio))


# ------------------------------------------------------------------------------------------------ trees and models ---
@functools.lru_cache(maxsize=None)
def tree(which):
    """(padded size, nv, ancestor masks, words of a packed factor, slot[k][i]) of an instantiated dof tree."""
    return _wave_check("emu").tree(which)


def descendants(anc, nv):
    return [[k for k in range(nv) if (anc[k] >> i) & 1] for i in range(nv)]


def pattern(anc, nv):
    """[nv][nv] bool: (k, i) with i a proper ancestor of k."""
    return np.array([[bool((anc[k] >> i) & 1) for i in range(nv)] for k in range(nv)])


def copy_pod(pod):
    from cassie_amd._lib import CmModel
    out = CmModel()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(pod), ctypes.sizeof(CmModel))
    return out


@functools.lru_cache(maxsize=None)
def model_matrices(name):
    """(a) of the inputs: the oracle's mass matrix (armature included) of model `name` at 16 random poses, each with the
    model's own inertias and with body masses and inertias scaled per body by log-uniform factors in MASS_SCALE.
    Returns (pod, [32][nv][nv])."""
    from cassie_amd import Model
    from oracle_py import Oracle
    m = Model(name)
    pod = m.pod
    rng = np.random.default_rng(31)
    q0 = m.qpos_init()
    out = []
    for s in range(16):
        q = q0.copy()
        for j in range(pod.njnt):
            if pod.jnt_type[j] in (2, 3):  # slide, hinge
                q[pod.jnt_qposadr[j]] += rng.uniform(-0.4, 0.4)
        scaled = copy_pod(pod)
        f = np.exp(rng.uniform(math.log(MASS_SCALE[0]), math.log(MASS_SCALE[1]), pod.nbody))
        for b in range(pod.nbody):
            scaled.body_mass[b] = pod.body_mass[b] * f[b]
            for i in range(3):
                scaled.body_inertia[b][i] = pod.body_inertia[b][i] * f[b]
        for p in (pod, scaled):
            o = Oracle(p, q)
            o.forward()
            out.append(np.array(o.qM))
    return pod, np.array(out)


def synthetic(rng, anc, nv, lo, hi):
    """(b) of the inputs: A = L^T D L rounded to fp64, L unit lower with random entries on exactly the ancestor pattern,
    D log-uniform in [lo, hi]: tree-sparse by construction."""
    L = np.eye(nv) + pattern(anc, nv) * rng.uniform(-1, 1, (nv, nv))
    D = np.exp(rng.uniform(math.log(lo), math.log(hi), nv))
    return (L.T * D) @ L


@functools.lru_cache(maxsize=None)
def pivot_range():
    """The range test_model_pivots_are_positive_and_normal establishes, widened by 10^3 at both ends."""
    p = model_pivots()
    lo, hi = float(p.min()) * 1e-3, float(p.max()) * 1e3
    assert 2.0 ** -500 < lo < hi < 2.0 ** 500
    return lo, hi


# ------------------------------------------------------------------------------------------- factorisation inputs ---
class FactorCase:
    """One call of a factor body: a model block (nv, masks, armature, damping, h) and trials that share it.  The kernel is handed
    col = colh = the matrix less the armature on its diagonal (as the mass-matrix stage leaves it); the matrices it has to factor
    are, exactly, A = col + diag(arm) and AH = colh + diag(arm + h damping)."""

    def __init__(self, label, pod, anc, nv, nvp, h, mats, mats_h=None):
        self.label, self.pod, self.anc, self.nv, self.nvp, self.h = label, pod, anc, nv, nvp, h
        self.arm = np.array(pod.dof_armature[:nv])
        self.damp = np.array(pod.params.dof_damping[:nv])
        keep = pattern(anc, nv) | np.eye(nv, dtype=bool)
        self.col = np.array([np.where(keep, np.tril(A), 0.0) - np.diag(self.arm) for A in mats])
        self.colh = self.col if mats_h is None else np.array([np.where(keep, np.tril(A), 0.0) - np.diag(self.arm) for A in mats_h])

    def inputs(self):
        """[ntrial][2 nvp][64]: zero below the diagonal outside the ancestor pattern (the updates multiply it), NaN wherever
        the factorisations claim not to read: above the diagonal, and the rows and lanes past nv."""
        n, nv, nvp = len(self.col), self.nv, self.nvp
        x = np.full((n, 2 * nvp, 64), np.nan)
        for t, src in enumerate((self.col, self.colh)):
            blk = np.full((n, nvp, 64), np.nan)
            blk[:, :nv, :nv] = np.where(np.tril(np.ones((nv, nv), dtype=bool)), src, np.nan)
            x[:, t * nvp: (t + 1) * nvp] = blk
        return x


def edited(pod, nv=None, anc=None, damping=None):
    p = copy_pod(pod)
    if nv is not None:
        p.nv = nv
    if anc is not None:
        for k, a in enumerate(anc):
            p.dof_ancmask[k] = a
    if damping is not None:
        for k in range(len(damping)):
            p.dof_damping[k] = damping[k]
            p.params.dof_damping[k] = damping[k]
    return p


@functools.lru_cache(maxsize=None)
def factor_cases(which):
    """About 64 trials per tree, in as few calls as there are model blocks."""
    rng = np.random.default_rng(40 + which)
    lo, hi = pivot_range()
    name = TREE_MODEL.get(which, "cassie")
    pod, mats = model_matrices(name)
    nv, h = pod.nv, pod.timestep
    nvp = tree(which)[0]
    anc = [int(pod.dof_ancmask[k]) for k in range(nv)]
    if which != RT:
        assert anc == tree(which)[2][:nv] and nv == tree(which)[1]
    syn = [synthetic(rng, anc, nv, lo, hi) for _ in range(24)]
    syn_h = [synthetic(rng, anc, nv, lo, hi) for _ in range(24)]
    diag = [np.diag(np.exp(rng.uniform(math.log(lo), math.log(hi), nv)))]
    d0 = np.array(pod.dof_damping[:nv])
    big = np.full(nv, 1e6 * float(np.max(np.abs(mats))) / h)  # h B dominates M by 10^6
    cases = [FactorCase("model matrices", pod, anc, nv, nvp, h, mats),
             FactorCase("synthetic", pod, anc, nv, nvp, h, syn + diag, syn_h + diag),
             FactorCase("no damping", edited(pod, damping=0 * d0), anc, nv, nvp, h, mats[:4]),
             FactorCase("damping dominates", edited(pod, damping=big), anc, nv, nvp, h, mats[:4])]
    if which == RT:
        for n in (1, 2):  # the smallest trees: a single dof, a parent and its child
            a = [0, 1][:n]
            cases.append(FactorCase("nv = %d" % n, edited(pod, nv=n, anc=a), a, n, nvp, h, [synthetic(rng, a, n, lo, hi) for _ in range(4)]))
        tpod, tmats = model_matrices("cassie_tray_box")  # 38 of the 40 dofs the form is instantiated for
        tanc = [int(tpod.dof_ancmask[k]) for k in range(tpod.nv)]
        cases.append(FactorCase("nv = 38 of 40", tpod, tanc, tpod.nv, nvp, tpod.timestep, tmats[:8]))
    return cases


def read_factors(which, out, nv, sets=(0,)):
    """The output sets of a factor body as dicts of [ntrial] arrays: L / LH [nv][nv] (entry (k, i), NaN where the form keeps
    none), dinv, dinvH, rsd [nv], col / colh [nvp][64] and, for the packed forms, the raw Lp / LHp words."""
    nvp, _, _, count, slot = tree(which)
    R = (count + 63) // 64
    rows = 2 * R + 3 + 2 * nvp
    res = []
    for s in sets:
        o = out[:, s * rows: (s + 1) * rows]
        d = {"dinv": o[:, 2 * R, :nv], "dinvH": o[:, 2 * R + 1, :nv], "rsd": o[:, 2 * R + 2, :nv],
             "col": o[:, 2 * R + 3: 2 * R + 3 + nvp], "colh": o[:, 2 * R + 3 + nvp: 2 * R + 3 + 2 * nvp]}
        if which == RT:
            d["L"], d["LH"] = d["col"][:, :nv, :nv], d["colh"][:, :nv, :nv]
        else:
            sl = slot[:nv, :nv]
            for key, at in (("L", 0), ("LH", R)):
                flat = o[:, at: at + R].reshape(len(o), -1)
                d[key + "p"] = flat[:, :count]
                d[key] = np.where(sl >= 0, flat[:, np.maximum(sl, 0)], np.nan)
        res.append(d)
    return res


# ------------------------------------------------------------------------------- factorisation: the backward error ---
def backward_error_ratio(C, extra, L, dinv, anc, nv):
    """max over the diagonal and the ancestor pairs of |A - L^T D L|_ij / ((nv + 8) u (|L^T| |D| |L|)_ij), with A = C + diag(extra)
    (C fp64, extra exact), D = 1 / dinv, in exact integer arithmetic over one common denominator.

    c = nv + 8: at most nv - 1 update terms per entry, each one multiply-add, the multiplier's own rounding, a reciprocal
    within 1.86 ulp (the worst csrc/pk_factor_solve.h records), the final scaling, and the roundings of the diagonal terms."""
    desc = descendants(anc, nv)
    assert np.all(np.isfinite(dinv)) and np.all(dinv != 0)
    num, den = zip(*[float(d).as_integer_ratio() for d in dinv])
    Pn = math.prod(num)
    w = [Pn // num[k] * den[k] for k in range(nv)]  # 1 / dinv[k] = w[k] / Pn
    pairs = [(k, i) for k in range(nv) for i in range(k) if (anc[k] >> i) & 1]
    ratios = {(k, i): float(L[k][i]).as_integer_ratio() for k, i in pairs}
    assert all(math.isfinite(L[k][i]) for k, i in pairs)
    A = {(i, j): Fraction(float(C[i][j])) + (extra[i] if i == j else 0) for i, j in pairs + [(i, i) for i in range(nv)]}
    S = max([r[1].bit_length() - 1 for r in ratios.values()] + [(a.denominator.bit_length() + 1) // 2 for a in A.values()] + [0])
    Li = {key: r[0] << (S - (r[1].bit_length() - 1)) for key, r in ratios.items()}
    for k in range(nv):
        Li[(k, k)] = 1 << S
    scale = Pn << (2 * S)
    c = nv + 8
    worst = 0.0
    for (i, j), a in A.items():
        ks = [i] + desc[i]
        got = sum(Li[(k, i)] * Li[(k, j)] * w[k] for k in ks)
        assert scale % a.denominator == 0
        err = abs(a.numerator * (scale // a.denominator) - got) / abs(scale)
        mag = sum(abs((1.0 if k == i else L[k][i]) * (1.0 if k == j else L[k][j]) / dinv[k]) for k in ks)
        if mag == 0.0:  # (an entry of the pattern the model leaves zero: orthogonal axes)
            assert err == 0.0, (i, j, err)
            continue
        ratio = err / (c * U * mag)
        assert math.isfinite(ratio), (i, j, err, mag)
        worst = max(worst, ratio)
    return worst


def case_extras(case):
    arm = [Fraction(float(a)) for a in case.arm]
    return arm, [a + Fraction(float(case.h)) * Fraction(float(d)) for a, d in zip(arm, case.damp)]


def factor_ratios(case, f):
    """The largest backward-error ratio of the two factorisations over the trials of a case, and the largest distance of rsd
    from sqrt(dinv) in ulps."""
    arm, armh = case_extras(case)
    worst = rs = 0.0
    for t in range(len(case.col)):
        assert np.all(f["dinv"][t] > 0) and np.all(f["dinvH"][t] > 0)  # (finite: backward_error_ratio)
        worst = max(worst, backward_error_ratio(case.col[t], arm, f["L"][t], f["dinv"][t], case.anc, case.nv),
                    backward_error_ratio(case.colh[t], armh, f["LH"][t], f["dinvH"][t], case.anc, case.nv))
        for d, r in zip(f["dinv"][t], f["rsd"][t]):
            want = mpmath.sqrt(mpmath.mpf(float(d)))
            rs = max(rs, float(abs(mpmath.mpf(float(r)) - want) / mpmath.ldexp(1, int(mpmath.floor(mpmath.log(want, 2))) - 52)))
    return worst, rs


@functools.lru_cache(maxsize=None)
def run_factor(backend, which):
    wc = _wave_check(backend)
    return [wc.run(FACTOR_BODY[which], case.inputs(), aux=wc.factor_aux(case.pod, case.h)) for case in factor_cases(which)]


@pytest.mark.parametrize("which", [RT, CASSIE, TRAY], ids=["runtime", "cassie", "tray"])
def test_factorisations_meet_the_componentwise_backward_error_bound(wc, which):
    """|A - L^T D L|_ij <= (nv + 8) u (|L^T| |D| |L|)_ij on the diagonal and every ancestor pair, for the factors of M and of
    M + hB as returned (read through LPack::idx for the packed forms), and rsd within 1 ulp of sqrt(dinv): the oracle's mass
    matrices at 16 poses with nominal and with per-body scaled inertias, synthetic L^T D L over the widened pivot range, a diagonal
    matrix, damping 0 and damping that dominates M, and for the run-time form nv = 1, 2 and 38 of 40 (Cassie's matrices through
    the run-time form with Cassie's masks and through the Cassie-32 form are the same matrices; the two eliminate in different
    orders, so their bits are not compared).
    Largest error / bound, emulator: runtime 0.226, cassie 0.238, tray 0.18; rsd 0.5 ulp.
    Device: runtime 0.231, cassie 0.279, tray 0.18; rsd 0.5 ulp."""
    mp_prec = mpmath.mp.prec
    mpmath.mp.prec = 200
    try:
        worst = rs = 0.0
        for case, out in zip(factor_cases(which), run_factor(wc.backend, which)):
            sets = read_factors(which, out, case.nv, sets=(0,) if which == RT else (0, 1))
            r, s = factor_ratios(case, sets[0])
            assert r <= 1.0 and s <= 1.0, (case.label, r, s)
            worst, rs = max(worst, r), max(rs, s)
    finally:
        mpmath.mp.prec = mp_prec
    report(wc, "factorisation (%s)" % FACTOR_BODY[which], worst)
    report(wc, "rsd against sqrt(dinv), in ulps, (%s)" % FACTOR_BODY[which], rs)


@pytest.mark.parametrize("which", [CASSIE, TRAY], ids=["cassie", "tray"])
def test_split_factorisation_gives_the_bits_of_the_interleaved_one(wc, which):
    """WHICH = 0 followed by WHICH = 1 (the two-wave form) leaves the bits WHICH = 2 leaves: every packed entry a row keeps,
    dinv, dinvH, rsd, and the columns at and below the diagonal."""
    nv = tree(which)[1]
    sl = tree(which)[4][:nv, :nv]
    low = np.tril(np.ones((nv, nv), dtype=bool))
    for case, out in zip(factor_cases(which), run_factor(wc.backend, which)):
        a, b = read_factors(which, out, case.nv, sets=(0, 1))
        for key in ("dinv", "dinvH", "rsd"):
            assert np.all(np.isfinite(a[key])) and np.all(same_bits(a[key], b[key])), (case.label, key)
        for key in ("L", "LH"):
            assert np.all(np.isfinite(a[key][:, sl >= 0])) and np.all(same_bits(a[key][:, sl >= 0], b[key][:, sl >= 0])), (case.label, key)
        for key in ("col", "colh"):
            assert np.all(same_bits(a[key][:, :nv, :nv][:, low], b[key][:, :nv, :nv][:, low])), (case.label, key)


# ------------------------------------------------------------------------------------------------------- the solves ---
@functools.lru_cache(maxsize=None)
def solve_cases(which):
    """(anc, nv, L [n][nv][nv], LH, z [n][nv], w): random unit-triangular factors on the tree's pattern with random vectors,
    every unit vector (a wrong level assignment shows as a missing term) and vectors spanning 10^+-8."""
    rng = np.random.default_rng(50 + which)
    nvp = tree(which)[0]
    if which == RT:
        pod = model_matrices("cassie_tray_box")[0]
        nv, anc = pod.nv, [int(pod.dof_ancmask[k]) for k in range(pod.nv)]
    else:
        nv, anc = tree(which)[1], tree(which)[2][:tree(which)[1]]
    pat = pattern(anc, nv)
    vec = [rng.normal(size=nv) for _ in range(8)] + list(np.eye(nv)) + [rng.normal(size=nv) * 10.0 ** rng.uniform(-8, 8, nv) for _ in range(8)]
    n = len(vec)
    L = pat * rng.uniform(-1, 1, (n, nv, nv))
    LH = pat * rng.uniform(-1, 1, (n, nv, nv))
    z = np.array(vec)
    w = np.array(vec[::-1])
    return anc, nv, nvp, L, LH, z, w


def solve_inputs(which):
    anc, nv, nvp, L, LH, z, w = solve_cases(which)
    n = len(z)
    x = np.full((n, 2 * nvp + 3, 64), np.nan)  # (NaN where the staging claims not to read: the diagonal, above it, past nv)
    for t, M in enumerate((L, LH)):
        blk = np.full((n, nvp, 64), np.nan)
        blk[:, :nv, :nv] = np.where(np.tril(np.ones((nv, nv), dtype=bool), -1), M, np.nan)
        x[:, t * nvp: (t + 1) * nvp] = blk
    x[:, 2 * nvp] = 0.0
    x[:, 2 * nvp + 1] = 0.0
    x[:, 2 * nvp, :nv] = z
    x[:, 2 * nvp + 1, :nv] = w
    x[:, 2 * nvp + 2] = nv
    return x


def residual_ratio(T, rhs, x, nterms):
    """max_i |rhs - T x|_i / ((n_i + 2) u (|T| |x| + |rhs|)_i) for unit-triangular T (T = I + strict part), exactly."""
    n = len(rhs)
    worst = 0.0
    assert np.all(np.isfinite(x))
    fx = [Fraction(float(v)) for v in x]
    for i in range(n):
        nz = [j for j in range(n) if j != i and T[i][j] != 0.0]
        r = Fraction(float(rhs[i])) - fx[i] - sum(Fraction(float(T[i][j])) * fx[j] for j in nz)
        mag = abs(x[i]) + sum(abs(T[i][j] * x[j]) for j in nz) + abs(rhs[i])
        if mag == 0.0:
            assert r == 0
            continue
        worst = max(worst, float(abs(r)) / ((nterms[i] + 2) * U * mag))
    return worst


def solve_ratios(which, xf, xb):
    """Forward: L x = z, n_i = ancestors of dof i.  Backward: LH^T x = w, n_i = descendants of dof i."""
    anc, nv, nvp, L, LH, z, w = solve_cases(which)
    na = [bin(a).count("1") for a in anc]
    nd = [len(d) for d in descendants(anc, nv)]
    fwd = max(residual_ratio(L[t], z[t], xf[t], na) for t in range(len(z)))
    bwd = max(residual_ratio(LH[t].T, w[t], xb[t], nd) for t in range(len(z)))
    return fwd, bwd


@pytest.mark.parametrize("which", [RT, CASSIE, TRAY], ids=["runtime", "cassie", "tray"])
def test_solves_meet_the_componentwise_residual_bound(wc, which):
    """Forward |z - L x|_i <= (n_i + 2) u (|L| |x| + |z|)_i with n_i the ancestors of dof i (the terms of its row), backward the
    same with the descendants; the order of summation does not enter.  The factors reach the solves the way the kernel's do:
    parked in the (packed) rows, staged per lane by stage_factor_row / stage_factor_h.  The run-time form runs the tray model's
    38-dof tree.
    Largest error / bound, emulator: forward 0.216 / 0.213 / 0.212, backward 0.249 / 0.231 / 0.257 (runtime / cassie / tray).
    Device: forward 0.117 / 0.213 / 0.212, backward 0.2 / 0.231 / 0.257."""
    nv = solve_cases(which)[1]
    out = wc.run(SOLVE_BODY[which], solve_inputs(which))
    fwd, bwd = solve_ratios(which, out[:, 0, :nv], out[:, 1, :nv])
    report(wc, "forward solve (%s)" % SOLVE_BODY[which], fwd)
    report(wc, "backward solve (%s)" % SOLVE_BODY[which], bwd)
    assert fwd <= 1.0 and bwd <= 1.0, (fwd, bwd)
    assert np.all(out[:, :, nv:] == 0.0)  # lanes that are no dof pass their zeros through


# --------------------------------------------------------------------------------------------------- the PGS sweeps ---
NOT_BOUNDED = -1e300  # flo of an unclamped row (csrc/env_step_solve.inc)
GUARD = Fraction(1e-10)
MARGIN = 1000.0
SWEEP_KINDS = ("unclamped", "clamped at 0", "mixed", "guard fires")


class Sweep:
    """One trial: `nrows` rows of an N-row instantiation in the scaled domain (B = -A / diag(A), s = -res / diag(A)) from an SPD
    A = Y Y^T + R; lanes past nrows are not rows, padded as the kernel pads them: zero row and zero column of B, Aii = 1, f = s = 0,
    no lower bound."""

    def __init__(self, N, nrows, kind, seed):
        rng = np.random.default_rng(seed)
        self.N, self.nrows, self.kind = N, nrows, kind
        Y = rng.normal(size=(nrows, 12))
        A = Y @ Y.T + np.diag(rng.uniform(0.05, 0.5, nrows))
        d = np.diag(A).copy()
        self.B = np.zeros((64, N))
        self.B[:nrows, :nrows] = -A / d[:, None]
        self.Aii = np.ones(64)
        self.Aii[:nrows] = d
        self.flo = np.full(64, NOT_BOUNDED)
        self.f = np.zeros(64)
        self.s = np.zeros(64)
        r = slice(0, nrows)
        if kind == "unclamped":
            self.s[r] = rng.normal(size=nrows)
        elif kind == "clamped at 0":       # f = 0 at its bound and the residual pushes further down: every step is max(s, 0) = 0
            self.flo[r] = 0.0
            self.s[r] = -rng.uniform(0.5, 2.0, nrows)
        elif kind == "mixed":
            self.flo[r] = np.where(rng.random(nrows) < 0.6, 0.0, NOT_BOUNDED)
            self.f[r] = np.where(self.flo[r] == 0.0, rng.uniform(0.0, 0.3, nrows) * (rng.random(nrows) < 0.7), rng.normal(size=nrows))
            self.s[r] = rng.normal(size=nrows)
        else:                              # f below its bound: the clamped step up to the bound raises the cost by a wide margin
            below = rng.random(nrows) < 0.7
            below[:1] = True
            self.flo[r] = np.where(below, 0.0, NOT_BOUNDED)
            self.f[r] = np.where(self.flo[r] == 0.0, -rng.uniform(0.5, 1.5, nrows), rng.normal(size=nrows))
            self.s[r] = np.where(self.flo[r] == 0.0, -rng.uniform(0.0, 0.5, nrows), rng.normal(size=nrows))

    def inputs(self, nrows=None):
        x = np.zeros((self.N + 5, 64))
        x[: self.N] = self.B.T
        x[self.N] = self.nrows if nrows is None else nrows
        x[self.N + 1], x[self.N + 2], x[self.N + 3], x[self.N + 4] = self.Aii, self.flo, self.f, self.s
        return x

    @functools.lru_cache(maxsize=None)
    def exact(self, guarded):
        """The sweep in rationals -- the kernel's row order, its clamp max(s, flo - f), its guard change > 1e-10 (guarded) -- and,
        alongside, first-order running bounds on what fp64 can differ by.  With ed the bound on a row's step (that of the operand
        the clamp selects: e_I unclamped, ef_I + u |flo - f| clamped; max is 1-Lipschitz and the margins below keep the selection
        the same), after row I
            e_j  <- e_j + |B_jI| ed + u (|B_jI delta| + |s_j|)     (the product's rounding, absent when contracted, and the sum's)
            ef_I <- ef_I + ed + u |f_I|
            ec    = |delta| (halfAii ed + Aii e_I + u (|halfAii delta| + |Aii s_I| + |g|)) + |g| ed + u |change|,  g = halfAii delta - Aii s_I
            ei   <- ei + ec + u |improvement|.
        Returns the exact f, s, improvement, the residual each row started from (mys), their bounds, which rows' guards fired, and
        the smallest margin of any comparison: distance to the threshold / its error bound."""
        n = self.nrows
        B = [[Fraction(float(v)) for v in row[:n]] for row in self.B[:n]]
        aB = np.abs(self.B[:n, :n])
        Aii = [Fraction(float(v)) for v in self.Aii[:n]]
        flo = [Fraction(float(v)) for v in self.flo[:n]]
        f = [Fraction(float(v)) for v in self.f[:n]]
        s = [Fraction(float(v)) for v in self.s[:n]]
        mys = list(s)
        e, ef, emys = np.zeros(n), np.zeros(n), np.zeros(n)
        imp, ei = Fraction(0), 0.0
        fired = np.zeros(n, dtype=bool)
        margin = math.inf
        lo0 = [flo[i] - f[i] for i in range(n)]
        for I in range(n):
            lo = flo[I] - f[I] if guarded else lo0[I]
            elo = (ef[I] if guarded else 0.0) + U * abs(float(lo))
            mys[I], emys[I] = s[I], e[I]
            margin = min(margin, abs(float(s[I] - lo)) / max(e[I] + elo, 1e-300))
            clamped = lo > s[I]
            delta, ed = (lo, elo) if clamped else (s[I], e[I])
            if guarded:
                g = Aii[I] / 2 * delta - Aii[I] * s[I]
                change = delta * g
                a, fd, fs, fg = float(Aii[I]), abs(float(delta)), abs(float(s[I])), abs(float(g))
                ec = fd * (0.5 * a * ed + a * e[I] + U * (0.5 * a * fd + a * fs + fg)) + fg * ed + U * abs(float(change))
                margin = min(margin, abs(float(change - GUARD)) / max(ec, 1e-300))
                if change > GUARD:
                    fired[I] = True
                    continue
                f[I] += delta
                ef[I] += ed + U * abs(float(f[I]))
                imp -= change
                ei += ec + U * abs(float(imp))
            for j in range(n):
                p = B[j][I] * delta
                s[j] += p
                e[j] += aB[j][I] * ed + U * (abs(float(p)) + abs(float(s[j])))
        return {"f": f, "s": s, "imp": imp, "mys": mys, "ef": ef, "e": e, "ei": ei, "emys": emys, "fired": fired, "margin": margin}


NROWS = lambda N: (0, 1, 3, 4, 5, N - 2, N - 1)


@functools.lru_cache(maxsize=None)
def sweep_cases(N):
    """Every nrows x kind; the seed of a trial is the first at which every comparison of both sweeps (clamp and guard) is farther
    from its threshold than MARGIN times its error bound, so that no assertion can hide behind a discontinuity."""
    cases = []
    for nrows in NROWS(N):
        for k, kind in enumerate(SWEEP_KINDS):
            for seed in range(1000 * N + 10 * nrows + k, 1 << 30, 7919):
                c = Sweep(N, nrows, kind, seed)
                if min(c.exact(True)["margin"], c.exact(False)["margin"]) > MARGIN:
                    break
            cases.append(c)
    return cases


def within(got, exact, bound):
    """max |got - exact| / (2 bound); where the bound is 0 the result must be exact.  The factor 2 covers the second-order terms
    the first-order recurrences drop."""
    worst = 0.0
    for g, x, b in zip(np.ravel(got), exact, np.ravel(bound)):
        assert math.isfinite(g)
        err = abs(float(Fraction(float(g)) - x))
        if b == 0.0:
            assert err == 0.0, (g, float(x))
        else:
            worst = max(worst, err / (2 * b))
    return worst


def not_rows_untouched(c, *pairs):
    for got, start in pairs:
        assert np.all(same_bits(got[c.nrows:], start[c.nrows:]))


def guarded_ratio(c, out):
    x = c.exact(True)
    n = c.nrows
    f, s, imp = out[0], out[1], out[2]
    assert np.all(same_bits(f[:n][x["fired"]], c.f[:n][x["fired"]]))  # a fired row leaves f untouched
    not_rows_untouched(c, (f, c.f), (s, c.s))
    assert np.all(same_bits(imp, np.full(64, imp[0])))  # wave-uniform
    return max(within(f[:n], x["f"], x["ef"]), within(s[:n], x["s"], x["e"]), within(imp[:1], [x["imp"]], [x["ei"]]))


def fast_ratio(c, out):
    x = c.exact(False)
    n = c.nrows
    not_rows_untouched(c, (out[0], c.s), (out[1], np.zeros(64)))
    return max(within(out[0][:n], x["s"], x["e"]), within(out[1][:n], x["mys"], x["emys"]))


@pytest.mark.parametrize("N", [32, 48, 64])
def test_sweep_inputs_stay_clear_of_every_threshold(N):
    """In the exact reference every row's cost change lies outside 1e-10 +- 1000 e and every clamp comparison is decided by more
    than 1000 e, in all cases; the guard fires in the cases made for it (by a wide margin: a cost increase above 0.05) and nowhere else."""
    cases = sweep_cases(N)
    assert len(cases) == len(NROWS(N)) * len(SWEEP_KINDS)
    for c in cases:
        g, f = c.exact(True), c.exact(False)
        assert g["margin"] > MARGIN and f["margin"] > MARGIN, (c.nrows, c.kind)
        if c.kind == "guard fires":
            assert g["fired"].any() == (c.nrows > 0)
        else:
            assert not g["fired"].any()


@pytest.mark.parametrize("N", [32, 48, 64])
def test_guarded_sweep_meets_its_running_bound(wc, N):
    """pgs_rows at FAST_ROWS + 1, FAST_ROWS_TRAY + 1 and NROW rows, nrows in {0, 1, 3, 4, 5, N - 2, N - 1}, all rows unclamped /
    clamped at 0 / mixed / started below their bound so that the guard fires: f, sres and the improvement within twice the running
    bound of Sweep.exact; rows whose guard fired leave f and every sres untouched and stay out of the improvement (they are in
    the exact sweep, which the bound holds the result to); lanes that are no row come back as they went in.
    Largest error / (2 bound), emulator: 0.296 / 0.387 / 0.497 (N = 32 / 48 / 64).  Device: the same three figures."""
    cases = sweep_cases(N)
    out = wc.run("pgs_guarded%d" % N, np.array([c.inputs() for c in cases]))
    worst = 0.0
    for c, o in zip(cases, out):
        worst = max(worst, guarded_ratio(c, o))
        if c.kind == "guard fires" and c.exact(True)["fired"].all():  # nothing moved at all
            assert np.all(same_bits(o[1], c.s)) and np.all(o[2] == 0.0)
    report(wc, "guarded sweep (N = %d)" % N, worst)
    assert worst <= 1.0


@pytest.mark.parametrize("N", [32, 48, 64])
def test_fast_sweep_meets_its_running_bound_and_its_padding_is_inert(wc, N):
    """pgs_rows_fast on the same cases: sres and the residual each row started from (mys) within twice the running bound.
    The premise of its four-rows-to-a-branch form: run with the true nrows it gives, bit for bit, what it gives with nrows rounded
    up to the next multiple of four on the same padded inputs.  Where no guard fires, the guarded and the fast sweep agree
    within the sum of their bounds (their bits are not compared: fmax against the raw maximum).
    Largest error / (2 bound), emulator: 0.385 / 0.298 / 0.408 (N = 32 / 48 / 64).  Device: 0.385 / 0.285 / 0.408."""
    cases = sweep_cases(N)
    out = wc.run("pgs_fast%d" % N, np.array([c.inputs() for c in cases]))
    up = wc.run("pgs_fast%d" % N, np.array([c.inputs(nrows=-(-c.nrows // 4) * 4) for c in cases]))
    assert all(-(-c.nrows // 4) * 4 <= N for c in cases)
    assert np.all(same_bits(out, up))
    guarded = wc.run("pgs_guarded%d" % N, np.array([c.inputs() for c in cases]))
    worst = 0.0
    for c, o, g in zip(cases, out, guarded):
        worst = max(worst, fast_ratio(c, o))
        xg, xf = c.exact(True), c.exact(False)
        if not xg["fired"].any():
            n = c.nrows
            assert [a == b for a, b in zip(xg["s"], xf["s"])] == [True] * n  # one sweep in exact arithmetic
            assert np.all(np.abs(o[0][:n] - g[1][:n]) <= 2 * (xg["e"] + xf["e"]))
    report(wc, "fast sweep (N = %d)" % N, worst)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ negative controls ---
def fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def rcp_np(x, newton_steps=2):
    """fast_rcp restated: a seed as far off as the seeds may be (2^-17, inside the 2^-16 test_wave_primitives.py bounds both backends'
    seeds by), r (2 - x r), then r + r (1 - x r) with fused steps."""
    r = float(np.float32(1.0) / np.float32(x)) * (1 + 2.0 ** -17)
    if newton_steps >= 1:
        r = r * (2.0 - x * r)
    if newton_steps >= 2:
        r = fma(r, fma(-x, r, 1.0), r)
    return r


def factor_np(C, diag, anc, nv, drop=None, newton_steps=2):
    """factor_pair_in_registers restated in plain fp64 on one matrix: C lower triangle, diag = the diagonal terms added at the
    pivot.  drop = (k, i): that ancestor update is left out."""
    C = np.array(C, dtype=np.float64)
    dinv = np.zeros(nv)
    for k in range(nv - 1, -1, -1):
        inv = dinv[k] = rcp_np(C[k][k] + diag[k], newton_steps)
        for i in range(k - 1, -1, -1):
            if (anc[k] >> i) & 1 and (k, i) != drop:
                C[i, : i + 1] -= (C[k][i] * inv) * C[k, : i + 1]
        C[k, :k] *= inv
    return C, dinv


def test_controls_factorisation():
    """A plain fp64 restatement of the factorisation stays inside the backward-error bound; with one ancestor update dropped, or
    with one Newton step taken out of the reciprocal, it leaves it by more than 100 x."""
    case = factor_cases(CASSIE)[0]
    arm, _ = case_extras(case)
    C = case.col[0]
    good = backward_error_ratio(C, arm, *factor_np(C, case.arm, case.anc, case.nv), case.anc, case.nv)
    dropped = backward_error_ratio(C, arm, *factor_np(C, case.arm, case.anc, case.nv, drop=(20, 19)), case.anc, case.nv)
    short = backward_error_ratio(C, arm, *factor_np(C, case.arm, case.anc, case.nv, newton_steps=1), case.anc, case.nv)
    print("factorisation controls: faithful %.3g, one update dropped %.3g, one Newton step fewer %.3g" % (good, dropped, short))
    assert good <= 1.0 and dropped >= 100.0 and short >= 100.0


def solve_forward_np(L, z, anc, nv, drop_level=None):
    """solve_forward restated: level by level of the dof tree, a level's terms summed before they touch the vector."""
    x = np.array(z, dtype=np.float64)
    level = [bin(a).count("1") for a in anc]
    for d in range(max(level)):
        js = [j for j in range(nv) if level[j] == d]
        t = sum(L[:, j] * x[j] for j in js)
        if d != drop_level:
            x = x - t
    return x


def test_controls_solve():
    """A plain fp64 restatement of the forward solve stays inside the residual bound; with one level's term dropped it leaves it
    by more than 100 x."""
    anc, nv, nvp, L, LH, z, w = solve_cases(CASSIE)
    na = [bin(a).count("1") for a in anc]
    good = max(residual_ratio(L[t], z[t], solve_forward_np(L[t], z[t], anc, nv), na) for t in range(8))
    bad = min(residual_ratio(L[t], z[t], solve_forward_np(L[t], z[t], anc, nv, drop_level=5), na) for t in range(8))
    print("solve controls: faithful %.3g, one level dropped %.3g" % (good, bad))
    assert good <= 1.0 and bad >= 100.0


def sweep_np(c, zeroed=None):
    """pgs_rows restated in plain fp64; zeroed = (j, I): lane j's brow entry of row I is zero."""
    B = c.B.copy()
    if zeroed:
        B[zeroed] = 0.0
    f, s, imp = c.f.copy(), c.s.copy(), 0.0
    for I in range(c.nrows):
        delta = max(s[I], c.flo[I] - f[I])
        change = delta * (0.5 * c.Aii[I] * delta - c.Aii[I] * s[I])
        if change > 1e-10:
            continue
        f[I] += delta
        imp -= change
        s = s + B[:, I] * delta
    return np.array([f, s, np.full(64, imp)])


def test_controls_sweep():
    """A plain fp64 restatement of the guarded sweep stays inside its running bound; with one row's brow entry zeroed it leaves
    it by more than 100 x."""
    cases = [c for c in sweep_cases(32) if c.nrows == 30 and c.kind in ("unclamped", "mixed")]
    good = max(guarded_ratio(c, sweep_np(c)) for c in cases)
    bad = min(guarded_ratio(c, sweep_np(c, zeroed=(7, 3))) for c in cases)
    print("sweep controls: faithful %.3g, one brow entry zeroed %.3g" % (good, bad))
    assert good <= 1.0 and bad >= 100.0
