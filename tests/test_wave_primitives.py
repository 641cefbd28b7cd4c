"""The wavefront primitives of csrc/wave.h and the kernel's small numerical helpers, one at a time, against exact
references -- on the CPU wave emulator (the stand-ins of tests/emu/wave.h, which every emulator test of the step kernel
rests on) and, with -m gpu, on the device build of the same bodies (tests/device/wave_bodies.h, product flags).

Cross-lane primitives are bit-exact on both backends, and the device gives the emulator's bits.  The arithmetic helpers
(fast_rcp, normalize*_fast, sincos_reduced) are held to one accuracy bound on both backends; their bits may differ
(the device build contracts into FMAs and starts from the hardware seeds)."""
import functools
import math
import os
import subprocess
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from wave_check import LIBS, REPO, WaveCheck

BACKENDS = ["emu", pytest.param("device", marks=pytest.mark.gpu)]
U = 2.0 ** -53  # unit roundoff, fp64


@functools.lru_cache(maxsize=None)
def _wave_check(backend):
    if not os.path.exists(LIBS[backend]):
        subprocess.check_call(["make", "-C", REPO, "emu"], stdout=subprocess.DEVNULL)
    return WaveCheck(backend)


@pytest.fixture(params=BACKENDS)
def wc(request):
    return _wave_check(request.param)


def same_bits(a, b):
    """Elementwise: the same IEEE bits, or both NaN (NaN payloads are not part of any contract here)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))


# ----------------------------------------------------------------------------------------------- DPP and the sums ---
LANE = np.arange(64)
ROW = LANE >> 4
# the moves of wave_sum / wave_sum_f32 in their order: (DPP control, row mask)
SUM_STEPS = [(0xB1, 0xF), (0x4E, 0xF), (0x141, 0xF), (0x140, 0xF), (0x142, 0xA), (0x143, 0xC)]


def dpp_ref(v, ctrl, row_mask):
    """v_mov_dpp with old = 0 and bound_ctrl off, from the ISA's definition of the controls: quad_perm (lane i of a quad
    takes lane ctrl[2i+1:2i] of it), row_mirror, row_half_mirror, row_bcast15 (lane 15 of each row into the next row),
    row_bcast31 (lane 31 into rows 2 and 3).  A lane of a row outside the row mask, or one the control gives no source,
    keeps old = 0."""
    valid = np.ones(64, dtype=bool)
    if ctrl <= 0xFF:
        src = (LANE & ~3) | ((ctrl >> (2 * (LANE & 3))) & 3)
    elif ctrl == 0x140:
        src = (LANE & ~15) | (15 - (LANE & 15))
    elif ctrl == 0x141:
        src = (LANE & ~7) | (7 - (LANE & 7))
    elif ctrl == 0x142:
        src, valid = 16 * ROW - 1, ROW > 0
    elif ctrl == 0x143:
        src, valid = np.full(64, 31), ROW >= 2
    else:
        raise ValueError(hex(ctrl))
    take = v[np.where(valid, src, LANE)]
    return np.where(valid & (((row_mask >> ROW) & 1) == 1), take, v.dtype.type(0))


def wave_sum_ref(x, dtype=np.float64):
    """The documented tree (csrc/wave.h wave_sum): six DPP adds, each a correctly rounded add in `dtype`, lane 63's
    value returned."""
    v = np.asarray(x, dtype=dtype).copy()
    with np.errstate(all="ignore"):
        for ctrl, mask in SUM_STEPS:
            v = v + dpp_ref(v, ctrl, mask)
    return v[63]


def sum_cases(single):
    """(label, 64 inputs) for the sums; in float32 range and values for `single`."""
    rng = np.random.default_rng(11 if single else 10)
    big, tiny = (1e36, 1e-38) if single else (1e300, 1e-300)
    den = np.float32(1e-41) if single else 5e-324
    c = [("random %d" % i, rng.normal(size=64) * 10.0 ** rng.integers(-3, 4)) for i in range(8)]
    for i in range(4):  # heavy cancellation: pairs that nearly annihilate, one large residue
        x = rng.normal(size=64) * 1e6
        x[32:] = -x[:32] * (1 + rng.normal(size=32) * (1e-5 if single else 1e-13))
        x[rng.integers(64)] += 1e-3
        c.append(("cancellation %d" % i, rng.permutation(x)))
    for i in range(4):  # magnitudes from tiny to big in one wave
        e = rng.uniform(math.log10(tiny), math.log10(big), 64)
        c.append(("mixed magnitudes %d" % i, np.where(rng.random(64) < 0.5, -1.0, 1.0) * 10.0 ** e))
    c.append(("all -0", np.full(64, -0.0)))
    x = rng.normal(size=64); x[37] = np.inf
    c.append(("one +inf", x))
    x = rng.normal(size=64); x[5] = -np.inf
    c.append(("one -inf", x))
    x = rng.normal(size=64); x[3], x[60] = np.inf, -np.inf
    c.append(("+inf and -inf", x))
    x = rng.normal(size=64); x[44] = np.nan
    c.append(("one NaN", x))
    c.append(("denormals", rng.integers(-1000, 1000, 64) * float(den)))
    x = np.zeros(64); x[rng.integers(64)] = den
    c.append(("one denormal", x))
    if single:
        c = [(k, np.asarray(v, dtype=np.float32).astype(np.float64)) for k, v in c]
    return c


def check_sum(wc, single):
    name, dtype, u = ("wave_sum_f32", np.float32, 2.0 ** -24) if single else ("wave_sum", np.float64, U)
    cases = sum_cases(single)
    out = wc.run(name, np.array([v for _, v in cases])[:, None, :])[:, 0, :]
    for (label, x), got in zip(cases, out):
        assert np.all(same_bits(got, got[0])), (label, "not wave-uniform")
        want = float(wave_sum_ref(x, dtype))
        assert same_bits(got[0], want), (label, got[0], want)
        if np.all(np.isfinite(x)):
            err = abs(Fraction(float(got[0])) - sum(Fraction(float(t)) for t in x))
            assert err <= Fraction(6 * u) * sum(abs(Fraction(float(t))) for t in x), (label, float(err))
            assert abs(got[0] - math.fsum(x)) <= 6 * u * math.fsum(abs(x)) * (1 + 1e-12), label
    specials = {k: o[0] for (k, _), o in zip(cases, out)}
    assert same_bits(specials["all -0"], -0.0)
    assert specials["one +inf"] == np.inf and specials["one -inf"] == -np.inf
    assert np.isnan(specials["+inf and -inf"]) and np.isnan(specials["one NaN"])


@pytest.mark.parametrize("single", [False, True], ids=["f64", "f32"])
def test_wave_sum_is_the_documented_tree(wc, single):
    check_sum(wc, single)


def test_wave_sum_inputs_tell_the_tree_orders_apart():
    """The random cases above round differently under another order of the same six steps (so a swap is caught)."""
    x = sum_cases(False)[0][1]
    swapped = [SUM_STEPS[1], SUM_STEPS[0]] + SUM_STEPS[2:]
    v = x.copy()
    for ctrl, mask in swapped:
        v = v + dpp_ref(v, ctrl, mask)
    assert wave_sum_ref(x) != v[63]


def dpp_inputs():
    rng = np.random.default_rng(12)
    x = rng.normal(size=(3, 2, 64))
    x[:, 0, :] += 1000.0 * LANE  # distinct, and telling which lane a value came from
    x[:, 1, :] = np.asarray(x[:, 1, :] + 100.0 * LANE, dtype=np.float32)
    return x


def test_dpp_take_moves(wc):
    """Each DPP move of the sums, alone: the lane it takes from, and 0.0 in the masked and the source-less rows (the
    row_bcast15 move into rows 1 and 3 only, whatever lane 31 holds -- the sum's result would not show it)."""
    x = dpp_inputs()
    out = wc.run("dpp_take", x)
    for t in range(x.shape[0]):
        for i, (ctrl, mask) in enumerate(SUM_STEPS):
            assert np.all(same_bits(out[t, i], dpp_ref(x[t, 0], ctrl, mask))), ("f64", hex(ctrl), hex(mask))
            want32 = dpp_ref(x[t, 1].astype(np.float32), ctrl, mask).astype(np.float64)
            assert np.all(same_bits(out[t, 6 + i], want32)), ("f32", hex(ctrl), hex(mask))
    # the row masks, spelled out: rows 0 and 2 of row_bcast15, rows 0 and 1 of row_bcast31 receive nothing
    assert np.all(out[:, 4, ROW % 2 == 0] == 0.0) and np.all(out[:, 4, ROW == 1] == x[:, 0, 15:16])
    assert np.all(out[:, 5, ROW < 2] == 0.0) and np.all(out[:, 5, ROW >= 2] == x[:, 0, 31:32])


# ---------------------------------------------------------------------------------------------------- lane moves ---
READLANE_SOURCES = [0, 15, 16, 31, 32, 47, 63]


def test_readlane(wc):
    rng = np.random.default_rng(13)
    x = rng.normal(size=(len(READLANE_SOURCES), 2, 64))
    x[:, 1, :] = np.array(READLANE_SOURCES)[:, None]
    out = wc.run("readlane", x)
    for t, src in enumerate(READLANE_SOURCES):
        assert np.all(same_bits(out[t, 0], x[t, 0, src])), src


def test_writelane(wc):
    rng = np.random.default_rng(14)
    x = rng.normal(size=(3, 3, 64))
    x[:, 2, :] = rng.normal(size=(3, 1))  # the wave-uniform value
    out = wc.run("writelane", x)
    for t in range(3):
        for i, dst in enumerate((0, 31, 32, 63)):
            want = x[t, 0] + x[t, 1]
            want[dst] = x[t, 2, 0]
            assert np.all(same_bits(out[t, i], want)), dst


def test_from_upper_half(wc):
    rng = np.random.default_rng(15)
    x = rng.normal(size=(2, 1, 64)) + 1000.0 * LANE
    out = wc.run("from_upper_half", x)[:, 0]
    for t in range(2):
        assert np.all(same_bits(out[t, :32], x[t, 0, 32:])), "lanes 0..31 take lane + 32"
        assert np.all(same_bits(out[t, 32:], x[t, 0, 32:])), "lanes 32..63 keep their own value"


def shfl_inputs():
    rng = np.random.default_rng(16)
    srcs = [rng.integers(0, 64, 64), LANE, 63 - LANE, np.full(64, 17), rng.permutation(64)]
    x = np.empty((len(srcs), 3, 64))
    for t, s in enumerate(srcs):
        x[t, 0] = rng.normal(size=64) + 1000.0 * LANE
        x[t, 1] = s
        x[t, 2] = rng.integers(-2 ** 31, 2 ** 31, 64)
    return x


def test_shfl(wc):
    x = shfl_inputs()
    out = wc.run("shfl", x)
    for t in range(x.shape[0]):
        src = x[t, 1].astype(int)
        assert np.all(same_bits(out[t, 0], x[t, 0, src]))
        assert np.all(out[t, 1] == x[t, 2, src])
        for i, m in enumerate((1, 2, 4, 8, 16, 32)):
            assert np.all(same_bits(out[t, 2 + i], x[t, 0, LANE ^ m])), m


BALLOT_PATTERNS = {"none": LANE < 0, "all": LANE >= 0, "alternating": LANE % 2 == 1, "alternating from 0": LANE % 2 == 0,
                   "lane 0 only": LANE == 0, "lane 63 only": LANE == 63, "upper half": LANE >= 32}


def test_ballot_and_popc64(wc):
    names = list(BALLOT_PATTERNS)
    x = np.array([BALLOT_PATTERNS[k] for k in names], dtype=np.float64)[:, None, :]
    x[:, 0, :] *= np.linspace(-3, 5, 64) + 0.5  # any non-zero value is true
    out = wc.run("ballot", x)
    for t, k in enumerate(names):
        mask = sum(1 << int(l) for l in LANE[BALLOT_PATTERNS[k]])
        assert np.all(out[t, 0] == mask & 0xFFFFFFFF) and np.all(out[t, 1] == mask >> 32), k
        assert np.all(out[t, 2] == bin(mask).count("1")), k


# ------------------------------------------------------------------------------------------------- matrix core -----
def fma_exact(a, b, c):
    """fma(a, b, c) correctly rounded (Python 3.10 has no math.fma)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def mfma_ref(a, b, c, order=(0, 1, 2, 3), fused=True):
    """D = A B + C of v_mfma_f64_16x16x4_f64 from the lane layout: lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15]
    and holds C / D[(l >> 4) + 4 v][l & 15] in register v; every element is the FMA chain over k on top of C."""
    A, B, C = np.empty((16, 4)), np.empty((4, 16)), np.empty((16, 16))
    A[LANE & 15, LANE >> 4] = a
    B[LANE >> 4, LANE & 15] = b
    for v in range(4):
        C[(LANE >> 4) + 4 * v, LANE & 15] = c[v]
    D = np.empty((4, 64))
    for v in range(4):
        for l in range(64):
            i, j = (l >> 4) + 4 * v, l & 15
            acc = float(C[i, j])
            for k in order:
                acc = fma_exact(A[i, k], B[k, j], acc) if fused else float(A[i, k] * B[k, j]) + acc
            D[v, l] = acc
    return D


def mfma_inputs(n, rng):
    """Operands whose products span many binades, so that another k order or unfused products round differently."""
    return rng.normal(size=(n, 6, 64)) * 2.0 ** rng.integers(-4, 5, (n, 6, 64))


def test_mfma_inputs_tell_orders_apart():
    x = mfma_inputs(1, np.random.default_rng(17))[0]
    fwd = mfma_ref(x[0], x[1], x[2:])
    assert np.mean(fwd != mfma_ref(x[0], x[1], x[2:], order=(3, 2, 1, 0))) > 0.3
    assert np.mean(fwd != mfma_ref(x[0], x[1], x[2:], order=(1, 0, 2, 3))) > 0.1
    assert np.mean(fwd != mfma_ref(x[0], x[1], x[2:], fused=False)) > 0.2


def test_mfma_f64_16x16x4(wc):
    x = mfma_inputs(3, np.random.default_rng(17))
    out = wc.run("mfma1", x)
    for t in range(x.shape[0]):
        want = mfma_ref(x[t, 0], x[t, 1], x[t, 2:])
        assert np.all(same_bits(out[t], want)), np.argwhere(~same_bits(out[t], want))[:4]


def test_mfma_f64_16x16x4_chain_of_four(wc):
    rng = np.random.default_rng(18)
    x = np.concatenate([mfma_inputs(2, rng), mfma_inputs(2, rng)], axis=1)  # a[0..3], b[0..3], c[0..3]
    out = wc.run("mfma4", x)
    for t in range(x.shape[0]):
        acc = x[t, 8:12]
        for s in range(4):
            acc = mfma_ref(x[t, s], x[t, 4 + s], acc)
        assert np.all(same_bits(out[t], acc))


# ----------------------------------------------------------------------------------------------------- max_raw -----
DENORMAL = 2.5e-310
MAX_VALUES = [-0.0, 0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, DENORMAL, -DENORMAL]


def v_max_f64(a, b):
    """V_MAX_F64 in IEEE mode (the mode compute kernels run in), as the ISA's pseudo-code gives it: a quiet NaN operand
    yields the other operand (a NaN only when both are); +0 is larger than -0 (either order); otherwise the larger
    value.  Denormal operands are kept (fp64 denormals are not flushed)."""
    if math.isnan(a):
        return b
    if math.isnan(b):
        return a
    if a == 0.0 and b == 0.0:
        return 0.0 if (math.copysign(1, a) > 0 or math.copysign(1, b) > 0) else -0.0
    return a if a >= b else b


def test_max_raw_is_v_max_f64(wc):
    pairs = [(a, b) for a in MAX_VALUES for b in MAX_VALUES]
    got = wc.lanes("max_raw", np.array(pairs).T)[0]
    for (a, b), r in zip(pairs, got):
        assert same_bits(r, v_max_f64(a, b)), (a, b, r)


# ------------------------------------------------------------------------------------------- seeds and fast_rcp -----
mpmath.mp.dps = 60


def ulp_exact(q):
    """ulp of the binade holding the exact positive rational q."""
    e = math.frexp(float(q))[1] - 1
    if Fraction(2) ** e > q:
        e -= 1
    elif Fraction(2) ** (e + 1) <= q:
        e += 1
    return Fraction(2) ** (e - 52)


def log_uniform(rng, n, lo=-60, hi=60):
    return 2.0 ** rng.uniform(lo, hi, n)


def ltdl_pivots(A):
    """The pivots of A = L^T D L, eliminated from the last row up (mj_factorM's order, the kernel's)."""
    A = np.array(A, dtype=np.float64)
    piv = []
    for k in range(len(A) - 1, -1, -1):
        d = A[k, k]
        piv.append(d)
        A[:k, :k] -= np.outer(A[k, :k] / d, A[k, :k])
    return piv


@functools.lru_cache(maxsize=None)
def model_pivots():
    """The pivots fast_rcp sees: those of M + armature and of M + h B (B = the dof damping) for the three models, at
    qpos0 and at randomised joint angles (the oracle's mass matrix, which holds the armature)."""
    from cassie_amd import Model
    from oracle_py import Oracle
    piv = []
    rng = np.random.default_rng(19)
    for name in ("cassie", "cassie_hfield", "cassie_tray_box"):
        m = Model(name)
        p = m.pod
        hB = p.timestep * np.array(p.dof_damping[: p.nv])
        q0 = m.qpos_init()
        for s in range(4):
            q = q0.copy()
            if s:
                for j in range(p.njnt):
                    if p.jnt_type[j] in (2, 3):  # slide, hinge
                        q[p.jnt_qposadr[j]] += rng.uniform(-0.4, 0.4)
            o = Oracle(p, q)
            o.forward()
            M = np.array(o.qM)
            piv += ltdl_pivots(M) + ltdl_pivots(M + np.diag(hB))
    return np.array(piv)


@functools.lru_cache(maxsize=None)
def rcp_inputs():
    rng = np.random.default_rng(20)
    ks = np.arange(1, 65)
    x = [log_uniform(rng, 16384),
         2.0 ** np.arange(-60, 61),                                            # powers of two
         1 + ks * 2.0 ** -52, 1 - ks * 2.0 ** -53,                             # 1 +- k ulp
         (2 - 2.0 ** -52) * 2.0 ** np.arange(-60, 61),                         # all-ones mantissas
         (1 + ks * 2.0 ** -52) * 2.0 ** rng.integers(-60, 61, 64),
         (2 - ks * 2.0 ** -52) * 2.0 ** rng.integers(-60, 61, 64),
         model_pivots()]
    x = np.concatenate(x)
    assert np.all(x > 0) and np.all(np.isfinite(x)) and np.all(x >= 2.0 ** -1022)
    return x


def rcp_ulps(x, r):
    return np.array([float(abs(Fraction(ri) - 1 / Fraction(xi)) / ulp_exact(1 / Fraction(xi))) for xi, ri in zip(x, r)])


def measure_fast_rcp(wc):
    x = rcp_inputs()
    return float(np.max(rcp_ulps(x, wc.lanes("fast_rcp", x)[0])))


def test_fast_rcp_is_faithful(wc):
    """|fast_rcp(x) - 1/x| < ulp(1/x) for positive normal x: random, powers of two, 1 +- k ulp, all-ones mantissas and
    the pivots of the three models' factorisations."""
    x = rcp_inputs()
    err = rcp_ulps(x, wc.lanes("fast_rcp", x)[0])
    assert err.max() < 1.0, (x[err.argmax()], err.max())
    assert np.all(err[np.arange(121) + 16384] == 0)  # 1 / 2^k is exact


def test_model_pivots_are_positive_and_normal():
    """fast_rcp's precondition, on the pivots the kernel factors."""
    p = model_pivots()
    assert len(p) > 500 and np.all(p > 2.0 ** -500) and np.all(p < 2.0 ** 500)


def seed_errors(wc):
    """The largest relative errors |seed x - 1| of the rcp seed and |seed sqrt(x) - 1| of the rsq seed over the sweep."""
    rng = np.random.default_rng(21)
    x = np.concatenate([log_uniform(rng, 8192), model_pivots(), 1 + np.arange(64) * 2.0 ** -52])
    out = wc.lanes("estimates", x)
    rcp = max(abs(float(Fraction(r) * Fraction(v) - 1)) for v, r in zip(x, out[0]))
    rsq = max(abs(float(mpmath.mpf(r) * mpmath.sqrt(mpmath.mpf(v)) - 1)) for v, r in zip(x, out[1]))
    return rcp, rsq


# Newton on the reciprocal, r' = r (2 - x r): with x r = 1 - e, x r' = (1 - e)(1 + e) = 1 - e^2, so two steps take a
# seed's relative error e0 to e0^4.  Newton on the reciprocal square root, y' = y + y (1 - n y^2) / 2: with
# y = (1 + e) / sqrt(n), y' sqrt(n) = 1 - 3 e^2 / 2 - e^3 / 2, so two steps leave about 3.4 e0^4.  For the result to be
# decided by the last step's own rounding (half an ulp, 2^-53 relative) the method error must lie well below it, say
# under 2^-60: e0^4 <= 2^-60 / 3.4, i.e. e0 <= 2^-15.4.  Bound both seeds by 2^-16.
SEED_BOUND = 2.0 ** -16


def test_seed_accuracy_suffices_for_two_newton_steps(wc):
    rcp, rsq = seed_errors(wc)
    assert rcp <= SEED_BOUND and rsq <= SEED_BOUND, (rcp, rsq)


# ------------------------------------------------------------------------------------ normalisations and sincos -----
def _f(x):
    return float(x)


@functools.lru_cache(maxsize=None)
def normalize4_cases():
    rng = np.random.default_rng(22)
    q = np.concatenate([rng.normal(size=(1024, 4)) * s for s in (1.0, 1e-6, 1e6, 1 + 1e-12)])
    want = np.array([[_f(mpmath.mpf(c) / mpmath.sqrt(sum(mpmath.mpf(t) ** 2 for t in v))) for c in v] for v in q])
    return q, want


@functools.lru_cache(maxsize=None)
def normalize3_cases():
    rng = np.random.default_rng(23)
    a = np.concatenate([rng.normal(size=(1024, 3)) * s for s in (1.0, 1e-9, 1e4)])
    norm = [mpmath.sqrt(sum(mpmath.mpf(t) ** 2 for t in v)) for v in a]
    return a, np.array([_f(n) for n in norm]), np.array([[_f(mpmath.mpf(c) / n) for c in v] for v, n in zip(a, norm)])


def measure_normalize(wc):
    q, want4 = normalize4_cases()
    got4 = wc.lanes("normalize4_fast", q.T).T
    a, norm, want3 = normalize3_cases()
    got3 = wc.lanes("normalize3_fast", a.T).T
    return (float(np.max(np.abs(got4 - want4))), float(np.max(np.abs(got3[:, :3] - want3))),
            float(np.max(np.abs(got3[:, 3] - norm) / np.spacing(norm))))


def test_normalize4_fast_and_normalize3_fast(wc):
    """test_kinematics_records.py's bounds: components within 4.5e-16 of the exact unit vector, the norm within 1.01 ulp;
    below the thresholds the identity / the x axis."""
    e4, e3, en = measure_normalize(wc)
    assert e4 < 4.5e-16 and e3 < 4.5e-16 and en <= 1.01, (e4, e3, en)
    out = wc.lanes("normalize4_fast", np.array([[1e-16, 0, 1e-17, 0]]).T)[:, 0]
    assert list(out) == [1, 0, 0, 0]
    out = wc.lanes("normalize3_fast", np.array([[3e-16, 0, -4e-16]]).T)[:, 0]
    assert list(out[:3]) == [1, 0, 0] and abs(out[3] - 5e-16) <= np.spacing(5e-16)


SINCOS_RANGES = ((0.78, 0.8, 12800), (10.0, 1.6, 25600), (524287.0, 2.5, 25600))
LIBRARY_ULPS = 2.0


def sincos_ulps(x, s, c):
    """Worst error of (s, c) against sin / cos at 60 digits, in ulps of the rounded exact value (abs error for sin = 0)."""
    worst = 0.0
    for xi, si, ci in zip(x, s, c):
        rs, rc = mpmath.sin(mpmath.mpf(xi)), mpmath.cos(mpmath.mpf(xi))
        es = abs(_f(mpmath.mpf(si) - rs)) / np.spacing(abs(_f(rs))) if rs != 0 else abs(si)
        ec = abs(_f(mpmath.mpf(ci) - rc)) / np.spacing(abs(_f(rc)))
        worst = max(worst, es, ec)
    return worst


@functools.lru_cache(maxsize=None)
def sincos_range_inputs():
    rng = np.random.default_rng(24)
    return [(np.concatenate([rng.uniform(-b, b, n), [0.0, b, -b, 1e-300, -3e-9]]), tol) for b, tol, n in SINCOS_RANGES]


def measure_sincos(wc):
    """Worst ulps of sincos_reduced per range, and of sincos_bounded in waves with a lane at or beyond 2^19."""
    worst = []
    for x, _ in sincos_range_inputs():
        out = wc.lanes("sincos", x)
        assert np.all(same_bits(out[0], out[2])) and np.all(same_bits(out[1], out[3])), "inside 2^19 sincos_bounded is sincos_reduced"
        worst.append(sincos_ulps(x, out[0], out[1]))
    rng = np.random.default_rng(25)
    far = rng.uniform(-10, 10, (4, 64))
    far[0] = rng.uniform(2.0 ** 19, 2.0 ** 30, 64) * np.where(rng.random(64) < 0.5, -1, 1)  # every lane beyond
    far[1, 7] = 524288.0                                                                   # one lane at 2^19
    far[2, 63] = -3.0e6
    far[3, 0] = 2.0 ** 29 + 0.25
    out = wc.run("sincos", far[:, None, :])
    worst.append(max(sincos_ulps(far[t], out[t, 2], out[t, 3]) for t in range(4)))
    return worst


def test_sincos_reduced_and_the_library_path(wc):
    worst = measure_sincos(wc)
    for (b, tol, _), w in zip(SINCOS_RANGES, worst):
        assert w < tol, (b, w)
    assert worst[-1] < LIBRARY_ULPS, worst[-1]
    # multiples of pi/2 and their neighbourhoods: quadrant bookkeeping, both signs
    x = np.array([k * (math.pi / 2) + d for k in range(-41, 42) for d in (0.0, 1e-9, -1e-9)])
    out = wc.lanes("sincos", x)
    assert np.all(np.abs(out[0] - np.sin(x)) < 4e-16) and np.all(np.abs(out[1] - np.cos(x)) < 4e-16)


# ------------------------------------------------------------------------------------------ device against emulator -
def cross_lane_cases():
    """(body, inputs [ntrial][nin][64]) for every cross-lane body, the inputs of the tests above."""
    rng = np.random.default_rng(26)
    c = [("wave_sum", np.array([v for _, v in sum_cases(False)])[:, None, :]),
         ("wave_sum_f32", np.array([v for _, v in sum_cases(True)])[:, None, :]),
         ("dpp_take", dpp_inputs()),
         ("shfl", shfl_inputs()),
         ("mfma1", mfma_inputs(3, rng)),
         ("mfma4", np.concatenate([mfma_inputs(2, rng), mfma_inputs(2, rng)], axis=1))]
    x = rng.normal(size=(len(READLANE_SOURCES), 2, 64))
    x[:, 1, :] = np.array(READLANE_SOURCES)[:, None]
    c.append(("readlane", x))
    x = rng.normal(size=(2, 3, 64))
    x[:, 2, :] = rng.normal(size=(2, 1))
    c.append(("writelane", x))
    c.append(("from_upper_half", rng.normal(size=(2, 1, 64))))
    c.append(("ballot", np.array(list(BALLOT_PATTERNS.values()), dtype=np.float64)[:, None, :]))
    pairs = np.array([(a, b) for a in MAX_VALUES for b in MAX_VALUES] + [(1.0, 1.0)] * 47)
    c.append(("max_raw", pairs.T.reshape(2, 2, 64).transpose(1, 0, 2)))
    return c


@pytest.mark.gpu
def test_device_cross_lane_bits_are_the_emulators():
    """Every cross-lane primitive gives the emulator's bits: the emulator runs the program the device runs."""
    dev, emu = _wave_check("device"), _wave_check("emu")
    for name, x in cross_lane_cases():
        a, b = dev.run(name, x), emu.run(name, x)
        assert np.all(same_bits(a, b)), (name, np.argwhere(~same_bits(a, b))[:4])
