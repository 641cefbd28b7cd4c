"""Draw rows (csrc/draw_kernels.h, csrc/logn.h) on the wave emulator against the definition restated in numpy (tests/draw_check.py), BIT FOR
BIT on every word: the normal rows, the counts, the permutation.  Also: Philox's known answer, logn and the Box-Muller value against
mpmath at 60 digits, independence of the range cuts and the grid, both store widths, words nobody may touch, the wrap of the count, the
shuffle's bijection and its bounded walk, the sanity of both definitions as distributions, and every refusal by its message."""
import itertools
import math

import numpy as np
import pytest

import draw_cases as cases
import draw_check as dc
import draw_emu_py as de
import obs_check
from cassie_amd import phys as P

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    de.lib()


# ---- the pieces ----

def test_philox_known_answer():
    """Counter 0, key 0: 6627e8d5 e169c58d bc57ac4c 9b00dbd8 -- by the Python-integer restatement, the numpy one and the kernels' routine."""
    want = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert obs_check.philox4x32_10((0, 0, 0, 0), (0, 0)) == want
    assert tuple(int(v) for v in dc.philox(0, 0, 0, 0, 0)) == want
    assert de.philox((0, 0, 0, 0), (0, 0)) == want
    rng = np.random.default_rng(5)
    for _ in range(20):
        c, seed = [int(v) for v in rng.integers(0, 1 << 32, size=4)], int(rng.integers(0, 1 << 63)) * 2 + 1
        key = (seed & 0xFFFFFFFF, seed >> 32)
        assert tuple(int(v) for v in dc.philox(*c, seed)) == obs_check.philox4x32_10(c, key) == de.philox(c, key)


def logn_words():
    """The words of the issue's points: the ends, the middle, 20 000 random words, 2 000 within 4096 of each end."""
    rng = np.random.default_rng(11)
    edge = [0, 1, 2, 3, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1]
    return np.concatenate([np.array(edge, dtype=np.uint64), rng.integers(0, 1 << 32, size=20000, dtype=np.uint64),
                           rng.integers(0, 4096, size=2000, dtype=np.uint64), np.uint64(2 ** 32 - 1) - rng.integers(0, 4096, size=2000, dtype=np.uint64)])


def test_logn_and_the_draw_against_mpmath():
    """logn(u), rad and (float) z against mpmath at 60 digits on u = (w + 0.5) 2^-32.  The bound 2^-40 on the relative error of logn and of
    rad is derived: a relative error below 2^-25 in fp64 leaves (float) z within one float32 ulp of the exact Box-Muller value of the same
    words -- which is asserted too, with mpmath's own sin and cos of 2 pi theta.  Measured here (printed below; DESIGN 4.3 has them):
    logn 2^-52.05, rad 2^-52.23, (float) z 0.4999960 ulp.  The emulator's logn and pair equal the restatement's in every bit."""
    import mpmath
    mpmath.mp.dps = 60
    a = logn_words()
    rng = np.random.default_rng(12)
    b = rng.integers(0, 1 << 32, size=a.size, dtype=np.uint64)
    b[:9] = [0, 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31, 2 ** 31 - 1, 3 * 2 ** 30, 2 ** 32 - 1, 2 ** 29]      # theta at and next to the quadrants' ends
    u, rad = dc.radius(a)
    ln = dc.logn(u)
    zc, zs = dc.pair(a, b)
    assert cases.same_bits(de.logn(u), ln)
    ec, es = de.pair(a, b)
    assert cases.same_bits(ec, zc) and cases.same_bits(es, zs)
    top = math.sqrt(66 * math.log(2)) * (1 + 2.0 ** -50)           # (w = 0: u = 2^-33, the radius sqrt(66 ln 2) but for its roundings)
    assert np.all((u > 0) & (u < 1)) and np.all(np.abs(zc) <= top) and np.all(np.abs(zs) <= top)
    worst_ln = worst_rad = worst_z = 0.0
    two_pi = 2 * mpmath.pi
    for i in range(a.size):
        t = mpmath.log(mpmath.mpf(int(a[i])) + mpmath.mpf("0.5")) - 32 * mpmath.log(2)
        r = mpmath.sqrt(-2 * t)
        worst_ln = max(worst_ln, float(abs((mpmath.mpf(float(ln[i])) - t) / t)))
        worst_rad = max(worst_rad, float(abs((mpmath.mpf(float(rad[i])) - r) / r)))
        th = two_pi * mpmath.mpf(int(b[i])) / 2 ** 32
        for got, exact in ((zc[i], r * mpmath.cos(th)), (zs[i], r * mpmath.sin(th))):
            ulp = mpmath.mpf(2) ** max(int(mpmath.floor(mpmath.log(abs(exact), 2))) - 23, -149) if exact != 0 else mpmath.mpf(2) ** -149
            worst_z = max(worst_z, float(abs(mpmath.mpf(float(F32(got))) - exact) / ulp))
    print("logn: worst relative error 2^%.2f; rad: 2^%.2f; (float) z: %.7f ulp" % (math.log2(worst_ln), math.log2(worst_rad), worst_z))
    assert worst_ln <= 2.0 ** -40 and worst_rad <= 2.0 ** -40
    assert worst_z <= 1.0


def test_logn_special_values_and_the_whole_range():
    """The selects: a NaN gives NaN, x < 0 NaN, +-0.0 -inf, +inf +inf; logn(1) = +0.0; powers of two, subnormals and the largest double
    lie within 2^-50 of libm's; the emulator equals the restatement in every bit."""
    x = np.array([np.nan, -1.0, -np.inf, 0.0, -0.0, np.inf, 1.0], dtype=F64)
    for got in (dc.logn(x), de.logn(x)):
        assert np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(got[2]) and got[3] == -np.inf and got[4] == -np.inf and got[5] == np.inf
        assert got[6] == 0.0 and not np.signbit(got[6])
    rng = np.random.default_rng(13)
    y = np.concatenate([2.0 ** np.arange(-1074, 1024, 7, dtype=F64), [5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308],
                        np.nextafter(1.0, 0) * np.ones(1), np.nextafter(1.0, 2) * np.ones(1), np.sqrt(2.0) * np.ones(1), np.nextafter(np.sqrt(2.0), 0) * np.ones(1),
                        np.exp(rng.uniform(-700, 700, size=2000))])
    got = dc.logn(y)
    assert cases.same_bits(de.logn(y), got)
    assert np.all(np.abs(got - np.log(y)) <= 2.0 ** -50 * np.abs(np.log(y)))


# ---- the normal rows: the emulator equals the restatement ----

def emu_case(nenv, A, **kw):
    stride, env_base, seed = cases.case(nenv, A)
    return de.Draw(nenv, A, 0, seed, env_base, stride, fill=cases.SENTINEL, **kw)


@pytest.mark.parametrize("A", cases.WIDTHS)
@pytest.mark.parametrize("nenv", cases.NENVS)
def test_three_calls(nenv, A):
    """Three calls in a row over the whole batch through a row stride larger than A with env_base != 0: every word of the rows -- the
    sentinel past column A included -- and the counts."""
    rows, counts = cases.reference(nenv, A)
    e = emu_case(nenv, A)
    for k in range(cases.CALLS):
        assert cases.same_bits(e.draw(), rows[k]), (nenv, A, k)
    assert cases.same_bits(e.counts, counts) and np.all(e.counts == cases.CALLS)
    assert e.info["lanes"] * e.info["per_wave"] == 64 and 4 * e.info["lanes"] >= A
    stride = cases.case(nenv, A)[0]
    assert e.info["vec"] == (1 if stride % 4 == 0 and e.rows.ctypes.data % 16 == 0 else 0)     # (A = 1, 5: a stride of 4, 8 words)


@pytest.mark.parametrize("A", (10, 64))
def test_range_cuts_in_any_order(A):
    """The batch drawn as one range and as the ranges (0, 17), (17, 47), (64, rest) in any order: the same words; envs 47 .. 63, which no
    range names, keep the sentinel and their count."""
    nenv = 130
    rows, _ = cases.reference(nenv, A)
    for order in itertools.permutations(cases.cut_ranges(nenv)):
        e = emu_case(nenv, A)
        for env0, n in order:
            e.draw(env0, n)
        want = rows[0].copy()
        want[47:64] = cases.SENTINEL
        assert cases.same_bits(e.rows, want), order
        assert np.all(e.counts[:47] == 1) and np.all(e.counts[47:64] == 0) and np.all(e.counts[64:] == 1)
        e.draw(47, 17)
        assert cases.same_bits(e.rows, rows[0])


@pytest.mark.parametrize("grid", (1, 3, 1000))
def test_any_grid(grid):
    rows, _ = cases.reference(130, 10)
    e = emu_case(130, 10)
    assert cases.same_bits(e.draw(grid=grid), rows[0])
    assert cases.same_bits(e.draw(grid=grid), rows[1])


@pytest.mark.parametrize("A", (4, 64))
def test_both_store_widths(A):
    """A destination that begins a word behind a 16-byte boundary takes the same words a word at a time."""
    nenv = 65
    rows, _ = cases.reference(nenv, A)
    stride = cases.case(nenv, A)[0]
    e = emu_case(nenv, A)
    raw = np.full(nenv * stride + 8, cases.SENTINEL, dtype=F32)
    at = (-(raw.ctypes.data // 4)) % 4 + 1
    e.rows = raw[at: at + nenv * stride].reshape(nenv, stride)
    e.a.dst = e.rows.ctypes.data
    assert cases.same_bits(e.draw(), rows[0]) and e.info["vec"] == 0
    assert raw[at - 1] == cases.SENTINEL and raw[at + nenv * stride] == cases.SENTINEL


def test_empty_range_and_the_count_wraps():
    nenv, A = 65, 5
    stride, env_base, seed = cases.case(nenv, A)
    e, r = emu_case(nenv, A), dc.Draws(nenv, A, seed, env_base, stride, fill=cases.SENTINEL)
    e.draw(10, 0)
    assert np.all(e.rows == cases.SENTINEL) and np.all(e.counts == 0)
    e.counts[:] = r.counts[:] = 0xFFFFFFFF                      # (set_draw_state)
    e.counts[3] = r.counts[3] = 12345
    assert cases.same_bits(e.draw(), r.draw())
    assert e.counts[0] == 0 and e.counts[3] == 12346 and cases.same_bits(e.counts, r.counts)
    assert cases.same_bits(e.draw(), r.draw())


def test_default_destination_is_the_policys_eps():
    """Nothing bound: the rows go where the policy's sample binding says, with its stride."""
    nenv, A = 65, 3
    rows, _ = cases.reference(nenv, A)
    e = emu_case(nenv, A, bind=False)
    e.policy(A)
    assert cases.same_bits(e.draw(), rows[0])


# ---- the shuffle ----

@pytest.mark.parametrize("n", cases.PERM_NS)
def test_shuffle(n):
    """Epochs 0 and 1: a bijection of [0, n); they differ for n >= 64; the emulator equals the restatement for n <= 4097; the longest walk
    stays inside the derived bound 2^b - n + 1."""
    h = dc.perm_half(n)
    bound = (1 << (2 * h)) - n + 1
    assert (1 << (2 * h)) >= max(n, 4) and (h == 1 or (1 << (2 * h - 2)) < n) and bound <= max(3 * n, 4)
    perms = []
    for epoch in (0, 1):
        p, walk = cases.perm_reference(n, epoch)
        print("n %d epoch %d: longest walk %d (bound %d)" % (n, epoch, walk, bound))
        assert walk <= bound
        assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(n))
        perms.append(p)
        if n <= cases.PERM_EMU_MAX:
            e = de.Draw(1, 0, n, cases.SEED)
            assert cases.same_bits(e.draw_perm(epoch), p)
            assert e.pinfo["h"] == h and e.pinfo["walk_max"] == bound
    if n >= 64:
        assert not np.array_equal(perms[0], perms[1])


def test_shuffle_any_grid_and_a_bound_tensor():
    n = 1000
    p, _ = cases.perm_reference(n, 1)
    e = de.Draw(1, 0, n, cases.SEED)
    assert cases.same_bits(e.draw_perm(1, grid=1), p)
    mine = np.full(n + 2, -5, dtype=np.int32)
    e.perm[:] = -1
    e.a.perm_dst = mine[1:].ctypes.data
    e.draw_perm(1, grid=5)
    assert cases.same_bits(mine[1:-1], p) and mine[0] == -5 and mine[-1] == -5 and np.all(e.perm == -1)
    other, _ = cases.perm_reference(n, 1, seed=cases.SEED + 1)
    assert not np.array_equal(other, p)


# ---- the sanity of the definition (the restatement; deterministic) ----

def normal_cdf(x):
    return np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x])


@pytest.mark.parametrize("shape", ((256, 10, 16), (4096, 10, 1)))
@pytest.mark.parametrize("seed", (1, 2, 0x0123456789ABCDEF))
def test_normal_rows_look_normal(seed, shape):
    """n = 40 960 values: mean, variance, Kolmogorov-Smirnov distance and the largest correlation between two columns, each scaled to a
    standard deviation or a critical value (bounds of the issue; the largest seen with libm's log: 1.81, 1.31, 1.32, 3.19)."""
    nenv, A, calls = shape
    r = dc.Draws(nenv, A, seed)
    x = np.concatenate([r.draw().copy() for _ in range(calls)]).astype(F64)
    n, N = x.size, x.shape[0]
    assert n == 40960 and np.all(np.isfinite(x))
    mean, var = x.mean(), x.var()
    xs = np.sort(x.reshape(-1))
    cdf = normal_cdf(xs)
    ks = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(0, n) / n))
    corr = np.corrcoef(x, rowvar=False)
    off = np.max(np.abs(corr - np.eye(A)))
    figures = (abs(mean) * math.sqrt(n), abs(var - 1) * math.sqrt(n / 2), ks * math.sqrt(n), off * math.sqrt(N))
    print("seed %x shape %s: mean %.2f var %.2f ks %.2f corr %.2f" % ((seed, shape) + figures))
    assert figures[0] <= 4 and figures[1] <= 4 and figures[2] <= 1.95 and figures[3] <= 4.5


@pytest.mark.parametrize("seed", (7, 8))
def test_minibatches_mix_the_index_range(seed):
    """n = 4096, 64 epochs, minibatches of 1024: the 4 x 4 table minibatch k x quarter of the index range against equal cells; chi-square
    below 27.9 (9 degrees of freedom at p = 0.001; seen with this definition: below 10)."""
    n, M = 4096, 1024
    table = np.zeros((4, 4))
    for epoch in range(64):
        p = dc.perm(n, epoch, seed)
        for k in range(4):
            table[k] += np.bincount(p[k * M: (k + 1) * M] // M, minlength=4)
    expect = 64 * M / 4
    chi2 = float(np.sum((table - expect) ** 2 / expect))
    print("seed %d: chi-square %.2f" % (seed, chi2))
    assert chi2 < 27.9


# ---- the refusals ----

def test_refusals():
    """Each refusal by its message, and nothing is launched: the sentinel and the counts stay."""
    assert de.Draw(4, 0, 0).why == "not configured (phys_batch_draw_configure first)"
    assert "A lies in 1 .. 64" in de.Draw(4, 65, 0).why and "A lies in 1 .. 64" in de.Draw(4, -1, 0).why
    assert "perm_n lies in 1 .. 2^30" in de.Draw(4, 3, (1 << 30) + 1).why and "perm_n lies in 1 .. 2^30" in de.Draw(4, 3, -1).why
    assert de.Draw(4, 64, 1 << 30).why is None
    e = de.Draw(8, 3, 0, fill=cases.SENTINEL)
    for env0, n in ((0, 9), (8, 1), (-1, 2), (2, -1)):
        assert e.try_draw(env0, n) == "env range out of bounds"
    e = de.Draw(8, 3, 0, fill=cases.SENTINEL, bind=False)
    assert e.try_draw().startswith("no destination")
    e.policy(3, bound=False)
    assert e.try_draw().startswith("no destination")
    e.policy(4)
    assert e.try_draw() == "the actor's output width is not A"
    assert np.all(e.rows == cases.SENTINEL) and np.all(e.counts == 0)
    e = de.Draw(8, 3, 0, stride=2, fill=cases.SENTINEL)
    assert e.try_draw() == "a row stride of at least A"
    assert de.Draw(8, 3, 0).try_perm(0) == "no shuffle is configured (perm_n is 0)"
    e = de.Draw(8, 0, 16, fill=cases.SENTINEL)
    e.a.dst = None
    assert e.try_draw() == "no normal rows are configured (A is 0)" and e.try_perm(0) is None
    assert (P.DRAW_MAXA, P.DRAW_MAXPERM) == (64, 1 << 30)
