"""Normaliser rows (csrc/norm_kernels.h) on the wave emulator against the definition restated in numpy (tests/norm_check.py), BIT FOR BIT on
every word: the state, the two outputs, mb, the counts, every partial and the statistics.  Also: both load paths, the grid, the values
that are not finite, the Chan merge over three updates, a per-policy-step source, a checkpoint restored, every refusal by its message, and
the restatement against exact rational arithmetic inside the textbook bound of recursive summation."""
import fractions

import numpy as np
import pytest

import norm_cases as cases
import norm_check as nc
import norm_emu_py as ne
from cassie_amd import phys as P

F32, F64 = np.float32, np.float64
STEPS, ROWS = 3, 50


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    ne.lib()


def run_both(D, block, shift=0, grid=0, steps=STEPS, rows=ROWS):
    """Three updates of a case on the emulator and by the restatement -> (the emulator's run, per update (its snapshot, the restatement's))."""
    src = cases.Source(D, steps, rows, shift)
    e, r = ne.Norm(D, block), cases.Ref(D, block)
    e.bind_source(*src.bind_args(), keep=src)
    out = []
    for x in cases.datasets(D, steps, rows):
        src.fill(x)
        out.append((e.update(grid), r.update(src.dense())))
    return e, out


@pytest.mark.parametrize("block", cases.BLOCKS)
@pytest.mark.parametrize("D", cases.DIMS)
def test_three_updates(D, block):
    """Three updates in a row with different data through padded strides whose padding holds NaN: n, mean and m2 carry over (the Chan
    merge).  block 64: three blocks, the last short, one astride a step; 16: ten blocks; 4096: one block."""
    e, out = run_both(D, block)
    assert e.info["vec"] == (D % 4 == 0) and e.info["R"] == STEPS * ROWS and e.info["blocks"] == -(-STEPS * ROWS // block)
    for k, (got, want) in enumerate(out):
        assert cases.differing(got, want) == [], "update %d" % k
    assert np.all(np.isfinite(out[-1][0]["mean"])) and np.all(np.isfinite(out[-1][0]["m2"]))   # (no padding word, no NaN env reached a sum)


@pytest.mark.parametrize("D", [d for d in cases.DIMS if d % 4 == 0])
def test_word_path_gives_the_same_bits(D):
    """The pointer moved by one word forces the word path on a D that otherwise goes 16 bytes a lane: the same bits."""
    e16, out16 = run_both(D, 64)
    e4, out4 = run_both(D, 64, shift=1)
    assert (e16.info["vec"], e4.info["vec"]) == (1, 0)
    for (g16, _), (g4, want) in zip(out16, out4):
        assert cases.differing(g4, want) == [] and cases.differing(g4, g16) == []


@pytest.mark.parametrize("D", (67, 340))
def test_grid_override(D):
    """One workgroup and the launcher's grid: the same bits."""
    e, out = run_both(D, 16)
    assert e.info["grid"] > 1
    _, one = run_both(D, 16, grid=1)
    for (g, _), (g1, want) in zip(out, one):
        assert cases.differing(g1, want) == [] and cases.differing(g1, g) == []


def test_first_update_is_the_batch_itself():
    """The first update of a column gives mean' = mb and m2' = S2 exactly (w = 1, n * w = 0)."""
    _, out = run_both(67, 64)
    got = out[0][0]
    upd = got["counts"] > 0
    assert upd.sum() == 66
    assert nc.same_bits(got["mean"][upd], got["mb"][upd]) and nc.same_bits(got["m2"][upd], nc.chain(got["a2"])[upd])
    assert nc.same_bits(got["n"], got["counts"])


def test_not_finite_values():
    """A column that is never finite is skipped: its state and its two output words stay untouched; skipped and excluded are exact.  The
    env that is NaN throughout and the scattered NaN, +inf and -inf are excluded from every other column and poison none."""
    D = 130
    _, out = run_both(D, 64)
    R = STEPS * ROWS
    excluded = np.zeros(D)
    for k, x in enumerate(cases.datasets(D, STEPS, ROWS)):
        got = out[k][0]
        bad = (~np.isfinite(x.reshape(R, D))).sum(axis=0)
        excluded += bad
        dead = cases.COL_DEAD
        assert bad[dead] == R and got["skipped"][dead] == k + 1 and got["excluded"][dead] == 0 and got["n"][dead] == 0
        assert got["mean"][dead] == 0 and got["m2"][dead] == 0 and got["out_mean"][dead] == ne.FILL and got["out_inv"][dead] == ne.FILL
        live = np.arange(D) != dead
        assert np.all(bad[live] >= STEPS) and np.all(got["counts"][live] == R - bad[live])           # (the NaN env, at least)
        assert np.all(got["excluded"][live] == excluded[live]) and np.all(got["skipped"][live] == 0)
        assert np.all(np.isfinite(got["out_mean"][live])) and np.all(np.isfinite(got["out_inv"][live]))
        assert got["stats"][2] == D - 1 and got["stats"][3] == 1 and got["stats"][4] == bad[live].sum() and got["stats"][5] == k + 1


def test_constant_and_huge_columns():
    """A constant column gives var = 0 and inv = 1 / sqrt(eps); so does a constant column of 3e38 -- nothing overflows -- and a column of
    +-3e38 stays finite."""
    D, R = 5, STEPS * ROWS
    src = cases.Source(D, STEPS, ROWS)
    x = np.array(cases.datasets(D, STEPS, ROWS)[0])
    x[:, :, 3] = F32(3e38)
    x[:, :, 4] = F32(-3e38)
    src.fill(x)
    e, r = ne.Norm(D, 64), cases.Ref(D, 64)
    e.bind_source(*src.bind_args(), keep=src)
    got, want = e.update(), r.update(src.dense())
    assert cases.differing(got, want) == []
    flat = F32(F64(1.0) / np.sqrt(F64(cases.EPS)))
    for col, value in ((cases.COL_CONST, 1.25), (3, 3e38), (4, -3e38)):
        assert got["m2"][col] == 0 and got["out_inv"][col] == flat and got["out_mean"][col] == F32(value), col
    huge = cases.COL_HUGE
    assert np.isfinite(got["m2"][huge]) and got["m2"][huge] > 1e78 and abs(got["mean"][huge]) < 3e38 and got["out_inv"][huge] > 0


def test_per_policy_step_source():
    """steps = 1: one policy step's live observation as the source, updated eight times."""
    D, rows = 67, 50
    src = cases.Source(D, 1, rows)
    e, r = ne.Norm(D, 16), cases.Ref(D, 16)
    e.bind_source(*src.bind_args(), keep=src)
    for seed in range(8):
        src.fill(cases.data(D, 1, rows, 10 + seed))
        got, want = e.update(), r.update(src.dense())
    assert cases.differing(got, want) == [] and got["stats"][5] == 8 and got["n"].max() <= 8 * rows


def test_checkpoint():
    """Download, upload into a fresh state and write reproduce the output words; a further update from there equals the uninterrupted run."""
    D = 130
    src = cases.Source(D, STEPS, ROWS)
    sets = cases.datasets(D, STEPS, ROWS)
    a, b = ne.Norm(D, 64), ne.Norm(D, 64)
    for e in (a, b):
        e.bind_source(*src.bind_args(), keep=src)
    for x in sets[:2]:
        src.fill(x)
        before = a.update()
    kinds = (P.NORM_N, P.NORM_MEAN, P.NORM_M2, P.NORM_SKIPPED, P.NORM_EXCLUDED)
    for what in kinds:
        b.region(what, upload=True)[:] = a.region(what)
    assert b.region(P.NORM_MB, upload=True) is None and b.region(P.NORM_PARTIALS, upload=True) is None and a.region(8) is None
    b.write()
    dead = cases.COL_DEAD
    assert b.mean[dead] == ne.FILL and b.inv[dead] == ne.FILL                               # (n = 0: not written)
    assert nc.same_bits(b.mean, before["out_mean"]) and nc.same_bits(b.inv, before["out_inv"])
    src.fill(sets[2])
    b.a.calls = a.a.calls
    assert cases.differing(b.update(), a.update()) == []


def test_resolved_source_and_output():
    """Unbound, the source is the rollout's OBS store with steps = T and rows = nenv, the outputs the policy's bound normalisation."""
    D = 67
    src = cases.Source(D, STEPS, ROWS)
    src.fill(cases.datasets(D, STEPS, ROWS)[0])
    e, r = ne.Norm(D, 64, bind_output=False), cases.Ref(D, 64)
    e.rollout(STEPS, ROWS, D, src.buf, src.step_stride, src.row_stride)
    e.policy(D)
    assert cases.differing(e.update(), r.update(src.dense())) == []


def test_refusals():
    """Every refusal by its message."""
    for args, msg in (((0, 64), "not configured"), ((513, 64), "dim lies in 1 .. 512"), ((-1, 64), "dim lies in 1 .. 512"),
                      ((5, 8), "block is a multiple of 16"), ((5, 72), "block is a multiple of 16"), ((5, 8192), "block is a multiple of 16"),
                      ((5, 64, 0), "max_rows lies in"), ((5, 64, (1 << 30) + 1), "max_rows lies in"),
                      ((5, 64, 100, 0.0), "eps is finite and > 0"), ((5, 64, 100, np.inf), "eps is finite and > 0"), ((5, 64, 100, np.nan), "eps is finite and > 0")):
        e = ne.Norm(*args)
        assert not e.ok and msg in ne.refusal(), (args, ne.refusal())
    D = 5
    src = cases.Source(D, STEPS, ROWS)
    src.fill(cases.datasets(D, STEPS, ROWS)[0])

    def fresh(**kw):
        e = ne.Norm(D, 64, **kw)
        e.bind_source(*src.bind_args(), keep=src)
        return e
    e = fresh(max_rows=STEPS * ROWS - 1)
    assert "more samples than max_rows" in e.try_update()
    e = fresh(max_rows=STEPS * ROWS)
    assert e.try_update() is None
    e = fresh()
    e.a.row_stride = D - 1
    assert "strides of at least dim words" in e.try_update()
    e = fresh()
    e.a.step_stride = D - 1
    assert "strides of at least dim words" in e.try_update()
    e = fresh()
    e.a.steps = 0
    assert "at least one step" in e.try_update()
    e = fresh()
    e.a.out_inv = None
    assert "both or neither" in e.try_update() and "both or neither" in e.try_write()
    # unresolved: no rollout, no OBS source, an OBS source of another dim; no policy, no bound normalisation, another in_dim
    e = ne.Norm(D, 64)
    assert "no rollout is configured" in e.try_update()
    e.rollout(STEPS, ROWS, 0)
    assert "no OBS source" in e.try_update()
    e.rollout(STEPS, ROWS, D + 1, src.buf, src.step_stride, src.row_stride)
    assert "does not have dim words" in e.try_update()
    e.rollout(STEPS, ROWS, D, src.buf, src.step_stride, src.row_stride)
    assert e.try_update() is None
    e = fresh(bind_output=False)
    assert "no normalisation bound" in e.try_update() and "no normalisation bound" in e.try_write()
    e.policy(D, bound=False)
    assert "no normalisation bound" in e.try_update()
    e.policy(D + 1)
    assert "in_dim is not dim" in e.try_update() and "in_dim is not dim" in e.try_write()
    e.policy(D)
    assert e.try_update() is None and e.try_write() is None


def test_exact_reference():
    """The smallest case (R = 150, D = 5) against exact rational arithmetic over the finite values.  Recursive summation of m terms in
    blocks errs by at most (m - 1) u sum |x| to first order, u = 2^-53; with the chain over the blocks, the division and the second-order
    terms, (R + 8) u sum |x| bounds the sum's error, and the mean's error is that over M plus one rounding.  m2 sums the rounded squares of
    the rounded differences from the rounded mean: each term carries three roundings, the sum by
    (R + 8) u sum d^2 more, and a mean off by dmb moves the exact sum of squares about it by M dmb^2 -- all computed from the data.  The
    float32 outputs lie within half a float32 ulp more."""
    D, block, R = 5, 64, STEPS * ROWS
    x = cases.datasets(D, STEPS, ROWS)[0].reshape(R, D)
    r = cases.Ref(D, block)
    got = r.update(x)
    u, Fr = fractions.Fraction(1, 2 ** 53), fractions.Fraction
    for j in range(D):
        vals = [Fr(float(v)) for v in x[:, j] if np.isfinite(v)]
        if not vals:
            assert j == cases.COL_DEAD and got["n"][j] == 0
            continue
        M = len(vals)
        assert got["n"][j] == M
        mean = sum(vals) / M
        bound_sum = (R + 8) * u * sum(abs(v) for v in vals)
        dmb = abs(Fr(float(got["mean"][j])) - mean)
        bound_mean = bound_sum / M + u * abs(mean)
        assert dmb <= bound_mean, (j, float(dmb), float(bound_mean))
        m2 = sum((v - mean) ** 2 for v in vals)
        moved = M * bound_mean ** 2                                 # (the sum of squares about a mean off by at most bound_mean)
        bound_m2 = (R + 8 + 4) * u * (m2 + moved) + moved
        err_m2 = abs(Fr(float(got["m2"][j])) - m2)
        assert err_m2 <= bound_m2, (j, float(err_m2), float(bound_m2))
        # the outputs: (float) mean is the mean's bound and half a float32 ulp of the computed mean away; inv comes from a variance within
        # bound_m2 / M through a function of relative slope 1/2 and four roundings, and half a float32 ulp (2^-150 where it is subnormal)
        half32 = Fr(1, 2 ** 24)
        om = Fr(float(got["out_mean"][j]))
        assert abs(om - mean) <= bound_mean + half32 * (abs(mean) + bound_mean), j
        var = m2 / M
        inv_exact = 1.0 / np.sqrt(float(var) + cases.EPS)          # (float64 from the exact variance: four roundings of its own)
        rel = float(bound_m2 / M) / (float(var) + cases.EPS) / 2 + 8 * float(u)
        assert abs(float(got["out_inv"][j]) - inv_exact) <= inv_exact * rel + max(inv_exact * (1 + rel) * float(half32), 2.0 ** -150), j
