"""Task rows (phys_batch_task, include/cassie_phys.h: held random commands and pushes, gait clocks, their waveforms and the row of a
reference trajectory in one launch) on the CPU wave emulator: cassie_task_kernel launched through the launcher's own records, grid and
checks (csrc/small_launch.h) against the definition restated in numpy and Python integers (tests/task_check.py), BIT FOR BIT -- every
step of a column's value is one individually rounded operation -- and the launch rules one by one.  All comparisons are on IEEE bits, a
NaN equal to a NaN.  The GPU counterpart is tests/test_task_gpu.py."""
import numpy as np
import pytest

import obs_check as oc
import task_cases as cases
import task_check as tc
import task_emu_py as te
from cassie_amd import phys as P

DTYPES = [np.float64, np.float32]
FILL = -7.25
# the worst error of sin2pi / cos2pi against the exact value, in ulp of the exact value, over the points of sincos_points(): measured
# 1.652 (sin) and 1.702 (cos), rounded up to the next half ulp
SINCOS_ULP_BOUND = 2.0


@pytest.fixture(scope="module")
def cols(cassie):
    return cases.columns_of(cassie.pod)


@pytest.fixture(scope="module")
def table():
    return cases.make_table()


@pytest.fixture(scope="module")
def start(cassie):
    return cases.start_fields(cassie)


@pytest.fixture(scope="module")
def want(cols, table, start):
    """The reference of the shared case in both dtypes (computed once, left unchanged)."""
    return {dt: cases.reference(cols, table, dt, start) for dt in DTYPES}


def run_emulator(cols, table, dtype, start, schedule=cases.SCHEDULE, nenv=cases.NENV, env_base=0, pad=4, grid=0, seed=cases.SEED, begin=None):
    """The schedule on the emulator: rows with a stride `pad` elements beyond the row, xfrc_applied a column block of a wider array ->
    [(rows, state, words, counts, {field: array})] after every call, the raw row buffer and the wide array, whose gaps hold FILL."""
    ncols = len(cols)
    raw = np.full((nenv, ncols + pad), FILL, dtype=dtype)
    state, words, counts = np.zeros((nenv, ncols)), np.zeros((nenv, 3, ncols), dtype=np.uint32), np.zeros(nenv, dtype=np.uint32)
    if begin is not None:
        state[:], words[:], counts[:] = begin
    held = {f: a.copy() for f, a in start.items()}
    nx = held[P.F_XFRC_APPLIED].shape[1]
    wide = np.full((nenv, nx + 3), FILL)
    wide[:, 2: 2 + nx] = held[P.F_XFRC_APPLIED]
    held[P.F_XFRC_APPLIED] = wide[:, 2: 2 + nx]
    out = []
    for env0, n, reset in schedule:
        te.Call(held, nenv, cols, dtype, seed, env_base, table=table, rows=raw, state=state, words=words, counts=counts).task(env0, n, reset, grid)
        out.append((raw[:, :ncols].copy(), state.copy(), words.copy(), counts.copy(), {f: np.ascontiguousarray(held[f]).copy() for f in cases.DEST_FIELDS}))
    return out, raw, wide


def same_call(got, want):
    return (oc.same_bits(got[0], want[0]) and oc.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
            and all(oc.same_bits(got[4][f], want[4][f]) for f in cases.DEST_FIELDS))


def test_the_case_reaches_every_branch(cassie, want, table):
    """Conditions on the shared case, in the numpy restatement: every SAMPLE column draws and holds, rests and does not rest; a push is
    shown and hidden; a clock wraps; a TABLE column lands in the last frame, so that its second frame is frame 0; a reset is seen."""
    ref = want[np.float64]
    drew = np.stack([r[5] for r in ref])
    resting = np.stack([r[6] for r in ref])
    wrapped = np.stack([r[7] for r in ref])
    ran = np.zeros(drew.shape[:2], dtype=bool)
    for k, (env0, n, _) in enumerate(cases.SCHEDULE):
        ran[k, env0: env0 + n] = True
    for c in cases.SAMPLES:
        assert (drew[:, :, c] & ran).any() and (~drew[:, :, c] & ran).any(), c
        assert (resting[:, :, c] & drew[:, :, c]).any() and (~resting[:, :, c] & drew[:, :, c]).any(), c
    # draws that no first call and no reset caused: a period ran out
    plain = [k for k, (_, _, reset) in enumerate(cases.SCHEDULE) if k > 0 and reset is None]
    for c in cases.SAMPLES:
        assert drew[plain][:, :, c].any(), c
    # every period length of the command group is met: the words right after a draw hold L - 1
    seen = {int(ref[k][2][e, 0, cases.VX]) + 1 for k in range(len(ref)) for e in range(cases.NENV) if drew[k, e, cases.VX]}
    assert seen == {2, 3, 4}
    assert wrapped[:, :, cases.CLOCK].any() and wrapped[:, :, cases.CLOCK2].any()
    last = [(k, e) for k in range(len(ref)) for e in range(cases.NENV) if ran[k, e] and ref[k][1][e, cases.CLOCK2] * cases.NFRAMES >= cases.NFRAMES - 1]
    assert last, "no phase in the table's last frame"
    # a push is non-zero in the call of its draw and 0 in the two that follow; its two columns are on together
    px, py = ref[0][0][:, cases.PUSH_X], ref[0][0][:, cases.PUSH_Y]
    on = np.stack([r[0][:, cases.PUSH_X] != 0 for r in ref])
    assert on.any() and (~on).any() and np.array_equal(on, np.stack([r[0][:, cases.PUSH_Y] != 0 for r in ref]))
    assert np.array_equal(px != 0, py != 0)
    # the reset call draws in the two envs it names, in every SAMPLE column, and in the others only where a period ran out
    k = [i for i, s in enumerate(cases.SCHEDULE) if s[2] is not None][0]
    assert drew[k][[1, 3]][:, list(cases.SAMPLES)].all() and not drew[k][[0, 2, 4]][:, list(cases.SAMPLES)].all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulator_against_the_definition(cassie, cols, table, start, want, dtype):
    """19 columns of every kind over fourteen calls (a first call, periods that run out, a sub-range, a reset): rows, state, words,
    counts and the destination field are the numpy restatement's after every call, bit for bit; envs outside a call's range, the padding
    of the bound rows and every element of xfrc_applied that no column names are untouched."""
    ref = want[dtype]
    got, raw, wide = run_emulator(cols, table, dtype, start)
    for k, (g, w) in enumerate(zip(got, ref)):
        assert np.array_equal(g[3], w[3]), k
        assert np.array_equal(g[2], w[2]), k
        assert oc.same_bits(g[1], w[1]), k
        assert oc.same_bits(g[0], w[0]), k
        for f in cases.DEST_FIELDS:
            assert oc.same_bits(g[4][f], w[4][f]), (k, f)
    assert list(got[-1][3]) == [13, 14, 14, 14, 13]
    assert np.all(raw[:, len(cols):] == dtype(FILL)) and np.all(wide[:, :2] == FILL) and np.all(wide[:, -1:] == FILL)
    px, py = cases.push_elems(cassie.pod)
    rest = [j for j in range(start[P.F_XFRC_APPLIED].shape[1]) if j not in (px, py)]
    for g in got:
        x = g[4][P.F_XFRC_APPLIED]
        assert np.array_equal(x[:, rest], start[P.F_XFRC_APPLIED][:, rest])
        assert oc.same_bits(x[:, px].astype(dtype), g[0][:, cases.PUSH_X]) and oc.same_bits(x[:, py].astype(dtype), g[0][:, cases.PUSH_Y])
    # the sub-range call leaves envs 0 and 4 alone, byte for byte
    k = [i for i, s in enumerate(cases.SCHEDULE) if s[:2] == (1, 3)][0]
    for e in (0, 4):
        assert all(got[k][j][e].tobytes() == got[k - 1][j][e].tobytes() for j in range(4))
        assert got[k][4][P.F_XFRC_APPLIED][e].tobytes() == got[k - 1][4][P.F_XFRC_APPLIED][e].tobytes()
    assert not oc.same_bits(got[k][0][1:4], got[k - 1][0][1:4])
    # the values themselves: finite rows, clocks in [0, 1), the gates in [0, 1], an unscaled saw equal to its clock
    for g in got:
        r = g[0].astype(np.float64)
        assert np.isfinite(r).all() and (r[:, [cases.CLOCK, cases.CLOCK2]] >= 0).all() and (r[:, [cases.CLOCK, cases.CLOCK2]] < 1).all()
        assert (r[:, [cases.GATE, cases.GATE_B]] >= 0).all() and (r[:, [cases.GATE, cases.GATE_B]] <= 1).all()
        assert oc.same_bits(g[0][:, cases.SAW_B], g[0][:, cases.CLOCK2])


def test_grids_give_the_same_bits(cols, table, start, want):
    for grid in (1, 3, 64):
        got, _, _ = run_emulator(cols, table, np.float32, start, grid=grid)
        assert all(same_call(g, w) for g, w in zip(got, want[np.float32])), grid


def test_env_base_cuts_the_batch(cols, table, start, want):
    """Two batches holding envs [0, 3) and [3, 5) with env_base 0 and 3 make what one batch of 5 makes (the draws belong to the env)."""
    sched = tuple((0, 5, r) for _, _, r in cases.SCHEDULE)
    whole = cases.reference(cols, table, np.float64, start, schedule=sched)
    lo, _, _ = run_emulator(cols, table, np.float64, {f: a[:3] for f, a in start.items()}, nenv=3, env_base=0,
                            schedule=tuple((0, 3, None if r is None else r[:3]) for _, _, r in sched))
    hi, _, _ = run_emulator(cols, table, np.float64, {f: a[3:] for f, a in start.items()}, nenv=2, env_base=3,
                            schedule=tuple((0, 2, None if r is None else r[3:]) for _, _, r in sched))
    for a, b, w in zip(lo, hi, whole):
        for j in range(4):
            assert oc.same_bits(np.concatenate([a[j], b[j]]), w[j])
        assert oc.same_bits(np.concatenate([a[4][P.F_XFRC_APPLIED], b[4][P.F_XFRC_APPLIED]]), w[4][P.F_XFRC_APPLIED])


def test_a_group_moves_in_lockstep(cols, table, start):
    """left, age, epoch and the resting pattern of a group's members are the same in every call; their values differ."""
    got, _, _ = run_emulator(cols, table, np.float64, start)
    for group in (cases.COMMAND, cases.PUSH):
        lead = group[0]
        differ = False
        for g in got:
            for c in group[1:]:
                assert np.array_equal(g[2][:, :, c], g[2][:, :, lead])
                assert np.array_equal(g[1][:, c] == 0.0, g[1][:, lead] == 0.0)        # (rest = 0: resting together)
                differ = differ or (g[1][:, c] != g[1][:, lead]).any()
        assert differ
    # two groups are not in step with each other
    assert any(not np.array_equal(g[2][:, :, cases.VX], g[2][:, :, cases.FREQ]) for g in got)


def test_period_lengths_and_the_integer_formula():
    """L takes every value of [period_lo, period_hi] and none outside over a few thousand epochs of the integer formula, and the
    emulator's state holds what the formula gives: a column with period 3 .. 9 run call by call, each epoch's length read off `left`
    right after its draw."""
    seed, lo, hi, env_base = 77, 3, 9, 5
    lengths = [tc.period(tc.schedule_words(seed, env_base, 0, 0, e)[0], lo, hi) for e in range(4000)]
    assert set(lengths) == set(range(lo, hi + 1))
    assert tc.period(0, lo, hi) == lo and tc.period(0xFFFFFFFF, lo, hi) == hi and tc.period(0xFFFFFFFF, 1, 1 << 30) == 1 << 30
    rows, state, words, counts = np.zeros((1, 1)), np.zeros((1, 1)), np.zeros((1, 3, 1), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    call = te.Call({}, 1, [P.task_sample(0.0, 1.0, lo, hi)], np.float64, seed, env_base, rows=rows, state=state, words=words, counts=counts)
    seen, epoch = [], 0
    for _ in range(400):
        before = int(words[0, 0, 0])
        call.task()
        if before == 0:                                     # a draw: left = L - 1 now, epoch the next
            assert int(words[0, 2, 0]) == epoch and int(words[0, 1, 0]) == 1
            seen.append(int(words[0, 0, 0]) + 1)
            assert rows[0, 0] == 0.0 + 1.0 * oc.uniform(tc.value_word(seed, env_base, 0, 0, epoch))
            epoch += 1
    assert seen == lengths[: len(seen)] and len(seen) > 50


def test_p_rest_of_0_never_rests_and_of_1_always(built):
    n = 4
    cols = [P.task_sample(2.0, 0.5, 1, 2, rest=-9.0, p_rest=0.0), P.task_sample(2.0, 0.5, 1, 2, rest=-9.0, p_rest=1.0)]
    rows, state, words, counts = np.zeros((n, 2)), np.zeros((n, 2)), np.zeros((n, 3, 2), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    call = te.Call({}, n, cols, np.float64, 3, rows=rows, state=state, words=words, counts=counts)
    table = call.columns()
    assert int(table["thr"][0]) == 0 and int(table["thr"][1]) == 1 << 32
    for _ in range(200):
        call.task()
        assert (np.abs(rows[:, 0] - 2.0) <= 0.5).all() and (rows[:, 1] == -9.0).all()
    assert int(te.Call({}, 1, [P.task_sample(p_rest=0.3)]).columns()["thr"][0]) == round(0.3 * 2 ** 32) == tc.threshold(0.3)


def sincos_points():
    """64 000 points over [0, 1) -- a grid shifted off the quarter points and random ones -- then points within 1e-9 of every quarter
    (those of 0 and of 1 inside [0, 1)) and within 1e-12 of 0."""
    rng = np.random.default_rng(11)
    pts = [(np.arange(32000) + 0.37) / 32000.0, rng.uniform(0.0, 1.0, 32000)]
    for quarter in (0.0, 0.25, 0.5, 0.75, 1.0):
        d = np.concatenate([rng.uniform(0.0, 1e-9, 250), 10.0 ** rng.uniform(-17, -9, 250)])
        pts.append(quarter + d if quarter < 1.0 else quarter - d)
        if 0.0 < quarter < 1.0:
            pts.append(quarter - d)
    pts.append(10.0 ** rng.uniform(-300, -12, 500))
    pts.append(np.array([5e-324, 2.0 ** -1022, 1.0 - 2.0 ** -53, 0.125, 0.375, 0.625, 0.875, np.nextafter(0.125, 0), np.nextafter(0.125, 1)]))
    t = np.concatenate(pts)
    t = t[(t >= 0.0) & (t < 1.0)]
    quarters = np.isin(t, (0.0, 0.25, 0.5, 0.75))
    return t[~quarters]


def test_sin2pi_and_cos2pi():
    """The emulator and the numpy restatement agree on every point; the worst error against a 60-digit reference, in ulp of the exact
    value, is inside the bound measured for these points (rounded up to the next half ulp); the quarter points give 0 and +-1."""
    import mpmath
    mpmath.mp.dps = 60
    t = sincos_points()
    assert t.size >= 64000
    sn, cs, wr = te.sincos(t)
    assert oc.same_bits(wr, t)
    ref = [tc.sincos2pi(v) for v in t]
    assert oc.same_bits(sn, np.array([r[0] for r in ref])) and oc.same_bits(cs, np.array([r[1] for r in ref]))
    two_pi = 2 * mpmath.pi
    worst = [0.0, 0.0]
    for v, s, c in zip(t, sn, cs):
        a = two_pi * mpmath.mpf(float(v))
        for k, (got, exact) in enumerate(((s, mpmath.sin(a)), (c, mpmath.cos(a)))):
            ulp = mpmath.ldexp(1, max(mpmath.frexp(exact)[1] - 53, -1074))       # (the spacing of the doubles at the exact value)
            err = float(abs(mpmath.mpf(float(got)) - exact) / ulp)
            worst[k] = max(worst[k], err)
    print("sin2pi worst error %.3f ulp, cos2pi %.3f ulp over %d points" % (worst[0], worst[1], t.size))
    assert worst[0] <= SINCOS_ULP_BOUND and worst[1] <= SINCOS_ULP_BOUND
    # the quarter points: exact
    sn, cs, _ = te.sincos(np.array([0.0, 0.25, 0.5, 0.75]))
    assert list(sn) == [0.0, 1.0, 0.0, -1.0] and list(cs) == [1.0, 0.0, -1.0, 0.0]
    assert [tuple(float(x) for x in tc.sincos2pi(v)) for v in (0.0, 0.25, 0.5, 0.75)] == [(0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0)]
    # a NaN stays a NaN; wrap
    sn, cs, wr = te.sincos(np.array([np.nan, -0.25, 1.75, -1e-300, np.inf, 3.0]))
    assert np.isnan(sn[0]) and np.isnan(cs[0]) and np.isnan(wr[0]) and np.isnan(wr[4])
    assert list(wr[[1, 2, 3, 5]]) == [0.75, 0.75, 0.0, 0.0] and all(float(tc.wrap(v)) == w for v, w in ((-0.25, 0.75), (1.75, 0.75), (-1e-300, 0.0), (3.0, 0.0)))


def one_env(cols, ncalls, table=None, state=None, dtype=np.float64):
    """cols on one env for ncalls calls -> the rows after every call [ncalls][ncols]."""
    n = len(cols)
    rows, st, words, counts = np.zeros((1, n), dtype=dtype), np.zeros((1, n)), np.zeros((1, 3, n), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    call = te.Call({}, 1, cols, dtype, 1, table=table, rows=rows, state=st, words=words, counts=counts)
    out = []
    for _ in range(ncalls):
        call.task()
        out.append(rows[0].copy())
    return np.array(out)


def test_trapezoid_gate(built):
    """A TRAPEZOID column is 0 at theta = 0 and at duty + ramp, and 1 on [ramp, duty]: a clock of rate 1/64 (exact) from 0, duty 0.5,
    ramp 0.125."""
    got = one_env([P.task_phase(rate=1.0 / 64), P.task_wave(0, P.TASK_TRAPEZOID, duty=0.5, ramp=0.125)], 64)
    theta, g = got[:, 0], got[:, 1]
    assert list(theta) == [k / 64 for k in range(64)]
    assert g[0] == 0.0 and g[40] == 0.0 and (g[41:] == 0.0).all()
    assert (g[8:33] == 1.0).all() and (g[1:8] > 0).all() and (g[1:8] < 1).all() and (g[33:40] > 0).all() and (g[33:40] < 1).all()
    assert g[4] == 0.5 and g[36] == 0.5


def test_table_frames_come_back_exactly(built):
    """A TABLE column at theta = k / nframes returns frame k's bits when offset = 0 and scale = 1 (8 frames: every k / 8 is exact), and
    half way between two frames their mean; the last frame interpolates towards frame 0."""
    T = np.random.default_rng(3).uniform(-1, 1, (8, 3))
    got = one_env([P.task_phase(rate=1.0 / 16), P.task_table(0, 1), P.task_table(0, 2, shift=0.5)], 16, table=T)
    for k in range(8):
        assert got[2 * k, 1] == T[k, 1] and got[2 * k, 2] == T[(k + 4) % 8, 2]
        a, b = T[k, 1], T[(k + 1) % 8, 1]
        assert got[2 * k + 1, 1] == a + 0.5 * (b - a)


def test_counts_and_epochs_wrap_and_a_run_resumes(cols, table, start):
    """Counts near 2^32 and epochs near 2^32 wrap as the restatement's do (a count that comes round to 0 starts the env afresh at epoch
    0); and a run cut in two, its state handed over, equals the uninterrupted one."""
    n = len(cols)
    state, words, counts = np.zeros((cases.NENV, n)), np.zeros((cases.NENV, 3, n), dtype=np.uint32), np.array([2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 5, 1], dtype=np.uint32)
    words[:, 2, :] = np.array([2 ** 32 - 2, 2 ** 32 - 1, 7, 2 ** 32 - 1, 0], dtype=np.uint32)[:, None]
    begin = (state, words, counts)
    sched = ((0, 5, None),) * 6
    ref = cases.reference(cols, table, np.float64, start, schedule=sched, start=begin)
    got, _, _ = run_emulator(cols, table, np.float64, start, schedule=sched, begin=begin)
    assert all(same_call(g, w) for g, w in zip(got, ref))
    assert list(got[-1][3]) == [3, 4, 5, 11, 7] and (got[3][2][1, 2, list(cases.SAMPLES)] < 4).all()
    assert (got[0][2][3, 2, list(cases.SAMPLES)] == 0).all()           # (epoch 2^32 - 1 + 1)
    # a resumed run
    whole = cases.reference(cols, table, np.float32, start)
    first, _, _ = run_emulator(cols, table, np.float32, start, schedule=cases.SCHEDULE[:6])
    held = {P.F_XFRC_APPLIED: first[-1][4][P.F_XFRC_APPLIED]}
    rest, _, _ = run_emulator(cols, table, np.float32, held, schedule=cases.SCHEDULE[6:], begin=first[-1][1:4])
    for g, w in zip(rest, whole[6:]):
        # (rows of envs a later sub-range call skips are those of the first half: compare what the second half wrote)
        assert oc.same_bits(g[1], w[1]) and np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3])
        assert oc.same_bits(g[4][P.F_XFRC_APPLIED], w[4][P.F_XFRC_APPLIED])
    assert oc.same_bits(rest[-1][0], whole[-1][0])


# ---- the launch rules ----

def held(cassie, nenv=3):
    """What a fresh batch holds: the state and command fields."""
    pod = cassie.pod
    dims = {P.F_QPOS: pod.nq, P.F_QVEL: pod.nv, P.F_TIME: 1, P.F_CTRL: pod.nu, P.F_SENSORDATA: pod.nsensordata, P.F_PD_PTARGET: pod.nu, P.F_PD_KP: pod.nu,
            P.F_PD_KD: pod.nu, P.F_PD_DTARGET: pod.nu, P.F_PD_TORQUE: pod.nu, P.F_DRIVE_CMD: pod.nu + 1, P.F_QFRC_APPLIED: pod.nv,
            P.F_XFRC_APPLIED: 6 * pod.nbody, P.F_MEAS: P.MEAS_DIM, P.F_DEPTH: 16}
    return {f: np.zeros((nenv, d)) for f, d in dims.items()}


def refusal(cassie, c, nenv=3, fields=None, **kw):
    return te.Call(held(cassie, nenv) if fields is None else fields, nenv, c, **kw).check()[0]


def test_configure_refusals(cassie):
    pod = cassie.pod
    T = np.zeros((7, 5))
    S, PH = P.task_sample(), P.task_phase()
    assert refusal(cassie, [S]) is None and refusal(cassie, [S, PH, P.task_wave(1), P.task_table(1, 4)], table=T) is None
    bad = lambda c, word, **kw: word in (refusal(cassie, c if isinstance(c, list) else [c], **kw) or "")
    # sizes and the dtype
    assert bad([], "1 .. 64 columns") and bad([S], "1 .. 64 columns", ncols=-1) and bad([S] * 65, "1 .. 64 columns") and refusal(cassie, [S] * 64) is None
    assert bad(S, "dtype", dtype=2) and bad(S, "dtype", dtype=np.int32) and refusal(cassie, [S], dtype=np.float64) is None
    # kinds and forms
    assert bad(P._task_col(4), "a column's kind is") and bad(P._task_col(-1), "a column's kind is")
    assert bad([PH, P.task_wave(0, form=4)], "a WAVE's form is") and bad([PH, P.task_wave(0, form=-1)], "a WAVE's form is")
    # non-finite constants
    for v in (np.nan, np.inf, -np.inf):
        for name in ("center", "half", "rest", "p_rest"):
            assert bad(P.task_sample(**{name: v}), "finite center, half, rest and p_rest"), name
        for name in ("rate", "rate_scale", "phase0"):
            assert bad(P.task_phase(**{name: v}), "finite rate, rate_scale and phase0"), name
        for name in ("shift", "offset", "scale"):
            assert bad([PH, P.task_wave(0, **{name: v})], "finite shift, offset and scale") and bad([PH, P.task_table(0, 0, **{name: v})], "finite shift, offset and scale", table=T)
        for name in ("duty", "ramp"):
            assert bad([PH, P.task_wave(0, P.TASK_TRAPEZOID, **{"duty": 0.5, "ramp": 0.1, name: v})], "TRAPEZOID needs")
    # a SAMPLE's ranges
    assert bad(P.task_sample(half=-0.1), "half is a half width") and refusal(cassie, [P.task_sample(half=0.0)]) is None
    assert bad(P.task_sample(p_rest=-0.01), "p_rest is a probability") and bad(P.task_sample(p_rest=1.0 + 2.0 ** -52), "p_rest is a probability")
    assert refusal(cassie, [P.task_sample(p_rest=0.0), P.task_sample(p_rest=1.0)]) is None
    for lo, hi in ((0, 3), (4, 3), (1, (1 << 30) + 1)):
        assert bad(P.task_sample(period_lo=lo, period_hi=hi), "1 <= period_lo <= period_hi <= 2^30")
    assert refusal(cassie, [P.task_sample(period_lo=1, period_hi=1 << 30), P.task_sample(period_lo=1 << 30)]) is None
    # groups
    assert bad([S, PH, P.task_sample(group=1)], "group names a SAMPLE column") and bad([S, P.task_sample(group=2)], "group names a SAMPLE column")
    assert bad([S, P.task_sample(group=0), P.task_sample(group=1)], "group names a SAMPLE column")      # (column 1 is not its own group)
    assert refusal(cassie, [P.task_sample(group=0), P.task_sample(group=0), P.task_sample(group=-1)]) is None
    lead = dict(period_lo=2, period_hi=4, hold=1, p_rest=0.3)
    assert refusal(cassie, [P.task_sample(**lead), P.task_sample(1.0, 2.0, rest=3.0, group=0, **lead)]) is None
    for name, v in (("period_lo", 1), ("period_hi", 5), ("hold", 0), ("p_rest", 0.31)):
        assert bad([P.task_sample(**lead), P.task_sample(group=0, **{**lead, name: v})], "the members of a group share"), name
    # a clock's columns, a waveform's source
    assert bad([S, PH, P.task_phase(rate_col=1)], "rate_col is -1 or a SAMPLE column") and bad([S, P.task_phase(rate_col=2)], "rate_col is -1 or a SAMPLE column")
    assert bad([S, PH, P.task_phase(phase_col=1)], "phase_col is -1 or a SAMPLE column") and bad([S, P.task_phase(phase_col=7)], "phase_col is -1 or a SAMPLE column")
    assert refusal(cassie, [S, P.task_phase(rate_col=0, phase_col=0)]) is None
    for src in (0, -1, 2, 3):
        assert bad([S, PH, P.task_wave(src)], "src is a PHASE column") and bad([S, PH, P.task_table(src, 0)], "src is a PHASE column", table=T)
    # the gate
    tz = lambda duty, ramp: [PH, P.task_wave(0, P.TASK_TRAPEZOID, duty=duty, ramp=ramp)]
    assert bad(tz(0.5, 0.0), "TRAPEZOID needs") and bad(tz(0.5, -0.1), "TRAPEZOID needs") and bad(tz(-0.1, 0.1), "TRAPEZOID needs") and bad(tz(0.95, 0.1), "TRAPEZOID needs")
    assert refusal(cassie, tz(0.9, 0.1)) is None and refusal(cassie, tz(0.0, 1.0)) is None
    # the table
    assert bad([PH, P.task_table(0, 0)], "a TABLE column and no table") and bad([PH, P.task_table(0, 5)], "tcol lies beyond", table=T) and bad([PH, P.task_table(0, -1)], "tcol lies beyond", table=T)
    assert bad([S], "a table of 1 .. 4096 frames", table=np.zeros((4097, 1))) and bad([S], "a table of 1 .. 4096 frames", table=np.zeros((1, 65)))
    assert bad([S], "a table of 1 .. 4096 frames", table=T, table_shape=(0, 5)) and bad([S], "a table of 1 .. 4096 frames", table=np.full((2, 2), np.nan))
    assert refusal(cassie, [S], table=np.zeros((4096, 64))) is None
    k = te.Call(held(cassie), 3, [PH, P.task_table(0, 4)], table=T)
    assert k.table_check(np.zeros((3, 5))) is None and "reach beyond the new table" in k.table_check(np.zeros((3, 4)))
    # the destination: the action's rules
    for f in P.ACT_CMD_FIELDS:
        assert refusal(cassie, [P.task_sample(dfield=f)]) is None
    for f in (P.F_QPOS, P.F_MEAS, P.F_DEPTH, P.F_PROBES + 1, -1, -2):
        assert bad(P.task_sample(dfield=f), "a column's dfield is PHYS_ACT_NONE or a command field")
    less = held(cassie)
    del less[P.F_XFRC_APPLIED]
    assert "does not hold" in refusal(cassie, [P.task_sample(dfield=P.F_XFRC_APPLIED)], fields=less)
    assert bad(P.task_sample(dfield=P.F_XFRC_APPLIED, dindex=6 * pod.nbody), "dindex lies beyond") and bad(P.task_phase(dfield=P.F_CTRL, dindex=-1), "dindex lies beyond")
    assert bad([P.task_sample(dfield=P.F_CTRL, dindex=1), PH, P.task_wave(1, dfield=P.F_CTRL, dindex=1)], "same destination element")
    assert refusal(cassie, [P.task_sample(dfield=P.F_CTRL, dindex=1), PH, P.task_wave(1, dfield=P.F_CTRL, dindex=2)]) is None


def test_the_record_of_a_configuration(cassie, cols, table):
    pod = cassie.pod
    why, rec = te.Call(held(cassie), 3, cols, table=table).check()
    assert why is None
    assert (rec["ncols"], rec["dtype"], rec["tcol_need"]) == (cases.NCOLS, 4, 5)
    assert rec["dst_field"] == [P.F_XFRC_APPLIED] and rec["dst_dim"] == [6 * pod.nbody]
    t = te.Call(held(cassie), 3, cols, table=table).columns()
    assert len(t) == cases.NCOLS
    assert list(t["kind"]) == [0] * 7 + [1, 1] + [2] * 6 + [3] * 4
    assert list(t["group"][:7]) == [0, 0, 0, 3, 3, 5, 6] and list(t["period_lo"][:7]) == [2, 2, 2, 3, 3, 3, 4] and list(t["span"][:7]) == [3, 3, 3, 1, 1, 3, 3]
    assert list(t["hold"][:7]) == [0, 0, 0, 1, 1, 0, 0] and [int(v) for v in t["thr"][:5]] == [tc.threshold(0.3)] * 3 + [1 << 31] * 2
    assert (t["rate_col"][cases.CLOCK], t["phase_col"][cases.CLOCK], t["rate_col"][cases.CLOCK2], t["phase_col"][cases.CLOCK2]) == (cases.FREQ, cases.PHASE0, -1, -1)
    assert np.all(t["rate_col"][:7] == -1) and np.all(t["src"][:9] == -1) and list(t["src"][9:]) == [7, 7, 7, 7, 7, 8, 7, 7, 8, 8]
    assert list(t["dslot"]) == [-1] * 3 + [0, 0] + [-1] * 14 and tuple(t["delem"][3:5]) == cases.push_elems(pod)
    assert list(t["tcol"][15:]) == [0, 4, 2, 1] and list(t["form"][9:15]) == [P.TASK_SAW, P.TASK_SIN, P.TASK_COS, P.TASK_TRAPEZOID, P.TASK_TRAPEZOID, P.TASK_SAW]


def test_bind_and_call_refusals(cassie):
    pod = cassie.pod
    c = [P.task_sample(dfield=P.F_CTRL, dindex=j) for j in range(4)] + [P.task_phase(), P.task_table(4, 2)]
    T = np.zeros((4, 3))
    kw = dict(state=np.zeros((3, 6)), words=np.zeros((3, 3, 6), dtype=np.uint32), counts=np.zeros(3, dtype=np.uint32), table=T)
    assert "row stride" in te.Call(held(cassie), 3, c, rows=np.zeros((3, 5), dtype=np.float32), **kw).check()[0]
    assert te.Call(held(cassie), 3, c, rows=np.zeros((3, 6), dtype=np.float32), **kw).check()[0] is None
    k = te.Call(held(cassie), 3, c, rows=np.zeros((3, 6), dtype=np.float32), **kw)
    assert k.call_check(0, 3) is None and k.call_check(3, 0) is None and k.call_check(1, 2) is None
    assert "not configured" in k.call_check(0, 3, configured=False)
    assert "not configured" in te.Call(held(cassie), 3, c, **kw).call_check(0, 3)          # (no rows)
    for env0, n in ((-1, 2), (0, 4), (2, 2), (0, -1)):
        assert "out of bounds" in k.call_check(env0, n)
    assert "destination field has changed" in k.call_check(0, 3, now={P.F_CTRL: (np.zeros((3, pod.nu + 1)), pod.nu + 1)})
    assert "destination field has changed" in k.call_check(0, 3, now={P.F_CTRL: (None, 0)})
    assert k.call_check(0, 3, now={P.F_QVEL: (None, 0), P.F_PD_KP: (None, 0)}) is None      # (no column names them)
    assert te.lib().emu_task(k.a, 0, 4, None, 0) == -1 and b"out of bounds" in te.lib().emu_task_last_refusal()


def test_launch_record(cassie, cols, table):
    """The grid, and the IO's pointers and strides: a destination bound as a column block of a wider tensor with its row stride, the
    table, the rows, the state, the words, the counts and the reset words."""
    assert [te.grid(n) for n in (0, 1, 5, 64, 65, 4096)] == [0, 1, 5, 64, 64, 64] and te.TASK_GRID == 64
    pod = cassie.pod
    f = held(cassie, 6)
    wide = np.zeros((6, 6 * pod.nbody + 3))
    f[P.F_XFRC_APPLIED] = wide[:, 2: 2 + 6 * pod.nbody]
    rows, state, words, counts = np.zeros((6, 30), dtype=np.float32), np.zeros((6, 19)), np.zeros((6, 3, 19), dtype=np.uint32), np.zeros(6, dtype=np.uint32)
    reset = np.zeros(3, dtype=np.int32)
    k = te.Call(f, 6, cols, np.float32, seed=0x0123456789abcdef, env_base=40, table=table, rows=rows, state=state, words=words, counts=counts)
    rec, dst = k.record(2, 3, reset)
    assert (rec["env0"], rec["n"], rec["ncols"], rec["f32"], rec["nframes"], rec["tcols"], rec["env_base"]) == (2, 3, 19, 1, 7, 5, 40)
    assert (rec["key0"], rec["key1"]) == (0x89abcdef, 0x01234567) and rec["cols"] == 1 and rec["table"] == table.ctypes.data
    assert (rec["rows"], rec["srow"], rec["state"], rec["words"]) == (rows.ctypes.data, 30, state.ctypes.data, words.ctypes.data)
    assert (rec["counts"], rec["reset"]) == (counts.ctypes.data, reset.ctypes.data)
    assert dst == [(wide.ctypes.data + 16, wide.shape[1])]
    # float64 rows, no reset words; a configuration without TABLE columns is handed no table
    k64 = te.Call(f, 6, cols[:15], np.float64, table=table, rows=np.zeros((6, 15)), state=state, words=words, counts=counts)
    rec64, _ = k64.record(0, 6)
    assert (rec64["f32"], rec64["srow"], rec64["reset"], rec64["table"], rec64["nframes"], rec64["tcols"]) == (0, 15, 0, 0, 0, 0)
