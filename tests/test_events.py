"""Event rows (phys_batch_events, include/cassie_phys.h: measures, Schmitt triggers, timers, edges, latches, running extremes and sums,
combinations and the done words in one launch) on the CPU wave emulator: cassie_event_kernel launched through the launcher's own records,
grid and checks (csrc/small_launch.h) against the definition restated in numpy (tests/events_check.py), BIT FOR BIT; known answers that
neither implementation made; and the launch rules one by one.  All comparisons are on IEEE bits, a NaN equal to a NaN.  The GPU
counterpart is tests/test_events_gpu.py."""
import numpy as np
import pytest

import events_cases as cases
import events_check as ec
import events_emu_py as ee
from cassie_amd import phys as P
from obs_check import same_bits

DTYPES = [np.float64, np.float32]
FILL = -7.25
NAMES = ("rows", "done words", "state", "words", "counts")


@pytest.fixture(scope="module")
def ids(cassie):
    return cases.feet(cassie)


@pytest.fixture(scope="module")
def cols(ids):
    return cases.columns_of(ids[0], ids[1])


@pytest.fixture(scope="module")
def calls(cassie, ids):
    """The sources and reset words of every call of the schedule (shared, left unchanged)."""
    return cases.make_calls(cassie.pod.nbody, ids[0], ids[1])


def run_emulator(cols, calls, dtype, ranges=cases.RANGES, nenv=cases.NENV, done_mask=cases.DONE_MASK, start=None, grid=0):
    """The schedule on the emulator, the rows ROW_PAD elements wider than the columns and filled with FILL -> [(rows, done words, state,
    words, counts)] after every call, and the raw rows."""
    keep, out = None, []
    for (cfrc, inp, reset), (env0, n) in zip(calls, ranges):
        call = ee.Call({P.F_BODY_CFRC: cfrc}, nenv, cols, dtype, done_mask, inp=inp, input_dim=cases.INPUT_DIM, pad=cases.ROW_PAD, fill=FILL)
        if keep is not None:
            call.rows_raw[:], call.flags[:], call.state[:], call.words[:], call.counts[:] = keep
        elif start is not None:
            call.state[:], call.words[:], call.counts[:] = start
        call.events(env0, n, reset, grid=grid)
        keep = (call.rows_raw.copy(), call.flags.copy(), call.state.copy(), call.words.copy(), call.counts.copy())
        out.append((call.rows.copy(),) + keep[1:])
    return out, keep[0]


def assert_same(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b, name in zip(g, w, NAMES):
            assert a.dtype == b.dtype and same_bits(a, b), (what, k, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulator_against_the_definition(cols, calls, dtype):
    """64 columns over fourteen calls on 70 envs: the rows, both state slots, the words, the counts and the done words are the numpy
    restatement's after every call, bit for bit; the gaps of the strided rows stay; and the case holds what it says it holds."""
    want = cases.reference(cols, calls, dtype)
    got, raw = run_emulator(cols, calls, dtype)
    assert_same(got, want)
    assert np.all(raw[:, cases.NCOLS:] == dtype(FILL))
    t = P.ev_cols(cols)
    # every kind, norm (SUMSQ with and without the root), op and polarity; the column at index 63 under mask bit 63; counts 1 and 3
    assert len(t) == 64 and set(t["kind"]) == set(range(7)) and cases.DONE_MASK >> 63 == 1 and bin(cases.DONE_MASK).count("1") == 2
    m = t[t["kind"] == P.EV_MEASURE]
    assert {(int(a), int(b)) for a, b in zip(m["norm"], m["root"])} == {(P.EV_SIGNED, 0), (P.EV_SUMABS, 0), (P.EV_SUMSQ, 0), (P.EV_SUMSQ, 1), (P.EV_MAXABS, 0)}
    assert set(m["field"]) == {P.F_BODY_CFRC, P.EV_INPUT} and {1, 3} <= set(m["count"])
    for kind, ops in ((P.EV_EDGE, 3), (P.EV_ACCUM, 3), (P.EV_LOGIC, 4)):
        assert set(t[t["kind"] == kind]["op"]) == set(range(ops))
    assert set(t[t["kind"] == P.EV_TIMER]["polarity"]) == {0, 1} and set(t[t["kind"] == P.EV_LEVEL]["sense"]) == {1, -1}
    la = t[t["kind"] == P.EV_LATCH]
    assert set(la["lag"]) == {0, 1} and set(la["keep"]) == {0, 1}
    ac = t[t["kind"] == P.EV_ACCUM]
    assert (ac["gate"] >= 0).any() and (ac["gate"] < 0).any() and (ac["clear"] >= 0).any() and (ac["clear"] < 0).any()
    # what happened: both feet made and broke contact, air times were paid, both done columns fired, done words of both values
    rows = np.array([g[0] for g in got], dtype=np.float64)
    for c in (cases.TDL, cases.TDR, cases.LOL, cases.LOR, cases.FLY_DONE, cases.LAST, cases.BOTH, cases.NEITHER, cases.LOW):
        assert (rows[:, :, c] == 1).any() and (rows[:, :, c] == 0).any(), c
    assert (rows[:, :, cases.AIRL] > 0).any() and (rows[:, :, cases.AIRR] < 0).any() and set(np.unique(rows[:, :, cases.CNT])) == {0.0, 1.0, 2.0, 3.0}
    flags = np.array([g[1] for g in got])
    assert set(np.unique(flags)) == {0, 1}
    # the thresholds are met exactly: a force of on_thr switches a foot on, a force of off_thr switches it off
    hit_on = hit_off = False
    for k in range(1, len(got)):
        env0, n = cases.RANGES[k]
        for e in range(env0, env0 + n, 2):      # (even envs: the force along z alone)
            f, was, now = rows[k, e, cases.FL], _last_value(got, k, e, cases.CL), rows[k, e, cases.CL]
            fresh = calls[k][2] is not None and calls[k][2][e - env0] != 0
            hit_on |= f == cases.ON_THR and now == 1 and (was == 0 or fresh)
            hit_off |= f == cases.OFF_THR and now == 0 and was == 1 and not fresh
    assert hit_on and hit_off
    # the NaN and the infinities: a NaN force is off, an infinite one on; the NaN of the input sticks in the gated sum until a touchdown
    assert np.isnan(rows[5, cases.ENV_NAN, cases.FL]) and rows[5, cases.ENV_NAN, cases.CL] == 0 and np.isnan(rows[5, cases.ENV_NAN, cases.SQ])
    assert rows[3, cases.ENV_PINF, cases.FL] == np.inf and rows[3, cases.ENV_PINF, cases.CL] == 1 and rows[3, cases.ENV_PINF, cases.PEAKL] == np.inf
    assert rows[6, cases.ENV_NINF, cases.FL] == np.inf and rows[6, cases.ENV_NINF, cases.CL] == 1
    assert np.isnan(rows[5, cases.ENV_NAN_IN, cases.SA]) and np.isfinite(rows[5, cases.ENV_NAN_IN, cases.MA])
    # resets hit envs in stance and in flight
    for k in cases.RESETS:
        env0, n = cases.RANGES[k]
        hit = [e for e in range(env0, env0 + n) if calls[k][2][e - env0] != 0]
        before = [_last_value(got, k, e, cases.CL) for e in hit]
        assert 0.0 in before and 1.0 in before, k


def _last_value(got, k, e, c):
    """Column c of env e as the call before call k left it."""
    return float(got[k - 1][0][e, c])


def test_known_answers():
    """A hand-written contact pattern for one env: the air times, stance times, edge calls and latched values written out as integers
    times dt -- on the emulator and by the numpy restatement, neither of which made them."""
    dt = 0.02
    contact = [0, 0, 1, 1, 1, 0, 0, 0, 0, 1, 1, 0, 1]
    off_t = [1, 2, 0, 0, 0, 1, 2, 3, 4, 0, 0, 1, 0]
    on_t = [0, 0, 1, 2, 3, 0, 0, 0, 0, 1, 2, 0, 1]
    rising = [0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1]
    falling = [0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0]
    air = [0, 0, 2, 0, 0, 0, 0, 0, 0, 4, 0, 0, 1]            # paid on the touchdown call alone: the off-timer of the call before
    stance = [0, 0, 0, 0, 0, 3, 3, 3, 3, 3, 3, 2, 2]         # held: the on-timer of the call before a lift-off
    peak = [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]           # (the running maximum of a 0/1 signal from 0)
    steps = [0, 0, 1, 2, 3, 3, 3, 3, 3, 1, 2, 2, 1]          # calls in contact since the last touchdown (a gated sum cleared by it)
    cols = [P.ev_measure(P.EV_INPUT, 0), P.ev_level(0, 0.5), P.ev_timer(1, dt, 0), P.ev_timer(1, dt, 1), P.ev_edge(1, P.EV_RISING), P.ev_edge(1, P.EV_FALLING),
            P.ev_latch(2, 4, lag=1), P.ev_latch(3, 5, lag=1, keep=1), P.ev_accum(0, P.EV_MAX), P.ev_accum(1, P.EV_SUM, clear=4, gate=1)]
    want = np.array([contact, contact, [dt * t for t in off_t], [dt * t for t in on_t], rising, falling, [dt * t for t in air], [dt * t for t in stance],
                     peak, steps], dtype=np.float64).T
    ref = ec.Events(cols, 1, np.float64)
    keep = None
    for k, c in enumerate(contact):
        inp = np.array([[float(c)]], dtype=np.float64)
        ref.events({P.EV_INPUT: inp})
        call = ee.Call({}, 1, cols, np.float64, inp=inp)
        if keep is not None:
            call.state[:], call.words[:], call.counts[:] = keep
        call.events()
        keep = (call.state.copy(), call.words.copy(), call.counts.copy())
        assert same_bits(call.rows[0], want[k]), (k, call.rows[0], want[k])
        assert same_bits(ref.rows[0], want[k]), k
    # a reset in flight: no edge on the first call, the timers and the latches start again
    call = ee.Call({}, 1, cols, np.float64, inp=np.array([[1.0]]))
    call.state[:], call.words[:], call.counts[:] = keep
    call.events(reset=[1])
    assert same_bits(call.rows[0], np.array([1, 1, 0, dt * 1, 0, 0, 0, 0, 1, 1], dtype=np.float64))


def test_a_call_changes_nothing_outside_its_range(cols, calls):
    """(3, 64) leaves envs 0 .. 2 and 67 .. 69 alone and (69, 1) everybody but the last, byte for byte; inside, everything moves on."""
    got, _ = run_emulator(cols, calls, np.float32)
    for k, (env0, n) in enumerate(cases.RANGES):
        if k == 0:
            continue
        outside = [e for e in range(cases.NENV) if not env0 <= e < env0 + n]
        for a, b, name in zip(got[k], got[k - 1], NAMES):
            assert a[outside].tobytes() == b[outside].tobytes(), (k, name)
        assert np.array_equal(got[k][4][env0:env0 + n], got[k - 1][4][env0:env0 + n] + 1)


def test_the_cut_into_ranges_and_the_grid_do_not_matter(cols, calls):
    """Two ranges (0, 33) and (33, 37) give the whole call's bits, and so does one workgroup that walks both waves' envs."""
    whole, _ = run_emulator(cols, calls[:3], np.float64, ranges=((0, 70),) * 3)
    split = [c for c in calls[:3] for _ in range(2)]
    parts, _ = run_emulator(cols, split, np.float64, ranges=((0, 33), (33, 37)) * 3)
    assert_same(parts[1::2], whole, "two ranges")
    walked, _ = run_emulator(cols, calls[:3], np.float64, ranges=((0, 70),) * 3, grid=1)
    assert_same(walked, whole, "one workgroup")
    assert ee.grid(1) == 1 and ee.grid(64) == 1 and ee.grid(65) == 2 and ee.grid(64 * ee.EVENT_GRID + 65) == ee.EVENT_GRID == 64


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_resumed_run_is_the_uninterrupted_one(cols, calls, dtype):
    """The state, the words and the counts taken after seven calls and put into a new run: the remaining seven are the first run's."""
    whole, _ = run_emulator(cols, calls, dtype)
    start = whole[6][2:5]
    rest, _ = run_emulator(cols, calls[7:], dtype, ranges=cases.RANGES[7:], start=start)
    for k, (g, w) in enumerate(zip(rest, whole[7:])):
        env0, n = cases.RANGES[7 + k]
        for a, b, name in zip(g[2:], w[2:], NAMES[2:]):
            assert same_bits(a, b), (k, name)
        assert same_bits(g[0][env0:env0 + n], w[0][env0:env0 + n]) and np.array_equal(g[1][env0:env0 + n], w[1][env0:env0 + n])
    assert same_bits(rest[-1][0], whole[-1][0]) and np.array_equal(rest[-1][1], whole[-1][1])


def test_a_wrapped_count_is_fresh():
    """counts wraps; an env whose count comes round to 0 starts afresh, and a timer stops at 0xffffffff."""
    cols = [P.ev_measure(P.EV_INPUT, 0), P.ev_timer(0, 1.0, 1), P.ev_accum(0, P.EV_SUM)]
    inp = np.array([[2.0]])
    call = ee.Call({}, 1, cols, np.float64, inp=inp)
    call.counts[:], call.words[0, 1], call.state[0, 0, 2] = 0xFFFFFFFF, 0xFFFFFFFF, 5.0
    call.events()
    assert call.counts[0] == 0 and call.words[0, 1] == 0xFFFFFFFF and call.rows[0, 1] == 4294967295.0 and call.rows[0, 2] == 7.0
    call.events()
    assert call.counts[0] == 1 and call.words[0, 1] == 1 and call.rows[0, 2] == 2.0


def _col(base, **kw):
    t = P.ev_cols([base])
    for k, v in kw.items():
        t[0][k] = v
    return t[0].copy()


M0 = P.ev_measure(P.F_QPOS, 0)
LOWER = "a column's src, trig, clear and gate name columns with a lower index (clear and gate may be -1)"
FINITE = "a column's constants must be finite"
REFUSALS = [
    ("65 columns", [M0] * 65, {}, "1 .. 64 columns (0 releases them), rows of PHYS_OBS_F32 or PHYS_OBS_F64"),
    ("a negative count of columns", [M0], {"ncols": -1}, "1 .. 64 columns (0 releases them), rows of PHYS_OBS_F32 or PHYS_OBS_F64"),
    ("an unknown dtype", [M0], {"dtype": 2}, "the rows' dtype is PHYS_OBS_F32 or PHYS_OBS_F64"),
    ("an unknown kind", [_col(M0, kind=7)], {}, "a column's kind is PHYS_EV_MEASURE, _LEVEL, _TIMER, _EDGE, _LATCH, _ACCUM or _LOGIC"),
    ("an unknown norm", [_col(M0, norm=4)], {}, "a MEASURE's norm is PHYS_EV_SIGNED, _SUMABS, _SUMSQ or _MAXABS"),
    ("an unknown edge", [M0, P.ev_edge(0, 3)], {}, "an EDGE's op is PHYS_EV_RISING, _FALLING or _EITHER"),
    ("an unknown accumulation", [M0, P.ev_accum(0, 3)], {}, "an ACCUM's op is PHYS_EV_MAX, _MIN or _SUM"),
    ("an unknown combination", [M0, P.ev_logic([0], 4)], {}, "a LOGIC's op is PHYS_EV_ANY, _ALL, _NONE or _COUNT"),
    ("a LEVEL on itself", [M0, P.ev_level(1, 0.0)], {}, LOWER),
    ("a TIMER on a higher column", [M0, P.ev_timer(2, 0.1), M0], {}, LOWER),
    ("an EDGE on no column", [M0, P.ev_edge(-1)], {}, LOWER),
    ("a LATCH triggered by itself", [M0, P.ev_latch(0, 1)], {}, LOWER),
    ("a LATCH of a higher column", [M0, P.ev_latch(2, 0), M0], {}, LOWER),
    ("an ACCUM cleared by itself", [M0, P.ev_accum(0, clear=1)], {}, LOWER),
    ("an ACCUM gated by -2", [M0, P.ev_accum(0, gate=-2)], {}, LOWER),
    ("a LEVEL in column 0", [P.ev_level(0, 0.0)], {}, LOWER),
    ("a done bit at ncols", [M0, M0], {"done_mask": 4}, "done_mask has a bit at or above ncols"),
    ("a LOGIC bit at ncols", [M0, P.ev_logic(0b101)], {}, "a LOGIC's mask has a bit at or above ncols"),
    ("a LOGIC bit at its own index", [M0, P.ev_logic(0b11), M0], {}, "a LOGIC's mask names columns with a lower index"),
    ("a LOGIC bit above its own index", [M0, P.ev_logic(0b100), M0], {}, "a LOGIC's mask names columns with a lower index"),
    ("an empty LOGIC", [M0, P.ev_logic(0)], {}, "a LOGIC's mask names at least one column"),
    ("a NaN target", [P.ev_measure(P.F_QPOS, 0, target=np.nan)], {}, FINITE),
    ("an infinite threshold", [M0, P.ev_level(0, np.inf)], {}, FINITE),
    ("a NaN off_thr", [M0, P.ev_level(0, 1.0, np.nan)], {}, FINITE),
    ("an infinite dt", [M0, P.ev_timer(0, -np.inf)], {}, FINITE),
    ("a NaN scale", [M0, M0, P.ev_latch(0, 1, scale=np.nan)], {}, FINITE),
    ("an infinite offset", [M0, M0, P.ev_latch(0, 1, offset=np.inf)], {}, FINITE),
    ("an infinite init", [M0, P.ev_accum(0, init=np.inf)], {}, FINITE),
    ("off_thr above on_thr", [M0, P.ev_level(0, 1.0, 1.5)], {}, "off_thr <= on_thr"),
    ("a sense of 0", [M0, P.ev_level(0, 1.0, sense=0)], {}, "a LEVEL's sense is +1 or -1"),
    ("a lag of 2", [M0, M0, P.ev_latch(0, 1, lag=2)], {}, "a LATCH's lag and keep are 0 or 1"),
    ("no elements", [P.ev_measure(P.F_QPOS, 0, 0, norm=P.EV_SUMABS)], {}, "a MEASURE takes 1 .. 8 elements"),
    ("nine elements", [P.ev_measure(P.F_QPOS, 0, 9, norm=P.EV_SUMABS)], {}, "a MEASURE takes 1 .. 8 elements"),
    ("SIGNED of two", [P.ev_measure(P.F_QPOS, 0, 2)], {}, "a SIGNED MEASURE takes one element"),
    ("the depth image", [P.ev_measure(P.F_DEPTH, 0)], {}, "PHYS_F_DEPTH is no source of an event (images are not columns)"),
    ("an unknown field", [P.ev_measure(-2, 0)], {}, "a MEASURE's field is a PHYS_F_* field of the batch or PHYS_EV_INPUT"),
    ("a field past the last", [P.ev_measure(1000, 0)], {}, "a MEASURE's field is a PHYS_F_* field of the batch or PHYS_EV_INPUT"),
    ("a field the batch does not hold", [P.ev_measure(P.F_STEP_SUMS, 0)], {},
     "a column reads a field the batch does not hold yet (the scan, the rays, the probes, the step sums, the derived block: configure or enable them first)"),
    ("a slice beyond the row", [P.ev_measure(P.F_QPOS, 33, 3, norm=P.EV_SUMSQ)], {}, "index + count lies beyond the field's row"),
    ("a negative index", [P.ev_measure(P.F_QPOS, -1)], {}, "index + count lies beyond the field's row"),
    ("17 sources", [P.ev_measure(f, 0) for f in range(17)], {"many": True}, "more than 16 distinct source fields"),
]


def _fields(nenv, many=False):
    f = {P.F_QPOS: np.zeros((nenv, 35)), P.F_QVEL: np.zeros((nenv, 32))}
    if many:
        f = {k: np.zeros((nenv, 4)) for k in range(17)}
    return f


@pytest.mark.parametrize("what,cols,kw,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_configure_refuses(what, cols, kw, message):
    """Every refusal of phys_batch_events_configure with its message; the emulator's launch is refused with the same."""
    kw = dict(kw)
    many = kw.pop("many", False)
    depth = -5 if many else P.F_DEPTH           # (17 fields that are all sources: none of them the depth image)
    call = ee.Call(_fields(4, many), 4, cols, kw.pop("dtype", np.float32), kw.pop("done_mask", 0), depth_field=depth, **kw)
    why, rec, table = call.check()
    assert why == message and rec is None
    assert call.refusal() == message


def test_configure_accepts_and_fills_the_record():
    """What configure makes of accepted columns: the slots of the sources in order of appearance, the reach into the input, the fields a
    kind does not name cleared, -1 for a clear and a gate that are absent, 64 columns with LOGIC and done bits up to 62 and 63."""
    cols = [P.ev_measure(P.F_QVEL, 3, 2, norm=P.EV_MAXABS, root=True), P.ev_measure(P.EV_INPUT, 4, 3, norm=P.EV_SUMSQ, root=True), P.ev_measure(P.F_QPOS, 34),
            P.ev_measure(P.F_QVEL, 0), _col(P.ev_level(0, 1.0, 1.0, sense=-1), dt=np.nan, count=99), P.ev_accum(1)]
    call = ee.Call(_fields(3), 3, cols, np.float64, 0b100000)
    why, rec, table = call.check()
    assert why is None and rec == {"ncols": 6, "dtype": 8, "nslots": 3, "input_need": 7, "slot_field": [P.F_QVEL, P.EV_INPUT, P.F_QPOS], "slot_dim": [32, 0, 35]}
    assert [int(x) for x in table["field"][:4]] == [0, 1, 2, 0] and [int(x) for x in table["root"][:2]] == [0, 1]
    assert table[4]["dt"] == 0 and table[4]["count"] == 0 and table[4]["sense"] == -1 and table[4]["src"] == 0
    assert (table[5]["clear"], table[5]["gate"], table[5]["src"]) == (-1, -1, 1)
    full = [M0] * 63 + [P.ev_logic((1 << 63) - 1, P.EV_COUNT)]
    why, rec, _ = ee.Call(_fields(2), 2, full, np.float32, 1 << 63).check()
    assert why is None and rec["ncols"] == 64
    assert ee.Call(_fields(2), 2, [], np.float32).check()[0] is None         # (0 columns: accepted, the launcher releases)
    assert ee.Call(_fields(2), 2, [], np.float32).refusal() == "0 columns: nothing to launch (the launcher releases)"


def test_bindings_and_calls_refuse():
    """What the bind calls and a call refuse, each with its message."""
    nenv = 4
    fields = _fields(nenv)
    cols = [P.ev_measure(P.F_QPOS, 0), P.ev_measure(P.EV_INPUT, 5)]
    inp = np.zeros((nenv, 8), dtype=np.float32)
    ok = ee.Call(fields, nenv, cols, np.float32, inp=inp)
    assert ok.call_check(0, nenv) is None and ok.call_check(nenv, 0) is None and ok.call_check(1, 3) is None
    for env0, n in ((-1, 2), (0, nenv + 1), (nenv, 1), (2, -1), (2, 3)):
        assert ok.call_check(env0, n) == "env range out of bounds"
    assert ok.call_check(0, nenv, configured=False) == "not configured (phys_batch_events_configure first)"
    assert ee.Call(fields, nenv, cols, np.float32, inp=inp, own_rows=False).call_check(0, nenv) == "not configured (phys_batch_events_configure first)"
    assert ee.Call(fields, nenv, cols, np.float32).call_check(0, nenv) == "a PHYS_EV_INPUT column and no input bound (phys_batch_events_bind_input first)"
    assert ee.Call(fields, nenv, cols, np.float32, inp=inp, input_dim=5).call_check(0, nenv) == "the bound input's rows are shorter than the PHYS_EV_INPUT columns reach"
    changed = "the row length of a source field has changed since phys_batch_events_configure (configure again)"
    assert ok.call_check(0, nenv, now={P.F_QPOS: (fields[P.F_QPOS], 34)}) == changed
    assert ok.call_check(0, nenv, now={P.F_QPOS: (None, 35)}) == changed
    assert ok.call_check(0, nenv, now={P.F_QVEL: (fields[P.F_QVEL], 3)}) is None        # (no source)
    # the bind checks
    short = ee.Call(fields, nenv, cols, np.float32, inp=inp)
    short.a.srow = 1
    assert short.check()[0] == "a row stride of at least the columns"
    bad = ee.Call(fields, nenv, cols, np.float32, inp=inp)
    bad.a.input_dtype = 2
    assert bad.check()[0] == "the input's dtype is PHYS_OBS_F32 or PHYS_OBS_F64"
    bad.a.input_dtype, bad.a.input_stride = 4, 7
    assert bad.check()[0] == "an input of at least one element a row and a row stride of at least that"
    bad.a.input_stride, bad.a.input_dim = 8, 0
    assert bad.check()[0] == "an input of at least one element a row and a row stride of at least that"
