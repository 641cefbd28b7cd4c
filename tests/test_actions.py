"""Action rows (phys_batch_act, include/cassie_phys.h: clip, noise, latency, low-pass, the map onto a pose, the store into the command
fields and the action row in one launch) on the CPU wave emulator: cassie_act_kernel launched through the launcher's own records, grid and
checks (csrc/small_launch.h) against the definition restated in numpy and Python integers (tests/actions_check.py), BIT FOR BIT -- every
step of a column's value is one individually rounded operation -- and the launch rules one by one.  All comparisons are on IEEE bits, a
NaN equal to a NaN.  The GPU counterpart is tests/test_actions_gpu.py."""
import numpy as np
import pytest

import actions_cases as cases
import actions_check as ac
import actions_emu_py as ae
import obs_check as oc
import obs_emu_py as oe
from cassie_amd import phys as P

DTYPES = [np.float64, np.float32]
FILL = -7.25


@pytest.fixture(scope="module")
def calls(cassie):
    """The actions and the input of every call of the schedule (shared, left unchanged)."""
    return cases.make_calls(cassie)


@pytest.fixture(scope="module")
def cols(cassie):
    return cases.columns_of(cassie.pod)


@pytest.fixture(scope="module")
def start(cassie):
    return cases.start_fields(cassie)


def run_emulator(cols, calls, dtype, start, schedule=cases.SCHEDULE, nenv=cases.NENV, env_base=0, pad=5, grid=0, delays=cases.DELAYS):
    """The schedule on the emulator: rows with a stride `pad` elements beyond the row, xfrc_applied a column block of a wider array ->
    [(rows, state, counts, {field: array})] after every call, the raw row buffer and the wide array, whose gaps were filled with FILL."""
    ncols, D = len(cols), cases.DELAY_MAX
    raw = np.full((nenv, 3 * ncols + pad), FILL, dtype=dtype)
    state, counts = np.zeros((nenv, (D + 3) * ncols)), np.zeros(nenv, dtype=np.uint32)
    held = {f: a.copy() for f, a in start.items()}
    nx = held[P.F_XFRC_APPLIED].shape[1]
    wide = np.full((nenv, nx + 3), FILL)
    wide[:, 2: 2 + nx] = held[P.F_XFRC_APPLIED]
    held[P.F_XFRC_APPLIED] = wide[:, 2: 2 + nx]
    delay = np.array(delays, dtype=np.int32)
    out = []
    for (act, inp), (env0, n, reset) in zip(calls, schedule):
        call = ae.Call(held, nenv, cols, D, dtype, cases.SEED, env_base, actions=act[:, : ncols + 1], inp=inp, input_dim=cases.INPUT_DIM, delay=delay, rows=raw,
                       state=state, counts=counts)
        call.act(env0, n, reset, grid)
        out.append((raw[:, : 3 * ncols].reshape(nenv, 3, ncols).copy(), state.reshape(nenv, D + 3, ncols).copy(), counts.copy(),
                    {f: np.ascontiguousarray(held[f]).copy() for f in cases.DEST_FIELDS}))
    return out, raw, wide


def same_call(got, want):
    return (oc.same_bits(got[0], want[0]) and oc.same_bits(got[1], want[1]) and np.array_equal(got[2], want[2])
            and all(oc.same_bits(got[3][f], want[3][f]) for f in cases.DEST_FIELDS))


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulator_against_the_definition(cassie, cols, calls, start, dtype):
    """70 columns, a delay line of depth 3 with per-env delays over seven calls (fill, three shifts, a sub-range, a reset, a shift) on
    actions and an input that change: rows, state, counts and destination fields are the numpy restatement's after every call, bit for
    bit; envs outside a call's range, the gaps of the strided buffers and every element of a destination field that no column names are
    untouched."""
    assert len(cols) > 64 and len(cols) % 64 != 0
    want = cases.reference(cols, calls, dtype, start)
    got, raw, wide = run_emulator(cols, calls, dtype, start)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[2], w[2]), k
        assert oc.same_bits(g[0], w[0]), k
        assert oc.same_bits(g[1], w[1]), k
        for f in cases.DEST_FIELDS:
            assert oc.same_bits(g[3][f], w[3][f]), (k, f)
    assert list(got[-1][2]) == [6, 7, 7, 7, 6]
    # the gaps of the strided buffers, and what no column names of the destination fields
    assert np.all(raw[:, 3 * len(cols):] == dtype(FILL)) and np.all(wide[:, :2] == FILL) and np.all(wide[:, -1:] == FILL)
    last = got[-1][3]
    assert np.array_equal(last[P.F_XFRC_APPLIED][:, :-1], start[P.F_XFRC_APPLIED][:, :-1]) and not np.array_equal(last[P.F_XFRC_APPLIED][:, -1], start[P.F_XFRC_APPLIED][:, -1])
    for f in (P.F_PD_PTARGET, P.F_PD_DTARGET, P.F_PD_TORQUE):
        assert not (last[f] == start[f]).any()
    # the first call: PREV == NOW, every slot of the line the same, f == z
    rows0, st0 = got[0][0], got[0][1]
    D = cases.DELAY_MAX
    assert oc.same_bits(rows0[:, P.ACT_PREV], rows0[:, P.ACT_NOW])
    for h in range(1, D + 1):
        assert oc.same_bits(st0[:, h], st0[:, 0])
    assert oc.same_bits(st0[:, D + 1], st0[:, 0])
    # the second call shifts: PREV is the first call's NOW, slot 1 the first call's slot 0
    assert oc.same_bits(got[1][0][:, P.ACT_PREV], rows0[:, P.ACT_NOW]) and oc.same_bits(got[1][1][:, 1], st0[:, 0])
    # an unfiltered column without noise or clip (36): APPLIED is NOW of d calls ago, d the env's delay -- 9 clamped to 3
    c = 36
    assert cols[c][4:8] == (-np.inf, np.inf, 0.0, 1.0)
    for e, d in enumerate((0, 1, 2, 3, 3)):
        assert got[3][0][e, P.ACT_APPLIED, c] == got[3 - d][0][e, P.ACT_NOW, c], e
        assert got[3][0][e, P.ACT_NOW, c] == dtype(calls[3][0][e, c])
    # the fifth call goes over [1, 4): envs 0 and 4 keep everything, byte for byte
    for e in (0, 4):
        assert got[4][0][e].tobytes() == got[3][0][e].tobytes() and got[4][1][e].tobytes() == got[3][1][e].tobytes() and got[4][2][e] == got[3][2][e]
        for f in cases.DEST_FIELDS:
            assert got[4][3][f][e].tobytes() == got[3][3][f][e].tobytes()
    assert not np.array_equal(got[4][0][1:4, P.ACT_NOW], got[3][0][1:4, P.ACT_NOW])
    # the sixth restarts env 2 alone
    r5, s5 = got[5][0], got[5][1]
    assert oc.same_bits(r5[2, P.ACT_PREV], r5[2, P.ACT_NOW]) and all(oc.same_bits(s5[2, h], s5[2, 0]) for h in range(1, D + 2))
    assert oc.same_bits(r5[1, P.ACT_PREV], got[4][0][1, P.ACT_NOW]) and not oc.same_bits(r5[1, P.ACT_PREV], r5[1, P.ACT_NOW])
    # env 4's actions leave the clips, carry infinities and NaN; envs 0 .. 3 never meet a clip
    assert (np.abs(got[1][0][4, P.ACT_NOW, :10]) == 1.0).any() and got[1][0][4, P.ACT_NOW, 5] == 1.0 and got[1][0][4, P.ACT_NOW, 33] == -np.inf
    # (env 4's NaN of its third call leaves the line, delayed by 3, at its sixth: the last of the schedule)
    assert np.isnan(got[2][0][4, P.ACT_NOW, 12]) and not np.isnan(got[5][3][P.F_PD_DTARGET][4, 2])
    assert np.isnan(got[-1][3][P.F_PD_DTARGET][4, 2]) and np.isnan(got[-1][0][4, P.ACT_APPLIED, 12])
    assert all(np.isfinite(g[0][:4]).all() and np.isfinite(g[1][:4]).all() for g in got)
    assert all(oc.same_bits(g[0][:4, P.ACT_NOW], c_[0][:4, : len(cols)].astype(dtype)) for g, c_ in zip(got[:4], calls[:4]))
    # the tightly clipped torques clip some entries and pass others
    tq = last[P.F_PD_TORQUE]
    assert (np.abs(tq) == 0.3).any() and (np.abs(tq) < 0.3).any() and np.nanmax(np.abs(tq)) == 0.3


def test_the_counters_fourth_word(built):
    """With equal seed, env, column and count the action's draw is Philox on (.., 1) and differs from the observation's on (.., 0): a
    noisy column's first value against the kernel's own Philox routine, and against an observation column drawing with the same seed."""
    seed, env_base, nenv, amp = cases.SEED, 40, 3, 0.25
    act = np.zeros((nenv, 2), dtype=np.float64)
    rows, state, counts = np.zeros((nenv, 6)), np.zeros((nenv, 6)), np.full(nenv, 11, dtype=np.uint32)
    ae.Call({}, nenv, [P.act_col(noise=amp), P.act_col(noise=amp)], 0, np.float64, seed, env_base, actions=act, rows=rows, state=state, counts=counts).act()
    zero = np.zeros((nenv, 2))
    orow, frames = np.zeros((nenv, 2)), np.full(nenv, 11, dtype=np.uint32)
    oe.Call({P.F_QPOS: zero}, nenv, [P.obs_copy(P.F_QPOS, 0, 2, noise=amp)], 1, np.float64, seed, env_base, rows=orow, frames=frames).observe()
    key = (seed & 0xffffffff, seed >> 32)
    for e in range(nenv):
        for c in range(2):
            w1, w0 = oe.philox((env_base + e, c, 11, 1), key)[0], oe.philox((env_base + e, c, 11, 0), key)[0]
            assert w1 == ac.noise_word(seed, env_base, e, c, 11) and w0 == oc.noise_word(seed, env_base, e, c, 11) and w1 != w0
            assert state[e, c] == np.float64(amp) * oc.uniform(w1) == rows[e, 2 * P.ACT_APPLIED + c]       # (slot 0 of D = 0: v)
            assert orow[e, c] == np.float64(amp) * oc.uniform(w0) and orow[e, c] != state[e, c]
    assert np.all(rows[:, :2] == 0.0) and list(counts) == [12] * nenv


@pytest.mark.parametrize("grid", [1, 3, 64])
def test_any_grid_gives_the_same_bits(cassie, cols, calls, start, grid):
    """One workgroup walking the range, three, or ACT_GRID: the same rows, state, counts and destinations."""
    assert ae.lib() and ae.ACT_GRID == 64
    want = cases.reference(cols, calls[:3], np.float32, start)
    got, _, _ = run_emulator(cols, calls[:3], np.float32, start, grid=grid)
    assert all(same_call(g, w) for g, w in zip(got, want))


def test_a_plain_column_reproduces_the_clip(built):
    """smooth == 1 and noise == 0 through D = 0: APPLIED is clampd(a) itself, never f + 1 (z - f); -0.0 stays -0.0, a NaN passes, the
    infinities clip."""
    a = np.array([[np.nan, -0.0, 3.0, -3.0, np.inf, -np.inf, 0.1, 1e300]], dtype=np.float64)
    n = a.shape[1]
    cols = [P.act_col(P.F_CTRL, j, lo=-1.0, hi=1.0) for j in range(n)]
    ctrl, rows, state, counts = np.zeros((1, n)), np.zeros((1, 3 * n)), np.zeros((1, 3 * n)), np.zeros(1, dtype=np.uint32)
    call = ae.Call({P.F_CTRL: ctrl}, 1, cols, 0, np.float64, actions=a, rows=rows, state=state, counts=counts)
    want = ac.Actions(cols, 1, 0, np.float64)
    ref = {P.F_CTRL: np.zeros((1, n))}
    for k in range(3):       # (the second and third call are not fresh: the filter's branch is the skip)
        state[0, n: 2 * n] = 1e30      # (a filter state the formula would have to cancel exactly)
        want.state[0, 1] = 1e30
        call.act()
        want.act(a, ref)
        r = rows.reshape(1, 3, n)
        assert oc.same_bits(r, want.rows) and oc.same_bits(ctrl, ref[P.F_CTRL])
        assert oc.same_bits(r[0, P.ACT_APPLIED], r[0, P.ACT_NOW]) and np.array_equal(ctrl[0, 1:], r[0, P.ACT_NOW, 1:]) and np.isnan(ctrl[0, 0])
        assert np.isnan(r[0, 0, 0]) and np.signbit(r[0, 0, 1]) and list(r[0, 0, 2:]) == [1.0, -1.0, 1.0, -1.0, 0.1, 1.0]
    assert counts[0] == 3


def test_counts_wrap(built):
    """The count is a uint32 that wraps; the env whose count returns to zero starts afresh."""
    a = np.array([[0.5], [0.25]])
    cols = [P.act_col(noise=0.1, smooth=0.5)]
    rows, state, counts = np.zeros((2, 3)), np.full((2, 4), 9.0), np.array([0xffffffff, 0xfffffffe], dtype=np.uint32)
    call = ae.Call({}, 2, cols, 1, np.float64, 5, actions=a, rows=rows, state=state, counts=counts)
    want = ac.Actions(cols, 2, 1, np.float64, 5)
    want.state[:], want.counts[:] = 9.0, counts
    for _ in range(2):
        call.act()
        want.act(a, {})
        assert list(counts) == list(want.counts) and oc.same_bits(state.reshape(2, 4, 1), want.state) and oc.same_bits(rows.reshape(2, 3, 1), want.rows)
    assert list(counts) == [1, 0] and rows[0, P.ACT_PREV] == 0.5


# ---- the launch rules ----

def held(cassie, nenv=3):
    """What a fresh batch holds: the state and command fields, not the scan, the rays, the probes, the sums or the derived block."""
    pod = cassie.pod
    dims = {P.F_QPOS: pod.nq, P.F_QVEL: pod.nv, P.F_TIME: 1, P.F_CTRL: pod.nu, P.F_SENSORDATA: pod.nsensordata, P.F_PD_PTARGET: pod.nu, P.F_PD_KP: pod.nu,
            P.F_PD_KD: pod.nu, P.F_PD_DTARGET: pod.nu, P.F_PD_TORQUE: pod.nu, P.F_DRIVE_CMD: pod.nu + 1, P.F_QFRC_APPLIED: pod.nv,
            P.F_XFRC_APPLIED: 6 * pod.nbody, P.F_MEAS: P.MEAS_DIM, P.F_DEPTH: 16}
    return {f: np.zeros((nenv, d)) for f, d in dims.items()}


def refusal(cassie, c, nenv=3, fields=None, **kw):
    return ae.Call(held(cassie, nenv) if fields is None else fields, nenv, c, **kw).check()[0]


def test_configure_refusals(cassie):
    pod = cassie.pod
    ok = P.act_col(P.F_PD_PTARGET, 0)
    assert refusal(cassie, [ok]) is None
    bad = lambda c, word, **kw: word in (refusal(cassie, c if isinstance(c, list) else [c], **kw) or "")
    # sizes and the dtype
    assert refusal(cassie, []) is None and bad([ok], "0 .. 256 columns", ncols=-1)
    assert refusal(cassie, [P.act_col()] * P.ACT_MAXCOLS) is None and bad([P.act_col()] * (P.ACT_MAXCOLS + 1), "0 .. 256 columns")
    assert bad(ok, "delay depth", delay_max=-1) and bad(ok, "delay depth", delay_max=P.ACT_MAXDELAY + 1) and refusal(cassie, [ok], delay_max=P.ACT_MAXDELAY) is None
    assert bad(ok, "dtype", dtype=2) and bad(ok, "dtype", dtype=np.int32) and refusal(cassie, [ok], dtype=np.float64) is None
    # non-finite constants, a negative amplitude, the filter's coefficient, bounds out of order
    for name in ("offset", "scale"):
        for v in (np.nan, np.inf, -np.inf):
            assert bad(P.act_col(**{name: v}), "finite offset and scale")
    assert bad(P.act_col(noise=-0.1), "noise is an amplitude") and bad(P.act_col(noise=np.nan), "noise is an amplitude") and bad(P.act_col(noise=np.inf), "noise is an amplitude")
    for v in (0.0, -0.5, 1.0 + 2.0 ** -52, np.nan, np.inf):
        assert bad(P.act_col(smooth=v), "smooth lies in (0, 1]")
    assert refusal(cassie, [P.act_col(smooth=1.0), P.act_col(smooth=5e-324)]) is None
    assert bad(P.act_col(lo=1.0, hi=0.5), "lo <= hi") and bad(P.act_col(lo=np.nan), "lo <= hi") and bad(P.act_col(hi=np.nan), "lo <= hi")
    assert bad(P.act_col(out_lo=1.0, out_hi=0.5), "out_lo <= out_hi") and bad(P.act_col(out_hi=np.nan), "out_lo <= out_hi")
    assert refusal(cassie, [P.act_col(lo=-np.inf, hi=np.inf, out_lo=0.5, out_hi=0.5)]) is None
    # the destination: a command field the batch holds, inside its row, named once
    for f in P.ACT_CMD_FIELDS:
        assert refusal(cassie, [P.act_col(f, 0)]) is None
    for f in (P.F_QPOS, P.F_QVEL, P.F_MEAS, P.F_SENSORDATA, P.F_DEPTH, P.F_PROBES + 1, -1, -2, -7):
        assert bad(P.act_col(f, 0), "a column's dfield is PHYS_ACT_NONE or a command field")
    less = held(cassie)
    del less[P.F_XFRC_APPLIED]
    assert "does not hold" in refusal(cassie, [P.act_col(P.F_XFRC_APPLIED, 0)], fields=less)
    assert refusal(cassie, [P.act_col(P.F_DRIVE_CMD, pod.nu)]) is None and bad(P.act_col(P.F_DRIVE_CMD, pod.nu + 1), "dindex lies beyond")
    assert bad(P.act_col(P.F_CTRL, pod.nu), "dindex lies beyond") and bad(P.act_col(P.F_CTRL, -1), "dindex lies beyond")
    assert bad([P.act_col(P.F_CTRL, 1), P.act_col(P.F_PD_KP, 1), P.act_col(P.F_CTRL, 1)], "same destination element")
    assert refusal(cassie, [P.act_col(P.F_CTRL, 1), P.act_col(P.F_PD_KP, 1), P.act_col(P.F_CTRL, 2), P.act_col(), P.act_col()]) is None
    # the base: a source an observation may read
    assert bad(P.act_col(bfield=P.F_DEPTH), "PHYS_F_DEPTH") and bad(P.act_col(bfield=P.F_PROBES + 1), "a column's bfield is") and bad(P.act_col(bfield=-3), "a column's bfield is")
    for f in (P.F_HEIGHT_SCAN, P.F_RAYS, P.F_PROBES, P.F_STEP_SUMS, P.F_DERIVED):
        assert bad(P.act_col(bfield=f), "does not hold yet")
    assert refusal(cassie, [P.act_col(bfield=P.F_QPOS, bindex=pod.nq - 1)]) is None and bad(P.act_col(bfield=P.F_QPOS, bindex=pod.nq), "bindex lies beyond")
    assert bad(P.act_col(bfield=P.F_QPOS, bindex=-1), "bindex lies beyond") and bad(P.act_col(bfield=P.ACT_INPUT, bindex=-1), "bindex lies beyond")
    # more sources than a call carries
    src = list(range(17))
    wide = {f: np.zeros((3, 4)) for f in src}
    assert ae.Call(wide, 3, [P.act_col(bfield=f) for f in src[:15]] + [P.act_col(bfield=P.ACT_INPUT)]).check()[0] is None
    assert "16 distinct" in ae.Call(wide, 3, [P.act_col(bfield=f) for f in src]).check()[0]


def test_the_record_of_a_configuration(cassie, cols):
    pod = cassie.pod
    why, rec = ae.Call(held(cassie), 3, cols, cases.DELAY_MAX).check()
    assert why is None
    assert (rec["ncols"], rec["delay_max"], rec["dtype"], rec["input_need"], rec["state_dim"]) == (70, 3, 4, 12, 6 * 70)
    assert rec["slot_field"] == [P.ACT_INPUT, P.F_QPOS] and rec["slot_dim"] == [0, pod.nq]
    assert rec["dst_field"] == list(cases.DEST_FIELDS) and rec["dst_dim"] == [pod.nu, pod.nu, pod.nu, 6 * pod.nbody]
    table = ae.Call(held(cassie), 3, cols, cases.DELAY_MAX).columns()
    assert len(table) == 70
    assert list(table["slot"][:10]) == [0] * 10 and list(table["elem"][:10]) == list(range(2, 12)) and list(table["dslot"][:30]) == [0] * 10 + [1] * 10 + [2] * 10
    assert list(table["delem"][:30]) == list(range(10)) * 3 and (table["slot"][30], table["elem"][30], table["dslot"][30], table["delem"][30]) == (1, 2, 3, 6 * pod.nbody - 1)
    assert np.all(table["slot"][31:] == -1) and np.all(table["dslot"][31:] == -1) and np.all(table["slot"][10:30] == -1)
    assert np.all(table["smooth"][10:20] == 0.5) and np.all(table["noise"][20:30] == 0.1) and np.all(table["out_hi"][20:30] == 0.3) and np.all(table["scale"][:10] == 0.5)


def test_bind_refusals(cassie):
    c = [P.act_col(P.F_CTRL, j) for j in range(4)] + [P.act_col(bfield=P.ACT_INPUT, bindex=2)]
    kw = dict(state=np.zeros((3, 15)), counts=np.zeros(3, dtype=np.uint32))
    assert "row stride" in ae.Call(held(cassie), 3, c, rows=np.zeros((3, 14), dtype=np.float32), **kw).check()[0]
    assert ae.Call(held(cassie), 3, c, rows=np.zeros((3, 15), dtype=np.float32), **kw).check()[0] is None
    assert "at least the columns" in ae.Call(held(cassie), 3, c, actions=np.zeros((3, 4), dtype=np.float32)).check()[0]
    assert ae.Call(held(cassie), 3, c, actions=np.zeros((3, 5), dtype=np.float32)).check()[0] is None
    k = ae.Call(held(cassie), 3, c)
    k.bind_actions(np.zeros((3, 5), dtype=np.float32), dtype=2)
    assert "actions' dtype" in k.check()[0]
    k = ae.Call(held(cassie), 3, c)
    k.bind_input(np.zeros((3, 4), dtype=np.float32), dtype=2)
    assert "input's dtype" in k.check()[0]
    k.bind_input(np.zeros((3, 4), dtype=np.float32), input_dim=0)
    assert "at least one element" in k.check()[0]
    k.bind_input(np.zeros((3, 4), dtype=np.float32), input_dim=4, stride=3)
    assert "at least one element" in k.check()[0]


def test_call_refusals(cassie):
    pod = cassie.pod
    c = [P.act_col(P.F_CTRL, j, bfield=P.F_QPOS, bindex=j) for j in range(4)] + [P.act_col(bfield=P.ACT_INPUT, bindex=2)]
    kw = dict(rows=np.zeros((3, 15), dtype=np.float32), state=np.zeros((3, 15)), counts=np.zeros(3, dtype=np.uint32))
    act, inp = np.zeros((3, 5), dtype=np.float32), np.zeros((3, 5), dtype=np.float32)
    k = ae.Call(held(cassie), 3, c, actions=act, inp=inp, **kw)
    assert k.call_check(0, 3) is None and k.call_check(3, 0) is None and k.call_check(1, 2) is None
    assert "not configured" in k.call_check(0, 3, configured=False)
    assert "no actions bound" in ae.Call(held(cassie), 3, c, inp=inp, **kw).call_check(0, 3)
    for env0, n in ((-1, 2), (0, 4), (2, 2), (0, -1)):
        assert "out of bounds" in k.call_check(env0, n)
    # a source or a destination whose row has changed, or gone, since the configure call
    assert "source field has changed" in k.call_check(0, 3, now={P.F_QPOS: (np.zeros((3, pod.nq + 1)), pod.nq + 1)})
    assert "source field has changed" in k.call_check(0, 3, now={P.F_QPOS: (None, 0)})
    assert "destination field has changed" in k.call_check(0, 3, now={P.F_CTRL: (np.zeros((3, pod.nu + 1)), pod.nu + 1)})
    assert "destination field has changed" in k.call_check(0, 3, now={P.F_CTRL: (None, 0)})
    assert k.call_check(0, 3, now={P.F_QVEL: (None, 0), P.F_PD_KP: (None, 0)}) is None      # (no column names them)
    # the input: nothing bound, or bound too short
    assert "no input bound" in ae.Call(held(cassie), 3, c, actions=act, **kw).call_check(0, 3)
    assert "shorter" in ae.Call(held(cassie), 3, c, actions=act, inp=inp, input_dim=2, **kw).call_check(0, 3)
    assert ae.Call(held(cassie), 3, c, actions=act, inp=inp, input_dim=3, **kw).call_check(0, 3) is None
    # the emulator's launch refuses the same
    assert ae.lib().emu_act(k.a, 0, 4, None, 0) == -1 and b"out of bounds" in ae.lib().emu_act_last_refusal()


def test_launch_record(cassie, cols):
    """The grid, and the IO's pointers and strides: the batch's own dense buffers, a destination and a source bound as column blocks of
    a wider tensor with their row stride, the actions, the input, the rows, the state, the counts, the delays and the reset words."""
    assert [ae.grid(n) for n in (0, 1, 5, 64, 65, 4096)] == [0, 1, 5, 64, 64, 64] and ae.ACT_GRID == 64
    pod = cassie.pod
    f = held(cassie, 6)
    wide = np.zeros((6, pod.nq + 6 * pod.nbody + 3))
    f[P.F_QPOS] = wide[:, : pod.nq]                          # (bound as column blocks of one tensor)
    f[P.F_XFRC_APPLIED] = wide[:, pod.nq: pod.nq + 6 * pod.nbody]
    act, inp = np.zeros((6, cases.ACT_STRIDE), dtype=np.float32), np.zeros((6, cases.INPUT_STRIDE), dtype=np.float32)
    rows, state, counts = np.zeros((6, 250), dtype=np.float32), np.zeros((6, 6 * 70)), np.zeros(6, dtype=np.uint32)
    delay, reset = np.zeros(6, dtype=np.int32), np.zeros(3, dtype=np.int32)
    k = ae.Call(f, 6, cols, cases.DELAY_MAX, np.float32, seed=0x0123456789abcdef, env_base=40, actions=act, inp=inp, input_dim=cases.INPUT_DIM, delay=delay,
                rows=rows, state=state, counts=counts)
    rec, src, dst = k.record(2, 3, reset)
    assert (rec["env0"], rec["n"], rec["ncols"], rec["delay_max"], rec["f32"], rec["act_f32"], rec["env_base"]) == (2, 3, 70, 3, 1, 1, 40)
    assert (rec["key0"], rec["key1"]) == (0x89abcdef, 0x01234567) and rec["cols"] == 1
    assert (rec["actions"], rec["sact"], rec["rows"], rec["srow"]) == (act.ctypes.data, cases.ACT_STRIDE, rows.ctypes.data, 250)
    assert (rec["state"], rec["counts"], rec["delay"], rec["reset"]) == (state.ctypes.data, counts.ctypes.data, delay.ctypes.data, reset.ctypes.data)
    assert src == [(inp.ctypes.data, cases.INPUT_STRIDE, 1), (wide.ctypes.data, wide.shape[1], 0)]
    assert dst == [(f[P.F_PD_PTARGET].ctypes.data, pod.nu), (f[P.F_PD_DTARGET].ctypes.data, pod.nu), (f[P.F_PD_TORQUE].ctypes.data, pod.nu),
                   (wide.ctypes.data + 8 * pod.nq, wide.shape[1])]
    k64 = ae.Call(f, 6, cols, cases.DELAY_MAX, np.float64, actions=act.astype(np.float64), inp=inp.astype(np.float64), input_dim=cases.INPUT_DIM,
                  rows=np.zeros((6, 210)), state=state, counts=counts)
    rec64, src64, _ = k64.record(0, 6)
    assert (rec64["f32"], rec64["act_f32"], rec64["srow"], rec64["delay"], rec64["reset"], src64[0][2]) == (0, 0, 210, 0, 0, 0)
