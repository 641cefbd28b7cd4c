"""Observation rows (phys_batch_obs, include/cassie_phys.h: gather, offset, noise, scale, clip, cast and history in one launch) on the CPU
wave emulator: cassie_obs_kernel launched through the launcher's own records, grid and checks (csrc/small_launch.h) against the definition
restated in numpy and Python integers (tests/obs_check.py), BIT FOR BIT -- every step of a column's value is one individually rounded
operation -- and the launch rules one by one.  All comparisons are on IEEE bits, a NaN equal to a NaN.  The GPU counterpart is
tests/test_obs_gpu.py."""
import numpy as np
import pytest

import obs_cases as cases
import obs_check as oc
import obs_emu_py as oe
from cassie_amd import phys as P

KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
DTYPES = [np.float64, np.float32]


@pytest.fixture(scope="module")
def states(cassie):
    """One state per call of the schedule (shared, left unchanged)."""
    return cases.make_states(cassie)


@pytest.fixture(scope="module")
def terms(cassie):
    return cases.terms_of(cassie.pod)


def fields_of(state):
    return {f: a for f, a in state.items() if f != P.OBS_INPUT}


def run_emulator(terms, states, dtype, schedule=cases.SCHEDULE, nenv=cases.NENV, env_base=0, pad=7, envs=slice(None)):
    """The schedule on the emulator, into rows with a stride `pad` elements beyond the row -> [(rows, frames)] after every call and the raw
    row buffer, whose gaps were filled with -7.25."""
    ncols = len(oc.columns(terms)[0])
    row = cases.HISTORY * ncols
    raw = np.full((nenv, row + pad), -7.25, dtype=dtype)
    frames = np.zeros(nenv, dtype=np.uint32)
    out = []
    for state, (env0, n, refill) in zip(states, schedule):
        st = {f: np.ascontiguousarray(a[envs]) for f, a in state.items()}
        call = oe.Call(fields_of(st), nenv, terms, cases.HISTORY, dtype, cases.SEED, env_base, inp=st[P.OBS_INPUT], input_dim=cases.INPUT_DIM, rows=raw, frames=frames)
        call.observe(env0, n, refill)
        out.append((raw[:, :row].reshape(nenv, cases.HISTORY, ncols).copy(), frames.copy()))
    return out, raw


@pytest.mark.parametrize("which", ["emulator", "numpy"])
def test_philox_known_answers(built, which):
    """Philox4x32-10's published vectors, from the kernel's own routine on the emulator and from the Python restatement."""
    f = oe.philox if which == "emulator" else oc.philox4x32_10
    for counter, key, want in KNOWN:
        assert tuple(f(counter, key)) == want


def test_uniform_map(built):
    """The kernel's map of a word to (-1, 1) is the restatement's, on the ends and on random words."""
    rng = np.random.default_rng(3)
    for w in [0, 1, 0x7fffffff, 0x80000000, 0xffffffff] + [int(v) for v in rng.integers(0, 2 ** 32, 200)]:
        assert oe.uniform(w) == oc.uniform(w) and -1.0 < oe.uniform(w) < 1.0
    assert oc.uniform(0x7fffffff) == -2.0 ** -32 and oc.uniform(0x80000000) == 2.0 ** -32


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulator_against_the_definition(cassie, terms, states, dtype):
    """Seven terms, a frame that crosses the wave's 64 lanes, history 3 over five calls (fill, shift, a sub-range, a refill, shift) on
    states that change: rows and frame counts are the numpy restatement's after every call, bit for bit; envs outside a call's range and
    the gaps of a strided row buffer are untouched."""
    ncols = len(oc.columns(terms)[0])
    assert ncols > 64 and ncols % 64 != 0
    want = cases.reference(terms, states, dtype)
    got, raw = run_emulator(terms, states, dtype)
    for k, ((rows, frames), (wrows, wframes)) in enumerate(zip(got, want)):
        assert np.array_equal(frames, wframes), k
        assert oc.same_bits(rows, wrows), k
    assert list(got[-1][1]) == [3, 5, 5, 5, 3]
    # the gaps of the strided buffer
    assert np.all(raw[:, cases.HISTORY * ncols:] == dtype(-7.25))
    # the first call fills every frame; the second shifts
    assert np.array_equal(got[0][0][:, 0], got[0][0][:, 1]) and np.array_equal(got[0][0][:, 0], got[0][0][:, 2])
    assert np.array_equal(got[1][0][:, 1:], got[0][0][:, :2]) and not np.array_equal(got[1][0][:, 0], got[0][0][:, 0])
    # the third and fourth calls go over [1, 4): envs 0 and 4 keep their rows and counts, byte for byte
    for k in (2, 3):
        for e in (0, 4):
            assert got[k][0][e].tobytes() == got[1][0][e].tobytes() and got[k][1][e] == got[1][1][e]
        assert not np.array_equal(got[k][0][1:4, 0], got[k - 1][0][1:4, 0])
    # the fourth refills env 2 alone
    assert np.array_equal(got[3][0][2, 0], got[3][0][2, 1]) and np.array_equal(got[3][0][2, 0], got[3][0][2, 2])
    assert np.array_equal(got[3][0][1, 1:], got[2][0][1, :2]) and not np.array_equal(got[3][0][1, 0], got[3][0][1, 1])
    # the clipped term clips some entries and passes others
    first = oc.columns(terms)[1]
    clip = got[-1][0][:, :, first[5]: first[5] + 6]
    assert (np.abs(clip) == 0.5).any() and (np.abs(clip) < 0.5).any() and np.abs(clip).max() == 0.5


def test_clip_passes_nan_and_orders_bounds(built):
    """clampd's rule: a NaN source passes through the clip, +-inf bounds clip nothing, -0.0 stays -0.0."""
    x = np.array([[np.nan, -0.0, 3.0, -3.0, np.inf]])
    t = [P.obs_copy(P.F_QPOS, 0, 5, lo=-1.0, hi=1.0), P.obs_copy(P.F_QPOS, 0, 5)]
    rows, frames = np.zeros((1, 10)), np.zeros(1, dtype=np.uint32)
    oe.Call({P.F_QPOS: x}, 1, t, 1, np.float64, rows=rows, frames=frames).observe()
    want = oc.Obs(t, 1, 1, np.float64).observe({P.F_QPOS: x})
    assert oc.same_bits(rows.reshape(1, 1, 10), want)
    assert np.isnan(rows[0, 0]) and np.signbit(rows[0, 1]) and list(rows[0, 2:5]) == [1.0, -1.0, 1.0] and rows[0, 9] == np.inf


def test_sharding_by_env_base(cassie, terms, states):
    """A batch of 4 envs with env_base 4 and envs 4 .. 7 of a batch of 8 with the same seed, given the same states, make the same rows."""
    rng = np.random.default_rng(5)
    big = []
    for s in states[:3]:
        idx = np.array([0, 1, 2, 3, 4, 0, 1, 2])
        st = {f: a[idx].copy() for f, a in s.items()}
        st[P.F_QVEL][5:] += rng.uniform(-0.1, 0.1, st[P.F_QVEL][5:].shape)
        big.append(st)
    sched = ((0, 8, None), (0, 8, None), (0, 8, None))
    whole, _ = run_emulator(terms, big, np.float32, schedule=sched, nenv=8)
    shard, _ = run_emulator(terms, big, np.float32, schedule=((0, 4, None),) * 3, nenv=4, env_base=4, envs=slice(4, 8))
    other, _ = run_emulator(terms, big, np.float32, schedule=((0, 4, None),) * 3, nenv=4, env_base=0, envs=slice(4, 8))
    for k in range(3):
        assert oc.same_bits(shard[k][0], whole[k][0][4:8])
    assert not oc.same_bits(other[2][0], whole[2][0][4:8])         # (without the offset the draws are other envs')
    assert oc.same_bits(whole[2][0], cases.reference(terms, big, np.float32, sched, nenv=8)[2][0])


def test_one_call_or_two_ranges(cassie, terms, states):
    """One call over the batch and the same work as two calls over two ranges make the same rows and counts."""
    one, _ = run_emulator(terms, states[:3], np.float32, schedule=((0, 5, None),) * 3)
    ncols = one[0][0].shape[2]
    raw, frames = np.zeros((5, cases.HISTORY * ncols), dtype=np.float32), np.zeros(5, dtype=np.uint32)
    for s in states[:3]:
        call = oe.Call(fields_of(s), 5, terms, cases.HISTORY, np.float32, cases.SEED, inp=s[P.OBS_INPUT], input_dim=cases.INPUT_DIM, rows=raw, frames=frames)
        call.observe(2, 3)
        call.observe(0, 2)
    assert oc.same_bits(raw.reshape(one[2][0].shape), one[2][0]) and np.array_equal(frames, one[2][1])


def test_noise_words_never_coincide(cassie, terms):
    """Over the 5 x ncols x 5 (env, column, frame) triples of the case no two noise words coincide."""
    ncols = len(oc.columns(terms)[0])
    words = [oc.noise_word(cases.SEED, 0, e, c, f) for e in range(5) for c in range(ncols) for f in range(5)]
    assert len(set(words)) == len(words) == 25 * ncols


def test_uniform_law():
    """2^16 draws of xi (the restatement alone): strictly inside (-1, 1), mean within 4 / sqrt(3 * 2^16) of zero (four standard errors
    of the mean of a uniform law of variance 1/3), mean square within 0.01 of 1/3."""
    xi = np.array([oc.uniform(oc.noise_word(cases.SEED, 0, e, c, 7)) for e in range(256) for c in range(256)])
    assert xi.size == 2 ** 16 and np.all(xi > -1.0) and np.all(xi < 1.0)
    assert abs(xi.mean()) < 4.0 / np.sqrt(3.0 * 2 ** 16)
    assert abs((xi * xi).mean() - 1.0 / 3.0) < 0.01


# ---- the launch rules ----

def held(cassie, nenv=3):
    """What a fresh batch holds: the state and command fields, not the scan, the rays, the probes, the sums or the derived block."""
    pod = cassie.pod
    dims = {P.F_QPOS: pod.nq, P.F_QVEL: pod.nv, P.F_QACC: pod.nv, P.F_TIME: 1, P.F_CTRL: pod.nu, P.F_SENSORDATA: pod.nsensordata, P.F_XPOS: 3 * pod.nbody,
            P.F_XQUAT: 4 * pod.nbody, P.F_DEPTH: 16}
    return {f: np.zeros((nenv, d)) for f, d in dims.items()}


def refusal(cassie, t, nenv=3, **kw):
    return oe.Call(held(cassie, nenv), nenv, t, **kw).check()[0]


def test_configure_refusals(cassie):
    pod = cassie.pod
    ok = P.obs_copy(P.F_QPOS, 0, 3)
    assert refusal(cassie, [ok]) is None
    bad = lambda t, word, **kw: word in (refusal(cassie, t if isinstance(t, list) else [t], **kw) or "")
    # unknown kind or field
    assert bad((7,) + ok[1:], "kind")
    assert bad(P.obs_copy(P.F_PROBES + 1, 0, 1), "a term's field is") and bad(P.obs_copy(-3, 0, 1), "a term's field is")
    assert bad(P.obs_rot_inv(P.F_QVEL, 0, 99, 3), "a term's field is")
    # the depth image is no source, even where the batch holds it
    assert bad(P.obs_copy(P.F_DEPTH, 0, 1), "PHYS_F_DEPTH") and bad(P.obs_rot_inv(P.F_QVEL, 0, P.F_DEPTH, 0), "PHYS_F_DEPTH")
    # fields the batch does not hold yet
    for f in (P.F_HEIGHT_SCAN, P.F_RAYS, P.F_PROBES, P.F_STEP_SUMS, P.F_DERIVED):
        assert bad(P.obs_copy(f, 0, 1), "does not hold yet")
    # beyond the field's row
    assert refusal(cassie, [P.obs_copy(P.F_QPOS, pod.nq - 2, 2)]) is None and bad(P.obs_copy(P.F_QPOS, pod.nq - 2, 3), "index + count")
    assert bad(P.obs_copy(P.F_QPOS, -1, 2), "index + count") and bad(P.obs_copy(P.F_QPOS, 0, 0), "at least one column")
    assert refusal(cassie, [P.obs_rot_inv(P.F_QVEL, pod.nv - 3, P.F_QPOS, pod.nq - 4)]) is None
    assert bad(P.obs_rot_inv(P.F_QVEL, pod.nv - 2, P.F_QPOS, 3), "index + 3") and bad(P.obs_rot_inv(P.F_QVEL, 0, P.F_QPOS, pod.nq - 3), "qindex + 4")
    # the constant vector belongs to a ROT_INV's field
    assert bad(P.obs_copy(P.OBS_CONST, 0, 3), "PHYS_OBS_CONST") and bad(P.obs_rot_inv(P.F_QVEL, 0, P.OBS_CONST, 0), "PHYS_OBS_CONST")
    assert refusal(cassie, [P.obs_rot_inv(P.OBS_CONST, 0, P.F_QPOS, 3, vec=(0, 0, -1))]) is None
    # non-finite constants, a negative amplitude, bounds out of order
    for name in ("offset", "scale", "noise"):
        for v in (np.nan, np.inf):
            assert bad(P.obs_copy(P.F_QPOS, 0, 1, **{name: v}), "finite offset, scale and noise")
    assert bad(P.obs_rot_inv(P.OBS_CONST, 0, P.F_QPOS, 3, vec=(0, np.inf, 0)), "constant vector") and bad(P.obs_rot_inv(P.OBS_CONST, 0, P.F_QPOS, 3, vec=(np.nan, 0, 0)), "constant vector")
    assert bad(P.obs_copy(P.F_QPOS, 0, 1, noise=-0.1), "noise is an amplitude")
    assert bad(P.obs_copy(P.F_QPOS, 0, 1, lo=1.0, hi=0.5), "lo <= hi") and bad(P.obs_copy(P.F_QPOS, 0, 1, lo=np.nan), "lo <= hi")
    assert refusal(cassie, [P.obs_copy(P.F_QPOS, 0, 1, lo=-np.inf, hi=np.inf), P.obs_copy(P.F_QPOS, 0, 1, lo=0.5, hi=0.5)]) is None
    # too many columns, too long a row, the history, the dtype
    full = [P.obs_copy(P.F_QPOS, 0, pod.nq)] * (P.OBS_MAXCOLS // pod.nq)
    rest = P.OBS_MAXCOLS - len(full) * pod.nq
    assert refusal(cassie, full + [P.obs_copy(P.F_QPOS, 0, rest)]) is None and bad(full + [P.obs_copy(P.F_QPOS, 0, rest + 1)], "PHYS_OBS_MAXCOLS")
    assert bad(full, "65536", history=64) and refusal(cassie, [P.obs_copy(P.F_QPOS, 0, 16)] * 64, history=64) is None
    assert bad(ok, "history", history=0) and bad(ok, "history", history=65)
    assert bad(ok, "dtype", dtype=2) and bad(ok, "dtype", dtype=np.int32) and refusal(cassie, [ok], dtype=np.float64) is None
    # no terms releases; a negative count is refused
    assert refusal(cassie, []) is None and bad([ok], "0 .. 2048 terms", nterms=-1)
    # more sources than a call carries
    many = [P.obs_copy(f, 0, 1) for f in (P.F_QPOS, P.F_QVEL, P.F_QACC, P.F_TIME, P.F_CTRL, P.F_SENSORDATA, P.F_XPOS, P.F_XQUAT, P.OBS_INPUT)]
    assert refusal(cassie, many) is None
    wide = {f: np.zeros((3, 4)) for f in range(17)}
    assert oe.Call(wide, 3, [P.obs_copy(f, 0, 1) for f in range(16)]).check()[0] is None
    assert "16 distinct" in oe.Call(wide, 3, [P.obs_copy(f, 0, 1) for f in range(17)]).check()[0]


def test_bind_refusals(cassie):
    t = [P.obs_copy(P.F_QPOS, 0, 5), P.obs_copy(P.OBS_INPUT, 2, 3)]
    frames = np.zeros(3, dtype=np.uint32)
    assert "row stride" in oe.Call(held(cassie), 3, t, history=2, rows=np.zeros((3, 15), dtype=np.float32), frames=frames).check()[0]
    assert oe.Call(held(cassie), 3, t, history=2, rows=np.zeros((3, 16), dtype=np.float32), frames=frames).check()[0] is None
    c = oe.Call(held(cassie), 3, t)
    c.bind_input(np.zeros((3, 4), dtype=np.float32), dtype=2)
    assert "input's dtype" in c.check()[0]
    c.bind_input(np.zeros((3, 4), dtype=np.float32), input_dim=0)
    assert "at least one element" in c.check()[0]
    c.bind_input(np.zeros((3, 4), dtype=np.float32), input_dim=4, stride=3)
    assert "at least one element" in c.check()[0]


def test_call_refusals(cassie):
    pod = cassie.pod
    t = [P.obs_copy(P.F_QPOS, 0, 5), P.obs_copy(P.OBS_INPUT, 2, 3)]
    rows, frames = np.zeros((3, 8), dtype=np.float32), np.zeros(3, dtype=np.uint32)
    inp = np.zeros((3, 5), dtype=np.float32)
    c = oe.Call(held(cassie), 3, t, inp=inp, rows=rows, frames=frames)
    assert c.call_check(0, 3) is None and c.call_check(3, 0) is None and c.call_check(1, 2) is None
    assert "not configured" in c.call_check(0, 3, configured=False)
    for env0, n in ((-1, 2), (0, 4), (2, 2), (0, -1)):
        assert "out of bounds" in c.call_check(env0, n)
    # a source whose row has changed, or gone, since the configure call
    assert "has changed" in c.call_check(0, 3, now={P.F_QPOS: (np.zeros((3, pod.nq + 1)), pod.nq + 1)})
    assert "has changed" in c.call_check(0, 3, now={P.F_QPOS: (None, 0)})
    assert c.call_check(0, 3, now={P.F_QVEL: (None, 0)}) is None      # (no term reads it)
    # the input: nothing bound, or bound too short
    assert "no input bound" in oe.Call(held(cassie), 3, t, rows=rows, frames=frames).call_check(0, 3)
    assert "shorter" in oe.Call(held(cassie), 3, t, inp=inp, input_dim=4, rows=rows, frames=frames).call_check(0, 3)
    assert oe.Call(held(cassie), 3, t, inp=inp, input_dim=5, rows=rows, frames=frames).call_check(0, 3) is None
    # the emulator's launch refuses the same
    assert oe.lib().emu_obs(c.a, 0, 4, None, 0) == -1 and b"out of bounds" in oe.lib().emu_obs_last_refusal()


def test_layout_dims_and_columns(cassie, terms):
    pod = cassie.pod
    ns = min(70, pod.nsensordata)
    why, rec, first = oe.Call(held(cassie), 3, terms, history=3).check()
    assert why is None
    assert first == [0, 2, 2 + ns, 5 + ns, 8 + ns, 12 + ns, 18 + ns] == oc.columns(terms)[1]
    assert (rec["nterms"], rec["ncols"], rec["history"], rec["dtype"], rec["input_need"]) == (7, 18 + ns + pod.nv, 3, 4, 5)
    assert rec["slot_field"] == [P.F_QPOS, P.F_SENSORDATA, P.F_QVEL, P.OBS_INPUT] and rec["slot_dim"] == [pod.nq, pod.nsensordata, pod.nv, 0]
    cols = oe.Call(held(cassie), 3, terms, history=3).columns()
    assert len(cols) == 18 + ns + pod.nv
    assert [int(v) for v in cols["slot"][:3]] == [0, 0, 1] and [int(v) for v in cols["elem"][:4]] == [7, 8, 0, 1] and np.all(cols["comp"][: 2 + ns] == -1)
    rot = cols[2 + ns: 5 + ns]
    assert list(rot["comp"]) == [0, 1, 2] and np.all(rot["slot"] == 2) and np.all(rot["elem"] == 0) and np.all(rot["qslot"] == 0) and np.all(rot["qelem"] == 3)
    grav = cols[5 + ns: 8 + ns]
    assert np.all(grav["slot"] == -1) and np.all(grav["vec"] == [0, 0, -1]) and list(grav["comp"]) == [0, 1, 2]
    assert np.all(cols["noise"][2: 2 + ns] == 0.05) and np.all(cols["scale"][2: 2 + ns] == 2.0) and np.all(cols["offset"][2: 2 + ns] == 0.1)
    assert np.all(cols["lo"][12 + ns: 18 + ns] == -0.5) and np.all(cols["hi"][12 + ns: 18 + ns] == 0.5) and np.all(np.isinf(cols["lo"][: 12 + ns]))


def test_launch_record(cassie, terms):
    """The grid, and the IO's pointers and strides: the batch's own dense buffers, a bound tensor with its row stride, the input, the rows."""
    assert [oe.grid(n) for n in (0, 1, 5, 64, 65, 4096)] == [0, 1, 5, 64, 64, 64] and oe.OBS_GRID == 64
    pod = cassie.pod
    f = held(cassie, 6)
    wide = np.zeros((6, pod.nq + pod.nv + 3))
    f[P.F_QPOS] = wide[:, : pod.nq]            # (bound as column blocks of one tensor)
    f[P.F_QVEL] = wide[:, pod.nq: pod.nq + pod.nv]
    inp = np.zeros((6, cases.INPUT_STRIDE), dtype=np.float32)
    rows, frames, refill = np.zeros((6, 400), dtype=np.float32), np.zeros(6, dtype=np.uint32), np.zeros(3, dtype=np.int32)
    c = oe.Call(f, 6, terms, cases.HISTORY, np.float32, seed=0x0123456789abcdef, env_base=40, inp=inp, input_dim=cases.INPUT_DIM, rows=rows, frames=frames)
    rec, src = c.record(2, 3, refill)
    ncols = len(oc.columns(terms)[0])
    assert (rec["env0"], rec["n"], rec["ncols"], rec["history"], rec["f32"], rec["env_base"]) == (2, 3, ncols, 3, 1, 40)
    assert (rec["key0"], rec["key1"]) == (0x89abcdef, 0x01234567) and rec["cols"] == 1
    assert (rec["rows"], rec["srow"], rec["frames"], rec["refill"]) == (rows.ctypes.data, 400, frames.ctypes.data, refill.ctypes.data)
    assert src == [(wide.ctypes.data, wide.shape[1], 0), (f[P.F_SENSORDATA].ctypes.data, pod.nsensordata, 0),
                   (wide.ctypes.data + 8 * pod.nq, wide.shape[1], 0), (inp.ctypes.data, cases.INPUT_STRIDE, 1)]
    rec64, src64 = oe.Call(f, 6, terms, cases.HISTORY, np.float64, inp=inp.astype(np.float64), input_dim=cases.INPUT_DIM,
                           rows=np.zeros((6, 3 * ncols)), frames=frames).record(0, 6)
    assert (rec64["f32"], rec64["srow"], rec64["refill"], src64[3][2]) == (0, 3 * ncols, 0, 0)


def test_strided_sources_read_where_bound(cassie, terms, states):
    """Sources bound as column blocks of one wide tensor give the rows of dense sources."""
    s = states[0]
    pod = cassie.pod
    wide = np.full((5, pod.nq + pod.nv + pod.nsensordata + 5), np.nan)
    wide[:, : pod.nq], wide[:, pod.nq: pod.nq + pod.nv], wide[:, pod.nq + pod.nv: -5] = s[P.F_QPOS], s[P.F_QVEL], s[P.F_SENSORDATA]
    bound = {P.F_QPOS: wide[:, : pod.nq], P.F_QVEL: wide[:, pod.nq: pod.nq + pod.nv], P.F_SENSORDATA: wide[:, pod.nq + pod.nv: -5]}
    ncols = len(oc.columns(terms)[0])
    out = []
    for f in (fields_of(s), bound):
        rows, frames = np.zeros((5, 3 * ncols)), np.zeros(5, dtype=np.uint32)
        oe.Call(f, 5, terms, cases.HISTORY, np.float64, cases.SEED, inp=s[P.OBS_INPUT], input_dim=cases.INPUT_DIM, rows=rows, frames=frames).observe()
        out.append(rows)
    assert oc.same_bits(out[0], out[1]) and oc.same_bits(out[0].reshape(5, 3, ncols), cases.reference(terms, [s], np.float64, cases.SCHEDULE[:1])[0][0])


def test_frames_wrap_and_resume(cassie, terms, states):
    """The count is a uint32 that wraps, and a run resumed from downloaded counts draws what the first run drew."""
    s = states[0]
    ncols = len(oc.columns(terms)[0])
    rows, frames = np.zeros((5, 3 * ncols), dtype=np.float32), np.full(5, 0xffffffff, dtype=np.uint32)
    c = oe.Call(fields_of(s), 5, terms, cases.HISTORY, np.float32, cases.SEED, inp=s[P.OBS_INPUT], input_dim=cases.INPUT_DIM, rows=rows, frames=frames)
    c.observe()
    assert np.all(frames == 0)
    ref = oc.Obs(terms, 5, cases.HISTORY, np.float32, cases.SEED)
    ref.frames[:] = 0xffffffff
    assert oc.same_bits(rows.reshape(5, 3, ncols), ref.observe(s)) and np.all(ref.frames == 0)
