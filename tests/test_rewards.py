"""Reward rows (phys_batch_reward, include/cassie_phys.h: errors, norms, shapes, weights, gates, the clip and the episode returns in one
launch) on the CPU wave emulator: cassie_reward_kernel launched through the launcher's own records, grid and checks
(csrc/small_launch.h) against the definition restated in numpy (tests/rewards_check.py), BIT FOR BIT -- every step of a term is one
individually rounded operation -- expn against an exact reference, and the launch rules one by one.  All comparisons are on IEEE bits, a
NaN equal to a NaN.  The GPU counterpart is tests/test_rewards_gpu.py."""
import decimal

import numpy as np
import pytest

import rewards_cases as cases
import rewards_check as rc
import rewards_emu_py as re_
from cassie_amd import phys as P

DTYPES = [np.float64, np.float32]
FILL = -7.25
NGRID = 60001                      # the points of expn's grid over [0, 708]
EXPN_BOUND_ULP = 1.5               # the largest error measured on that grid (1.06 ulp) rounded up to the next half ulp


@pytest.fixture(scope="module")
def states(cassie):
    """One state per call of the schedule (shared, left unchanged)."""
    return cases.make_states(cassie)


@pytest.fixture(scope="module")
def terms(cassie):
    return cases.terms_of(cassie.pod)


def fields_of(state):
    return {f: a for f, a in state.items() if f != P.REW_INPUT}


def run_emulator(terms, states, dtype, schedule=cases.SCHEDULE, nenv=cases.NENV, envs=slice(None), pad=5):
    """The schedule on the emulator, the rewards into column 1 of a [nenv][3] buffer and the term rows into rows `pad` elements wider than
    the terms, both filled with FILL -> [(rewards, term rows, ret, final)] after every call and the two raw buffers."""
    nt = len(terms)
    raw, rows = np.full((nenv, 3), FILL, dtype=dtype), np.full((nenv, nt + pad), FILL, dtype=dtype)
    ret, fin = np.zeros(nenv), np.zeros(nenv)
    out = []
    for state, (env0, n, reset) in zip(states, schedule):
        st = {f: np.ascontiguousarray(a[envs]) for f, a in state.items()}
        call = re_.Call(fields_of(st), nenv, terms, dtype, cases.LO, cases.HI, inp=st[P.REW_INPUT], input_dim=cases.INPUT_DIM, rew=raw[:, 1], rows=rows, ret=ret, fin=fin)
        call.reward(env0, n, reset)
        out.append((raw[:, 1].copy(), rows[:, :nt].copy(), ret.copy(), fin.copy()))
    return out, raw, rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulator_against_the_definition(cassie, terms, states, dtype):
    """Thirteen terms over five calls (the batch twice, a sub-range, two episodes reset, the batch again) on states that change: the
    rewards, the term rows, ret and final are the numpy restatement's after every call, bit for bit; envs outside a call's range and the
    gaps of the strided buffers are untouched; the case holds what it says it holds."""
    want = cases.reference(terms, states, dtype)
    got, raw, rows = run_emulator(terms, states, dtype)
    for k, (g, w) in enumerate(zip(got, want)):
        for a, b, name in zip(g, w, ("rewards", "term rows", "ret", "final")):
            assert rc.same_bits(a, b), (k, name)
    nt = len(terms)
    assert np.all(raw[:, 0] == dtype(FILL)) and np.all(raw[:, 2] == dtype(FILL)) and np.all(rows[:, nt:] == dtype(FILL))
    # what the case is made of: every kind, norm (with and without root), shape, a deadband, both gates, the three targets, counts 1 and 64
    t = P.rew_terms(terms)
    assert set(t["kind"]) == {P.REW_VEC, P.REW_ROT_INV, P.REW_QUAT} and set(t["shape"]) == {P.REW_LINEAR, P.REW_EXP, P.REW_RATIONAL}
    vec = t[t["kind"] != P.REW_QUAT]
    assert {(int(a), int(b)) for a, b in zip(vec["norm"], vec["root"])} == {(n, r) for n in range(3) for r in range(2)}
    assert (t["dead"] > 0).any() and {1, 64} <= set(t["count"])
    assert {P.REW_INPUT, P.REW_NONE} < set(t["gfield"]) and (t["gfield"] >= 0).any()
    assert {P.REW_INPUT, P.REW_CONST} < set(t["tfield"]) and (t["tfield"] >= 0).any()
    # the env past expn's cut: its steep term contributes +0.0 exactly, the others' do not
    steep = got[0][1][:, 11]
    assert steep[cases.ENV_CUT] == 0 and not np.signbit(steep[cases.ENV_CUT]) and np.all(np.delete(steep, [cases.ENV_CUT, cases.ENV_NAN]) > 0)
    assert 50.0 * float(states[0][P.F_QPOS][cases.ENV_CUT, :2] @ states[0][P.F_QPOS][cases.ENV_CUT, :2]) > 708
    # the NaN env: its SUMABS term, reward and return are NaN, its MAXABS term passes over the NaN, nobody else's is
    for k in range(5):
        nan = np.isnan(got[k][0])
        assert nan[cases.ENV_NAN] and nan.sum() == 1 and np.isnan(got[k][2][cases.ENV_NAN])
    assert np.isnan(got[0][1][cases.ENV_NAN, 8]) and np.isfinite(got[0][1][cases.ENV_NAN, 5])
    # the clip bites somewhere and not everywhere
    r = np.delete(got[-1][0], cases.ENV_NAN)
    assert (r == dtype(cases.HI)).any() or (r == dtype(cases.LO)).any()
    assert ((r > dtype(cases.LO)) & (r < dtype(cases.HI))).any()
    # the third call goes over [1, 4): envs 0, 4 and 5 keep everything, byte for byte
    for e in (0, 4, 5):
        for a, b in zip(got[2], got[1]):
            assert a[e].tobytes() == b[e].tobytes()
    assert not np.array_equal(got[2][0][[1, 3]], got[1][0][[1, 3]])
    # the fourth moves the returns of envs 1 and 4 to final and restarts them; everybody else's goes on
    assert rc.same_bits(got[3][3][[1, 4]], got[2][2][[1, 4]]) and np.all(got[3][3][[0, 3, 5]] == 0)
    if dtype is np.float64:
        assert rc.same_bits(got[3][2][[1, 4]], got[3][0][[1, 4]])          # (+0.0 + r)
    for e in (0, 3, 5):
        assert got[3][2][e] != got[2][2][e] and got[3][2][e] != float(got[3][0][e])
    assert rc.same_bits(got[4][3], got[3][3])


def test_returns_sum_the_uncast_reward(cassie, terms, states):
    """ret adds the clipped fp64 reward, not the float32 element written: the float32 run's returns are the float64 run's."""
    a, _, _ = run_emulator(terms, states, np.float32)
    b, _, _ = run_emulator(terms, states, np.float64)
    assert rc.same_bits(a[-1][2], b[-1][2]) and rc.same_bits(a[-1][3], b[-1][3])
    assert rc.same_bits(a[-1][0], b[-1][0].astype(np.float32)) and not np.array_equal(a[-1][0].astype(np.float64), b[-1][0], equal_nan=True)


def test_one_call_or_two_ranges(cassie, terms, states):
    """A reward does not depend on how the batch is cut: ranges (0, 3) and (3, 3) give the whole call's bits."""
    one, _, _ = run_emulator(terms, states[:2], np.float64, schedule=((0, 6, None), (0, 6, (1, 0, 0, 1, 0, 0))))
    nt = len(terms)
    rew, rows, ret, fin = np.zeros(6), np.zeros((6, nt)), np.zeros(6), np.zeros(6)
    for s, reset in zip(states[:2], (None, (1, 0, 0, 1, 0, 0))):
        call = re_.Call(fields_of(s), 6, terms, np.float64, cases.LO, cases.HI, inp=s[P.REW_INPUT], input_dim=cases.INPUT_DIM, rew=rew, rows=rows, ret=ret, fin=fin)
        call.reward(3, 3, None if reset is None else reset[3:])
        call.reward(0, 3, None if reset is None else reset[:3])
    for a, b in zip((rew, rows, ret, fin), one[1]):
        assert rc.same_bits(a, b)


def test_more_envs_than_a_wave_and_any_grid(built):
    """150 envs -- three workgroups, the last one partly empty -- and the same range walked by a grid of one and of two."""
    rng = np.random.default_rng(4)
    q = rng.uniform(-1.0, 1.0, (150, 9))
    t = [P.rew_vec(P.F_QPOS, 0, 9, target=0.1, shape=P.REW_EXP, k=2.0, weight=0.5), P.rew_quat(P.F_QPOS, 2, weight=0.25, gate=(P.F_QPOS, 8)),
         P.rew_rot_inv(P.F_QPOS, 6, P.F_QPOS, 1, norm=P.REW_MAXABS, root=True)]
    want = rc.Rewards(t, 150, np.float64)
    want.reward({P.F_QPOS: q}, 10, 137)
    assert re_.grid(137) == 3
    for grid in (0, 1, 2):
        rew, ret, fin = np.zeros(150), np.zeros(150), np.zeros(150)
        re_.Call({P.F_QPOS: q}, 150, t, np.float64, rew=rew, ret=ret, fin=fin).reward(10, 137, grid=grid)
        assert rc.same_bits(rew, want.rew) and rc.same_bits(ret, want.ret) and np.all(rew[:10] == 0) and np.all(rew[147:] == 0) and np.all(rew[10:147] != 0)


def test_clip_nan_and_deadband(built):
    """The clip passes a NaN and orders its bounds; the deadband passes a NaN, zeroes what is inside and shifts what is outside."""
    x = np.array([[np.nan, 0.0], [0.3, 0.0], [-0.3, 0.0], [0.05, 0.0], [-2.0, 0.0], [2.0, 0.0]])
    t = [P.rew_vec(P.F_QPOS, 0, 1, dead=0.1, norm=P.REW_SUMABS)]
    rew, rows, ret, fin = np.zeros(6), np.zeros((6, 1)), np.zeros(6), np.zeros(6)
    re_.Call({P.F_QPOS: x}, 6, t, np.float64, lo=-1.0, hi=1.0, rew=rew, rows=rows, ret=ret, fin=fin).reward()
    want = rc.Rewards(t, 6, np.float64, -1.0, 1.0)
    want.reward({P.F_QPOS: x})
    assert rc.same_bits(rew, want.rew) and rc.same_bits(rows, want.rows)
    assert np.isnan(rew[0]) and rew[1] == np.float64(0.3) - np.float64(0.1) and rew[2] == rew[1] and rew[3] == 0 and rew[4] == 1.0 and rows[4, 0] == 1.9
    t = [P.rew_vec(P.F_QPOS, 0, 1, weight=-1.0)]
    re_.Call({P.F_QPOS: x}, 6, t, np.float64, lo=-1.0, hi=np.inf, rew=rew, ret=ret, fin=fin).reward()
    assert np.isnan(rew[0]) and rew[4] == -1.0 and rew[1] == -(np.float64(0.3) * np.float64(0.3))


# ---- expn ----

def expn_grid():
    """NGRID points over [0, 708], and small arguments down to 1e-12."""
    return np.concatenate([np.linspace(0.0, 708.0, NGRID), np.logspace(-12, 0, 600)])


def test_expn_emulator_is_the_restatement(built):
    """The kernel's expn on the emulator equals the numpy restatement bit for bit on the grid and at the edges: 0, ln2 / 2 on both sides,
    708, the next double above 708, inf and NaN (and, beyond the issue, below zero down to the other cut)."""
    a = expn_grid()
    assert a.size >= 50000 + 600
    assert rc.same_bits(re_.expn(a), rc.expn_array(a))
    half = np.float64(0.34657359027997264)          # ln2 / 2
    edges = np.array([0.0, -0.0, np.nextafter(half, 0), half, np.nextafter(half, 1), 708.0, np.nextafter(708.0, 709), 1e300, np.inf, np.nan,
                      -1e-300, -1.0, -708.0, np.nextafter(-708.0, -709), -np.inf, 5e-324, 2.0 ** -1022])
    got = re_.expn(edges)
    assert rc.same_bits(got, np.array([rc.expn(v) for v in edges]))
    assert rc.same_bits(rc.expn_array(edges[np.abs(edges) <= 708]), got[np.abs(edges) <= 708])      # (the vectorised form is the scalar one)
    assert got[0] == 1.0 and got[1] == 1.0 and got[5] > 0 and got[5] >= 2.0 ** -1022 and list(got[6:9]) == [0.0, 0.0, 0.0] and not np.signbit(got[6])
    assert np.isnan(got[9]) and got[13] == np.inf and got[14] == np.inf and np.isfinite(got[12])


def test_expn_accuracy_and_order():
    """The restatement against exp(-a) at 60 digits on the grid: the largest error in ulp of the exact value is within EXPN_BOUND_ULP
    (the algorithm is deterministic: the margin covers nothing but the grid's sampling); expn(0) == 1; sorted arguments never produce an
    increase."""
    a = np.sort(expn_grid())
    v = rc.expn_array(a)
    assert v[0] == 1.0 and np.all(np.diff(v) <= 0) and np.all(v >= 2.0 ** -1022)
    decimal.getcontext().prec = 60
    worst = 0.0
    for ai, vi in zip(a, v):
        exact = (-decimal.Decimal(float(ai))).exp()
        ulp = decimal.Decimal(float(np.spacing(np.float64(float(exact)))))
        worst = max(worst, float(abs(decimal.Decimal(float(vi)) - exact) / ulp))
    print("expn: largest error %.4f ulp over %d points" % (worst, a.size))
    assert worst <= EXPN_BOUND_ULP


# ---- the launch rules ----

def held(cassie, nenv=3):
    """What a fresh batch holds: the state and command fields, not the scan, the rays, the probes, the sums or the derived block."""
    pod = cassie.pod
    dims = {P.F_QPOS: pod.nq, P.F_QVEL: pod.nv, P.F_QACC: pod.nv, P.F_TIME: 1, P.F_CTRL: pod.nu, P.F_SENSORDATA: pod.nsensordata, P.F_XPOS: 3 * pod.nbody,
            P.F_XQUAT: 4 * pod.nbody, P.F_DEPTH: 16}
    return {f: np.zeros((nenv, d)) for f, d in dims.items()}


def refusal(cassie, t, nenv=3, **kw):
    return re_.Call(held(cassie, nenv), nenv, t, **kw).check()[0]


def edit(term, **kw):
    """A term tuple with named members of REW_TERM_DTYPE replaced."""
    names = P.REW_TERM_DTYPE.names
    return tuple(kw.get(n, v) for n, v in zip(names, term))


def test_configure_refusals(cassie):
    pod = cassie.pod
    ok = P.rew_vec(P.F_QPOS, 0, 3)
    assert refusal(cassie, [ok]) is None
    bad = lambda t, word, **kw: word in (refusal(cassie, t if isinstance(t, list) else [t], **kw) or "")
    # unknown kind, norm, shape or field
    assert bad(edit(ok, kind=3), "kind") and bad(edit(ok, kind=-1), "kind")
    assert bad(edit(ok, norm=3), "norm") and bad(edit(ok, shape=3), "shape") and bad(edit(ok, shape=-1), "shape")
    assert refusal(cassie, [edit(P.rew_quat(P.F_QPOS, 3), norm=9)]) is None             # (a QUAT has no norm)
    for name in ("field", "tfield", "gfield"):
        assert bad(edit(ok, **{name: P.F_PROBES + 1}), "PHYS_F_* fields") and bad(edit(ok, **{name: -4}), "PHYS_F_* fields")
    assert bad(P.rew_rot_inv(P.F_QVEL, 0, 99, 3), "PHYS_F_* fields")
    # the depth image is no source, even where the batch holds it
    assert bad(P.rew_vec(P.F_DEPTH, 0, 1), "PHYS_F_DEPTH") and bad(P.rew_rot_inv(P.F_QVEL, 0, P.F_DEPTH, 0), "PHYS_F_DEPTH")
    assert bad(P.rew_vec(P.F_QPOS, 0, 1, tfield=P.F_DEPTH), "PHYS_F_DEPTH") and bad(P.rew_vec(P.F_QPOS, 0, 1, gate=(P.F_DEPTH, 0)), "PHYS_F_DEPTH")
    # fields the batch does not hold yet
    for f in (P.F_HEIGHT_SCAN, P.F_RAYS, P.F_PROBES, P.F_STEP_SUMS, P.F_DERIVED):
        assert bad(P.rew_vec(f, 0, 1), "does not hold yet") and bad(P.rew_vec(P.F_QPOS, 0, 1, gate=(f, 0)), "does not hold yet")
    # slices beyond a row
    assert refusal(cassie, [P.rew_vec(P.F_QPOS, pod.nq - 2, 2)]) is None and bad(P.rew_vec(P.F_QPOS, pod.nq - 2, 3), "index + count")
    assert bad(P.rew_vec(P.F_QPOS, -1, 2), "index + count")
    assert bad(P.rew_vec(P.F_QPOS, 0, 0), "1 .. 64 elements") and bad(P.rew_vec(P.REW_INPUT, 0, 65), "1 .. 64 elements")
    assert refusal(cassie, [P.rew_vec(P.REW_INPUT, 0, 64)]) is None
    assert refusal(cassie, [P.rew_rot_inv(P.F_QVEL, pod.nv - 3, P.F_QPOS, pod.nq - 4)]) is None
    assert bad(P.rew_rot_inv(P.F_QVEL, pod.nv - 2, P.F_QPOS, 3), "index + 3") and bad(P.rew_rot_inv(P.F_QVEL, 0, P.F_QPOS, pod.nq - 3), "qindex + 4")
    assert refusal(cassie, [P.rew_quat(P.F_QPOS, pod.nq - 4)]) is None and bad(P.rew_quat(P.F_QPOS, pod.nq - 3), "index + 4")
    assert refusal(cassie, [P.rew_vec(P.F_QPOS, 0, 4, tfield=P.F_QVEL, tindex=pod.nv - 4)]) is None
    assert bad(P.rew_vec(P.F_QPOS, 0, 4, tfield=P.F_QVEL, tindex=pod.nv - 3), "tindex") and bad(P.rew_quat(P.F_QPOS, 3, tfield=P.F_QVEL, tindex=pod.nv - 3), "tindex")
    assert refusal(cassie, [P.rew_vec(P.F_QPOS, 0, 1, gate=(P.F_TIME, 0))]) is None and bad(P.rew_vec(P.F_QPOS, 0, 1, gate=(P.F_TIME, 1)), "gindex")
    # CONST and NONE where they are not allowed
    assert bad(P.rew_vec(P.REW_CONST, 0, 3), "PHYS_REW_CONST") and bad(P.rew_quat(P.REW_CONST, 0), "PHYS_REW_CONST")
    assert bad(P.rew_rot_inv(P.F_QVEL, 0, P.REW_CONST, 0), "PHYS_REW_CONST") and bad(P.rew_vec(P.F_QPOS, 0, 1, gate=(P.REW_CONST, 0)), "PHYS_REW_CONST")
    assert refusal(cassie, [P.rew_rot_inv(P.REW_CONST, 0, P.F_QPOS, 3, vec=(0, 0, -1))]) is None
    assert bad(P.rew_vec(P.REW_NONE, 0, 1), "PHYS_REW_NONE") and bad(P.rew_vec(P.F_QPOS, 0, 1, tfield=P.REW_NONE), "PHYS_REW_NONE")
    assert bad(P.rew_rot_inv(P.F_QVEL, 0, P.REW_NONE, 0), "PHYS_REW_NONE")
    # non-finite constants, a negative deadband or k, bounds out of order
    for v in (np.nan, np.inf):
        for name in ("dead", "k", "weight"):
            assert bad(P.rew_vec(P.F_QPOS, 0, 1, **{name: v}), "finite dead, k and weight")
        assert bad(P.rew_vec(P.F_QPOS, 0, 1, target=v), "constant target")
        assert refusal(cassie, [P.rew_vec(P.F_QPOS, 0, 1, target=v, tfield=P.F_QVEL)]) is None       # (not read)
        assert bad(P.rew_rot_inv(P.REW_CONST, 0, P.F_QPOS, 3, vec=(0, v, 0)), "constant vector") and bad(P.rew_quat(P.F_QPOS, 3, vec=(1, 0, 0, v)), "constant vector")
        assert refusal(cassie, [P.rew_quat(P.F_QPOS, 3, vec=(1, 0, 0, v), tfield=P.F_QVEL)]) is None
    assert bad(P.rew_vec(P.F_QPOS, 0, 1, dead=-0.1), "dead is a half width") and bad(P.rew_vec(P.F_QPOS, 0, 1, k=-1e-9), "k >= 0")
    assert bad(ok, "lo <= hi", lo=1.0, hi=0.5) and bad(ok, "lo <= hi", lo=np.nan) and refusal(cassie, [ok], lo=0.5, hi=0.5) is None
    assert refusal(cassie, [ok], lo=-np.inf, hi=np.inf) is None
    # too many terms, the dtype; no terms releases; a negative count is refused
    assert refusal(cassie, [ok] * 64) is None and bad([ok] * 65, "0 .. 64 terms")
    assert bad(ok, "dtype", dtype=2) and bad(ok, "dtype", dtype=np.int32) and refusal(cassie, [ok], dtype=np.float64) is None
    assert refusal(cassie, []) is None and bad([ok], "0 .. 64 terms", nterms=-1)
    # more sources than a call carries
    wide = {f: np.zeros((3, 4)) for f in range(17)}
    assert re_.Call(wide, 3, [P.rew_vec(f, 0, 1) for f in range(16)]).check()[0] is None
    assert "16 distinct" in re_.Call(wide, 3, [P.rew_vec(f, 0, 1) for f in range(17)]).check()[0]
    assert "16 distinct" in re_.Call(wide, 3, [P.rew_vec(f, 0, 1) for f in range(16)] + [P.rew_vec(0, 0, 1, gate=(P.REW_INPUT, 0))]).check()[0]


def test_bind_refusals(cassie):
    t = [P.rew_vec(P.F_QPOS, 0, 5), P.rew_vec(P.REW_INPUT, 2, 3), P.rew_quat(P.F_QPOS, 3)]
    ret, fin = np.zeros(3), np.zeros(3)
    assert "row stride" in re_.Call(held(cassie), 3, t, rew=np.zeros(3, dtype=np.float32), rows=np.zeros((3, 2), dtype=np.float32), ret=ret, fin=fin).check()[0]
    assert re_.Call(held(cassie), 3, t, rew=np.zeros(3, dtype=np.float32), rows=np.zeros((3, 3), dtype=np.float32), ret=ret, fin=fin).check()[0] is None
    c = re_.Call(held(cassie), 3, t, rew=np.zeros(3, dtype=np.float32), ret=ret, fin=fin)
    c.a.srew = 0
    assert "element stride" in c.check()[0]
    c = re_.Call(held(cassie), 3, t)
    c.bind_input(np.zeros((3, 4), dtype=np.float32), dtype=2)
    assert "input's dtype" in c.check()[0]
    c.bind_input(np.zeros((3, 4), dtype=np.float32), input_dim=0)
    assert "at least one element" in c.check()[0]
    c.bind_input(np.zeros((3, 4), dtype=np.float32), input_dim=4, stride=3)
    assert "at least one element" in c.check()[0]
    assert "not configured" in re_.Call(held(cassie), 3, [], rew=np.zeros(3, dtype=np.float32)).call_check(0, 3)


def test_call_refusals(cassie):
    pod = cassie.pod
    t = [P.rew_vec(P.F_QPOS, 0, 5, gate=(P.REW_INPUT, 4)), P.rew_vec(P.F_QPOS, 0, 3, tfield=P.REW_INPUT, tindex=1)]
    rew, ret, fin = np.zeros(3, dtype=np.float32), np.zeros(3), np.zeros(3)
    inp = np.zeros((3, 5), dtype=np.float32)
    c = re_.Call(held(cassie), 3, t, inp=inp, rew=rew, ret=ret, fin=fin)
    assert c.call_check(0, 3) is None and c.call_check(3, 0) is None and c.call_check(1, 2) is None
    assert "not configured" in c.call_check(0, 3, configured=False)
    assert "not configured" in re_.Call(held(cassie), 3, t, inp=inp, ret=ret, fin=fin).call_check(0, 3)        # (no rewards to write)
    for env0, n in ((-1, 2), (0, 4), (2, 2), (0, -1)):
        assert "out of bounds" in c.call_check(env0, n)
    # a source whose row has changed, or gone, since the configure call
    assert "has changed" in c.call_check(0, 3, now={P.F_QPOS: (np.zeros((3, pod.nq + 1)), pod.nq + 1)})
    assert "has changed" in c.call_check(0, 3, now={P.F_QPOS: (None, 0)})
    assert c.call_check(0, 3, now={P.F_QVEL: (None, 0)}) is None      # (no term reads it)
    # the input: nothing bound, or bound too short (the gate reaches element 4)
    assert "no input bound" in re_.Call(held(cassie), 3, t, rew=rew, ret=ret, fin=fin).call_check(0, 3)
    assert "shorter" in re_.Call(held(cassie), 3, t, inp=inp, input_dim=4, rew=rew, ret=ret, fin=fin).call_check(0, 3)
    # the emulator's launch refuses the same
    assert re_.lib().emu_reward(c.a, 0, 4, None, 0) == -1 and b"out of bounds" in re_.lib().emu_reward_last_refusal()


def test_slots_and_launch_record(cassie, terms):
    """The record of the shared case's terms, the table a launch reads, reward_grid at its ends, and the IO's pointers and strides."""
    pod = cassie.pod
    why, rec, table = re_.Call(held(cassie), 6, terms, np.float32, cases.LO, cases.HI).check()
    assert why is None and (rec["nterms"], rec["dtype"], rec["input_need"]) == (13, 4, 70)
    assert rec["slot_field"] == [P.F_QVEL, P.F_QPOS, P.REW_INPUT, P.F_SENSORDATA] and rec["slot_dim"] == [pod.nv, pod.nq, 0, pod.nsensordata]
    assert [int(v) for v in table["field"]] == [0, 1, 1, 1, 1, 0, 0, 3, 0, 2, 3, 1, P.REW_CONST]
    assert [int(v) for v in table["tfield"]] == [2, P.REW_CONST, 2, 2] + [P.REW_CONST] * 3 + [1] + [P.REW_CONST] * 5
    assert [int(v) for v in table["gfield"]] == [P.REW_NONE] * 3 + [2] + [P.REW_NONE] * 6 + [3] + [P.REW_NONE] * 2
    assert [int(v) for v in table["count"]] == [3, 4, 4, 10, 1, 26, 3, 10, 8, 64, 3, 2, 3] and int(table["qfield"][0]) == 1 and int(table["qfield"][12]) == 1
    assert np.array_equal(table["k"], P.rew_terms(terms)["k"]) and np.array_equal(table["vec"], P.rew_terms(terms)["vec"])
    assert [re_.grid(n) for n in (0, 1, 64, 65, 128, 129, 4096, 4097, 2 ** 31 - 1)] == [0, 1, 1, 2, 2, 3, 64, 64, 64] and re_.REWARD_GRID == 64
    f = held(cassie, 6)
    wide = np.zeros((6, pod.nq + pod.nv + 3))
    f[P.F_QPOS] = wide[:, : pod.nq]            # (bound as column blocks of one tensor)
    f[P.F_QVEL] = wide[:, pod.nq: pod.nq + pod.nv]
    inp = np.zeros((6, cases.INPUT_STRIDE), dtype=np.float32)
    raw, rows, ret, fin, reset = np.zeros((6, 3), dtype=np.float32), np.zeros((6, 20), dtype=np.float32), np.zeros(6), np.zeros(6), np.zeros(3, dtype=np.int32)
    c = re_.Call(f, 6, terms, np.float32, cases.LO, cases.HI, inp=inp, input_dim=cases.INPUT_DIM, rew=raw[:, 1], rows=rows, ret=ret, fin=fin)
    io, src = c.record(2, 3, reset)
    assert (io["env0"], io["n"], io["nterms"], io["f32"], io["terms"], io["lo"], io["hi"]) == (2, 3, 13, 1, 1, cases.LO, cases.HI)
    assert (io["rew"], io["srew"], io["trows"], io["sterm"]) == (raw.ctypes.data + 4, 3, rows.ctypes.data, 20)
    assert (io["ret"], io["fin"], io["reset"]) == (ret.ctypes.data, fin.ctypes.data, reset.ctypes.data)
    assert src == [(wide.ctypes.data + 8 * pod.nq, wide.shape[1], 0), (wide.ctypes.data, wide.shape[1], 0), (inp.ctypes.data, cases.INPUT_STRIDE, 1),
                   (f[P.F_SENSORDATA].ctypes.data, pod.nsensordata, 0)]
    io64, src64 = re_.Call(f, 6, terms, np.float64, inp=inp.astype(np.float64), input_dim=cases.INPUT_DIM, rew=np.zeros(6), ret=ret, fin=fin).record(0, 6)
    assert (io64["f32"], io64["srew"], io64["trows"], io64["sterm"], io64["reset"], src64[2][2]) == (0, 1, 0, 0, 0, 0) and io64["lo"] == -np.inf


def test_strided_sources_read_where_bound(cassie, terms, states):
    """Sources bound as column blocks of one wide tensor give the rewards of dense sources."""
    s = states[0]
    pod = cassie.pod
    wide = np.full((6, pod.nq + pod.nv + pod.nsensordata + 5), np.nan)
    wide[:, : pod.nq], wide[:, pod.nq: pod.nq + pod.nv], wide[:, pod.nq + pod.nv: -5] = s[P.F_QPOS], s[P.F_QVEL], s[P.F_SENSORDATA]
    bound = {P.F_QPOS: wide[:, : pod.nq], P.F_QVEL: wide[:, pod.nq: pod.nq + pod.nv], P.F_SENSORDATA: wide[:, pod.nq + pod.nv: -5]}
    out = []
    for f in (fields_of(s), bound):
        rew, ret, fin = np.zeros(6), np.zeros(6), np.zeros(6)
        re_.Call(f, 6, terms, np.float64, cases.LO, cases.HI, inp=s[P.REW_INPUT], input_dim=cases.INPUT_DIM, rew=rew, ret=ret, fin=fin).reward()
        out.append(rew)
    assert rc.same_bits(out[0], out[1]) and rc.same_bits(out[0], cases.reference(terms, [s], np.float64, cases.SCHEDULE[:1])[0][0])
