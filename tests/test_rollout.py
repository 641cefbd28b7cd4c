"""Rollout rows (csrc/rollout_kernels.h) on the wave emulator against the definition restated in numpy (tests/rollout_check.py), BIT FOR
BIT on the words: the record is a copy, every step of the GAE and of the normalisation one rounded fp64 operation, every sum has one
order.  Also: the GAE against a plain Python loop and against the textbook form with (1 - done) products, its properties, the NaN that
stays behind its `done`, the normalisation's independence of the cut into ranges, and every refusal of the pure-host checks."""
import numpy as np
import pytest

import rollout_cases as cases
import rollout_check as rc
import rollout_emu_py as re_
from cassie_amd import phys as P

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    re_.lib()


@pytest.fixture(scope="module")
def shared():
    return cases.Case()


def record_all(case, call, ranges, order=cases.ORDER):
    """Every slot of `order`, every range -> [(t, env0, n)], and per call which sources took the 16-byte path."""
    calls, vecs = [], []
    for t in order:
        call.bind_step(case.steps[t])
        for env0, n in ranges:
            vecs.append(call.record(t, env0, n))
            calls.append((t, env0, n))
    return calls, vecs


def full_run(case, ranges, eps=cases.EPS):
    """Record, finish per range, normalise on fresh padded stores -> (stores, arrays, call, stats)."""
    stores, arrays = case.stores()
    call = re_.Call.of_case(case, stores, arrays)
    record_all(case, call, ranges)
    for env0, n in ranges:
        call.finish(env0, n, case.last)
    stats = call.normalise(eps)
    return stores, arrays, call, stats


@pytest.fixture(scope="module")
def one_range(shared):
    return full_run(shared, ((0, shared.nenv),))


@pytest.fixture(scope="module")
def two_ranges(shared):
    return full_run(shared, cases.RANGES)


# ------------------------------------------------------------------------------------------------------------ record ---
def test_record_is_the_restatement_and_leaves_the_rest_alone(shared):
    """Slots 3 and 0 of the range [37, 130) alone: those rows hold the sources' words; every other slot, every env outside the range and
    every word of padding still holds the sentinel.  The source of dim 68 goes 16 bytes a lane, the one of dim 70 with stride 73 a word."""
    stores, _ = shared.stores()
    call = re_.Call.of_case(shared, stores)
    calls, vecs = record_all(shared, call, (cases.RANGES[1],), order=(3, 0))
    assert all(tuple(v) == shared.VEC for v in vecs)
    written = shared.written(calls)
    assert written.sum() == 2 * 93
    for s, st in enumerate(stores):
        assert np.array_equal(st.buf, st.expected(shared.dense[s], written)), s
        ref = np.full((shared.T, shared.nenv, st.dim), cases.SENT, dtype=U32)     # rollout_check.record on a dense store says the same
        for t, env0, n in calls:
            rc.record(ref, t, shared.steps[t][s], env0, n)
        assert np.array_equal(st.view(), ref), s


def test_two_ranges_write_what_one_call_writes(one_range, two_ranges, shared):
    for a, b in zip(one_range[0], two_ranges[0]):
        assert np.array_equal(a.buf, b.buf)
    everything = np.ones((shared.T, shared.nenv), dtype=bool)
    for s, st in enumerate(two_ranges[0]):
        assert np.array_equal(st.buf, st.expected(shared.dense[s], everything)), s
    for name in ("adv", "ret", "advn"):
        assert np.array_equal(one_range[1][name].buf, two_ranges[1][name].buf), name
    assert np.array_equal(one_range[2].q, two_ranges[2].q)


def test_record_grid_of_one_and_n_zero(shared):
    """One workgroup walks every job of every source; a record of no env is accepted and writes nothing."""
    stores, _ = shared.stores()
    call = re_.Call.of_case(shared, stores)
    call.bind_step(shared.steps[2])
    call.record(2, 5, 0)
    assert all(np.all(st.buf == cases.SENT) for st in stores)
    call.record(2, 0, shared.nenv, grid=1)
    written = shared.written([(2, 0, shared.nenv)])
    for s, st in enumerate(stores):
        assert np.array_equal(st.buf, st.expected(shared.dense[s], written)), s


def test_misaligned_pointer_takes_the_word_path(shared):
    """The dim-68 source from a pointer 4 bytes past a 16-byte boundary: the host picks the word path, the words are the same."""
    stores, _ = shared.stores()
    call = re_.Call.of_case(shared, stores)
    s = shared.role(P.RO_OBS)
    shifted = cases.aligned_words(shared.nenv * 72 + 4)[1:1 + shared.nenv * 72].reshape(shared.nenv, 72)
    shifted[:, :68] = shared.dense[s][1].view(U32)
    tensors = list(shared.steps[1])
    tensors[s] = shifted
    call.bind_step(tensors)
    vec = call.record(1)
    assert vec[s] == 0
    assert np.array_equal(stores[s].buf, stores[s].expected(shared.dense[s], shared.written([(1, 0, shared.nenv)])))


# --------------------------------------------------------------------------------------------------------------- GAE ---
def test_gae_is_the_restatement(two_ranges, shared):
    """ADV, RET and q1 bit for bit, the padding of ADV and RET untouched."""
    adv, ret, q1 = shared.gae()
    everything = np.ones((shared.T, shared.nenv), dtype=bool)
    _, arrays, call, _ = two_ranges
    assert np.array_equal(arrays["adv"].buf, arrays["adv"].expected(adv[:, :, None], everything))
    assert np.array_equal(arrays["ret"].buf, arrays["ret"].expected(ret[:, :, None], everything))
    assert rc.same_bits(call.q[: shared.nenv], q1)
    assert shared.done.any() and not shared.done.all()
    cut = (shared.dense[shared.role(P.RO_REASON)][:, :, 0] == cases.TMASK)
    assert cut.any() and (shared.done & ~cut).any()            # both kinds of ending occur


def test_gae_restatement_is_the_plain_python_loop(shared):
    """Python floats are individually rounded doubles: the numpy restatement is the definition, bitwise."""
    f = lambda role: shared.dense[shared.role(role)][:, :, 0]
    adv, ret, _ = shared.gae()
    padv, pret = rc.gae_plain(f(P.RO_VALUE), f(P.RO_REWARD), f(P.RO_DONE), f(P.RO_REASON), shared.last[:, 0], shared.gamma, shared.lam, shared.tmask)
    assert rc.same_bits(adv, padv) and rc.same_bits(ret, pret)


def test_gae_equals_the_textbook_products_as_numbers(shared):
    """(1 - done) products in float64 on finite inputs: multiplying by 1.0 or 0.0 is exact, so only the sign of a zero may differ."""
    adv, ret, _ = shared.gae()
    tadv, tret, _ = shared.gae(products=True)
    assert np.all(np.isfinite(adv)) and np.all(adv == tadv) and np.all(ret == tret)


def emu_gae(val, rew, done, reason, last, gamma, lam, tmask=0):
    """ADV and RET of dense arrays [T][n] by the emulator's finish, the stores handed to it as they are."""
    steps, n = val.shape
    srcs = [(P.RO_VALUE, 1), (P.RO_REWARD, 1)] + ([(P.RO_DONE, 1)] if done is not None else []) + ([(P.RO_REASON, 1)] if reason is not None else [])
    call = re_.Call(srcs, steps, n, gamma, lam, tmask)
    arrs = [np.ascontiguousarray(val, dtype=F32), np.ascontiguousarray(rew, dtype=F32)]
    arrs += [np.ascontiguousarray(a, dtype=I32) for a in (done, reason) if a is not None]
    for s, a in enumerate(arrs):
        call.bind_storage(s, a, n, 1)
    adv, ret = np.zeros((steps, n), dtype=F32), np.zeros((steps, n), dtype=F32)
    call.bind_storage("adv", adv, n, 1)
    call.bind_storage("ret", ret, n, 1)
    call.finish(0, n, np.ascontiguousarray(last, dtype=F32))
    return adv, ret


def test_gae_properties():
    rng = np.random.default_rng(8)
    steps, n = 11, 70                      # T no multiple of the look-ahead; more than a wave of envs
    v, r = rng.normal(size=(steps, n)).astype(F32), rng.normal(size=(steps, n)).astype(F32)
    last = rng.normal(size=n).astype(F32)
    g = F64(0.97)
    # done at every step: adv = r - v
    adv, ret = emu_gae(v, r, np.ones((steps, n), dtype=I32), None, last, 0.97, 0.9)
    assert rc.same_bits(adv, (r.astype(F64) - v.astype(F64)).astype(F32))
    # lambda 0: the one-step delta
    adv, _ = emu_gae(v, r, None, None, last, 0.97, 0.0)
    nxt = np.concatenate([v[1:], last[None]]).astype(F64)
    assert np.all(adv == ((r.astype(F64) + g * nxt) - v.astype(F64)).astype(F32))
    # a reason inside the mask adds gamma * v; any bit outside it does not
    done = np.ones((steps, n), dtype=I32)
    reason = np.where(np.arange(n)[None, :] % 3 == 0, 0x6, np.where(np.arange(n)[None, :] % 3 == 1, 0x2, 0xA)).astype(I32) * np.ones((steps, 1), dtype=I32)
    adv, _ = emu_gae(v, r, done, reason, last, 0.97, 0.9, tmask=0x6)
    plain, boot = (r.astype(F64) - v.astype(F64)).astype(F32), ((r.astype(F64) + g * v.astype(F64)) - v.astype(F64)).astype(F32)
    inside = (np.arange(n) % 3 != 2)[None, :] * np.ones((steps, 1), dtype=bool)
    assert rc.same_bits(adv, np.where(inside, boot, plain)) and not np.array_equal(boot, plain)
    # ... and a step that is not done takes no bootstrap whatever its reason says
    adv2, _ = emu_gae(v, r, np.zeros((steps, n), dtype=I32), reason, last, 0.97, 0.9, tmask=0x6)
    adv3, _ = emu_gae(v, r, None, None, last, 0.97, 0.9)
    assert rc.same_bits(adv2, adv3)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_nan_behind_a_done_stays_there(bad):
    """Env 5's episode ends at step 4; a NaN / inf in its value and reward at steps 5 .. 8 leaves steps 0 .. 4 of that env, and every
    other env, bit-identical.  With (1 - done) products the NaN would reach step 4 (0 * NaN)."""
    rng = np.random.default_rng(9)
    steps, n, e = 9, 66, 5
    v, r = rng.normal(size=(steps, n)).astype(F32), rng.normal(size=(steps, n)).astype(F32)
    last = rng.normal(size=n).astype(F32)
    done = (rng.random((steps, n)) < 0.15).astype(I32)
    done[4, e] = 1
    clean = emu_gae(v, r, done, None, last, 0.99, 0.95)
    v2, r2, last2 = v.copy(), r.copy(), last.copy()
    v2[5:, e], r2[5:, e], last2[e] = bad, bad, bad
    dirty = emu_gae(v2, r2, done, None, last2, 0.99, 0.95)
    others = np.arange(n) != e
    for a, b in zip(clean, dirty):
        assert np.array_equal(a[:, others].view(U32), b[:, others].view(U32))
        assert np.array_equal(a[:5, e].view(U32), b[:5, e].view(U32))
    assert not np.all(np.isfinite(dirty[0][5:, e]))
    wrong, _, _ = rc.gae(v2, r2, done, None, last2, 0.99, 0.95, products=True)
    assert np.isnan(wrong[4, e])       # the control: the textbook form carries it across the done


# --------------------------------------------------------------------------------------------------------- normalise ---
def test_normalise_is_the_restatement(one_range, two_ranges, shared):
    """ADVN and the statistics bit for bit, identical whether finish ran as one range or two; padding untouched."""
    advn, stats, q2 = shared.normalised()
    everything = np.ones((shared.T, shared.nenv), dtype=bool)
    for run in (one_range, two_ranges):
        _, arrays, call, got = run
        assert rc.same_bits(np.array(got), np.array(stats))
        assert np.array_equal(arrays["advn"].buf, arrays["advn"].expected(advn[:, :, None], everything))
        assert rc.same_bits(call.q[shared.nenv: 2 * shared.nenv], q2)
    mean, std, inv = stats
    adv = shared.gae()[0].astype(F64)
    assert abs(mean - adv.mean()) < 1e-12 and abs(std - adv.std(ddof=1)) < 1e-12 * std     # and they ARE the mean and the sample deviation


def test_reduce_tree_is_not_a_sequential_sum(shared):
    """The control: the case can tell reduce's tree from a plain sequential sum.  (On q2: the partials of the mean, q1, are sums of a few
    float32 values and exact in a double whatever the order.)"""
    _, _, q2 = shared.normalised()
    seq = F64(0.0)
    for x in q2:
        seq = seq + x
    assert rc.reduce(q2) != seq


def test_normalise_grids(shared, one_range):
    """One workgroup for the lane = env and the scale launches gives the same bits."""
    stores, arrays, call, _ = one_range
    before = arrays["advn"].buf.copy()
    arrays["advn"].buf[:] = cases.SENT
    stats = call.normalise(cases.EPS, grid=1)
    assert np.array_equal(arrays["advn"].buf, before) and rc.same_bits(np.array(stats), np.array(shared.normalised()[1]))


# ---------------------------------------------------------------------------------------------------------- refusals ---
def refusal(srcs, steps=5, nenv=8, **kw):
    return re_.Call(srcs, steps, nenv, **kw).check()


BASE = [(P.RO_VALUE, 1), (P.RO_REWARD, 1)]


def test_configure_refusals():
    assert refusal(BASE) is None
    assert refusal(BASE, steps=P.RO_MAXT) is None and refusal([(P.RO_DATA, P.RO_MAXDIM)] * P.RO_MAXSRC) is None
    for steps in (0, -1, P.RO_MAXT + 1):
        assert "1 .. 1024 steps" in refusal(BASE, steps=steps)
    assert "1 .. 16 sources" in refusal([(P.RO_DATA, 1)] * (P.RO_MAXSRC + 1))
    assert "1 .. 16 sources" in re_.Call(BASE, 5, 8, nsrcs=-1).check()
    for role in (0, 15, 28, P.RO_ADV, P.RO_RET, P.RO_ADVN):
        assert "a source's role is" in refusal([(role, 1)])
    for dim in (0, -3, P.RO_MAXDIM + 1):
        assert "dim lies in 1 .. 4096" in refusal([(P.RO_OBS, dim)])
    for role in (P.RO_VALUE, P.RO_REWARD, P.RO_DONE, P.RO_REASON, P.RO_LOGP):
        assert "have dim 1" in refusal([(role, 2)])
    for role in (P.RO_OBS, P.RO_ACTION, P.RO_LOGP, P.RO_MU, P.RO_VALUE, P.RO_REWARD, P.RO_DONE, P.RO_REASON):
        assert "at most one source" in refusal([(role, 1), (P.RO_DATA, 2), (role, 1)])
    assert refusal([(P.RO_DATA, 2), (P.RO_DATA, 2)]) is None
    for bad in (np.nan, np.inf, -np.inf, -1e-9, 1.0 + 1e-9):
        assert "gamma is finite" in refusal(BASE, gamma=bad)
        assert "lambda is finite" in refusal(BASE, lam=bad)
    assert refusal(BASE, gamma=0.0, lam=1.0) is None
    assert "needs a REASON source" in refusal(BASE + [(P.RO_DONE, 1)], tmask=4)
    assert refusal(BASE + [(P.RO_DONE, 1), (P.RO_REASON, 1)], tmask=4) is None
    assert re_.Call([], 5, 8).check() is None                       # 0 sources: the launcher releases


def bound(srcs, steps=3, nenv=8):
    """A call with dense stores, ADV, RET, ADVN and every source bound."""
    call = re_.Call(srcs, steps, nenv)
    for s, (_, dim) in enumerate(srcs):
        call.bind_storage(s, np.zeros((steps, nenv, dim), dtype=U32), nenv * dim, dim)
        call.bind_source(s, np.zeros((nenv, dim), dtype=U32))
    for name in ("adv", "ret", "advn"):
        call.bind_storage(name, np.zeros((steps, nenv), dtype=F32), nenv, 1)
    return call


def test_call_refusals():
    srcs = BASE + [(P.RO_OBS, 6), (P.RO_DATA, 2)]
    ok = bound(srcs)
    assert ok.check(1, t=2, env0=0, n=8) is None and ok.check(2, env0=3, n=5, last=np.zeros(8, dtype=F32)) is None and ok.check(3) is None
    for t in (-1, 3, 100):
        assert "slot t lies in 0 .. T - 1" in ok.check(1, t=t, n=8)
    for env0, n in ((-1, 2), (0, 9), (8, 1), (2, -1)):
        assert "env range out of bounds" in ok.check(1, t=0, env0=env0, n=n)
        assert "env range out of bounds" in ok.check(2, env0=env0, n=n, last=np.zeros(8, dtype=F32))
    for what in (1, 2, 3):
        assert "not configured" in ok.check(what, configured=False)
    # bindings: a row stride below the dim, a step stride below a step's rows, a source that is none
    c = bound(srcs); c.bind_source(2, np.zeros((8, 6), dtype=U32), stride=5)
    assert "row stride of at least the source's dim" in c.check()
    c = bound(srcs); c.bind_storage(2, np.zeros(1, dtype=U32), 8 * 6, 5)
    assert "row stride of at least the source's dim" in c.check()
    c = bound(srcs); c.bind_storage(2, np.zeros(1, dtype=U32), 7 * 6 + 5, 6)
    assert "step stride of at least a step's rows" in c.check()
    c = bound(srcs); c.bind_storage(2, np.zeros((3, 8, 6), dtype=U32), 7 * 6 + 6, 6)
    assert c.check() is None
    # a DATA source must be bound; the others are resolved, and nothing is there to resolve them from
    c = bound(srcs); c.bind_source(3, None)
    assert "PHYS_RO_DATA source has no pointer" in c.check(1, t=0, n=8)
    c = bound(srcs); c.bind_source(2, None)
    assert "OBS: the policy has no input bound" in c.check(1, t=0, n=8)
    # finish without VALUE or REWARD; the last value resolved from nothing; normalise of fewer than two values
    for missing in (0, 1):
        c = bound([srcs[1 - missing], srcs[2]])
        assert "needs a VALUE and a REWARD" in c.check(2, n=8, last=np.zeros(8, dtype=F32))
    c = bound(srcs); c.bind_source(0, None)
    assert "VALUE: network 1 has no output bound" in c.check(2, n=8)
    assert "stride of the last values" in ok.check(2, n=8, last=np.zeros(8, dtype=F32), stride=0)
    assert "T * nenv >= 2" in bound(BASE, steps=1, nenv=1).check(3)
    assert bound(BASE, steps=2, nenv=1).check(3) is None and bound(BASE, steps=1, nenv=2).check(3) is None
    for eps in (-1e-9, np.nan, np.inf):
        assert "eps is finite" in ok.check(3, eps=eps)


def test_resolution_from_the_live_bindings():
    """An unbound source is read where the batch reads or writes the thing now; a width or stride that no longer fits is refused."""
    nenv, steps = 8, 2
    srcs = [(P.RO_VALUE, 1), (P.RO_REWARD, 1), (P.RO_OBS, 6), (P.RO_MU, 3), (P.RO_ACTION, 3), (P.RO_LOGP, 1), (P.RO_DONE, 1), (P.RO_REASON, 1)]
    rng = np.random.default_rng(3)
    call = re_.Call(srcs, steps, nenv)
    stores = [np.full((steps, nenv, d), cases.SENT, dtype=U32) for _, d in srcs]
    for s, (_, d) in enumerate(srcs):
        call.bind_storage(s, stores[s], nenv * d, d)
    obs, mu, act = (rng.normal(size=(nenv, w)).astype(F32) for w in (9, 4, 3))
    val, logp, rew = rng.normal(size=(nenv, 2)).astype(F32), rng.normal(size=nenv).astype(F32), rng.normal(size=(nenv, 2)).astype(F32)
    done, reason = rng.integers(0, 2, nenv).astype(I32), rng.integers(0, 8, nenv).astype(I32)
    L = call.a.live
    L.obs, L.obs_dim, L.obs_stride = obs.ctypes.data, 6, 9
    L.mu, L.mu_dim, L.mu_stride = mu.ctypes.data, 3, 4
    L.value, L.value_stride = val.ctypes.data, 2
    L.action, L.action_dim, L.action_stride, L.logp = act.ctypes.data, 3, 3, logp.ctypes.data
    L.rew, L.rew_stride, L.rew_dtype = rew.ctypes.data, 2, 4
    L.done, L.reason = done.ctypes.data, reason.ctypes.data
    call.record(1)
    want = [val[:, :1], rew[:, :1], obs[:, :6], mu[:, :3], act, logp[:, None], done[:, None], reason[:, None]]
    for s, w in enumerate(want):
        assert np.array_equal(stores[s][1], np.ascontiguousarray(w).view(U32)), s
        assert np.all(stores[s][0] == cases.SENT)
    L.rew_dtype = 8
    assert "must be configured PHYS_OBS_F32" in call.check(1, t=0, n=nenv)
    L.rew_dtype, L.obs_dim = 4, 7
    assert "dim no longer fits the configured dim" in call.check(1, t=0, n=nenv)
    L.obs_dim, L.mu_stride = 6, 2
    assert "row stride no longer fits" in call.check(1, t=0, n=nenv)
    L.mu_stride, L.done = 4, None
    assert "DONE: episodes are not enabled" in call.check(1, t=0, n=nenv)
