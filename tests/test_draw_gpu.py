"""Draw rows (phys_batch_draw_*) on the device against the wave emulator and the definition restated in numpy (tests/draw_check.py), BIT FOR
BIT on every word: the cases tests/test_draw.py runs on the emulator, into a bound tensor and into the policy's eps, cut into ranges on two
streams; the shuffle into the batch's own buffer and into a bound tensor.  Also: the rows through the policy, the permutation through the
gradient rows, a whole iteration replayed from its seed under another cut of the ranges, and the refusals that need a batch."""
import numpy as np
import pytest

import bench
import draw_cases as cases
import draw_check as dc
import draw_emu_py as de
import grad_cases as gcs
import grad_check as gc
import policy_cases
import policy_check as pc
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import make
from test_grad_gpu import Dev, fence, up

pytestmark = pytest.mark.gpu
F32 = np.float32


def sentinel(nenv, stride):
    import torch
    return torch.full((nenv, stride), float(cases.SENTINEL), dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("nenv", cases.NENVS)
def test_shared_cases_on_the_device(cassie, built, nenv):
    """Every width of the shared cases, three calls in a row into a bound tensor with a row stride larger than A: every word -- the
    sentinel past column A included -- and the counts, against the restatement and the emulator."""
    b = Batch(cassie, nenv)
    try:
        for A in cases.WIDTHS:
            stride, env_base, seed = cases.case(nenv, A)
            rows, counts = cases.reference(nenv, A)
            e = de.Draw(nenv, A, 0, seed, env_base, stride, fill=cases.SENTINEL)
            dst = sentinel(nenv, stride)
            b.configure_draws(A, 0, seed, env_base)
            b.bind_draws(dst.data_ptr(), stride)
            before = b.draw_launches()
            for k in range(cases.CALLS):
                fence(b)
                b.draw()
                fence(b)
                got = dst.cpu().numpy()
                assert cases.same_bits(got, rows[k]) and cases.same_bits(got, e.draw()), (nenv, A, k)
                assert cases.same_bits(b.draws(), rows[k][:, :A])
            assert cases.same_bits(b.draw_state(), counts) and cases.same_bits(e.counts, counts)
            assert tuple(x - y for x, y in zip(b.draw_launches(), before)) == (cases.CALLS, 0)
    finally:
        b.close()


@pytest.mark.parametrize("A", (10, 64))
def test_range_cuts_on_two_streams(cassie, built, A):
    """130 envs as one range and as (0, 17), (17, 47), (64, rest) on two streams, in two orders: the same words; envs 47 .. 63 keep the
    sentinel and their count.  Then a count of 0xffffffff wraps to 0."""
    import torch
    nenv = 130
    stride, env_base, seed = cases.case(nenv, A)
    rows, _ = cases.reference(nenv, A)
    b = Batch(cassie, nenv)
    try:
        st = [torch.cuda.Stream(), torch.cuda.Stream()]
        for order in (cases.cut_ranges(nenv), cases.cut_ranges(nenv)[::-1]):
            dst = sentinel(nenv, stride)
            b.configure_draws(A, 0, seed, env_base)
            b.bind_draws(dst.data_ptr(), stride)
            fence(b)
            for k, (env0, n) in enumerate(order):
                b.draw(env0, n, stream=st[k & 1].cuda_stream)
            fence(b)
            want = rows[0].copy()
            want[47:64] = cases.SENTINEL
            assert cases.same_bits(dst.cpu().numpy(), want), order
            counts = b.draw_state()
            assert np.all(counts[:47] == 1) and np.all(counts[47:64] == 0) and np.all(counts[64:] == 1)
            b.draw(47, 17)
            fence(b)
            assert cases.same_bits(dst.cpu().numpy(), rows[0])
        ref = dc.Draws(nenv, A, seed, env_base, stride, fill=cases.SENTINEL)
        ref.counts[:] = 0xFFFFFFFF
        ref.counts[5] = 77
        b.set_draw_state(ref.counts)
        dst.fill_(float(cases.SENTINEL))
        fence(b)
        b.draw()
        fence(b)
        assert cases.same_bits(dst.cpu().numpy(), ref.draw()) and cases.same_bits(b.draw_state(), ref.counts)
        assert b.draw_state()[0] == 0 and b.draw_state()[5] == 78
    finally:
        b.close()


@pytest.mark.parametrize("n", cases.PERM_NS)
def test_shuffle_on_the_device(cassie, built, n):
    """Epochs 0 and 1 into the batch's own buffer, epoch 1 into a bound tensor: the restatement's words (and with them a bijection)."""
    import torch
    b = Batch(cassie, 4)
    try:
        b.configure_draws(0, n, cases.SEED)
        for epoch in (0, 1):
            b.draw_perm(epoch)
            fence(b)
            assert cases.same_bits(b.draw_perm_values(), cases.perm_reference(n, epoch)[0]), (n, epoch)
        own = b.draw_perm_ptr()
        mine = torch.full((n + 2,), -5, dtype=torch.int32, device="cuda")
        b.bind_draw_perm(mine.data_ptr() + 4)
        assert b.draw_perm_ptr() == mine.data_ptr() + 4
        fence(b)
        st = torch.cuda.Stream()
        b.draw_perm(0, stream=st.cuda_stream)
        fence(b)
        got = mine.cpu().numpy()
        assert cases.same_bits(got[1:-1], cases.perm_reference(n, 0)[0]) and got[0] == -5 and got[-1] == -5
        b.bind_draw_perm(None)
        assert b.draw_perm_ptr() == own and cases.same_bits(b.draw_perm_values(), cases.perm_reference(n, 1)[0])
        assert b.draw_launches() == (0, 3)
    finally:
        b.close()


NIN, NHID, NACT, NPOL_ENV = 8, 16, 3, 65


def small_policy(rng, n=NPOL_ENV):
    nets = [policy_cases.dense(rng, (NIN, NHID, NACT), (P.POL_ELU, P.POL_TANH))]
    return nets, policy_cases.Case("draws", nets, np.zeros((n, NIN), dtype=F32), pad=0, wpad=0)


def test_through_the_policy(cassie, built):
    """draw then policy with nothing bound -- the rows go to the eps of the policy's sample binding, a stride of A + 1 --: action and
    log-probability are policy_check's fed with the restated draws, bit for bit, in one range and in two ranges on two streams."""
    import torch
    n, seed, env_base = NPOL_ENV, 2024, 300
    rng = np.random.default_rng(41)
    nets, proto = small_policy(rng)
    x = rng.normal(size=(n, NIN)).astype(F32)
    log_std = rng.uniform(-1.5, 0.0, NACT).astype(F32)
    b = Batch(cassie, n)
    try:
        x_d, ls_d = up(x), up(log_std)
        eps_d = sentinel(n, NACT + 1)
        act_d, logp_d = torch.zeros((n, NACT), dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
        b.configure_policy(proto.defs, NIN)
        b.load_policy(0, proto.weights[0])
        b.bind_policy_input(x_d.data_ptr(), NIN, NIN, torch.float32)
        b.bind_policy_sample(eps_d.data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr(), eps_stride=NACT + 1)
        b.configure_draws(seed=seed, env_base=env_base)              # (A: the actor's output width)
        assert b.draw_dim() == (NACT, 0)
        ref = dc.Draws(n, NACT, seed, env_base, NACT + 1, fill=cases.SENTINEL)
        st = [torch.cuda.Stream(), torch.cuda.Stream()]
        fence(b)
        for cuts in (((0, n),), ((0, 23), (23, n - 23))):
            for k, (env0, cnt) in enumerate(cuts):
                b.draw(env0, cnt, stream=st[k].cuda_stream)
                b.policy(env0, cnt, stream=st[k].cuda_stream)
            fence(b)
            eps = ref.draw()
            assert cases.same_bits(eps_d.cpu().numpy(), eps)
            want = pc.policy(x, nets, None, eps[:, :NACT], log_std)
            assert gc.same_bits(act_d.cpu().numpy(), want["action"]) and gc.same_bits(logp_d.cpu().numpy(), want["logp"])
        # the draw rows stay configured when the policy is configured anew, and resolve the new binding
        b.configure_policy(proto.defs, NIN)
        with pytest.raises(RuntimeError, match="no destination"):
            b.draw()
        assert np.all(b.draw_state() == 2)
    finally:
        b.close()


def test_through_the_update(cassie, built):
    """grad_cases' smallest case (one layer, 20 samples): grad on draw_perm_ptr() leaves the gradients grad leaves on the restated
    permutation uploaded from the host, bit for bit; an epoch of four minibatches visits every sample once."""
    case = gcs.one_layer_case()
    d = Dev(cassie, case, 16)
    try:
        b, S = d.b, case.S
        b.configure_draws(A=0, seed=99)                               # (perm_n: the rollout's T steps of every env)
        assert b.draw_dim() == (0, S)
        epoch = 3
        want_perm = dc.perm(S, epoch, 99)
        ref = d.grad(want_perm)
        b.draw_perm(epoch)
        b.grad(b.draw_perm_ptr(), S)
        fence(b)
        got = d.result(S)
        assert gc.differing(got, ref) == [] and gc.differing(got, case.reference(want_perm, 16)) == []
        assert cases.same_bits(b.draw_perm_values(), want_perm)
        M, seen = 5, 0
        for k in range(S // M):
            b.grad(b.draw_perm_ptr() + 4 * k * M, M)
            stats = b.grad_stats()
            assert stats["void"] == 0
            seen += int(stats["m"])
            part = d.result(M)
            assert gc.differing(part, case.reference(want_perm[k * M: (k + 1) * M], 16)) == [], k
        assert seen == S
    finally:
        d.close()


NOBS, T_REPLAY = 12, 4


def iteration(cassie, seed, cuts, streams):
    """A rollout of T_REPLAY policy steps on 65 envs (one substep a step) with draw in front of policy in every range, then one epoch of
    minibatches cut from draw_perm with an Adam step each -> (the packed weights, log_std, the draw counts)."""
    import torch
    n, A, M = NPOL_ENV, NACT, NPOL_ENV
    rng = np.random.default_rng(43)
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * rng.random(n)
    nets = [policy_cases.dense(rng, (NOBS, NHID, A), (P.POL_ELU, P.POL_TANH)), policy_cases.dense(rng, (NOBS, NHID, 1), (P.POL_TANH, P.POL_IDENTITY))]
    proto = policy_cases.Case("replay", nets, np.zeros((n, NOBS), dtype=F32), pad=0, wpad=0)
    b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
    try:
        dev = "cuda"
        b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
        obs_d = torch.zeros((n, NOBS), dtype=torch.float32, device=dev)
        act_d = torch.zeros((n, A), dtype=torch.float32, device=dev)
        eps_d = torch.zeros((n, A), dtype=torch.float32, device=dev)
        mu_d = torch.zeros((n, A), dtype=torch.float32, device=dev)
        val_d = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        logp_d = torch.zeros(n, dtype=torch.float32, device=dev)
        ls_d = up(np.full(A, -1.0, dtype=F32))
        b.configure_obs([P.obs_copy(P.F_QPOS, 7, 10, scale=1.0), P.obs_copy(P.F_QVEL, 0, 2, scale=0.1)], history=1, dtype=np.float32)
        b.bind_obs(obs_d.data_ptr(), NOBS)
        b.configure_actions([P.act_col(P.F_PD_PTARGET, j, lo=-1.5, hi=1.5, offset=float(bench.PD_OFFSET[j]), scale=0.2) for j in range(A)], dtype=np.float32)
        b.bind_actions(act_d.data_ptr(), A, torch.float32)
        b.configure_rewards([P.rew_vec(P.F_QPOS, 2, 1, target=0.9, norm=P.REW_SUMABS, shape=P.REW_EXP, k=10.0, weight=0.5),
                             P.rew_vec(P.F_QVEL, 0, 3, weight=-0.05)], dtype=np.float32, lo=-1.0, hi=1.0)
        b.configure_policy(proto.defs, NOBS)
        masters = [[(up(w), up(bb)) for w, bb in layers] for layers in proto.weights]
        fence(b)
        for a, layers in enumerate(masters):
            b.load_policy(a, [(w.data_ptr(), w.shape[1], bb.data_ptr()) for w, bb in layers])
        b.bind_policy_input(obs_d.data_ptr(), NOBS, NOBS, torch.float32)
        b.bind_policy_output(0, mu_d.data_ptr(), A)
        b.bind_policy_output(1, val_d.data_ptr(), 1)
        b.bind_policy_sample(eps_d.data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
        srcs = [("obs", NOBS), ("action", A), ("logp", 1), ("mu", A), ("value", 1), ("reward", 1), ("done", 1), ("reason", 1)]
        b.enable_episodes(max_steps=3, min_height=0.4)
        b.set_reset_bank(b.make_reset_bank(cassie.qpos_init()[None]))
        b.configure_rollout(T_REPLAY, srcs, 0.99, 0.95, timeout_mask=P.DONE_TIME)
        b.configure_grad(M, 16, 0.2, 0.5, 0.01)
        b.configure_opt(max_norm=0.5)
        for a, layers in enumerate(masters):
            for l, (w, bb) in enumerate(layers):
                b.bind_opt_param(a, l, w.data_ptr(), w.shape[1], bb.data_ptr())
        b.bind_opt_log_std(ls_d.data_ptr())
        b.configure_draws(seed=seed)
        assert b.draw_dim() == (A, T_REPLAY * n)
        fence(b)

        def forward():
            for k, (env0, cnt) in enumerate(cuts):
                s = streams[k % len(streams)].cuda_stream
                b.observe(env0, cnt, stream=s)
                b.draw(env0, cnt, stream=s)
                b.policy(env0, cnt, stream=s)
                b.act(env0, cnt, stream=s)
                b.step_range(env0, cnt, 1, s)
                b.reward(env0, cnt, stream=s)

        forward()
        for t in range(T_REPLAY):
            for k, (env0, cnt) in enumerate(cuts):
                s = streams[k % len(streams)].cuda_stream
                b.end_episodes(env0, cnt, True, stream=s)
                b.rollout_record(t, env0, cnt, stream=s)
            forward()
        fence(b)                                                     # (the caller orders the ranges' streams in front of what follows)
        s = streams[0].cuda_stream
        b.rollout_finish(stream=s)
        b.rollout_normalise(1e-8, stream=s)
        b.draw_perm(0, stream=s)
        for k in range(T_REPLAY * n // M):
            b.grad(b.draw_perm_ptr() + 4 * k * M, M, s)
            b.opt_step(3e-3, s)
        fence(b)
        assert b.opt_stats()["t"] == T_REPLAY and b.opt_stats()["skipped"] == 0
        return b.policy_packed().copy(), ls_d.cpu().numpy(), b.draw_state()
    finally:
        b.close()


def test_a_replay_from_the_seed(cassie, built):
    """Two fresh batches with the same seed, the ranges cut differently and issued on one stream and on two: the packed weights after the
    update are equal bit for bit.  Another seed gives other weights."""
    import torch
    n = NPOL_ENV
    st = [torch.cuda.Stream(), torch.cuda.Stream()]
    w0, ls0, c0 = iteration(cassie, 5, ((0, n),), st[:1])
    w1, ls1, c1 = iteration(cassie, 5, ((0, 23), (23, n - 23)), st)
    w2, ls2, _ = iteration(cassie, 6, ((0, n),), st[:1])
    assert np.all(np.isfinite(w0)) and np.all(c0 == T_REPLAY + 1) and np.all(c1 == T_REPLAY + 1)
    assert gc.same_bits(w0, w1) and gc.same_bits(ls0, ls1)
    assert not gc.same_bits(w0, w2) and not gc.same_bits(ls0, ls2)


def test_refusals_with_a_batch(cassie, built):
    import torch
    n = 8
    b = Batch(cassie, n)
    try:
        for call in (b.draw, lambda: b.draw_perm(0), b.draws, b.draw_state, b.draw_dim):
            with pytest.raises(RuntimeError, match="not configured"):
                call()
        with pytest.raises(ValueError, match="not configured"):
            b.bind_draw_perm(None)
        for kw, msg in ((dict(A=65), "A lies in 1 .. 64"), (dict(A=-1), "A lies in 1 .. 64"), (dict(perm_n=(1 << 30) + 1), "perm_n lies in 1 .. 2\\^30"),
                        (dict(perm_n=-1), "perm_n lies in 1 .. 2\\^30")):
            with pytest.raises(ValueError, match=msg):
                b.configure_draws(**dict(dict(A=3, perm_n=16), **kw))
        b.configure_draws(3, 0, seed=1)
        with pytest.raises(RuntimeError, match="no destination"):
            b.draw()
        with pytest.raises(RuntimeError, match="no shuffle is configured"):
            b.draw_perm(0)
        with pytest.raises(RuntimeError, match="no shuffle is configured"):
            b.draw_perm_ptr()
        dst = sentinel(n, 4)
        with pytest.raises(ValueError, match="a row stride of at least A"):
            b.bind_draws(dst.data_ptr(), 2)
        b.bind_draws(dst.data_ptr(), 4)
        for env0, cnt in ((0, n + 1), (n, 1), (-1, 2), (2, -1)):
            with pytest.raises(RuntimeError, match="env range out of bounds"):
                b.draw(env0, cnt)
        b.configure_policy([[P.pol_layer(NHID, P.POL_ELU), P.pol_layer(4, P.POL_TANH)]], NIN)
        b.bind_draws(None)
        eps_d, ls_d, act_d, logp_d = sentinel(n, 4), up(np.zeros(4, dtype=F32)), sentinel(n, 4), up(np.zeros(n, dtype=F32))
        b.bind_policy_sample(eps_d.data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
        with pytest.raises(RuntimeError, match="the actor's output width is not A"):
            b.draw()
        fence(b)
        assert b.draw_launches() == (0, 0) and np.all(b.draw_state() == 0)
        assert np.all(dst.cpu().numpy() == cases.SENTINEL) and np.all(eps_d.cpu().numpy() == cases.SENTINEL)
        b.configure_draws(0, 16, seed=1)
        with pytest.raises(RuntimeError, match="no normal rows are configured"):
            b.draw()
        b.draw_perm(0)
        fence(b)
        assert np.array_equal(np.sort(b.draw_perm_values()), np.arange(16))
        b.configure_draws(release=True)
        with pytest.raises(RuntimeError, match="not configured"):
            b.draw_perm(0)
    finally:
        b.close()
