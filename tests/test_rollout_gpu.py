"""Rollout rows (phys_batch_rollout_*) on the device against the wave emulator and the definition restated in numpy
(tests/rollout_check.py), BIT FOR BIT on the words: the case tests/test_rollout.py runs on the emulator, with the batch's own stores and
with bound, padded ones, the two ranges on two streams.  Also: a live batch whose sources are all resolved from the bindings, that the
calls change nothing of the batch, the launch counter, and the refusals that need a batch."""
import numpy as np
import pytest

import bench
import rollout_cases as cases
import rollout_check as rc
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import make
from test_rollout import full_run

pytestmark = pytest.mark.gpu
F32, U32, I32 = np.float32, np.uint32, np.int32


def fence(b):
    import torch
    b.sync()
    torch.cuda.synchronize()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(I32)).cuda()


def words(t):
    return t.cpu().numpy().view(U32)


@pytest.fixture(scope="module")
def shared():
    return cases.Case()


@pytest.fixture(scope="module")
def emulated(shared, built):
    """The emulator's stores, arrays and statistics of the shared case, the batch cut into the two ranges."""
    stores, arrays, call, stats = full_run(shared, cases.RANGES)
    return stores, arrays, stats


def run_on_device(b, case, streams):
    """The shared case on a configured batch: every slot out of order, the two ranges on two streams; finish per range; normalise."""
    import torch
    src = [[up(a) for a in per] for per in case.steps]
    last = up(case.last)
    fence(b)
    for t in cases.ORDER:
        for s, a in enumerate(src[t]):
            b.bind_rollout_source(s, a.data_ptr(), case.src_stride[s])
        for (env0, n), st in zip(cases.RANGES, streams):
            b.rollout_record(t, env0, n, stream=st.cuda_stream)
    for (env0, n), st in zip(cases.RANGES, streams):
        b.rollout_finish(env0, n, last.data_ptr(), 2, stream=st.cuda_stream)
    fence(b)                               # (ordering the streams is the caller's job)
    b.rollout_normalise(cases.EPS, stream=streams[0].cuda_stream)
    fence(b)
    return src, last


def test_shared_case_with_own_storage(cassie, shared, emulated):
    import torch
    b = Batch(cassie, shared.nenv)
    try:
        b.configure_rollout(shared.T, shared.srcs, shared.gamma, shared.lam, shared.tmask)
        assert b.rollout_ptr("advn")[0] is None and b.rollout_ptr("adv")[1:] == (shared.nenv, 1)
        assert b.rollout_ptr(shared.role(P.RO_OBS))[1:] == (shared.nenv * 68, 68)
        run_on_device(b, shared, [torch.cuda.Stream(), torch.cuda.Stream()])
        stores, arrays, stats = emulated
        for s, st in enumerate(stores):
            got = b.rollout(s).view(U32).reshape(shared.T, shared.nenv, st.dim)
            assert np.array_equal(got, shared.dense[s].view(U32)) and np.array_equal(got, st.view()), s
        adv, ret, _ = shared.gae()
        advn, want, _ = shared.normalised()
        for name, ref in (("adv", adv), ("ret", ret), ("advn", advn)):
            got = b.rollout(name)
            assert rc.same_bits(got, ref) and np.array_equal(got.view(U32), arrays[name].view()[:, :, 0]), name
        assert rc.same_bits(np.array(b.rollout_stats()), np.array(want)) and rc.same_bits(np.array(b.rollout_stats()), np.array(stats))
        assert np.array_equal(b.rollout("obs"), shared.dense[shared.role(P.RO_OBS)]) and b.rollout("done").dtype == I32
        assert b.rollout_launches() == (2 * shared.T, 2, 4)
        b.rollout_record(0, 5, 0)
        assert b.rollout_launches()[0] == 2 * shared.T
    finally:
        b.close()


def test_shared_case_with_bound_storage(cassie, shared, emulated):
    """Padded steps and rows in the caller's tensors, the sentinel beforehand: every word is the emulator's, so rows outside a range,
    other slots and the padding are left alone."""
    import torch
    b = Batch(cassie, shared.nenv)
    try:
        b.configure_rollout(shared.T, shared.srcs, shared.gamma, shared.lam, shared.tmask)
        stores, arrays = shared.stores()
        dev = [up(st.buf) for st in stores]
        arr = {name: up(st.buf) for name, st in arrays.items()}
        fence(b)
        for s, st in enumerate(stores):
            b.bind_rollout_storage(s, dev[s].data_ptr(), st.step, st.row)
        for name, st in arrays.items():
            b.bind_rollout_storage(name, arr[name].data_ptr(), st.step, st.row)
        assert b.rollout_ptr("advn") == (arr["advn"].data_ptr(), arrays["advn"].step, arrays["advn"].row)
        # one slot of one range first: everything else still holds the sentinel
        s_obs = shared.role(P.RO_OBS)
        keep = [up(a) for a in shared.steps[3]]
        fence(b)
        for s, a in enumerate(keep):
            b.bind_rollout_source(s, a.data_ptr(), shared.src_stride[s])
        b.rollout_record(3, *cases.RANGES[1])
        fence(b)
        written = shared.written([(3,) + cases.RANGES[1]])
        assert np.array_equal(words(dev[s_obs]), stores[s_obs].expected(shared.dense[s_obs], written))
        run_on_device(b, shared, [torch.cuda.Stream(), torch.cuda.Stream()])
        e_stores, e_arrays, stats = emulated
        for s, st in enumerate(e_stores):
            assert np.array_equal(words(dev[s]), st.buf), s
        for name, st in e_arrays.items():
            assert np.array_equal(words(arr[name]), st.buf), name
        assert rc.same_bits(np.array(b.rollout_stats()), np.array(stats))
        assert rc.same_bits(b.rollout("advn"), shared.normalised()[0])                     # the dense download of a padded tensor
        b.bind_rollout_storage("adv", None)                                                # the batch's own again, zeroed
        assert not b.rollout("adv").any() and b.rollout_ptr("adv")[1:] == (shared.nenv, 1)
    finally:
        b.close()


NOBS, NACT, NPOL = 12, 3, 3


def live_policy():
    import policy_cases
    rng = np.random.default_rng(21)
    return [policy_cases.dense(rng, (NOBS, 16, NACT), (P.POL_ELU, P.POL_TANH)), policy_cases.dense(rng, (NOBS, 16, 1), (P.POL_TANH, P.POL_IDENTITY))]


def test_live_batch_resolves_every_source(cassie):
    """130 envs, episodes (a time limit of 3 policy steps, the counters started apart), reward (float32), policy and sample bound, every
    source resolved from the bindings: three policy steps in the cycle end_episodes, record, observe, policy, act, step, reward.  Each
    slot equals the tensors downloaded at that step; finish with the NULL last value and normalise equal the restatement fed the
    downloaded slots; the calls change nothing of the batch or of the bound tensors."""
    import policy_cases
    import torch
    n = cases.NENV
    rng = np.random.default_rng(22)
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * rng.random(n)
    nets = live_policy()
    proto = policy_cases.Case("live", nets, np.zeros((n, NOBS), dtype=F32), pad=0, wpad=0)
    eps = np.clip(rng.normal(size=(NPOL + 1, n, NACT)), -4, 4).astype(F32)
    b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
    try:
        dev = "cuda"
        b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
        b.configure_states(n, P.STATE_CORE)
        b.enable_episodes(max_steps=3, min_height=0.4)
        b.set_reset_bank(b.make_reset_bank(cassie.qpos_init()[None]))
        steps0 = torch.from_numpy((np.arange(n) % 3).astype(I32)).cuda()
        b.bind_episode(P.EP_STEPS, steps0.data_ptr())
        obs_d = torch.zeros((n, NOBS + 2), dtype=torch.float32, device=dev)                 # a padded row
        act_d = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
        mu_d = torch.zeros((n, NACT + 1), dtype=torch.float32, device=dev)
        val_d = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        logp_d = torch.zeros(n, dtype=torch.float32, device=dev)
        eps_d, ls_d = torch.from_numpy(eps).cuda(), torch.full((NACT,), -1.5, dtype=torch.float32, device=dev)
        b.configure_obs([P.obs_copy(P.F_QPOS, 7, 10, scale=1.0), P.obs_copy(P.F_QVEL, 0, 2, scale=0.1)], history=1, dtype=np.float32)
        b.bind_obs(obs_d.data_ptr(), NOBS + 2)
        b.configure_actions([P.act_col(P.F_PD_PTARGET, j, lo=-1.5, hi=1.5, offset=float(bench.PD_OFFSET[j]), scale=0.2) for j in range(NACT)], dtype=np.float32)
        b.bind_actions(act_d.data_ptr(), NACT, torch.float32)
        b.configure_rewards([P.rew_vec(P.F_QPOS, 2, 1, target=0.9, norm=P.REW_SUMABS, shape=P.REW_EXP, k=10.0, weight=0.5),
                             P.rew_vec(P.F_QVEL, 0, 3, weight=-0.05)], dtype=np.float32, lo=-1.0, hi=1.0)
        b.configure_policy(proto.defs, NOBS)
        for a, layers in enumerate(proto.weights):
            b.load_policy(a, layers)
        b.bind_policy_input(obs_d.data_ptr(), NOBS, NOBS + 2, torch.float32)
        b.bind_policy_output(0, mu_d.data_ptr(), NACT + 1)
        b.bind_policy_output(1, val_d.data_ptr(), 2)
        srcs = [("obs", NOBS), ("action", NACT), ("logp", 1), ("mu", NACT), ("value", 1), ("reward", 1), ("done", 1), ("reason", 1)]
        b.configure_rollout(NPOL, srcs, 0.99, 0.95, timeout_mask=P.DONE_TIME)
        fence(b)
        st = torch.cuda.Stream()

        def forward(p):
            b.observe(stream=st.cuda_stream)
            b.bind_policy_sample(eps_d[p].data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
            b.policy(stream=st.cuda_stream)
            b.act(stream=st.cuda_stream)
            b.step_range(0, n, 50, st.cuda_stream)
            b.reward(stream=st.cuda_stream)

        def snapshot():
            fence(b)
            done, reason, steps, count, terminal = b.episodes()
            return {"obs": obs_d.cpu().numpy()[:, :NOBS].copy(), "action": act_d.cpu().numpy().copy(), "logp": logp_d.cpu().numpy().copy(),
                    "mu": mu_d.cpu().numpy()[:, :NACT].copy(), "value": val_d.cpu().numpy()[:, 0].copy(), "reward": b.rewards().copy(),
                    "done": done.copy(), "reason": reason.copy()}

        def everything():
            fence(b)
            b.save_states()
            tensors = [t.cpu().numpy().tobytes() for t in (obs_d, act_d, mu_d, val_d, logp_d, steps0)]
            return [b.states()[0].tobytes(), b.rewards().tobytes(), b.returns().tobytes()] + [a.tobytes() for a in b.episodes()] + tensors

        forward(0)
        slots = []
        for t in range(NPOL):
            b.end_episodes(0, n, True, stream=st.cuda_stream)
            slots.append(snapshot())
            before = everything() if t == NPOL - 1 else None
            for env0, cnt in cases.RANGES:
                b.rollout_record(t, env0, cnt, stream=st.cuda_stream)
            if before is not None:
                assert everything() == before
            forward(t + 1)
        last = snapshot()["value"]                                                          # V(o_T): observe and policy have run again
        before = everything()
        for env0, cnt in cases.RANGES:
            b.rollout_finish(env0, cnt, stream=st.cuda_stream)
        b.rollout_normalise(1e-8, stream=st.cuda_stream)
        assert everything() == before
        for name, dim in srcs:
            got, want = b.rollout(name), np.array([s[name] for s in slots])
            assert got.dtype == want.dtype and np.array_equal(got.view(U32), want.view(U32)), name
        done, reason = np.array([s["done"] for s in slots]), np.array([s["reason"] for s in slots])
        assert done.any() and not done.all() and np.all(reason[done != 0] == P.DONE_TIME)     # the time limit cut episodes, at every step some
        assert all(d.any() for d in done) and np.abs(slots[1]["obs"] - slots[0]["obs"]).max() > 1e-4
        val, rew = np.array([s["value"] for s in slots]), np.array([s["reward"] for s in slots])
        adv, ret, q1 = rc.gae(val, rew, done, reason, last, 0.99, 0.95, P.DONE_TIME)
        advn, stats, _ = rc.normalise(adv, q1, 1e-8)
        assert rc.same_bits(b.rollout("adv"), adv) and rc.same_bits(b.rollout("ret"), ret) and rc.same_bits(b.rollout("advn"), advn)
        assert rc.same_bits(np.array(b.rollout_stats()), np.array(stats)) and np.all(np.isfinite(advn))
        plain, _, _ = rc.gae(val, rew, done, reason, last, 0.99, 0.95, 0)
        assert not np.array_equal(plain, adv)                                                # the mask mattered
        assert b.rollout_launches() == (2 * NPOL, 2, 4)
    finally:
        b.close()


def test_refusals_with_a_batch(cassie):
    import policy_cases
    import torch
    n = 8
    b = Batch(cassie, n)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            b.rollout_record(0)
        base = [("value", 1), ("reward", 1)]
        val = torch.zeros(n, dtype=torch.float32, device="cuda")
        # rewards configured float64
        b.configure_rollout(2, base)
        b.bind_rollout_source("value", val.data_ptr())
        with pytest.raises(RuntimeError, match="REWARD: the rewards are not configured"):
            b.rollout_record(0)
        b.configure_rewards([P.rew_vec(P.F_QPOS, 2, 1)], dtype=np.float64, lo=-1.0, hi=1.0)
        with pytest.raises(RuntimeError, match="must be configured PHYS_OBS_F32"):
            b.rollout_record(0)
        b.configure_rewards([P.rew_vec(P.F_QPOS, 2, 1)], dtype=np.float32, lo=-1.0, hi=1.0)
        b.rollout_record(0)
        with pytest.raises(RuntimeError, match="slot t lies in"):
            b.rollout_record(2)
        # episodes not enabled with a DONE source unbound
        b.configure_rollout(2, base + [("done", 1)])
        b.bind_rollout_source("value", val.data_ptr())
        with pytest.raises(RuntimeError, match="DONE: episodes are not enabled"):
            b.rollout_record(0)
        done = torch.zeros(n, dtype=torch.int32, device="cuda")
        b.bind_rollout_source("done", done.data_ptr())
        b.rollout_record(0)
        b.bind_rollout_source("done", None)
        b.enable_episodes(max_steps=5)
        b.rollout_record(1)
        # a resolved dim that changed after configure
        rng = np.random.default_rng(4)
        obs = torch.zeros((n, 13), dtype=torch.float32, device="cuda")

        def policy(in_dim):
            proto = policy_cases.Case("p", [policy_cases.dense(rng, (in_dim, 4), (P.POL_TANH,))], np.zeros((n, in_dim), dtype=F32), pad=0, wpad=0)
            b.configure_policy(proto.defs, in_dim)
            b.bind_policy_input(obs.data_ptr(), in_dim, 13, torch.float32)

        policy(12)
        b.configure_rollout(2, base + [("obs", 12)])
        b.bind_rollout_source("value", val.data_ptr())
        b.rollout_record(0)
        policy(13)
        with pytest.raises(RuntimeError, match="dim no longer fits the configured dim"):
            b.rollout_record(0)
        policy(12)
        b.rollout_record(0)
        with pytest.raises(RuntimeError, match="VALUE"):
            b.bind_rollout_source("value", None)
            b.rollout_finish()
        with pytest.raises(ValueError, match="gamma is finite"):
            b.configure_rollout(2, base, gamma=1.5)
        with pytest.raises(ValueError, match="step stride"):
            b.bind_rollout_storage("adv", val.data_ptr(), step_stride=n - 1, row_stride=1)
        b.configure_rollout(2, [])
        with pytest.raises(RuntimeError, match="not configured"):
            b.rollout_normalise()
    finally:
        b.close()
