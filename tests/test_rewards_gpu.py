"""Reward rows (phys_batch_reward) on the device against the definition restated in numpy (tests/rewards_check.py), BIT FOR BIT: every
step of a term -- the rotation, the errors, the norm, expn's polynomial, the weight and the gate, the sum over the terms, the return --
is one individually rounded fp64 operation in the kernel (no fused multiply-add, nothing left to the compiler's contraction), so the
device, the wave emulator (tests/test_rewards.py) and numpy must agree on every bit.  Also: two ranges on two streams behind real step
launches with probes, step sums and episodes that end, where the calls must change nothing of the batch but their own outputs; and the
bindings, counters and refusals through Batch."""
import numpy as np
import pytest

import bench
import rewards_cases as cases
import rewards_check as rc
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import bank_states, drive_bytes, make
from test_probes import cassie_probes
from test_probes_gpu import STATE_FIELDS

pytestmark = pytest.mark.gpu
FILL = -7.25


@pytest.fixture(scope="module")
def states(cassie):
    """One state per call of the schedule (shared, left unchanged)."""
    return cases.make_states(cassie)


def put(b, state):
    for f in (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA):
        b.set(f, state[f])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_definition_on_the_device(cassie, states, dtype):
    """The emulator's case on the device: thirteen terms over five calls (the batch twice, a sub-range, two episodes reset, the batch
    again) on states that change, one env past expn's cut, one with a NaN velocity.  The float32 input is a torch tensor with a row
    stride; the rewards go into column 1 of a torch tensor [nenv][3] and the term rows into a torch tensor five elements wider than the
    terms, whose gaps stay.  Rewards, term rows, ret and final are tests/rewards_check.py's after every call, bit for bit."""
    import torch
    terms = cases.terms_of(cassie.pod)
    want = cases.reference(terms, states, dtype)
    nt, tdt = len(terms), torch.float32 if dtype is np.float32 else torch.float64
    b = Batch(cassie, cases.NENV)
    try:
        b.configure_rewards(terms, dtype=dtype, lo=cases.LO, hi=cases.HI)
        assert b.reward_dim() == (nt, np.dtype(dtype).itemsize, False)
        inp = torch.zeros((cases.NENV, cases.INPUT_STRIDE), dtype=torch.float32, device="cuda")
        b.bind_reward_input(inp.data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
        rew_d = torch.full((cases.NENV, 3), FILL, dtype=tdt, device="cuda")
        rows_d = torch.full((cases.NENV, nt + 5), FILL, dtype=tdt, device="cuda")
        b.bind_rewards(rew_d.data_ptr() + rew_d.element_size(), 3)
        b.bind_reward_terms(rows_d.data_ptr(), nt + 5)
        assert b.reward_dim()[2]
        st = torch.cuda.Stream()
        for k, (state, (env0, n, reset)) in enumerate(zip(states, cases.SCHEDULE)):
            put(b, state)
            b.sync()
            inp.copy_(torch.from_numpy(state[P.REW_INPUT]))
            reset_d = None if reset is None else torch.tensor(reset, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            b.reward(env0, n, reset_ptr=None if reset_d is None else reset_d.data_ptr(), stream=st.cuda_stream)
            b.sync()
            torch.cuda.synchronize()
            got = (b.rewards(), b.reward_terms(), b.returns(), b.final_returns())
            assert got[0].dtype == dtype and got[1].dtype == dtype
            for a, w, name in zip(got, want[k], ("rewards", "term rows", "ret", "final")):
                assert rc.same_bits(a, w), (k, name)
            raw, rows = rew_d.cpu().numpy(), rows_d.cpu().numpy()
            assert rc.same_bits(raw[:, 1], got[0]) and np.all(raw[:, 0] == dtype(FILL)) and np.all(raw[:, 2] == dtype(FILL))
            assert rc.same_bits(rows[:, :nt], got[1]) and np.all(rows[:, nt:] == dtype(FILL))
        assert b.reward_launches() == len(cases.SCHEDULE)
        assert rc.same_bits(b.rewards(1, 3), want[-1][0][1:4]) and rc.same_bits(b.reward_terms(4, 2), want[-1][1][4:6])
        assert want[0][1][cases.ENV_CUT, 11] == 0 and np.isnan(want[-1][2][cases.ENV_NAN])
    finally:
        b.close()


def test_the_loop_is_not_disturbed(cassie):
    """Two batches of 8 envs in DRIVE_PD_SAFE run step_range(50 substeps) x 4 on two ranges and two streams, with the step sums on and
    behind every step launch a probe and end_episodes with restart, on the range's stream; the second batch with a reward of the range
    between the two -- its sources F_PROBES, F_STEP_SUMS and F_QPOS, its reset words the range's slice of EP_DONE as the previous policy
    step left it.  Every field, the probes' rows, the step sums, the warning words, the solver statistics, the drive-level state and the
    episode arrays are byte for byte those of the loop without the reward calls.  For an env whose episode ended at policy step p, final
    is the sequential sum of its rewards up to p and ret restarts from the next one.  A last call over the batch gives the definition's
    rewards on the downloaded sources."""
    import torch
    pod = cassie.pod
    n, npol, k = 8, 4, 4
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * np.arange(n)
    tgd = torch.from_numpy(bench.pd_targets(np.arange(n), npol)).cuda()
    pick_d = torch.from_numpy(np.random.default_rng(7).integers(0, k, (npol, n)).astype(np.int32)).cuda()
    bq, bv = bank_states(cassie, k)
    probes = cassie_probes(cassie)[:3]
    ranges = [(0, 4), (4, 4)]
    foot = cassie.name2id(1, "left-foot")

    def terms_of(b):
        pos = b.probe_layout()["pos"][0]
        return [P.rew_vec(P.F_PROBES, pos + 2, 1, target=0.9, dead=0.01, norm=P.REW_SUMABS, shape=P.REW_RATIONAL, k=4.0, weight=0.3),     # the pelvis' height
                P.rew_vec(P.F_PROBES, pos + 3, 3, tfield=P.F_PROBES, tindex=pos + 6, root=True, shape=P.REW_EXP, k=2.0, weight=0.2),       # foot to foot
                P.rew_vec(P.F_STEP_SUMS, P.SUM_ACT_POWER, pod.nu, norm=P.REW_SUMABS, weight=-1e-4),
                P.rew_quat(P.F_QPOS, 3, shape=P.REW_EXP, k=3.0, weight=0.25),
                P.rew_vec(P.F_QPOS, 7, 5, norm=P.REW_MAXABS, weight=0.01, gate=(P.F_STEP_SUMS, P.SUM_BODY_TOUCH + foot)),
                P.rew_rot_inv(P.F_QVEL, 0, P.F_QPOS, 3, shape=P.REW_EXP, k=1.0, weight=0.25)]

    def snapshot(b):
        out = {f: b.get(f).tobytes() for f in STATE_FIELDS + (P.F_PROBES, P.F_STEP_SUMS)}
        w, info = b.warnings()
        out["warn"], out["info"], out["drive"] = w.tobytes(), info.tobytes(), drive_bytes(b)
        out["episodes"] = b"".join(a.tobytes() for a in b.episodes())
        return out

    def run(rewarding):
        b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
        try:
            b.enable_step_sums()
            b.enable_episodes(max_steps=2, min_height=0.6)
            bank_d = torch.from_numpy(b.make_reset_bank(bq, bv)).cuda()
            b.set_reset_bank(device_ptr=bank_d.data_ptr(), n=k)
            b.configure_probes(probes, P.PQ_POS | P.PQ_VEL)
            done_d = torch.zeros(n, dtype=torch.int32, device="cuda")
            b.bind_episode(P.EP_DONE, done_d.data_ptr())
            hist_d = torch.zeros((npol, n), dtype=torch.int32, device="cuda")       # the done words after every policy step
            rew_d = torch.zeros((npol, n), dtype=torch.float64, device="cuda")       # the rewards of every policy step
            b.step_range(0, n, 1)                                                    # (sizes F_STEP_SUMS)
            terms = terms_of(b)
            if rewarding:
                b.configure_rewards(terms, dtype=np.float64)
            b.sync()
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for p in range(npol):
                b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
                if rewarding:
                    b.bind_rewards(rew_d[p].data_ptr(), 1)
                for (e0, cnt), st in zip(ranges, streams):
                    b.step_range(e0, cnt, 50, st.cuda_stream)
                    b.probe(e0, cnt, stream=st.cuda_stream)
                    if rewarding:
                        b.reward(e0, cnt, reset_ptr=b.episode_ptr(P.EP_DONE) + 4 * e0, stream=st.cuda_stream)
                    b.end_episodes(e0, cnt, True, pick_ptr=pick_d[p].data_ptr() + 4 * e0, stream=st.cuda_stream)
                    with torch.cuda.stream(st):
                        hist_d[p, e0:e0 + cnt].copy_(done_d[e0:e0 + cnt])
            b.sync()
            torch.cuda.synchronize()
            res = None
            if rewarding:
                assert b.reward_launches() == 2 * npol
                loop = (rew_d.cpu().numpy(), hist_d.cpu().numpy(), b.returns(), b.final_returns())
                b.bind_rewards(None)
                b.reward()
                b.sync()
                assert b.reward_launches() == 2 * npol + 1
                fields = {f: b.get(f) for f in (P.F_PROBES, P.F_STEP_SUMS, P.F_QPOS, P.F_QVEL)}
                res = loop + (b.rewards(), fields, terms)
            return snapshot(b), res
        finally:
            b.close()

    want, _ = run(False)
    got, (rew, hist, ret, fin, last, fields, terms) = run(True)
    for key in want:
        assert got[key] == want[key], key
    # the returns, env by env, from the rewards and the done words of every policy step
    assert hist.any() and np.all(np.isfinite(rew)) and np.abs(rew).min() > 0
    for e in range(n):
        r, f, seen = np.float64(0.0), np.float64(0.0), False
        for p in range(npol):
            if p > 0 and hist[p - 1, e]:
                f, r, seen = r, np.float64(0.0), True
            r = r + rew[p, e]
        assert ret[e].tobytes() == r.tobytes() and fin[e].tobytes() == f.tobytes(), e
        assert seen and fin[e] != 0 and ret[e] != fin[e], e      # (max_steps = 2: every env ended an episode before the last policy step)
    # the last call: the definition on what the batch holds
    ref = rc.Rewards(terms, n, np.float64)
    assert rc.same_bits(last, ref.reward(fields)) and np.abs(last).min() > 0
    assert np.abs(fields[P.F_STEP_SUMS][:, P.SUM_ACT_POWER:P.SUM_ACT_POWER + pod.nu]).max() > 0 and fields[P.F_PROBES].any()


def test_counters_bindings_and_refusals(cassie):
    import torch
    pod = cassie.pod
    b = Batch(cassie, 4)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            b.reward()
        with pytest.raises(RuntimeError, match="not configured"):
            b.reward_dim()
        with pytest.raises(ValueError, match="does not hold yet"):
            b.configure_rewards([P.rew_vec(P.F_STEP_SUMS, 0, 1)])
        with pytest.raises(ValueError, match="PHYS_F_DEPTH"):
            b.configure_rewards([P.rew_vec(P.F_DEPTH, 0, 1)])
        with pytest.raises(ValueError, match="index \\+ count"):
            b.configure_rewards([P.rew_vec(P.F_QPOS, pod.nq - 1, 2)])
        with pytest.raises(ValueError, match="k >= 0"):
            b.configure_rewards([P.rew_vec(P.F_QPOS, 0, 2, shape=P.REW_EXP, k=-1.0)])
        with pytest.raises(ValueError, match="lo <= hi"):
            b.configure_rewards([P.rew_vec(P.F_QPOS, 0, 2)], lo=1.0, hi=0.0)
        with pytest.raises(ValueError, match="dtype"):
            b.configure_rewards([P.rew_vec(P.F_QPOS, 0, 2)], dtype=np.float16)
        with pytest.raises(ValueError, match="0 .. 64 terms"):
            b.configure_rewards([P.rew_vec(P.F_QPOS, 0, 2)] * 65)
        t = [P.rew_vec(P.F_QPOS, 2, 1, weight=2.0), P.rew_vec(P.REW_INPUT, 2, 3, norm=P.REW_SUMABS)]
        b.configure_rewards(t, dtype=np.float64)
        assert b.reward_dim() == (2, 8, False) and b.reward_launches() == 0
        with pytest.raises(RuntimeError, match="no term rows"):
            b.reward_terms()
        with pytest.raises(RuntimeError, match="no input bound"):
            b.reward()
        inp = torch.ones((4, 5), dtype=torch.float64, device="cuda")
        b.bind_reward_input(inp.data_ptr(), 4, 5, torch.float64)
        with pytest.raises(RuntimeError, match="shorter"):
            b.reward()
        b.bind_reward_input(inp.data_ptr(), 5, 5, torch.float64)
        with pytest.raises(RuntimeError, match="out of bounds"):
            b.reward(2, 3)
        with pytest.raises(ValueError, match="row stride"):
            b.bind_reward_terms(inp.data_ptr(), 1)
        with pytest.raises(ValueError, match="element stride"):
            b.bind_rewards(inp.data_ptr(), 0)
        b.bind_reward_terms(own=True)
        assert b.reward_dim() == (2, 8, True)
        b.reward()
        b.reward(1, 2)
        z = b.get(P.F_QPOS)[:, 2]
        r = (2.0 * (z * z)) + 3.0
        assert b.reward_launches() == 2 and np.array_equal(b.rewards(), r) and np.array_equal(b.reward_terms(), np.stack([2.0 * (z * z), np.full(4, 3.0)], axis=1))
        assert np.array_equal(b.returns(), r * np.array([1, 2, 2, 1])) and not b.final_returns().any()
        # returns set by the caller, moved to final by a reset word
        b.set_returns([10.0, 20.0, 30.0, 40.0])
        reset = torch.tensor([0, 1, 0, 0], dtype=torch.int32, device="cuda")
        b.reward(reset_ptr=reset.data_ptr())
        assert np.array_equal(b.returns(), np.array([10.0, 0.0, 30.0, 40.0]) + r) and list(b.final_returns()) == [0.0, 20.0, 0.0, 0.0]
        # the term rows off again; configuring again zeroes the returns and drops the bindings; no terms releases everything
        b.bind_reward_terms()
        assert b.reward_dim() == (2, 8, False)
        b.configure_rewards(t, dtype=np.float32)
        assert not b.returns().any() and not b.final_returns().any() and b.rewards().dtype == np.float32 and b.reward_dim() == (2, 4, False)
        with pytest.raises(RuntimeError, match="no input bound"):
            b.reward()
        b.configure_rewards([])
        with pytest.raises(RuntimeError, match="not configured"):
            b.reward()
        with pytest.raises(RuntimeError, match="not configured"):
            b.returns()
    finally:
        b.close()
