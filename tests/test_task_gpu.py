"""Task rows (phys_batch_task) on the device against the definition restated in numpy and Python integers (tests/task_check.py), BIT
FOR BIT: every step of a column's value -- the draws, the clocks, sin2pi / cos2pi, the gates, the interpolation -- is one individually
rounded fp64 operation in the kernel (no fused multiply-add outside a division's own expansion, nothing left to the compiler's
contraction), the draws are integer arithmetic, and the cast rounds to nearest even; so the device, the wave emulator
(tests/test_task.py) and numpy must agree on every bit.  Also: two ranges on two streams, that a call changes nothing of the batch but its
own rows, state, counts and destination elements, that a step launch reads the pushes the call wrote, the whole policy step with the
task row as the input of the observation, the reward and the action, and a resumed run."""
import numpy as np
import pytest

import actions_check as ac
import bench
import obs_check as oc
import rewards_check as rc
import task_cases as cases
import task_check as tc
from cassie_amd import Batch
from cassie_amd import phys as P
from test_actions_gpu import fence, snapshot
from test_episodes_gpu import bank_states, make

pytestmark = pytest.mark.gpu
FILL = -7.25


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_definition_on_the_device(cassie, dtype):
    """The emulator's case on the device: 19 columns of every kind over fourteen calls (a first call, periods that run out, a
    sub-range, a reset), the rows bound to a torch tensor with a row stride and padding that stays, the reset words in a torch tensor, a
    caller's stream.  After every call the rows, the state, the words, the counts and xfrc_applied are the reference's."""
    import torch
    cols, table, start = cases.columns_of(cassie.pod), cases.make_table(), cases.start_fields(cassie)
    want = cases.reference(cols, table, dtype, start)
    ncols, stride = cases.NCOLS, cases.ROW_STRIDE
    tdtype = torch.float32 if dtype is np.float32 else torch.float64
    b = Batch(cassie, cases.NENV)
    try:
        b.set(P.F_XFRC_APPLIED, start[P.F_XFRC_APPLIED])
        b.set_task_table(table)
        b.configure_task(cols, dtype=dtype, seed=cases.SEED)
        assert b.task_dim() == ncols and b.task_launches() == 0
        rows_d = torch.full((cases.NENV, stride), FILL, dtype=tdtype, device="cuda")
        b.bind_task_rows(rows_d.data_ptr(), stride)
        st = torch.cuda.Stream()
        for k, (env0, n, reset) in enumerate(cases.SCHEDULE):
            reset_d = None if reset is None else torch.tensor(reset, dtype=torch.int32, device="cuda")
            fence(b)
            b.task(env0, n, reset_ptr=None if reset_d is None else reset_d.data_ptr(), stream=st.cuda_stream)
            fence(b)
            rows, (state, words, counts) = b.task_rows(), b.task_state()
            assert rows.dtype == dtype and oc.same_bits(rows, want[k][0]), k
            assert oc.same_bits(state, want[k][1]) and np.array_equal(words, want[k][2]) and np.array_equal(counts, want[k][3]), k
            assert oc.same_bits(b.get(P.F_XFRC_APPLIED), want[k][4][P.F_XFRC_APPLIED]), k
            raw = rows_d.cpu().numpy()
            assert oc.same_bits(raw[:, :ncols], rows) and np.all(raw[:, ncols:] == dtype(FILL))
        assert b.task_launches() == len(cases.SCHEDULE)
        assert oc.same_bits(b.task_rows(1, 3), want[-1][0][1:4])
    finally:
        b.close()


def test_two_ranges_on_two_streams_equal_one(cassie):
    import torch
    cols, table, start = cases.columns_of(cassie.pod), cases.make_table(), cases.start_fields(cassie)
    sched = tuple((0, cases.NENV, r) for _, _, r in cases.SCHEDULE)
    want = cases.reference(cols, table, np.float32, start, schedule=sched)
    b = Batch(cassie, cases.NENV)
    try:
        b.set(P.F_XFRC_APPLIED, start[P.F_XFRC_APPLIED])
        b.set_task_table(table)
        b.configure_task(cols, dtype=np.float32, seed=cases.SEED)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        fence(b)
        for k, (_, _, reset) in enumerate(sched):
            reset_d = torch.tensor(reset if reset is not None else [0] * cases.NENV, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for (e0, cnt), st in zip(((0, 2), (2, 3)), streams):
                b.task(e0, cnt, reset_ptr=reset_d.data_ptr() + 4 * e0, stream=st.cuda_stream)
            fence(b)
            state, words, counts = b.task_state()
            assert oc.same_bits(b.task_rows(), want[k][0]) and oc.same_bits(state, want[k][1]) and np.array_equal(words, want[k][2]), k
            assert np.array_equal(counts, want[k][3]) and oc.same_bits(b.get(P.F_XFRC_APPLIED), want[k][4][P.F_XFRC_APPLIED]), k
        assert b.task_launches() == 2 * len(sched)
    finally:
        b.close()


def test_nothing_else_is_touched(cassie):
    """Around one task call of the whole batch in the middle of a loop, every field, the warning words, the solver statistics, the
    drive-level state and the episode arrays are byte for byte what they were -- except the two elements of xfrc_applied the push
    columns name."""
    n = 8
    cols, table = cases.columns_of(cassie.pod), cases.make_table()
    bq, bv = bank_states(cassie, 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
        b.set(P.F_XFRC_APPLIED, np.full((n, 6 * cassie.pod.nbody), 0.125))
        b.enable_episodes(max_steps=2, min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.set_task_table(table)
        b.configure_task(cols, dtype=np.float64, seed=1)
        for _ in range(2):
            b.step(20)
            b.end_episodes()
        fence(b)
        before = snapshot(b, episodes=True)
        b.task(reset_ptr=b.episode_ptr(P.EP_DONE))
        fence(b)
        after = snapshot(b, episodes=True)
        named = np.array(cases.push_elems(cassie.pod))
        for key in before:
            if key != P.F_XFRC_APPLIED:
                assert after[key] == before[key], key
                continue
            was, now = (np.frombuffer(s[key]).reshape(n, -1) for s in (before, after))
            rest = np.setdiff1d(np.arange(was.shape[1]), named)
            assert was[:, rest].tobytes() == now[:, rest].tobytes() and not (was[:, named] == now[:, named]).any()
        assert oc.same_bits(b.get(P.F_XFRC_APPLIED)[:, named], b.task_rows()[:, [cases.PUSH_X, cases.PUSH_Y]])
    finally:
        b.close()


def test_the_step_reads_the_pushes(cassie):
    """Three batches of 5 envs, 4 policy steps of 20 substeps.  The first calls task in front of every step_range; the second has the
    reference's xfrc_applied uploaded with set(); the third is never pushed.  The first two are equal in every state field; on a step
    where a push is on, they differ from the third."""
    import torch
    n, npol = cases.NENV, 4
    cols, table = cases.columns_of(cassie.pod), cases.make_table()
    zero = {P.F_XFRC_APPLIED: np.zeros((n, 6 * cassie.pod.nbody))}
    want = cases.reference(cols, table, np.float64, zero, schedule=((0, n, None),) * npol)
    pushed = [w[4][P.F_XFRC_APPLIED] for w in want]
    assert pushed[0].any() and not pushed[1].any() and any(p.any() for p in pushed[2:])        # (on at the draw, off the call after)

    def run(mode):
        b = make(cassie, n, P.DRIVE_PD_SAFE)
        try:
            b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
            b.set(P.F_XFRC_APPLIED, zero[P.F_XFRC_APPLIED])
            if mode == "task":
                b.set_task_table(table)
                b.configure_task(cols, dtype=np.float64, seed=cases.SEED)
            st = torch.cuda.Stream()
            fence(b)
            first = None
            for p in range(npol):
                if mode == "task":
                    b.task(stream=st.cuda_stream)
                elif mode == "set":
                    b.set(P.F_XFRC_APPLIED, pushed[p])
                b.step_range(0, n, 20, st.cuda_stream)
                fence(b)
                first = first or snapshot(b)
            return first, snapshot(b)
        finally:
            b.close()

    (t0, t), (s0, s), (z0, z) = run("task"), run("set"), run("none")
    for key in t:
        assert t[key] == s[key] and t0[key] == s0[key], key
    assert t0[P.F_QVEL] != z0[P.F_QVEL] and t[P.F_QPOS] != z[P.F_QPOS]


def test_the_whole_policy_step(cassie):
    """8 envs, 12 policy steps of 2 substeps in the order act, step, reward, end_episodes, task, observe on one stream.  ONE float32
    input tensor [n][task row | action rows] is bound by all four stages: the task row is its first column block, the action rows its
    second; the action adds onto the reference pose of the TABLE columns, the reward tracks the command and is gated by the swing gate,
    the observation shows command, clock and reference.  Rows, rewards and observations are those of the four numpy restatements chained;
    episodes end by step count at different steps for different envs, and the restarted envs draw anew."""
    import torch
    n, npol, nsub, seed, na = 8, 12, 2, 31, 10
    V, CLK, SN, CS, GT, REF = 0, 4, 5, 6, 7, 8            # the task row: vx vy yaw | freq | clock | sin cos | gate | 10 table columns
    tcols = [P.task_sample(0.4, 0.6, 2, 4, p_rest=0.3), P.task_sample(0.0, 0.2, 2, 4, p_rest=0.3, group=0), P.task_sample(0.0, 0.4, 2, 4, p_rest=0.3, group=0),
             P.task_sample(1.0, 0.4, 3, 6), P.task_phase(rate=0.04, rate_col=3, rate_scale=0.1), P.task_wave(4, P.TASK_SIN), P.task_wave(4, P.TASK_COS),
             P.task_wave(4, P.TASK_TRAPEZOID, duty=0.45, ramp=0.1)]
    tcols += [P.task_table(4, j, shift=0.5 * (j >= 5)) for j in range(na)]
    nt = len(tcols)
    W = nt + 3 * na
    now, prev = nt + P.ACT_NOW * na, nt + P.ACT_PREV * na
    rng = np.random.default_rng(17)
    table = (bench.PD_OFFSET + 0.05 * rng.uniform(-1.0, 1.0, (40, na)))
    acols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, noise=0.02, smooth=0.5, bfield=P.ACT_INPUT, bindex=REF + j, scale=0.1) for j in range(na)]
    oterms = [P.obs_copy(P.F_QPOS, 7, 4), P.obs_copy(P.OBS_INPUT, V, 3), P.obs_copy(P.OBS_INPUT, SN, 2, noise=0.01), P.obs_copy(P.OBS_INPUT, REF, na),
              P.obs_copy(P.OBS_INPUT, prev, na)]
    rterms = [P.rew_vec(P.F_QVEL, 0, 3, tfield=P.REW_INPUT, tindex=V, shape=P.REW_EXP, k=2.0, weight=0.5),
              P.rew_vec(P.F_QPOS, 7, 4, tfield=P.REW_INPUT, tindex=REF, weight=-0.2, gate=(P.REW_INPUT, GT)),
              P.rew_vec(P.REW_INPUT, now, na, tfield=P.REW_INPUT, tindex=prev, weight=-0.1)]
    acts = rng.uniform(-1.2, 1.2, (npol, n, na)).astype(np.float32)
    acts_d = torch.from_numpy(acts).cuda()
    inp_d = torch.zeros((n, W), dtype=torch.float32, device="cuda")
    bq, bv = bank_states(cassie, 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.enable_episodes(max_steps=5, min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        for _ in range(2):
            b.end_episodes(0, 3)                  # (envs 0 .. 2 are two steps ahead: they end at other steps than the rest)
        b.set_task_table(table)
        b.configure_task(tcols, dtype=np.float32, seed=seed)
        b.bind_task_rows(inp_d.data_ptr(), W)
        b.configure_actions(acols, delay_max=1, dtype=np.float32, seed=seed)
        b.bind_action_rows(inp_d.data_ptr() + 4 * nt, W)
        b.bind_action_input(inp_d.data_ptr(), W, W, torch.float32)
        b.configure_obs(oterms, history=2, dtype=np.float32, seed=seed)
        b.bind_obs_input(inp_d.data_ptr(), W, W, torch.float32)
        b.configure_rewards(rterms, dtype=np.float32)
        b.bind_reward_input(inp_d.data_ptr(), W, W, torch.float32)
        tref = tc.Task(tcols, n, np.float32, seed, table=table)
        aref, held = ac.Actions(acols, n, 1, np.float32, seed), {P.F_PD_PTARGET: np.zeros((n, cassie.pod.nu))}
        oref, rref = oc.Obs(oterms, n, 2, np.float32, seed), rc.Rewards(rterms, n, np.float32)
        st = torch.cuda.Stream()
        done_ptr = b.episode_ptr(P.EP_DONE)
        # the row of the first policy step: a task call before the loop, as a reset of the whole batch would make it
        b.task(stream=st.cuda_stream)
        tref.task({})
        fence(b)
        inp = np.zeros((n, W), dtype=np.float32)
        inp[:, :nt] = tref.rows
        done, restarts, resampled = np.zeros(n, dtype=np.int32), 0, 0
        for p in range(npol):
            b.bind_actions(acts_d[p].data_ptr(), na, torch.float32)
            b.act(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.step_range(0, n, nsub, st.cuda_stream)
            b.reward(reset_ptr=done_ptr, stream=st.cuda_stream)
            fence(b)                                  # (the test reads the state the reward saw, before a restart replaces it)
            held[P.ACT_INPUT] = inp
            aref.act(acts[p], held, reset=done)
            inp[:, nt:] = aref.rows.reshape(n, 3 * na)
            assert oc.same_bits(b.get(P.F_PD_PTARGET), held[P.F_PD_PTARGET]), p
            fields = {P.F_QPOS: b.get(P.F_QPOS), P.F_QVEL: b.get(P.F_QVEL), P.REW_INPUT: inp}
            assert oc.same_bits(b.rewards(), rref.reward(fields, reset=done)), p
            b.end_episodes(stream=st.cuda_stream)
            b.task(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.observe(refill_ptr=done_ptr, stream=st.cuda_stream)
            fence(b)
            done = b.episodes()[0].astype(np.int32)
            restarts += int(done.sum())
            tref.task({}, reset=done)
            resampled += int(tref.drew[done != 0][:, :4].all()) if done.any() else 0
            inp[:, :nt] = tref.rows
            assert oc.same_bits(inp_d.cpu().numpy(), inp) and oc.same_bits(b.task_rows(), tref.rows), p
            fields = {P.F_QPOS: b.get(P.F_QPOS), P.OBS_INPUT: inp}
            assert oc.same_bits(b.obs(), oref.observe(fields, refill=done)), p
        assert restarts >= n and resampled >= 2            # (every env ended once at least; the restarted envs drew on the reset)
        state, words, counts = b.task_state()
        assert oc.same_bits(state, tref.state) and np.array_equal(words, tref.words) and list(counts) == [npol + 1] * n
        assert b.task_launches() == npol + 1
    finally:
        b.close()


def test_resume_from_the_downloaded_state(cassie):
    """A second batch given task_state() of the first after six calls makes what the first makes from the seventh on."""
    cols, table, start = cases.columns_of(cassie.pod), cases.make_table(), cases.start_fields(cassie)
    sched = ((0, cases.NENV, None),) * 9
    want = cases.reference(cols, table, np.float64, start, schedule=sched)
    a, c = Batch(cassie, cases.NENV), Batch(cassie, cases.NENV)
    try:
        for b in (a, c):
            b.set(P.F_XFRC_APPLIED, start[P.F_XFRC_APPLIED])
            b.set_task_table(table)
            b.configure_task(cols, dtype=np.float64, seed=cases.SEED)
        for _ in range(6):
            a.task()
        state, words, counts = a.task_state()
        assert list(counts) == [6] * cases.NENV and not oc.same_bits(c.task_state()[0], state)
        c.set_task_state(state, words, counts)
        for k in range(6, 9):
            for b in (a, c):
                b.task()
                got = b.task_state()
                assert oc.same_bits(b.task_rows(), want[k][0]) and oc.same_bits(got[0], want[k][1]) and np.array_equal(got[1], want[k][2]), k
                assert np.array_equal(got[2], want[k][3]) and oc.same_bits(b.get(P.F_XFRC_APPLIED), want[k][4][P.F_XFRC_APPLIED]), k
    finally:
        a.close()
        c.close()


def test_counters_bindings_and_refusals(cassie):
    import torch
    pod = cassie.pod
    b = Batch(cassie, 4)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            b.task()
        with pytest.raises(RuntimeError, match="not configured"):
            b.task_dim()
        with pytest.raises(ValueError, match="1 .. 64 columns"):
            b.configure_task([])
        with pytest.raises(ValueError, match="a TABLE column and no table"):
            b.configure_task([P.task_phase(), P.task_table(0, 0)])
        with pytest.raises(ValueError, match="command field"):
            b.configure_task([P.task_sample(dfield=P.F_QPOS)])
        with pytest.raises(ValueError, match="dindex lies beyond"):
            b.configure_task([P.task_sample(dfield=P.F_XFRC_APPLIED, dindex=6 * pod.nbody)])
        with pytest.raises(ValueError, match="same destination element"):
            b.configure_task([P.task_sample(dfield=P.F_CTRL, dindex=1), P.task_sample(dfield=P.F_CTRL, dindex=1)])
        with pytest.raises(ValueError, match="group names a SAMPLE column"):
            b.configure_task([P.task_phase(), P.task_sample(group=0)])
        with pytest.raises(ValueError, match="src is a PHASE column"):
            b.configure_task([P.task_sample(), P.task_wave(0)])
        with pytest.raises(ValueError, match="dtype"):
            b.configure_task([P.task_sample()], dtype=np.float16)
        with pytest.raises(RuntimeError, match="a table of 1 .. 4096 frames"):
            b.set_task_table(np.zeros((2, 65)))
        with pytest.raises(ValueError, match="not configured"):
            b.bind_task_rows(1 << 20, 4)
        b.set_task_table(np.arange(12.0).reshape(4, 3))
        c = [P.task_sample(2.0, 0.0, dfield=P.F_CTRL, dindex=1), P.task_phase(rate=0.25), P.task_table(1, 2), P.task_wave(1, P.TASK_COS)]
        b.configure_task(c, dtype=np.float32)
        assert b.task_dim() == 4 and b.task_launches() == 0
        with pytest.raises(RuntimeError, match="out of bounds"):
            b.task(2, 3)
        with pytest.raises(RuntimeError, match="reach beyond the new table"):
            b.set_task_table(np.zeros((4, 2)))
        buf = torch.zeros((4, 5), dtype=torch.float32, device="cuda")
        with pytest.raises(ValueError, match="row stride"):
            b.bind_task_rows(buf.data_ptr(), 3)
        b.task()
        b.task(1, 2)
        state, words, counts = b.task_state()
        assert b.task_launches() == 2 and list(counts) == [1, 2, 2, 1] and state.shape == (4, 4) and words.shape == (4, 3, 4)
        rows = b.task_rows()
        assert rows.dtype == np.float32 and np.all(rows[:, 0] == 2.0) and list(rows[:, 1]) == [0.0, 0.25, 0.25, 0.0]
        assert list(rows[:, 2]) == [2.0, 5.0, 5.0, 2.0] and list(rows[:, 3]) == [1.0, 0.0, 0.0, 1.0]
        assert np.all(b.get(P.F_CTRL)[:, 1] == 2.0) and np.all(b.get(P.F_CTRL)[:, 2:] == 0.0)
        # configuring again zeroes the state and the counts and drops the binding
        b.bind_task_rows(buf.data_ptr(), 5)
        b.configure_task(c, dtype=np.float64)
        assert list(b.task_state()[2]) == [0] * 4 and not b.task_state()[0].any() and b.task_rows().dtype == np.float64 and not b.task_rows().any()
    finally:
        b.close()
