"""Action rows (phys_batch_act) on the device against the definition restated in numpy and Python integers (tests/actions_check.py),
BIT FOR BIT: every step of a column's value -- the noise, the low-pass, the affine map -- is one individually rounded fp64 operation in
the kernel (no fused multiply-add, nothing left to the compiler's contraction), the noise is integer arithmetic, and the cast rounds to
nearest even; so the device, the wave emulator (tests/test_actions.py) and numpy must agree on every bit.  Also: that a step launch reads
what the call wrote, two ranges on two streams, that a call changes nothing of the batch but its own rows, state, counts and destination
elements, the reset from the episodes' done words, a resumed run, and the action row as the input of the observation and the reward."""
import numpy as np
import pytest

import actions_cases as cases
import actions_check as ac
import bench
import obs_check as oc
import rewards_check as rc
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import bank_states, drive_bytes, make
from test_probes_gpu import STATE_FIELDS

pytestmark = pytest.mark.gpu
FILL = -7.25


@pytest.fixture(scope="module")
def calls(cassie):
    """The actions and the input of every call of the schedule (shared, left unchanged)."""
    return cases.make_calls(cassie)


def fence(b):
    import torch
    b.sync()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_definition_on_the_device(cassie, calls, dtype):
    """The emulator's case on the device: 70 columns, a delay line of depth 3 with per-env delays (one beyond the depth) over seven calls
    (fill, three shifts, a sub-range, a reset, a shift), the float32 actions in a torch tensor with a row stride, the rows bound to a
    torch tensor with padding that stays, the input and the delays in torch tensors.  float32: F_PD_PTARGET bound to a caller's tensor;
    float64: the batch's own.  After every call the rows, the state, the counts and the destination fields are the reference's.
    (xfrc_applied is the batch's own dense buffer here: phys_batch_bind_strided takes no command field, so a destination with a row
    stride is the emulator's case alone.)"""
    import torch
    cols, start = cases.columns_of(cassie.pod), cases.start_fields(cassie)
    want = cases.reference(cols, calls, dtype, start)
    ncols, D, pad = cases.NCOLS, cases.DELAY_MAX, 5
    tdtype = torch.float32 if dtype is np.float32 else torch.float64
    b = Batch(cassie, cases.NENV)
    try:
        tgt_d = None
        if dtype is np.float32:
            tgt_d = torch.from_numpy(start[P.F_PD_PTARGET]).cuda()
            torch.cuda.synchronize()
            b.bind(P.F_PD_PTARGET, tgt_d.data_ptr())
        for f, a in start.items():
            if not (f == P.F_PD_PTARGET and tgt_d is not None):
                b.set(f, a)
        b.configure_actions(cols, delay_max=D, dtype=dtype, seed=cases.SEED)
        assert b.action_dim() == (ncols, D, 3 * ncols, (D + 3) * ncols) and b.action_launches() == 0
        act_d = torch.zeros((cases.NENV, cases.ACT_STRIDE), dtype=torch.float32, device="cuda")
        inp_d = torch.zeros((cases.NENV, cases.INPUT_STRIDE), dtype=torch.float32, device="cuda")
        rows_d = torch.full((cases.NENV, 3 * ncols + pad), FILL, dtype=tdtype, device="cuda")
        delay_d = torch.tensor(cases.DELAYS, dtype=torch.int32, device="cuda")
        b.bind_actions(act_d.data_ptr(), cases.ACT_STRIDE, torch.float32)
        b.bind_action_input(inp_d.data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
        b.bind_action_rows(rows_d.data_ptr(), 3 * ncols + pad)
        b.bind_action_delay(delay_d.data_ptr())
        st = torch.cuda.Stream()
        for k, ((act, inp), (env0, n, reset)) in enumerate(zip(calls, cases.SCHEDULE)):
            act_d.copy_(torch.from_numpy(act))
            inp_d.copy_(torch.from_numpy(inp))
            reset_d = None if reset is None else torch.tensor(reset, dtype=torch.int32, device="cuda")
            fence(b)
            b.act(env0, n, reset_ptr=None if reset_d is None else reset_d.data_ptr(), stream=st.cuda_stream)
            fence(b)
            rows, (state, counts) = b.action_rows(), b.action_state()
            assert rows.dtype == dtype and oc.same_bits(rows, want[k][0]), k
            assert oc.same_bits(state, want[k][1]) and np.array_equal(counts, want[k][2]), k
            for f in cases.DEST_FIELDS:
                assert oc.same_bits(b.get(f), want[k][3][f]), (k, f)
            raw = rows_d.cpu().numpy()
            assert oc.same_bits(raw[:, : 3 * ncols].reshape(rows.shape), rows) and np.all(raw[:, 3 * ncols:] == dtype(FILL))
        if tgt_d is not None:
            assert oc.same_bits(tgt_d.cpu().numpy(), want[-1][3][P.F_PD_PTARGET])
        assert b.action_launches() == len(cases.SCHEDULE)
        assert oc.same_bits(b.action_rows(1, 3), want[-1][0][1:4])
        # what no column names of a destination field is what it was
        assert np.array_equal(b.get(P.F_XFRC_APPLIED)[:, :-1], start[P.F_XFRC_APPLIED][:, :-1])
    finally:
        b.close()


def loop_columns():
    """Ten columns into the PD's position targets on a pose from the input: clipped, noisy, delayed, low-passed."""
    return [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, noise=0.02, smooth=0.5, bfield=P.ACT_INPUT, bindex=j, scale=0.3,
                      out_lo=float(bench.PD_OFFSET[j]) - 0.5, out_hi=float(bench.PD_OFFSET[j]) + 0.5) for j in range(10)]


def snapshot(b, episodes=False):
    out = {f: b.get(f).tobytes() for f in STATE_FIELDS}
    w, info = b.warnings()
    out["warn"], out["info"], out["drive"] = w.tobytes(), info.tobytes(), drive_bytes(b)
    if episodes:
        out["episodes"] = b"".join(a.tobytes() for a in b.episodes())
    return out


def test_the_step_reads_what_act_wrote(cassie):
    """Two batches of 8 envs in DRIVE_PD_SAFE, two ranges on two streams, 4 policy steps of 50 substeps.  The first calls act from an
    action tensor in front of every step_range, on the range's stream; the second has the targets tests/actions_check.py computes on the
    host bound per step.  Every state field, the warning words, the solver statistics and the drive-level bytes are equal at the end."""
    import torch
    n, npol, D, seed = 8, 4, 2, 77
    rng = np.random.default_rng(3)
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * np.arange(n)
    acts = rng.uniform(-1.3, 1.3, (npol, n, 10)).astype(np.float32)
    pose = (bench.PD_OFFSET + rng.uniform(-0.05, 0.05, (npol, n, 10))).astype(np.float32)
    delays = np.array([0, 1, 2, 5, 1, 0, 2, 1], dtype=np.int32)
    cols, ranges = loop_columns(), [(0, 4), (4, 4)]
    # the targets of every policy step on the host
    ref, held, tg = ac.Actions(cols, n, D, np.float32, seed, delay=delays), {P.F_PD_PTARGET: np.zeros((n, 10))}, []
    for p in range(npol):
        held[P.ACT_INPUT] = pose[p]
        for e0, cnt in ranges:
            ref.act(acts[p], held, e0, cnt)
        tg.append(held[P.F_PD_PTARGET].copy())
    tg = np.array(tg)
    assert np.abs(tg - bench.PD_OFFSET).max() <= 0.5 + 1e-12 and np.abs(tg[1:] - tg[:-1]).max() > 0.05
    acts_d, pose_d, tgd, delay_d = torch.from_numpy(acts).cuda(), torch.from_numpy(pose).cuda(), torch.from_numpy(tg).cuda(), torch.from_numpy(delays).cuda()

    def run(acting):
        b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
        try:
            if acting:
                b.configure_actions(cols, delay_max=D, dtype=np.float32, seed=seed)
                b.bind_action_delay(delay_d.data_ptr())
            fence(b)
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for p in range(npol):
                if acting:
                    b.bind_actions(acts_d[p].data_ptr(), 10, torch.float32)
                    b.bind_action_input(pose_d[p].data_ptr(), 10, 10, torch.float32)
                else:
                    b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
                for (e0, cnt), st in zip(ranges, streams):
                    if acting:
                        b.act(e0, cnt, stream=st.cuda_stream)
                    b.step_range(e0, cnt, 50, st.cuda_stream)
            fence(b)
            out = snapshot(b)
            if acting:
                assert b.action_launches() == 2 * npol and list(b.action_state()[1]) == [npol] * n
                assert oc.same_bits(b.action_rows(), ref.rows) and oc.same_bits(b.action_state()[0], ref.state)
            return out
        finally:
            b.close()

    want, got = run(False), run(True)
    for key in want:
        assert got[key] == want[key], key
    assert got[P.F_PD_PTARGET] == tg[-1].tobytes()


def test_nothing_else_is_touched(cassie):
    """Around one act of the whole batch in the middle of a loop, every field, the warning words, the solver statistics, the drive-level
    state and the episode arrays are byte for byte what they were -- except the destination elements the columns name."""
    import torch
    n = 8
    rng = np.random.default_rng(5)
    cols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, offset=float(bench.PD_OFFSET[j]), scale=0.2, smooth=0.5) for j in range(5)]
    cols += [P.act_col(P.F_XFRC_APPLIED, 6 * cassie.pod.nbody - 1, scale=0.5), P.act_col(noise=0.1)]
    acts_d = torch.from_numpy(rng.uniform(-1.0, 1.0, (3, n, 7)).astype(np.float32)).cuda()
    bq, bv = bank_states(cassie, 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
        b.set(P.F_XFRC_APPLIED, np.zeros((n, 6 * cassie.pod.nbody)))
        b.enable_episodes(max_steps=2, min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.configure_actions(cols, delay_max=1, dtype=np.float64, seed=1)
        for p in range(2):
            b.bind_actions(acts_d[p].data_ptr(), 7, torch.float32)
            b.act()
            b.step(50)
            b.end_episodes()
        fence(b)
        before = snapshot(b, episodes=True)
        b.bind_actions(acts_d[2].data_ptr(), 7, torch.float32)
        b.act(reset_ptr=b.episode_ptr(P.EP_DONE))
        fence(b)
        after = snapshot(b, episodes=True)
        named = {P.F_PD_PTARGET: np.arange(5), P.F_XFRC_APPLIED: np.array([6 * cassie.pod.nbody - 1])}
        for key in before:
            if key not in named:
                assert after[key] == before[key], key
                continue
            was, now = (np.frombuffer(s[key]).reshape(n, -1) for s in (before, after))
            rest = np.setdiff1d(np.arange(was.shape[1]), named[key])
            assert was[:, rest].tobytes() == now[:, rest].tobytes() and not (was[:, named[key]] == now[:, named[key]]).any(), key
    finally:
        b.close()


def test_reset_from_the_done_words(cassie):
    """Five envs, two of them put below the height rule: end_episodes ends and restarts those two, and an act handed the EP_DONE words
    starts them afresh -- PREV == NOW, every slot of the line the same, f == z -- while the other three shift.  Then a sub-range with the
    words' pointer offset."""
    import torch
    n, D = 5, 2
    rng = np.random.default_rng(9)
    cols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, noise=0.05, smooth=0.5 if j % 2 else 1.0, offset=0.1 * j, scale=0.5) for j in range(6)] + [P.act_col(smooth=0.25)]
    acts = rng.uniform(-1.2, 1.2, (4, n, 7)).astype(np.float32)
    acts_d, delay_d = torch.from_numpy(acts).cuda(), torch.tensor([0, 1, 2, 2, 1], dtype=torch.int32, device="cuda")
    bq, bv = bank_states(cassie, 3)
    b = Batch(cassie, n)
    try:
        q = np.tile(cassie.qpos_init(), (n, 1))
        b.set(P.F_QPOS, q)
        b.enable_episodes(min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.configure_actions(cols, delay_max=D, dtype=np.float64, seed=9)
        b.bind_action_delay(delay_d.data_ptr())
        ref, held = ac.Actions(cols, n, D, np.float64, 9, delay=[0, 1, 2, 2, 1]), {P.F_PD_PTARGET: np.zeros((n, cassie.pod.nu))}
        for k in range(2):
            b.bind_actions(acts_d[k].data_ptr(), 7, torch.float32)
            b.act()
            ref.act(acts[k], held)
        q[[1, 3], 2] = 0.5
        b.set(P.F_QPOS, q)
        b.end_episodes()
        b.bind_actions(acts_d[2].data_ptr(), 7, torch.float32)
        b.act(reset_ptr=b.episode_ptr(P.EP_DONE))
        done = b.episodes()[0]
        assert list(done) == [0, 1, 0, 1, 0]
        ref.act(acts[2], held, reset=done)
        rows, (state, counts) = b.action_rows(), b.action_state()
        assert oc.same_bits(rows, ref.rows) and oc.same_bits(state, ref.state) and list(counts) == [3] * n
        assert oc.same_bits(b.get(P.F_PD_PTARGET), held[P.F_PD_PTARGET])
        for e in (1, 3):
            assert np.array_equal(rows[e, P.ACT_PREV], rows[e, P.ACT_NOW]) and all(np.array_equal(state[e, h], state[e, 0]) for h in range(1, D + 2))
        for e in (0, 2, 4):
            assert not np.array_equal(rows[e, P.ACT_PREV], rows[e, P.ACT_NOW]) and not np.array_equal(state[e, 1], state[e, 0])
            assert np.array_equal(rows[e, P.ACT_PREV], acts[1][e].astype(np.float64).clip([c[4] for c in cols], [c[5] for c in cols]))
        # a slice of the words for a sub-range: entry i stands for env env0 + i
        b.bind_actions(acts_d[3].data_ptr(), 7, torch.float32)
        b.act(1, 2, reset_ptr=b.episode_ptr(P.EP_DONE) + 4)
        ref.act(acts[3], held, 1, 2, reset=done[1:3])
        rows, (state, counts) = b.action_rows(), b.action_state()
        assert oc.same_bits(rows, ref.rows) and oc.same_bits(state, ref.state) and list(counts) == [3, 4, 4, 3, 3]
        assert np.array_equal(rows[1, P.ACT_PREV], rows[1, P.ACT_NOW]) and not np.array_equal(rows[2, P.ACT_PREV], rows[2, P.ACT_NOW])
    finally:
        b.close()


def test_resume_from_the_downloaded_state(cassie, calls):
    """A second batch given action_state() of the first after three calls makes what the first makes on the fourth."""
    import torch
    cols, start = cases.columns_of(cassie.pod), cases.start_fields(cassie)
    acts_d = [torch.from_numpy(c[0]).cuda() for c in calls[:4]]
    inps_d = [torch.from_numpy(c[1]).cuda() for c in calls[:4]]
    delay_d = torch.tensor(cases.DELAYS, dtype=torch.int32, device="cuda")
    a, c = Batch(cassie, cases.NENV), Batch(cassie, cases.NENV)
    try:
        for b in (a, c):
            b.set(P.F_QPOS, start[P.F_QPOS])
            b.configure_actions(cols, delay_max=cases.DELAY_MAX, dtype=np.float64, seed=cases.SEED)
            b.bind_action_delay(delay_d.data_ptr())

        def call(b, k):
            b.bind_actions(acts_d[k].data_ptr(), cases.ACT_STRIDE, torch.float32)
            b.bind_action_input(inps_d[k].data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
            b.act()

        for k in range(3):
            call(a, k)
        state, counts = a.action_state()
        assert list(counts) == [3] * cases.NENV and not oc.same_bits(c.action_state()[0], state)
        c.set_action_state(state, counts)
        call(a, 3)
        call(c, 3)
        want = cases.reference(cols, calls[:4], np.float64, start, schedule=((0, cases.NENV, None),) * 4)[3]
        for b in (a, c):
            assert oc.same_bits(b.action_rows(), want[0]) and oc.same_bits(b.action_state()[0], want[1]) and np.array_equal(b.action_state()[1], want[2])
            assert oc.same_bits(b.get(P.F_PD_DTARGET), a.get(P.F_PD_DTARGET)) and oc.same_bits(b.get(P.F_PD_TORQUE), a.get(P.F_PD_TORQUE))
    finally:
        a.close()
        c.close()


def test_the_row_feeds_the_observation_and_the_reward(cassie):
    """One float32 input tensor [n][commands | 3 ncols] with the action rows bound as its column block: an observation term copies the
    PREV block, a reward term takes NOW - PREV (the action rate) through tfield.  After act -> step -> reward -> end_episodes -> observe
    for two policy steps, both are what tests/obs_check.py and tests/rewards_check.py make of tests/actions_check.py's rows."""
    import torch
    n, ncols, ncmd, seed = 6, 10, 4, 21
    W = ncmd + 3 * ncols
    rng = np.random.default_rng(13)
    cols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, noise=0.02, smooth=0.5, offset=float(bench.PD_OFFSET[j]), scale=0.2) for j in range(ncols)]
    now, prev = ncmd + P.ACT_NOW * ncols, ncmd + P.ACT_PREV * ncols
    oterms = [P.obs_copy(P.F_QPOS, 7, 4), P.obs_copy(P.OBS_INPUT, 0, ncmd), P.obs_copy(P.OBS_INPUT, prev, ncols, scale=2.0)]
    rterms = [P.rew_vec(P.F_QVEL, 0, 3, shape=P.REW_EXP, k=2.0, weight=0.5), P.rew_vec(P.REW_INPUT, now, ncols, tfield=P.REW_INPUT, tindex=prev, weight=-0.1)]
    acts = rng.uniform(-1.2, 1.2, (2, n, ncols)).astype(np.float32)
    cmd = rng.uniform(-1.0, 1.0, (n, ncmd)).astype(np.float32)
    acts_d = torch.from_numpy(acts).cuda()
    inp_d = torch.zeros((n, W), dtype=torch.float32, device="cuda")
    inp_d[:, :ncmd] = torch.from_numpy(cmd).cuda()
    bq, bv = bank_states(cassie, 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.enable_episodes(min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.configure_actions(cols, delay_max=1, dtype=np.float32, seed=seed)
        b.bind_action_rows(inp_d.data_ptr() + 4 * ncmd, W)
        b.configure_obs(oterms, history=2, dtype=np.float32, seed=seed)
        b.bind_obs_input(inp_d.data_ptr(), W, W, torch.float32)
        b.configure_rewards(rterms, dtype=np.float32)
        b.bind_reward_input(inp_d.data_ptr(), W, W, torch.float32)
        fence(b)
        aref, held = ac.Actions(cols, n, 1, np.float32, seed), {P.F_PD_PTARGET: np.zeros((n, cassie.pod.nu))}
        oref, rref = oc.Obs(oterms, n, 2, np.float32, seed), rc.Rewards(rterms, n, np.float32)
        st = torch.cuda.Stream()
        done_ptr = b.episode_ptr(P.EP_DONE)
        for p in range(2):
            b.bind_actions(acts_d[p].data_ptr(), ncols, torch.float32)
            b.act(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.step_range(0, n, 10, st.cuda_stream)
            b.reward(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.end_episodes(stream=st.cuda_stream)
            b.observe(refill_ptr=done_ptr, stream=st.cuda_stream)
            fence(b)
            done = b.episodes()[0]
            assert not done.any()          # (nobody fell in 10 substeps: the state the reward saw is the one the observation sees)
            aref.act(acts[p], held)
            inp = np.concatenate([cmd, aref.rows.reshape(n, 3 * ncols)], axis=1)
            assert oc.same_bits(inp_d.cpu().numpy(), inp) and oc.same_bits(b.action_rows(), aref.rows), p
            assert oc.same_bits(b.get(P.F_PD_PTARGET), held[P.F_PD_PTARGET]), p
            fields = {P.F_QPOS: b.get(P.F_QPOS), P.F_QVEL: b.get(P.F_QVEL), P.OBS_INPUT: inp}
            assert oc.same_bits(b.rewards(), rref.reward(fields)), p
            assert oc.same_bits(b.obs(), oref.observe(fields)), p
        # the second step's action rate is no zero: PREV is the first step's NOW
        assert oc.same_bits(aref.rows[:, P.ACT_PREV], np.clip(acts[0], -1.0, 1.0)) and np.abs(aref.rows[:, P.ACT_NOW] - aref.rows[:, P.ACT_PREV]).max() > 0.1
        assert oc.same_bits(b.obs()[:, 0, 4 + ncmd:], (np.float64(2.0) * aref.rows[:, P.ACT_PREV].astype(np.float64)).astype(np.float32))
    finally:
        b.close()


def test_counters_bindings_and_refusals(cassie):
    import torch
    pod = cassie.pod
    b = Batch(cassie, 4)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            b.act()
        with pytest.raises(RuntimeError, match="not configured"):
            b.action_dim()
        with pytest.raises(ValueError, match="does not hold yet"):
            b.configure_actions([P.act_col(bfield=P.F_HEIGHT_SCAN)])
        with pytest.raises(ValueError, match="PHYS_F_DEPTH"):
            b.configure_actions([P.act_col(bfield=P.F_DEPTH)])
        with pytest.raises(ValueError, match="command field"):
            b.configure_actions([P.act_col(P.F_QPOS, 0)])
        with pytest.raises(ValueError, match="dindex lies beyond"):
            b.configure_actions([P.act_col(P.F_CTRL, pod.nu)])
        with pytest.raises(ValueError, match="same destination element"):
            b.configure_actions([P.act_col(P.F_CTRL, 1), P.act_col(P.F_CTRL, 1)])
        with pytest.raises(ValueError, match="smooth"):
            b.configure_actions([P.act_col(smooth=0.0)])
        with pytest.raises(ValueError, match="delay depth"):
            b.configure_actions([P.act_col()], delay_max=P.ACT_MAXDELAY + 1)
        with pytest.raises(ValueError, match="dtype"):
            b.configure_actions([P.act_col()], dtype=np.float16)
        with pytest.raises(ValueError, match="not configured"):
            b.bind_actions(1 << 20, 4)
        c = [P.act_col(P.F_CTRL, j, lo=-1.0, hi=1.0) for j in range(3)] + [P.act_col(bfield=P.ACT_INPUT, bindex=4, scale=2.0)]
        b.configure_actions(c, delay_max=1, dtype=np.float32)
        assert b.action_dim() == (4, 1, 12, 16) and b.action_launches() == 0
        with pytest.raises(RuntimeError, match="no actions bound"):
            b.act()
        act = torch.full((4, 6), 3.0, dtype=torch.float64, device="cuda")
        with pytest.raises(ValueError, match="at least the columns"):
            b.bind_actions(act.data_ptr(), 3, torch.float64)
        with pytest.raises(ValueError, match="actions' dtype"):
            b.bind_actions(act.data_ptr(), 6, torch.int32)
        b.bind_actions(act.data_ptr(), 6, torch.float64)
        with pytest.raises(RuntimeError, match="no input bound"):
            b.act()
        inp = torch.ones((4, 5), dtype=torch.float64, device="cuda")
        b.bind_action_input(inp.data_ptr(), 4, 5, torch.float64)
        with pytest.raises(RuntimeError, match="shorter"):
            b.act()
        b.bind_action_input(inp.data_ptr(), 5, 5, torch.float64)
        with pytest.raises(RuntimeError, match="out of bounds"):
            b.act(2, 3)
        with pytest.raises(ValueError, match="row stride"):
            b.bind_action_rows(inp.data_ptr(), 11)
        b.act()
        b.act(1, 2)
        state, counts = b.action_state()
        assert b.action_launches() == 2 and list(counts) == [1, 2, 2, 1] and state.shape == (4, 4, 4)
        rows = b.action_rows()
        assert rows.dtype == np.float32 and np.all(rows[:, :, :3] == 1.0) and np.all(rows[:, :, 3] == 3.0)
        assert np.all(b.get(P.F_CTRL)[:, :3] == 1.0) and np.all(b.get(P.F_CTRL)[:, 3:] == 0.0)
        # configuring again zeroes the state and the counts and drops the bindings; no columns releases everything
        b.configure_actions(c, delay_max=0)
        assert list(b.action_state()[1]) == [0] * 4 and not b.action_state()[0].any() and b.action_dim() == (4, 0, 12, 12)
        with pytest.raises(RuntimeError, match="no actions bound"):
            b.act()
        b.configure_actions([])
        with pytest.raises(RuntimeError, match="not configured"):
            b.act()
        with pytest.raises(RuntimeError, match="not configured"):
            b.action_rows()
    finally:
        b.close()
