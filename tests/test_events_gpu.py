"""Event rows (phys_batch_events) on the device against the definition restated in numpy and Python integers (tests/events_check.py),
BIT FOR BIT: every arithmetic step of a column is one individually rounded fp64 operation in the kernel and every comparison takes the
branch the definition states, so the device, the wave emulator (tests/test_events.py) and numpy must agree on every bit.  Also: two
ranges on two streams, workgroups that walk a long range, that a call changes nothing of the batch but its own outputs, a resumed run,
and the whole policy step with physics -- contact phases of real feet, episodes ended through the done words, the air time paid through
the reward."""
import numpy as np
import pytest

import events_cases as cases
import events_check as ec
from cassie_amd import Batch
from cassie_amd import phys as P
from obs_check import same_bits
from test_actions_gpu import fence, snapshot
from test_episodes_gpu import bank_states, make

pytestmark = pytest.mark.gpu
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


def outputs(b):
    return (b.event_rows(), b.event_flags()) + b.event_state()


def assert_same(got, want, what):
    for a, w, name in zip(got, want, NAMES):
        assert a.dtype == w.dtype and a.shape == w.shape, (what, name)
        if not same_bits(a, w):
            at = np.argwhere(~((a == w) | (np.isnan(a) & np.isnan(w))))[:6]
            raise AssertionError((what, name, [(tuple(int(i) for i in k), a[tuple(k)], w[tuple(k)]) for k in at]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_definition_on_the_device(cassie, cols, calls, dtype):
    """The emulator's case on the device: 64 columns over fourteen calls on 70 envs.  F_BODY_CFRC is uploaded, the float32 input is a
    torch tensor with a row stride, the rows are bound to a torch tensor with padding that stays, the done words to a torch int32 tensor,
    the reset words are a torch tensor and the call runs on a caller's stream.  After every call the rows, the done words, both state
    slots, the words and the counts are the reference's."""
    import torch
    want = cases.reference(cols, calls, dtype)
    nc, tdtype = cases.NCOLS, torch.float32 if dtype is np.float32 else torch.float64
    b = Batch(cassie, cases.NENV)
    try:
        b.configure_events(cols, dtype=dtype, done_mask=cases.DONE_MASK)
        assert b.event_dim() == nc and b.event_launches() == 0
        inp_d = torch.zeros((cases.NENV, cases.INPUT_STRIDE), dtype=torch.float32, device="cuda")
        rows_d = torch.full((cases.NENV, nc + cases.ROW_PAD), FILL, dtype=tdtype, device="cuda")
        flags_d = torch.full((cases.NENV,), 9, dtype=torch.int32, device="cuda")
        b.bind_event_input(inp_d.data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
        b.bind_event_rows(rows_d.data_ptr(), nc + cases.ROW_PAD)
        b.bind_event_flags(flags_d.data_ptr())
        assert b.event_flags_ptr() == flags_d.data_ptr() and b.event_flags_ptr(3) == flags_d.data_ptr() + 12
        st = torch.cuda.Stream()
        seen = np.zeros(cases.NENV, dtype=bool)
        for k, ((cfrc, inp, reset), (env0, n)) in enumerate(zip(calls, cases.RANGES)):
            b.set(P.F_BODY_CFRC, cfrc)
            inp_d.copy_(torch.from_numpy(inp))
            reset_d = None if reset is None else torch.from_numpy(reset).cuda()
            fence(b)
            b.events(env0, n, reset_ptr=None if reset_d is None else reset_d.data_ptr(), stream=st.cuda_stream)
            fence(b)
            assert_same(outputs(b), want[k], k)
            seen[env0:env0 + n] = True
            raw, flags = rows_d.cpu().numpy(), flags_d.cpu().numpy()
            assert same_bits(raw[:, :nc].copy(), want[k][0]) and np.all(raw[:, nc:] == dtype(FILL))
            assert np.array_equal(flags[seen], want[k][1][seen]) and np.all(flags[~seen] == 9)
        assert b.event_launches() == len(cases.RANGES)
        assert same_bits(b.event_rows(3, 5), want[-1][0][3:8])
    finally:
        b.close()


def test_two_ranges_on_two_streams_and_a_resumed_run(cassie, cols, calls):
    """(0, 33) and (33, 37) on two streams give one call's bits; and a second batch given event_state() of the first after four calls
    makes what the first makes from the fifth on."""
    import torch
    whole = ((0, cases.NENV),) * 7
    want = cases.reference(cols, calls[:7], np.float64, ranges=whole)
    a, c = Batch(cassie, cases.NENV), Batch(cassie, cases.NENV)
    try:
        inp_d = torch.zeros((cases.NENV, cases.INPUT_STRIDE), dtype=torch.float32, device="cuda")
        for b in (a, c):
            b.configure_events(cols, dtype=np.float64, done_mask=cases.DONE_MASK)
            b.bind_event_input(inp_d.data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for k, (cfrc, inp, reset) in enumerate(calls[:7]):
            if k == 4:
                c.set_event_state(*a.event_state())
            for b in (a, c) if k >= 4 else (a,):
                b.set(P.F_BODY_CFRC, cfrc)
            inp_d.copy_(torch.from_numpy(inp))
            reset_d = None if reset is None else torch.from_numpy(reset).cuda()
            fence(a)
            for (e0, cnt), st in zip(((0, 33), (33, 37)), streams):
                a.events(e0, cnt, reset_ptr=None if reset_d is None else reset_d.data_ptr() + 4 * e0, stream=st.cuda_stream)
            if k >= 4:
                c.events(reset_ptr=None if reset_d is None else reset_d.data_ptr())
            fence(a)
            fence(c)
            assert_same(outputs(a), want[k], ("two ranges", k))
            if k >= 4:
                assert_same(outputs(c), want[k], ("resumed", k))
        assert a.event_launches() == 14 and c.event_launches() == 3
    finally:
        a.close()
        c.close()


def test_workgroups_walk_a_long_range(cassie):
    """64 * EVENT_GRID + 65 envs and three columns from the input: every workgroup takes a second block of 64 envs, the first a third of
    one env; the rows, the state and the done words are the reference's over three calls, the last over an odd sub-range."""
    import torch
    n = 64 * 64 + 65
    cols = [P.ev_measure(P.EV_INPUT, 0), P.ev_level(0, 0.25, -0.25), P.ev_accum(0, P.EV_SUM, gate=1)]
    rng = np.random.default_rng(3)
    ref = ec.Events(cols, n, np.float32, 0b10)
    b = Batch(cassie, n)
    try:
        b.configure_events(cols, dtype=np.float32, done_mask=0b10)
        inp_d = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        b.bind_event_input(inp_d.data_ptr(), 1, 2, torch.float64)
        for env0, cnt in ((0, n), (0, n), (4095, 66)):
            inp = rng.uniform(-1.0, 1.0, (n, 2))
            inp_d.copy_(torch.from_numpy(inp))
            fence(b)
            b.events(env0, cnt)
            fence(b)
            ref.events({P.EV_INPUT: inp}, env0, cnt)
            assert_same(outputs(b), (ref.rows, ref.flags, ref.state, ref.words, ref.counts), (env0, cnt))
        assert 0 < ref.flags.sum() < n and list(ref.counts[[0, 4094, 4095, n - 1]]) == [2, 2, 3, 3]
    finally:
        b.close()


def loop_columns(lf, rf, pel, dt, k_off):
    """The biped chain of the loop on F_BODY_CFRC: contact flags of two feet, the air time paid at touchdown, the peak force of a
    stance, and two done columns: both feet off for k_off calls, the pelvis took a contact force."""
    cfrc = lambda body: P.ev_measure(P.F_BODY_CFRC, 3 * body, 3, norm=P.EV_SUMSQ, root=True)
    return [cfrc(lf), cfrc(rf), cfrc(pel), P.ev_level(0, 20.0, 5.0), P.ev_level(1, 20.0, 5.0), P.ev_timer(3, dt, 0), P.ev_edge(3, P.EV_RISING),
            P.ev_edge(3, P.EV_FALLING), P.ev_latch(5, 6, lag=1), P.ev_logic([3, 4], P.EV_NONE), P.ev_timer(9, dt, 1), P.ev_level(10, k_off * dt),
            P.ev_level(2, 1.0), P.ev_accum(0, P.EV_MAX, clear=6)]


CL, TDL, LOL, AIRL, FLY, PEL = 3, 6, 7, 8, 11, 12


def test_the_whole_policy_step_with_physics(cassie, ids):
    """8 envs in DRIVE_PD_SAFE, 40 policy steps of 50 substeps in the order act, step, events, reward, end_episodes(force = the done
    words), task, observe on one stream.  ONE float32 input tensor [n][push | pose | event row] is bound by all five stages.  The task
    stage pushes the pelvis up through xfrc_applied with three to four times the robot's weight for two calls of eight in about half of
    the envs and periods (checked on the CPU oracle beforehand: such a push lifts both feet off the ground for 0 .. 11 calls), so feet
    leave the ground and come back, and a done column fires on "both feet off for 6 calls".  After every step the rows, the done words
    and the state are tests/events_check.py's on the F_BODY_CFRC the device held at the call; EP_REASON carries DONE_FORCED exactly
    where the restated done words are 1; and a reward term of value 1 gated by the air-time column is weight * column."""
    import torch
    lf, rf, pel = ids
    n, npol, nsub, seed, na, k_off, weight = 8, 40, 50, 31, 10, 6, 0.7
    dt = nsub * 0.0005
    ecols = loop_columns(lf, rf, pel, dt, k_off)
    ne = len(ecols)
    POSE, EV0 = 1, 1 + na
    W = EV0 + ne
    tcols = [P.task_sample(1200.0, 300.0, 8, 8, hold=2, p_rest=0.5, dfield=P.F_XFRC_APPLIED, dindex=6 * pel + 2)]
    acols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, bfield=P.ACT_INPUT, bindex=POSE + j, scale=0.02) for j in range(na)]
    rterms = [P.rew_vec(P.REW_INPUT, POSE, 1, tfield=P.REW_INPUT, tindex=POSE, shape=P.REW_EXP, k=1.0, weight=weight, gate=(P.REW_INPUT, EV0 + AIRL))]
    oterms = [P.obs_copy(P.F_QPOS, 7, 4), P.obs_copy(P.OBS_INPUT, EV0, ne)]
    rng = np.random.default_rng(5)
    acts_d = torch.from_numpy(rng.uniform(-1.0, 1.0, (npol, n, na)).astype(np.float32)).cuda()
    inp0 = np.zeros((n, W), dtype=np.float32)
    inp0[:, POSE:POSE + na] = bench_pose()
    inp_d = torch.from_numpy(inp0).cuda()
    bq, bv = bank_states(cassie, 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.set(P.F_XFRC_APPLIED, np.zeros((n, 6 * cassie.pod.nbody)))
        b.enable_episodes(min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.configure_task(tcols, dtype=np.float32, seed=seed)
        b.bind_task_rows(inp_d.data_ptr(), W)
        b.configure_actions(acols, delay_max=1, dtype=np.float32, seed=seed)
        b.bind_action_input(inp_d.data_ptr(), W, W, torch.float32)
        b.configure_events(ecols, dtype=np.float32, done_mask=[FLY, PEL])
        b.bind_event_rows(inp_d.data_ptr() + 4 * EV0, W)
        b.configure_rewards(rterms, dtype=np.float32)
        b.bind_reward_input(inp_d.data_ptr(), W, W, torch.float32)
        b.bind_reward_terms(own=True)
        b.configure_obs(oterms, history=1, dtype=np.float32, seed=seed)
        b.bind_obs_input(inp_d.data_ptr(), W, W, torch.float32)
        ref = ec.Events(ecols, n, np.float32, (1 << FLY) | (1 << PEL))
        st = torch.cuda.Stream()
        done_ptr = b.episode_ptr(P.EP_DONE)
        b.task(stream=st.cuda_stream)                      # (the push of the first policy step, as a reset of the whole batch makes it)
        fence(b)
        done = np.zeros(n, dtype=np.int32)
        hist, forced, pushed = [], np.zeros(n, dtype=int), np.zeros(n, dtype=bool)
        for p in range(npol):
            pushed |= b.get(P.F_XFRC_APPLIED)[:, 6 * pel + 2] > 900.0
            b.bind_actions(acts_d[p].data_ptr(), na, torch.float32)
            b.act(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.step_range(0, n, nsub, st.cuda_stream)
            fence(b)
            cfrc = b.get(P.F_BODY_CFRC)                    # (what the device holds at the call)
            b.events(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.reward(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.end_episodes(force_ptr=b.event_flags_ptr(), stream=st.cuda_stream)
            fence(b)
            ref.events({P.F_BODY_CFRC: cfrc}, reset=done)
            assert_same(outputs(b), (ref.rows, ref.flags, ref.state, ref.words, ref.counts), p)
            assert same_bits(inp_d.cpu().numpy()[:, EV0:].copy(), ref.rows), p
            done, reason = (a.astype(np.int32) for a in b.episodes()[:2])
            assert np.array_equal((reason & P.DONE_FORCED) != 0, ref.flags == 1) and np.array_equal(done != 0, reason != 0), p
            want = (np.float64(weight) * ref.rows[:, AIRL].astype(np.float64)).astype(np.float32)
            assert same_bits(b.reward_terms()[:, 0].copy(), want), p
            hist.append(ref.rows.copy())
            forced += ref.flags
            b.task(reset_ptr=done_ptr, stream=st.cuda_stream)
            b.observe(refill_ptr=done_ptr, stream=st.cuda_stream)
            fence(b)
            assert same_bits(b.obs()[:, 0, 4:].copy(), ref.rows), p      # (the policy sees this step's event row)
        # the test is not vacuous: on the recorded sources feet left the ground and came back, air time was paid, an episode was force-ended
        hist = np.array(hist)
        both = (hist[:, :, TDL].sum(0) > 0) & (hist[:, :, LOL].sum(0) > 0)
        assert pushed.sum() >= 2 and both.sum() >= 2, (pushed, both)
        assert (hist[:, :, AIRL] > 0).any() and (forced > 0).sum() >= 1 and (hist[:, :, FLY] == 1).any()
        assert b.event_launches() == npol and list(ref.counts) == [npol] * n
    finally:
        b.close()


def bench_pose():
    import bench
    return bench.PD_OFFSET.astype(np.float32)


def test_a_call_changes_nothing_but_its_outputs(cassie, ids):
    """Two batches of 8 envs in DRIVE_PD_SAFE run step_range(50 substeps) x 3 on two ranges and two streams with episodes that end;
    the second with events of the range behind every step launch.  Every state field, the warning words, the solver statistics, the
    drive-level bytes and the episode arrays are byte for byte those of the loop without the calls."""
    import torch
    import bench
    n, npol = 8, 3
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * np.arange(n)
    tgd = torch.from_numpy(bench.pd_targets(np.arange(n), npol)).cuda()
    bq, bv = bank_states(cassie, 3)
    ecols = loop_columns(*ids, 0.025, 2)

    def run(with_events):
        b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
        try:
            b.enable_episodes(max_steps=2, min_height=0.6)
            b.set_reset_bank(b.make_reset_bank(bq, bv))
            if with_events:
                b.configure_events(ecols, dtype=np.float64, done_mask=[FLY, PEL])
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for p in range(npol):
                b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
                for (e0, cnt), st in zip(((0, 4), (4, 4)), streams):
                    b.step_range(e0, cnt, 50, st.cuda_stream)
                    if with_events:
                        b.events(e0, cnt, reset_ptr=b.episode_ptr(P.EP_DONE) + 4 * e0, stream=st.cuda_stream)
                    b.end_episodes(e0, cnt, True, stream=st.cuda_stream)
                fence(b)
            out = snapshot(b, episodes=True)
            out["cfrc"] = b.get(P.F_BODY_CFRC).tobytes()
            if with_events:
                assert b.event_launches() == 2 * npol and list(b.event_state()[2]) == [npol] * n and (b.event_rows()[:, :2] > 0).any()
            return out
        finally:
            b.close()

    plain, evented = run(False), run(True)
    for key in plain:
        assert plain[key] == evented[key], key


def test_refusals_through_the_batch(cassie, ids):
    """The messages reach the caller with the entry point's name; releasing and configuring again work."""
    b = Batch(cassie, 4)
    try:
        with pytest.raises(RuntimeError, match="phys_batch_events: not configured"):
            b.events()
        with pytest.raises(ValueError, match="phys_batch_events_configure: a column's src, trig, clear and gate name columns with a lower index"):
            b.configure_events([P.ev_measure(P.F_QPOS, 0), P.ev_edge(1)])
        with pytest.raises(ValueError, match="phys_batch_events_configure: done_mask has a bit at or above ncols"):
            b.configure_events([P.ev_measure(P.F_QPOS, 0)], done_mask=2)
        b.configure_events([P.ev_measure(P.F_QPOS, 2, target=0.5), P.ev_level(0, 0.1)], dtype=np.float64, done_mask=[1])
        with pytest.raises(RuntimeError, match="phys_batch_events: env range out of bounds"):
            b.events(2, 3)
        with pytest.raises(ValueError, match="phys_batch_events_bind_rows: a row stride of at least the columns"):
            b.bind_event_rows(b.event_flags_ptr(), 1)
        q = np.tile(cassie.qpos_init(), (4, 1))
        q[2, 2] = 0.55
        b.set(P.F_QPOS, q)
        b.events()
        assert list(b.event_flags()) == [1, 1, 0, 1] and same_bits(b.event_rows()[:, 0].copy(), q[:, 2] - 0.5)
        b.configure_events([])
        with pytest.raises(RuntimeError, match="phys_batch_events: not configured"):
            b.events()
        with pytest.raises(RuntimeError):
            b.event_flags_ptr()
    finally:
        b.close()
