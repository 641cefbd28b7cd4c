"""Observation rows (phys_batch_obs) on the device against the definition restated in numpy and Python integers (tests/obs_check.py),
BIT FOR BIT: every step of a column's value -- the rotation's products and sums, the offset, the noise, the scale -- is one individually
rounded fp64 operation in the kernel (no fused multiply-add, nothing left to the compiler's contraction), the noise is integer
arithmetic, and the cast rounds to nearest even; so the device, the wave emulator (tests/test_obs.py) and numpy must agree on every bit,
where the ray and depth tests can only bound an error.  Also: the bindings, two ranges on two streams behind real step launches, the
refill from the episodes' done words, and that a call changes nothing of the batch but its own rows and counts."""
import numpy as np
import pytest

import bench
import obs_cases as cases
import obs_check as oc
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import bank_states, drive_bytes, make
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
    """The emulator's case on the device: seven terms, a frame of more than 64 columns, history 3 over five calls (fill, shift, a
    sub-range, a refill, shift) on states that change, the float32 input bound to a torch tensor with a row stride.  float32: the rows
    bound to a torch float32 tensor with a row stride, whose gaps stay; float64: the batch's own rows, downloaded."""
    import torch
    terms = cases.terms_of(cassie.pod)
    want = cases.reference(terms, states, dtype)
    ncols = len(oc.columns(terms)[0])
    row, pad = cases.HISTORY * ncols, 7
    b = Batch(cassie, cases.NENV)
    try:
        b.configure_obs(terms, history=cases.HISTORY, dtype=dtype, seed=cases.SEED)
        assert b.obs_dim() == (ncols, cases.HISTORY, row) and b.obs_layout() == oc.columns(terms)[1]
        inp = torch.zeros((cases.NENV, cases.INPUT_STRIDE), dtype=torch.float32, device="cuda")
        b.bind_obs_input(inp.data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
        rows_d = None
        if dtype is np.float32:
            rows_d = torch.full((cases.NENV, row + pad), FILL, dtype=torch.float32, device="cuda")
            b.bind_obs(rows_d.data_ptr(), row + pad)
        st = torch.cuda.Stream()
        for k, (state, (env0, n, refill)) in enumerate(zip(states, cases.SCHEDULE)):
            put(b, state)
            b.sync()
            inp.copy_(torch.from_numpy(state[P.OBS_INPUT]))
            refill_d = None if refill is None else torch.tensor(refill, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            b.observe(env0, n, refill_ptr=None if refill_d is None else refill_d.data_ptr(), stream=st.cuda_stream)
            b.sync()
            torch.cuda.synchronize()
            got = b.obs()
            assert got.dtype == dtype and oc.same_bits(got, want[k][0]), k
            assert np.array_equal(b.obs_frames(), want[k][1]), k
            if rows_d is not None:
                raw = rows_d.cpu().numpy()
                assert oc.same_bits(raw[:, :row].reshape(got.shape), got) and np.all(raw[:, row:] == np.float32(FILL))
        assert b.obs_launches() == len(cases.SCHEDULE)
        assert oc.same_bits(b.obs(1, 3), want[-1][0][1:4])
    finally:
        b.close()


def test_resume_from_downloaded_frames(cassie, states):
    """A second batch given the first one's frame counts draws what the first draws next."""
    terms = cases.terms_of(cassie.pod)
    import torch
    inp = torch.from_numpy(states[1][P.OBS_INPUT]).cuda()
    a, c = Batch(cassie, cases.NENV), Batch(cassie, cases.NENV)
    try:
        for b in (a, c):
            b.configure_obs(terms, history=1, dtype=np.float64, seed=cases.SEED)
            b.bind_obs_input(inp.data_ptr(), cases.INPUT_DIM, cases.INPUT_STRIDE, torch.float32)
            put(b, states[1])
        for _ in range(3):
            a.observe()
        assert list(a.obs_frames()) == [3] * cases.NENV
        c.set_obs_frames(a.obs_frames())
        a.observe()
        c.observe()
        ref = oc.Obs(terms, cases.NENV, 1, np.float64, cases.SEED)
        ref.frames[:] = 3
        assert oc.same_bits(a.obs(), c.obs()) and oc.same_bits(a.obs(), ref.observe(states[1]))
    finally:
        a.close()
        c.close()


@pytest.mark.parametrize("extras", ["plain", "episodes"])
def test_the_loop_is_not_disturbed(cassie, extras):
    """Two batches of 8 envs in DRIVE_PD_SAFE run step_range(50 substeps) x 4 on two ranges and two streams; the second with an
    observe of each range behind every step launch, on the range's stream (with episodes: behind end_episodes, refilled from the
    range's slice of EP_DONE).  Around one observe of the whole batch every field, the warning words, the solver statistics, the
    drive-level state and the episode arrays are byte for byte what they were; at the end of the loop -- stepping went on after the
    calls -- they are what the loop without the calls leaves.  The newest frame is the definition's on the state the loop ended in."""
    import torch
    n, npol, k = 8, 4, 4
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * np.arange(n)
    tgd = torch.from_numpy(bench.pd_targets(np.arange(n), npol)).cuda()
    pick_d = torch.from_numpy(np.random.default_rng(7).integers(0, k, (npol, n)).astype(np.int32)).cuda()
    bq, bv = bank_states(cassie, k)
    terms = [t for t in cases.terms_of(cassie.pod) if t[1] != P.OBS_INPUT] + [P.obs_copy(P.F_MEAS, 0, 4), P.obs_copy(P.F_TIME, 0, 1)]
    ranges = [(0, 4), (4, 4)]

    def snapshot(b):
        out = {f: b.get(f).tobytes() for f in STATE_FIELDS}
        w, info = b.warnings()
        out["warn"], out["info"], out["drive"] = w.tobytes(), info.tobytes(), drive_bytes(b)
        if extras == "episodes":
            out["episodes"] = b"".join(a.tobytes() for a in b.episodes())
        return out

    def run(observing):
        b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
        try:
            if extras == "episodes":
                b.enable_episodes(max_steps=2, min_height=0.6)
                bank_d = torch.from_numpy(b.make_reset_bank(bq, bv)).cuda()
                b.set_reset_bank(device_ptr=bank_d.data_ptr(), n=k)
            if observing:
                b.configure_obs(terms, history=2, dtype=np.float32, seed=5)
            b.sync()
            torch.cuda.synchronize()
            streams = [torch.cuda.Stream(), torch.cuda.Stream()]
            for p in range(npol):
                b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
                for (e0, cnt), st in zip(ranges, streams):
                    b.step_range(e0, cnt, 50, st.cuda_stream)
                    if extras == "episodes":
                        b.end_episodes(e0, cnt, True, pick_ptr=pick_d[p].data_ptr() + 4 * e0, stream=st.cuda_stream)
                    if observing:
                        refill = b.episode_ptr(P.EP_DONE) + 4 * e0 if extras == "episodes" else None
                        b.observe(e0, cnt, refill_ptr=refill, stream=st.cuda_stream)
                if observing and p == 1:
                    b.sync()
                    torch.cuda.synchronize()
                    before = snapshot(b)
                    b.observe()
                    b.sync()
                    torch.cuda.synchronize()
                    after = snapshot(b)
                    for key in before:
                        assert after[key] == before[key], key
            b.sync()
            torch.cuda.synchronize()
            out = snapshot(b)
            rows = None
            if observing:
                assert b.obs_launches() == 2 * npol + 1
                fields = {f: b.get(f) for f in (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA, P.F_MEAS, P.F_TIME)}
                done = b.episodes()[0] if extras == "episodes" else None
                rows = (b.obs(), b.obs_frames(), fields, done)
            return out, rows
        finally:
            b.close()

    want, _ = run(False)
    got, (rows, frames, fields, done) = run(True)
    for key in want:
        assert got[key] == want[key], key
    assert list(frames) == [npol + 1] * n
    ref = oc.Obs(terms, n, 2, np.float32, 5)
    ref.frames[:] = npol
    newest = ref.observe(fields, refill=np.ones(n, dtype=np.int32))[:, 0]
    assert oc.same_bits(rows[:, 0], newest) and np.abs(newest).max() > 0.1
    # an env whose episode ended at the last policy step had its history refilled; every other env's older frame is another one
    ended = np.zeros(n, dtype=bool) if done is None else done.astype(bool)
    assert extras != "episodes" or ended.any()
    for e in range(n):
        assert np.array_equal(rows[e, 1], rows[e, 0]) == bool(ended[e]), e


def test_refill_from_the_done_words(cassie, states):
    """Five envs, two of them put below the height rule: end_episodes ends and restarts those two, and an observe handed the EP_DONE
    words refills their histories from the restarted state while the other three shift."""
    import torch
    terms = [P.obs_copy(P.F_QPOS, 0, 7, noise=0.01), P.obs_rot_inv(P.OBS_CONST, 0, P.F_QPOS, 3, vec=(0.0, 0.0, -1.0)), P.obs_copy(P.F_QVEL, 0, 6)]
    bq, bv = bank_states(cassie, 3)
    b = Batch(cassie, 5)
    try:
        b.enable_episodes(min_height=0.6)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.configure_obs(terms, history=3, dtype=np.float64, seed=9)
        ref = oc.Obs(terms, 5, 3, np.float64, 9)
        for k in range(2):
            put(b, states[k])
            b.observe()
            ref.observe(states[k])
        low = states[2][P.F_QPOS].copy()
        assert low[:, 2].min() > 0.7
        low[[1, 3], 2] = 0.5
        b.set(P.F_QPOS, low)
        b.set(P.F_QVEL, states[2][P.F_QVEL])
        b.end_episodes()
        b.observe(refill_ptr=b.episode_ptr(P.EP_DONE))
        done = b.episodes()[0]
        assert list(done) == [0, 1, 0, 1, 0]
        now = {f: b.get(f) for f in (P.F_QPOS, P.F_QVEL)}
        assert now[P.F_QPOS][1, 2] > 0.7 and np.array_equal(now[P.F_QPOS][0], low[0])      # (restarted from the bank / left alone)
        want = ref.observe(now, refill=done)
        got = b.obs()
        assert oc.same_bits(got, want) and list(b.obs_frames()) == [3] * 5
        for e in (1, 3):
            assert np.array_equal(got[e, 0], got[e, 1]) and np.array_equal(got[e, 0], got[e, 2])
        for e in (0, 2, 4):
            assert not np.array_equal(got[e, 0], got[e, 1]) and not np.array_equal(got[e, 1], got[e, 2])
        # a slice of the words for a sub-range: entry i stands for env env0 + i
        b.observe(1, 2, refill_ptr=b.episode_ptr(P.EP_DONE) + 4)
        want = ref.observe(now, 1, 2, refill=done[1:3])
        assert oc.same_bits(b.obs(), want) and list(b.obs_frames()) == [3, 4, 4, 3, 3]
    finally:
        b.close()


def test_counters_bindings_and_refusals(cassie):
    import torch
    pod = cassie.pod
    b = Batch(cassie, 4)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            b.observe()
        with pytest.raises(RuntimeError, match="not configured"):
            b.obs_dim()
        with pytest.raises(ValueError, match="does not hold yet"):
            b.configure_obs([P.obs_copy(P.F_HEIGHT_SCAN, 0, 1)])
        with pytest.raises(ValueError, match="PHYS_F_DEPTH"):
            b.configure_obs([P.obs_copy(P.F_DEPTH, 0, 1)])
        with pytest.raises(ValueError, match="index \\+ count"):
            b.configure_obs([P.obs_copy(P.F_QPOS, pod.nq - 1, 2)])
        with pytest.raises(ValueError, match="dtype"):
            b.configure_obs([P.obs_copy(P.F_QPOS, 0, 2)], dtype=np.float16)
        t = [P.obs_copy(P.F_QPOS, 0, 3), P.obs_copy(P.OBS_INPUT, 2, 3)]
        b.configure_obs(t, history=2, dtype=np.float32)
        assert b.obs_dim() == (6, 2, 12) and b.obs_layout() == [0, 3] and b.obs_launches() == 0
        with pytest.raises(RuntimeError, match="no input bound"):
            b.observe()
        inp = torch.ones((4, 5), dtype=torch.float64, device="cuda")
        b.bind_obs_input(inp.data_ptr(), 4, 5, torch.float64)
        with pytest.raises(RuntimeError, match="shorter"):
            b.observe()
        b.bind_obs_input(inp.data_ptr(), 5, 5, torch.float64)
        with pytest.raises(RuntimeError, match="out of bounds"):
            b.observe(2, 3)
        with pytest.raises(ValueError, match="row stride"):
            b.bind_obs(inp.data_ptr(), 11)
        b.observe()
        b.observe(1, 2)
        assert b.obs_launches() == 2 and list(b.obs_frames()) == [1, 2, 2, 1]
        assert np.all(b.obs()[:, :, 3:] == 1.0) and np.array_equal(b.obs()[:, 0, :3], b.get(P.F_QPOS)[:, :3].astype(np.float32))
        # configuring again zeroes the counts and drops the input's binding; no terms releases everything
        b.configure_obs(t, history=1)
        assert list(b.obs_frames()) == [0] * 4
        with pytest.raises(RuntimeError, match="no input bound"):
            b.observe()
        b.configure_obs([])
        with pytest.raises(RuntimeError, match="not configured"):
            b.observe()
    finally:
        b.close()
