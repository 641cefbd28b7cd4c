"""Episodes that end and restart on the device (phys_batch_end_episodes) on the GPU: a restarted env continues like an env of a
fresh batch, a diverged env comes back, the rules agree with the numpy restatement (tests/episode_check.py) on all 4096 envs, and a
rollout whose episodes are ended and restarted on the device -- two env ranges on two streams, nothing downloaded until the end --
ends byte for byte where the same rollout with the decision and the restart made on the host does.  The CPU counterpart (the same
kernel on the wave emulator, hand-placed states) is tests/test_episodes.py.

Every rule test asserts on its inputs that NO env lies within 1e-9 of min_height / min_upright before it compares."""
import ctypes

import numpy as np
import pytest

import bench
import episode_check as ec
from cassie_amd import Batch
from cassie_amd import phys as P
from cassie_amd.distributed import ObservationBlock
from hostchain_py import device_state_bytes

pytestmark = pytest.mark.gpu

STATE_FIELDS = (P.F_QPOS, P.F_QVEL, P.F_QACC_WARMSTART, P.F_TIME, P.F_CTRL, P.F_QACC, P.F_SENSORDATA, P.F_ACTUATOR_VELOCITY, P.F_MEAS)
BANK_FIELDS = (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA, P.F_ACTUATOR_VELOCITY, P.F_QACC)
# the falling workload of the loop tests, settled on the CPU reference (bench.SafeHostChainEnvs, 64 envs; see
# test_device_loop_equals_host_loop)
STRESS_SPREAD = 10.0
LOOP_RULES = ec.rules(min_height=0.8, min_upright=0.7, max_steps=4, warn_mask=P.WARN_DIVERGED, nonfinite=True)
LOOP_NPOL = 9


def bank_states(model, k, seed=11):
    """k start states near the init pose with non-zero velocities (a stand-in for the phases of a reference gait)."""
    rng = np.random.default_rng(seed)
    q = np.tile(model.qpos_init(), (k, 1))
    q[:, 7:] += rng.uniform(-0.02, 0.02, (k, model.pod.nq - 7))
    v = rng.uniform(-0.05, 0.05, (k, model.pod.nv))
    return q, v


def make(model, n, mode, qpos=None, qvel=None):
    """A fresh batch: set(qpos), set(qvel), forward(), then the drive mode."""
    b = Batch(model, n)
    b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)) if qpos is None else qpos)
    if qvel is not None:
        b.set(P.F_QVEL, qvel)
    b.forward()
    b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
    b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
    b.set_drive_mode(mode)
    return b


def stress_targets(n, npol):
    keep = bench.TARGET_SPREAD
    bench.TARGET_SPREAD = STRESS_SPREAD                    # (what bench.py --target-spread 10 sets)
    try:
        return bench.pd_targets(np.arange(n), npol)
    finally:
        bench.TARGET_SPREAD = keep


def drive_bytes(b, envs=None):
    s = b.get_drive_state()
    return [device_state_bytes(s[int(e)]) + (int(s[int(e)].safety_msg),) for e in (range(b.nenv) if envs is None else envs)]


def test_restart_equals_a_fresh_batch(cassie):
    """64 envs in DRIVE_PD_SAFE, 100 steps, then end_episodes with a force mask on a scattered set of envs and a bank of 16 poses with
    non-zero qvel, a distinct row per env; after two more policy steps the restarted envs are byte-equal to a fresh batch that was
    set to the same rows + forward() and given the same targets, the others to a run without the call."""
    import torch
    n, k = 64, 16
    tg = bench.pd_targets(np.arange(n), 4)
    forced = np.array([1, 2, 5, 11, 12, 20, 33, 34, 47, 58, 63])
    others = np.setdiff1d(np.arange(n), forced)
    bq, bv = bank_states(cassie, k)
    pick = np.random.default_rng(4).integers(0, k, n).astype(np.int32)
    pick[forced] = np.random.default_rng(5).permutation(k)[:len(forced)] + k * np.arange(len(forced))   # distinct rows, some given modulo k
    force = np.zeros(n, dtype=np.int32)
    force[forced] = 1 + np.arange(len(forced))
    a, c = make(cassie, n, P.DRIVE_PD_SAFE), make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        for p in range(2):
            for b in (a, c):
                b.set(P.F_PD_PTARGET, tg[p]); b.step(50)
        before = {f: a.get(f) for f in STATE_FIELDS}
        a.enable_episodes()                                  # no rule of its own: only the mask ends episodes
        bank = a.make_reset_bank(bq, bv)
        assert bank.shape == (k, a.episode_row_dim()) and np.array_equal(bank[:, :cassie.pod.nq], bq) and bank[:, -cassie.pod.nv:].any()
        a.set_reset_bank(bank)
        pick_d, force_d = torch.from_numpy(pick).cuda(), torch.from_numpy(force).cuda()
        a.end_episodes(pick_ptr=pick_d.data_ptr(), force_ptr=force_d.data_ptr())
        done, reason, steps, count, terminal = a.episodes()
        assert np.array_equal(np.nonzero(done)[0], forced) and np.array_equal(reason, np.where(force != 0, ec.DONE_FORCED, 0))
        assert np.array_equal(count, done) and np.array_equal(steps, 1 - done)
        assert terminal[forced].tobytes() == np.concatenate([before[P.F_QPOS], before[P.F_QVEL]], axis=1)[forced].tobytes()
        assert not terminal[others].any()
        rows = bank[pick % k]
        o = 0
        for f in BANK_FIELDS:                                # right after the call: the row's fields, zeros, everybody else as before
            w = a.dim(f)
            got = a.get(f)
            assert got[forced].tobytes() == rows[forced, o:o + w].tobytes() and got[others].tobytes() == before[f][others].tobytes(), f
            o += w
        for f in (P.F_QACC_WARMSTART, P.F_TIME, P.F_CTRL, P.F_MEAS):
            got = a.get(f)
            assert not got[forced].any() and got[others].tobytes() == before[f][others].tobytes(), f
        q0, v0 = np.tile(cassie.qpos_init(), (n, 1)), np.zeros((n, cassie.pod.nv))
        q0[forced], v0[forced] = bq[pick[forced] % k], bv[pick[forced] % k]
        fresh = make(cassie, n, P.DRIVE_PD_SAFE, q0, v0)
        try:
            for p in range(2, 4):
                for b in (a, c, fresh):
                    b.set(P.F_PD_PTARGET, tg[p]); b.step(50)
            for f in (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA, P.F_MEAS, P.F_QACC_WARMSTART, P.F_TIME, P.F_CTRL, P.F_QACC, P.F_ACTUATOR_VELOCITY):
                ga, gc_, gf = a.get(f), c.get(f), fresh.get(f)
                assert ga[forced].tobytes() == gf[forced].tobytes(), f
                assert ga[others].tobytes() == gc_[others].tobytes(), f
            assert drive_bytes(a, forced) == drive_bytes(fresh, forced) and drive_bytes(a, others) == drive_bytes(c, others)
            assert np.array_equal(a.warnings()[0], np.where(done != 0, fresh.warnings()[0], c.warnings()[0]))
        finally:
            fresh.close()
    finally:
        a.close(); c.close()


def test_a_diverged_env_comes_back(cassie):
    """A non-finite qvel entry uploaded into three envs: the step kernel's guard sets WARN_DIVERGED and leaves their state untouched,
    as ever; end_episodes with warn_mask = WARN_DIVERGED reports CM_DONE_WARN, clears the word, and from there they step byte-equal
    to fresh envs."""
    n, k = 64, 8
    sick = np.array([7, 30, 31])
    tg = bench.pd_targets(np.arange(n), 4)
    bq, bv = bank_states(cassie, k)
    b = make(cassie, n, P.DRIVE_PD)
    try:
        b.set(P.F_PD_PTARGET, tg[0]); b.step(50)
        v = b.get(P.F_QVEL)
        v[sick[0], 3], v[sick[1], 0], v[sick[2], cassie.pod.nv - 1] = np.nan, np.inf, np.nan
        b.set(P.F_QVEL, v)
        q = b.get(P.F_QPOS)
        b.set(P.F_PD_PTARGET, tg[1]); b.step(50)
        w = b.warnings()[0]
        assert np.array_equal(np.nonzero(w & P.WARN_DIVERGED)[0], sick)
        assert b.get(P.F_QVEL)[sick].tobytes() == v[sick].tobytes() and b.get(P.F_QPOS)[sick].tobytes() == q[sick].tobytes()
        b.enable_episodes(warn_mask=P.WARN_DIVERGED)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.end_episodes()
        done, reason, steps, count, terminal = b.episodes()
        assert np.array_equal(np.nonzero(done)[0], sick) and np.array_equal(reason, np.where(done != 0, ec.DONE_WARN, 0))
        assert terminal[sick].tobytes() == np.concatenate([q, v], axis=1)[sick].tobytes()
        assert not b.warnings()[0][sick].any() and np.array_equal(b.warnings()[0][done == 0], w[done == 0])
        rows = (sick + 1) % k                               # pick = NULL: (env + count) % nrows
        q0, v0 = np.tile(cassie.qpos_init(), (n, 1)), np.zeros((n, cassie.pod.nv))
        q0[sick], v0[sick] = bq[rows], bv[rows]
        fresh = make(cassie, n, P.DRIVE_PD, q0, v0)
        try:
            for p in range(2, 4):
                for x in (b, fresh):
                    x.set(P.F_PD_PTARGET, tg[p]); x.step(50)
            for f in (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA, P.F_MEAS, P.F_QACC_WARMSTART, P.F_TIME):
                assert b.get(f)[sick].tobytes() == fresh.get(f)[sick].tobytes(), f
            assert np.isfinite(b.get(P.F_QPOS)).all() and not b.warnings()[0][sick].any()
            assert drive_bytes(b, sick) == drive_bytes(fresh, sick)
        finally:
            fresh.close()
    finally:
        b.close()


def test_rules_exact_on_all_envs(cassie):
    """4096 envs spread by the falling workload: at three successive policy steps done / reason from the device (restart = 0) equal
    the numpy restatement on the downloaded state, every env clear of the thresholds by 1e-9, none left out."""
    n, npol = 4096, 8
    r = ec.rules(min_height=0.85, min_upright=0.7, max_steps=2, warn_mask=P.WARN_DIVERGED, nonfinite=True)
    tg = stress_targets(n, npol)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        b.enable_episodes(**r)
        seen = 0
        for p in range(npol):
            b.set(P.F_PD_PTARGET, tg[p]); b.step(50)
            if p < npol - 3:
                continue
            b.end_episodes(restart=False)
            q, v, w = b.get(P.F_QPOS), b.get(P.F_QVEL), b.warnings()[0]
            done, reason, steps, count, terminal = b.episodes()
            ec.assert_clear_of_thresholds(q, r)
            assert np.array_equal(steps, np.full(n, p - (npol - 3) + 1))
            want = ec.reasons(q, v, w, steps, r)
            print("policy step %d: %d envs done, by bit %s" % (p, (want != 0).sum(), {bit: int(((want & bit) != 0).sum()) for bit in ec.ALL_BITS}))
            assert np.array_equal(reason, want) and np.array_equal(done, (want != 0).astype(np.int32))
            ended = done != 0
            assert terminal[ended].tobytes() == np.concatenate([q, v], axis=1)[ended].tobytes()
            seen |= int(np.bitwise_or.reduce(reason))
        assert seen & ec.DONE_UPRIGHT and seen & ec.DONE_HEIGHT and seen & ec.DONE_TIME
    finally:
        b.close()


def _host_restart(b, ended, rows, bank, warn):
    """Loop B's restart: the bank rows and the zeros uploaded field by field, drive state and warnings cleared through the host calls."""
    o = 0
    for f in BANK_FIELDS:
        w = b.dim(f)
        a = b.get(f)
        a[ended] = bank[rows, o:o + w]
        b.set(f, a)
        o += w
    for f in (P.F_QACC_WARMSTART, P.F_TIME, P.F_CTRL, P.F_MEAS):
        a = b.get(f)
        a[ended] = 0
        b.set(f, a)
    for e in ended:
        b.clear_drive_state(int(e), 1, 1)
        if warn[e]:
            b.clear_warnings(int(e), 1)
    b.sync()


def _loops(cassie, n, strided):
    import torch
    k = 8
    npol, r = LOOP_NPOL, LOOP_RULES
    tg = stress_targets(n, npol)
    bq, bv = bank_states(cassie, k)
    pick = np.random.default_rng(2024).integers(0, k, (npol, n)).astype(np.int32)
    tgd, pick_d = torch.from_numpy(tg).cuda(), torch.from_numpy(pick).cuda()
    half = n // 2
    ranges = [(0, half), (half, n - half)]

    def final(b):
        out = {f: b.get(f) for f in STATE_FIELDS}
        out["warn"] = b.warnings()[0]
        out["drive"] = drive_bytes(b)
        return out

    # loop A: the device loop -- two ranges on two streams, end_episodes per range, nothing downloaded until the end
    a = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        obs = None
        if strided:
            init = torch.from_numpy(np.concatenate([a.get(P.F_QPOS)[0], a.get(P.F_QVEL)[0], a.get(P.F_SENSORDATA)[0]]))
            obs = ObservationBlock(a, cassie.pod, torch.device("cuda", 0), init)
        a.enable_episodes(**r)
        bank = a.make_reset_bank(bq, bv)
        bank_d = torch.from_numpy(bank).cuda()
        a.set_reset_bank(device_ptr=bank_d.data_ptr(), n=k)
        a.sync()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for p in range(npol):
            a.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
            for (e0, cnt), st in zip(ranges, streams):
                a.step_range(e0, cnt, 50, st.cuda_stream)
                a.end_episodes(e0, cnt, True, pick_ptr=pick_d[p].data_ptr() + 4 * e0, stream=st.cuda_stream)
        got = final(a)
        _, _, got["steps"], got["count"], _ = a.episodes()
        if strided:
            assert obs.tensor.cpu().numpy().tobytes() == np.concatenate([got[P.F_QPOS], got[P.F_QVEL], got[P.F_SENSORDATA]], axis=1).tobytes()
    finally:
        a.close()

    # loop B: the host loop -- the whole batch, downloaded after every policy step, decided by episode_check, restarted by uploads
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        steps, count = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        ended_by = {bit: 0 for bit in ec.ALL_BITS}
        for p in range(npol):
            b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
            b.step(50)
            q, v, w = b.get(P.F_QPOS), b.get(P.F_QVEL), b.warnings()[0]
            ec.assert_clear_of_thresholds(q, r)
            steps += 1
            reason = ec.reasons(q, v, w, steps, r)
            ended = np.nonzero(reason)[0]
            for bit in ec.ALL_BITS:
                ended_by[bit] += int(((reason & bit) != 0).sum())
            count[ended] += 1
            steps[ended] = 0
            if len(ended):
                _host_restart(b, ended, ec.bank_rows(0, n, count, k, pick[p])[ended], bank, w)
        want = final(b)
        want["steps"], want["count"] = steps, count
    finally:
        b.close()
    print("%d envs, %d policy steps: episodes ended by bit %s, restarts per env %s" % (n, npol, ended_by, np.bincount(count)))
    for key in want:
        if key == "drive":
            assert got[key] == want[key], key
        else:
            assert got[key].tobytes() == want[key].tobytes(), (key, np.nonzero((got[key] != want[key]).reshape(n, -1).any(axis=1))[0][:16])
    # not vacuous: robots fell, episodes timed out, and some env restarted more than once
    assert ended_by[ec.DONE_HEIGHT] + ended_by[ec.DONE_UPRIGHT] > 0 and ended_by[ec.DONE_TIME] > 0 and count.max() > 1


def test_device_loop_equals_host_loop(cassie):
    """4096 cassie.xml envs, DRIVE_PD_SAFE, 50 substeps per policy step, bench.pd_targets at the stress spread 10 (what
    `bench.py --target-spread 10` sets; restored afterwards).  After the last policy step every state array, the drive state, the
    warning words, `count` and `steps` are byte-equal between the device loop and the host loop, with the same seeded `pick`.

    Chosen on the CPU reference (bench.SafeHostChainEnvs, 64 envs, the same targets / bank / pick seed), the smallest horizon that
    meets the three assertions with room: min_height 0.8, min_upright 0.7, max_steps 4, 9 policy steps.  Observed there: 25 episodes
    ended by CM_DONE_UPRIGHT, 126 by CM_DONE_TIME, none by CM_DONE_HEIGHT (the robots tilt long before the pelvis sinks: the first
    env passes 0.7 after 3 policy steps, the first pelvis 0.8 after 7), every one of the 64 envs restarted exactly twice.  (With
    max_steps 5 / 11 steps: 37 and 99; with 6 / 13: 51 and 94.)  On the MI355X at 4096 envs: 1443 episodes ended by CM_DONE_UPRIGHT,
    8016 by CM_DONE_TIME, every env restarted exactly twice; at 256 envs (the strided test below): 97 and 503."""
    _loops(cassie, 4096, strided=False)


def test_device_loop_equals_host_loop_with_a_strided_observation_block(cassie):
    """The same at 256 envs with qpos / qvel / sensordata bound as the column blocks of one ObservationBlock in the device loop."""
    _loops(cassie, 256, strided=True)
