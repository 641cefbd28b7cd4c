"""phys_batch_end_episodes restated in numpy (include/cassie_phys.h: the four steps, per env, in order) -- shared by the emulator
suite (tests/test_episodes.py) and the GPU suite (tests/test_episodes_gpu.py).

A `state` is a dict of per-env arrays indexed by the absolute env: qpos, qvel, sensordata, actuator_velocity, qacc,
qacc_warmstart, ctrl, time, warn (int32), done, reason, steps, count (int32), terminal [nenv][nq + nv], and -- once a drive mode
is in use, else None -- meas [nenv][56] and drive (uint8 [nenv][sizeof cm_drive_state_t])."""
import ctypes

import numpy as np

from cassie_amd._lib import CmDriveState

DONE_HEIGHT, DONE_UPRIGHT, DONE_TIME, DONE_WARN, DONE_NONFINITE, DONE_FORCED = 1, 2, 4, 8, 16, 32
ALL_BITS = (DONE_HEIGHT, DONE_UPRIGHT, DONE_TIME, DONE_WARN, DONE_NONFINITE, DONE_FORCED)
THRESHOLD_MARGIN = 1e-9          # no env of a rule test may lie closer than this to min_height / min_upright
DRIVE_BYTES = ctypes.sizeof(CmDriveState)
STATE_ARRAYS = ("qpos", "qvel", "sensordata", "actuator_velocity", "qacc", "qacc_warmstart", "ctrl", "time", "warn", "meas", "drive")
EPISODE_ARRAYS = ("done", "reason", "steps", "count", "terminal")


def rules(min_height=-np.inf, min_upright=-np.inf, max_steps=0, warn_mask=0, nonfinite=False):
    return dict(min_height=float(min_height), min_upright=float(min_upright), max_steps=int(max_steps), warn_mask=int(warn_mask),
                nonfinite=bool(nonfinite))


def height(qpos):
    return qpos[:, 2]


def upright(qpos):
    """World-z component of the pelvis' z axis, q = qpos[3..6] = (w, x, y, z), in float64 exactly as the header writes it."""
    qx, qy = qpos[:, 4], qpos[:, 5]
    return 1.0 - 2.0 * (qx * qx + qy * qy)


def row_dim(pod):
    return pod.nq + pod.nv + pod.nsensordata + pod.nu + pod.nv


def assert_clear_of_thresholds(qpos, r):
    """The condition on every rule test's inputs: every env (none left out) is further than THRESHOLD_MARGIN from both thresholds
    (NaN / huge entries are compared like any other: a NaN is on neither side and never within the margin)."""
    with np.errstate(invalid="ignore"):
        for value, limit, what in ((height(qpos), r["min_height"], "min_height"), (upright(qpos), r["min_upright"], "min_upright")):
            if np.isfinite(limit):
                close = np.abs(value - limit) <= THRESHOLD_MARGIN
                assert not close.any(), "envs %s lie within %g of %s" % (np.nonzero(close)[0], THRESHOLD_MARGIN, what)


def reasons(qpos, qvel, warn, steps, r, force=None):
    """Step 2: the reason word of every env from its state, warning word and (already incremented) step counter."""
    n = qpos.shape[0]
    out = np.zeros(n, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        out[height(qpos) < r["min_height"]] |= DONE_HEIGHT
        out[upright(qpos) < r["min_upright"]] |= DONE_UPRIGHT
        if r["max_steps"] > 0:
            out[steps >= r["max_steps"]] |= DONE_TIME
        out[(warn.astype(np.int64) & r["warn_mask"]) != 0] |= DONE_WARN
        if r["nonfinite"]:
            bad = lambda a: (~(a == a) | (np.abs(a) > 1e10)).any(axis=1)
            out[bad(qpos) | bad(qvel)] |= DONE_NONFINITE
    if force is not None:
        out[np.asarray(force) != 0] |= DONE_FORCED
    return out


def bank_rows(env0, n, count, nrows, pick=None):
    """Step 4's row for every env of the range (count: the range's counters AFTER step 3)."""
    if pick is not None:
        return np.mod(np.asarray(pick, dtype=np.int64), nrows)
    return (np.arange(env0, env0 + n, dtype=np.int64) + count.astype(np.int64)) % nrows


def end_episodes(state, pod, r, env0, n, restart, bank=None, pick=None, force=None):
    """The whole call on `state`, in place; returns the mask (over the range) of the envs that ended."""
    s = state
    sl = slice(env0, env0 + n)
    s["steps"][sl] += 1                                                                     # 1
    reason = reasons(s["qpos"][sl], s["qvel"][sl], s["warn"][sl], s["steps"][sl], r, force)  # 2
    done = reason != 0
    s["reason"][sl] = reason
    s["done"][sl] = done.astype(np.int32)
    ended = env0 + np.nonzero(done)[0]
    s["terminal"][ended] = np.concatenate([s["qpos"][ended], s["qvel"][ended]], axis=1)      # 3
    s["count"][ended] += 1
    if restart and len(ended):                                                              # 4
        rows = bank[bank_rows(env0, n, s["count"][sl], bank.shape[0], pick)[done]]
        o = 0
        for f, w in (("qpos", pod.nq), ("qvel", pod.nv), ("sensordata", pod.nsensordata), ("actuator_velocity", pod.nu), ("qacc", pod.nv)):
            s[f][ended] = rows[:, o:o + w]
            o += w
        for f in ("qacc_warmstart", "ctrl", "time", "warn", "steps"):
            s[f][ended] = 0
        for f in ("meas", "drive"):
            if s.get(f) is not None:
                s[f][ended] = 0
    return done


def copy_state(state):
    return {k: (None if v is None else v.copy()) for k, v in state.items()}


def assert_states_equal(a, b, what=""):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), "%s: %s differs in envs %s" % (
            what, k, np.nonzero((a[k].reshape(len(a[k]), -1).view(np.uint8) != b[k].reshape(len(b[k]), -1).view(np.uint8)).any(axis=1))[0][:16])
