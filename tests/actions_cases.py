"""The case the action rows are checked on, shared by the CPU test (tests/test_actions.py: the wave emulator) and the GPU test
(tests/test_actions_gpu.py: the device) -- test infrastructure only.  Five cassie envs, 70 columns (a frame crosses a wave's 64 lanes at
a width that is no multiple of 64) into the PD's position targets on a reference pose from a float32 input, its low-passed velocity
targets, its noisy and tightly clipped feed-forward torques and the last word of xfrc_applied; a delay line of depth 3 with per-env delays
(one beyond the depth); float32 actions that change every call, env 4's out of range, infinite and NaN; seven calls; and what
tests/actions_check.py makes of it."""
import numpy as np

import actions_check as ac
from cassie_amd import phys as P

NENV, NCOLS, DELAY_MAX, SEED, INPUT_DIM, INPUT_STRIDE, ACT_STRIDE = 5, 70, 3, 0x9E3779B97F4A7C15, 12, 14, 73
DELAYS = (0, 1, 2, 3, 9)          # (the 9 clamps to 3)
# the calls: (env0, n, reset) -- the first fills every line, three shifts cycle it fully, the fifth leaves envs 0 and 4 alone, the sixth
# restarts env 2, the seventh shifts again
SCHEDULE = ((0, 5, None), (0, 5, None), (0, 5, None), (0, 5, None), (1, 3, None), (0, 5, (0, 0, 1, 0, 0)), (0, 5, None))
DEST_FIELDS = (P.F_PD_PTARGET, P.F_PD_DTARGET, P.F_PD_TORQUE, P.F_XFRC_APPLIED)


def columns_of(pod):
    """0 .. 9 position targets on the input's pose | 10 .. 19 velocity targets, low-passed | 20 .. 29 torques, noisy, clipped tightly |
    30 the last word of xfrc_applied on a base from qpos | 31 .. 69 tracked only, with mixed clips, noise and filters."""
    assert pod.nu == 10
    cols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, bfield=P.ACT_INPUT, bindex=2 + j, scale=0.5) for j in range(10)]
    cols += [P.act_col(P.F_PD_DTARGET, j, lo=-2.0, hi=2.0, smooth=0.5, scale=2.0) for j in range(10)]
    cols += [P.act_col(P.F_PD_TORQUE, j, noise=0.1, offset=0.05, out_lo=-0.3, out_hi=0.3) for j in range(10)]
    cols += [P.act_col(P.F_XFRC_APPLIED, 6 * pod.nbody - 1, bfield=P.F_QPOS, bindex=2, offset=-1.0, scale=10.0, smooth=0.75)]
    for c in range(31, NCOLS):
        lo, hi = (-0.6, 0.8) if c % 5 == 0 else (-np.inf, np.inf)
        cols.append(P.act_col(lo=lo, hi=hi, noise=0.05 if c % 2 else 0.0, smooth=(1.0, 0.25, 0.75)[c % 3], scale=1.5, offset=0.5))
    assert len(cols) == NCOLS
    return cols


def make_calls(cassie, ncalls=len(SCHEDULE), nenv=NENV, seed=17):
    """One (actions float32 [nenv][ACT_STRIDE], input float32 [nenv][INPUT_STRIDE]) per call.  Envs 0 .. 3 stay inside every clip; env 4
    leaves them, and carries +inf (column 5), -inf (column 33) and NaN (columns 12 and 40) in some calls."""
    rng = np.random.default_rng(seed)
    calls = []
    for k in range(ncalls):
        act = rng.uniform(-0.55, 0.55, (nenv, ACT_STRIDE)).astype(np.float32)
        act[4] *= np.float32(4.0)
        if k in (1, 4):
            act[4, 5], act[4, 33] = np.inf, -np.inf
        if k == 2:
            act[4, 12], act[4, 40] = np.nan, np.nan
        calls.append((act, rng.uniform(-1.0, 1.0, (nenv, INPUT_STRIDE)).astype(np.float32)))
    return calls


def start_fields(cassie, nenv=NENV, seed=23):
    """What the fields hold before the first call: {field: array [nenv][dim]} of the destinations, every element its own value, and qpos."""
    pod = cassie.pod
    rng = np.random.default_rng(seed)
    dims = {P.F_PD_PTARGET: pod.nu, P.F_PD_DTARGET: pod.nu, P.F_PD_TORQUE: pod.nu, P.F_XFRC_APPLIED: 6 * pod.nbody, P.F_QPOS: pod.nq}
    return {f: rng.uniform(-1.0, 1.0, (nenv, d)) for f, d in dims.items()}


def reference(cols, calls, dtype, fields, schedule=SCHEDULE, nenv=NENV, delay_max=DELAY_MAX, seed=SEED, env_base=0, delays=DELAYS):
    """The rows, state, counts and destination fields after every call of the schedule by tests/actions_check.py ->
    [(rows [nenv][3][ncols], state [nenv][D + 3][ncols], counts, {field: array})]; `fields` is left unchanged."""
    ref = ac.Actions(cols, nenv, delay_max, dtype, seed, env_base, delay=delays)
    held = {f: a.copy() for f, a in fields.items()}
    out = []
    for (act, inp), (env0, n, reset) in zip(calls, schedule):
        held[P.ACT_INPUT] = inp
        ref.act(act, held, env0, n, reset)
        out.append((ref.rows.copy(), ref.state.copy(), ref.counts.copy(), {f: held[f].copy() for f in DEST_FIELDS}))
    return out
