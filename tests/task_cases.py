"""The case the task rows are checked on, shared by the CPU test (tests/test_task.py: the wave emulator) and the GPU test
(tests/test_task_gpu.py: the device) -- test infrastructure only.  Five envs, 19 columns: a command group of three (period 2 .. 4, resting
with probability 0.3), a push group of two into xfrc_applied (shown for one call of three, else 0), a gait frequency, an initial phase, a
clock driven by those two and one with a constant rate, the four waveforms (two shifted by half a cycle) and four columns of a 7-frame,
5-column table; fourteen calls; and what tests/task_check.py makes of it."""
import numpy as np

import task_check as tc
from cassie_amd import phys as P

NENV, SEED, ROW_STRIDE = 5, 0x243F6A8885A308D3, 23
# the columns by name
(VX, VY, YAW, PUSH_X, PUSH_Y, FREQ, PHASE0, CLOCK, CLOCK2, SAW, SIN, COS, GATE, GATE_B, SAW_B, TAB0, TAB1, TAB2, TAB3) = range(19)
NCOLS = 19
COMMAND, PUSH = (VX, VY, YAW), (PUSH_X, PUSH_Y)
SAMPLES = (VX, VY, YAW, PUSH_X, PUSH_Y, FREQ, PHASE0)
NFRAMES, TCOLS = 7, 5
# the calls: (env0, n, reset) -- a first call, plain calls long enough for every period length (2, 3, 4) to expire more than once, a call
# that leaves envs 0 and 4 alone, and a call that restarts envs 1 and 3
SCHEDULE = ((0, 5, None),) + ((0, 5, None),) * 7 + ((1, 3, None),) + ((0, 5, None),) * 2 + ((0, 5, (0, 1, 0, 1, 0)),) + ((0, 5, None),) * 2
DEST_FIELDS = (P.F_XFRC_APPLIED,)


def push_elems(pod):
    """The two elements of an env's xfrc_applied row the push group writes: the x and y force on body 1."""
    return 6 * 1 + 0, 6 * 1 + 1


def columns_of(pod):
    px, py = push_elems(pod)
    cols = [None] * NCOLS
    cols[VX] = P.task_sample(0.5, 1.0, 2, 4, rest=0.0, p_rest=0.3)
    cols[VY] = P.task_sample(0.0, 0.3, 2, 4, rest=0.0, p_rest=0.3, group=VX)
    cols[YAW] = P.task_sample(0.0, 0.5, 2, 4, rest=0.0, p_rest=0.3, group=VX)
    cols[PUSH_X] = P.task_sample(0.0, 50.0, 3, 3, rest=0.0, p_rest=0.5, hold=1, dfield=P.F_XFRC_APPLIED, dindex=px)
    cols[PUSH_Y] = P.task_sample(0.0, 30.0, 3, 3, rest=0.0, p_rest=0.5, hold=1, group=PUSH_X, dfield=P.F_XFRC_APPLIED, dindex=py)
    cols[FREQ] = P.task_sample(1.0, 0.5, 3, 5, rest=1.0, p_rest=0.25)
    cols[PHASE0] = P.task_sample(0.5, 0.5, 4, 6, rest=0.0, p_rest=0.25)
    cols[CLOCK] = P.task_phase(rate=0.05, rate_col=FREQ, rate_scale=0.22, phase_col=PHASE0)
    cols[CLOCK2] = P.task_phase(rate=0.135, phase0=0.9)
    cols[SAW] = P.task_wave(CLOCK, P.TASK_SAW, offset=-1.0, scale=2.0)
    cols[SIN] = P.task_wave(CLOCK, P.TASK_SIN)
    cols[COS] = P.task_wave(CLOCK, P.TASK_COS, shift=0.5, scale=0.75, offset=0.125)
    cols[GATE] = P.task_wave(CLOCK, P.TASK_TRAPEZOID, duty=0.5, ramp=0.1)
    cols[GATE_B] = P.task_wave(CLOCK, P.TASK_TRAPEZOID, shift=0.5, duty=0.5, ramp=0.1)
    cols[SAW_B] = P.task_wave(CLOCK2, P.TASK_SAW)
    cols[TAB0] = P.task_table(CLOCK, 0)
    cols[TAB1] = P.task_table(CLOCK, 4, shift=0.5, offset=0.1, scale=-2.0)
    cols[TAB2] = P.task_table(CLOCK2, 2)
    cols[TAB3] = P.task_table(CLOCK2, 1, shift=0.25, scale=0.5)
    return cols


def make_table(seed=5):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (NFRAMES, TCOLS))


def start_fields(cassie, nenv=NENV, seed=29):
    """What the destination field holds before the first call: {field: array [nenv][dim]}, every element its own value."""
    return {P.F_XFRC_APPLIED: np.random.default_rng(seed).uniform(-1.0, 1.0, (nenv, 6 * cassie.pod.nbody))}


def reference(cols, table, dtype, fields, schedule=SCHEDULE, nenv=NENV, seed=SEED, env_base=0, start=None):
    """The rows, state, words, counts, destination fields and what every column did after every call of the schedule by
    tests/task_check.py -> [(rows, state, words, counts, {field: array}, drew, resting, wrapped)]; `fields` is left unchanged."""
    ref = tc.Task(cols, nenv, dtype, seed, env_base, table=table)
    if start is not None:
        ref.state[:], ref.words[:], ref.counts[:] = start
    held = {f: a.copy() for f, a in fields.items()}
    out = []
    for env0, n, reset in schedule:
        ref.task(held, env0, n, reset)
        out.append((ref.rows.copy(), ref.state.copy(), ref.words.copy(), ref.counts.copy(), {f: held[f].copy() for f in DEST_FIELDS}, ref.drew.copy(),
                    ref.resting.copy(), ref.wrapped.copy()))
    return out
