"""The case the observation rows are checked on, shared by the CPU test (tests/test_obs.py: the wave emulator) and the GPU test
(tests/test_obs_gpu.py: the device) -- test infrastructure only.  Five cassie envs advanced a few substeps by the emulator, seven terms
that cross a wave's 64 lanes, a history of three frames over five calls with the state changed between them, and what tests/obs_check.py
makes of it."""
import numpy as np

import obs_check as oc
from cassie_amd import phys as P
from emu_py import EmuBatch

NENV, HISTORY, SEED, INPUT_DIM, INPUT_STRIDE = 5, 3, 0x9E3779B97F4A7C15, 6, 8
# the calls: (env0, n, refill) -- the first fills every frame, the second shifts, the third and fourth leave envs 0 and 4 alone, the
# fourth refills env 2, the fifth shifts again
SCHEDULE = ((0, 5, None), (0, 5, None), (1, 3, None), (1, 3, (0, 1, 0)), (0, 5, None))


def terms_of(pod):
    """qpos[7:9] | 70 noisy sensors, or as many as the model has (cassie: 29) | the base velocity in the body frame | the projected
    gravity | four noisy columns of a float32 input | six joint velocities, scaled and clipped | every joint velocity, noisy: with it the
    frame crosses a wave's 64 lanes on a model of fewer than 70 sensors, at a width that is no multiple of 64."""
    ns = min(70, pod.nsensordata)
    return [P.obs_copy(P.F_QPOS, 7, 2),
            P.obs_copy(P.F_SENSORDATA, 0, ns, offset=0.1, scale=2.0, noise=0.05),
            P.obs_rot_inv(P.F_QVEL, 0, P.F_QPOS, 3, scale=0.5),
            P.obs_rot_inv(P.OBS_CONST, 0, P.F_QPOS, 3, vec=(0.0, 0.0, -1.0)),
            P.obs_copy(P.OBS_INPUT, 1, 4, offset=-0.25, scale=3.0, noise=0.5),
            P.obs_copy(P.F_QVEL, 6, 6, scale=10.0, lo=-0.5, hi=0.5),
            P.obs_copy(P.F_QVEL, 0, pod.nv, scale=0.25, noise=0.02)]


def make_states(cassie, ncalls=len(SCHEDULE), nenv=NENV, seed=11):
    """One state per call: {field: array [nenv][dim]} of qpos, qvel, sensordata and the float32 input [nenv][INPUT_STRIDE] (INPUT_DIM
    columns bound), the emulator's after 2 + k substeps under random torques from a perturbed start."""
    pod = cassie.pod
    rng = np.random.default_rng(seed)
    emu = EmuBatch(pod, nenv)
    emu.qpos[:] = cassie.qpos_init()
    emu.qpos[:, 2] += rng.uniform(0.0, 0.05, nenv)
    emu.qpos[:, 3:7] += 0.1 * rng.standard_normal((nenv, 4))       # (left unnormalised: the quaternion is used as stored)
    emu.qvel[:] = rng.uniform(-0.5, 0.5, (nenv, pod.nv))
    emu.ctrl[:] = rng.uniform(-2.0, 2.0, (nenv, pod.nu))
    states = []
    for k in range(ncalls):
        emu.step(2 if k == 0 else 1)
        states.append({P.F_QPOS: emu.qpos.copy(), P.F_QVEL: emu.qvel.copy(), P.F_SENSORDATA: emu.sensordata.copy(),
                       P.OBS_INPUT: rng.uniform(-1.0, 1.0, (nenv, INPUT_STRIDE)).astype(np.float32)})
    assert not emu.warn.any() and np.abs(states[0][P.F_SENSORDATA]).max() > 0
    return states


def reference(terms, states, dtype, schedule=SCHEDULE, nenv=NENV, history=HISTORY, seed=SEED, env_base=0):
    """The rows and frame counts after every call of the schedule by tests/obs_check.py -> [(rows [nenv][history][ncols], frames)]."""
    ref = oc.Obs(terms, nenv, history, dtype, seed, env_base)
    out = []
    for state, (env0, n, refill) in zip(states, schedule):
        ref.observe(state, env0, n, refill)
        out.append((ref.rows.copy(), ref.frames.copy()))
    return out
