"""The case the reward rows are checked on, shared by the CPU test (tests/test_rewards.py: the wave emulator) and the GPU test
(tests/test_rewards_gpu.py: the device) -- test infrastructure only.  Six cassie envs from the observation case's generator, a float32
input whose row stride is wider than its dim, thirteen terms that between them use every kind, norm, shape and source the definition has,
one env whose k s passes expn's cut, one env with a NaN velocity, five calls with the state changed between them, and what
tests/rewards_check.py makes of it."""
import numpy as np

import obs_cases
import rewards_check as rc
from cassie_amd import phys as P

NENV, INPUT_DIM, INPUT_STRIDE, LO, HI = 6, 70, 75, 0.12, 0.35
ENV_CUT, ENV_NAN = 4, 2
# the calls: (env0, n, reset) -- two over the batch, a sub-range that leaves envs 0, 4 and 5 alone, one that ends the episodes of envs 1
# and 4 first, a last one
SCHEDULE = ((0, 6, None), (0, 6, None), (1, 3, None), (0, 6, (0, 1, 0, 0, 1, 0)), (0, 6, None))
# input columns: 0..2 a commanded velocity | 3 a clock coefficient | 4..7 a target quaternion | 8..17 a reference pose | 6..69 stands
# for the actions (64 elements)


def terms_of(pod):
    assert pod.nq >= 17 and pod.nv >= 32 and pod.nsensordata >= 19
    IN = P.REW_INPUT
    return [
        # the base velocity in the body frame against the commanded one (ROT_INV, a target from the input, SUMSQ, EXP)
        P.rew_rot_inv(P.F_QVEL, 0, P.F_QPOS, 3, tfield=IN, tindex=0, shape=P.REW_EXP, k=2.0, weight=0.3),
        # the orientation against a constant and against the input's quaternion (QUAT; EXP and LINEAR)
        P.rew_quat(P.F_QPOS, 3, vec=(1.0, 0.0, 0.0, 0.0), shape=P.REW_EXP, k=3.0, weight=0.2),
        P.rew_quat(P.F_QPOS, 3, tfield=IN, tindex=4, weight=-0.1),
        # ten joints against the reference pose, gated by the clock (root of SUMSQ, EXP, a gate from the input)
        P.rew_vec(P.F_QPOS, 7, 10, tfield=IN, tindex=8, root=True, shape=P.REW_EXP, k=1.5, weight=0.25, gate=(IN, 3)),
        # the height against a constant through a deadband (count 1, SUMABS, RATIONAL)
        P.rew_vec(P.F_QPOS, 2, 1, target=0.9, dead=0.02, norm=P.REW_SUMABS, shape=P.REW_RATIONAL, k=10.0, weight=0.1),
        # the largest joint velocity (MAXABS, LINEAR: passes over the NaN), and its root through a RATIONAL
        P.rew_vec(P.F_QVEL, 6, 26, norm=P.REW_MAXABS, weight=-0.001),
        P.rew_vec(P.F_QVEL, 0, 3, norm=P.REW_MAXABS, root=True, shape=P.REW_RATIONAL, k=0.5, weight=0.05),
        # ten sensors against ten joint positions (a target from a field, root of SUMABS), and eight velocities (SUMABS: the NaN flows)
        P.rew_vec(P.F_SENSORDATA, 0, 10, tfield=P.F_QPOS, tindex=7, norm=P.REW_SUMABS, root=True, weight=-0.01),
        P.rew_vec(P.F_QVEL, 6, 8, norm=P.REW_SUMABS, weight=-0.002),
        # 64 elements of the input (the widest term), EXP
        P.rew_vec(IN, 6, 64, shape=P.REW_EXP, k=0.05, weight=0.05),
        # three sensors gated by a fourth (a gate from a batch field)
        P.rew_vec(P.F_SENSORDATA, 16, 3, weight=0.001, gate=(P.F_SENSORDATA, 5)),
        # the distance from the origin, steep: k s > 708 in env ENV_CUT
        P.rew_vec(P.F_QPOS, 0, 2, shape=P.REW_EXP, k=50.0, weight=0.1),
        # the projected gravity's horizontal part (ROT_INV of a constant vector, a deadband on three elements)
        P.rew_rot_inv(P.REW_CONST, 0, P.F_QPOS, 3, vec=(0.0, 0.0, -1.0), dead=0.05, norm=P.REW_SUMABS, shape=P.REW_RATIONAL, k=1.0, weight=0.05)]


def make_states(cassie, ncalls=len(SCHEDULE), nenv=NENV, seed=23):
    """One state per call: the observation case's states for nenv envs with env ENV_CUT moved 4 m from the origin and a NaN in env
    ENV_NAN's qvel[7], and the float32 input [nenv][INPUT_STRIDE] (INPUT_DIM columns bound) under P.REW_INPUT."""
    rng = np.random.default_rng(seed)
    states = []
    for s in obs_cases.make_states(cassie, ncalls, nenv):
        st = {f: s[f].copy() for f in (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA)}
        st[P.F_QPOS][ENV_CUT, 0] = 4.0
        st[P.F_QVEL][ENV_NAN, 7] = np.nan
        inp = rng.uniform(-1.0, 1.0, (nenv, INPUT_STRIDE)).astype(np.float32)
        inp[:, 8:18] = (st[P.F_QPOS][:, 7:17] + rng.uniform(-0.2, 0.2, (nenv, 10))).astype(np.float32)
        st[P.REW_INPUT] = inp
        states.append(st)
    return states


def reference(terms, states, dtype, schedule=SCHEDULE, nenv=NENV, lo=LO, hi=HI):
    """The rewards, term rows, returns and final returns after every call of the schedule by tests/rewards_check.py."""
    ref = rc.Rewards(terms, nenv, dtype, lo, hi)
    out = []
    for state, (env0, n, reset) in zip(states, schedule):
        ref.reward(state, env0, n, reset)
        out.append((ref.rew.copy(), ref.rows.copy(), ref.ret.copy(), ref.final.copy()))
    return out
