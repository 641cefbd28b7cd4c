"""The case the event rows are checked on, shared by the CPU test (tests/test_events.py: the wave emulator) and the GPU test
(tests/test_events_gpu.py: the device) -- test infrastructure only.  Seventy envs (one full wave and six), 64 columns that between them
use every kind, norm, op and polarity: a biped's chain on the contact forces of two feet (F_BODY_CFRC), measures of a float32 input with
a row stride, fillers up to a column at index 63 whose done bit is bit 63; fourteen calls over five ranges with reset words; sources that
ramp and jump across both thresholds, sit exactly on on_thr and off_thr and hold a NaN and both infinities in some envs; and what
tests/events_check.py makes of it."""
import numpy as np

import events_check as ec
from cassie_amd import phys as P

NENV, NCOLS, DT, ON_THR, OFF_THR = 70, 64, 0.025, 5.0, 2.0
INPUT_DIM, INPUT_STRIDE, ROW_PAD = 6, 9, 5
# the columns of the chain by name
(FL, FR, CL, CR, ONL, ONR, OFFL, OFFR, TDL, TDR, LOL, LOR, AIRL, AIRR, PEAKL, PEAKR, H, LOW, SA, MA, SQ, ENERGY, MINH, BOTH, NEITHER, CNT, SWL, ANYEDGE,
 FLIGHT, FLY_DONE, STANCEL) = range(31)
LAST = 63
DONE_MASK = (1 << FLY_DONE) | (1 << LAST)
ENV_NAN, ENV_PINF, ENV_NINF, ENV_NAN_IN = 5, 6, 7, 9
# the calls: (env0, n) -- the batch, a range that starts inside the first wave and ends inside the second, the second wave's six, the last
# env, the first env
RANGES = ((0, 70), (0, 70), (0, 70), (3, 64), (64, 6), (0, 70), (0, 70), (69, 1), (0, 1), (0, 70), (3, 64), (0, 70), (64, 6), (0, 70))
RESETS = {5: 0.2, 10: 0.25, 12: 0.4}     # the calls with reset words, and the share of their envs that start afresh
# a foot's force over eight calls: a ramp that sits on on_thr going up (on: >=) and on off_thr coming down (off: not >), and a square
RAMP = (0.0, 1.0, 2.0, 3.5, 5.0, 7.0, 2.0, 0.5)
SQUARE = (0.0, 0.0, 9.0, 9.0, 9.0, 0.0, 0.0, 9.0)


def feet(pod_or_model):
    """The two foot bodies and the pelvis of cassie (body ids)."""
    return pod_or_model.name2id(1, "left-foot"), pod_or_model.name2id(1, "right-foot"), pod_or_model.name2id(1, "cassie-pelvis")


def columns_of(lf, rf):
    IN, C = P.EV_INPUT, [None] * NCOLS
    C[FL] = P.ev_measure(P.F_BODY_CFRC, 3 * lf, 3, norm=P.EV_SUMSQ, root=True)
    C[FR] = P.ev_measure(P.F_BODY_CFRC, 3 * rf, 3, norm=P.EV_SUMSQ, root=True)
    C[CL], C[CR] = P.ev_level(FL, ON_THR, OFF_THR), P.ev_level(FR, ON_THR, OFF_THR)
    C[ONL], C[ONR] = P.ev_timer(CL, DT, 1), P.ev_timer(CR, DT, 1)
    C[OFFL], C[OFFR] = P.ev_timer(CL, DT, 0), P.ev_timer(CR, DT, 0)
    C[TDL], C[TDR] = P.ev_edge(CL, P.EV_RISING), P.ev_edge(CR, P.EV_RISING)
    C[LOL], C[LOR] = P.ev_edge(CL, P.EV_FALLING), P.ev_edge(CR, P.EV_FALLING)
    C[AIRL] = P.ev_latch(OFFL, TDL, lag=1)                                       # air time paid at touchdown
    C[AIRR] = P.ev_latch(OFFR, TDR, lag=1, keep=1, offset=-0.5, scale=2.0)       # ... shaped and held
    C[PEAKL] = P.ev_accum(FL, P.EV_MAX, clear=TDL)                               # the peak force of a stance
    C[PEAKR] = P.ev_accum(FR, P.EV_MAX, clear=TDR, gate=CR)
    C[H] = P.ev_measure(IN, 0, 1, target=0.9, norm=P.EV_SIGNED)
    C[LOW] = P.ev_level(H, 0.2, 0.1, sense=-1)                                   # the height below 0.7, until above 0.8
    C[SA] = P.ev_measure(IN, 1, 3, target=0.1, norm=P.EV_SUMABS)
    C[MA] = P.ev_measure(IN, 1, 3, norm=P.EV_MAXABS)
    C[SQ] = P.ev_measure(P.F_BODY_CFRC, 3 * lf, 3, norm=P.EV_SUMSQ)
    C[ENERGY] = P.ev_accum(SA, P.EV_SUM, clear=TDL, gate=CL)                     # a gated sum: a NaN sticks until the next touchdown
    C[MINH] = P.ev_accum(H, P.EV_MIN, init=10.0)
    C[BOTH], C[NEITHER], C[CNT] = P.ev_logic([CL, CR], P.EV_ALL), P.ev_logic([CL, CR], P.EV_NONE), P.ev_logic([CL, CR, LOW], P.EV_COUNT)
    C[SWL] = P.ev_edge(CL, P.EV_EITHER)
    C[ANYEDGE] = P.ev_logic([TDL, TDR, LOL, LOR], P.EV_ANY)
    C[FLIGHT] = P.ev_timer(NEITHER, DT, 1)
    C[FLY_DONE] = P.ev_level(FLIGHT, 3 * DT)                                     # both feet off for three calls
    C[STANCEL] = P.ev_latch(ONL, LOL, lag=0, keep=0, scale=-1.0)
    for k in range(STANCEL + 1, LAST):                                           # fillers: every kind but MEASURE on lower columns
        r = k % 5
        C[k] = (P.ev_accum(k - 20, P.EV_SUM, clear=TDR) if r == 0 else P.ev_timer(k - 25, DT, k % 2) if r == 1 else P.ev_edge(k - 29, P.EV_EITHER) if r == 2
                else P.ev_latch(k - 3, k - 1, lag=k % 2, keep=1) if r == 3 else P.ev_logic([k - 1, k - 2, k - 30], P.EV_COUNT))
    C[LAST] = P.ev_logic([LOW, LAST - 1], P.EV_ANY)
    return C


def make_calls(nbody, lf, rf, ncalls=len(RANGES), nenv=NENV, seed=41):
    """One (F_BODY_CFRC [nenv][3 nbody], float32 input [nenv][INPUT_STRIDE], reset words [n] or None) per call."""
    rng = np.random.default_rng(seed)
    calls = []
    e = np.arange(nenv)
    for k, (env0, n) in enumerate(RANGES[:ncalls]):
        cfrc = rng.uniform(-1.0, 1.0, (nenv, 3 * nbody))
        left = np.where(e % 3 == 0, np.take(SQUARE, (k + e) % 8), np.take(RAMP, (k + e) % 8))
        right = np.where(e % 4 == 1, np.take(SQUARE, (k + 3 * e + 4) % 8), np.take(RAMP, (k + 3 * e + 4) % 8))
        # even envs: the force along z alone, so the root of the sum of squares is the number itself and the thresholds are met exactly
        cfrc[:, 3 * lf:3 * lf + 3] = np.where((e % 2 == 0)[:, None], np.stack([0 * left, 0 * left, left], 1), np.stack([0.6 * left, 0.8 * left, 0 * left], 1))
        cfrc[:, 3 * rf:3 * rf + 3] = np.stack([0 * right, -right, 0 * right], 1)
        if k in (4, 5):
            cfrc[ENV_NAN, 3 * lf + 2] = np.nan
        if k == 3:
            cfrc[ENV_PINF, 3 * lf + 2] = np.inf
        if k == 6:
            cfrc[ENV_NINF, 3 * lf] = -np.inf
        inp = rng.uniform(-1.0, 1.0, (nenv, INPUT_STRIDE)).astype(np.float32)
        inp[:, 0] = (0.9 - 0.25 * np.abs(np.sin(0.7 * k + 0.3 * e))).astype(np.float32)      # a height that dips below 0.7 and comes back
        if k in (5, 6):
            inp[ENV_NAN_IN, 2] = np.nan
        reset = None
        if k in RESETS:
            reset = (rng.uniform(0.0, 1.0, n) < RESETS[k]).astype(np.int32) * np.int32(1 + k)   # (any non-zero word)
        calls.append((cfrc, inp, reset))
    return calls


def reference(cols, calls, dtype, nenv=NENV, done_mask=DONE_MASK, start=None, ranges=RANGES):
    """The rows, done words, state, words and counts after every call by tests/events_check.py; the calls are left unchanged."""
    ref = ec.Events(cols, nenv, dtype, done_mask)
    if start is not None:
        ref.state[:], ref.words[:], ref.counts[:] = start
    out = []
    for (cfrc, inp, reset), (env0, n) in zip(calls, ranges):
        ref.events({P.F_BODY_CFRC: cfrc, P.EV_INPUT: inp}, env0, n, reset)
        out.append((ref.rows.copy(), ref.flags.copy(), ref.state.copy(), ref.words.copy(), ref.counts.copy()))
    return out
