"""Python face of the inner C ABI (include/cassie_phys.h): Model and Batch.

``Batch`` is the batched, HBM-resident counterpart of the reference's one
``cassie_sim_t`` per process (reference example/cassiemujoco.py:31-72): N
environments stepped by one HIP launch.  All heavy lifting is in the shared
library; this module only moves numpy arrays across the boundary.
"""
import ctypes
import os

import numpy as np

from ._lib import CmDriveState, CmEnvParams, CmEpisodeRules, CmModel, MODEL_DIR, lib

# field ids (enum in cassie_phys.h)
(F_QPOS, F_QVEL, F_QACC_WARMSTART, F_TIME, F_CTRL, F_QFRC_APPLIED, F_XFRC_APPLIED, F_QACC, F_SENSORDATA,
 F_ACTUATOR_VELOCITY, F_XPOS, F_XQUAT, F_PD_PTARGET, F_PD_KP, F_PD_KD, F_BODY_CFRC, F_DRIVE_CMD, F_MEAS, F_PD_DTARGET,
 F_PD_TORQUE, F_DERIVED, F_QM, F_HEIGHT_SCAN, F_DEPTH, F_RAYS, F_STEP_SUMS, F_PROBES) = range(27)

# layout of the step-sums block F_STEP_SUMS (CM_SUM_* in cm_model.h): what a stepping launch added up over its substeps
# (Batch.enable_step_sums); MAXBODY = CM_MAXBODY, MAXU = CM_MAXU
MAXBODY, MAXU = 32, 12
SUM_COUNT, SUM_BODY_CFRC = 0, 1
SUM_BODY_TOUCH = SUM_BODY_CFRC + 3 * MAXBODY
SUM_BODY_CFRC_MAX2 = SUM_BODY_TOUCH + MAXBODY
SUM_ACT_FORCE = SUM_BODY_CFRC_MAX2 + MAXBODY
SUM_ACT_FORCE2 = SUM_ACT_FORCE + MAXU
SUM_ACT_POWER = SUM_ACT_FORCE2 + MAXU
SUM_ACT_POSPOWER = SUM_ACT_POWER + MAXU
SUM_DIM = SUM_ACT_POSPOWER + MAXU

# layout of the derived block F_DERIVED (CM_DRV_* in cm_model.h); MAXV = CM_MAXV
MAXV = 40
DRV_COM_POS, DRV_COM_VEL, DRV_ANGMOM, DRV_FOOT_POS, DRV_FOOT_VEL, DRV_FOOT_FORCE, DRV_TOE_FORCE, DRV_HEEL_FORCE, DRV_MASS = 0, 3, 6, 9, 15, 27, 39, 45, 51
DRV_FOOT_JACP, DRV_FOOT_JACR, DRV_DIM = 52, 52 + 6 * MAXV, 52 + 12 * MAXV

# drive modes (CM_DRIVE_* in cm_model.h) and the layout of the measurement block F_MEAS (CM_MEAS_*)
DRIVE_OFF, DRIVE_TORQUE, DRIVE_PD, DRIVE_PD_SAFE = 0, 1, 2, 3     # (PD_SAFE: + cassie_core_sim's safety layer, csrc/pk_safety.h)
SAFETY_MSG_LIMIT, SAFETY_MSG_TORQUE = 1, 2    # bits of cm_drive_state_t::safety_msg: diagnostic codes 635 / 630
MEAS_DRIVE_POS, MEAS_DRIVE_VEL, MEAS_DRIVE_TORQUE, MEAS_JOINT_POS, MEAS_JOINT_VEL = 0, 10, 20, 30, 36
MEAS_ORIENTATION, MEAS_ANGVEL, MEAS_LINACC, MEAS_MAG, MEAS_DIM = 42, 46, 49, 52, 56

FLAG_EULERDAMP, FLAG_WARMSTART, FLAG_REFSAFE, FLAG_HFDENSE, FLAG_HFMULTI, FLAG_HFPRISM, FLAG_BOX8 = 1, 2, 4, 8, 16, 32, 64      # CM_FLAG_* (cm_model.h)
WARN_CONTACT_FULL, WARN_CONSTRAINT_FULL, WARN_UNSUPPORTED_PAIR, WARN_DIVERGED = 1, 2, 4, 8
WARN_CHUNK_PLACEMENT = 16   # a chunk of a stepping launch found its predecessor on another XCD: the env's state may be stale, discard its results
WARN_TERRAIN_INDEX = 32     # the env's terrain index lay outside the bank and was clamped to it
WARN_SCAN_TILTED = 64       # height scan: the env's height-field geom is tilted out of the world's z axis and was left out
WARN_PLACE_MISS = 128       # placed restart: the footprint met no ground anywhere, the env was put down at ground_ref
SCAN_MAXPOINTS = 1024
DEPTH_MAXPIXELS = 16384
# range sensors on any body: the frames of a ray (PHYS_RAY_* in cassie_phys.h) and the layout of phys_ray_t
RAY_BODY, RAY_WORLD_DIR, RAY_HEADING = range(3)
RAYS_MAX = 1024
RAY_DTYPE = np.dtype([("body", np.int32), ("frame", np.int32), ("origin", np.float64, 3), ("dir", np.float64, 3)])
# probes: the kinds (PHYS_PROBE_* in cassie_phys.h), the layout of phys_probe_t, the quantities (PHYS_PQ_*: bits, in the order their
# blocks lie in a row; PQ_CONTACTS is the per-env word) with their names and shapes per probe (nv stands for the model's), and the
# bits of the contact word (PHYS_PC_*: PC_GROUP0 << g = a geom of group 1 touches one of group g, g = 0 .. 5)
PROBE_BODY, PROBE_SITE = range(2)
PROBES_MAX = 32
PROBE_DTYPE = np.dtype([("kind", np.int32), ("id", np.int32), ("offset", np.float64, 3)])
PQ_POS, PQ_QUAT, PQ_VEL, PQ_CVEL, PQ_ACC, PQ_JACP, PQ_JACR, PQ_CFRC, PQ_CONTACTS = (1 << k for k in range(9))
PQ_ALL = PQ_CONTACTS * 2 - 1
PQ_ROW = (("pos", (3,)), ("quat", (4,)), ("vel", (6,)), ("cvel", (6,)), ("acc", (6,)), ("jacp", (3, "nv")), ("jacr", (3, "nv")), ("cfrc", (3,)))
PC_OBSTACLE, PC_SELF, PC_GROUP0 = 1, 2, 256
# observation rows: the kinds of a term (PHYS_OBS_* in cassie_phys.h), the two sources that are no field of the batch, the layout of
# phys_obs_term_t and the limits
OBS_COPY, OBS_ROT_INV = range(2)
OBS_INPUT, OBS_CONST = -1, -2
OBS_MAXCOLS, OBS_MAXHISTORY, OBS_MAXROW = 2048, 64, 65536
OBS_TERM_DTYPE = np.dtype([("kind", np.int32), ("field", np.int32), ("index", np.int32), ("count", np.int32), ("qfield", np.int32),
                           ("qindex", np.int32), ("vec", np.float64, 3), ("offset", np.float64), ("scale", np.float64), ("noise", np.float64),
                           ("lo", np.float64), ("hi", np.float64)])


def obs_copy(field, index, count, offset=0.0, scale=1.0, noise=0.0, lo=-np.inf, hi=np.inf):
    """An OBS_TERM_DTYPE entry: count columns, field_row[index + j]."""
    return (OBS_COPY, int(field), int(index), int(count), 0, 0, (0.0, 0.0, 0.0), offset, scale, noise, lo, hi)


def obs_rot_inv(field, index, qfield, qindex, vec=(0.0, 0.0, 0.0), offset=0.0, scale=1.0, noise=0.0, lo=-np.inf, hi=np.inf):
    """An OBS_TERM_DTYPE entry: 3 columns, R(q)^T v with q = qfield_row[qindex : qindex + 4] and v = field_row[index : index + 3], or
    `vec` where field is OBS_CONST."""
    return (OBS_ROT_INV, int(field), int(index), 3, int(qfield), int(qindex), tuple(float(x) for x in vec), offset, scale, noise, lo, hi)


def obs_terms(terms):
    """A list of term tuples (obs_copy / obs_rot_inv) or a structured array -> OBS_TERM_DTYPE entries."""
    if isinstance(terms, np.ndarray) and terms.dtype.names:
        return np.ascontiguousarray(terms.astype(OBS_TERM_DTYPE, copy=False)).reshape(-1)
    terms = list(terms)
    table = np.zeros(len(terms), dtype=OBS_TERM_DTYPE)
    for k, t in enumerate(terms):
        table[k] = tuple(t[:6]) + (np.asarray(t[6], dtype=np.float64),) + tuple(t[7:])
    return table


def _obs_dtype(dtype):
    """numpy / torch float32 or float64 -> the bytes of an element (PHYS_OBS_F32 / PHYS_OBS_F64); anything else -> 0 (refused by the library)."""
    name = str(dtype).replace("torch.", "")
    try:
        name = np.dtype(dtype).name
    except TypeError:
        pass
    return {"float32": 4, "float64": 8}.get(name, 0)


# reward rows: the kinds, norms and shapes of a term (PHYS_REW_* in cassie_phys.h), what is no field of the batch, the layout of
# phys_reward_term_t and the limits
REW_VEC, REW_ROT_INV, REW_QUAT = range(3)
REW_SUMSQ, REW_SUMABS, REW_MAXABS = range(3)
REW_LINEAR, REW_EXP, REW_RATIONAL = range(3)
REW_INPUT, REW_CONST, REW_NONE = -1, -2, -3
REW_MAXTERMS, REW_MAXCOUNT = 64, 64
REW_TERM_DTYPE = np.dtype([("kind", np.int32), ("field", np.int32), ("index", np.int32), ("count", np.int32), ("qfield", np.int32), ("qindex", np.int32),
                           ("tfield", np.int32), ("tindex", np.int32), ("gfield", np.int32), ("gindex", np.int32), ("norm", np.int32), ("shape", np.int32),
                           ("root", np.int32), ("vec", np.float64, 4), ("target", np.float64), ("dead", np.float64), ("k", np.float64), ("weight", np.float64)],
                          align=True)


def _rew(kind, field, index, count, qfield, qindex, tfield, tindex, gate, norm, shape, root, vec, target, dead, k, weight):
    gfield, gindex = (REW_NONE, 0) if gate is None else gate
    vec = tuple(float(x) for x in vec) + (0.0,) * (4 - len(vec))
    return (int(kind), int(field), int(index), int(count), int(qfield), int(qindex), int(tfield), int(tindex), int(gfield), int(gindex), int(norm), int(shape),
            int(bool(root)), vec, float(target), float(dead), float(k), float(weight))


def rew_vec(field, index, count, target=0.0, tfield=REW_CONST, tindex=0, dead=0.0, norm=REW_SUMSQ, root=False, shape=REW_LINEAR, k=0.0, weight=1.0, gate=None):
    """A REW_TERM_DTYPE entry: the error of field_row[index : index + count] against `target` (or tfield_row[tindex : tindex + count]),
    through the deadband, the norm, the root and the shape, times weight and the gate (gfield, gindex)."""
    return _rew(REW_VEC, field, index, count, 0, 0, tfield, tindex, gate, norm, shape, root, (), target, dead, k, weight)


def rew_rot_inv(field, index, qfield, qindex, vec=(0.0, 0.0, 0.0), target=0.0, tfield=REW_CONST, tindex=0, dead=0.0, norm=REW_SUMSQ, root=False,
                shape=REW_LINEAR, k=0.0, weight=1.0, gate=None):
    """A REW_TERM_DTYPE entry: the three elements R(q)^T v, q = qfield_row[qindex : qindex + 4], v = field_row[index : index + 3] or `vec`
    where field is REW_CONST, then as rew_vec."""
    return _rew(REW_ROT_INV, field, index, 3, qfield, qindex, tfield, tindex, gate, norm, shape, root, vec, target, dead, k, weight)


def rew_quat(field, index, tfield=REW_CONST, tindex=0, vec=(1.0, 0.0, 0.0, 0.0), shape=REW_LINEAR, k=0.0, weight=1.0, gate=None):
    """A REW_TERM_DTYPE entry: s = 1 - (q . t)^2 with q = field_row[index : index + 4] and t = tfield_row[tindex : tindex + 4] or `vec`
    where tfield is REW_CONST, then the shape, the weight and the gate."""
    return _rew(REW_QUAT, field, index, 4, 0, 0, tfield, tindex, gate, REW_SUMSQ, shape, False, vec, 0.0, 0.0, k, weight)


def rew_terms(terms):
    """A list of term tuples (rew_vec / rew_rot_inv / rew_quat) or a structured array -> REW_TERM_DTYPE entries."""
    if isinstance(terms, np.ndarray) and terms.dtype.names:
        return np.ascontiguousarray(terms.astype(REW_TERM_DTYPE, copy=False)).reshape(-1)
    terms = list(terms)
    table = np.zeros(len(terms), dtype=REW_TERM_DTYPE)
    for i, t in enumerate(terms):
        table[i] = tuple(t[:13]) + (np.asarray(t[13], dtype=np.float64),) + tuple(t[14:])
    return table


# action rows: what is no field of the batch in a column's bfield / dfield (PHYS_ACT_* in cassie_phys.h), the frames of an action row, the
# layout of phys_act_col_t, the limits and the fields a column may write
ACT_INPUT, ACT_CONST, ACT_NONE = -1, -2, -3
ACT_NOW, ACT_PREV, ACT_APPLIED = range(3)
ACT_MAXCOLS, ACT_MAXDELAY = 256, 8
ACT_COL_DTYPE = np.dtype([("bfield", np.int32), ("bindex", np.int32), ("dfield", np.int32), ("dindex", np.int32), ("lo", np.float64), ("hi", np.float64),
                          ("noise", np.float64), ("smooth", np.float64), ("offset", np.float64), ("scale", np.float64), ("out_lo", np.float64),
                          ("out_hi", np.float64)])
ACT_CMD_FIELDS = (F_PD_PTARGET, F_PD_DTARGET, F_PD_KP, F_PD_KD, F_PD_TORQUE, F_DRIVE_CMD, F_CTRL, F_QFRC_APPLIED, F_XFRC_APPLIED)


def act_col(dfield=ACT_NONE, dindex=0, lo=-np.inf, hi=np.inf, noise=0.0, smooth=1.0, bfield=ACT_CONST, bindex=0, offset=0.0, scale=1.0,
            out_lo=-np.inf, out_hi=np.inf):
    """An ACT_COL_DTYPE entry: the action clipped to [lo, hi], noisy, delayed and low-passed (y), then offset (+ bfield_row[bindex]) +
    scale * y clipped to [out_lo, out_hi] into dfield_row[dindex] (ACT_NONE: a column that is only tracked)."""
    return (int(bfield), int(bindex), int(dfield), int(dindex), lo, hi, noise, smooth, offset, scale, out_lo, out_hi)


def act_cols(cols):
    """A list of column tuples (act_col) or a structured array -> ACT_COL_DTYPE entries."""
    if isinstance(cols, np.ndarray) and cols.dtype.names:
        return np.ascontiguousarray(cols.astype(ACT_COL_DTYPE, copy=False)).reshape(-1)
    cols = list(cols)
    table = np.zeros(len(cols), dtype=ACT_COL_DTYPE)
    for k, t in enumerate(cols):
        table[k] = tuple(t)
    return table


# task rows: the kinds of a column and the forms of a WAVE (PHYS_TASK_* in cassie_phys.h), what is no destination, the layout of
# phys_task_col_t and the limits
TASK_SAMPLE, TASK_PHASE, TASK_WAVE, TASK_TABLE = range(4)
TASK_SAW, TASK_SIN, TASK_COS, TASK_TRAPEZOID = range(4)
TASK_NONE = ACT_NONE
TASK_MAXCOLS, TASK_MAXFRAMES, TASK_MAXTCOLS, TASK_MAXPERIOD = 64, 4096, 64, 1 << 30
TASK_COL_DTYPE = np.dtype([(k, np.int32) for k in ("kind", "form", "group", "rate_col", "phase_col", "src", "tcol", "dfield", "dindex")] +
                          [(k, np.uint32) for k in ("period_lo", "period_hi", "hold")] +
                          [(k, np.float64) for k in ("center", "half", "rest", "p_rest", "rate", "rate_scale", "phase0", "shift", "duty", "ramp", "offset", "scale")])


def _task_col(kind, **kw):
    col = dict(kind=kind, form=0, group=-1, rate_col=-1, phase_col=-1, src=-1, tcol=0, dfield=TASK_NONE, dindex=0, period_lo=1, period_hi=1, hold=0,
               center=0.0, half=0.0, rest=0.0, p_rest=0.0, rate=0.0, rate_scale=0.0, phase0=0.0, shift=0.0, duty=0.0, ramp=0.0, offset=0.0, scale=1.0)
    col.update(kw)
    return tuple(col[k] for k in TASK_COL_DTYPE.names)


def task_sample(center=0.0, half=0.0, period_lo=1, period_hi=None, rest=0.0, p_rest=0.0, hold=0, group=-1, dfield=TASK_NONE, dindex=0):
    """A TASK_COL_DTYPE entry: a value center + half * uniform(-1, 1), or `rest` with probability p_rest, held for period_lo ..
    period_hi calls (shown for the first `hold` of them, then `rest`; 0: all).  group: the SAMPLE column whose schedule it shares
    (-1: its own).  dfield, dindex: a command-field element that gets the value too (TASK_NONE: none)."""
    return _task_col(TASK_SAMPLE, center=center, half=half, period_lo=period_lo, period_hi=period_lo if period_hi is None else period_hi, rest=rest,
                     p_rest=p_rest, hold=hold, group=group, dfield=dfield, dindex=dindex)


def task_phase(rate=0.0, rate_col=-1, rate_scale=1.0, phase0=0.0, phase_col=-1, dfield=TASK_NONE, dindex=0):
    """A clock in [0, 1): advanced by rate (+ rate_scale * the SAMPLE column rate_col) cycles per call, started at phase0 or at the SAMPLE
    column phase_col."""
    return _task_col(TASK_PHASE, rate=rate, rate_col=rate_col, rate_scale=rate_scale, phase0=phase0, phase_col=phase_col, dfield=dfield, dindex=dindex)


def task_wave(src, form=TASK_SIN, shift=0.0, offset=0.0, scale=1.0, duty=0.0, ramp=0.0, dfield=TASK_NONE, dindex=0):
    """offset + scale * g(wrap(phase of the PHASE column src + shift)), g the form: TASK_SAW, TASK_SIN, TASK_COS (of 2 pi theta) or
    TASK_TRAPEZOID (0 at 0, 1 on [ramp, duty], 0 from duty + ramp on)."""
    return _task_col(TASK_WAVE, src=src, form=form, shift=shift, offset=offset, scale=scale, duty=duty, ramp=ramp, dfield=dfield, dindex=dindex)


def task_table(src, tcol, shift=0.0, offset=0.0, scale=1.0, dfield=TASK_NONE, dindex=0):
    """offset + scale * column tcol of the periodic table (Batch.set_task_table), linearly interpolated at wrap(phase of src + shift)."""
    return _task_col(TASK_TABLE, src=src, tcol=tcol, shift=shift, offset=offset, scale=scale, dfield=dfield, dindex=dindex)


def task_cols(cols):
    """A list of column tuples (task_sample, task_phase, task_wave, task_table) or a structured array -> TASK_COL_DTYPE entries."""
    if isinstance(cols, np.ndarray) and cols.dtype.names:
        return np.ascontiguousarray(cols.astype(TASK_COL_DTYPE, copy=False)).reshape(-1)
    cols = list(cols)
    table = np.zeros(len(cols), dtype=TASK_COL_DTYPE)
    for k, t in enumerate(cols):
        table[k] = tuple(t)
    return table


# event rows: the kinds of a column, a MEASURE's norms and the ops of an EDGE, an ACCUM and a LOGIC (PHYS_EV_* in cassie_phys.h), what is
# no field of the batch, the layout of phys_event_col_t and the limits
EV_MEASURE, EV_LEVEL, EV_TIMER, EV_EDGE, EV_LATCH, EV_ACCUM, EV_LOGIC = range(7)
EV_SIGNED, EV_SUMABS, EV_SUMSQ, EV_MAXABS = range(4)
EV_RISING, EV_FALLING, EV_EITHER = range(3)
EV_MAX, EV_MIN, EV_SUM = range(3)
EV_ANY, EV_ALL, EV_NONE, EV_COUNT = range(4)
EV_INPUT = -1
EV_MAXCOLS, EV_MAXCOUNT = 64, 8
EV_COL_DTYPE = np.dtype([(k, np.int32) for k in ("kind", "field", "index", "count", "norm", "root", "src", "trig", "clear", "gate", "op", "sense", "polarity",
                                                 "lag", "keep", "pad")] + [("mask", np.uint64)] +
                        [(k, np.float64) for k in ("target", "on_thr", "off_thr", "dt", "offset", "scale", "init")])


def _ev_col(kind, **kw):
    col = dict(kind=kind, field=0, index=0, count=1, norm=0, root=0, src=-1, trig=-1, clear=-1, gate=-1, op=0, sense=1, polarity=1, lag=0, keep=0, pad=0,
               mask=0, target=0.0, on_thr=0.0, off_thr=0.0, dt=0.0, offset=0.0, scale=1.0, init=0.0)
    col.update(kw)
    return tuple(col[k] for k in EV_COL_DTYPE.names)


def ev_measure(field, index, count=1, target=0.0, norm=EV_SIGNED, root=False):
    """An EV_COL_DTYPE entry: a number from field_row[index : index + count] (count 1 .. 8) minus `target`, through the norm EV_SIGNED
    (count 1), EV_SUMABS, EV_SUMSQ (root: its square root) or EV_MAXABS.  field: an F_* field or EV_INPUT (Batch.bind_event_input)."""
    return _ev_col(EV_MEASURE, field=int(field), index=int(index), count=int(count), target=float(target), norm=int(norm), root=int(bool(root)))


def ev_level(src, on_thr, off_thr=None, sense=1):
    """A Schmitt trigger on column src: on from sense * value >= on_thr until it is no longer > off_thr (default: on_thr)."""
    return _ev_col(EV_LEVEL, src=int(src), on_thr=float(on_thr), off_thr=float(on_thr if off_thr is None else off_thr), sense=int(sense))


def ev_timer(src, dt, polarity=1):
    """dt times the consecutive calls column src has been on (polarity 0: off)."""
    return _ev_col(EV_TIMER, src=int(src), dt=float(dt), polarity=int(polarity))


def ev_edge(src, which=EV_RISING):
    """1 on the call on which column src switched on (EV_RISING), off (EV_FALLING) or either way (EV_EITHER)."""
    return _ev_col(EV_EDGE, src=int(src), op=int(which))


def ev_latch(src, trig, lag=0, keep=0, offset=0.0, scale=1.0):
    """offset + scale * column src (lag 1: its value on the call before), taken when column trig is on; shown on that call alone, or
    with keep=1 until the next one."""
    return _ev_col(EV_LATCH, src=int(src), trig=int(trig), lag=int(lag), keep=int(keep), offset=float(offset), scale=float(scale))


def ev_accum(src, op=EV_MAX, clear=-1, gate=-1, init=0.0):
    """The running EV_MAX, EV_MIN or EV_SUM of column src from `init`, restarted when column clear is on, fed while column gate is on."""
    return _ev_col(EV_ACCUM, src=int(src), op=int(op), clear=int(clear), gate=int(gate), init=float(init))


def ev_logic(cols, op=EV_ANY):
    """EV_ANY, EV_ALL, EV_NONE or EV_COUNT of the lower columns `cols` (a list of indices, or a uint64 mask) that are on."""
    mask = int(cols) if isinstance(cols, (int, np.integer)) else sum(1 << int(k) for k in set(cols))
    return _ev_col(EV_LOGIC, mask=mask, op=int(op))


def ev_cols(cols):
    """A list of column tuples (ev_measure ... ev_logic) or a structured array -> EV_COL_DTYPE entries."""
    if isinstance(cols, np.ndarray) and cols.dtype.names:
        return np.ascontiguousarray(cols.astype(EV_COL_DTYPE, copy=False)).reshape(-1)
    cols = list(cols)
    table = np.zeros(len(cols), dtype=EV_COL_DTYPE)
    for k, t in enumerate(cols):
        table[k] = tuple(t)
    return table

# policy rows: a layer's activations (PHYS_POL_* in cassie_phys.h), the limits and the layout of phys_pol_net_t
POL_IDENTITY, POL_RELU, POL_ELU, POL_TANH = range(4)
POL_MAXNETS, POL_MAXLAYERS, POL_MAXDIM, POL_MAXOUT = 2, 4, 512, 64
POL_NET_DTYPE = np.dtype([("nlayers", np.int32), ("layer", np.int32, (POL_MAXLAYERS, 3))])   # a layer: (in, out, act)


def pol_layer(out, act=POL_IDENTITY):
    """A dense layer of `out` units with an activation POL_IDENTITY, POL_RELU, POL_ELU or POL_TANH; what it reads is the width of the layer
    before it (the first: in_dim)."""
    return (int(out), int(act))


def pol_nets(nets, in_dim):
    """A list of networks, each a list of pol_layer(...) (or of (in, out, act) triples, taken as written) -> POL_NET_DTYPE entries."""
    nets = list(nets)
    table = np.zeros(max(len(nets), 1), dtype=POL_NET_DTYPE)
    for a, layers in enumerate(nets[:POL_MAXNETS]):
        layers, width = list(layers), int(in_dim)
        table[a]["nlayers"] = len(layers)
        for l, L in enumerate(layers[:POL_MAXLAYERS]):
            table[a]["layer"][l] = (width, int(L[0]), int(L[1])) if len(L) == 2 else tuple(int(v) for v in L)
            width = int(table[a]["layer"][l][1])
    return table


# rollout rows: the roles of a source and of the arrays (PHYS_RO_* in cassie_phys.h: numbered from RO_MAXSRC, so that one int names a source by
# index or by role), the limits and the layout of phys_rollout_src_t
(RO_DATA, RO_OBS, RO_ACTION, RO_LOGP, RO_MU, RO_VALUE, RO_REWARD, RO_DONE, RO_REASON, RO_ADV, RO_RET, RO_ADVN) = range(16, 28)
RO_MAXT, RO_MAXSRC, RO_MAXDIM = 1024, 16, 4096
RO_SRC_DTYPE = np.dtype([("role", np.int32), ("dim", np.int32)])
RO_NAMES = {"data": RO_DATA, "obs": RO_OBS, "action": RO_ACTION, "logp": RO_LOGP, "mu": RO_MU, "value": RO_VALUE, "reward": RO_REWARD,
            "done": RO_DONE, "reason": RO_REASON, "adv": RO_ADV, "ret": RO_RET, "advn": RO_ADVN}
RO_INT_ROLES = (RO_DONE, RO_REASON)      # int32 words; every other role reads as float32


def ro_srcs(srcs):
    """A list of (role, dim) pairs -> RO_SRC_DTYPE entries."""
    srcs = list(srcs)
    table = np.zeros(max(len(srcs), 1), dtype=RO_SRC_DTYPE)
    for k, (role, dim) in enumerate(srcs):
        table[k] = (RO_NAMES.get(role, role) if isinstance(role, str) else int(role), int(dim))
    return table


# gradient rows: what Batch.grad_download names (PHYS_GRAD_* in cassie_phys.h), the chunk's limits, the count of statistics and their names
(GRAD_DW, GRAD_DB, GRAD_DLS, GRAD_ACT, GRAD_DELTA, GRAD_PARTIAL, GRAD_PACKT) = range(7)
GRAD_MINCHUNK, GRAD_MAXCHUNK, GRAD_NSTATS = 16, 4096, 8
GRAD_STATS = ("policy_loss", "value_loss", "kl", "clipped", "entropy", "void", "m", "spare")

# optimiser rows: what Batch.opt_download / opt_upload name (PHYS_OPT_* in cassie_phys.h), the NORM's segment, the statistics and their names
(OPT_M_W, OPT_M_B, OPT_V_W, OPT_V_B, OPT_M_LS, OPT_V_LS, OPT_SCALARS, OPT_PARTIALS) = range(8)
OPT_SEG, OPT_NSTATS = 256, 8
OPT_STATS = ("norm", "scale", "skip", "t", "skipped", "lr", "p1", "p2")

# normaliser rows: what Batch.norm_download / norm_upload name (PHYS_NORM_* in cassie_phys.h), the limits, the statistics and their names
(NORM_N, NORM_MEAN, NORM_M2, NORM_SKIPPED, NORM_EXCLUDED, NORM_MB, NORM_COUNTS, NORM_PARTIALS) = range(8)
NORM_MINBLOCK, NORM_MAXBLOCK, NORM_MAXROWS, NORM_NSTATS = 16, 4096, 1 << 30, 8
NORM_STATS = ("rows", "blocks", "updated", "skipped", "excluded", "calls", "n_max", "spare")

# draw rows: the limits (PHYS_DRAW_* in cassie_phys.h)
DRAW_MAXA, DRAW_MAXPERM = 64, 1 << 30


# per-env physical parameters (CM_P_* in cm_model.h): what Batch.randomize takes
(P_BODY_MASS, P_BODY_IPOS, P_BODY_INERTIA, P_DOF_DAMPING, P_GEOM_FRICTION,
 P_GEOM_POS, P_GEOM_QUAT, P_JNT_STIFFNESS, P_QPOS_SPRING) = range(9)
# views of the host model's arrays (PHYS_M_* in cassie_phys.h) that Model.array hands out
(M_BODY_MASS, M_BODY_IPOS, M_BODY_POS, M_BODY_QUAT, M_DOF_DAMPING, M_JNT_STIFFNESS, M_QPOS_SPRING, M_GEOM_POS, M_GEOM_QUAT,
 M_GEOM_SIZE, M_GEOM_FRICTION, M_ACTUATOR_GEAR, M_ACTUATOR_CTRLRANGE, M_ACTUATOR_USER, M_SENSOR_USER, M_HFIELD_SIZE, M_TIMESTEP,
 M_QPOS0, M_JNT_RANGE, M_STAT_CENTER, M_STAT_EXTENT, M_GEOM_USER, M_BODY_INERTIA) = range(23)
SIZE_NGEOM = 5               # PHYS_NGEOM: geoms in the host model's full list
# episodes on the device: bits of an env's reason word (CM_DONE_* in cm_model.h) and the per-env arrays (PHYS_EP_* in cassie_phys.h)
DONE_HEIGHT, DONE_UPRIGHT, DONE_TIME, DONE_WARN, DONE_NONFINITE, DONE_FORCED = 1, 2, 4, 8, 16, 32
EP_DONE, EP_REASON, EP_STEPS, EP_COUNT, EP_TERMINAL = range(5)
# placed restarts: the per-env arrays (PHYS_PLACE_* in cassie_phys.h)
PLACE_POSE, PLACE_NEXT_TERRAIN, PLACE_GROUND = range(3)
PLACE_MAXPOINTS = 1024
# the bank of full states: the groups of a row (PHYS_STATE_* in cassie_phys.h), the warning bit of a slot outside the bank, and the
# sections of a row in the order of PHYS_SS_*, each with the dtype its words are read as (int32 sections hold one value, zero-extended
# to a word; the drive-level state and the parameter block are the bytes of cm_drive_state_t / cm_envparams_t)
STATE_CORE, STATE_COMMANDS, STATE_EPISODE, STATE_PARAMS = 1, 2, 4, 8
WARN_STATE_SLOT = 256       # save_states / restore_states: the env's slot lay outside the bank, nothing was copied
STATE_SECTIONS = (("time", np.float64), ("qpos", np.float64), ("qvel", np.float64), ("qacc_warmstart", np.float64), ("ctrl", np.float64),
                  ("qacc", np.float64), ("sensordata", np.float64), ("actuator_velocity", np.float64), ("meas", np.float64),
                  ("drive_state", np.uint8), ("xpos", np.float64), ("xquat", np.float64), ("warn", np.int32),
                  ("pd_ptarget", np.float64), ("pd_kp", np.float64), ("pd_kd", np.float64), ("pd_dtarget", np.float64), ("pd_torque", np.float64),
                  ("drive_cmd", np.float64), ("qfrc_applied", np.float64), ("xfrc_applied", np.float64),
                  ("ep_steps", np.int32), ("ep_count", np.int32), ("terrain", np.int32), ("params", np.uint8))

# joint configuration the reference writes at init (reference src/cassiemujoco.c:1023-1028)
QPOS_INIT_JOINTS = np.array(
    [0.0045, 0, 0.4973, 0.9785, -0.0164, 0.01787, -0.2049, -1.1997, 0, 1.4267, 0, -1.5244, 1.5244, -1.5968,
     -0.0045, 0, 0.4973, 0.9786, 0.00386, -0.01524, -0.2051, -1.1997, 0, 1.4267, 0, -1.5244, 1.5244, -1.5968])


def model_path(name):
    """Resolves 'cassie' / 'cassie_hfield' / 'cassie_tray_box' (or a path) to a loadable model file."""
    if os.path.exists(name):
        return name
    p = os.path.join(MODEL_DIR, name + ".cmodel")
    if os.path.exists(p):
        return p
    raise FileNotFoundError("no model file for %r (looked in %s)" % (name, MODEL_DIR))


class Model:
    """Host model (names, all geoms, ...) plus its compiled pointer-free form ``.pod`` (cm_model_t)."""

    def __init__(self, path_or_name="cassie"):
        L = lib()
        err = ctypes.create_string_buffer(1024)
        self.name = os.path.splitext(os.path.basename(str(path_or_name)))[0]   # "cassie", "cassie_hfield", ...
        self._h = L.phys_model_load(model_path(path_or_name).encode(), err, len(err))
        if not self._h:
            raise RuntimeError("model load failed: " + err.value.decode())
        self.pod = CmModel()
        self.compile()

    def compile(self):
        err = ctypes.create_string_buffer(1024)
        if lib().phys_model_compile(self._h, ctypes.byref(self.pod), err, len(err)) != 0:
            raise RuntimeError("model compile failed: " + err.value.decode())
        return self.pod

    def set_const(self):
        lib().phys_model_set_const(self._h)
        self.compile()

    def set_flag(self, flag, on=True):
        """Option flag of the model (CM_FLAG_*: FLAG_HFDENSE = denser capsule sampling against height fields); recompiles."""
        if lib().phys_model_set_flag(self._h, int(flag), 1 if on else 0) != 0:
            raise RuntimeError("bad model flag")
        self.compile()

    def save(self, path):
        if lib().phys_model_save(self._h, path.encode()) != 0:
            raise RuntimeError("cannot write " + path)

    def array(self, which, n):
        """Read-write numpy view of `n` doubles of a host-model array (M_*: the mjModel arrays the reference's setters write);
        follow edits of masses / inertial frames with set_const(), of anything with compile()."""
        p = lib().phys_model_array(self._h, int(which))
        if not p:
            raise ValueError("no such model array")
        return np.ctypeslib.as_array(p, shape=(int(n),))

    def name2id(self, objtype, name):
        return lib().phys_model_name2id(self._h, objtype, name.encode())

    def size(self, what):
        return lib().phys_model_size(self._h, what)

    def qpos_init(self):
        """The state cassie_sim_init leaves the robot in (qpos0 with the nominal joint pose)."""
        q = np.array(self.pod.qpos0[: self.pod.nq])
        q[7:35] = QPOS_INIT_JOINTS
        return q

    def __del__(self):
        try:
            if self._h:
                lib().phys_model_free(self._h)
                self._h = None
        except Exception:
            pass


class Batch:
    """N environments resident in HBM on one MI355X."""

    def __init__(self, model, nenv, device=0):
        self.model = model
        self.nenv = int(nenv)
        pod = model.pod if isinstance(model, Model) else model
        self.pod = pod
        self.device = int(device)
        self._h = lib().phys_batch_create(ctypes.byref(pod), self.nenv, device)
        if not self._h:
            raise RuntimeError("phys_batch_create failed: " + (lib().phys_last_error() or b"").decode())

    def dim(self, field):
        return lib().phys_batch_field_dim(self._h, field)

    def set(self, field, arr, env0=0):
        a = np.ascontiguousarray(arr, dtype=np.float64).reshape(-1, self.dim(field))
        if lib().phys_batch_upload(self._h, field, a.ctypes.data, env0, a.shape[0]) != 0:
            raise RuntimeError("upload failed: " + (lib().phys_last_error() or b"").decode())

    def get(self, field, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        out = np.empty((n, self.dim(field)), dtype=np.float64)
        if lib().phys_batch_download(self._h, field, out.ctypes.data, env0, n) != 0:
            raise RuntimeError("download failed: " + (lib().phys_last_error() or b"").decode())
        return out

    def warnings(self):
        w = np.zeros(self.nenv, dtype=np.int32)
        info = np.zeros((self.nenv, 4), dtype=np.int32)
        if lib().phys_batch_download_warn(self._h, w.ctypes.data, info.ctypes.data) != 0:
            raise RuntimeError("download failed")
        return w, info

    def device_ptr(self, field):
        return lib().phys_batch_device_ptr(self._h, field)

    def bind(self, field, device_ptr, row_stride=None):
        """Aliases a field to caller-owned HBM; `row_stride` (doubles, qpos / qvel / sensordata / the height scan / the depth image / the ray ranges only) lets the field be a
        column block of a wider tensor, e.g. one [nenv][nq + nv + nsensordata] observation block."""
        rc = (lib().phys_batch_bind(self._h, field, device_ptr) if row_stride is None
              else lib().phys_batch_bind_strided(self._h, field, device_ptr, int(row_stride)))
        if rc != 0:
            raise RuntimeError("bind failed: " + (lib().phys_last_error() or b"").decode())

    def clear_warnings(self, env0=0, n=None):
        if lib().phys_batch_clear_warn(self._h, env0, self.nenv - env0 if n is None else n) != 0:
            raise RuntimeError("clear_warn failed")

    def param_dim(self, param):
        return lib().phys_batch_param_dim(self._h, int(param))

    def randomize(self, param, values, env0=0, device_ptr=None, n=None, stream=None):
        """Per-env physical parameters (P_BODY_MASS [nbody], P_BODY_IPOS [nbody*3], P_BODY_INERTIA [nbody*3], P_DOF_DAMPING [nv],
        P_GEOM_FRICTION [pod.ngeom*3], P_GEOM_POS [pod.ngeom*3], P_GEOM_QUAT [pod.ngeom*4], P_JNT_STIFFNESS [njnt],
        P_QPOS_SPRING [nq]; geoms are the collision geoms in compiled order, pod.geom_fullid maps them to the full list) for envs
        env0 ...: `values` is a host array [n][dim], or pass `device_ptr` and n to read rows that are already in HBM (a torch
        tensor's data_ptr()).  Masses / inertial offsets / inertias: follow with set_const().  Geometry (unit quaternions
        expected: they are not normalised) and springs act from the next step on with no set_const().
        The rows are written in order on `stream` (default: the batch's own): ranges stepped on other streams must be joined
        with it first."""
        if device_ptr is not None:
            if n is None:
                raise ValueError("randomize: device_ptr needs n, the number of rows to read")
            rc = lib().phys_batch_randomize(self._h, int(param), device_ptr, 1, int(env0), int(n), stream)
        else:
            a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1, self.param_dim(param))
            rc = lib().phys_batch_randomize(self._h, int(param), a.ctypes.data, 0, int(env0), a.shape[0], stream)
        if rc != 0:
            raise RuntimeError("randomize failed: " + (lib().phys_last_error() or b"").decode())

    def set_const(self, env0=0, n=None, stream=None):
        """mj_setConst per env on the device: inverse weights and mean inertia from every env's own masses / inertial frames."""
        if lib().phys_batch_set_const(self._h, int(env0), self.nenv - env0 if n is None else int(n), stream) != 0:
            raise RuntimeError("set_const failed: " + (lib().phys_last_error() or b"").decode())

    def params(self, env0=0, n=None):
        """The envs' parameter blocks (ctypes array of CmEnvParams), downloaded."""
        n = self.nenv - env0 if n is None else n
        out = (CmEnvParams * n)()
        if lib().phys_batch_download_params(self._h, ctypes.byref(out), int(env0), int(n)) != 0:
            raise RuntimeError("parameter download failed")
        return out

    def set_model(self, pod, env=-1):
        if lib().phys_batch_set_model(self._h, ctypes.byref(pod), env) != 0:
            raise RuntimeError("set_model failed: " + (lib().phys_last_error() or b"").decode())

    def step(self, nsub=1, stream=None):
        if lib().phys_batch_step(self._h, nsub, stream) != 0:
            raise RuntimeError("step failed: " + (lib().phys_last_error() or b"").decode())

    def step_range(self, env0, n, nsub=1, stream=None):
        """Steps the env range [env0, env0 + n) only; ranges may be in flight on different streams at once."""
        if lib().phys_batch_step_range(self._h, int(env0), int(n), nsub, stream) != 0:
            raise RuntimeError("step_range failed: " + (lib().phys_last_error() or b"").decode())

    def forward(self, stream=None):
        if lib().phys_batch_forward(self._h, stream) != 0:
            raise RuntimeError("forward failed: " + (lib().phys_last_error() or b"").decode())

    def forward_kinematics(self, stream=None):
        """The forward pass with qacc / sensordata / actuator_velocity sent to scratch: refreshes F_XPOS / F_XQUAT (and the other
        position-level outputs) from qpos and leaves the fields a policy reads alone.  Not in a drive mode."""
        if lib().phys_batch_forward_kinematics(self._h, stream) != 0:
            raise RuntimeError("forward_kinematics failed: " + (lib().phys_last_error() or b"").decode())

    def set_hfield(self, data, env=None):
        """Height-field samples for all envs (env=None, one shared grid) or for one env only (per-env terrain)."""
        a = np.ascontiguousarray(data, dtype=np.float32)
        ptr = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        rc = lib().phys_batch_set_hfield(self._h, ptr, a.size) if env is None else lib().phys_batch_set_hfield_env(self._h, int(env), ptr, a.size)
        if rc != 0:
            raise RuntimeError("set_hfield failed")

    # ---- a bank of terrains shared by the envs, a per-env index, and the height scan ----
    def set_hfield_bank(self, grids=None, device_ptr=None, nterrain=None):
        """A bank of terrains: host `grids` [T][nrow * ncol] (or [T][nrow][ncol]) float32, or `device_ptr` and nterrain for grids that
        are already in HBM (a torch tensor's data_ptr(): float32, contiguous).  The batch keeps a copy.  Every env starts on terrain 0;
        set_terrain / the terrain index choose per env.  set_hfield afterwards returns to one shared grid or per-env grids."""
        n = self.pod.hfield_nrow * self.pod.hfield_ncol
        if self.pod.hfield_geom < 0 or n <= 0:
            raise ValueError("set_hfield_bank: the model has no height field")
        if device_ptr is not None:
            if nterrain is None or int(nterrain) < 1:
                raise ValueError("set_hfield_bank: device_ptr needs nterrain >= 1, the number of grids")
            rc = lib().phys_batch_set_hfield_bank(self._h, device_ptr, 1, int(nterrain), n)
        else:
            a = np.ascontiguousarray(grids, dtype=np.float32)
            if a.size == 0 or a.size % n != 0:
                raise ValueError("set_hfield_bank: every grid needs nrow * ncol = %d samples (got %d values)" % (n, a.size))
            rc = lib().phys_batch_set_hfield_bank(self._h, a.ctypes.data, 0, a.size // n, n)
        if rc != 0:
            raise RuntimeError("set_hfield_bank failed: " + (lib().phys_last_error() or b"").decode())

    @property
    def nterrain(self):
        """Terrains of the bank in use (0: none)."""
        return lib().phys_batch_nterrain(self._h)

    @property
    def terrain_index(self):
        """Device pointer of the terrain index, int32 [nenv]: plain device memory a loop may rewrite in stream order (wrap it in a
        torch tensor, or bind one with bind_terrain_index).  Values outside the bank are clamped by the kernels and raise
        WARN_TERRAIN_INDEX."""
        p = lib().phys_batch_terrain_index_ptr(self._h)
        if not p:
            raise RuntimeError("terrain index: " + (lib().phys_last_error() or b"").decode())
        return p

    def bind_terrain_index(self, device_ptr):
        """Caller-owned HBM (an int32 torch tensor [nenv]) in the place of the terrain index."""
        if lib().phys_batch_bind_terrain_index(self._h, device_ptr) != 0:
            raise RuntimeError("bind_terrain_index failed: " + (lib().phys_last_error() or b"").decode())

    def set_terrain(self, ids=None, env0=0, device_ptr=None, n=None, stream=None):
        """Terrain ids of envs env0 ...: a host array [n] (checked against the bank) or `device_ptr` and n for int32 ids in HBM; in
        order on `stream` (default: the batch's own)."""
        if self.nterrain <= 0:
            raise ValueError("set_terrain: no bank of terrains (set_hfield_bank)")
        if device_ptr is not None:
            if n is None:
                raise ValueError("set_terrain: device_ptr needs n, the number of ids to read")
            if env0 < 0 or n < 0 or env0 + n > self.nenv:
                raise ValueError("set_terrain: envs [%d, %d) are not in the batch" % (env0, env0 + n))
            rc = lib().phys_batch_set_terrain(self._h, device_ptr, 1, int(env0), int(n), stream)
        else:
            a = np.asarray(ids)
            if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("set_terrain: ids must be a one-dimensional integer array")
            if env0 < 0 or env0 + a.size > self.nenv:
                raise ValueError("set_terrain: envs [%d, %d) are not in the batch" % (env0, env0 + a.size))
            if a.size and (a.min() < 0 or a.max() >= self.nterrain):
                raise ValueError("set_terrain: ids must lie in [0, %d)" % self.nterrain)
            a = np.ascontiguousarray(a, dtype=np.int32)
            rc = lib().phys_batch_set_terrain(self._h, a.ctypes.data, 0, int(env0), a.size, stream)
        if rc != 0:
            raise RuntimeError("set_terrain failed: " + (lib().phys_last_error() or b"").decode())

    def configure_scan(self, offsets_xy, body, scan_range):
        """The height scan's pattern: offsets_xy [P][2] (P <= SCAN_MAXPOINTS) in the heading frame of `body` (a child of the world: Cassie's
        pelvis), values clamped to +-scan_range.  Sizes F_HEIGHT_SCAN to P doubles per env (bind a tensor after this call)."""
        a = np.ascontiguousarray(offsets_xy, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 2 or not 1 <= a.shape[0] <= SCAN_MAXPOINTS:
            raise ValueError("configure_scan: offsets_xy must be [P][2] with 1 <= P <= %d" % SCAN_MAXPOINTS)
        if not float(scan_range) > 0:
            raise ValueError("configure_scan: the range must be positive")
        if not 0 < int(body) < self.pod.nbody:
            raise ValueError("configure_scan: no such body")
        if lib().phys_batch_scan_configure(self._h, a.ctypes.data, a.shape[0], int(body), float(scan_range)) != 0:
            raise ValueError("configure_scan failed: " + (lib().phys_last_error() or b"").decode())

    def height_scan(self, env0=0, n=None, stream=None):
        """One small launch on `stream` (default: the batch's own), in order with the step launches there: F_HEIGHT_SCAN of envs
        [env0, env0 + n) = clamp(z_body - highest static surface under the scan point, +-range), +range where there is none."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_height_scan(self._h, int(env0), int(n), stream) != 0:
            raise RuntimeError("height_scan failed: " + (lib().phys_last_error() or b"").decode())

    def configure_depth(self, body, cam_pos, cam_quat, width, height, fovy_deg, near, far):
        """The depth camera: rigidly mounted on `body` (a child of the world: Cassie's pelvis) at cam_pos [3], cam_quat [4] (w, x, y, z) in
        the body's frame, looking along -z of its own frame with +x right and +y up (MuJoCo's convention); `height` rows of `width`
        pixels (width * height <= DEPTH_MAXPIXELS), vertical field of view fovy_deg in degrees, 0 < near < far.  Sizes F_DEPTH to
        height * width doubles per env, row-major, row 0 at the top (bind a tensor after this call)."""
        p, q = np.ascontiguousarray(cam_pos, dtype=np.float64), np.ascontiguousarray(cam_quat, dtype=np.float64)
        if p.shape != (3,) or q.shape != (4,) or not np.linalg.norm(q) > 0:
            raise ValueError("configure_depth: cam_pos [3] and a non-zero cam_quat [4]")
        if int(width) < 1 or int(height) < 1 or int(width) * int(height) > DEPTH_MAXPIXELS:
            raise ValueError("configure_depth: 1 <= width, height and width * height <= %d" % DEPTH_MAXPIXELS)
        if not 0 < float(fovy_deg) < 180:
            raise ValueError("configure_depth: the field of view must lie in (0, 180) degrees")
        if not 0 < float(near) < float(far):
            raise ValueError("configure_depth: 0 < near < far")
        if not 0 < int(body) < self.pod.nbody:
            raise ValueError("configure_depth: no such body")
        if lib().phys_batch_depth_configure(self._h, int(body), p.ctypes.data, q.ctypes.data, int(width), int(height),
                                            float(np.radians(float(fovy_deg))), float(near), float(far)) != 0:
            raise ValueError("configure_depth failed: " + (lib().phys_last_error() or b"").decode())

    def bind_depth_pose(self, device_ptr):
        """Per-env camera extrinsics: float64 [nenv][7] (pos, quat; normalised by the kernel) in HBM, e.g. a torch tensor's data_ptr(), in
        the place of configure_depth's cam_pos / cam_quat; None returns to the shared pose."""
        if lib().phys_batch_depth_bind_pose(self._h, device_ptr) != 0:
            raise RuntimeError("bind_depth_pose failed: " + (lib().phys_last_error() or b"").decode())

    def depth_default_geoms(self):
        """The mask of the geoms a depth image shows by default: the planes, boxes and height field on bodies welded to the world."""
        return int(lib().phys_batch_depth_default_geoms(self._h))

    def depth_all_geoms(self):
        """The mask of every compiled collision geom."""
        return int(lib().phys_batch_depth_all_geoms(self._h))

    def depth_geoms(self, mask=None, *, moving=None):
        """Which geoms the depth image shows: bit g of `mask` = compiled collision geom g (the order of pod.geom_fullid), or
        moving=True for all of them -- the robot's own legs, the tray and the cube included, drawn where F_XPOS / F_XQUAT have the
        bodies: as the last step launch or forward pass left them, NOT refreshed by reset_envs, end_episodes or set(F_QPOS) -- or
        moving=False for the default.  configure_depth restores the default.  -> the mask now in force."""
        if (mask is None) == (moving is None):
            raise ValueError("depth_geoms: a mask or moving=True / False")
        if mask is None:
            mask = self.depth_all_geoms() if moving else self.depth_default_geoms()
        mask = int(mask)
        if mask < 0 or mask >> self.pod.ngeom:
            raise ValueError("depth_geoms: the mask names a geom at or above ngeom = %d" % self.pod.ngeom)
        if lib().phys_batch_depth_set_geoms(self._h, mask) != 0:
            raise RuntimeError("depth_geoms failed: " + (lib().phys_last_error() or b"").decode())
        return mask

    def bind_depth_ids(self, device_ptr):
        """The hit-id image: int32 [nenv][height * width] in HBM, contiguous, e.g. a torch tensor's data_ptr(): per pixel the compiled
        index of the geom that gave the depth, -1 where the depth is `far`.  None unbinds; configure_depth drops the binding."""
        if lib().phys_batch_depth_bind_ids(self._h, device_ptr) != 0:
            raise RuntimeError("bind_depth_ids failed: " + (lib().phys_last_error() or b"").decode())

    def depth_launches(self):
        """Diagnostics: (launches of the static depth kernel, launches of the scene kernel) so far."""
        a, b = ctypes.c_longlong(0), ctypes.c_longlong(0)
        lib().phys_batch_debug_depth_launches(self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def depth_image(self, env0=0, n=None, stream=None):
        """One launch on `stream` (default: the batch's own), in order with the step launches there: F_DEPTH of envs [env0, env0 + n) =
        per pixel the depth along the optical axis of the nearest rendered geom (by default the static planes, boxes and height field;
        depth_geoms chooses others) in [near, far], `far` where the ray meets none."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_depth_image(self._h, int(env0), int(n), stream) != 0:
            raise RuntimeError("depth_image failed: " + (lib().phys_last_error() or b"").decode())

    # ---- range sensors on any body (phys_batch_rays_cast) ----
    def configure_rays(self, rays, rmin, rmax):
        """The table of rays: a list of (body, frame, origin [3], dir [3]) or a structured array of RAY_DTYPE, 1 .. RAYS_MAX of them; frame
        is RAY_BODY (origin and direction turn with the body), RAY_WORLD_DIR (the origin turns with the body, the direction is the
        world's: straight down from a toe) or RAY_HEADING (both turn with the body's yaw only).  Body 0 is the world.  Directions are
        normalised, so a value is a metric range in [rmin, rmax], 0 <= rmin < rmax.  The bodies' poses are F_XPOS / F_XQUAT as the last
        step launch or forward pass left them (NOT refreshed by reset_envs, end_episodes or set(F_QPOS)).  Sizes F_RAYS to one double per
        ray and env (bind a tensor after this call), restores the default geoms and drops bound ids and normals."""
        if isinstance(rays, np.ndarray) and rays.dtype.names:
            table = np.ascontiguousarray(rays.astype(RAY_DTYPE, copy=False)).reshape(-1)
        else:
            rays = list(rays)
            table = np.zeros(len(rays), dtype=RAY_DTYPE)
            for k, (body, frame, origin, direction) in enumerate(rays):
                table[k] = (int(body), int(frame), np.asarray(origin, dtype=np.float64), np.asarray(direction, dtype=np.float64))
        assert RAY_DTYPE.itemsize == 56
        if lib().phys_batch_rays_configure(self._h, table.ctypes.data, int(table.size), float(rmin), float(rmax)) != 0:
            raise ValueError("configure_rays failed: " + (lib().phys_last_error() or b"").decode())

    def ray_geoms(self, mask=None):
        """Which geoms the rays see: bit g of `mask` = compiled collision geom g; None: the default (the static planes, boxes and height
        field).  Whatever the mask, a ray never sees the geoms of its own body.  -> the mask now in force."""
        mask = self.depth_default_geoms() if mask is None else int(mask)
        if mask < 0 or mask >> 32:
            raise ValueError("ray_geoms: the mask is one 32-bit word")
        if lib().phys_batch_rays_set_geoms(self._h, mask) != 0:
            raise ValueError("ray_geoms failed: " + (lib().phys_last_error() or b"").decode())
        return mask

    def bind_ray_ids(self, device_ptr):
        """The hit ids: int32 [nenv][nrays] in HBM, contiguous: per ray the compiled geom that gave the range, -1 where it is rmax.  None
        unbinds; configure_rays drops the binding."""
        if lib().phys_batch_rays_bind_ids(self._h, device_ptr) != 0:
            raise RuntimeError("bind_ray_ids failed: " + (lib().phys_last_error() or b"").decode())

    def bind_ray_normals(self, device_ptr):
        """The normals: float64 [nenv][nrays][3] in HBM, contiguous: the world-frame unit normal of the surface at the hit, against the
        ray; zero on a miss and where the range is rmin from inside a solid.  None unbinds; configure_rays drops the binding."""
        if lib().phys_batch_rays_bind_normals(self._h, device_ptr) != 0:
            raise RuntimeError("bind_ray_normals failed: " + (lib().phys_last_error() or b"").decode())

    def cast_rays(self, env0=0, n=None, stream=None):
        """One launch on `stream` (default: the batch's own), in order with the step launches there: F_RAYS (and the bound ids and
        normals) of envs [env0, env0 + n)."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_rays_cast(self._h, int(env0), int(n), stream) != 0:
            raise RuntimeError("cast_rays failed: " + (lib().phys_last_error() or b"").decode())

    def ray_launches(self):
        """Diagnostics: the ray launches so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_ray_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- probes: the reward-side getters for any body or site (phys_batch_probe) ----
    def configure_probes(self, probes, quantities):
        """The list of probes: a list of (kind, id, offset [3]) or a structured array of PROBE_DTYPE, 1 .. PROBES_MAX of them (none:
        release); kind is PROBE_BODY or PROBE_SITE, id the body or site, offset a point in the body's / site's own frame.  quantities: an
        OR of PQ_*.  Allocates the rows (F_PROBES: bind a tensor after this call), the contact words and the probes' own read-out block
        (sizeof(cm_ext_t) = 34 KB per env).  PQ_CONTACTS reads the geoms' classes from the batch's Model (a batch made from a compiled model alone has none)."""
        if isinstance(probes, np.ndarray) and probes.dtype.names:
            table = np.ascontiguousarray(probes.astype(PROBE_DTYPE, copy=False)).reshape(-1)
        else:
            probes = list(probes)
            table = np.zeros(len(probes), dtype=PROBE_DTYPE)
            for k, (kind, ident, offset) in enumerate(probes):
                table[k] = (int(kind), int(ident), np.asarray(offset, dtype=np.float64))
        assert PROBE_DTYPE.itemsize == 32
        if table.size and (int(quantities) & PQ_CONTACTS) and isinstance(self.model, Model):
            if lib().phys_batch_probe_geom_classes(self._h, self.model._h) != 0:
                raise ValueError("configure_probes failed: " + (lib().phys_last_error() or b"").decode())
        if lib().phys_batch_probes_configure(self._h, table.ctypes.data if table.size else None, int(table.size), int(quantities)) != 0:
            raise ValueError("configure_probes failed: " + (lib().phys_last_error() or b"").decode())

    def probe(self, env0=0, n=None, stream=None):
        """One forward pass of envs [env0, env0 + n) into the probes' own read-out block and the reduction behind it, on `stream`
        (default: the batch's own), in order with the step launches there: F_PROBES and the contact words of the range.  Nothing else
        of the batch changes; no host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_probe(self._h, int(env0), int(n), stream) != 0:
            raise RuntimeError("probe failed: " + (lib().phys_last_error() or b"").decode())

    def probe_layout(self):
        """{name: (offset in the row, (nprobes, *shape))} of the quantities configured, in row order."""
        off, dims = (ctypes.c_int * len(PQ_ROW))(), (ctypes.c_int * len(PQ_ROW))()
        nprobes = lib().phys_batch_probe_layout(self._h, off, dims)
        if nprobes < 0:
            raise RuntimeError("probe_layout failed: " + (lib().phys_last_error() or b"").decode())
        nv = self.pod.nv
        return {name: (off[k], (nprobes,) + tuple(nv if d == "nv" else d for d in shape)) for k, (name, shape) in enumerate(PQ_ROW) if off[k] >= 0}

    def probes(self, env0=0, n=None):
        """The rows [env0, env0 + n) of F_PROBES as named arrays of one download: pos [n][nprobes][3] ... jacp [n][nprobes][3][nv]."""
        n = self.nenv - env0 if n is None else n
        raw = self.get(F_PROBES, env0, n)
        return {name: raw[:, o: o + int(np.prod(shape))].reshape((n,) + shape) for name, (o, shape) in self.probe_layout().items()}

    def probe_contacts(self):
        """The contact words [nenv] (int32; PC_* bits), downloaded -- the batch's own, or the bound tensor's."""
        out = np.empty(self.nenv, dtype=np.int32)
        if lib().phys_batch_probe_download_contacts(self._h, out.ctypes.data) != 0:
            raise RuntimeError("probe_contacts failed: " + (lib().phys_last_error() or b"").decode())
        return out

    def bind_probe_contacts(self, device_ptr):
        """The contact words in caller-owned HBM: int32 [nenv]; None: the batch's own again.  configure_probes drops the binding."""
        if lib().phys_batch_probe_bind_contacts(self._h, device_ptr) != 0:
            raise RuntimeError("bind_probe_contacts failed: " + (lib().phys_last_error() or b"").decode())

    def probe_launches(self):
        """Diagnostics: (forward passes, reductions) probe() has launched so far."""
        a, c_ = ctypes.c_longlong(0), ctypes.c_longlong(0)
        lib().phys_batch_debug_probe_launches(self._h, ctypes.byref(a), ctypes.byref(c_))
        return a.value, c_.value

    # ---- observation rows: gather, offset, noise, scale, clip, cast and history in one launch (phys_batch_obs) ----
    def _obs_fail(self, what):
        raise (ValueError if what.startswith("configure") or what.startswith("bind") else RuntimeError)(
            what + " failed: " + (lib().phys_last_error() or b"").decode())

    def configure_obs(self, terms, history=1, dtype=np.float32, seed=0, env_base=0):
        """The terms of a frame: a list of obs_copy(...) / obs_rot_inv(...) tuples or a structured array of OBS_TERM_DTYPE (none:
        release).  history: the frames of an env's row, newest first; dtype: float32 or float64 rows; seed: the noise's key; env_base:
        what is added to the env index in the noise's counter (a rank that holds envs [k n, (k + 1) n) of a larger run passes k n).
        Allocates the rows and the frame counts, zeroed; drops the bindings of the rows and of the input."""
        table = obs_terms(terms)
        assert OBS_TERM_DTYPE.itemsize == 88
        if lib().phys_batch_obs_configure(self._h, table.ctypes.data if table.size else None, int(table.size), int(history), _obs_dtype(dtype),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_base) & 0xFFFFFFFF) != 0:
            self._obs_fail("configure_obs")
        self._obs_np = np.float64 if _obs_dtype(dtype) == 8 else np.float32

    def bind_obs(self, device_ptr, row_stride=None):
        """The rows in caller-owned HBM of the configured dtype, `row_stride` elements (default: the row's) between two envs' rows; None:
        the batch's own again."""
        if lib().phys_batch_obs_bind(self._h, device_ptr, int(row_stride if row_stride is not None else self.obs_dim()[2]) if device_ptr else 0) != 0:
            self._obs_fail("bind_obs")

    def bind_obs_input(self, device_ptr, dim=0, row_stride=None, dtype=np.float32):
        """The caller's per-env array the OBS_INPUT terms read: [nenv] rows of `dim` float32 / float64 elements, `row_stride` elements
        apart (default: dim).  None un-binds."""
        if lib().phys_batch_obs_bind_input(self._h, device_ptr, int(dim), int(dim if row_stride is None else row_stride), _obs_dtype(dtype)) != 0:
            self._obs_fail("bind_obs_input")

    def observe(self, env0=0, n=None, refill_ptr=None, stream=None):
        """One launch on `stream` (default: the batch's own), in order with the step launches there: the new frame of every env of
        [env0, env0 + n) and the shift of its history.  refill_ptr: an int32 device array [n] (the range's slice of EP_DONE), non-zero =
        the env's whole history becomes the new frame.  No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_obs(self._h, int(env0), int(n), refill_ptr, stream) != 0:
            self._obs_fail("observe")

    def obs_dim(self):
        """(ncols, history, elements of a row)."""
        a, h, r = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        if lib().phys_batch_obs_dim(self._h, ctypes.byref(a), ctypes.byref(h), ctypes.byref(r)) != 0:
            self._obs_fail("obs_dim")
        return a.value, h.value, r.value

    def obs_layout(self):
        """The first column of every term, in the terms' order."""
        n = lib().phys_batch_obs_layout(self._h, None)
        if n < 0:
            self._obs_fail("obs_layout")
        first = np.zeros(n, dtype=np.int32)
        lib().phys_batch_obs_layout(self._h, first.ctypes.data)
        return [int(v) for v in first]

    def obs(self, env0=0, n=None):
        """The rows [env0, env0 + n) downloaded: [n][history][ncols] in the configured dtype."""
        n = self.nenv - env0 if n is None else n
        ncols, history, _ = self.obs_dim()
        out = np.empty((n, history, ncols), dtype=self._obs_np)
        if lib().phys_batch_obs_download(self._h, out.ctypes.data, int(env0), int(n)) != 0:
            self._obs_fail("obs")
        return out

    def obs_frames(self):
        """The calls every env's row has seen (uint32 [nenv]): the third word of the noise's counter."""
        out = np.empty(self.nenv, dtype=np.uint32)
        if lib().phys_batch_obs_frames(self._h, out.ctypes.data) != 0:
            self._obs_fail("obs_frames")
        return out

    def set_obs_frames(self, frames):
        a = np.ascontiguousarray(frames, dtype=np.uint32).reshape(self.nenv)
        if lib().phys_batch_obs_set_frames(self._h, a.ctypes.data) != 0:
            self._obs_fail("set_obs_frames")

    def obs_launches(self):
        """Diagnostics: the launches observe() has made so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_obs_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- reward rows: errors, norms, shapes, weights, gates, the clip and the episode returns in one launch (phys_batch_reward) ----
    def configure_rewards(self, terms, dtype=np.float32, lo=-np.inf, hi=np.inf):
        """The terms of the reward: a list of rew_vec(...) / rew_rot_inv(...) / rew_quat(...) tuples or a structured array of
        REW_TERM_DTYPE (none: release).  dtype: float32 or float64 rewards and term rows; lo, hi: the clip of the reward.  Allocates the
        rewards, the returns and the final returns, zeroed; drops the bindings of the rewards, the term rows and the input."""
        table = rew_terms(terms)
        assert REW_TERM_DTYPE.itemsize == 120
        if lib().phys_batch_reward_configure(self._h, table.ctypes.data if table.size else None, int(table.size), _obs_dtype(dtype), float(lo), float(hi)) != 0:
            self._obs_fail("configure_rewards")
        self._rew_np = np.float64 if _obs_dtype(dtype) == 8 else np.float32

    def bind_rewards(self, device_ptr, stride=1):
        """The rewards in caller-owned HBM of the configured dtype, `stride` elements between two envs'; None: the batch's own again."""
        if lib().phys_batch_reward_bind(self._h, device_ptr, int(stride) if device_ptr else 0) != 0:
            self._obs_fail("bind_rewards")

    def bind_reward_terms(self, device_ptr=None, row_stride=None, own=False):
        """Every term's contribution [nenv][nterms]: in caller-owned HBM, `row_stride` elements (default: nterms) between two envs' rows;
        or, with own=True, in rows of the batch's own; neither: none are written (the state after configure_rewards)."""
        stride = int(row_stride if row_stride is not None else self.reward_dim()[0]) if device_ptr else 0
        if lib().phys_batch_reward_bind_terms(self._h, device_ptr, stride, 1 if own else 0) != 0:
            self._obs_fail("bind_reward_terms")

    def bind_reward_input(self, device_ptr, dim=0, row_stride=None, dtype=np.float32):
        """The caller's per-env array the REW_INPUT terms read: [nenv] rows of `dim` float32 / float64 elements, `row_stride` elements
        apart (default: dim); it may be the observation's input.  None un-binds."""
        if lib().phys_batch_reward_bind_input(self._h, device_ptr, int(dim), int(dim if row_stride is None else row_stride), _obs_dtype(dtype)) != 0:
            self._obs_fail("bind_reward_input")

    def reward(self, env0=0, n=None, reset_ptr=None, stream=None):
        """One launch on `stream` (default: the batch's own), in order with the step launches there: the reward, the term rows and the
        return of every env of [env0, env0 + n).  reset_ptr: an int32 device array [n] (the range's slice of EP_DONE as the previous
        policy step's end_episodes left it), non-zero = the env's return moves to the final returns and restarts.  Call it in front of
        end_episodes.  No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_reward(self._h, int(env0), int(n), reset_ptr, stream) != 0:
            self._obs_fail("reward")

    def reward_dim(self):
        """(nterms, bytes of an element, whether term rows are written)."""
        a, d, t = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        if lib().phys_batch_reward_dim(self._h, ctypes.byref(a), ctypes.byref(d), ctypes.byref(t)) != 0:
            self._obs_fail("reward_dim")
        return a.value, d.value, bool(t.value)

    def rewards(self, env0=0, n=None):
        """The rewards [env0, env0 + n) downloaded, in the configured dtype."""
        n = self.nenv - env0 if n is None else n
        self.reward_dim()
        out = np.empty(n, dtype=self._rew_np)
        if lib().phys_batch_reward_download(self._h, out.ctypes.data, int(env0), int(n)) != 0:
            self._obs_fail("rewards")
        return out

    def reward_terms(self, env0=0, n=None):
        """The term rows [env0, env0 + n) downloaded: [n][nterms] in the configured dtype."""
        n = self.nenv - env0 if n is None else n
        out = np.empty((n, self.reward_dim()[0]), dtype=self._rew_np)
        if lib().phys_batch_reward_download_terms(self._h, out.ctypes.data, int(env0), int(n)) != 0:
            self._obs_fail("reward_terms")
        return out

    def returns(self):
        """The running return of every env's episode (float64 [nenv])."""
        out = np.empty(self.nenv, dtype=np.float64)
        if lib().phys_batch_reward_returns(self._h, out.ctypes.data) != 0:
            self._obs_fail("returns")
        return out

    def set_returns(self, returns):
        a = np.ascontiguousarray(returns, dtype=np.float64).reshape(self.nenv)
        if lib().phys_batch_reward_set_returns(self._h, a.ctypes.data) != 0:
            self._obs_fail("set_returns")

    def final_returns(self):
        """The return of the last episode of every env that ended (float64 [nenv])."""
        out = np.empty(self.nenv, dtype=np.float64)
        if lib().phys_batch_reward_final(self._h, out.ctypes.data) != 0:
            self._obs_fail("final_returns")
        return out

    def reward_launches(self):
        """Diagnostics: the launches reward() has made so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_reward_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- action rows: clip, noise, latency, low-pass, the map onto a pose and the store into the command fields in one launch (phys_batch_act) ----
    def configure_actions(self, cols, delay_max=0, dtype=np.float32, seed=0, env_base=0):
        """The columns of an action: a list of act_col(...) tuples or a structured array of ACT_COL_DTYPE (none: release).  delay_max:
        the depth of the per-env delay line in calls (0 .. ACT_MAXDELAY); dtype: float32 or float64 action rows; seed, env_base: the
        noise's key and the offset of its env counter, as configure_obs takes them.  Allocates the rows, the state and the call counts,
        zeroed; drops the bindings of the actions, the rows, the input and the delays."""
        table = act_cols(cols)
        assert ACT_COL_DTYPE.itemsize == 80
        if lib().phys_batch_act_configure(self._h, table.ctypes.data if table.size else None, int(table.size), int(delay_max), _obs_dtype(dtype),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_base) & 0xFFFFFFFF) != 0:
            self._obs_fail("configure_actions")
        self._act_np = np.float64 if _obs_dtype(dtype) == 8 else np.float32

    def bind_actions(self, device_ptr, row_stride=None, dtype=np.float32):
        """The policy's output in device memory: [nenv] rows of ncols float32 / float64 elements, `row_stride` elements (default: ncols)
        apart.  None un-binds."""
        stride = int(row_stride if row_stride is not None else self.action_dim()[0]) if device_ptr else 0
        if lib().phys_batch_act_bind_actions(self._h, device_ptr, stride, _obs_dtype(dtype)) != 0:
            self._obs_fail("bind_actions")

    def bind_action_rows(self, device_ptr, row_stride=None):
        """The action rows [3][ncols] (ACT_NOW | ACT_PREV | ACT_APPLIED) in caller-owned HBM of the configured dtype, `row_stride`
        elements (default: 3 ncols) between two envs' rows -- a column block of the tensor bound as the observation's and the reward's
        input; None: the batch's own again."""
        if lib().phys_batch_act_bind_rows(self._h, device_ptr, int(row_stride if row_stride is not None else self.action_dim()[2]) if device_ptr else 0) != 0:
            self._obs_fail("bind_action_rows")

    def bind_action_input(self, device_ptr, dim=0, row_stride=None, dtype=np.float32):
        """The caller's per-env array the ACT_INPUT columns read (a reference pose for this step): [nenv] rows of `dim` float32 / float64
        elements, `row_stride` elements apart (default: dim); it may be the observation's input.  None un-binds."""
        if lib().phys_batch_act_bind_input(self._h, device_ptr, int(dim), int(dim if row_stride is None else row_stride), _obs_dtype(dtype)) != 0:
            self._obs_fail("bind_action_input")

    def bind_action_delay(self, device_ptr):
        """The per-env latency in calls: an int32 device array [nenv], clamped to [0, delay_max] without a word.  None: no delay."""
        if lib().phys_batch_act_bind_delay(self._h, device_ptr) != 0:
            self._obs_fail("bind_action_delay")

    def act(self, env0=0, n=None, reset_ptr=None, stream=None):
        """One launch on `stream` (default: the batch's own), in front of the range's step launch: the command fields, the action rows
        and the delay-line and filter state of every env of [env0, env0 + n) from the bound action tensor.  reset_ptr: an int32 device
        array [n] (the range's slice of EP_DONE as the previous policy step's end_episodes left it), non-zero = the env starts afresh.
        No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_act(self._h, int(env0), int(n), reset_ptr, stream) != 0:
            self._obs_fail("act")

    def action_dim(self):
        """(ncols, delay_max, elements of a row = 3 ncols, doubles of an env's state = (delay_max + 3) ncols)."""
        a, d, r, s = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        if lib().phys_batch_act_dim(self._h, ctypes.byref(a), ctypes.byref(d), ctypes.byref(r), ctypes.byref(s)) != 0:
            self._obs_fail("action_dim")
        return a.value, d.value, r.value, s.value

    def action_rows(self, env0=0, n=None):
        """The rows [env0, env0 + n) downloaded: [n][3][ncols] in the configured dtype."""
        n = self.nenv - env0 if n is None else n
        ncols = self.action_dim()[0]
        out = np.empty((n, 3, ncols), dtype=self._act_np)
        if lib().phys_batch_act_download(self._h, out.ctypes.data, int(env0), int(n)) != 0:
            self._obs_fail("action_rows")
        return out

    def action_state(self):
        """(state float64 [nenv][delay_max + 3][ncols]: the delay line's slots, newest first | the filter state | the previous clipped
        action; counts uint32 [nenv]: the calls every env has seen, the third word of the noise's counter)."""
        ncols, D, _, _ = self.action_dim()
        state, counts = np.empty((self.nenv, D + 3, ncols), dtype=np.float64), np.empty(self.nenv, dtype=np.uint32)
        if lib().phys_batch_act_state(self._h, state.ctypes.data, counts.ctypes.data) != 0:
            self._obs_fail("action_state")
        return state, counts

    def set_action_state(self, state, counts):
        ncols, D, _, _ = self.action_dim()
        s = np.ascontiguousarray(state, dtype=np.float64).reshape(self.nenv, D + 3, ncols)
        k = np.ascontiguousarray(counts, dtype=np.uint32).reshape(self.nenv)
        if lib().phys_batch_act_set_state(self._h, s.ctypes.data, k.ctypes.data) != 0:
            self._obs_fail("set_action_state")

    def action_launches(self):
        """Diagnostics: the launches act() has made so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_act_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- task rows: commands, gait clocks, waveforms, a reference trajectory and pushes in one launch (phys_batch_task) ----
    def configure_task(self, cols, dtype=np.float32, seed=0, env_base=0):
        """The columns of a task row: a list of task_sample / task_phase / task_wave / task_table tuples or a structured array of
        TASK_COL_DTYPE (1 .. TASK_MAXCOLS).  dtype: float32 or float64 rows; seed, env_base: the key of the draws and the offset of
        their env counter, as configure_obs takes them.  A table the TABLE columns read is set first (set_task_table).  Allocates the
        rows, the state and the call counts, zeroed; drops the binding of the rows."""
        table = task_cols(cols)
        assert TASK_COL_DTYPE.itemsize == 144
        if lib().phys_batch_task_configure(self._h, table.ctypes.data if table.size else None, int(table.size), _obs_dtype(dtype),
                                           int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_base) & 0xFFFFFFFF) != 0:
            self._obs_fail("configure_task")
        self._task_np = np.float64 if _obs_dtype(dtype) == 8 else np.float32

    def set_task_table(self, table):
        """The periodic reference trajectory the TABLE columns interpolate: float64 [nframes][tcols] (<= 4096 x 64), uploaded once."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        if t.ndim != 2:
            raise ValueError("set_task_table: a table is [nframes][tcols]")
        if lib().phys_batch_task_set_table(self._h, t.ctypes.data if t.size else None, int(t.shape[0]), int(t.shape[1])) != 0:
            self._obs_fail("set_task_table")

    def bind_task_rows(self, device_ptr, row_stride=None):
        """The task rows [ncols] in caller-owned HBM of the configured dtype, `row_stride` elements (default: ncols) between two envs' rows
        -- a column block of the tensor bound as the observation's, the reward's and the action's input; None: the batch's own again."""
        if lib().phys_batch_task_bind_rows(self._h, device_ptr, int(row_stride if row_stride is not None else self.task_dim()) if device_ptr else 0) != 0:
            self._obs_fail("bind_task_rows")

    def task(self, env0=0, n=None, reset_ptr=None, stream=None):
        """One launch on `stream` (default: the batch's own), between the range's end_episodes and its observation: the task rows, the
        state and the destination elements of every env of [env0, env0 + n).  reset_ptr: an int32 device array [n] (the range's slice
        of EP_DONE as this policy step's end_episodes left it), non-zero = the env starts afresh.  No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_task(self._h, int(env0), int(n), reset_ptr, stream) != 0:
            self._obs_fail("task")

    def task_dim(self):
        """The columns of a task row."""
        a = ctypes.c_int(0)
        if lib().phys_batch_task_dim(self._h, ctypes.byref(a), None) != 0:
            self._obs_fail("task_dim")
        return a.value

    def task_rows(self, env0=0, n=None):
        """The rows [env0, env0 + n) downloaded: [n][ncols] in the configured dtype."""
        n = self.nenv - env0 if n is None else n
        out = np.empty((n, self.task_dim()), dtype=self._task_np)
        if lib().phys_batch_task_download(self._h, out.ctypes.data, int(env0), int(n)) != 0:
            self._obs_fail("task_rows")
        return out

    def task_state(self):
        """(state float64 [nenv][ncols]: a SAMPLE's held value, a PHASE's phase; words uint32 [nenv][3][ncols]: a SAMPLE's left | age |
        epoch; counts uint32 [nenv]: the calls every env has seen)."""
        ncols = self.task_dim()
        state, words, counts = np.empty((self.nenv, ncols), dtype=np.float64), np.empty((self.nenv, 3, ncols), dtype=np.uint32), np.empty(self.nenv, dtype=np.uint32)
        if lib().phys_batch_task_state(self._h, state.ctypes.data, words.ctypes.data, counts.ctypes.data) != 0:
            self._obs_fail("task_state")
        return state, words, counts

    def set_task_state(self, state, words, counts):
        ncols = self.task_dim()
        s = np.ascontiguousarray(state, dtype=np.float64).reshape(self.nenv, ncols)
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(self.nenv, 3, ncols)
        k = np.ascontiguousarray(counts, dtype=np.uint32).reshape(self.nenv)
        if lib().phys_batch_task_set_state(self._h, s.ctypes.data, w.ctypes.data, k.ctypes.data) != 0:
            self._obs_fail("set_task_state")

    def task_launches(self):
        """Diagnostics: the launches task() has made so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_task_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- event rows: contact flags, timers, edges, latches, running extremes and done words in one launch (phys_batch_events) ----
    def configure_events(self, cols, dtype=np.float32, done_mask=0):
        """The columns of an event row: a list of ev_measure / ev_level / ev_timer / ev_edge / ev_latch / ev_accum / ev_logic tuples or a
        structured array of EV_COL_DTYPE (1 .. EV_MAXCOLS; none: release), evaluated in index order; a column names lower columns only.
        dtype: float32 or float64 rows; done_mask: a uint64 (or a list of columns) whose on columns set the env's done word.  Allocates
        the rows, the done words, the state and the call counts, zeroed; drops the bindings of the rows, the input and the done words."""
        table = ev_cols(cols)
        assert EV_COL_DTYPE.itemsize == 128
        mask = int(done_mask) if isinstance(done_mask, (int, np.integer)) else sum(1 << int(k) for k in set(done_mask))
        if lib().phys_batch_events_configure(self._h, table.ctypes.data if table.size else None, int(table.size), _obs_dtype(dtype), mask & 0xFFFFFFFFFFFFFFFF) != 0:
            self._obs_fail("configure_events")
        self._ev_np = np.float64 if _obs_dtype(dtype) == 8 else np.float32

    def bind_event_rows(self, device_ptr, row_stride=None):
        """The event rows [ncols] in caller-owned HBM of the configured dtype, `row_stride` elements (default: ncols) between two envs' rows
        -- a column block of the tensor bound as the observation's, the reward's and the action's input; None: the batch's own again."""
        if lib().phys_batch_events_bind_rows(self._h, device_ptr, int(row_stride if row_stride is not None else self.event_dim()) if device_ptr else 0) != 0:
            self._obs_fail("bind_event_rows")

    def bind_event_input(self, device_ptr, dim=0, row_stride=None, dtype=np.float32):
        """The caller's per-env array the EV_INPUT columns read: [nenv] rows of `dim` float32 / float64 elements, `row_stride` elements
        apart (default: dim).  None un-binds."""
        if lib().phys_batch_events_bind_input(self._h, device_ptr, int(dim), int(dim if row_stride is None else row_stride), _obs_dtype(dtype)) != 0:
            self._obs_fail("bind_event_input")

    def bind_event_flags(self, device_ptr):
        """The done words in caller-owned HBM: int32 [nenv], dense (a torch tensor the loop reads); None: the batch's own again."""
        if lib().phys_batch_events_bind_flags(self._h, device_ptr) != 0:
            self._obs_fail("bind_event_flags")

    def event_flags_ptr(self, env0=0):
        """The device address of env env0's done word: what end_episodes takes as force_ptr for a range that starts there."""
        p = lib().phys_batch_events_flags_ptr(self._h)
        if not p:
            raise RuntimeError("event_flags_ptr: not configured (configure_events first)")
        return p + 4 * int(env0)

    def events(self, env0=0, n=None, reset_ptr=None, stream=None):
        """One launch on `stream` (default: the batch's own), behind the step launch and the launches that make sources, in front of
        reward and end_episodes: the event rows, the done words and the state of every env of [env0, env0 + n).  reset_ptr: an int32
        device array [n] (the range's slice of EP_DONE as the previous policy step's end_episodes left it), non-zero = the env's columns
        start afresh.  No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_events(self._h, int(env0), int(n), reset_ptr, stream) != 0:
            self._obs_fail("events")

    def event_dim(self):
        """The columns of an event row."""
        a = ctypes.c_int(0)
        if lib().phys_batch_events_dim(self._h, ctypes.byref(a), None, None) != 0:
            self._obs_fail("event_dim")
        return a.value

    def event_rows(self, env0=0, n=None):
        """The rows [env0, env0 + n) downloaded: [n][ncols] in the configured dtype."""
        n = self.nenv - env0 if n is None else n
        out = np.empty((n, self.event_dim()), dtype=self._ev_np)
        if lib().phys_batch_events_download(self._h, out.ctypes.data, int(env0), int(n)) != 0:
            self._obs_fail("event_rows")
        return out

    def event_flags(self):
        """The done words downloaded: int32 [nenv]."""
        out = np.empty(self.nenv, dtype=np.int32)
        if lib().phys_batch_events_download_flags(self._h, out.ctypes.data) != 0:
            self._obs_fail("event_flags")
        return out

    def event_state(self):
        """(state float64 [nenv][2][ncols]: slot 0 a LATCH's h and an ACCUM's m, slot 1 a LATCH's q; words uint32 [nenv][ncols]: a LEVEL's
        s, a TIMER's t, an EDGE's p; counts uint32 [nenv]: the calls every env has seen)."""
        ncols = self.event_dim()
        state, words, counts = np.empty((self.nenv, 2, ncols), dtype=np.float64), np.empty((self.nenv, ncols), dtype=np.uint32), np.empty(self.nenv, dtype=np.uint32)
        if lib().phys_batch_events_state(self._h, state.ctypes.data, words.ctypes.data, counts.ctypes.data) != 0:
            self._obs_fail("event_state")
        return state, words, counts

    def set_event_state(self, state, words, counts):
        ncols = self.event_dim()
        s = np.ascontiguousarray(state, dtype=np.float64).reshape(self.nenv, 2, ncols)
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(self.nenv, ncols)
        k = np.ascontiguousarray(counts, dtype=np.uint32).reshape(self.nenv)
        if lib().phys_batch_events_set_state(self._h, s.ctypes.data, w.ctypes.data, k.ctypes.data) != 0:
            self._obs_fail("set_event_state")

    def event_launches(self):
        """Diagnostics: the launches events() has made so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_events_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- policy rows: an exact MLP actor and critic, the sampled action and its log-probability in one launch (phys_batch_policy) ----
    def configure_policy(self, nets, in_dim):
        """The networks of a policy: a list of 1 or 2 networks (the actor, then the critic), each a list of pol_layer(out, act) (none:
        release); both read the bound input row of in_dim float32.  Allocates the packed weights; drops every binding and every loaded
        layer."""
        nets = list(nets)
        table = pol_nets(nets, in_dim)
        assert POL_NET_DTYPE.itemsize == 52
        if lib().phys_batch_policy_configure(self._h, table.ctypes.data if nets else None, len(nets), int(in_dim)) != 0:
            self._obs_fail("configure_policy")
        self._pol_out = [int(table[a]["layer"][int(table[a]["nlayers"]) - 1][1]) for a in range(len(nets))]

    def load_policy(self, net, layers, stream=None):
        """The weights of network `net`: per layer (W, b) as numpy arrays (W float32 [out][in], as torch.nn.Linear.weight) -- the call waits
        for the batch's streams -- or (w_ptr, w_row_stride, b_ptr) as float32 device pointers -- one small launch per layer on `stream`,
        no host synchronisation: call it after an optimiser step on the stream the policy call follows on."""
        for l, L in enumerate(layers):
            if len(L) == 3:
                rc = lib().phys_batch_policy_load(self._h, int(net), l, L[0], int(L[1]), L[2], stream)
            else:
                w, bias = np.ascontiguousarray(L[0], dtype=np.float32), np.ascontiguousarray(L[1], dtype=np.float32)
                assert w.ndim == 2 and bias.shape == (w.shape[0],)
                rc = lib().phys_batch_policy_load_host(self._h, int(net), l, w.ctypes.data, int(w.shape[1]), bias.ctypes.data)
            if rc != 0:
                self._obs_fail("load_policy")

    def bind_policy_input(self, device_ptr, dim=0, row_stride=None, dtype=np.float32):
        """The input rows in device memory: [nenv] rows of `dim` (= in_dim) float32 elements, `row_stride` elements (default: dim) apart --
        the observation rows.  float64 is refused.  None un-binds."""
        if lib().phys_batch_policy_bind_input(self._h, device_ptr, int(dim), int(dim if row_stride is None else row_stride), _obs_dtype(dtype)) != 0:
            self._obs_fail("bind_policy_input")

    def bind_policy_norm(self, mean_ptr, inv_ptr=None, clip=np.inf):
        """The input's normalisation: float32 device arrays [in_dim] of the mean and of 1 / std, read at every call, and the clip of the
        result.  None releases."""
        if lib().phys_batch_policy_bind_norm(self._h, mean_ptr, inv_ptr, float(clip)) != 0:
            self._obs_fail("bind_policy_norm")

    def bind_policy_output(self, net, device_ptr, row_stride=None):
        """Network net's output rows in caller-owned HBM: float32 [nenv] rows of its last layer's width, `row_stride` elements apart.
        None un-binds."""
        stride = int(row_stride if row_stride is not None else self._pol_out[net]) if device_ptr else 0
        if lib().phys_batch_policy_bind_output(self._h, int(net), device_ptr, stride) != 0:
            self._obs_fail("bind_policy_output")

    def bind_policy_sample(self, eps_ptr, log_std_ptr=None, action_ptr=None, logp_ptr=None, eps_stride=None, action_stride=None):
        """The sampled action: eps float32 [nenv][A] (the caller's standard normal draws), log_std float32 [A] (read at every call), the
        action tensor float32 [nenv][A] -- what bind_actions points at -- and logp float32 [nenv]; strides default to A, the actor's output
        width.  None releases."""
        A = self._pol_out[0] if getattr(self, "_pol_out", None) else 0
        if lib().phys_batch_policy_bind_sample(self._h, eps_ptr, int(A if eps_stride is None else eps_stride), log_std_ptr, action_ptr,
                                               int(A if action_stride is None else action_stride), logp_ptr) != 0:
            self._obs_fail("bind_policy_sample")

    def policy(self, env0=0, n=None, stream=None):
        """One launch on `stream` (default: the batch's own), between observe and act: the outputs of every network, and the action and
        its log-probability where a sample is bound, of every env of [env0, env0 + n).  No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_policy(self._h, int(env0), int(n), stream) != 0:
            self._obs_fail("policy")

    def policy_outputs(self, net):
        """Network net's bound output rows downloaded: float32 [nenv][width] (waits for the batch's streams)."""
        out = np.empty((self.nenv, self._pol_out[net]), dtype=np.float32)
        if lib().phys_batch_policy_download(self._h, int(net), out.ctypes.data) != 0:
            self._obs_fail("policy_outputs")
        return out

    def policy_packed(self):
        """Diagnostics: the packed weights and biases as the kernel reads them (float32; waits for the batch's streams)."""
        n = ctypes.c_longlong(0)
        if lib().phys_batch_policy_download_packed(self._h, None, ctypes.byref(n)) != 0:
            self._obs_fail("policy_packed")
        out = np.empty(n.value, dtype=np.float32)
        if lib().phys_batch_policy_download_packed(self._h, out.ctypes.data, ctypes.byref(n)) != 0:
            self._obs_fail("policy_packed")
        return out

    def policy_launches(self):
        """Diagnostics: the launches policy() has made so far."""
        a = ctypes.c_longlong(0)
        lib().phys_batch_debug_policy_launches(self._h, ctypes.byref(a))
        return a.value

    # ---- rollout rows: the transitions of T policy steps, their advantages and returns, the normalised advantages (phys_batch_rollout_*) ----
    def configure_rollout(self, T, srcs, gamma=0.99, lam=0.95, timeout_mask=0):
        """The rollout: T steps of the sources `srcs`, a list of (role, dim) pairs -- role RO_DATA, RO_OBS, ... RO_REASON or its lower-case
        name, dim in 32-bit words (none: release).  Allocates the stores, ADV and RET, zeroed; drops every binding; waits for the streams."""
        srcs = list(srcs)
        table = ro_srcs(srcs)
        assert RO_SRC_DTYPE.itemsize == 8
        if lib().phys_batch_rollout_configure(self._h, int(T), table.ctypes.data if srcs else None, len(srcs), float(gamma), float(lam), int(timeout_mask)) != 0:
            self._obs_fail("configure_rollout")
        self._ro = (int(T), [(int(r), int(d)) for r, d in table[: len(srcs)]])

    @staticmethod
    def _ro_id(s):
        return RO_NAMES[s] if isinstance(s, str) else int(s)

    def bind_rollout_source(self, s, device_ptr, row_stride=None):
        """Source s (an index, a role or its name) read from caller-owned HBM: [nenv] rows of its dim words, `row_stride` words (default:
        dim) apart.  None un-binds: a source other than RO_DATA is then resolved at every call from where the batch reads or writes it."""
        s = self._ro_id(s)
        stride = 0
        if device_ptr:
            stride = int(row_stride) if row_stride is not None else self.rollout_dim(s)
        if lib().phys_batch_rollout_bind_source(self._h, s, device_ptr, stride) != 0:
            self._obs_fail("bind_rollout_source")

    def bind_rollout_storage(self, s, device_ptr, step_stride=None, row_stride=None):
        """A caller's tensor in the place of the store of source s, or of RO_ADV / RO_RET / RO_ADVN: [T][nenv][dim] words, `step_stride`
        words between two steps and `row_stride` between two envs (default: dense).  None: the batch's own again, zeroed."""
        s = self._ro_id(s)
        dim = self.rollout_dim(s)
        row = int(dim if row_stride is None else row_stride)
        step = int(self.nenv * row if step_stride is None else step_stride)
        if lib().phys_batch_rollout_bind_storage(self._h, s, device_ptr, step if device_ptr else 0, row if device_ptr else 0) != 0:
            self._obs_fail("bind_rollout_storage")

    def rollout_dim(self, s):
        """The words of a row of source s (an index, a role or its name); 1 for RO_ADV, RO_RET, RO_ADVN."""
        s = self._ro_id(s)
        if s in (RO_ADV, RO_RET, RO_ADVN):
            return 1
        srcs = self._ro[1]
        if 0 <= s < RO_MAXSRC:
            return srcs[s][1]
        hits = [d for r, d in srcs if r == s]
        if len(hits) != 1:
            raise ValueError("rollout: no such source, or a role several sources share")
        return hits[0]

    def rollout_ptr(self, s):
        """(device pointer, step stride, row stride) of the store of source s, or of RO_ADV / RO_RET / RO_ADVN; strides in words."""
        step, row = ctypes.c_longlong(0), ctypes.c_longlong(0)
        p = lib().phys_batch_rollout_ptr(self._h, self._ro_id(s), ctypes.byref(step), ctypes.byref(row))
        return p, step.value, row.value

    def rollout_record(self, t, env0=0, n=None, stream=None):
        """One launch on `stream` (default: the batch's own), behind end_episodes of policy step t: every source's rows of the envs
        [env0, env0 + n) into slot t of its store.  No host synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_rollout_record(self._h, int(t), int(env0), int(n), stream) != 0:
            self._obs_fail("rollout_record")

    def rollout_finish(self, env0=0, n=None, last_value_ptr=None, stride=1, stream=None):
        """One launch on `stream`, behind the range's T records: ADV and RET of the envs [env0, env0 + n).  last_value_ptr: float32 [nenv]
        in device memory, `stride` words apart (None: the VALUE source as resolved now, V(o_T) after the next observe and policy)."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_rollout_finish(self._h, int(env0), int(n), last_value_ptr, int(stride), stream) != 0:
            self._obs_fail("rollout_finish")

    def rollout_normalise(self, eps=1e-8, stream=None):
        """Four short launches on `stream` over the whole batch, behind every range's finish (ordering the streams is the caller's job):
        ADVN = (ADV - mean) / (std + eps)."""
        if lib().phys_batch_rollout_normalise(self._h, float(eps), stream) != 0:
            self._obs_fail("rollout_normalise")

    def rollout_stats(self):
        """(mean, std, inv) of the last rollout_normalise (waits for the batch's streams)."""
        out = np.zeros(3, dtype=np.float64)
        if lib().phys_batch_rollout_stats(self._h, out.ctypes.data) != 0:
            self._obs_fail("rollout_stats")
        return tuple(out)

    def rollout(self, s):
        """The store of source s (an index, a role or its name: "obs", "action", ...), or "adv" / "ret" / "advn", downloaded: [T][nenv][dim]
        (dim 1: [T][nenv]), int32 for RO_DONE / RO_REASON, uint32 words for RO_DATA, float32 otherwise (waits for the batch's streams)."""
        s = self._ro_id(s)
        dim = self.rollout_dim(s)
        role = self._ro[1][s][0] if 0 <= s < RO_MAXSRC else s
        out = np.empty((self._ro[0], self.nenv, dim), dtype=np.uint32)
        if lib().phys_batch_rollout_download(self._h, s, out.ctypes.data) != 0:
            self._obs_fail("rollout")
        out = out.view(np.int32 if role in RO_INT_ROLES else np.uint32 if role == RO_DATA else np.float32)
        return out[:, :, 0] if dim == 1 else out

    def rollout_launches(self):
        """Diagnostics: the launches rollout_record, rollout_finish and rollout_normalise (four a call) have made so far."""
        a = (ctypes.c_longlong * 3)()
        lib().phys_batch_debug_rollout_launches(self._h, a)
        return tuple(a)

    # ---- gradient rows: the PPO loss of a minibatch of the rollout and its exact gradient (phys_batch_grad_*) ----
    def configure_grad(self, max_m, chunk=512, clip_eps=0.2, c_v=0.5, c_ent=0.0):
        """The gradient of minibatches of up to max_m samples of the rollout (0: release): the clipped surrogate with clip_eps, c_v times
        the value loss, c_ent times the entropy.  `chunk`, a multiple of 16 in 16 .. 4096, is the run of positions a weight sum's partial
        covers: part of the definition.  Needs configure_policy and configure_rollout; waits for the batch's streams."""
        if lib().phys_batch_grad_configure(self._h, int(max_m), int(chunk), float(clip_eps), float(c_v), float(c_ent)) != 0:
            self._obs_fail("configure_grad")

    def bind_grad(self, net, layer, dw_ptr, dw_row_stride=None, db_ptr=None):
        """A caller's float32 device tensors for a layer's gradients: dW [out][in], `dw_row_stride` elements (default: in) apart, as
        torch.nn.Linear.weight.grad, and db [out].  None: the batch's own again."""
        stride = 0
        if dw_ptr:
            stride = int(dw_row_stride) if dw_row_stride is not None else int(self.grad_count(GRAD_DW, net, layer) // max(self.grad_count(GRAD_DB, net, layer), 1))
        if lib().phys_batch_grad_bind(self._h, int(net), int(layer), dw_ptr, stride, db_ptr) != 0:
            self._obs_fail("bind_grad")

    def bind_grad_log_std(self, device_ptr):
        """A caller's float32 device tensor [A] for log_std's gradient.  None: the batch's own again."""
        if lib().phys_batch_grad_bind_log_std(self._h, device_ptr) != 0:
            self._obs_fail("bind_grad_log_std")

    def grad(self, idx_ptr, m, stream=None):
        """The launches of one minibatch on `stream` (default: the batch's own): idx_ptr int32 [m] in device memory, sample indices
        t * nenv + env into the rollout.  The gradients land in the bound tensors (or the batch's own).  No host synchronisation."""
        if lib().phys_batch_grad(self._h, idx_ptr, int(m), stream) != 0:
            self._obs_fail("grad")

    def grad_stats(self):
        """The eight statistics of the last grad call, by name (GRAD_STATS), and as an array under "all" (waits for the batch's streams)."""
        out = np.zeros(GRAD_NSTATS, dtype=np.float64)
        if lib().phys_batch_grad_stats(self._h, out.ctypes.data) != 0:
            self._obs_fail("grad_stats")
        d = dict(zip(GRAD_STATS, out))
        d["all"] = out
        return d

    def grad_count(self, what, net=0, layer=0):
        """The elements grad_download(what, net, layer) returns (-1: no such thing)."""
        return int(lib().phys_batch_grad_count(self._h, int(what), int(net), int(layer)))

    def grad_download(self, what, net=0, layer=0):
        """GRAD_DW / _DB / _DLS: a gradient (bound or own); GRAD_ACT: the kept activations h_layer of the last call's m positions; GRAD_DELTA:
        its deltas; GRAD_PARTIAL: the float64 partials; GRAD_PACKT: the transposed packing.  A flat array (waits for the batch's streams)."""
        n = self.grad_count(what, net, layer)
        if n < 0:
            raise ValueError("grad_download: no such network, layer or kind")
        out = np.zeros(n, dtype=np.float64 if what == GRAD_PARTIAL else np.float32)
        if n and lib().phys_batch_grad_download(self._h, int(what), int(net), int(layer), out.ctypes.data) != 0:
            self._obs_fail("grad_download")
        return out

    def grad_launch_mask(self, mask=31):
        """Measurement aid: bit k set = grad() makes launch k (forward, backward, partials, reduce, statistics); 31: all, the default."""
        lib().phys_batch_debug_grad_mask(self._h, int(mask))

    def grad_launches(self):
        """Diagnostics: the launches so far of forward, backward, partials, reduce, statistics and the transposed packing."""
        a = (ctypes.c_longlong * 6)()
        lib().phys_batch_debug_grad_launches(self._h, a)
        return tuple(a)

    # ---- optimiser rows: the global-norm clip, an Adam step and the packed weights rewritten in place (phys_batch_opt_*) ----
    def configure_opt(self, beta1=0.9, beta2=0.999, eps=1e-8, max_norm=float("inf"), release=False):
        """Adam with a clip of the global gradient norm at max_norm (+inf: none) on every weight, bias and log_std the gradient rows
        differentiate (release: drop it).  Needs configure_grad; the moments start at +0.0, t at 0; waits for the batch's streams."""
        args = (0.0, 0.0, 0.0, 0.0) if release else (float(beta1), float(beta2), float(eps), float(max_norm))
        if lib().phys_batch_opt_configure(self._h, *args) != 0:
            self._obs_fail("configure_opt")

    def bind_opt_param(self, net, layer, w_ptr, w_row_stride, b_ptr):
        """The master tensors of a layer, float32 in device memory and writable: W [out][in], `w_row_stride` elements apart, as
        torch.nn.Linear.weight, and b [out].  They must hold what load_policy was last given."""
        if lib().phys_batch_opt_bind_param(self._h, int(net), int(layer), w_ptr, int(w_row_stride), b_ptr) != 0:
            self._obs_fail("bind_opt_param")

    def bind_opt_log_std(self, device_ptr):
        """The master log_std [A]: the very tensor bind_policy_sample names."""
        if lib().phys_batch_opt_bind_log_std(self._h, device_ptr) != 0:
            self._obs_fail("bind_opt_log_std")

    def opt_step(self, lr, stream=None):
        """Three launches on `stream` (default: the batch's own) behind grad(): the norm and the clip coefficient, the Adam step, and every
        new parameter into its master tensor, the policy's packed weights and the transposed packing -- policy() and the next grad()
        follow with no load_policy.  A norm that is not finite skips the call on the device.  No host synchronisation."""
        if lib().phys_batch_opt_step(self._h, float(lr), stream) != 0:
            self._obs_fail("opt_step")

    def opt_stats(self):
        """The eight statistics of the last opt_step, by name (OPT_STATS), and as an array under "all" (waits for the batch's streams)."""
        out = np.zeros(OPT_NSTATS, dtype=np.float64)
        if lib().phys_batch_opt_stats(self._h, out.ctypes.data) != 0:
            self._obs_fail("opt_stats")
        d = dict(zip(OPT_STATS, out))
        d["all"] = out
        return d

    def opt_count(self, what, net=0, layer=0):
        """The elements opt_download(what, net, layer) returns (-1: no such thing)."""
        return int(lib().phys_batch_opt_count(self._h, int(what), int(net), int(layer)))

    def opt_download(self, what, net=0, layer=0):
        """OPT_M_W / _V_W [out][in], OPT_M_B / _V_B [out] of a layer, OPT_M_LS / _V_LS [A]: the moments, float32; OPT_SCALARS: (t, p1, p2,
        skipped); OPT_PARTIALS: the norm's partials of the last call; float64.  A flat array (waits for the batch's streams)."""
        n = self.opt_count(what, net, layer)
        if n < 0:
            raise ValueError("opt_download: no such network, layer or kind")
        out = np.zeros(n, dtype=np.float64 if what in (OPT_SCALARS, OPT_PARTIALS) else np.float32)
        if n and lib().phys_batch_opt_download(self._h, int(what), int(net), int(layer), out.ctypes.data) != 0:
            self._obs_fail("opt_download")
        return out

    def opt_upload(self, what, values, net=0, layer=0):
        """What opt_download(what, net, layer) gave, back into the batch: a checkpoint restored bit for bit."""
        n = self.opt_count(what, net, layer)
        a = np.ascontiguousarray(values, dtype=np.float64 if what == OPT_SCALARS else np.float32).reshape(-1)
        if n < 0 or what == OPT_PARTIALS or a.size != n:
            raise ValueError("opt_upload: no such network, layer or kind, or not its count of elements")
        if n and lib().phys_batch_opt_upload(self._h, int(what), int(net), int(layer), a.ctypes.data) != 0:
            self._obs_fail("opt_upload")

    def opt_launch_mask(self, mask=7):
        """Measurement aid: bit k set = opt_step() makes launch k (squares, scalars, step); 7: all, the default."""
        lib().phys_batch_debug_opt_mask(self._h, int(mask))

    def opt_launches(self):
        """Diagnostics: the launches so far of the norm's squares, the scalars and the step."""
        a = (ctypes.c_longlong * 3)()
        lib().phys_batch_debug_opt_launches(self._h, a)
        return tuple(a)

    # ---- normaliser rows: the running mean and variance of the observation columns, written where the policy reads them (phys_batch_norm_*) ----
    def configure_norm(self, dim, block=256, max_rows=None, eps=1e-8, release=False):
        """Running statistics of `dim` float32 columns, summed in blocks of `block` samples (part of the definition), at most `max_rows`
        samples a call (default: the configured rollout's T steps of every env; one step without a rollout).  n, mean and m2 start at +0.0 (release: drop them).  Stays configured when the
        policy, the rollout, the gradient rows or the optimiser rows are reconfigured; waits for the batch's streams."""
        if max_rows is None:
            max_rows = (self._ro[0] if getattr(self, "_ro", None) and self._ro[1] else 1) * self.nenv
        args = (0, 0, 0, 0.0) if release else (int(dim), int(block), int(max_rows), float(eps))
        if lib().phys_batch_norm_configure(self._h, *args) != 0:
            self._obs_fail("configure_norm")

    def bind_norm_source(self, device_ptr, steps=1, rows=None, step_stride=0, row_stride=None):
        """A float32 tensor of the caller's as the source: sample step * rows + row at device_ptr + step * step_stride + row * row_stride
        words (None: the store of the rollout's OBS source again).  One policy step's live observation is steps = 1, rows = nenv."""
        if device_ptr is None:
            rc = lib().phys_batch_norm_bind_source(self._h, None, 0, 0, 0, 0)
        else:
            row = int(max(self.norm_count(NORM_N), 0) if row_stride is None else row_stride)      # (default: dense rows)
            rows = int(self.nenv if rows is None else rows)
            rc = lib().phys_batch_norm_bind_source(self._h, device_ptr, int(steps), rows, int(step_stride) if step_stride else rows * row, row)
        if rc != 0:
            self._obs_fail("bind_norm_source")

    def bind_norm_output(self, mean_ptr, inv_ptr):
        """Two float32 [dim] tensors of the caller's as the outputs (both None: the tensors bind_policy_norm names, resolved at every call)."""
        if lib().phys_batch_norm_bind_output(self._h, mean_ptr, inv_ptr) != 0:
            self._obs_fail("bind_norm_output")

    def norm_update(self, stream=None):
        """Four launches on `stream` (default: the batch's own): the source's finite values merged into the state, and every updated
        column's mean and inv written as float32 where the policy reads them -- policy() and grad() behind it on the stream act with the
        new words.  No host synchronisation."""
        if lib().phys_batch_norm_update(self._h, stream) != 0:
            self._obs_fail("norm_update")

    def norm_write(self, stream=None):
        """One launch: mean and inv of every column with n > 0 from the state, no update (what follows norm_upload of a checkpoint)."""
        if lib().phys_batch_norm_write(self._h, stream) != 0:
            self._obs_fail("norm_write")

    def norm_stats(self):
        """The eight statistics of the last norm_update, by name (NORM_STATS), and as an array under "all" (waits for the batch's streams)."""
        out = np.zeros(NORM_NSTATS, dtype=np.float64)
        if lib().phys_batch_norm_stats(self._h, out.ctypes.data) != 0:
            self._obs_fail("norm_stats")
        d = dict(zip(NORM_STATS, out))
        d["all"] = out
        return d

    def norm_count(self, what):
        """The doubles norm_download(what) returns (-1: no such thing)."""
        return int(lib().phys_batch_norm_count(self._h, int(what)))

    def norm_download(self, what):
        """NORM_N, _MEAN, _M2, _SKIPPED, _EXCLUDED, _MB, _COUNTS: float64 [dim]; NORM_PARTIALS: a1 then a2 of the last call,
        [2][blocks][dim] (waits for the batch's streams)."""
        n = self.norm_count(what)
        if n < 0:
            raise ValueError("norm_download: no such kind")
        out = np.zeros(n, dtype=np.float64)
        if n and lib().phys_batch_norm_download(self._h, int(what), out.ctypes.data) != 0:
            self._obs_fail("norm_download")
        D = self.norm_count(NORM_N)
        return out.reshape(2, n // (2 * D), D) if what == NORM_PARTIALS else out

    def norm_upload(self, what, values):
        """What norm_download(what) gave for NORM_N, _MEAN, _M2, _SKIPPED or _EXCLUDED, back into the batch; norm_write() then restores the
        two output vectors bit for bit."""
        a = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if what not in (NORM_N, NORM_MEAN, NORM_M2, NORM_SKIPPED, NORM_EXCLUDED) or a.size != self.norm_count(what):
            raise ValueError("norm_upload: no such kind, or not its count of elements")
        if lib().phys_batch_norm_upload(self._h, int(what), a.ctypes.data) != 0:
            self._obs_fail("norm_upload")

    def norm_launch_mask(self, mask=15):
        """Measurement aid: bit k set = norm_update() makes launch k (sum, mean, sq, merge); 15: all, the default."""
        lib().phys_batch_debug_norm_mask(self._h, int(mask))

    def norm_launches(self):
        """Diagnostics: the launches so far of sum, mean, sq, merge and write."""
        a = (ctypes.c_longlong * 5)()
        lib().phys_batch_debug_norm_launches(self._h, a)
        return tuple(a)

    # ---- draw rows: the policy's standard normal eps and the minibatch shuffle from one seed, every bit defined (phys_batch_draw_*) ----
    def configure_draws(self, A=None, perm_n=None, seed=0, env_base=0, release=False):
        """Standard normal float32 rows of `A` columns (default: the configured actor's output width; 0: none) and a shuffle of `perm_n`
        indices (default: the configured rollout's T steps of every env; 0: none), both keyed by `seed`; env_base: what is added to the
        env index in the counter (a rank that holds envs [k n, (k + 1) n) of a larger run passes k n).  The envs' call counts start at 0
        (release: drop them).  Stays configured when the policy, the rollout, the gradient, the optimiser or the normaliser rows are
        reconfigured; waits for the batch's streams."""
        if A is None:
            A = self._pol_out[0] if getattr(self, "_pol_out", None) else 0
        if perm_n is None:
            perm_n = self._ro[0] * self.nenv if getattr(self, "_ro", None) and self._ro[1] else 0
        args = (0, 0, 0, 0) if release else (int(A), int(perm_n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(env_base) & 0xFFFFFFFF)
        if lib().phys_batch_draw_configure(self._h, *args) != 0:
            self._obs_fail("configure_draws")

    def draw_dim(self):
        """(A, perm_n) as configured."""
        a, n = ctypes.c_int(0), ctypes.c_longlong(0)
        if lib().phys_batch_draw_dim(self._h, ctypes.byref(a), ctypes.byref(n)) != 0:
            self._obs_fail("draw_dim")
        return a.value, n.value

    def bind_draws(self, device_ptr, row_stride=None):
        """A float32 tensor of the caller's as the destination: [nenv] rows of A words, `row_stride` words (default: A) apart (None: the
        eps tensor bind_policy_sample names again, resolved at every call)."""
        stride = int(self.draw_dim()[0] if row_stride is None else row_stride) if device_ptr else 0
        if lib().phys_batch_draw_bind(self._h, device_ptr, stride) != 0:
            self._obs_fail("bind_draws")

    def bind_draw_perm(self, device_ptr):
        """An int32 tensor of the caller's of perm_n words as the shuffle's destination (None: the batch's own buffer again)."""
        if lib().phys_batch_draw_bind_perm(self._h, device_ptr) != 0:
            self._obs_fail("bind_draw_perm")

    def draw(self, env0=0, n=None, stream=None):
        """One launch on `stream` (default: the batch's own), in front of policy(): the standard normal row of every env of
        [env0, env0 + n), a function of (seed, env_base + env, column, the env's call count) alone; the count moves on.  No host
        synchronisation."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_draw(self._h, int(env0), int(n), stream) != 0:
            self._obs_fail("draw")

    def draw_perm(self, epoch, stream=None):
        """One launch on `stream`: the permutation of [0, perm_n) keyed by (seed, epoch), int32, where draw_perm_ptr() points; minibatch k
        of M samples is grad(draw_perm_ptr() + 4 * k * M, M).  No host synchronisation."""
        if lib().phys_batch_draw_perm(self._h, int(epoch) & 0xFFFFFFFF, stream) != 0:
            self._obs_fail("draw_perm")

    def draw_perm_ptr(self):
        """The device address of the permutation: the bound tensor's, or the batch's own buffer's."""
        p = lib().phys_batch_draw_perm_ptr(self._h)
        if not p:
            raise RuntimeError("draw_perm_ptr failed: no shuffle is configured (configure_draws with perm_n first)")
        return int(p)

    def draws(self):
        """The destination's rows downloaded: float32 [nenv][A] (waits for the batch's streams)."""
        out = np.empty((self.nenv, self.draw_dim()[0]), dtype=np.float32)
        if lib().phys_batch_draw_rows(self._h, out.ctypes.data) != 0:
            self._obs_fail("draws")
        return out

    def draw_perm_values(self):
        """The permutation downloaded: int32 [perm_n] (waits for the batch's streams)."""
        out = np.empty(self.draw_dim()[1], dtype=np.int32)
        if lib().phys_batch_draw_perm_rows(self._h, out.ctypes.data) != 0:
            self._obs_fail("draw_perm_values")
        return out

    def draw_state(self):
        """counts uint32 [nenv]: the draws every env has seen, the third word of the counter.  With the seed and the caller's epoch
        counter, a checkpoint of the run's randomness."""
        counts = np.empty(self.nenv, dtype=np.uint32)
        if lib().phys_batch_draw_download(self._h, counts.ctypes.data) != 0:
            self._obs_fail("draw_state")
        return counts

    def set_draw_state(self, counts):
        k = np.ascontiguousarray(counts, dtype=np.uint32).reshape(self.nenv)
        if lib().phys_batch_draw_upload(self._h, k.ctypes.data) != 0:
            self._obs_fail("set_draw_state")

    def draw_launches(self):
        """Diagnostics: the launches so far of draw() and of draw_perm()."""
        a = (ctypes.c_longlong * 2)()
        lib().phys_batch_debug_draw_launches(self._h, a)
        return tuple(a)

    def set_pd_mode(self, on=True):
        lib().phys_batch_set_pd_mode(self._h, 1 if on else 0)

    def set_drive_mode(self, mode):
        """DRIVE_OFF / DRIVE_TORQUE (cassie_sim_step_ethercat on the device) / DRIVE_PD (pd_input's motor PD on the encoder
        measurements): the encoder + motor models of reference src/cassiemujoco.c:558-664 run in the step kernel."""
        if lib().phys_batch_set_drive_mode(self._h, int(mode)) != 0:
            raise RuntimeError("set_drive_mode failed: " + (lib().phys_last_error() or b"").decode())

    def derive(self, ids, stream=None):
        """Batched derived getters: one forward pass + a reduction kernel fill F_DERIVED and F_QM for every env.
        ids = (left foot body, right foot body, left heel site, right heel site, left toe site, right toe site), -1 = absent."""
        arr = (ctypes.c_int * 6)(*[int(i) for i in ids])
        if lib().phys_batch_derive(self._h, arr, stream) != 0:
            raise RuntimeError("derive failed: " + (lib().phys_last_error() or b"").decode())

    def drive_pass(self, mode=DRIVE_TORQUE, stream=None):
        """The drive-level models alone (no physics): reads the command / PD fields and the last step's sensordata and
        actuator_velocity, writes F_CTRL, F_MEAS and the drive state."""
        if lib().phys_batch_drive_pass(self._h, int(mode), stream) != 0:
            raise RuntimeError("drive_pass failed: " + (lib().phys_last_error() or b"").decode())

    def clear_drive_state(self, first=0, stride=1, count=None, stream=None):
        count = (self.nenv - first + stride - 1) // stride if count is None else count
        if lib().phys_batch_clear_drive_state(self._h, first, stride, count, stream) != 0:
            raise RuntimeError("clear_drive_state failed")

    def reset_envs(self, first, stride, count, qpos_row_ptr, sens_row_ptr=None, stream=None):
        """Episode restart of envs first, first + stride, ... on the device in one launch (phys_batch_reset_envs): qpos from
        the device row `qpos_row_ptr`, velocities / warm start / ctrl / time zero, drive-level state and measurement block
        zero, sensordata from `sens_row_ptr` if given."""
        if lib().phys_batch_reset_envs(self._h, int(first), int(stride), int(count), qpos_row_ptr, sens_row_ptr, stream) != 0:
            raise RuntimeError("reset_envs failed: " + (lib().phys_last_error() or b"").decode())

    # ---- episodes that end and restart on the device (phys_batch_end_episodes) ----
    def enable_episodes(self, min_height=-np.inf, min_upright=-np.inf, max_steps=0, warn_mask=0, nonfinite=False):
        """Allocates the per-env episode arrays (first call) and sets the termination rules; every rule is off by default:
        pelvis height qpos[2] < min_height, pelvis z axis' world-z component 1 - 2 (qx^2 + qy^2) < min_upright, episode step counter
        >= max_steps, (warning word & warn_mask) != 0 (WARN_DIVERGED: MuJoCo's auto-reset), any non-finite qpos / qvel entry."""
        r = CmEpisodeRules(min_height=float(min_height), min_upright=float(min_upright), max_steps=int(max_steps),
                           warn_mask=int(warn_mask), nonfinite=1 if nonfinite else 0)
        if lib().phys_batch_episodes_enable(self._h, ctypes.byref(r)) != 0:
            raise RuntimeError("enable_episodes failed: " + (lib().phys_last_error() or b"").decode())

    def episode_row_dim(self):
        """Doubles per row of the bank of start states: qpos | qvel | sensordata | actuator_velocity | qacc."""
        return lib().phys_batch_episode_row_dim(self._h)

    def make_reset_bank(self, qpos, qvel=None):
        """The bank rows [K][episode_row_dim()] of K start states: a K-env batch of the same (shared) model is set to qpos[K] /
        qvel[K] (default zero) and run through forward() on the GPU, which gives the sensordata / actuator_velocity / qacc a
        restarted env needs to continue exactly like a fresh one.  Hand the result to set_reset_bank."""
        pod = self.pod
        q = np.ascontiguousarray(qpos, dtype=np.float64).reshape(-1, pod.nq)
        v = np.zeros((q.shape[0], pod.nv)) if qvel is None else np.ascontiguousarray(qvel, dtype=np.float64).reshape(-1, pod.nv)
        if v.shape[0] != q.shape[0]:
            raise ValueError("make_reset_bank: qpos and qvel need the same number of rows")
        t = Batch(self.model, q.shape[0], self.device)
        try:
            t.set(F_QPOS, q)
            t.set(F_QVEL, v)
            t.forward()
            return np.concatenate([t.get(f) for f in (F_QPOS, F_QVEL, F_SENSORDATA, F_ACTUATOR_VELOCITY, F_QACC)], axis=1)
        finally:
            t.close()

    def set_reset_bank(self, rows=None, device_ptr=None, n=None):
        """The start states restarted envs take: host `rows` [K][episode_row_dim()] (copied; waits for the batch's streams), or
        `device_ptr` and n for rows already in HBM (used in place: keep them alive; they may be rewritten in stream order)."""
        if device_ptr is not None:
            if n is None:
                raise ValueError("set_reset_bank: device_ptr needs n, the number of rows")
            rc = lib().phys_batch_episodes_set_bank(self._h, device_ptr, 1, int(n))
        else:
            a = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, self.episode_row_dim())
            rc = lib().phys_batch_episodes_set_bank(self._h, a.ctypes.data, 0, a.shape[0])
        if rc != 0:
            raise RuntimeError("set_reset_bank failed: " + (lib().phys_last_error() or b"").decode())

    def end_episodes(self, env0=0, n=None, restart=True, pick_ptr=None, force_ptr=None, stream=None):
        """One small launch on `stream` (default: the batch's own), in order with the step launches there and with no host read:
        for every env of [env0, env0 + n) counts the policy step, evaluates the rules on the env's own state (| DONE_FORCED where
        the int32 device array force_ptr[n] is non-zero), writes EP_DONE / EP_REASON, and for the envs that ended keeps the
        terminal state, counts the episode and -- with `restart` -- restarts them from bank row pick_ptr[i] (int32 device array
        [n]; default (env + episodes ended) % rows): state from the row, time / ctrl / warm start / drive-level state /
        measurement block zero, warning word clear.

        Once configure_placement has named an anchor, a restart is PLACED (include/cassie_phys.h: "placed restarts"): the env first takes
        its next terrain (PLACE_NEXT_TERRAIN, if bound and a bank is set), the row's moving root bodies -- the pelvis, the cube of
        cassie_tray_box -- are turned by the env's yaw about the vertical through the anchor and shifted by (dx, dy, dz + G - ground_ref),
        G = the highest ground under the placed footprint (PLACE_GROUND[env]; ground_ref without a footprint or where nothing is hit,
        then with WARN_PLACE_MISS); their linear qvel / qacc entries, the framequat and the magnetometer are turned along, every other
        entry is the row's (the accelerometer, qacc and rangefinders are those of the ground the row was recorded on until the first
        substep replaces them); the warning word is cleared and then holds WARN_TERRAIN_INDEX / WARN_SCAN_TILTED / WARN_PLACE_MISS as
        the placement raised them.  The pose (0, 0, 0, 0) with no footprint leaves what an unplaced restart leaves."""
        n = self.nenv - env0 if n is None else n
        if lib().phys_batch_end_episodes(self._h, int(env0), int(n), 1 if restart else 0, pick_ptr, force_ptr, stream) != 0:
            raise RuntimeError("end_episodes failed: " + (lib().phys_last_error() or b"").decode())

    # ---- placed restarts (phys_batch_place_configure) ----
    def configure_placement(self, anchor, footprint_xy=None, ground_ref=0.0):
        """Restarts of end_episodes are placed from now on: `anchor` is a child of the world whose pose follows from qpos alone (Cassie's
        pelvis: pod.root_body[0]); footprint_xy [P][2] (P <= PLACE_MAXPOINTS; None or empty: no ground following) are the points, in the
        anchor's heading frame after placement, under which the ground is looked up; ground_ref is the world z of the ground the bank's
        rows were recorded on.  anchor <= 0 turns placement off again.  Waits for the batch's streams."""
        a = np.zeros((0, 2)) if footprint_xy is None else np.ascontiguousarray(footprint_xy, dtype=np.float64)
        if a.size == 0:
            a = a.reshape(0, 2)
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("configure_placement: footprint_xy must be [P][2]")
        if lib().phys_batch_place_configure(self._h, int(anchor), a.ctypes.data if a.shape[0] else None, a.shape[0], float(ground_ref)) != 0:
            raise ValueError("configure_placement failed: " + (lib().phys_last_error() or b"").decode())

    def placement_ptr(self, which):
        """Device pointer of a placement array: PLACE_POSE float64 [nenv][4] (dx, dy, dz, yaw), PLACE_GROUND float64 [nenv], or the bound
        PLACE_NEXT_TERRAIN int32 [nenv] (None while none is bound: the batch keeps none of its own)."""
        return lib().phys_batch_place_ptr(self._h, int(which))

    def bind_placement(self, which, device_ptr):
        """Caller-owned HBM (a torch tensor's data_ptr()) in the place of a placement array; None un-binds: the batch's own array again
        (zeros), for PLACE_NEXT_TERRAIN none -- restarts then leave the terrain index alone."""
        if lib().phys_batch_place_bind(self._h, int(which), device_ptr) != 0:
            raise RuntimeError("bind_placement failed: " + (lib().phys_last_error() or b"").decode())

    def set_placement(self, poses, env0=0):
        """Host upload of spawn poses [n][4] = (dx, dy, dz, yaw) for envs env0 ... into PLACE_POSE (the batch's own array or the bound
        one); waits for the batch's streams."""
        a = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
        if env0 < 0 or env0 + a.shape[0] > self.nenv:
            raise ValueError("set_placement: envs [%d, %d) are not in the batch" % (env0, env0 + a.shape[0]))
        if lib().phys_batch_place_upload(self._h, PLACE_POSE, a.ctypes.data, int(env0), a.shape[0]) != 0:
            raise RuntimeError("set_placement failed: " + (lib().phys_last_error() or b"").decode())

    def placement_ground(self):
        """PLACE_GROUND downloaded: the ground height found at every env's last placed restart; waits for the batch's streams."""
        out = np.zeros(self.nenv)
        if lib().phys_batch_place_download(self._h, PLACE_GROUND, out.ctypes.data) != 0:
            raise RuntimeError("placement_ground failed: " + (lib().phys_last_error() or b"").decode())
        return out

    def episode_ptr(self, which):
        """Device pointer of an episode array (EP_DONE / EP_REASON / EP_STEPS / EP_COUNT: int32 [nenv]; EP_TERMINAL: float64
        [nenv][nq + nv])."""
        return lib().phys_batch_episode_ptr(self._h, int(which))

    def bind_episode(self, which, device_ptr):
        """Caller-owned HBM (e.g. a torch tensor the policy reads) in the place of an episode array."""
        if lib().phys_batch_episode_bind(self._h, int(which), device_ptr) != 0:
            raise RuntimeError("bind_episode failed: " + (lib().phys_last_error() or b"").decode())

    def episodes(self):
        """(done, reason, steps, count, terminal) downloaded; waits for the batch's streams."""
        out = []
        for which in (EP_DONE, EP_REASON, EP_STEPS, EP_COUNT, EP_TERMINAL):
            a = (np.empty((self.nenv, self.pod.nq + self.pod.nv), dtype=np.float64) if which == EP_TERMINAL
                 else np.empty(self.nenv, dtype=np.int32))
            if lib().phys_batch_download_episodes(self._h, which, a.ctypes.data) != 0:
                raise RuntimeError("episode download failed: " + (lib().phys_last_error() or b"").decode())
            out.append(a)
        return tuple(out)

    # ---- a bank of full states: save, rewind and fork envs on the device (phys_batch_state_*) ----
    def _err(self, what):
        return RuntimeError(what + " failed: " + (lib().phys_last_error() or b"").decode())

    def configure_states(self, nslots, groups=STATE_CORE):
        """Allocates a bank of `nslots` rows of full env states in HBM (include/cassie_phys.h: "a bank of full states").  STATE_CORE is
        always in a row: everything a stepping launch leaves for the next one or for a reader -- time, qpos, qvel, warm start, ctrl, qacc,
        sensordata, actuator_velocity, F_MEAS, the drive-level state, F_XPOS / F_XQUAT and the warning word -- so that a restored env
        continues byte for byte as the saved one did.  Optional: STATE_COMMANDS (the PD fields, F_DRIVE_CMD, the applied forces: upload or
        bind those first), STATE_EPISODE (EP_STEPS, EP_COUNT, the terrain index: enable_episodes first), STATE_PARAMS (the env's parameter
        block: randomize first; without it a restored env keeps its own masses, friction, ...).  Not in a row: per-env terrains and models,
        outputs (F_BODY_CFRC, info, ext, derived, the step sums).  Waits for the batch's streams; calling it again replaces the bank."""
        if lib().phys_batch_state_configure(self._h, int(nslots), int(groups)) != 0:
            raise ValueError("configure_states failed: " + (lib().phys_last_error() or b"").decode())

    def state_row_dim(self):
        """8-byte words per row of the bank (0 before configure_states)."""
        return lib().phys_batch_state_row_dim(self._h)

    def state_layout(self):
        """name -> (offset, count, dtype) of the sections in this bank's rows, offset and count in 8-byte words (STATE_SECTIONS: float64
        sections hold count values; int32 sections one value in the low half of their word; 'drive_state' and 'params' the bytes of
        cm_drive_state_t / cm_envparams_t).  Every offset is even: rows and sections start on 16-byte boundaries."""
        oc = (ctypes.c_int * (2 * len(STATE_SECTIONS)))()
        if lib().phys_batch_state_layout(self._h, oc) != len(STATE_SECTIONS):
            raise self._err("state_layout")
        return {name: (oc[2 * s], oc[2 * s + 1], dt) for s, (name, dt) in enumerate(STATE_SECTIONS) if oc[2 * s] >= 0}

    def state_signature(self):
        """Hash of the layout version, the groups, the row dim and the batch's compiled model: what rows saved elsewhere must come with."""
        return int(lib().phys_batch_state_signature(self._h))

    def _state_call(self, fn, what, slots, env0, n, slots_ptr, stream):
        n = self.nenv - env0 if n is None else int(n)
        if slots is not None:
            if slots_ptr is not None:
                raise ValueError(what + ": give slots (a host array) or slots_ptr (device int32), not both")
            a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
            if a.shape[0] != n:
                raise ValueError("%s: %d slots for %d envs" % (what, a.shape[0], n))
            if n > 0:
                slots_ptr = lib().phys_batch_state_stage_slots(self._h, a.ctypes.data, n)   # (waits for the batch's streams)
                if not slots_ptr:
                    raise self._err(what)
        if fn(self._h, int(env0), n, slots_ptr, stream) != 0:
            raise self._err(what)

    def save_states(self, slots=None, env0=0, n=None, slots_ptr=None, stream=None):
        """One small launch on `stream` (default: the batch's own), in order with the step launches there, no host read: env env0 + i goes
        to bank slot slots_ptr[i] (a DEVICE int32 [n], e.g. a torch tensor's data_ptr(); default: slot env0 + i).  A negative slot skips
        the env, a slot >= nslots skips it and raises WARN_STATE_SLOT.  A host array `slots` is uploaded first, which waits for the
        batch's streams: a convenience outside the hot loop."""
        self._state_call(lib().phys_batch_state_save, "save_states", slots, env0, n, slots_ptr, stream)

    def restore_states(self, slots=None, env0=0, n=None, slots_ptr=None, stream=None):
        """The reverse, same arguments: env env0 + i takes slot slots_ptr[i] and then continues byte for byte as the env saved there did
        (negative: left alone; out of range: left alone, WARN_STATE_SLOT).  Any number of envs may take one slot: a fork is save_states
        followed by restore_states on the same stream."""
        self._state_call(lib().phys_batch_state_restore, "restore_states", slots, env0, n, slots_ptr, stream)

    def states(self, slot0=0, n=None):
        """(rows, signature): bank rows [slot0, slot0 + n) as an int64 array [n][state_row_dim()] and the signature set_states asks for
        (numpy.save the pair to keep states across processes); waits for the batch's streams."""
        nslots = lib().phys_batch_state_nslots(self._h)
        n = nslots - slot0 if n is None else int(n)
        out = np.empty((max(n, 0), self.state_row_dim()), dtype=np.int64)
        if lib().phys_batch_state_download(self._h, int(slot0), n, out.ctypes.data) != 0:
            raise self._err("states")
        return out, self.state_signature()

    def set_states(self, rows, slot0=0, signature=None):
        """Host rows [n][state_row_dim()] (int64, as states() returns them) into bank slots slot0 ...; `signature` is the one the rows
        came with (default: this batch's own -- rows it saved itself) and must equal state_signature(), else the rows belong to another
        model, other groups or another layout version and are refused.  Waits for the batch's streams."""
        a = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, self.state_row_dim())
        sig = self.state_signature() if signature is None else int(signature)
        if lib().phys_batch_state_upload(self._h, int(slot0), a.shape[0], a.ctypes.data, sig) != 0:
            raise ValueError("set_states failed: " + (lib().phys_last_error() or b"").decode())

    def bind_states(self, ptr, nslots):
        """Caller-owned HBM [nslots][state_row_dim()] of 8-byte words (a torch int64 tensor's data_ptr(), 16-byte aligned) in the bank's
        place; configure_states first (it fixes the groups); None un-binds: the batch's own bank again."""
        if lib().phys_batch_state_bind(self._h, ptr, int(nslots)) != 0:
            raise ValueError("bind_states failed: " + (lib().phys_last_error() or b"").decode())

    def state_ptr(self):
        """Device pointer of the bank in use (None before configure_states)."""
        return lib().phys_batch_state_ptr(self._h)

    def get_drive_state(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        out = (CmDriveState * n)()
        if lib().phys_batch_download_drive_state(self._h, ctypes.byref(out), env0, n) != 0:
            raise RuntimeError("drive state download failed")
        return out

    def set_drive_state(self, states, env0=0):
        if lib().phys_batch_upload_drive_state(self._h, ctypes.byref(states), env0, len(states)) != 0:
            raise RuntimeError("drive state upload failed")

    def sync(self):
        if lib().phys_batch_sync(self._h) != 0:
            raise RuntimeError("sync failed: " + (lib().phys_last_error() or b"").decode())

    def time_steps(self, nsub, reps):
        """Mean milliseconds per launch of `nsub` steps, measured with HIP events on the launch stream."""
        ms = ctypes.c_float(0)
        if lib().phys_batch_time_steps(self._h, nsub, reps, ctypes.byref(ms)) != 0:
            raise RuntimeError("timing failed: " + (lib().phys_last_error() or b"").decode())
        return ms.value

    def set_balance(self, on=True):
        """Longest-job-first launch order from the previous launch's per-env cost (default on for >= 2048 envs)."""
        lib().phys_batch_set_balance(self._h, 1 if on else 0)

    def enable_kernel_timing(self, on=True):
        lib().phys_batch_enable_kernel_timing(self._h, 1 if on else 0)

    def kernel_timing(self):
        """(launches, total ms) of the work-doing kernel of every stepping launch since the last call (HIP event pairs)."""
        n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        if lib().phys_batch_kernel_timing(self._h, ctypes.byref(n), ctypes.byref(ms)) != 0:
            raise RuntimeError("kernel timing failed")
        return n.value, ms.value

    def set_fast_rows(self, on=True):
        """Row-capped fast kernel ahead of the full one (default on; results are bit for bit the same either way)."""
        lib().phys_batch_set_fast_rows(self._h, 1 if on else 0)

    def set_inplace(self, mode=2):
        """Form of the two-wave fast kernel: 0 = kernel + list-walking pass, 1 = finishes the substeps it cannot hold in place,
        2 = per env range by what its recent launches needed (default).  Same results bit for bit."""
        if lib().phys_batch_set_inplace(self._h, int(mode)) != 0:
            raise ValueError("in-place mode: 0, 1 or 2")

    def form_launches(self):
        """Diagnostics: (plain, in place) -- stepping launches of the two-wave fast kernel so far, by form."""
        import ctypes
        a, c_ = ctypes.c_longlong(0), ctypes.c_longlong(0)
        lib().phys_batch_debug_form_launches(self._h, ctypes.byref(a), ctypes.byref(c_))
        return int(a.value), int(c_.value)

    def inplace_ranges(self):
        """Diagnostics: env ranges whose next stepping launch takes the in-place form of the fast kernel."""
        return lib().phys_batch_debug_inplace_ranges(self._h)

    def set_waves_per_env(self, waves=2):
        """Two-wave form of the fast kernels (default 2; results are bit for bit the same either way)."""
        if lib().phys_batch_set_waves_per_env(self._h, int(waves)) != 0:
            raise ValueError("waves per env: 1 or 2")

    def set_chunks(self, chunks=4):
        """Stepping launches of the fast kernels as `chunks` workgroups per env (1 = off); results are bit for bit the same."""
        if lib().phys_batch_set_chunks(self._h, int(chunks)) != 0:
            raise ValueError("chunks per env-launch: 1 .. 7")

    def enable_step_sums(self, on=True):
        """The step sums: while on, every stepping launch (step, step_range) zeroes the rows of its env range of F_STEP_SUMS on its
        stream and then adds up, over the substeps it integrates, each body's net contact force (what F_BODY_CFRC holds for the last
        substep alone), the substeps in which the body touched anything, the largest squared force, and per actuator the applied
        torque, its square, the mechanical power and its positive part -- sequential sums in substep order, whatever tier or chunk of
        the launch finished a substep (layout: SUM_*; exact definitions: CM_SUM_* in csrc/cm_model.h).  Forward passes, derive(),
        end_episodes() and restarts leave the block alone.  Off by default, and off again restores the launches as they were.
        The block is allocated on first use unless a tensor is bound to the field (bind(F_STEP_SUMS, ptr): [nenv][SUM_DIM] float64)."""
        if not hasattr(lib(), "phys_batch_step_sums_enable"):
            raise RuntimeError("this build of the library has no step sums")
        if lib().phys_batch_step_sums_enable(self._h, 1 if on else 0) != 0:
            raise RuntimeError("enable_step_sums failed: " + (lib().phys_last_error() or b"").decode())

    def step_sums(self, env0=0, n=None):
        """The rows [env0, env0 + n) of F_STEP_SUMS as named views of one download: count [n], body_cfrc [n][nbody][3], body_touch
        [n][nbody], body_cfrc_max2 [n][nbody], act_force / act_force2 / act_power / act_pospower [n][nu], and the rows themselves
        under "raw".  Means are the caller's: divide by count.  An env whose launch diverged (WARN_DIVERGED): count is the number of
        substeps it finished, the rest is unspecified."""
        raw = self.get(F_STEP_SUMS, env0, n)
        nb, nu = self.pod.nbody, self.pod.nu
        per_body = lambda at, w=1: raw[:, at:at + w * MAXBODY].reshape(raw.shape[0], MAXBODY, w)[:, :nb]
        out = dict(raw=raw, count=raw[:, SUM_COUNT], body_cfrc=per_body(SUM_BODY_CFRC, 3), body_touch=per_body(SUM_BODY_TOUCH)[:, :, 0],
                   body_cfrc_max2=per_body(SUM_BODY_CFRC_MAX2)[:, :, 0])
        for name, at in (("act_force", SUM_ACT_FORCE), ("act_force2", SUM_ACT_FORCE2), ("act_power", SUM_ACT_POWER), ("act_pospower", SUM_ACT_POSPOWER)):
            out[name] = raw[:, at:at + nu]
        return out

    def launch_cost(self):
        """Shader clocks every env's last stepping launch took, first to last instruction (diagnostics; batches >= 2048 envs)."""
        out = np.zeros(self.nenv, dtype=np.uint32)
        if lib().phys_batch_download_cost(self._h, out.ctypes.data) != 0:
            raise RuntimeError("cost download failed (balancing is off or the batch is small)")
        return out.astype(np.float64) * 64.0

    def measured_shader_clock(self):
        """Hz the last stepping launch ran at: the envs' spans in shader clocks over the same spans on the 100 MHz clock
        (None where the launch-cost arrays do not exist: small batches, balancing off)."""
        import ctypes
        hz = ctypes.c_double(0.0)
        if lib().phys_batch_measured_shader_clock(self._h, ctypes.byref(hz)) != 0:
            return None
        return float(hz.value)

    def wide_pass_envs(self, env0=0):
        """Envs that the last stepping launch over the env range starting at env0 passed on to the 127-row instantiation (they met a
        substep with more than 63 constraint rows or 16 contacts); waits for the batch's streams."""
        r = lib().phys_batch_wide_pass_envs(self._h, int(env0))
        if r < 0:
            raise RuntimeError("phys_batch_wide_pass_envs failed")
        return r

    def handover_pending(self):
        """Validation aid: entries left in the hand-over lists once the batch's streams are idle (0 in every mode)."""
        r = lib().phys_batch_debug_handover_pending(self._h)
        if r < 0:
            raise RuntimeError("hand-over count download failed")
        return r

    def fast_rows_progress(self):
        """Substeps of the last stepping launch the fast kernel completed per env (< the launch's count: handed over there)."""
        out = np.zeros(self.nenv, dtype=np.int32)
        if lib().phys_batch_download_progress(self._h, out.ctypes.data) != 0:
            raise RuntimeError("progress download failed")
        return out

    def set_all_outputs_every_substep(self, on=True):
        """Measurement aid: every substep of a fused launch evaluates every output (IMU sensors, body quaternions), not only
        the substeps whose values can be read."""
        lib().phys_batch_set_all_outputs_every_substep(self._h, 1 if on else 0)

    def poison_lds(self):
        """Validation aid: NaN bit patterns into every CU's LDS before the next launch."""
        if lib().phys_batch_debug_poison_lds(self._h) != 0:
            raise RuntimeError("poison failed")

    def set_generic_kernel(self, on=True):
        """Validation aid: use the run-time-topology instantiation of the step kernel."""
        lib().phys_batch_set_generic_kernel(self._h, 1 if on else 0)

    def profile_step(self, nsub=1):
        """Runs one launch of `nsub` fused substeps and returns the per-env shader-clock stamps [nenv][48] taken at the
        stage boundaries of the last substep."""
        st = np.zeros((self.nenv, 48), dtype=np.int64)
        if lib().phys_batch_profile_substeps(self._h, int(nsub), st.ctypes.data) != 0:
            raise RuntimeError("profile_step failed")
        return st

    def close(self):
        if self._h:
            lib().phys_batch_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
