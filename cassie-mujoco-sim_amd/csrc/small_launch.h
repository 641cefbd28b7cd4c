/*
 * small_launch.h -- how the kernels around the step kernel (small_kernels.h, surface_kernels.h, depth_kernel.h, ray_kernel.h, episode_kernels.h, probe_kernels.h, obs_kernels.h, reward_kernels.h, act_kernels.h, task_kernels.h, event_kernels.h, policy_kernels.h, rollout_kernels.h, grad_kernels.h, opt_kernels.h, norm_kernels.h, draw_kernels.h) are
 * launched: the records a kernel's arguments are built from, one builder per kernel that returns its filled argument struct for an env
 * range, the grid of every launch, and the checks of what a caller configures, each returning the message of its refusal (null: fine).
 * Pure host code, no HIP runtime calls, in the spirit of step_policy.h: the launcher (phys_batch.hip) keeps the records in the batch,
 * prefixes a message with its entry point's name and launches what a builder returns on the grid given here; the wave emulator's entry
 * points (tests/emu) fill the same records from their arguments and go through the same builders, grids and checks, so a CPU test of
 * one of these kernels also runs the launcher's refusals, grid and choice of kernel (tests/test_small_launch.py pins them one by one).
 * No field of ScanIO, DepthIO, RayIO, EpisodeIO, ResetIO, DeriveIO, SetConstIO, StateIO, ProbeIO, ObsIO, RewardIO, ActIO, TaskIO, EventIO, PolicyIO, PolicyPackIO, RolloutRecIO, RolloutFinIO, RolloutNormIO, GradIO, GradPackIO, OptIO, NormIO, DrawIO or DrawPermIO is assigned anywhere else.
 */
#ifndef CASSIE_SMALL_LAUNCH_H
#define CASSIE_SMALL_LAUNCH_H

#include <cmath>
#include <cstring>

#include "act_kernels.h"
#include "depth_kernel.h"
#include "draw_kernels.h"
#include "episode_kernels.h"
#include "event_kernels.h"
#include "grad_kernels.h"
#include "opt_kernels.h"
#include "norm_kernels.h"
#include "obs_kernels.h"
#include "policy_kernels.h"
#include "probe_kernels.h"
#include "ray_kernel.h"
#include "reward_kernels.h"
#include "rollout_kernels.h"
#include "small_kernels.h"
#include "state_kernels.h"
#include "task_kernels.h"

namespace ck {

/* ---- the records ---- */

/* What the kernels read of the batch, whatever they compute.  The surface source: the model(s), the envs' parameter blocks (null: the
 * model's own), the height field(s) and -- while a bank of terrains is set, hfield_nterrain > 0 -- the envs' index into it, which a
 * placed restart WRITES; all as the fields of PhysIO of the same names.  The state rows: the model's sizes, the doubles between the rows
 * of qpos / qvel / sensordata, the arrays a restart writes (meas, drive: null until a drive mode is in use), the sticky warning word, and
 * the body poses the last step launch or forward pass stored (rows of 3 nbody / 4 nbody doubles).  Appended for the bank of full states
 * (state_layout below), which restores what every other kernel here only reads: the poses again, writable; the command fields (dense rows;
 * the applied forces null until uploaded or bound, as the step kernel is handed them); the episode counters (null until episodes are
 * enabled); the parameter blocks, writable. */
struct BatchView {
    const cm_model_t *models; int model_stride;
    const cm_envparams_t *envparams;
    const float *hfield; size_t hfield_stride; int *hfield_index; int hfield_nterrain;
    int nq, nv, nu, nsd, nbody, sq, sqv, ssd;
    double *qpos, *qvel, *warm, *ctrl, *qacc, *time, *sens, *actvel, *meas;
    cm_drive_state_t *drive;
    int *warn;
    const double *xpos, *xquat;
    double *xpos_w, *xquat_w;
    double *pd_ptarget, *pd_kp, *pd_kd, *pd_dtarget, *pd_torque, *drive_cmd, *qfrc_applied, *xfrc_applied;
    int *ep_steps, *ep_count;
    cm_envparams_t *params_w;
};
/* the sizes of a view from the (host's copy of the) shared model, with dense rows */
inline void view_sizes(BatchView &v, const cm_model_t &m) {
    v.nq = m.nq; v.nv = m.nv; v.nu = m.nu; v.nsd = m.nsensordata; v.nbody = m.nbody; v.sq = m.nq; v.sqv = m.nv; v.ssd = m.nsensordata;
}
/* the height scan (phys_batch_scan_configure; npoints 0: not configured): the pattern [npoints][2], its body and range */
struct ScanCfg { int npoints, body; double range; const double *offsets; };
/* the depth image (phys_batch_depth_configure; width 0: not configured): the camera on its body, tan(fovy / 2), the caller's per-env
 * extrinsics (null: the shared pose), the geoms it renders and the caller's hit-id image (null: none) */
struct DepthCfg { int width, height, body; double tan_half, znear, zfar, cam_pos[3], cam_quat[4]; const double *pose; unsigned geoms; int *ids; };
/* the range sensors (phys_batch_rays_configure; nrays 0: not configured): the table [nrays] (where it lies once a kernel reads it, which
 * the caller names), the range, the geoms they see and the caller's hit ids / normals (null: none) */
struct RayCfg { int nrays; double rmin, rmax; const RayDef *rays; unsigned geoms; int *ids; double *normals; };
/* placed restarts (phys_batch_place_configure; anchor 0: off): the footprint [npoints][2], the table of what a placement moves, and the
 * per-env arrays: poses [nenv][4], next terrains [nenv] (null: none bound), ground heights [nenv] */
struct PlaceCfg { int anchor, npoints; double ground_ref; const PlaceTable *table; const double *offsets, *pose; const int *next; double *ground; };
/* episodes (phys_batch_episodes_enable): the rules, the per-env arrays and the bank of start states [nrows][episode_row_dim] */
struct EpisodeCfg { cm_episode_rules_t rules; int *done, *reason, *steps, *count; double *terminal; const double *bank; int nrows; };
/* the bank of full states (phys_batch_state_configure, _bind; nslots 0: not configured): the groups of its rows (STATE_* below) and the
 * rows [nslots][state_layout().row_dim] of 8-byte words */
struct StateCfg { int nslots, groups; unsigned long long *bank; };
/* the probes (phys_batch_probes_configure; nprobes 0: not configured): the table [nprobes] and the quantities as configured; then what the
 * caller names once a kernel reads them: where the table lies, the classes of the geoms of the full list [ngeom] (null: none were given),
 * what the probes' own forward pass leaves -- its read-out block [nenv], its body poses (dense rows of 3 nbody / 4 nbody doubles) and its
 * qacc (dense rows of nv) -- and the contact words [nenv] (null: not asked for) */
struct ProbeCfg {
    int nprobes; unsigned quantities; const ProbeDef *probes; const int *geom_class; int ngeom;
    const cm_ext_t *ext; const double *xpos, *xquat, *qacc; int *contacts;
};

/* the observation rows (phys_batch_obs_configure; nterms 0: not configured): the frame's columns, the frames of a row, the rows' type
 * (OBS_F32 / OBS_F64), the noise's seed and the offset of its env counter; the sources of a call -- slot s is field slot_field[s] (or
 * OBS_INPUT), whose row held slot_dim[s] elements when the terms were checked against it -- and the elements the input terms need of the
 * caller's array.  Then what the caller names once a kernel reads them: the column table [ncols], the rows with their stride in elements,
 * the counts [nenv], and the caller's input array (null: none bound) with its row length, row stride and type */
struct ObsCfg {
    int nterms, ncols, history, dtype, nslots, input_need;
    unsigned long long seed; unsigned env_base;
    int slot_field[OBS_MAXSLOTS], slot_dim[OBS_MAXSLOTS];
    const ObsCol *cols; void *rows; long long srow; unsigned *frames;
    const void *input; int input_dim, input_stride, input_dtype;
};
/* what the batch holds of a field: its rows (null: the batch does not hold it yet), their length and the doubles between two of them */
struct ObsField { const double *base; int dim, stride; };

/* the reward rows (phys_batch_reward_configure; nterms 0: not configured): the terms, the type of the rewards and the term rows (OBS_F32 /
 * OBS_F64), the clip; the sources of a call as the observation's -- slot s is field slot_field[s] (or REW_INPUT), whose row held
 * slot_dim[s] elements when the terms were checked against it -- and the elements the terms need of the caller's input array.  Then what
 * the caller names once a kernel reads them: the term table [nterms] with the fields as slots, the rewards with their stride in
 * elements, the term rows (null: not written) with theirs, the returns and final returns [nenv], and the caller's input array (null:
 * none bound) with its row length, row stride and type */
struct RewardCfg {
    int nterms, dtype, nslots, input_need;
    double lo, hi;
    int slot_field[REWARD_MAXSLOTS], slot_dim[REWARD_MAXSLOTS];
    const RewardTerm *terms; void *rew; long long srew; void *trows; long long sterm; double *ret, *fin;
    const void *input; int input_dim, input_stride, input_dtype;
};

/* the action rows (phys_batch_act_configure; ncols 0: not configured): the columns, the depth of the delay line, the rows' type (OBS_F32 /
 * OBS_F64), the noise's seed and the offset of its env counter; the sources of a call as the observation's -- slot s is field
 * slot_field[s] (or ACT_INPUT), whose row held slot_dim[s] elements when the columns were checked against it -- the destinations of a
 * call -- slot s is the command field dst_field[s], whose row held dst_dim[s] -- and the elements the INPUT columns need of the caller's
 * array.  Then what the caller names once a kernel reads them: the column table [ncols], the rows with their stride in elements, the
 * state [nenv][delay_max + 3][ncols], the counts [nenv], the policy's actions (null: none bound) with their row stride and type, the
 * caller's input array (null: none bound) with its row length, row stride and type, and the per-env delays (null: 0) */
struct ActCfg {
    int ncols, delay_max, dtype, nslots, ndst, input_need;
    unsigned long long seed; unsigned env_base;
    int slot_field[ACT_MAXSLOTS], slot_dim[ACT_MAXSLOTS];
    int dst_field[ACT_MAXDST], dst_dim[ACT_MAXDST];
    const ActCol *cols; void *rows; long long srow; double *state; unsigned *counts;
    const void *actions; long long act_stride; int act_dtype;
    const void *input; int input_dim, input_stride, input_dtype;
    const int *delay;
};

/* the task rows (phys_batch_task_configure; ncols 0: not configured): the columns, the rows' type (OBS_F32 / OBS_F64), the seed of the draws
 * and the offset of their env counter; the destinations of a call as the action's -- slot s is the command field dst_field[s], whose row
 * held dst_dim[s] -- and the columns of the table the TABLE columns reach (0: none).  Then what the caller names once a kernel reads them:
 * the column table [ncols], the rows with their stride in elements, the state [nenv][ncols], the words [nenv][TASK_WORDS][ncols], the
 * counts [nenv], and the reference table [nframes][tcols] (null: none set) */
struct TaskCfg {
    int ncols, dtype, ndst, tcol_need;
    unsigned long long seed; unsigned env_base;
    int dst_field[ACT_MAXDST], dst_dim[ACT_MAXDST];
    const TaskCol *cols; void *rows; long long srow; double *state; unsigned *words; unsigned *counts;
    const double *table; int nframes, tcols;
};

/* the event rows (phys_batch_events_configure; ncols 0: not configured): the columns, the rows' type (OBS_F32 / OBS_F64), the done mask;
 * the sources of a call as the observation's -- slot s is field slot_field[s] (or EV_INPUT), whose row held slot_dim[s] elements when the
 * columns were checked against it -- and the elements the columns need of the caller's input array.  Then what the caller names once a
 * kernel reads them: the column table [ncols] with the fields as slots, the rows with their stride in elements, the done words [nenv],
 * the state [2][ncols][nenv], the words [ncols][nenv], the counts [nenv], and the caller's input array (null: none bound) with its row
 * length, row stride and type */
struct EventCfg {
    int ncols, dtype, nslots, input_need;
    unsigned long long done_mask;
    int slot_field[EVENT_MAXSLOTS], slot_dim[EVENT_MAXSLOTS];
    const EventCol *cols; void *rows; long long srow; int *flags; double *state; unsigned *words; unsigned *counts;
    const void *input; int input_dim, input_stride, input_dtype;
};

/* ---- the row of a full state ---- */

/* The groups of a row (PHYS_STATE_* of include/cassie_phys.h) and its sections, in the order they lie in a row.  CORE is every word one
 * stepping launch writes and a later launch reads, or that a reader uses as stored: the state proper, what the drive-level pass of the next
 * substep reads of the last one (sensordata, actuator_velocity, ctrl), qacc, the measurement block, the drive-level state with its message
 * word, the stored body poses (the depth image, the range sensors and the derived read-out take them as stored) and the sticky warning word.
 * Per launch only, or cost only, and therefore in no row: PhysIO::progress, the chunk words (tagged with the launch's own number), the
 * hand-over lists and their counts (zero between launches), the launch order and the per-env cost (they move an env's wave in the grid,
 * never its result), info, ext, derived, body_cfrc, the step sums (outputs).
 * A change of the list or of the order of the sections is a new STATE_LAYOUT_VERSION: the signature of rows kept elsewhere then differs. */
constexpr int STATE_LAYOUT_VERSION = 1;
enum { STATE_CORE = 1, STATE_COMMANDS = 2, STATE_EPISODE = 4, STATE_PARAMS = 8, STATE_ALL_GROUPS = 15 };
enum { SS_TIME, SS_QPOS, SS_QVEL, SS_WARM, SS_CTRL, SS_QACC, SS_SENS, SS_ACTVEL, SS_MEAS, SS_DRIVE, SS_XPOS, SS_XQUAT, SS_WARN,
       SS_PD_PTARGET, SS_PD_KP, SS_PD_KD, SS_PD_DTARGET, SS_PD_TORQUE, SS_DRIVE_CMD, SS_QFRC_APPLIED, SS_XFRC_APPLIED,
       SS_EP_STEPS, SS_EP_COUNT, SS_TERRAIN, SS_PARAMS, SS_COUNT };
static_assert(SS_COUNT <= STATE_MAXSECT, "StateIO holds every section");
static_assert(sizeof(cm_drive_state_t) % 8 == 0 && sizeof(cm_envparams_t) % 8 == 0, "sections are whole 8-byte words");
/* offsets and counts in 8-byte words (off -1: the section's group is not in the row); every section starts on an even word, the row
 * dim is the sum of the padded counts */
struct StateLayout { int version, groups, row_dim, nsect; int off[SS_COUNT], count[SS_COUNT]; };
inline int state_section_group(int s) { return s <= SS_WARN ? STATE_CORE : s <= SS_XFRC_APPLIED ? STATE_COMMANDS : s <= SS_TERRAIN ? STATE_EPISODE : STATE_PARAMS; }
inline StateLayout state_layout(int nq, int nv, int nu, int nsd, int nbody, int groups) {
    const int words[SS_COUNT] = {1, nq, nv, nv, nu, nv, nsd, nu, CM_MEAS_DIM, (int)(sizeof(cm_drive_state_t) / 8), 3 * nbody, 4 * nbody, 1,
                                 nu, nu, nu, nu, nu, nu + 1, nv, 6 * nbody, 1, 1, 1, (int)(sizeof(cm_envparams_t) / 8)};
    StateLayout L;
    L.version = STATE_LAYOUT_VERSION; L.groups = (groups & STATE_ALL_GROUPS) | STATE_CORE; L.row_dim = 0; L.nsect = 0;
    for (int s = 0; s < SS_COUNT; ++s) {
        L.off[s] = -1; L.count[s] = 0;
        if (!(L.groups & state_section_group(s))) continue;
        L.off[s] = L.row_dim; L.count[s] = words[s]; L.row_dim += (words[s] + 1) & ~1; ++L.nsect;
    }
    return L;
}
inline StateLayout state_layout(const BatchView &v, int groups) { return state_layout(v.nq, v.nv, v.nu, v.nsd, v.nbody, groups); }
/* what keeps rows saved from one model (or with other groups) out of another: the layout's version, groups and row dim and the compiled
 * model's sizes, options, tree, reference pose, masses and geoms, hashed (FNV-1a over the words) */
inline unsigned long long state_signature(const cm_model_t &m, const StateLayout &L) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&h](const void *p, size_t bytes) { for (size_t i = 0; i < bytes; ++i) { h ^= ((const unsigned char *)p)[i]; h *= 1099511628211ull; } };
    const int head[] = {L.version, L.groups, L.row_dim, m.nq, m.nv, m.nu, m.nbody, m.njnt, m.ngeom, m.npair, m.neq, m.nsensordata, (int)m.flags,
                        m.hfield_geom, m.hfield_nrow, m.hfield_ncol, m.iterations};
    mix(head, sizeof head);
    mix(&m.timestep, sizeof m.timestep); mix(m.gravity, sizeof m.gravity); mix(m.hfield_size, sizeof m.hfield_size);
    mix(m.body_parentid, sizeof(int) * (size_t)m.nbody); mix(m.body_pos, sizeof(double) * 3 * (size_t)m.nbody);
    mix(m.body_mass, sizeof(double) * (size_t)m.nbody); mix(m.jnt_type, sizeof(int) * (size_t)m.njnt);
    mix(m.qpos0, sizeof(double) * (size_t)m.nq); mix(m.geom_type, sizeof(int) * (size_t)m.ngeom);
    return h;
}

/* ---- the checks ---- */

/* the body a scan pattern or a camera hangs on: a child of the world whose pose follows from qpos alone (static_body_pose) */
inline const char *check_body_pose_from_qpos(const cm_model_t &m, int model_stride, int body) {
    const int rt = body > 0 && body < m.nbody ? m.body_kin[body].rot_type : 0;
    const bool ok = body > 0 && body < m.nbody && m.kin_simple && m.body_parentid[body] == 0 && model_stride == 0 && (rt == CM_JNT_BALL || rt == CM_JNT_FREE || rt == -1);
    return ok ? nullptr : "the body must be a child of the world whose joints are slides and at most a ball or free joint (a shared kin_simple model)";
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *SCAN_SIZE_REFUSAL = "1 .. 1024 points and a positive range", *DEPTH_SIZE_REFUSAL = "an image of 1 .. 16384 pixels and a camera pose";
/* the height scan's configuration; fills c but for where the pattern lies once a kernel reads it, which the caller names */
inline const char *scan_configure(const cm_model_t &m, int model_stride, const double *offsets_xy, int npoints, int body, double range, ScanCfg &c) {
    if (!offsets_xy || npoints <= 0 || npoints > SCAN_MAXPOINTS || !(range > 0)) return SCAN_SIZE_REFUSAL;
    if (const char *why = check_body_pose_from_qpos(m, model_stride, body)) return why;
    c = {npoints, body, range, nullptr};
    return nullptr;
}
/* the geoms a depth image may render (every compiled geom) and those it renders by default (the static planes, boxes and height field:
 * what the static kernel sees); a mask must name none at or above ngeom */
inline unsigned depth_all_geoms(const cm_model_t &m) { return m.ngeom >= 32 ? 0xffffffffu : (1u << m.ngeom) - 1u; }
inline unsigned depth_default_geoms(const cm_model_t &m) {
    unsigned mask = 0;
    for (int g = 0; g < m.ngeom; ++g) {
        const int gt = m.geom_type[g];
        if (m.body_weldid[m.geom_bodyid[g]] == 0 && (gt == CM_GEOM_PLANE || gt == CM_GEOM_BOX || gt == CM_GEOM_HFIELD)) mask |= 1u << g;
    }
    return mask;
}
inline const char *check_depth_geoms(const cm_model_t &m, unsigned mask) { return mask & ~depth_all_geoms(m) ? "the mask names a geom at or above ngeom" : nullptr; }
/* the depth image's configuration (fovy in radians); fills c: the default geoms, no per-env pose, no ids */
inline const char *depth_configure(const cm_model_t &m, int model_stride, int body, const double *cam_pos, const double *cam_quat, int width, int height,
                                   double fovy, double znear, double zfar, DepthCfg &c) {
    if (!cam_pos || !cam_quat || width < 1 || height < 1 || (long long)width * height > DEPTH_MAXPIXELS) return DEPTH_SIZE_REFUSAL;
    if (!(fovy > 0 && fovy < 3.14159265358979323846) || !(znear > 0 && znear < zfar)) return "0 < fovy < pi (radians) and 0 < near < far";
    const double qn = cam_quat[0] * cam_quat[0] + cam_quat[1] * cam_quat[1] + cam_quat[2] * cam_quat[2] + cam_quat[3] * cam_quat[3];
    if (!(qn > 0)) return "the camera's quaternion is zero";
    if (const char *why = check_body_pose_from_qpos(m, model_stride, body)) return why;
    c = {width, height, body, tan(0.5 * fovy), znear, zfar, {cam_pos[0], cam_pos[1], cam_pos[2]}, {cam_quat[0], cam_quat[1], cam_quat[2], cam_quat[3]},
         nullptr, depth_default_geoms(m), nullptr};
    return nullptr;
}
/* the geoms a ray may see: the depth image's rule */
inline const char *check_ray_geoms(const cm_model_t &m, unsigned mask) { return check_depth_geoms(m, mask); }
/* (what the launcher also answers a call without a batch) */
constexpr const char *RAYS_SIZE_REFUSAL = "1 .. 1024 rays and 0 <= rmin < rmax";
/* the range sensors' configuration: checks the caller's rays [nrays] and writes them, the directions normalised, to table [nrays]
 * (which the caller then hands to the kernel: c.rays stays null); fills c: the default geoms, no ids, no normals */
inline const char *rays_configure(const cm_model_t &m, const RayDef *rays, int nrays, double rmin, double rmax, RayDef *table, RayCfg &c) {
    if (!rays || !table || nrays < 1 || nrays > RAYS_MAX || !(rmin >= 0 && rmin < rmax && rmax < INFINITY)) return RAYS_SIZE_REFUSAL;
    for (int j = 0; j < nrays; ++j) {
        const RayDef &r = rays[j];
        if (r.body < 0 || r.body >= m.nbody) return "a ray's body must lie in [0, nbody)";
        if (r.frame != RAY_BODY && r.frame != RAY_WORLD_DIR && r.frame != RAY_HEADING) return "a ray's frame is PHYS_RAY_BODY, PHYS_RAY_WORLD_DIR or PHYS_RAY_HEADING";
        const double len = sqrt(r.dir[0] * r.dir[0] + r.dir[1] * r.dir[1] + r.dir[2] * r.dir[2]);
        const bool finite = std::isfinite(r.origin[0]) && std::isfinite(r.origin[1]) && std::isfinite(r.origin[2]);
        if (!(len > 0 && len < INFINITY) || !finite) return "a ray needs a finite origin and a finite direction that is not zero";
        table[j] = r;
        for (int k = 0; k < 3; ++k) table[j].dir[k] = r.dir[k] / len;
    }
    c = {nrays, rmin, rmax, nullptr, depth_default_geoms(m), nullptr, nullptr};
    return nullptr;
}
/* a placement's configuration; fills the table (place_classify, episode_kernels.h) */
inline const char *place_configure(const cm_model_t &m, int model_stride, int anchor, const double *offsets_xy, int npoints, double ground_ref, PlaceTable &tab) {
    if (npoints < 0 || npoints > PLACE_MAXPOINTS || (npoints > 0 && !offsets_xy) || !(ground_ref == ground_ref)) return "a footprint of 0 .. 1024 points and a ground height";
    if (model_stride != 0) return "not with per-env models (phys_batch_set_model with env >= 0)";
    memset(&tab, 0, sizeof tab);
    return place_classify(m, anchor, tab);
}
/* the probes' row: quantity-major, for every quantity of the mask in bit order a block [nprobes][dim] with nothing between the blocks;
 * offsets[q] = where quantity q's block starts (-1: not in the mask), dims[q] = its doubles per probe (either may be null) -> the row's length */
constexpr unsigned PROBE_ALL_QUANTITIES = (1u << (PQ_COUNT + 1)) - 1u;
inline int probe_layout(int nprobes, unsigned quantities, int nv, int *offsets, int *dims) {
    const int dim[PQ_COUNT] = {3, 4, 6, 6, 6, 3 * nv, 3 * nv, 3};
    int row = 0;
    for (int q = 0; q < PQ_COUNT; ++q) {
        const bool has = (quantities >> q & 1u) != 0;
        if (offsets) offsets[q] = has ? row : -1;
        if (dims) dims[q] = dim[q];
        if (has) row += nprobes * dim[q];
    }
    return row;
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *PROBES_SIZE_REFUSAL = "0 .. 32 probes (0 releases them)";
/* the probes' configuration: checks the caller's probes [nprobes] and fills c (the table and the quantities; everything the caller
 * names later stays null).  nprobes 0 is accepted and leaves c empty: the launcher releases what it holds */
inline const char *probes_configure(const cm_model_t &m, const ProbeDef *probes, int nprobes, unsigned quantities, ProbeCfg &c) {
    if (nprobes < 0 || nprobes > PROBES_MAX || (nprobes > 0 && !probes)) return PROBES_SIZE_REFUSAL;
    c = {};
    if (nprobes == 0) return nullptr;
    const int nsite = m.nsite < CM_MAXSITE ? m.nsite : CM_MAXSITE;
    for (int j = 0; j < nprobes; ++j) {
        const ProbeDef &d = probes[j];
        if (d.kind != PROBE_BODY && d.kind != PROBE_SITE) return "a probe's kind is PHYS_PROBE_BODY or PHYS_PROBE_SITE";
        if (d.kind == PROBE_BODY && (d.id < 0 || d.id >= m.nbody)) return "a body probe's id must lie in [0, nbody)";
        if (d.kind == PROBE_SITE && (d.id < 0 || d.id >= nsite)) return "a site probe's id must lie in [0, nsite) and below CM_MAXSITE, the sites of the read-out";
        if (!(std::isfinite(d.offset[0]) && std::isfinite(d.offset[1]) && std::isfinite(d.offset[2]))) return "a probe needs a finite offset";
    }
    if (quantities == 0 || (quantities & ~PROBE_ALL_QUANTITIES)) return "quantities is a non-empty OR of PHYS_PQ_*";
    c.nprobes = nprobes; c.quantities = quantities; c.probes = probes;
    return nullptr;
}
/* the classes of the geoms of the host model's FULL list, as the contact word's rules read them (csrc/cassiemujoco.c: the three collision
 * checks): geom_user[0] == 1 an obstacle, == 2 a geom of the robot (geom_user null or nuser_geom < 1: no classes, as there); geom_group as it is */
inline void probe_classify_geoms(const double *geom_user, int nuser_geom, const int *geom_group, int ngeom, int *table) {
    for (int g = 0; g < ngeom; ++g) {
        const double u = geom_user && nuser_geom >= 1 ? geom_user[(size_t)nuser_geom * g] : 0.0;
        const int grp = geom_group ? geom_group[g] : PROBE_NO_GROUP;
        table[g] = (u == 1 ? 1 : u == 2 ? 2 : 0) | ((grp >= 0 && grp < PROBE_NO_GROUP ? grp : PROBE_NO_GROUP) << PROBE_GROUP_SHIFT);
    }
}
/* what a probe call refuses */
inline const char *check_probe_call(const ProbeCfg &c, int nenv, int env0, int n) {
    if (c.nprobes < 1 || !c.probes || !c.ext) return "not configured (phys_batch_probes_configure first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    return nullptr;
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *OBS_SIZE_REFUSAL = "0 .. 2048 terms (0 releases them), a history of 1 .. 64 frames, rows of PHYS_OBS_F32 or PHYS_OBS_F64";
/* the observation's configuration: checks the caller's terms [nterms] against the row lengths the batch holds now (field_dim [nfields],
 * 0: a field it does not hold yet; depth_field: the one field that is never a source), expands them into the column table
 * (table [OBS_MAXCOLS]) and the first column of every term (term_col [nterms], may be null) and fills c but for what the caller names
 * later.  nterms 0 is accepted and leaves c empty: the launcher releases what it holds.  The emulator goes through the same expansion */
inline const char *obs_configure(const int *field_dim, int nfields, int depth_field, const ObsTerm *terms, int nterms, int history, int dtype,
                                 unsigned long long seed, unsigned env_base, ObsCol *table, int *term_col, ObsCfg &c) {
    if (nterms < 0 || nterms > OBS_MAXCOLS || (nterms > 0 && (!terms || !table))) return OBS_SIZE_REFUSAL;
    c = {};
    if (nterms == 0) return nullptr;
    if (history < 1 || history > OBS_MAXHISTORY) return "a history of 1 .. 64 frames";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the rows' dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    int ncols = 0;
    /* the slot of a source among the call's (-1: a seventeenth) */
    auto slot_of = [&c](int field, int dim) {
        for (int s = 0; s < c.nslots; ++s) if (c.slot_field[s] == field) return s;
        if (c.nslots == OBS_MAXSLOTS) return -1;
        c.slot_field[c.nslots] = field; c.slot_dim[c.nslots] = dim;
        return c.nslots++;
    };
    /* the row length of a source as a term may index it (-1: no such source; 0: not held yet; the input's is checked at the call) */
    auto dim_of = [&](int field) { return field == OBS_INPUT ? 0x7fffffff : field >= 0 && field < nfields && field != depth_field ? field_dim[field] : -1; };
    for (int t = 0; t < nterms; ++t) {
        const ObsTerm &d = terms[t];
        if (d.kind != OBS_COPY && d.kind != OBS_ROT_INV) return "a term's kind is PHYS_OBS_COPY or PHYS_OBS_ROT_INV";
        const bool rot = d.kind == OBS_ROT_INV, constant = d.field == OBS_CONST;
        if (constant && !rot) return "PHYS_OBS_CONST is the field of a PHYS_OBS_ROT_INV term only (never a COPY's, never a qfield)";
        if (rot && d.qfield == OBS_CONST) return "PHYS_OBS_CONST is the field of a PHYS_OBS_ROT_INV term only (never a COPY's, never a qfield)";
        if (d.field == depth_field || (rot && d.qfield == depth_field)) return "PHYS_F_DEPTH is no source of an observation (images are not columns)";
        const int dim = constant ? 0 : dim_of(d.field), qdim = rot ? dim_of(d.qfield) : 0;
        if (dim < 0 || qdim < 0) return "a term's field is a PHYS_F_* field of the batch or PHYS_OBS_INPUT (PHYS_OBS_CONST in a ROT_INV's field)";
        if ((!constant && dim == 0) || (rot && qdim == 0))
            return "a term reads a field the batch does not hold yet (the scan, the rays, the probes, the step sums, the derived block: configure or enable them first)";
        const int count = rot ? 3 : d.count;
        if (!rot && count < 1) return "a COPY term makes at least one column";
        if (!constant && (d.index < 0 || (long long)d.index + count > dim)) return rot ? "index + 3 lies beyond the field's row" : "index + count lies beyond the field's row";
        if (rot && (d.qindex < 0 || (long long)d.qindex + 4 > qdim)) return "qindex + 4 lies beyond the field's row";
        if (!(std::isfinite(d.offset) && std::isfinite(d.scale) && std::isfinite(d.noise))) return "a term needs a finite offset, scale and noise";
        if (constant && !(std::isfinite(d.vec[0]) && std::isfinite(d.vec[1]) && std::isfinite(d.vec[2]))) return "a constant vector must be finite";
        if (d.noise < 0) return "noise is an amplitude: >= 0";
        if (!(d.lo <= d.hi)) return "lo <= hi (either may be infinite, neither NaN)";
        if ((long long)ncols + count > OBS_MAXCOLS) return "more than PHYS_OBS_MAXCOLS (2048) columns in a frame";
        const int slot = constant ? -1 : slot_of(d.field, dim == 0x7fffffff ? 0 : dim), qslot = rot ? slot_of(d.qfield, qdim == 0x7fffffff ? 0 : qdim) : -1;
        if ((!constant && slot < 0) || (rot && qslot < 0)) return "more than 16 distinct source fields";
        if (d.field == OBS_INPUT && d.index + count > c.input_need) c.input_need = d.index + count;
        if (rot && d.qfield == OBS_INPUT && d.qindex + 4 > c.input_need) c.input_need = d.qindex + 4;
        if (term_col) term_col[t] = ncols;
        for (int j = 0; j < count; ++j) {
            ObsCol &o = table[ncols++];
            o.slot = slot; o.elem = rot ? d.index : d.index + j; o.comp = rot ? j : -1; o.qslot = qslot; o.qelem = rot ? d.qindex : 0; o.pad = 0;
            for (int k = 0; k < 3; ++k) o.vec[k] = constant ? d.vec[k] : 0.0;
            o.offset = d.offset; o.scale = d.scale; o.noise = d.noise; o.lo = d.lo; o.hi = d.hi;
        }
    }
    if ((long long)ncols * history > OBS_MAXROW) return "a row of more than 65536 elements (history x columns)";
    c.nterms = nterms; c.ncols = ncols; c.history = history; c.dtype = dtype; c.seed = seed; c.env_base = env_base;
    return nullptr;
}
/* what phys_batch_obs_bind / _bind_input refuse */
inline const char *check_obs_bind(const ObsCfg &c, long long row_stride) {
    if (c.nterms < 1) return "not configured (phys_batch_obs_configure first)";
    if (row_stride < (long long)c.ncols * c.history) return "a row stride of at least the row's elements (history x columns)";
    return nullptr;
}
inline const char *check_obs_input(const ObsCfg &c, int dim, long long row_stride, int dtype) {
    if (c.nterms < 1) return "not configured (phys_batch_obs_configure first)";
    if (dim < 1 || row_stride < dim || row_stride > 0x7fffffff) return "an input of at least one element a row and a row stride of at least that";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the input's dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    return nullptr;
}
/* what an observation call refuses; fields [nfields]: what the batch holds NOW */
inline const char *check_obs_call(const ObsCfg &c, const ObsField *fields, int nfields, int nenv, int env0, int n) {
    if (c.nterms < 1 || !c.cols || !c.rows || !c.frames) return "not configured (phys_batch_obs_configure first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == OBS_INPUT) {
            if (!c.input) return "a PHYS_OBS_INPUT term and no input bound (phys_batch_obs_bind_input first)";
            if (c.input_dim < c.input_need) return "the bound input's rows are shorter than the PHYS_OBS_INPUT terms reach";
        } else if (f < 0 || f >= nfields || !fields[f].base || fields[f].dim != c.slot_dim[s])
            return "the row length of a source field has changed since phys_batch_obs_configure (configure again)";
    }
    return nullptr;
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *REWARD_SIZE_REFUSAL = "0 .. 64 terms (0 releases them), rewards of PHYS_OBS_F32 or PHYS_OBS_F64";
/* the reward's configuration: checks the caller's terms [nterms] against the row lengths the batch holds now (as obs_configure: field_dim
 * [nfields], 0: a field it does not hold yet; depth_field: the one field that is never a source), writes the table a launch reads (table
 * [REWARD_MAXTERMS]: the terms with their fields replaced by slots) and fills c but for what the caller names later.  nterms 0 is
 * accepted and leaves c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *reward_configure(const int *field_dim, int nfields, int depth_field, const RewardTerm *terms, int nterms, int dtype, double lo, double hi,
                                    RewardTerm *table, RewardCfg &c) {
    if (nterms < 0 || nterms > REWARD_MAXTERMS || (nterms > 0 && (!terms || !table))) return REWARD_SIZE_REFUSAL;
    c = {};
    if (nterms == 0) return nullptr;
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the rewards' dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    if (!(lo <= hi)) return "lo <= hi (either may be infinite, neither NaN)";
    auto slot_of = [&c](int field, int dim) {
        for (int s = 0; s < c.nslots; ++s) if (c.slot_field[s] == field) return s;
        if (c.nslots == REWARD_MAXSLOTS) return -1;
        c.slot_field[c.nslots] = field; c.slot_dim[c.nslots] = dim;
        return c.nslots++;
    };
    /* the row length of a source as a term may index it (-1: no such source; 0: not held yet; the input's is checked at the call) */
    auto dim_of = [&](int field) { return field == REW_INPUT ? 0x7fffffff : field >= 0 && field < nfields && field != depth_field ? field_dim[field] : -1; };
    const char *why = nullptr;
    /* a slice [index, index + len) of a source -> its slot (-1 with why set: refused) */
    auto slice = [&](int field, int index, int len, const char *beyond) {
        if (field == depth_field) { why = "PHYS_F_DEPTH is no source of a reward (images are not terms)"; return -1; }
        const int dim = dim_of(field);
        if (dim < 0) { why = "a term's field, qfield, tfield and gfield are PHYS_F_* fields of the batch or PHYS_REW_INPUT (PHYS_REW_CONST and PHYS_REW_NONE where the definition allows them)"; return -1; }
        if (dim == 0) { why = "a term reads a field the batch does not hold yet (the scan, the rays, the probes, the step sums, the derived block: configure or enable them first)"; return -1; }
        if (index < 0 || (long long)index + len > dim) { why = beyond; return -1; }
        const int s = slot_of(field, dim == 0x7fffffff ? 0 : dim);
        if (s < 0) { why = "more than 16 distinct source fields"; return -1; }
        if (field == REW_INPUT && index + len > c.input_need) c.input_need = index + len;
        return s;
    };
    for (int t = 0; t < nterms; ++t) {
        const RewardTerm &d = terms[t];
        RewardTerm &o = table[t];
        o = d;
        if (d.kind != REW_VEC && d.kind != REW_ROT_INV && d.kind != REW_QUAT) return "a term's kind is PHYS_REW_VEC, PHYS_REW_ROT_INV or PHYS_REW_QUAT";
        if (d.shape != REW_LINEAR && d.shape != REW_EXP && d.shape != REW_RATIONAL) return "a term's shape is PHYS_REW_LINEAR, PHYS_REW_EXP or PHYS_REW_RATIONAL";
        const bool rot = d.kind == REW_ROT_INV, quat = d.kind == REW_QUAT;
        if (!quat && d.norm != REW_SUMSQ && d.norm != REW_SUMABS && d.norm != REW_MAXABS) return "a term's norm is PHYS_REW_SUMSQ, PHYS_REW_SUMABS or PHYS_REW_MAXABS";
        if ((d.field == REW_CONST && !rot) || (rot && d.qfield == REW_CONST) || d.gfield == REW_CONST)
            return "PHYS_REW_CONST is a tfield, or the field of a PHYS_REW_ROT_INV term (never a VEC's or a QUAT's field, never a qfield or a gfield)";
        if (d.field == REW_NONE || (rot && d.qfield == REW_NONE) || d.tfield == REW_NONE) return "PHYS_REW_NONE is a gfield only (no gate)";
        if (d.kind == REW_VEC && (d.count < 1 || d.count > REWARD_MAXCOUNT)) return "a VEC term takes 1 .. 64 elements";
        const int count = rot ? 3 : quat ? 4 : d.count;
        if (!(std::isfinite(d.dead) && std::isfinite(d.k) && std::isfinite(d.weight))) return "a term needs a finite dead, k and weight";
        if (!quat && d.tfield == REW_CONST && !std::isfinite(d.target)) return "a constant target must be finite";
        const int nvec = rot && d.field == REW_CONST ? 3 : quat && d.tfield == REW_CONST ? 4 : 0;
        for (int k = 0; k < nvec; ++k) if (!std::isfinite(d.vec[k])) return "a constant vector must be finite";
        if (d.dead < 0) return "dead is a half width: >= 0";
        if (d.k < 0) return "k >= 0 (the shapes fall with the error)";
        if (d.field != REW_CONST) {
            o.field = slice(d.field, d.index, count, rot ? "index + 3 lies beyond the field's row" : quat ? "index + 4 lies beyond the field's row" : "index + count lies beyond the field's row");
            if (o.field < 0) return why;
        }
        if (rot) { o.qfield = slice(d.qfield, d.qindex, 4, "qindex + 4 lies beyond the field's row"); if (o.qfield < 0) return why; }
        else { o.qfield = 0; o.qindex = 0; }
        if (d.tfield != REW_CONST) { o.tfield = slice(d.tfield, d.tindex, count, "tindex + the term's elements lies beyond the target's row"); if (o.tfield < 0) return why; }
        if (d.gfield != REW_NONE) { o.gfield = slice(d.gfield, d.gindex, 1, "gindex lies beyond the gate's row"); if (o.gfield < 0) return why; }
        o.count = count;
    }
    c.nterms = nterms; c.dtype = dtype; c.lo = lo; c.hi = hi;
    return nullptr;
}
/* what phys_batch_reward_bind / _bind_terms / _bind_input refuse.  min_stride: 1 for the rewards, nterms for the term rows */
inline const char *check_reward_bind(const RewardCfg &c, long long stride, long long min_stride) {
    if (c.nterms < 1) return "not configured (phys_batch_reward_configure first)";
    if (stride < min_stride) return min_stride > 1 ? "a row stride of at least the terms" : "an element stride of at least 1";
    return nullptr;
}
inline const char *check_reward_input(const RewardCfg &c, int dim, long long row_stride, int dtype) {
    if (c.nterms < 1) return "not configured (phys_batch_reward_configure first)";
    if (dim < 1 || row_stride < dim || row_stride > 0x7fffffff) return "an input of at least one element a row and a row stride of at least that";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the input's dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    return nullptr;
}
/* what a reward call refuses; fields [nfields]: what the batch holds NOW */
inline const char *check_reward_call(const RewardCfg &c, const ObsField *fields, int nfields, int nenv, int env0, int n) {
    if (c.nterms < 1 || !c.terms || !c.rew || !c.ret || !c.fin) return "not configured (phys_batch_reward_configure first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == REW_INPUT) {
            if (!c.input) return "a PHYS_REW_INPUT term and no input bound (phys_batch_reward_bind_input first)";
            if (c.input_dim < c.input_need) return "the bound input's rows are shorter than the PHYS_REW_INPUT terms reach";
        } else if (f < 0 || f >= nfields || !fields[f].base || fields[f].dim != c.slot_dim[s])
            return "the row length of a source field has changed since phys_batch_reward_configure (configure again)";
    }
    return nullptr;
}
/* the destination of column k of cols [..] (any column type with a dfield and a dindex; ACT_NONE: none), shared by the stages that write
 * command fields (the action rows, the task rows): one element of a command field (cmd_fields [ncmd]) the batch holds, inside its row,
 * that no earlier column names -> its slot among the call's destinations (ndst, dst_field, dst_dim [ACT_MAXDST]: extended by a new
 * field) and its element; dslot -1 for none */
template <class ColDef>
inline const char *claim_destination(const int *field_dim, int nfields, const int *cmd_fields, int ncmd, const ColDef *cols, int k,
                                     int &ndst, int *dst_field, int *dst_dim, int &dslot, int &delem) {
    const ColDef &d = cols[k];
    dslot = -1; delem = 0;
    if (d.dfield == ACT_NONE) return nullptr;
    bool cmd = false;
    for (int j = 0; j < ncmd; ++j) cmd = cmd || cmd_fields[j] == d.dfield;
    if (!cmd || d.dfield < 0 || d.dfield >= nfields)
        return "a column's dfield is PHYS_ACT_NONE or a command field (PHYS_F_PD_PTARGET, _PD_DTARGET, _PD_KP, _PD_KD, _PD_TORQUE, PHYS_F_DRIVE_CMD, PHYS_F_CTRL, PHYS_F_QFRC_APPLIED, PHYS_F_XFRC_APPLIED)";
    const int dim = field_dim[d.dfield];
    if (dim == 0) return "a column writes a field the batch does not hold";
    if (d.dindex < 0 || d.dindex >= dim) return "dindex lies beyond the field's row";
    for (int j = 0; j < k; ++j)
        if (cols[j].dfield == d.dfield && cols[j].dindex == d.dindex) return "two columns write the same destination element";
    int s = 0;
    while (s < ndst && dst_field[s] != d.dfield) ++s;
    if (s == ndst) {
        if (ndst == ACT_MAXDST) return "more destination fields than there are command fields";
        dst_field[s] = d.dfield; dst_dim[s] = dim; ++ndst;
    }
    dslot = s; delem = d.dindex;
    return nullptr;
}
/* whether every destination field of a call is held NOW with the row length it had at the configure call (fields [nfields]) */
inline bool destinations_unchanged(int ndst, const int *dst_field, const int *dst_dim, const ObsField *fields, int nfields) {
    for (int s = 0; s < ndst; ++s) {
        const int f = dst_field[s];
        if (f < 0 || f >= nfields || !fields[f].base || fields[f].dim != dst_dim[s]) return false;
    }
    return true;
}
/* the destinations of a launch where the batch reads them today */
inline void fill_destinations(ActDst *dst, int ndst, const int *dst_field, const ObsField *fields) {
    for (int s = 0; s < ndst; ++s) dst[s] = {const_cast<double *>(fields[dst_field[s]].base), fields[dst_field[s]].stride};
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *ACT_SIZE_REFUSAL = "0 .. 256 columns (0 releases them), a delay depth of 0 .. 8, rows of PHYS_OBS_F32 or PHYS_OBS_F64";
/* the actions' configuration: checks the caller's columns [ncols] against the row lengths the batch holds now (as obs_configure: field_dim
 * [nfields], 0: a field it does not hold yet; depth_field: the one field that is never a source; cmd_fields [ncmd]: the fields a column
 * may write), writes the table a launch reads (table [ACT_MAXCOLS]: the fields replaced by slots) and fills c but for what the caller
 * names later.  ncols 0 is accepted and leaves c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *act_configure(const int *field_dim, int nfields, int depth_field, const int *cmd_fields, int ncmd, const ActColDef *cols, int ncols,
                                 int delay_max, int dtype, unsigned long long seed, unsigned env_base, ActCol *table, ActCfg &c) {
    if (ncols < 0 || ncols > ACT_MAXCOLS || (ncols > 0 && (!cols || !table))) return ACT_SIZE_REFUSAL;
    c = {};
    if (ncols == 0) return nullptr;
    if (delay_max < 0 || delay_max > ACT_MAXDELAY) return "a delay depth of 0 .. 8 calls";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the rows' dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    for (int k = 0; k < ncols; ++k) {
        const ActColDef &d = cols[k];
        ActCol &o = table[k];
        if (!(d.lo <= d.hi) || !(d.out_lo <= d.out_hi)) return "lo <= hi and out_lo <= out_hi (either may be infinite, neither NaN)";
        if (!(d.noise >= 0) || !std::isfinite(d.noise)) return "noise is an amplitude: finite and >= 0";
        if (!(d.smooth > 0 && d.smooth <= 1)) return "smooth lies in (0, 1] (1: no filter)";
        if (!(std::isfinite(d.offset) && std::isfinite(d.scale))) return "a column needs a finite offset and scale";
        /* the base: the offset alone, or a slice of one element of a source */
        o.slot = -1; o.elem = 0;
        if (d.bfield != ACT_CONST) {
            if (d.bfield == depth_field) return "PHYS_F_DEPTH is no source of an action (images are not columns)";
            const bool input = d.bfield == ACT_INPUT;
            if (!input && (d.bfield < 0 || d.bfield >= nfields)) return "a column's bfield is PHYS_ACT_CONST, PHYS_ACT_INPUT or a PHYS_F_* field of the batch";
            const int dim = input ? 0x7fffffff : field_dim[d.bfield];
            if (dim == 0) return "a column reads a field the batch does not hold yet (the scan, the rays, the probes, the step sums, the derived block: configure or enable them first)";
            if (d.bindex < 0 || d.bindex >= dim) return "bindex lies beyond the field's row";
            int s = 0;
            while (s < c.nslots && c.slot_field[s] != d.bfield) ++s;
            if (s == c.nslots) {
                if (c.nslots == ACT_MAXSLOTS) return "more than 16 distinct source fields";
                c.slot_field[s] = d.bfield; c.slot_dim[s] = input ? 0 : dim; ++c.nslots;
            }
            if (input && d.bindex + 1 > c.input_need) c.input_need = d.bindex + 1;
            o.slot = s; o.elem = d.bindex;
        }
        /* the destination: none, or one element of a command field that no other column writes */
        if (const char *why = claim_destination(field_dim, nfields, cmd_fields, ncmd, cols, k, c.ndst, c.dst_field, c.dst_dim, o.dslot, o.delem)) return why;
        o.lo = d.lo; o.hi = d.hi; o.noise = d.noise; o.smooth = d.smooth; o.offset = d.offset; o.scale = d.scale; o.out_lo = d.out_lo; o.out_hi = d.out_hi;
    }
    c.ncols = ncols; c.delay_max = delay_max; c.dtype = dtype; c.seed = seed; c.env_base = env_base;
    return nullptr;
}
/* the doubles of an env's state: the line's delay_max + 1 slots, the filter state, the previous clipped action */
inline long long act_state_dim(const ActCfg &c) { return (long long)(c.delay_max + 3) * c.ncols; }
/* what phys_batch_act_bind_actions / _bind_rows / _bind_input refuse */
inline const char *check_act_bind_actions(const ActCfg &c, long long row_stride, int dtype) {
    if (c.ncols < 1) return "not configured (phys_batch_act_configure first)";
    if (row_stride < c.ncols) return "a row stride of at least the columns";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the actions' dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    return nullptr;
}
inline const char *check_act_bind_rows(const ActCfg &c, long long row_stride) {
    if (c.ncols < 1) return "not configured (phys_batch_act_configure first)";
    if (row_stride < (long long)ACT_FRAMES * c.ncols) return "a row stride of at least the row's elements (3 x columns)";
    return nullptr;
}
inline const char *check_act_bind_input(const ActCfg &c, int dim, long long row_stride, int dtype) {
    if (c.ncols < 1) return "not configured (phys_batch_act_configure first)";
    if (dim < 1 || row_stride < dim || row_stride > 0x7fffffff) return "an input of at least one element a row and a row stride of at least that";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the input's dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    return nullptr;
}
/* what an action call refuses; fields [nfields]: what the batch holds NOW */
inline const char *check_act_call(const ActCfg &c, const ObsField *fields, int nfields, int nenv, int env0, int n) {
    if (c.ncols < 1 || !c.cols || !c.rows || !c.state || !c.counts) return "not configured (phys_batch_act_configure first)";
    if (!c.actions) return "no actions bound (phys_batch_act_bind_actions first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == ACT_INPUT) {
            if (!c.input) return "a PHYS_ACT_INPUT column and no input bound (phys_batch_act_bind_input first)";
            if (c.input_dim < c.input_need) return "the bound input's rows are shorter than the PHYS_ACT_INPUT columns reach";
        } else if (f < 0 || f >= nfields || !fields[f].base || fields[f].dim != c.slot_dim[s])
            return "the row length of a source field has changed since phys_batch_act_configure (configure again)";
    }
    if (!destinations_unchanged(c.ndst, c.dst_field, c.dst_dim, fields, nfields))
        return "the row length of a destination field has changed since phys_batch_act_configure (configure again)";
    return nullptr;
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *TASK_SIZE_REFUSAL = "1 .. 64 columns (a lane makes a column), rows of PHYS_OBS_F32 or PHYS_OBS_F64";
constexpr const char *TASK_TABLE_REFUSAL = "a table of 1 .. 4096 frames of 1 .. 64 finite columns";
/* the reference table of the TABLE columns (phys_batch_task_set_table): host [nframes][tcols] */
inline const char *check_task_table(const TaskCfg &c, const double *host, int nframes, int tcols) {
    if (!host || nframes < 1 || nframes > TASK_MAXFRAMES || tcols < 1 || tcols > TASK_MAXTCOLS) return TASK_TABLE_REFUSAL;
    for (long long k = 0; k < (long long)nframes * tcols; ++k) if (!std::isfinite(host[k])) return TASK_TABLE_REFUSAL;
    if (c.ncols > 0 && tcols < c.tcol_need) return "the configured TABLE columns reach beyond the new table's columns (configure again)";
    return nullptr;
}
/* the task rows' configuration: checks the caller's columns [ncols] against the row lengths the batch holds now (field_dim [nfields], 0: a
 * field it does not hold; cmd_fields [ncmd]: the fields a column may write) and against the table that is set (nframes x tcols, 0: none),
 * writes the table a launch reads (table [TASK_MAXCOLS]: the defaults resolved to lanes, the periods as a span, the resting threshold)
 * and fills c but for what the caller names later.  The emulator goes through the same */
inline const char *task_configure(const int *field_dim, int nfields, const int *cmd_fields, int ncmd, const TaskColDef *cols, int ncols, int dtype,
                                  unsigned long long seed, unsigned env_base, int nframes, int tcols, TaskCol *table, TaskCfg &c) {
    if (ncols < 1 || ncols > TASK_MAXCOLS || !cols || !table) return TASK_SIZE_REFUSAL;
    c = {};
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the rows' dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    auto is_kind = [&](int col, int kind) { return col >= 0 && col < ncols && cols[col].kind == kind; };
    for (int k = 0; k < ncols; ++k) {
        const TaskColDef &d = cols[k];
        TaskCol &o = table[k];
        memset(&o, 0, sizeof o);
        o.kind = d.kind; o.group = k; o.rate_col = -1; o.phase_col = -1; o.src = -1;
        if (d.kind == TASK_SAMPLE) {
            if (!(std::isfinite(d.center) && std::isfinite(d.half) && std::isfinite(d.rest) && std::isfinite(d.p_rest))) return "a SAMPLE column needs a finite center, half, rest and p_rest";
            if (d.half < 0) return "half is a half width: >= 0";
            if (!(d.p_rest >= 0 && d.p_rest <= 1)) return "p_rest is a probability: in [0, 1]";
            if (d.period_lo < 1u || d.period_lo > d.period_hi || d.period_hi > TASK_MAXPERIOD) return "1 <= period_lo <= period_hi <= 2^30 calls";
            const int g = d.group < 0 ? k : d.group;
            if (!is_kind(g, TASK_SAMPLE) || (cols[g].group >= 0 && cols[g].group != g)) return "group names a SAMPLE column that is its own group (-1: the column itself)";
            const TaskColDef &l = cols[g];
            if (l.period_lo != d.period_lo || l.period_hi != d.period_hi || l.hold != d.hold || l.p_rest != d.p_rest)
                return "the members of a group share period_lo, period_hi, hold and p_rest with the column the group names";
            o.group = g; o.period_lo = d.period_lo; o.span = d.period_hi - d.period_lo + 1u; o.hold = d.hold;
            o.thr = (unsigned long long)llrint(d.p_rest * 4294967296.0);
            o.center = d.center; o.half = d.half; o.rest = d.rest;
        } else if (d.kind == TASK_PHASE) {
            if (!(std::isfinite(d.rate) && std::isfinite(d.rate_scale) && std::isfinite(d.phase0))) return "a PHASE column needs a finite rate, rate_scale and phase0";
            if (d.rate_col >= 0 && !is_kind(d.rate_col, TASK_SAMPLE)) return "rate_col is -1 or a SAMPLE column";
            if (d.phase_col >= 0 && !is_kind(d.phase_col, TASK_SAMPLE)) return "phase_col is -1 or a SAMPLE column";
            o.rate_col = d.rate_col < 0 ? -1 : d.rate_col; o.phase_col = d.phase_col < 0 ? -1 : d.phase_col;
            o.rate = d.rate; o.rate_scale = d.rate_scale; o.phase0 = d.phase0;
        } else if (d.kind == TASK_WAVE || d.kind == TASK_TABLE) {
            if (!is_kind(d.src, TASK_PHASE)) return "src is a PHASE column";
            if (!(std::isfinite(d.shift) && std::isfinite(d.offset) && std::isfinite(d.scale))) return "a WAVE or TABLE column needs a finite shift, offset and scale";
            if (d.kind == TASK_WAVE) {
                if (d.form != TASK_SAW && d.form != TASK_SIN && d.form != TASK_COS && d.form != TASK_TRAPEZOID) return "a WAVE's form is PHYS_TASK_SAW, _SIN, _COS or _TRAPEZOID";
                if (d.form == TASK_TRAPEZOID) {
                    if (!(std::isfinite(d.duty) && std::isfinite(d.ramp)) || !(d.ramp > 0) || d.duty < 0 || d.duty + d.ramp > 1) return "a TRAPEZOID needs ramp > 0, duty >= 0 and duty + ramp <= 1";
                    o.duty = d.duty; o.ramp = d.ramp;
                }
                o.form = d.form;
            } else {
                if (nframes < 1 || tcols < 1) return "a TABLE column and no table (phys_batch_task_set_table first)";
                if (d.tcol < 0 || d.tcol >= tcols) return "tcol lies beyond the table's columns";
                o.tcol = d.tcol;
                if (d.tcol + 1 > c.tcol_need) c.tcol_need = d.tcol + 1;
            }
            o.src = d.src; o.shift = d.shift; o.offset = d.offset; o.scale = d.scale;
        } else return "a column's kind is PHYS_TASK_SAMPLE, _PHASE, _WAVE or _TABLE";
        if (const char *why = claim_destination(field_dim, nfields, cmd_fields, ncmd, cols, k, c.ndst, c.dst_field, c.dst_dim, o.dslot, o.delem)) return why;
    }
    c.ncols = ncols; c.dtype = dtype; c.seed = seed; c.env_base = env_base;
    return nullptr;
}
/* what phys_batch_task_bind_rows refuses */
inline const char *check_task_bind_rows(const TaskCfg &c, long long row_stride) {
    if (c.ncols < 1) return "not configured (phys_batch_task_configure first)";
    if (row_stride < c.ncols) return "a row stride of at least the columns";
    return nullptr;
}
/* what a task call refuses; fields [nfields]: what the batch holds NOW */
inline const char *check_task_call(const TaskCfg &c, const ObsField *fields, int nfields, int nenv, int env0, int n) {
    if (c.ncols < 1 || !c.cols || !c.rows || !c.state || !c.words || !c.counts) return "not configured (phys_batch_task_configure first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    if (c.tcol_need > 0 && (!c.table || c.nframes < 1 || c.tcols < c.tcol_need)) return "a TABLE column and no table that holds its column (phys_batch_task_set_table)";
    if (!destinations_unchanged(c.ndst, c.dst_field, c.dst_dim, fields, nfields))
        return "the row length of a destination field has changed since phys_batch_task_configure (configure again)";
    return nullptr;
}
/* (what the launcher also answers a call without a batch) */
constexpr const char *EVENT_SIZE_REFUSAL = "1 .. 64 columns (0 releases them), rows of PHYS_OBS_F32 or PHYS_OBS_F64";
/* the event rows' configuration: checks the caller's columns [ncols] against the row lengths the batch holds now (as reward_configure:
 * field_dim [nfields], 0: a field it does not hold; depth_field: the one field that is never a source), writes the table a launch reads
 * (table [EVENT_MAXCOLS]: the columns with a MEASURE's field replaced by its slot and the fields its kind does not name cleared) and
 * fills c but for what the caller names later.  ncols 0 is accepted and leaves c empty: the launcher releases what it holds.  The
 * emulator goes through the same */
inline const char *events_configure(const int *field_dim, int nfields, int depth_field, const EventCol *cols, int ncols, int dtype,
                                    unsigned long long done_mask, EventCol *table, EventCfg &c) {
    if (ncols < 0 || ncols > EVENT_MAXCOLS || (ncols > 0 && (!cols || !table))) return EVENT_SIZE_REFUSAL;
    c = {};
    if (ncols == 0) return nullptr;
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the rows' dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    if (ncols < 64 && (done_mask >> ncols) != 0ull) return "done_mask has a bit at or above ncols";
    const char *const lower = "a column's src, trig, clear and gate name columns with a lower index (clear and gate may be -1)";
    for (int k = 0; k < ncols; ++k) {
        const EventCol &d = cols[k];
        EventCol &o = table[k];
        o = EventCol();
        o.kind = d.kind; o.src = o.trig = o.clear = o.gate = -1;
        auto is_lower = [k](int j) { return j >= 0 && j < k; };
        if (d.kind == EV_MEASURE) {
            if (d.norm != EV_SIGNED && d.norm != EV_SUMABS && d.norm != EV_SUMSQ && d.norm != EV_MAXABS) return "a MEASURE's norm is PHYS_EV_SIGNED, _SUMABS, _SUMSQ or _MAXABS";
            if (d.count < 1 || d.count > EVENT_MAXCOUNT) return "a MEASURE takes 1 .. 8 elements";
            if (d.norm == EV_SIGNED && d.count != 1) return "a SIGNED MEASURE takes one element";
            if (!std::isfinite(d.target)) return "a column's constants must be finite";
            if (d.field == depth_field) return "PHYS_F_DEPTH is no source of an event (images are not columns)";
            const int dim = d.field == EV_INPUT ? 0x7fffffff : d.field >= 0 && d.field < nfields ? field_dim[d.field] : -1;
            if (dim < 0) return "a MEASURE's field is a PHYS_F_* field of the batch or PHYS_EV_INPUT";
            if (dim == 0) return "a column reads a field the batch does not hold yet (the scan, the rays, the probes, the step sums, the derived block: configure or enable them first)";
            if (d.index < 0 || (long long)d.index + d.count > dim) return "index + count lies beyond the field's row";
            int s = 0;
            while (s < c.nslots && c.slot_field[s] != d.field) ++s;
            if (s == c.nslots) {
                if (c.nslots == EVENT_MAXSLOTS) return "more than 16 distinct source fields";
                c.slot_field[s] = d.field; c.slot_dim[s] = d.field == EV_INPUT ? 0 : dim; ++c.nslots;
            }
            if (d.field == EV_INPUT && d.index + d.count > c.input_need) c.input_need = d.index + d.count;
            o.field = s; o.index = d.index; o.count = d.count; o.norm = d.norm; o.root = d.norm == EV_SUMSQ && d.root != 0; o.target = d.target;
        } else if (d.kind == EV_LEVEL) {
            if (!is_lower(d.src)) return lower;
            if (!(std::isfinite(d.on_thr) && std::isfinite(d.off_thr))) return "a column's constants must be finite";
            if (d.off_thr > d.on_thr) return "off_thr <= on_thr";
            if (d.sense != 1 && d.sense != -1) return "a LEVEL's sense is +1 or -1";
            o.src = d.src; o.on_thr = d.on_thr; o.off_thr = d.off_thr; o.sense = d.sense;
        } else if (d.kind == EV_TIMER) {
            if (!is_lower(d.src)) return lower;
            if (!std::isfinite(d.dt)) return "a column's constants must be finite";
            o.src = d.src; o.dt = d.dt; o.polarity = d.polarity != 0;
        } else if (d.kind == EV_EDGE) {
            if (!is_lower(d.src)) return lower;
            if (d.op != EV_RISING && d.op != EV_FALLING && d.op != EV_EITHER) return "an EDGE's op is PHYS_EV_RISING, _FALLING or _EITHER";
            o.src = d.src; o.op = d.op;
        } else if (d.kind == EV_LATCH) {
            if (!is_lower(d.src) || !is_lower(d.trig)) return lower;
            if (!(std::isfinite(d.offset) && std::isfinite(d.scale))) return "a column's constants must be finite";
            if ((d.lag != 0 && d.lag != 1) || (d.keep != 0 && d.keep != 1)) return "a LATCH's lag and keep are 0 or 1";
            o.src = d.src; o.trig = d.trig; o.lag = d.lag; o.keep = d.keep; o.offset = d.offset; o.scale = d.scale;
        } else if (d.kind == EV_ACCUM) {
            if (!is_lower(d.src) || (d.clear != -1 && !is_lower(d.clear)) || (d.gate != -1 && !is_lower(d.gate))) return lower;
            if (d.op != EV_MAX && d.op != EV_MIN && d.op != EV_SUM) return "an ACCUM's op is PHYS_EV_MAX, _MIN or _SUM";
            if (!std::isfinite(d.init)) return "a column's constants must be finite";
            o.src = d.src; o.clear = d.clear; o.gate = d.gate; o.op = d.op; o.init = d.init;
        } else if (d.kind == EV_LOGIC) {
            if (d.op != EV_ANY && d.op != EV_ALL && d.op != EV_NONE && d.op != EV_COUNT) return "a LOGIC's op is PHYS_EV_ANY, _ALL, _NONE or _COUNT";
            if (d.mask == 0ull) return "a LOGIC's mask names at least one column";
            if (ncols < 64 && (d.mask >> ncols) != 0ull) return "a LOGIC's mask has a bit at or above ncols";
            if ((d.mask >> k) != 0ull) return "a LOGIC's mask names columns with a lower index";
            o.op = d.op; o.mask = d.mask;
        } else return "a column's kind is PHYS_EV_MEASURE, _LEVEL, _TIMER, _EDGE, _LATCH, _ACCUM or _LOGIC";
    }
    c.ncols = ncols; c.dtype = dtype; c.done_mask = done_mask;
    return nullptr;
}
/* what phys_batch_events_bind_rows / _bind_input / _bind_flags refuse */
inline const char *check_events_bind_rows(const EventCfg &c, long long row_stride) {
    if (c.ncols < 1) return "not configured (phys_batch_events_configure first)";
    if (row_stride < c.ncols) return "a row stride of at least the columns";
    return nullptr;
}
inline const char *check_events_input(const EventCfg &c, int dim, long long row_stride, int dtype) {
    if (c.ncols < 1) return "not configured (phys_batch_events_configure first)";
    if (dim < 1 || row_stride < dim || row_stride > 0x7fffffff) return "an input of at least one element a row and a row stride of at least that";
    if (dtype != OBS_F32 && dtype != OBS_F64) return "the input's dtype is PHYS_OBS_F32 or PHYS_OBS_F64";
    return nullptr;
}
inline const char *check_events_bind_flags(const EventCfg &c) {
    if (c.ncols < 1) return "not configured (phys_batch_events_configure first)";
    return nullptr;
}
/* what an events call refuses; fields [nfields]: what the batch holds NOW */
inline const char *check_events_call(const EventCfg &c, const ObsField *fields, int nfields, int nenv, int env0, int n) {
    if (c.ncols < 1 || !c.cols || !c.rows || !c.flags || !c.state || !c.words || !c.counts) return "not configured (phys_batch_events_configure first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == EV_INPUT) {
            if (!c.input) return "a PHYS_EV_INPUT column and no input bound (phys_batch_events_bind_input first)";
            if (c.input_dim < c.input_need) return "the bound input's rows are shorter than the PHYS_EV_INPUT columns reach";
        } else if (f < 0 || f >= nfields || !fields[f].base || fields[f].dim != c.slot_dim[s])
            return "the row length of a source field has changed since phys_batch_events_configure (configure again)";
    }
    return nullptr;
}
/* the bank of full states: what phys_batch_state_configure / _bind refuse (the view tells what the batch has), and what a save or a
 * restore refuses */
inline const char *state_configure(const BatchView &v, int nslots, int groups) {
    if (nslots < 1) return "a bank of at least one slot";
    if (groups & ~STATE_ALL_GROUPS) return "groups is an OR of PHYS_STATE_CORE, PHYS_STATE_COMMANDS, PHYS_STATE_EPISODE and PHYS_STATE_PARAMS";
    if ((groups & STATE_EPISODE) && !(v.ep_steps && v.ep_count)) return "PHYS_STATE_EPISODE needs the episode arrays (phys_batch_episodes_enable first)";
    if ((groups & STATE_PARAMS) && !v.params_w) return "PHYS_STATE_PARAMS needs per-env parameter blocks (phys_batch_randomize first); without the group a restored env keeps its own";
    if ((groups & STATE_COMMANDS) && !(v.qfrc_applied && v.xfrc_applied))
        return "PHYS_STATE_COMMANDS holds qfrc_applied / xfrc_applied, which this batch has never uploaded or bound: they would be restored into nothing (upload or bind both first)";
    return nullptr;
}
inline const char *check_state_call(const StateCfg &c, int nenv, int env0, int n) {
    if (c.nslots < 1 || !c.bank) return "not configured (phys_batch_state_configure or phys_batch_state_bind first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    return nullptr;
}

/* ---- the grids ---- */

/* one workgroup per CU walks the range: an env's scan is a chain of dependent reads */
inline int scan_grid(int n) { return n < SCAN_GRID ? n : SCAN_GRID; }
/* a few workgroups walk the range, with or without placement: the launch runs behind a range's step launch while the other range's step
 * kernel fills the chip, where every workgroup waits for a wave slot to free (cassie_reset_kernel) */
inline int episode_grid(int n) { return n < EPISODE_GRID ? n : EPISODE_GRID; }
/* one wave per env up to STATE_GRID workgroups, which then walk the range (state_kernels.h) */
inline int state_grid(int n) { return n < STATE_GRID ? n : STATE_GRID; }
/* one wave per env up to PROBE_GRID workgroups, which then walk the range: few, as the episode kernel's -- the launch runs behind a range's
 * forward pass while the other range's step kernel fills the chip, where every workgroup waits for a wave slot to free (probe_kernels.h) */
inline int probe_grid(int n) { return n < PROBE_GRID ? n : PROBE_GRID; }
/* one wave per env up to OBS_GRID workgroups, which then walk the range: few, as the probes' (obs_kernels.h) */
inline int obs_grid(int n) { return n < OBS_GRID ? n : OBS_GRID; }
/* one wave per 64 envs (a lane takes an env) up to REWARD_GRID workgroups, which then walk the range (reward_kernels.h) */
inline int reward_grid(int n) { const long long w = ((long long)n + WV_WAVE - 1) / WV_WAVE; return w < REWARD_GRID ? (int)w : REWARD_GRID; }
/* one wave per env up to ACT_GRID workgroups, which then walk the range: few, as the observation's (act_kernels.h) */
inline int act_grid(int n) { return n < ACT_GRID ? n : ACT_GRID; }
/* one wave per env up to TASK_GRID workgroups, which then walk the range: few, as the action's (task_kernels.h) */
inline int task_grid(int n) { return n < TASK_GRID ? n : TASK_GRID; }
/* one wave per 64 envs (a lane takes an env) up to EVENT_GRID workgroups, which then walk the range (event_kernels.h) */
inline int events_grid(int n) { const long long w = ((long long)n + WV_WAVE - 1) / WV_WAVE; return w < EVENT_GRID ? (int)w : EVENT_GRID; }
/* a job is (env, tile of DEPTH_TILE x DEPTH_TILE pixels); a fixed grid walks the job list (a first choice: depth_kernel.h) */
inline int depth_grid(int n, int width, int height) {
    const int T = DEPTH_TILE;
    const long long jobs = (long long)n * (((width + T - 1) / T) * ((height + T - 1) / T));
    return (int)(jobs < DEPTH_GRID ? jobs : DEPTH_GRID);
}
/* a job is (env, block of 64 rays); a fixed grid walks the job list (a first choice: ray_kernel.h) */
inline int rays_grid(int n, int nrays) {
    const long long jobs = (long long)n * ((nrays + WV_WAVE - 1) / WV_WAVE);
    return (int)(jobs < RAYS_GRID ? jobs : RAYS_GRID);
}
/* a few workgroups walk the envs: one workgroup per env made the kernel a 0.5 ms stall of its stream on a saturated GPU (cassie_reset_kernel) */
inline int reset_grid(int count) { return count < 4 ? count : 4; }
/* one wave per env, at most a few thousand workgroups walking the range (58 KB of LDS each: two to a CU) */
inline int setconst_grid(int n) { return n < 2048 ? n : 2048; }
/* a few workgroups walk the rows (cassie_param_scatter_kernel) */
inline int param_scatter_grid(int n) { return n < 1024 ? n : 1024; }

/* ---- the builders ---- */

/* what ScanIO, DepthIO and EpisodeIO share: where the surface comes from (the terrain index counts only while a bank is set) */
template <class IO>
inline void fill_surface(IO &io, const BatchView &v) {
    io.envparams = v.envparams; io.hfield = v.hfield; io.hfield_stride = v.hfield_stride;
    if (v.hfield_nterrain > 0) { io.hfield_index = v.hfield_index; io.hfield_nterrain = v.hfield_nterrain; }
}
/* what ResetIO and EpisodeIO share: sizes, row strides and the state arrays a restart writes */
template <class IO>
inline void fill_state(IO &io, const BatchView &v) {
    io.nq = v.nq; io.nv = v.nv; io.nu = v.nu; io.nsd = v.nsd; io.sq = v.sq; io.sqv = v.sqv; io.ssd = v.ssd;
    io.qpos = v.qpos; io.qvel = v.qvel; io.warm = v.warm; io.ctrl = v.ctrl; io.qacc = v.qacc; io.time = v.time;
    io.sens = v.sens; io.actvel = v.actvel; io.meas = v.meas; io.drive = v.drive;
}
template <class IO>
inline IO zeroed() { IO io; memset(&io, 0, sizeof io); return io; }

inline ScanIO make_scan_io(const BatchView &v, const ScanCfg &c, double *out, int sout, int env0, int n) {
    ScanIO io = zeroed<ScanIO>();
    fill_surface(io, v);
    io.models = v.models; io.model_stride = v.model_stride;
    io.env0 = env0; io.n = n; io.npoints = c.npoints; io.body = c.body; io.range = c.range; io.offsets = c.offsets;
    io.qpos = v.qpos; io.sq = v.sq; io.out = out; io.sout = sout; io.warn = v.warn;
    return io;
}
/* The static kernel unless the caller has chosen other geoms than the default or wants the ids: the default image is the static
 * kernel's, bit for bit and at its cost.  (Any other mask goes to the scene kernel, also one that renders the same geoms.) */
inline bool depth_scene_kernel(const cm_model_t &m, const DepthCfg &c) { return c.geoms != depth_default_geoms(m) || c.ids; }
/* scene: for cassie_depth_scene_kernel; else its fields stay zero (the static kernel reads none of them) */
inline DepthIO make_depth_io(const BatchView &v, const DepthCfg &c, double *out, int sout, int env0, int n, bool scene) {
    DepthIO io = zeroed<DepthIO>();
    fill_surface(io, v);
    io.models = v.models; io.model_stride = v.model_stride;
    io.env0 = env0; io.n = n; io.body = c.body; io.width = c.width; io.height = c.height;
    io.tan_half = c.tan_half; io.znear = c.znear; io.zfar = c.zfar;
    for (int k = 0; k < 3; ++k) io.cam_pos[k] = c.cam_pos[k];
    for (int k = 0; k < 4; ++k) io.cam_quat[k] = c.cam_quat[k];
    io.pose = c.pose;
    io.qpos = v.qpos; io.sq = v.sq; io.out = out; io.sout = sout; io.warn = v.warn;
    if (scene) { io.geoms = c.geoms; io.xpos = v.xpos; io.xquat = v.xquat; io.sxp = 3 * v.nbody; io.sxq = 4 * v.nbody; io.ids = c.ids; }
    return io;
}
inline RayIO make_rays_io(const BatchView &v, const RayCfg &c, double *out, int sout, int env0, int n) {
    RayIO io = zeroed<RayIO>();
    fill_surface(io, v);
    io.models = v.models; io.model_stride = v.model_stride;
    io.env0 = env0; io.n = n; io.nrays = c.nrays; io.rmin = c.rmin; io.rmax = c.rmax; io.rays = c.rays; io.geoms = c.geoms;
    io.xpos = v.xpos; io.xquat = v.xquat; io.sxp = 3 * v.nbody; io.sxq = 4 * v.nbody;
    io.out = out; io.sout = sout; io.ids = c.ids; io.normals = c.normals; io.warn = v.warn;
    return io;
}
/* cassie_probe_kernel's: the state rows of the view, the forward pass's outputs and the tables of the record, the row's layout; the
 * contact word only where it was asked for AND the geoms' classes are there */
inline ProbeIO make_probe_io(const BatchView &v, const ProbeCfg &c, double *out, int sout, int env0, int n) {
    ProbeIO io = zeroed<ProbeIO>();
    io.models = v.models; io.model_stride = v.model_stride;
    io.env0 = env0; io.n = n; io.nprobes = c.nprobes; io.quantities = c.quantities; io.probes = c.probes;
    io.ext = c.ext; io.xpos = c.xpos; io.xquat = c.xquat; io.sxp = 3 * v.nbody; io.sxq = 4 * v.nbody;
    io.qpos = v.qpos; io.sq = v.sq; io.qvel = v.qvel; io.sqv = v.sqv; io.qacc = c.qacc; io.sv = v.nv;
    io.out = out; io.sout = sout;
    if ((c.quantities >> PQ_CONTACTS & 1u) && c.geom_class) { io.geom_class = c.geom_class; io.ngeom = c.ngeom; io.contacts = c.contacts; }
    io.row_dim = probe_layout(c.nprobes, c.quantities, v.nv, io.off, nullptr);
    return io;
}
/* cassie_obs_kernel's: the sources of the record's slots where the batch reads them today (fields [nfields]: its own buffers or the
 * caller's bound tensors, with their row strides; the caller's input array), the column table, the rows, the counts and the key */
inline ObsIO make_obs_io(const ObsCfg &c, const ObsField *fields, int env0, int n, const int *refill) {
    ObsIO io = zeroed<ObsIO>();
    io.env0 = env0; io.n = n; io.ncols = c.ncols; io.history = c.history; io.f32 = c.dtype == OBS_F32;
    io.env_base = c.env_base; io.key0 = (unsigned)(c.seed & 0xffffffffull); io.key1 = (unsigned)(c.seed >> 32);
    io.cols = c.cols;
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == OBS_INPUT) io.src[s] = {c.input, c.input_stride, c.input_dtype == OBS_F32, 0};
        else io.src[s] = {fields[f].base, fields[f].stride, 0, 0};
    }
    io.rows = c.rows; io.srow = c.srow; io.frames = c.frames; io.refill = refill;
    return io;
}
/* cassie_reward_kernel's: the sources of the record's slots where the batch reads them today (as make_obs_io), the term table, the
 * rewards, the term rows, the returns and the clip */
inline RewardIO make_reward_io(const RewardCfg &c, const ObsField *fields, int env0, int n, const int *reset) {
    RewardIO io = zeroed<RewardIO>();
    io.env0 = env0; io.n = n; io.nterms = c.nterms; io.f32 = c.dtype == OBS_F32;
    io.lo = c.lo; io.hi = c.hi;
    io.terms = c.terms;
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == REW_INPUT) io.src[s] = {c.input, c.input_stride, c.input_dtype == OBS_F32, 0};
        else io.src[s] = {fields[f].base, fields[f].stride, 0, 0};
    }
    io.rew = c.rew; io.srew = c.srew; io.trows = c.trows; io.sterm = c.sterm; io.ret = c.ret; io.fin = c.fin; io.reset = reset;
    return io;
}
/* cassie_act_kernel's: the sources and the destinations of the record's slots where the batch reads them today (fields [nfields]: its own
 * buffers or the caller's bound tensors, with their row strides; the caller's input array), the column table, the actions, the rows, the
 * state, the counts, the delays and the key */
inline ActIO make_act_io(const ActCfg &c, const ObsField *fields, int env0, int n, const int *reset) {
    ActIO io = zeroed<ActIO>();
    io.env0 = env0; io.n = n; io.ncols = c.ncols; io.delay_max = c.delay_max; io.f32 = c.dtype == OBS_F32; io.act_f32 = c.act_dtype == OBS_F32;
    io.env_base = c.env_base; io.key0 = (unsigned)(c.seed & 0xffffffffull); io.key1 = (unsigned)(c.seed >> 32);
    io.cols = c.cols;
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == ACT_INPUT) io.src[s] = {c.input, c.input_stride, c.input_dtype == OBS_F32, 0};
        else io.src[s] = {fields[f].base, fields[f].stride, 0, 0};
    }
    fill_destinations(io.dst, c.ndst, c.dst_field, fields);
    io.actions = c.actions; io.sact = c.act_stride;
    io.rows = c.rows; io.srow = c.srow; io.state = c.state; io.counts = c.counts; io.delay = c.delay; io.reset = reset;
    return io;
}
/* cassie_task_kernel's: the destinations of the record's slots where the batch reads them today (as make_act_io), the column table, the
 * reference table, the rows, the state, the words, the counts and the key */
inline TaskIO make_task_io(const TaskCfg &c, const ObsField *fields, int env0, int n, const int *reset) {
    TaskIO io = zeroed<TaskIO>();
    io.env0 = env0; io.n = n; io.ncols = c.ncols; io.f32 = c.dtype == OBS_F32;
    io.env_base = c.env_base; io.key0 = (unsigned)(c.seed & 0xffffffffull); io.key1 = (unsigned)(c.seed >> 32);
    io.cols = c.cols;
    if (c.tcol_need > 0) { io.table = c.table; io.nframes = c.nframes; io.tcols = c.tcols; }
    fill_destinations(io.dst, c.ndst, c.dst_field, fields);
    io.rows = c.rows; io.srow = c.srow; io.state = c.state; io.words = c.words; io.counts = c.counts; io.reset = reset;
    return io;
}
/* cassie_event_kernel's: the sources of the record's slots where the batch reads them today (as make_reward_io), the column table, the
 * rows, the done words, the state, the words and the counts; nenv: the envs of the batch (the stride of the state's columns) */
inline EventIO make_events_io(const EventCfg &c, const ObsField *fields, int nenv, int env0, int n, const int *reset) {
    EventIO io = zeroed<EventIO>();
    io.env0 = env0; io.n = n; io.ncols = c.ncols; io.f32 = c.dtype == OBS_F32; io.nenv = nenv; io.done_mask = c.done_mask;
    io.cols = c.cols;
    for (int s = 0; s < c.nslots; ++s) {
        const int f = c.slot_field[s];
        if (f == EV_INPUT) io.src[s] = {c.input, c.input_stride, c.input_dtype == OBS_F32, 0};
        else io.src[s] = {fields[f].base, fields[f].stride, 0, 0};
    }
    io.rows = c.rows; io.srow = c.srow; io.flags = c.flags; io.state = c.state; io.words = c.words; io.counts = c.counts; io.reset = reset;
    return io;
}
inline int episode_row_dim(const BatchView &v) { return v.nq + v.nv + v.nsd + v.nu + v.nv; }
/* place null: cassie_episode_kernel's; else cassie_episode_place_kernel's (the next terrains count only while a bank is set) */
inline EpisodeIO make_episode_io(const BatchView &v, const EpisodeCfg &e, const PlaceCfg *place, int env0, int n, int restart, const int *pick, const int *force) {
    EpisodeIO io = zeroed<EpisodeIO>();
    fill_state(io, v);
    io.env0 = env0; io.n = n; io.restart = restart ? 1 : 0; io.nrows = e.nrows; io.row_dim = episode_row_dim(v);
    io.rules = e.rules; io.warn = v.warn;
    io.done = e.done; io.reason = e.reason; io.steps = e.steps; io.count = e.count; io.terminal = e.terminal;
    io.bank = e.bank; io.pick = pick; io.force = force;
    if (place) {
        fill_surface(io, v);
        io.model = v.models;
        io.place_anchor = place->anchor; io.place_npoints = place->npoints; io.place_ground_ref = place->ground_ref; io.place_table = place->table;
        io.place_offsets = place->offsets; io.place_pose = place->pose; io.place_ground = place->ground;
        if (v.hfield_nterrain > 0) io.place_next = place->next;
    }
    return io;
}
/* cassie_state_save_kernel's and cassie_state_restore_kernel's: the sections of the configured groups, each with the view's array (null
 * where the batch has none: the measurement block and the drive-level state until a drive mode is in use, the terrain index without a
 * bank of terrains), its stride in bytes and its place in the row */
inline StateIO make_state_io(const BatchView &v, const StateCfg &c, int env0, int n, const int *slots) {
    StateIO io = zeroed<StateIO>();
    const StateLayout L = state_layout(v, c.groups);
    io.env0 = env0; io.n = n; io.nslots = c.nslots; io.row_dim = L.row_dim; io.bank = c.bank; io.slots = slots; io.warn = v.warn;
    const size_t D = sizeof(double);
    void *const env[SS_COUNT] = {v.time, v.qpos, v.qvel, v.warm, v.ctrl, v.qacc, v.sens, v.actvel, v.meas, v.drive, v.xpos_w, v.xquat_w, v.warn,
                                 v.pd_ptarget, v.pd_kp, v.pd_kd, v.pd_dtarget, v.pd_torque, v.drive_cmd, v.qfrc_applied, v.xfrc_applied,
                                 v.ep_steps, v.ep_count, v.hfield_nterrain > 0 ? v.hfield_index : nullptr, v.params_w};
    const size_t stride[SS_COUNT] = {D, D * v.sq, D * v.sqv, D * v.nv, D * v.nu, D * v.nv, D * v.ssd, D * v.nu, D * CM_MEAS_DIM, sizeof(cm_drive_state_t),
                                     D * 3 * v.nbody, D * 4 * v.nbody, sizeof(int), D * v.nu, D * v.nu, D * v.nu, D * v.nu, D * v.nu, D * (v.nu + 1), D * v.nv,
                                     D * 6 * v.nbody, sizeof(int), sizeof(int), sizeof(int), sizeof(cm_envparams_t)};
    for (int s = 0; s < SS_COUNT; ++s) {
        if (L.off[s] < 0) continue;
        const bool word32 = s == SS_WARN || s == SS_EP_STEPS || s == SS_EP_COUNT || s == SS_TERRAIN;
        io.sect[io.nsect++] = {env[s], (unsigned long)stride[s], L.off[s], L.count[s], word32 ? STATE_INT32 : STATE_WORDS, 0};
    }
    return io;
}
inline ResetIO make_reset_io(const BatchView &v, int first, int stride, int count, const double *qpos_row, const double *sens_row) {
    ResetIO io = zeroed<ResetIO>();
    fill_state(io, v);
    io.first = first; io.stride = stride; io.count = count; io.qpos_row = qpos_row; io.sens_row = sens_row;
    return io;
}
inline DeriveIO make_derive_io(const BatchView &v, int nenv, const cm_ext_t *ext, double *derived, double *qM, const int *ids) {
    DeriveIO io = zeroed<DeriveIO>();
    io.models = v.models; io.model_stride = v.model_stride; io.nenv = nenv; io.envparams = v.envparams;
    io.ext = ext; io.xpos = v.xpos; io.xquat = v.xquat; io.derived = derived; io.qM = qM;
    for (int i = 0; i < 6; ++i) io.ids[i] = ids[i];
    return io;
}
/* mode: a SETCONST_* value */
inline SetConstIO make_setconst_io(const cm_model_t *model, cm_envparams_t *params, int env0, int n, int mode) {
    SetConstIO io = zeroed<SetConstIO>();
    io.model = model; io.params = params; io.env0 = env0; io.nenv = n; io.derive_inertial = mode;
    return io;
}

/* ---- the policy rows ---- */

/* the policy (phys_batch_policy_configure; nnets 0: not configured): the networks with the offsets of their packed layers, the packed
 * floats in all, and a bit per (network, layer) that has been loaded (bit POLICY_MAXLAYERS net + layer).  Then what the caller names once
 * a kernel reads them: the packed floats, the input rows with their stride, the normalisation (mean null: none), the outputs, the sample
 * (eps null: none) */
struct PolicyCfg {
    int nnets, in_dim;
    int rows0, rows1;       /* the rows of the kernel's two LDS buffers: buffer 0 holds the input and the output of a network's layers 1 and 3, buffer 1 of layers 0 and 2 */
    unsigned loaded;
    long long packed_floats;
    PolicyNet net[POLICY_MAXNETS];
    float *packed;
    const float *x; long long sx;
    const float *mean, *inv; double clip;
    float *out[POLICY_MAXNETS]; long long sout[POLICY_MAXNETS];
    const float *eps; long long seps; const float *log_std; float *action; long long saction; float *logp;
};
constexpr const char *POLICY_NOT_CONFIGURED = "not configured (phys_batch_policy_configure first)";
/* (what the launcher also answers a call without a batch) */
constexpr const char *POLICY_SIZE_REFUSAL = "a policy is 1 or 2 networks (0 releases them) of 1 .. 4 layers";
/* the policy's configuration: checks the caller's networks and fills c but for what the caller names later.  nnets 0 is accepted and
 * leaves c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *policy_configure(const PolicyNetDef *nets, int nnets, int in_dim, PolicyCfg &c) {
    c = {};
    if (nnets < 0 || nnets > POLICY_MAXNETS || (nnets > 0 && !nets)) return POLICY_SIZE_REFUSAL;
    if (nnets == 0) return nullptr;
    if (in_dim < 1 || in_dim > POLICY_MAXDIM) return "in_dim lies in 1 .. 512";
    long long at = 0;
    for (int a = 0; a < nnets; ++a) {
        const PolicyNetDef &d = nets[a];
        if (d.nlayers < 1 || d.nlayers > POLICY_MAXLAYERS) return POLICY_SIZE_REFUSAL;
        PolicyNet &N = c.net[a];
        N.nlayers = d.nlayers;
        for (int l = 0; l < d.nlayers; ++l) {
            const PolicyLayerDef &L = d.layer[l];
            if (L.out < 1 || L.out > POLICY_MAXDIM || L.in < 1 || L.in > POLICY_MAXDIM) return "a layer's width lies in 1 .. 512";
            if (L.act != POL_IDENTITY && L.act != POL_RELU && L.act != POL_ELU && L.act != POL_TANH)
                return "a layer's activation is PHYS_POL_IDENTITY, PHYS_POL_RELU, PHYS_POL_ELU or PHYS_POL_TANH";
            if (l == 0 && L.in != in_dim) return "a network's first layer reads in_dim elements";
            if (l > 0 && L.in != d.layer[l - 1].out) return "a layer reads as many elements as the layer before it has units";
            if (l == d.nlayers - 1 && L.out > POLICY_MAXOUT) return "a network's last layer has at most 64 units";
            PolicyLayer &P = N.layer[l];
            P.in = L.in; P.out = L.out; P.act = L.act; P.k4 = (L.in + 3) & ~3; P.out16 = (L.out + 15) & ~15;
            if (l == 0 && P.k4 > c.rows0) c.rows0 = P.k4;
            int &rows = (l & 1) ? c.rows0 : c.rows1;
            if (P.out16 > rows) rows = P.out16;
            P.w_off = at; at += (long long)P.out16 * P.k4;
            P.b_off = at; at += P.out16;
        }
    }
    c.nnets = nnets; c.in_dim = in_dim; c.packed_floats = at;
    return nullptr;
}
inline unsigned policy_layer_bit(int net, int layer) { return 1u << (POLICY_MAXLAYERS * net + layer); }
/* what phys_batch_policy_load / _load_host and the binding functions refuse */
inline const char *check_policy_load(const PolicyCfg &c, int net, int layer, const void *w, long long w_row_stride, const void *b) {
    if (c.nnets < 1) return POLICY_NOT_CONFIGURED;
    if (net < 0 || net >= c.nnets || layer < 0 || layer >= c.net[net].nlayers) return "no such network or layer";
    if (!w || !b) return "a layer needs its weights and its biases";
    if (w_row_stride < c.net[net].layer[layer].in) return "a weight row stride of at least the layer's in";
    return nullptr;
}
inline const char *check_policy_bind_input(const PolicyCfg &c, int dim, long long row_stride, int dtype) {
    if (c.nnets < 1) return POLICY_NOT_CONFIGURED;
    if (dtype == OBS_F64) return "a float64 input is refused: the products with float32 weights would not be exact in a double (bind the float32 row)";
    if (dtype != OBS_F32) return "the input's dtype is PHYS_OBS_F32";
    if (dim != c.in_dim) return "the input's rows hold in_dim elements";
    if (row_stride < dim) return "a row stride of at least the row";
    return nullptr;
}
inline const char *check_policy_bind_norm(const PolicyCfg &c, const void *mean, const void *inv, double clip) {
    if (c.nnets < 1) return POLICY_NOT_CONFIGURED;
    if (!mean || !inv) return "a normalisation needs its mean and its inv";
    if (!(clip >= 0)) return "the clip is >= 0 or +inf";
    return nullptr;
}
inline const char *check_policy_bind_output(const PolicyCfg &c, int net, long long row_stride) {
    if (c.nnets < 1) return POLICY_NOT_CONFIGURED;
    if (net < 0 || net >= c.nnets) return "no such network";
    if (row_stride < c.net[net].layer[c.net[net].nlayers - 1].out) return "a row stride of at least the network's output width";
    return nullptr;
}
inline const char *check_policy_bind_sample(const PolicyCfg &c, long long eps_stride, const void *log_std, const void *action, long long action_stride, const void *logp) {
    if (c.nnets < 1) return POLICY_NOT_CONFIGURED;
    if (!log_std || !action || !logp) return "a sample needs eps, log_std, the action tensor and logp";
    const int A = c.net[0].layer[c.net[0].nlayers - 1].out;
    if (eps_stride < A || action_stride < A) return "row strides of eps and of the action tensor of at least the actor's output width";
    return nullptr;
}
/* what a policy call refuses */
inline const char *check_policy_call(const PolicyCfg &c, int nenv, int env0, int n) {
    if (c.nnets < 1 || !c.packed) return POLICY_NOT_CONFIGURED;
    for (int a = 0; a < c.nnets; ++a)
        for (int l = 0; l < c.net[a].nlayers; ++l)
            if (!(c.loaded & policy_layer_bit(a, l))) return "a layer was never loaded (phys_batch_policy_load first)";
    if (!c.x) return "no input bound (phys_batch_policy_bind_input first)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    return nullptr;
}
/* a workgroup per network of a tile of POLICY_TILE envs up to POLICY_GRID workgroups, which then walk the jobs (policy_kernels.h) */
inline int policy_grid(int n, int nnets) { const long long t = ((long long)n + POLICY_TILE - 1) / POLICY_TILE * nnets; return t < POLICY_GRID ? (int)t : POLICY_GRID; }
/* a wave per 64 packed words up to POLICY_PACK_GRID workgroups */
inline int policy_pack_grid(const PolicyLayer &L) {
    const long long w = ((long long)L.out16 * L.k4 + L.out16 + WV_WAVE - 1) / WV_WAVE;
    return w < POLICY_PACK_GRID ? (int)w : POLICY_PACK_GRID;
}
/* the dynamic LDS of a policy launch: the two buffers' rows of POLICY_TILE floats (at most 64 KiB) */
inline unsigned policy_lds_bytes(const PolicyCfg &c) { return (unsigned)(c.rows0 + c.rows1) * POLICY_TILE * (unsigned)sizeof(float); }
/* cassie_policy_kernel's */
inline PolicyIO make_policy_io(const PolicyCfg &c, int env0, int n) {
    PolicyIO io = zeroed<PolicyIO>();
    io.env0 = env0; io.n = n; io.nnets = c.nnets; io.in_dim = c.in_dim; io.rows0 = c.rows0; io.rows1 = c.rows1;
    for (int a = 0; a < c.nnets; ++a) { io.net[a] = c.net[a]; io.out[a] = c.out[a]; io.sout[a] = c.sout[a]; }
    io.packed = c.packed; io.x = c.x; io.sx = c.sx;
    io.mean = c.mean; io.inv = c.inv; io.clip = c.clip;
    io.eps = c.eps; io.seps = c.seps; io.log_std = c.log_std; io.action = c.action; io.saction = c.saction; io.logp = c.logp;
    return io;
}
/* cassie_policy_pack_kernel's: layer `layer` of network `net` from w (rows sw elements apart) and b to dst, where the layer's packed
 * weights begin (the batch's packed floats + w_off, or a staging array of the layer's own); its biases follow them */
inline PolicyPackIO make_policy_pack_io(const PolicyCfg &c, int net, int layer, const float *w, long long sw, const float *b, float *dst) {
    PolicyPackIO io = zeroed<PolicyPackIO>();
    const PolicyLayer &L = c.net[net].layer[layer];
    io.w = w; io.sw = sw; io.b = b; io.dst_w = dst; io.dst_b = dst + (L.b_off - L.w_off);
    io.in = L.in; io.out = L.out; io.k4 = L.k4; io.out16 = L.out16;
    return io;
}
/* the pack kernel's words on the host (phys_batch_policy_load_host): the same index arithmetic, word for word */
inline void policy_pack_host(const PolicyPackIO &io) {
    const long long per = 16ll * io.k4, total = (long long)(io.out16 >> 4) * per;
    for (long long p = 0; p < total; ++p) {
        const long long ub = p / per, r = p - ub * per;
        const int l = (int)(r & 63), unit = (int)ub * 16 + (l & 15), k = (int)(r >> 6) * 4 + (l >> 4);
        io.dst_w[p] = unit < io.out && k < io.in ? io.w[(size_t)unit * (size_t)io.sw + (size_t)k] : 0.0f;
    }
    for (int unit = 0; unit < io.out16; ++unit) io.dst_b[unit] = unit < io.out ? io.b[unit] : 0.0f;
}

/* ---- the rollout rows ---- */

/* an array of the rollout in device memory: its first word, the words between two steps and between two envs */
struct RolloutStore { void *ptr; long long step, row; };
/* the rollout (phys_batch_rollout_configure; nsrc 0: not configured): the steps, the sources with their roles and dims, gamma, lambda and
 * their product rounded once, the mask of the reasons that count as a time limit; the pointers and row strides the caller bound to
 * sources (null: resolved at every call).  Then what the caller or the launcher names once a kernel reads them: the store of every
 * source, ADV, RET and ADVN (null until normalise is first used, or bound), the per-env partials and the statistics */
struct RolloutCfg {
    int T, nsrc; unsigned tmask;
    double gamma, lambda, gl;
    int role[ROLLOUT_MAXSRC], dim[ROLLOUT_MAXSRC];
    const void *src[ROLLOUT_MAXSRC]; long long ssrc[ROLLOUT_MAXSRC];
    RolloutStore store[ROLLOUT_MAXSRC], adv, ret, advn;
    double *q1, *q2, *stats;
};
/* where the batch reads or writes the things a source without a pointer of its own is resolved from, at this moment: the policy's bound
 * input (null: none) with its width and row stride, network 0's bound output, network 1's, the sample's action tensor and log-probabilities
 * with the actor's width, the rewards with their type (0: not configured), the episodes' done and reason words (null: not enabled) */
struct RolloutLive {
    const void *obs; int obs_dim; long long obs_stride;
    const void *mu; int mu_dim; long long mu_stride;
    const void *value; long long value_stride;
    const void *action; int action_dim; long long action_stride; const void *logp;
    const void *rew; long long rew_stride; int rew_dtype;
    const void *done, *reason;
};
constexpr const char *ROLLOUT_NOT_CONFIGURED = "not configured (phys_batch_rollout_configure first)";
/* (what the launcher also answers a call without a batch) */
constexpr const char *ROLLOUT_SIZE_REFUSAL = "a rollout is 1 .. 1024 steps of 1 .. 16 sources (0 releases them)";
inline bool rollout_is_single_role(int role) { return role >= RO_OBS && role <= RO_REASON; }
/* the rollout's configuration: checks the caller's sources and fills c but for what is bound or named later.  nsrc 0 is accepted and leaves
 * c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *rollout_configure(const RolloutSrcDef *srcs, int nsrc, int T, double gamma, double lambda, unsigned tmask, RolloutCfg &c) {
    c = {};
    if (nsrc < 0 || nsrc > ROLLOUT_MAXSRC || (nsrc > 0 && !srcs)) return ROLLOUT_SIZE_REFUSAL;
    if (nsrc == 0) return nullptr;
    if (T < 1 || T > ROLLOUT_MAXT) return ROLLOUT_SIZE_REFUSAL;
    if (!(gamma >= 0.0 && gamma <= 1.0)) return "gamma is finite and lies in [0, 1]";
    if (!(lambda >= 0.0 && lambda <= 1.0)) return "lambda is finite and lies in [0, 1]";
    bool reason = false;
    for (int s = 0; s < nsrc; ++s) {
        const int role = srcs[s].role, dim = srcs[s].dim;
        if (role != RO_DATA && !rollout_is_single_role(role)) return "a source's role is PHYS_RO_DATA, _OBS, _ACTION, _LOGP, _MU, _VALUE, _REWARD, _DONE or _REASON";
        if (dim < 1 || dim > ROLLOUT_MAXDIM) return "a source's dim lies in 1 .. 4096 words";
        if ((role == RO_VALUE || role == RO_REWARD || role == RO_DONE || role == RO_REASON || role == RO_LOGP) && dim != 1)
            return "VALUE, REWARD, DONE, REASON and LOGP have dim 1";
        if (role != RO_DATA)
            for (int k = 0; k < s; ++k) if (srcs[k].role == role) return "a role other than PHYS_RO_DATA names at most one source";
        reason = reason || role == RO_REASON;
        c.role[s] = role; c.dim[s] = dim;
    }
    if (tmask != 0u && !reason) return "a timeout_mask needs a REASON source";
    c.T = T; c.nsrc = nsrc; c.tmask = tmask; c.gamma = gamma; c.lambda = lambda; c.gl = gamma * lambda;
    return nullptr;
}
/* the source an int names: an index 0 .. nsrc - 1, or the role of exactly one source (-1: none, or a role several DATA sources share) */
inline int rollout_source_of(const RolloutCfg &c, int s_or_role) {
    if (s_or_role >= 0 && s_or_role < ROLLOUT_MAXSRC) return s_or_role < c.nsrc ? s_or_role : -1;
    int found = -1;
    for (int s = 0; s < c.nsrc; ++s) if (c.role[s] == s_or_role) { if (found >= 0) return -1; found = s; }
    return found;
}
/* the array an int names: a source's store, or ADV / RET / ADVN (null: none) -- with the words of its rows */
inline RolloutStore *rollout_store_of(RolloutCfg &c, int s_or_role, int &dim) {
    dim = 1;
    if (s_or_role == RO_ADV) return &c.adv;
    if (s_or_role == RO_RET) return &c.ret;
    if (s_or_role == RO_ADVN) return &c.advn;
    const int s = rollout_source_of(c, s_or_role);
    if (s < 0) return nullptr;
    dim = c.dim[s];
    return &c.store[s];
}
constexpr const char *ROLLOUT_NO_SUCH = "no such source: an index below the configured count, the role of exactly one source, or PHYS_RO_ADV, _RET, _ADVN";
inline const char *check_rollout_bind_source(const RolloutCfg &c, int s_or_role, const void *ptr, long long row_stride) {
    if (c.nsrc < 1) return ROLLOUT_NOT_CONFIGURED;
    const int s = rollout_source_of(c, s_or_role);
    if (s < 0) return ROLLOUT_NO_SUCH;
    if (ptr && row_stride < c.dim[s]) return "a row stride of at least the source's dim";
    return nullptr;
}
/* a caller's tensor in the place of a store: steps and rows may be padded, never overlap */
inline const char *check_rollout_bind_storage(RolloutCfg &c, int nenv, int s_or_role, const void *ptr, long long step_stride, long long row_stride) {
    if (c.nsrc < 1) return ROLLOUT_NOT_CONFIGURED;
    int dim;
    if (!rollout_store_of(c, s_or_role, dim)) return ROLLOUT_NO_SUCH;
    if (!ptr) return nullptr;
    if (row_stride < dim) return "a row stride of at least the source's dim";
    if (step_stride < (long long)(nenv - 1) * row_stride + dim) return "a step stride of at least a step's rows";
    return nullptr;
}
/* where source s is read at this call: the caller's pointer, or what the batch reads or writes of its role now.  DONE and REASON are
 * int32 words, everything else resolved is float32 */
inline const char *rollout_resolve(const RolloutCfg &c, const RolloutLive &L, int s, const void *&ptr, long long &stride) {
    if (c.src[s]) { ptr = c.src[s]; stride = c.ssrc[s]; return nullptr; }
    int dim = 1;
    switch (c.role[s]) {
    case RO_DATA: return "a PHYS_RO_DATA source has no pointer (phys_batch_rollout_bind_source first)";
    case RO_OBS: ptr = L.obs; stride = L.obs_stride; dim = L.obs_dim; if (!ptr) return "OBS: the policy has no input bound to resolve it from"; break;
    case RO_MU: ptr = L.mu; stride = L.mu_stride; dim = L.mu_dim; if (!ptr) return "MU: network 0 has no output bound to resolve it from"; break;
    case RO_VALUE: ptr = L.value; stride = L.value_stride; if (!ptr) return "VALUE: network 1 has no output bound to resolve it from"; break;
    case RO_ACTION: ptr = L.action; stride = L.action_stride; dim = L.action_dim; if (!ptr) return "ACTION: the policy has no sample bound to resolve it from"; break;
    case RO_LOGP: ptr = L.logp; stride = 1; if (!ptr) return "LOGP: the policy has no sample bound to resolve it from"; break;
    case RO_REWARD:
        if (!L.rew) return "REWARD: the rewards are not configured";
        if (L.rew_dtype != OBS_F32) return "REWARD: the rewards must be configured PHYS_OBS_F32 (a source is 32-bit words)";
        ptr = L.rew; stride = L.rew_stride; break;
    case RO_DONE: ptr = L.done; stride = 1; if (!ptr) return "DONE: episodes are not enabled (phys_batch_episodes_enable, or bind the source)"; break;
    case RO_REASON: ptr = L.reason; stride = 1; if (!ptr) return "REASON: episodes are not enabled (phys_batch_episodes_enable, or bind the source)"; break;
    default: return ROLLOUT_NO_SUCH;
    }
    if (dim != c.dim[s]) return "a resolved source's dim no longer fits the configured dim";
    if (stride < c.dim[s]) return "a resolved source's row stride no longer fits the configured dim";
    return nullptr;
}
/* what a record call refuses */
inline const char *check_rollout_record(const RolloutCfg &c, const RolloutLive &L, int nenv, int t, int env0, int n) {
    if (c.nsrc < 1) return ROLLOUT_NOT_CONFIGURED;
    if (t < 0 || t >= c.T) return "the slot t lies in 0 .. T - 1";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    for (int s = 0; s < c.nsrc; ++s) {
        const void *p; long long st;
        if (const char *why = rollout_resolve(c, L, s, p, st)) return why;
        if (!c.store[s].ptr) return "a source has no store";
    }
    return nullptr;
}
inline bool rollout_aligned16(const void *p) { return ((unsigned long long)(__UINTPTR_TYPE__)p & 15ull) == 0ull; }
/* cassie_rollout_record_kernel's (after check_rollout_record): per source the rows of env0 on both sides, and whether a lane moves 16 bytes */
inline RolloutRecIO make_rollout_rec_io(const RolloutCfg &c, const RolloutLive &L, int t, int env0, int n) {
    RolloutRecIO io = zeroed<RolloutRecIO>();
    io.n = n; io.nsrc = c.nsrc;
    long long job = 0;
    for (int s = 0; s < c.nsrc; ++s) {
        const void *p = nullptr; long long st = 0;
        (void)rollout_resolve(c, L, s, p, st);
        RolloutRecSrc &S = io.s[s];
        S.src = (const unsigned *)p + (size_t)env0 * (size_t)st; S.ssrc = st;
        S.dst = (unsigned *)c.store[s].ptr + (size_t)t * (size_t)c.store[s].step + (size_t)env0 * (size_t)c.store[s].row; S.sdst = c.store[s].row;
        S.dim = c.dim[s];
        S.vec = rollout_aligned16(S.src) && rollout_aligned16(S.dst) && (S.dim & 3) == 0 && (S.ssrc & 3) == 0 && (S.sdst & 3) == 0;
        S.job0 = job;
        job += ((long long)n * S.dim + ROLLOUT_JOB - 1) / ROLLOUT_JOB;
    }
    io.njobs = job;
    return io;
}
/* a workgroup per job up to ROLLOUT_GRID, which then walk the jobs */
inline int rollout_record_grid(const RolloutRecIO &io) { return io.njobs < ROLLOUT_GRID ? (int)io.njobs : ROLLOUT_GRID; }
/* the source of a role (-1: none) */
inline int rollout_role(const RolloutCfg &c, int role) { for (int s = 0; s < c.nsrc; ++s) if (c.role[s] == role) return s; return -1; }
/* what a finish call refuses.  last null: the VALUE source as resolved now */
inline const char *check_rollout_finish(const RolloutCfg &c, const RolloutLive &L, int nenv, int env0, int n, const void *last, long long stride) {
    if (c.nsrc < 1) return ROLLOUT_NOT_CONFIGURED;
    const int sv = rollout_role(c, RO_VALUE), sr = rollout_role(c, RO_REWARD);
    if (sv < 0 || sr < 0) return "finish needs a VALUE and a REWARD source";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    if (!c.adv.ptr || !c.ret.ptr || !c.q1) return "ADV or RET has no store";
    if (last) return stride < 1 ? "a stride of the last values of at least 1" : nullptr;
    const void *p; long long st;
    return rollout_resolve(c, L, sv, p, st);
}
/* cassie_rollout_finish_kernel's (after check_rollout_finish) */
inline RolloutFinIO make_rollout_fin_io(const RolloutCfg &c, const RolloutLive &L, int env0, int n, const void *last, long long stride) {
    RolloutFinIO io = zeroed<RolloutFinIO>();
    const int sv = rollout_role(c, RO_VALUE), sr = rollout_role(c, RO_REWARD), sd = rollout_role(c, RO_DONE), sq = rollout_role(c, RO_REASON);
    io.env0 = env0; io.n = n; io.T = c.T; io.tmask = sd >= 0 && sq >= 0 ? c.tmask : 0u; io.gamma = c.gamma; io.gl = c.gl;
    io.val = (const float *)c.store[sv].ptr; io.val_step = c.store[sv].step; io.val_row = c.store[sv].row;
    io.rew = (const float *)c.store[sr].ptr; io.rew_step = c.store[sr].step; io.rew_row = c.store[sr].row;
    if (sd >= 0) { io.done = (const int *)c.store[sd].ptr; io.done_step = c.store[sd].step; io.done_row = c.store[sd].row; }
    if (sq >= 0) { io.reason = (const int *)c.store[sq].ptr; io.reason_step = c.store[sq].step; io.reason_row = c.store[sq].row; }
    if (!last) (void)rollout_resolve(c, L, sv, last, stride);
    io.last = (const float *)last; io.last_row = stride;
    io.adv = (float *)c.adv.ptr; io.adv_step = c.adv.step; io.adv_row = c.adv.row;
    io.ret = (float *)c.ret.ptr; io.ret_step = c.ret.step; io.ret_row = c.ret.row;
    io.q1 = c.q1;
    return io;
}
/* lane = env: a workgroup per 64 envs up to ROLLOUT_FIN_GRID */
inline int rollout_env_grid(int n) { const int w = (n + WV_WAVE - 1) / WV_WAVE; return w < ROLLOUT_FIN_GRID ? w : ROLLOUT_FIN_GRID; }
/* what a normalise call refuses (ADVN: the launcher allocates it before this check, or the caller bound it) */
inline const char *check_rollout_normalise(const RolloutCfg &c, int nenv, double eps) {
    if (c.nsrc < 1) return ROLLOUT_NOT_CONFIGURED;
    if ((long long)c.T * nenv < 2) return "normalise needs T * nenv >= 2";
    if (!(eps >= 0.0 && eps < INFINITY)) return "eps is finite and >= 0";
    if (!c.adv.ptr || !c.advn.ptr || !c.q1 || !c.q2 || !c.stats) return "ADV or ADVN has no store";
    return nullptr;
}
/* the three normalise kernels' (stage: the reduce kernel's) */
inline RolloutNormIO make_rollout_norm_io(const RolloutCfg &c, int nenv, double eps, int stage) {
    RolloutNormIO io = zeroed<RolloutNormIO>();
    const long long M = (long long)c.T * nenv;
    io.nenv = nenv; io.T = c.T; io.stage = stage; io.count = (double)M; io.count1 = (double)(M - 1); io.eps = eps;
    io.adv = (const float *)c.adv.ptr; io.adv_step = c.adv.step; io.adv_row = c.adv.row;
    io.advn = (float *)c.advn.ptr; io.advn_step = c.advn.step; io.advn_row = c.advn.row;
    io.q1 = c.q1; io.q2 = c.q2; io.stats = c.stats;
    return io;
}
/* a workgroup per (step, block of 64 envs) up to ROLLOUT_SCALE_GRID */
inline int rollout_scale_grid(int nenv, int T) { const long long j = ((long long)nenv + WV_WAVE - 1) / WV_WAVE * T; return j < ROLLOUT_SCALE_GRID ? (int)j : ROLLOUT_SCALE_GRID; }

/* ---- the gradient rows ---- */

/* the gradient (phys_batch_grad_configure; max_m 0: not configured): the largest minibatch, the chunk (part of the definition: it fixes the
 * order of the weight sums), max_m rounded up to the chunk and the chunks that makes; eps with 1 - eps and 1 + eps rounded once, the two
 * coefficients; where every network's rows begin in the stores and how large the stores are; the (network, layer) slots in launch order
 * with the first float of their dW and db among the batch's own gradient floats (dls follows the last).  The caller's gradient tensors
 * (null: the batch's own).  Then what the launcher names once a kernel reads them */
struct GradCfg {
    int max_m, chunk, mcap, maxchunks, nslots, A;
    double eps, lo, hi, c_v, c_ent;
    GradNet g[POLICY_MAXNETS];
    long long act_floats, delta_floats, part_doubles, packt_floats, pos_doubles, own_floats, own_ls;
    int slot_net[GRAD_MAXSLOTS], slot_layer[GRAD_MAXSLOTS];
    long long own_w[GRAD_MAXSLOTS], own_b[GRAD_MAXSLOTS];
    float *dw[GRAD_MAXSLOTS]; long long sdw[GRAD_MAXSLOTS]; float *db[GRAD_MAXSLOTS]; float *dls;
    float *act, *delta, *packt, *own; double *part, *pos, *stats;
};
/* the rollout's arrays a minibatch is gathered from, and the samples the rollout holds */
struct GradSources { GradSrc obs, action, logp, advn, ret; int total; };
constexpr const char *GRAD_NOT_CONFIGURED = "not configured (phys_batch_grad_configure first)";
constexpr const char *GRAD_NEEDS = "the gradient needs a configured policy and rollout (phys_batch_policy_configure, phys_batch_rollout_configure first)";
inline int grad_slot(const GradCfg &c, int net, int layer) {
    for (int s = 0; s < c.nslots; ++s) if (c.slot_net[s] == net && c.slot_layer[s] == layer) return s;
    return -1;
}
/* the gradient's configuration: checks the caller's numbers against the policy and fills c but for what is bound or named later.  max_m 0
 * is accepted and leaves c empty: the launcher releases what it holds.  total: the rollout's T nenv.  The emulator goes through the same */
inline const char *grad_configure(const PolicyCfg &p, long long total, int max_m, int chunk, double eps, double c_v, double c_ent, GradCfg &c) {
    c = {};
    if (max_m == 0) return nullptr;
    if (p.nnets < 1 || total < 1) return GRAD_NEEDS;
    if (total > 0x7fffffffll) return "the rollout's T nenv must fit an int32 index";
    if (max_m < 0 || max_m > total) return "max_m lies in 1 .. T nenv (0 releases)";
    if (chunk < GRAD_MINCHUNK || chunk > GRAD_MAXCHUNK || (chunk & 15) != 0) return "chunk is a multiple of 16 in 16 .. 4096";
    if (!(eps >= 0.0 && eps < INFINITY)) return "clip_eps is finite and >= 0";
    if (!(c_v >= 0.0 && c_v < INFINITY)) return "c_v is finite and >= 0";
    if (!(c_ent >= 0.0 && c_ent < INFINITY)) return "c_ent is finite and >= 0";
    if (p.nnets > 1 && p.net[1].layer[p.net[1].nlayers - 1].out != 1) return "the critic's last layer has one unit";
    c.max_m = max_m; c.chunk = chunk; c.mcap = (int)(((long long)max_m + chunk - 1) / chunk * chunk); c.maxchunks = c.mcap / chunk;
    c.eps = eps; c.lo = 1.0 - eps; c.hi = 1.0 + eps; c.c_v = c_v; c.c_ent = c_ent;
    c.A = p.net[0].layer[p.net[0].nlayers - 1].out;
    const long long mcap = c.mcap;
    long long act = 0, delta = 0, part = 0, packt = 0, own = 0;
    const int in16 = (p.in_dim + 15) & ~15;
    for (int a = 0; a < p.nnets; ++a) {
        GradNet &G = c.g[a];
        const PolicyNet &N = p.net[a];
        G.hw[0] = in16;
        if (a == 0) { G.h_off[0] = act; act += mcap * in16; } else G.h_off[0] = c.g[0].h_off[0];
        for (int l = 0; l < N.nlayers; ++l) {
            const PolicyLayer &L = N.layer[l];
            G.hw[l + 1] = L.out16; G.h_off[l + 1] = act; act += mcap * L.out16;
            G.d_off[l] = delta; delta += mcap * L.out16;
            G.p_off[l] = part; part += (long long)c.maxchunks * L.out * (L.in + 1);
            G.t_off[l] = packt; packt += (long long)G.hw[l] * ((L.out + 3) & ~3);
            const int s = c.nslots++;
            c.slot_net[s] = a; c.slot_layer[s] = l;
            c.own_w[s] = own; own += (long long)L.out * L.in;
            c.own_b[s] = own; own += L.out;
        }
    }
    c.own_ls = own; own += c.A;
    c.act_floats = act; c.delta_floats = delta; c.part_doubles = part; c.packt_floats = packt; c.own_floats = own;
    c.pos_doubles = (long long)(c.A + GRAD_POS_ROWS) * mcap;
    return nullptr;
}
/* what phys_batch_grad_bind refuses (ptr null: the batch's own again) */
inline const char *check_grad_bind(const GradCfg &c, const PolicyCfg &p, int net, int layer, const void *dw, long long dw_row_stride, const void *db) {
    if (c.max_m < 1) return GRAD_NOT_CONFIGURED;
    if (net < 0 || net >= p.nnets || layer < 0 || layer >= p.net[net].nlayers) return "no such network or layer";
    if (!dw != !db) return "a layer's dW and db are bound together (both null: the batch's own)";
    if (dw && dw_row_stride < p.net[net].layer[layer].in) return "a dW row stride of at least the layer's in";
    return nullptr;
}
/* the rollout's arrays the gradient gathers from (null message: all there).  VALUE and RET only with a critic */
inline const char *grad_sources(const RolloutCfg &r, const PolicyCfg &p, int nenv, GradSources &S) {
    S = {};
    if (r.nsrc < 1 || p.nnets < 1) return GRAD_NEEDS;
    const int so = rollout_role(r, RO_OBS), sa = rollout_role(r, RO_ACTION), sl = rollout_role(r, RO_LOGP), sv = rollout_role(r, RO_VALUE);
    if (so < 0 || sa < 0 || sl < 0) return "the rollout needs sources of role OBS, ACTION and LOGP";
    if (p.nnets > 1 && sv < 0) return "with a critic the rollout needs a source of role VALUE";
    if (r.dim[so] != p.in_dim) return "the rollout's OBS rows hold in_dim elements";
    if (r.dim[sa] != p.net[0].layer[p.net[0].nlayers - 1].out) return "the rollout's ACTION rows hold as many elements as the actor has outputs";
    if (!r.store[so].ptr || !r.store[sa].ptr || !r.store[sl].ptr) return "a source has no store";
    if (!r.advn.ptr) return "no ADVN (phys_batch_rollout_normalise first, or bind its storage)";
    if (p.nnets > 1 && !r.ret.ptr) return "no RET (phys_batch_rollout_finish first)";
    auto src = [](const RolloutStore &st) { GradSrc g; g.ptr = (const float *)st.ptr; g.step = st.step; g.row = st.row; return g; };
    S.obs = src(r.store[so]); S.action = src(r.store[sa]); S.logp = src(r.store[sl]); S.advn = src(r.advn);
    if (p.nnets > 1) S.ret = src(r.ret);
    S.total = (int)((long long)r.T * nenv);
    return nullptr;
}
/* what a grad call refuses (after grad_sources) */
inline const char *check_grad_call(const GradCfg &c, const PolicyCfg &p, const void *idx, int m) {
    if (c.max_m < 1 || !c.act || !c.delta || !c.part || !c.packt || !c.pos || !c.stats || !c.own) return GRAD_NOT_CONFIGURED;
    if (p.nnets < 1 || !p.packed) return POLICY_NOT_CONFIGURED;
    for (int a = 0; a < p.nnets; ++a)
        for (int l = 0; l < p.net[a].nlayers; ++l)
            if (!(p.loaded & policy_layer_bit(a, l))) return "a layer was never loaded (phys_batch_policy_load first)";
    if (!p.log_std) return "no log_std (phys_batch_policy_bind_sample first)";
    if (!idx) return "no idx";
    if (m < 1 || m > c.max_m) return "m lies in 1 .. max_m";
    return nullptr;
}
/* the five kernels' (after check_grad_call) */
inline GradIO make_grad_io(const GradCfg &c, const PolicyCfg &p, const GradSources &S, int nenv, const int *idx, int m) {
    GradIO io = zeroed<GradIO>();
    io.m = m; io.chunk = c.chunk; io.mcap = (int)(((long long)m + c.chunk - 1) / c.chunk * c.chunk); io.nchunks = io.mcap / c.chunk;
    io.nnets = p.nnets; io.in_dim = p.in_dim; io.rows0 = p.rows0; io.rows1 = p.rows1;
    io.nenv = nenv; io.total = S.total; io.A = c.A; io.nslots = c.nslots;
    for (int a = 0; a < p.nnets; ++a) { io.net[a] = p.net[a]; io.g[a] = c.g[a]; }
    io.packed = p.packed; io.packt = c.packt; io.idx = idx;
    io.obs = S.obs; io.action = S.action; io.logp = S.logp; io.advn = S.advn; io.ret = S.ret;
    io.mean = p.mean; io.inv = p.inv; io.clip = p.clip; io.log_std = p.log_std;
    io.act = c.act; io.delta = c.delta; io.part = c.part; io.pos = c.pos; io.stats = c.stats;
    io.lo = c.lo; io.hi = c.hi; io.eps = c.eps; io.c_v = c.c_v; io.c_ent = c.c_ent; io.inv_m = 1.0 / (double)m;
    long long job = 0, par = 0;
    for (int s = 0; s < c.nslots; ++s) {
        const PolicyLayer &L = p.net[c.slot_net[s]].layer[c.slot_layer[s]];
        io.slot_net[s] = c.slot_net[s]; io.slot_layer[s] = c.slot_layer[s];
        io.dw[s] = c.dw[s] ? c.dw[s] : c.own + c.own_w[s]; io.sdw[s] = c.dw[s] ? c.sdw[s] : L.in; io.db[s] = c.db[s] ? c.db[s] : c.own + c.own_b[s];
        io.job0[s] = job; io.par0[s] = par;
        job += (long long)io.nchunks * (L.out16 >> 4) * ((((L.in + 16) >> 4) + 3) >> 2);
        par += (long long)L.out * (L.in + 1);
    }
    io.job0[c.nslots] = job; io.par0[c.nslots] = par;
    io.dls = c.dls ? c.dls : c.own + c.own_ls;
    return io;
}
/* note: the chunks of a call are those of ITS m; the stores are laid out for max_m (GradNet's offsets use the configured mcap, a call's
 * rows are its first io.mcap) */
inline int grad_tile_grid(const GradIO &io) { const long long t = (long long)(io.mcap / POLICY_TILE) * io.nnets; return t < GRAD_GRID ? (int)t : GRAD_GRID; }
inline int grad_partial_grid(const GradIO &io) { const long long j = io.job0[io.nslots]; return j < GRAD_PART_GRID ? (int)j : GRAD_PART_GRID; }
inline int grad_reduce_grid(const GradIO &io) { const long long w = (io.par0[io.nslots] + WV_WAVE - 1) / WV_WAVE; return w < GRAD_RED_GRID ? (int)w : GRAD_RED_GRID; }
inline int grad_stats_grid(const GradIO &io) { return io.A + GRAD_POS_ROWS; }
inline bool grad_has_backward(const PolicyCfg &p) { for (int a = 0; a < p.nnets; ++a) if (p.net[a].nlayers > 1) return true; return false; }
/* the dynamic LDS of launches 1 and 2: the policy's two buffers and a word per position of the tile */
inline unsigned grad_lds_bytes(const PolicyCfg &p) { return policy_lds_bytes(p) + POLICY_TILE * (unsigned)sizeof(int); }
/* cassie_grad_pack_kernel's: the transposed packing of layer `layer` of network `net` from the policy's packed weights */
inline GradPackIO make_grad_pack_io(const GradCfg &c, const PolicyCfg &p, int net, int layer) {
    GradPackIO io = zeroed<GradPackIO>();
    const PolicyLayer &L = p.net[net].layer[layer];
    io.src = p.packed + L.w_off; io.dst = c.packt + c.g[net].t_off[layer];
    io.in = L.in; io.out = L.out; io.k4 = L.k4; io.in16 = c.g[net].hw[layer]; io.u4 = (L.out + 3) & ~3;
    return io;
}
inline int grad_pack_grid(const GradPackIO &io) {
    const long long w = ((long long)io.in16 * io.u4 + WV_WAVE - 1) / WV_WAVE;
    return w < GRAD_PACK_GRID ? (int)w : GRAD_PACK_GRID;
}

/* ---- the optimiser rows ---- */

/* the optimiser (phys_batch_opt_configure; on 0: not configured): the betas with 1 - beta rounded once, eps, max_norm (+inf: no clipping);
 * the parameters of the flat order and the segments of the NORM; the master tensors the caller bound (null: not yet).  Then what the
 * launcher names once a kernel reads them: the moments (m [Q], then v [Q]), the segments' partials and the doubles */
struct OptCfg {
    int on, nseg;
    double beta1, beta2, omb1, omb2, eps, max_norm;
    long long Q;
    float *w[GRAD_MAXSLOTS]; long long sw[GRAD_MAXSLOTS]; float *b[GRAD_MAXSLOTS]; float *ls;
    float *mom; double *part, *sc;
};
constexpr const char *OPT_NOT_CONFIGURED = "not configured (phys_batch_opt_configure first)";
constexpr const char *OPT_NEEDS = "the optimiser needs configured gradient rows (phys_batch_grad_configure first)";
/* the release form of phys_batch_opt_configure: eps 0 and max_norm 0 */
inline bool opt_is_release(double eps, double max_norm) { return eps == 0.0 && max_norm == 0.0; }
/* the first parameter of slot s in the flat order (s = nslots: log_std's first) */
inline long long opt_par0(const GradCfg &g, const PolicyCfg &p, int s) {
    long long par = 0;
    for (int k = 0; k < s; ++k) { const PolicyLayer &L = p.net[g.slot_net[k]].layer[g.slot_layer[k]]; par += (long long)L.out * (L.in + 1); }
    return par;
}
/* the optimiser's configuration: checks the caller's numbers and fills c but for what is bound or named later.  The release form is
 * accepted and leaves c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *opt_configure(const GradCfg &g, const PolicyCfg &p, double beta1, double beta2, double eps, double max_norm, OptCfg &c) {
    c = {};
    if (opt_is_release(eps, max_norm)) return nullptr;
    if (g.max_m < 1 || p.nnets < 1) return OPT_NEEDS;
    if (!(beta1 >= 0.0 && beta1 < 1.0)) return "beta1 lies in [0, 1)";
    if (!(beta2 >= 0.0 && beta2 < 1.0)) return "beta2 lies in [0, 1)";
    if (!(eps > 0.0 && eps < INFINITY)) return "eps is finite and > 0";
    if (!(max_norm > 0.0)) return "max_norm is > 0 (+inf: no clipping)";
    c.on = 1; c.beta1 = beta1; c.beta2 = beta2; c.omb1 = 1.0 - beta1; c.omb2 = 1.0 - beta2; c.eps = eps; c.max_norm = max_norm;
    c.Q = opt_par0(g, p, g.nslots) + g.A;
    c.nseg = (int)((c.Q + OPT_SEG - 1) / OPT_SEG);
    return nullptr;
}
/* what phys_batch_opt_bind_param refuses */
inline const char *check_opt_bind_param(const OptCfg &c, const PolicyCfg &p, int net, int layer, const void *w, long long w_row_stride, const void *b) {
    if (!c.on) return OPT_NOT_CONFIGURED;
    if (net < 0 || net >= p.nnets || layer < 0 || layer >= p.net[net].nlayers) return "no such network or layer";
    if (!w || !b) return "a layer's master W and b are both needed";
    if (w_row_stride < p.net[net].layer[layer].in) return "a W row stride of at least the layer's in";
    return nullptr;
}
constexpr const char *OPT_LS_MISMATCH = "the log_std pointer must be the one phys_batch_policy_bind_sample names";
inline const char *check_opt_bind_log_std(const OptCfg &c, const PolicyCfg &p, const void *ptr) {
    if (!c.on) return OPT_NOT_CONFIGURED;
    if (!ptr || ptr != (const void *)p.log_std) return OPT_LS_MISMATCH;
    return nullptr;
}
/* what a step call refuses.  grad_called: whether a phys_batch_grad call has been made since the gradient rows were configured */
inline const char *check_opt_step(const OptCfg &c, const GradCfg &g, const PolicyCfg &p, double lr, bool grad_called) {
    if (!c.on || !c.mom || !c.part || !c.sc) return OPT_NOT_CONFIGURED;
    if (g.max_m < 1 || !g.packt || !g.own || p.nnets < 1 || !p.packed) return OPT_NEEDS;
    for (int s = 0; s < g.nslots; ++s) if (!c.w[s] || !c.b[s]) return "a master tensor is not bound (phys_batch_opt_bind_param for every layer first)";
    if (!c.ls) return "the master log_std is not bound (phys_batch_opt_bind_log_std first)";
    if (c.ls != p.log_std) return OPT_LS_MISMATCH;
    for (int s = 0; s < g.nslots; ++s)
        if (!(p.loaded & policy_layer_bit(g.slot_net[s], g.slot_layer[s]))) return "a layer was never loaded (phys_batch_policy_load first: the packings' padding comes from it)";
    if (!(lr >= 0.0 && lr < INFINITY)) return "lr is finite and >= 0";
    if (!grad_called) return "no gradient yet (phys_batch_grad first)";
    return nullptr;
}
/* the three kernels' (after check_opt_step) */
inline OptIO make_opt_io(const OptCfg &c, const GradCfg &g, const PolicyCfg &p, double lr) {
    OptIO io = zeroed<OptIO>();
    io.nslots = g.nslots; io.A = g.A; io.nseg = c.nseg; io.Q = c.Q;
    long long job = 0, par = 0;
    for (int s = 0; s < g.nslots; ++s) {
        const int net = g.slot_net[s], layer = g.slot_layer[s];
        const PolicyLayer &L = p.net[net].layer[layer];
        OptSlot &S = io.s[s];
        S.gw = g.dw[s] ? g.dw[s] : g.own + g.own_w[s]; S.sgw = g.dw[s] ? g.sdw[s] : L.in; S.gb = g.db[s] ? g.db[s] : g.own + g.own_b[s];
        S.w = c.w[s]; S.sw = c.sw[s]; S.b = c.b[s];
        S.pw = p.packed + L.w_off; S.pb = p.packed + L.b_off; S.pt = g.packt + g.g[net].t_off[layer];
        S.in = L.in; S.out = L.out; S.k4 = L.k4; S.u4 = (L.out + 3) & ~3;
        S.par0 = par; S.job0 = job;
        par += (long long)L.out * (L.in + 1);
        job += (long long)(L.out16 >> 4) * ((L.in + 16) >> 4);
    }
    io.tiles = job; io.njobs = job + (g.A + WV_WAVE - 1) / WV_WAVE;
    io.gls = g.dls ? g.dls : g.own + g.own_ls; io.ls = c.ls;
    io.m = c.mom; io.v = c.mom + c.Q; io.part = c.part; io.sc = c.sc;
    io.beta1 = c.beta1; io.beta2 = c.beta2; io.omb1 = c.omb1; io.omb2 = c.omb2; io.eps = c.eps; io.max_norm = c.max_norm; io.lr = lr;
    return io;
}
inline int opt_sq_grid(const OptIO &io) { return io.nseg < OPT_SQ_GRID ? io.nseg : OPT_SQ_GRID; }
inline int opt_step_grid(const OptIO &io) { return io.njobs < OPT_STEP_GRID ? (int)io.njobs : OPT_STEP_GRID; }
/* the doubles at configuration: t = 0, p1 = p2 = 1, nothing skipped, everything else +0.0 */
inline void opt_initial_scalars(double *sc) {
    for (int k = 0; k < OPT_SC_COUNT; ++k) sc[k] = 0.0;
    sc[OPT_SC_P1] = sc[OPT_SC_P2] = 1.0; sc[6] = sc[7] = 1.0;
}
/* where a thing phys_batch_opt_download / _upload names lies: rows of `width` elements, `pitch` elements apart (floats, or doubles for
 * OPT_SCALARS and OPT_PARTIALS); false: no such thing */
struct OptRegion { void *ptr; long long rows, width, pitch; int doubles; };
inline bool opt_region(const OptCfg &c, const GradCfg &g, const PolicyCfg &p, int what, int net, int layer, OptRegion &R) {
    R = {};
    if (!c.on) return false;
    if (what == OPT_SCALARS) { R.ptr = c.sc ? c.sc + OPT_SC_T : nullptr; R.rows = 1; R.width = R.pitch = 4; R.doubles = 1; return true; }
    if (what == OPT_PARTIALS) { R.ptr = c.part; R.rows = 1; R.width = R.pitch = c.nseg; R.doubles = 1; return true; }
    if (what == OPT_M_LS || what == OPT_V_LS) {
        R.ptr = c.mom ? c.mom + (what == OPT_V_LS ? c.Q : 0) + (c.Q - g.A) : nullptr; R.rows = 1; R.width = R.pitch = g.A; return true;
    }
    if (what < OPT_M_W || what > OPT_V_B) return false;
    const int s = net >= 0 && net < p.nnets && layer >= 0 && layer < p.net[net].nlayers ? grad_slot(g, net, layer) : -1;
    if (s < 0) return false;
    const PolicyLayer &L = p.net[net].layer[layer];
    const bool second = what == OPT_V_W || what == OPT_V_B, bias = what == OPT_M_B || what == OPT_V_B;
    R.ptr = c.mom ? c.mom + (second ? c.Q : 0) + opt_par0(g, p, s) + (bias ? L.in : 0) : nullptr;
    R.rows = L.out; R.width = bias ? 1 : L.in; R.pitch = L.in + 1;
    return true;
}

/* ---- the normaliser rows ---- */

/* the normaliser (phys_batch_norm_configure; on 0: not configured): the columns, the samples of a block, the most samples of a call with
 * the blocks they make, eps; the source the caller bound (src null: the rollout's OBS store, resolved at every call) and the outputs
 * (null: the policy's bound normalisation, resolved at every call).  Then what the launcher names once a kernel reads them: the state
 * [NORM_STATE_ROWS][D], the partials (a1 [max_blocks][D], then a2) and the blocks' counts -- and what the last call left for the
 * statistics and the downloads: its samples, its blocks, the calls so far */
struct NormCfg {
    int on, D, block;
    long long max_rows, max_blocks;
    double eps;
    const float *src; int steps, rows; long long step_stride, row_stride;
    float *out_mean, *out_inv;
    double *state, *part; int *cnt;
    long long last_R, last_blocks, calls;
};
/* a source and the outputs as resolved at a call */
struct NormSource { const float *ptr; int steps, rows; long long step_stride, row_stride; };
struct NormOutput { float *mean, *inv; };
constexpr const char *NORM_NOT_CONFIGURED = "not configured (phys_batch_norm_configure first)";
constexpr const char *NORM_STRIDE_REFUSAL = "strides of at least dim words";
/* the normaliser's configuration: checks the caller's numbers and fills c but for what is bound or named later.  dim 0 is accepted and
 * leaves c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *norm_configure(int dim, int block, long long max_rows, double eps, NormCfg &c) {
    c = {};
    if (dim == 0) return nullptr;
    if (dim < 1 || dim > NORM_MAXDIM) return "dim lies in 1 .. 512 (0 releases)";
    if (block < NORM_MINBLOCK || block > NORM_MAXBLOCK || (block & 15) != 0) return "block is a multiple of 16 in 16 .. 4096";
    if (max_rows < 1 || max_rows > NORM_MAXROWS) return "max_rows lies in 1 .. 2^30";
    if (!(eps > 0.0 && eps < INFINITY)) return "eps is finite and > 0";
    c.on = 1; c.D = dim; c.block = block; c.max_rows = max_rows; c.max_blocks = (max_rows + block - 1) / block; c.eps = eps;
    return nullptr;
}
/* what phys_batch_norm_bind_source refuses (ptr null: back to the rollout's OBS store) */
inline const char *check_norm_bind_source(const NormCfg &c, const void *ptr, int steps, int rows, long long step_stride, long long row_stride) {
    if (!c.on) return NORM_NOT_CONFIGURED;
    if (!ptr) return nullptr;
    if (steps < 1 || rows < 1) return "a source has at least one step of at least one row";
    if (row_stride < c.D || (steps > 1 && step_stride < c.D)) return NORM_STRIDE_REFUSAL;
    return nullptr;
}
/* what phys_batch_norm_bind_output refuses (both null: back to the policy's bound normalisation) */
inline const char *check_norm_bind_output(const NormCfg &c, const void *mean, const void *inv) {
    if (!c.on) return NORM_NOT_CONFIGURED;
    if ((mean == nullptr) != (inv == nullptr)) return "the outputs are a mean and an inv, both or neither";
    return nullptr;
}
/* the source of a call: the caller's, or the store of the rollout's OBS source as it is now, by the reward's convention */
inline const char *norm_resolve_source(const NormCfg &c, const RolloutCfg &r, int nenv, NormSource &S) {
    S = {};
    if (c.src) { S.ptr = c.src; S.steps = c.steps; S.rows = c.rows; S.step_stride = c.step_stride; S.row_stride = c.row_stride; return nullptr; }
    if (r.nsrc < 1) return "no source: no rollout is configured (phys_batch_rollout_configure, or phys_batch_norm_bind_source)";
    const int so = rollout_role(r, RO_OBS);
    if (so < 0 || !r.store[so].ptr) return "no source: the rollout has no OBS source (or phys_batch_norm_bind_source)";
    if (r.dim[so] != c.D) return "the rollout's OBS source does not have dim words";
    S.ptr = (const float *)r.store[so].ptr; S.steps = r.T; S.rows = nenv; S.step_stride = r.store[so].step; S.row_stride = r.store[so].row;
    if (S.row_stride < c.D || (S.steps > 1 && S.step_stride < c.D)) return NORM_STRIDE_REFUSAL;
    return nullptr;
}
/* the outputs of a call: the caller's, or the tensors phys_batch_policy_bind_norm names now */
inline const char *norm_resolve_output(const NormCfg &c, const PolicyCfg &p, NormOutput &O) {
    O = {};
    if (c.out_mean) { O.mean = c.out_mean; O.inv = c.out_inv; return nullptr; }
    if (p.nnets < 1 || !p.mean || !p.inv) return "no output: the policy has no normalisation bound (phys_batch_policy_bind_norm, or phys_batch_norm_bind_output)";
    if (p.in_dim != c.D) return "the policy's in_dim is not dim";
    O.mean = (float *)p.mean; O.inv = (float *)p.inv;
    return nullptr;
}
/* what an update refuses (S and O filled where it accepts) */
inline const char *check_norm_update(const NormCfg &c, const RolloutCfg &r, const PolicyCfg &p, int nenv, NormSource &S, NormOutput &O) {
    if (!c.on || !c.state || !c.part || !c.cnt) return NORM_NOT_CONFIGURED;
    if (const char *why = norm_resolve_source(c, r, nenv, S)) return why;
    if ((long long)S.steps * S.rows > c.max_rows) return "more samples than max_rows";
    return norm_resolve_output(c, p, O);
}
/* what a write refuses */
inline const char *check_norm_write(const NormCfg &c, const PolicyCfg &p, NormOutput &O) {
    if (!c.on || !c.state) return NORM_NOT_CONFIGURED;
    return norm_resolve_output(c, p, O);
}
/* the five kernels' (after the check; a write reads no source: S empty) */
inline NormIO make_norm_io(const NormCfg &c, const NormSource &S, const NormOutput &O) {
    NormIO io = zeroed<NormIO>();
    io.D = c.D; io.block = c.block; io.eps = c.eps;
    io.state = c.state; io.a1 = c.part; io.a2 = c.part ? c.part + (size_t)c.max_blocks * (size_t)c.D : nullptr; io.cnt = c.cnt;
    io.mean = O.mean; io.inv = O.inv;
    io.src = S.ptr; io.rows = S.rows > 0 ? S.rows : 1; io.step_stride = S.step_stride; io.row_stride = S.row_stride;
    io.wrap = S.step_stride - (long long)(io.rows - 1) * S.row_stride;
    io.R = (long long)S.steps * S.rows; io.Rd = (double)io.R;
    io.blocks = (io.R + c.block - 1) / c.block;
    io.vec = rollout_aligned16(S.ptr) && (c.D & 3) == 0 && (S.step_stride & 3) == 0 && (S.row_stride & 3) == 0;
    io.groups = io.vec ? (c.D / 4 + WV_WAVE - 1) / WV_WAVE : (c.D + WV_WAVE - 1) / WV_WAVE;
    io.njobs = io.blocks * io.groups;
    return io;
}
/* a workgroup per job up to NORM_GRID, which then walk the jobs (launches 1 and 3); a wave per 64 columns (launches 2 and 4, the write) */
inline int norm_pass_grid(const NormIO &io) { return io.njobs < NORM_GRID ? (int)io.njobs : NORM_GRID; }
inline int norm_column_grid(const NormIO &io) { return (io.D + WV_WAVE - 1) / WV_WAVE; }
/* where a thing phys_batch_norm_download / _upload names lies: `rows` runs of `width` doubles, `pitch` doubles apart; false: no such
 * thing.  Uploads take the state's first five alone */
struct NormRegion { double *ptr; long long rows, width, pitch; };
inline bool norm_region(const NormCfg &c, int what, bool upload, NormRegion &R) {
    R = {};
    if (!c.on) return false;
    if (what >= NORM_N && what < (upload ? NORM_MB : NORM_PARTIALS)) {
        R.ptr = c.state ? c.state + (size_t)what * (size_t)c.D : nullptr; R.rows = 1; R.width = R.pitch = c.D; return true;
    }
    if (what == NORM_PARTIALS && !upload) { R.ptr = c.part; R.rows = 2; R.width = c.last_blocks * c.D; R.pitch = c.max_blocks * c.D; return true; }
    return false;
}
/* the eight statistics from the per-column arrays of the state (n, the last call's counts) and what the host knows of the last call */
inline void norm_stats_host(const NormCfg &c, const double *n, const double *counts, double *stats) {
    double updated = 0, skipped = 0, excluded = 0, nmax = 0;
    for (int j = 0; j < c.D; ++j) {
        if (c.calls > 0) { if (counts[j] > 0) { updated += 1; excluded += (double)c.last_R - counts[j]; } else skipped += 1; }
        if (n[j] > nmax) nmax = n[j];
    }
    stats[0] = (double)c.last_R; stats[1] = (double)c.last_blocks; stats[2] = updated; stats[3] = skipped; stats[4] = excluded;
    stats[5] = (double)c.calls; stats[6] = nmax; stats[7] = 0.0;
}

/* ---- the draw rows ---- */

/* the draws (phys_batch_draw_configure; on 0: not configured): the columns of a normal row (0: none), the shuffle's n (0: none), the
 * counter's offset and the key; the destinations the caller bound (dst null: the eps the policy's sample binding names, resolved at every
 * call; perm_dst null: the batch's own buffer).  Then what the launcher names once a kernel reads them: the envs' call counts and the
 * batch's permutation */
struct DrawCfg {
    int on, A;
    long long perm_n;
    unsigned env_base, key0, key1, pad;
    float *dst; long long sdst;
    int *perm_dst;
    unsigned *counts; int *perm;
};
/* the destination of a call of the normal rows as resolved */
struct DrawDst { float *ptr; long long stride; };
constexpr const char *DRAW_NOT_CONFIGURED = "not configured (phys_batch_draw_configure first)";
/* the draws' configuration: checks the caller's numbers and fills c but for what is bound or named later.  A 0 with perm_n 0 is accepted
 * and leaves c empty: the launcher releases what it holds.  The emulator goes through the same */
inline const char *draw_configure(int A, long long perm_n, unsigned long long seed, unsigned env_base, DrawCfg &c) {
    c = {};
    if (A == 0 && perm_n == 0) return nullptr;
    if (A < 0 || A > DRAW_MAXA) return "A lies in 1 .. 64 (0: no normal rows; 0 with perm_n 0 releases)";
    if (perm_n < 0 || perm_n > DRAW_MAXPERM) return "perm_n lies in 1 .. 2^30 (0: no shuffle)";
    c.on = 1; c.A = A; c.perm_n = perm_n; c.env_base = env_base; c.key0 = (unsigned)(seed & 0xffffffffull); c.key1 = (unsigned)(seed >> 32);
    return nullptr;
}
/* what phys_batch_draw_bind refuses (ptr null: back to the policy's eps) */
inline const char *check_draw_bind(const DrawCfg &c, const void *ptr, long long row_stride) {
    if (!c.on) return DRAW_NOT_CONFIGURED;
    if (c.A < 1) return "no normal rows are configured (A is 0)";
    if (ptr && row_stride < c.A) return "a row stride of at least A";
    return nullptr;
}
/* what phys_batch_draw_bind_perm refuses (ptr null: back to the batch's own buffer) */
inline const char *check_draw_bind_perm(const DrawCfg &c, const void *) {
    if (!c.on) return DRAW_NOT_CONFIGURED;
    if (c.perm_n < 1) return "no shuffle is configured (perm_n is 0)";
    return nullptr;
}
/* what a call of the normal rows refuses (D filled where it accepts): the destination is the caller's, or the eps tensor and stride that
 * phys_batch_policy_bind_sample names now */
inline const char *check_draw(const DrawCfg &c, const PolicyCfg &p, int nenv, int env0, int n, DrawDst &D) {
    D = {};
    if (!c.on || !c.counts) return DRAW_NOT_CONFIGURED;
    if (c.A < 1) return "no normal rows are configured (A is 0)";
    if (env0 < 0 || n < 0 || (long long)env0 + n > nenv) return "env range out of bounds";
    if (c.dst) { D.ptr = c.dst; D.stride = c.sdst; return nullptr; }
    if (p.nnets < 1 || !p.eps) return "no destination: nothing is bound and the policy has no sample bound (phys_batch_policy_bind_sample, or phys_batch_draw_bind)";
    if (p.net[0].layer[p.net[0].nlayers - 1].out != c.A) return "the actor's output width is not A";
    D.ptr = (float *)p.eps; D.stride = p.seps;
    return nullptr;
}
/* what a shuffle refuses */
inline const char *check_draw_perm(const DrawCfg &c) {
    if (!c.on) return DRAW_NOT_CONFIGURED;
    if (c.perm_n < 1) return "no shuffle is configured (perm_n is 0)";
    if (!c.perm_dst && !c.perm) return "no destination: nothing is bound and the batch holds no permutation";
    return nullptr;
}
/* cassie_draw_kernel's (after the check) */
inline DrawIO make_draw_io(const DrawCfg &c, const DrawDst &D, int env0, int n) {
    DrawIO io = zeroed<DrawIO>();
    io.env0 = env0; io.n = n; io.A = c.A;
    const int blocks = (c.A + 3) / 4;
    io.lanes = 1;
    while (io.lanes < blocks) io.lanes *= 2;
    io.per_wave = WV_WAVE / io.lanes;
    io.vec = rollout_aligned16(D.ptr) && (D.stride & 3) == 0;
    io.env_base = c.env_base; io.key0 = c.key0; io.key1 = c.key1;
    io.rows = D.ptr; io.srow = D.stride; io.counts = c.counts;
    return io;
}
/* the bits of a half of the shuffle's word: b = 2 h the smallest even number of bits with 2^b >= max(n, 4) */
inline unsigned draw_perm_half(long long n) {
    unsigned h = 1;
    while ((1ll << (2 * h)) < n) ++h;
    return h;
}
/* cassie_draw_perm_kernel's (after the check) */
inline DrawPermIO make_draw_perm_io(const DrawCfg &c, unsigned epoch) {
    DrawPermIO io = zeroed<DrawPermIO>();
    io.n = (unsigned)c.perm_n; io.h = draw_perm_half(c.perm_n); io.mask = (1u << io.h) - 1u;
    io.walk_max = (1ll << (2 * io.h)) - c.perm_n + 1;
    io.epoch = epoch; io.key0 = c.key0; io.key1 = c.key1;
    io.perm = c.perm_dst ? c.perm_dst : c.perm;
    return io;
}
/* a wave per 64 / lanes envs up to DRAW_GRID workgroups, a wave per 64 indices up to DRAW_PERM_GRID, which then walk */
inline int draw_grid(const DrawIO &io) { const int w = (io.n + io.per_wave - 1) / io.per_wave; return w < 1 ? 1 : (w < DRAW_GRID ? w : DRAW_GRID); }
inline int draw_perm_grid(const DrawPermIO &io) { const long long w = ((long long)io.n + WV_WAVE - 1) / WV_WAVE; return w < DRAW_PERM_GRID ? (int)w : DRAW_PERM_GRID; }

}  // namespace ck
#endif
