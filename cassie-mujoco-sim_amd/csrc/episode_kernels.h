/*
 * episode_kernels.h -- the kernels that end and restart episodes: the reset of chosen envs to one row (cassie_reset_kernel), episodes
 * that end and restart from each env's own state (cassie_episode_kernel), and the same with every restart PLACED on the env's own ground
 * (cassie_episode_place_kernel: the table of what a placement moves, its classifier for the host, the placement itself).  Included by
 * phys_batch.hip (which launches them) and by the CPU wave emulator; the launch records, grids and checks are small_launch.h's.
 */
#ifndef CASSIE_EPISODE_KERNELS_H
#define CASSIE_EPISODE_KERNELS_H

#include "surface_kernels.h"

namespace ck {

/* Episode restarts on the device (the batched form of what a fresh cassie_sim_t / cassie_sim_full_reset leaves, reference
 * src/cassiemujoco.c:1023-1029, :2008-2034): envs first, first + stride, ... (count of them) get qpos = qpos_row, zero
 * qvel / qacc_warmstart / ctrl / qacc / actuator_velocity / time, optionally sensordata = sens_row (what the first drive-level
 * pass of the new episode reads: the init pose's), a zero measurement block and zero drive-level state (encoder filter
 * histories, torque delay lines) -- one launch instead of a scatter per field.  The sticky warning word is left alone. */
struct ResetIO {
    int first, stride, count;
    int nq, nv, nu, nsd, sq, sqv, ssd;
    double *qpos, *qvel, *warm, *ctrl, *qacc, *time, *sens, *actvel, *meas;
    cm_drive_state_t *drive;    /* may be null */
    const double *qpos_row;     /* [nq] */
    const double *sens_row;     /* [nsensordata] or null: sensordata is left alone */
};
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_reset_kernel(ResetIO io) {
#ifndef CK_EMULATED
    /* a few workgroups walk all the envs: on a GPU saturated by another stream's step kernel every workgroup waits for a
     * wave slot to free, and one workgroup per env made this kernel a 0.5 ms stall of its stream (rocprofv3, two-range stepping) */
    const int lane = wv::lane();
    for (int i = (int)blockIdx.x; i < io.count; i += (int)gridDim.x) {
    const size_t env = (size_t)io.first + (size_t)i * io.stride;
    if (lane < io.nq) io.qpos[env * io.sq + lane] = io.qpos_row[lane];
    if (lane < io.nv) { io.qvel[env * io.sqv + lane] = 0.0; io.warm[env * io.nv + lane] = 0.0; io.qacc[env * io.nv + lane] = 0.0; }
    if (lane < io.nu) { io.ctrl[env * io.nu + lane] = 0.0; io.actvel[env * io.nu + lane] = 0.0; }
    if (io.sens_row && lane < io.nsd) io.sens[env * io.ssd + lane] = io.sens_row[lane];
    if (io.meas && lane < CM_MEAS_DIM) io.meas[env * CM_MEAS_DIM + lane] = 0.0;
    if (io.drive) {
        int *w = (int *)(io.drive + env);
        for (int k = lane; k < (int)(sizeof(cm_drive_state_t) / sizeof(int)); k += WV_WAVE) w[k] = 0;
    }
    if (lane == 0) io.time[env] = 0.0;
    }
#endif
}

/* Episodes that end and restart on the device from each env's own state (phys_batch_end_episodes, include/cassie_phys.h), one wave
 * per env: the lanes load the env's qpos / qvel entries; the non-finite test (the step kernel's own: NaN or |v| > 1e10) and the
 * height / tilt thresholds are combined with wv::ballot; lane 0 writes done / reason / steps / count; the envs that ended keep their
 * terminal state and -- with `restart` -- take a row of the bank of start states [qpos | qvel | sensordata | actuator_velocity | qacc]
 * (what upload + forward leave on a fresh batch), zero time / ctrl / warm start / measurement block / drive-level state and a clear
 * warning word.  The tilt expression is 1 - 2 (qx qx + qy qy) as written (it may contract to an fma on the device: thresholds are
 * not meant to be met to the last bit).
 * Like cassie_reset_kernel a few workgroups walk the range, for the reason given there: the launch runs behind a range's step launch
 * while the other range's step kernel fills the chip. */
constexpr int EPISODE_GRID = 32;
/* Placed restarts (phys_batch_place_configure, include/cassie_phys.h: "placed restarts"): what the launcher works out of the model once
 * and hands every launch through a table in device memory (the kernel walks it with run-time indices).  A moving root body (a child of the world with joints) takes a pose through a few qpos entries: the
 * addresses of its world x, y, z (a free joint's first three entries, or the three slides along the world's axes), of its quaternion
 * (the free joint's, or the ball's), and the dofs of its world x and y velocity.  A placed sensor is a framequat or a magnetometer. */
constexpr int PLACE_MAXROOTS = 4, PLACE_MAXSENSORS = 8, PLACE_MAXPOINTS = 1024;
/* (the table also carries what the kernel would otherwise fetch from the model field by field, in chains of dependent reads -- by
 * reasoning, not by measurement: the loop's rate was the same with and without it: a root's world position is qpos[q.] + o. (o = the
 * body's place minus the slides' references; 0 for a free joint), its world quaternion the normalised joint quaternion (the accepted
 * make-ups have the world's frame at qpos0); a sensor brings its site's quaternion and cutoff, the table the magnetic field) */
struct PlaceRoot { int body, qx, qy, qz, qq, vx, vy, pad; double ox, oy, oz; };
struct PlaceSensor { int type, adr, body, sensor, qq, pad; double squat[4], cutoff; };
struct PlaceTable { int nroot, nsensor, anchor_root, pad; double magnetic[3]; PlaceRoot root[PLACE_MAXROOTS]; PlaceSensor sensor[PLACE_MAXSENSORS]; };
struct EpisodeIO {
    int env0, n, restart, nrows;
    int nq, nv, nu, nsd, sq, sqv, ssd, row_dim;
    cm_episode_rules_t rules;
    double *qpos, *qvel, *warm, *ctrl, *qacc, *time, *sens, *actvel, *meas;   /* meas: null until a drive mode is in use */
    cm_drive_state_t *drive;    /* likewise */
    int *warn;
    int *done, *reason, *steps, *count;
    double *terminal;           /* [nenv][nq + nv] */
    const double *bank;         /* [nrows][row_dim], may be null when restart == 0 */
    const int *pick, *force;    /* [n] or null */
    /* placement (appended; all zero = none, and cassie_episode_kernel reads none of it): the anchor body (0: off), the footprint, the
     * roots and sensors a placement moves, the per-env arrays (indexed by the absolute env), and what the surface needs -- the shared
     * model, the envs' parameter blocks, the terrains and their index, which step 1 WRITES */
    int place_anchor, place_npoints;
    double place_ground_ref;
    const PlaceTable *place_table;
    const double *place_offsets;        /* [npoints][2] */
    const double *place_pose;           /* [nenv][4] dx, dy, dz, yaw */
    const int *place_next;              /* [nenv] or null */
    double *place_ground;               /* [nenv] */
    const cm_model_t *model;
    const cm_envparams_t *envparams;    /* null, or one block per env */
    const float *hfield; size_t hfield_stride; int *hfield_index; int hfield_nterrain;   /* as in PhysIO */
};

/* What a placement moves, from the (host's copy of the) shared model: fills the table, or returns what is wrong with the model (null: fine).  Host code: the launcher and the emulator's entry point share it. */
inline const char *place_classify(const cm_model_t &m, int anchor, PlaceTable &tab) {
    if (!m.kin_simple) return "the model's bodies are not slides followed by at most one rotational joint (kin_simple)";
    if (anchor <= 0 || anchor >= m.nbody || m.body_parentid[anchor] != 0) return "the anchor must be a child of the world";
    const int art = m.body_kin[anchor].rot_type;
    if (art != CM_JNT_BALL && art != CM_JNT_FREE && art != -1) return "the anchor's joints must be slides and at most a ball or free joint";
    tab.nroot = 0; tab.nsensor = 0; tab.anchor_root = -1;
    for (int k = 0; k < 3; ++k) tab.magnetic[k] = m.magnetic[k];
    for (int b = 1; b < m.nbody; ++b) {
        if (m.body_parentid[b] != 0 || m.body_jntnum[b] <= 0) continue;
        if (tab.nroot >= PLACE_MAXROOTS) return "more than four moving root bodies";
        const cm_kinrec_t &kr = m.body_kin[b];
        PlaceRoot r;
        r.body = b; r.pad = 0; r.ox = r.oy = r.oz = 0.0;
        if (kr.rot_type == CM_JNT_FREE && kr.nslide == 0) {
            const int da = m.jnt_dofadr[kr.rot_jnt];
            r.qx = kr.rot_qadr; r.qy = r.qx + 1; r.qz = r.qx + 2; r.qq = r.qx + 3; r.vx = da; r.vy = da + 1;
        } else if (kr.rot_type == CM_JNT_BALL && kr.nslide == 3) {
            /* the three slides along the world's x, y and z, one each; the ball at the body's origin, the body frame the world's at
             * qpos0: the body's world pose is then (slides, ball quaternion) and any pose can be written back */
            int q[3] = {-1, -1, -1}, v[3] = {-1, -1, -1};
            for (int sl = 0; sl < 3; ++sl) {
                const double *ax = kr.slide_axis_p[sl];
                const int k = ax[0] == 1.0 && ax[1] == 0.0 && ax[2] == 0.0 ? 0 : ax[0] == 0.0 && ax[1] == 1.0 && ax[2] == 0.0 ? 1
                            : ax[0] == 0.0 && ax[1] == 0.0 && ax[2] == 1.0 ? 2 : -1;
                if (k < 0 || q[k] >= 0) return "a moving root's slides must run along the world's x, y and z, one each";
                q[k] = kr.slide_qadr[sl]; v[k] = m.jnt_dofadr[kr.jnt0 + sl];
            }
            for (int k = 0; k < 3; ++k)
                if (kr.rot_pos[k] != 0.0 || kr.rot_pos_p[k] != 0.0) return "a moving root's ball joint must sit at the body's origin";
            if (kr.quat[0] != 1.0 || kr.quat[1] != 0.0 || kr.quat[2] != 0.0 || kr.quat[3] != 0.0) return "a moving root with a ball joint must have the world's orientation at qpos0";
            r.qx = q[0]; r.qy = q[1]; r.qz = q[2]; r.qq = kr.rot_qadr; r.vx = v[0]; r.vy = v[1];
            double o[3] = {kr.pos[0], kr.pos[1], kr.pos[2]};
            for (int sl = 0; sl < 3; ++sl) for (int k = 0; k < 3; ++k) if (q[k] == kr.slide_qadr[sl]) o[k] -= kr.slide_ref[sl];
            r.ox = o[0]; r.oy = o[1]; r.oz = o[2];
        } else return "a moving root body must have a free joint, or three slides along the world's axes and a ball";
        if (b == anchor) tab.anchor_root = tab.nroot;
        tab.root[tab.nroot++] = r;
    }
    for (int s = 0; s < m.nsensor; ++s) {
        const int t = m.sensor_type[s];
        if (t != CM_SENS_FRAMEQUAT && t != CM_SENS_MAGNETOMETER) continue;
        const int sb = m.sensor_body[s];
        if (sb <= 0 || sb >= m.nbody || m.body_parentid[sb] != 0 || m.body_jntnum[sb] <= 0) return "a framequat or magnetometer sensor sits on a body that is not a moving root";
        if (tab.nsensor >= PLACE_MAXSENSORS) return "more than eight framequat / magnetometer sensors";
        PlaceSensor ps;
        ps.type = t; ps.adr = m.sensor_adr[s]; ps.body = sb; ps.sensor = s; ps.pad = 0; ps.qq = 0;
        for (int r = 0; r < tab.nroot; ++r) if (tab.root[r].body == sb) ps.qq = tab.root[r].qq;
        for (int k = 0; k < 4; ++k) ps.squat[k] = m.sensor_squat[s][k];
        ps.cutoff = m.sensor_cutoff[s];
        tab.sensor[tab.nsensor++] = ps;
    }
    return nullptr;
}

/* Steps 1 to 3 of a placed restart for one env, by the whole wave (everything wave-uniform but the footprint points, which the lanes
 * share out): the terrain, the anchor's position in the row, the ground G under the placed footprint.  Returns the warning bits. */
struct Placement { double dx, dy, h, c1, s, ch, sh, yaw, ax, ay; };
WV_DEVICE int place_ground(const EpisodeIO &io, ModelPtr m, size_t env, const double *rowq, int lane, Placement &P) {
    const double *pose = io.place_pose + env * 4;
    const double dz = pose[2], yaw = pose[3];
    /* (the turn as Rz(yaw) - I and the half-angle quaternion: a yaw of 0 gives c1 = s = sh = 0 and ch = 1 exactly, so that the pose
     * (0, 0, 0, 0) adds exact zeros below) */
    const double c = cos(yaw), s = sin(yaw);
    P.dx = pose[0]; P.dy = pose[1]; P.yaw = yaw; P.c1 = c - 1.0; P.s = s; P.ch = cos(0.5 * yaw); P.sh = sin(0.5 * yaw);
    int warn = 0;
    const float *grid = nullptr;
    if (io.place_next && io.hfield_index) {
        const int want = io.place_next[env], last = io.hfield_nterrain - 1;
        const int t = want > last ? last : (want < 0 ? 0 : want);
        if (t != want) warn |= WARN_TERRAIN_INDEX;
        if (lane == 0) io.hfield_index[env] = t;
        if (io.hfield) grid = io.hfield + (size_t)t * io.hfield_stride;
    } else if (io.place_npoints > 0) {
        bool clamped;
        grid = terrain_grid(io.hfield, io.hfield_stride, io.hfield_index, io.hfield_nterrain, (int)env, &clamped);
        if (clamped) warn |= WARN_TERRAIN_INDEX;
    }
    double ap[3], aq[4];
    const int ar = io.place_table->anchor_root;
    if (ar >= 0) {                       /* the anchor is one of the moving roots (the pelvis): its pose as place_qpos takes it */
        const PlaceRoot A = io.place_table->root[ar];
        ap[0] = rowq[A.qx] + A.ox; ap[1] = rowq[A.qy] + A.oy; ap[2] = rowq[A.qz] + A.oz;
        for (int k = 0; k < 4; ++k) aq[k] = rowq[A.qq + k];
        normalize4(aq);
    } else static_body_pose(m, io.place_anchor, rowq, ap, aq);
    P.ax = ap[0]; P.ay = ap[1];
    double G = io.place_ground_ref;
    if (io.place_npoints > 0) {
        const ParamPtr PG = env_geometry(io.envparams, m, env);
        /* the heading of the anchor as the scan takes it, turned on by yaw */
        double cy, sy;
        quat_heading(aq, cy, sy);
        const double hc = cy * c - sy * s, hs = sy * c + cy * s;
        const double bx = ap[0] + P.dx, by = ap[1] + P.dy;
        bool any = false;
        double best = -1e300;
        for (int j0 = 0; j0 < io.place_npoints; j0 += WV_WAVE) {
            const int j = j0 + lane;
            const bool mine = j < io.place_npoints;
            const double ox = mine ? io.place_offsets[2 * j] : 0.0, oy = mine ? io.place_offsets[2 * j + 1] : 0.0;
            const double X = bx + (hc * ox - hs * oy), Y = by + (hs * ox + hc * oy);
            double top;
            const bool hit = scan_surface(m, PG, grid, X, Y, &top, &warn);
            if (mine && hit && (!any || top > best)) { any = true; best = top; }
        }
        if (!any) best = -1e300;
        for (int mask = WV_WAVE / 2; mask; mask >>= 1) { const double o = wv::shfl_xor(best, mask); best = o > best ? o : best; }
        if (wv::ballot(any) != 0ull) G = best;
        else warn |= WARN_PLACE_MISS;
    }
    if (lane == 0) io.place_ground[env] = G;
    P.h = dz + G - io.place_ground_ref;
    return warn;
}
/* Steps 4 to 6: entry k of the row's qpos / of its qvel or qacc (src: that block of the row) / of its sensordata as the placed env
 * holds it -- the row's own value unless the entry belongs to a moving root's pose, to its linear velocity, to a framequat or to a
 * magnetometer.  Wave-uniform but for k. */
WV_DEVICE double place_qpos(const EpisodeIO &io, const Placement &P, const double *rowq, int k) {
    double v = rowq[k];
    for (int r = 0; r < io.place_table->nroot; ++r) {
        const PlaceRoot R = io.place_table->root[r];
        const double rx = (rowq[R.qx] + R.ox) - P.ax, ry = (rowq[R.qy] + R.oy) - P.ay;
        const double tx = P.dx + (P.c1 * rx - P.s * ry), ty = P.dy + (P.s * rx + P.c1 * ry);
        const double w = rowq[R.qq], x = rowq[R.qq + 1], y = rowq[R.qq + 2], z = rowq[R.qq + 3];
        if (k == R.qx) v += tx;
        else if (k == R.qy) v += ty;
        else if (k == R.qz) v += P.h;
        else if (k == R.qq) v = P.ch * w - P.sh * z;
        else if (k == R.qq + 1) v = P.ch * x - P.sh * y;
        else if (k == R.qq + 2) v = P.ch * y + P.sh * x;
        else if (k == R.qq + 3) v = P.ch * z + P.sh * w;
    }
    return v;
}
WV_DEVICE double place_qvel(const EpisodeIO &io, const Placement &P, const double *src, int k) {
    double v = src[k];
    for (int r = 0; r < io.place_table->nroot; ++r) {
        const PlaceRoot R = io.place_table->root[r];
        const double vx = src[R.vx], vy = src[R.vy];
        if (k == R.vx) v += P.c1 * vx - P.s * vy;
        else if (k == R.vy) v += P.s * vx + P.c1 * vy;
    }
    return v;
}
WV_DEVICE double place_sens(const EpisodeIO &io, const Placement &P, const double *rowq, const double *src, int k) {
    double v = src[k];
    for (int i = 0; i < io.place_table->nsensor; ++i) {
        const PlaceSensor S = io.place_table->sensor[i];
        if (S.type == CM_SENS_FRAMEQUAT) {
            const double w = src[S.adr], x = src[S.adr + 1], y = src[S.adr + 2], z = src[S.adr + 3];
            if (k == S.adr) v = P.ch * w - P.sh * z;
            else if (k == S.adr + 1) v = P.ch * x - P.sh * y;
            else if (k == S.adr + 2) v = P.ch * y + P.sh * x;
            else if (k == S.adr + 3) v = P.ch * z + P.sh * w;
        } else if (P.yaw != 0.0) {   /* (a yaw of exactly 0 turns no frame: the magnetometer keeps the row's words) */
            double bq[4] = {rowq[S.qq], rowq[S.qq + 1], rowq[S.qq + 2], rowq[S.qq + 3]}, t[4], q[4], R[9], out[3];
            normalize4(bq);
            const double sq[4] = {S.squat[0], S.squat[1], S.squat[2], S.squat[3]};
            const double qz[4] = {P.ch, 0.0, 0.0, P.sh}, mg[3] = {io.place_table->magnetic[0], io.place_table->magnetic[1], io.place_table->magnetic[2]};
            mulquat(t, bq, sq);
            mulquat(q, qz, t);
            quat2mat(R, q);
            mulmatTvec3(out, R, mg);
            const double cut = S.cutoff;
            for (int c = 0; c < 3; ++c)
                if (k == S.adr + c) v = cut > 0 ? clampd(out[c], -cut, cut) : out[c];
        }
    }
    return v;
}

template <bool PLACED>
WV_DEVICE void episode_walk(const EpisodeIO &io) {
    const int lane = wv::lane();
    const cm_episode_rules_t &R = io.rules;
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) {
        const size_t env = (size_t)io.env0 + (size_t)i;
        const double qp = lane < io.nq ? io.qpos[env * io.sq + lane] : 0.0;
        const double qv = lane < io.nv ? io.qvel[env * io.sqv + lane] : 0.0;
        const int warn = io.warn[env], steps = io.steps[env] + 1;
        const int forced = io.force ? io.force[i] : 0, picked = io.pick ? io.pick[i] : 0;
        int count = io.count[env];
        const bool bad = (lane < io.nq && (!(qp == qp) || fabs(qp) > 1e10)) || (lane < io.nv && (!(qv == qv) || fabs(qv) > 1e10));
        const double qx = wv::shfl(qp, 4), qy = wv::shfl(qp, 5);
        const double upright = 1.0 - 2.0 * (qx * qx + qy * qy);
        int reason = 0;
        if (wv::ballot(lane == 2 && qp < R.min_height) != 0ull) reason |= CM_DONE_HEIGHT;
        if (wv::ballot(upright < R.min_upright) != 0ull) reason |= CM_DONE_UPRIGHT;
        if (R.max_steps > 0 && steps >= R.max_steps) reason |= CM_DONE_TIME;
        if (((unsigned)warn & R.warn_mask) != 0u) reason |= CM_DONE_WARN;
        if (wv::ballot(bad) != 0ull && R.nonfinite) reason |= CM_DONE_NONFINITE;
        if (forced) reason |= CM_DONE_FORCED;
        const bool done = reason != 0, restart = done && io.restart;
        if (done) {
            ++count;
            double *t = io.terminal + env * (size_t)(io.nq + io.nv);
            if (lane < io.nq) t[lane] = qp;
            if (lane < io.nv) t[io.nq + lane] = qv;
        }
        if (lane == 0) {
            io.done[env] = done ? 1 : 0; io.reason[env] = reason; io.steps[env] = restart ? 0 : steps;
            if (done) io.count[env] = count;
        }
        if (restart) {
            int r = io.pick ? picked % io.nrows : (int)((env + (size_t)count) % (size_t)io.nrows);
            if (r < 0) r += io.nrows;
            const double *row = io.bank + (size_t)r * io.row_dim;
            int newwarn = 0;
            if constexpr (PLACED) {
                const ModelPtr m = (ModelPtr)io.model;
                const double *rowq = row, *rowv = row + io.nq, *rows = rowv + io.nv, *rowa = rows + io.nsd + io.nu;
                Placement P;
                newwarn = place_ground(io, m, env, rowq, lane, P);
                for (int k = lane; k < io.nq; k += WV_WAVE) io.qpos[env * io.sq + k] = place_qpos(io, P, rowq, k);
                for (int k = lane; k < io.nv; k += WV_WAVE) {
                    io.qvel[env * io.sqv + k] = place_qvel(io, P, rowv, k);
                    io.qacc[env * io.nv + k] = place_qvel(io, P, rowa, k);
                    io.warm[env * io.nv + k] = 0.0;
                }
                for (int k = lane; k < io.nsd; k += WV_WAVE) io.sens[env * io.ssd + k] = place_sens(io, P, rowq, rows, k);
                row = rows + io.nsd;
                for (int k = lane; k < io.nu; k += WV_WAVE) { io.actvel[env * io.nu + k] = row[k]; io.ctrl[env * io.nu + k] = 0.0; }
            } else {
                for (int k = lane; k < io.nq; k += WV_WAVE) io.qpos[env * io.sq + k] = row[k];
                row += io.nq;
                for (int k = lane; k < io.nv; k += WV_WAVE) { io.qvel[env * io.sqv + k] = row[k]; io.warm[env * io.nv + k] = 0.0; }
                row += io.nv;
                for (int k = lane; k < io.nsd; k += WV_WAVE) io.sens[env * io.ssd + k] = row[k];
                row += io.nsd;
                for (int k = lane; k < io.nu; k += WV_WAVE) { io.actvel[env * io.nu + k] = row[k]; io.ctrl[env * io.nu + k] = 0.0; }
                row += io.nu;
                for (int k = lane; k < io.nv; k += WV_WAVE) io.qacc[env * io.nv + k] = row[k];
            }
            if (io.meas) for (int k = lane; k < CM_MEAS_DIM; k += WV_WAVE) io.meas[env * CM_MEAS_DIM + k] = 0.0;
            if (io.drive) {
                int *w = (int *)(io.drive + env);
                for (int k = lane; k < (int)(sizeof(cm_drive_state_t) / sizeof(int)); k += WV_WAVE) w[k] = 0;
            }
            if (lane == 0) { io.time[env] = 0.0; io.warn[env] = newwarn; }
        }
    }
}
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_episode_kernel(EpisodeIO io) { episode_walk<false>(io); }
/* The same with every restart PLACED (EpisodeIO::place_*; the launcher picks this kernel once phys_batch_place_configure has named an
 * anchor): still one launch per call, on the same grid -- what a placement adds runs for the envs that restart only, a few per launch. */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_episode_place_kernel(EpisodeIO io) { episode_walk<true>(io); }

}  // namespace ck
#endif
