/*
 * small_kernels.h -- the kernels around the step kernel (physics_kernel.h): the longest-job-first launch order, the
 * drive-level pass on its own, the batched derived getters.  Included by phys_batch.hip (which launches them) and by the
 * CPU wave emulator; the step kernel's own translation units (kernels_*.hip) do not need them.
 */
#ifndef CASSIE_SMALL_KERNELS_H
#define CASSIE_SMALL_KERNELS_H

#include "physics_kernel.h"

namespace ck {

/* Longest-job-first launch order.  A launch is nenv independent jobs (one env x nsub substeps each) handed to the
 * chip's wave slots in workgroup order; with only a few jobs per slot -- 4096 envs on 1024 SIMDs -- the launch ends
 * when the unluckiest slot does, measured ~15 % after the average one.  An env's cost persists from launch to launch
 * (it is its contact situation), so the next launch starts the expensive envs first and lets the cheap ones fill the
 * tail.  One workgroup: counting sort of the envs by the cost of their last launch into NBIN bins, descending; the
 * order inside a bin is arbitrary, which is harmless -- envs are independent and every env is stepped exactly once. */
/* one wave: on a GPU saturated by another stream's step kernel (whose workgroups hold every register of their SIMD and all
 * but 0.8 KB of a CU's LDS) a workgroup is dispatched only when a wave slot frees, and a 1024-thread workgroup only when a
 * whole CU does -- which, measured, took milliseconds and stalled the launching stream (round 3, two-stream stepping) */
constexpr int ORDER_THREADS = 64, ORDER_NBIN = 256;
WV_GLOBAL void __launch_bounds__(ORDER_THREADS) cassie_order_kernel(const unsigned *cost, int *order, int nenv, int base, int *inplace_count, volatile int *inplace_seen) {
    /* sorts the env range [base, base + nenv): cost / order are indexed by the absolute env, the order entries are absolute */
    cost += base; order += base;
#ifndef CK_EMULATED
    /* (round 6: the kernel that runs behind the stepping launches of a range also reports, through host memory, how many env-launches
     * of the in-place fast kernel finished a substep in place since the last report -- or, negated, how many reports in a row had none:
     * the launcher picks the range's next form by it.  The run length is counted HERE, in stream order: the launcher may be hundreds
     * of launches ahead of the device and would count the same stale word again and again) */
    if (inplace_count && threadIdx.x == 0) {
        const int c = inplace_count[0], quiet = c > 0 ? 0 : inplace_count[1] + 1;
        inplace_count[0] = 0; inplace_count[1] = quiet;
        *inplace_seen = c > 0 ? c : -quiet;
    }
    __shared__ unsigned lo_s, hi_s, count[ORDER_NBIN], start[ORDER_NBIN];
    const int t = threadIdx.x;
    if (t == 0) { lo_s = 0xffffffffu; hi_s = 0; }
    for (int b = t; b < ORDER_NBIN; b += ORDER_THREADS) count[b] = 0;
    __syncthreads();
    unsigned lo = 0xffffffffu, hi = 0;
    for (int e = t; e < nenv; e += ORDER_THREADS) { const unsigned c = cost[e]; lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
    atomicMin(&lo_s, lo); atomicMax(&hi_s, hi);
    __syncthreads();
    lo = lo_s; hi = hi_s;
    const float scale = hi > lo ? (float)(ORDER_NBIN - 1) / (float)(hi - lo) : 0.0f;
    auto bin_of = [&](unsigned c) { return ORDER_NBIN - 1 - (int)((float)(c - lo) * scale); }; /* bin 0 = most expensive */
    for (int e = t; e < nenv; e += ORDER_THREADS) atomicAdd(&count[bin_of(cost[e])], 1u);
    __syncthreads();
    if (t == 0) { unsigned acc = 0; for (int b = 0; b < ORDER_NBIN; ++b) { start[b] = acc; acc += count[b]; } }
    __syncthreads();
    for (int e = t; e < nenv; e += ORDER_THREADS) order[atomicAdd(&start[bin_of(cost[e])], 1u)] = base + e;
#endif
}

/* The drive-level pass on its own, one wave per env: cassie_motor_data + cassie_sensor_data for every env on the
 * sensordata / actuator_velocity the last physics step left in HBM; writes ctrl (for the next physics launch), the
 * measurement block and the drive state.  The batched host API launches it ahead of the physics kernel so that the
 * measurements reach the host -- and the state estimators start -- while the physics is still running. */
struct DriveShared {
    double sens[CM_MAXSENSORDATA], actvel[CM_MAXU], ctrl[CM_MAXU];
    int drv_x[CM_NUM_DRIVES][CM_DRIVE_FILTER_NB];
    double drv_jx[CM_NUM_JOINTS][CM_JOINT_FILTER_NB], drv_jy[CM_NUM_JOINTS][CM_JOINT_FILTER_NA];
    double drv_delay[CM_NUM_DRIVES][CM_TORQUE_DELAY_CYCLES];
    double drv_pos[CM_NUM_DRIVES], drv_vel[CM_NUM_DRIVES];
    double drv_c[CM_NUM_DRIVES][10], drv_jc[CM_NUM_JOINTS][2];
    int drv_msg[2];
};

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_drive_kernel(PhysIO io, double *ctrl_out) {
    WV_SHARED DriveShared S;
    const int env = wv::env_id();
    if (env >= io.nenv) return;
    const ModelPtr m = (ModelPtr)(io.models + (size_t)env * io.model_stride);
    const int lane = wv::lane(), nu = m->nu;
    if (lane < m->nsensordata) S.sens[lane] = io.sensordata[(size_t)env * io.ssd + lane];
    if (lane < nu) S.actvel[lane] = io.actuator_velocity[(size_t)env * io.su + lane];
    drive_state_load(io, S, env, lane);
    drive_consts_load(io, S, m, env, lane);
    wv::sync();
    drive_level_io(io, S, m, env, lane, true);
    wv::sync();
    drive_state_store(io, S, env, lane);
    if (lane < nu) ctrl_out[(size_t)env * io.su + lane] = S.ctrl[lane];
}

/* ------------------------------------------------ derived getters, batched ---- */
/* What the reference's reward-side getters compute from mjData, for one env from the read-out (cm_ext_t) a forward
 * pass left in HBM: whole-model centre of mass, its velocity, angular momentum about it (reference
 * src/cassiemujoco.c:1632-1700), foot positions / velocities (:1604-1630, :1752-1770), foot and heel / toe contact
 * forces (:1812-1898), the feet's Jacobians (:1254-1301) and the dense mass matrix (:1702-1712).  Same arithmetic as
 * the single-simulator getters in csrc/cassiemujoco.c.  ids: left / right foot body, left / right heel site, left /
 * right toe site (-1 = the model has none). */
struct DeriveIO {
    const cm_model_t *models; int model_stride; int nenv;
    const cm_envparams_t *envparams; /* null, or one block per env (PhysIO::envparams) */
    const cm_ext_t *ext;
    const double *xpos, *xquat;   /* [nenv][nbody][3], [nenv][nbody][4] */
    double *derived;              /* [nenv][CM_DRV_DIM] */
    double *qM;                   /* [nenv][nv][nv] or null */
    int ids[6];
};

WV_DEVICE void derive_env(const DeriveIO &io, int env, int lane) {
    const ModelPtr m = (ModelPtr)(io.models + (size_t)env * io.model_stride);
    const ParamPtr P = io.envparams ? (ParamPtr)(io.envparams + (size_t)env) : (ParamPtr)&m->params;
    const cm_ext_t *ex = io.ext + env;
    const int nb = m->nbody, nv = m->nv;
    double *out = io.derived + (size_t)env * CM_DRV_DIM;
    const double *xpos = io.xpos + (size_t)env * nb * 3, *xquat = io.xquat + (size_t)env * nb * 4;
    /* lane = body: mass-weighted sums */
    const bool isb = lane > 0 && lane < nb;
    const int b = isb ? lane : 0;
    const double mb = isb ? P->body_mass[b] : 0.0;
    double xi[3], vb[3] = {0, 0, 0}, w[3] = {0, 0, 0};
    for (int i = 0; i < 3; ++i) xi[i] = ex->xipos[b][i];
    if (isb) {
        const double *cv = ex->cvel[b], *rc = ex->subtree_com[m->body_rootid[b]];
        double off[3] = {xi[0] - rc[0], xi[1] - rc[1], xi[2] - rc[2]}, t[3];
        for (int i = 0; i < 3; ++i) w[i] = cv[i];
        cross3(t, w, off);
        for (int i = 0; i < 3; ++i) vb[i] = cv[3 + i] + t[i];
    }
    const double M = wv::wave_sum(mb), Mi = M > 0 ? 1.0 / M : 0.0;
    double com[3], vcom[3];
    for (int i = 0; i < 3; ++i) { com[i] = wv::wave_sum(mb * xi[i]) * Mi; vcom[i] = wv::wave_sum(mb * vb[i]) * Mi; }
    /* angular momentum about the whole-model com: spin R diag(I) R^T w + orbital r x m (v - vcom) */
    double L[3] = {0, 0, 0};
    if (isb) {
        double q[4], R[9], iq[4] = {m->body_iquat[b][0], m->body_iquat[b][1], m->body_iquat[b][2], m->body_iquat[b][3]};
        double xq[4] = {xquat[4 * b], xquat[4 * b + 1], xquat[4 * b + 2], xquat[4 * b + 3]};
        mulquat(q, xq, iq);
        quat2mat(R, q);
        double wl[3];
        mulmatTvec3(wl, R, w);
        for (int i = 0; i < 3; ++i) wl[i] *= P->body_inertia[b][i];
        mulmatvec3(L, R, wl);
        double r[3], mv[3], t[3];
        for (int i = 0; i < 3; ++i) { r[i] = xi[i] - com[i]; mv[i] = mb * (vb[i] - vcom[i]); }
        cross3(t, r, mv);
        for (int i = 0; i < 3; ++i) L[i] += t[i];
    }
    for (int i = 0; i < 3; ++i) L[i] = wv::wave_sum(L[i]);
    if (lane == 0) {
        for (int i = 0; i < 3; ++i) { out[CM_DRV_COM_POS + i] = com[i]; out[CM_DRV_COM_VEL + i] = vcom[i]; out[CM_DRV_ANGMOM + i] = L[i]; }
        out[CM_DRV_MASS] = M;
    }
    /* lane = side: foot kinematics and contact forces */
    if (lane < 2) {
        const int side = lane, foot = io.ids[side], heel = io.ids[2 + side], toe = io.ids[4 + side];
        const double off = sqrt(0.01762 * 0.01762 + 0.05219 * 0.05219); /* foot joint to mid-foot (reference :1612) */
        for (int i = 0; i < 3; ++i) out[CM_DRV_FOOT_POS + 3 * side + i] = (foot > 0 ? xpos[3 * foot + i] : 0.0) - (i == 2 ? off : 0.0);
        for (int i = 0; i < 6; ++i) out[CM_DRV_FOOT_VEL + 6 * side + i] = foot > 0 ? ex->cvel[foot][i] : 0.0;
        double ff[3] = {0, 0, 0}, tf[3] = {0, 0, 0}, hf[3] = {0, 0, 0};
        for (int c = 0; c < ex->ncon; ++c) {
            const int b1 = ex->con_body1[c], b2 = ex->con_body2[c];
            if (b1 != foot && b2 != foot) continue;
            const double *fr = ex->con_frame[c], *f = ex->con_force[c];
            const double sgn = (b1 == foot) ? -1.0 : 1.0;
            double fw[3];
            for (int k = 0; k < 3; ++k) fw[k] = fr[k] * f[0] + fr[3 + k] * f[1] + fr[6 + k] * f[2];
            for (int k = 0; k < 3; ++k) ff[k] += sgn * fw[k];
            if (heel >= 0 && toe >= 0 && heel < CM_MAXSITE && toe < CM_MAXSITE) {
                const double *p = ex->con_pos[c], *tp = ex->site_xpos[toe], *hp = ex->site_xpos[heel];
                const double td = sqrt((tp[0] - p[0]) * (tp[0] - p[0]) + (tp[1] - p[1]) * (tp[1] - p[1]));
                const double hd = sqrt((hp[0] - p[0]) * (hp[0] - p[0]) + (hp[1] - p[1]) * (hp[1] - p[1]));
                double *dst = td < hd ? tf : hf;
                for (int k = 0; k < 3; ++k) dst[k] += sgn * fw[k];
            }
        }
        for (int k = 0; k < 3; ++k) {
            out[CM_DRV_FOOT_FORCE + 6 * side + k] = ff[k]; out[CM_DRV_FOOT_FORCE + 6 * side + 3 + k] = 0.0;
            out[CM_DRV_TOE_FORCE + 3 * side + k] = tf[k]; out[CM_DRV_HEEL_FORCE + 3 * side + k] = hf[k];
        }
    }
    /* lane = dof: Jacobian columns of the two foot origins, and this dof's column of the mass matrix */
    if (lane < CM_MAXV) {
        const int k = lane;
        for (int side = 0; side < 2; ++side) {
            const int foot = io.ids[side];
            double jp[3] = {0, 0, 0}, jr[3] = {0, 0, 0};
            if (k < nv && foot > 0 && ((m->body_dofmask[foot] >> k) & 1ull)) {
                const double *cm = ex->subtree_com[m->body_rootid[foot]];
                double off[3] = {xpos[3 * foot] - cm[0], xpos[3 * foot + 1] - cm[1], xpos[3 * foot + 2] - cm[2]}, t[3];
                double cd[6];
                for (int i = 0; i < 6; ++i) cd[i] = ex->cdof[k][i];
                cross3(t, cd, off);
                for (int i = 0; i < 3; ++i) { jp[i] = cd[3 + i] + t[i]; jr[i] = cd[i]; }
            }
            for (int i = 0; i < 3; ++i) {
                out[CM_DRV_FOOT_JACP + (side * 3 + i) * CM_MAXV + k] = jp[i];
                out[CM_DRV_FOOT_JACR + (side * 3 + i) * CM_MAXV + k] = jr[i];
            }
        }
        if (io.qM && k < nv) {
            double *Mo = io.qM + (size_t)env * nv * nv;
            for (int i = 0; i < nv; ++i) Mo[(size_t)i * nv + k] = ex->qM[i][k];
        }
    }
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_derive_kernel(DeriveIO io) {
    const int env = wv::env_id();
    if (env >= io.nenv) return;
    derive_env(io, env, wv::lane());
}

/* ------------------------------------------- per-env physical parameters ---- */
/* phys_batch_randomize: rows [n][dim] of one input array of cm_envparams_t (cm_model.h: CM_P_*) into the blocks of envs
 * env0 .. env0 + n - 1.  off = the array's offset in the block in doubles.  A few workgroups walk the rows. */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_param_scatter_kernel(cm_envparams_t *params, int off, int dim, const double *src, int env0, int n) {
#ifndef CK_EMULATED
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
        double *dst = (double *)(params + env0 + i) + off;
        for (int k = (int)threadIdx.x; k < dim; k += WV_WAVE) dst[k] = src[(size_t)i * dim + k];
    }
#endif
}

/* The mj_setConst role on the device (reference src/cassiemujoco.c:952, :976 after the mass / inertial-offset setters of
 * :1367-1412), one wave per env: from the env's masses, inertial offsets and principal inertias and the model's kinematics at
 * qpos0 (cm_model_t::body_xpos0 ...: no randomised parameter moves a body frame) it builds the dense joint-space inertia at qpos0,
 * its Cholesky factor, and from it the mean inertia, the bodies' translational / rotational inverse weights
 * (1/3 tr J M^-1 J^T at the inertial origin) and the dofs' (diag M^-1, averaged over ball / free joints); then the values the
 * constraint stages read per joint limit / equality / contact pair, and the pairs' mixed friction.
 *
 * Every floating-point operation is an individually rounded IEEE operation in the order of HostModel::set_const /
 * HostModel::compile (csrc/mjcf_loader.cpp), so an env's block is BIT FOR BIT what compiling a host model with the same
 * parameters gives (tests/test_domain_randomisation.py on the emulator, tests/test_randomise_gpu.py on the device) -- the
 * oracle, which is handed such per-env models, and the kernel then solve the same problem.
 * Lanes: dofs (Jacobian columns, columns of M, rows of the factor), then (body, translational | rotational) for the bodies'
 * solves, then dofs again for the unit-vector solves; the right-hand sides live one to a lane in LDS. */
struct SetConstShared {
    double M[CM_MAXV][CM_MAXV + 1];
    double Jp[3][CM_MAXV], Jl[3][CM_MAXV];
    double X[WV_WAVE][CM_MAXV + 1], X0[WV_WAVE][CM_MAXV + 1];
    double xipos[CM_MAXBODY][3];
    double bw[CM_MAXBODY][2], dinv[CM_MAXV], dw[CM_MAXV];
    double piv;
    int ok;
    double glen[CM_MAXGEOM];      /* geometry: each collision geom's distance bound from its tree's root body */
};
/* what a launch of the set_const kernel re-derives (SetConstIO::derive_inertial) */
enum { SETCONST_FRICTION = 0,     /* the pairs' mixed friction (phys_batch_randomize of CM_P_GEOM_FRICTION) */
       SETCONST_ALL = 1,          /* everything: inverse weights, mean inertia, the pair tables, geometry and springs (phys_batch_set_const) */
       SETCONST_GEOMETRY = 2,     /* geom_mat and body_reach only (CM_P_GEOM_POS / CM_P_GEOM_QUAT) */
       SETCONST_SPRINGS = 3 };    /* dof_stiffness and dof_springref only (CM_P_JNT_STIFFNESS / CM_P_QPOS_SPRING) */
struct SetConstIO {
    const cm_model_t *model;      /* the shared model (topology, kinematics at qpos0, armature, pair / equality tables) */
    cm_envparams_t *params;       /* [nenv] blocks, indexed by the absolute env */
    int env0, nenv;               /* the range to (re)derive */
    int derive_inertial;          /* a SETCONST_* value (0 and 1 as before the geometry / spring modes existed) */
};

/* Jacobian column of dof d for a world point p attached to body b (HostKin::jac): translational part jp, rotational jr */
WV_DEVICE void setconst_jac_col(ModelPtr m, int b, int d, const double *p, double (&jp)[3], double (&jr)[3]) {
    for (int i = 0; i < 3; ++i) { jp[i] = 0.0; jr[i] = 0.0; }
    if (!((m->body_dofmask[b] >> d) & 1ull)) return;
    double ax[3] = {m->dof_axis0[d][0], m->dof_axis0[d][1], m->dof_axis0[d][2]};
    if (m->dof_trans0[d]) { for (int i = 0; i < 3; ++i) jp[i] = ax[i]; return; }
    const double off[3] = {wv::sub_rn(p[0], m->dof_anchor0[d][0]), wv::sub_rn(p[1], m->dof_anchor0[d][1]), wv::sub_rn(p[2], m->dof_anchor0[d][2])};
    jp[0] = wv::sub_rn(wv::mul_rn(ax[1], off[2]), wv::mul_rn(ax[2], off[1]));
    jp[1] = wv::sub_rn(wv::mul_rn(ax[2], off[0]), wv::mul_rn(ax[0], off[2]));
    jp[2] = wv::sub_rn(wv::mul_rn(ax[0], off[1]), wv::mul_rn(ax[1], off[0]));
    for (int i = 0; i < 3; ++i) jr[i] = ax[i];
}
/* x = (L L^T)^-1 x with L in the lower triangle of S.M (chol_solve of the host compile), x in LDS */
WV_DEVICE void setconst_chol_solve(const SetConstShared &S, int n, double *x) {
    for (int i = 0; i < n; ++i) {
        double s = x[i];
        for (int k = 0; k < i; ++k) s = wv::sub_rn(s, wv::mul_rn(S.M[i][k], x[k]));
        x[i] = wv::div_rn(s, S.M[i][i]);
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = x[i];
        for (int k = i + 1; k < n; ++k) s = wv::sub_rn(s, wv::mul_rn(S.M[k][i], x[k]));
        x[i] = wv::div_rn(s, S.M[i][i]);
    }
}

/* |v| of a 3-vector, as the host compile's sqrt(x x + y y + z z) */
WV_DEVICE double setconst_norm3(double x, double y, double z) {
    return wv::sqrt_rn(wv::add_rn(wv::add_rn(wv::mul_rn(x, x), wv::mul_rn(y, y)), wv::mul_rn(z, z)));
}
/* Geometry of an env (lane = collision geom, then lane = body): geom_mat = the host compile's quat2mat of geom_quat (no
 * normalisation, like phys_model_compile), and body_reach = for every tree root the largest distance bound of the tree's collision
 * geoms -- |geom_pos| + rbound, plus |body_pos| and 2 |jnt_pos| of every body / joint on the way to the root, unbounded past a slide
 * or free joint below the root, plus 2 |jnt_pos| of the root's own joints (HostModel::compile, the same additions in the same order).
 * (f64 sqrt on the device is the correctly rounded one, __dsqrt_rn, so the bound is the host's bit for bit -- as the Cholesky
 * pivots of the inertial part are.) */
WV_DEVICE void setconst_geometry(SetConstShared &S, ModelPtr m, cm_envparams_t *P, int lane) {
    const int ngeom = m->ngeom, nbody = m->nbody;
    if (lane < ngeom) {
        const double *q = P->geom_quat[lane];
        double *R = P->geom_mat[lane];
        const double q00 = wv::mul_rn(q[0], q[0]), q11 = wv::mul_rn(q[1], q[1]), q22 = wv::mul_rn(q[2], q[2]), q33 = wv::mul_rn(q[3], q[3]);
        const double q01 = wv::mul_rn(q[0], q[1]), q02 = wv::mul_rn(q[0], q[2]), q03 = wv::mul_rn(q[0], q[3]);
        const double q12 = wv::mul_rn(q[1], q[2]), q13 = wv::mul_rn(q[1], q[3]), q23 = wv::mul_rn(q[2], q[3]);
        R[0] = wv::sub_rn(wv::sub_rn(wv::add_rn(q00, q11), q22), q33);
        R[1] = wv::mul_rn(2.0, wv::sub_rn(q12, q03));
        R[2] = wv::mul_rn(2.0, wv::add_rn(q13, q02));
        R[3] = wv::mul_rn(2.0, wv::add_rn(q12, q03));
        R[4] = wv::sub_rn(wv::add_rn(wv::sub_rn(q00, q11), q22), q33);
        R[5] = wv::mul_rn(2.0, wv::sub_rn(q23, q01));
        R[6] = wv::mul_rn(2.0, wv::sub_rn(q13, q02));
        R[7] = wv::mul_rn(2.0, wv::add_rn(q23, q01));
        R[8] = wv::add_rn(wv::sub_rn(wv::sub_rn(q00, q11), q22), q33);
        const int b = m->geom_bodyid[lane];
        double len = 0.0;
        if (m->body_weldid[b] != 0) {
            len = wv::add_rn(setconst_norm3(P->geom_pos[lane][0], P->geom_pos[lane][1], P->geom_pos[lane][2]), m->geom_rbound[lane]);
            const int r = m->body_rootid[b];
            for (int a = b; a != r && a > 0; a = m->body_parentid[a]) {
                len = wv::add_rn(len, setconst_norm3(m->body_pos[a][0], m->body_pos[a][1], m->body_pos[a][2]));
                for (int jj = 0; jj < m->body_jntnum[a]; ++jj) {
                    const int j = m->body_jntadr[a] + jj;
                    len = wv::add_rn(len, wv::mul_rn(2.0, setconst_norm3(m->jnt_pos[j][0], m->jnt_pos[j][1], m->jnt_pos[j][2])));
                    if (m->jnt_type[j] == CM_JNT_SLIDE || m->jnt_type[j] == CM_JNT_FREE) len = 1e30;
                }
            }
            for (int jj = 0; jj < m->body_jntnum[r]; ++jj) {
                const int j = m->body_jntadr[r] + jj;
                len = wv::add_rn(len, wv::mul_rn(2.0, setconst_norm3(m->jnt_pos[j][0], m->jnt_pos[j][1], m->jnt_pos[j][2])));
            }
        }
        S.glen[lane] = len;
    }
    wv::sync();
    if (lane < nbody) {
        double reach = 0.0;
        for (int g = 0; g < ngeom; ++g) {
            const int b = m->geom_bodyid[g];
            if (m->body_weldid[b] != 0 && m->body_rootid[b] == lane && S.glen[g] > reach) reach = S.glen[g];
        }
        P->body_reach[lane] = reach;
    }
    wv::sync();
}
/* Springs of an env (lane = dof): the passive stage's per-dof records of the dof's hinge / slide joint (zero stiffness otherwise) */
WV_DEVICE void setconst_springs(ModelPtr m, cm_envparams_t *P, int lane) {
    if (lane < m->nv) {
        const int j = m->dof_jntid[lane], jt = m->jnt_type[j];
        const bool scalar = jt == CM_JNT_HINGE || jt == CM_JNT_SLIDE;
        P->dof_stiffness[lane] = scalar ? P->jnt_stiffness[j] : 0.0;
        P->dof_springref[lane] = scalar ? P->qpos_spring[m->jnt_qposadr[j]] : 0.0;
    }
    wv::sync();
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_setconst_kernel(SetConstIO io) {
    WV_SHARED SetConstShared S;
    const int lane = wv::lane();
    for (int idx = wv::env_id(); idx < io.nenv; idx += wv::grid_size()) {
    const int env = io.env0 + idx;
    const ModelPtr m = (ModelPtr)io.model;
    cm_envparams_t *P = io.params + env;
    const int nv = m->nv, nbody = m->nbody, njnt = m->njnt;
    if (io.derive_inertial == SETCONST_GEOMETRY || io.derive_inertial == SETCONST_ALL) setconst_geometry(S, m, P, lane);
    if (io.derive_inertial == SETCONST_SPRINGS || io.derive_inertial == SETCONST_ALL) setconst_springs(m, P, lane);
    if (io.derive_inertial == SETCONST_GEOMETRY || io.derive_inertial == SETCONST_SPRINGS) continue;
    if (io.derive_inertial == SETCONST_ALL) {
    /* inertial origins at qpos0: xipos = xmat0 ipos + xpos0 */
    if (lane < nbody) {
        const int b = lane;
        double v[3] = {0, 0, 0};
        if (b > 0) {
            const double *ip = P->body_ipos[b];
            for (int i = 0; i < 3; ++i)
                v[i] = wv::add_rn(wv::add_rn(wv::add_rn(wv::mul_rn(m->body_xmat0[b][3 * i], ip[0]), wv::mul_rn(m->body_xmat0[b][3 * i + 1], ip[1])), wv::mul_rn(m->body_xmat0[b][3 * i + 2], ip[2])), m->body_xpos0[b][i]);
        }
        for (int i = 0; i < 3; ++i) S.xipos[b][i] = v[i];
    }
    if (lane < CM_MAXV) for (int r = 0; r < CM_MAXV; ++r) S.M[r][lane] = 0.0;
    if (lane == 0) S.ok = 1;
    wv::sync();
    /* M(qpos0) = sum over bodies of J^T diag(m, I) J (lane = column), + armature */
    for (int b = 1; b < nbody; ++b) {
        const double mass = P->body_mass[b];
        if (mass <= 0) continue;
        if (lane < nv) {
            double jp[3], jr[3];
            setconst_jac_col(m, b, lane, S.xipos[b], jp, jr);
            for (int i = 0; i < 3; ++i) {
                S.Jp[i][lane] = jp[i];
                S.Jl[i][lane] = wv::add_rn(wv::add_rn(wv::mul_rn(m->body_ximat0[b][i], jr[0]), wv::mul_rn(m->body_ximat0[b][3 + i], jr[1])), wv::mul_rn(m->body_ximat0[b][6 + i], jr[2]));
            }
        }
        wv::sync();
        if (lane < nv) {
            const int c = lane;
            for (int r = 0; r < nv; ++r) {
                double s = 0;
                for (int i = 0; i < 3; ++i)
                    s = wv::add_rn(s, wv::add_rn(wv::mul_rn(wv::mul_rn(mass, S.Jp[i][r]), S.Jp[i][c]),
                                                 wv::mul_rn(wv::mul_rn(P->body_inertia[b][i], S.Jl[i][r]), S.Jl[i][c])));
                S.M[r][c] = wv::add_rn(S.M[r][c], s);
            }
        }
        wv::sync();
    }
    if (lane < nv) S.M[lane][lane] = wv::add_rn(S.M[lane][lane], m->dof_armature[lane]);
    wv::sync();
    if (lane == 0) {
        double mean = 0;
        for (int d = 0; d < nv; ++d) mean = wv::add_rn(mean, S.M[d][d]);
        P->meaninertia = nv > 0 ? wv::div_rn(mean, (double)nv) : 1.0;
    }
    /* Cholesky factor in place, column by column (lane = row) */
    for (int j = 0; j < nv; ++j) {
        double s = 0;
        if (lane >= j && lane < nv) {
            s = S.M[lane][j];
            for (int k = 0; k < j; ++k) s = wv::sub_rn(s, wv::mul_rn(S.M[lane][k], S.M[j][k]));
            if (lane == j) { if (s <= 0) S.ok = 0; S.piv = wv::sqrt_rn(s > 0 ? s : 1.0); }
        }
        wv::sync();
        if (lane >= j && lane < nv) S.M[lane][j] = lane == j ? S.piv : wv::div_rn(s, S.piv);
        wv::sync();
    }
    if (S.ok) { /* (a mass matrix that is not positive definite leaves the weights as they were, like the host compile) */
    /* bodies: lane = 2 body + (0 translational | 1 rotational); three solves each, summed in order */
    {
        const int b = lane >> 1, kind = lane & 1;
        const bool live = b > 0 && b < nbody && m->body_weldid[b] != 0;
        double acc = 0;
        for (int i = 0; i < 3; ++i) {
            if (live) {
                for (int d = 0; d < nv; ++d) {
                    double jp[3], jr[3];
                    setconst_jac_col(m, b, d, S.xipos[b], jp, jr);
                    const double v = kind ? jr[i] : jp[i];
                    S.X[lane][d] = v; S.X0[lane][d] = v;
                }
                setconst_chol_solve(S, nv, S.X[lane]);
                for (int d = 0; d < nv; ++d) acc = wv::add_rn(acc, wv::mul_rn(S.X0[lane][d], S.X[lane][d]));
            }
        }
        if (b < nbody) S.bw[b][kind] = live ? wv::div_rn(acc, 3.0) : 0.0;
    }
    wv::sync();
    /* dofs: diag(M^-1) by unit-vector solves, averaged over the dofs of ball / free joints */
    if (lane < nv) {
        for (int d = 0; d < nv; ++d) S.X[lane][d] = d == lane ? 1.0 : 0.0;
        setconst_chol_solve(S, nv, S.X[lane]);
        S.dinv[lane] = S.X[lane][lane];
    }
    wv::sync();
    if (lane < njnt) {
        const int j = lane, d = m->jnt_dofadr[j], jt = m->jnt_type[j];
        if (jt == CM_JNT_FREE) {
            const double a = wv::div_rn(wv::add_rn(wv::add_rn(S.dinv[d], S.dinv[d + 1]), S.dinv[d + 2]), 3.0);
            const double r = wv::div_rn(wv::add_rn(wv::add_rn(S.dinv[d + 3], S.dinv[d + 4]), S.dinv[d + 5]), 3.0);
            for (int k = 0; k < 3; ++k) { S.dw[d + k] = a; S.dw[d + 3 + k] = r; }
        } else if (jt == CM_JNT_BALL) {
            const double r = wv::div_rn(wv::add_rn(wv::add_rn(S.dinv[d], S.dinv[d + 1]), S.dinv[d + 2]), 3.0);
            for (int k = 0; k < 3; ++k) S.dw[d + k] = r;
        } else S.dw[d] = S.dinv[d];
    }
    wv::sync();
    if (lane < nbody) { P->body_invweight0[lane][0] = S.bw[lane][0]; P->body_invweight0[lane][1] = S.bw[lane][1]; }
    if (lane < nv) P->dof_invweight0[lane] = S.dw[lane];
    wv::sync();
    }
    /* what the constraint stages read: per limited joint, per equality, per candidate pair (HostModel::compile) */
    if (lane < njnt) P->jnt_liminvweight[lane] = P->dof_invweight0[m->jnt_dofadr[lane]];
    if (lane < m->neq) P->eq_invweight[lane] = wv::add_rn(wv::add_rn(0.0, P->body_invweight0[m->eq_body1[lane]][0]), P->body_invweight0[m->eq_body2[lane]][0]);
    for (int p = lane; p < m->npair; p += WV_WAVE) {
        const int g1 = m->pair_geom1[p], g2 = m->pair_geom2[p];
        P->pair_invweight[p] = wv::add_rn(wv::add_rn(0.0, P->body_invweight0[m->geom_bodyid[g1]][0]), P->body_invweight0[m->geom_bodyid[g2]][0]);
    }
    }
    /* contact friction of every candidate pair: the geom with the higher priority wins outright, else the larger coefficient */
    for (int p = lane; p < m->npair; p += WV_WAVE) {
        const int g1 = m->pair_geom1[p], g2 = m->pair_geom2[p], pa = m->geom_priority[g1], pb = m->geom_priority[g2];
        for (int k = 0; k < 3; ++k) {
            const double f1 = P->geom_friction[g1][k], f2 = P->geom_friction[g2][k];
            P->pair_friction[p][k] = pa != pb ? (pa > pb ? f1 : f2) : (f1 > f2 ? f1 : f2);
        }
    }
    wv::sync();
    }
}

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

/* The world pose of a body that is a child of the world in a kin_simple model, from the env's qpos alone -- up to CM_MAXSLIDE slides and
 * a ball or free joint, whose quaternion is normalised here, as in the step kernel's kinematics stage (the height scan and the depth
 * image both start from it: no forward pass) */
WV_DEVICE void static_body_pose(ModelPtr m, int body, const double *q, double *bp, double *bq) {
    const auto *kr = &m->body_kin[body];
    for (int k = 0; k < 3; ++k) bp[k] = kr->pos[k];
    for (int k = 0; k < 4; ++k) bq[k] = kr->quat[k];
    for (int sl = 0; sl < kr->nslide; ++sl) {
        const double d = q[kr->slide_qadr[sl]] - kr->slide_ref[sl];
        for (int k = 0; k < 3; ++k) bp[k] += kr->slide_axis_p[sl][k] * d;
    }
    if (kr->rot_type == CM_JNT_BALL || kr->rot_type == CM_JNT_FREE) {
        const int qa = kr->rot_qadr, qo = kr->rot_type == CM_JNT_FREE ? qa + 3 : qa;
        double qj[4] = {q[qo], q[qo + 1], q[qo + 2], q[qo + 3]}, q0[4] = {bq[0], bq[1], bq[2], bq[3]}, R[9], r[3];
        normalize4(qj);
        if (kr->rot_type == CM_JNT_FREE) for (int k = 0; k < 3; ++k) bp[k] = q[qa + k];
        mulquat(bq, q0, qj);
        const double jp[3] = {kr->rot_pos[0], kr->rot_pos[1], kr->rot_pos[2]};
        quat2mat(R, bq);
        mulmatvec3(r, R, jp);
        for (int k = 0; k < 3; ++k) bp[k] = bp[k] + kr->rot_pos_p[k] - r[k];
    }
}
/* The world pose (position gp, rotation R, row-major) of geom g of a body welded to the world: the geom's own pose from PG (the env's
 * block or the model's), composed with the static bodies between it and the world */
WV_DEVICE void static_geom_pose(ModelPtr m, ParamPtr PG, int g, double *gp, double *R) {
    for (int k = 0; k < 3; ++k) gp[k] = PG->geom_pos[g][k];
    for (int k = 0; k < 9; ++k) R[k] = PG->geom_mat[g][k];
    for (int a = m->geom_bodyid[g]; a > 0; a = m->body_parentid[a]) {
        double Rn[9], pn[3];
        double Rb[9];
        for (int k = 0; k < 9; ++k) Rb[k] = m->body_mat[a][k];
        for (int r_ = 0; r_ < 3; ++r_) {
            for (int c = 0; c < 3; ++c) Rn[3 * r_ + c] = Rb[3 * r_] * R[c] + Rb[3 * r_ + 1] * R[3 + c] + Rb[3 * r_ + 2] * R[6 + c];
            pn[r_] = m->body_pos[a][r_] + (Rb[3 * r_] * gp[0] + Rb[3 * r_ + 1] * gp[1] + Rb[3 * r_ + 2] * gp[2]);
        }
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
        for (int k = 0; k < 3; ++k) gp[k] = pn[k];
    }
}

/* The surface S(X, Y) of the height scan and of the placed restart: the highest point at which the vertical line through the world point
 * (X, Y) meets a static collision geom of the env -- planes, boxes, the height field on `grid` (null: no samples, a miss), as the
 * comment of cassie_scan_kernel below lists them.  Returns whether it meets any, the height in *top; a tilted height-field geom is
 * left out and sets WARN_SCAN_TILTED in *warn. */
WV_DEVICE bool scan_surface(ModelPtr m, ParamPtr PG, const float *grid, double X, double Y, double *top_out, int *warn_out) {
    bool hit = false;
    double top = 0.0;
    int warn = 0;
    for (int g = 0; g < m->ngeom; ++g) {
        const int gb = m->geom_bodyid[g], gt = m->geom_type[g];
        if (m->body_weldid[gb] != 0 || (gt != CM_GEOM_PLANE && gt != CM_GEOM_BOX && gt != CM_GEOM_HFIELD)) continue;
        double gp[3], R[9];
        static_geom_pose(m, PG, g, gp, R);
        const double dx = X - gp[0], dy = Y - gp[1];
        bool has = false;
        double z = 0.0;
        if (gt == CM_GEOM_PLANE) {
            if (R[8] > 0.0) { has = true; z = gp[2] - (R[2] * dx + R[5] * dy) / R[8]; }
        } else if (gt == CM_GEOM_BOX) {
            /* the line (X, Y, t) in the box's frame: origin R^T ((X, Y, 0) - pos), direction R^T e_z = the third row of R */
            const double o[3] = {R[0] * dx + R[3] * dy - R[6] * gp[2], R[1] * dx + R[4] * dy - R[7] * gp[2], R[2] * dx + R[5] * dy - R[8] * gp[2]};
            double t0 = -1e300, t1 = 1e300;
            bool inside = true;
            for (int k = 0; k < 3; ++k) {
                const double d = R[6 + k], s = m->geom_size[g][k];
                if (d != 0.0) {
                    const double ta = (-s - o[k]) / d, tb = (s - o[k]) / d;
                    const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
                    t0 = lo > t0 ? lo : t0; t1 = hi < t1 ? hi : t1;
                } else if (fabs(o[k]) > s) inside = false;
            }
            if (inside && t0 <= t1) { has = true; z = t1; }
        } else {
            const bool upright = fabs(R[2]) <= 1e-12 && fabs(R[5]) <= 1e-12 && R[8] > 0.0;
            if (!upright) warn |= WARN_SCAN_TILTED;
            else if (grid && m->hfield_nrow >= 2 && m->hfield_ncol >= 2) {
                const double sx = m->hfield_size[0], sy_ = m->hfield_size[1], sz = m->hfield_size[2];
                const int nc = m->hfield_ncol, nr = m->hfield_nrow;
                const double xl = R[0] * dx + R[3] * dy, yl = R[1] * dx + R[4] * dy;   /* (translation and yaw) */
                if (fabs(xl) <= sx && fabs(yl) <= sy_) {
                    const double cx = 2 * sx / (nc - 1), cyl = 2 * sy_ / (nr - 1);
                    int cj = (int)floor((xl + sx) / cx), ci = (int)floor((yl + sy_) / cyl);
                    cj = cj < 0 ? 0 : (cj > nc - 2 ? nc - 2 : cj); ci = ci < 0 ? 0 : (ci > nr - 2 ? nr - 2 : ci);
                    const double u = (xl - (-sx + cj * cx)) / cx, v = (yl - (-sy_ + ci * cyl)) / cyl;
                    const double z00 = sz * grid[ci * nc + cj], z10 = sz * grid[ci * nc + cj + 1];
                    const double z01 = sz * grid[(ci + 1) * nc + cj], z11 = sz * grid[(ci + 1) * nc + cj + 1];
                    const double h = u + v <= 1.0 ? z00 + (u * (z10 - z00) + v * (z01 - z00))
                                                  : z11 + ((1.0 - u) * (z01 - z11) + (1.0 - v) * (z10 - z11));
                    has = true; z = gp[2] + h;
                }
            }
        }
        if (has && (!hit || z > top)) { hit = true; top = z; }
    }
    *top_out = top; *warn_out |= warn;
    return hit;
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
        const ParamPtr PG = (io.envparams && m->env_geom) ? (ParamPtr)(io.envparams + env) : (ParamPtr)&m->params;
        /* the heading of the anchor as the scan takes it, turned on by yaw */
        const double ys = 2.0 * (aq[0] * aq[3] + aq[1] * aq[2]), yc = 1.0 - 2.0 * (aq[2] * aq[2] + aq[3] * aq[3]);
        const double yn = sqrt(ys * ys + yc * yc);
        const double cy = yn > 0.0 ? yc / yn : 1.0, sy = yn > 0.0 ? ys / yn : 0.0;
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

/* The height scan (phys_batch_height_scan, include/cassie_phys.h), one wave per env, lanes over the scan points (a loop for more than
 * 64): point j of the pattern, given in the HEADING frame of a body -- origin at the body's world x, y, turned about world z by the
 * yaw of the body's world quaternion -- is the world point (X, Y); the env's value for it is clamp(z_body - S(X, Y), -range, range),
 * S = the highest point at which the vertical line through (X, Y) meets a static collision geom (a geom of a body welded to the
 * world) of the env, +range where it meets none:
 *   plane          the line's intersection with it (normal with a positive world z only);
 *   box            where the line leaves the box upwards: the far end of a slab test in the box's frame, any pose;
 *   height field   the env's own grid (terrain_grid: shared, per env, or the bank's terrain of the env's index) on the surface the narrow
 *                  phase collides with (pk_collision.h hfield_sphere: vertices on the grid scaled by hfield_size, every cell split
 *                  into the triangles v00 v10 v01 and v11 v01 v10), linear within the triangle, a miss outside the grid's footprint;
 *                  only for a geom whose z axis is the world's (translation and yaw): a tilted one is left out and raises
 *                  WARN_SCAN_TILTED.
 * Geom poses are the env's own once the batch has randomised geometry (cm_model_t::env_geom: the step kernel's gate), else the
 * model's.  The body is a child of the world in a kin_simple model (Cassie's pelvis): its pose follows from the env's qpos alone --
 * up to CM_MAXSLIDE slides and a ball or free joint, as in the step kernel's kinematics stage -- so no forward pass is needed.
 * Like cassie_episode_kernel a fixed grid of workgroups walks the range (one per CU: an env's scan is a chain of dependent reads). */
constexpr int SCAN_GRID = 256, SCAN_MAXPOINTS = 1024;
struct ScanIO {
    const cm_model_t *models; int model_stride;
    const cm_envparams_t *envparams;   /* null, or one block per env (PhysIO::envparams) */
    int env0, n, npoints, body;
    double range;
    const double *offsets;             /* [npoints][2] */
    const double *qpos; int sq;
    double *out; int sout;             /* [nenv][npoints] with a row stride in doubles */
    const float *hfield; size_t hfield_stride; const int *hfield_index; int hfield_nterrain;   /* as in PhysIO */
    int *warn;
};
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_scan_kernel(ScanIO io) {
    const int lane = wv::lane();
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) {
        const int env = io.env0 + i;
        const ModelPtr m = (ModelPtr)(io.models + (size_t)env * io.model_stride);
        const ParamPtr PG = (io.envparams && m->env_geom) ? (ParamPtr)(io.envparams + (size_t)env) : (ParamPtr)&m->params;
        const double *q = io.qpos + (size_t)env * io.sq;
        double bp[3], bq[4];
        static_body_pose(m, io.body, q, bp, bq);                  /* (wave-uniform) */
        const double ys = 2.0 * (bq[0] * bq[3] + bq[1] * bq[2]), yc = 1.0 - 2.0 * (bq[2] * bq[2] + bq[3] * bq[3]);
        const double yn = sqrt(ys * ys + yc * yc);
        const double cy = yn > 0.0 ? yc / yn : 1.0, sy = yn > 0.0 ? ys / yn : 0.0;
        bool clamped;
        const float *grid = terrain_grid(io.hfield, io.hfield_stride, io.hfield_index, io.hfield_nterrain, env, &clamped);
        int warn = clamped ? WARN_TERRAIN_INDEX : 0;
        for (int j0 = 0; j0 < io.npoints; j0 += WV_WAVE) {
            const int j = j0 + lane;
            const bool mine = j < io.npoints;
            const double ox = mine ? io.offsets[2 * j] : 0.0, oy = mine ? io.offsets[2 * j + 1] : 0.0;
            const double X = bp[0] + (cy * ox - sy * oy), Y = bp[1] + (sy * ox + cy * oy);
            double top;
            const bool hit = scan_surface(m, PG, grid, X, Y, &top, &warn);
            double val = io.range;
            if (hit) { val = bp[2] - top; val = val > io.range ? io.range : (val < -io.range ? -io.range : val); }
            if (mine) io.out[(size_t)env * io.sout + j] = val;
        }
        if (warn && lane == 0) io.warn[env] |= warn;
    }
}

}  // namespace ck
#endif
