/*
 * probe_kernels.h -- probes: the reward-side getters of the reference for ANY body or site, batched (phys_batch_probe, include/cassie_phys.h:
 * the definition is there).  A configured list of points, each fixed in the frame of a body or of a site, evaluated for an env range from
 * the read-out (cm_ext_t) and the body poses a forward pass of the range has just left: position, orientation, the point's velocity, the
 * body's cvel and acceleration, the point's Jacobians, the summed contact force on the body, and one word per env that says which classes
 * of geoms touch.  Each value is the arithmetic of the single-simulator getter of csrc/cassiemujoco.c it stands for (point_jacobian,
 * cassie_sim_body_acceleration, cassie_sim_body_contact_force, the three collision checks).  Written with the wv:: primitives only,
 * workgroups of one wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_probes.cpp) runs the same text.  The launch
 * record, the row's layout, the grid and the checks are small_launch.h's (no field of ProbeIO is assigned anywhere else).
 *
 * One wave takes an env at a time and PROBE_GRID workgroups walk the range (as cassie_scan_kernel and state_walk do).  Per env:
 *   lane = probe   the frame (a body's xpos / xquat as the forward pass stored them; a site's site_xpos / site_xmat of the read-out), the
 *                  point p = x + R offset, and POS, QUAT, VEL, CVEL, ACC (a loop over the body's dofs) and CFRC (a loop over the contacts);
 *   lane = dof     the Jacobians, probe by probe (the probe's point and body come from its lane by wv::shfl): lane k writes column k of
 *                  each of the six rows [nv], so a row's stores are contiguous across the wave (derive_env's pattern, nv columns);
 *   lane 0         the contact word, from the contact list's geom ids (in the FULL geom list) through the table of the geoms' classes
 *                  that the host built when the probes were configured: the kernel does not know the host model.
 * An env whose state fails the step kernel's own divergence test (a NaN or an entry beyond 1e10 in qpos / qvel) has no read-out -- the
 * forward pass leaves such an env at once -- so its row is NaN throughout and its contact word 0; nothing is indexed by such a value.
 * Vector loads and stores only; an env's wave touches that env's read-out, its row and its word alone.
 */
#ifndef CASSIE_PROBE_KERNELS_H
#define CASSIE_PROBE_KERNELS_H

#include "physics_kernel.h"

namespace ck {

/* PROBE_GRID: the workgroups that walk a range.  A few, like the episode kernel's: the launch runs behind a range's forward pass while
 * the other range's step kernel fills the chip, where every workgroup waits for a wave slot to free; an env costs a few dependent reads
 * of its read-out and at most PROBES_MAX * (25 + 6 nv) stores.  A first choice, by that arithmetic (tools/probe_rate.py measures the
 * call in the loop it is meant for). */
constexpr int PROBE_GRID = 64, PROBES_MAX = 32;
enum { PROBE_BODY = 0, PROBE_SITE = 1 };   /* (PHYS_PROBE_* of cassie_phys.h) */
/* the quantities of a row in bit order (bit q of the mask: PHYS_PQ_* of cassie_phys.h), and the per-env word behind them */
enum { PQ_POS, PQ_QUAT, PQ_VEL, PQ_CVEL, PQ_ACC, PQ_JACP, PQ_JACR, PQ_CFRC, PQ_COUNT, PQ_CONTACTS = PQ_COUNT };
/* bits of the contact word (PHYS_PC_*): an obstacle geom touches anything, two geoms of the robot touch, a geom of group 1 touches one of group g */
enum { PC_OBSTACLE = 1, PC_SELF = 2, PC_GROUP0 = 1 << 8, PC_NGROUPS = 6 };
/* an entry of the geoms' class table: the class of geom_user[0] (1: obstacle, 2: robot, else 0) in the low byte, geom_group above it
 * (PROBE_NO_GROUP: a group that is none of 0 .. PC_NGROUPS - 1 and not 1) */
constexpr int PROBE_CLASS_MASK = 0xff, PROBE_GROUP_SHIFT = 8, PROBE_NO_GROUP = 0xffff;

/* an entry of the table (phys_probe_t of cassie_phys.h) */
struct ProbeDef { int kind, id; double offset[3]; };

struct ProbeIO {
    const cm_model_t *models; int model_stride;
    int env0, n, nprobes;
    unsigned quantities;                /* bit q: quantity q is in the row; bit PQ_CONTACTS: the contact word is written */
    const ProbeDef *probes;             /* [nprobes] */
    const int *geom_class; int ngeom;   /* [ngeom]: the classes of the geoms of the FULL list (null: no contact word) */
    const cm_ext_t *ext;                /* [nenv] the read-out of the forward pass */
    const double *xpos, *xquat;         /* [nenv][nbody][3 / 4] body poses of the forward pass, rows sxp / sxq doubles apart */
    int sxp, sxq;
    const double *qpos, *qvel, *qacc;   /* the state, and the forward pass's qacc; rows sq / sqv / sv doubles apart */
    int sq, sqv, sv;
    double *out; int sout;              /* [nenv] rows, a row stride in doubles */
    int *contacts;                      /* [nenv] or null */
    int off[PQ_COUNT];                  /* where a quantity's [nprobes][dim] block starts in the row (-1: absent) */
    int row_dim;
};

WV_DEVICE void probe_env(const ProbeIO &io, size_t env, int lane) {
    const ModelPtr m = (ModelPtr)(io.models + env * io.model_stride);
    const int nq = m->nq, nv = m->nv;
    double *out = io.out + env * io.sout;
    const double *qvel = io.qvel + env * io.sqv;
    /* the step kernel's divergence test: the forward pass has left this env without a read-out */
    {
        bool bad = false;
        for (int k = lane; k < nq; k += WV_WAVE) { const double v = io.qpos[env * io.sq + k]; bad |= !(v == v) || fabs(v) > 1e10; }
        for (int k = lane; k < nv; k += WV_WAVE) { const double v = qvel[k]; bad |= !(v == v) || fabs(v) > 1e10; }
        if (wv::ballot(bad) != 0ull) {
            const double nan = __builtin_nan("");
            for (int k = lane; k < io.row_dim; k += WV_WAVE) out[k] = nan;
            if (io.contacts && lane == 0) io.contacts[env] = 0;
            return;
        }
    }
    const cm_ext_t *ex = io.ext + env;
    const double *xpos = io.xpos + env * io.sxp, *xquat = io.xquat + env * io.sxq, *qacc = io.qacc + env * io.sv;
    int ncon = ex->ncon;
    ncon = ncon < 0 ? 0 : ncon > CM_MAXCON ? CM_MAXCON : ncon;
    const unsigned Q = io.quantities;

    /* ---- lane = probe ---- */
    const bool mine = lane < io.nprobes;
    const ProbeDef *pd = io.probes + (mine ? lane : 0);
    const int kind = pd->kind, id = pd->id;
    const int body = kind == PROBE_SITE ? m->site_bodyid[id] : id;
    double p[3];
    {
        double x[3], R[9], quat[4];
        if (kind == PROBE_SITE) {
            for (int i = 0; i < 3; ++i) x[i] = ex->site_xpos[id][i];
            for (int i = 0; i < 9; ++i) R[i] = ex->site_xmat[id][i];
            mat2quat(quat, R);
        } else {
            for (int i = 0; i < 3; ++i) x[i] = xpos[3 * body + i];
            for (int i = 0; i < 4; ++i) quat[i] = xquat[4 * body + i];
            quat2mat(R, quat);
        }
        const double o[3] = {pd->offset[0], pd->offset[1], pd->offset[2]};
        double t[3];
        mulmatvec3(t, R, o);
        for (int i = 0; i < 3; ++i) p[i] = x[i] + t[i];
        if (mine && (Q >> PQ_POS & 1u)) for (int i = 0; i < 3; ++i) out[io.off[PQ_POS] + 3 * lane + i] = p[i];
        if (mine && (Q >> PQ_QUAT & 1u)) for (int i = 0; i < 4; ++i) out[io.off[PQ_QUAT] + 4 * lane + i] = quat[i];
    }
    const int root = m->body_rootid[body];
    if (mine && (Q >> PQ_VEL & 1u)) {
        const double *cv = ex->cvel[body], *rc = ex->subtree_com[root];
        const double w[3] = {cv[0], cv[1], cv[2]}, off[3] = {p[0] - rc[0], p[1] - rc[1], p[2] - rc[2]};
        double t[3];
        cross3(t, w, off);
        for (int i = 0; i < 3; ++i) { out[io.off[PQ_VEL] + 6 * lane + i] = w[i]; out[io.off[PQ_VEL] + 6 * lane + 3 + i] = cv[3 + i] + t[i]; }
    }
    if (mine && (Q >> PQ_CVEL & 1u)) for (int i = 0; i < 6; ++i) out[io.off[PQ_CVEL] + 6 * lane + i] = ex->cvel[body][i];
    if (mine && (Q >> PQ_ACC & 1u)) {
        /* cassie_sim_body_acceleration: -gravity in the linear part, then the body's dofs in order */
        double a[6] = {0, 0, 0, -m->gravity[0], -m->gravity[1], -m->gravity[2]};
        const unsigned long long mask = m->body_dofmask[body];
        for (int k = 0; k < nv; ++k) {
            if (!((mask >> k) & 1ull)) continue;
            const double v = qvel[k], ac = qacc[k];
            for (int i = 0; i < 6; ++i) a[i] += ex->cdof_dot[k][i] * v + ex->cdof[k][i] * ac;
        }
        for (int i = 0; i < 6; ++i) out[io.off[PQ_ACC] + 6 * lane + i] = a[i];
    }
    if (mine && (Q >> PQ_CFRC & 1u)) {
        /* cassie_sim_body_contact_force: frame^T [normal, tangent 1, tangent 2] of every contact of the body, minus where it is geom1's */
        double f3[3] = {0, 0, 0};
        for (int c = 0; c < ncon; ++c) {
            const int b1 = ex->con_body1[c], b2 = ex->con_body2[c];
            if (body != b1 && body != b2) continue;
            const double *fr = ex->con_frame[c], *f = ex->con_force[c];
            const double sgn = (body == b1) ? -1.0 : 1.0;
            for (int k = 0; k < 3; ++k) f3[k] += sgn * (fr[k] * f[0] + fr[3 + k] * f[1] + fr[6 + k] * f[2]);
        }
        for (int i = 0; i < 3; ++i) out[io.off[PQ_CFRC] + 3 * lane + i] = f3[i];
    }

    /* ---- lane = dof: point_jacobian, probe by probe ---- */
    if (Q & (1u << PQ_JACP | 1u << PQ_JACR)) {
        for (int k0 = 0; k0 < nv; k0 += WV_WAVE) {
            const int k = k0 + lane;
            const bool isdof = k < nv;
            double cd[6] = {0, 0, 0, 0, 0, 0};
            if (isdof) for (int i = 0; i < 6; ++i) cd[i] = ex->cdof[k][i];
            for (int j = 0; j < io.nprobes; ++j) {
                const int bj = wv::shfl_i(body, j), rj = wv::shfl_i(root, j);
                const double pj[3] = {wv::shfl(p[0], j), wv::shfl(p[1], j), wv::shfl(p[2], j)};
                if (!isdof) continue;
                double jp[3] = {0, 0, 0}, jr[3] = {0, 0, 0};
                if (bj > 0 && ((m->body_dofmask[bj] >> k) & 1ull)) {
                    const double *com = ex->subtree_com[rj];
                    const double off[3] = {pj[0] - com[0], pj[1] - com[1], pj[2] - com[2]};
                    double t[3];
                    cross3(t, cd, off);
                    for (int i = 0; i < 3; ++i) { jp[i] = cd[3 + i] + t[i]; jr[i] = cd[i]; }
                }
                for (int i = 0; i < 3; ++i) {
                    if (Q >> PQ_JACP & 1u) out[io.off[PQ_JACP] + (size_t)(3 * j + i) * nv + k] = jp[i];
                    if (Q >> PQ_JACR & 1u) out[io.off[PQ_JACR] + (size_t)(3 * j + i) * nv + k] = jr[i];
                }
            }
        }
    }

    /* ---- lane 0: the contact word ---- */
    if (io.contacts && lane == 0) {
        int word = 0;
        for (int c = 0; c < ncon; ++c) {
            const int g1 = ex->con_geom1[c], g2 = ex->con_geom2[c];
            if (g1 < 0 || g1 >= io.ngeom || g2 < 0 || g2 >= io.ngeom) continue;
            const int c1 = io.geom_class[g1], c2 = io.geom_class[g2];
            const int u1 = c1 & PROBE_CLASS_MASK, u2 = c2 & PROBE_CLASS_MASK, r1 = c1 >> PROBE_GROUP_SHIFT, r2 = c2 >> PROBE_GROUP_SHIFT;
            if (u1 == 1 || u2 == 1) word |= PC_OBSTACLE;
            if (u1 == 2 && u2 == 2) word |= PC_SELF;
            if (r1 == 1 && r2 < PC_NGROUPS) word |= PC_GROUP0 << r2;
            if (r2 == 1 && r1 < PC_NGROUPS) word |= PC_GROUP0 << r1;
        }
        io.contacts[env] = word;
    }
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_probe_kernel(ProbeIO io) {
    const int lane = wv::lane();
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) probe_env(io, (size_t)io.env0 + (size_t)i, lane);
}

}  // namespace ck
#endif
