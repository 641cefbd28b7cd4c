/*
 * ray_kernel.h -- range sensors on any body (phys_batch_rays_cast, include/cassie_phys.h: the definition is there): a table of rays,
 * each attached to a body of its own in one of three frames, against any chosen set of the env's collision geoms, the moving bodies'
 * included -- the range, the geom hit and the surface normal.  The intersection routines, the geoms' poses and the cull are the depth
 * scene kernel's (depth_kernel.h, which stays as it is); what is new is that the ray's origin, direction and body are the lane's and
 * not the wave's, the self-exclusion, and the normal.  Written with the wv:: primitives only, workgroups of one wave: phys_batch.hip
 * launches it, the wave emulator (tests/emu/emu_rays.cpp) runs the same text.
 */
#ifndef CASSIE_RAY_KERNEL_H
#define CASSIE_RAY_KERNEL_H

#include "depth_kernel.h"

namespace ck {

/* A job is (env, block of 64 rays of the table), lane l of the wave the block's ray l: a fixed grid of RAYS_GRID workgroups walks the
 * job list of the env range, the blocks of one env next to each other (a first choice, like the depth image's: DESIGN 4.3 has what the
 * launch was measured to cost with it).
 *
 * Per job, lane g builds the world frame of geom g (the scene kernel's text: static_geom_pose, or xpos / xquat as stored composed with
 * the geom's own pose) and the geom loop, whose index is wave-uniform, reads it with wv::readlane.  Per lane: the ray's body pose, read
 * from xpos / xquat as stored, the ray o + t u in the world (u is the table's unit direction turned by the body's rotation, by its
 * heading, or not at all), and -- geom by geom -- the scene kernel's tests with near = rmin, far = rmax.  A lane leaves out the geoms
 * of its own ray's body; a solid is tested only by the lanes whose ray meets its bounding sphere, and by nobody where no lane's does
 * (wv::ballot, a uniform branch).  The loop keeps the value, the geom and whether the value is `rmin` taken from inside a solid.
 *
 * The normal is worked out once, behind the loop, from the hit point: the winning geom's frame comes from its lane (wv::shfl: the
 * geom is the lane's own here), the ray goes into that frame once more, and
 *   plane          -+ z, against the ray;
 *   box            the slab test again: the axis whose entry is the largest (the one that gave t0; the first of equals), against the ray;
 *   sphere         the hit point, normalised;
 *   capsule        the hit point less its projection clamp(z, -h, h) onto the axis, normalised;
 *   height field   the cell under the hit point (clamped: nothing is indexed by a NaN) and in it the triangle v00 v10 v01 where
 *                  u + v <= 1, else v11 v01 v10: the cross product of its edges, turned against the ray;
 * rotated into the world.  A ray through an edge of a box or of a triangle takes either side's normal: the tests leave those out. */
constexpr int RAYS_GRID = 2048, RAYS_MAX = 1024;
enum { RAY_BODY = 0, RAY_WORLD_DIR = 1, RAY_HEADING = 2 };   /* (PHYS_RAY_* of cassie_phys.h) */

/* an entry of the table (phys_ray_t of cassie_phys.h, the direction normalised by the host) */
struct RayDef { int body, frame; double origin[3], dir[3]; };

struct RayIO {
    const cm_model_t *models; int model_stride;
    const cm_envparams_t *envparams;   /* null, or one block per env (PhysIO::envparams) */
    int env0, n, nrays;
    double rmin, rmax;
    const RayDef *rays;                /* [nrays] */
    unsigned geoms;                    /* bit g: compiled geom g is seen */
    const double *xpos, *xquat;        /* [nenv][nbody][3 / 4] body poses in the world, rows sxp / sxq doubles apart */
    int sxp, sxq;
    double *out; int sout;             /* [nenv][nrays] with a row stride in doubles */
    int *ids;                          /* null, or [nenv][nrays]: the geom that gave the value, -1 where it is `rmax` */
    double *normals;                   /* null, or [nenv][nrays][3] */
    const float *hfield; size_t hfield_stride; const int *hfield_index; int hfield_nterrain;   /* as in PhysIO */
    int *warn;
};

/* the normal (geom frame, not normalised) of the height field's triangle under the point p of its surface */
WV_DEVICE void ray_hfield_normal(const float *grid, int nr, int nc, double sx, double sy, double sz, const double *p, double *nl) {
    const double cx = 2 * sx / (nc - 1), cy = 2 * sy / (nr - 1);
    const double gx = (p[0] + sx) / cx, gy = (p[1] + sy) / cy;
    const int j = depth_cell(gx, nc - 2), i = depth_cell(gy, nr - 2);
    const double h00 = sz * grid[i * nc + j], h10 = sz * grid[i * nc + j + 1];
    const double h01 = sz * grid[(i + 1) * nc + j], h11 = sz * grid[(i + 1) * nc + j + 1];
    const bool lower = (gx - j) + (gy - i) <= 1.0;
    /* (v10 - v00) x (v01 - v00), or (v01 - v11) x (v10 - v11): both point up */
    nl[0] = lower ? -(h10 - h00) * cy : (h01 - h11) * cy;
    nl[1] = lower ? -(h01 - h00) * cx : (h10 - h11) * cx;
    nl[2] = cx * cy;
}

/* the axis whose slab the ray (geom frame) enters last: the face of a box's entry t0 (the first of equals) */
WV_DEVICE int ray_box_face(const double *o, const double *d, double s0, double s1, double s2) {
    const double s[3] = {s0, s1, s2};
    double t0 = -1e300;
    int axis = 0;
    for (int k = 0; k < 3; ++k) {
        if (d[k] != 0.0) {
            const double ta = (-s[k] - o[k]) / d[k], tb = (s[k] - o[k]) / d[k];
            const double lo = ta < tb ? ta : tb;
            if (lo > t0) { t0 = lo; axis = k; }
        }
    }
    return axis;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_rays_kernel(RayIO io) {
    const int lane = wv::lane();
    const int nblocks = (io.nrays + WV_WAVE - 1) / WV_WAVE;
    const long long njobs = (long long)io.n * nblocks;
    for (long long job = wv::env_id(); job < njobs; job += wv::grid_size()) {
        const int env = io.env0 + (int)(job / nblocks), block = (int)(job % nblocks);
        const ModelPtr m = env_model(io.models, io.model_stride, env);
        const ParamPtr PG = env_geometry(io.envparams, m, (size_t)env);
        const double *xpe = io.xpos + (size_t)env * io.sxp, *xqe = io.xquat + (size_t)env * io.sxq;
        /* this lane's ray in the world */
        const int j = block * WV_WAVE + lane;
        const bool mine = j < io.nrays;
        const RayDef *rd = io.rays + (mine ? j : 0);
        const int rbody = rd->body, frame = rd->frame;
        double o[3], D[3];
        {
            const double bq[4] = {xqe[4 * rbody], xqe[4 * rbody + 1], xqe[4 * rbody + 2], xqe[4 * rbody + 3]};
            const double ro[3] = {rd->origin[0], rd->origin[1], rd->origin[2]}, ru[3] = {rd->dir[0], rd->dir[1], rd->dir[2]};
            double Rb[9], off[3];
            if (frame == RAY_HEADING) {
                double cy, sy;
                quat_heading(bq, cy, sy);
                Rb[0] = cy; Rb[1] = -sy; Rb[2] = 0.0; Rb[3] = sy; Rb[4] = cy; Rb[5] = 0.0; Rb[6] = 0.0; Rb[7] = 0.0; Rb[8] = 1.0;
            } else quat2mat(Rb, bq);
            mulmatvec3(off, Rb, ro);
            mulmatvec3(D, Rb, ru);
            if (frame == RAY_WORLD_DIR) { D[0] = ru[0]; D[1] = ru[1]; D[2] = ru[2]; }
            /* (quat_heading answers a NaN quaternion with a heading of zero: such a ray sees nothing, whatever its frame) */
            const double poison = 0.0 * (bq[0] + bq[1] + bq[2] + bq[3]);
            for (int k = 0; k < 3; ++k) o[k] = xpe[3 * rbody + k] + off[k] + poison;
        }
        const double DD = dot3(D, D);
        bool clamped;
        const float *grid = terrain_grid(io.hfield, io.hfield_stride, io.hfield_index, io.hfield_nterrain, env, &clamped);
        /* lane g's own geom: its world position and rotation, where it is seen */
        double fp[3] = {0.0, 0.0, 0.0}, fR[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (lane < m->ngeom && ((io.geoms >> lane) & 1u)) {
            const int B = m->geom_bodyid[lane];
            if (m->body_weldid[B] == 0) static_geom_pose(m, PG, lane, fp, fR);
            else {
                const double q[4] = {xqe[4 * B], xqe[4 * B + 1], xqe[4 * B + 2], xqe[4 * B + 3]};
                const double lp[3] = {PG->geom_pos[lane][0], PG->geom_pos[lane][1], PG->geom_pos[lane][2]};
                double RB[9], w[3];
                quat2mat(RB, q);
                mulmatvec3(w, RB, lp);
                for (int k = 0; k < 3; ++k) fp[k] = xpe[3 * B + k] + w[k];
                for (int r_ = 0; r_ < 3; ++r_)
                    for (int c_ = 0; c_ < 3; ++c_)
                        fR[3 * r_ + c_] = RB[3 * r_] * PG->geom_mat[lane][c_] + RB[3 * r_ + 1] * PG->geom_mat[lane][3 + c_] + RB[3 * r_ + 2] * PG->geom_mat[lane][6 + c_];
            }
        }
        double best = io.rmax;
        int best_id = -1;
        bool best_inside = false;                           /* the value is `rmin`, taken from inside a solid */
        for (int g = 0; g < m->ngeom; ++g) {              /* (the same trip for every lane: the geom's pose is the wave's, not the lane's) */
            if (!((io.geoms >> g) & 1u)) continue;
            const int gt = m->geom_type[g], gb = m->geom_bodyid[g];
            const bool solid = gt == CM_GEOM_SPHERE || gt == CM_GEOM_CAPSULE || gt == CM_GEOM_BOX;
            if (m->body_weldid[gb] != 0 ? !solid : !(solid || gt == CM_GEOM_PLANE || gt == CM_GEOM_HFIELD)) continue;
            double gp[3], R[9], og[3], dg[3];
            for (int k = 0; k < 3; ++k) gp[k] = wv::readlane(fp[k], g);
            for (int k = 0; k < 9; ++k) R[k] = wv::readlane(fR[k], g);
            const double rel[3] = {o[0] - gp[0], o[1] - gp[1], o[2] - gp[2]};
            double t = io.rmax + 1.0;
            bool inside = false;
            bool live = mine && gb != rbody;                /* (a lane past the table's end has no ray; a ray does not see its own body) */
            if (solid) {
                /* the bounding sphere (the sphere itself): who meets it at all, in range and in front of the best so far */
                const double rb = gt == CM_GEOM_SPHERE ? m->geom_size[g][0] : m->geom_rbound[g] + DEPTH_CULL_PAD;
                double e0 = 0.0, e1 = 0.0;
                const bool meets = live && depth_ray_round(rel, D, DD, rb * rb, &e0, &e1) && e1 >= io.rmin && e0 < best;
                if (wv::ballot(meets) == 0ull) continue;
                if (gt == CM_GEOM_SPHERE) {
                    if (meets) t = depth_convex(e0, e1, io.rmin, t);
                    if (t >= io.rmin && t < best) { best = t; best_id = g; best_inside = e0 < io.rmin; }
                    continue;
                }
                live = meets;
            }
            mulmatTvec3(og, R, rel);
            mulmatTvec3(dg, R, D);
            if (!live) {
            } else if (gt == CM_GEOM_PLANE) {
                if (dg[2] != 0.0) t = -og[2] / dg[2];
            } else if (gt == CM_GEOM_BOX) {
                double t0 = -1e300, t1 = 1e300;
                bool within = true;
                for (int k = 0; k < 3; ++k) {
                    const double s = m->geom_size[g][k];
                    if (dg[k] != 0.0) {
                        const double ta = (-s - og[k]) / dg[k], tb = (s - og[k]) / dg[k];
                        const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
                        t0 = lo > t0 ? lo : t0; t1 = hi < t1 ? hi : t1;
                    } else if (fabs(og[k]) > s) within = false;
                }
                if (within && t0 <= t1) { t = depth_convex(t0, t1, io.rmin, t); inside = t0 < io.rmin; }
            } else if (gt == CM_GEOM_CAPSULE) {
                double t0, t1;
                if (depth_ray_capsule(og, dg, m->geom_size[g][0], m->geom_size[g][1], &t0, &t1)) { t = depth_convex(t0, t1, io.rmin, t); inside = t0 < io.rmin; }
            } else if (grid && m->hfield_nrow >= 2 && m->hfield_ncol >= 2) {
                t = depth_ray_hfield(grid, m->hfield_nrow, m->hfield_ncol, m->hfield_size[0], m->hfield_size[1], m->hfield_size[2], og, dg,
                                     io.rmin, io.rmax);
            }
            if (t >= io.rmin && t < best) { best = t; best_id = g; best_inside = inside; }
        }
        if (mine) io.out[(size_t)env * io.sout + j] = best;
        if (io.ids && mine) io.ids[(size_t)env * io.nrays + j] = best_id;
        if (io.normals) {                                   /* (wave-uniform) */
            /* the frame of the geom this lane's ray met, from that geom's lane */
            const int src = best_id >= 0 ? best_id : 0;
            double gp[3], R[9], og[3], dg[3], nl[3] = {0.0, 0.0, 0.0}, nw[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < 3; ++k) gp[k] = wv::shfl(fp[k], src);
            for (int k = 0; k < 9; ++k) R[k] = wv::shfl(fR[k], src);
            if (best_id >= 0 && !best_inside) {
                const int gt = m->geom_type[src];
                const double rel[3] = {o[0] - gp[0], o[1] - gp[1], o[2] - gp[2]};
                mulmatTvec3(og, R, rel);
                mulmatTvec3(dg, R, D);
                const double p[3] = {og[0] + best * dg[0], og[1] + best * dg[1], og[2] + best * dg[2]};
                if (gt == CM_GEOM_PLANE) nl[2] = 1.0;
                else if (gt == CM_GEOM_SPHERE) { nl[0] = p[0]; nl[1] = p[1]; nl[2] = p[2]; }
                else if (gt == CM_GEOM_CAPSULE) {
                    const double h = m->geom_size[src][1];
                    nl[0] = p[0]; nl[1] = p[1]; nl[2] = p[2] - (p[2] > h ? h : (p[2] < -h ? -h : p[2]));
                } else if (gt == CM_GEOM_BOX) {
                    const int axis = ray_box_face(og, dg, m->geom_size[src][0], m->geom_size[src][1], m->geom_size[src][2]);
                    nl[0] = axis == 0 ? 1.0 : 0.0; nl[1] = axis == 1 ? 1.0 : 0.0; nl[2] = axis == 2 ? 1.0 : 0.0;
                } else if (grid && m->hfield_nrow >= 2 && m->hfield_ncol >= 2) {
                    ray_hfield_normal(grid, m->hfield_nrow, m->hfield_ncol, m->hfield_size[0], m->hfield_size[1], m->hfield_size[2], p, nl);
                }
                const double len = sqrt(dot3(nl, nl));
                /* against the ray (n . u <= 0); a NaN or a length of zero leaves the zero vector */
                const double sgn = len > 0.0 ? (dot3(nl, dg) > 0.0 ? -1.0 / len : 1.0 / len) : 0.0;
                if (sgn != 0.0) {
                    for (int k = 0; k < 3; ++k) nl[k] *= sgn;
                    mulmatvec3(nw, R, nl);
                }
            }
            if (mine) {
                double *dst = io.normals + ((size_t)env * io.nrays + j) * 3;
                dst[0] = nw[0]; dst[1] = nw[1]; dst[2] = nw[2];
            }
        }
        if (clamped && block == 0 && lane == 0) wv::atomic_or(io.warn + env, WARN_TERRAIN_INDEX);
    }
}

}  // namespace ck
#endif
