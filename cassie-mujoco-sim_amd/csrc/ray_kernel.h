/*
 * ray_kernel.h -- range sensors on any body (phys_batch_rays_cast, include/cassie_phys.h: the definition is there): a table of rays,
 * each attached to a body of its own in one of three frames, against any chosen set of the env's collision geoms, the moving bodies'
 * included -- the range, the geom hit and the surface normal.  It holds the table, the ray's construction from its body's pose, the
 * self-exclusion and the normal; the geoms' world frames and the ray against a geom are scene_rays.h's, as for the depth images.
 * The ray's origin, direction and body are the lane's and not the wave's.  Written with the wv:: primitives only, workgroups of one
 * wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_rays.cpp) runs the same text.
 */
#ifndef CASSIE_RAY_KERNEL_H
#define CASSIE_RAY_KERNEL_H

#include "scene_rays.h"

namespace ck {

/* A job is (env, block of 64 rays of the table), lane l of the wave the block's ray l: a fixed grid of RAYS_GRID workgroups walks the
 * job list of the env range, the blocks of one env next to each other (a first choice, like the depth image's: DESIGN 4.3 has what the
 * launch was measured to cost with it).
 *
 * Per job, lane g builds the world frame of geom g (scene_geom_frame, from the env's rows of xpos / xquat) and the geom loop, whose
 * index is wave-uniform, reads it with wv::readlane.  Per lane: the ray's body pose, read from xpos / xquat as stored, the ray o + t u
 * in the world (u is the table's unit direction turned by the body's rotation, by its heading, or not at all), and -- geom by geom --
 * the solids' cull (scene_ray_bound), the sphere's shortcut and scene_ray_geom, near = rmin, far = rmax.  A lane leaves out the geoms
 * of its own ray's body: it is not live for them.  The loop keeps the value, the geom and whether the value is `rmin` taken from inside a solid.
 *
 * The normal is worked out once, behind the loop, from the hit point: the winning geom's frame comes from its lane (wv::shfl: the
 * geom is the lane's own here), the ray goes into that frame once more, and
 *   plane          -+ z, against the ray;
 *   box            the slab test again (ray_box): the axis that gave the entry t0, against the ray;
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
        if (lane < m->ngeom && ((io.geoms >> lane) & 1u)) scene_geom_frame(m, PG, lane, xpe, xqe, fp, fR);
        double best = io.rmax;
        int best_id = -1;
        bool best_inside = false;                           /* the value is `rmin`, taken from inside a solid */
        for (int g = 0; g < m->ngeom; ++g) {              /* (the same trip for every lane: the geom's pose is the wave's, not the lane's) */
            if (!((io.geoms >> g) & 1u)) continue;
            const int gt = m->geom_type[g], gb = m->geom_bodyid[g];
            const bool solid = gt == CM_GEOM_SPHERE || gt == CM_GEOM_CAPSULE || gt == CM_GEOM_BOX;
            if (m->body_weldid[gb] != 0 ? !solid : !(solid || gt == CM_GEOM_PLANE || gt == CM_GEOM_HFIELD)) continue;
            double gp[3], R[9];
            for (int k = 0; k < 3; ++k) gp[k] = wv::readlane(fp[k], g);
            for (int k = 0; k < 9; ++k) R[k] = wv::readlane(fR[k], g);
            const double rel[3] = {o[0] - gp[0], o[1] - gp[1], o[2] - gp[2]};
            double t = io.rmax + 1.0;
            bool live = mine && gb != rbody;                /* (a lane past the table's end has no ray; a ray does not see its own body) */
            if (solid) {
                double e0, e1;
                const bool meets = scene_ray_bound(m, g, rel, D, DD, live, io.rmin, best, &e0, &e1);
                if (wv::ballot(meets) == 0ull) continue;
                if (gt == CM_GEOM_SPHERE) {                 /* (the shortcut: the bound is the test; kept in the loop, scene_rays.h says why) */
                    if (meets) t = depth_convex(e0, e1, io.rmin, t);
                    if (t >= io.rmin && t < best) { best = t; best_id = g; best_inside = e0 < io.rmin; }
                    continue;
                }
                live = meets;
            }
            bool inside;
            t = scene_ray_geom<true>(m, g, R, rel, D, live, io.rmin, io.rmax, t, grid, &inside);
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
                    double t0, t1;
                    int axis;
                    ray_box(og, dg, m->geom_size[src][0], m->geom_size[src][1], m->geom_size[src][2], &t0, &t1, &axis);
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
