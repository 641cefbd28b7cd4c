/*
 * surface_kernels.h -- what the kernels that look at an env's static geometry share, and the first of them: the world pose of a body
 * from qpos alone and of a static geom (static_body_pose, static_geom_pose), a ray against a box (ray_box), the surface under a world
 * point (scan_surface), which model and which geometry block an env reads (env_model, env_geometry), the heading of a quaternion
 * (quat_heading), and the height scan (cassie_scan_kernel).  Included by scene_rays.h (a ray against the scene's geoms: the depth
 * images and the range sensors build on that) and episode_kernels.h (placed restarts); the step kernel's own translation units
 * (kernels_*.hip) do not need it.  The launch records, grids and checks are small_launch.h's.
 */
#ifndef CASSIE_SURFACE_KERNELS_H
#define CASSIE_SURFACE_KERNELS_H

#include "physics_kernel.h"

namespace ck {

/* What a kernel reads of env `env`: the env's model (one shared by the envs, stride 0, or one each), and the block its geoms' poses come
 * from -- the env's own once the batch has randomised geometry (cm_model_t::env_geom: the step kernel's gate), else the model's.  They
 * take the argument struct's fields, not the struct: a kernel that hands its arguments on by reference fetches them in other portions,
 * which cost the static depth kernel scalar registers (depth_jobs.inc).  The env's terrain is terrain_grid's (pk_types.h) */
WV_DEVICE ModelPtr env_model(const cm_model_t *models, int model_stride, int env) { return (ModelPtr)(models + (size_t)env * model_stride); }
WV_DEVICE ParamPtr env_geometry(const cm_envparams_t *envparams, ModelPtr m, size_t env) { return (envparams && m->env_geom) ? (ParamPtr)(envparams + env) : (ParamPtr)&m->params; }

/* The heading of a body with world quaternion q: cos and sin of its yaw about world z ((1, 0) where its x axis is vertical) */
WV_DEVICE void quat_heading(const double *q, double &cy, double &sy) {
    const double ys = 2.0 * (q[0] * q[3] + q[1] * q[2]), yc = 1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3]);
    const double yn = sqrt(ys * ys + yc * yc);
    cy = yn > 0.0 ? yc / yn : 1.0; sy = yn > 0.0 ? ys / yn : 0.0;
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

/* The slab test: the interval [t0, t1] over which the ray o + t d, given in a box's frame, lies within the box of half-sizes s0, s1, s2,
 * and the axis whose slab it enters last -- the face of the entry t0 (the first of equals).  False where it misses the box, a ray
 * parallel to a slab that lies outside it included.  The one slab test of the kernels that look at the scene: the height scan and the
 * placed restart (scan_surface: the exit t1 of a vertical line), the depth images and the range sensors (scene_rays.h: the entry, and
 * the face for the normal) */
WV_DEVICE bool ray_box(const double *o, const double *d, double s0, double s1, double s2, double *t0_out, double *t1_out, int *axis_out) {
    const double size[3] = {s0, s1, s2};
    double t0 = -1e300, t1 = 1e300;
    int axis = 0;
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
        const double s = size[k];
        if (d[k] != 0.0) {
            const double ta = (-s - o[k]) / d[k], tb = (s - o[k]) / d[k];
            const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
            if (lo > t0) { t0 = lo; axis = k; }
            t1 = hi < t1 ? hi : t1;
        } else if (fabs(o[k]) > s) inside = false;
    }
    *t0_out = t0; *t1_out = t1; *axis_out = axis;
    return inside && t0 <= t1;
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
            double t0, t1;
            int axis;
            if (ray_box(o, R + 6, m->geom_size[g][0], m->geom_size[g][1], m->geom_size[g][2], &t0, &t1, &axis)) { has = true; z = t1; }
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
        const ModelPtr m = env_model(io.models, io.model_stride, env);
        const ParamPtr PG = env_geometry(io.envparams, m, (size_t)env);
        const double *q = io.qpos + (size_t)env * io.sq;
        double bp[3], bq[4], cy, sy;
        static_body_pose(m, io.body, q, bp, bq);                  /* (wave-uniform) */
        quat_heading(bq, cy, sy);
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
