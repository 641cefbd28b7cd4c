/*
 * depth_kernel.h -- the egocentric depth image (phys_batch_depth_image, include/cassie_phys.h: the definition is there): one ray
 * per pixel of a pinhole camera mounted on a body, against the env's static collision geometry (cassie_depth_kernel) or against any
 * chosen set of its collision geoms, the moving bodies' included (cassie_depth_scene_kernel).  Written with the wv:: primitives only,
 * workgroups of one wave: phys_batch.hip launches them, the wave emulator (tests/emu/emu_depth.cpp, emu_depth_scene.cpp) runs the same
 * text.
 */
#ifndef CASSIE_DEPTH_KERNEL_H
#define CASSIE_DEPTH_KERNEL_H

#include "surface_kernels.h"

namespace ck {

/* A job is (env, tile of DEPTH_TILE x DEPTH_TILE pixels), lane l of the wave the tile's pixel (l / 8, l % 8): the 64 rays of a wave
 * leave through neighbouring pixels and walk neighbouring cells of the grid, so their loops are of similar length and their reads
 * share cache lines.  A fixed grid of DEPTH_GRID workgroups walks the job list of the env range, tiles of one env next to each other.
 * The grid's size and the tile's shape are first choices: DESIGN 4.3 has what the launch was measured to cost with them, and no
 * other size or shape has been tried.
 *
 * Per job, the same in every lane: the body's world pose from qpos (static_body_pose, as the height scan), the camera's world pose,
 * and -- geom by geom -- the static geom's world pose (static_geom_pose).  Per lane: the pixel's ray o + t D, D = R_cam d with
 * d = (a T (2 (c + 1/2) / W - 1), T (1 - 2 (r + 1/2) / H), -1) NOT normalised (t is the depth along the optical axis), taken into
 * the geom's frame, and there
 *   plane          t = -o_z / D_z, from either side;
 *   box            slab test: the entry t0, or `near` where the origin is inside (t0 < near <= t1);
 *   height field   the ray is clipped to [near, far] and to the box [-sx, sx] x [-sy, sy] x [0, sz] (elevations are 0 .. 1); the cells
 *                  under the clipped segment are walked in order from the cell of its start (a step across the x or the y grid line,
 *                  whichever the ray meets first); a cell whose four corners all lie above or all below the ray's z-interval within
 *                  the cell is skipped, else its triangles v00 v10 v01 and v11 v01 v10 are intersected (either face) and the nearer hit
 *                  within [near, far] ends the walk: a hit lies inside its cell, so it is in front of everything the cells behind hold.
 * The value is the smallest t over the geoms, `far` where there is none.  Every grid read is of a clamped cell and the walk is capped
 * at ncol + nrow steps, so a state of NaNs reads nothing out of bounds and ends. */
constexpr int DEPTH_GRID = 2048, DEPTH_TILE = 8, DEPTH_MAXPIXELS = 16384;
/* slack of the tests that decide which piece of a surface a ray meets: a ray through an edge shared by two triangles must not slip
 * between them (barycentric coordinates, dimensionless), a cell whose corners touch the ray's z-interval is not skipped (metres) */
constexpr double DEPTH_EDGE_EPS = 1e-12, DEPTH_CULL_PAD = 1e-9;

/* THE SCENE KERNEL (cassie_depth_scene_kernel) renders the geoms of the mask DepthIO::geoms: besides the static planes, boxes and
 * height field also spheres and capsules, and spheres, capsules and boxes on moving bodies, whose world pose is that of the body as
 * the last step launch or forward pass stored it (xpos / xquat, used as stored) composed with the geom's own pose from PG.  It is the
 * same per-pixel body as the static kernel's (depth_jobs.inc, with a compile-time switch): the static kernel keeps its text.
 *
 * The geoms' world frames are needed once per job, not once per lane: lane g builds geom g's (position and rotation, 12 doubles) and
 * the geom loop, whose index is wave-uniform, reads them with wv::readlane -- 24 v_readlane_b32 into scalars per rendered geom, no
 * LDS, no barrier, nothing to allocate at launch, and the emulator runs it as it stands.  (LDS would cost a write, a wait and 24
 * ds_reads per geom and lane for values that are the wave's, not the lane's.)  The size and the bounding radius are the model's, at a
 * wave-uniform address: scalar loads, not lane reads.
 *
 * A solid (sphere, capsule, box) is convex: the ray meets it over an interval [t0, t1], and the pixel takes t0 where t0 >= near, `near`
 * where t0 < near <= t1, nothing otherwise.  A lane runs a solid's test only where its ray meets the geom's bounding sphere
 * (geom_rbound + DEPTH_CULL_PAD) over an interval that reaches `near` and starts in front of the lane's best so far; a wave in which
 * no lane does skips the geom (wv::ballot, a uniform branch).  The solid lies inside the bound, so the cull changes no value; for the
 * sphere the bound (unpadded) is the test.  The quadratics are solved about the ray's point of closest approach, tc = -(o.d) / (d.d),
 * q = o + tc d, t = tc -+ sqrt((r^2 - q.q) / (d.d)): r^2 - q.q is a difference of terms of the size of r^2, not of |o|^2.  The
 * capsule is the cylinder side (the same in x, y, a root kept where |z| <= h) and the two spheres at z = -+h: the interval runs from
 * the smallest to the largest of the roots kept; a ray along the axis (dx^2 + dy^2 == 0) has the spheres alone.  A NaN pose fails
 * every comparison: the geom is unseen, and nothing is indexed by these values. */

struct DepthIO {
    const cm_model_t *models; int model_stride;
    const cm_envparams_t *envparams;   /* null, or one block per env (PhysIO::envparams) */
    int env0, n, body, width, height;
    double tan_half, znear, zfar;      /* tan(fovy / 2) */
    double cam_pos[3], cam_quat[4];    /* the camera in the body's frame, shared by the envs ... */
    const double *pose;                /* ... or null / [nenv][7] (pos, quat) per env, indexed by the absolute env */
    const double *qpos; int sq;
    double *out; int sout;             /* [nenv][height * width] with a row stride in doubles */
    const float *hfield; size_t hfield_stride; const int *hfield_index; int hfield_nterrain;   /* as in PhysIO */
    int *warn;
    /* the scene kernel's (all zero: the static kernel's behaviour) */
    unsigned geoms;                    /* bit g: compiled geom g is rendered */
    const double *xpos, *xquat;        /* [nenv][nbody][3 / 4] body poses in the world, rows sxp / sxq doubles apart */
    int sxp, sxq;
    int *ids;                          /* null, or [nenv][height * width]: the geom that gave the value, -1 where it is `far` */
};

/* the ray o + t d against the triangle a, a + e1, a + e2 (Moeller-Trumbore, either face): t, or -1 where it misses */
WV_DEVICE double depth_ray_triangle(const double *o, const double *d, const double *a, const double *e1, const double *e2) {
    double p[3], s[3], q[3];
    cross3(p, d, e2);
    const double det = dot3(e1, p);
    if (det == 0.0) return -1.0;
    const double inv = 1.0 / det;
    for (int k = 0; k < 3; ++k) s[k] = o[k] - a[k];
    const double u = dot3(s, p) * inv;
    cross3(q, s, e1);
    const double v = dot3(d, q) * inv;
    if (!(u >= -DEPTH_EDGE_EPS && v >= -DEPTH_EDGE_EPS && u + v <= 1.0 + DEPTH_EDGE_EPS)) return -1.0;
    return dot3(e2, q) * inv;
}

/* floor(x) clamped to the cells 0 .. last, the clamp made in double ahead of the conversion (a NaN gives cell 0) */
WV_DEVICE int depth_cell(double x, int last) {
    const double f = floor(x);
    return f >= 0.0 ? (f < (double)last ? (int)f : last) : 0;
}

/* the ray (geom frame) against the height field `grid`: the first hit in [tn, tf], or tf + 1 where there is none */
WV_DEVICE double depth_ray_hfield(const float *grid, int nr, int nc, double sx, double sy, double sz, const double *o, const double *d,
                                  double tn, double tf) {
    const double miss = tf + 1.0;
    /* the clip: [tn, tf] and the three slabs of the box */
    double t0 = tn, t1 = tf;
    const double lo[3] = {-sx, -sy, 0.0}, hi[3] = {sx, sy, sz};
    for (int k = 0; k < 3; ++k) {
        if (d[k] != 0.0) {
            const double ta = (lo[k] - o[k]) / d[k], tb = (hi[k] - o[k]) / d[k];
            const double a = ta < tb ? ta : tb, b = ta < tb ? tb : ta;
            t0 = a > t0 ? a : t0; t1 = b < t1 ? b : t1;
        } else if (!(o[k] >= lo[k] && o[k] <= hi[k])) return miss;
    }
    if (!(t0 <= t1)) return miss;
    const double cx = 2 * sx / (nc - 1), cy = 2 * sy / (nr - 1);
    /* the cell of the segment's start, then a step at a time */
    const int j0 = depth_cell((o[0] + t0 * d[0] + sx) / cx, nc - 2), i0 = depth_cell((o[1] + t0 * d[1] + sy) / cy, nr - 2);
    int j = j0, i = i0;
    const int dj = d[0] > 0.0 ? 1 : -1, di = d[1] > 0.0 ? 1 : -1;
    double tin = t0;
    for (int step = 0; step < nc + nr; ++step) {
        /* where the ray leaves the cell: the next x or y grid line ahead of it */
        const double tx = d[0] != 0.0 ? ((-sx + (j + (dj > 0 ? 1 : 0)) * cx) - o[0]) / d[0] : 1e300;
        const double ty = d[1] != 0.0 ? ((-sy + (i + (di > 0 ? 1 : 0)) * cy) - o[1]) / d[1] : 1e300;
        const double tnext = tx < ty ? tx : ty, tout = tnext < t1 ? tnext : t1;
        const double h00 = sz * grid[i * nc + j], h10 = sz * grid[i * nc + j + 1];
        const double h01 = sz * grid[(i + 1) * nc + j], h11 = sz * grid[(i + 1) * nc + j + 1];
        const double za = o[2] + tin * d[2], zb = o[2] + tout * d[2];
        const double zlo = (za < zb ? za : zb) - DEPTH_CULL_PAD, zhi = (za < zb ? zb : za) + DEPTH_CULL_PAD;
        const double hmin = fmin(fmin(h00, h10), fmin(h01, h11)), hmax = fmax(fmax(h00, h10), fmax(h01, h11));
        if (zlo <= hmax && zhi >= hmin) {
            const double x0 = -sx + j * cx, y0 = -sy + i * cy;
            const double v00[3] = {x0, y0, h00}, v11[3] = {x0 + cx, y0 + cy, h11};
            const double a1[3] = {cx, 0.0, h10 - h00}, a2[3] = {0.0, cy, h01 - h00};       /* v10 - v00, v01 - v00 */
            const double b1[3] = {-cx, 0.0, h01 - h11}, b2[3] = {0.0, -cy, h10 - h11};     /* v01 - v11, v10 - v11 */
            const double ta = depth_ray_triangle(o, d, v00, a1, a2), tb = depth_ray_triangle(o, d, v11, b1, b2);
            const bool oka = ta >= tn && ta <= tf, okb = tb >= tn && tb <= tf;
            if (oka || okb) return oka && (!okb || ta <= tb) ? ta : tb;
        }
        if (!(tnext < t1)) break;
        if (tx < ty) j += dj; else i += di;
        if (j < 0 || j > nc - 2 || i < 0 || i > nr - 2) break;
        tin = tnext;
    }
    return miss;
}

/* the roots of |o + t d|^2 = r2 for a ray with d.d = dd (2-D: pass z components of zero): false where there are none */
WV_DEVICE bool depth_ray_round(const double *o, const double *d, double dd, double r2, double *ta, double *tb) {
    const double tc = -dot3(o, d) / dd;
    const double q[3] = {o[0] + tc * d[0], o[1] + tc * d[1], o[2] + tc * d[2]};
    const double h2 = r2 - dot3(q, q);
    if (!(h2 >= 0.0)) return false;
    const double s = sqrt(h2 / dd);
    *ta = tc - s; *tb = tc + s;
    return true;
}

/* the interval of the ray (geom frame) within the capsule of radius r, half-length h along z: false where it misses */
WV_DEVICE bool depth_ray_capsule(const double *o, const double *d, double r, double h, double *t0, double *t1) {
    double lo = 1e300, hi = -1e300, ta, tb;
    const double r2 = r * r, dd = dot3(d, d), a = d[0] * d[0] + d[1] * d[1];
    const double o2[3] = {o[0], o[1], 0.0}, d2[3] = {d[0], d[1], 0.0};
    if (a != 0.0 && depth_ray_round(o2, d2, a, r2, &ta, &tb)) {
        if (fabs(o[2] + ta * d[2]) <= h) { lo = ta < lo ? ta : lo; hi = ta > hi ? ta : hi; }
        if (fabs(o[2] + tb * d[2]) <= h) { lo = tb < lo ? tb : lo; hi = tb > hi ? tb : hi; }
    }
    for (int e = 0; e < 2; ++e) {
        const double oc[3] = {o[0], o[1], e ? o[2] - h : o[2] + h};
        if (depth_ray_round(oc, d, dd, r2, &ta, &tb)) { lo = ta < lo ? ta : lo; hi = tb > hi ? tb : hi; }
    }
    *t0 = lo; *t1 = hi;
    return lo <= hi;
}

/* the value a convex solid met over [t0, t1] gives the pixel: the entry, `near` where the near plane cuts the solid, else `miss` */
WV_DEVICE double depth_convex(double t0, double t1, double znear, double miss) { return t0 >= znear ? t0 : (t1 >= znear ? znear : miss); }

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_depth_kernel(DepthIO io) {
    constexpr bool SCENE = false;
#include "depth_jobs.inc"
}
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_depth_scene_kernel(DepthIO io) {
    constexpr bool SCENE = true;
#include "depth_jobs.inc"
}

}  // namespace ck
#endif
