/*
 * scene_rays.h -- a ray against the scene's geoms, for every kernel that casts rays: the depth images (depth_kernel.h) and the range
 * sensors (ray_kernel.h).  It holds the intersection routines (triangle, height field, sphere and circle, capsule; the box's is
 * ray_box of surface_kernels.h, which the height scan uses too), the value a convex solid gives a ray, the normal of the height
 * field's surface, the world frame of a geom (scene_geom_frame), the cull of the solids (scene_ray_bound) and the test of one ray
 * against one geom (scene_ray_geom).  One copy of each: a grazing-ray rule, a new geom type or another cull pad is changed here and
 * holds for every kernel.  One piece is left UNSHARED, for speed: the sphere's shortcut behind the cull, three lines in each kernel's
 * geom loop (the comment of scene_ray_bound says why).  The functions take values -- pointers, doubles, flags -- never a kernel's argument struct: inlined into the static depth
 * kernel, a function that is handed the struct has the compiler fetch the launch arguments in other portions and costs that kernel six
 * more parked scalars; these cost it none.  Written with the wv:: primitives only; the wave emulator runs the same text.
 */
#ifndef CASSIE_SCENE_RAYS_H
#define CASSIE_SCENE_RAYS_H

#include "surface_kernels.h"

namespace ck {

/* slack of the tests that decide which piece of a surface a ray meets: a ray through an edge shared by two triangles must not slip
 * between them (barycentric coordinates, dimensionless), a cell whose corners touch the ray's z-interval is not skipped (metres) */
constexpr double DEPTH_EDGE_EPS = 1e-12, DEPTH_CULL_PAD = 1e-9;

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

/* The ray (geom frame) against the height field `grid`: the first hit in [tn, tf], or tf + 1 where there is none.  The ray is clipped
 * to [tn, tf] and to the box [-sx, sx] x [-sy, sy] x [0, sz] (elevations are 0 .. 1); the cells under the clipped segment are walked in
 * order from the cell of its start (a step across the x or the y grid line, whichever the ray meets first); a cell whose four corners
 * all lie above or all below the ray's z-interval within the cell is skipped, else its triangles v00 v10 v01 and v11 v01 v10 are
 * intersected (either face) and the nearer hit within [tn, tf] ends the walk: a hit lies inside its cell, so it is in front of
 * everything the cells behind hold.  Every grid read is of a clamped cell and the walk is capped at ncol + nrow steps, so a state of
 * NaNs reads nothing out of bounds and ends. */
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

/* The roots of |o + t d|^2 = r2 for a ray with d.d = dd (2-D: pass z components of zero): false where there are none.  Solved about
 * the ray's point of closest approach, tc = -(o.d) / (d.d), q = o + tc d, t = tc -+ sqrt((r^2 - q.q) / (d.d)): r^2 - q.q is a
 * difference of terms of the size of r^2, not of |o|^2. */
WV_DEVICE bool depth_ray_round(const double *o, const double *d, double dd, double r2, double *ta, double *tb) {
    const double tc = -dot3(o, d) / dd;
    const double q[3] = {o[0] + tc * d[0], o[1] + tc * d[1], o[2] + tc * d[2]};
    const double h2 = r2 - dot3(q, q);
    if (!(h2 >= 0.0)) return false;
    const double s = sqrt(h2 / dd);
    *ta = tc - s; *tb = tc + s;
    return true;
}

/* The interval of the ray (geom frame) within the capsule of radius r, half-length h along z: false where it misses.  The capsule is
 * the cylinder side (the circle in x, y, a root kept where |z| <= h) and the two spheres at z = -+h: the interval runs from the smallest
 * to the largest of the roots kept; a ray along the axis (dx^2 + dy^2 == 0) has the spheres alone. */
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

/* the value a convex solid met over [t0, t1] gives the ray: the entry, `near` where the near plane cuts the solid, else `miss` */
WV_DEVICE double depth_convex(double t0, double t1, double znear, double miss) { return t0 >= znear ? t0 : (t1 >= znear ? znear : miss); }

/* The world frame (position fp, rotation fR, row-major) of geom g where a kernel sees it: static_geom_pose for a geom of a body
 * welded to the world, else the body's pose as the last step launch or forward pass stored it (xpos / xquat: the env's rows, used as
 * stored) composed with the geom's own pose from PG.  The rows are read for a moving geom only and must be there for one: a kernel
 * that may run without body poses (the scene kernel) does not call this for a moving geom then, whose frame stays the zeros it set
 * -- the test is the caller's because the range sensors, which always have their rows, paid for one in here with two more parked
 * scalars and a dozen moves per job.  A kernel has lane g build geom g's frame once per job and its geom loop, whose index is wave-uniform, read
 * it with wv::readlane -- 24 v_readlane_b32 into scalars per geom, no LDS, no barrier. */
WV_DEVICE void scene_geom_frame(ModelPtr m, ParamPtr PG, int g, const double *xpos, const double *xquat, double *fp, double *fR) {
    const int B = m->geom_bodyid[g];
    if (m->body_weldid[B] == 0) static_geom_pose(m, PG, g, fp, fR);
    else {
        const double *xp = xpos + 3 * B, *xq = xquat + 4 * B;
        const double q[4] = {xq[0], xq[1], xq[2], xq[3]}, lp[3] = {PG->geom_pos[g][0], PG->geom_pos[g][1], PG->geom_pos[g][2]};
        double RB[9], w[3];
        quat2mat(RB, q);
        mulmatvec3(w, RB, lp);
        for (int k = 0; k < 3; ++k) fp[k] = xp[k] + w[k];
        for (int r_ = 0; r_ < 3; ++r_)
            for (int c_ = 0; c_ < 3; ++c_)
                fR[3 * r_ + c_] = RB[3 * r_] * PG->geom_mat[g][c_] + RB[3 * r_ + 1] * PG->geom_mat[g][3 + c_] + RB[3 * r_ + 2] * PG->geom_mat[g][6 + c_];
    }
}

/* THE CULL of a solid (sphere, capsule, box), made in the world frame ahead of the rotations into the geom's: whether the lane's ray
 * o + t D (D.D = DD) meets the bounding sphere of geom g at gp -- the sphere itself, else geom_rbound + DEPTH_CULL_PAD -- over an
 * interval [*e0, *e1] that reaches `near` and starts in front of the lane's `best` so far; false for a lane that is not `live` (no
 * ray, or a geom the ray leaves out).  The caller skips the geom where wv::ballot of this is zero (a uniform branch) and hands the
 * answer on to scene_ray_geom as its `live`.  The solid lies inside the bound, so the cull changes no value; for the sphere the bound
 * (unpadded) is the test, and [*e0, *e1] the interval depth_convex takes.  The size and the bounding radius are the model's, at a
 * wave-uniform address: scalar loads.  A NaN pose fails every comparison: the geom is unseen.
 * THE SPHERE'S SHORTCUT behind it -- value, comparison with the best so far, on to the next geom -- is NOT shared: it stays in each
 * kernel's geom loop (depth_jobs.inc, ray_kernel.h), three lines.  As an early return of scene_ray_geom it joined the caller's one
 * comparison, the compiler carried a flag through the loop body and branched on it once more per geom, and the scene kernel's
 * launch alone measured 1.4 % slower than with the shortcut in the loop. */
WV_DEVICE bool scene_ray_bound(ModelPtr m, int g, const double *rel, const double *D, double DD, bool live, double near, double best, double *e0, double *e1) {
    const double rb = m->geom_type[g] == CM_GEOM_SPHERE ? m->geom_size[g][0] : m->geom_rbound[g] + DEPTH_CULL_PAD;
    *e0 = 0.0; *e1 = 0.0;
    return live && depth_ray_round(rel, D, DD, rb * rb, e0, e1) && *e1 >= near && *e0 < best;
}

/* The lane's ray rel + t D (world axes, origin at the geom's position) against geom g, whose rotation is R, for every geom but the sphere: where the ray meets it,
 * `t` as handed in (the caller's far + 1) where it does not, for a lane that is not `live` too (for a solid: scene_ray_bound's answer); *inside says that the value
 * is `near` taken from inside a solid.  The caller keeps the smallest t in [near, best).  Taken into the geom's frame,
 *   plane          t = -o_z / D_z, from either side;
 *   box            the slab test (ray_box);
 *   capsule        depth_ray_capsule, where CAPSULES is set (the static depth kernel never meets one);
 *   height field   depth_ray_hfield on `grid` (null: no samples, a miss).
 * A solid is convex: the ray meets it over an interval [t0, t1] and takes t0 where t0 >= near, `near` where t0 < near <= t1, nothing
 * otherwise (depth_convex).  Nothing is indexed by a pose's values: NaNs fail the comparisons and the geom is unseen. */
template <bool CAPSULES>
WV_DEVICE double scene_ray_geom(ModelPtr m, int g, const double *R, const double *rel, const double *D, bool live, double near, double far,
                                double t, const float *grid, bool *inside_out) {
    const int gt = m->geom_type[g];
    double og[3], dg[3];
    bool inside = false;
    mulmatTvec3(og, R, rel);
    mulmatTvec3(dg, R, D);
    if (!live) {
    } else if (gt == CM_GEOM_PLANE) {
        if (dg[2] != 0.0) t = -og[2] / dg[2];
    } else if (gt == CM_GEOM_BOX) {
        double t0, t1;
        int axis;
        if (ray_box(og, dg, m->geom_size[g][0], m->geom_size[g][1], m->geom_size[g][2], &t0, &t1, &axis)) { t = depth_convex(t0, t1, near, t); inside = t0 < near; }
    } else if (CAPSULES && gt == CM_GEOM_CAPSULE) {
        double t0, t1;
        if (depth_ray_capsule(og, dg, m->geom_size[g][0], m->geom_size[g][1], &t0, &t1)) { t = depth_convex(t0, t1, near, t); inside = t0 < near; }
    } else if (grid && m->hfield_nrow >= 2 && m->hfield_ncol >= 2) {
        t = depth_ray_hfield(grid, m->hfield_nrow, m->hfield_ncol, m->hfield_size[0], m->hfield_size[1], m->hfield_size[2], og, dg, near, far);
    }
    *inside_out = inside;
    return t;
}

}  // namespace ck
#endif
