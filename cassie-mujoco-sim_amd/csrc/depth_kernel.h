/*
 * depth_kernel.h -- the egocentric depth image (phys_batch_depth_image, include/cassie_phys.h: the definition is there): one ray
 * per pixel of a pinhole camera mounted on a body, against the env's static collision geometry.  Written with the wv:: primitives
 * only, workgroups of one wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_depth.cpp) runs the same text.
 */
#ifndef CASSIE_DEPTH_KERNEL_H
#define CASSIE_DEPTH_KERNEL_H

#include "small_kernels.h"

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

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_depth_kernel(DepthIO io) {
    const int lane = wv::lane();
    const int W = io.width, H = io.height;
    const int tiles_x = (W + DEPTH_TILE - 1) / DEPTH_TILE, tiles = tiles_x * ((H + DEPTH_TILE - 1) / DEPTH_TILE);
    const long long njobs = (long long)io.n * tiles;
    for (long long job = wv::env_id(); job < njobs; job += wv::grid_size()) {
        const int env = io.env0 + (int)(job / tiles), tile = (int)(job % tiles);
        const ModelPtr m = (ModelPtr)(io.models + (size_t)env * io.model_stride);
        const ParamPtr PG = (io.envparams && m->env_geom) ? (ParamPtr)(io.envparams + (size_t)env) : (ParamPtr)&m->params;
        /* the camera's world pose (wave-uniform) */
        double bp[3], bq[4], Rb[9], cp[3], cq[4], wq[4], Rc[9], off[3];
        static_body_pose(m, io.body, io.qpos + (size_t)env * io.sq, bp, bq);
        const double *own = io.pose ? io.pose + (size_t)env * 7 : nullptr;
        for (int k = 0; k < 3; ++k) cp[k] = own ? own[k] : io.cam_pos[k];
        for (int k = 0; k < 4; ++k) cq[k] = own ? own[3 + k] : io.cam_quat[k];
        normalize4(cq);
        quat2mat(Rb, bq);
        mulmatvec3(off, Rb, cp);
        mulquat(wq, bq, cq);
        quat2mat(Rc, wq);
        const double o[3] = {bp[0] + off[0], bp[1] + off[1], bp[2] + off[2]};
        /* this lane's pixel and its ray */
        const int r = (tile / tiles_x) * DEPTH_TILE + (lane >> 3), c = (tile % tiles_x) * DEPTH_TILE + (lane & 7);
        const bool mine = r < H && c < W;
        const double aspect = (double)W / (double)H;
        const double dc[3] = {aspect * io.tan_half * (2.0 * (c + 0.5) / W - 1.0), io.tan_half * (1.0 - 2.0 * (r + 0.5) / H), -1.0};
        double D[3];
        mulmatvec3(D, Rc, dc);
        bool clamped;
        const float *grid = terrain_grid(io.hfield, io.hfield_stride, io.hfield_index, io.hfield_nterrain, env, &clamped);
        double best = io.zfar;
        for (int g = 0; g < m->ngeom; ++g) {              /* (the same trip for every lane: the geom's pose is the wave's, not the lane's) */
            const int gt = m->geom_type[g];
            if (m->body_weldid[m->geom_bodyid[g]] != 0 || (gt != CM_GEOM_PLANE && gt != CM_GEOM_BOX && gt != CM_GEOM_HFIELD)) continue;
            double gp[3], R[9], og[3], dg[3];
            static_geom_pose(m, PG, g, gp, R);
            const double rel[3] = {o[0] - gp[0], o[1] - gp[1], o[2] - gp[2]};
            mulmatTvec3(og, R, rel);
            mulmatTvec3(dg, R, D);
            double t = io.zfar + 1.0;
            if (!mine) {                                    /* (a lane past the image's edge has no ray) */
            } else if (gt == CM_GEOM_PLANE) {
                if (dg[2] != 0.0) t = -og[2] / dg[2];
            } else if (gt == CM_GEOM_BOX) {
                double t0 = -1e300, t1 = 1e300;
                bool inside = true;
                for (int k = 0; k < 3; ++k) {
                    const double s = m->geom_size[g][k];
                    if (dg[k] != 0.0) {
                        const double ta = (-s - og[k]) / dg[k], tb = (s - og[k]) / dg[k];
                        const double lo = ta < tb ? ta : tb, hi = ta < tb ? tb : ta;
                        t0 = lo > t0 ? lo : t0; t1 = hi < t1 ? hi : t1;
                    } else if (fabs(og[k]) > s) inside = false;
                }
                if (inside && t0 <= t1) t = t0 >= io.znear ? t0 : (t1 >= io.znear ? io.znear : t);
            } else if (grid && m->hfield_nrow >= 2 && m->hfield_ncol >= 2) {
                t = depth_ray_hfield(grid, m->hfield_nrow, m->hfield_ncol, m->hfield_size[0], m->hfield_size[1], m->hfield_size[2], og, dg,
                                     io.znear, io.zfar);
            }
            if (t >= io.znear && t < best) best = t;
        }
        if (mine) io.out[(size_t)env * io.sout + (size_t)r * W + c] = best;
        if (clamped && tile == 0 && lane == 0) wv::atomic_or(io.warn + env, WARN_TERRAIN_INDEX);
    }
}

}  // namespace ck
#endif
