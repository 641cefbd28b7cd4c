/*
 * obs_kernels.h -- observation rows: the last stage between the batch's fields and the row a policy network reads (phys_batch_obs,
 * include/cassie_phys.h: the definition is there).  A configured list of terms -- slices of any field of the batch or of the caller's own
 * per-env input array, and vectors rotated into the frame of a quaternion of the state -- is evaluated for an env range by ONE launch:
 * gather, offset, counter-based uniform noise, scale, clip, the cast to the rows' type and the shift of a per-env history of frames.
 * Written with the wv:: primitives only, workgroups of one wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_obs.cpp)
 * runs the same text.  The launch record, the column table, the grid and the checks are small_launch.h's (no field of ObsIO is assigned
 * anywhere else).
 *
 * One wave takes an env at a time and OBS_GRID workgroups walk the range (as cassie_probe_kernel's do).  Per env:
 *   lane = column  consecutive lanes take consecutive columns of the frame, 64 at a time (a frame wider than a wave goes in passes), so the
 *                  loads of the column table (one record per column, expanded from the terms on the host once) and the stores of a frame
 *                  are contiguous across the wave.  A lane forms its column's value -- the three lanes of a ROT_INV term each their own
 *                  component, from the same seven loads -- and then shifts the history of ITS column, oldest frame first: a column's
 *                  history never crosses lanes, so the shift needs no barrier and no second buffer.
 *   the noise      Philox4x32-10 on the counter (env_base + env, column, frames[env], 0), in the lanes whose column has noise != 0 only.
 *   the count      frames[env] is read by every lane through lane 0 before anything is stored and written by lane 0 after the last pass.
 * Every arithmetic step of a value is one individually rounded operation (wv::mul_rn / add_rn / sub_rn): the device, the emulator and a
 * numpy restatement (tests/obs_check.py) agree bit for bit.  Vector loads and stores only; an env's wave reads that env's source rows and
 * touches that env's row and count alone.  No stepping kernel is handed any of this.
 */
#ifndef CASSIE_OBS_KERNELS_H
#define CASSIE_OBS_KERNELS_H

#include "physics_kernel.h"

namespace ck {

/* OBS_GRID: the workgroups that walk a range.  A few, like the probes' and the episode kernel's: the launch runs behind a range's step
 * launch while the other range's step kernel fills the chip, where every workgroup waits for a wave slot to free; an env costs one pass
 * of loads and history * ncols stores.  A first choice, by that arithmetic (tools/obs_rate.py measures the call in the loop it is meant for). */
constexpr int OBS_GRID = 64, OBS_MAXCOLS = 2048, OBS_MAXHISTORY = 64, OBS_MAXROW = 65536, OBS_MAXSLOTS = 16;
enum { OBS_COPY = 0, OBS_ROT_INV = 1 };              /* (PHYS_OBS_COPY, PHYS_OBS_ROT_INV of cassie_phys.h) */
constexpr int OBS_INPUT = -1, OBS_CONST = -2;        /* (PHYS_OBS_INPUT, PHYS_OBS_CONST: sources that are no field of the batch) */
constexpr int OBS_F32 = 4, OBS_F64 = 8;              /* (PHYS_OBS_F32, PHYS_OBS_F64: the bytes of an element) */

/* a term as the caller writes it (phys_obs_term_t of cassie_phys.h) */
struct ObsTerm { int kind, field, index, count, qfield, qindex; double vec[3]; double offset, scale, noise, lo, hi; };

/* a column of the frame, expanded from its term: the slot of its source among the call's (-1: the term's vec), the element of the
 * source's row (ROT_INV: of v[0]), the component of a ROT_INV (-1: a COPY) with the slot and first element of its quaternion, the
 * term's vec and the five constants of the column's value */
struct ObsCol { int slot, elem, comp, qslot, qelem, pad; double vec[3]; double offset, scale, noise, lo, hi; };

/* a source of the call: the rows of a field (the batch's own buffer or the caller's bound tensor) or of the caller's input array, the
 * elements between two rows, and whether the elements are floats */
struct ObsSrc { const void *base; long long stride; int f32, pad; };

struct ObsIO {
    int env0, n, ncols, history, f32;   /* f32: the rows are floats */
    unsigned env_base, key0, key1;      /* the counter's offset and the key (seed & 0xffffffff, seed >> 32) */
    const ObsCol *cols;                 /* [ncols] */
    ObsSrc src[OBS_MAXSLOTS];
    void *rows; long long srow;         /* [nenv] rows [history][ncols], srow elements apart */
    unsigned *frames;                   /* [nenv] the calls an env's row has seen (wraps) */
    const int *refill;                  /* [n] or null: non-zero = every frame of the env's row becomes the new one */
};

/* Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds on the counter c with
 * the key k, the key bumped by the Weyl constants between the rounds; out: the four words */
WV_DEVICE void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned *out) {
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
/* uniform on (-1, 1) from a word: (w + 0.5) 2^-31 - 1, every step exact in fp64 */
WV_DEVICE double obs_uniform(unsigned w) { return wv::sub_rn(wv::mul_rn(wv::add_rn((double)w, 0.5), 4.656612873077392578125e-10), 1.0); }

/* element k of an env's row of a source, widened exactly */
WV_DEVICE double obs_load(const ObsSrc &s, size_t env, int k) {
    const size_t at = env * (size_t)s.stride + (size_t)k;
    return s.f32 ? (double)((const float *)s.base)[at] : ((const double *)s.base)[at];
}

/* component comp of R(q)^T v: quat2mat's matrix and mulmatTvec3's sums (pk_math.h), every product and sum rounded on its own, in the
 * order those two routines write them */
WV_DEVICE double obs_rot_inv(const double *q, const double *v, int comp) {
    using namespace wv;
    const double q00 = mul_rn(q[0], q[0]), q11 = mul_rn(q[1], q[1]), q22 = mul_rn(q[2], q[2]), q33 = mul_rn(q[3], q[3]);
    const double q01 = mul_rn(q[0], q[1]), q02 = mul_rn(q[0], q[2]), q03 = mul_rn(q[0], q[3]);
    const double q12 = mul_rn(q[1], q[2]), q13 = mul_rn(q[1], q[3]), q23 = mul_rn(q[2], q[3]);
    double a, b, c;   /* m[comp], m[3 + comp], m[6 + comp] */
    if (comp == 0) { a = sub_rn(sub_rn(add_rn(q00, q11), q22), q33); b = mul_rn(2.0, add_rn(q12, q03)); c = mul_rn(2.0, sub_rn(q13, q02)); }
    else if (comp == 1) { a = mul_rn(2.0, sub_rn(q12, q03)); b = sub_rn(add_rn(sub_rn(q00, q11), q22), q33); c = mul_rn(2.0, add_rn(q23, q01)); }
    else { a = mul_rn(2.0, add_rn(q13, q02)); b = mul_rn(2.0, sub_rn(q23, q01)); c = add_rn(sub_rn(sub_rn(q00, q11), q22), q33); }
    return add_rn(add_rn(mul_rn(a, v[0]), mul_rn(b, v[1])), mul_rn(c, v[2]));
}

WV_DEVICE void obs_env(const ObsIO &io, int i, int lane) {
    const size_t env = (size_t)io.env0 + (size_t)i;
    /* lane 0's reading of the count stands for the wave: nobody stores before every lane has it */
    const unsigned frames = (unsigned)wv::shfl_i((int)io.frames[env], 0);
    const bool fill = frames == 0u || (io.refill && io.refill[i] != 0);
    const int ncols = io.ncols, H = io.history;
    float *const row32 = (float *)io.rows + env * (size_t)io.srow;
    double *const row64 = (double *)io.rows + env * (size_t)io.srow;
    for (int c = lane; c < ncols; c += WV_WAVE) {
        const ObsCol col = io.cols[c];
        double x;
        if (col.comp < 0) x = obs_load(io.src[col.slot], env, col.elem);
        else {
            double q[4], v[3];
            for (int k = 0; k < 4; ++k) q[k] = obs_load(io.src[col.qslot], env, col.qelem + k);
            for (int k = 0; k < 3; ++k) v[k] = col.slot < 0 ? col.vec[k] : obs_load(io.src[col.slot], env, col.elem + k);
            x = obs_rot_inv(q, v, col.comp);
        }
        double e = wv::sub_rn(x, col.offset);
        if (col.noise != 0.0) {
            unsigned w[4];
            philox4x32_10(io.env_base + (unsigned)env, (unsigned)c, frames, 0u, io.key0, io.key1, w);
            e = wv::add_rn(e, wv::mul_rn(col.noise, obs_uniform(w[0])));
        }
        const double y = clampd(wv::mul_rn(e, col.scale), col.lo, col.hi);
        /* the history of this column, oldest frame first; then the new frame */
        if (io.f32) {
            const float y32 = (float)y;
            for (int h = H - 1; h >= 1; --h) row32[(size_t)h * ncols + c] = fill ? y32 : row32[(size_t)(h - 1) * ncols + c];
            row32[c] = y32;
        } else {
            for (int h = H - 1; h >= 1; --h) row64[(size_t)h * ncols + c] = fill ? y : row64[(size_t)(h - 1) * ncols + c];
            row64[c] = y;
        }
    }
    if (lane == 0) io.frames[env] = frames + 1u;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_obs_kernel(ObsIO io) {
    const int lane = wv::lane();
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) obs_env(io, i, lane);
}

}  // namespace ck
#endif
