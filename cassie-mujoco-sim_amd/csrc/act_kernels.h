/*
 * act_kernels.h -- action rows: the stage between the tensor a policy network writes and the command fields the step kernel reads
 * (phys_batch_act, include/cassie_phys.h: the definition is there).  A configured table of columns is evaluated for an env range by ONE
 * launch: the clip of the raw action, counter-based uniform actuation noise, a per-env delay line, a low-pass, the affine map onto a
 * constant or a source row (a reference pose), the clip of the result, the store into the destination element of a command field, and a
 * small per-env action row (now | previous | applied) that the observation and the reward take as their input.  Written with the wv::
 * primitives only, workgroups of one wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_actions.cpp) runs the same text.
 * The launch record, the column table, the grid and the checks are small_launch.h's (no field of ActIO is assigned anywhere else).
 *
 * One wave takes an env at a time and ACT_GRID workgroups walk the range (as cassie_obs_kernel's do).  Per env:
 *   lane = column  consecutive lanes take consecutive columns, 64 at a time (more columns than a wave go in passes), so the loads of the
 *                  column table and of the actions and the stores of a frame of the row are contiguous across the wave.  The state of an
 *                  env is laid out [slot][ncols] -- the delay line's D + 1 slots, newest first, then the filter state, then the previous
 *                  clipped action -- so a wave's loads and stores of a slot are contiguous too.  A column's delay line and filter state
 *                  never cross lanes: the shift, oldest slot first, needs no barrier and no second buffer.
 *   the noise      Philox4x32-10 (obs_kernels.h's routine) on the counter (env_base + env, column, counts[env], 1), in the lanes whose column
 *                  has noise != 0 only: the fourth word is 1 where the observation's is 0, so one seed gives the two their own streams.
 *   the count      counts[env] is read by every lane through lane 0 before anything is stored and written by lane 0 after the last pass.
 *   the delay      delay[env] clamped to [0, D] is the one value that picks among memory -- and only among the env's own D + 1 slots.
 * Every arithmetic step of a value is one individually rounded operation (wv::mul_rn / add_rn / sub_rn): the device, the emulator and a
 * numpy restatement (tests/actions_check.py) agree bit for bit.  Vector loads and stores only, no LDS; an env's wave reads that env's
 * action, source rows and state and touches that env's destination elements, row, state and count alone.
 */
#ifndef CASSIE_ACT_KERNELS_H
#define CASSIE_ACT_KERNELS_H

#include "obs_kernels.h"

namespace ck {

/* ACT_GRID: the workgroups that walk a range.  A few, as the observation's: the launch runs in front of a range's step launch while the
 * other range's step kernel fills the chip.  A first choice (tools/action_rate.py measures the call in the loop it is meant for). */
constexpr int ACT_GRID = 64, ACT_MAXCOLS = 256, ACT_MAXDELAY = 8, ACT_MAXSLOTS = 16, ACT_MAXDST = 9;
constexpr int ACT_INPUT = -1, ACT_CONST = -2, ACT_NONE = -3;   /* (PHYS_ACT_INPUT, PHYS_ACT_CONST: a base that is no field; PHYS_ACT_NONE: no destination) */
enum { ACT_NOW = 0, ACT_PREV = 1, ACT_APPLIED = 2, ACT_FRAMES = 3 };   /* (PHYS_ACT_NOW, _PREV, _APPLIED: the frames of an action row) */

/* a column as the caller writes it (phys_act_col_t of cassie_phys.h) */
struct ActColDef { int bfield, bindex, dfield, dindex; double lo, hi, noise, smooth, offset, scale, out_lo, out_hi; };

/* a column as a launch reads it: the slot of its base among the call's sources (-1: the offset alone) with the element of the source's
 * row, the slot of its destination among the call's (-1: none) with the element of that row, and the eight constants */
struct ActCol { int slot, elem, dslot, delem; double lo, hi, noise, smooth, offset, scale, out_lo, out_hi; };

/* a destination of the call: the rows of a command field where the batch reads them (its own buffer or the caller's bound tensor) and
 * the doubles between two rows */
struct ActDst { double *base; long long stride; };

struct ActIO {
    int env0, n, ncols, delay_max, f32, act_f32;   /* f32: the rows are floats; act_f32: the actions are */
    unsigned env_base, key0, key1;                 /* the counter's offset and the key (seed & 0xffffffff, seed >> 32) */
    const ActCol *cols;                            /* [ncols] */
    ObsSrc src[ACT_MAXSLOTS];
    ActDst dst[ACT_MAXDST];
    const void *actions; long long sact;           /* [nenv] rows of ncols elements, sact elements apart */
    void *rows; long long srow;                    /* [nenv] rows [ACT_FRAMES][ncols], srow elements apart */
    double *state;                                 /* [nenv][delay_max + 3][ncols]: the line | the filter state | the previous clipped action */
    unsigned *counts;                              /* [nenv] the calls an env has seen (wraps) */
    const int *delay;                              /* [nenv] or null (0): the env's latency in calls, clamped to [0, delay_max] */
    const int *reset;                              /* [n] or null: non-zero = the env starts afresh */
};

WV_DEVICE void act_env(const ActIO &io, int i, int lane) {
    const size_t env = (size_t)io.env0 + (size_t)i;
    /* lane 0's reading of the count stands for the wave: nobody stores before every lane has it */
    const unsigned count = (unsigned)wv::shfl_i((int)io.counts[env], 0);
    const bool fresh = count == 0u || (io.reset && io.reset[i] != 0);
    const int ncols = io.ncols, D = io.delay_max;
    int d = io.delay ? io.delay[env] : 0;
    d = d < 0 ? 0 : (d > D ? D : d);
    double *const st = io.state + env * (size_t)(D + 3) * (size_t)ncols;
    double *const filt = st + (size_t)(D + 1) * ncols, *const last = st + (size_t)(D + 2) * ncols;
    float *const row32 = (float *)io.rows + env * (size_t)io.srow;
    double *const row64 = (double *)io.rows + env * (size_t)io.srow;
    for (int c = lane; c < ncols; c += WV_WAVE) {
        const ActCol col = io.cols[c];
        const size_t at = env * (size_t)io.sact + (size_t)c;
        const double a = io.act_f32 ? (double)((const float *)io.actions)[at] : ((const double *)io.actions)[at];
        const double u = clampd(a, col.lo, col.hi);
        double v = u;
        if (col.noise != 0.0) {
            unsigned w[4];
            philox4x32_10(io.env_base + (unsigned)env, (unsigned)c, count, 1u, io.key0, io.key1, w);
            v = wv::add_rn(u, wv::mul_rn(col.noise, obs_uniform(w[0])));
        }
        /* the delay line of this column, oldest slot first; then the newest.  z: slot d after the shift */
        double z = v;
        for (int h = D; h >= 1; --h) {
            const double s = fresh ? v : st[(size_t)(h - 1) * ncols + c];
            st[(size_t)h * ncols + c] = s;
            if (h == d) z = s;
        }
        st[c] = v;
        /* the low-pass: skipped, not evaluated, where smooth == 1 */
        const double f = filt[c];
        const double y = (fresh || col.smooth == 1.0) ? z : wv::add_rn(f, wv::mul_rn(col.smooth, wv::sub_rn(z, f)));
        filt[c] = y;
        const double base = col.slot < 0 ? col.offset : wv::add_rn(col.offset, obs_load(io.src[col.slot], env, col.elem));
        const double t = clampd(wv::add_rn(base, wv::mul_rn(col.scale, y)), col.out_lo, col.out_hi);
        if (col.dslot >= 0) io.dst[col.dslot].base[env * (size_t)io.dst[col.dslot].stride + (size_t)col.delem] = t;
        const double prev = fresh ? u : last[c];
        last[c] = u;
        if (io.f32) {
            row32[(size_t)ACT_NOW * ncols + c] = (float)u; row32[(size_t)ACT_PREV * ncols + c] = (float)prev; row32[(size_t)ACT_APPLIED * ncols + c] = (float)y;
        } else {
            row64[(size_t)ACT_NOW * ncols + c] = u; row64[(size_t)ACT_PREV * ncols + c] = prev; row64[(size_t)ACT_APPLIED * ncols + c] = y;
        }
    }
    if (lane == 0) io.counts[env] = count + 1u;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_act_kernel(ActIO io) {
    const int lane = wv::lane();
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) act_env(io, i, lane);
}

}  // namespace ck
#endif
