/*
 * task_kernels.h -- task rows: the stage that makes what a policy step is ASKED -- the velocity command, the gait clock and its
 * waveforms, the swing / stance gates, the row of a reference trajectory, the pushes -- which the observation, the reward and the action
 * stages had taken as "the caller's input" (phys_batch_task, include/cassie_phys.h: the definition is there).  A configured table of at
 * most 64 columns is evaluated for an env range by ONE launch.  Written with the wv:: primitives only, workgroups of one wave:
 * phys_batch.hip launches it, the wave emulator (tests/emu/emu_task.cpp) runs the same text.  The launch record, the column table, the
 * grid and the checks are small_launch.h's (no field of TaskIO is assigned anywhere else).
 *
 * One wave takes an env at a time and TASK_GRID workgroups walk the range (as cassie_act_kernel's do).  Per env:
 *   lane = column  ONE pass: lane c makes column c, which is why a row has at most 64 columns.  The four kinds read each other downwards
 *                  only (SAMPLE <- PHASE <- WAVE, TABLE), so the three dependencies are three exchanges that ALL 64 lanes execute in
 *                  uniform control flow, idle lanes included: two wv::shfl of the SAMPLE outputs (a clock's rate_col and phase_col) and
 *                  one of the phases (a waveform's or a table column's src).  A lane without the dependency names itself.
 *   the state      [slot][ncols]: one double (a SAMPLE's held value, a PHASE's phi) and three words (left, age, epoch) per column, so a
 *                  wave's loads and stores of a slot are contiguous.
 *   the draws      Philox4x32-10 (obs_kernels.h's routine) in the lanes that draw in this call only: the schedule from the counter
 *                  (env_base + env, group, epoch, 2), the value from (env_base + env, column, epoch, 3).  A group's lanes compute the same
 *                  schedule each for itself: no lane talks to another for that.
 *   the count      counts[env] is read by every lane through lane 0 before anything is stored and written by lane 0 after the stores.
 *   the table      the clamped frame index is the one value that picks among memory, and it picks inside the table.
 * Every arithmetic step of a value is one individually rounded operation (wv::mul_rn / add_rn / sub_rn / div_rn; floor and rint are
 * exact): the device, the emulator and a numpy restatement (tests/task_check.py) agree bit for bit -- sin and cos included, which are
 * written out step by step here (task_sincos2pi) because no library's reproduce between a device and a host.  Vector loads and stores
 * only, no LDS; an env's wave touches that env's row, state, count and destination elements alone.  No stepping kernel is handed any of it.
 */
#ifndef CASSIE_TASK_KERNELS_H
#define CASSIE_TASK_KERNELS_H

#include "act_kernels.h"

namespace ck {

/* TASK_GRID: the workgroups that walk a range.  A few, as the action's: the launch runs behind a range's step launch while the other
 * range's step kernel fills the chip.  A first choice (tools/task_rate.py measures the call in the loop it is meant for). */
constexpr int TASK_GRID = 64, TASK_MAXCOLS = 64, TASK_MAXFRAMES = 4096, TASK_MAXTCOLS = 64, TASK_WORDS = 3;
constexpr unsigned TASK_MAXPERIOD = 1u << 30;
enum { TASK_SAMPLE = 0, TASK_PHASE = 1, TASK_WAVE = 2, TASK_TABLE = 3 };          /* (PHYS_TASK_SAMPLE .. _TABLE: the kinds) */
enum { TASK_SAW = 0, TASK_SIN = 1, TASK_COS = 2, TASK_TRAPEZOID = 3 };            /* (PHYS_TASK_SAW .. _TRAPEZOID: a WAVE's forms) */
enum { TASK_LEFT = 0, TASK_AGE = 1, TASK_EPOCH = 2 };                             /* the slots of the state's words */
constexpr int TASK_NONE = ACT_NONE;                                               /* (PHYS_TASK_NONE: no destination) */

/* a column as the caller writes it (phys_task_col_t of cassie_phys.h) */
struct TaskColDef {
    int kind, form, group, rate_col, phase_col, src, tcol, dfield, dindex;
    unsigned period_lo, period_hi, hold;
    double center, half, rest, p_rest, rate, rate_scale, phase0, shift, duty, ramp, offset, scale;
};

/* a column as a launch reads it: the kinds' column references as lanes (-1: none; a SAMPLE's group is never -1), the slot of its
 * destination among the call's (-1: none) with the element of that row, the periods as (lo, hi - lo + 1), the resting threshold
 * (the uint64 nearest p_rest 2^32) and the constants */
struct TaskCol {
    int kind, form, group, rate_col, phase_col, src, tcol, dslot, delem;
    unsigned period_lo, span, hold;
    unsigned long long thr;
    double center, half, rest, rate, rate_scale, phase0, shift, duty, ramp, offset, scale;
};

struct TaskIO {
    int env0, n, ncols, f32, nframes, tcols;       /* f32: the rows are floats; the table's frames and columns (0: no table) */
    unsigned env_base, key0, key1;                 /* the counter's offset and the key (seed & 0xffffffff, seed >> 32) */
    const TaskCol *cols;                           /* [ncols] */
    const double *table;                           /* [nframes][tcols] or null */
    ActDst dst[ACT_MAXDST];
    void *rows; long long srow;                    /* [nenv] rows of ncols elements, srow elements apart */
    double *state;                                 /* [nenv][ncols]: a SAMPLE's x, a PHASE's phi */
    unsigned *words;                               /* [nenv][TASK_WORDS][ncols]: a SAMPLE's left | age | epoch */
    unsigned *counts;                              /* [nenv] the calls an env has seen (wraps) */
    const int *reset;                              /* [n] or null: non-zero = the env starts afresh */
};

/* p - floor(p), in [0, 1): a p just below an integer rounds to 1 and becomes 0; a NaN or an infinity gives NaN */
WV_DEVICE double task_wrap(double p) {
    const double f = wv::sub_rn(p, floor(p));
    return f >= 1.0 ? 0.0 : f;
}

/* sin(2 pi theta) and cos(2 pi theta) for theta in [0, 1), step by step: q = rint(4 theta) and r = theta - q / 4 are exact, |r| <= 1/8;
 * x = 2 pi r, rounded once; S and C by Horner in z = x x from the doubles nearest the Taylor coefficients +-1 / k! (degree 19 and 20),
 * every step rounded on its own; the quadrant q & 3 picks among (S, C), (C, -S), (-S, -C), (-C, S).  A NaN gives NaN before the
 * quadrant is taken.  At theta = 0, 1/4, 1/2, 3/4: r = 0, S = 0 and C = 1 exactly.  (tests/test_task.py measures the error.) */
WV_DEVICE void task_sincos2pi(double theta, double &sn, double &cs) {
    using namespace wv;
    if (!(theta == theta)) { sn = theta; cs = theta; return; }
    const double q = rint(mul_rn(4.0, theta));
    const double r = sub_rn(theta, mul_rn(0.25, q));
    const double x = mul_rn(r, 6.283185307179586);
    const double z = mul_rn(x, x);
    double p = -8.22063524662433e-18;                     /* -1 / 19! */
    p = add_rn(2.8114572543455206e-15, mul_rn(z, p));      /*  1 / 17! */
    p = add_rn(-7.647163731819816e-13, mul_rn(z, p));     /* -1 / 15! */
    p = add_rn(1.6059043836821613e-10, mul_rn(z, p));      /*  1 / 13! */
    p = add_rn(-2.505210838544172e-08, mul_rn(z, p));     /* -1 / 11! */
    p = add_rn(2.7557319223985893e-06, mul_rn(z, p));      /*  1 / 9! */
    p = add_rn(-0.0001984126984126984, mul_rn(z, p));     /* -1 / 7! */
    p = add_rn(0.008333333333333333, mul_rn(z, p));      /*  1 / 5! */
    p = add_rn(-0.16666666666666666, mul_rn(z, p));     /* -1 / 3! */
    const double S = add_rn(x, mul_rn(mul_rn(x, z), p));
    double c = 4.110317623312165e-19;                      /*  1 / 20! */
    c = add_rn(-1.5619206968586225e-16, mul_rn(z, c));     /* -1 / 18! */
    c = add_rn(4.779477332387385e-14, mul_rn(z, c));      /*  1 / 16! */
    c = add_rn(-1.1470745597729725e-11, mul_rn(z, c));     /* -1 / 14! */
    c = add_rn(2.08767569878681e-09, mul_rn(z, c));      /*  1 / 12! */
    c = add_rn(-2.755731922398589e-07, mul_rn(z, c));     /* -1 / 10! */
    c = add_rn(2.48015873015873e-05, mul_rn(z, c));      /*  1 / 8! */
    c = add_rn(-0.001388888888888889, mul_rn(z, c));     /* -1 / 6! */
    c = add_rn(0.041666666666666664, mul_rn(z, c));      /*  1 / 4! */
    c = add_rn(-0.5, mul_rn(z, c));                                        /* -1 / 2! */
    const double C = add_rn(1.0, mul_rn(z, c));
    const int quad = (int)q & 3;
    sn = quad == 0 ? S : quad == 1 ? C : quad == 2 ? -S : -C;
    cs = quad == 0 ? C : quad == 1 ? -S : quad == 2 ? -C : S;
}

WV_DEVICE void task_env(const TaskIO &io, int i, int lane) {
    using namespace wv;
    const size_t env = (size_t)io.env0 + (size_t)i;
    /* lane 0's reading of the count stands for the wave: nobody stores before every lane has it */
    const unsigned count = (unsigned)shfl_i((int)io.counts[env], 0);
    const bool fresh = count == 0u || (io.reset && io.reset[i] != 0);
    const int ncols = io.ncols, c = lane;
    const bool mine = c < ncols;
    const TaskCol col = io.cols[mine ? c : 0];
    const int kind = mine ? col.kind : -1;
    double *const st = io.state + env * (size_t)ncols;
    unsigned *const wd = io.words + env * (size_t)TASK_WORDS * (size_t)ncols;
    double out = 0.0;

    /* 1. SAMPLE: a value held for a random number of calls */
    if (kind == TASK_SAMPLE) {
        double x = st[c];
        unsigned left = wd[TASK_LEFT * ncols + c], age = wd[TASK_AGE * ncols + c], epoch = wd[TASK_EPOCH * ncols + c];
        if (fresh || left == 0u) {
            epoch = count == 0u ? 0u : epoch + 1u;
            unsigned s[4], v[4];
            philox4x32_10(io.env_base + (unsigned)env, (unsigned)col.group, epoch, 2u, io.key0, io.key1, s);
            left = col.period_lo + (unsigned)(((unsigned long long)s[0] * (unsigned long long)col.span) >> 32);
            const bool resting = (unsigned long long)s[1] < col.thr;
            philox4x32_10(io.env_base + (unsigned)env, (unsigned)c, epoch, 3u, io.key0, io.key1, v);
            x = resting ? col.rest : add_rn(col.center, mul_rn(col.half, obs_uniform(v[0])));
            age = 0u;
        }
        out = (col.hold == 0u || age < col.hold) ? x : col.rest;
        st[c] = x;
        wd[TASK_LEFT * ncols + c] = left - 1u; wd[TASK_AGE * ncols + c] = age + 1u; wd[TASK_EPOCH * ncols + c] = epoch;
    }

    /* 2. PHASE: a clock, from the SAMPLE outputs of two lanes (every lane takes part in the exchanges; one without the dependency
     * names itself) */
    const bool clock = kind == TASK_PHASE;
    const double rate_x = shfl(out, clock && col.rate_col >= 0 ? col.rate_col : lane);
    const double phase_x = shfl(out, clock && col.phase_col >= 0 ? col.phase_col : lane);
    if (clock) {
        if (fresh) out = task_wrap(col.phase_col < 0 ? col.phase0 : phase_x);
        else {
            const double inc = col.rate_col < 0 ? col.rate : add_rn(col.rate, mul_rn(col.rate_scale, rate_x));
            out = task_wrap(add_rn(st[c], inc));
        }
        st[c] = out;
    }

    /* 3. WAVE and 4. TABLE: functions of a clock's phase */
    const bool reads_clock = kind == TASK_WAVE || kind == TASK_TABLE;
    const double phi = shfl(out, reads_clock ? col.src : lane);
    if (reads_clock) {
        const double theta = task_wrap(add_rn(phi, col.shift));
        double g;
        if (kind == TASK_WAVE) {
            if (col.form == TASK_SAW) g = theta;
            else if (col.form == TASK_TRAPEZOID) {
                const double up = clampd(div_rn(theta, col.ramp), 0.0, 1.0), down = clampd(div_rn(sub_rn(theta, col.duty), col.ramp), 0.0, 1.0);
                g = sub_rn(up, down);
            } else {
                double sn, cs;
                task_sincos2pi(theta, sn, cs);
                g = col.form == TASK_SIN ? sn : cs;
            }
        } else {
            const int nf = io.nframes;
            const double s = mul_rn(theta, (double)nf);
            int a = s >= 0.0 ? (int)floor(s) : 0;       /* (a NaN gives 0) */
            a = a < nf - 1 ? a : nf - 1;
            const double fr = sub_rn(s, (double)a);
            const int b = a + 1 == nf ? 0 : a + 1;
            const double ta = io.table[(size_t)a * io.tcols + col.tcol], tb = io.table[(size_t)b * io.tcols + col.tcol];
            g = add_rn(ta, mul_rn(fr, sub_rn(tb, ta)));
        }
        out = add_rn(col.offset, mul_rn(col.scale, g));
    }

    if (mine) {
        if (col.dslot >= 0) io.dst[col.dslot].base[env * (size_t)io.dst[col.dslot].stride + (size_t)col.delem] = out;
        if (io.f32) ((float *)io.rows)[env * (size_t)io.srow + c] = (float)out;
        else ((double *)io.rows)[env * (size_t)io.srow + c] = out;
    }
    if (lane == 0) io.counts[env] = count + 1u;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_task_kernel(TaskIO io) {
    const int lane = wv::lane();
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) task_env(io, i, lane);
}

}  // namespace ck
#endif
