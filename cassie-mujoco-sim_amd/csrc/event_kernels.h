/*
 * event_kernels.h -- event rows: what a policy step REMEMBERS of the steps before it (phys_batch_events, include/cassie_phys.h: the
 * definition is there).  A configured table of columns -- a number measured from a field, a Schmitt trigger, a timer, an edge, a latch,
 * a running maximum / minimum / sum, a combination of flags -- is evaluated in index order for an env range by ONE launch: the event
 * row, one int32 done word per env (what phys_batch_end_episodes takes as `force`), and the columns' state.  Written with the wv::
 * primitives only, workgroups of one wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_events.cpp) runs the same text.
 * The launch record, the column table, the grid and the checks are small_launch.h's (no field of EventIO is assigned anywhere else).
 *
 * The mapping:
 *   lane = env     as the reward's: a lane takes one env and walks the column table; workgroup w of the grid takes envs 64 w .. 64 w + 63
 *                  of the range and EVENT_GRID workgroups walk a longer one.  The column table is indexed by the loop counter, which the
 *                  compiler keeps in scalar registers: every lane reads the same entry, so the branches on a column's kind and op are
 *                  uniform, the wave diverges only at the selects a value decides, and nothing crosses lanes: no shuffle, no barrier.
 *                  (This compiler reads the entry with vector loads of one address, not scalar loads: the kernel stores to global
 *                  memory and the table is not in the constant address space.  DESIGN 7.)
 *   the selects    a column's state is loaded unconditionally and VALUES are selected: `cleared ? C.init : *state`, a choice between two
 *                  loads, compiled to code that never took the init (accumulators were not cleared on the device; the emulator was right).
 *   the values     a column reads earlier columns' fp64 values by an index of the TABLE (run-time, wave-uniform).  A register array
 *                  indexed that way goes to scratch; the values of the call live in an LDS tile [EVENT_MAXCOLS][64] of doubles instead,
 *                  column-major across lanes: lane l touches slot [c][l] alone (consecutive lanes, consecutive banks: no conflict), so no
 *                  barrier is needed, and a workgroup that walks on to its next 64 envs overwrites what it has finished with.
 *   the state      [slot][ncols][nenv] doubles and [ncols][nenv] words in device memory: the 64 lanes load and store 64 consecutive
 *                  elements.  The [nenv][...] shape is the host API's only (phys_batch_events_state transposes).
 *   the sums       every arithmetic step is one individually rounded fp64 operation and every sum sequential in index order, so the
 *                  device, the emulator and a numpy restatement (tests/events_check.py) agree bit for bit.
 * Vector loads and stores only; a lane reads its env's source rows and touches its env's row, done word, state and count alone.  No
 * value indexes memory: a column names lower COLUMNS, which configure checks; a NaN flows through as the definition says.  No stepping
 * kernel is handed any of this.  Lane = column with shuffles per dependency level is the alternative; not measured.
 */
#ifndef CASSIE_EVENT_KERNELS_H
#define CASSIE_EVENT_KERNELS_H

#include "obs_kernels.h"

namespace ck {

/* EVENT_GRID: the workgroups that walk a range, 64 envs each: one pass up to 4096 envs (as REWARD_GRID) */
constexpr int EVENT_GRID = 64, EVENT_MAXCOLS = 64, EVENT_MAXCOUNT = 8, EVENT_MAXSLOTS = OBS_MAXSLOTS;
enum { EV_MEASURE = 0, EV_LEVEL = 1, EV_TIMER = 2, EV_EDGE = 3, EV_LATCH = 4, EV_ACCUM = 5, EV_LOGIC = 6 };   /* (PHYS_EV_MEASURE ... _LOGIC) */
enum { EV_SIGNED = 0, EV_SUMABS = 1, EV_SUMSQ = 2, EV_MAXABS = 3 };    /* (PHYS_EV_SIGNED, _SUMABS, _SUMSQ, _MAXABS: a MEASURE's norm) */
enum { EV_RISING = 0, EV_FALLING = 1, EV_EITHER = 2 };                 /* (PHYS_EV_RISING, _FALLING, _EITHER: an EDGE's op) */
enum { EV_MAX = 0, EV_MIN = 1, EV_SUM = 2 };                           /* (PHYS_EV_MAX, _MIN, _SUM: an ACCUM's op) */
enum { EV_ANY = 0, EV_ALL = 1, EV_NONE = 2, EV_COUNT = 3 };            /* (PHYS_EV_ANY, _ALL, _NONE, _COUNT: a LOGIC's op) */
constexpr int EV_INPUT = OBS_INPUT;                                    /* (PHYS_EV_INPUT: the caller's array) */

/* a column as the caller writes it (phys_event_col_t of cassie_phys.h).  In the table a launch reads, a MEASURE's field holds the SLOT of
 * its source among the call's instead */
struct EventCol {
    int kind, field, index, count, norm, root;      /* MEASURE */
    int src, trig, clear, gate;                     /* lower columns (-1: none, where the definition allows it) */
    int op, sense, polarity, lag, keep, pad;        /* EDGE / ACCUM / LOGIC: op; LEVEL: sense; TIMER: polarity; LATCH: lag, keep */
    unsigned long long mask;                        /* LOGIC */
    double target, on_thr, off_thr, dt, offset, scale, init;
};

typedef ObsSrc EventSrc;

struct EventIO {
    int env0, n, ncols, f32;            /* f32: the rows are floats */
    long long nenv;                     /* the envs of the batch: the stride of the state's columns */
    unsigned long long done_mask;
    const EventCol *cols;               /* [ncols], the fields as slots */
    EventSrc src[EVENT_MAXSLOTS];
    void *rows; long long srow;         /* [nenv] rows [ncols], srow elements apart */
    int *flags;                         /* [nenv] the done words */
    double *state;                      /* [2][ncols][nenv] */
    unsigned *words;                    /* [ncols][nenv] */
    unsigned *counts;                   /* [nenv] the calls an env has seen (wraps) */
    const int *reset;                   /* [n] or null: non-zero = the env starts afresh */
};

/* a MEASURE: the errors against the target, the norm in the reward's order of operations, the root */
WV_DEVICE double event_measure(const EventIO &io, const EventCol &C, size_t env) {
    using namespace wv;
    const EventSrc &S = io.src[C.field];
    if (C.norm == EV_SIGNED) return sub_rn(obs_load(S, env, C.index), C.target);
    double s = 0.0;
    for (int j = 0; j < C.count; ++j) {
        const double e = sub_rn(obs_load(S, env, C.index + j), C.target);
        if (C.norm == EV_SUMSQ) s = add_rn(s, mul_rn(e, e));
        else if (C.norm == EV_SUMABS) s = add_rn(s, fabs(e));
        else { const double m = fabs(e); if (m > s) s = m; }
    }
    return C.norm == EV_SUMSQ && C.root != 0 ? sqrt_rn(s) : s;
}

/* env env0 + i of the range: the columns in order, the stores, the done word and the count.  V: the wave's tile, l: this lane */
WV_DEVICE void event_env(const EventIO &io, int i, double (*V)[WV_WAVE], int l) {
    using namespace wv;
    const size_t env = (size_t)io.env0 + (size_t)i, nenv = (size_t)io.nenv, nc = (size_t)io.ncols;
    const unsigned count = io.counts[env];
    const bool fresh = count == 0u || (io.reset && io.reset[i] != 0);
    int done = 0;
    for (int c = 0; c < io.ncols; ++c) {
        const EventCol &C = io.cols[c];
        double *const st0 = io.state + (size_t)c * nenv + env, *const st1 = st0 + nc * nenv;
        unsigned *const wd = io.words + (size_t)c * nenv + env;
        double out;
        if (C.kind == EV_MEASURE) out = event_measure(io, C, env);
        else if (C.kind == EV_LEVEL) {
            const double x = V[C.src][l], w = C.sense < 0 ? -x : x;
            const unsigned was = *wd;
            const bool s = fresh | (was == 0u) ? w >= C.on_thr : w > C.off_thr;
            *wd = s ? 1u : 0u;
            out = s ? 1.0 : 0.0;
        } else if (C.kind == EV_TIMER) {
            const unsigned told = *wd;
            unsigned t = fresh ? 0u : told;
            if ((V[C.src][l] > 0.0) != (C.polarity == 0)) t = t == 0xffffffffu ? t : t + 1u; else t = 0u;
            *wd = t;
            out = mul_rn(C.dt, (double)t);
        } else if (C.kind == EV_EDGE) {
            const unsigned pold = *wd;
            const bool cur = V[C.src][l] > 0.0, p = fresh ? cur : pold != 0u;
            out = (C.op == EV_RISING ? cur && !p : C.op == EV_FALLING ? !cur && p : cur != p) ? 1.0 : 0.0;
            *wd = cur ? 1u : 0u;
        } else if (C.kind == EV_LATCH) {
            const double x = V[C.src][l];
            const double hold = *st0, qold = *st1;
            double h = fresh ? 0.0 : hold;
            const double q = fresh ? 0.0 : qold;
            const bool fire = V[C.trig][l] > 0.0;
            if (fire) h = add_rn(C.offset, mul_rn(C.scale, C.lag != 0 ? q : x));
            out = C.keep != 0 || fire ? h : 0.0;
            *st0 = h; *st1 = x;
        } else if (C.kind == EV_ACCUM) {
            /* (straight-line: the values of column 0 stand in for an absent clear or gate, and values are selected, never addresses) */
            const double v = V[C.src][l], vclear = V[C.clear >= 0 ? C.clear : 0][l], vgate = V[C.gate >= 0 ? C.gate : 0][l];
            const double init = C.init, old = *st0;
            const bool cleared = fresh | ((C.clear >= 0) & (vclear > 0.0)), fed = (C.gate < 0) | (vgate > 0.0);
            const double m0 = cleared ? init : old;
            const double m1 = C.op == EV_MAX ? (v > m0 ? v : m0) : C.op == EV_MIN ? (v < m0 ? v : m0) : add_rn(m0, v);
            out = fed ? m1 : m0;
            *st0 = out;
        } else {   /* EV_LOGIC */
            int k = 0;
            for (int j = 0; j < c; ++j) if (((C.mask >> j) & 1ull) != 0ull && V[j][l] > 0.0) ++k;
            out = C.op == EV_ANY ? (k > 0 ? 1.0 : 0.0) : C.op == EV_ALL ? (k == popc64(C.mask) ? 1.0 : 0.0) : C.op == EV_NONE ? (k == 0 ? 1.0 : 0.0) : (double)k;
        }
        V[c][l] = out;
        const size_t at = env * (size_t)io.srow + (size_t)c;
        if (io.f32) ((float *)io.rows)[at] = (float)out; else ((double *)io.rows)[at] = out;
        if (((io.done_mask >> c) & 1ull) != 0ull && out > 0.0) done = 1;
    }
    io.flags[env] = done;
    io.counts[env] = count + 1u;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_event_kernel(EventIO io) {
    WV_SHARED double V[EVENT_MAXCOLS][WV_WAVE];
    const int l = wv::lane();
    for (int i = wv::env_id() * WV_WAVE + l; i < io.n; i += wv::grid_size() * WV_WAVE) event_env(io, i, V, l);
}

}  // namespace ck
#endif
