/*
 * emu_norm.cpp -- TEST-ONLY: the normaliser rows (csrc/norm_kernels.h: cassie_norm_sum_kernel, _mean_kernel, _sq_kernel, _merge_kernel,
 * _write_kernel) on the wave emulator, configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h: norm_configure,
 * check_norm_bind_source, check_norm_bind_output, check_norm_update, check_norm_write, make_norm_io, the grids and norm_region).  Every
 * array is the caller's: the source, the outputs, and what the batch owns on the device -- the state, the partials and the counts --, so
 * the library keeps nothing from call to call.
 */
#include <cstring>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: the configuration; the bound source (src null: resolved from the rollout below) and the bound outputs (null: resolved from the
 * policy below); what the batch would resolve them from -- a rollout (ro_T 0: none) with an OBS source of ro_dim words (0: none) whose
 * store is ro_store, and a policy (pol_in_dim 0: none) with a bound normalisation (null: none) --; the batch's arrays (emu_norm_sizes
 * says how large); what the last call left; grid > 0: that many workgroups for every launch in the place of the launcher's */
struct emu_norm_args {
    int dim, block; long long max_rows; double eps;
    const float *src; int steps, rows; long long step_stride, row_stride;
    float *out_mean, *out_inv;
    int nenv, ro_T, ro_dim, pol_in_dim; const float *ro_store; long long ro_step, ro_row;
    float *pol_mean, *pol_inv;
    double *state, *part; int *cnt;
    long long last_R, last_blocks, calls;
    int grid, pad;
};

static const char *g_norm_why = nullptr;
extern "C" const char *emu_norm_last_refusal(void) { return g_norm_why; }

/* {NORM_MINBLOCK, NORM_MAXBLOCK, NORM_MAXROWS, NORM_NSTATS, NORM_STATE_ROWS, NORM_AHEAD, NORM_GRID, sizeof(emu_norm_args)}, for the binding's own checks */
extern "C" void emu_norm_constants(long long *out) {
    const long long a[8] = {ck::NORM_MINBLOCK, ck::NORM_MAXBLOCK, ck::NORM_MAXROWS, ck::NORM_NSTATS, ck::NORM_STATE_ROWS, ck::NORM_AHEAD, ck::NORM_GRID,
                            (long long)sizeof(emu_norm_args)};
    memcpy(out, a, sizeof a);
}

static ck::NormCfg g_cfg;
static ck::RolloutCfg g_ro;
static ck::PolicyCfg g_pol;

/* what the launcher does between configure and a launch */
static const char *norm_setup(const emu_norm_args &a) {
    if (const char *why = ck::norm_configure(a.dim, a.block, a.max_rows, a.eps, g_cfg)) return why;
    ck::NormCfg &c = g_cfg;
    if (!c.on) return ck::NORM_NOT_CONFIGURED;
    if (const char *why = ck::check_norm_bind_source(c, a.src, a.steps, a.rows, a.step_stride, a.row_stride)) return why;
    if (a.src) { c.src = a.src; c.steps = a.steps; c.rows = a.rows; c.step_stride = a.step_stride; c.row_stride = a.row_stride; }
    if (const char *why = ck::check_norm_bind_output(c, a.out_mean, a.out_inv)) return why;
    c.out_mean = a.out_mean; c.out_inv = a.out_inv;
    c.state = a.state; c.part = a.part; c.cnt = a.cnt;
    c.last_R = a.last_R; c.last_blocks = a.last_blocks; c.calls = a.calls;
    g_ro = {};
    if (a.ro_T > 0) {
        g_ro.T = a.ro_T; g_ro.nsrc = 1; g_ro.role[0] = a.ro_dim > 0 ? ck::RO_OBS : ck::RO_DATA; g_ro.dim[0] = a.ro_dim > 0 ? a.ro_dim : 1;
        g_ro.store[0].ptr = (void *)a.ro_store; g_ro.store[0].step = a.ro_step; g_ro.store[0].row = a.ro_row;
    }
    g_pol = {};
    if (a.pol_in_dim > 0) { g_pol.nnets = 1; g_pol.in_dim = a.pol_in_dim; g_pol.mean = a.pol_mean; g_pol.inv = a.pol_inv; }
    return nullptr;
}

/* {the state's doubles, the partials' doubles, the counts' ints, max_blocks}; -1 where the configuration is refused */
extern "C" int emu_norm_sizes(const emu_norm_args *a, long long *out) {
    ck::NormCfg c;
    g_norm_why = ck::norm_configure(a->dim, a->block, a->max_rows, a->eps, c);
    if (!g_norm_why && !c.on) g_norm_why = ck::NORM_NOT_CONFIGURED;
    if (g_norm_why) return -1;
    const long long words = c.max_blocks * c.D, r[4] = {(long long)ck::NORM_STATE_ROWS * c.D, 2 * words, words, c.max_blocks};
    memcpy(out, r, sizeof r);
    return 0;
}

static ck::NormIO g_io;
static void body_sum() { ck::cassie_norm_sum_kernel(g_io); }
static void body_mean() { ck::cassie_norm_mean_kernel(g_io); }
static void body_sq() { ck::cassie_norm_sq_kernel(g_io); }
static void body_merge() { ck::cassie_norm_merge_kernel(g_io); }
static void body_write() { ck::cassie_norm_write_kernel(g_io); }

/* phys_batch_norm_update on the emulator.  -1 where the launcher would refuse (emu_norm_last_refusal has the message); out: {R, blocks,
 * whether a lane took 16 bytes, the grid of launches 1 and 3} */
extern "C" int emu_norm_update(const emu_norm_args *a, long long *out) {
    ck::NormSource S;
    ck::NormOutput O;
    g_norm_why = norm_setup(*a);
    if (!g_norm_why) g_norm_why = ck::check_norm_update(g_cfg, g_ro, g_pol, a->nenv, S, O);
    if (g_norm_why) return -1;
    g_io = ck::make_norm_io(g_cfg, S, O);
    const int pass = a->grid > 0 ? a->grid : ck::norm_pass_grid(g_io), cols = a->grid > 0 ? a->grid : ck::norm_column_grid(g_io);
    emu::run_grid(body_sum, pass);
    emu::run_grid(body_mean, cols);
    emu::run_grid(body_sq, pass);
    emu::run_grid(body_merge, cols);
    const long long r[4] = {g_io.R, g_io.blocks, g_io.vec, ck::norm_pass_grid(g_io)};
    if (out) memcpy(out, r, sizeof r);
    return 0;
}

/* phys_batch_norm_write on the emulator */
extern "C" int emu_norm_write(const emu_norm_args *a) {
    ck::NormOutput O;
    g_norm_why = norm_setup(*a);
    if (!g_norm_why) g_norm_why = ck::check_norm_write(g_cfg, g_pol, O);
    if (g_norm_why) return -1;
    g_io = ck::make_norm_io(g_cfg, ck::NormSource{}, O);
    emu::run_grid(body_write, a->grid > 0 ? a->grid : ck::norm_column_grid(g_io));
    return 0;
}

/* phys_batch_norm_stats on the emulator: the eight doubles from the caller's state */
extern "C" int emu_norm_stats(const emu_norm_args *a, double *stats) {
    g_norm_why = norm_setup(*a);
    if (g_norm_why) return -1;
    ck::norm_stats_host(g_cfg, a->state + (size_t)ck::NORM_N * a->dim, a->state + (size_t)ck::NORM_COUNTS * a->dim, stats);
    return 0;
}

/* where phys_batch_norm_download (upload 0) / _upload (1) find `what` among the caller's arrays: {whether it lies in the partials, the
 * offset in doubles, the runs, their width and pitch} -> 0, or -1: no such thing */
extern "C" int emu_norm_region(const emu_norm_args *a, int what, int upload, long long *out) {
    g_norm_why = norm_setup(*a);
    if (g_norm_why) return -1;
    ck::NormRegion R;
    if (!ck::norm_region(g_cfg, what, upload != 0, R)) return -1;
    const bool part = what == ck::NORM_PARTIALS;
    const long long r[5] = {part, part ? R.ptr - a->part : R.ptr - a->state, R.rows, R.width, R.pitch};
    memcpy(out, r, sizeof r);
    return 0;
}
