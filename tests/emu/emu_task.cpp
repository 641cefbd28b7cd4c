/*
 * emu_task.cpp -- TEST-ONLY: the task rows (csrc/task_kernels.h: cassie_task_kernel) on the wave emulator, configured, checked and
 * launched as phys_batch.hip does it (csrc/small_launch.h: check_task_table, task_configure, check_task_bind_rows, check_task_call,
 * make_task_io, task_grid).  The emulator keeps nothing between calls: the rows, the state, the words and the call counts are the
 * caller's arrays, as they are the batch's buffers on the device, and so are the destination fields and the reference table.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: what the batch holds of every field (fields [nfields]; cmd_fields [ncmd]: the command fields), the configuration, the table
 * [nframes][tcols] (null: none set), the rows (null: not bound) with their stride in elements, the state [nenv][ncols], the words
 * [nenv][3][ncols] and the counts [nenv] */
struct emu_task_args {
    const ck::ObsField *fields; int nfields, nenv;
    const int *cmd_fields; int ncmd;
    const ck::TaskColDef *cols; int ncols, dtype; unsigned long long seed; unsigned env_base;
    const double *table; int nframes, tcols;
    void *rows; long long srow; double *state; unsigned *words; unsigned *counts;
};

static const char *g_task_why = nullptr;
extern "C" const char *emu_task_last_refusal(void) { return g_task_why; }

/* {TASK_GRID, TASK_MAXCOLS, TASK_MAXFRAMES, TASK_MAXTCOLS, TASK_WORDS, sizeof(TaskColDef), sizeof(TaskCol), sizeof(emu_task_args)}, for the binding's own checks */
extern "C" void emu_task_constants(long long *out) {
    const long long a[8] = {ck::TASK_GRID, ck::TASK_MAXCOLS, ck::TASK_MAXFRAMES, ck::TASK_MAXTCOLS, ck::TASK_WORDS, (long long)sizeof(ck::TaskColDef),
                            (long long)sizeof(ck::TaskCol), (long long)sizeof(emu_task_args)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_task_grid(int n) { return ck::task_grid(n); }

/* what the launcher does between a set_table call, a configure call and a launch: the checked table, the checked record with the
 * column table, then the binding */
static const char *task_setup(const emu_task_args &a, std::vector<ck::TaskCol> &table, ck::TaskCfg &cfg) {
    cfg = {};
    if (a.table) if (const char *why = ck::check_task_table(cfg, a.table, a.nframes, a.tcols)) return why;
    std::vector<int> dims((size_t)(a.nfields > 0 ? a.nfields : 1), 0);
    for (int k = 0; k < a.nfields; ++k) dims[k] = a.fields[k].base ? a.fields[k].dim : 0;
    table.assign((size_t)ck::TASK_MAXCOLS, ck::TaskCol());
    if (const char *why = ck::task_configure(dims.data(), a.nfields, a.cmd_fields, a.ncmd, a.cols, a.ncols, a.dtype, a.seed, a.env_base,
                                             a.table ? a.nframes : 0, a.table ? a.tcols : 0, table.data(), cfg)) return why;
    cfg.cols = table.data(); cfg.state = a.state; cfg.words = a.words; cfg.counts = a.counts;
    cfg.table = a.table; cfg.nframes = a.table ? a.nframes : 0; cfg.tcols = a.table ? a.tcols : 0;
    if (a.rows) {
        if (const char *why = ck::check_task_bind_rows(cfg, a.srow)) return why;
        cfg.rows = a.rows; cfg.srow = a.srow;
    }
    return nullptr;
}

/* check_task_table, task_configure and the bind check alone -> the message of the refusal, null where they accept; ints (may be null):
 * {ncols, dtype, ndst, tcol_need} of the record, then dst_field [9], dst_dim [9] */
extern "C" const char *emu_task_check(const emu_task_args *a, long long *ints) {
    std::vector<ck::TaskCol> table;
    ck::TaskCfg cfg;
    const char *why = task_setup(*a, table, cfg);
    if (why) return why;
    if (ints) {
        const long long head[4] = {cfg.ncols, cfg.dtype, cfg.ndst, cfg.tcol_need};
        memcpy(ints, head, sizeof head);
        for (int s = 0; s < ck::ACT_MAXDST; ++s) { ints[4 + s] = cfg.dst_field[s]; ints[4 + ck::ACT_MAXDST + s] = cfg.dst_dim[s]; }
    }
    return nullptr;
}
/* the column table of a configuration -> ncols (-1: refused); cols [TASK_MAXCOLS] */
extern "C" int emu_task_columns(const emu_task_args *a, ck::TaskCol *cols) {
    std::vector<ck::TaskCol> table;
    ck::TaskCfg cfg;
    g_task_why = task_setup(*a, table, cfg);
    if (g_task_why) return -1;
    memcpy(cols, table.data(), sizeof(ck::TaskCol) * (size_t)cfg.ncols);
    return cfg.ncols;
}
/* a later phys_batch_task_set_table against the record of a: check_task_table -> the message of its refusal, null where it accepts */
extern "C" const char *emu_task_table_check(const emu_task_args *a, const double *host, int nframes, int tcols) {
    std::vector<ck::TaskCol> table;
    ck::TaskCfg cfg;
    if (const char *why = task_setup(*a, table, cfg)) return why;
    return ck::check_task_table(cfg, host, nframes, tcols);
}
/* ck::check_task_call of the record of a -> the message of its refusal, null where it accepts.  configured 0: of an empty record;
 * now [nfields] (null: a's own): what the batch holds at the call, where that differs from what it held at the configure call */
extern "C" const char *emu_task_call_check(const emu_task_args *a, int configured, const ck::ObsField *now, int env0, int n) {
    std::vector<ck::TaskCol> table;
    ck::TaskCfg cfg = {};
    if (configured) if (const char *why = task_setup(*a, table, cfg)) return why;
    return ck::check_task_call(cfg, now ? now : a->fields, a->nfields, a->nenv, env0, n);
}
/* the record make_task_io builds for a launch, as numbers a test can read: {env0, n, ncols, f32, nframes, tcols, env_base, key0, key1,
 * cols passed, table, rows, srow, state, words, counts, reset, ndst} and for every destination slot {base, stride} -> 0, -1 where the
 * launcher would refuse */
extern "C" int emu_task_record(const emu_task_args *a, int env0, int n, const int *reset, unsigned long long *out) {
    typedef unsigned long long u64;
    std::vector<ck::TaskCol> table;
    ck::TaskCfg cfg;
    g_task_why = task_setup(*a, table, cfg);
    if (!g_task_why) g_task_why = ck::check_task_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_task_why) return -1;
    const ck::TaskIO io = ck::make_task_io(cfg, a->fields, env0, n, reset);
    const u64 head[18] = {(u64)io.env0, (u64)io.n, (u64)io.ncols, (u64)io.f32, (u64)io.nframes, (u64)io.tcols, io.env_base, io.key0, io.key1,
                          io.cols != nullptr, (u64)(size_t)io.table, (u64)(size_t)io.rows, (u64)io.srow, (u64)(size_t)io.state, (u64)(size_t)io.words,
                          (u64)(size_t)io.counts, (u64)(size_t)io.reset, (u64)cfg.ndst};
    memcpy(out, head, sizeof head);
    u64 *p = out + 18;
    for (int s = 0; s < ck::ACT_MAXDST; ++s) { p[2 * s] = (u64)(size_t)io.dst[s].base; p[2 * s + 1] = (u64)io.dst[s].stride; }
    return 0;
}

static ck::TaskIO g_taskio;
static void body_task() { ck::cassie_task_kernel(g_taskio); }

/* phys_batch_task on the emulator: one launch over [env0, env0 + n); reset: int32 [n] or null; grid 0: the launcher's.  -1 where the
 * launcher would refuse (emu_task_last_refusal has the message). */
extern "C" int emu_task(const emu_task_args *a, int env0, int n, const int *reset, int grid) {
    std::vector<ck::TaskCol> table;
    ck::TaskCfg cfg;
    g_task_why = task_setup(*a, table, cfg);
    if (!g_task_why) g_task_why = ck::check_task_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_task_why) return -1;
    if (n == 0) return 0;
    g_taskio = ck::make_task_io(cfg, a->fields, env0, n, reset);
    emu::run_grid(body_task, grid > 0 ? grid : ck::task_grid(n));
    return 0;
}

/* task_sincos2pi and task_wrap one at a time, for the measurement of their error: theta [count] -> sn, cs, wrapped [count] */
static const double *g_theta; static double *g_sn, *g_cs, *g_wr; static int g_count;
static void body_sincos() {
    const int lane = wv::lane();
    for (int k = wv::env_id() * WV_WAVE + lane; k < g_count; k += wv::grid_size() * WV_WAVE) {
        ck::task_sincos2pi(g_theta[k], g_sn[k], g_cs[k]);
        g_wr[k] = ck::task_wrap(g_theta[k]);
    }
}
extern "C" void emu_task_sincos(const double *theta, int count, double *sn, double *cs, double *wrapped) {
    g_theta = theta; g_sn = sn; g_cs = cs; g_wr = wrapped; g_count = count;
    emu::run_grid(body_sincos, 1);
}
