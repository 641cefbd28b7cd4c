/*
 * emu_actions.cpp -- TEST-ONLY: the action rows (csrc/act_kernels.h: cassie_act_kernel) on the wave emulator, configured, checked and
 * launched as phys_batch.hip does it (csrc/small_launch.h: act_configure, check_act_bind_actions, check_act_bind_rows,
 * check_act_bind_input, check_act_call, make_act_io, act_grid).  The emulator keeps nothing between calls: the rows, the state and the
 * call counts are the caller's arrays, as they are the batch's buffers on the device, and so are the destination fields.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: what the batch holds of every field (fields [nfields]; depth_field: PHYS_F_DEPTH; cmd_fields [ncmd]: the command fields), the
 * configuration, the bound actions, input (null: none) and delays (null: none), the rows with their stride in elements, the state
 * [nenv][delay_max + 3][ncols] and the counts [nenv] */
struct emu_act_args {
    const ck::ObsField *fields; int nfields, depth_field, nenv;
    const int *cmd_fields; int ncmd;
    const ck::ActColDef *cols; int ncols, delay_max, dtype; unsigned long long seed; unsigned env_base;
    const void *actions; long long act_stride; int act_dtype;
    const void *input; int input_dim; long long input_stride; int input_dtype;
    const int *delay;
    void *rows; long long srow; double *state; unsigned *counts;
};

static const char *g_act_why = nullptr;
extern "C" const char *emu_act_last_refusal(void) { return g_act_why; }

/* {ACT_GRID, ACT_MAXCOLS, ACT_MAXDELAY, ACT_MAXSLOTS, ACT_MAXDST, sizeof(ActColDef), sizeof(ActCol), sizeof(emu_act_args)}, for the binding's own checks */
extern "C" void emu_act_constants(long long *out) {
    const long long a[8] = {ck::ACT_GRID, ck::ACT_MAXCOLS, ck::ACT_MAXDELAY, ck::ACT_MAXSLOTS, ck::ACT_MAXDST, (long long)sizeof(ck::ActColDef),
                            (long long)sizeof(ck::ActCol), (long long)sizeof(emu_act_args)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_act_grid(int n) { return ck::act_grid(n); }

/* what the launcher does between a configure call and a launch: the checked record with the column table, then the bindings */
static const char *act_setup(const emu_act_args &a, std::vector<ck::ActCol> &table, ck::ActCfg &cfg) {
    std::vector<int> dims((size_t)(a.nfields > 0 ? a.nfields : 1), 0);
    for (int k = 0; k < a.nfields; ++k) dims[k] = a.fields[k].base ? a.fields[k].dim : 0;
    table.assign((size_t)ck::ACT_MAXCOLS, ck::ActCol());
    if (const char *why = ck::act_configure(dims.data(), a.nfields, a.depth_field, a.cmd_fields, a.ncmd, a.cols, a.ncols, a.delay_max, a.dtype, a.seed,
                                            a.env_base, table.data(), cfg)) return why;
    if (a.ncols == 0) return nullptr;
    cfg.cols = table.data(); cfg.state = a.state; cfg.counts = a.counts; cfg.delay = a.delay;
    if (a.rows) {
        if (const char *why = ck::check_act_bind_rows(cfg, a.srow)) return why;
        cfg.rows = a.rows; cfg.srow = a.srow;
    }
    if (a.actions) {
        if (const char *why = ck::check_act_bind_actions(cfg, a.act_stride, a.act_dtype)) return why;
        cfg.actions = a.actions; cfg.act_stride = a.act_stride; cfg.act_dtype = a.act_dtype;
    }
    if (a.input) {
        if (const char *why = ck::check_act_bind_input(cfg, a.input_dim, a.input_stride, a.input_dtype)) return why;
        cfg.input = a.input; cfg.input_dim = a.input_dim; cfg.input_stride = (int)a.input_stride; cfg.input_dtype = a.input_dtype;
    }
    return nullptr;
}

/* act_configure and the bind checks alone -> the message of the refusal, null where they accept; ints (may be null): {ncols, delay_max,
 * dtype, nslots, ndst, input_need, state doubles per env} of the record, then slot_field [16], slot_dim [16], dst_field [9], dst_dim [9] */
extern "C" const char *emu_act_check(const emu_act_args *a, long long *ints) {
    std::vector<ck::ActCol> table;
    ck::ActCfg cfg;
    const char *why = act_setup(*a, table, cfg);
    if (why) return why;
    if (ints) {
        const long long head[7] = {cfg.ncols, cfg.delay_max, cfg.dtype, cfg.nslots, cfg.ndst, cfg.input_need, ck::act_state_dim(cfg)};
        memcpy(ints, head, sizeof head);
        long long *p = ints + 7;
        for (int s = 0; s < ck::ACT_MAXSLOTS; ++s) { p[s] = cfg.slot_field[s]; p[ck::ACT_MAXSLOTS + s] = cfg.slot_dim[s]; }
        p += 2 * ck::ACT_MAXSLOTS;
        for (int s = 0; s < ck::ACT_MAXDST; ++s) { p[s] = cfg.dst_field[s]; p[ck::ACT_MAXDST + s] = cfg.dst_dim[s]; }
    }
    return nullptr;
}
/* the column table of a configuration -> ncols (-1: refused); cols [ACT_MAXCOLS] */
extern "C" int emu_act_columns(const emu_act_args *a, ck::ActCol *cols) {
    std::vector<ck::ActCol> table;
    ck::ActCfg cfg;
    g_act_why = act_setup(*a, table, cfg);
    if (g_act_why) return -1;
    memcpy(cols, table.data(), sizeof(ck::ActCol) * (size_t)cfg.ncols);
    return cfg.ncols;
}
/* ck::check_act_call of the record of a -> the message of its refusal, null where it accepts.  configured 0: of an empty record;
 * now [nfields] (null: a's own): what the batch holds at the call, where that differs from what it held at the configure call */
extern "C" const char *emu_act_call_check(const emu_act_args *a, int configured, const ck::ObsField *now, int env0, int n) {
    std::vector<ck::ActCol> table;
    ck::ActCfg cfg = {};
    if (configured) if (const char *why = act_setup(*a, table, cfg)) return why;
    return ck::check_act_call(cfg, now ? now : a->fields, a->nfields, a->nenv, env0, n);
}
/* the record make_act_io builds for a launch, as numbers a test can read: {env0, n, ncols, delay_max, f32, act_f32, env_base, key0, key1,
 * cols passed, actions, sact, rows, srow, state, counts, delay, reset, nslots, ndst}, for every source slot {base, stride, f32} and for
 * every destination slot {base, stride} -> 0, -1 where the launcher would refuse */
extern "C" int emu_act_record(const emu_act_args *a, int env0, int n, const int *reset, unsigned long long *out) {
    typedef unsigned long long u64;
    std::vector<ck::ActCol> table;
    ck::ActCfg cfg;
    g_act_why = act_setup(*a, table, cfg);
    if (!g_act_why) g_act_why = ck::check_act_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_act_why) return -1;
    const ck::ActIO io = ck::make_act_io(cfg, a->fields, env0, n, reset);
    const u64 head[20] = {(u64)io.env0, (u64)io.n, (u64)io.ncols, (u64)io.delay_max, (u64)io.f32, (u64)io.act_f32, io.env_base, io.key0, io.key1,
                          io.cols != nullptr, (u64)(size_t)io.actions, (u64)io.sact, (u64)(size_t)io.rows, (u64)io.srow, (u64)(size_t)io.state,
                          (u64)(size_t)io.counts, (u64)(size_t)io.delay, (u64)(size_t)io.reset, (u64)cfg.nslots, (u64)cfg.ndst};
    memcpy(out, head, sizeof head);
    u64 *p = out + 20;
    for (int s = 0; s < ck::ACT_MAXSLOTS; ++s) { p[3 * s] = (u64)(size_t)io.src[s].base; p[3 * s + 1] = (u64)io.src[s].stride; p[3 * s + 2] = (u64)io.src[s].f32; }
    p += 3 * ck::ACT_MAXSLOTS;
    for (int s = 0; s < ck::ACT_MAXDST; ++s) { p[2 * s] = (u64)(size_t)io.dst[s].base; p[2 * s + 1] = (u64)io.dst[s].stride; }
    return 0;
}

static ck::ActIO g_actio;
static void body_act() { ck::cassie_act_kernel(g_actio); }

/* phys_batch_act on the emulator: one launch over [env0, env0 + n); reset: int32 [n] or null; grid 0: the launcher's.  -1 where the
 * launcher would refuse (emu_act_last_refusal has the message). */
extern "C" int emu_act(const emu_act_args *a, int env0, int n, const int *reset, int grid) {
    std::vector<ck::ActCol> table;
    ck::ActCfg cfg;
    g_act_why = act_setup(*a, table, cfg);
    if (!g_act_why && a->ncols == 0) g_act_why = "0 columns: nothing to launch (the launcher releases)";
    if (!g_act_why) g_act_why = ck::check_act_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_act_why) return -1;
    if (n == 0) return 0;
    g_actio = ck::make_act_io(cfg, a->fields, env0, n, reset);
    emu::run_grid(body_act, grid > 0 ? grid : ck::act_grid(n));
    return 0;
}
