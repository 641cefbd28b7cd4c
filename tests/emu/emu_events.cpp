/*
 * emu_events.cpp -- TEST-ONLY: the event rows (csrc/event_kernels.h: cassie_event_kernel) on the wave emulator, configured, checked and
 * launched as phys_batch.hip does it (csrc/small_launch.h: events_configure, check_events_bind_rows, check_events_input,
 * check_events_bind_flags, check_events_call, make_events_io, events_grid).  The emulator keeps nothing between calls: the rows, the done
 * words, the state, the words and the call counts are the caller's arrays, as they are the batch's buffers on the device -- the state
 * and the words in the device's shape, [2][ncols][nenv] and [ncols][nenv].
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: what the batch holds of every field (fields [nfields]; depth_field: PHYS_F_DEPTH), the configuration, the bound input (null:
 * none), the rows (null: not bound) with their stride in elements, the done words [nenv], the state [2][ncols][nenv], the words
 * [ncols][nenv] and the counts [nenv] */
struct emu_events_args {
    const ck::ObsField *fields; int nfields, depth_field, nenv;
    const ck::EventCol *cols; int ncols, dtype; unsigned long long done_mask;
    const void *input; int input_dim; long long input_stride; int input_dtype;
    void *rows; long long srow; int *flags; double *state; unsigned *words; unsigned *counts;
};

static const char *g_events_why = nullptr;
extern "C" const char *emu_events_last_refusal(void) { return g_events_why; }

/* {EVENT_GRID, EVENT_MAXCOLS, EVENT_MAXCOUNT, EVENT_MAXSLOTS, sizeof(EventCol), sizeof(emu_events_args)}, for the binding's own checks */
extern "C" void emu_events_constants(long long *out) {
    const long long a[6] = {ck::EVENT_GRID, ck::EVENT_MAXCOLS, ck::EVENT_MAXCOUNT, ck::EVENT_MAXSLOTS, (long long)sizeof(ck::EventCol), (long long)sizeof(emu_events_args)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_events_grid(int n) { return ck::events_grid(n); }

/* what the launcher does between a configure call and a launch: the checked record with the column table, then the bindings */
static const char *events_setup(const emu_events_args &a, std::vector<ck::EventCol> &table, ck::EventCfg &cfg) {
    std::vector<int> dims((size_t)(a.nfields > 0 ? a.nfields : 1), 0);
    for (int k = 0; k < a.nfields; ++k) dims[k] = a.fields[k].base ? a.fields[k].dim : 0;
    table.assign((size_t)ck::EVENT_MAXCOLS, ck::EventCol());
    if (const char *why = ck::events_configure(dims.data(), a.nfields, a.depth_field, a.cols, a.ncols, a.dtype, a.done_mask, table.data(), cfg)) return why;
    if (a.ncols == 0) return nullptr;
    cfg.cols = table.data(); cfg.state = a.state; cfg.words = a.words; cfg.counts = a.counts;
    if (a.rows) {
        if (const char *why = ck::check_events_bind_rows(cfg, a.srow)) return why;
        cfg.rows = a.rows; cfg.srow = a.srow;
    }
    if (a.flags) {
        if (const char *why = ck::check_events_bind_flags(cfg)) return why;
        cfg.flags = a.flags;
    }
    if (a.input) {
        if (const char *why = ck::check_events_input(cfg, a.input_dim, a.input_stride, a.input_dtype)) return why;
        cfg.input = a.input; cfg.input_dim = a.input_dim; cfg.input_stride = (int)a.input_stride; cfg.input_dtype = a.input_dtype;
    }
    return nullptr;
}

/* events_configure and the bind checks alone -> the message of the refusal, null where they accept; ints (may be null): {ncols, dtype,
 * nslots, input_need} of the record, then slot_field [16] and slot_dim [16]; table_out [ncols] (may be null): the table a launch reads */
extern "C" const char *emu_events_check(const emu_events_args *a, long long *ints, ck::EventCol *table_out) {
    std::vector<ck::EventCol> table;
    ck::EventCfg cfg;
    const char *why = events_setup(*a, table, cfg);
    if (why) return why;
    if (ints) {
        const long long head[4] = {cfg.ncols, cfg.dtype, cfg.nslots, cfg.input_need};
        memcpy(ints, head, sizeof head);
        for (int s = 0; s < ck::EVENT_MAXSLOTS; ++s) { ints[4 + s] = cfg.slot_field[s]; ints[4 + ck::EVENT_MAXSLOTS + s] = cfg.slot_dim[s]; }
    }
    if (table_out) for (int t = 0; t < a->ncols; ++t) table_out[t] = table[t];
    return nullptr;
}
/* ck::check_events_call of the record of a -> the message of its refusal, null where it accepts.  configured 0: of an empty record;
 * now [nfields] (null: a's own): what the batch holds at the call, where that differs from what it held at the configure call */
extern "C" const char *emu_events_call_check(const emu_events_args *a, int configured, const ck::ObsField *now, int env0, int n) {
    std::vector<ck::EventCol> table;
    ck::EventCfg cfg = {};
    if (configured) if (const char *why = events_setup(*a, table, cfg)) return why;
    return ck::check_events_call(cfg, now ? now : a->fields, a->nfields, a->nenv, env0, n);
}

static ck::EventIO g_eventio;
static void body_events() { ck::cassie_event_kernel(g_eventio); }

/* phys_batch_events on the emulator: one launch over [env0, env0 + n); reset: int32 [n] or null; grid 0: the launcher's.  -1 where the
 * launcher would refuse (emu_events_last_refusal has the message). */
extern "C" int emu_events(const emu_events_args *a, int env0, int n, const int *reset, int grid) {
    std::vector<ck::EventCol> table;
    ck::EventCfg cfg;
    g_events_why = events_setup(*a, table, cfg);
    if (!g_events_why && a->ncols == 0) g_events_why = "0 columns: nothing to launch (the launcher releases)";
    if (!g_events_why) g_events_why = ck::check_events_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_events_why) return -1;
    if (n == 0) return 0;
    g_eventio = ck::make_events_io(cfg, a->fields, a->nenv, env0, n, reset);
    emu::run_grid(body_events, grid > 0 ? grid : ck::events_grid(n));
    return 0;
}
