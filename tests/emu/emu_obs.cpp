/*
 * emu_obs.cpp -- TEST-ONLY: the observation rows (csrc/obs_kernels.h: cassie_obs_kernel, philox4x32_10) on the wave emulator,
 * configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h: obs_configure, check_obs_bind, check_obs_input,
 * check_obs_call, make_obs_io, obs_grid).  The emulator keeps nothing between calls: the rows and the frame counts are the caller's
 * arrays, as they are the batch's buffers on the device.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: what the batch holds of every field (fields [nfields]; depth_field: PHYS_F_DEPTH), the configuration, the bound input
 * (null: none), the rows with their stride in elements and the counts [nenv] */
struct emu_obs_args {
    const ck::ObsField *fields; int nfields, depth_field, nenv;
    const ck::ObsTerm *terms; int nterms, history, dtype; unsigned long long seed; unsigned env_base;
    const void *input; int input_dim; long long input_stride; int input_dtype;
    void *rows; long long srow; unsigned *frames;
};

static const char *g_obs_why = nullptr;
extern "C" const char *emu_obs_last_refusal(void) { return g_obs_why; }

/* {OBS_GRID, OBS_MAXCOLS, OBS_MAXHISTORY, OBS_MAXROW, OBS_MAXSLOTS, sizeof(ObsTerm), sizeof(ObsCol), sizeof(emu_obs_args)}, for the binding's own checks */
extern "C" void emu_obs_constants(long long *out) {
    const long long a[8] = {ck::OBS_GRID, ck::OBS_MAXCOLS, ck::OBS_MAXHISTORY, ck::OBS_MAXROW, ck::OBS_MAXSLOTS, (long long)sizeof(ck::ObsTerm),
                            (long long)sizeof(ck::ObsCol), (long long)sizeof(emu_obs_args)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_obs_grid(int n) { return ck::obs_grid(n); }
/* the kernel's own Philox routine and its map of a word to (-1, 1) */
extern "C" void emu_obs_philox(const unsigned *counter, const unsigned *key, unsigned *out) {
    ck::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
}
extern "C" double emu_obs_uniform(unsigned w) { return ck::obs_uniform(w); }

/* what the launcher does between a configure call and a launch: the checked record with the column table, then the bindings */
static const char *obs_setup(const emu_obs_args &a, std::vector<ck::ObsCol> &table, std::vector<int> &term_col, ck::ObsCfg &cfg) {
    std::vector<int> dims((size_t)(a.nfields > 0 ? a.nfields : 1), 0);
    for (int k = 0; k < a.nfields; ++k) dims[k] = a.fields[k].base ? a.fields[k].dim : 0;
    table.assign((size_t)ck::OBS_MAXCOLS, ck::ObsCol());
    term_col.assign((size_t)(a.nterms > 0 ? a.nterms : 1), 0);
    if (const char *why = ck::obs_configure(dims.data(), a.nfields, a.depth_field, a.terms, a.nterms, a.history, a.dtype, a.seed, a.env_base,
                                            table.data(), term_col.data(), cfg)) return why;
    if (a.nterms == 0) return nullptr;
    cfg.cols = table.data(); cfg.frames = a.frames;
    if (a.rows) {
        if (const char *why = ck::check_obs_bind(cfg, a.srow)) return why;
        cfg.rows = a.rows; cfg.srow = a.srow;
    }
    if (a.input) {
        if (const char *why = ck::check_obs_input(cfg, a.input_dim, a.input_stride, a.input_dtype)) return why;
        cfg.input = a.input; cfg.input_dim = a.input_dim; cfg.input_stride = (int)a.input_stride; cfg.input_dtype = a.input_dtype;
    }
    return nullptr;
}

/* obs_configure and the bind checks alone -> the message of the refusal, null where they accept; ints (may be null): {nterms, ncols,
 * history, dtype, nslots, input_need} of the record, then slot_field [16] and slot_dim [16]; term_col [nterms] (may be null) */
extern "C" const char *emu_obs_check(const emu_obs_args *a, long long *ints, int *term_col) {
    std::vector<ck::ObsCol> table;
    std::vector<int> first;
    ck::ObsCfg cfg;
    const char *why = obs_setup(*a, table, first, cfg);
    if (why) return why;
    if (ints) {
        const long long head[6] = {cfg.nterms, cfg.ncols, cfg.history, cfg.dtype, cfg.nslots, cfg.input_need};
        memcpy(ints, head, sizeof head);
        for (int s = 0; s < ck::OBS_MAXSLOTS; ++s) { ints[6 + s] = cfg.slot_field[s]; ints[6 + ck::OBS_MAXSLOTS + s] = cfg.slot_dim[s]; }
    }
    if (term_col) for (int t = 0; t < a->nterms; ++t) term_col[t] = first[t];
    return nullptr;
}
/* the column table of a configuration -> ncols (-1: refused); cols [OBS_MAXCOLS] */
extern "C" int emu_obs_columns(const emu_obs_args *a, ck::ObsCol *cols) {
    std::vector<ck::ObsCol> table;
    std::vector<int> first;
    ck::ObsCfg cfg;
    g_obs_why = obs_setup(*a, table, first, cfg);
    if (g_obs_why) return -1;
    memcpy(cols, table.data(), sizeof(ck::ObsCol) * (size_t)cfg.ncols);
    return cfg.ncols;
}
/* ck::check_obs_call of the record of a -> the message of its refusal, null where it accepts.  configured 0: of an empty record;
 * now [nfields] (null: a's own): what the batch holds at the call, where that differs from what it held at the configure call */
extern "C" const char *emu_obs_call_check(const emu_obs_args *a, int configured, const ck::ObsField *now, int env0, int n) {
    std::vector<ck::ObsCol> table;
    std::vector<int> first;
    ck::ObsCfg cfg = {};
    if (configured) if (const char *why = obs_setup(*a, table, first, cfg)) return why;
    return ck::check_obs_call(cfg, now ? now : a->fields, a->nfields, a->nenv, env0, n);
}
/* the record make_obs_io builds for a launch, as numbers a test can read: {env0, n, ncols, history, f32, env_base, key0, key1, cols passed,
 * rows, srow, frames, refill} and for every slot {base, stride, f32} */
extern "C" int emu_obs_record(const emu_obs_args *a, int env0, int n, const int *refill, unsigned long long *out) {
    std::vector<ck::ObsCol> table;
    std::vector<int> first;
    ck::ObsCfg cfg;
    g_obs_why = obs_setup(*a, table, first, cfg);
    if (!g_obs_why) g_obs_why = ck::check_obs_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_obs_why) return -1;
    const ck::ObsIO io = ck::make_obs_io(cfg, a->fields, env0, n, refill);
    const unsigned long long head[13] = {(unsigned long long)io.env0, (unsigned long long)io.n, (unsigned long long)io.ncols, (unsigned long long)io.history,
                                         (unsigned long long)io.f32, io.env_base, io.key0, io.key1, io.cols != nullptr, (unsigned long long)(size_t)io.rows,
                                         (unsigned long long)io.srow, (unsigned long long)(size_t)io.frames, (unsigned long long)(size_t)io.refill};
    memcpy(out, head, sizeof head);
    for (int s = 0; s < ck::OBS_MAXSLOTS; ++s) {
        out[13 + 3 * s] = (unsigned long long)(size_t)io.src[s].base; out[14 + 3 * s] = (unsigned long long)io.src[s].stride; out[15 + 3 * s] = (unsigned long long)io.src[s].f32;
    }
    return cfg.nslots;
}

static ck::ObsIO g_obsio;
static void body_obs() { ck::cassie_obs_kernel(g_obsio); }

/* phys_batch_obs on the emulator: one launch over [env0, env0 + n); refill: int32 [n] or null; grid 0: the launcher's.  -1 where the
 * launcher would refuse (emu_obs_last_refusal has the message). */
extern "C" int emu_obs(const emu_obs_args *a, int env0, int n, const int *refill, int grid) {
    std::vector<ck::ObsCol> table;
    std::vector<int> first;
    ck::ObsCfg cfg;
    g_obs_why = obs_setup(*a, table, first, cfg);
    if (!g_obs_why && a->nterms == 0) g_obs_why = "0 terms: nothing to launch (the launcher releases)";
    if (!g_obs_why) g_obs_why = ck::check_obs_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_obs_why) return -1;
    if (n == 0) return 0;
    g_obsio = ck::make_obs_io(cfg, a->fields, env0, n, refill);
    emu::run_grid(body_obs, grid > 0 ? grid : ck::obs_grid(n));
    return 0;
}
