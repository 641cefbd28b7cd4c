/*
 * emu_rollout.cpp -- TEST-ONLY: the rollout rows (csrc/rollout_kernels.h: cassie_rollout_record_kernel, _finish_kernel, _reduce_kernel,
 * _square_kernel, _scale_kernel) on the wave emulator, configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h:
 * rollout_configure, check_rollout_bind_source, check_rollout_bind_storage, rollout_resolve, check_rollout_record / _finish / _normalise,
 * make_rollout_rec_io / _fin_io / _norm_io and the grids).  The emulator keeps nothing between calls: the stores, ADV, RET, ADVN and the
 * partials are the caller's arrays, and what an unbound source is resolved from is the `live` block the caller fills.
 */
#include <cstring>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: the configuration, the bound sources (null: resolved from live), the stores with their strides in words (every one the
 * caller's), ADV, RET, ADVN (null: none), the partials q [2 nenv + 4] (q1 | q2 | mean, std, inv, the last sum) and what the batch would
 * read or write now */
struct emu_rollout_args {
    const ck::RolloutSrcDef *srcs; int nsrcs, T, nenv; unsigned tmask;
    double gamma, lambda;
    const void *src[ck::ROLLOUT_MAXSRC]; long long ssrc[ck::ROLLOUT_MAXSRC];
    void *store[ck::ROLLOUT_MAXSRC]; long long step[ck::ROLLOUT_MAXSRC], row[ck::ROLLOUT_MAXSRC];
    void *arr[3]; long long arr_step[3], arr_row[3];     /* ADV, RET, ADVN */
    double *q;
    ck::RolloutLive live;
};

static const char *g_ro_why = nullptr;
extern "C" const char *emu_rollout_last_refusal(void) { return g_ro_why; }

/* {ROLLOUT_MAXT, _MAXSRC, _MAXDIM, _JOB, _GRID, _FIN_GRID, _SCALE_GRID, _AHEAD, sizeof(emu_rollout_args), sizeof(RolloutLive)}, for the
 * binding's own checks */
extern "C" void emu_rollout_constants(long long *out) {
    const long long a[10] = {ck::ROLLOUT_MAXT, ck::ROLLOUT_MAXSRC, ck::ROLLOUT_MAXDIM, ck::ROLLOUT_JOB, ck::ROLLOUT_GRID, ck::ROLLOUT_FIN_GRID,
                             ck::ROLLOUT_SCALE_GRID, ck::ROLLOUT_AHEAD, (long long)sizeof(emu_rollout_args), (long long)sizeof(ck::RolloutLive)};
    memcpy(out, a, sizeof a);
}

/* what the launcher does between a configure call and a launch: the checked record, the bindings */
static const char *rollout_setup(const emu_rollout_args &a, ck::RolloutCfg &cfg) {
    if (const char *why = ck::rollout_configure(a.srcs, a.nsrcs, a.T, a.gamma, a.lambda, a.tmask, cfg)) return why;
    if (a.nsrcs == 0) return nullptr;
    for (int s = 0; s < cfg.nsrc; ++s) {
        if (a.src[s]) {
            if (const char *why = ck::check_rollout_bind_source(cfg, s, a.src[s], a.ssrc[s])) return why;
            cfg.src[s] = a.src[s]; cfg.ssrc[s] = a.ssrc[s];
        }
        if (a.store[s]) {
            if (const char *why = ck::check_rollout_bind_storage(cfg, a.nenv, s, a.store[s], a.step[s], a.row[s])) return why;
            cfg.store[s] = {a.store[s], a.step[s], a.row[s]};
        }
    }
    const int roles[3] = {ck::RO_ADV, ck::RO_RET, ck::RO_ADVN};
    for (int k = 0; k < 3; ++k)
        if (a.arr[k]) {
            if (const char *why = ck::check_rollout_bind_storage(cfg, a.nenv, roles[k], a.arr[k], a.arr_step[k], a.arr_row[k])) return why;
            int dim;
            *ck::rollout_store_of(cfg, roles[k], dim) = {a.arr[k], a.arr_step[k], a.arr_row[k]};
        }
    if (a.q) { cfg.q1 = a.q; cfg.q2 = a.q + a.nenv; cfg.stats = a.q + 2 * (size_t)a.nenv; }
    return nullptr;
}

/* the checks of a call -> the message of the refusal, null where they accept.  what 0: configure and the bindings alone; 1: a record of
 * slot t over [env0, env0 + n); 2: a finish over the range with the last values (null: resolved); 3: a normalise.  configured 0: the
 * call's check of an empty record */
extern "C" const char *emu_rollout_check(const emu_rollout_args *a, int configured, int what, int t, int env0, int n, const void *last, long long stride, double eps) {
    ck::RolloutCfg cfg = {};
    if (configured) if (const char *why = rollout_setup(*a, cfg)) return why;
    if (what == 1) return ck::check_rollout_record(cfg, a->live, a->nenv, t, env0, n);
    if (what == 2) return ck::check_rollout_finish(cfg, a->live, a->nenv, env0, n, last, stride);
    if (what == 3) return ck::check_rollout_normalise(cfg, a->nenv, eps);
    return nullptr;
}

static ck::RolloutRecIO g_recio;
static void body_record() { ck::cassie_rollout_record_kernel(g_recio); }

/* phys_batch_rollout_record on the emulator: one launch; grid 0: the launcher's.  -1 where the launcher would refuse.  vec (may be
 * null) [nsrcs]: whether a source went 16 bytes a lane */
extern "C" int emu_rollout_record(const emu_rollout_args *a, int t, int env0, int n, int grid, int *vec) {
    ck::RolloutCfg cfg;
    g_ro_why = rollout_setup(*a, cfg);
    if (!g_ro_why) g_ro_why = ck::check_rollout_record(cfg, a->live, a->nenv, t, env0, n);
    if (g_ro_why) return -1;
    if (n == 0) return 0;
    g_recio = ck::make_rollout_rec_io(cfg, a->live, t, env0, n);
    if (vec) for (int s = 0; s < cfg.nsrc; ++s) vec[s] = g_recio.s[s].vec;
    emu::run_grid(body_record, grid > 0 ? grid : ck::rollout_record_grid(g_recio));
    return 0;
}

static ck::RolloutFinIO g_finio;
static void body_finish() { ck::cassie_rollout_finish_kernel(g_finio); }

/* phys_batch_rollout_finish on the emulator */
extern "C" int emu_rollout_finish(const emu_rollout_args *a, int env0, int n, const void *last, long long stride, int grid) {
    ck::RolloutCfg cfg;
    g_ro_why = rollout_setup(*a, cfg);
    if (!g_ro_why) g_ro_why = ck::check_rollout_finish(cfg, a->live, a->nenv, env0, n, last, stride);
    if (g_ro_why) return -1;
    if (n == 0) return 0;
    g_finio = ck::make_rollout_fin_io(cfg, a->live, env0, n, last, stride);
    emu::run_grid(body_finish, grid > 0 ? grid : ck::rollout_env_grid(n));
    return 0;
}

static ck::RolloutNormIO g_normio;
static void body_reduce() { ck::cassie_rollout_reduce_kernel(g_normio); }
static void body_square() { ck::cassie_rollout_square_kernel(g_normio); }
static void body_scale() { ck::cassie_rollout_scale_kernel(g_normio); }

/* phys_batch_rollout_normalise on the emulator: the launcher's four launches in its order (grid 0: its grids) */
extern "C" int emu_rollout_normalise(const emu_rollout_args *a, double eps, int grid) {
    ck::RolloutCfg cfg;
    g_ro_why = rollout_setup(*a, cfg);
    if (!g_ro_why) g_ro_why = ck::check_rollout_normalise(cfg, a->nenv, eps);
    if (g_ro_why) return -1;
    g_normio = ck::make_rollout_norm_io(cfg, a->nenv, eps, 0);
    emu::run_grid(body_reduce, 1);
    emu::run_grid(body_square, grid > 0 ? grid : ck::rollout_env_grid(a->nenv));
    g_normio = ck::make_rollout_norm_io(cfg, a->nenv, eps, 1);
    emu::run_grid(body_reduce, 1);
    emu::run_grid(body_scale, grid > 0 ? grid : ck::rollout_scale_grid(a->nenv, cfg.T));
    return 0;
}
