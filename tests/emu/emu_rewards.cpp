/*
 * emu_rewards.cpp -- TEST-ONLY: the reward rows (csrc/reward_kernels.h: cassie_reward_kernel, reward_expn) on the wave emulator,
 * configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h: reward_configure, check_reward_bind,
 * check_reward_input, check_reward_call, make_reward_io, reward_grid).  The emulator keeps nothing between calls: the rewards, the term
 * rows and the returns are the caller's arrays, as they are the batch's buffers on the device.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: what the batch holds of every field (fields [nfields]; depth_field: PHYS_F_DEPTH), the configuration, the bound input (null:
 * none), the rewards with their stride in elements, the term rows (null: none) with theirs, the returns and final returns [nenv] */
struct emu_reward_args {
    const ck::ObsField *fields; int nfields, depth_field, nenv;
    const ck::RewardTerm *terms; int nterms, dtype; double lo, hi;
    const void *input; int input_dim; long long input_stride; int input_dtype;
    void *rew; long long srew; void *trows; long long sterm; double *ret, *fin;
};

static const char *g_reward_why = nullptr;
extern "C" const char *emu_reward_last_refusal(void) { return g_reward_why; }

/* {REWARD_GRID, REWARD_MAXTERMS, REWARD_MAXCOUNT, REWARD_MAXSLOTS, sizeof(RewardTerm), sizeof(emu_reward_args)}, for the binding's own checks */
extern "C" void emu_reward_constants(long long *out) {
    const long long a[6] = {ck::REWARD_GRID, ck::REWARD_MAXTERMS, ck::REWARD_MAXCOUNT, ck::REWARD_MAXSLOTS, (long long)sizeof(ck::RewardTerm), (long long)sizeof(emu_reward_args)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_reward_grid(int n) { return ck::reward_grid(n); }
/* the kernel's own expn on an array */
extern "C" void emu_reward_expn(const double *a, double *out, long long n) { for (long long i = 0; i < n; ++i) out[i] = ck::reward_expn(a[i]); }

/* what the launcher does between a configure call and a launch: the checked record with the term table, then the bindings */
static const char *reward_setup(const emu_reward_args &a, std::vector<ck::RewardTerm> &table, ck::RewardCfg &cfg) {
    std::vector<int> dims((size_t)(a.nfields > 0 ? a.nfields : 1), 0);
    for (int k = 0; k < a.nfields; ++k) dims[k] = a.fields[k].base ? a.fields[k].dim : 0;
    table.assign((size_t)ck::REWARD_MAXTERMS, ck::RewardTerm());
    if (const char *why = ck::reward_configure(dims.data(), a.nfields, a.depth_field, a.terms, a.nterms, a.dtype, a.lo, a.hi, table.data(), cfg)) return why;
    if (a.nterms == 0) return nullptr;
    cfg.terms = table.data(); cfg.ret = a.ret; cfg.fin = a.fin;
    if (a.rew) {
        if (const char *why = ck::check_reward_bind(cfg, a.srew, 1)) return why;
        cfg.rew = a.rew; cfg.srew = a.srew;
    }
    if (a.trows) {
        if (const char *why = ck::check_reward_bind(cfg, a.sterm, cfg.nterms)) return why;
        cfg.trows = a.trows; cfg.sterm = a.sterm;
    }
    if (a.input) {
        if (const char *why = ck::check_reward_input(cfg, a.input_dim, a.input_stride, a.input_dtype)) return why;
        cfg.input = a.input; cfg.input_dim = a.input_dim; cfg.input_stride = (int)a.input_stride; cfg.input_dtype = a.input_dtype;
    }
    return nullptr;
}

/* reward_configure and the bind checks alone -> the message of the refusal, null where they accept; ints (may be null): {nterms, dtype,
 * nslots, input_need} of the record, then slot_field [16] and slot_dim [16]; table [nterms] (may be null): the terms with their slots */
extern "C" const char *emu_reward_check(const emu_reward_args *a, long long *ints, ck::RewardTerm *table_out) {
    std::vector<ck::RewardTerm> table;
    ck::RewardCfg cfg;
    const char *why = reward_setup(*a, table, cfg);
    if (why) return why;
    if (ints) {
        const long long head[4] = {cfg.nterms, cfg.dtype, cfg.nslots, cfg.input_need};
        memcpy(ints, head, sizeof head);
        for (int s = 0; s < ck::REWARD_MAXSLOTS; ++s) { ints[4 + s] = cfg.slot_field[s]; ints[4 + ck::REWARD_MAXSLOTS + s] = cfg.slot_dim[s]; }
    }
    if (table_out) for (int t = 0; t < a->nterms; ++t) table_out[t] = table[t];
    return nullptr;
}
/* ck::check_reward_call of the record of a -> the message of its refusal, null where it accepts.  configured 0: of an empty record;
 * now [nfields] (null: a's own): what the batch holds at the call, where that differs from what it held at the configure call */
extern "C" const char *emu_reward_call_check(const emu_reward_args *a, int configured, const ck::ObsField *now, int env0, int n) {
    std::vector<ck::RewardTerm> table;
    ck::RewardCfg cfg = {};
    if (configured) if (const char *why = reward_setup(*a, table, cfg)) return why;
    return ck::check_reward_call(cfg, now ? now : a->fields, a->nfields, a->nenv, env0, n);
}
/* the record make_reward_io builds for a launch, as numbers a test can read: {env0, n, nterms, f32, terms passed, rew, srew, trows, sterm,
 * ret, fin, reset}, lo and hi as their bits, and for every slot {base, stride, f32} */
extern "C" int emu_reward_record(const emu_reward_args *a, int env0, int n, const int *reset, unsigned long long *out) {
    std::vector<ck::RewardTerm> table;
    ck::RewardCfg cfg;
    g_reward_why = reward_setup(*a, table, cfg);
    if (!g_reward_why) g_reward_why = ck::check_reward_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_reward_why) return -1;
    const ck::RewardIO io = ck::make_reward_io(cfg, a->fields, env0, n, reset);
    unsigned long long lo, hi;
    memcpy(&lo, &io.lo, 8); memcpy(&hi, &io.hi, 8);
    const unsigned long long head[14] = {(unsigned long long)io.env0, (unsigned long long)io.n, (unsigned long long)io.nterms, (unsigned long long)io.f32,
                                         io.terms != nullptr, (unsigned long long)(size_t)io.rew, (unsigned long long)io.srew, (unsigned long long)(size_t)io.trows,
                                         (unsigned long long)io.sterm, (unsigned long long)(size_t)io.ret, (unsigned long long)(size_t)io.fin,
                                         (unsigned long long)(size_t)io.reset, lo, hi};
    memcpy(out, head, sizeof head);
    for (int s = 0; s < ck::REWARD_MAXSLOTS; ++s) {
        out[14 + 3 * s] = (unsigned long long)(size_t)io.src[s].base; out[15 + 3 * s] = (unsigned long long)io.src[s].stride; out[16 + 3 * s] = (unsigned long long)io.src[s].f32;
    }
    return cfg.nslots;
}

static ck::RewardIO g_rewardio;
static void body_reward() { ck::cassie_reward_kernel(g_rewardio); }

/* phys_batch_reward on the emulator: one launch over [env0, env0 + n); reset: int32 [n] or null; grid 0: the launcher's.  -1 where the
 * launcher would refuse (emu_reward_last_refusal has the message). */
extern "C" int emu_reward(const emu_reward_args *a, int env0, int n, const int *reset, int grid) {
    std::vector<ck::RewardTerm> table;
    ck::RewardCfg cfg;
    g_reward_why = reward_setup(*a, table, cfg);
    if (!g_reward_why && a->nterms == 0) g_reward_why = "0 terms: nothing to launch (the launcher releases)";
    if (!g_reward_why) g_reward_why = ck::check_reward_call(cfg, a->fields, a->nfields, a->nenv, env0, n);
    if (g_reward_why) return -1;
    if (n == 0) return 0;
    g_rewardio = ck::make_reward_io(cfg, a->fields, env0, n, reset);
    emu::run_grid(body_reward, grid > 0 ? grid : ck::reward_grid(n));
    return 0;
}
