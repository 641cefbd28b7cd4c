/*
 * emu_policy.cpp -- TEST-ONLY: the policy rows (csrc/policy_kernels.h: cassie_policy_kernel, cassie_policy_pack_kernel) on the wave
 * emulator, configured, checked, packed and launched as phys_batch.hip does it (csrc/small_launch.h: policy_configure,
 * check_policy_load, check_policy_bind_*, check_policy_call, make_policy_io, make_policy_pack_io, policy_grid, policy_pack_grid).  The
 * emulator keeps nothing between calls: the packed weights are made anew from the caller's layers by the pack kernel itself, and the
 * input, the outputs and the sample are the caller's arrays.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: the networks, the layers' weights (w[POLICY_MAXLAYERS net + layer] null: never loaded) with their row strides and biases, the
 * bound input, normalisation (mean null: none), outputs (null: none) and sample (eps null: none) */
struct emu_policy_args {
    const ck::PolicyNetDef *nets; int nnets, in_dim, nenv;
    const float *w[8]; long long sw[8]; const float *b[8];
    const void *x; int x_dim; long long sx; int x_dtype;
    const float *mean, *inv; double clip;
    float *out[2]; long long sout[2];
    const float *eps; long long seps; const float *log_std; float *action; long long saction; float *logp;
};

static const char *g_pol_why = nullptr;
extern "C" const char *emu_policy_last_refusal(void) { return g_pol_why; }

/* {POLICY_GRID, POLICY_TILE, POLICY_WAVES, POLICY_MAXNETS, POLICY_MAXLAYERS, POLICY_MAXDIM, POLICY_MAXOUT, sizeof(PolicyNetDef),
 * sizeof(emu_policy_args)}, for the binding's own checks */
extern "C" void emu_policy_constants(long long *out) {
    const long long a[9] = {ck::POLICY_GRID, ck::POLICY_TILE, ck::POLICY_WAVES, ck::POLICY_MAXNETS, ck::POLICY_MAXLAYERS, ck::POLICY_MAXDIM,
                            ck::POLICY_MAXOUT, (long long)sizeof(ck::PolicyNetDef), (long long)sizeof(emu_policy_args)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_policy_grid(int n, int nnets) { return ck::policy_grid(n, nnets); }

static ck::PolicyPackIO g_packio;
static void body_pack() { ck::cassie_policy_pack_kernel(g_packio); }

/* what the launcher does between a configure call and a launch: the checked record, the layers packed by the pack kernel, the bindings */
static const char *policy_setup(const emu_policy_args &a, std::vector<float> &packed, ck::PolicyCfg &cfg) {
    if (const char *why = ck::policy_configure(a.nets, a.nnets, a.in_dim, cfg)) return why;
    if (a.nnets == 0) return nullptr;
    packed.assign((size_t)cfg.packed_floats, 0.0f);
    cfg.packed = packed.data();
    for (int n = 0; n < cfg.nnets; ++n)
        for (int l = 0; l < cfg.net[n].nlayers; ++l) {
            const int s = ck::POLICY_MAXLAYERS * n + l;
            if (!a.w[s]) continue;
            if (const char *why = ck::check_policy_load(cfg, n, l, a.w[s], a.sw[s], a.b[s])) return why;
            g_packio = ck::make_policy_pack_io(cfg, n, l, a.w[s], a.sw[s], a.b[s], cfg.packed + cfg.net[n].layer[l].w_off);
            emu::run_grid(body_pack, ck::policy_pack_grid(cfg.net[n].layer[l]));
            cfg.loaded |= ck::policy_layer_bit(n, l);
        }
    if (a.x) {
        if (const char *why = ck::check_policy_bind_input(cfg, a.x_dim, a.sx, a.x_dtype)) return why;
        cfg.x = (const float *)a.x; cfg.sx = a.sx;
    }
    if (a.mean || a.inv) {
        if (const char *why = ck::check_policy_bind_norm(cfg, a.mean, a.inv, a.clip)) return why;
        cfg.mean = a.mean; cfg.inv = a.inv; cfg.clip = a.clip;
    }
    for (int n = 0; n < 2; ++n)
        if (a.out[n]) {
            if (const char *why = ck::check_policy_bind_output(cfg, n, a.sout[n])) return why;
            cfg.out[n] = a.out[n]; cfg.sout[n] = a.sout[n];
        }
    if (a.eps) {
        if (const char *why = ck::check_policy_bind_sample(cfg, a.seps, a.log_std, a.action, a.saction, a.logp)) return why;
        cfg.eps = a.eps; cfg.seps = a.seps; cfg.log_std = a.log_std; cfg.action = a.action; cfg.saction = a.saction; cfg.logp = a.logp;
    }
    return nullptr;
}

/* policy_configure, the load checks and the bind checks, then (call != 0) check_policy_call over [env0, env0 + n) -> the message of the
 * refusal, null where they accept.  configured 0: the call check of an empty record */
extern "C" const char *emu_policy_check(const emu_policy_args *a, int configured, int call, int env0, int n) {
    std::vector<float> packed;
    ck::PolicyCfg cfg = {};
    if (configured) if (const char *why = policy_setup(*a, packed, cfg)) return why;
    return call ? ck::check_policy_call(cfg, a->nenv, env0, n) : nullptr;
}
/* check_policy_load of an arbitrary (net, layer) of the configuration */
extern "C" const char *emu_policy_load_check(const emu_policy_args *a, int net, int layer, const float *w, long long sw, const float *b) {
    ck::PolicyCfg cfg = {};
    if (a->nnets > 0) if (const char *why = ck::policy_configure(a->nets, a->nnets, a->in_dim, cfg)) return why;
    return ck::check_policy_load(cfg, net, layer, w, sw, b);
}
/* the packed floats of a configuration -> their number (-1: refused); out (may be null) [that many]; offs (may be null): per (net,
 * layer) slot {w_off, b_off, k4, out16} */
extern "C" long long emu_policy_packed(const emu_policy_args *a, float *out, long long *offs) {
    std::vector<float> packed;
    ck::PolicyCfg cfg;
    g_pol_why = policy_setup(*a, packed, cfg);
    if (g_pol_why) return -1;
    if (out) memcpy(out, packed.data(), sizeof(float) * packed.size());
    if (offs)
        for (int n = 0; n < cfg.nnets; ++n)
            for (int l = 0; l < cfg.net[n].nlayers; ++l) {
                const ck::PolicyLayer &L = cfg.net[n].layer[l];
                long long *p = offs + 4 * (ck::POLICY_MAXLAYERS * n + l);
                p[0] = L.w_off; p[1] = L.b_off; p[2] = L.k4; p[3] = L.out16;
            }
    return cfg.packed_floats;
}

/* the dynamic LDS the launcher asks for (ck::policy_lds_bytes) -> bytes, -1: refused */
extern "C" long long emu_policy_lds_bytes(const emu_policy_args *a) {
    ck::PolicyCfg cfg;
    g_pol_why = ck::policy_configure(a->nets, a->nnets, a->in_dim, cfg);
    return g_pol_why ? -1 : (long long)ck::policy_lds_bytes(cfg);
}

static ck::PolicyIO g_polio;
static void body_policy() { ck::cassie_policy_kernel(g_polio); }

/* phys_batch_policy on the emulator: one launch over [env0, env0 + n); grid 0: the launcher's.  -1 where the launcher would refuse
 * (emu_policy_last_refusal has the message). */
extern "C" int emu_policy(const emu_policy_args *a, int env0, int n, int grid) {
    std::vector<float> packed;
    ck::PolicyCfg cfg;
    g_pol_why = policy_setup(*a, packed, cfg);
    if (!g_pol_why && a->nnets == 0) g_pol_why = "0 networks: nothing to launch (the launcher releases)";
    if (!g_pol_why) g_pol_why = ck::check_policy_call(cfg, a->nenv, env0, n);
    if (g_pol_why) return -1;
    if (n == 0) return 0;
    g_polio = ck::make_policy_io(cfg, env0, n);
    emu::run_grid(body_policy, grid > 0 ? grid : ck::policy_grid(n, cfg.nnets), ck::POLICY_WAVES);
    return 0;
}
