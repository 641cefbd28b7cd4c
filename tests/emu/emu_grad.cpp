/*
 * emu_grad.cpp -- TEST-ONLY: the gradient rows (csrc/grad_kernels.h: cassie_grad_forward_kernel, _backward_kernel, _partial_kernel,
 * _reduce_kernel, _stats_kernel, _pack_kernel) on the wave emulator, configured, checked and launched as phys_batch.hip does it
 * (csrc/small_launch.h: policy_configure and the policy's load and bind checks, grad_configure, check_grad_bind, check_grad_call,
 * make_grad_io, make_grad_pack_io and the grids).  The policy's weights are packed anew by the pack kernels at every call; the rollout's
 * arrays and the gradient tensors are the caller's; the stores of the last call are kept here for emu_grad_fetch.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: the policy (as emu_policy_args: networks, layers' weights with strides and biases -- w null: never loaded --, normalisation,
 * log_std), the rollout's arrays with their strides in words {OBS, ACTION, LOGP, ADVN, RET} (null: missing), T and nenv, the gradient's
 * configuration, the minibatch, the caller's gradient tensors per slot 4 net + layer (null: the emulator's own) */
struct emu_grad_args {
    const ck::PolicyNetDef *nets; int nnets, in_dim, nenv, T;
    const float *w[8]; long long sw[8]; const float *b[8];
    const float *mean, *inv; double clip;
    const float *log_std;
    const float *src[5]; long long step[5], row[5];
    int max_m, chunk; double eps, c_v, c_ent;
    const int *idx; int m, pad;
    float *dw[8]; long long sdw[8]; float *db[8]; float *dls;
};

static const char *g_grad_why = nullptr;
extern "C" const char *emu_grad_last_refusal(void) { return g_grad_why; }

/* {GRAD_GRID, GRAD_PART_GRID, GRAD_RED_GRID, GRAD_MINCHUNK, GRAD_MAXCHUNK, GRAD_NSTATS, sizeof(emu_grad_args)}, for the binding's own checks */
extern "C" void emu_grad_constants(long long *out) {
    const long long a[7] = {ck::GRAD_GRID, ck::GRAD_PART_GRID, ck::GRAD_RED_GRID, ck::GRAD_MINCHUNK, ck::GRAD_MAXCHUNK, ck::GRAD_NSTATS,
                            (long long)sizeof(emu_grad_args)};
    memcpy(out, a, sizeof a);
}

/* the last call's record and stores */
static ck::PolicyCfg g_pol;
static ck::GradCfg g_cfg;
static int g_m = 0;
static std::vector<float> g_packed, g_act, g_delta, g_packt, g_own;
static std::vector<double> g_part, g_pos;

static ck::PolicyPackIO g_packio;
static void body_pack() { ck::cassie_policy_pack_kernel(g_packio); }
static ck::GradPackIO g_tpackio;
static void body_tpack() { ck::cassie_grad_pack_kernel(g_tpackio); }

/* what the launcher does between the configure calls and a launch */
static const char *grad_setup(const emu_grad_args &a, ck::GradSources &S) {
    ck::PolicyCfg &p = g_pol;
    if (const char *why = ck::policy_configure(a.nets, a.nnets, a.in_dim, p)) return why;
    const long long total = (long long)a.T * a.nenv;
    if (const char *why = ck::grad_configure(p, total, a.max_m, a.chunk, a.eps, a.c_v, a.c_ent, g_cfg)) return why;
    if (a.max_m == 0) return ck::GRAD_NOT_CONFIGURED;
    ck::GradCfg &c = g_cfg;
    g_packed.assign((size_t)p.packed_floats, 0.0f);
    p.packed = g_packed.data();
    /* (sentinels in the stores: what a call must overwrite or leave is visible) */
    g_act.assign((size_t)c.act_floats, -7.25f); g_delta.assign((size_t)c.delta_floats, -7.25f); g_packt.assign((size_t)c.packt_floats, -7.25f);
    g_own.assign((size_t)c.own_floats, -7.25f); g_part.assign((size_t)c.part_doubles, -7.25); g_pos.assign((size_t)c.pos_doubles + ck::GRAD_NSTATS, -7.25);
    c.act = g_act.data(); c.delta = g_delta.data(); c.packt = g_packt.data(); c.own = g_own.data(); c.part = g_part.data(); c.pos = g_pos.data();
    c.stats = g_pos.data() + c.pos_doubles;
    for (int n = 0; n < p.nnets; ++n)
        for (int l = 0; l < p.net[n].nlayers; ++l) {
            const int s = ck::POLICY_MAXLAYERS * n + l;
            if (a.dw[s] || a.db[s]) {
                if (const char *why = ck::check_grad_bind(c, p, n, l, a.dw[s], a.sdw[s], a.db[s])) return why;
                const int k = ck::grad_slot(c, n, l);
                c.dw[k] = a.dw[s]; c.sdw[k] = a.sdw[s]; c.db[k] = a.db[s];
            }
            if (!a.w[s]) continue;
            if (const char *why = ck::check_policy_load(p, n, l, a.w[s], a.sw[s], a.b[s])) return why;
            g_packio = ck::make_policy_pack_io(p, n, l, a.w[s], a.sw[s], a.b[s], p.packed + p.net[n].layer[l].w_off);
            emu::run_grid(body_pack, ck::policy_pack_grid(p.net[n].layer[l]));
            p.loaded |= ck::policy_layer_bit(n, l);
            g_tpackio = ck::make_grad_pack_io(c, p, n, l);
            emu::run_grid(body_tpack, ck::grad_pack_grid(g_tpackio));
        }
    c.dls = a.dls;
    if (a.mean || a.inv) {
        if (const char *why = ck::check_policy_bind_norm(p, a.mean, a.inv, a.clip)) return why;
        p.mean = a.mean; p.inv = a.inv; p.clip = a.clip;
    }
    p.log_std = a.log_std;
    /* the rollout's arrays: as grad_sources hands them on, from the caller's pointers */
    S = {};
    ck::GradSrc *dst[5] = {&S.obs, &S.action, &S.logp, &S.advn, &S.ret};
    const char *missing[5] = {"the rollout needs sources of role OBS, ACTION and LOGP", "the rollout needs sources of role OBS, ACTION and LOGP",
                              "the rollout needs sources of role OBS, ACTION and LOGP", "no ADVN (phys_batch_rollout_normalise first, or bind its storage)",
                              "no RET (phys_batch_rollout_finish first)"};
    for (int k = 0; k < 5; ++k) {
        if (!a.src[k]) { if (k < 4 || p.nnets > 1) return missing[k]; continue; }
        dst[k]->ptr = a.src[k]; dst[k]->step = a.step[k]; dst[k]->row = a.row[k];
    }
    S.total = (int)total;
    return nullptr;
}

/* the checks alone -> the message of the refusal, null where they accept */
extern "C" const char *emu_grad_check(const emu_grad_args *a) {
    ck::GradSources S;
    if (const char *why = grad_setup(*a, S)) return why;
    return ck::check_grad_call(g_cfg, g_pol, a->idx, a->m);
}

static ck::GradIO g_io;
static void body_fwd() { ck::cassie_grad_forward_kernel(g_io); }
static void body_bwd() { ck::cassie_grad_backward_kernel(g_io); }
static void body_part() { ck::cassie_grad_partial_kernel(g_io); }
static void body_red() { ck::cassie_grad_reduce_kernel(g_io); }
static void body_stats() { ck::cassie_grad_stats_kernel(g_io); }

/* phys_batch_grad on the emulator; grid > 0: that many workgroups for launches 1 to 4 in the place of the launcher's.  -1 where the
 * launcher would refuse (emu_grad_last_refusal has the message) */
extern "C" int emu_grad(const emu_grad_args *a, int grid) {
    ck::GradSources S;
    g_m = 0;
    g_grad_why = grad_setup(*a, S);
    if (!g_grad_why) g_grad_why = ck::check_grad_call(g_cfg, g_pol, a->idx, a->m);
    if (g_grad_why) return -1;
    g_io = ck::make_grad_io(g_cfg, g_pol, S, a->nenv, a->idx, a->m);
    emu::run_grid(body_fwd, grid > 0 ? grid : ck::grad_tile_grid(g_io), ck::POLICY_WAVES);
    if (ck::grad_has_backward(g_pol)) emu::run_grid(body_bwd, grid > 0 ? grid : ck::grad_tile_grid(g_io), ck::POLICY_WAVES);
    emu::run_grid(body_part, grid > 0 ? grid : ck::grad_partial_grid(g_io));
    emu::run_grid(body_red, grid > 0 ? grid : ck::grad_reduce_grid(g_io));
    emu::run_grid(body_stats, ck::grad_stats_grid(g_io));
    g_m = a->m;
    return 0;
}

/* what phys_batch_grad_download hands out of the last call, dense; host null: the count of elements alone (-1: no such thing).  what
 * GRAD_NSTATS + 0: the eight statistics */
extern "C" long long emu_grad_fetch(int what, int net, int layer, void *host) {
    const ck::GradCfg &c = g_cfg;
    const ck::PolicyCfg &p = g_pol;
    if (c.max_m < 1) return -1;
    if (what == ck::GRAD_NSTATS) { if (host) memcpy(host, c.stats, sizeof(double) * ck::GRAD_NSTATS); return ck::GRAD_NSTATS; }
    if (what == ck::GRAD_DLS) { if (host) memcpy(host, c.dls ? c.dls : c.own + c.own_ls, sizeof(float) * (size_t)c.A); return c.A; }
    if (net < 0 || net >= p.nnets) return -1;
    const ck::PolicyNet &N = p.net[net];
    const ck::GradNet &G = c.g[net];
    const long long m = g_m;
    if (what == ck::GRAD_ACT) {
        if (layer < 0 || layer > N.nlayers) return -1;
        const int w = layer == 0 ? p.in_dim : N.layer[layer - 1].out;
        if (host) for (long long r = 0; r < m; ++r) memcpy((float *)host + r * w, c.act + G.h_off[layer] + r * G.hw[layer], sizeof(float) * (size_t)w);
        return m * w;
    }
    if (layer < 0 || layer >= N.nlayers) return -1;
    const ck::PolicyLayer &L = N.layer[layer];
    const int s = ck::grad_slot(c, net, layer);
    switch (what) {
    case ck::GRAD_DW: {
        const float *src = c.dw[s] ? c.dw[s] : c.own + c.own_w[s];
        const long long st = c.dw[s] ? c.sdw[s] : L.in;
        if (host) for (int u = 0; u < L.out; ++u) memcpy((float *)host + (long long)u * L.in, src + u * st, sizeof(float) * (size_t)L.in);
        return (long long)L.out * L.in;
    }
    case ck::GRAD_DB: if (host) memcpy(host, c.db[s] ? c.db[s] : c.own + c.own_b[s], sizeof(float) * (size_t)L.out); return L.out;
    case ck::GRAD_DELTA:
        if (host) for (long long r = 0; r < m; ++r) memcpy((float *)host + r * L.out, c.delta + G.d_off[layer] + r * L.out16, sizeof(float) * (size_t)L.out);
        return m * L.out;
    case ck::GRAD_PARTIAL: {
        const long long n = (m + c.chunk - 1) / c.chunk * L.out * (L.in + 1);
        if (host) memcpy(host, c.part + G.p_off[layer], sizeof(double) * (size_t)n);
        return n;
    }
    case ck::GRAD_PACKT: {
        const long long n = (long long)G.hw[layer] * ((L.out + 3) & ~3);
        if (host) memcpy(host, c.packt + G.t_off[layer], sizeof(float) * (size_t)n);
        return n;
    }
    default: return -1;
    }
}

/* the padded rows of the last call's stores as they lie (for the sentinel checks): what GRAD_ACT or GRAD_DELTA -> rows [mcap of the
 * configuration][row width], the count of floats returned; width (non-null): the row width */
extern "C" long long emu_grad_fetch_raw(int what, int net, int layer, float *host, int *width) {
    const ck::GradCfg &c = g_cfg;
    if (c.max_m < 1 || net < 0 || net >= g_pol.nnets) return -1;
    const ck::GradNet &G = c.g[net];
    const int nl = g_pol.net[net].nlayers;
    if (what == ck::GRAD_ACT && layer >= 0 && layer <= nl) {
        if (width) *width = G.hw[layer];
        if (host) memcpy(host, c.act + G.h_off[layer], sizeof(float) * (size_t)c.mcap * (size_t)G.hw[layer]);
        return (long long)c.mcap * G.hw[layer];
    }
    if (what == ck::GRAD_DELTA && layer >= 0 && layer < nl) {
        const int w = g_pol.net[net].layer[layer].out16;
        if (width) *width = w;
        if (host) memcpy(host, c.delta + G.d_off[layer], sizeof(float) * (size_t)c.mcap * (size_t)w);
        return (long long)c.mcap * w;
    }
    return -1;
}
