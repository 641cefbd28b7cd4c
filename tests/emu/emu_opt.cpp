/*
 * emu_opt.cpp -- TEST-ONLY: the optimiser rows (csrc/opt_kernels.h: cassie_opt_sq_kernel, _scalars_kernel, _step_kernel) on the wave
 * emulator, configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h: policy_configure, grad_configure,
 * opt_configure, check_opt_bind_param, check_opt_bind_log_std, check_opt_step, make_opt_io and the grids).  Every array is the caller's:
 * the master tensors, the gradients, and what the batch owns on the device -- the packed weights, the transposed packing, the moments,
 * the partials and the doubles --, so the library keeps nothing from call to call.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: the networks; per slot 4 net + layer the master tensors (null: not bound) and the gradients; the bits of the layers that
 * count as loaded; log_std as phys_batch_policy_bind_sample names it and as phys_batch_opt_bind_log_std is handed it; the optimiser's
 * configuration and the call's lr; whether a grad call has been made; grid > 0: that many workgroups for launches 1 and 3 in the place of
 * the launcher's; the batch's arrays (emu_opt_sizes says how large) */
struct emu_opt_args {
    const ck::PolicyNetDef *nets; int nnets, in_dim;
    float *w[8]; long long sw[8]; float *b[8];
    unsigned loaded; int pad;
    const float *log_std; float *opt_ls;
    float *dw[8]; long long sdw[8]; float *db[8]; float *dls;
    double beta1, beta2, eps, max_norm, lr;
    int grad_called, grid;
    float *packed, *packt, *mom; double *part, *sc;
};

static const char *g_opt_why = nullptr;
extern "C" const char *emu_opt_last_refusal(void) { return g_opt_why; }

/* {OPT_SEG, OPT_SQ_GRID, OPT_STEP_GRID, OPT_NSTATS, OPT_SC_COUNT, OPT_SC_T, sizeof(emu_opt_args)}, for the binding's own checks */
extern "C" void emu_opt_constants(long long *out) {
    const long long a[7] = {ck::OPT_SEG, ck::OPT_SQ_GRID, ck::OPT_STEP_GRID, ck::OPT_NSTATS, ck::OPT_SC_COUNT, ck::OPT_SC_T, (long long)sizeof(emu_opt_args)};
    memcpy(out, a, sizeof a);
}

static ck::PolicyCfg g_pol;
static ck::GradCfg g_grad;
static ck::OptCfg g_cfg;
static std::vector<float> g_own;

/* what the launcher does between the configure calls and a launch */
static const char *opt_setup(const emu_opt_args &a) {
    ck::PolicyCfg &p = g_pol;
    if (const char *why = ck::policy_configure(a.nets, a.nnets, a.in_dim, p)) return why;
    if (p.nnets < 1) return ck::OPT_NEEDS;
    if (const char *why = ck::grad_configure(p, 16, 16, 16, 0.2, 0.5, 0.0, g_grad)) return why;   /* (the slots and the layout of the transposed packing) */
    ck::GradCfg &g = g_grad;
    g_own.assign((size_t)g.own_floats, 0.0f);
    p.packed = a.packed; p.loaded = a.loaded; p.log_std = a.log_std;
    g.packt = a.packt; g.own = g_own.data();
    for (int n = 0; n < p.nnets; ++n)
        for (int l = 0; l < p.net[n].nlayers; ++l) {
            const int s = ck::POLICY_MAXLAYERS * n + l, k = ck::grad_slot(g, n, l);
            if (a.dw[s] || a.db[s]) {
                if (const char *why = ck::check_grad_bind(g, p, n, l, a.dw[s], a.sdw[s], a.db[s])) return why;
                g.dw[k] = a.dw[s]; g.sdw[k] = a.sdw[s]; g.db[k] = a.db[s];
            }
        }
    g.dls = a.dls;
    if (const char *why = ck::opt_configure(g, p, a.beta1, a.beta2, a.eps, a.max_norm, g_cfg)) return why;
    ck::OptCfg &c = g_cfg;
    if (!c.on) return ck::OPT_NOT_CONFIGURED;
    c.mom = a.mom; c.part = a.part; c.sc = a.sc;
    for (int n = 0; n < p.nnets; ++n)
        for (int l = 0; l < p.net[n].nlayers; ++l) {
            const int s = ck::POLICY_MAXLAYERS * n + l, k = ck::grad_slot(g, n, l);
            if (!a.w[s] && !a.b[s]) continue;
            if (const char *why = ck::check_opt_bind_param(c, p, n, l, a.w[s], a.sw[s], a.b[s])) return why;
            c.w[k] = a.w[s]; c.sw[k] = a.sw[s]; c.b[k] = a.b[s];
        }
    if (a.opt_ls) {
        if (const char *why = ck::check_opt_bind_log_std(c, p, a.opt_ls)) return why;
        c.ls = a.opt_ls;
    }
    return nullptr;
}

/* {the packed floats, the transposed packing's floats, Q, the segments, the doubles}; -1 where the configuration is refused */
extern "C" int emu_opt_sizes(const emu_opt_args *a, long long *out) {
    emu_opt_args b = *a;
    b.opt_ls = nullptr;
    for (int s = 0; s < 8; ++s) { b.w[s] = nullptr; b.b[s] = nullptr; }
    g_opt_why = opt_setup(b);
    if (g_opt_why) return -1;
    const long long r[5] = {g_pol.packed_floats, g_grad.packt_floats, g_cfg.Q, g_cfg.nseg, ck::OPT_SC_COUNT};
    memcpy(out, r, sizeof r);
    return 0;
}

static ck::PolicyPackIO g_packio;
static void body_pack() { ck::cassie_policy_pack_kernel(g_packio); }
static ck::GradPackIO g_tpackio;
static void body_tpack() { ck::cassie_grad_pack_kernel(g_tpackio); }

/* phys_batch_policy_load of every layer in a->loaded from the master tensors (both packings), and phys_batch_opt_configure's state: the
 * moments +0.0, t = 0, p1 = p2 = 1 */
extern "C" int emu_opt_begin(const emu_opt_args *a) {
    g_opt_why = opt_setup(*a);
    if (g_opt_why) return -1;
    ck::PolicyCfg &p = g_pol;
    for (int n = 0; n < p.nnets; ++n)
        for (int l = 0; l < p.net[n].nlayers; ++l) {
            const int s = ck::POLICY_MAXLAYERS * n + l;
            if (!(a->loaded & ck::policy_layer_bit(n, l))) continue;
            if ((g_opt_why = ck::check_policy_load(p, n, l, a->w[s], a->sw[s], a->b[s]))) return -1;
            g_packio = ck::make_policy_pack_io(p, n, l, a->w[s], a->sw[s], a->b[s], p.packed + p.net[n].layer[l].w_off);
            emu::run_grid(body_pack, ck::policy_pack_grid(p.net[n].layer[l]));
            g_tpackio = ck::make_grad_pack_io(g_grad, p, n, l);
            emu::run_grid(body_tpack, ck::grad_pack_grid(g_tpackio));
        }
    memset(a->mom, 0, sizeof(float) * 2 * (size_t)g_cfg.Q);
    ck::opt_initial_scalars(a->sc);
    return 0;
}

/* the checks alone -> the message of the refusal, null where they accept */
extern "C" const char *emu_opt_check(const emu_opt_args *a) {
    if (const char *why = opt_setup(*a)) return why;
    return ck::check_opt_step(g_cfg, g_grad, g_pol, a->lr, a->grad_called != 0);
}

static ck::OptIO g_io;
static void body_sq() { ck::cassie_opt_sq_kernel(g_io); }
static void body_scalars() { ck::cassie_opt_scalars_kernel(g_io); }
static void body_step() { ck::cassie_opt_step_kernel(g_io); }

/* phys_batch_opt_step on the emulator.  -1 where the launcher would refuse (emu_opt_last_refusal has the message) */
extern "C" int emu_opt_step(const emu_opt_args *a) {
    g_opt_why = opt_setup(*a);
    if (!g_opt_why) g_opt_why = ck::check_opt_step(g_cfg, g_grad, g_pol, a->lr, a->grad_called != 0);
    if (g_opt_why) return -1;
    g_io = ck::make_opt_io(g_cfg, g_grad, g_pol, a->lr);
    emu::run_grid(body_sq, a->grid > 0 ? a->grid : ck::opt_sq_grid(g_io));
    emu::run_grid(body_scalars, 1);
    emu::run_grid(body_step, a->grid > 0 ? a->grid : ck::opt_step_grid(g_io));
    return 0;
}

/* where phys_batch_opt_download / _upload find `what` among the caller's arrays: the element offset into mom (or sc, part), the rows,
 * their width and pitch -> 0, or -1: no such thing */
extern "C" int emu_opt_region(const emu_opt_args *a, int what, int net, int layer, long long *out) {
    g_opt_why = opt_setup(*a);
    if (g_opt_why) return -1;
    ck::OptRegion R;
    if (!ck::opt_region(g_cfg, g_grad, g_pol, what, net, layer, R)) return -1;
    const long long off = R.doubles ? (what == ck::OPT_SCALARS ? (double *)R.ptr - a->sc : (double *)R.ptr - a->part) : (float *)R.ptr - a->mom;
    const long long r[4] = {off, R.rows, R.width, R.pitch};
    memcpy(out, r, sizeof r);
    return 0;
}
