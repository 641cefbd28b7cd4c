/*
 * emu_draw.cpp -- TEST-ONLY: the draw rows (csrc/draw_kernels.h: cassie_draw_kernel, cassie_draw_perm_kernel) on the wave emulator,
 * configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h: draw_configure, check_draw_bind, check_draw_bind_perm,
 * check_draw, check_draw_perm, make_draw_io, make_draw_perm_io and the grids).  Every array is the caller's: the destinations, and what
 * the batch owns on the device -- the counts and the permutation --, so the library keeps nothing from call to call.
 */
#include <cstring>

#include "small_launch.h"
#include "emu_runtime.h"

/* a call: the configuration; the bound destinations (dst null: resolved from the policy below; perm_dst null: the batch's own); what the
 * batch would resolve the rows from -- a policy (pol_A 0: none) whose actor has pol_A outputs and whose sample binding names pol_eps
 * (null: none) with the stride pol_seps --; the batch's arrays; the range, the epoch; grid > 0: that many workgroups in the place of the
 * launcher's */
struct emu_draw_args {
    int A, nenv; long long perm_n; unsigned long long seed; unsigned env_base, epoch;
    float *dst; long long sdst; int *perm_dst;
    int pol_A, pad; float *pol_eps; long long pol_seps;
    unsigned *counts; int *perm;
    int env0, n, grid, pad2;
};

static const char *g_draw_why = nullptr;
extern "C" const char *emu_draw_last_refusal(void) { return g_draw_why; }

/* {DRAW_MAXA, DRAW_MAXPERM, DRAW_GRID, DRAW_PERM_GRID, DRAW_ROUNDS, sizeof(emu_draw_args)}, for the binding's own checks */
extern "C" void emu_draw_constants(long long *out) {
    const long long a[6] = {ck::DRAW_MAXA, ck::DRAW_MAXPERM, ck::DRAW_GRID, ck::DRAW_PERM_GRID, ck::DRAW_ROUNDS, (long long)sizeof(emu_draw_args)};
    memcpy(out, a, sizeof a);
}

static ck::DrawCfg g_cfg;
static ck::PolicyCfg g_pol;

/* what the launcher does between configure and a launch */
static const char *draw_setup(const emu_draw_args &a) {
    if (const char *why = ck::draw_configure(a.A, a.perm_n, a.seed, a.env_base, g_cfg)) return why;
    ck::DrawCfg &c = g_cfg;
    if (!c.on) return ck::DRAW_NOT_CONFIGURED;
    if (a.dst) {
        if (const char *why = ck::check_draw_bind(c, a.dst, a.sdst)) return why;
        c.dst = a.dst; c.sdst = a.sdst;
    }
    if (a.perm_dst) {
        if (const char *why = ck::check_draw_bind_perm(c, a.perm_dst)) return why;
        c.perm_dst = a.perm_dst;
    }
    c.counts = a.counts; c.perm = a.perm;
    g_pol = {};
    if (a.pol_A > 0) {
        g_pol.nnets = 1; g_pol.net[0].nlayers = 1; g_pol.net[0].layer[0].out = a.pol_A;
        g_pol.eps = a.pol_eps; g_pol.seps = a.pol_seps;
    }
    return nullptr;
}

/* whether phys_batch_draw_configure accepts the numbers: 0, or -1 with the message */
extern "C" int emu_draw_configure(const emu_draw_args *a) {
    ck::DrawCfg c;
    g_draw_why = ck::draw_configure(a->A, a->perm_n, a->seed, a->env_base, c);
    if (!g_draw_why && !c.on) g_draw_why = ck::DRAW_NOT_CONFIGURED;
    return g_draw_why ? -1 : 0;
}

static ck::DrawIO g_io;
static ck::DrawPermIO g_pio;
static void body_draw() { ck::cassie_draw_kernel(g_io); }
static void body_perm() { ck::cassie_draw_perm_kernel(g_pio); }

/* phys_batch_draw on the emulator.  -1 where the launcher would refuse (emu_draw_last_refusal has the message); out: {the lanes of an
 * env, the envs of a wave, whether a lane may store 16 bytes, the launcher's grid} */
extern "C" int emu_draw(const emu_draw_args *a, long long *out) {
    ck::DrawDst D;
    g_draw_why = draw_setup(*a);
    if (!g_draw_why) g_draw_why = ck::check_draw(g_cfg, g_pol, a->nenv, a->env0, a->n, D);
    if (g_draw_why) return -1;
    g_io = ck::make_draw_io(g_cfg, D, a->env0, a->n);
    const long long r[4] = {g_io.lanes, g_io.per_wave, g_io.vec, ck::draw_grid(g_io)};
    if (out) memcpy(out, r, sizeof r);
    if (a->n == 0) return 0;
    emu::run_grid(body_draw, a->grid > 0 ? a->grid : ck::draw_grid(g_io));
    return 0;
}

/* phys_batch_draw_perm on the emulator; out: {the bits of a half, walk_max, the launcher's grid} */
extern "C" int emu_draw_perm(const emu_draw_args *a, long long *out) {
    g_draw_why = draw_setup(*a);
    if (!g_draw_why) g_draw_why = ck::check_draw_perm(g_cfg);
    if (g_draw_why) return -1;
    g_pio = ck::make_draw_perm_io(g_cfg, a->epoch);
    const long long r[3] = {g_pio.h, g_pio.walk_max, ck::draw_perm_grid(g_pio)};
    if (out) memcpy(out, r, sizeof r);
    emu::run_grid(body_perm, a->grid > 0 ? a->grid : ck::draw_perm_grid(g_pio));
    return 0;
}

/* ck::logn and the Box-Muller pair of two words on the host, for the tests of the definition */
extern "C" void emu_draw_logn(const double *x, double *y, long long n) {
    for (long long i = 0; i < n; ++i) y[i] = ck::logn(x[i]);
}
extern "C" void emu_draw_pair(const unsigned *a, const unsigned *b, double *zc, double *zs, long long n) {
    for (long long i = 0; i < n; ++i) ck::draw_pair(a[i], b[i], zc[i], zs[i]);
}
extern "C" void emu_draw_philox(const unsigned *ctr, const unsigned *key, unsigned *out) {
    ck::philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out);
}
