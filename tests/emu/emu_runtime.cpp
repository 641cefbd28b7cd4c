/*
 * emu_runtime.cpp -- TEST-ONLY wavefront emulator (see tests/emu/wave.h).
 * Runs physics_kernel.h on the CPU: one coroutine per lane, round-robin
 * scheduling with a rendezvous at every cross-lane primitive.  Because the
 * kernel keeps all collectives in wave-uniform control flow, "resume every lane
 * until its next rendezvous" reproduces the SIMT semantics exactly.
 *
 * Workgroups of two waves (the step kernel's NW = 2 form): 128 coroutines; the
 * cross-lane primitives are rendezvous of ONE wave's 64 lanes, wv::block_barrier
 * is a rendezvous of the workgroup.  A wave that has ended does not take part in
 * later barriers (as on the hardware).  How the two waves interleave between
 * barriers is a test parameter (emu_settings::wave_schedule): a program free of
 * LDS races gives the same bits under every schedule.
 *
 * This unit is the scheduler and the wv:: primitives; the kernels' entry points
 * are emu_step.cpp (the step kernel) and emu_kernels.cpp (the small ones).
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <wave.h>

#include "emu_runtime.h"

namespace {
constexpr int NL = 64, NWMAX = 2, NLMAX = NL * NWMAX;
constexpr size_t STACK_BYTES = 1 << 20;

struct LaneCtx { void *sp; char *stack; bool done; };
LaneCtx g_lane[NLMAX];
void *g_sched_sp;
int g_cur = 0, g_env = 0, g_grid = 1;
double g_xd[NLMAX];
int g_xi[NLMAX];
int g_kind[NLMAX];      /* what the lane yielded at: 0 = a rendezvous of its wave, 1 = the workgroup barrier */
int g_wave_schedule = 0; /* 0: the waves take turns, one rendezvous each; 1: wave 0 runs whenever it can; 2: wave 1 does */
void (*g_body)() = nullptr;
bool g_mismatch = false;
inline int wave_base() { return g_cur & ~(NL - 1); }

extern "C" void emu_switch(void **save_sp, void *load_sp);
asm(R"(
.text
.globl emu_switch
.type emu_switch,@function
emu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
)");

void rendezvous() { g_kind[g_cur] = 0; emu_switch(&g_lane[g_cur].sp, g_sched_sp); }
void barrier_rendezvous() { g_kind[g_cur] = 1; emu_switch(&g_lane[g_cur].sp, g_sched_sp); }
void spin_rendezvous() { g_kind[g_cur] = 2; emu_switch(&g_lane[g_cur].sp, g_sched_sp); }

void lane_entry() {
    g_body();
    g_lane[g_cur].done = true;
    emu_switch(&g_lane[g_cur].sp, g_sched_sp);
    abort(); /* a finished lane is never resumed */
}

void run_block(void (*body)(), int nwaves = 1) {
    g_body = body;
    const int nl = NL * nwaves;
    for (int l = 0; l < nl; ++l) {
        if (!g_lane[l].stack) g_lane[l].stack = (char *)aligned_alloc(64, STACK_BYTES);
        uintptr_t top = ((uintptr_t)g_lane[l].stack + STACK_BYTES) & ~(uintptr_t)15;
        void **slot = (void **)(top - 16); /* 16-byte aligned return-address slot */
        *slot = (void *)&lane_entry;
        void **sp = slot - 6;
        for (int i = 0; i < 6; ++i) sp[i] = nullptr;
        g_lane[l].sp = sp;
        g_lane[l].done = false;
    }
    bool wave_done[NWMAX] = {false, false}, at_barrier[NWMAX] = {false, false};
    for (;;) {
        /* one turn: every wave that can run resumes its 64 lanes once, i.e. up to its next rendezvous */
        for (int t = 0; t < nwaves; ++t) {
            const int w = g_wave_schedule == 2 ? nwaves - 1 - t : t;
            if (wave_done[w] || at_barrier[w]) continue;
            int ndone = 0, nbar = 0, nspin = 0;
            for (int l = w * NL; l < (w + 1) * NL; ++l) {
                if (g_lane[l].done) { ++ndone; continue; }
                g_cur = l;
                emu_switch(&g_sched_sp, g_lane[l].sp);
                if (g_lane[l].done) ++ndone;
                else if (g_kind[l] == 1) ++nbar;
                else if (g_kind[l] == 2) ++nspin;
            }
            if (ndone == NL) wave_done[w] = true;
            else if (ndone != 0) { g_mismatch = true; fprintf(stderr, "emu: lanes of wave %d left the kernel at different rendezvous counts (%d done)\n", w, ndone); abort(); }
            else if (nbar == NL) at_barrier[w] = true;
            else if (nbar != 0) { g_mismatch = true; fprintf(stderr, "emu: %d lanes of wave %d are at the workgroup barrier, the others at a wave rendezvous\n", nbar, w); abort(); }
            if (nspin != 0 && nspin != NL) { g_mismatch = true; fprintf(stderr, "emu: %d lanes of wave %d poll a flag, the others do not\n", nspin, w); abort(); }
            if (g_wave_schedule != 0 && nspin == 0) break; /* the preferred wave runs on until it is blocked, polling or done */
        }
        bool all_done = true, all_blocked = true;
        for (int w = 0; w < nwaves; ++w) { all_done = all_done && wave_done[w]; all_blocked = all_blocked && (wave_done[w] || at_barrier[w]); }
        if (all_done) break;
        if (all_blocked) for (int w = 0; w < nwaves; ++w) at_barrier[w] = false; /* the barrier opens: every wave still alive has arrived */
    }
}
}  // namespace

namespace wv {
int lane() { return g_cur & (NL - 1); }
int wave_id() { return g_cur / NL; }
int env_id() { return g_env; }
int grid_size() { return g_grid; }
void sync() { rendezvous(); }
void block_barrier() { barrier_rendezvous(); }
void spin_yield() { spin_rendezvous(); }
double shfl(double v, int src) {
    g_xd[g_cur] = v;
    rendezvous();
    double r = g_xd[wave_base() + (src & 63)];
    rendezvous();
    return r;
}
double shfl_xor(double v, int mask) { return shfl(v, g_cur ^ mask); }
int shfl_i(int v, int src) {
    g_xi[g_cur] = v;
    rendezvous();
    int r = g_xi[wave_base() + (src & 63)];
    rendezvous();
    return r;
}
double readlane(double v, int src) { return shfl(v, src); }
/* the matrix-core instruction as the device performs it: per element the FMA chain over k = 0 .. 3 on top of C */
static double g_xa[NLMAX], g_xb[NLMAX];
void mfma_f64_16x16x4(double a, double b, double (&c)[4]) {
    g_xa[g_cur] = a; g_xb[g_cur] = b;
    rendezvous();
    const int l = g_cur & 63, j = l & 15, wb = wave_base();
    for (int v = 0; v < 4; ++v) {
        const int i = (l >> 4) + 4 * v;
        double acc = c[v];
        for (int k = 0; k < 4; ++k) acc = std::fma(g_xa[wb + i + 16 * k], g_xb[wb + j + 16 * k], acc);
        c[v] = acc;
    }
    rendezvous();
}
unsigned long long ballot(bool p) {
    g_xi[g_cur] = p ? 1 : 0;
    rendezvous();
    unsigned long long m = 0;
    for (int l = 0; l < NL; ++l) if (g_xi[wave_base() + l]) m |= 1ull << l;
    rendezvous();
    return m;
}
int g_force_guarded = 0;
int g_poison_lds = 0;
int g_skip_com_init = 0;
unsigned long g_poison_lo = 0, g_poison_hi = ~0ul;
static int g_producer_xcc = 0;
int emu_xcc() { return g_producer_xcc; }
void emu_fail(const char *what) { fprintf(stderr, "emu: %s\n", what); abort(); }
}  // namespace wv

namespace emu {
void run_grid(void (*body)(), int grid, int nwaves) {
    g_grid = grid;
    for (int wg = 0; wg < grid; ++wg) { g_env = wg; run_block(body, nwaves); }
    g_env = 0; g_grid = 1;
}
static void set_hooks(const emu_settings &s) {
    g_wave_schedule = s.wave_schedule;
    wv::g_force_guarded = s.force_guarded_pgs; wv::g_poison_lds = s.poison_lds; wv::g_skip_com_init = s.skip_com_init;
    wv::g_poison_lo = s.poison_lo; wv::g_poison_hi = s.poison_hi ? s.poison_hi : ~0ul;
    wv::g_producer_xcc = s.producer_xcc & 7;
}
with_settings::with_settings(const emu_settings &s) { set_hooks(s); }
with_settings::~with_settings() { set_hooks(emu_settings{}); }
}  // namespace emu

