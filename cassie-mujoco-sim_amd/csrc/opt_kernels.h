/*
 * opt_kernels.h -- optimiser rows: the global gradient norm with its clip coefficient, an Adam step on every weight, every bias and
 * log_std, and each new float32 parameter written to the caller's master tensor, to the policy's packed weights and to the gradient
 * rows' transposed packing (phys_batch_opt_step, include/cassie_phys.h: the definition is there, OPTIMISER ROWS).  Three launches on one
 * stream, which orders them: no kernel waits for another workgroup, nothing is summed by an atomic -- the order of the norm's sum is part
 * of the definition.  Written with the wv:: primitives only: phys_batch.hip launches it, the wave emulator (tests/emu/emu_opt.cpp) runs
 * the same text.  The launch record, the checks, the grids and the offsets are small_launch.h's (no field of OptIO is assigned anywhere
 * else).
 *
 * The launches:
 *   1 squares   cassie_opt_sq_kernel: a wave per segment of OPT_SEG = 256 consecutive parameters of the flat order (the slots in the
 *               gradient rows' order, r = u (in + 1) + k within a slot with the bias at k = in -- cassie_grad_reduce_kernel's walk --,
 *               log_std behind the last slot); lane l chains g g over the parameters 256 s + 64 i + l, i = 0 .. 3, the product of a
 *               float32 with itself being exact in a double; wave_sum gives the segment's partial.
 *   2 scalars   cassie_opt_scalars_kernel: one wave; the rollout's reduce over the partials, the norm, the clip coefficient, the
 *               verdict (a norm that is not finite SKIPS the call), the running products of the betas, and the eight statistics.
 *   3 step      cassie_opt_step_kernel: a job is a tile of 16 units by 16 k of a slot, one wave, lane l on (u = 4 i + (l >> 4),
 *               k = l & 15) for i = 0 .. 3: g, w, m, v come as four 64-byte row segments a wave instruction (as
 *               cassie_grad_partial_kernel loads its operands), the transposed packing's store is one coalesced 256-byte store, the
 *               packed weights' a 1 KB block.  The bias is the column k = in of the same tiles (its lane stores to the bias tensor and to
 *               the packed biases); log_std takes a lane per element in the jobs behind the last tile.  A skipped call leaves by a
 *               wave-uniform early exit on the verdict, before any load.
 * The packings' zero padding is never written: a lane past `out` or past the bias column stores nothing.  Vector loads and stores only.
 * No stepping kernel is handed any of this.
 */
#ifndef CASSIE_OPT_KERNELS_H
#define CASSIE_OPT_KERNELS_H

#include "grad_kernels.h"

namespace ck {

/* OPT_SEG: the parameters of a segment of the NORM -- part of the definition.  OPT_SQ_GRID, OPT_STEP_GRID: the waves that walk the
 * segments and the step's jobs.  First choices (tools/opt_rate.py measures the call) */
constexpr int OPT_SEG = 256, OPT_SQ_GRID = 4096, OPT_STEP_GRID = 4096, OPT_NSTATS = 8;
/* what phys_batch_opt_download / _upload name (PHYS_OPT_* of cassie_phys.h) */
enum { OPT_M_W = 0, OPT_M_B = 1, OPT_V_W = 2, OPT_V_B = 3, OPT_M_LS = 4, OPT_V_LS = 5, OPT_SCALARS = 6, OPT_PARTIALS = 7 };
/* the batch's doubles: the eight statistics (norm, scale, this call's skip, t, skipped, lr, p1, p2), what launch 3 reads beside them,
 * and the state (t, p1, p2, skipped) */
enum { OPT_SC_NORM = 0, OPT_SC_SCALE = 1, OPT_SC_SKIP = 2, OPT_SC_STEP = 8, OPT_SC_SBC2 = 9, OPT_SC_T = 10, OPT_SC_P1 = 11, OPT_SC_P2 = 12,
       OPT_SC_SKIPPED = 13, OPT_SC_COUNT = 16 };

/* a slot (network, layer): its gradients (dW rows sgw elements apart, db), the master tensors (W rows sw apart, b), where its packed
 * weights, packed biases and transposed packing begin, its first parameter in the flat order and its first job of launch 3 */
struct OptSlot {
    const float *gw, *gb;
    float *w, *b, *pw, *pb, *pt;
    long long sgw, sw, par0, job0;
    int in, out, k4, u4;
};

struct OptIO {
    int nslots, A, nseg, pad;
    long long Q, tiles, njobs;                /* Q: the parameters; launch 3's tiles, and its jobs with log_std's behind the tiles */
    OptSlot s[GRAD_MAXSLOTS];
    const float *gls; float *ls;              /* log_std's gradient and the bound log_std [A] */
    float *m, *v;                             /* the moments [Q] each, in the flat order */
    double *part, *sc;                        /* the segments' partials [nseg]; the doubles [OPT_SC_COUNT] */
    double beta1, beta2, omb1, omb2, eps, max_norm, lr;   /* omb = 1 - beta, rounded once on the host */
};

/* the gradient of parameter q of the flat order, q in [0, Q) */
WV_DEVICE float opt_grad_at(const OptIO &io, long long q) {
    if (q >= io.Q - io.A) return io.gls[q - (io.Q - io.A)];
    int s = 0;
    for (int k = 1; k < io.nslots; ++k) if (q >= io.s[k].par0) s = k;       /* (the slots' first parameters ascend) */
    const OptSlot &S = io.s[s];
    const long long r = q - S.par0;
    const int u = (int)(r / (S.in + 1)), k = (int)(r - (long long)u * (S.in + 1));
    return k < S.in ? S.gw[(size_t)u * (size_t)S.sgw + (size_t)k] : S.gb[u];
}

/* SQUARES: a wave per segment -- lane l chains g g over 256 s + 64 i + l, i ascending, from +0.0 (the product is exact, so the rounded
 * add is the fma's one rounding); the partial is wave_sum's */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_opt_sq_kernel(OptIO io) {
    using namespace wv;
    const int l = lane();
    for (int seg = env_id(); seg < io.nseg; seg += grid_size()) {           /* (wave-uniform: all 64 lanes meet in wave_sum) */
        double acc = 0.0;
        for (int i = 0; i < OPT_SEG / WV_WAVE; ++i) {
            const long long q = (long long)seg * OPT_SEG + (long long)i * WV_WAVE + l;
            const double g = (double)opt_grad_at(io, q < io.Q ? q : io.Q - 1);
            acc = add_rn(acc, q < io.Q ? mul_rn(g, g) : 0.0);
        }
        const double sum = wave_sum(acc);
        if (l == 0) io.part[seg] = sum;
    }
}

/* SCALARS: one wave -- reduce, the norm, the coefficient, the verdict, the products, the statistics */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_opt_scalars_kernel(OptIO io) {
    using namespace wv;
    const int l = lane();
    const double S = grad_reduce(io.part, io.nseg, l);
    if (l != 0 || env_id() != 0) return;
    double *sc = io.sc;
    const double norm = sqrt_rn(S);
    const bool finite = norm < (double)INFINITY;                            /* (false for a NaN) */
    const double raw = div_rn(io.max_norm, add_rn(norm, 1e-6)), scale = raw < 1.0 ? raw : 1.0;
    double t = sc[OPT_SC_T], p1 = sc[OPT_SC_P1], p2 = sc[OPT_SC_P2], skipped = sc[OPT_SC_SKIPPED];
    if (finite) {
        t = add_rn(t, 1.0); p1 = mul_rn(p1, io.beta1); p2 = mul_rn(p2, io.beta2);
        sc[OPT_SC_STEP] = div_rn(io.lr, sub_rn(1.0, p1));
        sc[OPT_SC_SBC2] = sqrt_rn(sub_rn(1.0, p2));
        sc[OPT_SC_T] = t; sc[OPT_SC_P1] = p1; sc[OPT_SC_P2] = p2;
    } else {
        skipped = add_rn(skipped, 1.0);
        sc[OPT_SC_SKIPPED] = skipped;
    }
    sc[OPT_SC_NORM] = norm; sc[OPT_SC_SCALE] = scale; sc[OPT_SC_SKIP] = finite ? 0.0 : 1.0;
    sc[3] = t; sc[4] = skipped; sc[5] = io.lr; sc[6] = p1; sc[7] = p2;
}

/* STEP of one parameter: its gradient, master value and moments -> the new moments (stored) and the new value (returned) */
WV_DEVICE float opt_adam(const OptIO &io, double scale, double step, double sbc2, float g, float w, float *m, float *v) {
    using namespace wv;
    const double gs = mul_rn((double)g, scale);
    const float m1 = (float)add_rn(mul_rn(io.beta1, (double)*m), mul_rn(io.omb1, gs));
    const float v1 = (float)add_rn(mul_rn(io.beta2, (double)*v), mul_rn(io.omb2, mul_rn(gs, gs)));
    const double den = add_rn(div_rn(sqrt_rn((double)v1), sbc2), io.eps);
    *m = m1; *v = v1;
    return (float)sub_rn((double)w, div_rn(mul_rn(step, (double)m1), den));
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_opt_step_kernel(OptIO io) {
    const int l = wv::lane();
    if (io.sc[OPT_SC_SKIP] != 0.0) return;                                  /* SKIPPED (wave-uniform): every word stays as it is */
    const double scale = io.sc[OPT_SC_SCALE], step = io.sc[OPT_SC_STEP], sbc2 = io.sc[OPT_SC_SBC2];
    for (long long job = wv::env_id(); job < io.njobs; job += wv::grid_size()) {
        if (job >= io.tiles) {                                                 /* log_std: a lane per element */
            const long long j = (job - io.tiles) * WV_WAVE + l;
            if (j < io.A) {
                const long long q = io.Q - io.A + j;
                io.ls[j] = opt_adam(io, scale, step, sbc2, io.gls[j], io.ls[j], io.m + q, io.v + q);
            }
            continue;
        }
        int s = 0;
        for (int k = 1; k < io.nslots; ++k) if (job >= io.s[k].job0) s = k; /* (the slots' first jobs ascend) */
        const OptSlot &S = io.s[s];
        const int nkb = (S.in + 16) >> 4, r = (int)(job - S.job0), ub = r / nkb, kb = r - ub * nkb;
        const int k = kb * 16 + (l & 15);
        for (int i = 0; i < 4; ++i) {
            const int u = ub * 16 + 4 * i + (l >> 4);
            if (u >= S.out || k > S.in) continue;                           /* (the padding: nothing loaded, nothing stored) */
            const long long q = S.par0 + (long long)u * (S.in + 1) + k;
            if (k == S.in) {                                                /* the bias column */
                const float b1 = opt_adam(io, scale, step, sbc2, S.gb[u], S.b[u], io.m + q, io.v + q);
                S.b[u] = b1; S.pb[u] = b1;
            } else {
                float *wp = S.w + (size_t)u * (size_t)S.sw + (size_t)k;
                const float w1 = opt_adam(io, scale, step, sbc2, S.gw[(size_t)u * (size_t)S.sgw + (size_t)k], *wp, io.m + q, io.v + q);
                *wp = w1;
                S.pw[(size_t)(u >> 4) * 16 * (size_t)S.k4 + (size_t)(k >> 2) * 64 + (size_t)(k & 3) * 16 + (size_t)(u & 15)] = w1;
                S.pt[(size_t)(k >> 4) * 16 * (size_t)S.u4 + (size_t)(u >> 2) * 64 + (size_t)(u & 3) * 16 + (size_t)(k & 15)] = w1;
            }
        }
    }
}

}  // namespace ck
#endif
