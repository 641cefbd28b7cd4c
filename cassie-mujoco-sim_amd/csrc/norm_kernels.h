/*
 * norm_kernels.h -- normaliser rows: the running per-column mean and variance of float32 rows, and the two float32 vectors the policy's
 * INPUT reads (phys_batch_norm_update, _write, include/cassie_phys.h: the definition is there, NORMALISER ROWS).  An update is four
 * launches on one stream, which orders them: no kernel waits for another workgroup, nothing is summed by an atomic -- the order of every
 * sum is part of the definition.  Written with the wv:: primitives only, workgroups of one wave: phys_batch.hip launches them, the wave
 * emulator (tests/emu/emu_norm.cpp) runs the same text.  The launch record, the checks, the grids and the regions are small_launch.h's
 * (no field of NormIO is assigned anywhere else).
 *
 * The launches:
 *   1 sum     cassie_norm_sum_kernel: lane = column.  A job is one block of the samples by one group of 64 lanes' columns; a lane takes
 *             16 bytes (four columns) of a row where the host found pointer, D and both strides multiples of 4 words, a word otherwise,
 *             so consecutive lanes load consecutive words of a row.  The chain over a block's rows is one dependent fp64 add a row and
 *             column; the loads do not depend on it: the next NORM_AHEAD rows are requested while the chain works through the NORM_AHEAD
 *             before them (rollout_kernels.h's finish).  A row past the block's end is never requested: the walk stays on the block's
 *             last row, whose words are loaded again and left out by the select that leaves a value that is not finite out.
 *   2 mean    cassie_norm_mean_kernel: lane = column; the blocks' a1 in block order, the counts as integers.
 *   3 sq      cassie_norm_sq_kernel: launch 1's walk with d = x - mb and d d in the place of x.
 *   4 merge   cassie_norm_merge_kernel: lane = column; the blocks' a2 in block order, the Chan merge into the state, the two words.
 *   write     cassie_norm_write_kernel: lane = column; the two words of every column with n > 0 from the state.
 * Nothing crosses a lane: a column's words depend on its own values alone.  Vector loads and stores only; nothing is indexed by a value.
 * No stepping kernel is handed any of this.
 */
#ifndef CASSIE_NORM_KERNELS_H
#define CASSIE_NORM_KERNELS_H

#include "wave.h"

namespace ck {

/* the limits of a configuration (PHYS_NORM_*); NORM_GRID: the most workgroups of launches 1 and 3, which then walk the jobs; NORM_AHEAD:
 * the rows a wave requests ahead of its chain (8 rows of 1 KiB a wave on the 16-byte path: DESIGN 4.3); NORM_CHAIN_AHEAD: the blocks whose
 * partials launches 2 and 4 request ahead of theirs */
constexpr int NORM_MAXDIM = 512, NORM_MINBLOCK = 16, NORM_MAXBLOCK = 4096, NORM_GRID = 8192, NORM_AHEAD = 8, NORM_CHAIN_AHEAD = 32, NORM_NSTATS = 8;
constexpr long long NORM_MAXROWS = 1ll << 30;
/* what phys_batch_norm_download / _upload name (PHYS_NORM_* of cassie_phys.h): the first seven are rows of D doubles of the state buffer,
 * in this order */
enum { NORM_N = 0, NORM_MEAN = 1, NORM_M2 = 2, NORM_SKIPPED = 3, NORM_EXCLUDED = 4, NORM_MB = 5, NORM_COUNTS = 6, NORM_PARTIALS = 7,
       NORM_STATE_ROWS = 7 };

/* 16 bytes of a row (a vector type, which lives in registers) */
typedef float NormVec __attribute__((vector_size(16)));

/* an update or a write: the source (sample s = step * rows + row at src + step * step_stride + row * row_stride, R samples in blocks of
 * `block`), whether a lane takes 16 bytes, the groups of 64 lanes a row is cut into and the jobs of launches 1 and 3; the state
 * [NORM_STATE_ROWS][D], the partials a1 and a2 [blocks][D] each, the blocks' counts [blocks][D]; the two outputs */
struct NormIO {
    int D, block, rows, vec, groups, pad;
    long long R, blocks, njobs, step_stride, row_stride, wrap;   /* wrap: from a step's last row to the next step's first */
    const float *src;
    double *state, *a1, *a2; int *cnt;
    float *mean, *inv;
    double eps, Rd;
};

WV_DEVICE float norm_elem(float v, int) { return v; }
WV_DEVICE float norm_elem(const NormVec &v, int i) { return v[i]; }

/* PASS 1 (SQ false) or PASS 2 (SQ true) of one job: block c, the lane's W columns from j0.  The way from a sample to the next is a select
 * between the row stride and `wrap`, what leads from a step's last row to the next step's first; both are held PER LANE (a zero the
 * compiler cannot see through is added to them), as rollout_kernels.h's finish holds its steps and for its reason */
template <class V, int W, bool SQ> WV_DEVICE void norm_pass_job(const NormIO &io, long long c, int j0, bool active) {
    using namespace wv;
    const long long s0 = c * io.block;
    const int nb = (int)(io.R - s0 < io.block ? io.R - s0 : io.block);       /* (the last block may be short) */
    const size_t jj = active ? (size_t)j0 : 0;                               /* (a lane past D loads the first columns again) */
    const long long step0 = s0 / io.rows;
    int zero = 0;
    keep(zero);
    const long long rs = io.row_stride + zero, ws = io.wrap + zero;
    int row = (int)(s0 - step0 * io.rows), left = nb - 1;                    /* left: the moves that stay inside the block */
    const float *p = io.src + (size_t)step0 * (size_t)io.step_stride + (size_t)row * (size_t)io.row_stride + jj;
#define NORM_NEXT(dst) do { \
        dst = *(const V *)p; \
        const bool move = left > 0, wrapped = row + 1 == io.rows; \
        p += move ? (wrapped ? ws : rs) : 0ll; \
        row = move ? (wrapped ? 0 : row + 1) : row; \
        left -= move ? 1 : 0; \
    } while (0)
    double mb[W], acc[W];
    int n[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { mb[i] = SQ ? io.state[(size_t)NORM_MB * (size_t)io.D + jj + i] : 0.0; acc[i] = 0.0; n[i] = 0; }
    V cur[NORM_AHEAD], nxt[NORM_AHEAD];
#pragma unroll
    for (int k = 0; k < NORM_AHEAD; ++k) NORM_NEXT(cur[k]);
    for (int r0 = 0; r0 < nb; r0 += NORM_AHEAD) {
#pragma unroll
        for (int k = 0; k < NORM_AHEAD; ++k) NORM_NEXT(nxt[k]);
#pragma unroll
        for (int k = 0; k < NORM_AHEAD; ++k) {
            const bool in = r0 + k < nb;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const double x = (double)norm_elem(cur[k], i);
                const bool fin = in && __builtin_fabs(x) < __builtin_inf();    /* (false for a NaN) */
                double t = x;
                if (SQ) { const double d = sub_rn(x, mb[i]); t = mul_rn(d, d); }
                const double sum = add_rn(acc[i], t);
                acc[i] = fin ? sum : acc[i];
                n[i] += fin ? 1 : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < NORM_AHEAD; ++k) cur[k] = nxt[k];
    }
#undef NORM_NEXT
    if (!active) return;
    const size_t at = (size_t)c * (size_t)io.D + jj;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        if (SQ) io.a2[at + i] = acc[i];
        else { io.a1[at + i] = acc[i]; io.cnt[at + i] = n[i]; }
    }
}

template <bool SQ> WV_DEVICE void norm_pass(const NormIO &io) {
    const int l = wv::lane();
    for (long long job = wv::env_id(); job < io.njobs; job += wv::grid_size()) {
        const long long c = job / io.groups;
        const int g = (int)(job - c * io.groups);
        if (io.vec) { const int j0 = (g * WV_WAVE + l) * 4; norm_pass_job<NormVec, 4, SQ>(io, c, j0, j0 < io.D); }
        else { const int j0 = g * WV_WAVE + l; norm_pass_job<float, 1, SQ>(io, c, j0, j0 < io.D); }
    }
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_norm_sum_kernel(NormIO io) { norm_pass<false>(io); }
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_norm_sq_kernel(NormIO io) { norm_pass<true>(io); }

/* the blocks' partials of column j in block order from +0.0, and the integer sum of their counts where cnt is given.  A lane's chain is
 * one dependent add a block and the loads do not depend on it: the next NORM_CHAIN_AHEAD blocks' words are all requested before the chain
 * takes the first of them (a wave a 64 columns: nothing else hides the latency) */
template <bool COUNT> WV_DEVICE double norm_chain(const double *a, const int *cnt, long long blocks, int D, int j, long long &M) {
    double S = 0.0;
    M = 0;
    int zero = 0;
    wv::keep(zero);
    const long long stride = D + zero;                                       /* (per lane, as the passes hold theirs) */
    const double *p = a + j;
    const int *q = cnt + j;
    long long left = blocks - 1;                                             /* the moves that stay inside the partials */
    for (long long c0 = 0; c0 < blocks; c0 += NORM_CHAIN_AHEAD) {
        double x[NORM_CHAIN_AHEAD];
        int n[NORM_CHAIN_AHEAD];
#pragma unroll
        for (int k = 0; k < NORM_CHAIN_AHEAD; ++k) {
            x[k] = *p;
            n[k] = COUNT ? *q : 0;
            const long long move = left > 0 ? stride : 0ll;                  /* (past the end: the last block's words again, not added) */
            p += move;
            if (COUNT) q += move;
            left -= left > 0 ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < NORM_CHAIN_AHEAD; ++k)
            if (c0 + k < blocks) { S = wv::add_rn(S, x[k]); M += n[k]; }
    }
    return S;
}

/* MEAN: S1, Mj, mb */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_norm_mean_kernel(NormIO io) {
    using namespace wv;
    for (int j = env_id() * WV_WAVE + lane(); j < io.D; j += grid_size() * WV_WAVE) {
        long long M;
        const double S1 = norm_chain<true>(io.a1, io.cnt, io.blocks, io.D, j, M);
        const double Md = (double)M;                                         /* (exact: at most 2^30) */
        io.state[(size_t)NORM_MB * (size_t)io.D + (size_t)j] = M > 0 ? div_rn(S1, Md) : 0.0;
        io.state[(size_t)NORM_COUNTS * (size_t)io.D + (size_t)j] = Md;
    }
}

/* the two words of a column from n and m2 */
WV_DEVICE float norm_inv(const NormIO &io, double m2, double n) {
    using namespace wv;
    return (float)div_rn(1.0, sqrt_rn(add_rn(div_rn(m2, n), io.eps)));
}

/* MERGE: S2, the state, the two words; a column with no finite value is SKIPPED */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_norm_merge_kernel(NormIO io) {
    using namespace wv;
    const size_t D = (size_t)io.D;
    for (int j = env_id() * WV_WAVE + lane(); j < io.D; j += grid_size() * WV_WAVE) {
        double *st = io.state + j;
        long long unused;
        const double S2 = norm_chain<false>(io.a2, nullptr, io.blocks, io.D, j, unused);
        const double Mj = st[NORM_COUNTS * D], mb = st[NORM_MB * D];
        if (!(Mj > 0.0)) { st[NORM_SKIPPED * D] = add_rn(st[NORM_SKIPPED * D], 1.0); continue; }
        const double n = st[NORM_N * D], mean = st[NORM_MEAN * D], m2 = st[NORM_M2 * D];
        const double nn = add_rn(n, Mj), delta = sub_rn(mb, mean), w = div_rn(Mj, nn);
        const double mean1 = add_rn(mean, mul_rn(delta, w));
        const double m21 = add_rn(add_rn(m2, S2), mul_rn(mul_rn(delta, delta), mul_rn(n, w)));
        st[NORM_N * D] = nn; st[NORM_MEAN * D] = mean1; st[NORM_M2 * D] = m21;
        st[NORM_EXCLUDED * D] = add_rn(st[NORM_EXCLUDED * D], sub_rn(io.Rd, Mj));
        io.mean[j] = (float)mean1; io.inv[j] = norm_inv(io, m21, nn);
    }
}

/* WRITE: the two words of every column with n > 0 from the state, no update */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_norm_write_kernel(NormIO io) {
    const size_t D = (size_t)io.D;
    for (int j = wv::env_id() * WV_WAVE + wv::lane(); j < io.D; j += wv::grid_size() * WV_WAVE) {
        const double *st = io.state + j;
        const double n = st[NORM_N * D];
        if (!(n > 0.0)) continue;
        io.mean[j] = (float)st[NORM_MEAN * D]; io.inv[j] = norm_inv(io, st[NORM_M2 * D], n);
    }
}

}  // namespace ck
#endif
