/*
 * grad_kernels.h -- gradient rows: the PPO clipped-surrogate loss, the value loss and the entropy term of a minibatch of the rollout's
 * samples, and their gradient with respect to every weight, every bias and log_std (phys_batch_grad, include/cassie_phys.h: the definition
 * is there, GRADIENT ROWS).  Five launches on one stream, which orders them: no kernel waits for another workgroup, nothing is summed by
 * an atomic -- the order of every sum is part of the definition.  Written with the wv:: primitives only: phys_batch.hip launches it, the
 * wave emulator (tests/emu/emu_grad.cpp) runs the same text.  The launch record, the checks, the grids and the offsets of the stores are
 * small_launch.h's (no field of GradIO or GradPackIO is assigned anywhere else).
 *
 * Why it is exact: as in policy_kernels.h, every chain multiplies two float32 values, so fma((double) a, (double) b, acc) is ONE rounding
 * of acc + a b, and wv::mfma_f64_16x16x4 is that chain over its four k on top of C.  A numpy restatement (tests/grad_check.py) writes
 * every chain as acc = acc + a * b on doubles.
 *
 * The launches:
 *   1 forward + head   cassie_grad_forward_kernel: a job is (tile of 16 positions, network), a workgroup of POLICY_WAVES waves, the LDS
 *                      [k][pos] and the layers of cassie_policy_kernel itself (policy_layer, called as it stands) on the rows gathered
 *                      through idx; every layer's h, and the normalised input, also goes to the activation store [pos][width16] -- the
 *                      layout launch 3 loads rows of.  The head takes a lane per position and leaves the top layer's delta, the log_std
 *                      terms and the per-position statistics.
 *   2 backward deltas  cassie_grad_backward_kernel: a job is (tile, network); from the top layer down, delta_l [u][pos] in LDS is the A
 *                      operand, the TRANSPOSED packing of W_l (cassie_grad_pack_kernel makes it from the policy's packed weights) the B
 *                      operand -- one coalesced 256-byte load a wave instruction --, and D(act, g, h) with the kept h of the layer below runs
 *                      on the accumulators: delta_{l-1} to the other LDS buffer and to the delta store.  The k loop is policy_layer's,
 *                      operands requested a chunk ahead.
 *   3 weight partials  cassie_grad_partial_kernel: a job is (network, layer, chunk, block of 16 units, group of four blocks of 16 k), one
 *                      wave; the reduction index is the position, A = delta[p0 + (l >> 4)][u0 + (l & 15)], B = h[p0 + (l >> 4)][k0 + (l & 15)]
 *                      straight from the two stores (four 64-byte segments a wave instruction); the bias is the column k = in, a select of
 *                      1.0 at the load.  C[u][k] goes to the fp64 partials [chunk][out][in + 1].
 *   4 reduce           cassie_grad_reduce_kernel: a lane per parameter adds the chunks in ascending order and writes float32 into the
 *                      gradient tensors (the caller's, or the batch's own).
 *   5 statistics       cassie_grad_stats_kernel: a wave per log_std element and per statistic, the rollout's reduce over the positions.
 * A void position (idx outside the rollout, or past m) loads +0.0 rows, and every word it leaves -- kept activations, deltas, head
 * values -- is +0.0 by a select at the store, never a product with zero: a weight of +inf makes a NaN of a void position's sums, and
 * that NaN goes nowhere.  Vector loads and stores only.  No stepping kernel is handed any of this.
 */
#ifndef CASSIE_GRAD_KERNELS_H
#define CASSIE_GRAD_KERNELS_H

#include "policy_kernels.h"

namespace ck {

/* GRAD_GRID: the workgroups that walk the (tile, network) jobs of launches 1 and 2; GRAD_PART_GRID: the waves that walk the jobs of
 * launch 3; GRAD_RED_GRID: the waves of launch 4; GRAD_PACK_GRID: of the transposed packing.  First choices (tools/grad_rate.py measures
 * the call) */
constexpr int GRAD_GRID = 1024, GRAD_PART_GRID = 8192, GRAD_RED_GRID = 1024, GRAD_PACK_GRID = 64;
constexpr int GRAD_MINCHUNK = 16, GRAD_MAXCHUNK = 4096, GRAD_NSTATS = 8, GRAD_MAXSLOTS = POLICY_MAXNETS * POLICY_MAXLAYERS;
/* what phys_batch_grad_download names (PHYS_GRAD_* of cassie_phys.h) */
enum { GRAD_DW = 0, GRAD_DB = 1, GRAD_DLS = 2, GRAD_ACT = 3, GRAD_DELTA = 4, GRAD_PARTIAL = 5, GRAD_PACKT = 6 };
/* the rows of the per-position doubles behind the A rows of log_std terms: policy loss, value loss, kl, clipped, void */
enum { GRAD_POS_PLOSS = 0, GRAD_POS_VLOSS = 1, GRAD_POS_KL = 2, GRAD_POS_CLIPPED = 3, GRAD_POS_VOID = 4, GRAD_POS_ROWS = 5 };

/* where a network's rows begin in the stores: h_off[a], a = 0 .. nlayers: the kept activations [mcap][hw[a]] (a = 0: the normalised input,
 * shared by the networks; a = l + 1: layer l's h), hw = the width rounded up to 16; per layer the deltas [mcap][out16], the fp64 partials
 * [chunks][out][in + 1], the transposed packing [out16 of the layer below / 16][u4 / 4][64] with u4 = out rounded up to 4 */
struct GradNet {
    long long h_off[POLICY_MAXLAYERS + 1]; int hw[POLICY_MAXLAYERS + 1], pad;
    long long d_off[POLICY_MAXLAYERS], p_off[POLICY_MAXLAYERS], t_off[POLICY_MAXLAYERS];
};
/* an array of the rollout a sample s = t nenv + env is gathered from: words between two steps and between two envs */
struct GradSrc { const float *ptr; long long step, row; };

struct GradIO {
    int m, mcap, chunk, nchunks, nnets, in_dim, rows0, rows1;   /* mcap: m rounded up to the chunk; nchunks = mcap / chunk */
    int nenv, total, A, nslots;                                 /* total = T nenv: idx lies in [0, total) or the position is void */
    PolicyNet net[POLICY_MAXNETS];
    GradNet g[POLICY_MAXNETS];
    const float *packed, *packt;
    const int *idx;
    GradSrc obs, action, logp, advn, ret;
    const float *mean, *inv; double clip;
    const float *log_std;
    float *act, *delta; double *part, *pos, *stats;             /* pos: [A + GRAD_POS_ROWS][mcap] */
    double lo, hi, eps, c_v, c_ent, inv_m;                      /* 1 - eps and 1 + eps, 1 / m: rounded once on the host */
    float *dw[GRAD_MAXSLOTS]; long long sdw[GRAD_MAXSLOTS]; float *db[GRAD_MAXSLOTS]; float *dls;
    long long job0[GRAD_MAXSLOTS + 1], par0[GRAD_MAXSLOTS + 1]; /* launch 3's first job and launch 4's first parameter of every slot, ascending */
    int slot_net[GRAD_MAXSLOTS], slot_layer[GRAD_MAXSLOTS];
};

/* the transposed packing of one layer from its packed weights: word p is W[u][k] of block p / (16 u4) of 16 k, u-step (p % (16 u4)) / 64,
 * lane p % 64: u = 4 u-step + (lane >> 4), k = 16 block + (lane & 15); +0.0 where u >= out or k >= in */
struct GradPackIO {
    const float *src; float *dst;     /* the layer's packed weights; its transposed packing */
    int in, out, k4, in16, u4, pad;
};

#ifdef CK_EMULATED
#define GRAD_LDS(name) WV_SHARED float name[2 * POLICY_MAXDIM * POLICY_TILE + POLICY_TILE]
#else
#define GRAD_LDS(name) extern __shared__ float name[]
#endif

/* D(act, g, h): the activation's derivative in terms of its OUTPUT h, times g; every step one rounded fp64 operation */
WV_DEVICE double grad_d(int act, double g, double h) {
    using namespace wv;
    if (act == POL_RELU) return h > 0.0 ? g : 0.0;
    if (act == POL_TANH) return mul_rn(g, sub_rn(1.0, mul_rn(h, h)));
    if (act == POL_ELU) return h > 0.0 ? g : mul_rn(g, add_rn(h, 1.0));
    return g;
}

/* the sample of position p (-1: void) */
WV_DEVICE int grad_sample(const GradIO &io, int p) {
    const int s = io.idx[p < io.m ? p : 0];
    return p < io.m && s >= 0 && s < io.total ? s : -1;
}
WV_DEVICE const float *grad_row(const GradSrc &S, int s, int nenv) {
    const int t = s / nenv, env = s - t * nenv;
    return S.ptr + (size_t)t * (size_t)S.step + (size_t)env * (size_t)S.row;
}

/* INPUT: the tile's gathered rows into X[k][pos], normalised where a normalisation is bound; +0.0 in the padding k and in void positions */
WV_DEVICE void grad_load_input(const GradIO &io, int p0, float (*X)[POLICY_TILE], int tid) {
    using namespace wv;
    const int k4 = io.net[0].layer[0].k4;
    for (int i = tid; i < POLICY_TILE * k4; i += WV_WAVE * POLICY_WAVES) {
        const int e = i / k4, k = i - e * k4;
        const int s = grad_sample(io, p0 + e);
        float v = 0.0f;
        if (s >= 0 && k < io.in_dim) {
            v = grad_row(io.obs, s, io.nenv)[k];
            if (io.mean) {
                const double y = mul_rn(sub_rn((double)v, (double)io.mean[k]), (double)io.inv[k]);
                const double lo = -io.clip, hi = io.clip;
                v = (float)(y < lo ? lo : (y > hi ? hi : y));              /* (a NaN passes) */
            }
        }
        X[k][e] = v;
    }
}

/* the tile's rows of a buffer [unit][pos] into a store [pos][w16]; rows: the units the buffer holds (+0.0 beyond); void positions +0.0 */
WV_DEVICE void grad_store_rows(float *dst, int w16, int rows, const float (*Y)[POLICY_TILE], const int *live, int p0, int tid) {
    for (int i = tid; i < POLICY_TILE * w16; i += WV_WAVE * POLICY_WAVES) {
        const int e = i / w16, u = i - e * w16;
        const float v = Y[u < rows ? u : 0][e];
        dst[(size_t)(p0 + e) * (size_t)w16 + (size_t)u] = live[e] && u < rows ? v : 0.0f;
    }
}

/* HEAD, actor: position p0 + e; MU: the actor's last h */
WV_DEVICE void grad_head_actor(const GradIO &io, int p0, int e, const float (*MU)[POLICY_TILE]) {
    using namespace wv;
    const PolicyNet &N = io.net[0];
    const PolicyLayer &L = N.layer[N.nlayers - 1];
    const int p = p0 + e, s = grad_sample(io, p), A = L.out;
    const bool live = s >= 0;
    const int ss = live ? s : 0;
    const float *arow = grad_row(io.action, ss, io.nenv);
    double q = 0.0, ls_sum = 0.0;
    for (int j = 0; j < A; ++j) {
        const double ls = (double)io.log_std[j], is = reward_expn(ls);
        const double a = live ? (double)arow[j] : 0.0;
        const double d = mul_rn(sub_rn(a, (double)MU[j][e]), is);
        q = add_rn(q, mul_rn(d, d));
        ls_sum = add_rn(ls_sum, ls);
    }
    const double logp = sub_rn(sub_rn(mul_rn(-0.5, q), ls_sum), mul_rn((double)A, 0.91893853320467267));
    const double lr = sub_rn(logp, live ? (double)*grad_row(io.logp, ss, io.nenv) : 0.0);
    const double ratio = reward_expn(-lr);
    const double adv = live ? (double)*grad_row(io.advn, ss, io.nenv) : 0.0;
    const double s1 = mul_rn(ratio, adv);
    const double rc = ratio < io.lo ? io.lo : (ratio > io.hi ? io.hi : ratio);
    const double s2 = mul_rn(rc, adv);
    const bool active = !(s2 < s1);
    const double g = active ? -s1 : 0.0;
    float *drow = io.delta + io.g[0].d_off[N.nlayers - 1] + (size_t)p * (size_t)L.out16;
    double *pos = io.pos + p;
    for (int j = 0; j < L.out16; ++j) {
        float dl = 0.0f;
        if (j < A) {
            const double is = reward_expn((double)io.log_std[j]), mu = (double)MU[j][e];
            const double d = mul_rn(sub_rn(live ? (double)arow[j] : 0.0, mu), is);
            const float gmu = (float)mul_rn(g, mul_rn(d, is));
            dl = (float)grad_d(L.act, (double)gmu, mu);
            const double gls = mul_rn(g, sub_rn(mul_rn(d, d), 1.0));
            pos[(size_t)j * (size_t)io.mcap] = live ? gls : 0.0;
        }
        drow[j] = live ? dl : 0.0f;
    }
    pos += (size_t)A * (size_t)io.mcap;
    const double r1 = sub_rn(ratio, 1.0);
    pos[(size_t)GRAD_POS_PLOSS * (size_t)io.mcap] = live ? -(active ? s1 : s2) : 0.0;
    pos[(size_t)GRAD_POS_KL * (size_t)io.mcap] = live ? sub_rn(r1, lr) : 0.0;
    pos[(size_t)GRAD_POS_CLIPPED * (size_t)io.mcap] = live && fabs(r1) > io.eps ? 1.0 : 0.0;
    pos[(size_t)GRAD_POS_VOID * (size_t)io.mcap] = !live && p < io.m ? 1.0 : 0.0;
}

/* HEAD, critic: position p0 + e; V: the critic's last h (one unit) */
WV_DEVICE void grad_head_critic(const GradIO &io, int p0, int e, const float (*V)[POLICY_TILE]) {
    using namespace wv;
    const PolicyNet &N = io.net[1];
    const PolicyLayer &L = N.layer[N.nlayers - 1];
    const int p = p0 + e, s = grad_sample(io, p);
    const bool live = s >= 0;
    const double v = (double)V[0][e];
    const double dv = sub_rn(v, live ? (double)*grad_row(io.ret, live ? s : 0, io.nenv) : 0.0);
    const float gv = (float)mul_rn(io.c_v, dv);
    const float dl = (float)grad_d(L.act, (double)gv, v);
    float *drow = io.delta + io.g[1].d_off[N.nlayers - 1] + (size_t)p * (size_t)L.out16;
    for (int j = 0; j < L.out16; ++j) drow[j] = live && j == 0 ? dl : 0.0f;
    io.pos[(size_t)(io.A + GRAD_POS_VLOSS) * (size_t)io.mcap + (size_t)p] = live ? mul_rn(mul_rn(0.5, dv), dv) : 0.0;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE * POLICY_WAVES) cassie_grad_forward_kernel(GradIO io) {
    GRAD_LDS(lds);
    float (*const B0)[POLICY_TILE] = (float (*)[POLICY_TILE])lds, (*const B1)[POLICY_TILE] = B0 + io.rows0;
    int *const live = (int *)(lds + (size_t)(io.rows0 + io.rows1) * POLICY_TILE);
    const int lane = wv::lane(), wave = wv::wave_id(), tid = wave * WV_WAVE + lane;
    const int tiles = io.mcap / POLICY_TILE;
    for (int job = wv::env_id(); job < tiles * io.nnets; job += wv::grid_size()) {
        const int tile = job / io.nnets, net = job - tile * io.nnets, p0 = tile * POLICY_TILE;
        const PolicyNet &N = io.net[net];
        const GradNet &G = io.g[net];
        policy_barrier();                                                   /* (whoever still reads the buffers of the job before) */
        if (tid < POLICY_TILE) live[tid] = grad_sample(io, p0 + tid) >= 0;
        grad_load_input(io, p0, B0, tid);
        policy_barrier();
        if (net == 0) grad_store_rows(io.act + G.h_off[0], G.hw[0], N.layer[0].k4, B0, live, p0, tid);
        float (*X)[POLICY_TILE] = B0, (*Y)[POLICY_TILE] = B1;
        for (int l = 0; l < N.nlayers; ++l) {
            policy_layer(N.layer[l], io.packed, X, Y, wave, lane);
            policy_barrier();
            grad_store_rows(io.act + G.h_off[l + 1], G.hw[l + 1], N.layer[l].out16, Y, live, p0, tid);
            float (*const t)[POLICY_TILE] = X; X = Y; Y = t;
        }
        if (tid < POLICY_TILE) {                                            /* X: the network's last h */
            if (net == 0) grad_head_actor(io, p0, tid, X);
            else grad_head_critic(io, p0, tid, X);
        }
    }
}

/* BACKWARD of layer L (l >= 1): g = delta_l W_l by this wave's groups of four blocks of 16 k, from DX [u][pos] and the transposed
 * packing; delta_{l-1} = (float) D(act of the layer below, g, its kept h) into DY [k][pos] and the delta store.  The loop is
 * policy_layer's, the accumulators begin at +0.0 */
WV_DEVICE void grad_back_layer(const GradIO &io, const PolicyLayer &L, const PolicyLayer &Lb, const float *packt, const float *hkept, float *dstore,
                               const float (*DX)[POLICY_TILE], float (*DY)[POLICY_TILE], const int *live, int p0, int wave, int lane) {
    using namespace wv;
    const int w16 = Lb.out16, nkb = w16 >> 4, ksteps = ((L.out + 3) & ~3) >> 2;
    const float *const xs = &DX[0][0] + lane;                               /* word 64 us + lane = DX[4 us + (lane >> 4)][lane & 15] */
    for (int kb0 = 4 * wave; kb0 < nkb; kb0 += 4 * POLICY_WAVES) {
        const float *wp[4];
        mfma_acc c[4];
        float h[4][4];
        for (int j = 0; j < 4; ++j) {
            const int kb = kb0 + j < nkb ? kb0 + j : nkb - 1;
            wp[j] = packt + (size_t)kb * (size_t)ksteps * 64 + lane;
            for (int v = 0; v < 4; ++v) {
                c[j].c[v] = 0.0;
                h[j][v] = hkept[(size_t)(p0 + (lane >> 4) + 4 * v) * (size_t)w16 + (size_t)(kb * 16 + (lane & 15))];
            }
        }
        const int nchunks = ksteps / POLICY_CHUNK;
        float an[POLICY_CHUNK], wn[4][POLICY_CHUNK];
        if (nchunks > 0)
            for (int u = 0; u < POLICY_CHUNK; ++u) {
                an[u] = xs[64 * u];
                for (int j = 0; j < 4; ++j) wn[j][u] = wp[j][64 * u];
            }
        for (int ch = 0; ch < nchunks; ++ch) {
            float ac[POLICY_CHUNK], wc[4][POLICY_CHUNK];
            for (int u = 0; u < POLICY_CHUNK; ++u) {
                ac[u] = an[u];
                for (int j = 0; j < 4; ++j) wc[j][u] = wn[j][u];
            }
            if (ch + 1 < nchunks)
                for (int u = 0; u < POLICY_CHUNK; ++u) {
                    const int ks = (ch + 1) * POLICY_CHUNK + u;
                    an[u] = xs[64 * ks];
                    for (int j = 0; j < 4; ++j) wn[j][u] = wp[j][64 * ks];
                }
            for (int u = 0; u < POLICY_CHUNK; ++u) {
                const double a = (double)ac[u];
                mfma_f64_16x16x4_x4(a, (double)wc[0][u], c[0], a, (double)wc[1][u], c[1], a, (double)wc[2][u], c[2], a, (double)wc[3][u], c[3]);
            }
        }
        for (int ks = nchunks * POLICY_CHUNK; ks < ksteps; ++ks) {
            const double a = (double)xs[64 * ks];
            mfma_f64_16x16x4_x4(a, (double)wp[0][64 * ks], c[0], a, (double)wp[1][64 * ks], c[1], a, (double)wp[2][64 * ks], c[2],
                                a, (double)wp[3][64 * ks], c[3]);
        }
        mfma_f64_drain4(c[0], c[1], c[2], c[3]);
        for (int j = 0; j < 4; ++j) {
            if (kb0 + j >= nkb) break;                                      /* (wave-uniform) */
            const int k = (kb0 + j) * 16 + (lane & 15);
            for (int v = 0; v < 4; ++v) {
                const int e = (lane >> 4) + 4 * v;
                const float d = (float)grad_d(Lb.act, c[j].c[v], (double)h[j][v]);
                const float dl = live[e] && k < Lb.out ? d : 0.0f;
                DY[k][e] = dl;
                dstore[(size_t)(p0 + e) * (size_t)w16 + (size_t)k] = dl;
            }
        }
    }
}

WV_GLOBAL void __launch_bounds__(WV_WAVE * POLICY_WAVES) cassie_grad_backward_kernel(GradIO io) {
    GRAD_LDS(lds);
    float (*const B0)[POLICY_TILE] = (float (*)[POLICY_TILE])lds, (*const B1)[POLICY_TILE] = B0 + io.rows0;
    int *const live = (int *)(lds + (size_t)(io.rows0 + io.rows1) * POLICY_TILE);
    const int lane = wv::lane(), wave = wv::wave_id(), tid = wave * WV_WAVE + lane;
    const int tiles = io.mcap / POLICY_TILE;
    for (int job = wv::env_id(); job < tiles * io.nnets; job += wv::grid_size()) {
        const int tile = job / io.nnets, net = job - tile * io.nnets, p0 = tile * POLICY_TILE;
        const PolicyNet &N = io.net[net];
        const GradNet &G = io.g[net];
        if (N.nlayers < 2) continue;                                        /* (wave-uniform: the head left the only delta) */
        policy_barrier();
        if (tid < POLICY_TILE) live[tid] = grad_sample(io, p0 + tid) >= 0;
        /* layer l's delta lives where its h lived in the forward pass: buffer 1 for even l, buffer 0 for odd l */
        int l = N.nlayers - 1;
        float (*X)[POLICY_TILE] = (l & 1) ? B0 : B1, (*Y)[POLICY_TILE] = (l & 1) ? B1 : B0;
        {
            const int w16 = N.layer[l].out16;
            const float *src = io.delta + G.d_off[l];
            for (int i = tid; i < POLICY_TILE * w16; i += WV_WAVE * POLICY_WAVES) {
                const int e = i / w16, u = i - e * w16;
                X[u][e] = src[(size_t)(p0 + e) * (size_t)w16 + (size_t)u];
            }
        }
        policy_barrier();
        for (; l >= 1; --l) {
            grad_back_layer(io, N.layer[l], N.layer[l - 1], io.packt + G.t_off[l], io.act + G.h_off[l], io.delta + G.d_off[l - 1], X, Y, live, p0, wave, lane);
            policy_barrier();
            float (*const t)[POLICY_TILE] = X; X = Y; Y = t;
        }
    }
}

/* WEIGHT PARTIALS: one job -- chunk c of slot (net, layer), block ub of 16 units, the four blocks of 16 k from 4 kg */
WV_DEVICE void grad_partial_job(const GradIO &io, int net, int layer, int c, int ub, int kg, int lane) {
    using namespace wv;
    const PolicyLayer &L = io.net[net].layer[layer];
    const GradNet &G = io.g[net];
    const int hw = G.hw[layer], nkb = (L.in + 16) >> 4, p0 = c * io.chunk, steps = io.chunk >> 2;
    const float *ap = io.delta + G.d_off[layer] + (size_t)(p0 + (lane >> 4)) * (size_t)L.out16 + (size_t)(ub * 16 + (lane & 15));
    const size_t astep = 4 * (size_t)L.out16, bstep = 4 * (size_t)hw;
    const float *bp[4];
    float fill[4];
    bool load[4];
    mfma_acc acc[4];
    for (int j = 0; j < 4; ++j) {
        const int kb = 4 * kg + j < nkb ? 4 * kg + j : nkb - 1, k = kb * 16 + (lane & 15);
        load[j] = k < L.in;                                                 /* the column k = in is the bias': h = 1; beyond it +0.0 */
        fill[j] = k == L.in ? 1.0f : 0.0f;
        bp[j] = io.act + G.h_off[layer] + (size_t)(p0 + (lane >> 4)) * (size_t)hw + (size_t)(k < hw ? k : hw - 1);
        for (int v = 0; v < 4; ++v) acc[j].c[v] = 0.0;
    }
    /* the position steps in chunks of POLICY_CHUNK, requested a chunk ahead as in policy_layer (steps is a multiple of 4) */
    const int nch = steps / POLICY_CHUNK;
    float an[POLICY_CHUNK], bn[4][POLICY_CHUNK];
    for (int u = 0; u < POLICY_CHUNK; ++u) {
        an[u] = ap[(size_t)u * astep];
        for (int j = 0; j < 4; ++j) bn[j][u] = bp[j][(size_t)u * bstep];
    }
    for (int ch = 0; ch < nch; ++ch) {
        float ac[POLICY_CHUNK], bc[4][POLICY_CHUNK];
        for (int u = 0; u < POLICY_CHUNK; ++u) {
            ac[u] = an[u];
            for (int j = 0; j < 4; ++j) bc[j][u] = load[j] ? bn[j][u] : fill[j];
        }
        if (ch + 1 < nch)
            for (int u = 0; u < POLICY_CHUNK; ++u) {
                const size_t st = (size_t)((ch + 1) * POLICY_CHUNK + u);
                an[u] = ap[st * astep];
                for (int j = 0; j < 4; ++j) bn[j][u] = bp[j][st * bstep];
            }
        for (int u = 0; u < POLICY_CHUNK; ++u) {
            const double a = (double)ac[u];
            mfma_f64_16x16x4_x4(a, (double)bc[0][u], acc[0], a, (double)bc[1][u], acc[1], a, (double)bc[2][u], acc[2], a, (double)bc[3][u], acc[3]);
        }
    }
    mfma_f64_drain4(acc[0], acc[1], acc[2], acc[3]);
    double *dst = io.part + G.p_off[layer] + (size_t)c * (size_t)L.out * (size_t)(L.in + 1);
    for (int j = 0; j < 4; ++j) {
        if (4 * kg + j >= nkb) break;                                       /* (wave-uniform) */
        const int k = (4 * kg + j) * 16 + (lane & 15);
        for (int v = 0; v < 4; ++v) {
            const int u = ub * 16 + (lane >> 4) + 4 * v;
            if (u < L.out && k <= L.in) dst[(size_t)u * (size_t)(L.in + 1) + (size_t)k] = acc[j].c[v];
        }
    }
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_grad_partial_kernel(GradIO io) {
    const int lane = wv::lane();
    for (long long job = wv::env_id(); job < io.job0[io.nslots]; job += wv::grid_size()) {
        int s = 0;
        for (int k = 1; k < io.nslots; ++k) if (job >= io.job0[k]) s = k;   /* (the slots' first jobs ascend) */
        const int net = io.slot_net[s], layer = io.slot_layer[s];
        const PolicyLayer &L = io.net[net].layer[layer];
        const int nub = L.out16 >> 4, nkg = (((L.in + 16) >> 4) + 3) >> 2;
        const int r = (int)(job - io.job0[s]), c = r / (nub * nkg), r2 = r - c * (nub * nkg), ub = r2 / nkg;
        grad_partial_job(io, net, layer, c, ub, r2 - ub * nkg, lane);
    }
}

/* REDUCE: a lane per parameter -- the chunks' partials added in ascending order from +0.0, times 1 / m, as float32 into dW or db */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_grad_reduce_kernel(GradIO io) {
    using namespace wv;
    const long long total = io.par0[io.nslots];
    for (long long q = (long long)env_id() * WV_WAVE + lane(); q < total; q += (long long)grid_size() * WV_WAVE) {
        int s = 0;
        for (int k = 1; k < io.nslots; ++k) if (q >= io.par0[k]) s = k;
        const int net = io.slot_net[s], layer = io.slot_layer[s];
        const PolicyLayer &L = io.net[net].layer[layer];
        const long long r = q - io.par0[s], per = (long long)L.out * (L.in + 1);
        const int u = (int)(r / (L.in + 1)), k = (int)(r - (long long)u * (L.in + 1));
        const double *src = io.part + io.g[net].p_off[layer] + r;
        double sum = 0.0;
        for (int c = 0; c < io.nchunks; ++c) sum = add_rn(sum, src[(size_t)c * (size_t)per]);
        const float v = (float)mul_rn(sum, io.inv_m);
        if (k < L.in) io.dw[s][(size_t)u * (size_t)io.sdw[s] + (size_t)k] = v;
        else io.db[s][u] = v;
    }
}

/* reduce(x[m]) by ONE wave, the rollout's: padded with +0.0 to a multiple of 64, every block of 64 by wave_sum's tree, the block sums
 * added in block order from +0.0 */
WV_DEVICE double grad_reduce(const double *x, int m, int l) {
    using namespace wv;
    double sum = 0.0;
    for (int e0 = 0; e0 < m; e0 += WV_WAVE) {    /* (the bound is wave-uniform: all 64 lanes meet in wave_sum) */
        const int e = e0 + l;
        const double v = x[e < m ? e : m - 1];
        sum = add_rn(sum, wave_sum(e < m ? v : 0.0));
    }
    return sum;
}

/* STATISTICS: workgroup j < A: dls_j; A + r: the statistic of row r; the wave of the void count also writes the entropy, m and the spare */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_grad_stats_kernel(GradIO io) {
    using namespace wv;
    const int l = lane();
    for (int job = env_id(); job < io.A + GRAD_POS_ROWS; job += grid_size()) {
        const int r = job - io.A;
        if (r == GRAD_POS_VLOSS && io.nnets < 2) { if (l == 0) io.stats[1] = 0.0; continue; }   /* (nobody wrote the row) */
        const double sum = grad_reduce(io.pos + (size_t)job * (size_t)io.mcap, io.m, l);
        if (l != 0) continue;
        if (r < 0) io.dls[job] = (float)sub_rn(mul_rn(sum, io.inv_m), io.c_ent);
        else if (r == GRAD_POS_VOID) {
            double ls_sum = 0.0;
            for (int j = 0; j < io.A; ++j) ls_sum = add_rn(ls_sum, (double)io.log_std[j]);
            io.stats[4] = add_rn(ls_sum, mul_rn((double)io.A, add_rn(0.5, 0.91893853320467267)));
            io.stats[5] = sum; io.stats[6] = (double)io.m; io.stats[7] = 0.0;
        } else io.stats[r] = mul_rn(sum, io.inv_m);
    }
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_grad_pack_kernel(GradPackIO io) {
    const long long per = 16ll * io.u4, total = (long long)(io.in16 >> 4) * per;
    for (long long p = (long long)wv::env_id() * WV_WAVE + wv::lane(); p < total; p += (long long)wv::grid_size() * WV_WAVE) {
        const long long kb = p / per, r = p - kb * per;
        const int l = (int)(r & 63), u = (int)(r >> 6) * 4 + (l >> 4), k = (int)kb * 16 + (l & 15);
        const bool in = u < io.out && k < io.in;
        const size_t at = in ? (size_t)(u >> 4) * 16 * (size_t)io.k4 + (size_t)(k >> 2) * 64 + (size_t)(k & 3) * 16 + (size_t)(u & 15) : 0;
        const float w = io.src[at];
        io.dst[p] = in ? w : 0.0f;
    }
}

}  // namespace ck
#endif
