/*
 * policy_kernels.h -- policy rows: the function between the observation row and the action tensor, a small MLP actor (and critic) with
 * float32 weights and activations accumulated in fp64 on the matrix core (phys_batch_policy, include/cassie_phys.h: the definition is
 * there).  ONE launch per env range evaluates up to two networks of up to four dense layers on the bound input rows, and optionally draws
 * the action from the caller's standard normal numbers with its log-probability.  Written with the wv:: primitives only: phys_batch.hip
 * launches it, the wave emulator (tests/emu/emu_policy.cpp) runs the same text.  The launch record, the checks, the grid and the packed
 * layout's offsets are small_launch.h's (no field of PolicyIO or PolicyPackIO is assigned anywhere else).
 *
 * Why it is exact: the product of two float32 values is exact in a double, so fma((double) w, (double) x, acc) is ONE rounding of
 * acc + w x, and wv::mfma_f64_16x16x4 is pinned to the plain FMA chain over k on top of C (tests/test_wave_primitives.py).  A layer is
 * therefore the sequential sum over k ascending from the bias, whichever unit takes it; a numpy restatement (tests/policy_check.py)
 * writes it as acc = acc + w * x on doubles.
 *
 * The mapping:
 *   a job          a workgroup of POLICY_WAVES waves takes one network of a tile of 16 consecutive envs of the range (the actor and the
 *                  critic share nothing but the input rows, and two workgroups fill a CU's four SIMDs where one leaves two idle);
 *                  min(tiles x networks, POLICY_GRID) workgroups walk the jobs.
 *   the LDS        two buffers of rows of 16 float32, input and output of alternating layers -- dynamic LDS the launcher sizes by the
 *                  policy's widths (policy_lds_bytes: 64 KiB at the limits, 37 KiB for 340 -> 256 -> 256: under a step workgroup's 40) -- laid out
 *                  [k][env]: lane l's A operand of the k-step k0, x[env l & 15][k0 + (l >> 4)], is then word 16 k0 + l -- one
 *                  conflict-free 256-byte read per wave instruction.  ([env][k], 512 words between two envs, is a 16-way bank conflict on
 *                  every such read.)  The tile's input rows are loaded coalesced along k, normalised and converted once per network.
 *   the weights    packed by cassie_policy_pack_kernel: per block of 16 units and k-step of 4, the 64 words w[unit l & 15][k0 + (l >> 4)]
 *                  in lane order, zero-padded to K4 and to 16 units -- lane l's B operand is one coalesced 256-byte load per wave
 *                  instruction.  The biases follow a layer's weights, padded to 16 units.
 *   a layer        a wave takes groups of four unit blocks (wave w the groups w, w + POLICY_WAVES, ...) and runs k in steps of 4 through
 *                  wv::mfma_f64_16x16x4_x4, four independent accumulations in flight, one A operand for the four.  A group that reaches
 *                  past the layer's blocks computes its last block again and drops it: all 64 lanes are active in every matrix
 *                  instruction, and nothing in the loop is conditional.  Lane l holds C[env (l >> 4) + 4 v][unit l & 15], initialised
 *                  with the bias; the activation and the conversion run on these registers and h goes to the other buffer (+0.0 in the
 *                  padded units, which the next layer's padding k reads).  A workgroup barrier separates the layers.
 *   the outputs    a network's last h is stored from LDS, consecutive lanes to consecutive elements of a row.
 *   the sample     one lane per env of the tile, sequential in j.
 * Envs past the end of the range load +0.0 and store nothing.  Vector loads and stores only; nothing indexes memory by a value; an
 * env's lanes read that env's input and eps rows and write that env's outputs alone (the elements of C are independent, so a NaN of
 * one env stays in its row of C).  No stepping kernel is handed any of this.
 */
#ifndef CASSIE_POLICY_KERNELS_H
#define CASSIE_POLICY_KERNELS_H

#include "expn.h"

namespace ck {

/* POLICY_GRID: the workgroups that walk a range's jobs, a network of a tile of 16 envs at a time: one pass up to 4096 envs of an actor and
 * a critic.  POLICY_WAVES: the waves of a workgroup, which split a layer's unit blocks (two: what emu::run_grid schedules).
 * POLICY_CHUNK: the k-steps whose operands are requested ahead.  First choices but for what the first device run forced
 * (tools/policy_rate.py measures the call) */
constexpr int POLICY_GRID = 512, POLICY_TILE = 16, POLICY_WAVES = 2, POLICY_CHUNK = 4, POLICY_PACK_GRID = 64;
constexpr int POLICY_MAXNETS = 2, POLICY_MAXLAYERS = 4, POLICY_MAXDIM = 512, POLICY_MAXOUT = 64;
enum { POL_IDENTITY = 0, POL_RELU = 1, POL_ELU = 2, POL_TANH = 3 };   /* (PHYS_POL_IDENTITY, _RELU, _ELU, _TANH of cassie_phys.h) */

/* a layer and a network as the caller writes them (phys_pol_layer_t, phys_pol_net_t of cassie_phys.h) */
struct PolicyLayerDef { int in, out, act; };
struct PolicyNetDef { int nlayers; PolicyLayerDef layer[POLICY_MAXLAYERS]; };

/* a layer as a launch reads it: k4 = in rounded up to 4, out16 = out rounded up to 16, and where its packed weights [out16 / 16][k4 / 4][64]
 * and biases [out16] begin among the packed floats */
struct PolicyLayer { int in, out, act, k4, out16, pad; long long w_off, b_off; };
struct PolicyNet { int nlayers, pad; PolicyLayer layer[POLICY_MAXLAYERS]; };

struct PolicyIO {
    int env0, n, nnets, in_dim;
    int rows0, rows1;                         /* the rows [16] of the two LDS buffers: what the widest input and output of the layers need */
    PolicyNet net[POLICY_MAXNETS];
    const float *packed;                      /* the packed weights and biases of every layer */
    const float *x; long long sx;             /* [nenv] input rows of in_dim floats, sx elements apart */
    const float *mean, *inv; double clip;     /* null, or [in_dim] each: the normalisation and its clip (+inf: none) */
    float *out[POLICY_MAXNETS]; long long sout[POLICY_MAXNETS];   /* null, or [nenv] rows of the network's last h, sout elements apart */
    const float *eps; long long seps;         /* null, or [nenv] rows of A standard normal draws, seps elements apart */
    const float *log_std;                     /* [A] */
    float *action; long long saction;         /* [nenv] rows of A, saction elements apart */
    float *logp;                              /* [nenv] */
};

/* one layer's weights [out][in] (rows sw elements apart) and biases [out] into the packed layout */
struct PolicyPackIO {
    const float *w; long long sw; const float *b;
    float *dst_w, *dst_b;
    int in, out, k4, out16;
};

/* the activations, every step one individually rounded fp64 operation (the definition: cassie_phys.h) */
WV_DEVICE double policy_act(int act, double z) {
    using namespace wv;
    if (act == POL_RELU) return z < 0.0 ? 0.0 : z;                         /* (a NaN and -0.0 pass) */
    if (act == POL_TANH) {
        if (z != z) return z;
        const double m = fabs(z);
        if (m < 0.0009765625) return sub_rn(z, mul_rn(z, mul_rn(mul_rn(z, z), 0.33333333333333331)));
        const double t = reward_expn(mul_rn(2.0, m));
        const double v = div_rn(sub_rn(1.0, t), add_rn(1.0, t));
        return z < 0.0 ? -v : v;
    }
    if (act == POL_ELU) {
        if (!(z < 0.0)) return z;                                           /* z >= 0, -0.0 or NaN */
        if (z > -0.0009765625) return add_rn(z, mul_rn(mul_rn(z, z), add_rn(0.5, mul_rn(z, 0.16666666666666666))));
        return sub_rn(reward_expn(-z), 1.0);
    }
    return z;
}

/* the workgroup's LDS: io.rows0 + io.rows1 rows of 16 floats, sized by the launcher from the policy's widths (policy_lds_bytes), so that a
 * policy of 340 -> 256 -> 256 takes 37 KiB where the limits take 64: a workgroup then fits where ONE workgroup of the step kernel has ended.
 * The emulator's is static and sized for the limits */
#ifdef CK_EMULATED
#define POLICY_LDS(name) WV_SHARED float name[2 * POLICY_MAXDIM * POLICY_TILE]
#else
#define POLICY_LDS(name) extern __shared__ float name[]
#endif

WV_DEVICE void policy_barrier() { if (POLICY_WAVES > 1) wv::block_barrier(); else wv::sync(); }

/* INPUT: the tile's rows into X[k][env], normalised where a normalisation is bound; +0.0 in the padding k and in the envs past the range */
WV_DEVICE void policy_load_input(const PolicyIO &io, int e0, int cnt, float (*X)[POLICY_TILE], int tid) {
    using namespace wv;
    const int k4 = io.net[0].layer[0].k4;
    for (int idx = tid; idx < POLICY_TILE * k4; idx += WV_WAVE * POLICY_WAVES) {
        const int e = idx / k4, k = idx - e * k4;
        float v = 0.0f;
        if (e < cnt && k < io.in_dim) {
            v = io.x[((size_t)io.env0 + (size_t)(e0 + e)) * (size_t)io.sx + (size_t)k];
            if (io.mean) {
                const double y = mul_rn(sub_rn((double)v, (double)io.mean[k]), (double)io.inv[k]);
                const double lo = -io.clip, hi = io.clip;
                v = (float)(y < lo ? lo : (y > hi ? hi : y));              /* (a NaN passes) */
            }
        }
        X[k][e] = v;
    }
}

/* LAYER: this wave's groups of four unit blocks of L, from X into Y */
WV_DEVICE void policy_layer(const PolicyLayer &L, const float *packed, const float (*X)[POLICY_TILE], float (*Y)[POLICY_TILE], int wave, int lane) {
    using namespace wv;
    const int nub = L.out16 >> 4, ksteps = L.k4 >> 2;
    const float *const xs = &X[0][0] + lane;                                /* word 64 ks + lane = X[4 ks + (lane >> 4)][lane & 15] */
    for (int ub0 = 4 * wave; ub0 < nub; ub0 += 4 * POLICY_WAVES) {
        const float *wp[4];
        mfma_acc c[4];
        for (int j = 0; j < 4; ++j) {
            const int ub = ub0 + j < nub ? ub0 + j : nub - 1;
            wp[j] = packed + L.w_off + (size_t)ub * (size_t)ksteps * 64 + lane;
            const double bias = (double)packed[L.b_off + ub * 16 + (lane & 15)];
            for (int v = 0; v < 4; ++v) c[j].c[v] = bias;
        }
        /* k-steps in chunks of POLICY_CHUNK, the operands of the chunk after this one requested before this one's matrix instructions
         * are issued: a wave has its SIMD to itself, so nobody else hides the latency of its loads (the plain loop waited for every
         * k-step's five loads: 311 us a 4096-env call where this form takes a third).  The k-steps past the last whole chunk
         * go one by one: K4 is the definition's, padding it further would turn a bias of -0.0 into +0.0 */
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
            if (ub0 + j >= nub) break;                                      /* (wave-uniform) */
            const int unit = (ub0 + j) * 16 + (lane & 15);
            for (int v = 0; v < 4; ++v) {
                const float h = (float)policy_act(L.act, c[j].c[v]);
                Y[unit][(lane >> 4) + 4 * v] = unit < L.out ? h : 0.0f;
            }
        }
    }
}

/* SAMPLE: env e of the tile, sequential in j; MU: the actor's last h */
WV_DEVICE void policy_sample(const PolicyIO &io, int A, size_t env, int e, const float (*MU)[POLICY_TILE]) {
    using namespace wv;
    double q = 0.0, ls_sum = 0.0;
    for (int j = 0; j < A; ++j) {
        const double ls = (double)io.log_std[j], s = reward_expn(-ls);
        const double ep = (double)io.eps[env * (size_t)io.seps + (size_t)j];
        io.action[env * (size_t)io.saction + (size_t)j] = (float)add_rn((double)MU[j][e], mul_rn(s, ep));
        q = add_rn(q, mul_rn(ep, ep));
        ls_sum = add_rn(ls_sum, ls);
    }
    io.logp[env] = (float)sub_rn(sub_rn(mul_rn(-0.5, q), ls_sum), mul_rn((double)A, 0.91893853320467267));
}

WV_GLOBAL void __launch_bounds__(WV_WAVE * POLICY_WAVES) cassie_policy_kernel(PolicyIO io) {
    POLICY_LDS(lds);
    float (*const B0)[POLICY_TILE] = (float (*)[POLICY_TILE])lds, (*const B1)[POLICY_TILE] = B0 + io.rows0;
    const int lane = wv::lane(), wave = wv::wave_id(), tid = wave * WV_WAVE + lane;
    const int tiles = (io.n + POLICY_TILE - 1) / POLICY_TILE;
    /* a job is (tile, network): the actor and the critic of a tile share nothing but the input rows */
    for (int job = wv::env_id(); job < tiles * io.nnets; job += wv::grid_size()) {
        const int tile = job / io.nnets, net = job - tile * io.nnets;
        const int e0 = tile * POLICY_TILE, cnt = io.n - e0 < POLICY_TILE ? io.n - e0 : POLICY_TILE;
        const PolicyNet &N = io.net[net];
        policy_barrier();                                                   /* (whoever still reads the buffers of the job before) */
        policy_load_input(io, e0, cnt, B0, tid);
        policy_barrier();
        float (*X)[POLICY_TILE] = B0, (*Y)[POLICY_TILE] = B1;
        for (int l = 0; l < N.nlayers; ++l) {
            policy_layer(N.layer[l], io.packed, X, Y, wave, lane);
            policy_barrier();
            float (*const t)[POLICY_TILE] = X; X = Y; Y = t;
        }
        const int A = N.layer[N.nlayers - 1].out;                           /* X: the network's last h */
        if (io.out[net])
            for (int idx = tid; idx < cnt * A; idx += WV_WAVE * POLICY_WAVES) {
                const int e = idx / A, j = idx - e * A;
                io.out[net][((size_t)io.env0 + (size_t)(e0 + e)) * (size_t)io.sout[net] + (size_t)j] = X[j][e];
            }
        if (net == 0 && io.eps && tid < cnt) policy_sample(io, A, (size_t)io.env0 + (size_t)(e0 + tid), tid, X);
    }
}

/* word p of a layer's packed weights is w[unit][k] of block p / (16 k4), k-step (p % (16 k4)) / 64, lane p % 64: unit = 16 block +
 * (lane & 15), k = 4 k-step + (lane >> 4); +0.0 where unit >= out or k >= in.  Then the biases, +0.0 where unit >= out. */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_policy_pack_kernel(PolicyPackIO io) {
    const long long per = 16ll * io.k4, total = (long long)(io.out16 >> 4) * per;
    for (long long p = (long long)wv::env_id() * WV_WAVE + wv::lane(); p < total + io.out16; p += (long long)wv::grid_size() * WV_WAVE) {
        if (p < total) {
            const long long ub = p / per, r = p - ub * per;
            const int l = (int)(r & 63), unit = (int)ub * 16 + (l & 15), k = (int)(r >> 6) * 4 + (l >> 4);
            io.dst_w[p] = unit < io.out && k < io.in ? io.w[(size_t)unit * (size_t)io.sw + (size_t)k] : 0.0f;
        } else {
            const int unit = (int)(p - total);
            io.dst_b[unit] = unit < io.out ? io.b[unit] : 0.0f;
        }
    }
}

}  // namespace ck
#endif
