/*
 * rollout_kernels.h -- rollout rows: what lies between the policy step and the optimiser (phys_batch_rollout_*, include/cassie_phys.h:
 * the definition is there).  The transitions of a policy step are copied into slot t of a time-major store by ONE launch per env range
 * (cassie_rollout_record_kernel), the advantages and returns of a range's T steps are made by ONE launch (cassie_rollout_finish_kernel),
 * and the advantages of the whole batch are normalised by four short launches on one stream (cassie_rollout_reduce_kernel,
 * _square_kernel, _reduce_kernel again, _scale_kernel).  Written with the wv:: primitives only, workgroups of one wave: phys_batch.hip
 * launches them, the wave emulator (tests/emu/emu_rollout.cpp) runs the same text.  The launch records, the grids and the checks are
 * small_launch.h's (no field of RolloutRecIO, RolloutFinIO or RolloutNormIO is assigned anywhere else).
 *
 * The mapping:
 *   record    a fixed grid of workgroups walks JOBS; a job is ROLLOUT_JOB consecutive words of ONE source's flattened (env, j) index, so
 *             consecutive lanes store consecutive words of the slot and load consecutive words of a row.  The host decides per source
 *             whether it goes 16 bytes a lane (both pointers, dim and both row strides multiples of 4 words) or a word a lane.  A job's
 *             loads are all requested before its first store.  A word is a word: float32 and int32 alike, the copy is type-blind.
 *   finish    lane = env, ROLLOUT_FIN_GRID workgroups walk a longer range.  The chain over t is four dependent fp64 operations a step;
 *             the loads do not depend on it, and a wave alone on its SIMD hides nobody's latency (the policy kernel's lesson): the values
 *             of the next ROLLOUT_AHEAD steps are requested while the chain works through the ROLLOUT_AHEAD before them.  The sum of an
 *             env's advantages (q1) is a second pass, ascending in t, over what the lane has just stored.
 *   normalise reduce: ONE wave walks the envs in blocks of 64 -- wv::wave_sum per block, the block sums added in block order -- so the
 *             result does not depend on the grid or on how finish was cut into ranges; square: lane = env, sequential in t; scale:
 *             lane = env, a workgroup per (step, block of 64 envs).  No kernel waits for another workgroup: the stream orders them.
 * Every arithmetic step is one individually rounded fp64 operation (wv::add_rn and its kin), every sum has one order, a `done` SELECTS
 * +0.0 and never multiplies by it.  Vector loads and stores only; nothing is indexed by a value; a lane of finish touches its env alone.
 */
#ifndef CASSIE_ROLLOUT_KERNELS_H
#define CASSIE_ROLLOUT_KERNELS_H

#include "wave.h"

namespace ck {

/* the limits (PHYS_RO_MAXT, _MAXSRC, _MAXDIM); ROLLOUT_JOB: the words of a job; ROLLOUT_GRID / _FIN_GRID / _SCALE_GRID: the most
 * workgroups of a record / a lane = env / a scale launch; ROLLOUT_AHEAD: the steps whose values finish requests ahead of its chain */
constexpr int ROLLOUT_MAXT = 1024, ROLLOUT_MAXSRC = 16, ROLLOUT_MAXDIM = 4096;
constexpr int ROLLOUT_JOB = 1024, ROLLOUT_GRID = 1024, ROLLOUT_FIN_GRID = 256, ROLLOUT_SCALE_GRID = 1024, ROLLOUT_AHEAD = 8;
/* the roles of a source (PHYS_RO_DATA ... _REASON) and of the arrays a storage binding or a download names (PHYS_RO_ADV, _RET, _ADVN):
 * numbered from ROLLOUT_MAXSRC, so that one int names a source by index or by role */
enum { RO_DATA = 16, RO_OBS = 17, RO_ACTION = 18, RO_LOGP = 19, RO_MU = 20, RO_VALUE = 21, RO_REWARD = 22, RO_DONE = 23, RO_REASON = 24,
       RO_ADV = 25, RO_RET = 26, RO_ADVN = 27 };

/* a source as the caller writes it (phys_rollout_src_t of cassie_phys.h) */
struct RolloutSrcDef { int role, dim; };

/* 16 bytes of a row (a vector type, which lives in registers: an array of a four-word STRUCT was promoted to 4 KiB of LDS) */
typedef unsigned RolloutVec __attribute__((vector_size(16)));

/* a source of a record launch: the rows of the range's first env on both sides (src: where the batch reads or writes the thing; dst: slot t
 * of its store), the words between two rows, the words of a row, whether a lane moves 16 bytes, and the source's first job */
struct RolloutRecSrc { const unsigned *src; unsigned *dst; long long ssrc, sdst; int dim, vec; long long job0; };
struct RolloutRecIO { int n, nsrc; long long njobs; RolloutRecSrc s[ROLLOUT_MAXSRC]; };

/* finish: the stores of VALUE, REWARD, DONE (null: none) and REASON (null: none), ADV and RET, each with the words between two steps and
 * two envs; the value behind the last step with its stride; gamma, gamma * lambda, the mask; q1 [nenv] */
struct RolloutFinIO {
    int env0, n, T; unsigned tmask;
    double gamma, gl;
    const float *val, *rew; const int *done, *reason; const float *last;
    long long val_step, val_row, rew_step, rew_row, done_step, done_row, reason_step, reason_row, last_row;
    float *adv, *ret; long long adv_step, adv_row, ret_step, ret_row;
    double *q1;
};

/* normalise: ADV and ADVN with their strides, the per-env partials, the statistics {mean, std, inv, reduce's last sum}; reduce's stage
 * (0: mean of q1, 1: std and inv of q2) */
struct RolloutNormIO {
    int nenv, T, stage, pad;
    double count, count1, eps;           /* M and M - 1 as doubles */
    const float *adv; long long adv_step, adv_row;
    float *advn; long long advn_step, advn_row;
    double *q1, *q2, *stats;
};

/* the words [at, at + ROLLOUT_JOB) of a source's flattened index, W words a lane */
template <class V, int W> WV_DEVICE void rollout_copy_job(const RolloutRecSrc &S, long long at, long long total, int l) {
    constexpr int NIT = ROLLOUT_JOB / (WV_WAVE * W);
    const unsigned dim = (unsigned)S.dim;
    const long long env_at = at / S.dim;                       /* (wave-uniform: once a job) */
    const unsigned j_at = (unsigned)(at - env_at * S.dim);
    V v[NIT];
    size_t from[NIT], to[NIT];
    bool in[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const unsigned o = (unsigned)((k * WV_WAVE + l) * W);
        const unsigned t = j_at + o, e = t / dim, j = t - e * dim;
        in[k] = at + (long long)o < total;
        const size_t env = in[k] ? (size_t)env_at + (size_t)e : 0, jj = in[k] ? (size_t)j : 0;   /* (a lane past the end loads the first word again) */
        from[k] = env * (size_t)S.ssrc + jj; to[k] = env * (size_t)S.sdst + jj;
        v[k] = *(const V *)(S.src + from[k]);
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k)
        if (in[k]) *(V *)(S.dst + to[k]) = v[k];
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_rollout_record_kernel(RolloutRecIO io) {
    const int l = wv::lane();
    for (long long job = wv::env_id(); job < io.njobs; job += wv::grid_size()) {
        int s = 0;
        for (int k = 1; k < io.nsrc; ++k) if (job >= io.s[k].job0) s = k;   /* (the sources' first jobs ascend) */
        const RolloutRecSrc &S = io.s[s];
        const long long at = (job - S.job0) * ROLLOUT_JOB, total = (long long)io.n * S.dim;
        if (S.vec) rollout_copy_job<RolloutVec, 4>(S, at, total, l);
        else rollout_copy_job<unsigned, 1>(S, at, total, l);
    }
}

/* what finish reads of a step */
struct RolloutStep { float v, r; int d, q; };
/* the lane's place in the four stores and in ADV and RET, walked from the last step down, with the words between two steps of each.  The
 * steps are held PER LANE (a zero the compiler cannot see through is added to them): with wave-uniform steps the compiler splits every
 * address into a lane's part and a scalar k * step per step in flight -- 106 scalar registers and 90 to 147 of them spilled */
struct RolloutCursor { const float *v, *r; const int *d, *q; float *adv, *ret; long long sv, sr, sd, sq, sadv, sret; };
/* the step at the cursor, which moves a step down; below the first step (t < 0, wave-uniform) nothing is loaded */
WV_DEVICE RolloutStep rollout_load_step(const RolloutFinIO &io, RolloutCursor &c, int t) {
    RolloutStep s = {0.0f, 0.0f, 0, 0};
    if (t >= 0) {
        s.v = *c.v; s.r = *c.r;
        if (io.done) s.d = *c.d;
        if (io.reason) s.q = *c.q;
    }
    c.v -= c.sv; c.r -= c.sr; c.d -= c.sd; c.q -= c.sq;
    return s;
}

/* env env0 + i of the range: the chain from T - 1 down, then q1 from 0 up */
WV_DEVICE void rollout_finish_env(const RolloutFinIO &io, int i) {
    using namespace wv;
    const size_t env = (size_t)io.env0 + (size_t)i, top = (size_t)(io.T - 1);
    double nv = (double)io.last[env * (size_t)io.last_row], a = 0.0;
    int zero = 0;
    keep(zero);
    RolloutCursor c;
    c.sv = io.val_step + zero; c.sr = io.rew_step + zero; c.sd = io.done_step + zero; c.sq = io.reason_step + zero;
    c.sadv = io.adv_step + zero; c.sret = io.ret_step + zero;
    c.v = io.val + top * (size_t)c.sv + env * (size_t)io.val_row;
    c.r = io.rew + top * (size_t)c.sr + env * (size_t)io.rew_row;
    c.d = io.done + top * (size_t)c.sd + env * (size_t)io.done_row;          /* (null: never read, and its step is 0) */
    c.q = io.reason + top * (size_t)c.sq + env * (size_t)io.reason_row;
    c.adv = io.adv + top * (size_t)c.sadv + env * (size_t)io.adv_row;
    c.ret = io.ret + top * (size_t)c.sret + env * (size_t)io.ret_row;
    RolloutStep cur[ROLLOUT_AHEAD], nxt[ROLLOUT_AHEAD];
#pragma unroll
    for (int k = 0; k < ROLLOUT_AHEAD; ++k) cur[k] = rollout_load_step(io, c, io.T - 1 - k);
    for (int t0 = io.T - 1; t0 >= 0; t0 -= ROLLOUT_AHEAD) {
#pragma unroll
        for (int k = 0; k < ROLLOUT_AHEAD; ++k) nxt[k] = rollout_load_step(io, c, t0 - ROLLOUT_AHEAD - k);
#pragma unroll
        for (int k = 0; k < ROLLOUT_AHEAD; ++k) {
            const int t = t0 - k;
            if (t >= 0) {
                const double v = (double)cur[k].v;
                double r = (double)cur[k].r;
                const bool d = cur[k].d != 0;
                const unsigned q = (unsigned)cur[k].q;
                const double rb = add_rn(r, mul_rn(io.gamma, v));   /* (an episode cut by the time limit bootstraps from the step's own value) */
                if (io.tmask != 0u && d && (q & io.tmask) != 0u && (q & ~io.tmask) == 0u) r = rb;
                const double nvs = d ? 0.0 : nv, as = d ? 0.0 : a;
                const double delta = sub_rn(add_rn(r, mul_rn(io.gamma, nvs)), v);
                a = add_rn(delta, mul_rn(io.gl, as));
                *c.adv = (float)a; *c.ret = (float)add_rn(a, v);
                c.adv -= c.sadv; c.ret -= c.sret;
                nv = v;
            }
        }
#pragma unroll
        for (int k = 0; k < ROLLOUT_AHEAD; ++k) cur[k] = nxt[k];
    }
    double q1 = 0.0;
    c.adv += c.sadv;     /* (the chain left it a step below the first) */
    for (int t0 = 0; t0 < io.T; t0 += ROLLOUT_AHEAD) {
        float x[ROLLOUT_AHEAD];
#pragma unroll
        for (int k = 0; k < ROLLOUT_AHEAD; ++k) {
            x[k] = 0.0f;
            if (t0 + k < io.T) x[k] = *c.adv;
            c.adv += c.sadv;
        }
#pragma unroll
        for (int k = 0; k < ROLLOUT_AHEAD; ++k)
            if (t0 + k < io.T) q1 = add_rn(q1, (double)x[k]);
    }
    io.q1[env] = q1;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_rollout_finish_kernel(RolloutFinIO io) {
    for (int i = wv::env_id() * WV_WAVE + wv::lane(); i < io.n; i += wv::grid_size() * WV_WAVE) rollout_finish_env(io, i);
}

/* reduce(x[nenv]) by ONE wave: the envs padded with +0.0 to a multiple of 64, every block of 64 summed by wave_sum's tree, the block
 * sums added in block order from +0.0.  Stage 0: mean = reduce(q1) / M; stage 1: std = sqrt(reduce(q2) / (M - 1)), inv = 1 / (std + eps) */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_rollout_reduce_kernel(RolloutNormIO io) {
    using namespace wv;
    const int l = lane();
    const double *x = io.stage == 0 ? io.q1 : io.q2;
    double sum = 0.0;
    for (int e0 = 0; e0 < io.nenv; e0 += WV_WAVE) {    /* (the bound is wave-uniform: all 64 lanes meet in wave_sum) */
        const int e = e0 + l;
        const double v = x[e < io.nenv ? e : io.nenv - 1];
        sum = add_rn(sum, wave_sum(e < io.nenv ? v : 0.0));
    }
    if (l == 0) {
        io.stats[3] = sum;
        if (io.stage == 0) io.stats[0] = div_rn(sum, io.count);
        else {
            const double sd = sqrt_rn(div_rn(sum, io.count1));
            io.stats[1] = sd;
            io.stats[2] = div_rn(1.0, add_rn(sd, io.eps));
        }
    }
}

/* q2[env] = sum over t ascending from +0.0 of ((double) ADV[t][env] - mean)^2 */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_rollout_square_kernel(RolloutNormIO io) {
    using namespace wv;
    const double mean = io.stats[0];
    for (int e = env_id() * WV_WAVE + lane(); e < io.nenv; e += grid_size() * WV_WAVE) {
        double q2 = 0.0;
        for (int t0 = 0; t0 < io.T; t0 += ROLLOUT_AHEAD) {
            float x[ROLLOUT_AHEAD];
#pragma unroll
            for (int k = 0; k < ROLLOUT_AHEAD; ++k) {
                const int t = t0 + k < io.T ? t0 + k : io.T - 1;
                x[k] = io.adv[(size_t)t * (size_t)io.adv_step + (size_t)e * (size_t)io.adv_row];
            }
#pragma unroll
            for (int k = 0; k < ROLLOUT_AHEAD; ++k)
                if (t0 + k < io.T) { const double c = sub_rn((double)x[k], mean); q2 = add_rn(q2, mul_rn(c, c)); }
        }
        io.q2[e] = q2;
    }
}

/* ADVN[t][env] = (float)(((double) ADV[t][env] - mean) * inv): a job is a step's block of 64 envs */
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_rollout_scale_kernel(RolloutNormIO io) {
    using namespace wv;
    const double mean = io.stats[0], inv = io.stats[2];
    const long long blocks = ((long long)io.nenv + WV_WAVE - 1) / WV_WAVE, njobs = blocks * io.T;
    for (long long job = env_id(); job < njobs; job += grid_size()) {
        const long long t = job / blocks;
        const int e = (int)(job - t * blocks) * WV_WAVE + lane();
        if (e < io.nenv) {
            const float x = io.adv[(size_t)t * (size_t)io.adv_step + (size_t)e * (size_t)io.adv_row];
            io.advn[(size_t)t * (size_t)io.advn_step + (size_t)e * (size_t)io.advn_row] = (float)mul_rn(sub_rn((double)x, mean), inv);
        }
    }
}

}  // namespace ck
#endif
