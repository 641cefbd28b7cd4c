/*
 * draw_kernels.h -- draw rows: the two random inputs of a training iteration that were the caller's generator's -- the standard normal
 * rows the policy's SAMPLE reads as eps (phys_batch_draw) and the permutation an epoch's minibatches are cut from (phys_batch_draw_perm;
 * include/cassie_phys.h: the definition is there, DRAW ROWS).  Both are functions of a seed and a counter alone: Philox4x32-10
 * (obs_kernels.h's routine, called, not copied) on (env_base + env, column block, the env's call count, 4) for the normal rows and on
 * (R, round, epoch, 5) for the shuffle's round function.  Written with the wv:: primitives only, workgroups of one wave: phys_batch.hip
 * launches them, the wave emulator (tests/emu/emu_draw.cpp) runs the same text.  The launch records, the checks and the grids are
 * small_launch.h's (no field of DrawIO or DrawPermIO is assigned anywhere else).
 *
 *   normal rows  cassie_draw_kernel: lane = (env, block of four columns).  An env takes `lanes` consecutive lanes of ONE wave (the power
 *                of two >= ceil(A / 4), at most 16), so a wave takes 64 / lanes envs at a time and DRAW_GRID workgroups walk the range.
 *                One Philox a lane gives four words, two Box-Muller pairs, four values: u = (w + 0.5) 2^-32 in (0, 1), the radius
 *                sqrt(-2 logn(u)) (logn.h), the angle by task_kernels.h's task_sincos2pi.  No rejection, no loop: |z| <= sqrt(66 ln 2).
 *                Where the host found the destination's pointer and stride multiples of 16 bytes, a lane whose four columns all lie
 *                below A stores them as 16 bytes; a word a column otherwise.  Envs past the range and columns past A store nothing.
 *   the count    counts[env] is read by every lane of the env for itself; wv::sync() (no instruction on the device: the env's lanes are
 *                lanes of one wave, which issues the loads before the store) stands between those loads and the store of count + 1 by
 *                the env's first lane.  No value crosses a lane.
 *   the shuffle  cassie_draw_perm_kernel: lane = index.  Six Feistel rounds on the halves of a b-bit word, b the smallest even number
 *                of bits with 2^b >= max(n, 4), repeated while the word is >= n (cycle walking).  THE WALK IS BOUNDED: the six rounds
 *                are a bijection of [0, 2^b), so the values >= n a walk from i < n meets are distinct, and it ends within
 *                2^b - n + 1 <= max(3 n, 4) applications (`walk_max`, which the loop also counts against: it never gets there).  No atomic, no
 *                waiting on another lane or workgroup: every index stands alone.
 * Vector loads and stores only, no LDS; nothing is indexed by a drawn value.  No stepping kernel is handed any of this.
 */
#ifndef CASSIE_DRAW_KERNELS_H
#define CASSIE_DRAW_KERNELS_H

#include "obs_kernels.h"
#include "task_kernels.h"
#include "logn.h"

namespace ck {

/* the limits of a configuration (PHYS_DRAW_*); DRAW_GRID, DRAW_PERM_GRID: the most workgroups of a launch, which then walk; the words 3
 * of the two counters (0 .. 3 are the observation's, the action's and the task's two) */
constexpr int DRAW_MAXA = 64, DRAW_GRID = 1024, DRAW_PERM_GRID = 4096, DRAW_ROUNDS = 6;
constexpr long long DRAW_MAXPERM = 1ll << 30;
constexpr unsigned DRAW_TAG_NORMAL = 4u, DRAW_TAG_PERM = 5u;

/* 16 bytes of a row (a vector type, which lives in registers) */
typedef float DrawVec __attribute__((vector_size(16)));

/* a call of the normal rows: the range, the columns, the lanes of an env and the envs of a wave, whether a lane may store 16 bytes; the
 * counter's offset and the key (seed & 0xffffffff, seed >> 32); the rows [nenv][A], srow floats apart; the envs' call counts */
struct DrawIO {
    int env0, n, A, lanes, per_wave, vec;
    unsigned env_base, key0, key1, pad;
    float *rows; long long srow;
    unsigned *counts;
};

/* a shuffle: n, the bits of a half with its mask, the most applications of a walk; the epoch and the key; perm[0 .. n) */
struct DrawPermIO {
    unsigned n, h, mask, epoch, key0, key1;
    long long walk_max;
    int *perm;
};

/* the two values of a Box-Muller pair from two words: (rad cos, rad sin) */
WV_DEVICE void draw_pair(unsigned a, unsigned b, double &zc, double &zs) {
    using namespace wv;
    const double u = mul_rn(add_rn((double)a, 0.5), 2.3283064365386962890625e-10);      /* (a + 0.5) 2^-32: exact, in (0, 1) */
    const double theta = mul_rn((double)b, 2.3283064365386962890625e-10);                /* b 2^-32: exact, in [0, 1) */
    const double rad = sqrt_rn(mul_rn(-2.0, logn(u)));
    double sn, cs;
    task_sincos2pi(theta, sn, cs);
    zc = mul_rn(rad, cs); zs = mul_rn(rad, sn);
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_draw_kernel(DrawIO io) {
    using namespace wv;
    const int l = lane(), q = l & (io.lanes - 1), sub = l / io.lanes;
    const int j0 = 4 * q;
    for (int base = env_id() * io.per_wave; base < io.n; base += grid_size() * io.per_wave) {
        const int i = base + sub;
        const bool live = i < io.n && j0 < io.A;
        const size_t env = (size_t)io.env0 + (size_t)(live ? i : base);     /* (an idle lane reads the wave's first env's count again) */
        const unsigned count = io.counts[env];
        sync();                                                              /* every lane of the env has its count: now it may move */
        if (!live) continue;
        unsigned w[4];
        philox4x32_10(io.env_base + (unsigned)env, (unsigned)q, count, DRAW_TAG_NORMAL, io.key0, io.key1, w);
        double z[4];
        draw_pair(w[0], w[1], z[0], z[1]);
        draw_pair(w[2], w[3], z[2], z[3]);
        float *const row = io.rows + env * (size_t)io.srow + (size_t)j0;
        if (io.vec && j0 + 3 < io.A) {
            DrawVec v;
            v[0] = (float)z[0]; v[1] = (float)z[1]; v[2] = (float)z[2]; v[3] = (float)z[3];
            *(DrawVec *)row = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k < io.A) row[k] = (float)z[k];
        }
        if (q == 0) io.counts[env] = count + 1u;
    }
}

/* one application of the six rounds to x < 2^(2 h) */
WV_DEVICE unsigned draw_feistel(const DrawPermIO &io, unsigned x) {
    unsigned L = x >> io.h, R = x & io.mask;
    for (unsigned r = 0; r < (unsigned)DRAW_ROUNDS; ++r) {
        unsigned w[4];
        philox4x32_10(R, r, io.epoch, DRAW_TAG_PERM, io.key0, io.key1, w);
        const unsigned t = L ^ (w[0] & io.mask);
        L = R; R = t;
    }
    return (L << io.h) | R;
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_draw_perm_kernel(DrawPermIO io) {
    const long long step = (long long)wv::grid_size() * WV_WAVE;
    for (long long i = (long long)wv::env_id() * WV_WAVE + wv::lane(); i < (long long)io.n; i += step) {
        unsigned x = draw_feistel(io, (unsigned)i);
        for (long long k = 1; x >= io.n && k < io.walk_max; ++k) x = draw_feistel(io, x);   /* (bounded: the header says why) */
        io.perm[i] = (int)x;
    }
}

}  // namespace ck
#endif
