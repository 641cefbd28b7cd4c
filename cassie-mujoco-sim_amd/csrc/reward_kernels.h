/*
 * reward_kernels.h -- reward rows: the scalar a training loop gives its policy for a step (phys_batch_reward, include/cassie_phys.h: the
 * definition is there).  A configured table of terms -- each a slice of a field of the batch or of the caller's own per-env input array,
 * minus a target, through a deadband, a norm and a shape, times a weight and a gate -- is evaluated for an env range by ONE launch: the
 * reward, optionally every term's contribution, and the running return of the env's episode.  Written with the wv:: primitives only,
 * workgroups of one wave: phys_batch.hip launches it, the wave emulator (tests/emu/emu_rewards.cpp) runs the same text.  The launch
 * record, the term table, the grid and the checks are small_launch.h's (no field of RewardIO is assigned anywhere else).
 *
 * The mapping, and why it is not the observation's:
 *   lane = env     a lane takes one env and walks the term table; workgroup w of the grid takes envs 64 w .. 64 w + 63 of the range and
 *                  REWARD_GRID workgroups walk a longer one.  The output is one scalar per env, so consecutive lanes store consecutive
 *                  rewards and returns; the term table and the sources' descriptors are the same for every lane (the index into them is
 *                  the loop counter, which the compiler keeps in scalar registers and reads with scalar LOADS), so no lane diverges from
 *                  its neighbours but at a NaN or at expn's cut, and nothing crosses lanes: no shuffle, no barrier, no LDS.
 *   the loads      element k of a source is read by the 64 lanes at 64 rows, one row stride apart: uncoalesced, 8 (or 4) bytes a lane.
 *                  A 12-term locomotion reward reads ~60 elements of an env: 60 such loads a wave, from rows the step kernel has just
 *                  written (L2).  lane = term with a reduction would coalesce them and pay for it with a sum whose ORDER the definition
 *                  fixes (sequential, in term order): 12 dependent adds through a shuffle each.  Not measured; a first choice.
 *   the sums       every sum is sequential from +0.0 in index order and every step one individually rounded operation (wv::mul_rn /
 *                  add_rn / sub_rn / div_rn / sqrt_rn), so the choice of mapping cannot change a bit: the device, the emulator and a
 *                  numpy restatement (tests/rewards_check.py) agree bit for bit.
 *   arithmetic     per env and term: count loads, ~3 count + 4 fp64 operations, and for an EXP shape 31 more (reward_expn): a few
 *                  hundred fp64 operations an env, against the ~10^6 of the 50 substeps in front of it.
 * Vector loads and stores only; a lane reads its env's source rows and touches its env's reward, term row, return and final return
 * alone.  No value indexes memory: a NaN or a diverged env flows through to its own outputs.  No stepping kernel is handed any of this.
 */
#ifndef CASSIE_REWARD_KERNELS_H
#define CASSIE_REWARD_KERNELS_H

#include "expn.h"
#include "obs_kernels.h"

namespace ck {

/* REWARD_GRID: the workgroups that walk a range, 64 envs each: one pass up to 4096 envs.  Few, as the observation's: the launch runs
 * behind a range's step launch while the other range's step kernel fills the chip (tools/reward_rate.py measures it there). */
constexpr int REWARD_GRID = 64, REWARD_MAXTERMS = 64, REWARD_MAXCOUNT = 64, REWARD_MAXSLOTS = OBS_MAXSLOTS;
enum { REW_VEC = 0, REW_ROT_INV = 1, REW_QUAT = 2 };                 /* (PHYS_REW_VEC, _ROT_INV, _QUAT of cassie_phys.h) */
enum { REW_SUMSQ = 0, REW_SUMABS = 1, REW_MAXABS = 2 };              /* (PHYS_REW_SUMSQ, _SUMABS, _MAXABS) */
enum { REW_LINEAR = 0, REW_EXP = 1, REW_RATIONAL = 2 };              /* (PHYS_REW_LINEAR, _EXP, _RATIONAL) */
constexpr int REW_INPUT = OBS_INPUT, REW_CONST = OBS_CONST, REW_NONE = -3;   /* (PHYS_REW_INPUT, _CONST, _NONE: what is no field of the batch) */

/* a term as the caller writes it (phys_reward_term_t of cassie_phys.h).  In the table a launch reads, field / qfield / tfield / gfield
 * hold the SLOT of the source among the call's instead (REW_CONST and REW_NONE stay as they are) */
struct RewardTerm {
    int kind, field, index, count, qfield, qindex, tfield, tindex, gfield, gindex, norm, shape, root;
    double vec[4];
    double target, dead, k, weight;
};

/* a source of the call: the observation's record (rows, the elements between two of them, whether they are floats) */
typedef ObsSrc RewardSrc;

struct RewardIO {
    int env0, n, nterms, f32;           /* f32: the rewards and the term rows are floats */
    double lo, hi;                      /* the clip of the reward */
    const RewardTerm *terms;            /* [nterms], the fields as slots */
    RewardSrc src[REWARD_MAXSLOTS];
    void *rew; long long srew;          /* [nenv] rewards, srew elements apart */
    void *trows; long long sterm;       /* null, or [nenv] rows [nterms] of contributions, sterm elements apart */
    double *ret, *fin;                  /* [nenv] the running return of the env's episode; the return of the last one that ended */
    const int *reset;                   /* [n] or null: non-zero = the env's return moves to fin and restarts from +0.0 first */
};

/* a term's s for a VEC or ROT_INV: the errors against the target through the deadband, then the norm and the root */
WV_DEVICE double reward_norm(const RewardIO &io, const RewardTerm &T, size_t env) {
    using namespace wv;
    const bool rot = T.kind == REW_ROT_INV;
    double q[4] = {0, 0, 0, 0}, v[3] = {0, 0, 0};
    if (rot) {
        for (int k = 0; k < 4; ++k) q[k] = obs_load(io.src[T.qfield], env, T.qindex + k);
        for (int k = 0; k < 3; ++k) v[k] = T.field == REW_CONST ? T.vec[k] : obs_load(io.src[T.field], env, T.index + k);
    }
    const int count = rot ? 3 : T.count;
    double s = 0.0;
    for (int j = 0; j < count; ++j) {
        const double x = rot ? obs_rot_inv(q, v, j) : obs_load(io.src[T.field], env, T.index + j);
        double e = sub_rn(x, T.tfield == REW_CONST ? T.target : obs_load(io.src[T.tfield], env, T.tindex + j));
        if (T.dead > 0.0) { const double m = sub_rn(fabs(e), T.dead); e = m < 0.0 ? 0.0 : m; }   /* (a NaN passes) */
        if (T.norm == REW_SUMSQ) s = add_rn(s, mul_rn(e, e));
        else if (T.norm == REW_SUMABS) s = add_rn(s, fabs(e));
        else { const double m = fabs(e); if (m > s) s = m; }
    }
    return T.root != 0 ? sqrt_rn(s) : s;
}

/* a QUAT term's s: 1 - d d with d the dot of the four values as stored with the target's four */
WV_DEVICE double reward_quat(const RewardIO &io, const RewardTerm &T, size_t env) {
    using namespace wv;
    double d = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double p = mul_rn(obs_load(io.src[T.field], env, T.index + k), T.tfield == REW_CONST ? T.vec[k] : obs_load(io.src[T.tfield], env, T.tindex + k));
        d = k == 0 ? p : add_rn(d, p);
    }
    return sub_rn(1.0, mul_rn(d, d));
}

/* env env0 + i of the range: the terms in order, the clip, the stores and the return */
WV_DEVICE void reward_env(const RewardIO &io, int i) {
    using namespace wv;
    const size_t env = (size_t)io.env0 + (size_t)i;
    double r = 0.0;
    for (int t = 0; t < io.nterms; ++t) {
        const RewardTerm &T = io.terms[t];
        const double s = T.kind == REW_QUAT ? reward_quat(io, T, env) : reward_norm(io, T, env);
        double v = s;
        if (T.shape == REW_EXP) v = reward_expn(mul_rn(T.k, s));
        else if (T.shape == REW_RATIONAL) v = div_rn(1.0, add_rn(1.0, mul_rn(T.k, s)));
        double c = mul_rn(T.weight, v);
        if (T.gfield != REW_NONE) c = mul_rn(c, obs_load(io.src[T.gfield], env, T.gindex));
        if (io.trows) {
            const size_t at = env * (size_t)io.sterm + (size_t)t;
            if (io.f32) ((float *)io.trows)[at] = (float)c; else ((double *)io.trows)[at] = c;
        }
        r = add_rn(r, c);
    }
    r = clampd(r, io.lo, io.hi);
    if (io.f32) ((float *)io.rew)[env * (size_t)io.srew] = (float)r; else ((double *)io.rew)[env * (size_t)io.srew] = r;
    double ret = io.ret[env];
    if (io.reset && io.reset[i] != 0) { io.fin[env] = ret; ret = 0.0; }
    io.ret[env] = add_rn(ret, r);
}

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_reward_kernel(RewardIO io) {
    for (int i = wv::env_id() * WV_WAVE + wv::lane(); i < io.n; i += wv::grid_size() * WV_WAVE) reward_env(io, i);
}

}  // namespace ck
#endif
