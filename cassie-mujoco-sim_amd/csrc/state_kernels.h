/*
 * state_kernels.h -- the kernels that save full env states to a bank of rows and restore envs from it (phys_batch_state_save /
 * phys_batch_state_restore, include/cassie_phys.h: "a bank of full states"): cassie_state_save_kernel, cassie_state_restore_kernel.
 * Included by phys_batch.hip (which launches them) and by the CPU wave emulator; the row's layout, the launch record, the grid and the
 * checks are small_launch.h's (ck::state_layout, ck::make_state_io: no field of StateIO is assigned anywhere else).
 *
 * A row is a sequence of SECTIONS of 8-byte words, each starting on a 16-byte boundary (an even word); a section is one per-env array of
 * the batch -- its words are the array's bytes as stored, so a restore puts back exactly what a save read.  The kernels know nothing of
 * what a section means: StateIO lists, per section, where env 0's entry lies, the bytes between two envs' entries, the section's place in
 * the row and its length.  One wave takes an env at a time and walks the range (as cassie_episode_kernel does); within a section lane l
 * moves words l, l + 64, ...: contiguous 8-byte accesses on both sides (the env side may be a strided column of a caller's observation
 * block, of which only 8-byte alignment is known).  Vector loads and stores only; an env's wave touches that env's entries and its
 * slot's row alone.
 */
#ifndef CASSIE_STATE_KERNELS_H
#define CASSIE_STATE_KERNELS_H

#include <wave.h> /* csrc/wave.h in the product build; tests/emu/wave.h under the CPU wave emulator */

#include "cm_model.h"

namespace ck {

/* a slot outside the bank was named for the env: nothing was copied (phys_batch_state_save / _restore; sticky like the other bits) */
constexpr int WARN_STATE_SLOT = 256;
/* sections a row may have (CORE 13, COMMANDS 8, EPISODE 3, PARAMS 1), and the workgroups that walk a range: more than the episode
 * kernel's few, since every env of the range moves a few KB -- a first choice, by arithmetic: 256 waves of 64 lanes keep 128 KB in
 * flight per section pass (tools/state_rate.py measures the call in the loop it is meant for) */
constexpr int STATE_MAXSECT = 28, STATE_GRID = 256;
/* what a section's words are on the env side: 8-byte words (doubles, or a struct whose size is a multiple of 8), or ONE 32-bit word
 * per env (a warning word, a counter, a terrain index), which the row holds zero-extended to 8 bytes */
enum { STATE_WORDS = 0, STATE_INT32 = 1 };
struct StateSect {
    void *env;              /* env 0's entry; null: the batch does not have the array -- zeros at a save, skipped at a restore */
    unsigned long stride;   /* bytes between the entries of consecutive envs */
    int off, count;         /* place in the row and length, in 8-byte words (off even; the padding word of an odd count follows) */
    int kind, pad;
};
struct StateIO {
    int env0, n, nslots, row_dim;       /* row_dim: 8-byte words between rows */
    unsigned long long *bank;           /* [nslots][row_dim] */
    const int *slots;                   /* [n] or null: env env0 + i has slot env0 + i */
    int *warn;                          /* [nenv] the sticky warning words */
    int nsect, pad;
    StateSect sect[STATE_MAXSECT];
};

template <bool RESTORE>
WV_DEVICE void state_walk(const StateIO &io) {
    typedef unsigned long long word;
    const int lane = wv::lane();
    for (int i = wv::env_id(); i < io.n; i += wv::grid_size()) {
        const size_t env = (size_t)io.env0 + (size_t)i;
        const int slot = io.slots ? io.slots[i] : (int)env;
        if (slot < 0) continue;
        if (slot >= io.nslots) {
            if (lane == 0) io.warn[env] |= WARN_STATE_SLOT;
            continue;
        }
        word *row = io.bank + (size_t)slot * (size_t)io.row_dim;
        for (int s = 0; s < io.nsect; ++s) {
            const StateSect S = io.sect[s];
            word *dst = row + S.off;
            if (S.kind == STATE_INT32) {
                int *p = S.env ? (int *)((char *)S.env + env * S.stride) : nullptr;
                if constexpr (RESTORE) {
                    if (p && lane == 0) *p = (int)(unsigned)dst[0];
                } else if (lane < 2) dst[lane] = p && lane == 0 ? (word)(unsigned)*p : 0ull;
                continue;
            }
            word *src = S.env ? (word *)((char *)S.env + env * S.stride) : nullptr;
            if constexpr (RESTORE) {
                if (src) for (int k = lane; k < S.count; k += WV_WAVE) src[k] = dst[k];
            } else {
                const int padded = (S.count + 1) & ~1;   /* (the padding word is written too: a saved row is the same bytes every time) */
                for (int k = lane; k < padded; k += WV_WAVE) dst[k] = src && k < S.count ? src[k] : 0ull;
            }
        }
    }
}
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_state_save_kernel(StateIO io) { state_walk<false>(io); }
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_state_restore_kernel(StateIO io) { state_walk<true>(io); }

}  // namespace ck
#endif
