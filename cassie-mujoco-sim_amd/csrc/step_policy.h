/*
 * step_policy.h -- the rules by which the launcher (phys_batch.hip) decides what a stepping launch looks like: its forms, its chunk
 * count, the grids of its list-walking passes, the form of a range's fast kernel, the cadence of the order kernel -- as functions of
 * plain values, each constant with the measurement it rests on -- and the table of env ranges the launcher keeps its per-range facts
 * in.  No HIP runtime calls: the launcher turns the answers into PhysIO fields and launches (step_plan.h: plan_step), the tests run
 * the rules on the CPU (tests/test_launch_policy.py, through the emulator library).  The emulator's own launches do NOT go through
 * these rules: it is handed its forms explicitly, so that a test can force every form at a handful of envs.
 */
#ifndef CASSIE_STEP_POLICY_H
#define CASSIE_STEP_POLICY_H

#include <vector>

#include "step_plan.h"

namespace ck {

/* ---- the forms of a launch ---- */

constexpr int SMALL_BATCH_NSUB = 4;  /* substeps per launch up to which a small batch skips the fast kernel + passes (three launches) for one instantiation alone */
constexpr int SMALL_BATCH = 512;     /* envs up to which that holds (half the chip's workgroup slots) */
/* (inplace_stay_rows: once in the 63-row code an env stays there until a substep needs at most FAST_ROWS - 4 rows again -- the
 * margin keeps an env that hovers about the fast code's capacity from changing codes every substep) */
constexpr int INPLACE_STAY_ROWS = FAST_ROWS - 4;

/* The forms of the launch of nsub substeps over n envs of a model of family fam (has_inplace: the family has a FORM_FAST_INPLACE
 * instantiation; maxefc: the model's row cap; ext: the read-out block is on; fast_rows, waves_per_env, waves_per_env_tray: the
 * batch's settings; inplace: what the launch's range has decided about the form of its two-wave fast kernel, next_inplace below;
 * prof: the batch's profile buffer is on, PhysIO::prof).
 * The fast forms are LEAN (step_plan.h: is_lean_form): they are chosen only where integrate && !ext -- every branch below that
 * answers one says so -- and with prof their _PROF forms take their place: the plain form whatever `inplace` says, since the stamps
 * are in the plain fast kernel alone and a profile is of the code it names.
 * sums: the launch accumulates the step-sums block (PhysIO::sums; stepping launches only).  The fast forms have a sibling with that
 * code in the two-wave form alone (FEAT_SUMS: phys_batch.hip's second table), so such a launch takes the PLAIN two-wave fast form +
 * the mid-walk pass whatever `inplace` says, as with prof -- a range whose envs keep leaving the fast tier (the stress workloads) then
 * pays the list-walking pass again, the 8 - 24 % the in-place form had gained it (profiles/round6/inplace_ab.txt) -- and where the batch
 * is set to one wave per env, or profiled at the same time, one full form alone, which holds every code. */
inline StepForms launch_forms(int fam, bool has_inplace, int maxefc, int integrate, bool ext, int n, int nsub, bool fast_rows,
                              int waves_per_env, int waves_per_env_tray, bool inplace, bool prof = false, bool sums = false) {
    StepForms forms = {FORM_ALONE, FORM_ALONE, false, INPLACE_STAY_ROWS};
    if (sums && integrate) {
        inplace = false;
        if (prof || (fam == TRAY ? waves_per_env_tray : waves_per_env) != 2) fast_rows = false;
    }
    if (fam == CASSIE || fam == CASSIE_HFIELD) {
        /* stepping launches go through the row-capped fast instantiation first; the 63-row pass behind it finishes the envs that met
         * a substep with more rows, and -- for a model with the wide caps (CM_FLAG_HFPRISM) -- the 127-row pass behind that one what
         * is left.  Forward / read-out passes take one instantiation alone, and so does a small batch stepping a few substeps per
         * launch (somebody's control loop around a handful of envs): one launch instead of two or three -- a launch costs what four
         * substeps' difference between the kernels saves */
        forms.wide = maxefc > CM_MAXEFC_NARROW;
        if (!fast_rows || !integrate || ext || (n <= SMALL_BATCH && nsub <= SMALL_BATCH_NSUB))
            /* (alone and a LARGE grid -- phys_batch_derive / forward passes of a whole batch, the fast kernel switched off -- with 63-row
             * caps: the one-wave form, whose 421 registers leave room for four envs per CU; the two-wave 512-register form halves that
             * and only pays where the chip is not full anyway, profiles/round6/alone_pass_ab.txt) */
            forms.first = forms.wide ? FORM_WIDE : n > SMALL_BATCH ? FORM_ALONE : FORM_ALONE_2W;
        else if (waves_per_env == 2) { forms.first = prof ? FORM_FAST_2W_PROF : inplace && has_inplace ? FORM_FAST_INPLACE : FORM_FAST_2W; forms.mid = FORM_MID_WALK_2W; }
        else forms.first = prof ? FORM_FAST_PROF : FORM_FAST;     /* (behind it the one-wave 63-row pass looks every env's record up: FORM_ALONE) */
    } else if (fam == TRAY) {
        /* the 40-dof model: a fast instantiation of 47 rows (the boxes resting on the tray take it to 32 .. 40 routinely) with the 63-row
         * one behind it walking the list, both in the two-wave form by default (waves_per_env_tray) -- or the 63-row one alone */
        const bool plain = integrate && !ext, two = plain && waves_per_env_tray == 2;
        if (plain && fast_rows) {
            forms.first = two ? (prof ? FORM_FAST_2W_PROF : FORM_FAST_2W) : (prof ? FORM_FAST_PROF : FORM_FAST);
            forms.mid = two ? FORM_MID_WALK_2W : FORM_MID_WALK;
        }
        else forms.first = two ? FORM_ALONE_2W : FORM_ALONE;
    }
    return forms;
}

/* What the launcher checks in front of every pass, whatever made the plan: a lean form does not hold the code for the read-out block,
 * a forward pass or the stage stamps -- launched with one of them it would silently do without -- and a profiled form not that for
 * the first two.  True: the pass must not be launched. */
inline bool lean_form_refuses(int form, bool ext, int integrate, bool prof) {
    if (is_lean_form(form)) return ext || !integrate || prof;
    if (is_prof_form(form)) return ext || !integrate;
    return false;
}

/* ... and the same check of a pass with the step-sums block in view (sums: PhysIO::sums is set; sums_inst: the pass's kernel comes from
 * the family's FEAT_SUMS table, phys_batch.hip).  A lean or profiled fast instantiation does not hold the accumulation code -- launched
 * with the block it would leave the zeroed rows as they are -- and a forward pass must neither zero nor add. */
inline bool step_sums_refuses(int form, bool ext, int integrate, bool prof, bool sums, bool sums_inst) {
    if (sums_inst ? (!is_lean_form(form) || ext || !integrate || prof) : lean_form_refuses(form, ext, integrate, prof)) return true;
    if (!sums) return sums_inst;        /* (a FEAT_SUMS instantiation is for accumulating launches alone) */
    if (!integrate) return true;
    return is_fast_form(form) && !sums_inst;
}

/* ---- the chunks of a launch ---- */

/* stepping launches of the fast instantiations in chunks (PhysIO::nchunk): chunks per env-launch, for launches of at least
 * CHUNK_MIN_ENVS envs (two jobs per workgroup slot: below that there is no queue whose end could be evened out) and chunks of at
 * least CHUNK_MIN_SUBSTEPS substeps */
/* Defaults by measurement (profiles/round4/chunks_ab.txt): a launch over the whole batch has nothing to fill the end of its queue
 * with: 4 chunks (+7 %); launches over env ranges (phys_batch_step_range: other ranges' launches fill in) gain nothing from more
 * than 2 in steady state, and as much as the whole-batch launch when they stand alone between two synchronisations. */
constexpr int DEFAULT_CHUNKS_WHOLE = 7 /* (round 6; 4 before: jobs of 7 substeps leave the shortest end of a queue, profiles/round6/one_stream_chunks.txt) */, DEFAULT_CHUNKS_RANGE = 2, CHUNK_MIN_ENVS = 2048, CHUNK_MIN_SUBSTEPS = 5;
/* (round 6: a range's launch of 15 .. 25 substeps -- a consumer that fences every few substeps, the driver's 20-step regions --
 * as three chunks instead of two: nothing fills the end of such a launch's queue, finer jobs shorten it, + 1.5 %; at 50
 * substeps between fences three cost 0.6 %, profiles/round6/chunks3_ab.txt) */
constexpr int SHORT_RANGE_NSUB = 25, SHORT_RANGE_CHUNKS = 3;

/* The chunks of the fast kernel's launch of nsub substeps over n envs of a batch of nenv (chunks, chunks_range: what the batch asks
 * for launches over the whole batch / over an env range; chunks_default: nobody has asked).  More than 1 only where the launch is
 * long enough; whether the stream places workgroups round the XCDs is the launcher's to ask, after this. */
inline int launch_chunks(int n, int nenv, int nsub, int chunks, int chunks_range, bool chunks_default) {
    /* (n % 8: workgroup w runs on XCD w % 8, so the chunks of an env -- workgroups n apart -- share an XCD and its L2) */
    if ((n == nenv ? chunks : chunks_range) <= 1 || n < CHUNK_MIN_ENVS || n % 8 != 0 || nsub < 2 * CHUNK_MIN_SUBSTEPS) return 1;
    const int range_chunks = chunks_default && nsub <= SHORT_RANGE_NSUB ? SHORT_RANGE_CHUNKS : chunks_range;
    const int most = nsub / CHUNK_MIN_SUBSTEPS, asked = n == nenv ? chunks : range_chunks;
    return asked < most ? asked : most;
}

/* ---- the grids of the passes that walk the hand-over lists ---- */

/* Twice what the range's last launch handed over (seen1, seen2: the range's words in host memory -- the launcher learns that a launch
 * late) plus 16, at most one workgroup per env; the 127-row pass behind that one (wide) likewise, plus 8.  (A floor of 256 workgroups
 * under both grids was measured: no gain on the prism workload, -0.6 % on config 2, profiles/round5.) */
inline StepGrids pass_grids(int n, int seen1, int seen2, bool wide) {
    if (!wide) seen2 = 0;
    const int seen12 = seen1 > seen2 ? seen1 : seen2; /* (the first pass is never smaller than the second: it feeds it) */
    const long want = 2L * (seen12 > 0 ? seen12 : 0) + 16, want2 = 2L * (seen2 > 0 ? seen2 : 0) + 8;
    return {(unsigned)n, (unsigned)(want < n ? want : n), (unsigned)(want2 < n ? want2 : n)};
}

/* ---- the form of a range's two-wave fast kernel ---- */

/* Which form of the two-wave fast kernel a range's launches take (phys_batch_set_inplace): mode 0 = the kernel + the list-walking pass
 * behind it, 1 = the kernel that finishes the substeps it cannot hold in place, 2 (default) = per range by what its recent launches
 * needed.  The in-place form costs the default workload 1.8 % (both codes share one register allocation) and gains 8 - 24 % where
 * envs leave the fast tier at all (profiles/round6/inplace_ab.txt): a range switches to it once a launch handed envs over
 * and back after INPLACE_QUIET reports in a row in which no env needed the wider code.  The range's first `seen` word is the signal in
 * both forms (the pass reports the list's length; in the in-place form the order kernel reports the kernel's count, or the run of
 * reports without one -- counted on the device, in stream order, because the launcher may run far ahead of it). */
constexpr int INPLACE_QUIET = 8;

/* was: the range's form so far; seen: its word in host memory: > 0 = env-launches the last reporting launch handed over (plain form:
 * the pass behind the kernel writes it) or finished in place (the order kernel does); -k = the last k reports of the in-place form had
 * none; auto_ok: the order kernel runs behind the range's launches (mode 2 needs it: it reports the in-place count) */
inline bool next_inplace(bool was, int seen, int mode, bool auto_ok) {
    if (mode != 2 || !auto_ok) return mode == 1;
    return was ? seen > -INPLACE_QUIET : seen > 0;
}

/* ---- the order kernel ---- */

/* the next launch's order from this one's per-env cost: after every long launch, now and then after short ones.  (Round 6: "long" is
 * more than 25 substeps, not 8 -- the sort is 20 - 25 us at the end of the launch's stream, 0.7 % of a fenced 20-substep launch, and the
 * order itself is worth nothing either way since launches go in chunks: profiles/round6/launch_order_ab.txt.) */
constexpr int ORDER_LONG_NSUB = 25, ORDER_EVERY = 16;

/* launches_since_sort: the range's launches since the order kernel last ran, this one included */
inline bool order_kernel_due(int nsub, int launches_since_sort) { return nsub > ORDER_LONG_NSUB || launches_since_sort >= ORDER_EVERY; }

/* ---- the env ranges of a batch ---- */

/* What the launcher knows about an env range [env0, env0 + n) that stepping launches went over -- a range is (env0, n), both:
 *   the launch-order array holds a permutation of the range's env ids (the order kernel sorts one launch's range at a time) and the
 *   identity outside every range: a launch may use the array only for a range that is exactly one of these, or that lies wholly in
 *   identity territory -- any other range would step envs outside itself and skip envs inside it;
 *   inplace: the form of the range's two-wave fast kernel (next_inplace), with which the meaning of the words indexed by env0 changes
 *   -- the first list's [count, ticket] pair and `seen` word are, in the in-place form, the in-place count and the run of quiet reports;
 *   launches_since_sort: order_kernel_due. */
struct LaunchRange { int env0, n; bool inplace; int launches_since_sort; };

/* The ranges are pairwise disjoint: a launch over a range that is none of them RETIRES every one it overlaps and starts a record of
 * its own in the plain form.  The caller undoes what a retired record stood for on the device, in stream order on the launch's stream
 * (ranges in flight on other streams must not overlap this one anyway -- their state would race). */
struct RangeTable {
    std::vector<LaunchRange> ranges;
    /* the record of [env0, env0 + n) (valid until the next claim); the records it retired are appended to `retired` */
    LaunchRange *claim(int env0, int n, std::vector<LaunchRange> &retired) {
        for (auto &r : ranges) if (r.env0 == env0 && r.n == n) return &r;
        for (size_t i = 0; i < ranges.size();) {
            const LaunchRange r = ranges[i];
            if (r.env0 < env0 + n && env0 < r.env0 + r.n) { retired.push_back(r); ranges.erase(ranges.begin() + (long)i); }
            else ++i;
        }
        ranges.push_back({env0, n, false, 0});
        return &ranges.back();
    }
};

}  // namespace ck
#endif
