/*
 * step_plan.h -- the passes of a stepping launch and what each one is handed (PhysIO's hand-over fields), as one plan that the
 * launcher (phys_batch.hip) and the CPU wave emulator (tests/emu) both run.  No HIP runtime calls: which kernel a form is, and how
 * it is launched, is the caller's (phys_batch.hip: one table of instantiations per model family).
 *
 * The tiers (round 5): the row-capped FAST instantiation (31 rows; 47 for the 40-dof model) steps every env until a substep needs
 * more rows or contacts than it holds; the MID pass (63 rows, 16 contacts) finishes the envs it handed over -- walking the list the
 * fast kernel appended them to, or (one wave per env, Cassie dof tree) one workgroup per env that looks its env's record up; the
 * WIDE pass (127 rows, 32 contacts: models whose caps are 127 rows, cm_model_t::maxefc) walks the list of envs the mid one handed
 * on.  Round 6: the fast kernel in its IN-PLACE form finishes the substeps it cannot hold with the 63-row code inside its own
 * workgroup -- no first list, no mid pass; with the wide caps the inner 63-row call hands on to the second list.  A launch without
 * a fast pass is ONE instantiation stepping every env alone.
 */
#ifndef CASSIE_STEP_PLAN_H
#define CASSIE_STEP_PLAN_H

#include "physics_kernel.h"

namespace ck {

/* the forms of the step kernel, by role; a model family has an instantiation for some of them */
enum StepForm {
    FORM_ALONE,         /* 63 rows, one wave per env: every env alone -- or, behind the one-wave fast kernel, the mid pass that looks records up */
    FORM_ALONE_2W,      /* 63 rows, two waves per env, alone */
    FORM_WIDE,          /* 127 rows, alone */
    FORM_FAST,          /* the row-capped fast instantiation, one wave per env */
    FORM_FAST_2W,       /* ... two waves per env */
    FORM_FAST_INPLACE,  /* ... two waves per env, with the 63-row code behind it in the same kernel */
    FORM_MID_WALK,      /* 63 rows walking the first list, one wave per env */
    FORM_MID_WALK_2W,   /* ... two waves per env */
    FORM_WIDE_WALK,     /* 127 rows walking the second list */
    FORM_FAST_PROF,     /* FORM_FAST with the stage stamps (FEAT_PROF): what a profiled stepping launch takes */
    FORM_FAST_2W_PROF,  /* FORM_FAST_2W likewise */
    FORM_COUNT
};

/* the model families: which instantiations step a model, by its dof tree and the collision code its pair list needs */
enum StepFamily {
    CASSIE,             /* the Cassie dof tree, neither height-field nor whole-wave (plane-box / box-box) pairs: all three tiers */
    CASSIE_HFIELD,      /* ... with height-field pairs: all three tiers */
    CASSIE_ALL,         /* ... with whole-wave pairs: one instantiation alone */
    TRAY,               /* the 40-dof tray model's tree without height-field pairs: fast (47 rows) and 63 rows */
    TRAY_HFIELD,        /* ... with height-field pairs: one instantiation alone */
    GENERIC32,          /* any other model: the dof tree read from the model at run time, up to 32 dofs */
    GENERIC40,          /* ... more than 32 */
    FAMILY_COUNT
};

/* the compile-time-topology instantiations are used only when the model's dof tree is exactly theirs (kin_simple, and a body tree no
 * deeper than theirs: the record-based local transforms and the round count of the recursion in their kinematics stage) */
template <class TOPO>
inline bool topo_matches(const cm_model_t &m) {
    if (m.nv != TOPO::nv || !m.kin_simple || m.maxdepth > TOPO::body_levels) return false;
    for (int k = 0; k < TOPO::nv; ++k) if (m.dof_ancmask[k] != TOPO::table[k]) return false;
    return true;
}

/* ... and the collision code of an instantiation is what the model's pair list needs (FEAT_*); generic_only: the run-time topology
 * whatever the tree (phys_batch's generic_kernel, the emulator's force_runtime_topology) */
inline StepFamily pick_family(const cm_model_t &m, bool generic_only) {
    const bool hf = m.nhfpair > 0 || m.hfield_geom >= 0, wp = m.npair > m.npair_simple;
    if (!generic_only && topo_matches<TopoCassie32>(m)) return wp ? CASSIE_ALL : hf ? CASSIE_HFIELD : CASSIE;
    if (!generic_only && topo_matches<TopoCassieTray38>(m)) return hf ? TRAY_HFIELD : TRAY;
    return m.nv > 32 ? GENERIC40 : GENERIC32;
}

/* the forms a launch takes: `first` is one of the FORM_FAST* forms (the tiers behind it follow) or the form that steps every env alone */
struct StepForms {
    int first;
    int mid;            /* behind FORM_FAST / FORM_FAST_2W (and their _PROF forms): FORM_MID_WALK(_2W), or FORM_ALONE (the lookup pass) */
    bool wide;          /* the model's caps are 127 rows: a FORM_WIDE_WALK pass walks the second list */
    int stay_rows;      /* FORM_FAST_INPLACE: PhysIO::inplace_stay_rows */
};

/* per env range: the two lists and their [count, ticket] pairs, the words the passes report into (list2 may be null without the wide caps) */
struct HandoverLists {
    int *list1, *count1; volatile int *seen1;
    int *list2, *count2; volatile int *seen2;
};

/* the grids: envs of the launch, and the workgroups of the passes that walk the first / the second list */
struct StepGrids { unsigned envs, mid, wide; };

struct StepPass { int form; unsigned grid; PhysIO io; };
struct StepPlan { int n; StepPass pass[3]; };

/* The LEAN forms: instantiated with neither FEAT_READOUT nor FEAT_PROF (pk_stages.h), so the read-out stores, the forward-mode exits
 * and the stage stamps are not in their code at all.  Only stepping launches without the read-out block and without the profile
 * buffer may take them (step_policy.h: launch_forms never answers otherwise, lean_form_refuses is the launcher's last check). */
inline bool is_lean_form(int form) { return form == FORM_FAST || form == FORM_FAST_2W || form == FORM_FAST_INPLACE; }
/* ... and the same code with the stamps (without FEAT_READOUT all the same: stepping launches, no read-out block) */
inline bool is_prof_form(int form) { return form == FORM_FAST_PROF || form == FORM_FAST_2W_PROF; }
inline bool is_fast_form(int form) { return is_lean_form(form) || is_prof_form(form); }

/* base: the launch's PhysIO with progress (for a fast first form) and the chunk fields set; the plan clears what the passes do not use */
inline StepPlan plan_step(const PhysIO &base, const StepForms &f, const HandoverLists &hl, const StepGrids &g) {
    StepPlan p;
    p.n = 0;
    PhysIO io = base;
    io.resume = 0;
    io.handover_list = nullptr; io.handover_count = nullptr; io.handover_seen = nullptr;
    io.handover_out_list = nullptr; io.handover_out_count = nullptr;
    if (!is_fast_form(f.first)) {
        io.progress = nullptr; io.has_next = 0; io.nchunk = 1;
        p.pass[p.n++] = {f.first, g.envs, io};
        return p;
    }
    /* the fast kernel: every env of the launch, in chunks perhaps (PhysIO::nchunk: workgroups [k envs, (k + 1) envs) are chunk k) */
    const unsigned fast_grid = g.envs * (unsigned)(io.nchunk > 1 ? io.nchunk : 1);
    io.has_next = 1;
    if (f.first == FORM_FAST_INPLACE) {
        io.inplace_count = hl.count1;       /* (the first list's count word is free in this form: it counts the env-launches that needed the wider code) */
        io.inplace_stay_rows = f.stay_rows;
        io.inplace_has_next = f.wide ? 1 : 0;
        io.inplace_out_list = f.wide ? hl.list2 : nullptr; io.inplace_out_count = f.wide ? hl.count2 : nullptr;
        p.pass[p.n++] = {f.first, fast_grid, io};
    } else {
        const bool walk1 = f.mid != FORM_ALONE;   /* (the lookup pass needs no list) */
        io.handover_out_list = walk1 ? hl.list1 : nullptr; io.handover_out_count = walk1 ? hl.count1 : nullptr;
        p.pass[p.n++] = {f.first, fast_grid, io};
        /* the 63-row pass: with the wide caps it hands on to the second list, otherwise 63 rows are the model's cap and it is the last */
        io.resume = 1; io.nchunk = 1; io.has_next = f.wide ? 1 : 0;
        io.handover_out_list = f.wide ? hl.list2 : nullptr; io.handover_out_count = f.wide ? hl.count2 : nullptr;
        if (walk1) { io.handover_list = hl.list1; io.handover_count = hl.count1; io.handover_seen = hl.seen1; }
        p.pass[p.n++] = {f.mid, walk1 ? g.mid : g.envs, io};
    }
    if (f.wide) {
        /* the 127-row pass: walks the second list */
        io.resume = 1; io.nchunk = 1; io.has_next = 0;
        io.handover_out_list = nullptr; io.handover_out_count = nullptr;
        io.handover_list = hl.list2; io.handover_count = hl.count2; io.handover_seen = hl.seen2;
        p.pass[p.n++] = {FORM_WIDE_WALK, g.wide, io};
    }
    return p;
}

}  // namespace ck
#endif
