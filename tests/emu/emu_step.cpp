/*
 * emu_step.cpp -- TEST-ONLY: the step kernel on the wave emulator (tests/emu/wave.h, emu_runtime.cpp).  The one translation unit that
 * instantiates ck::cassie_step_kernel: the bodies, their tables by form (step_plan.h), the family of a model (ck::pick_family) and the
 * one function that fills PhysIO from a call's argument block and runs ck::plan_step's passes.  The launcher's policy and range table
 * (step_policy.h) are exported for tests at the end; the emulator's own launches do not go through them.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_policy.h"
#include "emu_runtime.h"

static ck::PhysIO g_io;
static void body32s() { ck::cassie_step_kernel<32, ck::TopoCassie32>(g_io); }
static void body32s_fast() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::FAST_ROWS>(g_io); }
/* the two-wave forms (wave 1 runs the mass-matrix stage group beside wave 0's collision / velocity / row stages) */
static void body32s_2w() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::MID_ROWS, 2>(g_io); }
/* the full instantiation as the list-walking pass behind the fast kernel */
static void body32s_2w_walk() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::MID_ROWS, 2, true>(g_io); }
/* the 127-row instantiation (two wavefronts; the solve of a substep with more than 64 rows is spread over both): alone, and as the
 * pass that walks the list of envs the 63-row pass handed on */
static void body32s_wide() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::WIDE_ROWS, 2, false, 1>(g_io); }
static void body32s_wide_walk() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::WIDE_ROWS, 2, true, 1>(g_io); }
static void body32s_fast_2w() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::FAST_ROWS, 2>(g_io); }
/* ... with the 63-row code behind it in the same kernel (cassie_step_kernel's INROWS): substeps it cannot hold are finished in place */
static void body32s_fast_2w_inplace() { ck::cassie_step_kernel<32, ck::TopoCassie32, ck::FEAT_ALL, ck::FAST_ROWS, 2, false, 2, ck::MID_ROWS>(g_io); }
static void body40s() { ck::cassie_step_kernel<40, ck::TopoCassieTray38>(g_io); }
static void body40s_2w() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, ck::FEAT_WAVEPAIRS, ck::MID_ROWS, 2>(g_io); } /* (no height-field pairs) */
/* the 40-dof model's row-capped instantiation (47 rows, one wave per env: the Gram matrix through the staged tile's own LDS) and
 * the full one as the list-walking pass behind it (no height-field pairs) */
static void body40s_fast() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, ck::FEAT_WAVEPAIRS, ck::FAST_ROWS_TRAY>(g_io); }
static void body40s_walk() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, ck::FEAT_WAVEPAIRS, ck::MID_ROWS, 1, true>(g_io); }
static void body40s_2w_walk() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, ck::FEAT_WAVEPAIRS, ck::MID_ROWS, 2, true>(g_io); }
static void body32() { ck::cassie_step_kernel<32, ck::TopoRuntime>(g_io); }
static void body40() { ck::cassie_step_kernel<40, ck::TopoRuntime>(g_io); }
/* the bodies by form (step_plan.h) of the compile-time topologies and the run-time one: FEAT_ALL, except the 40-dof model's tiers
 * and its two-wave form alone (FEAT_WAVEPAIRS: no height-field pairs) */
struct EmuForm { void (*body)(); int nw; };
static const EmuForm CASSIE32_BODIES[ck::FORM_COUNT] = {
    {body32s, 1}, {body32s_2w, 2}, {body32s_wide, 2},                                  /* FORM_ALONE, FORM_ALONE_2W, FORM_WIDE */
    {body32s_fast, 1}, {body32s_fast_2w, 2}, {body32s_fast_2w_inplace, 2},             /* FORM_FAST, FORM_FAST_2W, FORM_FAST_INPLACE */
    {nullptr, 0}, {body32s_2w_walk, 2}, {body32s_wide_walk, 2},                        /* FORM_MID_WALK, FORM_MID_WALK_2W, FORM_WIDE_WALK */
};
static const EmuForm TRAY38_BODIES[ck::FORM_COUNT] = {
    {body40s, 1}, {body40s_2w, 2}, {nullptr, 0},
    {body40s_fast, 1}, {nullptr, 0}, {nullptr, 0},
    {body40s_walk, 1}, {body40s_2w_walk, 2}, {nullptr, 0},
};
static const EmuForm GENERIC32_BODIES[ck::FORM_COUNT] = {{body32, 1}}, GENERIC40_BODIES[ck::FORM_COUNT] = {{body40, 1}};
/* ... by family (ck::pick_family): the emulator's set of bodies is smaller than the device's, one collision code serves a tree */
static const EmuForm *const FAMILY_BODIES[ck::FAMILY_COUNT] = {
    CASSIE32_BODIES, CASSIE32_BODIES, CASSIE32_BODIES, TRAY38_BODIES, TRAY38_BODIES, GENERIC32_BODIES, GENERIC40_BODIES,
};

/* the launch's PhysIO from the argument block (the hand-over and chunk fields are run_step's) */
static ck::PhysIO phys_io(const emu_step_args &a, const cm_model_t *model, cm_ext_t *ext) {
    ck::PhysIO io;
    memset(&io, 0, sizeof io);
    io.models = model; io.model_stride = 0; io.envparams = a.envparams;
    io.nenv = a.nenv; io.nsub = a.nsub; io.integrate = a.integrate;
    io.sq = model->nq; io.sqv = model->nv; io.sv = model->nv; io.su = model->nu; io.ssd = model->nsensordata; io.sb = model->nbody;
    io.qpos = a.qpos; io.qvel = a.qvel; io.qacc_warmstart = a.qacc_warmstart; io.time = a.time;
    io.ctrl = (double *)a.ctrl; io.qfrc_applied = a.qfrc_applied; io.xfrc_applied = a.xfrc_applied;
    io.qacc = a.qacc; io.sensordata = a.sensordata; io.actuator_velocity = a.actuator_velocity;
    io.warn = a.warn; io.info = a.info; io.xpos_out = a.xpos; io.xquat_out = a.xquat;
    io.hfield = a.hfield; io.hfield_stride = a.hfield_stride; io.hfield_index = a.hfield_index; io.hfield_nterrain = a.nterrain;
    io.pd_ptarget = a.pd_ptarget; io.pd_kp = a.pd_kp; io.pd_kd = a.pd_kd;
    io.drive_mode = a.drive_mode; io.drive_state = a.drive_state; io.drive_cmd = a.drive_cmd; io.meas = a.meas;
    io.pd_dtarget = a.pd_dtarget; io.pd_torque = a.pd_torque;
    io.ext = ext;
    return io;
}

int emu::run_step(const emu_step_args &a, emu_step_result &r, cm_ext_t *ext) {
    const emu_settings &set = a.settings;
    const int nenv = a.nenv, nsub = a.nsub, resume_grid = set.resume_grid > 0 ? set.resume_grid : 1;
    /* (tests edit compiled models field by field: the top-level arrays are the authority, as in phys_batch_create / _set_model) */
    static cm_model_t synced;
    synced = *a.model; cm_model_sync_params(&synced);
    const cm_model_t *model = &synced;
    ck::PhysIO io = phys_io(a, model, ext);
    const ck::StepFamily fam = ck::pick_family(*model, !ext && set.force_runtime_topology);
    const bool cassie32 = fam == ck::CASSIE || fam == ck::CASSIE_HFIELD || fam == ck::CASSIE_ALL, tray38 = fam == ck::TRAY;
    const EmuForm *bodies = FAMILY_BODIES[fam];
    /* the forms, chosen by this call's settings alone (NOT by the launcher's policy, step_policy.h: a test must be able to force every
     * form at a handful of envs): the row-capped fast instantiation for every env, then the passes behind it -- a list-walking one as
     * ONE small grid (here: resume_grid workgroups) -- or one instantiation alone */
    ck::StepForms forms = {ck::FORM_ALONE, ck::FORM_ALONE, false, set.inplace_stay_rows};
    std::vector<int> progress, list, list2, chunk_flag;
    int count[2] = {0, 0}, count2[2] = {0, 0};
    volatile int seen = -1, seen2 = -1, chunk_fault = 0;
    ck::HandoverLists hl = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (ext) forms.first = cassie32 && set.two_waves ? ck::FORM_ALONE_2W : ck::FORM_ALONE;
    else if ((cassie32 || tray38) && set.fast_rows && a.integrate) {
        progress.assign((size_t)nenv, 0); list.assign((size_t)nenv, 0); list2.assign((size_t)nenv, 0); chunk_flag.assign((size_t)nenv, 0);
        hl = {list.data(), count, &seen, list2.data(), count2, &seen2};
        if (tray38) forms = {ck::FORM_FAST, set.two_waves ? ck::FORM_MID_WALK_2W : ck::FORM_MID_WALK, false, set.inplace_stay_rows};
        else forms = {!set.two_waves ? ck::FORM_FAST : set.inplace ? ck::FORM_FAST_INPLACE : ck::FORM_FAST_2W, set.two_waves ? ck::FORM_MID_WALK_2W : ck::FORM_ALONE,
                      model->maxefc > ck::MID_ROWS, set.inplace_stay_rows};
        io.progress = progress.data();
        io.nchunk = (set.chunks > 1 && nsub >= 2) ? set.chunks : 1;
        /* (the chunk words live for this call and start cleared: every call is launch 1 of its own words) */
        io.chunk_seq = 1; io.chunk_flag = chunk_flag.data(); io.chunk_fault = &chunk_fault;
    } else if (cassie32) forms.first = model->maxefc > ck::MID_ROWS ? ck::FORM_WIDE : set.two_waves ? ck::FORM_ALONE_2W : ck::FORM_ALONE;
    else if (tray38 && set.two_waves) forms.first = ck::FORM_ALONE_2W;
    const ck::StepPlan plan = ck::plan_step(io, forms, hl, {(unsigned)nenv, (unsigned)resume_grid, (unsigned)(resume_grid > 1 ? resume_grid - 1 : 1)});
    r.fast_bails = r.wide_envs = r.chunk_fault = 0;
    emu::with_settings hooks(set);
    for (int i = 0; i < plan.n; ++i) {
        const ck::StepPass &p = plan.pass[i];
        const EmuForm &f = bodies[p.form];
        if (!f.body) { fprintf(stderr, "emu: no instantiation of form %d\n", p.form); abort(); }
        g_io = p.io;
        const int handed = p.io.handover_list ? p.io.handover_count[0] : 0;
        if (p.form == ck::FORM_WIDE_WALK) r.wide_envs += handed;
        emu::run_grid(f.body, (int)p.grid, f.nw);
        if (ck::is_fast_form(p.form)) for (int e = 0; e < nenv; ++e) if (progress[e] < nsub) ++r.fast_bails;
        /* a pass that walks a list leaves it empty for the next launch and reports its length */
        if (p.io.handover_list && (p.io.handover_count[0] != 0 || p.io.handover_count[1] != 0 || *p.io.handover_seen != handed)) {
            fprintf(stderr, "emu: the pass of form %d left count %d ticket %d seen %d (handed %d)\n", p.form, p.io.handover_count[0], p.io.handover_count[1], (int)*p.io.handover_seen, handed);
            abort();
        }
    }
    r.chunk_fault = chunk_fault;
    return 0;
}

extern "C" int emu_phys_run(const emu_step_args *args, emu_step_result *result) { return emu::run_step(*args, *result); }
/* ck::pick_family (step_plan.h), for tests */
extern "C" int emu_pick_family(const cm_model_t *model, int generic_only) { return ck::pick_family(*model, generic_only != 0); }
/* the launcher's policy (step_policy.h), for tests: forms -> {first, mid, wide, stay_rows}, grids -> {envs, mid, wide} */
extern "C" void emu_launch_forms(int fam, int has_inplace, int maxefc, int integrate, int ext, int n, int nsub, int fast_rows, int waves_per_env,
                                 int waves_per_env_tray, int inplace, int *out) {
    const ck::StepForms f = ck::launch_forms(fam, has_inplace != 0, maxefc, integrate, ext != 0, n, nsub, fast_rows != 0, waves_per_env, waves_per_env_tray, inplace != 0);
    out[0] = f.first; out[1] = f.mid; out[2] = f.wide ? 1 : 0; out[3] = f.stay_rows;
}
extern "C" int emu_launch_chunks(int n, int nenv, int nsub, int chunks, int chunks_range, int chunks_default) {
    return ck::launch_chunks(n, nenv, nsub, chunks, chunks_range, chunks_default != 0);
}
extern "C" void emu_pass_grids(int n, int seen1, int seen2, int wide, unsigned *out) {
    const ck::StepGrids g = ck::pass_grids(n, seen1, seen2, wide != 0);
    out[0] = g.envs; out[1] = g.mid; out[2] = g.wide;
}
extern "C" int emu_next_inplace(int was, int seen, int mode, int auto_ok) { return ck::next_inplace(was != 0, seen, mode, auto_ok != 0) ? 1 : 0; }
extern "C" int emu_order_kernel_due(int nsub, int launches_since_sort) { return ck::order_kernel_due(nsub, launches_since_sort) ? 1 : 0; }
extern "C" void emu_policy_defaults(int *out) { out[0] = ck::DEFAULT_CHUNKS_WHOLE; out[1] = ck::DEFAULT_CHUNKS_RANGE; }
/* ck::RangeTable::claim on the caller's table: records [*nrec][4] = {env0, n, inplace, launches_since_sort} (room for one more), updated
 * in place; retired [as many as there were records][4]; -> the index of the claimed record */
extern "C" int emu_ranges_claim(int *records, int *nrec, int env0, int n, int *retired, int *nretired) {
    ck::RangeTable t;
    for (int i = 0; i < *nrec; ++i) t.ranges.push_back({records[4 * i], records[4 * i + 1], records[4 * i + 2] != 0, records[4 * i + 3]});
    std::vector<ck::LaunchRange> gone;
    const ck::LaunchRange *r = t.claim(env0, n, gone);
    const auto put = [](int *to, const ck::LaunchRange &g) { to[0] = g.env0; to[1] = g.n; to[2] = g.inplace ? 1 : 0; to[3] = g.launches_since_sort; };
    for (size_t i = 0; i < t.ranges.size(); ++i) put(records + 4 * i, t.ranges[i]);
    for (size_t i = 0; i < gone.size(); ++i) put(retired + 4 * i, gone[i]);
    *nrec = (int)t.ranges.size(); *nretired = (int)gone.size();
    return (int)(r - t.ranges.data());
}
