/*
 * emu_lean.cpp -- TEST-ONLY: the LEAN fast forms of the step kernel (step_plan.h: is_lean_form; cassie_step_kernel's SERVE = FEAT_LEAN)
 * and their profiled forms (SERVE = FEAT_PROF) on the wave emulator, given to it explicitly like emu_step.cpp's bodies -- whose fast
 * bodies carry both bits, as every instantiation that does not name SERVE does.  A stepping launch here is the lean (or profiled) fast
 * kernel and the passes behind it, by ck::plan_step as in emu::run_step, with the launcher's last check (ck::lean_form_refuses) in front
 * of every pass.  Also: the exports by which tests run the launcher's rules about these forms (step_policy.h) on the CPU.
 */
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_policy.h"
#include "emu_runtime.h"

static ck::PhysIO g_io;
using ck::FEAT_ALL; using ck::FEAT_WAVEPAIRS; using ck::FEAT_LEAN; using ck::FEAT_PROF; using ck::FAST_ROWS; using ck::FAST_ROWS_TRAY; using ck::MID_ROWS;
/* the lean fast forms and their profiled siblings ... */
static void lean32_fast() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, FAST_ROWS, 1, false, 1, 0, FEAT_LEAN>(g_io); }
static void lean32_fast_2w() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, FAST_ROWS, 2, false, 2, 0, FEAT_LEAN>(g_io); }
static void lean32_fast_2w_inplace() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, FAST_ROWS, 2, false, 2, MID_ROWS, FEAT_LEAN>(g_io); }
static void prof32_fast() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, FAST_ROWS, 1, false, 1, 0, FEAT_PROF>(g_io); }
static void prof32_fast_2w() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, FAST_ROWS, 2, false, 2, 0, FEAT_PROF>(g_io); }
static void lean40_fast() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 1, false, 1, 0, FEAT_LEAN>(g_io); }
static void prof40_fast() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 1, false, 1, 0, FEAT_PROF>(g_io); }
/* ... and the 63-row passes behind them (both bits: the instantiations of emu_step.cpp) */
static void full32() { ck::cassie_step_kernel<32, ck::TopoCassie32>(g_io); }
static void full32_2w_walk() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, MID_ROWS, 2, true>(g_io); }
static void full40_walk() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 1, true>(g_io); }
static void full40_2w_walk() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 2, true>(g_io); }
struct LeanForm { void (*body)(); int nw; };
static const LeanForm CASSIE32_LEAN[ck::FORM_COUNT] = {
    {full32, 1}, {nullptr, 0}, {nullptr, 0},                                            /* FORM_ALONE (the lookup pass), -, - */
    {lean32_fast, 1}, {lean32_fast_2w, 2}, {lean32_fast_2w_inplace, 2},                 /* FORM_FAST, FORM_FAST_2W, FORM_FAST_INPLACE */
    {nullptr, 0}, {full32_2w_walk, 2}, {nullptr, 0},                                    /* -, FORM_MID_WALK_2W, - */
    {prof32_fast, 1}, {prof32_fast_2w, 2},                                              /* FORM_FAST_PROF, FORM_FAST_2W_PROF */
};
static const LeanForm TRAY38_LEAN[ck::FORM_COUNT] = {
    {nullptr, 0}, {nullptr, 0}, {nullptr, 0},
    {lean40_fast, 1}, {nullptr, 0}, {nullptr, 0},
    {full40_walk, 1}, {full40_2w_walk, 2}, {nullptr, 0},
    {prof40_fast, 1}, {nullptr, 0},
};

/* A stepping launch of args (settings: two_waves, inplace, inplace_stay_rows, chunks, resume_grid and the scheduler's) through the lean
 * fast form, or with prof [nenv][NSTAMP] through its profiled form (the plain one whatever `inplace` says, as the launcher's policy has
 * it; the emulator's clocks read 0: a stamped slot is a cleared slot).  Models with the 63-row caps and one of the two compile-time
 * trees; -1 where that does not hold or a pass is refused. */
extern "C" int emu_phys_run_lean(const emu_step_args *args, emu_step_result *result, long long *prof) {
    const emu_step_args &a = *args;
    const emu_settings &set = a.settings;
    const int nenv = a.nenv, nsub = a.nsub, resume_grid = set.resume_grid > 0 ? set.resume_grid : 1;
    static cm_model_t synced;
    synced = *a.model; cm_model_sync_params(&synced);
    const cm_model_t *model = &synced;
    const ck::StepFamily fam = ck::pick_family(*model, false);
    const bool cassie32 = fam == ck::CASSIE || fam == ck::CASSIE_HFIELD || fam == ck::CASSIE_ALL, tray38 = fam == ck::TRAY;
    if (!(cassie32 || tray38) || !a.integrate || model->maxefc > ck::MID_ROWS) return -1;
    const LeanForm *bodies = cassie32 ? CASSIE32_LEAN : TRAY38_LEAN;
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
    io.prof = prof;
    std::vector<int> progress((size_t)nenv, 0), list((size_t)nenv, 0), list2((size_t)nenv, 0), chunk_flag((size_t)nenv, 0);
    int count[2] = {0, 0}, count2[2] = {0, 0};
    volatile int seen = -1, seen2 = -1, chunk_fault = 0;
    ck::HandoverLists hl = {list.data(), count, &seen, list2.data(), count2, &seen2};
    ck::StepForms forms;
    if (tray38) forms = {prof ? ck::FORM_FAST_PROF : ck::FORM_FAST, set.two_waves ? ck::FORM_MID_WALK_2W : ck::FORM_MID_WALK, false, set.inplace_stay_rows};
    else if (!set.two_waves) forms = {prof ? ck::FORM_FAST_PROF : ck::FORM_FAST, ck::FORM_ALONE, false, set.inplace_stay_rows};
    else forms = {prof ? ck::FORM_FAST_2W_PROF : set.inplace ? ck::FORM_FAST_INPLACE : ck::FORM_FAST_2W, ck::FORM_MID_WALK_2W, false, set.inplace_stay_rows};
    io.progress = progress.data();
    io.nchunk = (set.chunks > 1 && nsub >= 2) ? set.chunks : 1;
    io.chunk_seq = 1; io.chunk_flag = chunk_flag.data(); io.chunk_fault = &chunk_fault;
    const ck::StepPlan plan = ck::plan_step(io, forms, hl, {(unsigned)nenv, (unsigned)resume_grid, (unsigned)(resume_grid > 1 ? resume_grid - 1 : 1)});
    result->fast_bails = result->wide_envs = result->chunk_fault = 0;
    emu::with_settings hooks(set);
    for (int i = 0; i < plan.n; ++i) {
        const ck::StepPass &p = plan.pass[i];
        const LeanForm &f = bodies[p.form];
        if (!f.body) { fprintf(stderr, "emu (lean): no instantiation of form %d\n", p.form); abort(); }
        /* (the launcher's last check, step_policy.h: such a pass is an error, not a launch) */
        if (ck::lean_form_refuses(p.form, p.io.ext != nullptr, p.io.integrate, p.io.prof != nullptr)) return -1;
        g_io = p.io;
        const int handed = p.io.handover_list ? p.io.handover_count[0] : 0;
        emu::run_grid(f.body, (int)p.grid, f.nw);
        if (ck::is_fast_form(p.form)) for (int e = 0; e < nenv; ++e) if (progress[e] < nsub) ++result->fast_bails;
        if (p.io.handover_list && (p.io.handover_count[0] != 0 || p.io.handover_count[1] != 0 || *p.io.handover_seen != handed)) {
            fprintf(stderr, "emu (lean): the pass of form %d left count %d ticket %d seen %d (handed %d)\n", p.form, p.io.handover_count[0], p.io.handover_count[1], (int)*p.io.handover_seen, handed);
            abort();
        }
    }
    result->chunk_fault = chunk_fault;
    return 0;
}
extern "C" int emu_nstamp(void) { return ck::NSTAMP; }
extern "C" unsigned long emu_sizeof_ext(void) { return sizeof(cm_ext_t); }   /* (the read-out block, for tests that compare it as bytes) */
/* where the launch descriptor (the kernel's argument block) holds what the lean forms must not read: -> {ext, prof, integrate, cost, sizeof} */
extern "C" void emu_physio_offsets(unsigned long *out) {
    out[0] = offsetof(ck::PhysIO, ext); out[1] = offsetof(ck::PhysIO, prof); out[2] = offsetof(ck::PhysIO, integrate); out[3] = offsetof(ck::PhysIO, cost);
    out[4] = sizeof(ck::PhysIO);
}
/* ck::launch_forms with the profile buffer on or off -> {first, mid, wide, stay_rows}; the launcher's last check of a pass
 * (lean_form_refuses); form_kinds -> {FORM_COUNT, bit mask of the lean forms, bit mask of the profiled forms} */
extern "C" void emu_launch_forms_prof(int fam, int has_inplace, int maxefc, int integrate, int ext, int n, int nsub, int fast_rows, int waves_per_env,
                                      int waves_per_env_tray, int inplace, int prof, int *out) {
    const ck::StepForms f = ck::launch_forms(fam, has_inplace != 0, maxefc, integrate, ext != 0, n, nsub, fast_rows != 0, waves_per_env, waves_per_env_tray, inplace != 0, prof != 0);
    out[0] = f.first; out[1] = f.mid; out[2] = f.wide ? 1 : 0; out[3] = f.stay_rows;
}
extern "C" int emu_lean_form_refuses(int form, int ext, int integrate, int prof) { return ck::lean_form_refuses(form, ext != 0, integrate, prof != 0) ? 1 : 0; }
extern "C" void emu_form_kinds(int *out) {
    out[0] = ck::FORM_COUNT; out[1] = 0; out[2] = 0;
    for (int f = 0; f < ck::FORM_COUNT; ++f) { if (ck::is_lean_form(f)) out[1] |= 1 << f; if (ck::is_prof_form(f)) out[2] |= 1 << f; }
}
