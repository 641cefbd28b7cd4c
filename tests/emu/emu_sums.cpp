/*
 * emu_sums.cpp -- TEST-ONLY: stepping launches that accumulate the step-sums block (PhysIO::sums; cm_model.h CM_SUM_*) on the wave
 * emulator.  The fast kernel here is the FEAT_SUMS sibling of the two-wave fast form (the product's kernels_*_sums.hip), the passes
 * behind it and the forms that step every env alone are the full instantiations, which test the pointer at run time.  A launch is
 * ck::plan_step's passes as in emu::run_step, with the launcher's zeroing of the launch's rows in front and its last check
 * (ck::step_sums_refuses) in front of every pass.  The argument block is emu_step_args plus the block, a body_cfrc array and the
 * read-out block -- what the twin of a test (sums off, one substep per launch) is read through.  Also: the exports by which tests run
 * the launcher's rules about accumulating launches (step_policy.h) on the CPU.
 */
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "step_policy.h"
#include "emu_runtime.h"

extern "C" {
typedef struct {
    emu_step_args step;
    double *sums;           /* [nenv][CM_SUM_DIM], or null: the launch does not accumulate */
    double *body_cfrc;      /* [nenv][nbody][3] PhysIO::body_cfrc, or null */
    cm_ext_t *ext;          /* [nenv] PhysIO::ext, or null (with it: one full form alone, as the launcher has it) */
    int fast;               /* 0: one full form steps every env alone; 1: the fast kernel (settings: two_waves, chunks, resume_grid) + the passes behind it */
} emu_sums_args;
}

static ck::PhysIO g_io;
using ck::FEAT_ALL; using ck::FEAT_WAVEPAIRS; using ck::FEAT_READOUT; using ck::FEAT_SUMS; using ck::FAST_ROWS; using ck::FAST_ROWS_TRAY; using ck::MID_ROWS; using ck::WIDE_ROWS;
/* the fast forms' FEAT_SUMS siblings ... */
static void sums32_fast_2w() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, FAST_ROWS, 2, false, 2, 0, FEAT_SUMS>(g_io); }
static void sums40_fast_2w() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2, false, 2, 0, FEAT_READOUT | FEAT_SUMS>(g_io); }
/* ... and the full forms (both bits, hence the sums by the pointer: the instantiations of emu_step.cpp) */
static void full32() { ck::cassie_step_kernel<32, ck::TopoCassie32>(g_io); }
static void full32_2w() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, MID_ROWS, 2>(g_io); }
static void full32_wide() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, WIDE_ROWS, 2, false, 1>(g_io); }
static void full32_2w_walk() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, MID_ROWS, 2, true>(g_io); }
static void full32_wide_walk() { ck::cassie_step_kernel<32, ck::TopoCassie32, FEAT_ALL, WIDE_ROWS, 2, true, 1>(g_io); }
static void full40() { ck::cassie_step_kernel<40, ck::TopoCassieTray38>(g_io); }
static void full40_2w() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 2>(g_io); }
static void full40_2w_walk() { ck::cassie_step_kernel<40, ck::TopoCassieTray38, FEAT_WAVEPAIRS, MID_ROWS, 2, true>(g_io); }
struct SumsForm { void (*body)(); int nw; bool sums_inst; };
static const SumsForm CASSIE32_SUMS[ck::FORM_COUNT] = {
    {full32, 1, false}, {full32_2w, 2, false}, {full32_wide, 2, false},                 /* FORM_ALONE, FORM_ALONE_2W, FORM_WIDE */
    {nullptr, 0, false}, {sums32_fast_2w, 2, true}, {nullptr, 0, false},                /* -, FORM_FAST_2W, - */
    {nullptr, 0, false}, {full32_2w_walk, 2, false}, {full32_wide_walk, 2, false},      /* -, FORM_MID_WALK_2W, FORM_WIDE_WALK */
};
static const SumsForm TRAY38_SUMS[ck::FORM_COUNT] = {
    {full40, 1, false}, {full40_2w, 2, false}, {nullptr, 0, false},
    {nullptr, 0, false}, {sums40_fast_2w, 2, true}, {nullptr, 0, false},
    {nullptr, 0, false}, {full40_2w_walk, 2, false}, {nullptr, 0, false},
};

/* A launch of args->step (settings: two_waves, chunks, resume_grid and the scheduler's) that accumulates into args->sums, whose rows it
 * zeroes first -- or, with sums null, a launch as ever that also fills body_cfrc and the read-out block.  fast with one wave per env
 * falls back to the full form alone, as ck::launch_forms has it.  Models on one of the two compile-time trees; -1 where that does not
 * hold or a pass is refused. */
extern "C" int emu_sums_run(const emu_sums_args *args, emu_step_result *result) {
    const emu_step_args &a = args->step;
    const emu_settings &set = a.settings;
    const int nenv = a.nenv, nsub = a.nsub, resume_grid = set.resume_grid > 0 ? set.resume_grid : 1;
    static cm_model_t synced;
    synced = *a.model; cm_model_sync_params(&synced);
    const cm_model_t *model = &synced;
    const ck::StepFamily fam = ck::pick_family(*model, false);
    const bool cassie32 = fam == ck::CASSIE || fam == ck::CASSIE_HFIELD || fam == ck::CASSIE_ALL, tray38 = fam == ck::TRAY;
    if (!(cassie32 || tray38)) return -1;
    const SumsForm *bodies = cassie32 ? CASSIE32_SUMS : TRAY38_SUMS;
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
    io.body_cfrc = args->body_cfrc; io.ext = args->ext;
    /* (the launcher: a stepping launch zeroes the rows of its range ahead of its first substep; a forward pass is not handed the block) */
    const bool sums = args->sums && a.integrate;
    if (sums) { io.sums = args->sums; io.sums_stride = CM_SUM_DIM; memset(args->sums, 0, sizeof(double) * CM_SUM_DIM * (size_t)nenv); }
    const bool wide = cassie32 && model->maxefc > ck::MID_ROWS;
    const int alone = wide ? ck::FORM_WIDE : set.two_waves ? ck::FORM_ALONE_2W : ck::FORM_ALONE;
    ck::StepForms forms = {alone, ck::FORM_ALONE, false, set.inplace_stay_rows};
    std::vector<int> progress((size_t)nenv, 0), list((size_t)nenv, 0), list2((size_t)nenv, 0), chunk_flag((size_t)nenv, 0);
    int count[2] = {0, 0}, count2[2] = {0, 0};
    volatile int seen = -1, seen2 = -1, chunk_fault = 0;
    ck::HandoverLists hl = {list.data(), count, &seen, list2.data(), count2, &seen2};
    if (args->fast && a.integrate && !args->ext && set.two_waves) {
        forms = {ck::FORM_FAST_2W, ck::FORM_MID_WALK_2W, wide, set.inplace_stay_rows};
        io.progress = progress.data();
        io.nchunk = (set.chunks > 1 && nsub >= 2) ? set.chunks : 1;
        io.chunk_seq = 1; io.chunk_flag = chunk_flag.data(); io.chunk_fault = &chunk_fault;
    }
    const ck::StepPlan plan = ck::plan_step(io, forms, hl, {(unsigned)nenv, (unsigned)resume_grid, (unsigned)(resume_grid > 1 ? resume_grid - 1 : 1)});
    result->fast_bails = result->wide_envs = result->chunk_fault = 0;
    emu::with_settings hooks(set);
    for (int i = 0; i < plan.n; ++i) {
        const ck::StepPass &p = plan.pass[i];
        const SumsForm &f = bodies[p.form];
        if (!f.body) { fprintf(stderr, "emu (sums): no instantiation of form %d\n", p.form); abort(); }
        /* (a fast pass of a launch that does not accumulate would be the lean form's, which is not this unit's: refused like any other pairing the rule names) */
        if (ck::step_sums_refuses(p.form, p.io.ext != nullptr, p.io.integrate, p.io.prof != nullptr, p.io.sums != nullptr, f.sums_inst)) return -1;
        g_io = p.io;
        const int handed = p.io.handover_list ? p.io.handover_count[0] : 0;
        if (p.form == ck::FORM_WIDE_WALK) result->wide_envs += handed;
        emu::run_grid(f.body, (int)p.grid, f.nw);
        if (ck::is_fast_form(p.form)) for (int e = 0; e < nenv; ++e) if (progress[e] < nsub) ++result->fast_bails;
        if (p.io.handover_list && (p.io.handover_count[0] != 0 || p.io.handover_count[1] != 0 || *p.io.handover_seen != handed)) {
            fprintf(stderr, "emu (sums): the pass of form %d left count %d ticket %d seen %d (handed %d)\n", p.form, p.io.handover_count[0], p.io.handover_count[1], (int)*p.io.handover_seen, handed);
            abort();
        }
    }
    result->chunk_fault = chunk_fault;
    return 0;
}
extern "C" unsigned long emu_sizeof_sums_args(void) { return sizeof(emu_sums_args); }
extern "C" unsigned long emu_offsetof_sums_args(int k) {
    const unsigned long off[] = {offsetof(emu_sums_args, sums), offsetof(emu_sums_args, body_cfrc), offsetof(emu_sums_args, ext), offsetof(emu_sums_args, fast)};
    return off[k];
}
/* the block's layout (cm_model.h) -> {COUNT, BODY_CFRC, BODY_TOUCH, BODY_CFRC_MAX2, ACT_FORCE, ACT_FORCE2, ACT_POWER, ACT_POSPOWER, DIM, CM_MAXBODY, CM_MAXU} */
extern "C" void emu_sums_layout(int *out) {
    const int v[] = {CM_SUM_COUNT, CM_SUM_BODY_CFRC, CM_SUM_BODY_TOUCH, CM_SUM_BODY_CFRC_MAX2, CM_SUM_ACT_FORCE, CM_SUM_ACT_FORCE2, CM_SUM_ACT_POWER,
                     CM_SUM_ACT_POSPOWER, CM_SUM_DIM, CM_MAXBODY, CM_MAXU};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
}
/* where the launch descriptor holds the block (appended: everything in front of it is where it was) -> {sums, sums_stride, sizeof} */
extern "C" void emu_physio_sums_offsets(unsigned long *out) {
    out[0] = offsetof(ck::PhysIO, sums); out[1] = offsetof(ck::PhysIO, sums_stride); out[2] = sizeof(ck::PhysIO);
}
/* ck::launch_forms with the trailing arguments prof and sums -> {first, mid, wide, stay_rows}; the launcher's last check of a pass (step_sums_refuses) */
extern "C" void emu_launch_forms_sums(int fam, int has_inplace, int maxefc, int integrate, int ext, int n, int nsub, int fast_rows, int waves_per_env,
                                      int waves_per_env_tray, int inplace, int prof, int sums, int *out) {
    const ck::StepForms f = ck::launch_forms(fam, has_inplace != 0, maxefc, integrate, ext != 0, n, nsub, fast_rows != 0, waves_per_env, waves_per_env_tray, inplace != 0, prof != 0, sums != 0);
    out[0] = f.first; out[1] = f.mid; out[2] = f.wide ? 1 : 0; out[3] = f.stay_rows;
}
extern "C" int emu_step_sums_refuses(int form, int ext, int integrate, int prof, int sums, int sums_inst) {
    return ck::step_sums_refuses(form, ext != 0, integrate, prof != 0, sums != 0, sums_inst != 0) ? 1 : 0;
}
