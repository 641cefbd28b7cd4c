/*
 * emu_states.cpp -- TEST-ONLY: the bank of full states (csrc/state_kernels.h: cassie_state_save_kernel, cassie_state_restore_kernel) on
 * the wave emulator, laid out, checked and launched as phys_batch.hip does it (csrc/small_launch.h: state_layout, state_configure,
 * check_state_call, make_state_io, state_grid).
 */
#include <cstring>

#include "small_launch.h"
#include "emu_runtime.h"

/* what a call is handed, by pointer (tests/states_emu_py.py mirrors it; emu_state_sizeof lets it check the mirror).  env[s] is the
 * host array of section s (ck::SS_*: the order of PHYS_SS_*), indexed by the absolute env, or null where the batch would have none;
 * (the applied forces null: never uploaded; the episode counters null: episodes not enabled; the parameter blocks null: none);
 * sq / sqv / ssd = doubles between the rows of qpos / qvel / sensordata;
 * nterrain: terrains of the bank (0: the terrain index is not part of the env); grid 0: the grid phys_batch.hip launches. */
extern "C" {
typedef struct {
    const cm_model_t *model;
    int nenv, env0, n, grid, nslots, groups, sq, sqv, ssd, nterrain;
    void *env[ck::SS_COUNT];
    unsigned long long *bank;
    const int *slots;
} emu_state_args;
}

static ck::BatchView state_view(const emu_state_args *a, cm_model_t &synced) {
    synced = *a->model; cm_model_sync_params(&synced);
    void *const *e = a->env;
    ck::BatchView v = {&synced, 0, (const cm_envparams_t *)e[ck::SS_PARAMS], nullptr, 0, (int *)e[ck::SS_TERRAIN], a->nterrain};
    ck::view_sizes(v, synced);
    v.sq = a->sq; v.sqv = a->sqv; v.ssd = a->ssd;
    v.time = (double *)e[ck::SS_TIME]; v.qpos = (double *)e[ck::SS_QPOS]; v.qvel = (double *)e[ck::SS_QVEL]; v.warm = (double *)e[ck::SS_WARM];
    v.ctrl = (double *)e[ck::SS_CTRL]; v.qacc = (double *)e[ck::SS_QACC]; v.sens = (double *)e[ck::SS_SENS]; v.actvel = (double *)e[ck::SS_ACTVEL];
    v.meas = (double *)e[ck::SS_MEAS]; v.drive = (cm_drive_state_t *)e[ck::SS_DRIVE]; v.warn = (int *)e[ck::SS_WARN];
    v.xpos = v.xpos_w = (double *)e[ck::SS_XPOS]; v.xquat = v.xquat_w = (double *)e[ck::SS_XQUAT];
    v.pd_ptarget = (double *)e[ck::SS_PD_PTARGET]; v.pd_kp = (double *)e[ck::SS_PD_KP]; v.pd_kd = (double *)e[ck::SS_PD_KD];
    v.pd_dtarget = (double *)e[ck::SS_PD_DTARGET]; v.pd_torque = (double *)e[ck::SS_PD_TORQUE]; v.drive_cmd = (double *)e[ck::SS_DRIVE_CMD];
    v.qfrc_applied = (double *)e[ck::SS_QFRC_APPLIED]; v.xfrc_applied = (double *)e[ck::SS_XFRC_APPLIED];
    v.ep_steps = (int *)e[ck::SS_EP_STEPS]; v.ep_count = (int *)e[ck::SS_EP_COUNT];
    v.params_w = (cm_envparams_t *)e[ck::SS_PARAMS];
    return v;
}

static ck::StateIO g_stateio;
static void body_save() { ck::cassie_state_save_kernel(g_stateio); }
static void body_restore() { ck::cassie_state_restore_kernel(g_stateio); }

extern "C" unsigned long emu_state_sizeof(void) { return sizeof(emu_state_args); }
extern "C" int emu_state_nsections(void) { return ck::SS_COUNT; }
extern "C" int emu_state_warn_bit(void) { return ck::WARN_STATE_SLOT; }
extern "C" int emu_state_layout_version(void) { return ck::STATE_LAYOUT_VERSION; }
extern "C" int emu_state_grid(int n) { return ck::state_grid(n); }
extern "C" int emu_state_section_bytes(int which) { return which == 0 ? (int)sizeof(cm_drive_state_t) : (int)sizeof(cm_envparams_t); }
/* offsets_counts [SS_COUNT][2] of the row for these sizes and groups -> the row dim */
extern "C" int emu_state_layout(int nq, int nv, int nu, int nsd, int nbody, int groups, int *offsets_counts) {
    const ck::StateLayout L = ck::state_layout(nq, nv, nu, nsd, nbody, groups);
    for (int s = 0; s < ck::SS_COUNT; ++s) { offsets_counts[2 * s] = L.off[s]; offsets_counts[2 * s + 1] = L.count[s]; }
    return L.row_dim;
}
extern "C" unsigned long long emu_state_signature(const cm_model_t *model, int groups) {
    return ck::state_signature(*model, ck::state_layout(model->nq, model->nv, model->nu, model->nsensordata, model->nbody, groups));
}
/* what phys_batch_state_configure would refuse of these arrays ("" : nothing) */
extern "C" const char *emu_state_configure(const emu_state_args *a) {
    static cm_model_t synced;
    const char *why = ck::state_configure(state_view(a, synced), a->nslots, a->groups);
    return why ? why : "";
}
/* a save (restore 0) or a restore -> 0, or -1 with *why naming what phys_batch_state_save / _restore would refuse */
extern "C" int emu_state_call(const emu_state_args *a, int restore, const char **why) {
    static const char *none = "";
    if (why) *why = none;
    static cm_model_t synced;
    const ck::BatchView v = state_view(a, synced);
    const ck::StateCfg c = {a->nslots, a->groups, a->bank};
    const char *bad = ck::check_state_call(c, a->nenv, a->env0, a->n);
    if (!bad) bad = ck::state_configure(v, c.nslots, c.groups);
    if (bad) { if (why) *why = bad; return -1; }
    if (a->n == 0) return 0;
    g_stateio = ck::make_state_io(v, c, a->env0, a->n, a->slots);
    emu::run_grid(restore ? body_restore : body_save, a->grid > 0 ? a->grid : ck::state_grid(a->n));
    return 0;
}
