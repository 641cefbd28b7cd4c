/*
 * emu_placement.cpp -- TEST-ONLY: phys_batch_end_episodes with PLACED restarts (csrc/small_kernels.h: cassie_episode_place_kernel) on the
 * wave emulator.
 */
#include <cstring>

#include "small_kernels.h"
#include "emu_runtime.h"

/* what a call is handed, by pointer (tests/placement_emu_py.py mirrors it; emu_place_sizeof lets it check the mirror).  The arrays are
 * host arrays indexed by the absolute env, as in emu_end_episodes; sq / sqv / ssd = doubles between the rows of qpos / qvel / sensordata;
 * meas / drive / pick / force / envparams / hfield / hfield_index / next / offsets may be null. */
extern "C" {
typedef struct {
    const cm_model_t *model;
    const cm_episode_rules_t *rules;
    int env0, n, restart, grid;         /* grid 0: the grid phys_batch.hip launches */
    int sq, sqv, ssd, nrows;
    double *qpos, *qvel, *sensordata, *qacc_warmstart, *ctrl, *qacc, *time, *actuator_velocity, *meas;
    cm_drive_state_t *drive;
    int *warn, *done, *reason, *steps, *count;
    double *terminal;
    const double *bank;
    const int *pick, *force;
    /* placement: phys_batch_place_configure's arguments and the three per-env arrays */
    int anchor, npoints;
    double ground_ref;
    const double *offsets, *pose;
    const int *next;
    double *ground;
    /* what the surface reads, as emu_height_scan is handed it; the index is WRITTEN where next terrains are bound */
    const cm_envparams_t *envparams;
    const float *hfield;
    unsigned long hfield_stride;
    int *hfield_index;
    int nterrain;
} emu_place_args;
}

static ck::EpisodeIO g_placeio;
static void body_place() { ck::cassie_episode_place_kernel(g_placeio); }
extern "C" unsigned long emu_place_sizeof(void) { return sizeof(emu_place_args); }
/* -> 0, or -1 with *why (if given) naming what phys_batch_place_configure would refuse */
extern "C" int emu_place_end_episodes(const emu_place_args *a, const char **why) {
    static const char *none = "";
    if (why) *why = none;
    if (a->restart && (!a->bank || a->nrows <= 0)) return -1;
    if (a->npoints < 0 || a->npoints > ck::PLACE_MAXPOINTS || (a->npoints > 0 && !a->offsets)) { if (why) *why = "a footprint of 0 .. 1024 points"; return -1; }
    static cm_model_t synced;
    synced = *a->model; cm_model_sync_params(&synced);
    const cm_model_t *model = &synced;
    ck::EpisodeIO &io = g_placeio;
    memset(&io, 0, sizeof io);
    static ck::PlaceTable table;
    memset(&table, 0, sizeof table);
    if (const char *bad = ck::place_classify(*model, a->anchor, table)) { if (why) *why = bad; return -1; }
    io.place_anchor = a->anchor; io.place_table = &table;
    io.env0 = a->env0; io.n = a->n; io.restart = a->restart ? 1 : 0; io.nrows = a->nrows;
    io.nq = model->nq; io.nv = model->nv; io.nu = model->nu; io.nsd = model->nsensordata; io.sq = a->sq; io.sqv = a->sqv; io.ssd = a->ssd;
    io.row_dim = model->nq + model->nv + model->nsensordata + model->nu + model->nv;
    io.rules = *a->rules;
    io.qpos = a->qpos; io.qvel = a->qvel; io.warm = a->qacc_warmstart; io.ctrl = a->ctrl; io.qacc = a->qacc; io.time = a->time;
    io.sens = a->sensordata; io.actvel = a->actuator_velocity; io.meas = a->meas; io.drive = a->drive; io.warn = a->warn;
    io.done = a->done; io.reason = a->reason; io.steps = a->steps; io.count = a->count; io.terminal = a->terminal;
    io.bank = a->bank; io.pick = a->pick; io.force = a->force;
    io.place_npoints = a->npoints; io.place_ground_ref = a->ground_ref;
    io.place_offsets = a->offsets; io.place_pose = a->pose; io.place_ground = a->ground;
    io.model = model; io.envparams = a->envparams;
    io.hfield = a->hfield; io.hfield_stride = a->hfield_stride;
    if (a->nterrain > 0) { io.hfield_index = a->hfield_index; io.hfield_nterrain = a->nterrain; io.place_next = a->next; }
    emu::run_grid(body_place, a->grid > 0 ? a->grid : (a->n < ck::EPISODE_GRID ? a->n : ck::EPISODE_GRID));
    return 0;
}
extern "C" int emu_place_warn_bit(void) { return ck::WARN_PLACE_MISS; }
