/*
 * emu_placement.cpp -- TEST-ONLY: phys_batch_end_episodes with PLACED restarts (csrc/episode_kernels.h: cassie_episode_place_kernel) on the
 * wave emulator, configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h).
 */
#include <cstring>

#include "small_launch.h"
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
    static cm_model_t synced;
    synced = *a->model; cm_model_sync_params(&synced);
    static ck::PlaceTable table;
    if (const char *bad = ck::place_configure(synced, 0, a->anchor, a->offsets, a->npoints, a->ground_ref, table)) { if (why) *why = bad; return -1; }
    const ck::PlaceCfg place = {a->anchor, a->npoints, a->ground_ref, &table, a->offsets, a->pose, a->next, a->ground};
    ck::BatchView v = {&synced, 0, a->envparams, a->hfield, a->hfield_stride, a->hfield_index, a->nterrain};
    ck::view_sizes(v, synced);
    v.sq = a->sq; v.sqv = a->sqv; v.ssd = a->ssd;
    v.qpos = a->qpos; v.qvel = a->qvel; v.warm = a->qacc_warmstart; v.ctrl = a->ctrl; v.qacc = a->qacc; v.time = a->time;
    v.sens = a->sensordata; v.actvel = a->actuator_velocity; v.meas = a->meas; v.drive = a->drive; v.warn = a->warn;
    g_placeio = ck::make_episode_io(v, {*a->rules, a->done, a->reason, a->steps, a->count, a->terminal, a->bank, a->nrows}, &place, a->env0, a->n,
                                    a->restart, a->pick, a->force);
    emu::run_grid(body_place, a->grid > 0 ? a->grid : ck::episode_grid(a->n));
    return 0;
}
extern "C" int emu_place_warn_bit(void) { return ck::WARN_PLACE_MISS; }
