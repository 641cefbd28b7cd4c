/*
 * emu_episodes.cpp -- TEST-ONLY: phys_batch_end_episodes on the wave emulator.  The translation unit of the emulator library: it takes
 * in emu_runtime.cpp (the scheduler, the wv:: primitives and the entry points of the step / derive / set_const kernels, unchanged) and
 * adds the entry points of the episode kernel, which need the runtime's workgroup loop.
 */
#include "emu_runtime.cpp"

/* phys_batch_end_episodes on the emulator: the device's episode kernel on host arrays (all indexed by the absolute env; sq / sqv /
 * ssd = doubles between the rows of qpos / qvel / sensordata; meas / drive / bank / pick / force may be null), as `grid` workgroups
 * that walk the range [env0, env0 + n) (0: the grid phys_batch.hip launches) */
static ck::EpisodeIO g_epio;
static void body_episode() { ck::cassie_episode_kernel(g_epio); }
extern "C" int emu_end_episodes(const cm_model_t *model, const cm_episode_rules_t *rules, int env0, int n, int restart, int grid,
                                double *qpos, int sq, double *qvel, int sqv, double *sensordata, int ssd, double *qacc_warmstart, double *ctrl,
                                double *qacc, double *time, double *actuator_velocity, double *meas, cm_drive_state_t *drive, int *warn,
                                int *done, int *reason, int *steps, int *count, double *terminal,
                                const double *bank, int nrows, const int *pick, const int *force) {
    if (restart && (!bank || nrows <= 0)) return -1;
    ck::EpisodeIO &io = g_epio;
    memset(&io, 0, sizeof io);
    io.env0 = env0; io.n = n; io.restart = restart ? 1 : 0; io.nrows = nrows;
    io.nq = model->nq; io.nv = model->nv; io.nu = model->nu; io.nsd = model->nsensordata; io.sq = sq; io.sqv = sqv; io.ssd = ssd;
    io.row_dim = model->nq + model->nv + model->nsensordata + model->nu + model->nv;
    io.rules = *rules;
    io.qpos = qpos; io.qvel = qvel; io.warm = qacc_warmstart; io.ctrl = ctrl; io.qacc = qacc; io.time = time; io.sens = sensordata;
    io.actvel = actuator_velocity; io.meas = meas; io.drive = drive; io.warn = warn;
    io.done = done; io.reason = reason; io.steps = steps; io.count = count; io.terminal = terminal;
    io.bank = bank; io.pick = pick; io.force = force;
    g_grid = grid > 0 ? grid : (n < ck::EPISODE_GRID ? n : ck::EPISODE_GRID);
    for (int wg = 0; wg < g_grid; ++wg) { g_env = wg; run_block(body_episode); }
    g_grid = 1;
    return 0;
}
extern "C" unsigned long emu_sizeof_episode_rules(void) { return sizeof(cm_episode_rules_t); }
extern "C" long emu_offsetof_episode_rules(int which) {
    switch (which) {
    case 0: return offsetof(cm_episode_rules_t, min_height); case 1: return offsetof(cm_episode_rules_t, min_upright);
    case 2: return offsetof(cm_episode_rules_t, max_steps); case 3: return offsetof(cm_episode_rules_t, warn_mask);
    case 4: return offsetof(cm_episode_rules_t, nonfinite); default: return -1;
    }
}
