/*
 * emu_terrain.cpp -- TEST-ONLY: terrains on the wave emulator.  The translation unit of the emulator library: it takes in
 * emu_episodes.cpp (and through it emu_runtime.cpp, both unchanged) and adds the height scan kernel's entry point and a sibling of
 * emu_phys_run whose envs read their height field through PhysIO::hfield_stride / hfield_index (per-env grids, or a bank of terrains
 * and a per-env index).
 */
#include "emu_episodes.cpp"

/* phys_batch_height_scan on the emulator: the device's scan kernel on host arrays (indexed by the absolute env; sq / sout = doubles
 * between the rows of qpos / of the output), as `grid` workgroups that walk the range [env0, env0 + n) (0: the grid phys_batch.hip
 * launches).  envparams / hfield / hfield_index may be null. */
static ck::ScanIO g_scanio;
static void body_scan() { ck::cassie_scan_kernel(g_scanio); }
extern "C" int emu_height_scan(const cm_model_t *model, const cm_envparams_t *envparams, int env0, int n, int grid, const double *offsets,
                               int npoints, int body, double range, const double *qpos, int sq, double *out, int sout,
                               const float *hfield, unsigned long hfield_stride, const int *hfield_index, int nterrain, int *warn) {
    if (npoints <= 0 || npoints > ck::SCAN_MAXPOINTS || body <= 0 || body >= model->nbody) return -1;
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    ck::ScanIO &io = g_scanio;
    memset(&io, 0, sizeof io);
    io.models = &synced; io.model_stride = 0; io.envparams = envparams;
    io.env0 = env0; io.n = n; io.npoints = npoints; io.body = body; io.range = range; io.offsets = offsets;
    io.qpos = qpos; io.sq = sq; io.out = out; io.sout = sout;
    io.hfield = hfield; io.hfield_stride = hfield_stride; io.hfield_index = hfield_index; io.hfield_nterrain = nterrain;
    io.warn = warn;
    g_grid = grid > 0 ? grid : (n < ck::SCAN_GRID ? n : ck::SCAN_GRID);
    for (int wg = 0; wg < g_grid; ++wg) { g_env = wg; run_block(body_scan); }
    g_grid = 1;
    return 0;
}

/* emu_phys_run with the terrain fields of PhysIO: hfield_stride floats between the grids (0: one shared grid), hfield_index null (env e
 * reads grid e) or [nenv] indices into a bank of nterrain grids.  The set-up is emu_phys_run's (one instantiation alone, or the fast
 * kernel and the passes behind it, by the emulator's settings); no drive-level I/O, no PD fields. */
extern "C" int emu_phys_run_terrain(const cm_model_t *model, int nenv, int nsub, double *qpos, double *qvel, double *qacc_warmstart, double *time,
                                    const double *ctrl, double *qacc, double *sensordata, double *actuator_velocity, int *warn, int *info,
                                    const float *hfield, unsigned long hfield_stride, const int *hfield_index, int nterrain) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced); model = &synced;
    memset(&g_io, 0, sizeof g_io);
    g_io.models = model; g_io.model_stride = 0; g_io.envparams = g_envparams;
    g_io.nenv = nenv; g_io.nsub = nsub; g_io.integrate = 1;
    g_io.sq = model->nq; g_io.sqv = model->nv; g_io.sv = model->nv; g_io.su = model->nu; g_io.ssd = model->nsensordata; g_io.sb = model->nbody;
    g_io.qpos = qpos; g_io.qvel = qvel; g_io.qacc_warmstart = qacc_warmstart; g_io.time = time; g_io.ctrl = (double *)ctrl;
    g_io.qacc = qacc; g_io.sensordata = sensordata; g_io.actuator_velocity = actuator_velocity; g_io.warn = warn; g_io.info = info;
    g_io.hfield = hfield; g_io.hfield_stride = hfield_stride; g_io.hfield_index = hfield_index; g_io.hfield_nterrain = nterrain;
    if (!topo_matches(model, ck::TopoCassie32::table, ck::TopoCassie32::nv, ck::TopoCassie32::body_levels)) return -1;
    const EmuForm *bodies = CASSIE32_BODIES;
    ck::StepForms forms = {ck::FORM_ALONE, ck::FORM_ALONE, false, g_inplace_stay};
    static int progress[1 << 12], list[1 << 12], count[2], list2[1 << 12], count2[2], chunk_flag[1 << 12];
    static volatile int seen, seen2;
    ck::HandoverLists hl = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (g_fast_rows && nenv <= (1 << 12)) {
        count[0] = count[1] = 0; seen = -1; count2[0] = count2[1] = 0; seen2 = -1;
        hl = {list, count, &seen, list2, count2, &seen2};
        forms = {!g_two_waves ? ck::FORM_FAST : g_inplace ? ck::FORM_FAST_INPLACE : ck::FORM_FAST_2W, g_two_waves ? ck::FORM_MID_WALK_2W : ck::FORM_ALONE,
                 model->maxefc > ck::MID_ROWS, g_inplace_stay};
        g_io.progress = progress;
        g_io.nchunk = (g_chunks > 1 && nsub >= 2) ? g_chunks : 1;
        g_io.chunk_seq = ++g_chunk_seq; g_io.chunk_flag = chunk_flag; g_io.chunk_fault = &g_chunk_fault;
    } else forms.first = model->maxefc > ck::MID_ROWS ? ck::FORM_WIDE : g_two_waves ? ck::FORM_ALONE_2W : ck::FORM_ALONE;
    const ck::StepPlan plan = ck::plan_step(g_io, forms, hl, {(unsigned)nenv, (unsigned)g_resume_grid, (unsigned)(g_resume_grid > 1 ? g_resume_grid - 1 : 1)});
    for (int i = 0; i < plan.n; ++i) {
        const ck::StepPass &p = plan.pass[i];
        const EmuForm &f = bodies[p.form];
        if (!f.body) wv::emu_fail("no instantiation of this form");
        g_io = p.io;
        g_grid = (int)p.grid;
        for (int wg = 0; wg < g_grid; ++wg) { g_env = wg; run_block(f.body, f.nw); }
    }
    g_grid = 1;
    return 0;
}
extern "C" int emu_warn_bit(int which) { return which == 0 ? ck::WARN_TERRAIN_INDEX : ck::WARN_SCAN_TILTED; }
