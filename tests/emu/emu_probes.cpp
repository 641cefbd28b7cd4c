/*
 * emu_probes.cpp -- TEST-ONLY: the probes (csrc/probe_kernels.h: cassie_probe_kernel) on the wave emulator, configured, checked and
 * launched as phys_batch.hip does it (csrc/small_launch.h: probes_configure, probe_classify_geoms, check_probe_call, make_probe_io,
 * probe_grid, probe_layout).  emu_probe is phys_batch_probe: the emulator's forward pass with the read-out over an env range, storing
 * to scratch arrays alone, then the kernel; emu_probe_reduce is the kernel alone on read-out blocks the caller hands in.
 */
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

static const char *g_probe_why = nullptr;
extern "C" const char *emu_probe_last_refusal(void) { return g_probe_why; }

/* {PROBE_GRID, PROBES_MAX, sizeof(ProbeDef), PQ_COUNT, PC_NGROUPS} and sizeof(cm_ext_t), for the binding's own checks */
extern "C" void emu_probe_constants(long long *out) {
    const long long a[6] = {ck::PROBE_GRID, ck::PROBES_MAX, (long long)sizeof(ck::ProbeDef), ck::PQ_COUNT, ck::PC_NGROUPS, (long long)sizeof(cm_ext_t)};
    memcpy(out, a, sizeof a);
}
extern "C" int emu_probe_grid(int n) { return ck::probe_grid(n); }
extern "C" int emu_probe_layout(int nprobes, unsigned quantities, int nv, int *offsets, int *dims) { return ck::probe_layout(nprobes, quantities, nv, offsets, dims); }
/* ck::probes_configure -> the message of its refusal, null where it accepts; cfg_out (may be null): {nprobes, quantities} of the record */
extern "C" const char *emu_probe_check(const cm_model_t *model, const ck::ProbeDef *probes, int nprobes, unsigned quantities, long long *cfg_out) {
    ck::ProbeCfg cfg;
    const char *why = ck::probes_configure(*model, probes, nprobes, quantities, cfg);
    if (!why && cfg_out) { cfg_out[0] = cfg.nprobes; cfg_out[1] = cfg.quantities; }
    return why;
}
/* ck::check_probe_call of a record that is (not) configured */
extern "C" const char *emu_probe_call_check(int configured, int nenv, int env0, int n) {
    static const ck::ProbeDef def = {};
    static const cm_ext_t *const some = (const cm_ext_t *)&def;   /* (any address: only compared with null) */
    ck::ProbeCfg cfg = {};
    if (configured) { cfg.nprobes = 1; cfg.quantities = 1; cfg.probes = &def; cfg.ext = some; }
    return ck::check_probe_call(cfg, nenv, env0, n);
}
extern "C" void emu_probe_classify(const double *geom_user, int nuser_geom, const int *geom_group, int ngeom, int *table) {
    ck::probe_classify_geoms(geom_user, nuser_geom, geom_group, ngeom, table);
}
/* the record make_probe_io builds for a launch, as numbers a test can read: {env0, n, nprobes, quantities, sout, sxp, sxq, sq, sqv, sv,
 * row_dim, geom classes passed, ngeom, contacts passed} and the offsets [PQ_COUNT]; classes / contacts: whether the record names them */
extern "C" void emu_probe_record(const cm_model_t *model, int nprobes, unsigned quantities, int sout, int sq, int sqv, int env0, int n, int classes,
                                 int ngeom, int contacts, long long *ints, int *offsets) {
    static int dummy_i;
    static double dummy_d;
    static const ck::ProbeDef def = {};
    ck::BatchView v = {model, 0, nullptr};
    ck::view_sizes(v, *model);
    v.sq = sq; v.sqv = sqv; v.qpos = &dummy_d; v.qvel = &dummy_d;
    const ck::ProbeCfg cfg = {nprobes, quantities, &def, classes ? &dummy_i : nullptr, ngeom, (const cm_ext_t *)&def, &dummy_d, &dummy_d, &dummy_d,
                              contacts ? &dummy_i : nullptr};
    const ck::ProbeIO io = ck::make_probe_io(v, cfg, &dummy_d, sout, env0, n);
    const long long a[14] = {io.env0, io.n, io.nprobes, (long long)io.quantities, io.sout, io.sxp, io.sxq, io.sq, io.sqv, io.sv, io.row_dim,
                             io.geom_class != nullptr, io.ngeom, io.contacts != nullptr};
    memcpy(ints, a, sizeof a);
    for (int q = 0; q < ck::PQ_COUNT; ++q) offsets[q] = io.off[q];
}

static ck::ProbeIO g_probeio;
static void body_probe() { ck::cassie_probe_kernel(g_probeio); }

/* what both entry points share: the checked record (table and quantities), the geoms' classes (geom_group null: none) */
static const char *probe_setup(const cm_model_t &m, const ck::ProbeDef *probes, int nprobes, unsigned quantities, const double *geom_user, int nuser_geom,
                               const int *geom_group, int ngeom, std::vector<int> &classes, ck::ProbeCfg &cfg) {
    if (const char *why = ck::probes_configure(m, probes, nprobes, quantities, cfg)) return why;
    if (nprobes == 0) return "0 probes: nothing to launch (the launcher releases)";
    if (geom_group && ngeom > 0) {
        classes.assign((size_t)ngeom, 0);
        ck::probe_classify_geoms(geom_user, nuser_geom, geom_group, ngeom, classes.data());
        cfg.geom_class = classes.data(); cfg.ngeom = ngeom;
    }
    return nullptr;
}

/* phys_batch_probe on the emulator.  args: the batch's arrays ([args->nenv] rows of the model's sizes, indexed by the absolute env); the
 * range [env0, env0 + n); grid 0: the launcher's.  geom_user [ngeom][nuser_geom] / geom_group [ngeom]: the host model's full list (null:
 * no classes, no contact word).  out: [nenv] rows sout doubles apart; contacts: [nenv] int32 or null.  None of args' arrays is written
 * but the sticky warning words: the forward pass stores to scratch arrays of this call.  -1 where the launcher would refuse
 * (emu_probe_last_refusal has the message). */
extern "C" int emu_probe(const emu_step_args *args, int env0, int n, int grid, const ck::ProbeDef *probes, int nprobes, unsigned quantities,
                         const double *geom_user, int nuser_geom, const int *geom_group, int ngeom, double *out, int sout, int *contacts,
                         emu_step_result *result) {
    static cm_model_t synced;
    synced = *args->model; cm_model_sync_params(&synced);
    const cm_model_t &m = synced;
    const int nenv = args->nenv;
    std::vector<int> classes;
    ck::ProbeCfg cfg;
    g_probe_why = probe_setup(m, probes, nprobes, quantities, geom_user, nuser_geom, geom_group, ngeom, classes, cfg);
    if (g_probe_why) return -1;
    std::vector<cm_ext_t> ext((size_t)nenv);
    memset(ext.data(), 0, sizeof(cm_ext_t) * ext.size());
    std::vector<double> qacc((size_t)nenv * m.nv, 0.0), sens((size_t)nenv * m.nsensordata, 0.0), actvel((size_t)nenv * m.nu, 0.0);
    std::vector<double> xpos((size_t)nenv * m.nbody * 3, 0.0), xquat((size_t)nenv * m.nbody * 4, 0.0);
    cfg.ext = ext.data(); cfg.xpos = xpos.data(); cfg.xquat = xquat.data(); cfg.qacc = qacc.data(); cfg.contacts = contacts;
    g_probe_why = ck::check_probe_call(cfg, nenv, env0, n);
    if (g_probe_why) return -1;
    if (!out || sout < ck::probe_layout(nprobes, quantities, m.nv, nullptr, nullptr)) { g_probe_why = "an output of at least the row's doubles a row"; return -1; }
    if (n == 0) return 0;
    /* the forward pass of the range: the step unit's, on the range's rows of the caller's arrays, storing to the scratch arrays above */
    const size_t e0 = (size_t)env0;
    emu_step_args a = *args;
    a.model = &synced; a.nenv = n; a.nsub = 1; a.integrate = 0;
    a.qpos += e0 * m.nq; a.qvel += e0 * m.nv; a.qacc_warmstart += e0 * m.nv; a.time += e0; a.ctrl += e0 * m.nu;
    if (a.qfrc_applied) a.qfrc_applied += e0 * m.nv;
    if (a.xfrc_applied) a.xfrc_applied += e0 * 6 * m.nbody;
    a.qacc = qacc.data() + e0 * m.nv; a.sensordata = sens.data() + e0 * m.nsensordata; a.actuator_velocity = actvel.data() + e0 * m.nu;
    a.warn += e0; a.info = nullptr;
    a.xpos = xpos.data() + e0 * 3 * m.nbody; a.xquat = xquat.data() + e0 * 4 * m.nbody;
    if (a.pd_ptarget) { a.pd_ptarget += e0 * m.nu; a.pd_kp += e0 * m.nu; a.pd_kd += e0 * m.nu; }
    if (a.drive_state) a.drive_state += e0;
    if (a.drive_cmd) a.drive_cmd += e0 * (m.nu + 1);
    if (a.meas) a.meas += e0 * CM_MEAS_DIM;
    if (a.pd_dtarget) a.pd_dtarget += e0 * m.nu;
    if (a.pd_torque) a.pd_torque += e0 * m.nu;
    if (a.envparams) a.envparams += e0;
    if (a.hfield && a.hfield_stride && !a.hfield_index) a.hfield += e0 * a.hfield_stride;
    if (a.hfield_index) a.hfield_index += e0;
    emu::run_step(a, *result, ext.data() + e0);
    ck::BatchView v = {&synced, 0, args->envparams};
    ck::view_sizes(v, m);
    v.qpos = args->qpos; v.qvel = args->qvel;
    g_probeio = ck::make_probe_io(v, cfg, out, sout, env0, n);
    emu::with_settings hooks(args->settings);
    emu::run_grid(body_probe, grid > 0 ? grid : ck::probe_grid(n));
    return 0;
}

/* cassie_probe_kernel alone: ext [nenv], xpos [nenv][nbody][3], xquat [nenv][nbody][4], qpos / qvel / qacc [nenv] dense rows -- what a
 * forward pass would have left, made by hand -- for envs [env0, env0 + n).  The rest as emu_probe. */
extern "C" int emu_probe_reduce(const cm_model_t *model, int nenv, int env0, int n, int grid, const ck::ProbeDef *probes, int nprobes, unsigned quantities,
                                const double *geom_user, int nuser_geom, const int *geom_group, int ngeom, const cm_ext_t *ext, const double *xpos,
                                const double *xquat, const double *qpos, const double *qvel, const double *qacc, double *out, int sout, int *contacts) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    std::vector<int> classes;
    ck::ProbeCfg cfg;
    g_probe_why = probe_setup(synced, probes, nprobes, quantities, geom_user, nuser_geom, geom_group, ngeom, classes, cfg);
    if (g_probe_why) return -1;
    cfg.ext = ext; cfg.xpos = xpos; cfg.xquat = xquat; cfg.qacc = qacc; cfg.contacts = contacts;
    g_probe_why = ck::check_probe_call(cfg, nenv, env0, n);
    if (g_probe_why) return -1;
    if (!xpos || !xquat || !qpos || !qvel || !qacc || !out || sout < ck::probe_layout(nprobes, quantities, synced.nv, nullptr, nullptr)) {
        g_probe_why = "the forward pass's arrays and an output of at least the row's doubles a row";
        return -1;
    }
    if (n == 0) return 0;
    ck::BatchView v = {&synced, 0, nullptr};
    ck::view_sizes(v, synced);
    v.qpos = const_cast<double *>(qpos); v.qvel = const_cast<double *>(qvel);
    g_probeio = ck::make_probe_io(v, cfg, out, sout, env0, n);
    emu::run_grid(body_probe, grid > 0 ? grid : ck::probe_grid(n));
    return 0;
}
