/*
 * emu_kernels.cpp -- TEST-ONLY: the small kernels (csrc/small_kernels.h: set_const, derive; episode_kernels.h: episodes; surface_kernels.h:
 * height scan) on the wave emulator, launched as phys_batch.hip launches them (csrc/small_launch.h: the same records, builders, grids and
 * checks), the probes of those rules, the wave primitives' checks (tests/device/wave_bodies.h), and the probes of layouts, constants
 * and elementary functions the tests read.  The step kernel is emu_step.cpp's: nothing here instantiates it.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

extern "C" unsigned long emu_offsetof32(int which) {
    typedef ck::EnvShared<32> E;
    switch (which) {
    case 0: return offsetof(E, x); case 1: return offsetof(E, Lp); case 2: return offsetof(E, LHp); case 3: return offsetof(E, accel);
    case 4: return offsetof(E, dinv); case 5: return offsetof(E, cdof); case 6: return offsetof(E, com); case 7: return offsetof(E, qpos);
    case 8: return offsetof(E, qfrc_smooth); case 9: return offsetof(E, sens); case 10: return offsetof(E, drv_x); case 11: return offsetof(E, c_dist);
    case 12: return offsetof(E, c_dim); case 13: return offsetof(E, c_root); case 14: return offsetof(E, c_tran); default: return sizeof(E);
    }
}
/* phys_batch_set_const / the friction refresh of phys_batch_randomize on the emulator: the device's set_const kernel, env by env */
static ck::SetConstIO g_scio;
static void body_setconst() { ck::cassie_setconst_kernel(g_scio); }
extern "C" int emu_set_const(const cm_model_t *model, cm_envparams_t *params, int nenv, int derive_inertial) {
    g_scio = ck::make_setconst_io(model, params, 0, nenv, derive_inertial);
    emu::run_grid(body_setconst, nenv);
    return 0;
}
extern "C" unsigned long emu_sizeof_envparams(void) { return sizeof(cm_envparams_t); }
/* phys_batch_derive on the emulator: a forward pass with the read-out enabled, then the derive kernel.  The forward pass is the step
 * unit's (emu::run_step), handed what phys_batch_derive's reads: the state, ctrl and the shared height field, no applied forces, no PD
 * or drive-level input, body poses into scratch arrays */
static ck::DeriveIO g_dio;
static void body_derive() { ck::cassie_derive_kernel(g_dio); }
extern "C" int emu_derive(const emu_step_args *args, const int *ids, double *derived, double *qM, emu_step_result *result) {
    static cm_model_t synced;
    synced = *args->model; cm_model_sync_params(&synced);
    const cm_model_t *model = &synced;
    const int nenv = args->nenv;
    std::vector<cm_ext_t> ext((size_t)nenv);
    memset(ext.data(), 0, sizeof(cm_ext_t) * ext.size());
    std::vector<double> xpos((size_t)nenv * model->nbody * 3, 0.0), xquat((size_t)nenv * model->nbody * 4, 0.0);
    emu_step_args a = *args;
    a.nsub = 1; a.integrate = 0;
    a.qfrc_applied = a.xfrc_applied = nullptr; a.pd_ptarget = a.pd_kp = a.pd_kd = nullptr;
    a.drive_mode = 0; a.drive_state = nullptr; a.drive_cmd = nullptr; a.meas = nullptr; a.pd_dtarget = a.pd_torque = nullptr;
    a.hfield_stride = 0; a.hfield_index = nullptr; a.nterrain = 0;
    a.xpos = xpos.data(); a.xquat = xquat.data();
    emu::run_step(a, *result, ext.data());
    ck::BatchView v = {model, 0, a.envparams};
    v.xpos = a.xpos; v.xquat = a.xquat;
    g_dio = ck::make_derive_io(v, nenv, ext.data(), derived, qM, ids);
    emu::with_settings hooks(a.settings);
    emu::run_grid(body_derive, nenv);
    return 0;
}
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
    ck::BatchView v = {};
    ck::view_sizes(v, *model);
    v.sq = sq; v.sqv = sqv; v.ssd = ssd;
    v.qpos = qpos; v.qvel = qvel; v.warm = qacc_warmstart; v.ctrl = ctrl; v.qacc = qacc; v.time = time; v.sens = sensordata;
    v.actvel = actuator_velocity; v.meas = meas; v.drive = drive; v.warn = warn;
    g_epio = ck::make_episode_io(v, {*rules, done, reason, steps, count, terminal, bank, nrows}, nullptr, env0, n, restart, pick, force);
    emu::run_grid(body_episode, grid > 0 ? grid : ck::episode_grid(n));
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
/* phys_batch_height_scan on the emulator: the device's scan kernel on host arrays (indexed by the absolute env; sq / sout = doubles
 * between the rows of qpos / of the output), as `grid` workgroups that walk the range [env0, env0 + n) (0: the grid phys_batch.hip
 * launches).  envparams / hfield / hfield_index may be null. */
static ck::ScanIO g_scanio;
static void body_scan() { ck::cassie_scan_kernel(g_scanio); }
extern "C" int emu_height_scan(const cm_model_t *model, const cm_envparams_t *envparams, int env0, int n, int grid, const double *offsets,
                               int npoints, int body, double range, const double *qpos, int sq, double *out, int sout,
                               const float *hfield, unsigned long hfield_stride, const int *hfield_index, int nterrain, int *warn) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    ck::ScanCfg cfg;
    if (ck::scan_configure(synced, 0, offsets, npoints, body, range, cfg)) return -1;
    cfg.offsets = offsets;
    ck::BatchView v = {&synced, 0, envparams, hfield, hfield_stride, const_cast<int *>(hfield_index), nterrain};
    v.qpos = const_cast<double *>(qpos); v.sq = sq; v.warn = warn;
    g_scanio = ck::make_scan_io(v, cfg, out, sout, env0, n);
    emu::run_grid(body_scan, grid > 0 ? grid : ck::scan_grid(n));
    return 0;
}
/* the launcher's rules for the small kernels (csrc/small_launch.h) one at a time, for tests/test_small_launch.py.  The grid of kernel
 * `which` (0 scan, 1 episodes, 2 depth image of width x height, 3 reset, 4 set_const, 5 parameter scatter) over n envs; the depth
 * kernel (0 static, 1 scene) a mask and bound ids give; the message (null: accepted) of a scan / a depth / a mask configuration */
extern "C" int emu_small_grid(int which, int n, int width, int height) {
    return which == 0 ? ck::scan_grid(n) : which == 1 ? ck::episode_grid(n) : which == 2 ? ck::depth_grid(n, width, height)
         : which == 3 ? ck::reset_grid(n) : which == 4 ? ck::setconst_grid(n) : ck::param_scatter_grid(n);
}
extern "C" unsigned emu_depth_geoms(const cm_model_t *model, int all) { return all ? ck::depth_all_geoms(*model) : ck::depth_default_geoms(*model); }
extern "C" int emu_depth_scene_kernel(const cm_model_t *model, unsigned mask, int ids_bound) {
    ck::DepthCfg cfg = {};
    cfg.geoms = mask; cfg.ids = ids_bound ? (int *)model : nullptr;   /* (any address: only compared with null) */
    return ck::depth_scene_kernel(*model, cfg) ? 1 : 0;
}
extern "C" const char *emu_scan_check(const cm_model_t *model, int model_stride, const double *offsets, int npoints, int body, double range) {
    ck::ScanCfg cfg;
    return ck::scan_configure(*model, model_stride, offsets, npoints, body, range, cfg);
}
extern "C" const char *emu_depth_check(const cm_model_t *model, int model_stride, int body, const double *cam_pos, const double *cam_quat, int width,
                                       int height, double fovy, double znear, double zfar) {
    ck::DepthCfg cfg;
    return ck::depth_configure(*model, model_stride, body, cam_pos, cam_quat, width, height, fovy, znear, zfar, cfg);
}
extern "C" const char *emu_depth_geoms_check(const cm_model_t *model, unsigned mask) { return ck::check_depth_geoms(*model, mask); }

extern "C" int emu_warn_bit(int which) { return which == 0 ? ck::WARN_TERRAIN_INDEX : ck::WARN_SCAN_TILTED; }
/* the layout of emu_api.h's structs, for the ctypes mirror of tests/emu_py.py: which = 0 emu_settings, 1 emu_step_args, 2 emu_step_result;
 * field = its index in declaration order (-1 past the last) */
#define API_SETTINGS(F) F(two_waves) F(fast_rows) F(inplace) F(inplace_stay_rows) F(chunks) F(resume_grid) F(wave_schedule) F(force_runtime_topology) \
    F(force_guarded_pgs) F(poison_lds) F(poison_lo) F(poison_hi) F(skip_com_init) F(producer_xcc)
#define API_STEP_ARGS(F) F(model) F(nenv) F(nsub) F(integrate) F(qpos) F(qvel) F(qacc_warmstart) F(time) F(ctrl) F(qfrc_applied) F(xfrc_applied) \
    F(qacc) F(sensordata) F(actuator_velocity) F(warn) F(info) F(xpos) F(xquat) F(pd_ptarget) F(pd_kp) F(pd_kd) F(drive_mode) F(drive_state) \
    F(drive_cmd) F(meas) F(pd_dtarget) F(pd_torque) F(envparams) F(hfield) F(hfield_stride) F(hfield_index) F(nterrain) F(settings)
#define API_STEP_RESULT(F) F(fast_bails) F(wide_envs) F(chunk_fault)
extern "C" unsigned long emu_sizeof_api(int which) {
    return which == 0 ? sizeof(emu_settings) : which == 1 ? sizeof(emu_step_args) : which == 2 ? sizeof(emu_step_result) : 0;
}
extern "C" long emu_offsetof_api(int which, int field) {
#define API_OFFSET(f) (long)offsetof(API_T, f),
    static const long settings[] = {
#define API_T emu_settings
        API_SETTINGS(API_OFFSET)
#undef API_T
    }, step_args[] = {
#define API_T emu_step_args
        API_STEP_ARGS(API_OFFSET)
#undef API_T
    }, step_result[] = {
#define API_T emu_step_result
        API_STEP_RESULT(API_OFFSET)
#undef API_T
    };
    const long *t = which == 0 ? settings : which == 1 ? step_args : which == 2 ? step_result : nullptr;
    const int n = which == 0 ? (int)(sizeof settings / sizeof(long)) : which == 1 ? (int)(sizeof step_args / sizeof(long)) : which == 2 ? (int)(sizeof step_result / sizeof(long)) : 0;
    return field >= 0 && field < n ? t[field] : -1;
}
/* cassie_core_sim's safety layer as the step kernel computes it (csrc/pk_safety.h), sample by sample and drive by drive: the
 * ten torques and the message bits of n samples (u, q, w, L: [n][10]; sto: [n]) */
extern "C" void emu_core_safety(int n, const double *u, const double *q, const double *w, const double *L, const unsigned char *sto,
                                double *tau_out, int *msg_out) {
    for (int s = 0; s < n; ++s) {
        int msg = 0;
        for (int k = 0; k < 10; ++k)
            tau_out[10 * s + k] = ck::safety::drive_torque(k, u[10 * s + k], q + 10 * s, w[10 * s + k], L[10 * s + k], sto[s] != 0, &msg);
        msg_out[s] = msg;
    }
}
extern "C" double emu_core_safety_torque_limit(int k) { return ck::safety::torque_limit(k); }
/* the kinematics stage's own elementary functions, for direct accuracy tests */
extern "C" void emu_sincos_reduced(double x, double *s, double *c) { ck::sincos_reduced(x, *s, *c); }
extern "C" void emu_normalize4_fast(double *q) { ck::normalize4_fast(q); }
extern "C" double emu_normalize3_fast(double *a) { return ck::normalize3_fast(a); }
extern "C" unsigned long emu_sizeof_shared32(void) { return sizeof(ck::EnvShared<32>); }

/* packed factor rows (ck::LPack): the run-time-lane addressing agrees with the compile-time slots; returns the number of mismatches */
template <class TOPO, int NVP>
static int lpack_mismatches() {
    typedef ck::LPack<TOPO, NVP> LP;
    int bad = 0;
    for (int k = 0; k < NVP; ++k) {
        const typename LP::Row r = LP::row_of(k);
        for (int i = 0; i < NVP; ++i) {
            const bool has = LP::has(k, i);
            const int want = has ? LP::idx(k, i) : -1;
            if (has) {
                bad += LP::row_slot(k, i) != want;
                bad += !(LP::row_has(r, i) && LP::row_idx(r, i) == want);
                bad += !(LP::col_has(k, i) && LP::col_idx(k, i) == want);
            } else {
                if (LP::packed) bad += LP::row_slot(k, i) != LP::dump;
                if (i < k) bad += LP::row_has(r, i) || LP::col_has(k, i);
            }
        }
    }
    return bad;
}
extern "C" int emu_lpack_check(void) {
    return lpack_mismatches<ck::TopoCassieTray38, 40>() + lpack_mismatches<ck::TopoCassie32, 32>() + lpack_mismatches<ck::TopoRuntime, 40>();
}
extern "C" int emu_lpack_count(int which) { return which ? ck::LPack<ck::TopoCassieTray38, 40>::count : ck::LPack<ck::TopoCassie32, 32>::count; }

/* the primitive checks of tests/device/wave_bodies.h, one emulated wave per trial: the same entry points as the device's
 * wave_check.hip (tests/wave_check.py) */
#include "wave_bodies.h"
static const double *g_wc_in;
static double *g_wc_out;
static void (*g_wc_body)(const double *, double *);
static int g_wc_nin, g_wc_nout;
static void wc_trial() { g_wc_body(g_wc_in + (size_t)wv::env_id() * g_wc_nin * 64, g_wc_out + (size_t)wv::env_id() * g_wc_nout * 64); }
static int wc_run(void (*body)(const double *, double *), const double *in, double *out, int ntrial, int nin, int nout) {
    g_wc_body = body; g_wc_in = in; g_wc_out = out; g_wc_nin = nin; g_wc_nout = nout;
    emu::run_grid(wc_trial, ntrial);
    return 0;
}
#define WC_ENTRY(name, nin, nout) \
    extern "C" int wc_##name(const double *in, double *out, int ntrial) { return wc_run(wc::name, in, out, ntrial, nin, nout); }
WAVE_CHECK_BODIES(WC_ENTRY)
/* ... and those that read an auxiliary block every trial of the call shares */
static const void *g_wc_aux;
static void (*g_wc_aux_body)(const double *, double *, const void *);
static void wc_aux_trial() { g_wc_aux_body(g_wc_in + (size_t)wv::env_id() * g_wc_nin * 64, g_wc_out + (size_t)wv::env_id() * g_wc_nout * 64, g_wc_aux); }
static int wc_aux_run(void (*body)(const double *, double *, const void *), const double *in, double *out, int ntrial, int nin, int nout,
                      const void *aux, unsigned long aux_bytes) {
    if (!aux || aux_bytes < sizeof(wc::FactorAux)) return 1; /* (hipErrorInvalidValue, as the device's launcher answers) */
    g_wc_aux_body = body; g_wc_aux = aux; g_wc_in = in; g_wc_out = out; g_wc_nin = nin; g_wc_nout = nout;
    emu::run_grid(wc_aux_trial, ntrial);
    return 0;
}
#define WC_AUX_ENTRY(name, nin, nout)                                                                                    \
    extern "C" int wc_##name(const double *in, double *out, int ntrial, const void *aux, unsigned long aux_bytes) {     \
        return wc_aux_run(wc::name, in, out, ntrial, nin, nout, aux, aux_bytes);                                         \
    }
WAVE_CHECK_AUX_BODIES(WC_AUX_ENTRY)
