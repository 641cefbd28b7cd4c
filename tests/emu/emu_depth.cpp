/*
 * emu_depth.cpp -- TEST-ONLY: the depth-image kernel (csrc/depth_kernel.h) on the wave emulator, configured, checked and launched as
 * phys_batch.hip does it (csrc/small_launch.h).
 */
#include <cmath>
#include <cstring>

#include "small_launch.h"
#include "emu_runtime.h"

/* phys_batch_depth_image on the emulator: the device's depth kernel on host arrays (indexed by the absolute env; sq / sout = doubles
 * between the rows of qpos / of the output; fovy in radians), as `grid` workgroups that walk the jobs of the range [env0, env0 + n)
 * (0: the grid phys_batch.hip launches).  envparams / pose / hfield / hfield_index may be null. */
static ck::DepthIO g_depthio;
static void body_depth() { ck::cassie_depth_kernel(g_depthio); }
extern "C" int emu_depth_image(const cm_model_t *model, const cm_envparams_t *envparams, int env0, int n, int grid, int body,
                               const double *cam_pos, const double *cam_quat, const double *pose, int width, int height, double fovy,
                               double znear, double zfar, const double *qpos, int sq, double *out, int sout,
                               const float *hfield, unsigned long hfield_stride, const int *hfield_index, int nterrain, int *warn) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    ck::DepthCfg cfg;
    if (ck::depth_configure(synced, 0, body, cam_pos, cam_quat, width, height, fovy, znear, zfar, cfg)) return -1;
    cfg.pose = pose;
    if (ck::depth_scene_kernel(synced, cfg)) return -1;   /* (a fresh configuration is the static kernel's: this entry point's) */
    ck::BatchView v = {&synced, 0, envparams, hfield, hfield_stride, const_cast<int *>(hfield_index), nterrain};
    v.qpos = const_cast<double *>(qpos); v.sq = sq; v.warn = warn;
    g_depthio = ck::make_depth_io(v, cfg, out, sout, env0, n, false);
    emu::run_grid(body_depth, grid > 0 ? grid : ck::depth_grid(n, width, height));
    return 0;
}
