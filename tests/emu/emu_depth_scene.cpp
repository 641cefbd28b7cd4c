/*
 * emu_depth_scene.cpp -- TEST-ONLY: the depth image of a chosen set of geoms, moving bodies included (csrc/depth_kernel.h:
 * cassie_depth_scene_kernel), on the wave emulator, configured, checked and launched as phys_batch.hip does it (csrc/small_launch.h).
 * The entry point always runs the scene kernel, also where the launcher would pick the static one (the default mask, no ids): the tests
 * compare the two.
 */
#include <cmath>
#include <cstring>

#include "small_launch.h"
#include "emu_runtime.h"

/* phys_batch_depth_image with a geom mask and / or a hit-id image bound, on the emulator: emu_depth_image's arguments (tests/emu/
 * emu_depth.cpp), then the mask (bit g: compiled geom g), the body poses xpos [nenv][nbody][3] / xquat [nenv][nbody][4] (contiguous,
 * indexed by the absolute env; null: moving geoms are unseen) and ids [nenv][height * width] int32 (may be null). */
static ck::DepthIO g_sceneio;
static void body_depth_scene() { ck::cassie_depth_scene_kernel(g_sceneio); }
extern "C" int emu_depth_scene_image(const cm_model_t *model, const cm_envparams_t *envparams, int env0, int n, int grid, int body,
                                     const double *cam_pos, const double *cam_quat, const double *pose, int width, int height, double fovy,
                                     double znear, double zfar, const double *qpos, int sq, double *out, int sout,
                                     const float *hfield, unsigned long hfield_stride, const int *hfield_index, int nterrain, int *warn,
                                     unsigned mask, const double *xpos, const double *xquat, int *ids) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    ck::DepthCfg cfg;
    if (ck::depth_configure(synced, 0, body, cam_pos, cam_quat, width, height, fovy, znear, zfar, cfg) || ck::check_depth_geoms(synced, mask)) return -1;
    cfg.pose = pose; cfg.geoms = mask; cfg.ids = ids;
    ck::BatchView v = {&synced, 0, envparams, hfield, hfield_stride, const_cast<int *>(hfield_index), nterrain};
    ck::view_sizes(v, synced);
    v.qpos = const_cast<double *>(qpos); v.sq = sq; v.warn = warn; v.xpos = xpos; v.xquat = xquat;
    g_sceneio = ck::make_depth_io(v, cfg, out, sout, env0, n, true);
    emu::run_grid(body_depth_scene, grid > 0 ? grid : ck::depth_grid(n, width, height));
    return 0;
}
