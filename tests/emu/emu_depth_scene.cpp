/*
 * emu_depth_scene.cpp -- TEST-ONLY: the depth image of a chosen set of geoms, moving bodies included (csrc/depth_kernel.h:
 * cassie_depth_scene_kernel), on the wave emulator.
 */
#include <cmath>
#include <cstring>

#include "depth_kernel.h"
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
    if (width < 1 || height < 1 || (long long)width * height > ck::DEPTH_MAXPIXELS || body <= 0 || body >= model->nbody) return -1;
    if (!(fovy > 0 && fovy < M_PI) || !(znear > 0 && znear < zfar)) return -1;
    if (model->ngeom < 32 && (mask >> model->ngeom) != 0u) return -1;
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    ck::DepthIO &io = g_sceneio;
    memset(&io, 0, sizeof io);
    io.models = &synced; io.model_stride = 0; io.envparams = envparams;
    io.env0 = env0; io.n = n; io.body = body; io.width = width; io.height = height;
    io.tan_half = tan(0.5 * fovy); io.znear = znear; io.zfar = zfar;
    for (int k = 0; k < 3; ++k) io.cam_pos[k] = cam_pos[k];
    for (int k = 0; k < 4; ++k) io.cam_quat[k] = cam_quat[k];
    io.pose = pose;
    io.qpos = qpos; io.sq = sq; io.out = out; io.sout = sout;
    io.hfield = hfield; io.hfield_stride = hfield_stride; io.hfield_index = hfield_index; io.hfield_nterrain = nterrain;
    io.warn = warn;
    io.geoms = mask; io.xpos = xpos; io.xquat = xquat; io.sxp = 3 * model->nbody; io.sxq = 4 * model->nbody; io.ids = ids;
    const int tiles = ((width + ck::DEPTH_TILE - 1) / ck::DEPTH_TILE) * ((height + ck::DEPTH_TILE - 1) / ck::DEPTH_TILE);
    const long long jobs = (long long)n * tiles;
    emu::run_grid(body_depth_scene, grid > 0 ? grid : (int)(jobs < ck::DEPTH_GRID ? jobs : ck::DEPTH_GRID));
    return 0;
}
