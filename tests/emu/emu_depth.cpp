/*
 * emu_depth.cpp -- TEST-ONLY: the depth-image kernel (csrc/depth_kernel.h) on the wave emulator.
 */
#include <cmath>
#include <cstring>

#include "depth_kernel.h"
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
    if (width < 1 || height < 1 || (long long)width * height > ck::DEPTH_MAXPIXELS || body <= 0 || body >= model->nbody) return -1;
    if (!(fovy > 0 && fovy < M_PI) || !(znear > 0 && znear < zfar)) return -1;
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    ck::DepthIO &io = g_depthio;
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
    const int tiles = ((width + ck::DEPTH_TILE - 1) / ck::DEPTH_TILE) * ((height + ck::DEPTH_TILE - 1) / ck::DEPTH_TILE);
    const long long jobs = (long long)n * tiles;
    emu::run_grid(body_depth, grid > 0 ? grid : (int)(jobs < ck::DEPTH_GRID ? jobs : ck::DEPTH_GRID));
    return 0;
}
