/*
 * depth_kernel.h -- the egocentric depth image (phys_batch_depth_image, include/cassie_phys.h: the definition is there): one ray
 * per pixel of a pinhole camera mounted on a body, against the env's static collision geometry (cassie_depth_kernel) or against any
 * chosen set of its collision geoms, the moving bodies' included (cassie_depth_scene_kernel).  It holds the camera, the pixels and the
 * two kernels (one body, depth_jobs.inc); the ray against a geom is scene_rays.h's.  Written with the wv:: primitives only,
 * workgroups of one wave: phys_batch.hip launches them, the wave emulator (tests/emu/emu_depth.cpp, emu_depth_scene.cpp) runs the same
 * text.
 */
#ifndef CASSIE_DEPTH_KERNEL_H
#define CASSIE_DEPTH_KERNEL_H

#include "scene_rays.h"

namespace ck {

/* A job is (env, tile of DEPTH_TILE x DEPTH_TILE pixels), lane l of the wave the tile's pixel (l / 8, l % 8): the 64 rays of a wave
 * leave through neighbouring pixels and walk neighbouring cells of the grid, so their loops are of similar length and their reads
 * share cache lines.  A fixed grid of DEPTH_GRID workgroups walks the job list of the env range, tiles of one env next to each other.
 * The grid's size and the tile's shape are first choices: DESIGN 4.3 has what the launch was measured to cost with them, and no
 * other size or shape has been tried.
 *
 * Per job, the same in every lane: the body's world pose from qpos (static_body_pose, as the height scan), the camera's world pose,
 * and -- geom by geom -- the static geom's world pose (static_geom_pose).  Per lane: the pixel's ray o + t D, D = R_cam d with
 * d = (a T (2 (c + 1/2) / W - 1), T (1 - 2 (r + 1/2) / H), -1) NOT normalised (t is the depth along the optical axis), against the
 * geom (scene_ray_geom without the capsules: planes, boxes, the height field).  The value is the smallest t in [near, far) over the
 * geoms, `far` where there is none. */
constexpr int DEPTH_GRID = 2048, DEPTH_TILE = 8, DEPTH_MAXPIXELS = 16384;

/* THE SCENE KERNEL (cassie_depth_scene_kernel) renders the geoms of the mask DepthIO::geoms: besides the static planes, boxes and
 * height field also spheres and capsules, and spheres, capsules and boxes on moving bodies, whose world pose is that of the body as
 * the last step launch or forward pass stored it composed with the geom's own (scene_geom_frame).  It is the same per-pixel body as
 * the static kernel's (depth_jobs.inc, with a compile-time switch), with the solids' cull, the sphere's shortcut and the capsules.
 *
 * The geoms' world frames are needed once per job, not once per lane: lane g builds geom g's (position and rotation, 12 doubles) and
 * the geom loop, whose index is wave-uniform, reads them with wv::readlane -- 24 v_readlane_b32 into scalars per rendered geom, no
 * LDS, no barrier, nothing to allocate at launch, and the emulator runs it as it stands.  (LDS would cost a write, a wait and 24
 * ds_reads per geom and lane for values that are the wave's, not the lane's.) */

struct DepthIO {
    const cm_model_t *models; int model_stride;
    const cm_envparams_t *envparams;   /* null, or one block per env (PhysIO::envparams) */
    int env0, n, body, width, height;
    double tan_half, znear, zfar;      /* tan(fovy / 2) */
    double cam_pos[3], cam_quat[4];    /* the camera in the body's frame, shared by the envs ... */
    const double *pose;                /* ... or null / [nenv][7] (pos, quat) per env, indexed by the absolute env */
    const double *qpos; int sq;
    double *out; int sout;             /* [nenv][height * width] with a row stride in doubles */
    const float *hfield; size_t hfield_stride; const int *hfield_index; int hfield_nterrain;   /* as in PhysIO */
    int *warn;
    /* the scene kernel's (all zero: the static kernel's behaviour) */
    unsigned geoms;                    /* bit g: compiled geom g is rendered */
    const double *xpos, *xquat;        /* [nenv][nbody][3 / 4] body poses in the world, rows sxp / sxq doubles apart */
    int sxp, sxq;
    int *ids;                          /* null, or [nenv][height * width]: the geom that gave the value, -1 where it is `far` */
};

WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_depth_kernel(DepthIO io) {
    constexpr bool SCENE = false;
#include "depth_jobs.inc"
}
WV_GLOBAL void __launch_bounds__(WV_WAVE) cassie_depth_scene_kernel(DepthIO io) {
    constexpr bool SCENE = true;
#include "depth_jobs.inc"
}

}  // namespace ck
#endif
