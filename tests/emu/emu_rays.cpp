/*
 * emu_rays.cpp -- TEST-ONLY: the range sensors on any body (csrc/ray_kernel.h: cassie_rays_kernel) on the wave emulator, configured,
 * checked and launched as phys_batch.hip does it (csrc/small_launch.h: rays_configure, check_ray_geoms, make_rays_io, rays_grid).
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "small_launch.h"
#include "emu_runtime.h"

static const char *g_rays_why = nullptr;
/* the configuration a call's arguments make: the normalised table and the record, or the refusal's message */
static const char *rays_setup(const cm_model_t &m, const ck::RayDef *rays, int nrays, double rmin, double rmax, int use_mask, unsigned mask,
                              std::vector<ck::RayDef> &table, ck::RayCfg &cfg) {
    table.assign(nrays >= 1 && nrays <= ck::RAYS_MAX ? (size_t)nrays : 1, ck::RayDef());
    if (const char *why = ck::rays_configure(m, rays, nrays, rmin, rmax, table.data(), cfg)) return why;
    if (use_mask) {
        if (const char *why = ck::check_ray_geoms(m, mask)) return why;
        cfg.geoms = mask;
    }
    cfg.rays = table.data();
    return nullptr;
}
/* ck::rays_configure and ck::check_ray_geoms -> the message of the refusal, null where the configuration is accepted; table_out
 * (may be null): the table as the kernel would read it, [nrays] entries */
extern "C" const char *emu_rays_check(const cm_model_t *model, const ck::RayDef *rays, int nrays, double rmin, double rmax, int use_mask, unsigned mask,
                                      ck::RayDef *table_out, unsigned *mask_out) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    std::vector<ck::RayDef> table;
    ck::RayCfg cfg;
    if (const char *why = rays_setup(synced, rays, nrays, rmin, rmax, use_mask, mask, table, cfg)) return why;
    if (table_out) memcpy(table_out, table.data(), sizeof(ck::RayDef) * (size_t)nrays);
    if (mask_out) *mask_out = cfg.geoms;
    return nullptr;
}
extern "C" int emu_rays_grid(int n, int nrays) { return ck::rays_grid(n, nrays); }
extern "C" unsigned long emu_sizeof_ray(void) { return sizeof(ck::RayDef); }
/* the record make_rays_io builds for a launch, as numbers a test can read: {env0, n, nrays, sout, sxp, sxq, geoms, ids bound, normals
 * bound, terrain index passed, nterrain} and {rmin, rmax} */
extern "C" void emu_rays_record(const cm_model_t *model, int nrays, double rmin, double rmax, unsigned mask, int sout, int env0, int n, int ids,
                                int normals, int nterrain, long long *ints, double *reals) {
    static int dummy_i;
    static double dummy_d;
    ck::BatchView v = {model, 0, nullptr, nullptr, 0, &dummy_i, nterrain};
    ck::view_sizes(v, *model);
    const ck::RayCfg cfg = {nrays, rmin, rmax, nullptr, mask, ids ? &dummy_i : nullptr, normals ? &dummy_d : nullptr};
    const ck::RayIO io = ck::make_rays_io(v, cfg, &dummy_d, sout, env0, n);
    const long long a[11] = {io.env0, io.n, io.nrays, io.sout, io.sxp, io.sxq, (long long)io.geoms, io.ids != nullptr, io.normals != nullptr,
                             io.hfield_index != nullptr, io.hfield_nterrain};
    memcpy(ints, a, sizeof a);
    reals[0] = io.rmin; reals[1] = io.rmax;
}

/* phys_batch_rays_cast on the emulator: the rays [nrays] as the caller of phys_batch_rays_configure gives them, the mask (use_mask 0: the
 * default), the body poses xpos [nenv][nbody][3] / xquat [nenv][nbody][4] (contiguous, indexed by the absolute env), out [nenv] rows
 * sout doubles apart, ids [nenv][nrays] int32 and normals [nenv][nrays][3] (either may be null); grid 0: the launcher's.  -1 where the
 * launcher would refuse (emu_rays_last_refusal has the message). */
static ck::RayIO g_raysio;
static void body_rays() { ck::cassie_rays_kernel(g_raysio); }
extern "C" int emu_rays_cast(const cm_model_t *model, const cm_envparams_t *envparams, int env0, int n, int grid, const ck::RayDef *rays, int nrays,
                             double rmin, double rmax, int use_mask, unsigned mask, const double *xpos, const double *xquat, double *out, int sout,
                             const float *hfield, unsigned long hfield_stride, const int *hfield_index, int nterrain, int *warn, int *ids,
                             double *normals) {
    static cm_model_t synced;
    synced = *model; cm_model_sync_params(&synced);
    std::vector<ck::RayDef> table;
    ck::RayCfg cfg;
    g_rays_why = rays_setup(synced, rays, nrays, rmin, rmax, use_mask, mask, table, cfg);
    if (g_rays_why) return -1;
    if (!xpos || !xquat || !out || sout < nrays) { g_rays_why = "the body poses and an output of at least nrays doubles a row"; return -1; }
    cfg.ids = ids; cfg.normals = normals;
    ck::BatchView v = {&synced, 0, envparams, hfield, hfield_stride, const_cast<int *>(hfield_index), nterrain};
    ck::view_sizes(v, synced);
    v.warn = warn; v.xpos = xpos; v.xquat = xquat;
    g_raysio = ck::make_rays_io(v, cfg, out, sout, env0, n);
    emu::run_grid(body_rays, grid > 0 ? grid : ck::rays_grid(n, nrays));
    return 0;
}
extern "C" const char *emu_rays_last_refusal(void) { return g_rays_why; }
