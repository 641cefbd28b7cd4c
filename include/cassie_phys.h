/*
 * cassie_phys.h -- the INNER drop-in boundary: the thin C ABI the host C glue
 * (cassiemujoco.c-equivalent) calls where the reference calls into MuJoCo.
 *
 * The reference has no clean ABI at this seam: it is a dlsym'd function-pointer
 * table plus direct mjModel/mjData field access (reference src/cassiemujoco.c:67-122,
 * field census in SURVEY.md 8b).  Each entry point below names the reference
 * call(s) it replaces.  Plain C types only: handles, pointers, sizes.
 *
 * All phys_batch_* entry points run on the MI355X through HIP; creating a batch
 * without a usable GPU fails loudly (NULL + message on stderr) -- there is no CPU
 * fallback in this library.
 */
#ifndef CASSIE_PHYS_H
#define CASSIE_PHYS_H

#include <stddef.h>
#include "cm_model.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ model --- */
typedef struct phys_model phys_model_t; /* host model: names, all geoms, hfield samples ... */

/* mj_loadXML (reference src/cassiemujoco.c:851, :930, :997).  Accepts the MJCF subset of
 * the in-scope models (.xml) or the neutral .cmodel text form; NULL + err text on failure. */
phys_model_t *phys_model_load(const char *path, char *err, int errlen);
/* mj_copyModel (reference :1013, :1016, :1093) */
phys_model_t *phys_model_copy(const phys_model_t *src);
/* mj_deleteModel (reference :883, :1110) */
void phys_model_free(phys_model_t *m);
int phys_model_save(const phys_model_t *m, const char *path);
/* mj_setConst (reference :952, :976): recompute invweight0 / meaninertia after inertial edits */
void phys_model_set_const(phys_model_t *m);
/* derive the pointer-free kernel model; returns 0 on success */
int phys_model_compile(const phys_model_t *m, cm_model_t *out, char *err, int errlen);
/* option flags of the model (CM_FLAG_* in csrc/cm_model.h: implicit joint damping, warm start, refsafe -- the mjOption
 * disable / enable bits the in-scope models use -- and the height-field contact options CM_FLAG_HFDENSE / HFMULTI / HFPRISM);
 * a change takes effect with the next compile / the next step of a cassie_sim_t */
unsigned phys_model_flags(const phys_model_t *m);
int phys_model_set_flag(phys_model_t *m, unsigned flag, int on);
/* a 64-bit fingerprint of every model array / option a caller can change through the views below: compared before a step
 * instead of recompiling (the reference hands out raw mjModel pointers, so writes cannot be observed otherwise) */
unsigned long long phys_model_fingerprint(const phys_model_t *m);
unsigned long long phys_hash_floats(const float *data, size_t n);
/* mj_name2id / mj_id2name (reference :861-866, :1244, ...); objtype uses mjtObj numbering */
int phys_model_name2id(const phys_model_t *m, int objtype, const char *name);
const char *phys_model_id2name(const phys_model_t *m, int objtype, int id);

/* sizes: the mjModel ints the reference reads (nq nv nu nbody njnt ngeom nsensordata ...) */
enum { PHYS_NQ, PHYS_NV, PHYS_NU, PHYS_NBODY, PHYS_NJNT, PHYS_NGEOM, PHYS_NSITE, PHYS_NSENSOR, PHYS_NSENSORDATA,
       PHYS_NEQ, PHYS_NHFIELDDATA, PHYS_HFIELD_NROW, PHYS_HFIELD_NCOL, PHYS_NUSER_SENSOR, PHYS_NUSER_ACTUATOR,
       PHYS_NCAM, PHYS_NUSER_GEOM };
int phys_model_size(const phys_model_t *m, int what);

/* read-write views of the mjModel arrays the reference exposes through accessors
 * (reference :1303-1584, :2050-2112).  Layouts follow MuJoCo. */
enum { PHYS_M_BODY_MASS, PHYS_M_BODY_IPOS, PHYS_M_BODY_POS, PHYS_M_BODY_QUAT, PHYS_M_DOF_DAMPING, PHYS_M_JNT_STIFFNESS,
       PHYS_M_QPOS_SPRING, PHYS_M_GEOM_POS, PHYS_M_GEOM_QUAT, PHYS_M_GEOM_SIZE, PHYS_M_GEOM_FRICTION,
       PHYS_M_ACTUATOR_GEAR, PHYS_M_ACTUATOR_CTRLRANGE, PHYS_M_ACTUATOR_USER, PHYS_M_SENSOR_USER, PHYS_M_HFIELD_SIZE,
       PHYS_M_TIMESTEP, PHYS_M_QPOS0, PHYS_M_JNT_RANGE, PHYS_M_STAT_CENTER, PHYS_M_STAT_EXTENT, PHYS_M_GEOM_USER,
       PHYS_M_BODY_INERTIA /* [nbody][3] principal moments (mjModel.body_inertia) */ };
double *phys_model_array(phys_model_t *m, int which);
float *phys_model_geom_rgba(phys_model_t *m);
float *phys_model_hfield_data(phys_model_t *m);
enum { PHYS_MI_JNT_TYPE, PHYS_MI_JNT_QPOSADR, PHYS_MI_JNT_DOFADR, PHYS_MI_GEOM_BODYID, PHYS_MI_GEOM_GROUP,
       PHYS_MI_SENSOR_OBJID, PHYS_MI_SENSOR_TYPE, PHYS_MI_SENSOR_ADR, PHYS_MI_SENSOR_DIM, PHYS_MI_BODY_PARENTID,
       PHYS_MI_GEOM_TYPE, PHYS_MI_BODY_JNTADR, PHYS_MI_BODY_JNTNUM, PHYS_MI_BODY_DOFADR, PHYS_MI_BODY_DOFNUM };
int *phys_model_iarray(phys_model_t *m, int which);

/* ------------------------------------------------------------ batched data --- */
typedef struct phys_batch phys_batch_t; /* N envs resident in HBM: the mjData role, batched */

/* per-env arrays (env-major, contiguous rows) */
enum { PHYS_F_QPOS, PHYS_F_QVEL, PHYS_F_QACC_WARMSTART, PHYS_F_TIME, PHYS_F_CTRL, PHYS_F_QFRC_APPLIED,
       PHYS_F_XFRC_APPLIED, PHYS_F_QACC, PHYS_F_SENSORDATA, PHYS_F_ACTUATOR_VELOCITY, PHYS_F_XPOS, PHYS_F_XQUAT,
       PHYS_F_PD_PTARGET, PHYS_F_PD_KP, PHYS_F_PD_KD, /* on-device joint PD, see phys_batch_set_pd_mode */
       PHYS_F_BODY_CFRC, /* [nbody][3]: net contact force on every body, world frame (reaction on geom2's body, minus it on
                            geom1's; the foot rows are cassie_sim_foot_forces), of the last substep of a launch */
       PHYS_F_DRIVE_CMD,  /* [nu + 1]: commanded drive torques (the cassie_in_t torques, output side) and the STO flag (non-zero =
                             safe torque off), read every substep in CM_DRIVE_TORQUE mode */
       PHYS_F_MEAS,       /* [CM_MEAS_DIM]: the measurement fields of cassie_out_t written by the device-side encoder / motor
                             models (layout: CM_MEAS_* in cm_model.h) */
       PHYS_F_PD_DTARGET, PHYS_F_PD_TORQUE, /* [nu] each: optional velocity targets / feed-forward torques of CM_DRIVE_PD */
       PHYS_F_DERIVED,    /* [CM_DRV_DIM]: the derived block of phys_batch_derive (layout: CM_DRV_* in cm_model.h) */
       PHYS_F_QM,         /* [nv * nv]: dense joint-space inertia matrix (mj_fullM role), written by phys_batch_derive */
       PHYS_F_HEIGHT_SCAN, /* [npoints]: the height scan of phys_batch_height_scan (sized by phys_batch_scan_configure) */
       PHYS_F_DEPTH,      /* [height * width], row-major, row 0 at the top: the depth image of phys_batch_depth_image (sized by
                             phys_batch_depth_configure) */
       PHYS_F_RAYS,       /* [nrays]: the ranges of phys_batch_rays_cast (sized by phys_batch_rays_configure) */
       PHYS_F_STEP_SUMS,  /* [CM_SUM_DIM]: what a stepping launch added up over its substeps (layout: CM_SUM_* in cm_model.h; allocated by
                             phys_batch_step_sums_enable, or a caller's: phys_batch_bind) */
       PHYS_F_PROBES,     /* [phys_batch_probe_row_dim]: the rows of phys_batch_probe (sized by phys_batch_probes_configure; layout:
                             phys_batch_probe_layout) */
       PHYS_F_COUNT };

/* mj_makeData (reference :441-447) for nenv environments on HIP device `device`;
 * every env starts at qpos0 (mj_resetData role).  NULL + stderr message on failure. */
phys_batch_t *phys_batch_create(const cm_model_t *model, int nenv, int device);
void phys_batch_free(phys_batch_t *b);                                  /* mj_deleteData (reference :452) */
int phys_batch_nenv(const phys_batch_t *b);
int phys_batch_field_dim(const phys_batch_t *b, int field);            /* doubles per env */
/* replace the model of one env (env >= 0) or of all envs (env = -1): per-env domain randomisation.  One launch serves every
 * env with the kernel instantiation picked from the shared model, so a per-env model may vary parameters but must keep the
 * shared model's sizes, dof tree, body-tree depth, joint make-up of the bodies (cm_model_t::kin_simple) and kinds of collision
 * pairs (-1 + phys_last_error() otherwise) */
int phys_batch_set_model(phys_batch_t *b, const cm_model_t *model, int env);
/* Per-env domain randomisation ON THE DEVICE (the batched form of the reference's per-simulator setters
 * cassie_sim_set_body_mass / set_body_ipos / set_dof_damping / set_geom_friction, reference src/cassiemujoco.c:1323-1436, and of
 * cassie_sim_just_set_const = mj_setConst, :974-977).  Every env gets a compact parameter block (cm_envparams_t in csrc/cm_model.h,
 * 15.5 KB) that the step kernel reads INSTEAD OF the shared model's fields; the rest of the model stays shared.
 *   phys_batch_randomize   writes rows [n][phys_batch_param_dim] of one parameter (CM_P_BODY_MASS [nbody], CM_P_BODY_IPOS
 *                          [nbody][3], CM_P_BODY_INERTIA [nbody][3] principal moments, CM_P_DOF_DAMPING [nv], CM_P_GEOM_FRICTION
 *                          [model->ngeom][3]: the COLLISION geoms in compiled order, cm_model_t::geom_fullid maps them to the
 *                          reference's full geom list) for envs [env0, env0 + n); values may be a DEVICE pointer (on_device != 0:
 *                          e.g. a torch tensor, nothing crosses PCIe) or host memory.  Damping and friction act from the next
 *                          step on, like in the reference; masses / inertial offsets / inertias act on the dynamics at once and
 *                          on the constraint regularisers after phys_batch_set_const.  Geometry and springs (the reference's
 *                          cassie_sim_set_geom_name_pos / _quat, src/cassiemujoco.c:1478-1537, and jnt_stiffness / qpos_spring):
 *                          CM_P_GEOM_POS [model->ngeom][3] and CM_P_GEOM_QUAT [model->ngeom][4] (unit quaternions; collision geoms
 *                          as for friction: the floor's tilt, the stair boxes, the terrain geom's offset), CM_P_JNT_STIFFNESS
 *                          [njnt] and CM_P_QPOS_SPRING [nq] act from the next step on with no phys_batch_set_const: the rows'
 *                          derived records (rotation matrices, the trees' reach behind the cull of far static geoms, the per-dof
 *                          springs) are re-derived right behind the rows.  Until a batch has randomised geometry (springs) its
 *                          steps read those of the shared model.  Not randomisable: body_pos (it moves the kinematics at qpos0
 *                          set_const starts from), geom_size (MuJoCo does not recompute rbound after a raw edit either), the
 *                          timestep and the height-field size; the batched cassie_batch.h API takes none of these.
 *   phys_batch_set_const   recomputes, per env and on the device, what mj_setConst derives: body_invweight0,
 *                          dof_invweight0, meaninertia (M(qpos0) and its Cholesky factor per env) and the per-joint /
 *                          per-equality / per-pair values the constraint stages read -- bit for bit what compiling a host model
 *                          with the same parameters gives (phys_model_set_const + phys_model_compile).
 * Both are asynchronous on `stream` (NULL = the batch's own) and ordered with the stepping launches there: ranges stepped on
 * other streams must be joined with it first.  Replacing the shared
 * model (phys_batch_set_model, env = -1) drops the blocks; per-env MODELS (env >= 0) and per-env parameter blocks do not mix. */
int phys_batch_param_dim(const phys_batch_t *b, int param);
int phys_batch_randomize(phys_batch_t *b, int param, const double *values, int on_device, int env0, int n, void *stream);
int phys_batch_set_const(phys_batch_t *b, int env0, int n, void *stream);
int phys_batch_download_params(phys_batch_t *b, cm_envparams_t *host, int env0, int n); /* (the model's own block where none exist yet) */
int phys_batch_uses_env_params(const phys_batch_t *b);
size_t phys_sizeof_envparams(void);
/* height-field samples (nrow * ncol floats, MuJoCo's normalised 0..1 elevations): one grid shared by all envs, or --
 * per-env terrain randomisation -- a grid of its own for one env (the others keep what they had) */
int phys_batch_set_hfield(phys_batch_t *b, const float *data, int n);
int phys_batch_set_hfield_env(phys_batch_t *b, int env, const float *data, int n);
/* A BANK of terrains shared by the envs, and which of them each env stands on -- a few dozen grids for thousands of envs (a
 * curriculum) instead of one grid per env, and a terrain change at an episode restart that never leaves the device.
 *   phys_batch_set_hfield_bank   nterrain grids of n floats each (n = the model's hfield_nrow * hfield_ncol, checked), from host memory
 *                                or (on_device != 0) from device memory, e.g. a torch tensor generated on the GPU.  The batch keeps its
 *                                own copy (the call waits for the batch's streams).  Every env starts on terrain 0 (an index array the
 *                                caller bound keeps its contents).  phys_batch_set_hfield / _set_hfield_env afterwards return to those
 *                                modes (per-env grids then start from zeros).
 *   the terrain index            int32 [nenv] in HBM, indexed by the absolute env: phys_batch_terrain_index_ptr hands out the batch's
 *                                own array, phys_batch_bind_terrain_index puts caller-owned memory (a torch tensor) in its place.
 *                                Plain device memory: a loop switches terrains with one statement on the stream of the env range,
 *                                e.g. index[done] = next[done] behind phys_batch_end_episodes; the step launches queued behind it on
 *                                that stream read the new value (one read per env and launch, ahead of the substeps).
 *   phys_batch_set_terrain       ids [n] for envs [env0, env0 + n), from host memory (range-checked against the bank: -1 +
 *                                phys_last_error() for an id outside it; returns once the copy is done) or device memory (asynchronous),
 *                                in order on `stream` (NULL: the batch's own) like phys_batch_randomize.
 * An index outside the bank that reaches the device is CLAMPED to [0, nterrain - 1], never followed, and raises bit 32 of the env's
 * warning word (WARN_TERRAIN_INDEX).  Start states follow the terrain's height only through PLACED RESTARTS (phys_batch_place_configure,
 * below): without them a restart copies its bank row verbatim, and the bank's terrains must agree where restarted envs are put down.
 * A batch that never sets a bank runs exactly as before. */
int phys_batch_set_hfield_bank(phys_batch_t *b, const float *grids, int on_device, int nterrain, int n);
int phys_batch_nterrain(const phys_batch_t *b);   /* terrains of the bank in use, 0 = none */
void *phys_batch_terrain_index_ptr(phys_batch_t *b);
int phys_batch_bind_terrain_index(phys_batch_t *b, void *device_ptr);
int phys_batch_set_terrain(phys_batch_t *b, const int *ids, int on_device, int env0, int n, void *stream);
/* The HEIGHT SCAN: what a policy on rough terrain or stairs sees of the ground, read off the surfaces the contact code collides with.
 *   phys_batch_scan_configure   a pattern of npoints <= 1024 points offsets_xy [npoints][2] (host memory) in the HEADING FRAME of `body`:
 *                               origin at the body's world x, y, turned about world z by the yaw of the body's world quaternion
 *                               (w, x, y, z): atan2(2 (w z + x y), 1 - 2 (y y + z z)).  The body must be a child of the world whose
 *                               joints are slides and at most one ball or free joint (Cassie's pelvis: its pose is qpos[0:7], so the
 *                               scan needs no forward pass).  Sizes PHYS_F_HEIGHT_SCAN to npoints doubles per env in a buffer of the
 *                               batch's own (bind a tensor AFTER configuring; phys_batch_bind_strided takes a row stride for this
 *                               field, so it can be a column block of an observation tensor).  Waits for the batch's streams.
 *   phys_batch_height_scan      one small launch on `stream` (NULL: the batch's own), in order with the step launches there, for envs
 *                               [env0, env0 + n): value of point j = clamp(z_body - S(X_j, Y_j), -range, +range), S = the highest point
 *                               at which the vertical line through the point meets a STATIC collision geom of the env (a geom of a body
 *                               welded to the world), +range where it meets none:
 *                                 plane         the intersection, for planes whose normal has a positive world z;
 *                                 box           where the line leaves the box upwards (slab test in the box's frame, any pose);
 *                                 height field  the env's own grid (shared, per env, or the bank's terrain of the env's index) on the
 *                                               triangulated surface of the narrow phase (vertices on the grid scaled by hfield_size,
 *                                               cells split into v00 v10 v01 and v11 v01 v10), linear within the triangle; outside
 *                                               the grid's footprint a miss.  ONLY for a height-field geom whose z axis is the world's
 *                                               (translation and yaw): a tilted one is left out of that env's scan and raises bit 64
 *                                               of its warning word (WARN_SCAN_TILTED).
 *                               Geom poses are the env's own once geometry is randomised (CM_P_GEOM_POS / CM_P_GEOM_QUAT), the model's
 *                               otherwise.  Spheres, capsules and everything on moving bodies are not scanned; noise, history and fp32
 *                               conversion are the caller's. */
int phys_batch_scan_configure(phys_batch_t *b, const double *offsets_xy, int npoints, int body, double range);
int phys_batch_height_scan(phys_batch_t *b, int env0, int n, void *stream);
/* The DEPTH IMAGE: what a body-mounted pinhole camera sees of the env's static collision geometry, one ray per pixel, on the device
 * (the role of the reference's `egocentric` camera and cassie_vis_draw_depth, with no renderer and no OpenGL context).
 *   phys_batch_depth_configure  the camera is rigidly mounted on `body` (the scan's restriction: a child of the world whose joints are
 *                               slides and at most one ball or free joint, in a shared kin_simple model; its world pose is computed as
 *                               the scan computes it, the joint quaternion normalised), at cam_pos[3], cam_quat[4] (w, x, y, z;
 *                               normalised by the kernel) in the body's frame.  MuJoCo's camera convention: it looks along -z of its
 *                               frame, +x is right, +y is up.  The image has `height` rows of `width` pixels, row 0 at the top,
 *                               1 <= width, height and width * height <= 16384; fovy is the VERTICAL field of view in RADIANS;
 *                               0 < near < far.  Sizes PHYS_F_DEPTH to width * height doubles per env, row-major, in a buffer of the
 *                               batch's own (bind a tensor AFTER configuring; phys_batch_bind_strided takes a row stride for this
 *                               field).  Waits for the batch's streams; reconfiguring is allowed.  -1 + phys_last_error() on failure.
 *   phys_batch_depth_bind_pose  optional per-env extrinsics, [nenv][7] doubles in DEVICE memory (pos, quat; the quaternion is normalised
 *                               by the kernel), indexed by the absolute env: they replace cam_pos / cam_quat for that env (camera-mount
 *                               randomisation is one statement on a tensor).  NULL: back to the shared pose.
 *   phys_batch_depth_image      one launch on `stream` (NULL: the batch's own), in order with the step launches there, for envs
 *                               [env0, env0 + n).  Pixel (r, c) has the camera-frame direction
 *                                   d = (a T (2 (c + 1/2) / width - 1), T (1 - 2 (r + 1/2) / height), -1),  T = tan(fovy / 2), a = width / height,
 *                               NOT normalised, so the ray parameter t of o + t R d is the metric depth ALONG THE OPTICAL AXIS (what a
 *                               linearised depth buffer holds).  The pixel's value is the smallest t in [near, far] at which the ray
 *                               meets a static collision geom of the env, `far` where there is none; intersections at t < near are
 *                               ignored, as a near plane clips them.  The geoms are those the scan sees -- on a body welded to the
 *                               world (static parent bodies composed), poses the env's own once geometry is randomised (CM_P_GEOM_POS /
 *                               CM_P_GEOM_QUAT), the model's otherwise:
 *                                 plane         the crossing of the infinite plane, from either side;
 *                                 box           slab test in the box's frame: the hit is at the entry t0; an origin inside the box
 *                                               (t0 < near <= t1) gives `near`;
 *                                 height field  the triangulated surface of the narrow phase, as in the scan (vertices on the grid scaled
 *                                               by hfield_size, cells split into v00 v10 v01 and v11 v01 v10, at geom z + sz * grid), for
 *                                               ANY pose of the geom, tilted included (the ray is taken into the geom's frame): the first
 *                                               intersection with any triangle, from either face.  Side walls and the base below the
 *                                               surface are not rendered; a ray outside the footprint misses.  The grid is the env's own
 *                                               (shared, per env, or the bank's terrain of the env's index; an index outside the bank is
 *                                               clamped and raises WARN_TERRAIN_INDEX).
 *                               BY DEFAULT spheres, capsules, cylinders and everything on moving bodies -- the robot's own legs, the
 *                               tray and cube of cassie_tray_box -- are not seen; phys_batch_depth_set_geoms (below) chooses other
 *                               geoms.  Noise, history, fp32 conversion and inverse-depth encodings are the caller's.  A batch that
 *                               never configures the depth image runs exactly as before.
 *   phys_batch_depth_set_geoms  WHICH GEOMS ARE RENDERED: bit g of `mask` set = compiled collision geom g is (CM_MAXGEOM is 32: one word
 *                               holds every geom; compiled order is that of cm_model_t::geom_fullid, as for CM_P_GEOM_FRICTION).  The
 *                               default -- phys_batch_depth_default_geoms: the planes, boxes and height field on bodies welded to the
 *                               world, the set described above -- holds until this call is made and is restored by
 *                               phys_batch_depth_configure; phys_batch_depth_all_geoms is every compiled geom.  Configure first; a bit
 *                               at or above ngeom fails with -1 + phys_last_error().  Launches already queued keep their mask.  A batch
 *                               that never makes the call (or makes it with the default) and binds no ids produces, bit for bit, the
 *                               image described above, with the same kernel.  With any other mask, or with ids bound:
 *                                 geom poses    of a geom on a body welded to the world (body_weldid == 0) as above.  Of a geom g on a
 *                                               moving body B the world pose is p = xpos[B] + R(xquat[B]) geom_pos[g] and
 *                                               R = R(xquat[B]) geom_mat[g], xpos / xquat the env's rows of PHYS_F_XPOS / PHYS_F_XQUAT
 *                                               USED AS STORED (not normalised, not recomputed), geom_pos / geom_mat the env's own once
 *                                               geometry is randomised, the model's otherwise.  The camera's pose keeps coming from qpos.
 *                                 STALENESS     PHYS_F_XPOS / PHYS_F_XQUAT are written by the last substep of a stepping launch
 *                                               (phys_batch_step, phys_batch_step_range; also phys_batch_profile_step /
 *                                               _profile_substeps / _time_steps, which step) and by the forward passes
 *                                               (phys_batch_forward, phys_batch_forward_kinematics), for the envs of that launch -- and
 *                                               by an upload or a binding of the two fields themselves.  NOTHING ELSE refreshes them:
 *                                               not phys_batch_reset_envs, not phys_batch_end_episodes with restart, not an upload of
 *                                               qpos, not phys_batch_drive_pass.  After one of those the camera (qpos) is at the new
 *                                               state and the moving geoms are drawn where the bodies WERE; the next stepping launch or
 *                                               forward pass puts them right.  A fresh batch holds zeros there: run a forward pass first.
 *                                               (A stepping launch stores the poses its last substep computed from the qpos that substep
 *                                               STARTED from: behind a step launch the bodies are drawn one substep behind the camera.)
 *                                 solids        a sphere, capsule or box is convex: the ray o + t d (geom frame, d not normalised) meets
 *                                               it over an interval [t0, t1]; the pixel takes t0 if t0 >= near, `near` if t0 < near <= t1
 *                                               (the origin is inside, or the near plane cuts the solid), else the solid is missed.
 *                                                 sphere   radius size[0]: the roots of |o + t d|^2 = r^2;
 *                                                 capsule  radius size[0], half-length size[1] along the geom's z: the cylinder side
 *                                                          x^2 + y^2 = r^2 for |z| <= h and the two spheres at z = -+h; the interval
 *                                                          runs from the smallest entry to the largest exit over the pieces hit;
 *                                                 box      the slab test above, also on a moving body.
 *                                               Static spheres and capsules are rendered like moving ones.  Planes and height fields on
 *                                               MOVING bodies (none of the supported models has one) and any other kind of geom are not
 *                                               rendered whatever the mask says.
 *                                 the value     the smallest such t < far over the rendered geoms, `far` where there is none.
 *                                 NaN poses     a NaN in xpos / xquat fails every comparison made for that geom: it is unseen.  Nothing
 *                                               indexes memory by these values.
 *   phys_batch_depth_bind_ids   optional HIT-ID image: int32 [nenv][height * width] in DEVICE memory, contiguous, indexed by the
 *                               absolute env.  A pixel holds the compiled index of the geom that gave the pixel's value, -1 where the
 *                               value is `far`; ties go to the lower index.  (Mask the robot out, train on a self / other segmentation.)
 *                               Configure first; NULL unbinds; phys_batch_depth_configure drops the binding (the size may change).
 *   phys_batch_debug_depth_launches  diagnostics: the depth launches so far of the static kernel and of the scene kernel (the one that
 *                               takes a mask and ids). */
int phys_batch_depth_configure(phys_batch_t *b, int body, const double *cam_pos, const double *cam_quat, int width, int height, double fovy,
                               double znear, double zfar);
int phys_batch_depth_bind_pose(phys_batch_t *b, const void *device_ptr);
int phys_batch_depth_image(phys_batch_t *b, int env0, int n, void *stream);
int phys_batch_depth_set_geoms(phys_batch_t *b, unsigned mask);
unsigned phys_batch_depth_default_geoms(const phys_batch_t *b);
unsigned phys_batch_depth_all_geoms(const phys_batch_t *b);
int phys_batch_depth_bind_ids(phys_batch_t *b, void *device_ptr);
int phys_batch_debug_depth_launches(const phys_batch_t *b, long long *static_kernel, long long *scene_kernel);
/* RANGE SENSORS ON ANY BODY: a table of rays, each attached to a body of its own -- a foot, a shin, the world -- against the env's
 * collision geometry on the device: the range, the geom hit and the surface normal (foot clearance, the slope under a foothold, a forward
 * range reading, a fixed lidar fan).  Where the scan and the depth image start from one body whose pose follows from qpos, a ray starts
 * from ANY body, whose pose is read from PHYS_F_XPOS / PHYS_F_XQUAT.
 *   phys_batch_rays_configure   rays [nrays] (host memory), 1 <= nrays <= 1024, 0 <= rmin < rmax (finite), every `body` in [0, nbody) -- body 0, the
 *                               world, is allowed: a sensor fixed in the scene -- every `frame` one of PHYS_RAY_*, `origin` finite, `dir`
 *                               finite and not zero: the call NORMALISES dir on the host, so a ray's parameter is a metric range.  Sizes
 *                               PHYS_F_RAYS to nrays doubles per env in a buffer of the batch's own (bind a tensor AFTER configuring;
 *                               phys_batch_bind_strided takes a row stride for this field).  Uploads the table, waits for the batch's
 *                               streams, restores the default mask.  Reconfiguring is allowed; it drops the id and normal bindings (their
 *                               size may change).  -1 + phys_last_error() on failure.
 *                                 POSES         a ray's body pose is the env's row of PHYS_F_XPOS / PHYS_F_XQUAT USED AS STORED (not
 *                                               normalised, not recomputed), as for the moving geoms of the depth image: what the STALENESS
 *                                               paragraph of phys_batch_depth_set_geoms above says holds here word for word -- stepping
 *                                               launches and forward passes write these rows (and an upload or binding of the two fields);
 *                                               phys_batch_reset_envs, phys_batch_end_episodes with restart, an upload of qpos and
 *                                               phys_batch_drive_pass do NOT, and after one of those rays and moving geoms are where the
 *                                               bodies WERE; a fresh batch holds zeros there: run a forward pass first.
 *                                 FRAMES        with p = xpos[body], R = R(xquat[body]) and Rz the rotation about world z by the heading of
 *                                               xquat[body] (the scan's: atan2(2 (w z + x y), 1 - 2 (y y + z z))), the ray o + t u has
 *                                                 PHYS_RAY_BODY       o = p + R origin,   u = R dir;
 *                                                 PHYS_RAY_WORLD_DIR  o = p + R origin,   u = dir  (straight down from a toe, say);
 *                                                 PHYS_RAY_HEADING    o = p + Rz origin,  u = Rz dir.
 *   phys_batch_rays_cast        one launch on `stream` (NULL: the batch's own), in order with the stepping launches there, for envs
 *                               [env0, env0 + n).  A ray's VALUE is the smallest t in [rmin, rmax] at which o + t u meets a geom of the
 *                               mask, rmax where there is none.  Geoms, their poses (static bodies composed; moving bodies from xpos /
 *                               xquat as stored; CM_P_GEOM_POS / CM_P_GEOM_QUAT the env's own once geometry is randomised), the env's
 *                               terrain grid and WARN_TERRAIN_INDEX are exactly those of the depth image with a mask (phys_batch_depth_
 *                               set_geoms above): static planes, boxes, the height field, spheres and capsules; spheres, capsules and
 *                               boxes on moving bodies.  A convex solid met over [t0, t1] gives t0 if t0 >= rmin, rmin if t0 < rmin <= t1
 *                               (the origin is inside it), else nothing.  A NaN pose -- the geom's or the ray's body's -- fails every
 *                               comparison: the geom, or the ray, sees nothing (rmax, id -1, normal 0); nothing indexes memory by such a
 *                               value.  A batch that never configures rays runs exactly as before.
 *   phys_batch_rays_set_geoms   which geoms the rays see: bit g = compiled collision geom g, checked as phys_batch_depth_set_geoms checks
 *                               its mask.  The default, restored by every configure, is phys_batch_depth_default_geoms' set.
 *                               SELF-EXCLUSION: whatever the mask says, a ray skips every geom whose geom_bodyid equals the ray's `body`
 *                               (a toe-mounted ray does not read rmin off the toe's own capsule).
 *   phys_batch_rays_bind_ids    optional HIT IDS: int32 [nenv][nrays] in DEVICE memory, contiguous, indexed by the absolute env: the
 *                               compiled geom that gave the value, -1 where the value is rmax; ties go to the lower index.  Configure
 *                               first; NULL unbinds.
 *   phys_batch_rays_bind_normals optional NORMALS: double [nenv][nrays][3] in DEVICE memory, contiguous: the world-frame unit normal of the
 *                               surface at the hit, oriented against the ray (n . u <= 0); (0, 0, 0) on a miss and where the value is rmin
 *                               taken from inside a solid.
 *                                 plane         plus or minus the geom's z axis;
 *                                 box           the face of the slab axis that gave t0 (on a tie the lowest axis index);
 *                                 sphere        from the centre to the hit;
 *                                 capsule       from the axis point clamp(z, -h, h) to the hit;
 *                                 height field  the normal of the triangle that gave the hit (v00 v10 v01 or v11 v01 v10), rotated by the
 *                                               geom's frame; any pose of the geom, as in the depth image.
 *                               Configure first; NULL unbinds.
 *   phys_batch_debug_ray_launches  diagnostics: the ray launches so far. */
typedef struct { int body; int frame; double origin[3]; double dir[3]; } phys_ray_t;
enum { PHYS_RAY_BODY = 0, PHYS_RAY_WORLD_DIR = 1, PHYS_RAY_HEADING = 2 };
int phys_batch_rays_configure(phys_batch_t *b, const phys_ray_t *rays, int nrays, double rmin, double rmax);
int phys_batch_rays_set_geoms(phys_batch_t *b, unsigned mask);
int phys_batch_rays_bind_ids(phys_batch_t *b, void *device_ptr);      /* int32 [nenv][nrays], NULL unbinds */
int phys_batch_rays_bind_normals(phys_batch_t *b, void *device_ptr);  /* double [nenv][nrays][3], NULL unbinds */
int phys_batch_rays_cast(phys_batch_t *b, int env0, int n, void *stream);
int phys_batch_debug_ray_launches(const phys_batch_t *b, long long *launches);
/* host <-> HBM copies of whole fields or of a row range [env0, env0 + n) */
int phys_batch_upload(phys_batch_t *b, int field, const double *host, int env0, int n);
int phys_batch_download(phys_batch_t *b, int field, double *host, int env0, int n);
/* asynchronous variants on the batch's stream (no host synchronisation; pair with phys_batch_sync);
 * use phys_host_alloc'd (pinned) buffers for true overlap */
int phys_batch_upload_async(phys_batch_t *b, int field, const double *host, int env0, int n);
int phys_batch_download_async(phys_batch_t *b, int field, double *host, int env0, int n);
void *phys_host_alloc(size_t bytes);   /* pinned host memory (hipHostMalloc) */
void phys_host_free(void *p);
int phys_batch_download_warn(phys_batch_t *b, int *host_warn, int *host_info /* [nenv][4] or NULL */);
/* raw device pointer of a field (for torch / RCCL interop); bind replaces it with caller-owned HBM */
void *phys_batch_device_ptr(phys_batch_t *b, int field);
int phys_batch_bind(phys_batch_t *b, int field, void *device_ptr);
/* same with a row stride in doubles (>= the field's dim) for PHYS_F_QPOS / QVEL / SENSORDATA / HEIGHT_SCAN / DEPTH / RAYS / PROBES, so that they can be
 * column blocks of ONE caller-owned [nenv][nq + nv + nsensordata] observation tensor -- the buffer an RCCL all-gather
 * sends as is; uploads / downloads of a strided field are 2-D copies */
int phys_batch_bind_strided(phys_batch_t *b, int field, void *device_ptr, int row_stride);
/* clears the sticky warning bits of envs [env0, env0 + n) (the batched cassie_sim_full_reset does this for the envs it
 * resets; mj_resetData clears mjData.warning the same way) */
int phys_batch_clear_warn(phys_batch_t *b, int env0, int n);
/* non-zero once PHYS_F_QFRC_APPLIED / PHYS_F_XFRC_APPLIED have been uploaded or bound (until then the kernel skips them) */
int phys_batch_uses_applied(const phys_batch_t *b);
/* mj_step1 + mj_step2, nsub times with ctrl held (reference :1130-1134), on `stream`
 * (a hipStream_t passed as void*, NULL = the batch's own stream); asynchronous.  The output fields (sensordata, qacc,
 * xpos / xquat, the measurement block, solver statistics) hold the values of the LAST of the nsub steps -- what nsub
 * single-step launches would leave; the state fields (qpos, qvel, time, warm start, drive-level state) advance nsub steps */
int phys_batch_step(phys_batch_t *b, int nsub, void *stream);
/* mj_forward (reference :971, :1029, :1223, :3293): no integration */
/* The same for the env range [env0, env0 + n) only.  Ranges of one batch may be in flight on different streams at once (the
 * per-env arrays are disjoint): stepping two half-batches on two streams, each at its own pace, lets one half's workgroups
 * fill the wave slots the other half leaves idle at the end and the start of its launches -- +16 % on BASELINE config 2
 *  when nothing joins the halves between policy steps. */
int phys_batch_step_range(phys_batch_t *b, int env0, int n, int nsub, void *stream);
int phys_batch_forward(phys_batch_t *b, void *stream);
/* Episode restarts without leaving the device -- the batched form of what a fresh cassie_sim_t / cassie_sim_full_reset
 * leaves (reference src/cassiemujoco.c:1023-1029, :2008-2034): envs first, first + stride, ... (count of them) get
 * qpos = qpos_row [nq] (DEVICE pointer), zero qvel / qacc_warmstart / ctrl / qacc / actuator_velocity / time and -- once a drive mode is in use -- a zero measurement block and zero drive-level state (encoder filter histories,
 * torque delay lines); sens_row [nsensordata] (device pointer or NULL) becomes their sensordata: the init pose's, which the
 * new episode's first drive-level pass reads.  The sticky warning word stays (phys_batch_clear_warn).  One small launch on
 * `stream`, ordered with the step launches there. */
int phys_batch_reset_envs(phys_batch_t *b, int first, int stride, int count, const double *qpos_row, const double *sens_row, void *stream);
/* Episodes that end and restart on the device, from each env's own state: one small launch per env range per policy step, no host
 * read anywhere (MuJoCo's auto-reset and a training loop's "done" logic at policy rate).
 *
 * phys_batch_episodes_enable allocates the per-env arrays (all zero) and sets the rules (cm_episode_rules_t, cm_model.h); calling it
 * again only replaces the rules.  The arrays, in HBM (phys_batch_episode_ptr; phys_batch_episode_bind puts caller-owned memory in
 * their place, e.g. a torch tensor the policy reads):
 *   PHYS_EP_DONE     int32 [nenv]           1 if the env's episode ended in the last phys_batch_end_episodes over it, else 0
 *   PHYS_EP_REASON   int32 [nenv]           OR of the CM_DONE_* bits that ended it (0 if it goes on)
 *   PHYS_EP_STEPS    int32 [nenv]           policy steps (end_episodes calls) of the running episode
 *   PHYS_EP_COUNT    int32 [nenv]           episodes ended so far
 *   PHYS_EP_TERMINAL double [nenv][nq + nv] qpos | qvel that ended the env's last episode (rows of envs that go on are left alone)
 *
 * phys_batch_end_episodes over envs [env0, env0 + n), per env and in this order:
 *   1. steps += 1;
 *   2. reason = OR of the rules that hold on the env's qpos, qvel, warning word and steps, | CM_DONE_FORCED if force && force[i] != 0
 *      (i = env - env0); done = reason != 0.  Both words are written for every env of the range;
 *   3. if done: terminal[env] = qpos | qvel, count += 1;
 *   4. if done && restart: the env becomes what a fresh batch holds after upload(qpos), upload(qvel), forward for bank row
 *      r = pick ? pick[i] mod nrows : (env + count) % nrows (count as step 3 left it): qpos | qvel | sensordata | actuator_velocity |
 *      qacc from the row; time, ctrl and warm start zero; the measurement block and the drive-level state zero once a drive mode
 *      is in use; the warning word cleared; steps = 0.
 * pick / force are DEVICE arrays [n] of int32 or NULL.  A bank row holds phys_batch_episode_row_dim doubles,
 * [nq | nv | nsensordata | nu | nv] in the order above: everything a forward pass leaves that a later step reads, and qacc.
 * phys_batch_episodes_set_bank copies host rows (on_device == 0; waits for the batch's streams) or uses device rows in place
 * (on_device != 0: caller-owned, must outlive their use, and may be rewritten in stream order).
 * The launch honours strided qpos / qvel / sensordata bindings, goes to `stream` (NULL: the batch's own) in order with the step
 * launches there, and never synchronises the host.  -1 + phys_last_error(): episodes not enabled, restart without a bank, range out
 * of bounds. */
enum { PHYS_EP_DONE, PHYS_EP_REASON, PHYS_EP_STEPS, PHYS_EP_COUNT, PHYS_EP_TERMINAL, PHYS_EP_ARRAYS };
int phys_batch_episodes_enable(phys_batch_t *b, const cm_episode_rules_t *rules);
int phys_batch_episodes_set_bank(phys_batch_t *b, const double *rows, int on_device, int nrows);
int phys_batch_episode_row_dim(const phys_batch_t *b);
void *phys_batch_episode_ptr(phys_batch_t *b, int which);
int phys_batch_episode_bind(phys_batch_t *b, int which, void *device_ptr);
int phys_batch_end_episodes(phys_batch_t *b, int env0, int n, int restart, const int *pick, const int *force, void *stream);
/* one whole episode array to the host (int32 [nenv], or double [nenv][nq + nv] for PHYS_EP_TERMINAL); waits for the batch's streams */
int phys_batch_download_episodes(phys_batch_t *b, int which, void *host);
size_t phys_sizeof_episode_rules(void);
/* A BANK OF FULL STATES: save, rewind and fork envs without leaving the device -- the batched form of cassie_get_state / cassie_set_state /
 * cassie_sim_copy / cassie_sim_duplicate (reference src/cassiemujoco.c).  Where phys_batch_end_episodes starts a NEW EPISODE from a row of
 * poses (time, warm start, ctrl, measurement block, filter histories and delay lines zero), a row of this bank is a STATE: after a
 * restore the env continues byte for byte as the env that was saved did.  Sampling-based planning fans one env out to K candidates every
 * policy step, a reset archive holds states the policy itself reached, a study rewinds, changes one thing and steps again.
 *
 * A ROW is phys_batch_state_row_dim 8-byte words; it and every section of it start on a 16-byte boundary (an odd section is followed by
 * one padding word, zero in a saved row).  A section holds the bytes of one per-env array as stored.  phys_batch_state_layout writes
 * [PHYS_SS_COUNT][2] ints, (offset, count) in words per section in the order of PHYS_SS_* (offset -1: not in this bank's rows) and
 * returns PHYS_SS_COUNT.  Groups (`groups` is an OR; CORE is always there):
 *   PHYS_STATE_CORE      every word a stepping launch writes and a later launch reads, or that a reader uses as stored: time, qpos, qvel,
 *                        qacc_warmstart, ctrl, qacc, sensordata, actuator_velocity (the next substep's drive-level pass reads the last
 *                        three), PHYS_F_MEAS, the whole cm_drive_state_t (filter histories, delay lines, safety_msg), PHYS_F_XPOS and
 *                        PHYS_F_XQUAT, the sticky warning word (32 bits, zero-extended).  THE POSES are in the row because the depth
 *                        image, the range sensors and phys_batch_derive take them AS STORED (the STALENESS paragraph of
 *                        phys_batch_depth_set_geoms): a restore that left them alone would show the robot where it was before the restore.
 *                        A section whose array the batch does not have at a save (the measurement block and the drive-level state until a
 *                        drive mode is selected) is written as zeros, and skipped at a restore while the batch still has none -- zero is what selecting
 *                        the mode later leaves, and what a restore after that puts there.
 *   PHYS_STATE_COMMANDS  PD_PTARGET, PD_KP, PD_KD, PD_DTARGET, PD_TORQUE, DRIVE_CMD, QFRC_APPLIED, XFRC_APPLIED.  Refused by the configure
 *                        call until both applied forces have been uploaded or bound: the step kernel is not handed them before, and a
 *                        restore would put them into nothing.
 *   PHYS_STATE_EPISODE   PHYS_EP_STEPS, PHYS_EP_COUNT and the env's terrain index (zero without a bank of terrains, and then not
 *                        restored).  Needs phys_batch_episodes_enable.
 *   PHYS_STATE_PARAMS    the env's cm_envparams_t block.  Needs per-env parameter blocks (phys_batch_randomize).  WITHOUT this group a
 *                        restored env keeps its own physics -- a legitimate use: the same state under other masses or friction.
 * NOT in a row: per-env height-field grids and per-env models, the outputs PHYS_F_BODY_CFRC / info / ext / PHYS_F_DERIVED / PHYS_F_QM /
 * the scan, depth and ray fields / PHYS_F_STEP_SUMS, PHYS_EP_DONE / _REASON / _TERMINAL, the placement arrays, and what the launcher
 * keeps per env for one launch or for speed alone (progress, chunk words, hand-over lists, launch order and cost: none changes a result).
 * Neither are the observation rows and their per-env frame counts (phys_batch_obs below): a caller that rewinds an env keeps or sets
 * them itself (phys_batch_obs_set_frames; a refill entry refills the env's history from its restored state).  Nor are the running and
 * final returns of the reward rows (phys_batch_reward below: phys_batch_reward_returns / _set_returns), nor the state of the event rows
 * (phys_batch_events below: phys_batch_events_state / _set_state).
 *
 *   phys_batch_state_configure  allocates a bank of nslots >= 1 zeroed rows in HBM; waits for the batch's streams; calling it again
 *                               replaces the bank (and drops a binding).
 *   phys_batch_state_bind       caller-owned device memory [nslots][row_dim] of 8-byte words, 16-byte aligned, in the bank's place
 *                               (a torch int64 tensor); configure first (it fixes the groups); NULL un-binds: the batch's own bank again.
 *   phys_batch_state_save       over envs [env0, env0 + n): env env0 + i goes to slot slots[i] (`slots`: a DEVICE int32 [n]; NULL: slot
 *                               env0 + i).  A negative slot skips the env; a slot >= nslots skips it and raises bit 256 of the env's
 *                               warning word (WARN_STATE_SLOT).  Two envs saving to one slot in one call is a caller error: that slot
 *                               alone is unspecified.
 *   phys_batch_state_restore    env env0 + i takes slot slots[i]; negative: the env is left alone; out of range: left alone, bit 256
 *                               raised; any number of envs may take the same slot.  The warning word is the row's afterwards.
 *                               Both are one small launch on `stream` (NULL: the batch's own), in order with the stepping launches there,
 *                               honour strided qpos / qvel / sensordata bindings and never synchronise the host.  A FORK is a save
 *                               followed by a restore on the same stream.  -1 + phys_last_error(): not configured, range out of bounds,
 *                               something a group needs gone since the configure call.
 *   phys_batch_state_download / _upload   rows [slot0, slot0 + n) to / from host memory; both wait for the batch's streams.  An upload
 *                               names the signature its rows came with and is refused unless it is this batch's:
 *   phys_batch_state_signature  a hash of the layout version, the groups, the row dim and the batch's compiled shared model (sizes,
 *                               options, body tree, reference pose, masses, geoms): what keeps rows saved by one process out of another
 *                               model.  0 while not configured. */
enum { PHYS_STATE_CORE = 1, PHYS_STATE_COMMANDS = 2, PHYS_STATE_EPISODE = 4, PHYS_STATE_PARAMS = 8 };
enum { PHYS_SS_TIME, PHYS_SS_QPOS, PHYS_SS_QVEL, PHYS_SS_QACC_WARMSTART, PHYS_SS_CTRL, PHYS_SS_QACC, PHYS_SS_SENSORDATA, PHYS_SS_ACTUATOR_VELOCITY,
       PHYS_SS_MEAS, PHYS_SS_DRIVE_STATE, PHYS_SS_XPOS, PHYS_SS_XQUAT, PHYS_SS_WARN,
       PHYS_SS_PD_PTARGET, PHYS_SS_PD_KP, PHYS_SS_PD_KD, PHYS_SS_PD_DTARGET, PHYS_SS_PD_TORQUE, PHYS_SS_DRIVE_CMD, PHYS_SS_QFRC_APPLIED, PHYS_SS_XFRC_APPLIED,
       PHYS_SS_EP_STEPS, PHYS_SS_EP_COUNT, PHYS_SS_TERRAIN, PHYS_SS_PARAMS, PHYS_SS_COUNT };
int phys_batch_state_configure(phys_batch_t *b, int nslots, int groups);
int phys_batch_state_bind(phys_batch_t *b, void *device_ptr, int nslots);
void *phys_batch_state_ptr(phys_batch_t *b);
int phys_batch_state_nslots(const phys_batch_t *b);
int phys_batch_state_groups(const phys_batch_t *b);
int phys_batch_state_row_dim(const phys_batch_t *b);
int phys_batch_state_layout_version(void);
int phys_batch_state_layout(const phys_batch_t *b, int *offsets_counts);
unsigned long long phys_batch_state_signature(const phys_batch_t *b);
int phys_batch_state_save(phys_batch_t *b, int env0, int n, const int *slots, void *stream);
int phys_batch_state_restore(phys_batch_t *b, int env0, int n, const int *slots, void *stream);
/* a convenience outside the hot loop: copies a HOST int32 [n] of slots into a buffer of the batch's and returns its device pointer, for
 * the next save or restore (waits for the batch's streams first: the buffer is reused by the next call); NULL on failure */
void *phys_batch_state_stage_slots(phys_batch_t *b, const int *host_slots, int n);
int phys_batch_state_download(phys_batch_t *b, int slot0, int n, void *host);
int phys_batch_state_upload(phys_batch_t *b, int slot0, int n, const void *host, unsigned long long signature);
/* PLACED RESTARTS: a restarted env is put down at a pose of its own, on the ground it finds there -- a curriculum's envs no longer all
 * restart at the row's spot and heading, a terrain (or a stair box moved under the spawn point) no longer buries or drops the robot,
 * and the env's NEXT terrain is chosen inside the restart, which can therefore see the ground it is about to stand on.  Still one
 * launch per env range per policy step, no host read.
 *
 * phys_batch_place_configure(b, anchor, offsets_xy, npoints, ground_ref), once per batch (it waits for the batch's streams, like
 * phys_batch_scan_configure; anchor <= 0 turns placement off again):
 *   anchor        a body that is a child of the world and whose pose follows from qpos alone (the height scan's restriction:
 *                 Cassie's pelvis);
 *   offsets_xy    a footprint o[npoints][2], 0 <= npoints <= 1024, host memory; npoints == 0: no ground following;
 *   ground_ref    the world z of the ground the bank's rows were recorded on.
 * Per-env arrays in HBM, indexed by the absolute env, the batch's own (phys_batch_place_ptr) or a caller's (phys_batch_place_bind; NULL
 * un-binds), handled like the episode arrays:
 *   PHYS_PLACE_POSE          double [nenv][4] = (dx, dy, dz, yaw)   input; the batch's own array starts as zeros
 *   PHYS_PLACE_NEXT_TERRAIN  int32  [nenv]                          optional input: used only while bound and a bank of terrains is set
 *                                                                   (the batch has none of its own: NULL = unused)
 *   PHYS_PLACE_GROUND        double [nenv]                          output: the ground height G found at the env's last placed restart
 *
 * With placement configured, step 4 of phys_batch_end_episodes -- the restart of an env that ended; `row` is the bank row step 4 picks
 * -- becomes:
 *   1. Terrain.  If a next-terrain array is bound (and a bank is set): index[env] = clamp(next[env], 0, nterrain - 1); an id outside the
 *      bank raises WARN_TERRAIN_INDEX.  The step launches queued behind on the stream read the new index.  (With no array bound the
 *      index stays; if the ground lookup of step 3 has to clamp it, that raises the bit as well.)
 *   2. Anchor.  a = (ax, ay): the anchor's world x, y in the row (its pose from the row's qpos, as the scan computes it, the joint
 *      quaternion normalised); psi its heading by the scan's formula, atan2(2 (w z + x y), 1 - 2 (y y + z z)).
 *   3. Ground.  The footprint's world points are F_j = (ax + dx, ay + dy) + Rz(psi + yaw) o_j: the heading frame of the anchor AFTER
 *      placement, the height scan's own convention.  G = max_j S(F_j) over the points that hit, S exactly the height scan's surface
 *      (phys_batch_height_scan above): static planes, boxes and the height field; the env's own geom poses once geometry is
 *      randomised; the env's terrain grid after step 1; a tilted height-field geom is left out and raises WARN_SCAN_TILTED.  If no
 *      point hits, or npoints == 0, G = ground_ref; with npoints > 0 and no hit, bit 128 of the warning word (WARN_PLACE_MISS) is
 *      raised too.  PHYS_PLACE_GROUND[env] = G.
 *   4. Rigid motion.  T(p) = p + (dx, dy, h) + (Rz(yaw) - I)(p - (ax, ay, p_z)), h = dz + G - ground_ref: a turn by yaw about the
 *      vertical through the anchor, then a shift.  Every MOVING ROOT body (a child of the world with at least one joint: the pelvis,
 *      and the cube of cassie_tray_box.xml) gets T applied to its world pose in the row: position T(p), quaternion Qz(yaw) (x) q,
 *      Qz(yaw) = (cos yaw/2, 0, 0, sin yaw/2), q the body's joint quaternion as the row has it (not normalised).  Only the joint
 *      coordinates of those roots change; every other qpos entry is the row's.  A moving root must have a free joint, or three slides
 *      along the world's x, y and z (one each) followed by a ball at the body's origin, the body frame the world's at qpos0 (the pelvis
 *      of all three models) -- the make-ups whose joint coordinates can take ANY world pose; anything else makes the configure call
 *      fail with -1 and a phys_last_error() message.
 *   5. qvel and qacc.  The linear entries of those roots are world-frame vectors and are turned by Rz(yaw): the free joint's first
 *      three entries, or the slides' velocities taken together as a vector.  Angular entries (ball or free: body-local) and everything
 *      else are the row's.
 *   6. sensordata.  framequat becomes Qz(yaw) (x) value; magnetometer becomes R_s'^T B, clamped at the sensor's cutoff as the step
 *      does, R_s' the rotation of Qz(yaw) (x) (bq_row (x) sensor_squat), bq_row the world quaternion of the sensor's body in the row, B
 *      the model's magnetic field -- for yaw != 0; a yaw of exactly 0 turns no frame and leaves the row's words.  Both need the
 *      sensor's site on a moving root body (configure fails with -1 otherwise; at most eight such sensors).  Every other entry is the
 *      row's: joint and actuator positions, gyro, accelerometer, rangefinder.  THE ACCELEROMETER, QACC (up to the turn of step 5) AND THE
 *      RANGEFINDERS ARE THEREFORE THOSE OF THE GROUND THE ROW WAS RECORDED ON, contact forces included; the first substep replaces
 *      them.  The rest of step 4 is unchanged: time, ctrl, warm start zero; measurement block and drive-level state zero once a drive
 *      mode is in use; steps = 0.
 *   7. Warning word: cleared as before, then the bits of steps 1 and 3 are set.
 * IDENTITY: the pose (0, 0, 0, 0) with npoints == 0 leaves exactly what an unplaced restart leaves (as compared with ==: -0.0 may
 * stand for 0.0) -- the turn is applied as (Rz(yaw) - I), which adds exact zeros at yaw = 0.  A batch that never configures placement
 * runs phys_batch_end_episodes exactly as before, with the same kernel; so does a call with restart == 0.
 * Not done: roll and pitch are not aligned to a slope, the legs are not bent to the ground, per-env MODELS (phys_batch_set_model with
 * env >= 0) are refused, by the configure call and by phys_batch_end_episodes. */
enum { PHYS_PLACE_POSE, PHYS_PLACE_NEXT_TERRAIN, PHYS_PLACE_GROUND, PHYS_PLACE_ARRAYS };
int phys_batch_place_configure(phys_batch_t *b, int anchor, const double *offsets_xy, int npoints, double ground_ref);
void *phys_batch_place_ptr(phys_batch_t *b, int which);
int phys_batch_place_bind(phys_batch_t *b, int which, void *device_ptr);
/* host rows [n] of a placement array (4 doubles, 1 int32 or 1 double each) into envs [env0, env0 + n) of the array in use, and one whole
 * array to the host; both wait for the batch's streams.  -1 for PHYS_PLACE_NEXT_TERRAIN while none is bound. */
int phys_batch_place_upload(phys_batch_t *b, int which, const void *host, int env0, int n);
int phys_batch_place_download(phys_batch_t *b, int which, void *host);
/* the read-out half of mj_forward -- what the reference's getters obtain from mj_kinematics / mj_comPos / mj_comVel /
 * mj_fwdPosition (reference src/cassiemujoco.c:1223-1301, :1604-1770): xpos / xquat / the ext read-out / body_cfrc of the
 * current state, while the fields qacc, sensordata and actuator_velocity keep what the last STEP left (the encoder and
 * motor models of the next step read those) */
int phys_batch_forward_kinematics(phys_batch_t *b, void *stream);
int phys_batch_sync(phys_batch_t *b);
/* on != 0: every substep computes ctrl on the device from PHYS_F_PD_{PTARGET,KP,KD} -- the motor PD law of
 * pd_input_step (reference include/pd_input.h:34) followed by the speed-torque limit of motor()
 * (reference src/cassiemujoco.c:638-664), evaluated on the exact joint state; PHYS_F_CTRL is then ignored */
int phys_batch_set_pd_mode(phys_batch_t *b, int on);
/* Drive-level I/O on the device: with mode != CM_DRIVE_OFF every substep first runs
 * cassie_motor_data + cassie_sensor_data (reference src/cassiemujoco.c:737-803: encoder quantisation, integer FIR / IIR
 * velocity filters, motor speed-torque curve, STO, six-cycle torque delay) for every env, bit for bit the host chain,
 * on the sensordata / actuator_velocity the previous step left in HBM, writes PHYS_F_MEAS and takes ctrl from the
 * delay line.  CM_DRIVE_TORQUE reads the command from PHYS_F_DRIVE_CMD (cassie_sim_step_ethercat semantics);
 * CM_DRIVE_PD computes it as torque + kp (ptarget - position) + kd (dtarget - velocity) on the measured drive
 * position / velocity of the previous step (pd_input_step's motor PD, reference include/pd_input.h:34); CM_DRIVE_PD_SAFE
 * passes that command through cassie_core_sim's safety layer first (reference include/cassie_core_sim.h:34, called at
 * src/cassiemujoco.c:1141: joint-limit attenuation and restoring torques, torque-limit clamp, STO -- restated in
 * csrc/pk_safety.h bit for bit the closed binary), i.e. the whole torque path of cassie_sim_step_pd; the STO switch (radio
 * channel 8) is the last word of PHYS_F_DRIVE_CMD, the block's diagnostic messages collect in cm_drive_state_t::safety_msg.  The filter
 * histories and delay lines live in HBM (one cm_drive_state_t per env, zero-initialised like a fresh cassie_sim_t). */
int phys_batch_set_drive_mode(phys_batch_t *b, int mode);
/* the drive-level pass alone (no physics), whatever the drive mode of the step kernel is: reads PHYS_F_DRIVE_CMD (mode
 * CM_DRIVE_TORQUE) or the PD fields (CM_DRIVE_PD), PHYS_F_SENSORDATA and PHYS_F_ACTUATOR_VELOCITY; writes PHYS_F_CTRL,
 * PHYS_F_MEAS and the drive state.  Follow it with phys_batch_step in CM_DRIVE_OFF mode: together the two launches are
 * one cassie_sim_step_ethercat, and the measurements can travel to the host while the physics runs. */
int phys_batch_drive_pass(phys_batch_t *b, int mode, void *stream);
/* a marker on the batch's stream and a host wait for it (everything queued before the marker has completed) */
int phys_batch_mark(phys_batch_t *b);
int phys_batch_wait_mark(phys_batch_t *b);
/* zeroes the drive state (a fresh cassie_sim_t's filters and delay lines) of envs first, first + stride, ... (count of
 * them), asynchronously on `stream` (NULL = the batch's own): episode restarts of a device-resident rollout */
int phys_batch_clear_drive_state(phys_batch_t *b, int first, int stride, int count, void *stream);
int phys_batch_upload_drive_state(phys_batch_t *b, const cm_drive_state_t *host, int env0, int n);
int phys_batch_download_drive_state(phys_batch_t *b, cm_drive_state_t *host, int env0, int n);

/* times `reps` launches of nsub steps with HIP events on the launch stream; returns mean ms per launch */
int phys_batch_time_steps(phys_batch_t *b, int nsub, int reps, float *mean_ms);

/* extended per-env outputs (cm_ext_t: contacts + contact forces, body velocities, site frames, com): enable once,
 * then every step/forward refreshes them in HBM; download copies envs [env0, env0 + n) to the host */
int phys_batch_enable_ext(phys_batch_t *b, int on);
int phys_batch_download_ext(phys_batch_t *b, cm_ext_t *host, int env0, int n);
int phys_batch_download_ext_async(phys_batch_t *b, cm_ext_t *host, int env0, int n); /* pair with phys_batch_sync */

/* Batched derived getters: one forward pass (mj_forward role: nothing is integrated) that leaves the
 * full read-out of every env in HBM, then a small kernel that reduces it to PHYS_F_DERIVED -- whole-model centre of
 * mass / velocity / angular momentum, foot positions / velocities, foot and heel / toe contact forces, the feet's
 * Jacobians -- and PHYS_F_QM, i.e. what cassie_sim_cm_position / cm_velocity / angular_momentum / foot_positions /
 * foot_velocities / foot_forces / heeltoe_forces / get_jacobian_full / full_mass_matrix return for one simulator
 * (reference src/cassiemujoco.c:1254-1301, :1604-1712, :1812-1898), for every env, as device fields (bindable).
 * ids = {left foot body, right foot body, left heel site, right heel site, left toe site, right toe site}, -1 = absent.
 * The forces are those of the CURRENT state (like after cassie_sim_forward).  Costs about one physics step. */
int phys_batch_derive(phys_batch_t *b, const int ids[6], void *stream);

/* PROBES: the reference's reward-side getters for ANY body or site, for an env range, on the caller's stream.  A probe is a point fixed
 * in the frame of a body (the body's xpos / xquat) or of a site (site_xpos / site_xmat of the read-out; its body is site_bodyid): with x, R
 * the frame, the probe's point is p = x + R offset.  A configured list of up to PHYS_PROBES_MAX of them is evaluated by phys_batch_probe
 * into one row of PHYS_F_PROBES per env; all values are in world axes, and each is the arithmetic of the single-simulator getter named:
 *   PHYS_PQ_POS   3       p (offset 0: cassie_sim_xpos / cassie_sim_site_xpos)
 *   PHYS_PQ_QUAT  4       body: the body's xquat; site: the quaternion of site_xmat by the routine and sign convention of cassie_sim_site_xquat
 *   PHYS_PQ_VEL   6       [w; v_p]: w = cvel[body][0:3], v_p = cvel[body][3:6] + w x (p - subtree_com[body_rootid[body]]): the velocity of
 *                         the point itself
 *   PHYS_PQ_CVEL  6       cvel[body] as it is (cassie_sim_body_velocities)
 *   PHYS_PQ_ACC   6       cassie_sim_body_acceleration of the probe's body: sum over the body's dofs of cdof_dot[k] qvel[k] + cdof[k] qacc[k],
 *                         plus -gravity in the linear part, with the forward pass's qacc
 *   PHYS_PQ_JACP, _JACR   3 x nv each, row-major [3][nv]: the Jacobians of the point p moving with the body (offset 0 on a body:
 *                         cassie_sim_get_jacobian_full; on a site: cassie_sim_get_jacobian_full_site); zero for the world body
 *   PHYS_PQ_CFRC  3       the summed contact force on the probe's body: cassie_sim_body_contact_force(...)[0:3] with its sign
 * PHYS_PQ_CONTACTS adds one int32 word per ENV (not per probe, not in the row): bit 0 cassie_sim_check_obstacle_collision, bit 1
 * cassie_sim_check_self_collision, bit 8 + g (g = 0 .. 5) cassie_sim_geom_collision(g).  These read geom_user[0] and geom_group of the
 * host model's FULL geom list, which the compiled model a batch is created from does not carry: hand the host model over once with
 * phys_batch_probe_geom_classes, before configuring with PHYS_PQ_CONTACTS (the table it builds lives in device memory; it outlives
 * reconfigurations).
 * ROW LAYOUT: quantity-major -- for every quantity of the mask, in bit order, a block [nprobes][doubles per probe], nothing between the
 * blocks (a tensor view rows[:, off : off + nprobes * dim] reshapes to [n, nprobes, dim]); phys_batch_probe_layout reports the offsets.
 *   phys_batch_probes_configure  probes [nprobes] (host memory), the quantities (an OR of PHYS_PQ_*, not empty).  Checks every kind, a body
 *                               id in [0, nbody), a site id in [0, min(nsite, CM_MAXSITE)), finite offsets.  Allocates everything the
 *                               feature ever needs: the table, the rows (PHYS_F_PROBES takes their size in a buffer of the batch's own:
 *                               bind a tensor AFTER configuring; phys_batch_bind_strided takes a row stride for this field), the contact
 *                               words, and a read-out block of the probes' OWN, sizeof(cm_ext_t) * nenv -- 34 104 bytes per env, 140 MB at
 *                               4096 envs -- with the scratch outputs of the probes' forward pass ((2 nv + nsensordata + nu + 7 nbody) doubles
 *                               per env).  Stepping launches never see that block: their kernels and rates are what they were, and a
 *                               caller's phys_batch_enable_ext is neither needed nor disturbed.  Waits for the batch's streams.
 *                               Reconfiguring is allowed (it drops the bindings of the rows and of the contact words); nprobes 0 releases
 *                               everything.  -1 + phys_last_error() on failure.
 *   phys_batch_probe            enqueues, on `stream` (NULL: the batch's own), one forward pass (nothing is integrated) over
 *                               [env0, env0 + n) that writes the probes' read-out block and scratch outputs ONLY, and behind it
 *                               cassie_probe_kernel over the same range.  No host synchronisation, no allocation.  Everything else a
 *                               caller can read stays byte for byte: qpos, qvel, time, qacc, qacc_warmstart, sensordata,
 *                               actuator_velocity, ctrl, xpos / xquat, body_cfrc, the solver statistics, the drive-level state, the
 *                               episode words, the step sums -- but for the sticky warning bits a forward pass of the state raises anyway.
 *                               Works in every drive mode: the forward pass applies the ctrl last applied and does not advance filter
 *                               histories or delay lines.  Ranges on different streams may be probed concurrently: each touches its own
 *                               rows.  An env whose state fails the step kernel's divergence test (NaN, or beyond 1e10) gets a row of
 *                               NaN and a contact word of 0.
 *   phys_batch_probe_row_dim    doubles in a row (0: not configured).
 *   phys_batch_probe_layout     offsets [PHYS_PQ_COUNT] (-1: the quantity is absent) and dims [PHYS_PQ_COUNT] (doubles per probe), either
 *                               may be NULL -> nprobes, -1 when not configured.
 *   phys_batch_probe_contacts_ptr / _bind_contacts  the contact words, int32 [nenv] in device memory indexed by the absolute env: the
 *                               batch's own (NULL unless configured with PHYS_PQ_CONTACTS), or a caller's (NULL: the batch's own again).
 *   phys_batch_debug_probe_launches  diagnostics: the forward passes and the reductions phys_batch_probe has launched. */
enum { PHYS_PROBE_BODY = 0, PHYS_PROBE_SITE = 1 };
typedef struct phys_probe { int kind, id; double offset[3]; } phys_probe_t;   /* offset: in the body's / site's own frame */
#define PHYS_PROBES_MAX 32
enum { PHYS_PQ_POS = 1, PHYS_PQ_QUAT = 2, PHYS_PQ_VEL = 4, PHYS_PQ_CVEL = 8, PHYS_PQ_ACC = 16, PHYS_PQ_JACP = 32, PHYS_PQ_JACR = 64,
       PHYS_PQ_CFRC = 128, PHYS_PQ_CONTACTS = 256, PHYS_PQ_COUNT = 8 /* the quantities of a row */ };
enum { PHYS_PC_OBSTACLE = 1, PHYS_PC_SELF = 2, PHYS_PC_GROUP0 = 256 /* << g, g = 0 .. 5 */ };
int phys_batch_probes_configure(phys_batch_t *b, const phys_probe_t *probes, int nprobes, unsigned quantities);  /* nprobes 0: release */
int phys_batch_probe_geom_classes(phys_batch_t *b, const phys_model_t *host_model);   /* for PHYS_PQ_CONTACTS; NULL drops the table */
int phys_batch_probe(phys_batch_t *b, int env0, int n, void *stream);
int phys_batch_probe_row_dim(const phys_batch_t *b);
int phys_batch_probe_layout(const phys_batch_t *b, int *offsets /*[PHYS_PQ_COUNT], -1 = absent*/, int *dims);
void *phys_batch_probe_contacts_ptr(phys_batch_t *b);
int phys_batch_probe_bind_contacts(phys_batch_t *b, void *device_ptr);     /* int32 [nenv], NULL unbinds */
int phys_batch_probe_download_contacts(phys_batch_t *b, int *host);        /* the words [nenv] to the host, after waiting for the batch's streams */
int phys_batch_debug_probe_launches(const phys_batch_t *b, long long *forward, long long *reduce);

/* OBSERVATION ROWS: the row a policy network reads, made on the device from the batch's fields by ONE launch per env range: gather,
 * offset, uniform noise, scale, clip, the cast to the rows' type and a per-env history of frames.  A configured list of TERMS makes the
 * columns of a FRAME, term after term; an env's ROW is [history][ncols] with frame 0 the newest.
 * TERMS (phys_obs_term_t):
 *   PHYS_OBS_COPY     count columns; column j's source is x = field_row[index + j].
 *   PHYS_OBS_ROT_INV  3 columns: x = R(q)^T v, with q the four doubles qfield_row[qindex .. qindex + 3] AS STORED (not normalised) and v
 *                     the three doubles field_row[index .. index + 2], or the term's vec where field == PHYS_OBS_CONST.  R(q) is the matrix
 *                     of a quaternion (w, x, y, z) as the step kernel forms it, m = [q00+q11-q22-q33, 2(q12-q03), 2(q13+q02); 2(q12+q03),
 *                     q00-q11+q22-q33, 2(q23-q01); 2(q13-q02), 2(q23+q01), q00-q11-q22+q33] with qij = q[i] q[j], and x[k] = (m[k] v[0] +
 *                     m[3 + k] v[1]) + m[6 + k] v[2]; every product and every sum is rounded on its own, left to right as written (no
 *                     fused multiply-add).  vec = (0, 0, -1) with q = qpos[3:7] is the projected gravity; v = qvel[0:3] the base velocity
 *                     in the body frame; v from the input a heading-relative command.  count is ignored.
 *   field / qfield    any PHYS_F_* field but PHYS_F_DEPTH, with the row length the batch holds for it when the terms are configured (a field
 *                     that is sized later -- the scan, the rays, the probes, the step sums, the derived block -- must have been
 *                     configured or enabled before), or PHYS_OBS_INPUT: the caller's own per-env array (commands, a clock phase, the
 *                     previous action), bound with phys_batch_obs_bind_input as floats or doubles; floats are widened exactly.  A field is
 *                     read where the batch reads it at the call: its own buffer, or the caller's bound tensor with its row stride.
 * A COLUMN'S VALUE, every step one individually rounded fp64 operation:
 *       e = x - offset;   if (noise != 0) e = e + noise * xi;   y = e * scale;   y = y < lo ? lo : (y > hi ? hi : y)   (a NaN passes)
 *   and the element written is y, or (float)y rounded to nearest even where the rows are PHYS_OBS_F32.
 * NOISE: xi is uniform on (-1, 1), xi = (w + 0.5) 2^-31 - 1 (exact in fp64) with w word 0 of Philox4x32-10 (Salmon et al., SC 2011;
 *   multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) on the counter (env_base + env, column, frames[env], 0)
 *   -- column: the column's index in the frame; env_base + env modulo 2^32 -- with the key (seed & 0xffffffff, seed >> 32).  A draw depends
 *   on the env, the column and the number of calls the env has seen, never on how the batch is cut into ranges, streams or ranks: a rank
 *   that holds envs [k n, (k + 1) n) of a larger run and configures env_base = k n draws what one batch would draw for those envs.
 * HISTORY: a call over an env first forms the new frame.  If frames[env] == 0 or the call's refill entry for the env is non-zero, every
 *   frame of the row becomes the new frame; otherwise frame h takes frame h - 1 for h = history - 1 .. 1 and frame 0 the new one.  Then
 *   frames[env] += 1 (uint32, wraps).  refill: an optional int32 DEVICE array [n], entry i for env env0 + i -- the range's slice of
 *   PHYS_EP_DONE after phys_batch_end_episodes restarts the history of the envs it restarted.
 * LIMITS: PHYS_OBS_MAXCOLS columns in a frame, 1 .. 64 frames, a row of at most 65536 elements, 16 distinct sources.
 *   phys_batch_obs_configure    terms [nterms] (host memory), the frames of a row, the rows' type (PHYS_OBS_F32 / PHYS_OBS_F64), the seed
 *                               and env_base.  Refuses, with a message in phys_last_error(): an unknown kind or field, PHYS_F_DEPTH, a
 *                               field the batch does not hold yet, index + count / index + 3 / qindex + 4 beyond the field's row,
 *                               PHYS_OBS_CONST anywhere but in a ROT_INV's field, a non-finite offset, scale, noise or vec, noise < 0,
 *                               lo > hi (infinities are allowed), too many columns, a history outside 1 .. 64, an unknown dtype.
 *                               Allocates the column table, the rows and frames (zeroed); drops the bindings of the rows and of the input;
 *                               waits for the batch's streams.  nterms 0 releases everything.
 *   phys_batch_obs_bind         the rows in caller-owned HBM, of the configured type, row_stride elements (>= the row's) between two envs'
 *                               rows: a column block of the tensor an all-gather sends.  NULL: the batch's own rows again, zeroed.
 *   phys_batch_obs_bind_input   the caller's per-env array [nenv] rows of dim elements, row_stride elements apart, PHYS_OBS_F32 / _F64.
 *                               NULL un-binds.
 *   phys_batch_obs              ONE launch of cassie_obs_kernel over [env0, env0 + n) on `stream` (NULL: the batch's own), in order with
 *                               the launches there.  No host synchronisation, no allocation, no read on the host.  Writes the rows and
 *                               frames of the range and nothing else.  Refuses: not configured, a range outside the batch, a source field
 *                               whose row length is no longer what it was at the configure call, a PHYS_OBS_INPUT term with nothing bound
 *                               or with a bound dim that its terms reach beyond.
 *   phys_batch_obs_dim          ncols, history and the row's elements (any may be NULL) -> 0, -1 when not configured.
 *   phys_batch_obs_layout       first_col [nterms]: every term's first column -> nterms, -1 when not configured.
 *   phys_batch_obs_download     rows [env0, env0 + n) to dense host memory [n][history][ncols] of the rows' type; waits for the streams.
 *   phys_batch_obs_frames / _set_frames   the counts [nenv] (uint32) to / from the host, so that a resumed run draws what the first would
 *                               have drawn; both wait for the streams.
 *   phys_batch_debug_obs_launches  diagnostics: the launches phys_batch_obs has made. */
enum { PHYS_OBS_COPY = 0, PHYS_OBS_ROT_INV = 1 };
enum { PHYS_OBS_INPUT = -1, PHYS_OBS_CONST = -2 };   /* a term's field, beside PHYS_F_* */
enum { PHYS_OBS_F32 = 4, PHYS_OBS_F64 = 8 };         /* a dtype: the bytes of an element */
#define PHYS_OBS_MAXCOLS 2048
typedef struct phys_obs_term {
    int kind, field, index, count, qfield, qindex;
    double vec[3];
    double offset, scale, noise, lo, hi;
} phys_obs_term_t;
int phys_batch_obs_configure(phys_batch_t *b, const phys_obs_term_t *terms, int nterms, int history, int dtype, unsigned long long seed,
                             unsigned env_base);   /* nterms 0: release */
int phys_batch_obs_bind(phys_batch_t *b, void *device_ptr, long long row_stride);   /* NULL un-binds */
int phys_batch_obs_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype);   /* NULL un-binds */
int phys_batch_obs(phys_batch_t *b, int env0, int n, const void *refill_ptr /* int32 [n] or NULL */, void *stream);
int phys_batch_obs_dim(const phys_batch_t *b, int *ncols, int *history, int *row);
int phys_batch_obs_layout(const phys_batch_t *b, int *first_col /*[nterms]*/);
int phys_batch_obs_download(phys_batch_t *b, void *host, int env0, int n);
int phys_batch_obs_frames(phys_batch_t *b, unsigned *host /*[nenv]*/);
int phys_batch_obs_set_frames(phys_batch_t *b, const unsigned *host /*[nenv]*/);
int phys_batch_debug_obs_launches(const phys_batch_t *b, long long *launches);

/* REWARD ROWS: the scalar a training loop hands its policy for a step, made on the device by ONE launch per env range from a configured
 * table of at most PHYS_REW_MAXTERMS TERMS: per env the reward, optionally every term's contribution, and the running return of the
 * env's episode.  Every arithmetic step below is one individually rounded fp64 operation (multiply, add, subtract, divide, square root
 * to nearest even; no fused multiply-add, no reassociation), and every sum is sequential from +0.0 in index order: the device, the wave
 * emulator and a numpy restatement agree on every bit, so a reward can be replayed, rewound with the state bank and compared across ranks.
 * SOURCES are the observation's: field / qfield / tfield / gfield name any PHYS_F_* field but PHYS_F_DEPTH, with the row length the batch
 *   holds for it when the terms are configured (a field that is sized later must have been configured or enabled before), read where the
 *   batch reads it at the call (its own buffer, or the caller's bound tensor with its row stride); or PHYS_REW_INPUT, the caller's own
 *   per-env array bound with phys_batch_reward_bind_input as floats or doubles, floats widened exactly: commands, a reference pose for
 *   this step, clock coefficients, the previous and current action.  It may be the tensor bound as the observation's input.  At most 16
 *   distinct sources.
 * A TERM (phys_reward_term_t) makes ELEMENTS x[j] by its kind:
 *   PHYS_REW_VEC      x[j] = field_row[index + j], j < count, 1 <= count <= 64.
 *   PHYS_REW_ROT_INV  three elements, x = R(q)^T v exactly as PHYS_OBS_ROT_INV forms it above: q the four values qfield_row[qindex ..
 *                     qindex + 3] as stored, v = field_row[index .. index + 2], or vec[0 .. 2] where field == PHYS_REW_CONST (the base
 *                     velocity in the body frame against a commanded one).  count is ignored.
 *   PHYS_REW_QUAT     four values q = field_row[index .. index + 3] and four t = tfield_row[tindex .. tindex + 3], or vec[0 .. 3] where
 *                     tfield == PHYS_REW_CONST, both as stored: d = ((q0 t0 + q1 t1) + q2 t2) + q3 t3 and s = 1 - d d.  This kind skips
 *                     the errors, the norm and the root below (count, target, dead, norm and root are ignored).
 *   ERRORS (VEC, ROT_INV)  e[j] = x[j] - t[j], with t[j] = target where tfield == PHYS_REW_CONST, else tfield_row[tindex + j].  Where
 *                     dead > 0: m = |e[j]| - dead; e[j] = m < 0 ? 0 : m (a compare and a select: a NaN passes).
 *   NORM              PHYS_REW_SUMSQ: s = sum_j e[j] e[j];  PHYS_REW_SUMABS: s = sum_j |e[j]|;  PHYS_REW_MAXABS: s = +0.0, then for every j
 *                     in order  if (|e[j]| > s) s = |e[j]|  (a NaN element is passed over).  Where root != 0: s = sqrt(s).
 *   SHAPE             PHYS_REW_LINEAR: v = s;  PHYS_REW_EXP: v = expn(k s);  PHYS_REW_RATIONAL: v = 1 / (1 + k s).
 *   CONTRIBUTION      c = weight v; where gfield != PHYS_REW_NONE: c = c gfield_row[gindex] (a clock coefficient of the input, a touch
 *                     count of the step sums).
 * THE REWARD: r = sum_t c_t in term order; then r = r < lo ? lo : (r > hi ? hi : r) with the configured bounds (infinities are allowed; a
 *   NaN passes).  The element written is r, or (float)r rounded to nearest even where the rewards are PHYS_OBS_F32; the optional TERM ROWS
 *   [nenv][nterms] take c_t with the same cast.
 * RETURNS, always fp64: the call takes an optional int32 DEVICE array reset[n], entry i for env env0 + i.  An env whose entry is non-zero
 *   first does  final[env] = ret[env]; ret[env] = +0.0;  then every env of the range does  ret[env] = ret[env] + r  (the clipped r,
 *   before the cast).
 * ORDER IN A POLICY STEP: the step launch; the launches that make sources (probe, rays, scan); phys_batch_reward;
 *   phys_batch_end_episodes; phys_batch_obs.  The reward must see the state that ENDED an episode, not the restarted one, so it runs in
 *   front of phys_batch_end_episodes, and `reset` is the range's slice of PHYS_EP_DONE as the PREVIOUS policy step's
 *   phys_batch_end_episodes left it (the words hold until the next one on that stream): the reward of an episode's last step is added to
 *   its return, and the next call moves that return to `final`.  A termination bonus is the caller's one statement on r and the done
 *   words.  ret and final are not in a state-bank row: as with the observation's frame counts, a caller that rewinds an env keeps or sets
 *   them itself (phys_batch_reward_returns / _set_returns).
 * NaN AND DIVERGED ENVS: values flow through to the env's own reward, term row and return; nothing indexes memory by a value.
 * expn(a) ~ exp(-a), a = k s, k >= 0 finite:
 *   1. a NaN gives NaN.
 *   2. a > 708 gives +0.0 (the smallest result of the branch below is normal: no result depends on the denormal mode); a < -708 -- only a
 *      QUAT term of quaternions far from unit length gets there -- gives +inf.
 *   3. n = rint(a * 1.44269504088896338700e+00), to nearest even.
 *   4. rho = (a - n * 6.93147180369123816490e-01) - n * 1.90821492927058770002e-10   (the first product is exact).
 *   5. p = the degree-13 polynomial in x = -rho whose coefficient i is the double nearest 1/i!, by Horner from coefficient 13 down: p = c13;
 *      p = p x + c_i for i = 12 .. 0, one multiply and one add each.
 *   6. v = p 2^-n, exact.
 *   Against exp(-a) to 60 digits on 60 001 points over [0, 708] and 600 small arguments down to 1e-12 the largest error is 1.06 ulp of
 *   the exact value; expn(0) = 1, and sorted arguments never produce an increase (tests/test_rewards.py).
 *   phys_batch_reward_configure   terms [nterms] (host memory), the type of the rewards and term rows (PHYS_OBS_F32 / PHYS_OBS_F64) and the
 *                               clip.  Refuses, with a message in phys_last_error(): an unknown kind, norm or shape, an unknown field,
 *                               PHYS_F_DEPTH, a field the batch does not hold yet, a slice beyond a row, a count outside 1 .. 64,
 *                               PHYS_REW_CONST anywhere but in a tfield or a ROT_INV's field, PHYS_REW_NONE anywhere but in a gfield, a
 *                               non-finite target, vec, dead, k or weight, dead < 0, k < 0, lo > hi, more than PHYS_REW_MAXTERMS terms, an
 *                               unknown dtype, more than 16 sources.  Allocates the table, the rewards, ret and final (zeroed); drops the
 *                               bindings of the rewards, the term rows and the input; waits for the batch's streams.  nterms 0 releases.
 *   phys_batch_reward_bind        the rewards in caller-owned HBM of the configured type, `stride` elements (>= 1) between two envs': a
 *                               column of a wider tensor.  NULL: the batch's own again, zeroed.
 *   phys_batch_reward_bind_terms  the term rows: caller-owned HBM with row_stride (>= nterms) elements between two envs' rows; or NULL with
 *                               own != 0: rows of the batch's own, zeroed; or NULL with own == 0: none are written (the state after
 *                               a configure call).
 *   phys_batch_reward_bind_input  the caller's per-env array [nenv] rows of dim elements, row_stride elements apart, PHYS_OBS_F32 / _F64.
 *                               NULL un-binds.
 *   phys_batch_reward             ONE launch of cassie_reward_kernel over [env0, env0 + n) on `stream` (NULL: the batch's own), in order
 *                               with the launches there.  No host synchronisation, no allocation, no read on the host.  Writes the
 *                               rewards, term rows, ret and (where reset says so) final of the range and nothing else.  Refuses: not
 *                               configured, a range outside the batch, a source field whose row length is no longer what it was at the
 *                               configure call, a PHYS_REW_INPUT term with nothing bound or with a bound dim its terms reach beyond.
 *   phys_batch_reward_dim         nterms, the dtype and whether term rows are written (any may be NULL) -> 0, -1 when not configured.
 *   phys_batch_reward_download / _download_terms   rewards [env0, env0 + n) / their term rows to dense host memory [n] / [n][nterms] of the
 *                               configured type; wait for the streams.
 *   phys_batch_reward_returns / _set_returns / _final   ret [nenv] to and from the host, final [nenv] to the host (doubles); wait for the
 *                               streams.
 *   phys_batch_debug_reward_launches  diagnostics: the launches phys_batch_reward has made. */
enum { PHYS_REW_VEC = 0, PHYS_REW_ROT_INV = 1, PHYS_REW_QUAT = 2 };        /* a term's kind */
enum { PHYS_REW_SUMSQ = 0, PHYS_REW_SUMABS = 1, PHYS_REW_MAXABS = 2 };     /* its norm */
enum { PHYS_REW_LINEAR = 0, PHYS_REW_EXP = 1, PHYS_REW_RATIONAL = 2 };     /* its shape */
enum { PHYS_REW_INPUT = -1, PHYS_REW_CONST = -2, PHYS_REW_NONE = -3 };     /* a term's field / tfield / gfield, beside PHYS_F_* */
#define PHYS_REW_MAXTERMS 64
typedef struct phys_reward_term {
    int kind, field, index, count, qfield, qindex, tfield, tindex, gfield, gindex, norm, shape, root;
    double vec[4];
    double target, dead, k, weight;
} phys_reward_term_t;
int phys_batch_reward_configure(phys_batch_t *b, const phys_reward_term_t *terms, int nterms, int dtype, double lo, double hi);   /* nterms 0: release */
int phys_batch_reward_bind(phys_batch_t *b, void *device_ptr, long long stride);   /* NULL un-binds */
int phys_batch_reward_bind_terms(phys_batch_t *b, void *device_ptr, long long row_stride, int own);
int phys_batch_reward_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype);   /* NULL un-binds */
int phys_batch_reward(phys_batch_t *b, int env0, int n, const void *reset_ptr /* int32 [n] or NULL */, void *stream);
int phys_batch_reward_dim(const phys_batch_t *b, int *nterms, int *dtype, int *term_rows);
int phys_batch_reward_download(phys_batch_t *b, void *host, int env0, int n);
int phys_batch_reward_download_terms(phys_batch_t *b, void *host, int env0, int n);
int phys_batch_reward_returns(phys_batch_t *b, double *host /*[nenv]*/);
int phys_batch_reward_set_returns(phys_batch_t *b, const double *host /*[nenv]*/);
int phys_batch_reward_final(phys_batch_t *b, double *host /*[nenv]*/);
int phys_batch_debug_reward_launches(const phys_batch_t *b, long long *launches);

/* ACTION ROWS: what a policy step WRITES, made on the device by ONE launch per env range from the tensor the policy network put out: the
 * clip of the raw action, uniform actuation noise, a latency of a few policy steps that differs per env, a low-pass, the map onto a
 * reference pose, the clip of the result and the store into the command fields the step kernel reads; and per env a small ACTION ROW the
 * observation and the reward take as their input, so that "the previous action" and "the action rate" are the library's, not each user's
 * bookkeeping.  A configured table of ncols COLUMNS (1 .. PHYS_ACT_MAXCOLS), column c for element c of an env's action.
 * A COLUMN (phys_act_col_t):
 *   lo, hi            the clip of the raw action (infinities are allowed; a NaN passes).
 *   noise             >= 0, the amplitude of the uniform actuation noise.
 *   smooth            in (0, 1], the coefficient of the low-pass; 1: no filter.
 *   bfield, bindex    the base the scaled action is added to: PHYS_ACT_CONST (the offset alone), element bindex of the env's row of any
 *                     PHYS_F_* field an observation may read (every field but PHYS_F_DEPTH, with the row length the batch holds for it when
 *                     the columns are configured, read where the batch reads it at the call), or PHYS_ACT_INPUT: the caller's own per-env
 *                     array bound with phys_batch_act_bind_input as floats or doubles, floats widened exactly -- a reference pose for
 *                     this step.  It may be the tensor bound as the observation's and the reward's input.  At most 16 distinct sources.
 *   offset, scale     finite.
 *   out_lo, out_hi    the clip of what is written.
 *   dfield, dindex    the destination: element dindex of the env's row of a command field -- PHYS_F_PD_PTARGET, PHYS_F_PD_DTARGET,
 *                     PHYS_F_PD_KP, PHYS_F_PD_KD, PHYS_F_PD_TORQUE, PHYS_F_DRIVE_CMD, PHYS_F_CTRL, PHYS_F_QFRC_APPLIED, PHYS_F_XFRC_APPLIED --
 *                     written where the batch reads the field at the call: its own buffer, or the tensor bound with phys_batch_bind /
 *                     _bind_strided with its row stride.  PHYS_ACT_NONE: a column that is only tracked (its row entries and state).  No two
 *                     columns name the same element.  Fields a stepping launch is handed only once somebody wrote them (the applied forces,
 *                     PHYS_F_PD_DTARGET, PHYS_F_PD_TORQUE) count as written from the configure call on, as after an upload.
 * PER ENV AND COLUMN c, PER CALL, every arithmetic step one individually rounded fp64 operation (multiply, add, subtract to nearest even;
 *   no fused multiply-add).  k = counts[env] before the call; a = the env's element c of the bound action tensor (floats widened exactly);
 *   d = delay[env] clamped to [0, D], D the configured delay depth (0 .. PHYS_ACT_MAXDELAY), delay an int32 DEVICE array [nenv] bound by the
 *   caller, or unbound for 0 -- the clamp is silent; fresh = (k == 0 or the call's reset entry for the env is non-zero).
 *     1. u = a < lo ? lo : (a > hi ? hi : a).
 *     2. v = u, or where noise != 0: v = u + noise * xi, with xi = (w + 0.5) 2^-31 - 1 as the observation's and w word 0 of Philox4x32-10
 *        on the counter (env_base + env, c, k, 1) with the key (seed & 0xffffffff, seed >> 32).  The fourth word is 1 where the
 *        observation's is 0: the same seed gives the two their own streams.
 *     3. THE DELAY LINE, D + 1 slots per column, newest first.  fresh: every slot becomes v.  Otherwise slot h takes slot h - 1 for
 *        h = D .. 1 and slot 0 becomes v.  z = slot[d].
 *     4. THE FILTER STATE f.  fresh or smooth == 1: y = z (a skip, not the formula: an unfiltered column reproduces z exactly).  Otherwise
 *        y = f + smooth * (z - f).  Then f = y.
 *     5. base = offset for PHYS_ACT_CONST, else offset + source_row[bindex];  t = base + scale * y;  t = t < out_lo ? out_lo : (t > out_hi ?
 *        out_hi : t).
 *     6. Where there is a destination: dfield_row[dindex] = t.
 *     7. THE ACTION ROW [3][ncols] of the configured type (PHYS_OBS_F32 / PHYS_OBS_F64; the cast rounds to nearest even): frame
 *        PHYS_ACT_NOW = u; frame PHYS_ACT_PREV = the u of the env's previous call, or this u when fresh; frame PHYS_ACT_APPLIED = y.
 *     8. The previous u is kept in the fp64 state, never read back from the row.
 *   Then counts[env] += 1 (uint32, wraps).
 * STATE: per env [D + 3][ncols] doubles -- the line's slots | f | the previous u -- and the count; the batch owns both.  Neither is in a
 *   state-bank row: as with the observation's frame counts, a caller that rewinds or resumes moves them itself (phys_batch_act_state /
 *   _set_state).
 * ORDER IN A POLICY STEP: phys_batch_act; the step launch; the launches that make sources; phys_batch_reward; phys_batch_end_episodes;
 *   phys_batch_obs -- five launches per range that nothing on the host has to touch.  `reset` is an optional int32 DEVICE array [n], entry i
 *   for env env0 + i: the range's slice of PHYS_EP_DONE as the PREVIOUS policy step's phys_batch_end_episodes left it, exactly what
 *   phys_batch_reward is handed -- the first action of a restarted env fills its delay line, and its previous action is that action.
 * NaN, DIVERGED ENVS AND THE DELAY: values flow through to the env's own destinations, row and state; nothing but the clamped d picks among
 *   memory by a value, and it picks among the env's own D + 1 slots.
 *   phys_batch_act_configure    cols [ncols] (host memory), the delay depth, the rows' type, the seed and env_base (as the observation's).
 *                               Refuses, with a message in phys_last_error(): ncols outside 0 .. PHYS_ACT_MAXCOLS, a depth outside 0 ..
 *                               PHYS_ACT_MAXDELAY, an unknown dtype, a non-finite offset or scale, noise < 0 or not finite, smooth outside
 *                               (0, 1], lo > hi or out_lo > out_hi, a destination that is no command field, that the batch does not hold, whose
 *                               dindex lies beyond its row or that an earlier column names, a source the batch does not hold yet,
 *                               PHYS_F_DEPTH, bindex beyond the source's row, more than 16 sources.  Allocates the table, the rows, the
 *                               state and the counts (zeroed); drops the bindings of the actions, the rows, the input and the delays; waits
 *                               for the batch's streams.  ncols 0 releases everything.
 *   phys_batch_act_bind_actions the policy's output in device memory: [nenv] rows of ncols elements, row_stride elements (>= ncols) apart,
 *                               PHYS_OBS_F32 / _F64.  NULL un-binds.
 *   phys_batch_act_bind_rows    the action rows in caller-owned HBM of the configured type, row_stride elements (>= 3 ncols) between two
 *                               envs' rows: a column block of the tensor bound as the observation's and the reward's input.  NULL: the
 *                               batch's own rows again, zeroed.
 *   phys_batch_act_bind_input   the caller's per-env array [nenv] rows of dim elements, row_stride elements apart, PHYS_OBS_F32 / _F64.
 *                               NULL un-binds.
 *   phys_batch_act_bind_delay   the per-env delays, int32 [nenv] in device memory indexed by the absolute env.  NULL: no delay.
 *   phys_batch_act              ONE launch of cassie_act_kernel over [env0, env0 + n) on `stream` (NULL: the batch's own), in order with
 *                               the launches there.  No host synchronisation, no allocation, no read on the host.  Writes the destination
 *                               elements, the action rows, the state and the counts of the range and nothing else.  Refuses: not
 *                               configured, no actions bound, a PHYS_ACT_INPUT column with nothing bound or with a bound dim its columns
 *                               reach beyond, a source or destination field whose row length is no longer what it was at the configure
 *                               call, a range outside the batch.
 *   phys_batch_act_dim          ncols, the delay depth, the row's elements (3 ncols) and the doubles of an env's state ((D + 3) ncols); any
 *                               may be NULL -> 0, -1 when not configured.
 *   phys_batch_act_download     rows [env0, env0 + n) to dense host memory [n][3][ncols] of the rows' type; waits for the streams.
 *   phys_batch_act_state / _set_state   the state [nenv][D + 3][ncols] (doubles) and the counts [nenv] (uint32) to / from the host, so that
 *                               a resumed or rewound run makes what the first would have made; both wait for the streams.
 *   phys_batch_debug_act_launches  diagnostics: the launches phys_batch_act has made. */
enum { PHYS_ACT_INPUT = -1, PHYS_ACT_CONST = -2, PHYS_ACT_NONE = -3 };     /* a column's bfield / dfield, beside PHYS_F_* */
enum { PHYS_ACT_NOW = 0, PHYS_ACT_PREV = 1, PHYS_ACT_APPLIED = 2 };        /* the frames of an action row */
#define PHYS_ACT_MAXCOLS 256
#define PHYS_ACT_MAXDELAY 8
typedef struct phys_act_col {
    int bfield, bindex, dfield, dindex;
    double lo, hi, noise, smooth, offset, scale, out_lo, out_hi;
} phys_act_col_t;
int phys_batch_act_configure(phys_batch_t *b, const phys_act_col_t *cols, int ncols, int delay_max, int dtype, unsigned long long seed,
                             unsigned env_base);   /* ncols 0: release */
int phys_batch_act_bind_actions(phys_batch_t *b, const void *device_ptr, long long row_stride, int dtype);   /* NULL un-binds */
int phys_batch_act_bind_rows(phys_batch_t *b, void *device_ptr, long long row_stride);   /* NULL un-binds */
int phys_batch_act_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype);   /* NULL un-binds */
int phys_batch_act_bind_delay(phys_batch_t *b, const void *device_ptr /* int32 [nenv] or NULL */);
int phys_batch_act(phys_batch_t *b, int env0, int n, const void *reset_ptr /* int32 [n] or NULL */, void *stream);
int phys_batch_act_dim(const phys_batch_t *b, int *ncols, int *delay_max, int *row, int *state);
int phys_batch_act_download(phys_batch_t *b, void *host, int env0, int n);
int phys_batch_act_state(phys_batch_t *b, double *state_host /*[nenv][D + 3][ncols]*/, unsigned *counts_host /*[nenv]*/);
int phys_batch_act_set_state(phys_batch_t *b, const double *state_host, const unsigned *counts_host);
int phys_batch_debug_act_launches(const phys_batch_t *b, long long *launches);

/* TASK ROWS: what a policy step is ASKED, made on the device by ONE launch per env range: the velocity command with its resampling timer
 * and its "stand still", a per-env gait frequency, the gait clock and its sin / cos, the swing / stance gates, the interpolated row of a
 * periodic reference trajectory, and random pushes into PHYS_F_XFRC_APPLIED -- everything the observation, the reward and the action
 * stages took as "the caller's input", so that nothing a policy step reads or writes but the network itself is made on the host, and all
 * of it reproduces whatever the cut of the batch into ranges and ranks.  A configured table of ncols COLUMNS (1 .. PHYS_TASK_MAXCOLS =
 * 64: a lane of the wave makes a column), column c for element c of an env's TASK ROW [ncols] of the configured type (PHYS_OBS_F32 /
 * PHYS_OBS_F64; the cast rounds to nearest even).  The row is the batch's own, or the caller's tensor bound with a row stride -- typically a
 * column block of the tensor phys_batch_obs, _reward and _act bind as their input.
 * A COLUMN (phys_task_col_t) has a kind and, whatever the kind,
 *   dfield, dindex    a destination for its fp64 value besides the row, exactly as an action column's: element dindex of the env's row of
 *                     a command field (the same nine: PHYS_F_PD_PTARGET, _PD_DTARGET, _PD_KP, _PD_KD, _PD_TORQUE, PHYS_F_DRIVE_CMD,
 *                     PHYS_F_CTRL, PHYS_F_QFRC_APPLIED, PHYS_F_XFRC_APPLIED), written where the batch reads the field at the call;
 *                     PHYS_TASK_NONE (= PHYS_ACT_NONE): none.  No two columns name the same element.  A field a stepping launch is handed
 *                     only once somebody wrote it counts as written from the configure call on.
 * PER ENV AND CALL, every arithmetic step one individually rounded fp64 operation (multiply, add, subtract, divide to nearest even; no fused
 *   multiply-add; floor and rint are exact).  count = counts[env] before the call; fresh = (count == 0 or the call's reset entry for the
 *   env is non-zero).  The kinds are evaluated in this order, and a kind only reads kinds above it.  out[c] is column c's value.
 *   wrap(p): f = p - floor(p); f >= 1 ? 0 : f  (a p just below an integer rounds to 1; NaN and the infinities give NaN).
 *   xi(w) = (w + 0.5) 2^-31 - 1, the observation's uniform.  Philox is Philox4x32-10 with the key (seed & 0xffffffff, seed >> 32); the
 *   fourth counter words 2 and 3 are this stage's (the observation uses 0, the action 1).
 * 1. PHYS_TASK_SAMPLE -- a value held for a random number of calls: a command, a gait frequency, an initial phase, a push.
 *      constants: center, half (>= 0), rest, p_rest in [0, 1], period_lo <= period_hi (1 .. 2^30 calls), hold (0: the whole period),
 *      group (-1: the column itself; else a SAMPLE column that is its own group, with which the column must share period_lo, period_hi,
 *      hold and p_rest).  State per (env, column): x (double); left, age, epoch (uint32).
 *      A DRAW happens when fresh or left == 0:
 *        epoch = count == 0 ? 0 : epoch + 1
 *        s = Philox(env_base + env, group, epoch, 2)
 *        L = period_lo + (uint32)(((uint64)s[0] * (uint64)(period_hi - period_lo + 1)) >> 32)
 *        resting = (uint64)s[1] < thr, thr the uint64 nearest p_rest 2^32 (computed once by the configure call)
 *        v = Philox(env_base + env, c, epoch, 3)
 *        x = resting ? rest : center + half * xi(v[0]);   left = L;   age = 0
 *      EVERY call: out = (hold == 0 or age < hold) ? x : rest;  then left -= 1, age += 1.
 *      The schedule is keyed by the group, the value by the column: the columns of a group resample and rest in the same calls while
 *      each draws its own value.  A command (vx, vy, yaw) is a group of three; a push is a group of PHYS_F_XFRC_APPLIED columns with a hold
 *      of a few calls and rest = 0.
 * 2. PHYS_TASK_PHASE -- a clock.  constants: rate (cycles per call), rate_scale, rate_col (-1 or a SAMPLE column), phase0, phase_col (-1
 *      or a SAMPLE column).  State: phi.
 *        fresh:      phi = wrap(phase_col < 0 ? phase0 : out[phase_col])
 *        otherwise:  phi = wrap(phi + inc),  inc = rate_col < 0 ? rate : rate + rate_scale * out[rate_col]
 *      out = phi.  (A restarted env gets a new initial phase because its SAMPLE column drew on the reset.)
 * 3. PHYS_TASK_WAVE -- a waveform of a clock.  constants: src (a PHASE column), shift, form, offset, scale (TRAPEZOID: duty, ramp).
 *        theta = wrap(out[src] + shift)
 *        PHYS_TASK_SAW:        g = theta
 *        PHYS_TASK_SIN, _COS:  g = sin2pi(theta), cos2pi(theta), below
 *        PHYS_TASK_TRAPEZOID:  up = clamp(theta / ramp, 0, 1);  down = clamp((theta - duty) / ramp, 0, 1);  g = up - down
 *                              (ramp > 0, duty >= 0, duty + ramp <= 1: 0 at theta = 0, 1 on [ramp, duty], 0 from duty + ramp on -- the
 *                              swing / stance gate of a clock-gated reward term; clamp(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x))
 *        out = offset + scale * g
 * 4. PHYS_TASK_TABLE -- one column of a periodic reference trajectory T [nframes][tcols] (doubles; phys_batch_task_set_table; nframes <=
 *      4096, tcols <= 64).  constants: src, shift, tcol, offset, scale.
 *        theta as for a WAVE;  s = theta * (double)nframes;  i = s >= 0 ? (int)floor(s) : 0  (a NaN gives 0);  i = min(i, nframes - 1)
 *        fr = s - (double)i;  j = i + 1 == nframes ? 0 : i + 1;  g = T[i][tcol] + fr * (T[j][tcol] - T[i][tcol])
 *        out = offset + scale * g
 *      The clamped i is the only value that picks among memory, and it picks inside the table.
 * sin2pi / cos2pi, for theta in [0, 1) (a library's sin does not reproduce between a device and a host):
 *        a NaN gives NaN.  q = rint(4 theta) (exact);  r = theta - 0.25 q (exact, |r| <= 1/8);  x = r * 6.283185307179586 (the double
 *        nearest 2 pi; ONE rounding);  z = x * x
 *        p = -1/19!;  p = k + z * p for k = 1/17!, -1/15!, 1/13!, -1/11!, 1/9!, -1/7!, 1/5!, -1/3!;  S = x + ((x * z) * p)
 *        c = 1/20!;   c = k + z * c for k = -1/18!, 1/16!, -1/14!, 1/12!, -1/10!, 1/8!, -1/6!, 1/4!, -1/2!;  C = 1 + z * c
 *        (every 1/k! the double nearest it; every product and every sum rounded on its own)
 *        (sin2pi, cos2pi) = (S, C), (C, -S), (-S, -C), (-C, S) for q & 3 = 0, 1, 2, 3.
 *      At theta = 0, 1/4, 1/2, 3/4 the results compare equal to 0 and +-1.  Elsewhere the error against the exact sin(2 pi theta) /
 *      cos(2 pi theta) is measured by tests/test_task.py (DESIGN.md 4.3 has the figure).
 * Then the stores: out[c] into the row (cast), into the destination element where there is one; counts[env] += 1 (uint32, wraps: a count
 *   that comes round to 0 starts the env afresh at epoch 0).
 * STATE: per env [ncols] doubles (a SAMPLE's x, a PHASE's phi, 0 for the other kinds), [3][ncols] uint32 words (left | age | epoch, 0 for
 *   other kinds than SAMPLE) and the count; the batch owns them.  None is in a state-bank row: as with the action state, a caller that
 *   rewinds or resumes moves them itself (phys_batch_task_state / _set_state) and then draws on as the first run would have.
 * ORDER IN A POLICY STEP: phys_batch_act; the step launch; the launches that make sources; phys_batch_reward; phys_batch_end_episodes;
 *   phys_batch_task; phys_batch_obs.  `reset` is an optional int32 DEVICE array [n], entry i for env env0 + i: the range's slice of
 *   PHYS_EP_DONE as THIS step's phys_batch_end_episodes left it, the same words phys_batch_obs takes as `refill`.  The reward therefore
 *   judges a step against the row the policy saw before it; the observation shows the command, clock and reference of the coming step;
 *   and phys_batch_act adds onto that reference pose.
 * NaN AND DIVERGED ENVS: nothing of the state of the simulation is read; a NaN can only come from the caller's constants, which the
 *   configure call refuses, or from an uploaded state.
 *   phys_batch_task_configure   cols [ncols] (host memory), the rows' type, the seed and env_base (as the observation's).  Refuses, with a
 *                               message in phys_last_error(): ncols outside 1 .. PHYS_TASK_MAXCOLS, an unknown kind, form or dtype, a
 *                               constant of the column's kind that is not finite, half < 0, p_rest outside [0, 1], a period outside
 *                               1 <= period_lo <= period_hi <= 2^30, a group, rate_col or phase_col that is no SAMPLE column, a group that
 *                               is not its own group or whose member disagrees with it, a src that is no PHASE column, a TRAPEZOID with
 *                               ramp <= 0, duty < 0 or duty + ramp > 1, a TABLE column with no table set or with tcol beyond it, and
 *                               what phys_batch_act_configure refuses of a destination.  Allocates the table, the rows, the state and the
 *                               counts (zeroed); drops the binding of the rows; waits for the batch's streams.
 *   phys_batch_task_set_table   the reference trajectory, host [nframes][tcols] doubles (1 .. 4096 frames, 1 .. 64 columns, finite), uploaded
 *                               once and owned by the batch; set it before the configure call that names it.  Refuses a table narrower
 *                               than the configured TABLE columns reach.  Waits for the batch's streams.
 *   phys_batch_task_bind_rows   the task rows in caller-owned HBM of the configured type, row_stride elements (>= ncols) between two envs'
 *                               rows.  NULL: the batch's own rows again, zeroed.
 *   phys_batch_task             ONE launch of cassie_task_kernel over [env0, env0 + n) on `stream` (NULL: the batch's own), in order with
 *                               the launches there.  No host synchronisation, no allocation, no read on the host.  Writes the rows, the
 *                               state, the counts and the destination elements of the range and nothing else.  Refuses: not configured,
 *                               a range outside the batch, a destination field whose row length is no longer what it was at the
 *                               configure call.
 *   phys_batch_task_dim         ncols and the rows' type; either may be NULL -> 0, -1 when not configured.
 *   phys_batch_task_download    rows [env0, env0 + n) to dense host memory [n][ncols] of the rows' type; waits for the streams.
 *   phys_batch_task_state / _set_state   the state [nenv][ncols] (doubles), the words [nenv][3][ncols] (uint32) and the counts [nenv]
 *                               (uint32) to / from the host; both wait for the streams.
 *   phys_batch_debug_task_launches  diagnostics: the launches phys_batch_task has made. */
enum { PHYS_TASK_SAMPLE = 0, PHYS_TASK_PHASE = 1, PHYS_TASK_WAVE = 2, PHYS_TASK_TABLE = 3 };         /* a column's kind */
enum { PHYS_TASK_SAW = 0, PHYS_TASK_SIN = 1, PHYS_TASK_COS = 2, PHYS_TASK_TRAPEZOID = 3 };           /* a WAVE column's form */
enum { PHYS_TASK_NONE = -3 };                                                                        /* no destination (= PHYS_ACT_NONE) */
#define PHYS_TASK_MAXCOLS 64
#define PHYS_TASK_MAXFRAMES 4096
#define PHYS_TASK_MAXTCOLS 64
typedef struct phys_task_col {
    int kind, form, group, rate_col, phase_col, src, tcol, dfield, dindex;
    unsigned period_lo, period_hi, hold;
    double center, half, rest, p_rest;        /* SAMPLE */
    double rate, rate_scale, phase0;          /* PHASE */
    double shift, duty, ramp, offset, scale;  /* WAVE, TABLE */
} phys_task_col_t;
int phys_batch_task_configure(phys_batch_t *b, const phys_task_col_t *cols, int ncols, int dtype, unsigned long long seed, unsigned env_base);
int phys_batch_task_set_table(phys_batch_t *b, const double *host /*[nframes][tcols]*/, int nframes, int tcols);
int phys_batch_task_bind_rows(phys_batch_t *b, void *device_ptr, long long row_stride);   /* NULL un-binds */
int phys_batch_task(phys_batch_t *b, int env0, int n, const void *reset_ptr /* int32 [n] or NULL */, void *stream);
int phys_batch_task_dim(const phys_batch_t *b, int *ncols, int *dtype);
int phys_batch_task_download(phys_batch_t *b, void *host, int env0, int n);
int phys_batch_task_state(phys_batch_t *b, double *state_host /*[nenv][ncols]*/, unsigned *words_host /*[nenv][3][ncols]*/, unsigned *counts_host /*[nenv]*/);
int phys_batch_task_set_state(phys_batch_t *b, const double *state_host, const unsigned *words_host, const unsigned *counts_host);
int phys_batch_debug_task_launches(const phys_batch_t *b, long long *launches);

/* EVENT ROWS: what a policy step remembers of the steps before it -- contact flags with hysteresis, the time a foot has been in the air,
 * the call on which it touched down, the peak force of a stance, and terminations the fixed rules of phys_batch_episodes_enable cannot
 * state -- made on the device by ONE launch per env range.  A configured table of ncols COLUMNS (1 .. PHYS_EV_MAXCOLS = 64) is evaluated
 * IN INDEX ORDER; a column names only columns with a LOWER index (the configure call refuses anything else), so no value ever picks
 * among memory.  Per env the call writes the EVENT ROW [ncols] (floats or doubles; the batch's own rows or a caller's tensor bound with
 * a row stride -- typically a column block of the tensor phys_batch_obs, _reward, _act and _task bind as their input) and one int32 DONE
 * WORD, 1 or 0 (the batch's own array, phys_batch_events_flags_ptr, or a bound one), which phys_batch_end_episodes takes as `force`.
 * COMMON RULES, per env and call:
 *   count = counts[env] before the call;  fresh = (count == 0 or the call's reset entry is non-zero);
 *   out[k] is column k's fp64 value of THIS call; on(k) means out[k] > 0.0, so a NaN is off.
 *   Every arithmetic step is one individually rounded fp64 operation (multiply, add, subtract, square root to nearest even; no fused
 *   multiply-add, no reassociation); every sum is sequential from +0.0 in index order; every comparison is written so that a NaN takes
 *   the branch stated.  The device, the wave emulator and a numpy restatement agree on every bit, whatever the cut into ranges.
 * A COLUMN (phys_event_col_t) by its kind; the fields a kind does not name are ignored:
 *   PHYS_EV_MEASURE  a number from a source.  field: any PHYS_F_* field but PHYS_F_DEPTH, with the row length the batch holds for it at
 *                    the configure call, read where the batch reads it at the call; or PHYS_EV_INPUT, the caller's per-env array bound
 *                    with phys_batch_events_bind_input (floats widened exactly).  At most 16 distinct sources.  index, count (1 .. 8),
 *                    target, norm, root.  e[j] = src_row[index + j] - target, j < count.
 *                      PHYS_EV_SIGNED (count must be 1): out = e[0].
 *                      PHYS_EV_SUMABS: out = sum_j |e[j]|.
 *                      PHYS_EV_SUMSQ:  s = sum_j e[j] e[j]; out = root != 0 ? sqrt(s) : s.  (root is ignored by the other norms.)
 *                      PHYS_EV_MAXABS: s = +0.0, then for every j in order  if (|e[j]| > s) s = |e[j]|  (a NaN element is passed over).
 *   PHYS_EV_LEVEL    a Schmitt trigger on column src.  on_thr, off_thr (off_thr <= on_thr), sense (+1 or -1).  State word s.
 *                    w = sense < 0 ? -out[src] : out[src].  Fresh: s = w >= on_thr.  Otherwise: s = s ? (w > off_thr) : (w >= on_thr).
 *                    out = s (0.0 or 1.0).  A NaN switches it off.
 *   PHYS_EV_TIMER    the consecutive calls column src has been on (polarity != 0) or off (polarity == 0), times dt.  State word t.
 *                    Fresh: t = 0.  Then, if on(src) != (polarity == 0): t = t == 0xffffffff ? t : t + 1; otherwise t = 0.
 *                    out = dt * (double)t: one multiply of an exact conversion.  (A first call on which the condition holds shows dt.)
 *   PHYS_EV_EDGE     the call on which column src switched.  op: PHYS_EV_RISING, _FALLING or _EITHER.  State word p.
 *                    c = on(src).  Fresh: p = c, so a first call has no edge.  out = RISING: c && !p; FALLING: !c && p; EITHER: c != p
 *                    (0.0 or 1.0).  Then p = c.
 *   PHYS_EV_LATCH    column src's value taken when column trig fires.  lag (0 or 1), keep (0 or 1), offset, scale.  State doubles h, q.
 *                    Fresh: h = 0, q = 0.  If on(trig): h = offset + scale * (lag ? q : out[src]).  out = (keep or on(trig)) ? h : 0.
 *                    Then q = out[src].  Air time paid at touchdown is a LATCH with lag = 1 of the off-TIMER, triggered by the
 *                    rising EDGE: the timer's value on the call before.
 *   PHYS_EV_ACCUM    a running maximum, minimum or sum of column src.  op: PHYS_EV_MAX, _MIN or _SUM; clear, gate (-1 or a column);
 *                    init (finite).  State double m.  v = out[src].  If fresh or on(clear): m = init.  Then, if gate < 0 or on(gate):
 *                    MAX: m = v > m ? v : m;  MIN: m = v < m ? v : m;  SUM: m = m + v.  out = m.  A NaN v is passed over by MAX and
 *                    MIN; in a SUM it sticks until the next clear.
 *   PHYS_EV_LOGIC    a combination of columns.  mask: a uint64 over lower columns, not 0; op.  c = the number of on columns of the
 *                    mask.  out = PHYS_EV_ANY: c > 0;  _ALL: c == popcount(mask);  _NONE: c == 0;  _COUNT: (double)c.
 * STORES: out[c] goes into the row, cast to nearest even where the rows are PHYS_OBS_F32;  flag[env] = (any on(c) with bit c of
 *   done_mask set) ? 1 : 0, done_mask a uint64 given to the configure call (0: the word is always 0);  counts[env] += 1 (it wraps, and
 *   a count that comes round to 0 is fresh).
 * STATE: per env [2][ncols] doubles (slot 0: a LATCH's h, an ACCUM's m; slot 1: a LATCH's q; 0 elsewhere), [ncols] uint32 words (a
 *   LEVEL's s, a TIMER's t, an EDGE's p; 0 elsewhere) and the count; the batch owns them.  None is in a state-bank row: as with the action
 *   and task state, a caller that rewinds or resumes moves them itself (phys_batch_events_state / _set_state).  A fresh env reads none
 *   of its state.
 * ORDER IN A POLICY STEP: phys_batch_act; the step launch; the launches that make sources (probe, rays, scan); phys_batch_events;
 *   phys_batch_reward (a term gated by an event column reads this step's value); phys_batch_end_episodes(force = the range's slice of
 *   the done words); phys_batch_task; phys_batch_obs.  `reset` is an optional int32 DEVICE array [n], entry i for env env0 + i: the
 *   range's slice of PHYS_EP_DONE as the PREVIOUS step's phys_batch_end_episodes left it -- the words phys_batch_reward and
 *   phys_batch_act take -- so the first call that sees a restarted env's state starts its columns afresh.
 * NaN AND DIVERGED ENVS: values flow through to the env's own row; nothing indexes memory by a value.
 *   phys_batch_events_configure   cols [ncols] (host memory), the rows' type (PHYS_OBS_F32 / PHYS_OBS_F64) and done_mask.  Refuses, with a
 *                               message in phys_last_error(): ncols outside 1 .. 64 (0 releases), an unknown kind, norm, op or dtype, a
 *                               src, trig, clear or gate that is no lower index (clear and gate may be -1), a done_mask or LOGIC mask
 *                               bit at or above ncols, a LOGIC mask that is 0 or has a bit at or above the column's own index, a
 *                               constant of the column's kind that is not finite, off_thr > on_thr, a sense other than +1 or -1, a
 *                               count outside 1 .. 8, SIGNED with count != 1, PHYS_F_DEPTH, an unknown field, a field the batch does
 *                               not hold, a slice beyond a row, more than 16 sources.  Allocates the table, the rows, the done words,
 *                               the state and the counts (zeroed); drops the bindings of the rows, the input and the done words; waits
 *                               for the batch's streams.
 *   phys_batch_events_bind_rows   the event rows in caller-owned HBM of the configured type, row_stride elements (>= ncols) between two
 *                               envs' rows.  NULL: the batch's own rows again, zeroed.
 *   phys_batch_events_bind_input  the caller's per-env array [nenv] rows of dim elements, row_stride elements apart, PHYS_OBS_F32 / _F64.
 *                               NULL un-binds.
 *   phys_batch_events_bind_flags  the done words in caller-owned HBM: int32 [nenv], dense.  NULL: the batch's own again, zeroed.
 *   phys_batch_events_flags_ptr   the device address of the done words now in use (NULL when not configured): env e's word is element e.
 *   phys_batch_events             ONE launch of cassie_event_kernel over [env0, env0 + n) on `stream` (NULL: the batch's own), in order
 *                               with the launches there.  No host synchronisation, no allocation, no read on the host.  Writes the
 *                               rows, the done words, the state and the counts of the range and nothing else.  Refuses: not configured,
 *                               a range outside the batch, a source field whose row length is no longer what it was at the configure
 *                               call, a PHYS_EV_INPUT column with nothing bound or with a bound dim its columns reach beyond.
 *   phys_batch_events_dim         ncols, the rows' type and done_mask; any may be NULL -> 0, -1 when not configured.
 *   phys_batch_events_download    rows [env0, env0 + n) to dense host memory [n][ncols] of the rows' type; waits for the streams.
 *   phys_batch_events_download_flags  the done words [nenv] to the host; waits for the streams.
 *   phys_batch_events_state / _set_state   the state [nenv][2][ncols] (doubles), the words [nenv][ncols] (uint32) and the counts [nenv]
 *                               (uint32) to / from the host (on the device they lie [2][ncols][nenv] and [ncols][nenv]); both wait
 *                               for the streams.
 *   phys_batch_debug_events_launches  diagnostics: the launches phys_batch_events has made. */
enum { PHYS_EV_MEASURE = 0, PHYS_EV_LEVEL = 1, PHYS_EV_TIMER = 2, PHYS_EV_EDGE = 3, PHYS_EV_LATCH = 4, PHYS_EV_ACCUM = 5, PHYS_EV_LOGIC = 6 };   /* a column's kind */
enum { PHYS_EV_SIGNED = 0, PHYS_EV_SUMABS = 1, PHYS_EV_SUMSQ = 2, PHYS_EV_MAXABS = 3 };   /* a MEASURE's norm */
enum { PHYS_EV_RISING = 0, PHYS_EV_FALLING = 1, PHYS_EV_EITHER = 2 };                     /* an EDGE's op */
enum { PHYS_EV_MAX = 0, PHYS_EV_MIN = 1, PHYS_EV_SUM = 2 };                               /* an ACCUM's op */
enum { PHYS_EV_ANY = 0, PHYS_EV_ALL = 1, PHYS_EV_NONE = 2, PHYS_EV_COUNT = 3 };           /* a LOGIC's op */
enum { PHYS_EV_INPUT = -1 };                                                              /* a MEASURE's field, beside PHYS_F_* */
#define PHYS_EV_MAXCOLS 64
#define PHYS_EV_MAXCOUNT 8
typedef struct phys_event_col {
    int kind, field, index, count, norm, root;        /* MEASURE */
    int src, trig, clear, gate;                       /* lower columns */
    int op, sense, polarity, lag, keep, pad;          /* EDGE / ACCUM / LOGIC: op; LEVEL: sense; TIMER: polarity; LATCH: lag, keep */
    unsigned long long mask;                          /* LOGIC */
    double target, on_thr, off_thr, dt, offset, scale, init;
} phys_event_col_t;
int phys_batch_events_configure(phys_batch_t *b, const phys_event_col_t *cols, int ncols, int dtype, unsigned long long done_mask);   /* ncols 0: release */
int phys_batch_events_bind_rows(phys_batch_t *b, void *device_ptr, long long row_stride);   /* NULL un-binds */
int phys_batch_events_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype);   /* NULL un-binds */
int phys_batch_events_bind_flags(phys_batch_t *b, void *device_ptr /* int32 [nenv] */);   /* NULL un-binds */
void *phys_batch_events_flags_ptr(phys_batch_t *b);
int phys_batch_events(phys_batch_t *b, int env0, int n, const void *reset_ptr /* int32 [n] or NULL */, void *stream);
int phys_batch_events_dim(const phys_batch_t *b, int *ncols, int *dtype, unsigned long long *done_mask);
int phys_batch_events_download(phys_batch_t *b, void *host, int env0, int n);
int phys_batch_events_download_flags(phys_batch_t *b, int *host /*[nenv]*/);
int phys_batch_events_state(phys_batch_t *b, double *state_host /*[nenv][2][ncols]*/, unsigned *words_host /*[nenv][ncols]*/, unsigned *counts_host /*[nenv]*/);
int phys_batch_events_set_state(phys_batch_t *b, const double *state_host, const unsigned *words_host, const unsigned *counts_host);
int phys_batch_debug_events_launches(const phys_batch_t *b, long long *launches);

/* POLICY ROWS: the function between the observation row and the action tensor -- a small MLP actor, optionally a critic, and optionally
 * the sampled action with its log-probability -- in ONE launch per env range on the caller's stream, with every bit of the result
 * defined.  Weights and activations are float32 and every sum is accumulated in fp64 by fused multiply-add on the matrix core: the product
 * of two float32 values is exact in a double, so every fma is ONE rounding of acc + w x, and the order of the sum is fixed here, not by
 * whichever GEMM a BLAS library picks.  The device (cassie_policy_kernel, csrc/policy_kernels.h), the wave emulator and a numpy
 * restatement (tests/policy_check.py: acc = acc + w * x on doubles) agree bit for bit.  No stepping kernel is handed any of this.
 *
 * LIMITS.  A POLICY is 1 or 2 NETWORKS: network 0 is the actor, network 1 if present the critic.  Both read the same input row of in_dim
 *   float32, 1 <= in_dim <= 512.  A network is 1 .. 4 dense layers; a layer has `out` units, 1 <= out <= 512, a network's last layer at
 *   most 64, and an activation PHYS_POL_IDENTITY, _RELU, _ELU or _TANH.  Weights are float32 [out][in], row-major with a row stride, as
 *   torch.nn.Linear.weight; biases float32 [out].
 * INPUT.  x[k] is the bound row's element k.  Where a normalisation is bound: x[k] = (float) clip((x[k] - mean[k]) * inv[k], -c, c), mean
 *   and inv float32 [in_dim] in device memory READ AT EVERY CALL (a caller's running statistics, or NORMALISER ROWS' below, act at once); the subtraction and the
 *   product are individually rounded fp64 operations, the clip is two compares and selects (y < -c ? -c : y > c ? c : y: a NaN passes),
 *   c >= 0 or +inf, and the conversion rounds to nearest even.
 * LAYER.  K4 = in rounded up to a multiple of 4.  acc = (double) b[j]; for k = 0 .. K4 - 1 ascending: acc = fma((double) w[j][k],
 *   (double) x[k], acc), with w and x of the padding k >= in being +0.0 -- so a bias of -0.0 ends as +0.0 when `in` is no multiple of 4
 *   (the restatement does the same).  z = acc; h[j] = (float) act(z), rounded to nearest even; the next layer's x is h.
 * ACTIVATIONS, in individually rounded fp64 operations; expn is the reward's (expn(a) ~ exp(-a), above), C3 and C6 the doubles nearest
 *   1/3 and 1/6:
 *     IDENTITY  z.
 *     RELU      z < 0 ? +0.0 : z (a NaN and -0.0 pass).
 *     TANH      NaN -> NaN; m = |z|; m < 2^-10: v = z - z * ((z * z) * C3); otherwise t = expn(2 m), v = (1 - t) / (1 + t), negated
 *               where z < 0.
 *     ELU       (alpha 1) z >= 0 or NaN: z; z > -2^-10: v = z + (z * z) * (0.5 + z * C6); otherwise v = expn(-z) - 1.
 *   The small branches exist because the large-argument forms lose RELATIVE accuracy near 0 (1 - t and expn - 1 cancel): with them the
 *   fp64 value is within 2^-34 relative of the exact function (the dropped series terms: z^3 / 24 of ELU at 2^-10 is 2^-34.6 of z), so the
 *   float32 result is within 1 float32 ulp of the exact value.
 * OUTPUTS.  A network's last h goes to its bound output: float32 [nenv][out] with a row stride.
 * SAMPLE (optional, network 0; A its output width, mu its output).  Bound: eps float32 [nenv][A], the caller's standard normal draws;
 *   log_std float32 [A] in device memory, read at every call; an action tensor float32 [nenv][A] (what phys_batch_act_bind_actions
 *   points at, so phys_batch_act follows with nothing in between); logp float32 [nenv].  In individually rounded fp64 operations:
 *   s[j] = expn(-(double) log_std[j]); a[j] = (float)(mu[j] + s[j] * eps[j]); q = sum_j eps[j] * eps[j] and L = sum_j log_std[j], both
 *   sequential in j from +0.0; logp = (float)((-0.5 * q - L) - A * H), H the double nearest 0.5 ln(2 pi).  mu still goes to the actor's
 *   output where one is bound.
 * A NaN flows through an env's own outputs; nothing indexes memory by a value; no env reads another's data; a call over [env0, env0 + n)
 *   writes what two calls over its halves write.  Rows outside the range are left alone.
 * ORDER IN A POLICY STEP: end_episodes, task, observe, policy, act, the step launch, events, reward.
 *
 *   phys_batch_policy_configure   nets [nnets] (host memory) and in_dim: checks the shapes and allocates the packed weights; drops every
 *                                 binding and every loaded layer.  nnets 0 releases.  Refuses, with a message in phys_last_error():
 *                                 more than 2 networks or 4 layers, a width or in_dim outside the limits, an unknown activation, a first
 *                                 layer whose `in` is not in_dim, a layer whose `in` is not the previous `out`, a last layer wider than 64.
 *   phys_batch_policy_load        a layer's weights and biases from DEVICE pointers (float32; w rows w_row_stride elements apart): one
 *                                 small launch on `stream` (NULL: the batch's own) packs them into the layout the kernel reads
 *                                 (zero-padded to K4 and to 16 units; per block of 16 units and k-step of 4 the 64 words
 *                                 w[unit l & 15][k0 + (l >> 4)] in lane order).  Called after an optimiser step, on the stream the policy
 *                                 call follows on.  phys_batch_policy_load_host: the same from host arrays (waits for the streams).
 *                                 A policy call with a layer that was never loaded is refused.
 *   phys_batch_policy_bind_input  the input rows: [nenv] rows of dim (= in_dim) float32, row_stride elements apart; dtype PHYS_OBS_F32
 *                                 (float64 is refused: the products would not be exact).  NULL un-binds.
 *   phys_batch_policy_bind_norm   mean and inv [in_dim] float32 in device memory and the clip c.  NULL releases.
 *   phys_batch_policy_bind_output network net's output rows, row_stride elements (>= its width) apart.  NULL un-binds.
 *   phys_batch_policy_bind_sample eps, log_std, the action tensor and logp (strides >= A).  A NULL eps releases.
 *   phys_batch_policy             ONE launch of cassie_policy_kernel over [env0, env0 + n) on `stream`; n 0 is accepted.  No host
 *                                 synchronisation.
 *   phys_batch_policy_download    network net's bound output rows to dense host memory [nenv][width]; waits for the streams.
 *   phys_batch_policy_download_packed  the packed floats to the host (count: their number; host NULL: the count alone); waits.
 *   phys_batch_debug_policy_launches   diagnostics: the launches phys_batch_policy has made. */
enum { PHYS_POL_IDENTITY = 0, PHYS_POL_RELU = 1, PHYS_POL_ELU = 2, PHYS_POL_TANH = 3 };
#define PHYS_POL_MAXNETS 2
#define PHYS_POL_MAXLAYERS 4
#define PHYS_POL_MAXDIM 512
#define PHYS_POL_MAXOUT 64
typedef struct phys_pol_layer { int in, out, act; } phys_pol_layer_t;
typedef struct phys_pol_net { int nlayers; phys_pol_layer_t layer[PHYS_POL_MAXLAYERS]; } phys_pol_net_t;
int phys_batch_policy_configure(phys_batch_t *b, const phys_pol_net_t *nets, int nnets, int in_dim);   /* nnets 0: release */
int phys_batch_policy_load(phys_batch_t *b, int net, int layer, const void *w_ptr, long long w_row_stride, const void *b_ptr, void *stream);
int phys_batch_policy_load_host(phys_batch_t *b, int net, int layer, const float *w, long long w_row_stride, const float *bias);
int phys_batch_policy_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype);   /* NULL un-binds */
int phys_batch_policy_bind_norm(phys_batch_t *b, const void *mean_ptr, const void *inv_ptr, double clip);   /* NULL releases */
int phys_batch_policy_bind_output(phys_batch_t *b, int net, void *device_ptr, long long row_stride);   /* NULL un-binds */
int phys_batch_policy_bind_sample(phys_batch_t *b, const void *eps_ptr, long long eps_stride, const void *log_std_ptr, void *action_ptr,
                                  long long action_stride, void *logp_ptr);   /* NULL eps releases */
int phys_batch_policy(phys_batch_t *b, int env0, int n, void *stream);
int phys_batch_policy_download(phys_batch_t *b, int net, float *host);
int phys_batch_policy_download_packed(phys_batch_t *b, float *host, long long *count);
int phys_batch_debug_policy_launches(const phys_batch_t *b, long long *launches);

/* ROLLOUT ROWS: what lies between the policy step and the optimiser -- the T transitions of a rollout stored by ONE launch per env range
 * per policy step, their advantages and returns (GAE) by ONE launch per range, and the advantages normalised over the whole batch -- with
 * every bit of the result defined.  The device (csrc/rollout_kernels.h), the wave emulator and a numpy restatement
 * (tests/rollout_check.py) agree bit for bit; a recorded run can be replayed, or compared across ranks, up to the tensors the optimiser
 * reads.  No stepping kernel is handed any of this.
 *
 * LIMITS.  1 <= T <= 1024 steps (PHYS_RO_MAXT); 1 .. 16 SOURCES (PHYS_RO_MAXSRC); a source is {role, dim} with 1 <= dim <= 4096
 *   (PHYS_RO_MAXDIM) 32-BIT WORDS a row: float32 and int32 are both copied as words, the copy is bit-exact and type-blind (float64 is out
 *   of scope).  Where a function takes `s`, it is a source's index 0 .. nsrcs - 1, or the role of exactly one source, or -- for storage
 *   and downloads -- PHYS_RO_ADV, _RET, _ADVN (the roles are numbered from 16 on, so that one int does for both).
 * ROLES.  PHYS_RO_DATA: any rows of the caller's; its pointer is mandatory (phys_batch_rollout_bind_source) and several sources may have
 *   the role.  PHYS_RO_OBS, _ACTION, _LOGP, _MU, _VALUE, _REWARD, _DONE, _REASON: at most one source each; VALUE, REWARD, DONE, REASON and
 *   LOGP have dim 1.  A source of these roles that is unbound (or bound to NULL) is RESOLVED AT EVERY CALL from where the batch reads or
 *   writes that thing at that moment, the reward's convention:
 *     OBS            the policy's bound input (phys_batch_policy_bind_input)
 *     MU             network 0's bound output
 *     VALUE          network 1's bound output, column 0
 *     ACTION, LOGP   the sample binding (phys_batch_policy_bind_sample)
 *     REWARD         the rewards, the batch's own or bound; they must be configured PHYS_OBS_F32, refused at the call otherwise
 *     DONE, REASON   PHYS_EP_DONE / PHYS_EP_REASON, the batch's own or bound (int32)
 *   A resolved width or row stride that no longer fits the configured dim refuses the call, with a message in phys_last_error().
 * STORAGE.  Per source [T][nenv][dim] words, TIME-MAJOR: a range's slot is one contiguous block, and the GAE reads consecutive envs.  The
 *   batch's own, zeroed at configure (phys_batch_rollout_ptr), or a caller's tensor in its place (phys_batch_rollout_bind_storage: the
 *   words between two steps and between two rows, both may be padded; NULL goes back to the batch's own, zeroed), so that the update
 *   reads a torch view with no copy.  ADV and RET, float32 [T][nenv], are own or bound the same way; ADVN, a third array of that shape, is
 *   allocated on the first phys_batch_rollout_normalise, or bound.  None of it is in a state-bank row: as with the reward's returns, a
 *   caller that rewinds an env decides itself what becomes of the steps it had recorded.
 * RECORD.  phys_batch_rollout_record(b, t, env0, n, stream) is ONE launch: for every source s, every env of the range and every j < dim,
 *   store[s][t][env][j] = src_s[env * row_stride + j].  Nothing else is written: rows outside the range, slots other than t and the
 *   padding between rows are left alone.  t is the caller's (0 <= t < T): there is no device counter, and two ranges on two streams stay
 *   independent.  n 0 is accepted.  The call never synchronises the host.  Where a source's pointer, its slot, its dim and both row
 *   strides are multiples of 4 words a lane moves 16 bytes, otherwise a word; the host decides per source and call.
 * ORDER IN A POLICY STEP, as a cycle: end_episodes, ROLLOUT_RECORD, task, observe, policy, act, the step launch, events, reward.  Behind
 *   end_episodes of step t the bound tensors still hold o_t, a_t, logp_t, mu_t, v_t and r_t -- observe and policy have not run again --
 *   and PHYS_EP_DONE / _REASON are that step's verdict.
 * FINISH.  phys_batch_rollout_finish(b, env0, n, last_value_ptr, stride, stream) is ONE launch, a lane per env, behind the range's T
 *   records.  last_value float32 [nenv] rows `stride` words apart; NULL: the VALUE source as resolved now, which is V(o_T) after the
 *   caller's next observe and policy (it runs them anyway).  VALUE and REWARD sources are required; without a DONE source every d is
 *   false.  Every step is ONE individually rounded fp64 operation, no fma, no reassociation; gl = gamma * lambda is rounded once on the host:
 *     nv = (double) last_value[env];  a = +0.0
 *     for t = T - 1 .. 0:
 *         v = (double) V[t][env];  r = (double) R[t][env];  d = DONE[t][env] != 0
 *         if timeout_mask and d and (REASON[t][env] & timeout_mask) != 0 and (REASON[t][env] & ~timeout_mask) == 0:
 *             r = r + gamma * v        (an episode cut by the time limit alone bootstraps from the step's own value)
 *         nvs = d ? +0.0 : nv;  as = d ? +0.0 : a        (SELECTS, not products: 0 * NaN would carry an ended episode's NaN backwards)
 *         delta = (r + gamma * nvs) - v
 *         a = delta + gl * as
 *         ADV[t][env] = (float) a;  RET[t][env] = (float)(a + v);  nv = v
 *     q1[env] = sum over t ascending from +0.0 of (double) ADV[t][env]        (the env's partial of the mean)
 *   A NaN stays in its env; a call over a range writes what two calls over its halves write.
 * NORMALISE.  phys_batch_rollout_normalise(b, eps, stream) is FOUR short launches on `stream` over the WHOLE batch, behind every range's
 *   finish: ORDERING THE STREAMS IS THE CALLER'S JOB (the ranges' streams wait for nothing here).  No kernel spins on another workgroup
 *   or uses a grid-wide barrier: the stream orders the four.  Refuses M = T * nenv < 2 and an eps that is negative or not finite.
 *   reduce(x[nenv]): the envs padded with +0.0 to a multiple of 64; every block of 64 consecutive envs summed by the wave's tree
 *   (wv::wave_sum, pinned by tests/test_wave_primitives.py); the block sums added sequentially in block order from +0.0.
 *     mean = reduce(q1) / M
 *     q2[env] = sum over t ascending from +0.0 of ((double) ADV[t][env] - mean)^2
 *     std = sqrt(reduce(q2) / (M - 1));  inv = 1 / (std + eps)
 *     ADVN[t][env] = (float)(((double) ADV[t][env] - mean) * inv)
 *   The result does not depend on how finish was cut into ranges.  phys_batch_rollout_stats downloads {mean, std, inv}.
 *
 *   phys_batch_rollout_configure     srcs [nsrcs] (host memory), T, gamma, lambda, timeout_mask: allocates and zeroes the stores, ADV and
 *                                    RET; drops every binding.  Waits for the streams.  nsrcs 0 releases.  Refuses: T or a dim outside
 *                                    the limits, an unknown or duplicate role, a dim other than 1 where the role fixes it, a gamma or
 *                                    lambda that is not finite or outside [0, 1], a non-zero timeout_mask without a REASON source.
 *   phys_batch_rollout_bind_source   a source's rows in device memory, row_stride words (>= dim) apart.  NULL un-binds.
 *   phys_batch_rollout_bind_storage  a caller's tensor in the place of a store, of ADV, RET or ADVN: step_stride and row_stride in words.
 *   phys_batch_rollout_ptr           where a store, ADV, RET or ADVN lies now (NULL: none), with its strides.
 *   phys_batch_rollout_record / _finish / _normalise   above.
 *   phys_batch_rollout_stats         {mean, std, inv} of the last normalise to the host; waits for the streams.
 *   phys_batch_rollout_download      a store, ADV, RET or ADVN to dense host memory [T][nenv][dim] words; waits for the streams.
 *   phys_batch_rollout_dim           T, the count of sources and (dims non-NULL) their dims.
 *   phys_batch_debug_rollout_launches  diagnostics: the launches of record, of finish and of normalise (4 a call) so far. */
enum { PHYS_RO_DATA = 16, PHYS_RO_OBS = 17, PHYS_RO_ACTION = 18, PHYS_RO_LOGP = 19, PHYS_RO_MU = 20, PHYS_RO_VALUE = 21, PHYS_RO_REWARD = 22,
       PHYS_RO_DONE = 23, PHYS_RO_REASON = 24, PHYS_RO_ADV = 25, PHYS_RO_RET = 26, PHYS_RO_ADVN = 27 };
#define PHYS_RO_MAXT 1024
#define PHYS_RO_MAXSRC 16
#define PHYS_RO_MAXDIM 4096
typedef struct phys_rollout_src { int role, dim; } phys_rollout_src_t;
int phys_batch_rollout_configure(phys_batch_t *b, int T, const phys_rollout_src_t *srcs, int nsrcs, double gamma, double lambda, unsigned timeout_mask);   /* nsrcs 0: release */
int phys_batch_rollout_bind_source(phys_batch_t *b, int s, const void *device_ptr, long long row_stride);   /* NULL un-binds */
int phys_batch_rollout_bind_storage(phys_batch_t *b, int s, void *device_ptr, long long step_stride, long long row_stride);   /* NULL: the batch's own */
void *phys_batch_rollout_ptr(phys_batch_t *b, int s, long long *step_stride, long long *row_stride);
int phys_batch_rollout_record(phys_batch_t *b, int t, int env0, int n, void *stream);
int phys_batch_rollout_finish(phys_batch_t *b, int env0, int n, const void *last_value_ptr, long long stride, void *stream);
int phys_batch_rollout_normalise(phys_batch_t *b, double eps, void *stream);
int phys_batch_rollout_stats(phys_batch_t *b, double *mean_std_inv /*[3]*/);
int phys_batch_rollout_download(phys_batch_t *b, int s, void *host);
int phys_batch_rollout_dim(const phys_batch_t *b, int *T, int *nsrcs, int *dims /*[nsrcs] or NULL*/);
int phys_batch_debug_rollout_launches(const phys_batch_t *b, long long *launches /*[3]: record, finish, normalise*/);

/* GRADIENT ROWS: for a minibatch of the rollout's samples, the PPO clipped-surrogate loss, the value loss and the entropy term, and their
 * gradient with respect to every weight, every bias and log_std of the policy, by FIVE launches on the caller's stream with every bit
 * defined.  The forward pass the gradient is taken through IS the one the policy acts with (POLICY ROWS); the gradients land in float32
 * tensors an optimiser takes as param.grad with no copy; the optimiser step is the caller's (phys_batch_policy_load follows it) or
 * OPTIMISER ROWS' below (nothing follows it).
 * The device (csrc/grad_kernels.h), the wave emulator and a numpy restatement (tests/grad_check.py) agree bit for bit.  No stepping kernel
 * is handed any of this.
 *
 * All arithmetic is individually rounded fp64 operations unless stated as an fma chain; every fma chain multiplies two float32 values, so
 * its products are exact and every step is ONE rounding of acc + a b.  expn is the reward's (expn(a) ~ exp(-a)), H the double nearest
 * 0.5 ln(2 pi).
 *
 * MINIBATCH.  idx int32 [M] in device memory, 1 <= M <= max_m <= T nenv; a value is s = t nenv + env, an index into the rollout's stores;
 *   position p of the minibatch is sample idx[p].  Rows are gathered through the strides of the stores of the sources of role OBS,
 *   ACTION and LOGP (and VALUE must exist with a critic), of ADVN and -- with a critic -- of RET; a call is refused when one is missing.
 *   A position whose idx lies outside [0, T nenv) is VOID, and so are the positions from M up to the next multiple of the chunk.  A void
 *   position loads +0.0 rows; every kept activation, every delta row and every head value of a void position is +0.0 BY A SELECT AT THE
 *   STORE, never a product with zero (a weight of +inf makes NaN of a void position's own sums, which go nowhere).  Void positions inside
 *   [0, M) are counted in the statistics, and 1 / M is the divisor whatever their number.
 * FORWARD.  POLICY ROWS' INPUT (the normalisation as bound at the call: NORMALISER ROWS say where an update goes) and LAYER on the gathered observation row: h_0 is the normalised
 *   input, h_l layer l's float32 output, bit for bit what phys_batch_policy writes for that row with the same weights.  Every h_l,
 *   l = 0 .. L, is KEPT in a device store for the backward passes.
 * HEAD, ACTOR (A its output width, mu = h_L, a the stored action, ls = log_std as bound by phys_batch_policy_bind_sample and read at the
 *   call; all float32 read as doubles):
 *     is_j = expn(ls_j);  d_j = (a_j - mu_j) * is_j;  q = sum_j d_j * d_j and L = sum_j ls_j, sequential in j from +0.0
 *     logp = (-0.5 * q - L) - A * H;  lr = logp - logp_old;  ratio = expn(-lr);  adv = ADVN[s]
 *     s1 = ratio * adv;  rc = ratio < lo ? lo : ratio > hi ? hi : ratio  (lo = 1 - eps and hi = 1 + eps rounded once on the host)
 *     s2 = rc * adv;  active = !(s2 < s1);  g = active ? -s1 : +0.0
 *     gmu_j = (float)(g * (d_j * is_j));  gls_j = g * (d_j * d_j - 1), a double kept per position
 *   per-position statistics, doubles: policy loss -(active ? s1 : s2); kl = (ratio - 1) - lr; clipped = |ratio - 1| > eps ? 1 : 0.
 * HEAD, CRITIC (network 1, whose last layer has ONE unit; v = h_L[0]): dv = v - RET[s]; gv = (float)(c_v * dv); per-position value loss
 *   (0.5 * dv) * dv.  A clipped value loss is out of scope.
 * BACKWARD, per network, from the last layer down; g_L is gmu (actor) or gv (critic).  delta_l[u] = (float) D(act_l, g_l[u], h_l[u]):
 *     IDENTITY g;  RELU h > 0 ? g : +0.0;  TANH g * (1 - h * h);  ELU h > 0 ? g : g * (h + 1)
 *   For l > 1, g_{l-1}[k] is the fma chain from +0.0 over u ascending to out_l rounded up to 4 (+0.0 in the padding):
 *   acc = fma((double) delta_l[u], (double) W_l[u][k], acc); g stays a double until D has been applied.  The input's gradient is not formed.
 * WEIGHT GRADIENTS.  The positions are cut into CHUNKS of `chunk` consecutive positions, a multiple of 16 in 16 .. 4096 set at
 *   configuration: it is part of the definition, for it fixes the order.  P[c][u][k] is the fma chain from +0.0 over p ascending within
 *   chunk c: acc = fma((double) delta_l[p][u], (double) h_{l-1}[p][k], acc); the bias' partial is the same chain with h = 1 (column
 *   k = in).  dW_l[u][k] = (float)((sum_c P[c][u][k]) * invM), the sum over c sequential and ascending from +0.0, invM = 1 / M rounded
 *   once on the host; db_l alike.
 * LOG_STD AND STATISTICS.  reduce(x[M]) is the rollout's: padded with +0.0 to a multiple of 64, every block of 64 consecutive positions
 *   summed by wv::wave_sum's tree, the block sums added in block order from +0.0.  dls_j = (float)(reduce(gls_j) * invM - c_ent).  The
 *   statistics are eight doubles: reduce(policy loss) * invM, the same of the value loss (+0.0 without a critic), of kl, of clipped, the
 *   entropy L + A * (0.5 + H), the count of void positions in [0, M), M, a spare +0.0.
 * A NaN of one sample stays in that sample's activations and deltas; it reaches the sums that sample enters -- every weight gradient its
 *   chunk's partial enters, and the statistics -- and no other sample's rows.
 *
 *   phys_batch_grad_configure   needs a configured policy and rollout (reconfiguring either releases the gradient rows).  Allocates the
 *                               stores for max_m positions and max_m / chunk partials, and makes the TRANSPOSED PACKING of every layer
 *                               already loaded: per block of 16 k and u-step of 4 the 64 words W[4 ustep + (l >> 4)][16 block + (l & 15)]
 *                               in lane order, zero-padded.  While gradient rows are configured phys_batch_policy_load (and _load_host)
 *                               make it too, on the same stream.  max_m 0 releases.  Refuses a chunk outside the limits, coefficients
 *                               that are not finite or negative, a critic whose last layer is wider than 1.
 *   phys_batch_grad_bind        a caller's float32 tensors for a layer's dW ([out][in], dw_row_stride elements apart, as
 *                               torch.nn.Linear.weight.grad) and db; both NULL: the batch's own again.  phys_batch_grad_bind_log_std: the same
 *                               for log_std's gradient [A].
 *   phys_batch_grad             the launches (forward + head, backward deltas -- where a network has more than one layer --, weight
 *                               partials, reduce, statistics) on `stream`; no host synchronisation.  Refused when a layer was never
 *                               loaded, when m > max_m, when a needed source or the sample's log_std is missing.
 *   phys_batch_grad_stats       the eight doubles to the host; waits for the streams.
 *   phys_batch_grad_download    what = PHYS_GRAD_DW [out][in], _DB [out], _DLS [A] (bound or own), _ACT: the kept activations h_layer
 *                               [m][width], layer 0 .. L; _DELTA [m][out]; _PARTIAL: the fp64 partials [chunks of the last call][out][in + 1];
 *                               _PACKT: the transposed packing.  Dense host memory; m is the last call's.  phys_batch_grad_count: the
 *                               elements such a download writes (-1: no such thing).
 *   phys_batch_debug_grad_launches  diagnostics: the launches so far of the five kernels and of the transposed packing.
 *   phys_batch_debug_grad_mask  measurement aid: bit k set = a call makes launch k (default 31, all five); the stores keep what the last
 *                               full call left, so one launch alone can be timed (tools/grad_rate.py). */
enum { PHYS_GRAD_DW = 0, PHYS_GRAD_DB = 1, PHYS_GRAD_DLS = 2, PHYS_GRAD_ACT = 3, PHYS_GRAD_DELTA = 4, PHYS_GRAD_PARTIAL = 5, PHYS_GRAD_PACKT = 6 };
#define PHYS_GRAD_MINCHUNK 16
#define PHYS_GRAD_MAXCHUNK 4096
#define PHYS_GRAD_NSTATS 8
int phys_batch_grad_configure(phys_batch_t *b, int max_m, int chunk, double clip_eps, double c_v, double c_ent);   /* max_m 0: release */
int phys_batch_grad_bind(phys_batch_t *b, int net, int layer, void *dw_ptr, long long dw_row_stride, void *db_ptr);   /* NULL: the batch's own */
int phys_batch_grad_bind_log_std(phys_batch_t *b, void *ptr);   /* NULL: the batch's own */
int phys_batch_grad(phys_batch_t *b, const void *idx_ptr, int m, void *stream);
int phys_batch_grad_stats(phys_batch_t *b, double *stats /*[8]*/);
long long phys_batch_grad_count(const phys_batch_t *b, int what, int net, int layer);
int phys_batch_grad_download(phys_batch_t *b, int what, int net, int layer, void *host);
int phys_batch_debug_grad_launches(const phys_batch_t *b, long long *launches /*[6]*/);
int phys_batch_debug_grad_mask(phys_batch_t *b, unsigned mask);

/* OPTIMISER ROWS: from the gradients GRADIENT ROWS left, the global gradient norm with its clip coefficient, an Adam step on every weight,
 * every bias and log_std, and each new float32 parameter written to the caller's master tensor, to the policy's packed weights and to the
 * transposed packing, by THREE launches on the caller's stream with every bit defined: phys_batch_policy and the next phys_batch_grad
 * follow on the same stream with no phys_batch_policy_load.  No float atomics, no grid-wide barrier, no kernel waits for another
 * workgroup, no host synchronisation.  The device (csrc/opt_kernels.h), the wave emulator and a numpy restatement (tests/opt_check.py)
 * agree bit for bit.  No stepping kernel is handed any of this.
 *
 * All arithmetic is individually rounded fp64 operations (add, mul, sub, div, sqrt) unless stated as an fma chain; float32 values are
 * read as doubles; conversions to float32 round to nearest even.
 *
 * PARAMETERS, flat order.  The slots (network, layer) in the gradient rows' slot order; within a slot r = u (in + 1) + k with the bias at
 *   column k = in; the A elements of log_std behind the last slot; Q the total count.  Gradients are read from where the gradient rows
 *   write them: the caller's bound tensors, or the batch's own.
 * NORM.  [0, Q) is cut into segments of 256 consecutive parameters (part of the definition).  In segment s lane l runs the fma chain
 *   from +0.0 over i = 0 .. 3 ascending, acc = fma(g, g, acc) with g the gradient of parameter 256 s + 64 i + l (+0.0 past Q); g is
 *   float32, so the product is exact.  The segment's partial is wave_sum(acc).  S = reduce(partials), the rollout's reduce: blocks of 64
 *   by wv::wave_sum's tree, block sums in block order from +0.0.  norm = sqrt(S); finite = norm < +inf (false for a NaN);
 *   raw = max_norm / (norm + 1e-6); scale = raw < 1 ? raw : 1 (max_norm = +inf gives scale = 1).
 * SCALARS, device state the batch owns, doubles: t (steps taken), p1 and p2 (the running products of beta1 and beta2, from 1.0),
 *   skipped (a count).  If !finite the call is SKIPPED: skipped += 1, and t, p1, p2 and every word of every parameter, moment and packing
 *   stay as they are.  Otherwise t += 1; p1 = p1 * beta1; p2 = p2 * beta2; bc1 = 1 - p1; sbc2 = sqrt(1 - p2); step = lr / bc1.  There
 *   is no pow: the host never needs to know how many calls were skipped.
 * STEP, per parameter; m and v are the batch's own float32 moments, +0.0 at configuration; omb1 = 1 - beta1 and omb2 = 1 - beta2 are
 *   rounded once on the host; the update uses m' and v' AS STORED, after rounding to float32:
 *     gs = g * scale
 *     m' = (float)(beta1 * m + omb1 * gs)
 *     v' = (float)(beta2 * v + omb2 * (gs * gs))
 *     den = sqrt(v') / sbc2 + eps
 *     w' = (float)(w - (step * m') / den)
 *   w is read from the caller's master tensor ([out][in] with a row stride and a bias [out], torch.nn.Linear's); w' goes to the master
 *   tensor, to word (u >> 4) * 16 * k4 + (k >> 2) * 64 + (k & 3) * 16 + (u & 15) of the layer's packed weights (b_off + u for a bias) and
 *   to the word of the transposed packing phys_batch_grad_configure describes for (u, k).  The packings' zero padding is never touched.
 *   log_std' goes to the bound log_std tensor alone.
 * STATISTICS, eight doubles: norm, scale, this call's skip (0 or 1), t, skipped, lr, p1, p2.
 * Out of scope: weight decay, per-group learning rates, a KL-adaptive lr on the device, amsgrad, an all-reduce across ranks.
 *
 *   phys_batch_opt_configure    needs configured gradient rows (reconfiguring the policy, the rollout or the gradient rows releases the
 *                               optimiser rows).  Allocates the moments, the partials and the scalars; moments +0.0, t = 0, p1 = p2 = 1.
 *                               Refuses a beta outside [0, 1), an eps that is not finite or <= 0, a max_norm <= 0 or NaN (+inf: no
 *                               clipping).  eps 0 with max_norm 0 releases.
 *   phys_batch_opt_bind_param   the master tensors of a layer, writable: W [out][in], w_row_stride elements apart, and b [out].
 *   phys_batch_opt_bind_log_std the master log_std [A]: it must be the pointer phys_batch_policy_bind_sample names (checked here and at
 *                               the step).
 *   phys_batch_opt_step         the three launches on `stream`.  Refused when a master tensor is not bound, when a layer was never loaded
 *                               (the padding of the packings comes from the first load), when lr is not finite or negative, when no
 *                               phys_batch_grad call has been made.  The master tensors must hold what was last loaded: after the caller
 *                               changes them itself (a checkpoint) phys_batch_policy_load is called as before.
 *   phys_batch_opt_stats        the eight doubles to the host; waits for the streams.
 *   phys_batch_opt_download, _upload   what = PHYS_OPT_M_W [out][in], _M_B [out], _V_W, _V_B of a layer, _M_LS, _V_LS [A], _SCALARS
 *                               (t, p1, p2, skipped: four doubles), and -- download only -- _PARTIALS (the NORM's partials of the last
 *                               call, doubles).  Dense host memory.  An upload of everything a download gave restores a checkpoint bit
 *                               for bit.  phys_batch_opt_count: the elements (-1: no such thing).
 *   phys_batch_debug_opt_launches  diagnostics: the launches so far of the three kernels.
 *   phys_batch_debug_opt_mask   measurement aid: bit k set = a call makes launch k (default 7, all three); the partials and the doubles keep
 *                               what the last full call left, so one launch alone can be timed (tools/opt_rate.py). */
enum { PHYS_OPT_M_W = 0, PHYS_OPT_M_B = 1, PHYS_OPT_V_W = 2, PHYS_OPT_V_B = 3, PHYS_OPT_M_LS = 4, PHYS_OPT_V_LS = 5, PHYS_OPT_SCALARS = 6,
       PHYS_OPT_PARTIALS = 7 };
#define PHYS_OPT_SEG 256
#define PHYS_OPT_NSTATS 8
int phys_batch_opt_configure(phys_batch_t *b, double beta1, double beta2, double eps, double max_norm);   /* eps 0, max_norm 0: release */
int phys_batch_opt_bind_param(phys_batch_t *b, int net, int layer, void *w_ptr, long long w_row_stride, void *b_ptr);
int phys_batch_opt_bind_log_std(phys_batch_t *b, void *ptr);
int phys_batch_opt_step(phys_batch_t *b, double lr, void *stream);
int phys_batch_opt_stats(phys_batch_t *b, double *stats /*[8]*/);
long long phys_batch_opt_count(const phys_batch_t *b, int what, int net, int layer);
int phys_batch_opt_download(phys_batch_t *b, int what, int net, int layer, void *host);
int phys_batch_opt_upload(phys_batch_t *b, int what, int net, int layer, const void *host);
int phys_batch_debug_opt_launches(const phys_batch_t *b, long long *launches /*[3]*/);
int phys_batch_debug_opt_mask(phys_batch_t *b, unsigned mask);

/* NORMALISER ROWS: the running per-column mean and variance of float32 rows -- the observations -- and from them the `mean` and `inv` that
 * INPUT of POLICY ROWS applies, by FOUR launches on the caller's stream with every bit defined.  The policy READS the two tensors
 * phys_batch_policy_bind_norm names and THIS CALL WRITES them (or two tensors of the caller's, phys_batch_norm_bind_output): the policy
 * and the gradient rows read them at every call, so an update acts on the next launch behind it on the stream.  No float atomics, no
 * grid-wide barrier, no kernel waits for another workgroup, no host synchronisation in update or write.  The device
 * (csrc/norm_kernels.h), the wave emulator and a numpy restatement (tests/norm_check.py) agree bit for bit.  No stepping kernel is
 * handed any of this.
 *
 * All arithmetic is individually rounded fp64 operations (add, sub, mul, div, sqrt), no fma; float32 values are read as doubles;
 * conversions to float32 round to nearest even.
 *
 * SOURCE.  Rows of D float32 words, 1 <= D <= PHYS_POL_MAXDIM, laid out as steps x rows: sample s = step * rows + row lies at
 *   ptr + step * step_stride + row * row_stride (strides in words, row_stride >= D).  Unbound, the source is resolved at every call from
 *   the rollout, by the reward's convention: the store of the source of role PHYS_RO_OBS, the batch's own or bound, steps = T,
 *   rows = nenv, with its strides; refused when there is no rollout, no OBS source, or its dim is not D.  Bound
 *   (phys_batch_norm_bind_source), it is any tensor of the caller's: one policy step's live observation (steps = 1, rows = nenv) is a
 *   valid source and needs no rollout.  R = steps * rows, 1 <= R <= max_rows.
 * BLOCKS.  [0, R) is cut into blocks of `block` consecutive samples; `block` is set at configuration, a multiple of 16 in 16 .. 4096, and
 *   PART OF THE DEFINITION, as the gradient rows' chunk is.  The last block may be short; a block may straddle a step.
 * FINITE.  fin(x) = |x| < +inf, false for a NaN.  A value that is not finite is left out by a select: never added, never multiplied by
 *   zero.  A diverged env does not poison a column and does not stop the others from updating it.
 * PASS 1, per block c and column j: a1[c][j], from +0.0 over the block's samples ascending, acc = fin ? acc + x : acc; n1[c][j], the
 *   count of the finite values, an integer.
 * MEAN, per column: S1 the sum of a1[c][j] over c ascending from +0.0; Mj the integer sum of n1, converted exactly;
 *   mb = Mj > 0 ? S1 / Mj : +0.0.
 * PASS 2, per block and column: a2[c][j], from +0.0 ascending, d = x - mb, acc = fin ? acc + d * d : acc.
 * MERGE, per column; the state is three doubles the batch owns, n, mean and m2, +0.0 at configuration.  S2 the sum of a2 over c
 *   ascending.  If Mj == 0 the column is SKIPPED: its state and its two output words stay as they are, skipped[j] += 1.  Otherwise
 *     nn = n + Mj;  delta = mb - mean;  w = Mj / nn
 *     mean' = mean + delta * w
 *     m2'   = (m2 + S2) + (delta * delta) * (n * w)
 *     var = m2' / nn;  inv = 1 / sqrt(var + eps)
 *   (float) mean' and (float) inv go to the outputs, excluded[j] += (R - Mj).  The first update of a column gives mean' = mb and
 *   m2' = S2 exactly (w = 1, n * w = 0).
 * OUTPUTS.  mean and inv, float32 [D] in device memory.  Unbound, they are resolved at every call from phys_batch_policy_bind_norm's
 *   pointers; refused when no normalisation is bound or in_dim != D.  Bound (phys_batch_norm_bind_output), any two tensors.
 * WRITE.  One launch writes (float) mean and (float) inv of every column with n > 0 from the state, with no update: what follows an
 *   upload of a checkpoint.
 * The result depends on nothing but the source's words, `block`, eps and the state: not on the grid, not on whether a lane moves 16
 * bytes or a word, not on how phys_batch_rollout_record was cut into ranges.  As with phys_batch_rollout_normalise, ordering the ranges'
 * streams in front of the call is the caller's job.
 * WHERE THE UPDATE GOES.  The gradient rows read the normalisation AS BOUND AT THE CALL.  An update between the rollout and the first
 * phys_batch_grad makes the first minibatch's ratio differ from 1 (the stored log-probabilities were made with the old words); an update
 * behind the iteration's last phys_batch_opt_step does not.  Both are legitimate; the choice is the caller's.
 * Out of scope: a count cap or forgetting factor; a return or value normaliser; merging states across ranks (a download, a host merge and
 * an upload is possible and bit-exact); per-column masks.
 *
 *   phys_batch_norm_configure   dim columns, block, the most samples of a call, eps (finite, > 0); allocates the state, the partials and
 *                               the counts; n = mean = m2 = +0.0.  dim 0 releases.  Waits for the batch's streams.  The normaliser rows
 *                               STAY configured when the policy, the rollout, the gradient rows or the optimiser rows are reconfigured:
 *                               they resolve at the call and hold no pointer of theirs.
 *   phys_batch_norm_bind_source a tensor of the caller's as the source (ptr NULL: the rollout's OBS store again).  Refuses a stride
 *                               smaller than dim.
 *   phys_batch_norm_bind_output two tensors of the caller's as the outputs (both NULL: the policy's bound normalisation again).  Refuses
 *                               one pointer without the other.
 *   phys_batch_norm_update      the four launches on `stream`: sum, mean, sq, merge.  Refuses an unresolved source or output and
 *                               R > max_rows.
 *   phys_batch_norm_write       the one launch on `stream`.
 *   phys_batch_norm_stats       eight doubles, summarised on the host from the per-column arrays; waits for the streams: R of the last
 *                               call, its blocks, the columns it updated, the columns it skipped, the values it excluded (R - Mj over the
 *                               columns it updated), the calls so far, the largest n[j], a spare +0.0.
 *   phys_batch_norm_download, _upload   what = PHYS_NORM_N, _MEAN, _M2, _SKIPPED, _EXCLUDED: doubles [D]; download only: _MB, _COUNTS
 *                               (Mj as doubles) [D] and _PARTIALS (a1 then a2, [blocks of the last call][D] each).  Dense host memory.
 *                               An upload of everything a download gave, followed by phys_batch_norm_write, restores a checkpoint bit for
 *                               bit.  phys_batch_norm_count: the doubles (-1: no such thing).
 *   phys_batch_debug_norm_launches  diagnostics: the launches so far of sum, mean, sq, merge and write.
 *   phys_batch_debug_norm_mask  measurement aid: bit k set = an update makes launch k (default 15, all four); the partials and the state
 *                               keep what the last full call left, so one launch alone can be timed (tools/norm_rate.py). */
enum { PHYS_NORM_N = 0, PHYS_NORM_MEAN = 1, PHYS_NORM_M2 = 2, PHYS_NORM_SKIPPED = 3, PHYS_NORM_EXCLUDED = 4, PHYS_NORM_MB = 5,
       PHYS_NORM_COUNTS = 6, PHYS_NORM_PARTIALS = 7 };
#define PHYS_NORM_MINBLOCK 16
#define PHYS_NORM_MAXBLOCK 4096
#define PHYS_NORM_MAXROWS (1ll << 30)
#define PHYS_NORM_NSTATS 8
int phys_batch_norm_configure(phys_batch_t *b, int dim, int block, long long max_rows, double eps);   /* dim 0: release */
int phys_batch_norm_bind_source(phys_batch_t *b, const void *ptr, int steps, int rows, long long step_stride, long long row_stride);   /* NULL: the rollout's OBS store */
int phys_batch_norm_bind_output(phys_batch_t *b, void *mean_ptr, void *inv_ptr);   /* both NULL: the policy's bound normalisation */
int phys_batch_norm_update(phys_batch_t *b, void *stream);     /* four launches */
int phys_batch_norm_write(phys_batch_t *b, void *stream);      /* one launch */
int phys_batch_norm_stats(phys_batch_t *b, double *stats /*[8]*/);
long long phys_batch_norm_count(const phys_batch_t *b, int what);
int phys_batch_norm_download(phys_batch_t *b, int what, void *host);
int phys_batch_norm_upload(phys_batch_t *b, int what, const void *host);
int phys_batch_debug_norm_launches(const phys_batch_t *b, long long *launches /*[5]*/);
int phys_batch_debug_norm_mask(phys_batch_t *b, unsigned mask);   /* default 15 */

/* DRAW ROWS: the two random inputs of an iteration -- the standard normal rows SAMPLE of POLICY ROWS reads as eps, and the permutation an
 * epoch's minibatches are cut from (the idx of GRADIENT ROWS) -- as functions of ONE seed and counters of the batch's own, with every bit
 * defined.  One launch per env range on the caller's stream fills the normal rows; one launch writes a permutation.  The device
 * (csrc/draw_kernels.h), the wave emulator and a numpy restatement (tests/draw_check.py) agree bit for bit.  The result for an env
 * depends on (seed, env_base + env, column, the env's call count) alone: not on the range, the grid, the stream or the order of calls for
 * other envs.  No stepping kernel is handed any of this; the observation, action and task rows' own noise stays uniform and untouched.
 *
 * All arithmetic is individually rounded fp64 operations (add, sub, mul, div, sqrt), no fma, no library call; the conversion to float32
 * rounds to nearest even.  philox(c0, c1, c2, c3) is Philox4x32-10 (OBSERVATION ROWS) with the key (seed & 0xffffffff, seed >> 32).
 *
 * LOGN.  logn(x) ~ ln x for a finite double x > 0 (csrc/logn.h):
 *   1. selects, before anything else: a NaN gives that NaN; x < 0 (and -inf) gives NaN; +0.0 and -0.0 give -inf; +inf gives +inf.
 *   2. x = m 2^e, by integer operations on the bits (a subnormal x is first multiplied by 2^54, exact, and e lowered by 54): m in [1, 2)
 *      has x's mantissa; if m >= 1.4142135623730951 (the double nearest sqrt 2), m = m / 2 (exact) and e = e + 1.  So m lies in
 *      [sqrt 1/2, sqrt 2).
 *   3. f = m - 1, exact.  s = f / (2 + f).  z = s s.
 *   4. P = 1/23; P = 1/k + z P for k = 21, 19, ..., 3: the doubles nearest 1/k, one multiply and one add a step.
 *   5. t = s + (s z) P;  r = 2 t.
 *   6. logn = e ln2_hi + (e ln2_lo + r), with ln2_hi = 6.93147180369123816490e-01 and ln2_lo = 1.90821492927058770002e-10 (REWARD ROWS'
 *      expn's constants; e ln2_hi is exact).
 *   logn(1) = +0.0.  On the points the draws can produce the relative error is measured by tests/test_draw.py (DESIGN 4.3 has the figure).
 *
 * NORMAL ROWS.  phys_batch_draw(b, env0, n, stream) fills float32 rows [nenv][A], 1 <= A <= PHYS_DRAW_MAXA.  counts[env], a uint32 per
 *   env, starts at 0, is incremented behind the env's draw and wraps.  For env i and column j:
 *     w = philox(env_base + i, j >> 2, counts[i], 4)          (word 3: 0 .. 3 are the observation's, the action's and the task's two)
 *     a = w[j & 2];  b = w[(j & 2) + 1]
 *     u = (a + 0.5) 2^-32, exact, in (0, 1);   theta = b 2^-32, exact, in [0, 1)
 *     rad = sqrt(-2 logn(u));   (sn, cs) = sincos2pi(theta) of TASK ROWS
 *     z = rad * ((j & 1) ? sn : cs);   the row takes (float) z, one rounding.
 *   |z| <= sqrt(66 ln 2) ~ 6.76; no rejection, no loop.  Envs outside the range and words past column A are not touched.
 *   DESTINATION.  Unbound, the rows go to the eps tensor with the stride that phys_batch_policy_bind_sample names, resolved at every call
 *   (refused when no sample is bound or the actor's output width is not A); phys_batch_draw_bind names another tensor.
 *
 * SHUFFLE.  phys_batch_draw_perm(b, epoch, stream) writes int32 perm[0 .. n), a bijection of [0, n) keyed by (seed, epoch),
 *   1 <= n <= PHYS_DRAW_MAXPERM.  b is the smallest even number of bits with 2^b >= max(n, 4); h = b / 2; mask = 2^h - 1.  For index i:
 *     x = i
 *     repeat:  (L, R) = (x >> h, x & mask);  for r = 0 .. 5: (L, R) = (R, L ^ (philox(R, r, epoch, 5)[0] & mask));  x = L << h | R
 *     while x >= n                                                                                       (cycle walking)
 *     perm[i] = x
 *   The six rounds are a bijection of [0, 2^b), so the values >= n a walk from i < n meets are distinct: a walk ends within
 *   2^b - n + 1 <= max(3 n, 4) applications.  The destination is the batch's own buffer (phys_batch_draw_perm_ptr) or a bound int32 tensor;
 *   phys_batch_grad(b, perm + k M, M, ...) reads minibatch k from it.
 *
 * A checkpoint of a run's randomness is the seed, the counts (phys_batch_draw_download) and the caller's epoch counter.
 * Out of scope: uniform or truncated draws as a kind; Gaussian noise inside the observation, action and task kernels; more than one draw
 * configuration per batch; A > 64; a sort-based shuffle.
 *
 *   phys_batch_draw_configure   A columns (0: no normal rows), the shuffle's n (0: no shuffle), the seed, env_base (what a rank that
 *                               holds envs [k nenv, (k + 1) nenv) of a larger run passes: k nenv).  Allocates the counts, zeroed, and the
 *                               batch's permutation.  A 0 with perm_n 0 releases.  Waits for the batch's streams.  The draw rows STAY
 *                               configured when the policy, the rollout, the gradient, the optimiser or the normaliser rows are
 *                               reconfigured: they resolve at the call and hold no pointer of theirs.
 *   phys_batch_draw_bind        a float32 tensor of the caller's, rows row_stride >= A words apart, as the destination (NULL: the policy's
 *                               eps again).
 *   phys_batch_draw_bind_perm   an int32 tensor of the caller's of n words as the shuffle's destination (NULL: the batch's own again).
 *   phys_batch_draw             the one launch on `stream`.  Refuses: not configured, A 0, a range beyond nenv, no destination.
 *   phys_batch_draw_perm        the one launch on `stream`.  Refuses: not configured, no shuffle configured.
 *   phys_batch_draw_perm_ptr    where the permutation is written, in device memory (NULL: none).
 *   phys_batch_draw_dim         A and n.
 *   phys_batch_draw_rows, _perm_rows   the destination's rows [nenv][A], dense, and the permutation [n] to the host; wait for the streams.
 *   phys_batch_draw_download, _upload  the counts, uint32 [nenv]; wait for the streams.
 *   phys_batch_debug_draw_launches     diagnostics: the launches so far of the normal rows and of the shuffle. */
#define PHYS_DRAW_MAXA 64
#define PHYS_DRAW_MAXPERM (1ll << 30)
int phys_batch_draw_configure(phys_batch_t *b, int A, long long perm_n, unsigned long long seed, unsigned env_base);   /* A 0, perm_n 0: release */
int phys_batch_draw_bind(phys_batch_t *b, void *ptr, long long row_stride);   /* NULL: the policy's eps */
int phys_batch_draw_bind_perm(phys_batch_t *b, void *ptr);                    /* NULL: the batch's own buffer */
int phys_batch_draw(phys_batch_t *b, int env0, int n, void *stream);          /* one launch */
int phys_batch_draw_perm(phys_batch_t *b, unsigned epoch, void *stream);      /* one launch */
void *phys_batch_draw_perm_ptr(const phys_batch_t *b);
int phys_batch_draw_dim(const phys_batch_t *b, int *A, long long *perm_n);
int phys_batch_draw_rows(phys_batch_t *b, float *host);
int phys_batch_draw_perm_rows(phys_batch_t *b, int *host);
int phys_batch_draw_download(phys_batch_t *b, unsigned *counts_host);
int phys_batch_draw_upload(phys_batch_t *b, const unsigned *counts_host);
int phys_batch_debug_draw_launches(const phys_batch_t *b, long long *launches /*[2]*/);

/* measurement aid: on = every substep of a fused launch evaluates every output (IMU sensors, body quaternions), although
 * only the last substep's values can be read; off (default) = those are formed by the substeps whose values are read */
int phys_batch_set_all_outputs_every_substep(phys_batch_t *b, int on);
/* Launch-order balancing (on by default for batches of 2048 envs and more): every launch records what each env cost
 * and the next launch starts the expensive envs first, so the wave slots finish together instead of the launch waiting
 * for whichever slot drew the slow envs last.  Results do not depend on it (envs are independent). */
int phys_batch_set_balance(phys_batch_t *b, int on);
/* diagnostics (batches of 2048 envs and more, balancing on): what the last stepping launch cost every env, in units of 64
 * shader clocks from the env's first to its last instruction ([nenv] unsigned) -- the figure the launch order is sorted by */
int phys_batch_download_cost(phys_batch_t *b, unsigned *host);
/* the shader clock the last stepping launch ran at, measured by the kernel itself: every env's span in shader clocks (s_memtime)
 * over the same span on the constant 100 MHz clock (s_memrealtime), summed over the envs.  -1 where the launch-cost arrays do not
 * exist (batches under 2048 envs, balancing off). */
int phys_batch_measured_shader_clock(phys_batch_t *b, double *hz);
/* diagnostics: envs that the last stepping launch over the env range starting at env0 passed on to the 127-row instantiation (the
 * count its pass reported: envs that met a substep with more than 63 constraint rows or 16 contacts) */
int phys_batch_wide_pass_envs(phys_batch_t *b, int env0);
/* validation aid: entries (and walker tickets) left in the hand-over lists of the batch's env ranges once its streams are idle
 * -- 0 whatever the mode: the pass behind the fast kernel clears what it walked, and a fast kernel whose pass does not walk the
 * list is not given one; -1 on error */
int phys_batch_debug_handover_pending(phys_batch_t *b);
/* on (default): stepping launches of the Cassie instantiations run the row-capped fast kernel first and the full kernel
 * only finishes envs that needed more than 31 constraint rows in some substep; off: the full kernel alone (same results,
 * bit for bit -- a validation / measurement aid) */
/* measurement aid: with timing enabled every stepping launch records a HIP event pair around the kernel that does its work
 * (the row-capped fast kernel where one exists, else the step kernel) on the launch's stream; phys_batch_kernel_timing waits
 * for the batch's streams and returns the number of launches since the last call and the sum of their kernel durations -- the
 * same quantity rocprofv3 --kernel-trace --stats averages, also when launches of several env ranges overlap */
int phys_batch_enable_kernel_timing(phys_batch_t *b, int on);
int phys_batch_kernel_timing(phys_batch_t *b, int *launches, double *total_ms);
int phys_batch_set_fast_rows(phys_batch_t *b, int on);
/* Which form of the two-wave fast kernel the stepping launches of an env range take (round 6): 0 = the fast kernel and, behind it, the
 * pass that walks the list of envs it handed over (an env's remaining substeps then run as one serial chain while the range's stream
 * waits); 1 = the fast kernel that finishes a substep it cannot hold IN PLACE -- the 63-row code inside the same workgroup -- and goes
 * on with the next one itself; 2 (default) = per range by what its recent launches needed: in place once a launch handed envs over,
 * back to the plain form after eight launches in a row (as the device reports them) in which no env left the fast tier.  Same results, bit for bit.  The in-place form costs
 * a workload that never leaves the fast tier 1.8 % and gains 8 - 24 % on one that does (profiles/round6/inplace_ab.txt). */
int phys_batch_set_inplace(phys_batch_t *b, int mode);
/* diagnostics: env ranges whose next stepping launch takes the in-place form */
int phys_batch_debug_inplace_ranges(const phys_batch_t *b);
/* ... and the stepping launches of the two-wave fast kernel so far, by form */
int phys_batch_debug_form_launches(const phys_batch_t *b, long long *plain, long long *inplace);
/* 2 (default): the row-capped fast kernels run in their two-wave form -- two wavefronts per env, the mass-matrix stage group
 * (centres of mass, composite inertias, M, its two factorisations) on the second wave beside the first wave's collision,
 * velocity and constraint-row stages; 1: one wavefront per env.  Same results, bit for bit (a measurement aid). */
int phys_batch_set_waves_per_env(phys_batch_t *b, int waves);
/* Stepping launches of the row-capped fast kernels in CHUNKS (1 = off .. 7; default: 7 for launches over the whole batch, 2 for
 * launches over an env range, whose neighbours' launches fill the end of its queue anyway -- 3 for a range's launch of at most 25
 * substeps, the shape of a consumer that fences every few substeps): a launch of at least 2048 envs and 10 substeps is
 * dispatched as `chunks` workgroups per env, each stepping a share of the substeps (5 at least) from the state the chunk before it
 * stored -- the jobs the GPU's workgroup slots queue up are that much shorter, and so is the time the slots stand idle at the
 * end of a launch while the last-started jobs finish.  Same results, bit for bit (a chunk ends and the next begins exactly
 * like two launches). */
int phys_batch_set_chunks(phys_batch_t *b, int chunks);
/* THE STEP SUMS: contact forces, touches and actuator work added up over the substeps of a fused launch.
 * A stepping launch keeps a policy step's 50 substeps on the device, and everything readable afterwards (PHYS_F_BODY_CFRC, ctrl,
 * actuator_velocity, sensordata) is the LAST substep's.  The reference's users step cassie_sim_step_pd 50 - 60 times per policy step
 * and, over those calls, average cassie_sim_foot_forces, ask whether a body touched the ground at any time and integrate torque and
 * mechanical power.  With the step sums on, a launch does that itself, into one row of CM_SUM_DIM doubles per env (PHYS_F_STEP_SUMS;
 * layout and exact definitions: CM_SUM_* in cm_model.h):
 *   phys_batch_step_sums_enable(b, on)   on != 0: allocates the block on first use (unless a caller's tensor is bound to the field) and
 *                                        switches accumulation on; 0: off again -- nothing below happens and every launch is what it
 *                                        was without this call (the block keeps its last contents).  Off by default.
 *     ZEROING        every stepping launch (phys_batch_step, phys_batch_step_range) first zeroes the rows of ITS env range, on its own
 *                    stream, ahead of its first substep; rows outside the range are left alone, so ranges on several streams each
 *                    own their rows.
 *     ACCUMULATION   ... then adds every substep it integrates, in substep order (each sum is the sequential sum from +0.0, every
 *                    product rounded on its own), whatever tier, pass or chunk of the launch finished the substep: a substep the fast
 *                    kernel hands to the 63-row or 127-row code is counted once, by the code that finishes it.  Means are the
 *                    caller's: divide by CM_SUM_COUNT.
 *     LEFT ALONE     forward passes, phys_batch_derive, phys_batch_forward_kinematics, phys_batch_end_episodes and restarts neither
 *                    zero nor add: the rows read what the last stepping launch over them left.
 *     DIVERGED ENVS  an env whose launch raised warning bit 8: CM_SUM_COUNT = the substeps it finished, every other entry unspecified.
 *     FORMS          accumulating launches take the two-wave fast kernel's sibling with the accumulation code (the lean fast kernels
 *                    hold none) + the list-walking passes, never the in-place form; a batch set to one wave per env, or profiled, the
 *                    full 63-row / 127-row form alone.  Cost: README, "step sums" (tools/step_sums_rate.py). */
int phys_batch_step_sums_enable(phys_batch_t *b, int on);
/* diagnostics: how many substeps of the last stepping launch the fast kernel completed for every env ([nenv] ints; less than
 * the launch's substep count = the env was handed over to the full kernel there).  Meaningful after a launch that ran the fast
 * kernel: not with the read-out enabled, fast rows off, or a batch of at most 512 envs stepping at most 4 substeps per launch
 * (those go through the full kernel alone: one launch instead of two) */
int phys_batch_download_progress(phys_batch_t *b, int *host);

/* validation aid: fills every CU's LDS with NaN bit patterns before the next launch (LDS is neither initialised nor
 * cleared between kernels) -- a step kernel that read LDS it had not written would then show it */
int phys_batch_debug_poison_lds(phys_batch_t *b);

/* validation aid: run the generic instantiation of the step kernel (dof-tree topology read from the model at run
 * time) even when the model matches one of the compile-time-topology instantiations */
int phys_batch_set_generic_kernel(phys_batch_t *b, int on);

/* per-stage shader-clock stamps of the next launches: [nenv][48] long long on the host after the call (profiling aid) */
int phys_batch_profile_step(phys_batch_t *b, long long *host_stamps);
/* same for one launch of nsub fused substeps: the stamps are those of the last substep */
int phys_batch_profile_substeps(phys_batch_t *b, int nsub, long long *host_stamps);

size_t phys_sizeof_model(void);
const char *phys_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
