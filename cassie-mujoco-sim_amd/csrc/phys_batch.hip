/*
 * phys_batch.hip -- device half of the inner C ABI (include/cassie_phys.h): N
 * Cassie environments resident in HBM and the launch of the one-wave-per-env
 * step kernel (physics_kernel.h).  Replaces the reference's per-sim
 * mj_makeData / mj_step1 / mj_step2 / mj_forward / mj_deleteData calls
 * (reference src/cassiemujoco.c:441-447, :1130-1134, :1029, :452).
 *
 * Layout in HBM: every per-env field is one env-major array [nenv][dim] of fp64,
 * so the wave that owns env e touches one contiguous row per field.  The model
 * is a single cm_model_t (or one per env for domain randomisation).
 */
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "cassie_phys.h"
#include "device_mem.h"
#include "small_launch.h"
#include "step_launch.h"
#include "step_policy.h"

void phys_set_last_error(const char *s);

constexpr int DEFAULT_TRAY_WAVES = 2; /* the 40-dof model's default form (by measurement: round 5, 17.77 against 15.72 M with one wave, profiles/round5/tray_two_waves_ab.txt; round 4 had it at -7.5 %) */

struct phys_batch {
    int nenv = 0, device = 0;
    cm_model_t host_model;          /* copy of the shared model (sizes) */
    DevBuf<cm_model_t> d_models;    /* 1 or nenv models in HBM */
    DevBuf<cm_envparams_t> d_envparams; /* null, or one parameter block per env (phys_batch_randomize: PhysIO::envparams) */
    int model_stride = 0;
    bool generic_kernel = false;   /* validation aid: never pick a compile-time-topology instantiation */
    int dim[PHYS_F_COUNT];
    int stride[PHYS_F_COUNT];       /* doubles between consecutive envs' rows (= dim unless bound with a stride) */
    DevBuf<double> d_field[PHYS_F_COUNT]; /* the batch's own, or a caller's (phys_batch_bind) */
    DevBuf<int> d_warn, d_info;
    DevBuf<float> d_hfield;
    size_t hfield_stride = 0, hfield_floats = 0; /* stride 0: one grid shared by all envs; else one grid of hfield_floats per env */
    /* a bank of terrains (phys_batch_set_hfield_bank): d_hfield then holds nterrain grids and env e stands on grid d_terrain_index[e]
     * (PhysIO::hfield_index; the array is created on first use and may be the caller's) */
    int nterrain = 0;
    DevBuf<int> d_terrain_index;
    /* what the kernels around the step kernel are configured with (small_launch.h: the records a launch's arguments are built from);
     * a pointer into one of the batch's buffers is filled in at the launch, from the buffer */
    ck::ScanCfg scan = {};          /* the height scan (phys_batch_scan_configure): its pattern is d_scan_offsets */
    DevBuf<double> d_scan_offsets;
    ck::DepthCfg depth = {};        /* the depth image (phys_batch_depth_configure, _bind_pose, _set_geoms, _bind_ids: the caller's arrays) */
    long long depth_launches[2] = {0, 0}; /* launches of the static / the scene kernel (phys_batch_debug_depth_launches) */
    ck::RayCfg rays = {};           /* the range sensors (phys_batch_rays_configure, _set_geoms, _bind_ids, _bind_normals): their table is d_rays */
    DevBuf<ck::RayDef> d_rays;
    long long ray_launches = 0;     /* launches of the ray kernel (phys_batch_debug_ray_launches) */
    hipStream_t stream = nullptr;
    hipStream_t recent_streams[4] = {nullptr, nullptr, nullptr, nullptr}; /* streams of the most recent launches (callers may pass
                                       their own, and ranges of one batch may be in flight on several at once) */
    int recent_next = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mark = nullptr;
    bool use_applied = false;       /* qfrc_applied / xfrc_applied are passed only once uploaded */
    bool pd_mode = false;
    int drive_mode = CM_DRIVE_OFF;
    DevBuf<cm_drive_state_t> d_drive; /* [nenv], allocated when a drive mode is first selected */
    bool use_pd_dtarget = false, use_pd_torque = false;
    DevBuf<long long> d_prof;
    bool all_outputs = false;       /* measurement aid: see PhysIO::all_outputs_every_substep */
    DevBuf<cm_ext_t> d_ext;

    /* ---- the launcher's (launch(): the rules are step_policy.h's, these are the settings they read and the state they keep) ---- */
    bool fast_rows = true;          /* use the row-capped fast instantiation where one exists (phys_batch_set_fast_rows) */
    int waves_per_env = 2;          /* two-wave form of the fast instantiations (phys_batch_set_waves_per_env) */
    int waves_per_env_tray = DEFAULT_TRAY_WAVES; /* ... of the 40-dof instantiations (CASSIE_TRAY_TWO_WAVES=0/1 overrides the default: A/B aid) */
    int inplace_mode = 2;           /* form of the two-wave fast kernel (phys_batch_set_inplace; ck::next_inplace) */
    long long form_launches[2] = {0, 0};   /* stepping launches of the two-wave fast kernel in the plain / the in-place form (diagnostics) */
    bool step_sums = false;         /* stepping launches zero and accumulate PHYS_F_STEP_SUMS (phys_batch_step_sums_enable) */
    /* launch-order balancing (see ck::cassie_order_kernel) */
    bool balance = true;
    DevBuf<unsigned> d_cost, d_cost_wall; /* per-env span of the last launch in 64 shader clocks / in 100 MHz ticks */
    DevBuf<int> d_order;            /* a permutation of the env ids of every range it was last sorted for, the identity elsewhere */
    std::vector<int> order_ident;   /* 0 .. nenv - 1, the source of the resets of retired ranges' segments */
    ck::RangeTable ranges;          /* the env ranges stepping launches went over: their order segment, form, launches since a sort */
    DevBuf<int> d_progress;         /* [nenv] substeps completed by the row-capped fast instantiation (PhysIO::progress) */
    /* stepping launches of the fast instantiations in chunks (PhysIO::nchunk): chunks per env-launch asked for (1 = off), the
     * words the chunks of an env hand over through, and the tag of the last chunked launch */
    int chunks = ck::DEFAULT_CHUNKS_WHOLE, chunks_range = ck::DEFAULT_CHUNKS_RANGE; /* (launches over the whole batch / over an env range) */
    bool chunks_default = true;    /* nobody has asked for a chunk count: a range's SHORT launches go as three (ck::launch_chunks) */
    DevBuf<int> d_chunk_flag;
    int chunk_seq = 0;
    bool chunks_allowed = true;     /* (false: this device does not place workgroup w on XCD w % 8 -- launches stay in one piece) */
    /* the placement rule is a property of the QUEUE a launch goes to (a CU-masked stream, another partition mode ...): every stream
     * is probed the first time a chunked launch is about to go to it -- with the step kernel's own workgroup shape -- and the
     * kernel checks every hand-over besides (PhysIO::chunk_fault: a word in pinned host memory a consumer sets when it finds its
     * producer on another XCD; launches stay in one piece from then on) */
    std::vector<std::pair<hipStream_t, bool>> probed_streams;
    HostWords chunk_fault;
    bool chunk_fault_reported = false;
    /* the hand-over list (PhysIO::handover_list): env ids per range, [count, ticket] pairs indexed by a range's first env, and
     * -- in pinned host memory the device writes -- the number of envs the last launch of a range handed over; the same for the
     * second list: what the 63-row pass hands on to the 127-row pass (models on the Cassie dof tree) */
    DevBuf<int> d_handover_list, d_handover_count, d_handover_list2, d_handover_count2;
    HostWords handover_seen, handover_seen2;
    /* per-kernel timing (phys_batch_kernel_timing): event pairs around the kernel of every stepping launch that does the work */
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;

    DevBuf<double> d_scratch_out;    /* [nenv][nv + nsensordata + nu]: where phys_batch_forward_kinematics sends qacc / sensordata / actuator_velocity */
    /* episodes on the device (phys_batch_end_episodes): the rules, the bank's rows (ep), the per-env arrays PHYS_EP_* and the bank */
    bool episodes = false;
    ck::EpisodeCfg ep = {};
    DevBuf<char> d_ep[PHYS_EP_ARRAYS]; /* (ints, or doubles: PHYS_EP_TERMINAL; the batch's own or a caller's) */
    DevBuf<const double> d_ep_bank;    /* (a copy of the host's rows, or the caller's device rows) */
    /* placed restarts (phys_batch_place_configure): the anchor (0: off), the footprint and the table of what a placement moves
     * (worked out of the model once) in HBM, and the per-env arrays PHYS_PLACE_* (the batch's own or a caller's; the next terrains the caller's only) */
    ck::PlaceCfg place = {};
    DevBuf<ck::PlaceTable> d_place_table;
    DevBuf<double> d_place_offsets, d_place_pose, d_place_ground;
    /* the bank of full states (phys_batch_state_configure): its groups and the slots of the bank in use (state.nslots 0: not configured;
     * state.bank is filled in at the launch), the batch's own rows and -- while bound -- a caller's in their place */
    ck::StateCfg state = {};
    DevBuf<unsigned long long> d_state;
    int state_own_slots = 0;
    unsigned long long *state_bound = nullptr;
    DevBuf<int> d_state_staged;     /* a host array of slots on its way to a launch (phys_batch_state_stage_slots) */
    int state_staged_cap = 0;
    /* probes (phys_batch_probes_configure): the list and the quantities (probes.nprobes 0: not configured; the pointers are filled in at
     * the launch, from the buffers), the table and the classes of the full list's geoms in HBM, the read-out block and the scratch
     * outputs of the probes' OWN forward pass -- no stepping launch is handed either -- and the contact words (the batch's own, or a caller's) */
    ck::ProbeCfg probes = {};
    DevBuf<ck::ProbeDef> d_probes;
    DevBuf<int> d_probe_geoms;
    int probe_ngeom = 0;
    DevBuf<cm_ext_t> d_probe_ext;
    DevBuf<double> d_probe_scratch;  /* [nenv] rows of qacc | sensordata | actuator_velocity | xpos | xquat, one array after the other */
    DevBuf<int> d_probe_contacts;
    long long probe_launches[2] = {0, 0}; /* forward passes / reductions of phys_batch_probe (phys_batch_debug_probe_launches) */
    /* observation rows (phys_batch_obs_configure): the record (obs.nterms 0: not configured; its pointers are filled in at the launch, from
     * the buffers), every term's first column, the column table, the rows (the batch's own or a caller's, floats or doubles) with their
     * stride in elements, the per-env frame counts and the caller's input array.  No stepping launch reads any of it */
    ck::ObsCfg obs = {};
    std::vector<int> obs_term_col;
    DevBuf<ck::ObsCol> d_obs_cols;
    DevBuf<char> d_obs_rows;
    long long obs_srow = 0;
    DevBuf<unsigned> d_obs_frames;
    long long obs_launches = 0;     /* launches of cassie_obs_kernel (phys_batch_debug_obs_launches) */
    /* reward rows (phys_batch_reward_configure): the record (reward.nterms 0: not configured; its pointers are filled in at the launch,
     * from the buffers), the term table with the fields as slots, the rewards (the batch's own or a caller's, floats or doubles) with their
     * stride in elements, the term rows (empty: not written) with theirs, the per-env returns and final returns.  No stepping launch reads
     * any of it */
    ck::RewardCfg reward = {};
    DevBuf<ck::RewardTerm> d_reward_terms;
    DevBuf<char> d_reward, d_reward_trows;
    long long reward_srew = 0, reward_sterm = 0;
    DevBuf<double> d_reward_ret, d_reward_final;
    long long reward_launches = 0;  /* launches of cassie_reward_kernel (phys_batch_debug_reward_launches) */
    /* action rows (phys_batch_act_configure): the record (act.ncols 0: not configured; its pointers are filled in at the launch, from the
     * buffers; the actions, the input and the delays are the caller's arrays), the column table, the rows (the batch's own or a caller's,
     * floats or doubles) with their stride in elements, the per-env state [delay_max + 3][ncols] and call counts.  No stepping launch
     * reads any of it: a step reads the command fields the call wrote */
    ck::ActCfg act = {};
    DevBuf<ck::ActCol> d_act_cols;
    DevBuf<char> d_act_rows;
    long long act_srow = 0;
    DevBuf<double> d_act_state;
    DevBuf<unsigned> d_act_counts;
    long long act_launches = 0;     /* launches of cassie_act_kernel (phys_batch_debug_act_launches) */
    /* task rows (phys_batch_task_configure): the record (task.ncols 0: not configured; its pointers are filled in at the launch, from the
     * buffers), the column table, the reference table [task_nframes][task_tcols] (phys_batch_task_set_table), the rows (the batch's own
     * or a caller's, floats or doubles) with their stride in elements, the per-env state [ncols], words [3][ncols] and call counts.  No
     * stepping launch reads any of it: a step reads the command fields the call wrote */
    ck::TaskCfg task = {};
    DevBuf<ck::TaskCol> d_task_cols;
    DevBuf<double> d_task_table;
    int task_nframes = 0, task_tcols = 0;
    DevBuf<char> d_task_rows;
    long long task_srow = 0;
    DevBuf<double> d_task_state;
    DevBuf<unsigned> d_task_words, d_task_counts;
    long long task_launches = 0;    /* launches of cassie_task_kernel (phys_batch_debug_task_launches) */
    /* event rows (phys_batch_events_configure): the record (events.ncols 0: not configured; its pointers are filled in at the launch, from
     * the buffers), the column table, the rows (the batch's own or a caller's, floats or doubles) with their stride in elements, the done
     * words (the batch's own or a caller's), the per-env state [2][ncols][nenv], words [ncols][nenv] and call counts.  No stepping launch
     * reads any of it */
    ck::EventCfg events = {};
    DevBuf<ck::EventCol> d_event_cols;
    DevBuf<char> d_event_rows;
    long long event_srow = 0;
    DevBuf<int> d_event_flags;
    DevBuf<double> d_event_state;
    DevBuf<unsigned> d_event_words, d_event_counts;
    long long event_launches = 0;   /* launches of cassie_event_kernel (phys_batch_debug_events_launches) */
    /* policy rows (phys_batch_policy_configure): the record (policy.nnets 0: not configured; the input, the normalisation, the outputs and
     * the sample are the caller's arrays) and the packed weights and biases of every layer.  No stepping launch reads any of it */
    ck::PolicyCfg policy = {};
    DevBuf<float> d_policy_packed;
    long long policy_launches = 0;  /* launches of cassie_policy_kernel (phys_batch_debug_policy_launches) */
    /* rollout rows (phys_batch_rollout_configure): the record (rollout.nsrc 0: not configured; the pointers of its stores are filled in at the
     * launch, from the buffers; bound sources are the caller's arrays), the store of every source, ADV, RET and ADVN (the batch's own or a
     * caller's), and the per-env partials with the statistics behind them: q1 [nenv] | q2 [nenv] | {mean, std, inv, the last sum}.  No
     * stepping launch reads any of it */
    ck::RolloutCfg rollout = {};
    DevBuf<unsigned> d_ro_store[ck::ROLLOUT_MAXSRC];
    DevBuf<unsigned> d_ro_adv, d_ro_ret, d_ro_advn;
    DevBuf<double> d_ro_q;
    long long rollout_launches[3] = {0, 0, 0};  /* launches of record, finish and normalise (phys_batch_debug_rollout_launches) */
    /* gradient rows (phys_batch_grad_configure): the record (grad.max_m 0: not configured; bound gradient tensors are the caller's), the kept
     * activations, the deltas, the fp64 partials of the weight sums, the transposed packing of the weights, the per-position doubles of the
     * head with the eight statistics behind them, and the batch's own gradient floats.  No stepping launch reads any of it */
    ck::GradCfg grad = {};
    DevBuf<float> d_grad_act, d_grad_delta, d_grad_packt, d_grad_own;
    DevBuf<double> d_grad_part, d_grad_pos;
    int grad_last_m = 0;            /* the m of the last phys_batch_grad (what the downloads of activations and deltas hold) */
    unsigned grad_mask = 31u;       /* measurement aid (phys_batch_debug_grad_mask): which of the five launches a call makes */
    long long grad_launches[6] = {0, 0, 0, 0, 0, 0};  /* forward, backward, partials, reduce, statistics, transposed packings */
    /* optimiser rows (phys_batch_opt_configure): the record (opt.on 0: not configured; the master tensors are the caller's), the moments
     * (m [Q], then v [Q]), the NORM's partials with the doubles behind them.  No stepping launch reads any of it */
    ck::OptCfg opt = {};
    DevBuf<float> d_opt_mom;
    DevBuf<double> d_opt_part;
    unsigned opt_mask = 7u;                           /* measurement aid (phys_batch_debug_opt_mask): which of the three launches a call makes */
    long long opt_launches[3] = {0, 0, 0};            /* squares, scalars, step */
    /* normaliser rows (phys_batch_norm_configure): the record (norm.on 0: not configured; it holds no pointer of the policy's or the
     * rollout's: both are resolved at the call), the state [NORM_STATE_ROWS][D], the partials and the blocks' counts.  No stepping launch
     * reads any of it */
    ck::NormCfg norm = {};
    DevBuf<double> d_norm_state, d_norm_part;
    DevBuf<int> d_norm_cnt;
    unsigned norm_mask = 15u;                         /* measurement aid (phys_batch_debug_norm_mask): which of the four launches an update makes */
    long long norm_launches[5] = {0, 0, 0, 0, 0};     /* sum, mean, sq, merge, write */
    /* draw rows (phys_batch_draw_configure): the record (draw.on 0: not configured; it holds no pointer of the policy's: the eps of the
     * sample binding is resolved at the call), the envs' call counts and the batch's own permutation.  No stepping launch reads any of it */
    ck::DrawCfg draw = {};
    DevBuf<unsigned> d_draw_counts;
    DevBuf<int> d_draw_perm;
    long long draw_launches[2] = {0, 0};              /* normal rows, shuffle */
};

static bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    std::string msg = std::string("HIP error in ") + what + ": " + hipGetErrorString(e);
    phys_set_last_error(msg.c_str());
    fprintf(stderr, "cassie_phys: %s\n", msg.c_str());
    return false;
}

static ck::PhysIO make_io(phys_batch *b, int nsub, int integrate) {
    ck::PhysIO io;
    memset(&io, 0, sizeof io);
    io.models = b->d_models;
    io.model_stride = b->model_stride;
    io.envparams = b->d_envparams;
    io.nenv = b->nenv; io.nsub = nsub; io.integrate = integrate;
    io.sq = b->stride[PHYS_F_QPOS]; io.sqv = b->stride[PHYS_F_QVEL]; io.sv = b->host_model.nv; io.su = b->host_model.nu;
    io.ssd = b->stride[PHYS_F_SENSORDATA]; io.sb = b->host_model.nbody;
    io.qpos = b->d_field[PHYS_F_QPOS]; io.qvel = b->d_field[PHYS_F_QVEL];
    io.qacc_warmstart = b->d_field[PHYS_F_QACC_WARMSTART]; io.time = b->d_field[PHYS_F_TIME];
    io.ctrl = b->d_field[PHYS_F_CTRL];
    io.qfrc_applied = b->use_applied ? b->d_field[PHYS_F_QFRC_APPLIED] : nullptr;
    io.xfrc_applied = b->use_applied ? b->d_field[PHYS_F_XFRC_APPLIED] : nullptr;
    io.qacc = b->d_field[PHYS_F_QACC]; io.sensordata = b->d_field[PHYS_F_SENSORDATA];
    io.actuator_velocity = b->d_field[PHYS_F_ACTUATOR_VELOCITY];
    io.warn = b->d_warn; io.info = b->d_info;
    io.xpos_out = b->d_field[PHYS_F_XPOS]; io.xquat_out = b->d_field[PHYS_F_XQUAT];
    io.body_cfrc = b->d_field[PHYS_F_BODY_CFRC];
    io.hfield = b->d_hfield;
    io.hfield_stride = b->hfield_stride;
    if (b->nterrain > 0) { io.hfield_index = b->d_terrain_index; io.hfield_nterrain = b->nterrain; }
    if (b->pd_mode) {
        io.pd_ptarget = b->d_field[PHYS_F_PD_PTARGET]; io.pd_kp = b->d_field[PHYS_F_PD_KP]; io.pd_kd = b->d_field[PHYS_F_PD_KD];
    }
    io.drive_mode = b->d_drive ? b->drive_mode : CM_DRIVE_OFF;
    if (io.drive_mode != CM_DRIVE_OFF) {
        io.drive_state = b->d_drive;
        io.drive_cmd = b->d_field[PHYS_F_DRIVE_CMD];
        io.meas = b->d_field[PHYS_F_MEAS];
        if (io.drive_mode == CM_DRIVE_PD || io.drive_mode == CM_DRIVE_PD_SAFE) {
            io.pd_ptarget = b->d_field[PHYS_F_PD_PTARGET]; io.pd_kp = b->d_field[PHYS_F_PD_KP]; io.pd_kd = b->d_field[PHYS_F_PD_KD];
            io.pd_dtarget = b->use_pd_dtarget ? b->d_field[PHYS_F_PD_DTARGET] : nullptr;
            io.pd_torque = b->use_pd_torque ? b->d_field[PHYS_F_PD_TORQUE] : nullptr;
        }
    }
    io.all_outputs_every_substep = b->all_outputs ? 1 : 0;
    io.prof = b->d_prof;
    io.ext = b->d_ext;
    if (b->balance && b->d_order) { io.order = b->d_order; io.cost = b->d_cost; io.cost_wall = b->d_cost_wall; }
    return io;
}

/* Model, terrain and ext-buffer updates are blocking copies that must not overtake (or be overtaken by) a kernel that
 * is still in flight on the batch's stream or on the caller's: wait for both first. */
static bool quiesce(phys_batch *b) {
    bool ok = hip_ok(hipStreamSynchronize(b->stream), "hipStreamSynchronize");
    for (hipStream_t r : b->recent_streams)
        if (r && r != b->stream) ok = hip_ok(hipStreamSynchronize(r), "hipStreamSynchronize(caller stream)") && ok;
    return ok;
}

static void note_stream(phys_batch *b, hipStream_t s) {
    for (hipStream_t r : b->recent_streams) if (r == s) return;
    b->recent_streams[b->recent_next] = s;
    b->recent_next = (b->recent_next + 1) % 4;
}

/* the stream an entry point enqueues on: the caller's, or the batch's own -- noted, so that quiesce waits for it */
static hipStream_t launch_stream(phys_batch *b, void *stream) {
    const hipStream_t s = stream ? (hipStream_t)stream : b->stream;
    note_stream(b, s);
    return s;
}

/* envs [env0, env0 + n), or envs first, first + stride, ... (count of them), inside the batch? */
static bool range_ok(const phys_batch *b, int env0, int n) {
    return env0 >= 0 && n >= 0 && (size_t)env0 + (size_t)n <= (size_t)b->nenv;
}
static bool strided_ok(const phys_batch *b, int first, int stride, int count) {
    return first >= 0 && stride >= 1 && count >= 0 && (count == 0 || (size_t)first + (size_t)(count - 1) * (size_t)stride < (size_t)b->nenv);
}

/* what the kernels around the step kernel read of the batch (small_launch.h), as make_io hands the same to the step kernel */
static ck::BatchView view_of(const phys_batch *b) {
    ck::BatchView v = {b->d_models, b->model_stride, b->d_envparams, b->d_hfield, b->hfield_stride, b->d_terrain_index, b->nterrain};
    ck::view_sizes(v, b->host_model);
    v.sq = b->stride[PHYS_F_QPOS]; v.sqv = b->stride[PHYS_F_QVEL]; v.ssd = b->stride[PHYS_F_SENSORDATA];
    v.qpos = b->d_field[PHYS_F_QPOS]; v.qvel = b->d_field[PHYS_F_QVEL]; v.warm = b->d_field[PHYS_F_QACC_WARMSTART];
    v.ctrl = b->d_field[PHYS_F_CTRL]; v.qacc = b->d_field[PHYS_F_QACC]; v.time = b->d_field[PHYS_F_TIME];
    v.sens = b->d_field[PHYS_F_SENSORDATA]; v.actvel = b->d_field[PHYS_F_ACTUATOR_VELOCITY];
    v.meas = b->d_drive ? b->d_field[PHYS_F_MEAS].get() : nullptr;
    v.drive = b->d_drive; v.warn = b->d_warn;
    v.xpos = b->d_field[PHYS_F_XPOS]; v.xquat = b->d_field[PHYS_F_XQUAT];
    v.xpos_w = b->d_field[PHYS_F_XPOS]; v.xquat_w = b->d_field[PHYS_F_XQUAT];
    v.pd_ptarget = b->d_field[PHYS_F_PD_PTARGET]; v.pd_kp = b->d_field[PHYS_F_PD_KP]; v.pd_kd = b->d_field[PHYS_F_PD_KD];
    v.pd_dtarget = b->d_field[PHYS_F_PD_DTARGET]; v.pd_torque = b->d_field[PHYS_F_PD_TORQUE]; v.drive_cmd = b->d_field[PHYS_F_DRIVE_CMD];
    v.qfrc_applied = b->use_applied ? b->d_field[PHYS_F_QFRC_APPLIED].get() : nullptr;
    v.xfrc_applied = b->use_applied ? b->d_field[PHYS_F_XFRC_APPLIED].get() : nullptr;
    v.ep_steps = b->episodes ? (int *)b->d_ep[PHYS_EP_STEPS].get() : nullptr; v.ep_count = b->episodes ? (int *)b->d_ep[PHYS_EP_COUNT].get() : nullptr;
    v.params_w = b->d_envparams;
    return v;
}
/* the refusal of an entry point: its name in front of a check's message (small_launch.h) */
static int refuse(const char *entry, const char *why) {
    phys_set_last_error((std::string(entry) + ": " + why).c_str());
    return -1;
}

/* The step kernel's instantiations per model family, by form (step_plan.h; null: the family has no such form).  Each is instantiated
 * explicitly in one of the kernels_*.hip translation units. */
using ck::launch_step;
using ck::FAST_ROWS; using ck::FAST_ROWS_TRAY; using ck::MID_ROWS; using ck::WIDE_ROWS;
using ck::TopoCassie32; using ck::TopoCassieTray38; using ck::TopoRuntime;
/* plain cassie.xml (FEAT 0) and cassie_hfield.xml (FEAT_HFIELD): all three tiers.  The fast forms are LEAN (step_plan.h: is_lean_form --
 * the kernel's trailing SERVE parameter is FEAT_LEAN), their _PROF forms add the stage stamps, every other form carries both FEAT_READOUT
 * and FEAT_PROF (the default) */
using ck::FEAT_LEAN; using ck::FEAT_PROF; using ck::FEAT_READOUT; using ck::FEAT_FULL;
template <int FEAT>
static const ck::StepLauncher CASSIE_FORMS[ck::FORM_COUNT] = {
    launch_step<32, TopoCassie32, FEAT>,                                              /* FORM_ALONE (+ the one-wave lookup pass) */
    launch_step<32, TopoCassie32, FEAT, MID_ROWS, 2, false, 1>,                      /* FORM_ALONE_2W: 512 registers a lane */
    launch_step<32, TopoCassie32, FEAT, WIDE_ROWS, 2, false, 1>,                     /* FORM_WIDE */
    launch_step<32, TopoCassie32, FEAT, FAST_ROWS, 1, false, 1, 0, FEAT_LEAN>,        /* FORM_FAST */
    launch_step<32, TopoCassie32, FEAT, FAST_ROWS, 2, false, 2, 0, FEAT_LEAN>,        /* FORM_FAST_2W */
    launch_step<32, TopoCassie32, FEAT, FAST_ROWS, 2, false, 2, MID_ROWS, FEAT_LEAN>, /* FORM_FAST_INPLACE */
    nullptr,                                                                          /* FORM_MID_WALK */
    launch_step<32, TopoCassie32, FEAT, MID_ROWS, 2, true>,                          /* FORM_MID_WALK_2W */
    launch_step<32, TopoCassie32, FEAT, WIDE_ROWS, 2, true, 1>,                      /* FORM_WIDE_WALK */
    launch_step<32, TopoCassie32, FEAT, FAST_ROWS, 1, false, 1, 0, FEAT_PROF>,        /* FORM_FAST_PROF */
    launch_step<32, TopoCassie32, FEAT, FAST_ROWS, 2, false, 2, 0, FEAT_PROF>,        /* FORM_FAST_2W_PROF */
};
/* cassie_tray_box.xml without height-field pairs: fast (47 rows) and 63 rows */
static const ck::StepLauncher TRAY_FORMS[ck::FORM_COUNT] = {
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS>,                                              /* FORM_ALONE */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, MID_ROWS, 2>,                                 /* FORM_ALONE_2W */
    nullptr,                                                                                            /* FORM_WIDE */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 1, false, 1, 0, FEAT_LEAN>,    /* FORM_FAST */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2, false, 2, 0, FEAT_READOUT>, /* FORM_FAST_2W (keeps the read-out code: kernels_tray_2w.hip) */
    nullptr,                                                                                            /* FORM_FAST_INPLACE */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, MID_ROWS, 1, true>,                           /* FORM_MID_WALK */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, MID_ROWS, 2, true>,                           /* FORM_MID_WALK_2W */
    nullptr,                                                                                            /* FORM_WIDE_WALK */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 1, false, 1, 0, FEAT_PROF>,    /* FORM_FAST_PROF */
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2, false, 2, 0, FEAT_FULL>,    /* FORM_FAST_2W_PROF */
};
/* FORM_ALONE only: the Cassie topology with both height-field and box pairs, the tray model with height-field pairs, any other model */
static const ck::StepLauncher CASSIE_ALL_FORMS[ck::FORM_COUNT] = {launch_step<32, TopoCassie32, ck::FEAT_ALL>};
static const ck::StepLauncher TRAY_HFIELD_FORMS[ck::FORM_COUNT] = {launch_step<40, TopoCassieTray38, ck::FEAT_ALL>};
static const ck::StepLauncher GENERIC32_FORMS[ck::FORM_COUNT] = {launch_step<32, TopoRuntime, ck::FEAT_ALL>};
static const ck::StepLauncher GENERIC40_FORMS[ck::FORM_COUNT] = {launch_step<40, TopoRuntime, ck::FEAT_ALL>};
/* ... by family (ck::pick_family) */
static const ck::StepLauncher *const FAMILY_FORMS[ck::FAMILY_COUNT] = {
    CASSIE_FORMS<0>, CASSIE_FORMS<ck::FEAT_HFIELD>, CASSIE_ALL_FORMS, TRAY_FORMS, TRAY_HFIELD_FORMS, GENERIC32_FORMS, GENERIC40_FORMS,
};
/* The second table: the same forms for a launch that accumulates the step-sums block (PhysIO::sums).  The lean fast forms map to their
 * FEAT_SUMS siblings (kernels_*_sums.hip: the two-wave form alone -- ck::launch_forms answers no other fast form for such a launch; null
 * otherwise, and for the profiled forms); every other form, FEAT_FULL, is its own entry of the first table (ck::feat_sums: a run-time test
 * of the pointer).  By family; null: a family of full forms alone. */
using ck::FEAT_SUMS;
template <int FEAT>
static const ck::StepLauncher CASSIE_SUMS_FAST[ck::FORM_COUNT] = {
    nullptr, nullptr, nullptr, nullptr,
    launch_step<32, TopoCassie32, FEAT, FAST_ROWS, 2, false, 2, 0, FEAT_SUMS>,        /* FORM_FAST_2W */
};
static const ck::StepLauncher TRAY_SUMS_FAST[ck::FORM_COUNT] = {
    nullptr, nullptr, nullptr, nullptr,
    launch_step<40, TopoCassieTray38, ck::FEAT_WAVEPAIRS, FAST_ROWS_TRAY, 2, false, 2, 0, FEAT_READOUT | FEAT_SUMS>, /* FORM_FAST_2W */
};
static const ck::StepLauncher *const FAMILY_SUMS_FAST[ck::FAMILY_COUNT] = {
    CASSIE_SUMS_FAST<0>, CASSIE_SUMS_FAST<ck::FEAT_HFIELD>, nullptr, TRAY_SUMS_FAST, nullptr, nullptr, nullptr,
};
/* the kernel of a pass: from the second table for an accumulating launch (*sums_inst: it is a FEAT_SUMS instantiation), null where there is none */
static ck::StepLauncher pass_kernel(ck::StepFamily fam, int form, bool sums, bool *sums_inst) {
    *sums_inst = false;
    if (!sums || !ck::is_fast_form(form)) return FAMILY_FORMS[fam][form];
    *sums_inst = FAMILY_SUMS_FAST[fam] && FAMILY_SUMS_FAST[fam][form];
    return *sums_inst ? FAMILY_SUMS_FAST[fam][form] : nullptr;
}

/* A launch in chunks hands an env's state from one workgroup to another through the L2 both share (wave.h: publish_global): the
 * chunks of an env are workgroups a multiple of 8 apart, and workgroup w runs on XCD w % 8.  That assignment is checked here, once
 * per batch of a size that could be chunked: a grid of 1024 workgroups reports where it ran. */
extern "C" __global__ void __launch_bounds__(128) cassie_xcd_probe_kernel(int *xcc) {
    if (threadIdx.x == 0) xcc[blockIdx.x] = (int)(wv::hw_id() >> 32) & 7;
}
/* does the queue behind stream s place workgroup w on XCD w % 8 (in the sense that workgroups 8 apart share an XCD)?  A grid of 1024
 * workgroups of the step kernel's shape (128 threads) reports where it ran. */
static bool workgroups_go_round_the_xcds(hipStream_t s) {
    constexpr int NWG = 1024;
    DevBuf<int> d;
    int h[NWG];
    bool ok = d.alloc(NWG, false, "XCD probe");
    if (ok) {
        hipLaunchKernelGGL(cassie_xcd_probe_kernel, dim3(NWG), dim3(128), 0, s, d.get());
        ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        for (int w = 8; ok && w < NWG; ++w) ok = h[w] == h[w % 8];
    }
    return ok;
}
static bool stream_may_chunk(phys_batch *b, hipStream_t s) {
    if (!b->chunks_allowed) return false;
    if (b->chunk_fault.host() && *(volatile int *)b->chunk_fault.host()) {
        b->chunks_allowed = false;
        if (!b->chunk_fault_reported) {
            b->chunk_fault_reported = true;
            fprintf(stderr, "cassie_phys: a chunk of a stepping launch ran on another XCD than the chunk before it (a CU-masked stream or a partition mode that "
                            "breaks the round-robin placement): the envs concerned carry warning bit 16, launches go in one piece from now on\n");
        }
        return false;
    }
    for (const auto &ps : b->probed_streams) if (ps.first == s) return ps.second;
    const bool ok = workgroups_go_round_the_xcds(s);
    if (b->probed_streams.size() < 64) b->probed_streams.emplace_back(s, ok);
    return ok;
}

/* The launch of the fast kernel over n envs in chunks (PhysIO::nchunk, chunk_seq, chunk_flag, chunk_fault): as many as the policy
 * gives a launch of this length (ck::launch_chunks), where the stream places workgroups round the XCDs -- asked last: the first
 * question about a stream is a probe launch and a synchronisation */
static void set_chunks(phys_batch *b, ck::PhysIO &io, int n, int nsub, hipStream_t s) {
    const int nchunk = b->chunks_allowed ? ck::launch_chunks(n, b->nenv, nsub, b->chunks, b->chunks_range, b->chunks_default) : 1;
    io.nchunk = 1;
    if (nchunk <= 1 || !stream_may_chunk(b, s)) return;
    io.nchunk = nchunk;
    if (b->chunk_seq >= (1 << 24)) { /* (the tag has 25 bits: start over once NOTHING is in flight on the device -- the words of
                                       * envs in flight on a stream this batch does not remember must not be cleared under them --
                                       * and the clearing itself is complete before the next chunk can publish) */
        (void)hipDeviceSynchronize();
        (void)hipMemsetAsync(b->d_chunk_flag, 0, sizeof(int) * (size_t)b->nenv, s);
        (void)hipStreamSynchronize(s);
        b->chunk_seq = 0;
    }
    io.chunk_seq = ++b->chunk_seq;
    io.chunk_flag = b->d_chunk_flag;
    io.chunk_fault = b->chunk_fault.dev();
}

/* The first list's count word and the `seen` word of the range starting at env0 change their meaning with the form of the range's
 * fast kernel (ck::LaunchRange): start the new form from zero (stream-ordered).  (The host's store to the seen word is not ordered
 * against passes or order kernels of the old form still queued, which may write it after: that delays or repeats a change of form,
 * the results are the same bits either way.) */
static void reset_range_words(phys_batch *b, int env0, hipStream_t s) {
    (void)hipMemsetAsync(b->d_handover_count + 2 * (size_t)env0, 0, 2 * sizeof(int), s);
    b->handover_seen.host()[env0] = 0;
}

/* The record of the range [env0, env0 + n) of a stepping launch on stream s (ck::RangeTable::claim), after undoing, in stream order,
 * what the records it retired stood for: their segment of the order array goes back to the identity, the words of one that was in
 * the in-place form start over as a count and a ticket */
static ck::LaunchRange *claim_range(phys_batch *b, int env0, int n, hipStream_t s) {
    std::vector<ck::LaunchRange> retired;
    ck::LaunchRange *range = b->ranges.claim(env0, n, retired);
    for (const ck::LaunchRange &g : retired) {
        if (b->d_order && !hip_ok(hipMemcpyAsync(b->d_order + g.env0, b->order_ident.data() + g.env0, sizeof(int) * (size_t)g.n, hipMemcpyHostToDevice, s), "hipMemcpy(order reset)")) return nullptr;
        if (g.inplace) reset_range_words(b, g.env0, s);
    }
    return range;
}

/* per-kernel timing: records the event in front of a stepping launch and returns the one that goes behind its first kernel (or null) */
static hipEvent_t timing_begin(phys_batch *b, hipStream_t s) {
    if (b->ev_used == b->ev_pool.size() && b->ev_pool.size() < 65536) { /* (launches beyond that between two queries go untimed) */
        hipEvent_t a = nullptr, c = nullptr;
        if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&c) == hipSuccess) b->ev_pool.emplace_back(a, c);
    }
    if (b->ev_used == b->ev_pool.size()) return nullptr;
    (void)hipEventRecord(b->ev_pool[b->ev_used].first, s);
    return b->ev_pool[b->ev_used++].second;
}

/* Where a read-out pass of the probes sends everything a forward pass stores (launch()'s `readout`): the read-out block, and arrays
 * [nenv] with dense rows in place of the caller's qacc, sensordata, actuator_velocity, xpos and xquat */
struct ReadoutPass { cm_ext_t *ext; double *qacc, *sensordata, *actuator_velocity, *xpos, *xquat; };

/* One launch: the PhysIO, the range's record, the policy's answers (step_policy.h), the plan (step_plan.h), its passes, the report */
static int launch(phys_batch *b, int nsub, int integrate, hipStream_t s, bool scratch_outputs = false, int env0 = 0, int n = -1, const ReadoutPass *readout = nullptr) {
    ck::PhysIO io = make_io(b, nsub, integrate);
    if (n < 0) n = b->nenv;
    io.env0 = env0; io.nenv = n;
    if (readout) {
        /* the probes' forward pass: into ITS read-out block (the batch's own, phys_batch_enable_ext, is not this pass's business, and the
         * override is this launch's alone: another range's launch may be made from another thread meanwhile), and nothing a caller can
         * read is stored to -- the step outputs and the body poses go to the probes' scratch, the per-body contact forces and the
         * solver statistics nowhere */
        const cm_model_t &m = b->host_model;
        io.ext = readout->ext;
        io.qacc = readout->qacc; io.sv = m.nv;
        io.sensordata = readout->sensordata; io.ssd = m.nsensordata;
        io.actuator_velocity = readout->actuator_velocity;
        io.xpos_out = readout->xpos; io.xquat_out = readout->xquat;
        io.body_cfrc = nullptr; io.info = nullptr;
    }
    if (!integrate) { io.order = nullptr; io.cost = nullptr; io.cost_wall = nullptr; } /* forward / read-out passes: one substep, nothing to balance (identity order) */
    if (scratch_outputs) {
        /* a read-out pass: the step outputs the caller's fields hold (sensordata and actuator_velocity of the last STEP feed
         * the encoder / motor models of the next one; qacc) stay as they are */
        const cm_model_t &m = b->host_model;
        io.qacc = b->d_scratch_out; io.sv = m.nv;
        io.sensordata = b->d_scratch_out + (size_t)b->nenv * m.nv; io.ssd = m.nsensordata;
        io.actuator_velocity = io.sensordata + (size_t)b->nenv * m.nsensordata;
    }
    note_stream(b, s);
    /* the family, and the forms of this launch while its range is in the plain form */
    const cm_model_t &hm = b->host_model;
    const ck::StepFamily fam = ck::pick_family(hm, b->generic_kernel);
    const ck::StepLauncher *family = FAMILY_FORMS[fam];
    const bool has_inplace = family[ck::FORM_FAST_INPLACE] != nullptr;
    const bool prof = io.prof != nullptr;
    /* the step sums (phys_batch_step_sums_enable): a stepping launch zeroes the rows of its range on its stream, ahead of its first
     * substep, and its passes add to them; forward / read-out passes are not handed the block */
    const bool sums = integrate && b->step_sums && b->d_field[PHYS_F_STEP_SUMS];
    if (sums) {
        io.sums = b->d_field[PHYS_F_STEP_SUMS]; io.sums_stride = b->stride[PHYS_F_STEP_SUMS];
        if (!hip_ok(hipMemsetAsync(io.sums + (size_t)env0 * CM_SUM_DIM, 0, sizeof(double) * CM_SUM_DIM * (size_t)n, s), "hipMemset(step sums)")) return -1;
    }
    auto forms_if = [&](bool inplace) {
        return ck::launch_forms(fam, has_inplace, hm.maxefc, integrate, io.ext != nullptr, n, nsub, b->fast_rows, b->waves_per_env, b->waves_per_env_tray, inplace, prof, sums);
    };
    ck::StepForms forms = forms_if(false);
    const bool fast = ck::is_fast_form(forms.first);
    /* the range's record: of a stepping launch that uses the order array or a fast kernel (forward / read-out passes claim nothing) */
    ck::LaunchRange *range = nullptr;
    if (integrate && (io.order || fast) && !(range = claim_range(b, env0, n, s))) return -1;
    const hipEvent_t ev_after = b->timing && integrate ? timing_begin(b, s) : nullptr;
    /* a fast kernel first: its record of completed substeps, its launch in chunks, the hand-over lists of the passes behind it, its form */
    ck::HandoverLists hl = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ck::StepGrids grids = {(unsigned)n, (unsigned)n, (unsigned)n};
    if (fast) {
        io.progress = b->d_progress;
        set_chunks(b, io, n, nsub, s);
        hl.list1 = b->d_handover_list; hl.count1 = b->d_handover_count + 2 * (size_t)env0; hl.seen1 = b->handover_seen.dev() + env0;
        if (forms.wide) { hl.list2 = b->d_handover_list2; hl.count2 = b->d_handover_count2 + 2 * (size_t)env0; hl.seen2 = b->handover_seen2.dev() + env0; }
        const int seen = *(volatile int *)(b->handover_seen.host() + env0);
        grids = ck::pass_grids(n, seen, forms.wide ? b->handover_seen2.host()[env0] : 0, forms.wide);
        if ((forms.first == ck::FORM_FAST_2W || forms.first == ck::FORM_FAST_2W_PROF) && has_inplace) {
            const bool was = range->inplace;
            /* (a profiled launch takes the plain form -- the stamps are in FORM_FAST_2W_PROF alone -- and the range goes with it) */
            /* (... and so does an accumulating launch: its kernel is the plain form's FEAT_SUMS sibling, which the count of the lean forms' launches leaves out) */
            range->inplace = !prof && !sums && ck::next_inplace(was, seen, b->inplace_mode, io.order != nullptr);
            if (was != range->inplace) reset_range_words(b, env0, s);
            if (!sums) ++b->form_launches[range->inplace ? 1 : 0];
            forms = forms_if(range->inplace);
        }
    }
    const ck::StepPlan plan = ck::plan_step(io, forms, hl, grids);
    for (int i = 0; i < plan.n; ++i) {
        const ck::StepPass &p = plan.pass[i];
        bool sums_inst = false;
        const ck::StepLauncher kernel = pass_kernel(fam, p.form, p.io.sums != nullptr, &sums_inst);
        if (!kernel) { (void)hip_ok(hipErrorInvalidDeviceFunction, "cassie_step_kernel launch (no instantiation of this form)"); return -1; }
        /* (the policy never pairs them; a plan that does is not launched: the code for it is not in the kernel) */
        if (ck::step_sums_refuses(p.form, p.io.ext != nullptr, p.io.integrate, p.io.prof != nullptr, p.io.sums != nullptr, sums_inst)) {
            (void)hip_ok(hipErrorInvalidValue, "cassie_step_kernel launch (a lean fast form with the read-out block, a forward pass, the stage stamps or the step sums)");
            return -1;
        }
        kernel(p.grid, s, p.io);
        if (!hip_ok(hipGetLastError(), "cassie_step_kernel launch")) return -1;
        if (i == 0 && ev_after) (void)hipEventRecord(ev_after, s);   /* (the first kernel of the launch does the work: per-kernel timing) */
    }
    /* the next launch's order from this one's per-env cost, when it is due (ck::order_kernel_due); it reports the in-place count of the
     * range when the in-place form ran */
    if (io.order && ck::order_kernel_due(nsub, ++range->launches_since_sort)) {
        range->launches_since_sort = 0;
        const bool inplace = forms.first == ck::FORM_FAST_INPLACE;
        hipLaunchKernelGGL(ck::cassie_order_kernel, dim3(1), dim3(ck::ORDER_THREADS), 0, s, b->d_cost, b->d_order, n, env0,
                           inplace ? hl.count1 : (int *)nullptr, inplace ? hl.seen1 : (volatile int *)nullptr);
        if (!hip_ok(hipGetLastError(), "cassie_order_kernel launch")) return -1;
    }
    return 0;
}

/* optional inputs are handed to the kernel only once somebody uploaded or bound them */
static void note_field_in_use(phys_batch *b, int field) {
    if (field == PHYS_F_QFRC_APPLIED || field == PHYS_F_XFRC_APPLIED) b->use_applied = true;
    if (field == PHYS_F_PD_DTARGET) b->use_pd_dtarget = true;
    if (field == PHYS_F_PD_TORQUE) b->use_pd_torque = true;
}

/* rows [env0, env0 + n) of a field between a dense host array and HBM (dense, or strided when the field is a column
 * block of a caller-owned tensor), asynchronously on the batch's stream */
static bool copy_rows(phys_batch *b, int field, void *host, int env0, int n, bool to_device, const char *what) {
    if (!b->d_field[field]) { phys_set_last_error("this field is allocated by phys_batch_derive (PHYS_F_HEIGHT_SCAN: phys_batch_scan_configure, PHYS_F_DEPTH: phys_batch_depth_configure, PHYS_F_RAYS: phys_batch_rays_configure, PHYS_F_PROBES: phys_batch_probes_configure); call it first"); return false; }
    const size_t row = (size_t)b->dim[field], st = (size_t)b->stride[field];
    double *dev = b->d_field[field] + st * env0;
    if (n == 0) return true;
    if (st == row)
        return hip_ok(to_device ? hipMemcpyAsync(dev, host, sizeof(double) * row * n, hipMemcpyHostToDevice, b->stream)
                                : hipMemcpyAsync(host, dev, sizeof(double) * row * n, hipMemcpyDeviceToHost, b->stream), what);
    return hip_ok(to_device ? hipMemcpy2DAsync(dev, sizeof(double) * st, host, sizeof(double) * row, sizeof(double) * row, n, hipMemcpyHostToDevice, b->stream)
                            : hipMemcpy2DAsync(host, sizeof(double) * row, dev, sizeof(double) * st, sizeof(double) * row, n, hipMemcpyDeviceToHost, b->stream), what);
}

extern "C" {

phys_batch_t *phys_batch_create(const cm_model_t *model, int nenv, int device) {
    if (!model || nenv <= 0) { phys_set_last_error("phys_batch_create: bad arguments"); return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        const char *msg = "phys_batch_create: no HIP device available -- this library has no CPU fallback";
        phys_set_last_error(msg);
        fprintf(stderr, "cassie_phys: %s\n", msg);
        return nullptr;
    }
    if (device < 0 || device >= ndev) { phys_set_last_error("phys_batch_create: bad device index"); return nullptr; }
    if (!hip_ok(hipSetDevice(device), "hipSetDevice")) return nullptr;
    phys_batch *b = new phys_batch;
    b->nenv = nenv; b->device = device;
    if (const char *tw = getenv("CASSIE_TRAY_TWO_WAVES")) b->waves_per_env_tray = atoi(tw) ? 2 : 1;
    b->host_model = *model;
    cm_model_sync_params(&b->host_model);
    b->host_model.env_geom = 0; b->host_model.env_springs = 0; /* (no blocks yet: the model's own geometry and springs) */
    model = &b->host_model;
    const int d[PHYS_F_COUNT] = {model->nq, model->nv, model->nv, 1, model->nu, model->nv, model->nbody * 6,
                                 model->nv, model->nsensordata, model->nu, model->nbody * 3, model->nbody * 4,
                                 model->nu, model->nu, model->nu, model->nbody * 3,
                                 model->nu + 1, CM_MEAS_DIM, model->nu, model->nu, CM_DRV_DIM, model->nv * model->nv, 0, 0, 0, CM_SUM_DIM, 0};
    const size_t n = (size_t)nenv;
    bool ok = true;
    for (int f = 0; f < PHYS_F_COUNT; ++f) {
        b->dim[f] = d[f]; b->stride[f] = d[f];
        if (f == PHYS_F_DERIVED || f == PHYS_F_QM) continue; /* large and optional: allocated by the first phys_batch_derive */
        if (f == PHYS_F_HEIGHT_SCAN) continue;              /* sized and allocated by phys_batch_scan_configure */
        if (f == PHYS_F_DEPTH) continue;                    /* ... by phys_batch_depth_configure */
        if (f == PHYS_F_RAYS) continue;                     /* ... by phys_batch_rays_configure */
        if (f == PHYS_F_STEP_SUMS) continue;                /* allocated by phys_batch_step_sums_enable */
        if (f == PHYS_F_PROBES) continue;                   /* sized and allocated by phys_batch_probes_configure */
        ok = ok && b->d_field[f].alloc(n * (d[f] > 0 ? d[f] : 1), true, "field");
    }
    ok = ok && b->d_models.alloc(1, false, "model");
    ok = ok && hip_ok(hipMemcpy(b->d_models, model, sizeof(cm_model_t), hipMemcpyHostToDevice), "hipMemcpy(model)");
    ok = ok && b->d_warn.alloc(n, true, "warn") && b->d_info.alloc(4 * n, true, "info");
    if (nenv >= 2048) { /* fewer envs than a couple per wave slot leave nothing to balance */
        b->order_ident.resize(n);
        for (int e = 0; e < nenv; ++e) b->order_ident[(size_t)e] = e;
        ok = ok && b->d_order.alloc(n, false, "order");
        ok = ok && hip_ok(hipMemcpy(b->d_order, b->order_ident.data(), sizeof(int) * n, hipMemcpyHostToDevice), "hipMemcpy(order)");
        ok = ok && b->d_cost.alloc(n, true, "cost") && b->d_cost_wall.alloc(n, true, "cost, wall clock");
    }
    ok = ok && b->d_progress.alloc(n, true, "progress") && b->d_chunk_flag.alloc(n, true, "chunk words");
    if (const char *ck = getenv("CASSIE_CHUNKS")) { b->chunks = b->chunks_range = atoi(ck) > 1 ? (atoi(ck) < 7 ? atoi(ck) : 7) : 1; b->chunks_default = false; } /* (A/B switch) */
    ok = ok && b->chunk_fault.alloc(1, "chunk fault word");
    ok = ok && b->d_handover_list.alloc(n, false, "hand-over list") && b->d_handover_count.alloc(2 * n, true, "hand-over counts");
    ok = ok && b->handover_seen.alloc(n, "hand-over seen");
    ok = ok && b->d_handover_list2.alloc(n, false, "second hand-over list") && b->d_handover_count2.alloc(2 * n, true, "second hand-over counts");
    ok = ok && b->handover_seen2.alloc(n, "second hand-over seen");
    ok = ok && hip_ok(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking), "hipStreamCreate");
    ok = ok && hip_ok(hipEventCreate(&b->ev0), "hipEventCreate") && hip_ok(hipEventCreate(&b->ev1), "hipEventCreate");
    ok = ok && hip_ok(hipEventCreateWithFlags(&b->ev_mark, hipEventDisableTiming), "hipEventCreate");
    if (ok) {
        /* every env starts at qpos0 */
        std::vector<double> q0((size_t)nenv * model->nq);
        for (int e = 0; e < nenv; ++e) memcpy(&q0[(size_t)e * model->nq], model->qpos0, sizeof(double) * model->nq);
        ok = hip_ok(hipMemcpy(b->d_field[PHYS_F_QPOS], q0.data(), q0.size() * sizeof(double), hipMemcpyHostToDevice),
                    "hipMemcpy(qpos0)");
    }
    if (!ok) { phys_batch_free(b); return nullptr; }
    return b;
}

void phys_batch_free(phys_batch_t *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    for (auto &e : b->ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->ev_mark) (void)hipEventDestroy(b->ev_mark);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b; /* (the buffers release what the batch owns, never a caller's) */
}

int phys_batch_nenv(const phys_batch_t *b) { return b ? b->nenv : 0; }
int phys_batch_field_dim(const phys_batch_t *b, int field) {
    return (b && field >= 0 && field < PHYS_F_COUNT) ? b->dim[field] : 0;
}

int phys_batch_set_model(phys_batch_t *b, const cm_model_t *model, int env) {
    if (!b || !model) return -1;
    if (model->nq != b->host_model.nq || model->nv != b->host_model.nv || model->nbody != b->host_model.nbody ||
        model->nu != b->host_model.nu || model->nsensordata != b->host_model.nsensordata) {
        phys_set_last_error("phys_batch_set_model: model dimensions differ from the batch's");
        return -1;
    }
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    cm_model_t synced = *model;     /* (the caller's top-level arrays are the authority: cm_model_sync_params) */
    cm_model_sync_params(&synced);
    synced.env_geom = 0; synced.env_springs = 0; /* (a new model drops the blocks; per-env models have none) */
    model = &synced;
    if (env < 0) {
        b->d_envparams.reset(); /* (the new model's own block again, for every env) */
        if (b->model_stride == 1) { /* back to one shared model */
            if (!b->d_models.alloc(1, false, "model")) return -1;
            b->model_stride = 0;
        }
        b->host_model = *model;
        return hip_ok(hipMemcpy(b->d_models, model, sizeof(cm_model_t), hipMemcpyHostToDevice), "hipMemcpy(model)") ? 0 : -1;
    }
    if (env >= b->nenv) return -1;
    if (b->d_envparams) { phys_set_last_error("phys_batch_set_model: per-env models and per-env parameter blocks (phys_batch_randomize) do not mix"); return -1; }
    /* one launch serves every env with the kernel instantiation picked from the shared model: a per-env model may vary
     * parameters, not the dof tree or the kinds of collision pairs */
    if (memcmp(model->dof_ancmask, b->host_model.dof_ancmask, sizeof(model->dof_ancmask[0]) * (size_t)model->nv) != 0 ||
        model->kin_simple != b->host_model.kin_simple || model->maxdepth != b->host_model.maxdepth ||
        (model->nhfpair > 0) != (b->host_model.nhfpair > 0) || (model->hfield_geom >= 0) != (b->host_model.hfield_geom >= 0) ||
        (model->npair > model->npair_simple) != (b->host_model.npair > b->host_model.npair_simple) ||
        /* the tier chain behind a launch (63-row pass only, or 63 + 127) is picked from the SHARED model's caps, the kernel reads the env's */
        model->maxefc != b->host_model.maxefc || model->maxcon != b->host_model.maxcon ||
        ((model->flags ^ b->host_model.flags) & (CM_FLAG_HFPRISM | CM_FLAG_HFMULTI | CM_FLAG_HFDENSE | CM_FLAG_BOX8)) != 0) {
        phys_set_last_error("phys_batch_set_model: a per-env model must keep the shared model's dof tree, collision pair kinds, contact / row caps and height-field contact option");
        return -1;
    }
    if (b->model_stride == 0) { /* expand to one model per env */
        DevBuf<cm_model_t> all;
        if (!all.alloc((size_t)b->nenv, false, "models")) return -1;
        std::vector<cm_model_t> tmp((size_t)b->nenv, b->host_model);
        if (!hip_ok(hipMemcpy(all, tmp.data(), sizeof(cm_model_t) * tmp.size(), hipMemcpyHostToDevice), "hipMemcpy(models)")) return -1;
        b->d_models = std::move(all);
        b->model_stride = 1;
    }
    return hip_ok(hipMemcpy(b->d_models + env, model, sizeof(cm_model_t), hipMemcpyHostToDevice), "hipMemcpy(model)") ? 0 : -1;
}

int phys_batch_set_hfield(phys_batch_t *b, const float *data, int n) {
    if (!b || !data || n <= 0) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    b->nterrain = 0;
    if (b->d_hfield && (b->hfield_stride != 0 || b->hfield_floats != (size_t)n)) b->d_hfield.reset(); /* back to one shared grid */
    if (!b->d_hfield && !b->d_hfield.alloc((size_t)n, false, "hfield")) return -1;
    b->hfield_stride = 0;
    b->hfield_floats = (size_t)n;
    return hip_ok(hipMemcpy(b->d_hfield, data, sizeof(float) * (size_t)n, hipMemcpyHostToDevice), "hipMemcpy(hfield)") ? 0 : -1;
}

int phys_batch_set_hfield_env(phys_batch_t *b, int env, const float *data, int n) {
    if (!b || !data || n <= 0 || env < 0 || env >= b->nenv) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (b->hfield_stride == 0 || b->hfield_floats != (size_t)n || b->nterrain > 0) {
        /* first per-env grid: expand to one grid per env, every env starting from the shared grid (or from zeros: no shared grid, or a
         * bank of terrains was in use) */
        DevBuf<float> all;
        const size_t bytes = sizeof(float) * (size_t)n;
        if (!all.alloc((size_t)n * (size_t)b->nenv, false, "hfield per env")) return -1;
        const bool seed = b->d_hfield && b->hfield_stride == 0 && b->hfield_floats == (size_t)n;
        if (!seed && !hip_ok(hipMemset(all, 0, bytes * (size_t)b->nenv), "hipMemset(hfield)")) return -1;
        for (int e = 0; seed && e < b->nenv; ++e)
            if (!hip_ok(hipMemcpy(all + (size_t)e * n, b->d_hfield, bytes, hipMemcpyDeviceToDevice), "hipMemcpy(hfield)")) return -1;
        b->d_hfield = std::move(all);
        b->nterrain = 0;
        b->hfield_stride = (size_t)n;
        b->hfield_floats = (size_t)n;
    }
    return hip_ok(hipMemcpy(b->d_hfield + (size_t)env * n, data, sizeof(float) * (size_t)n, hipMemcpyHostToDevice), "hipMemcpy(hfield)") ? 0 : -1;
}

int phys_batch_upload(phys_batch_t *b, int field, const double *host, int env0, int n) {
    if (!b || !host || field < 0 || field >= PHYS_F_COUNT || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    note_field_in_use(b, field);
    return copy_rows(b, field, (void *)host, env0, n, true, "upload") && hip_ok(hipStreamSynchronize(b->stream), "upload sync") ? 0 : -1;
}

int phys_batch_download(phys_batch_t *b, int field, double *host, int env0, int n) {
    if (!b || !host || field < 0 || field >= PHYS_F_COUNT || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    /* (launches on callers' streams -- step_range, reset_envs -- may still be writing the field) */
    return quiesce(b) && copy_rows(b, field, host, env0, n, false, "download") && hip_ok(hipStreamSynchronize(b->stream), "download sync") ? 0 : -1;
}

int phys_batch_upload_async(phys_batch_t *b, int field, const double *host, int env0, int n) {
    if (!b || !host || field < 0 || field >= PHYS_F_COUNT || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    note_field_in_use(b, field);
    return copy_rows(b, field, (void *)host, env0, n, true, "upload_async") ? 0 : -1;
}

int phys_batch_download_async(phys_batch_t *b, int field, double *host, int env0, int n) {
    if (!b || !host || field < 0 || field >= PHYS_F_COUNT || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    return copy_rows(b, field, host, env0, n, false, "download_async") ? 0 : -1;
}

void *phys_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    memset(p, 0, bytes);
    return p;
}
void phys_host_free(void *p) { if (p) (void)hipHostFree(p); }

int phys_batch_download_warn(phys_batch_t *b, int *host_warn, int *host_info) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    bool ok = quiesce(b);
    if (host_warn) ok = ok && hip_ok(hipMemcpy(host_warn, b->d_warn, sizeof(int) * b->nenv, hipMemcpyDeviceToHost), "warn");
    if (host_info) ok = ok && hip_ok(hipMemcpy(host_info, b->d_info, sizeof(int) * 4 * b->nenv, hipMemcpyDeviceToHost), "info");
    return ok ? 0 : -1;
}

int phys_batch_uses_applied(const phys_batch_t *b) { return (b && b->use_applied) ? 1 : 0; }

int phys_batch_clear_warn(phys_batch_t *b, int env0, int n) {
    if (!b || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    return hip_ok(hipMemsetAsync(b->d_warn + env0, 0, sizeof(int) * (size_t)n, b->stream), "hipMemset(warn)") &&
                   hip_ok(hipStreamSynchronize(b->stream), "warn sync") ? 0 : -1;
}

void *phys_batch_device_ptr(phys_batch_t *b, int field) {
    return (b && field >= 0 && field < PHYS_F_COUNT) ? (void *)b->d_field[field] : nullptr;
}

int phys_batch_bind(phys_batch_t *b, int field, void *device_ptr) {
    return phys_batch_bind_strided(b, field, device_ptr, (b && field >= 0 && field < PHYS_F_COUNT) ? b->dim[field] : 0);
}

int phys_batch_bind_strided(phys_batch_t *b, int field, void *device_ptr, int row_stride) {
    if (!b || !device_ptr || field < 0 || field >= PHYS_F_COUNT) return -1;
    if (row_stride != b->dim[field]) {
        const bool may = field == PHYS_F_QPOS || field == PHYS_F_QVEL || field == PHYS_F_SENSORDATA || field == PHYS_F_HEIGHT_SCAN || field == PHYS_F_DEPTH || field == PHYS_F_RAYS || field == PHYS_F_PROBES;
        if (!may || row_stride < b->dim[field]) {
            phys_set_last_error("phys_batch_bind_strided: only qpos / qvel / sensordata / the height scan / the depth image / the ray ranges / the probes' rows take a row stride, and it must be >= the field's dim");
            return -1;
        }
    }
    if (field == PHYS_F_HEIGHT_SCAN && b->scan.npoints <= 0) { phys_set_last_error("phys_batch_bind: configure the scan first (phys_batch_scan_configure sizes PHYS_F_HEIGHT_SCAN)"); return -1; }
    if (field == PHYS_F_DEPTH && b->depth.width <= 0) { phys_set_last_error("phys_batch_bind: configure the depth image first (phys_batch_depth_configure sizes PHYS_F_DEPTH)"); return -1; }
    if (field == PHYS_F_RAYS && b->rays.nrays <= 0) { phys_set_last_error("phys_batch_bind: configure the rays first (phys_batch_rays_configure sizes PHYS_F_RAYS)"); return -1; }
    if (field == PHYS_F_PROBES && b->probes.nprobes <= 0) { phys_set_last_error("phys_batch_bind: configure the probes first (phys_batch_probes_configure sizes PHYS_F_PROBES)"); return -1; }
    (void)hipSetDevice(b->device);
    /* no stream synchronisation: launches already queued keep the pointers they were given, and hipFree of the
     * replaced buffer waits for the device by itself */
    b->d_field[field].borrow((double *)device_ptr);
    b->stride[field] = row_stride;
    note_field_in_use(b, field);
    return 0;
}

int phys_batch_step(phys_batch_t *b, int nsub, void *stream) {
    if (!b || nsub <= 0) return -1;
    (void)hipSetDevice(b->device);
    return launch(b, nsub, 1, launch_stream(b, stream));
}

int phys_batch_step_range(phys_batch_t *b, int env0, int n, int nsub, void *stream) {
    if (!b || nsub <= 0 || n <= 0 || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    return launch(b, nsub, 1, launch_stream(b, stream), false, env0, n);
}

int phys_batch_forward(phys_batch_t *b, void *stream) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    return launch(b, 1, 0, launch_stream(b, stream));
}

int phys_batch_forward_kinematics(phys_batch_t *b, void *stream) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    if (b->drive_mode != CM_DRIVE_OFF) { phys_set_last_error("phys_batch_forward_kinematics: not in a drive mode (the pass reads the sensordata field)"); return -1; }
    if (!b->d_scratch_out) {
        const cm_model_t &m = b->host_model;
        if (!b->d_scratch_out.alloc((size_t)b->nenv * (size_t)(m.nv + m.nsensordata + m.nu), false, "scratch outputs")) return -1;
    }
    return launch(b, 1, 0, launch_stream(b, stream), true);
}

int phys_batch_set_pd_mode(phys_batch_t *b, int on) {
    if (!b) return -1;
    b->pd_mode = on != 0;
    return 0;
}

static bool ensure_drive_state(phys_batch *b) {
    if (b->d_drive) return true;
    if (b->host_model.nu != CM_NUM_DRIVES || b->host_model.nsensordata < 29) {
        phys_set_last_error("the drive-level models need Cassie's 10 drives and 29 sensor words");
        return false;
    }
    if (!quiesce(b)) return false;
    const size_t bytes = sizeof(cm_drive_state_t) * (size_t)b->nenv;
    if (!b->d_drive.alloc((size_t)b->nenv, false, "drive state")) return false;
    return hip_ok(hipMemsetAsync(b->d_drive, 0, bytes, b->stream), "hipMemset(drive state)") && hip_ok(hipStreamSynchronize(b->stream), "sync");
}

int phys_batch_set_drive_mode(phys_batch_t *b, int mode) {
    if (!b || mode < CM_DRIVE_OFF || mode > CM_DRIVE_PD_SAFE) return -1;
    (void)hipSetDevice(b->device);
    if (mode != CM_DRIVE_OFF && !ensure_drive_state(b)) return -1;
    b->drive_mode = mode;
    return 0;
}

int phys_batch_drive_pass(phys_batch_t *b, int mode, void *stream) {
    if (!b || (mode != CM_DRIVE_TORQUE && mode != CM_DRIVE_PD && mode != CM_DRIVE_PD_SAFE)) return -1;
    (void)hipSetDevice(b->device);
    if (!ensure_drive_state(b)) return -1;
    const int keep = b->drive_mode;
    b->drive_mode = mode;
    ck::PhysIO io = make_io(b, 1, 1);
    b->drive_mode = keep;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_drive_kernel, dim3(b->nenv), dim3(WV_WAVE), 0, s, io, b->d_field[PHYS_F_CTRL].get());
    return hip_ok(hipGetLastError(), "cassie_drive_kernel launch") ? 0 : -1;
}

int phys_batch_mark(phys_batch_t *b) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    return hip_ok(hipEventRecord(b->ev_mark, b->stream), "hipEventRecord") ? 0 : -1;
}
int phys_batch_wait_mark(phys_batch_t *b) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    return hip_ok(hipEventSynchronize(b->ev_mark), "hipEventSynchronize") ? 0 : -1;
}

int phys_batch_clear_drive_state(phys_batch_t *b, int first, int stride, int count, void *stream) {
    if (!b || !strided_ok(b, first, stride, count)) return -1;
    (void)hipSetDevice(b->device);
    if (!ensure_drive_state(b)) return -1;
    if (count == 0) return 0;
    return hip_ok(hipMemset2DAsync(b->d_drive + first, sizeof(cm_drive_state_t) * (size_t)stride, 0, sizeof(cm_drive_state_t), (size_t)count,
                                   launch_stream(b, stream)), "hipMemset2D(drive state)") ? 0 : -1;
}

int phys_batch_upload_drive_state(phys_batch_t *b, const cm_drive_state_t *host, int env0, int n) {
    if (!b || !host || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    if (!ensure_drive_state(b)) return -1;
    return hip_ok(hipMemcpyAsync(b->d_drive + env0, host, sizeof(cm_drive_state_t) * (size_t)n, hipMemcpyHostToDevice, b->stream), "drive state upload") &&
                   hip_ok(hipStreamSynchronize(b->stream), "drive state sync") ? 0 : -1;
}

int phys_batch_download_drive_state(phys_batch_t *b, cm_drive_state_t *host, int env0, int n) {
    if (!b || !host || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    if (!ensure_drive_state(b)) return -1;
    return hip_ok(hipMemcpyAsync(host, b->d_drive + env0, sizeof(cm_drive_state_t) * (size_t)n, hipMemcpyDeviceToHost, b->stream), "drive state download") &&
                   hip_ok(hipStreamSynchronize(b->stream), "drive state sync") ? 0 : -1;
}

int phys_batch_reset_envs(phys_batch_t *b, int first, int stride, int count, const double *qpos_row, const double *sens_row, void *stream) {
    if (!b || !qpos_row || !strided_ok(b, first, stride, count)) return -1;
    (void)hipSetDevice(b->device);
    if (count == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_reset_kernel, dim3(ck::reset_grid(count)), dim3(WV_WAVE), 0, s, ck::make_reset_io(view_of(b), first, stride, count, qpos_row, sens_row));
    return hip_ok(hipGetLastError(), "cassie_reset_kernel launch") ? 0 : -1;
}

/* ------------------------------------------------ episodes on the device ---- */
static size_t episode_array_bytes(const phys_batch *b, int which) {
    return which == PHYS_EP_TERMINAL ? sizeof(double) * (size_t)b->nenv * (size_t)(b->host_model.nq + b->host_model.nv) : sizeof(int) * (size_t)b->nenv;
}
int phys_batch_episodes_enable(phys_batch_t *b, const cm_episode_rules_t *rules) {
    if (!b || !rules) { phys_set_last_error("phys_batch_episodes_enable: bad arguments"); return -1; }
    (void)hipSetDevice(b->device);
    if (!b->episodes) {
        for (int a = 0; a < PHYS_EP_ARRAYS; ++a) {
            if (b->d_ep[a]) continue;
            if (!b->d_ep[a].alloc(episode_array_bytes(b, a), true, "episode array")) return -1;
        }
        if (!hip_ok(hipDeviceSynchronize(), "episode arrays sync")) return -1;
        b->episodes = true;
    }
    b->ep.rules = *rules; /* (passed to every launch by value: launches already queued keep the rules they were given) */
    return 0;
}
int phys_batch_episode_row_dim(const phys_batch_t *b) {
    if (!b) return 0;
    const cm_model_t &m = b->host_model;
    return m.nq + m.nv + m.nsensordata + m.nu + m.nv;
}
int phys_batch_episodes_set_bank(phys_batch_t *b, const double *rows, int on_device, int nrows) {
    if (!b || !rows || nrows <= 0) { phys_set_last_error("phys_batch_episodes_set_bank: bad arguments"); return -1; }
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1; /* (launches in flight may be reading the bank that goes away) */
    b->d_ep_bank.reset(); b->ep.nrows = 0;
    if (on_device) b->d_ep_bank.borrow(rows);
    else {
        const size_t count = (size_t)nrows * (size_t)phys_batch_episode_row_dim(b);
        DevBuf<const double> d;
        if (!d.alloc(count, false, "reset bank")) return -1;
        if (!hip_ok(hipMemcpy((void *)d.get(), rows, sizeof(double) * count, hipMemcpyHostToDevice), "hipMemcpy(reset bank)")) return -1;
        b->d_ep_bank = std::move(d);
    }
    b->ep.nrows = nrows;
    return 0;
}
void *phys_batch_episode_ptr(phys_batch_t *b, int which) {
    return (b && which >= 0 && which < PHYS_EP_ARRAYS) ? (void *)b->d_ep[which].get() : nullptr;
}
int phys_batch_episode_bind(phys_batch_t *b, int which, void *device_ptr) {
    if (!b || !device_ptr || which < 0 || which >= PHYS_EP_ARRAYS) { phys_set_last_error("phys_batch_episode_bind: bad arguments"); return -1; }
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    b->d_ep[which].borrow((char *)device_ptr);
    return 0;
}
static bool ensure_place_arrays(phys_batch *b);
int phys_batch_end_episodes(phys_batch_t *b, int env0, int n, int restart, const int *pick, const int *force, void *stream) {
    if (!b) return -1;
    if (!b->episodes) { phys_set_last_error("phys_batch_end_episodes: call phys_batch_episodes_enable first"); return -1; }
    if (!range_ok(b, env0, n)) { phys_set_last_error("phys_batch_end_episodes: env range out of bounds"); return -1; }
    if (restart && (!b->d_ep_bank || b->ep.nrows <= 0)) { phys_set_last_error("phys_batch_end_episodes: restart needs a bank of start states (phys_batch_episodes_set_bank)"); return -1; }
    for (int a = 0; a < PHYS_EP_ARRAYS; ++a) if (!b->d_ep[a]) { phys_set_last_error("phys_batch_end_episodes: an episode array is missing"); return -1; }
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    const bool placed = restart && b->place.anchor > 0;
    if (placed) {
        if (b->model_stride != 0) { phys_set_last_error("phys_batch_end_episodes: placed restarts and per-env models (phys_batch_set_model with env >= 0) do not mix"); return -1; }
        if (!ensure_place_arrays(b)) return -1;
    }
    ck::EpisodeCfg e = b->ep;
    ck::PlaceCfg place = b->place;
    place.table = b->d_place_table; place.offsets = b->d_place_offsets; place.pose = b->d_place_pose; place.ground = b->d_place_ground;
    e.bank = b->d_ep_bank;
    e.done = (int *)b->d_ep[PHYS_EP_DONE].get(); e.reason = (int *)b->d_ep[PHYS_EP_REASON].get(); e.steps = (int *)b->d_ep[PHYS_EP_STEPS].get();
    e.count = (int *)b->d_ep[PHYS_EP_COUNT].get(); e.terminal = (double *)b->d_ep[PHYS_EP_TERMINAL].get();
    const ck::EpisodeIO io = ck::make_episode_io(view_of(b), e, placed ? &place : nullptr, env0, n, restart, pick, force);
    hipStream_t s = launch_stream(b, stream);
    const dim3 grid((unsigned)ck::episode_grid(n));   /* (one launch either way, on the same few workgroups) */
    if (placed) hipLaunchKernelGGL(ck::cassie_episode_place_kernel, grid, dim3(WV_WAVE), 0, s, io);
    else hipLaunchKernelGGL(ck::cassie_episode_kernel, grid, dim3(WV_WAVE), 0, s, io);
    return hip_ok(hipGetLastError(), placed ? "cassie_episode_place_kernel launch" : "cassie_episode_kernel launch") ? 0 : -1;
}
int phys_batch_download_episodes(phys_batch_t *b, int which, void *host) {
    if (!b || !host || which < 0 || which >= PHYS_EP_ARRAYS || !b->d_ep[which]) { phys_set_last_error("phys_batch_download_episodes: bad arguments, or episodes not enabled"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_ep[which], episode_array_bytes(b, which), hipMemcpyDeviceToHost), "episode array download") ? 0 : -1;
}
size_t phys_sizeof_episode_rules(void) { return sizeof(cm_episode_rules_t); }

/* ------------------------------------------------ a bank of full states: save, rewind and fork envs on the device ---- */
static_assert((int)PHYS_SS_COUNT == (int)ck::SS_COUNT && (int)PHYS_SS_PARAMS == (int)ck::SS_PARAMS && (int)PHYS_STATE_PARAMS == (int)ck::STATE_PARAMS, "the header's sections and groups are small_launch.h's");
static ck::StateLayout state_layout_of(const phys_batch *b) { return ck::state_layout(view_of(b), b->state.groups); }
int phys_batch_state_configure(phys_batch_t *b, int nslots, int groups) {
    if (!b) { phys_set_last_error("phys_batch_state_configure: no batch"); return -1; }
    if (const char *why = ck::state_configure(view_of(b), nslots, groups)) return refuse("phys_batch_state_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1; /* (launches in flight may be using the bank that goes away) */
    const ck::StateLayout L = ck::state_layout(view_of(b), groups);
    b->state = {}; b->state_bound = nullptr; b->state_own_slots = 0;
    if (!b->d_state.alloc((size_t)nslots * (size_t)L.row_dim, true, "state bank")) return -1;
    b->state.nslots = b->state_own_slots = nslots; b->state.groups = L.groups;
    return 0;
}
int phys_batch_state_bind(phys_batch_t *b, void *device_ptr, int nslots) {
    if (!b) { phys_set_last_error("phys_batch_state_bind: no batch"); return -1; }
    if (b->state_own_slots < 1) return refuse("phys_batch_state_bind", "configure first (phys_batch_state_configure fixes the groups, and with them the row)");
    if (device_ptr && nslots < 1) return refuse("phys_batch_state_bind", "a bank of at least one slot");
    if (((size_t)device_ptr & 15u) != 0) return refuse("phys_batch_state_bind", "the rows must start on a 16-byte boundary");
    /* (as phys_batch_bind: launches already queued keep the pointer they were given) */
    b->state_bound = (unsigned long long *)device_ptr;
    b->state.nslots = device_ptr ? nslots : b->state_own_slots;
    return 0;
}
void *phys_batch_state_ptr(phys_batch_t *b) { return !b || b->state.nslots < 1 ? nullptr : b->state_bound ? (void *)b->state_bound : (void *)b->d_state.get(); }
int phys_batch_state_nslots(const phys_batch_t *b) { return b ? b->state.nslots : 0; }
int phys_batch_state_groups(const phys_batch_t *b) { return b ? b->state.groups : 0; }
int phys_batch_state_row_dim(const phys_batch_t *b) { return b && b->state.nslots > 0 ? state_layout_of(b).row_dim : 0; }
int phys_batch_state_layout_version(void) { return ck::STATE_LAYOUT_VERSION; }
int phys_batch_state_layout(const phys_batch_t *b, int *offsets_counts) {
    if (!b || b->state.nslots < 1) { phys_set_last_error("phys_batch_state_layout: not configured (phys_batch_state_configure first)"); return -1; }
    const ck::StateLayout L = state_layout_of(b);
    for (int s = 0; offsets_counts && s < ck::SS_COUNT; ++s) { offsets_counts[2 * s] = L.off[s]; offsets_counts[2 * s + 1] = L.count[s]; }
    return ck::SS_COUNT;
}
unsigned long long phys_batch_state_signature(const phys_batch_t *b) {
    return b && b->state.nslots > 0 ? ck::state_signature(b->host_model, state_layout_of(b)) : 0ull;
}
static int state_launch(phys_batch *b, const char *entry, bool restore, int env0, int n, const int *slots, void *stream) {
    if (!b) { phys_set_last_error((std::string(entry) + ": no batch").c_str()); return -1; }
    ck::StateCfg c = b->state;
    c.bank = (unsigned long long *)phys_batch_state_ptr(b);
    if (const char *why = ck::check_state_call(c, b->nenv, env0, n)) return refuse(entry, why);
    const ck::BatchView v = view_of(b);
    /* (what the groups need may have gone since: a new shared model drops the parameter blocks) */
    if (const char *why = ck::state_configure(v, c.nslots, c.groups)) return refuse(entry, why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    const ck::StateIO io = ck::make_state_io(v, c, env0, n, slots);
    hipStream_t s = launch_stream(b, stream);
    const dim3 grid((unsigned)ck::state_grid(n));
    if (restore) hipLaunchKernelGGL(ck::cassie_state_restore_kernel, grid, dim3(WV_WAVE), 0, s, io);
    else hipLaunchKernelGGL(ck::cassie_state_save_kernel, grid, dim3(WV_WAVE), 0, s, io);
    return hip_ok(hipGetLastError(), restore ? "cassie_state_restore_kernel launch" : "cassie_state_save_kernel launch") ? 0 : -1;
}
int phys_batch_state_save(phys_batch_t *b, int env0, int n, const int *slots, void *stream) {
    return state_launch(b, "phys_batch_state_save", false, env0, n, slots, stream);
}
int phys_batch_state_restore(phys_batch_t *b, int env0, int n, const int *slots, void *stream) {
    return state_launch(b, "phys_batch_state_restore", true, env0, n, slots, stream);
}
void *phys_batch_state_stage_slots(phys_batch_t *b, const int *host_slots, int n) {
    if (!b || !host_slots || n < 1) { phys_set_last_error("phys_batch_state_stage_slots: bad arguments"); return nullptr; }
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return nullptr; /* (a launch in flight may still be reading the slots staged before) */
    if (b->state_staged_cap < n) {
        b->state_staged_cap = 0;
        if (!b->d_state_staged.alloc((size_t)n, false, "staged slots")) return nullptr;
        b->state_staged_cap = n;
    }
    return hip_ok(hipMemcpy(b->d_state_staged, host_slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice), "hipMemcpy(staged slots)") ? (void *)b->d_state_staged.get() : nullptr;
}
static bool state_slots_ok(const phys_batch *b, int slot0, int n) {
    return b && b->state.nslots > 0 && slot0 >= 0 && n >= 0 && (long long)slot0 + n <= b->state.nslots;
}
int phys_batch_state_download(phys_batch_t *b, int slot0, int n, void *host) {
    if (!host || !state_slots_ok(b, slot0, n)) { phys_set_last_error("phys_batch_state_download: not configured, or slots outside the bank"); return -1; }
    (void)hipSetDevice(b->device);
    const size_t row = sizeof(unsigned long long) * (size_t)state_layout_of(b).row_dim;
    return quiesce(b) && (n == 0 || hip_ok(hipMemcpy(host, (char *)phys_batch_state_ptr(b) + row * (size_t)slot0, row * (size_t)n, hipMemcpyDeviceToHost), "state download")) ? 0 : -1;
}
int phys_batch_state_upload(phys_batch_t *b, int slot0, int n, const void *host, unsigned long long signature) {
    if (!host || !state_slots_ok(b, slot0, n)) { phys_set_last_error("phys_batch_state_upload: not configured, or slots outside the bank"); return -1; }
    if (signature != phys_batch_state_signature(b))
        return refuse("phys_batch_state_upload", "the rows' signature is not this batch's (phys_batch_state_signature): they were saved from another model, with other groups or by another layout version");
    (void)hipSetDevice(b->device);
    const size_t row = sizeof(unsigned long long) * (size_t)state_layout_of(b).row_dim;
    return quiesce(b) && (n == 0 || hip_ok(hipMemcpy((char *)phys_batch_state_ptr(b) + row * (size_t)slot0, host, row * (size_t)n, hipMemcpyHostToDevice), "state upload")) ? 0 : -1;
}

/* ------------------------------------------------ terrains: a bank shared by the envs, a per-env index ---- */
static bool ensure_terrain_index(phys_batch *b) {
    if (b->d_terrain_index) return true;
    return b->d_terrain_index.alloc((size_t)b->nenv, true, "terrain index");
}
int phys_batch_set_hfield_bank(phys_batch_t *b, const float *grids, int on_device, int nterrain, int n) {
    if (!b || !grids || nterrain <= 0 || n <= 0) { phys_set_last_error("phys_batch_set_hfield_bank: bad arguments"); return -1; }
    if (b->host_model.hfield_geom < 0 || n != b->host_model.hfield_nrow * b->host_model.hfield_ncol) {
        phys_set_last_error("phys_batch_set_hfield_bank: a grid must hold the model's hfield_nrow * hfield_ncol samples");
        return -1;
    }
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    const size_t count = (size_t)n * (size_t)nterrain;
    DevBuf<float> all;
    if (!all.alloc(count, false, "terrain bank")) return -1;
    if (!hip_ok(hipMemcpy(all, grids, sizeof(float) * count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice), "hipMemcpy(terrain bank)")) return -1;
    if (!ensure_terrain_index(b)) return -1;
    /* every env starts on terrain 0 (an index array of the caller's keeps what the caller put there) */
    if (b->d_terrain_index.owned() && !hip_ok(hipMemset(b->d_terrain_index, 0, sizeof(int) * (size_t)b->nenv), "hipMemset(terrain index)")) return -1;
    b->d_hfield = std::move(all);
    b->hfield_stride = (size_t)n; b->hfield_floats = (size_t)n;
    b->nterrain = nterrain;
    return 0;
}
int phys_batch_nterrain(const phys_batch_t *b) { return b ? b->nterrain : 0; }
void *phys_batch_terrain_index_ptr(phys_batch_t *b) {
    if (!b) return nullptr;
    (void)hipSetDevice(b->device);
    return ensure_terrain_index(b) ? (void *)b->d_terrain_index.get() : nullptr;
}
int phys_batch_bind_terrain_index(phys_batch_t *b, void *device_ptr) {
    if (!b || !device_ptr) { phys_set_last_error("phys_batch_bind_terrain_index: bad arguments"); return -1; }
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    b->d_terrain_index.borrow((int *)device_ptr);
    return 0;
}
int phys_batch_set_terrain(phys_batch_t *b, const int *ids, int on_device, int env0, int n, void *stream) {
    if (!b || !ids || !range_ok(b, env0, n)) { phys_set_last_error("phys_batch_set_terrain: bad arguments"); return -1; }
    if (b->nterrain <= 0) { phys_set_last_error("phys_batch_set_terrain: no bank of terrains (phys_batch_set_hfield_bank)"); return -1; }
    if (!on_device)
        for (int i = 0; i < n; ++i)
            if (ids[i] < 0 || ids[i] >= b->nterrain) { phys_set_last_error("phys_batch_set_terrain: a terrain id outside the bank"); return -1; }
    (void)hipSetDevice(b->device);
    if (!ensure_terrain_index(b)) return -1;
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    if (!hip_ok(hipMemcpyAsync(b->d_terrain_index + env0, ids, sizeof(int) * (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s), "hipMemcpy(terrain ids)")) return -1;
    /* (host ids: the caller's array may go away once the call returns) */
    return on_device || hip_ok(hipStreamSynchronize(s), "terrain ids sync") ? 0 : -1;
}

/* ------------------------------------------------ the height scan ---- */
int phys_batch_scan_configure(phys_batch_t *b, const double *offsets_xy, int npoints, int body, double range) {
    if (!b) return refuse("phys_batch_scan_configure", ck::SCAN_SIZE_REFUSAL);
    ck::ScanCfg cfg;
    if (const char *why = ck::scan_configure(b->host_model, b->model_stride, offsets_xy, npoints, body, range, cfg)) return refuse("phys_batch_scan_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    DevBuf<double> off, out;
    if (!off.alloc(2 * (size_t)npoints, false, "scan pattern")) return -1;
    if (!hip_ok(hipMemcpy(off, offsets_xy, sizeof(double) * 2 * (size_t)npoints, hipMemcpyHostToDevice), "hipMemcpy(scan pattern)")) return -1;
    /* the field takes the pattern's size: a buffer of the batch's own of the new size (a caller's binding is dropped: bind again) */
    if (!out.alloc((size_t)npoints * (size_t)b->nenv, true, "height scan")) return -1;
    b->d_scan_offsets = std::move(off);
    b->d_field[PHYS_F_HEIGHT_SCAN] = std::move(out);
    b->dim[PHYS_F_HEIGHT_SCAN] = npoints; b->stride[PHYS_F_HEIGHT_SCAN] = npoints;
    b->scan = cfg;
    return 0;
}
int phys_batch_height_scan(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b) return -1;
    if (b->scan.npoints <= 0 || !b->d_field[PHYS_F_HEIGHT_SCAN]) { phys_set_last_error("phys_batch_height_scan: call phys_batch_scan_configure first"); return -1; }
    if (!range_ok(b, env0, n)) { phys_set_last_error("phys_batch_height_scan: env range out of bounds"); return -1; }
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    ck::ScanCfg scan = b->scan;
    scan.offsets = b->d_scan_offsets;
    hipLaunchKernelGGL(ck::cassie_scan_kernel, dim3((unsigned)ck::scan_grid(n)), dim3(WV_WAVE), 0, s,
                       ck::make_scan_io(view_of(b), scan, b->d_field[PHYS_F_HEIGHT_SCAN], b->stride[PHYS_F_HEIGHT_SCAN], env0, n));
    return hip_ok(hipGetLastError(), "cassie_scan_kernel launch") ? 0 : -1;
}

/* ------------------------------------------------ placed restarts ---- */
/* the batch's own pose (zeros) and ground arrays, unless the caller's are bound */
static bool ensure_place_arrays(phys_batch *b) {
    if (!b->d_place_pose && !b->d_place_pose.alloc(4 * (size_t)b->nenv, true, "placement poses")) return false;
    if (!b->d_place_ground && !b->d_place_ground.alloc((size_t)b->nenv, true, "placement ground")) return false;
    return true;
}
int phys_batch_place_configure(phys_batch_t *b, int anchor, const double *offsets_xy, int npoints, double ground_ref) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    if (anchor <= 0) {           /* off again: restarts copy the row verbatim */
        if (!quiesce(b)) return -1;
        b->place.anchor = 0;
        return 0;
    }
    ck::PlaceTable tab;
    if (const char *why = ck::place_configure(b->host_model, b->model_stride, anchor, offsets_xy, npoints, ground_ref, tab)) return refuse("phys_batch_place_configure", why);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the footprint that goes away) */
    DevBuf<double> off;
    DevBuf<ck::PlaceTable> dtab;
    if (!dtab.alloc(1, false, "placement table")) return -1;
    if (!hip_ok(hipMemcpy(dtab, &tab, sizeof tab, hipMemcpyHostToDevice), "hipMemcpy(placement table)")) return -1;
    if (npoints > 0) {
        if (!off.alloc(2 * (size_t)npoints, false, "placement footprint")) return -1;
        if (!hip_ok(hipMemcpy(off, offsets_xy, sizeof(double) * 2 * (size_t)npoints, hipMemcpyHostToDevice), "hipMemcpy(placement footprint)")) return -1;
    }
    if (!ensure_place_arrays(b)) return -1;
    b->d_place_offsets = std::move(off);
    b->d_place_table = std::move(dtab);
    b->place.anchor = anchor; b->place.npoints = npoints; b->place.ground_ref = ground_ref;
    return 0;
}
void *phys_batch_place_ptr(phys_batch_t *b, int which) {
    if (!b || which < 0 || which >= PHYS_PLACE_ARRAYS) return nullptr;
    (void)hipSetDevice(b->device);
    if (which == PHYS_PLACE_NEXT_TERRAIN) return (void *)b->place.next;   /* (null unless bound: the batch keeps none of its own) */
    if (!ensure_place_arrays(b)) return nullptr;
    return which == PHYS_PLACE_POSE ? (void *)b->d_place_pose.get() : (void *)b->d_place_ground.get();
}
int phys_batch_place_bind(phys_batch_t *b, int which, void *device_ptr) {
    if (!b || which < 0 || which >= PHYS_PLACE_ARRAYS) { phys_set_last_error("phys_batch_place_bind: bad arguments"); return -1; }
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself.  NULL:
     * the batch's own array again -- zeros -- or, for the next terrains, none) */
    if (which == PHYS_PLACE_NEXT_TERRAIN) b->place.next = (const int *)device_ptr;
    else {
        DevBuf<double> &d = which == PHYS_PLACE_POSE ? b->d_place_pose : b->d_place_ground;
        d.borrow((double *)device_ptr);
        if (!device_ptr && !ensure_place_arrays(b)) return -1;
    }
    return 0;
}

static size_t place_row_bytes(int which) { return which == PHYS_PLACE_POSE ? 4 * sizeof(double) : which == PHYS_PLACE_GROUND ? sizeof(double) : sizeof(int); }
int phys_batch_place_upload(phys_batch_t *b, int which, const void *host, int env0, int n) {
    if (!b || !host || which < 0 || which >= PHYS_PLACE_ARRAYS || !range_ok(b, env0, n)) { phys_set_last_error("phys_batch_place_upload: bad arguments"); return -1; }
    char *dst = (char *)phys_batch_place_ptr(b, which);
    if (!dst) { phys_set_last_error("phys_batch_place_upload: no such array (bind the next terrains first)"); return -1; }
    const size_t row = place_row_bytes(which);
    return quiesce(b) && hip_ok(hipMemcpy(dst + row * (size_t)env0, host, row * (size_t)n, hipMemcpyHostToDevice), "placement array upload") ? 0 : -1;
}
int phys_batch_place_download(phys_batch_t *b, int which, void *host) {
    if (!b || !host || which < 0 || which >= PHYS_PLACE_ARRAYS) { phys_set_last_error("phys_batch_place_download: bad arguments"); return -1; }
    const char *src = (const char *)phys_batch_place_ptr(b, which);
    if (!src) { phys_set_last_error("phys_batch_place_download: no such array (bind the next terrains first)"); return -1; }
    return quiesce(b) && hip_ok(hipMemcpy(host, src, place_row_bytes(which) * (size_t)b->nenv, hipMemcpyDeviceToHost), "placement array download") ? 0 : -1;
}

/* ------------------------------------------------ the depth image ---- */
int phys_batch_depth_configure(phys_batch_t *b, int body, const double *cam_pos, const double *cam_quat, int width, int height, double fovy,
                               double znear, double zfar) {
    if (!b) return refuse("phys_batch_depth_configure", ck::DEPTH_SIZE_REFUSAL);
    ck::DepthCfg cfg;
    if (const char *why = ck::depth_configure(b->host_model, b->model_stride, body, cam_pos, cam_quat, width, height, fovy, znear, zfar, cfg)) return refuse("phys_batch_depth_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    /* the field takes the image's size: a buffer of the batch's own of the new size (a caller's binding is dropped: bind again) */
    DevBuf<double> out;
    if (!out.alloc((size_t)width * (size_t)height * (size_t)b->nenv, true, "depth image")) return -1;
    b->d_field[PHYS_F_DEPTH] = std::move(out);
    b->dim[PHYS_F_DEPTH] = width * height; b->stride[PHYS_F_DEPTH] = width * height;
    cfg.pose = b->depth.pose;           /* (the default geoms again, and no ids -- the image may have another size: bind them again) */
    b->depth = cfg;
    return 0;
}
unsigned phys_batch_depth_default_geoms(const phys_batch_t *b) { return b ? ck::depth_default_geoms(b->host_model) : 0u; }
unsigned phys_batch_depth_all_geoms(const phys_batch_t *b) { return b ? ck::depth_all_geoms(b->host_model) : 0u; }
int phys_batch_depth_set_geoms(phys_batch_t *b, unsigned mask) {
    if (!b) return -1;
    if (b->depth.width <= 0) { phys_set_last_error("phys_batch_depth_set_geoms: call phys_batch_depth_configure first (it restores the default set)"); return -1; }
    if (const char *why = ck::check_depth_geoms(b->host_model, mask)) return refuse("phys_batch_depth_set_geoms", why);
    /* (as phys_batch_bind: launches already queued keep the mask they were given) */
    b->depth.geoms = mask;
    return 0;
}
int phys_batch_depth_bind_ids(phys_batch_t *b, void *device_ptr) {
    if (!b) return -1;
    if (b->depth.width <= 0) { phys_set_last_error("phys_batch_depth_bind_ids: call phys_batch_depth_configure first (it sizes the image)"); return -1; }
    b->depth.ids = (int *)device_ptr;
    return 0;
}
int phys_batch_debug_depth_launches(const phys_batch_t *b, long long *static_kernel, long long *scene_kernel) {
    if (!b) return -1;
    if (static_kernel) *static_kernel = b->depth_launches[0];
    if (scene_kernel) *scene_kernel = b->depth_launches[1];
    return 0;
}
int phys_batch_depth_bind_pose(phys_batch_t *b, const void *device_ptr) {
    if (!b) return -1;
    b->depth.pose = (const double *)device_ptr;   /* (as phys_batch_bind: launches already queued keep the pointer they were given) */
    return 0;
}
int phys_batch_depth_image(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b) return -1;
    if (b->depth.width <= 0 || !b->d_field[PHYS_F_DEPTH]) { phys_set_last_error("phys_batch_depth_image: call phys_batch_depth_configure first"); return -1; }
    if (!range_ok(b, env0, n)) { phys_set_last_error("phys_batch_depth_image: env range out of bounds"); return -1; }
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    const bool scene = ck::depth_scene_kernel(b->host_model, b->depth);
    const ck::DepthIO io = ck::make_depth_io(view_of(b), b->depth, b->d_field[PHYS_F_DEPTH], b->stride[PHYS_F_DEPTH], env0, n, scene);
    const dim3 grid((unsigned)ck::depth_grid(n, b->depth.width, b->depth.height));
    ++b->depth_launches[scene ? 1 : 0];
    if (scene) hipLaunchKernelGGL(ck::cassie_depth_scene_kernel, grid, dim3(WV_WAVE), 0, s, io);
    else hipLaunchKernelGGL(ck::cassie_depth_kernel, grid, dim3(WV_WAVE), 0, s, io);
    return hip_ok(hipGetLastError(), scene ? "cassie_depth_scene_kernel launch" : "cassie_depth_kernel launch") ? 0 : -1;
}

/* ------------------------------------------------ range sensors ---- */
static_assert(sizeof(ck::RayDef) == sizeof(phys_ray_t) && offsetof(ck::RayDef, origin) == offsetof(phys_ray_t, origin) &&
              offsetof(ck::RayDef, dir) == offsetof(phys_ray_t, dir) && offsetof(ck::RayDef, frame) == offsetof(phys_ray_t, frame), "phys_ray_t is the kernel's table entry");
static_assert(PHYS_RAY_BODY == ck::RAY_BODY && PHYS_RAY_WORLD_DIR == ck::RAY_WORLD_DIR && PHYS_RAY_HEADING == ck::RAY_HEADING, "the frames' numbers");
int phys_batch_rays_configure(phys_batch_t *b, const phys_ray_t *rays, int nrays, double rmin, double rmax) {
    if (!b) return refuse("phys_batch_rays_configure", ck::RAYS_SIZE_REFUSAL);
    ck::RayCfg cfg;
    std::vector<ck::RayDef> table(nrays >= 1 && nrays <= ck::RAYS_MAX ? (size_t)nrays : 1);
    if (const char *why = ck::rays_configure(b->host_model, (const ck::RayDef *)rays, nrays, rmin, rmax, table.data(), cfg)) return refuse("phys_batch_rays_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table that goes away) */
    DevBuf<ck::RayDef> tab;
    DevBuf<double> out;
    if (!tab.alloc((size_t)nrays, false, "ray table")) return -1;
    if (!hip_ok(hipMemcpy(tab, table.data(), sizeof(ck::RayDef) * (size_t)nrays, hipMemcpyHostToDevice), "hipMemcpy(ray table)")) return -1;
    /* the field takes the table's size: a buffer of the batch's own of the new size (a caller's binding is dropped: bind again) */
    if (!out.alloc((size_t)nrays * (size_t)b->nenv, true, "ray ranges")) return -1;
    b->d_rays = std::move(tab);
    b->d_field[PHYS_F_RAYS] = std::move(out);
    b->dim[PHYS_F_RAYS] = nrays; b->stride[PHYS_F_RAYS] = nrays;
    b->rays = cfg;               /* (the default geoms again, no ids and no normals -- their size may have changed: bind them again) */
    return 0;
}
int phys_batch_rays_set_geoms(phys_batch_t *b, unsigned mask) {
    if (!b) return -1;
    if (b->rays.nrays <= 0) { phys_set_last_error("phys_batch_rays_set_geoms: call phys_batch_rays_configure first (it restores the default set)"); return -1; }
    if (const char *why = ck::check_ray_geoms(b->host_model, mask)) return refuse("phys_batch_rays_set_geoms", why);
    b->rays.geoms = mask;        /* (as phys_batch_bind: launches already queued keep the mask they were given) */
    return 0;
}
int phys_batch_rays_bind_ids(phys_batch_t *b, void *device_ptr) {
    if (!b) return -1;
    if (b->rays.nrays <= 0) { phys_set_last_error("phys_batch_rays_bind_ids: call phys_batch_rays_configure first (it sizes the table)"); return -1; }
    b->rays.ids = (int *)device_ptr;
    return 0;
}
int phys_batch_rays_bind_normals(phys_batch_t *b, void *device_ptr) {
    if (!b) return -1;
    if (b->rays.nrays <= 0) { phys_set_last_error("phys_batch_rays_bind_normals: call phys_batch_rays_configure first (it sizes the table)"); return -1; }
    b->rays.normals = (double *)device_ptr;
    return 0;
}
int phys_batch_debug_ray_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->ray_launches;
    return 0;
}
int phys_batch_rays_cast(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b) return -1;
    if (b->rays.nrays <= 0 || !b->d_field[PHYS_F_RAYS] || !b->d_rays) { phys_set_last_error("phys_batch_rays_cast: call phys_batch_rays_configure first"); return -1; }
    if (!range_ok(b, env0, n)) { phys_set_last_error("phys_batch_rays_cast: env range out of bounds"); return -1; }
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    ck::RayCfg rays = b->rays;
    rays.rays = b->d_rays;
    ++b->ray_launches;
    hipLaunchKernelGGL(ck::cassie_rays_kernel, dim3((unsigned)ck::rays_grid(n, rays.nrays)), dim3(WV_WAVE), 0, s,
                       ck::make_rays_io(view_of(b), rays, b->d_field[PHYS_F_RAYS], b->stride[PHYS_F_RAYS], env0, n));
    return hip_ok(hipGetLastError(), "cassie_rays_kernel launch") ? 0 : -1;
}

/* ------------------------------------------------ probes ---- */
static_assert(sizeof(ck::ProbeDef) == sizeof(phys_probe_t) && offsetof(ck::ProbeDef, id) == offsetof(phys_probe_t, id) &&
              offsetof(ck::ProbeDef, offset) == offsetof(phys_probe_t, offset), "phys_probe_t is the kernel's table entry");
static_assert(PHYS_PROBE_BODY == ck::PROBE_BODY && PHYS_PROBE_SITE == ck::PROBE_SITE && PHYS_PROBES_MAX == ck::PROBES_MAX, "the kinds' numbers");
static_assert((int)PHYS_PQ_COUNT == (int)ck::PQ_COUNT && PHYS_PQ_CFRC == 1 << ck::PQ_CFRC && PHYS_PQ_CONTACTS == 1 << ck::PQ_CONTACTS &&
              PHYS_PC_OBSTACLE == ck::PC_OBSTACLE && PHYS_PC_SELF == ck::PC_SELF && PHYS_PC_GROUP0 == ck::PC_GROUP0, "the header's quantities and contact bits are probe_kernels.h's");
/* doubles per env of the scratch outputs of the probes' forward pass */
static size_t probe_scratch_row(const cm_model_t &m) { return (size_t)(m.nv + m.nsensordata + m.nu + 7 * m.nbody); }
/* the record of a launch: what was configured, with the pointers into the batch's buffers */
static ck::ProbeCfg probe_cfg_of(const phys_batch *b) {
    ck::ProbeCfg c = b->probes;
    const cm_model_t &m = b->host_model;
    const size_t n = (size_t)b->nenv;
    c.probes = b->d_probes; c.geom_class = b->d_probe_geoms; c.ngeom = b->probe_ngeom; c.ext = b->d_probe_ext;
    c.qacc = b->d_probe_scratch;
    c.xpos = b->d_probe_scratch ? b->d_probe_scratch + n * (size_t)(m.nv + m.nsensordata + m.nu) : nullptr;
    c.xquat = c.xpos ? c.xpos + n * 3 * (size_t)m.nbody : nullptr;
    c.contacts = b->d_probe_contacts;
    return c;
}
int phys_batch_probe_geom_classes(phys_batch_t *b, const phys_model_t *host_model) {
    if (!b) { phys_set_last_error("phys_batch_probe_geom_classes: no batch"); return -1; }
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table that goes away) */
    if (!host_model) { b->d_probe_geoms.reset(); b->probe_ngeom = 0; return 0; }
    const int ngeom = phys_model_size(host_model, PHYS_NGEOM);
    /* (the contact list names geoms of the full list through the compiled model's geom_fullid: the table must hold them all) */
    for (int g = 0; g < b->host_model.ngeom; ++g)
        if (b->host_model.geom_fullid[g] < 0 || b->host_model.geom_fullid[g] >= ngeom) return refuse("phys_batch_probe_geom_classes", "not the host model the batch's model was compiled from (a geom_fullid lies outside its geom list)");
    std::vector<int> table((size_t)(ngeom > 0 ? ngeom : 1), 0);
    ck::probe_classify_geoms(phys_model_array((phys_model_t *)host_model, PHYS_M_GEOM_USER), phys_model_size(host_model, PHYS_NUSER_GEOM),
                             phys_model_iarray((phys_model_t *)host_model, PHYS_MI_GEOM_GROUP), ngeom, table.data());
    DevBuf<int> d;
    if (!d.alloc(table.size(), false, "geom classes")) return -1;
    if (!hip_ok(hipMemcpy(d, table.data(), sizeof(int) * table.size(), hipMemcpyHostToDevice), "hipMemcpy(geom classes)")) return -1;
    b->d_probe_geoms = std::move(d);
    b->probe_ngeom = ngeom;
    return 0;
}
int phys_batch_probes_configure(phys_batch_t *b, const phys_probe_t *probes, int nprobes, unsigned quantities) {
    if (!b) return refuse("phys_batch_probes_configure", ck::PROBES_SIZE_REFUSAL);
    ck::ProbeCfg cfg;
    if (const char *why = ck::probes_configure(b->host_model, (const ck::ProbeDef *)probes, nprobes, quantities, cfg)) return refuse("phys_batch_probes_configure", why);
    const bool words = nprobes > 0 && (quantities & PHYS_PQ_CONTACTS) != 0;
    if (words && !b->d_probe_geoms)
        return refuse("phys_batch_probes_configure", "PHYS_PQ_CONTACTS reads the geoms' classes, which the compiled model does not carry (phys_batch_probe_geom_classes first)");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table, or writing the rows, that go away) */
    if (nprobes == 0) {          /* release: everything but the geoms' classes, which are the model's */
        b->probes = {};
        b->d_probes.reset(); b->d_probe_ext.reset(); b->d_probe_scratch.reset(); b->d_probe_contacts.reset();
        b->d_field[PHYS_F_PROBES].reset();
        b->dim[PHYS_F_PROBES] = 0; b->stride[PHYS_F_PROBES] = 0;
        return 0;
    }
    const cm_model_t &m = b->host_model;
    const size_t n = (size_t)b->nenv;
    const int row = ck::probe_layout(nprobes, quantities, m.nv, nullptr, nullptr);
    DevBuf<ck::ProbeDef> tab;
    DevBuf<double> out;
    DevBuf<int> con;
    if (!tab.alloc((size_t)nprobes, false, "probe table")) return -1;
    if (!hip_ok(hipMemcpy(tab, probes, sizeof(ck::ProbeDef) * (size_t)nprobes, hipMemcpyHostToDevice), "hipMemcpy(probe table)")) return -1;
    /* the field takes the row's size: a buffer of the batch's own of the new size (a caller's binding is dropped: bind again); a row
     * without doubles -- the contact word alone -- keeps one, so that the field exists */
    if (!out.alloc(n * (size_t)(row > 0 ? row : 1), true, "probe rows")) return -1;
    if (words && !con.alloc(n, true, "probe contact words")) return -1;
    if (!b->d_probe_ext && !b->d_probe_ext.alloc(n, true, "probe read-out")) return -1;
    if (!b->d_probe_scratch && !b->d_probe_scratch.alloc(n * probe_scratch_row(m), true, "probe scratch outputs")) return -1;
    b->d_probes = std::move(tab);
    b->d_field[PHYS_F_PROBES] = std::move(out);
    b->dim[PHYS_F_PROBES] = row; b->stride[PHYS_F_PROBES] = row;
    b->d_probe_contacts = std::move(con);
    b->probes = cfg;
    b->probes.probes = nullptr;  /* (the caller's array: a launch reads the table in HBM) */
    return 0;
}
int phys_batch_probe_row_dim(const phys_batch_t *b) { return b && b->probes.nprobes > 0 ? b->dim[PHYS_F_PROBES] : 0; }
int phys_batch_probe_layout(const phys_batch_t *b, int *offsets, int *dims) {
    if (!b || b->probes.nprobes < 1) { phys_set_last_error("phys_batch_probe_layout: not configured (phys_batch_probes_configure first)"); return -1; }
    (void)ck::probe_layout(b->probes.nprobes, b->probes.quantities, b->host_model.nv, offsets, dims);
    return b->probes.nprobes;
}
void *phys_batch_probe_contacts_ptr(phys_batch_t *b) { return b ? (void *)b->d_probe_contacts.get() : nullptr; }
int phys_batch_probe_bind_contacts(phys_batch_t *b, void *device_ptr) {
    if (!b) { phys_set_last_error("phys_batch_probe_bind_contacts: no batch"); return -1; }
    if (b->probes.nprobes < 1 || !(b->probes.quantities & PHYS_PQ_CONTACTS)) return refuse("phys_batch_probe_bind_contacts", "configure the probes with PHYS_PQ_CONTACTS first");
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself.  NULL: the
     * batch's own words again, zeroed) */
    if (device_ptr) b->d_probe_contacts.borrow((int *)device_ptr);
    else if (!b->d_probe_contacts.owned() && !b->d_probe_contacts.alloc((size_t)b->nenv, true, "probe contact words")) return -1;
    return 0;
}
int phys_batch_probe_download_contacts(phys_batch_t *b, int *host) {
    if (!b || !host || !b->d_probe_contacts) { phys_set_last_error("phys_batch_probe_download_contacts: bad arguments, or the probes were not configured with PHYS_PQ_CONTACTS"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_probe_contacts, sizeof(int) * (size_t)b->nenv, hipMemcpyDeviceToHost), "probe contact words download") ? 0 : -1;
}
int phys_batch_debug_probe_launches(const phys_batch_t *b, long long *forward, long long *reduce) {
    if (!b) return -1;
    if (forward) *forward = b->probe_launches[0];
    if (reduce) *reduce = b->probe_launches[1];
    return 0;
}
int phys_batch_probe(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_probe: no batch"); return -1; }
    const ck::ProbeCfg c = probe_cfg_of(b);
    if (const char *why = ck::check_probe_call(c, b->nenv, env0, n)) return refuse("phys_batch_probe", why);
    if (!b->d_field[PHYS_F_PROBES] || !b->d_probe_scratch) return refuse("phys_batch_probe", "not configured (phys_batch_probes_configure first)");
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    /* the read-out of the current state of the range: a forward pass that stores to the probes' block and scratch alone */
    const cm_model_t &m = b->host_model;
    const size_t N = (size_t)b->nenv;
    double *const scratch = b->d_probe_scratch;
    const ReadoutPass pass = {b->d_probe_ext, scratch, scratch + N * (size_t)m.nv, scratch + N * (size_t)(m.nv + m.nsensordata),
                              const_cast<double *>(c.xpos), const_cast<double *>(c.xquat)};
    if (launch(b, 1, 0, s, false, env0, n, &pass) != 0) return -1;
    ++b->probe_launches[0];
    hipLaunchKernelGGL(ck::cassie_probe_kernel, dim3((unsigned)ck::probe_grid(n)), dim3(WV_WAVE), 0, s,
                       ck::make_probe_io(view_of(b), c, b->d_field[PHYS_F_PROBES], b->stride[PHYS_F_PROBES], env0, n));
    if (!hip_ok(hipGetLastError(), "cassie_probe_kernel launch")) return -1;
    ++b->probe_launches[1];
    return 0;
}

/* ------------------------------------------------ observation rows ---- */
static_assert(sizeof(ck::ObsTerm) == sizeof(phys_obs_term_t) && offsetof(ck::ObsTerm, qindex) == offsetof(phys_obs_term_t, qindex) &&
              offsetof(ck::ObsTerm, vec) == offsetof(phys_obs_term_t, vec) && offsetof(ck::ObsTerm, hi) == offsetof(phys_obs_term_t, hi),
              "phys_obs_term_t is the term obs_configure reads");
static_assert(PHYS_OBS_COPY == ck::OBS_COPY && PHYS_OBS_ROT_INV == ck::OBS_ROT_INV && PHYS_OBS_INPUT == ck::OBS_INPUT && PHYS_OBS_CONST == ck::OBS_CONST &&
              PHYS_OBS_F32 == ck::OBS_F32 && PHYS_OBS_F64 == ck::OBS_F64 && PHYS_OBS_MAXCOLS == ck::OBS_MAXCOLS, "the header's numbers are obs_kernels.h's");
/* what the batch holds of every field now: where a launch would read it */
static void obs_fields_of(const phys_batch *b, ck::ObsField *f) {
    for (int k = 0; k < PHYS_F_COUNT; ++k) f[k] = {b->d_field[k].get(), b->d_field[k] ? b->dim[k] : 0, b->stride[k]};
}
/* the record of a launch: what was configured, with the pointers into the batch's buffers */
static ck::ObsCfg obs_cfg_of(const phys_batch *b) {
    ck::ObsCfg c = b->obs;
    c.cols = b->d_obs_cols; c.rows = b->d_obs_rows.get(); c.srow = b->obs_srow; c.frames = b->d_obs_frames;
    return c;
}
int phys_batch_obs_configure(phys_batch_t *b, const phys_obs_term_t *terms, int nterms, int history, int dtype, unsigned long long seed, unsigned env_base) {
    if (!b) return refuse("phys_batch_obs_configure", ck::OBS_SIZE_REFUSAL);
    int dims[PHYS_F_COUNT];
    for (int k = 0; k < PHYS_F_COUNT; ++k) dims[k] = b->d_field[k] ? b->dim[k] : 0;
    std::vector<ck::ObsCol> table((size_t)ck::OBS_MAXCOLS);
    std::vector<int> term_col((size_t)(nterms > 0 ? nterms : 0));
    ck::ObsCfg cfg;
    if (const char *why = ck::obs_configure(dims, PHYS_F_COUNT, PHYS_F_DEPTH, (const ck::ObsTerm *)terms, nterms, history, dtype, seed, env_base,
                                            table.data(), term_col.data(), cfg)) return refuse("phys_batch_obs_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table, or writing the rows, that go away) */
    if (nterms == 0) {
        b->obs = {}; b->obs_term_col.clear(); b->obs_srow = 0;
        b->d_obs_cols.reset(); b->d_obs_rows.reset(); b->d_obs_frames.reset();
        return 0;
    }
    const size_t n = (size_t)b->nenv, row = (size_t)cfg.ncols * (size_t)cfg.history;
    DevBuf<ck::ObsCol> cols;
    DevBuf<char> rows;
    DevBuf<unsigned> frames;
    if (!cols.alloc((size_t)cfg.ncols, false, "observation columns")) return -1;
    if (!hip_ok(hipMemcpy(cols, table.data(), sizeof(ck::ObsCol) * (size_t)cfg.ncols, hipMemcpyHostToDevice), "hipMemcpy(observation columns)")) return -1;
    if (!rows.alloc(n * row * (size_t)dtype, true, "observation rows")) return -1;
    if (!frames.alloc(n, true, "observation frame counts")) return -1;
    b->d_obs_cols = std::move(cols); b->d_obs_rows = std::move(rows); b->d_obs_frames = std::move(frames);
    b->obs_srow = (long long)row;
    b->obs_term_col = std::move(term_col);
    b->obs = cfg;   /* (no input bound, and the rows are the batch's own: the bindings are dropped) */
    return 0;
}
int phys_batch_obs_bind(phys_batch_t *b, void *device_ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_obs_bind: no batch"); return -1; }
    const long long row = (long long)b->obs.ncols * b->obs.history;
    if (const char *why = ck::check_obs_bind(b->obs, device_ptr ? row_stride : row)) return refuse("phys_batch_obs_bind", why);
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    if (device_ptr) { b->d_obs_rows.borrow((char *)device_ptr); b->obs_srow = row_stride; }
    else if (!b->d_obs_rows.owned()) {
        if (!b->d_obs_rows.alloc((size_t)b->nenv * (size_t)row * (size_t)b->obs.dtype, true, "observation rows")) return -1;
        b->obs_srow = row;
    }
    return 0;
}
int phys_batch_obs_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype) {
    if (!b) { phys_set_last_error("phys_batch_obs_bind_input: no batch"); return -1; }
    if (!device_ptr) { b->obs.input = nullptr; b->obs.input_dim = 0; b->obs.input_stride = 0; b->obs.input_dtype = 0; return 0; }
    if (const char *why = ck::check_obs_input(b->obs, dim, row_stride, dtype)) return refuse("phys_batch_obs_bind_input", why);
    b->obs.input = device_ptr; b->obs.input_dim = dim; b->obs.input_stride = (int)row_stride; b->obs.input_dtype = dtype;
    return 0;
}
int phys_batch_obs(phys_batch_t *b, int env0, int n, const void *refill_ptr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_obs: no batch"); return -1; }
    const ck::ObsCfg c = obs_cfg_of(b);
    ck::ObsField fields[PHYS_F_COUNT];
    obs_fields_of(b, fields);
    if (const char *why = ck::check_obs_call(c, fields, PHYS_F_COUNT, b->nenv, env0, n)) return refuse("phys_batch_obs", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_obs_kernel, dim3((unsigned)ck::obs_grid(n)), dim3(WV_WAVE), 0, s, ck::make_obs_io(c, fields, env0, n, (const int *)refill_ptr));
    if (!hip_ok(hipGetLastError(), "cassie_obs_kernel launch")) return -1;
    ++b->obs_launches;
    return 0;
}
int phys_batch_obs_dim(const phys_batch_t *b, int *ncols, int *history, int *row) {
    if (!b || b->obs.nterms < 1) { phys_set_last_error("phys_batch_obs_dim: not configured (phys_batch_obs_configure first)"); return -1; }
    if (ncols) *ncols = b->obs.ncols;
    if (history) *history = b->obs.history;
    if (row) *row = b->obs.ncols * b->obs.history;
    return 0;
}
int phys_batch_obs_layout(const phys_batch_t *b, int *first_col) {
    if (!b || b->obs.nterms < 1) { phys_set_last_error("phys_batch_obs_layout: not configured (phys_batch_obs_configure first)"); return -1; }
    if (first_col) memcpy(first_col, b->obs_term_col.data(), sizeof(int) * b->obs_term_col.size());
    return b->obs.nterms;
}
int phys_batch_obs_download(phys_batch_t *b, void *host, int env0, int n) {
    if (!b || !host || b->obs.nterms < 1 || !b->d_obs_rows) { phys_set_last_error("phys_batch_obs_download: bad arguments, or not configured (phys_batch_obs_configure first)"); return -1; }
    if (!range_ok(b, env0, n)) return refuse("phys_batch_obs_download", "env range out of bounds");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (n == 0) return 0;
    const size_t el = (size_t)b->obs.dtype, row = (size_t)b->obs.ncols * (size_t)b->obs.history, st = (size_t)b->obs_srow;
    return hip_ok(hipMemcpy2D(host, el * row, b->d_obs_rows.get() + el * st * (size_t)env0, el * st, el * row, (size_t)n, hipMemcpyDeviceToHost), "observation rows download") ? 0 : -1;
}
int phys_batch_obs_frames(phys_batch_t *b, unsigned *host) {
    if (!b || !host || !b->d_obs_frames) { phys_set_last_error("phys_batch_obs_frames: bad arguments, or not configured (phys_batch_obs_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_obs_frames, sizeof(unsigned) * (size_t)b->nenv, hipMemcpyDeviceToHost), "observation frame counts download") ? 0 : -1;
}
int phys_batch_obs_set_frames(phys_batch_t *b, const unsigned *host) {
    if (!b || !host || !b->d_obs_frames) { phys_set_last_error("phys_batch_obs_set_frames: bad arguments, or not configured (phys_batch_obs_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(b->d_obs_frames, host, sizeof(unsigned) * (size_t)b->nenv, hipMemcpyHostToDevice), "observation frame counts upload") ? 0 : -1;
}
int phys_batch_debug_obs_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->obs_launches;
    return 0;
}

/* ------------------------------------------------ reward rows ---- */
static_assert(sizeof(ck::RewardTerm) == sizeof(phys_reward_term_t) && offsetof(ck::RewardTerm, root) == offsetof(phys_reward_term_t, root) &&
              offsetof(ck::RewardTerm, vec) == offsetof(phys_reward_term_t, vec) && offsetof(ck::RewardTerm, weight) == offsetof(phys_reward_term_t, weight),
              "phys_reward_term_t is the term reward_configure reads");
static_assert(PHYS_REW_VEC == ck::REW_VEC && PHYS_REW_ROT_INV == ck::REW_ROT_INV && PHYS_REW_QUAT == ck::REW_QUAT && PHYS_REW_SUMSQ == ck::REW_SUMSQ &&
              PHYS_REW_SUMABS == ck::REW_SUMABS && PHYS_REW_MAXABS == ck::REW_MAXABS && PHYS_REW_LINEAR == ck::REW_LINEAR && PHYS_REW_EXP == ck::REW_EXP &&
              PHYS_REW_RATIONAL == ck::REW_RATIONAL && PHYS_REW_INPUT == ck::REW_INPUT && PHYS_REW_CONST == ck::REW_CONST && PHYS_REW_NONE == ck::REW_NONE &&
              PHYS_REW_MAXTERMS == ck::REWARD_MAXTERMS, "the header's numbers are reward_kernels.h's");
/* the record of a launch: what was configured, with the pointers into the batch's buffers */
static ck::RewardCfg reward_cfg_of(const phys_batch *b) {
    ck::RewardCfg c = b->reward;
    c.terms = b->d_reward_terms; c.rew = b->d_reward.get(); c.srew = b->reward_srew; c.trows = b->d_reward_trows.get(); c.sterm = b->reward_sterm;
    c.ret = b->d_reward_ret; c.fin = b->d_reward_final;
    return c;
}
int phys_batch_reward_configure(phys_batch_t *b, const phys_reward_term_t *terms, int nterms, int dtype, double lo, double hi) {
    if (!b) return refuse("phys_batch_reward_configure", ck::REWARD_SIZE_REFUSAL);
    int dims[PHYS_F_COUNT];
    for (int k = 0; k < PHYS_F_COUNT; ++k) dims[k] = b->d_field[k] ? b->dim[k] : 0;
    std::vector<ck::RewardTerm> table((size_t)ck::REWARD_MAXTERMS);
    ck::RewardCfg cfg;
    if (const char *why = ck::reward_configure(dims, PHYS_F_COUNT, PHYS_F_DEPTH, (const ck::RewardTerm *)terms, nterms, dtype, lo, hi, table.data(), cfg))
        return refuse("phys_batch_reward_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table, or writing the rewards, that go away) */
    if (nterms == 0) {
        b->reward = {}; b->reward_srew = 0; b->reward_sterm = 0;
        b->d_reward_terms.reset(); b->d_reward.reset(); b->d_reward_trows.reset(); b->d_reward_ret.reset(); b->d_reward_final.reset();
        return 0;
    }
    const size_t n = (size_t)b->nenv;
    DevBuf<ck::RewardTerm> tab;
    DevBuf<char> rew;
    DevBuf<double> ret, fin;
    if (!tab.alloc((size_t)nterms, false, "reward terms")) return -1;
    if (!hip_ok(hipMemcpy(tab, table.data(), sizeof(ck::RewardTerm) * (size_t)nterms, hipMemcpyHostToDevice), "hipMemcpy(reward terms)")) return -1;
    if (!rew.alloc(n * (size_t)dtype, true, "rewards")) return -1;
    if (!ret.alloc(n, true, "returns") || !fin.alloc(n, true, "final returns")) return -1;
    b->d_reward_terms = std::move(tab); b->d_reward = std::move(rew); b->d_reward_ret = std::move(ret); b->d_reward_final = std::move(fin);
    b->d_reward_trows.reset();
    b->reward_srew = 1; b->reward_sterm = 0;
    b->reward = cfg;   /* (no input bound, the rewards are the batch's own and no term rows are written: the bindings are dropped) */
    return 0;
}
int phys_batch_reward_bind(phys_batch_t *b, void *device_ptr, long long stride) {
    if (!b) { phys_set_last_error("phys_batch_reward_bind: no batch"); return -1; }
    if (const char *why = ck::check_reward_bind(b->reward, device_ptr ? stride : 1, 1)) return refuse("phys_batch_reward_bind", why);
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    if (device_ptr) { b->d_reward.borrow((char *)device_ptr); b->reward_srew = stride; }
    else if (!b->d_reward.owned()) {
        if (!b->d_reward.alloc((size_t)b->nenv * (size_t)b->reward.dtype, true, "rewards")) return -1;
        b->reward_srew = 1;
    }
    return 0;
}
int phys_batch_reward_bind_terms(phys_batch_t *b, void *device_ptr, long long row_stride, int own) {
    if (!b) { phys_set_last_error("phys_batch_reward_bind_terms: no batch"); return -1; }
    const long long nt = b->reward.nterms;
    if (const char *why = ck::check_reward_bind(b->reward, device_ptr ? row_stride : nt, nt > 1 ? nt : 1)) return refuse("phys_batch_reward_bind_terms", why);
    (void)hipSetDevice(b->device);
    if (device_ptr) { b->d_reward_trows.borrow((char *)device_ptr); b->reward_sterm = row_stride; }
    else if (own) {
        if (!b->d_reward_trows.owned() && !b->d_reward_trows.alloc((size_t)b->nenv * (size_t)nt * (size_t)b->reward.dtype, true, "reward term rows")) return -1;
        b->reward_sterm = nt;
    } else { b->d_reward_trows.reset(); b->reward_sterm = 0; }
    return 0;
}
int phys_batch_reward_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype) {
    if (!b) { phys_set_last_error("phys_batch_reward_bind_input: no batch"); return -1; }
    if (!device_ptr) { b->reward.input = nullptr; b->reward.input_dim = 0; b->reward.input_stride = 0; b->reward.input_dtype = 0; return 0; }
    if (const char *why = ck::check_reward_input(b->reward, dim, row_stride, dtype)) return refuse("phys_batch_reward_bind_input", why);
    b->reward.input = device_ptr; b->reward.input_dim = dim; b->reward.input_stride = (int)row_stride; b->reward.input_dtype = dtype;
    return 0;
}
int phys_batch_reward(phys_batch_t *b, int env0, int n, const void *reset_ptr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_reward: no batch"); return -1; }
    const ck::RewardCfg c = reward_cfg_of(b);
    ck::ObsField fields[PHYS_F_COUNT];
    obs_fields_of(b, fields);
    if (const char *why = ck::check_reward_call(c, fields, PHYS_F_COUNT, b->nenv, env0, n)) return refuse("phys_batch_reward", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_reward_kernel, dim3((unsigned)ck::reward_grid(n)), dim3(WV_WAVE), 0, s, ck::make_reward_io(c, fields, env0, n, (const int *)reset_ptr));
    if (!hip_ok(hipGetLastError(), "cassie_reward_kernel launch")) return -1;
    ++b->reward_launches;
    return 0;
}
int phys_batch_reward_dim(const phys_batch_t *b, int *nterms, int *dtype, int *term_rows) {
    if (!b || b->reward.nterms < 1) { phys_set_last_error("phys_batch_reward_dim: not configured (phys_batch_reward_configure first)"); return -1; }
    if (nterms) *nterms = b->reward.nterms;
    if (dtype) *dtype = b->reward.dtype;
    if (term_rows) *term_rows = b->d_reward_trows ? 1 : 0;
    return 0;
}
/* rows of `width` elements, `stride` elements apart on the device, to dense host memory */
static int reward_rows_down(phys_batch *b, const char *entry, const char *base, size_t width, size_t stride, void *host, int env0, int n) {
    if (!range_ok(b, env0, n)) return refuse(entry, "env range out of bounds");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (n == 0) return 0;
    const size_t el = (size_t)b->reward.dtype;
    return hip_ok(hipMemcpy2D(host, el * width, base + el * stride * (size_t)env0, el * stride, el * width, (size_t)n, hipMemcpyDeviceToHost), entry) ? 0 : -1;
}
int phys_batch_reward_download(phys_batch_t *b, void *host, int env0, int n) {
    if (!b || !host || b->reward.nterms < 1 || !b->d_reward) { phys_set_last_error("phys_batch_reward_download: bad arguments, or not configured (phys_batch_reward_configure first)"); return -1; }
    return reward_rows_down(b, "phys_batch_reward_download", b->d_reward.get(), 1, (size_t)b->reward_srew, host, env0, n);
}
int phys_batch_reward_download_terms(phys_batch_t *b, void *host, int env0, int n) {
    if (!b || !host || b->reward.nterms < 1) { phys_set_last_error("phys_batch_reward_download_terms: bad arguments, or not configured (phys_batch_reward_configure first)"); return -1; }
    if (!b->d_reward_trows) return refuse("phys_batch_reward_download_terms", "no term rows (phys_batch_reward_bind_terms first)");
    return reward_rows_down(b, "phys_batch_reward_download_terms", b->d_reward_trows.get(), (size_t)b->reward.nterms, (size_t)b->reward_sterm, host, env0, n);
}
int phys_batch_reward_returns(phys_batch_t *b, double *host) {
    if (!b || !host || !b->d_reward_ret) { phys_set_last_error("phys_batch_reward_returns: bad arguments, or not configured (phys_batch_reward_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_reward_ret, sizeof(double) * (size_t)b->nenv, hipMemcpyDeviceToHost), "returns download") ? 0 : -1;
}
int phys_batch_reward_set_returns(phys_batch_t *b, const double *host) {
    if (!b || !host || !b->d_reward_ret) { phys_set_last_error("phys_batch_reward_set_returns: bad arguments, or not configured (phys_batch_reward_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(b->d_reward_ret, host, sizeof(double) * (size_t)b->nenv, hipMemcpyHostToDevice), "returns upload") ? 0 : -1;
}
int phys_batch_reward_final(phys_batch_t *b, double *host) {
    if (!b || !host || !b->d_reward_final) { phys_set_last_error("phys_batch_reward_final: bad arguments, or not configured (phys_batch_reward_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_reward_final, sizeof(double) * (size_t)b->nenv, hipMemcpyDeviceToHost), "final returns download") ? 0 : -1;
}
int phys_batch_debug_reward_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->reward_launches;
    return 0;
}

/* ------------------------------------------------ action rows ---- */
static_assert(sizeof(ck::ActColDef) == sizeof(phys_act_col_t) && offsetof(ck::ActColDef, dindex) == offsetof(phys_act_col_t, dindex) &&
              offsetof(ck::ActColDef, lo) == offsetof(phys_act_col_t, lo) && offsetof(ck::ActColDef, smooth) == offsetof(phys_act_col_t, smooth) &&
              offsetof(ck::ActColDef, out_hi) == offsetof(phys_act_col_t, out_hi), "phys_act_col_t is the column act_configure reads");
static_assert(PHYS_ACT_INPUT == ck::ACT_INPUT && PHYS_ACT_CONST == ck::ACT_CONST && PHYS_ACT_NONE == ck::ACT_NONE && PHYS_ACT_NOW == ck::ACT_NOW &&
              PHYS_ACT_PREV == ck::ACT_PREV && PHYS_ACT_APPLIED == ck::ACT_APPLIED && PHYS_ACT_MAXCOLS == ck::ACT_MAXCOLS && PHYS_ACT_MAXDELAY == ck::ACT_MAXDELAY,
              "the header's numbers are act_kernels.h's");
/* the fields a column may write: what a stepping launch reads as its commands */
static const int ACT_CMD_FIELDS[ck::ACT_MAXDST] = {PHYS_F_PD_PTARGET, PHYS_F_PD_DTARGET, PHYS_F_PD_KP, PHYS_F_PD_KD, PHYS_F_PD_TORQUE, PHYS_F_DRIVE_CMD,
                                                   PHYS_F_CTRL, PHYS_F_QFRC_APPLIED, PHYS_F_XFRC_APPLIED};
/* the record of a launch: what was configured, with the pointers into the batch's buffers */
static ck::ActCfg act_cfg_of(const phys_batch *b) {
    ck::ActCfg c = b->act;
    c.cols = b->d_act_cols; c.rows = b->d_act_rows.get(); c.srow = b->act_srow; c.state = b->d_act_state; c.counts = b->d_act_counts;
    return c;
}
int phys_batch_act_configure(phys_batch_t *b, const phys_act_col_t *cols, int ncols, int delay_max, int dtype, unsigned long long seed, unsigned env_base) {
    if (!b) return refuse("phys_batch_act_configure", ck::ACT_SIZE_REFUSAL);
    int dims[PHYS_F_COUNT];
    for (int k = 0; k < PHYS_F_COUNT; ++k) dims[k] = b->d_field[k] ? b->dim[k] : 0;
    std::vector<ck::ActCol> table((size_t)ck::ACT_MAXCOLS);
    ck::ActCfg cfg;
    if (const char *why = ck::act_configure(dims, PHYS_F_COUNT, PHYS_F_DEPTH, ACT_CMD_FIELDS, ck::ACT_MAXDST, (const ck::ActColDef *)cols, ncols, delay_max, dtype,
                                            seed, env_base, table.data(), cfg)) return refuse("phys_batch_act_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table, or writing the rows, that go away) */
    if (ncols == 0) {
        b->act = {}; b->act_srow = 0;
        b->d_act_cols.reset(); b->d_act_rows.reset(); b->d_act_state.reset(); b->d_act_counts.reset();
        return 0;
    }
    const size_t n = (size_t)b->nenv, row = (size_t)ck::ACT_FRAMES * (size_t)ncols;
    DevBuf<ck::ActCol> tab;
    DevBuf<char> rows;
    DevBuf<double> state;
    DevBuf<unsigned> counts;
    if (!tab.alloc((size_t)ncols, false, "action columns")) return -1;
    if (!hip_ok(hipMemcpy(tab, table.data(), sizeof(ck::ActCol) * (size_t)ncols, hipMemcpyHostToDevice), "hipMemcpy(action columns)")) return -1;
    if (!rows.alloc(n * row * (size_t)dtype, true, "action rows")) return -1;
    if (!state.alloc(n * (size_t)ck::act_state_dim(cfg), true, "action state")) return -1;
    if (!counts.alloc(n, true, "action call counts")) return -1;
    b->d_act_cols = std::move(tab); b->d_act_rows = std::move(rows); b->d_act_state = std::move(state); b->d_act_counts = std::move(counts);
    b->act_srow = (long long)row;
    b->act = cfg;   /* (no actions, input or delays bound, and the rows are the batch's own: the bindings are dropped) */
    /* (a destination the step kernel is handed only once somebody writes it -- the applied forces, the PD's velocity targets and
     * feed-forward torques -- is in use from here on, as after an upload or a binding: the buffers are zeroed until the first call) */
    for (int s = 0; s < cfg.ndst; ++s) note_field_in_use(b, cfg.dst_field[s]);
    return 0;
}
int phys_batch_act_bind_actions(phys_batch_t *b, const void *device_ptr, long long row_stride, int dtype) {
    if (!b) { phys_set_last_error("phys_batch_act_bind_actions: no batch"); return -1; }
    if (!device_ptr) { b->act.actions = nullptr; b->act.act_stride = 0; b->act.act_dtype = 0; return 0; }
    if (const char *why = ck::check_act_bind_actions(b->act, row_stride, dtype)) return refuse("phys_batch_act_bind_actions", why);
    b->act.actions = device_ptr; b->act.act_stride = row_stride; b->act.act_dtype = dtype;
    return 0;
}
int phys_batch_act_bind_rows(phys_batch_t *b, void *device_ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_act_bind_rows: no batch"); return -1; }
    const long long row = (long long)ck::ACT_FRAMES * b->act.ncols;
    if (const char *why = ck::check_act_bind_rows(b->act, device_ptr ? row_stride : row)) return refuse("phys_batch_act_bind_rows", why);
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    if (device_ptr) { b->d_act_rows.borrow((char *)device_ptr); b->act_srow = row_stride; }
    else if (!b->d_act_rows.owned()) {
        if (!b->d_act_rows.alloc((size_t)b->nenv * (size_t)row * (size_t)b->act.dtype, true, "action rows")) return -1;
        b->act_srow = row;
    }
    return 0;
}
int phys_batch_act_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype) {
    if (!b) { phys_set_last_error("phys_batch_act_bind_input: no batch"); return -1; }
    if (!device_ptr) { b->act.input = nullptr; b->act.input_dim = 0; b->act.input_stride = 0; b->act.input_dtype = 0; return 0; }
    if (const char *why = ck::check_act_bind_input(b->act, dim, row_stride, dtype)) return refuse("phys_batch_act_bind_input", why);
    b->act.input = device_ptr; b->act.input_dim = dim; b->act.input_stride = (int)row_stride; b->act.input_dtype = dtype;
    return 0;
}
int phys_batch_act_bind_delay(phys_batch_t *b, const void *device_ptr) {
    if (!b) { phys_set_last_error("phys_batch_act_bind_delay: no batch"); return -1; }
    if (device_ptr && b->act.ncols < 1) return refuse("phys_batch_act_bind_delay", "not configured (phys_batch_act_configure first)");
    b->act.delay = (const int *)device_ptr;
    return 0;
}
int phys_batch_act(phys_batch_t *b, int env0, int n, const void *reset_ptr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_act: no batch"); return -1; }
    const ck::ActCfg c = act_cfg_of(b);
    ck::ObsField fields[PHYS_F_COUNT];
    obs_fields_of(b, fields);
    if (const char *why = ck::check_act_call(c, fields, PHYS_F_COUNT, b->nenv, env0, n)) return refuse("phys_batch_act", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_act_kernel, dim3((unsigned)ck::act_grid(n)), dim3(WV_WAVE), 0, s, ck::make_act_io(c, fields, env0, n, (const int *)reset_ptr));
    if (!hip_ok(hipGetLastError(), "cassie_act_kernel launch")) return -1;
    ++b->act_launches;
    return 0;
}
int phys_batch_act_dim(const phys_batch_t *b, int *ncols, int *delay_max, int *row, int *state) {
    if (!b || b->act.ncols < 1) { phys_set_last_error("phys_batch_act_dim: not configured (phys_batch_act_configure first)"); return -1; }
    if (ncols) *ncols = b->act.ncols;
    if (delay_max) *delay_max = b->act.delay_max;
    if (row) *row = ck::ACT_FRAMES * b->act.ncols;
    if (state) *state = (int)ck::act_state_dim(b->act);
    return 0;
}
int phys_batch_act_download(phys_batch_t *b, void *host, int env0, int n) {
    if (!b || !host || b->act.ncols < 1 || !b->d_act_rows) { phys_set_last_error("phys_batch_act_download: bad arguments, or not configured (phys_batch_act_configure first)"); return -1; }
    if (!range_ok(b, env0, n)) return refuse("phys_batch_act_download", "env range out of bounds");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (n == 0) return 0;
    const size_t el = (size_t)b->act.dtype, row = (size_t)ck::ACT_FRAMES * (size_t)b->act.ncols, st = (size_t)b->act_srow;
    return hip_ok(hipMemcpy2D(host, el * row, b->d_act_rows.get() + el * st * (size_t)env0, el * st, el * row, (size_t)n, hipMemcpyDeviceToHost), "action rows download") ? 0 : -1;
}
int phys_batch_act_state(phys_batch_t *b, double *state_host, unsigned *counts_host) {
    if (!b || !state_host || !counts_host || !b->d_act_state || !b->d_act_counts) { phys_set_last_error("phys_batch_act_state: bad arguments, or not configured (phys_batch_act_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    const size_t n = (size_t)b->nenv;
    return quiesce(b) && hip_ok(hipMemcpy(state_host, b->d_act_state, sizeof(double) * n * (size_t)ck::act_state_dim(b->act), hipMemcpyDeviceToHost), "action state download") &&
                   hip_ok(hipMemcpy(counts_host, b->d_act_counts, sizeof(unsigned) * n, hipMemcpyDeviceToHost), "action call counts download") ? 0 : -1;
}
int phys_batch_act_set_state(phys_batch_t *b, const double *state_host, const unsigned *counts_host) {
    if (!b || !state_host || !counts_host || !b->d_act_state || !b->d_act_counts) { phys_set_last_error("phys_batch_act_set_state: bad arguments, or not configured (phys_batch_act_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    const size_t n = (size_t)b->nenv;
    return quiesce(b) && hip_ok(hipMemcpy(b->d_act_state, state_host, sizeof(double) * n * (size_t)ck::act_state_dim(b->act), hipMemcpyHostToDevice), "action state upload") &&
                   hip_ok(hipMemcpy(b->d_act_counts, counts_host, sizeof(unsigned) * n, hipMemcpyHostToDevice), "action call counts upload") ? 0 : -1;
}
int phys_batch_debug_act_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->act_launches;
    return 0;
}

/* ------------------------------------------------ task rows ---- */
static_assert(sizeof(ck::TaskColDef) == sizeof(phys_task_col_t) && offsetof(ck::TaskColDef, dindex) == offsetof(phys_task_col_t, dindex) &&
              offsetof(ck::TaskColDef, hold) == offsetof(phys_task_col_t, hold) && offsetof(ck::TaskColDef, p_rest) == offsetof(phys_task_col_t, p_rest) &&
              offsetof(ck::TaskColDef, phase0) == offsetof(phys_task_col_t, phase0) && offsetof(ck::TaskColDef, scale) == offsetof(phys_task_col_t, scale),
              "phys_task_col_t is the column task_configure reads");
static_assert(PHYS_TASK_SAMPLE == ck::TASK_SAMPLE && PHYS_TASK_PHASE == ck::TASK_PHASE && PHYS_TASK_WAVE == ck::TASK_WAVE && PHYS_TASK_TABLE == ck::TASK_TABLE &&
              PHYS_TASK_SAW == ck::TASK_SAW && PHYS_TASK_SIN == ck::TASK_SIN && PHYS_TASK_COS == ck::TASK_COS && PHYS_TASK_TRAPEZOID == ck::TASK_TRAPEZOID &&
              PHYS_TASK_NONE == ck::TASK_NONE && PHYS_TASK_NONE == PHYS_ACT_NONE && PHYS_TASK_MAXCOLS == ck::TASK_MAXCOLS &&
              PHYS_TASK_MAXFRAMES == ck::TASK_MAXFRAMES && PHYS_TASK_MAXTCOLS == ck::TASK_MAXTCOLS, "the header's numbers are task_kernels.h's");
/* the record of a launch: what was configured, with the pointers into the batch's buffers */
static ck::TaskCfg task_cfg_of(const phys_batch *b) {
    ck::TaskCfg c = b->task;
    c.cols = b->d_task_cols; c.rows = b->d_task_rows.get(); c.srow = b->task_srow; c.state = b->d_task_state; c.words = b->d_task_words; c.counts = b->d_task_counts;
    c.table = b->d_task_table; c.nframes = b->task_nframes; c.tcols = b->task_tcols;
    return c;
}
int phys_batch_task_set_table(phys_batch_t *b, const double *host, int nframes, int tcols) {
    if (!b) return refuse("phys_batch_task_set_table", ck::TASK_TABLE_REFUSAL);
    if (const char *why = ck::check_task_table(b->task, host, nframes, tcols)) return refuse("phys_batch_task_set_table", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table that goes away) */
    const size_t count = (size_t)nframes * (size_t)tcols;
    DevBuf<double> tab;
    if (!tab.alloc(count, false, "task table")) return -1;
    if (!hip_ok(hipMemcpy(tab, host, sizeof(double) * count, hipMemcpyHostToDevice), "hipMemcpy(task table)")) return -1;
    b->d_task_table = std::move(tab); b->task_nframes = nframes; b->task_tcols = tcols;
    return 0;
}
int phys_batch_task_configure(phys_batch_t *b, const phys_task_col_t *cols, int ncols, int dtype, unsigned long long seed, unsigned env_base) {
    if (!b) return refuse("phys_batch_task_configure", ck::TASK_SIZE_REFUSAL);
    int dims[PHYS_F_COUNT];
    for (int k = 0; k < PHYS_F_COUNT; ++k) dims[k] = b->d_field[k] ? b->dim[k] : 0;
    std::vector<ck::TaskCol> table((size_t)ck::TASK_MAXCOLS);
    ck::TaskCfg cfg;
    if (const char *why = ck::task_configure(dims, PHYS_F_COUNT, ACT_CMD_FIELDS, ck::ACT_MAXDST, (const ck::TaskColDef *)cols, ncols, dtype, seed, env_base,
                                             b->d_task_table ? b->task_nframes : 0, b->d_task_table ? b->task_tcols : 0, table.data(), cfg))
        return refuse("phys_batch_task_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table, or writing the rows, that go away) */
    const size_t n = (size_t)b->nenv;
    DevBuf<ck::TaskCol> tab;
    DevBuf<char> rows;
    DevBuf<double> state;
    DevBuf<unsigned> words, counts;
    if (!tab.alloc((size_t)ncols, false, "task columns")) return -1;
    if (!hip_ok(hipMemcpy(tab, table.data(), sizeof(ck::TaskCol) * (size_t)ncols, hipMemcpyHostToDevice), "hipMemcpy(task columns)")) return -1;
    if (!rows.alloc(n * (size_t)ncols * (size_t)dtype, true, "task rows")) return -1;
    if (!state.alloc(n * (size_t)ncols, true, "task state")) return -1;
    if (!words.alloc(n * (size_t)ck::TASK_WORDS * (size_t)ncols, true, "task words")) return -1;
    if (!counts.alloc(n, true, "task call counts")) return -1;
    b->d_task_cols = std::move(tab); b->d_task_rows = std::move(rows); b->d_task_state = std::move(state); b->d_task_words = std::move(words);
    b->d_task_counts = std::move(counts);
    b->task_srow = (long long)ncols;
    b->task = cfg;   /* (the rows are the batch's own: the binding is dropped) */
    /* (as phys_batch_act_configure: a destination the step kernel is handed only once somebody writes it is in use from here on) */
    for (int s = 0; s < cfg.ndst; ++s) note_field_in_use(b, cfg.dst_field[s]);
    return 0;
}
int phys_batch_task_bind_rows(phys_batch_t *b, void *device_ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_task_bind_rows: no batch"); return -1; }
    const long long row = b->task.ncols;
    if (const char *why = ck::check_task_bind_rows(b->task, device_ptr ? row_stride : row)) return refuse("phys_batch_task_bind_rows", why);
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    if (device_ptr) { b->d_task_rows.borrow((char *)device_ptr); b->task_srow = row_stride; }
    else if (!b->d_task_rows.owned()) {
        if (!b->d_task_rows.alloc((size_t)b->nenv * (size_t)row * (size_t)b->task.dtype, true, "task rows")) return -1;
        b->task_srow = row;
    }
    return 0;
}
int phys_batch_task(phys_batch_t *b, int env0, int n, const void *reset_ptr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_task: no batch"); return -1; }
    const ck::TaskCfg c = task_cfg_of(b);
    ck::ObsField fields[PHYS_F_COUNT];
    obs_fields_of(b, fields);
    if (const char *why = ck::check_task_call(c, fields, PHYS_F_COUNT, b->nenv, env0, n)) return refuse("phys_batch_task", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_task_kernel, dim3((unsigned)ck::task_grid(n)), dim3(WV_WAVE), 0, s, ck::make_task_io(c, fields, env0, n, (const int *)reset_ptr));
    if (!hip_ok(hipGetLastError(), "cassie_task_kernel launch")) return -1;
    ++b->task_launches;
    return 0;
}
int phys_batch_task_dim(const phys_batch_t *b, int *ncols, int *dtype) {
    if (!b || b->task.ncols < 1) { phys_set_last_error("phys_batch_task_dim: not configured (phys_batch_task_configure first)"); return -1; }
    if (ncols) *ncols = b->task.ncols;
    if (dtype) *dtype = b->task.dtype;
    return 0;
}
int phys_batch_task_download(phys_batch_t *b, void *host, int env0, int n) {
    if (!b || !host || b->task.ncols < 1 || !b->d_task_rows) { phys_set_last_error("phys_batch_task_download: bad arguments, or not configured (phys_batch_task_configure first)"); return -1; }
    if (!range_ok(b, env0, n)) return refuse("phys_batch_task_download", "env range out of bounds");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (n == 0) return 0;
    const size_t el = (size_t)b->task.dtype, row = (size_t)b->task.ncols, st = (size_t)b->task_srow;
    return hip_ok(hipMemcpy2D(host, el * row, b->d_task_rows.get() + el * st * (size_t)env0, el * st, el * row, (size_t)n, hipMemcpyDeviceToHost), "task rows download") ? 0 : -1;
}
int phys_batch_task_state(phys_batch_t *b, double *state_host, unsigned *words_host, unsigned *counts_host) {
    if (!b || !state_host || !words_host || !counts_host || !b->d_task_state || !b->d_task_words || !b->d_task_counts) {
        phys_set_last_error("phys_batch_task_state: bad arguments, or not configured (phys_batch_task_configure first)"); return -1;
    }
    (void)hipSetDevice(b->device);
    const size_t n = (size_t)b->nenv, nc = (size_t)b->task.ncols;
    return quiesce(b) && hip_ok(hipMemcpy(state_host, b->d_task_state, sizeof(double) * n * nc, hipMemcpyDeviceToHost), "task state download") &&
                   hip_ok(hipMemcpy(words_host, b->d_task_words, sizeof(unsigned) * n * ck::TASK_WORDS * nc, hipMemcpyDeviceToHost), "task words download") &&
                   hip_ok(hipMemcpy(counts_host, b->d_task_counts, sizeof(unsigned) * n, hipMemcpyDeviceToHost), "task call counts download") ? 0 : -1;
}
int phys_batch_task_set_state(phys_batch_t *b, const double *state_host, const unsigned *words_host, const unsigned *counts_host) {
    if (!b || !state_host || !words_host || !counts_host || !b->d_task_state || !b->d_task_words || !b->d_task_counts) {
        phys_set_last_error("phys_batch_task_set_state: bad arguments, or not configured (phys_batch_task_configure first)"); return -1;
    }
    (void)hipSetDevice(b->device);
    const size_t n = (size_t)b->nenv, nc = (size_t)b->task.ncols;
    return quiesce(b) && hip_ok(hipMemcpy(b->d_task_state, state_host, sizeof(double) * n * nc, hipMemcpyHostToDevice), "task state upload") &&
                   hip_ok(hipMemcpy(b->d_task_words, words_host, sizeof(unsigned) * n * ck::TASK_WORDS * nc, hipMemcpyHostToDevice), "task words upload") &&
                   hip_ok(hipMemcpy(b->d_task_counts, counts_host, sizeof(unsigned) * n, hipMemcpyHostToDevice), "task call counts upload") ? 0 : -1;
}
int phys_batch_debug_task_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->task_launches;
    return 0;
}

/* ------------------------------------------------ event rows ---- */
static_assert(sizeof(ck::EventCol) == sizeof(phys_event_col_t) && offsetof(ck::EventCol, root) == offsetof(phys_event_col_t, root) &&
              offsetof(ck::EventCol, gate) == offsetof(phys_event_col_t, gate) && offsetof(ck::EventCol, keep) == offsetof(phys_event_col_t, keep) &&
              offsetof(ck::EventCol, mask) == offsetof(phys_event_col_t, mask) && offsetof(ck::EventCol, init) == offsetof(phys_event_col_t, init),
              "phys_event_col_t is the column events_configure reads");
static_assert(PHYS_EV_MEASURE == ck::EV_MEASURE && PHYS_EV_LEVEL == ck::EV_LEVEL && PHYS_EV_TIMER == ck::EV_TIMER && PHYS_EV_EDGE == ck::EV_EDGE &&
              PHYS_EV_LATCH == ck::EV_LATCH && PHYS_EV_ACCUM == ck::EV_ACCUM && PHYS_EV_LOGIC == ck::EV_LOGIC && PHYS_EV_SIGNED == ck::EV_SIGNED &&
              PHYS_EV_SUMABS == ck::EV_SUMABS && PHYS_EV_SUMSQ == ck::EV_SUMSQ && PHYS_EV_MAXABS == ck::EV_MAXABS && PHYS_EV_RISING == ck::EV_RISING &&
              PHYS_EV_FALLING == ck::EV_FALLING && PHYS_EV_EITHER == ck::EV_EITHER && PHYS_EV_MAX == ck::EV_MAX && PHYS_EV_MIN == ck::EV_MIN &&
              PHYS_EV_SUM == ck::EV_SUM && PHYS_EV_ANY == ck::EV_ANY && PHYS_EV_ALL == ck::EV_ALL && PHYS_EV_NONE == ck::EV_NONE &&
              PHYS_EV_COUNT == ck::EV_COUNT && PHYS_EV_INPUT == ck::EV_INPUT && PHYS_EV_MAXCOLS == ck::EVENT_MAXCOLS && PHYS_EV_MAXCOUNT == ck::EVENT_MAXCOUNT,
              "the header's numbers are event_kernels.h's");
/* the record of a launch: what was configured, with the pointers into the batch's buffers */
static ck::EventCfg events_cfg_of(const phys_batch *b) {
    ck::EventCfg c = b->events;
    c.cols = b->d_event_cols; c.rows = b->d_event_rows.get(); c.srow = b->event_srow; c.flags = b->d_event_flags; c.state = b->d_event_state;
    c.words = b->d_event_words; c.counts = b->d_event_counts;
    return c;
}
int phys_batch_events_configure(phys_batch_t *b, const phys_event_col_t *cols, int ncols, int dtype, unsigned long long done_mask) {
    if (!b) return refuse("phys_batch_events_configure", ck::EVENT_SIZE_REFUSAL);
    int dims[PHYS_F_COUNT];
    for (int k = 0; k < PHYS_F_COUNT; ++k) dims[k] = b->d_field[k] ? b->dim[k] : 0;
    std::vector<ck::EventCol> table((size_t)ck::EVENT_MAXCOLS);
    ck::EventCfg cfg;
    if (const char *why = ck::events_configure(dims, PHYS_F_COUNT, PHYS_F_DEPTH, (const ck::EventCol *)cols, ncols, dtype, done_mask, table.data(), cfg))
        return refuse("phys_batch_events_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the table, or writing the rows, that go away) */
    if (ncols == 0) {
        b->events = {}; b->event_srow = 0;
        b->d_event_cols.reset(); b->d_event_rows.reset(); b->d_event_flags.reset(); b->d_event_state.reset(); b->d_event_words.reset(); b->d_event_counts.reset();
        return 0;
    }
    const size_t n = (size_t)b->nenv;
    DevBuf<ck::EventCol> tab;
    DevBuf<char> rows;
    DevBuf<int> flags;
    DevBuf<double> state;
    DevBuf<unsigned> words, counts;
    if (!tab.alloc((size_t)ncols, false, "event columns")) return -1;
    if (!hip_ok(hipMemcpy(tab, table.data(), sizeof(ck::EventCol) * (size_t)ncols, hipMemcpyHostToDevice), "hipMemcpy(event columns)")) return -1;
    if (!rows.alloc(n * (size_t)ncols * (size_t)dtype, true, "event rows")) return -1;
    if (!flags.alloc(n, true, "event done words")) return -1;
    if (!state.alloc(2 * n * (size_t)ncols, true, "event state")) return -1;
    if (!words.alloc(n * (size_t)ncols, true, "event words")) return -1;
    if (!counts.alloc(n, true, "event call counts")) return -1;
    b->d_event_cols = std::move(tab); b->d_event_rows = std::move(rows); b->d_event_flags = std::move(flags); b->d_event_state = std::move(state);
    b->d_event_words = std::move(words); b->d_event_counts = std::move(counts);
    b->event_srow = (long long)ncols;
    b->events = cfg;   /* (no input bound, the rows and the done words are the batch's own: the bindings are dropped) */
    return 0;
}
int phys_batch_events_bind_rows(phys_batch_t *b, void *device_ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_events_bind_rows: no batch"); return -1; }
    const long long row = b->events.ncols;
    if (const char *why = ck::check_events_bind_rows(b->events, device_ptr ? row_stride : row)) return refuse("phys_batch_events_bind_rows", why);
    (void)hipSetDevice(b->device);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    if (device_ptr) { b->d_event_rows.borrow((char *)device_ptr); b->event_srow = row_stride; }
    else if (!b->d_event_rows.owned()) {
        if (!b->d_event_rows.alloc((size_t)b->nenv * (size_t)row * (size_t)b->events.dtype, true, "event rows")) return -1;
        b->event_srow = row;
    }
    return 0;
}
int phys_batch_events_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype) {
    if (!b) { phys_set_last_error("phys_batch_events_bind_input: no batch"); return -1; }
    if (!device_ptr) { b->events.input = nullptr; b->events.input_dim = 0; b->events.input_stride = 0; b->events.input_dtype = 0; return 0; }
    if (const char *why = ck::check_events_input(b->events, dim, row_stride, dtype)) return refuse("phys_batch_events_bind_input", why);
    b->events.input = device_ptr; b->events.input_dim = dim; b->events.input_stride = (int)row_stride; b->events.input_dtype = dtype;
    return 0;
}
int phys_batch_events_bind_flags(phys_batch_t *b, void *device_ptr) {
    if (!b) { phys_set_last_error("phys_batch_events_bind_flags: no batch"); return -1; }
    if (const char *why = ck::check_events_bind_flags(b->events)) return refuse("phys_batch_events_bind_flags", why);
    (void)hipSetDevice(b->device);
    if (device_ptr) b->d_event_flags.borrow((int *)device_ptr);
    else if (!b->d_event_flags.owned() && !b->d_event_flags.alloc((size_t)b->nenv, true, "event done words")) return -1;
    return 0;
}
void *phys_batch_events_flags_ptr(phys_batch_t *b) { return b && b->events.ncols > 0 ? (void *)b->d_event_flags.get() : nullptr; }
int phys_batch_events(phys_batch_t *b, int env0, int n, const void *reset_ptr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_events: no batch"); return -1; }
    const ck::EventCfg c = events_cfg_of(b);
    ck::ObsField fields[PHYS_F_COUNT];
    obs_fields_of(b, fields);
    if (const char *why = ck::check_events_call(c, fields, PHYS_F_COUNT, b->nenv, env0, n)) return refuse("phys_batch_events", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_event_kernel, dim3((unsigned)ck::events_grid(n)), dim3(WV_WAVE), 0, s, ck::make_events_io(c, fields, b->nenv, env0, n, (const int *)reset_ptr));
    if (!hip_ok(hipGetLastError(), "cassie_event_kernel launch")) return -1;
    ++b->event_launches;
    return 0;
}
int phys_batch_events_dim(const phys_batch_t *b, int *ncols, int *dtype, unsigned long long *done_mask) {
    if (!b || b->events.ncols < 1) { phys_set_last_error("phys_batch_events_dim: not configured (phys_batch_events_configure first)"); return -1; }
    if (ncols) *ncols = b->events.ncols;
    if (dtype) *dtype = b->events.dtype;
    if (done_mask) *done_mask = b->events.done_mask;
    return 0;
}
int phys_batch_events_download(phys_batch_t *b, void *host, int env0, int n) {
    if (!b || !host || b->events.ncols < 1 || !b->d_event_rows) { phys_set_last_error("phys_batch_events_download: bad arguments, or not configured (phys_batch_events_configure first)"); return -1; }
    if (!range_ok(b, env0, n)) return refuse("phys_batch_events_download", "env range out of bounds");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (n == 0) return 0;
    const size_t el = (size_t)b->events.dtype, row = (size_t)b->events.ncols, st = (size_t)b->event_srow;
    return hip_ok(hipMemcpy2D(host, el * row, b->d_event_rows.get() + el * st * (size_t)env0, el * st, el * row, (size_t)n, hipMemcpyDeviceToHost), "event rows download") ? 0 : -1;
}
int phys_batch_events_download_flags(phys_batch_t *b, int *host) {
    if (!b || !host || b->events.ncols < 1 || !b->d_event_flags) { phys_set_last_error("phys_batch_events_download_flags: bad arguments, or not configured (phys_batch_events_configure first)"); return -1; }
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_event_flags, sizeof(int) * (size_t)b->nenv, hipMemcpyDeviceToHost), "event done words download") ? 0 : -1;
}
/* the host's shape is [nenv][2][ncols] and [nenv][ncols]; the device's [2][ncols][nenv] and [ncols][nenv] (event_kernels.h) */
int phys_batch_events_state(phys_batch_t *b, double *state_host, unsigned *words_host, unsigned *counts_host) {
    if (!b || !state_host || !words_host || !counts_host || !b->d_event_state || !b->d_event_words || !b->d_event_counts) {
        phys_set_last_error("phys_batch_events_state: bad arguments, or not configured (phys_batch_events_configure first)"); return -1;
    }
    (void)hipSetDevice(b->device);
    const size_t n = (size_t)b->nenv, nc = (size_t)b->events.ncols;
    std::vector<double> st(2 * nc * n);
    std::vector<unsigned> wd(nc * n);
    if (!(quiesce(b) && hip_ok(hipMemcpy(st.data(), b->d_event_state, sizeof(double) * st.size(), hipMemcpyDeviceToHost), "event state download") &&
          hip_ok(hipMemcpy(wd.data(), b->d_event_words, sizeof(unsigned) * wd.size(), hipMemcpyDeviceToHost), "event words download") &&
          hip_ok(hipMemcpy(counts_host, b->d_event_counts, sizeof(unsigned) * n, hipMemcpyDeviceToHost), "event call counts download"))) return -1;
    for (size_t e = 0; e < n; ++e)
        for (size_t c = 0; c < nc; ++c) {
            for (size_t s = 0; s < 2; ++s) state_host[(e * 2 + s) * nc + c] = st[(s * nc + c) * n + e];
            words_host[e * nc + c] = wd[c * n + e];
        }
    return 0;
}
int phys_batch_events_set_state(phys_batch_t *b, const double *state_host, const unsigned *words_host, const unsigned *counts_host) {
    if (!b || !state_host || !words_host || !counts_host || !b->d_event_state || !b->d_event_words || !b->d_event_counts) {
        phys_set_last_error("phys_batch_events_set_state: bad arguments, or not configured (phys_batch_events_configure first)"); return -1;
    }
    (void)hipSetDevice(b->device);
    const size_t n = (size_t)b->nenv, nc = (size_t)b->events.ncols;
    std::vector<double> st(2 * nc * n);
    std::vector<unsigned> wd(nc * n);
    for (size_t e = 0; e < n; ++e)
        for (size_t c = 0; c < nc; ++c) {
            for (size_t s = 0; s < 2; ++s) st[(s * nc + c) * n + e] = state_host[(e * 2 + s) * nc + c];
            wd[c * n + e] = words_host[e * nc + c];
        }
    return quiesce(b) && hip_ok(hipMemcpy(b->d_event_state, st.data(), sizeof(double) * st.size(), hipMemcpyHostToDevice), "event state upload") &&
                   hip_ok(hipMemcpy(b->d_event_words, wd.data(), sizeof(unsigned) * wd.size(), hipMemcpyHostToDevice), "event words upload") &&
                   hip_ok(hipMemcpy(b->d_event_counts, counts_host, sizeof(unsigned) * n, hipMemcpyHostToDevice), "event call counts upload") ? 0 : -1;
}
int phys_batch_debug_events_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->event_launches;
    return 0;
}

/* ------------------------------------------------ policy rows ---- */
static void grad_release(phys_batch *b);
static bool grad_pack_layer(phys_batch *b, int net, int layer, hipStream_t s);
static_assert(sizeof(ck::PolicyNetDef) == sizeof(phys_pol_net_t) && sizeof(ck::PolicyLayerDef) == sizeof(phys_pol_layer_t) &&
              offsetof(ck::PolicyNetDef, layer) == offsetof(phys_pol_net_t, layer) && offsetof(ck::PolicyLayerDef, act) == offsetof(phys_pol_layer_t, act),
              "phys_pol_net_t is the network policy_configure reads");
static_assert(PHYS_POL_IDENTITY == ck::POL_IDENTITY && PHYS_POL_RELU == ck::POL_RELU && PHYS_POL_ELU == ck::POL_ELU && PHYS_POL_TANH == ck::POL_TANH &&
              PHYS_POL_MAXNETS == ck::POLICY_MAXNETS && PHYS_POL_MAXLAYERS == ck::POLICY_MAXLAYERS && PHYS_POL_MAXDIM == ck::POLICY_MAXDIM &&
              PHYS_POL_MAXOUT == ck::POLICY_MAXOUT, "the header's numbers are policy_kernels.h's");
/* the record of a launch: what was configured and bound, with the pointer to the batch's packed weights */
static ck::PolicyCfg policy_cfg_of(const phys_batch *b) {
    ck::PolicyCfg c = b->policy;
    c.packed = b->d_policy_packed;
    return c;
}
int phys_batch_policy_configure(phys_batch_t *b, const phys_pol_net_t *nets, int nnets, int in_dim) {
    if (!b) return refuse("phys_batch_policy_configure", ck::POLICY_SIZE_REFUSAL);
    ck::PolicyCfg cfg;
    if (const char *why = ck::policy_configure((const ck::PolicyNetDef *)nets, nnets, in_dim, cfg)) return refuse("phys_batch_policy_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be reading the weights that go away) */
    grad_release(b);             /* (the gradient rows are laid out for the policy that goes away) */
    if (nnets == 0) { b->policy = {}; b->d_policy_packed.reset(); return 0; }
    DevBuf<float> packed;
    if (!packed.alloc((size_t)cfg.packed_floats, true, "policy weights")) return -1;
    b->d_policy_packed = std::move(packed);
    b->policy = cfg;   /* (nothing bound, no layer loaded) */
    return 0;
}
int phys_batch_policy_load(phys_batch_t *b, int net, int layer, const void *w_ptr, long long w_row_stride, const void *b_ptr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_policy_load: no batch"); return -1; }
    const ck::PolicyCfg c = policy_cfg_of(b);
    if (const char *why = ck::check_policy_load(c, net, layer, w_ptr, w_row_stride, b_ptr)) return refuse("phys_batch_policy_load", why);
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_policy_pack_kernel, dim3((unsigned)ck::policy_pack_grid(c.net[net].layer[layer])), dim3(WV_WAVE), 0, s,
                       ck::make_policy_pack_io(c, net, layer, (const float *)w_ptr, w_row_stride, (const float *)b_ptr, c.packed + c.net[net].layer[layer].w_off));
    if (!hip_ok(hipGetLastError(), "cassie_policy_pack_kernel launch")) return -1;
    b->policy.loaded |= ck::policy_layer_bit(net, layer);
    if (b->grad.max_m > 0 && !grad_pack_layer(b, net, layer, s)) return -1;   /* (gradient rows configured: the transposed packing too) */
    return 0;
}
int phys_batch_policy_load_host(phys_batch_t *b, int net, int layer, const float *w, long long w_row_stride, const float *bias) {
    if (!b) { phys_set_last_error("phys_batch_policy_load_host: no batch"); return -1; }
    const ck::PolicyCfg c = policy_cfg_of(b);
    if (const char *why = ck::check_policy_load(c, net, layer, w, w_row_stride, bias)) return refuse("phys_batch_policy_load_host", why);
    (void)hipSetDevice(b->device);
    const ck::PolicyLayer &L = c.net[net].layer[layer];
    const size_t count = (size_t)L.out16 * (size_t)L.k4 + (size_t)L.out16;   /* (a layer's biases follow its weights) */
    std::vector<float> staged(count);
    ck::PolicyPackIO io = ck::make_policy_pack_io(c, net, layer, w, w_row_stride, bias, staged.data());
    ck::policy_pack_host(io);
    if (!quiesce(b)) return -1;  /* (a policy launch in flight may be reading the layer) */
    if (!hip_ok(hipMemcpy(c.packed + L.w_off, staged.data(), sizeof(float) * count, hipMemcpyHostToDevice), "hipMemcpy(policy weights)")) return -1;
    b->policy.loaded |= ck::policy_layer_bit(net, layer);
    if (b->grad.max_m > 0 && !(grad_pack_layer(b, net, layer, launch_stream(b, nullptr)) && quiesce(b))) return -1;
    return 0;
}
int phys_batch_policy_bind_input(phys_batch_t *b, const void *device_ptr, int dim, long long row_stride, int dtype) {
    if (!b) { phys_set_last_error("phys_batch_policy_bind_input: no batch"); return -1; }
    if (!device_ptr) { b->policy.x = nullptr; b->policy.sx = 0; return 0; }
    if (const char *why = ck::check_policy_bind_input(b->policy, dim, row_stride, dtype)) return refuse("phys_batch_policy_bind_input", why);
    b->policy.x = (const float *)device_ptr; b->policy.sx = row_stride;
    return 0;
}
int phys_batch_policy_bind_norm(phys_batch_t *b, const void *mean_ptr, const void *inv_ptr, double clip) {
    if (!b) { phys_set_last_error("phys_batch_policy_bind_norm: no batch"); return -1; }
    if (!mean_ptr && !inv_ptr) { b->policy.mean = b->policy.inv = nullptr; b->policy.clip = 0; return 0; }
    if (const char *why = ck::check_policy_bind_norm(b->policy, mean_ptr, inv_ptr, clip)) return refuse("phys_batch_policy_bind_norm", why);
    b->policy.mean = (const float *)mean_ptr; b->policy.inv = (const float *)inv_ptr; b->policy.clip = clip;
    return 0;
}
int phys_batch_policy_bind_output(phys_batch_t *b, int net, void *device_ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_policy_bind_output: no batch"); return -1; }
    if (const char *why = ck::check_policy_bind_output(b->policy, net, device_ptr ? row_stride : 0x7fffffff)) return refuse("phys_batch_policy_bind_output", why);
    b->policy.out[net] = (float *)device_ptr; b->policy.sout[net] = device_ptr ? row_stride : 0;
    return 0;
}
int phys_batch_policy_bind_sample(phys_batch_t *b, const void *eps_ptr, long long eps_stride, const void *log_std_ptr, void *action_ptr,
                                  long long action_stride, void *logp_ptr) {
    if (!b) { phys_set_last_error("phys_batch_policy_bind_sample: no batch"); return -1; }
    ck::PolicyCfg &c = b->policy;
    if (!eps_ptr) { c.eps = nullptr; c.seps = 0; c.log_std = nullptr; c.action = nullptr; c.saction = 0; c.logp = nullptr; return 0; }
    if (const char *why = ck::check_policy_bind_sample(c, eps_stride, log_std_ptr, action_ptr, action_stride, logp_ptr)) return refuse("phys_batch_policy_bind_sample", why);
    c.eps = (const float *)eps_ptr; c.seps = eps_stride; c.log_std = (const float *)log_std_ptr;
    c.action = (float *)action_ptr; c.saction = action_stride; c.logp = (float *)logp_ptr;
    return 0;
}
int phys_batch_policy(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_policy: no batch"); return -1; }
    const ck::PolicyCfg c = policy_cfg_of(b);
    if (const char *why = ck::check_policy_call(c, b->nenv, env0, n)) return refuse("phys_batch_policy", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_policy_kernel, dim3((unsigned)ck::policy_grid(n, c.nnets)), dim3(WV_WAVE * ck::POLICY_WAVES), ck::policy_lds_bytes(c), s, ck::make_policy_io(c, env0, n));
    if (!hip_ok(hipGetLastError(), "cassie_policy_kernel launch")) return -1;
    ++b->policy_launches;
    return 0;
}
int phys_batch_policy_download(phys_batch_t *b, int net, float *host) {
    if (!b || !host || b->policy.nnets < 1) return refuse("phys_batch_policy_download", ck::POLICY_NOT_CONFIGURED);
    if (net < 0 || net >= b->policy.nnets || !b->policy.out[net]) return refuse("phys_batch_policy_download", "no output bound to the network (phys_batch_policy_bind_output first)");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    const size_t row = sizeof(float) * (size_t)b->policy.net[net].layer[b->policy.net[net].nlayers - 1].out;
    return hip_ok(hipMemcpy2D(host, row, b->policy.out[net], sizeof(float) * (size_t)b->policy.sout[net], row, (size_t)b->nenv, hipMemcpyDeviceToHost), "policy output download") ? 0 : -1;
}
int phys_batch_policy_download_packed(phys_batch_t *b, float *host, long long *count) {
    if (!b || b->policy.nnets < 1 || !b->d_policy_packed) return refuse("phys_batch_policy_download_packed", ck::POLICY_NOT_CONFIGURED);
    if (count) *count = b->policy.packed_floats;
    if (!host) return 0;
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_policy_packed, sizeof(float) * (size_t)b->policy.packed_floats, hipMemcpyDeviceToHost), "policy weights download") ? 0 : -1;
}
int phys_batch_debug_policy_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) *launches = b->policy_launches;
    return 0;
}

/* ------------------------------------------------ rollout rows ---- */
static_assert(sizeof(ck::RolloutSrcDef) == sizeof(phys_rollout_src_t) && offsetof(ck::RolloutSrcDef, dim) == offsetof(phys_rollout_src_t, dim),
              "phys_rollout_src_t is the source rollout_configure reads");
static_assert(PHYS_RO_DATA == ck::RO_DATA && PHYS_RO_OBS == ck::RO_OBS && PHYS_RO_ACTION == ck::RO_ACTION && PHYS_RO_LOGP == ck::RO_LOGP &&
              PHYS_RO_MU == ck::RO_MU && PHYS_RO_VALUE == ck::RO_VALUE && PHYS_RO_REWARD == ck::RO_REWARD && PHYS_RO_DONE == ck::RO_DONE &&
              PHYS_RO_REASON == ck::RO_REASON && PHYS_RO_ADV == ck::RO_ADV && PHYS_RO_RET == ck::RO_RET && PHYS_RO_ADVN == ck::RO_ADVN &&
              PHYS_RO_MAXT == ck::ROLLOUT_MAXT && PHYS_RO_MAXSRC == ck::ROLLOUT_MAXSRC && PHYS_RO_MAXDIM == ck::ROLLOUT_MAXDIM,
              "the header's numbers are rollout_kernels.h's");
/* the record of a launch: what was configured and bound, with the pointers into the batch's buffers (or the caller's in their place) */
static ck::RolloutCfg rollout_cfg_of(const phys_batch *b) {
    ck::RolloutCfg c = b->rollout;
    for (int s = 0; s < c.nsrc; ++s) c.store[s].ptr = b->d_ro_store[s].get();
    c.adv.ptr = b->d_ro_adv.get(); c.ret.ptr = b->d_ro_ret.get(); c.advn.ptr = b->d_ro_advn.get();
    if (b->d_ro_q) { c.q1 = b->d_ro_q; c.q2 = b->d_ro_q + (size_t)b->nenv; c.stats = b->d_ro_q + 2 * (size_t)b->nenv; }
    return c;
}
/* where the batch reads or writes, at this moment, the things an unbound source is resolved from */
static ck::RolloutLive rollout_live_of(const phys_batch *b) {
    ck::RolloutLive L = {};
    const ck::PolicyCfg &p = b->policy;
    if (p.nnets >= 1) {
        const int A = p.net[0].layer[p.net[0].nlayers - 1].out;
        L.obs = p.x; L.obs_dim = p.in_dim; L.obs_stride = p.sx;
        L.mu = p.out[0]; L.mu_dim = A; L.mu_stride = p.sout[0];
        if (p.nnets >= 2) { L.value = p.out[1]; L.value_stride = p.sout[1]; }
        if (p.eps) { L.action = p.action; L.action_dim = A; L.action_stride = p.saction; L.logp = p.logp; }
    }
    if (b->reward.nterms >= 1) { L.rew = b->d_reward.get(); L.rew_stride = b->reward_srew; L.rew_dtype = b->reward.dtype; }
    if (b->episodes) { L.done = b->d_ep[PHYS_EP_DONE].get(); L.reason = b->d_ep[PHYS_EP_REASON].get(); }
    return L;
}
static void rollout_release(phys_batch *b) {
    b->rollout = {};
    for (auto &d : b->d_ro_store) d.reset();
    b->d_ro_adv.reset(); b->d_ro_ret.reset(); b->d_ro_advn.reset(); b->d_ro_q.reset();
}
int phys_batch_rollout_configure(phys_batch_t *b, int T, const phys_rollout_src_t *srcs, int nsrcs, double gamma, double lambda, unsigned timeout_mask) {
    if (!b) return refuse("phys_batch_rollout_configure", ck::ROLLOUT_SIZE_REFUSAL);
    ck::RolloutCfg cfg;
    if (const char *why = ck::rollout_configure((const ck::RolloutSrcDef *)srcs, nsrcs, T, gamma, lambda, timeout_mask, cfg)) return refuse("phys_batch_rollout_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be writing the stores that go away) */
    grad_release(b);             /* (the gradient rows gather from the stores that go away) */
    if (nsrcs == 0) { rollout_release(b); return 0; }
    const size_t n = (size_t)b->nenv, steps = (size_t)T;
    DevBuf<unsigned> store[ck::ROLLOUT_MAXSRC], adv, ret;
    DevBuf<double> q;
    for (int s = 0; s < nsrcs; ++s) {
        if (!store[s].alloc(steps * n * (size_t)cfg.dim[s], true, "rollout store")) return -1;
        cfg.store[s].row = cfg.dim[s]; cfg.store[s].step = (long long)n * cfg.dim[s];
    }
    if (!adv.alloc(steps * n, true, "rollout advantages") || !ret.alloc(steps * n, true, "rollout returns") || !q.alloc(2 * n + 4, true, "rollout partials")) return -1;
    cfg.adv.row = cfg.ret.row = cfg.advn.row = 1; cfg.adv.step = cfg.ret.step = cfg.advn.step = (long long)n;
    rollout_release(b);
    for (int s = 0; s < nsrcs; ++s) b->d_ro_store[s] = std::move(store[s]);
    b->d_ro_adv = std::move(adv); b->d_ro_ret = std::move(ret); b->d_ro_q = std::move(q);
    b->rollout = cfg;   /* (nothing bound: every store is the batch's own; ADVN comes with the first normalise) */
    return 0;
}
int phys_batch_rollout_bind_source(phys_batch_t *b, int s, const void *device_ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_rollout_bind_source: no batch"); return -1; }
    if (const char *why = ck::check_rollout_bind_source(b->rollout, s, device_ptr, row_stride)) return refuse("phys_batch_rollout_bind_source", why);
    const int k = ck::rollout_source_of(b->rollout, s);
    b->rollout.src[k] = device_ptr; b->rollout.ssrc[k] = device_ptr ? row_stride : 0;
    return 0;
}
/* the buffer behind a store, ADV, RET or ADVN */
static DevBuf<unsigned> *rollout_buf_of(phys_batch *b, int s) {
    if (s == PHYS_RO_ADV) return &b->d_ro_adv;
    if (s == PHYS_RO_RET) return &b->d_ro_ret;
    if (s == PHYS_RO_ADVN) return &b->d_ro_advn;
    const int k = ck::rollout_source_of(b->rollout, s);
    return k < 0 ? nullptr : &b->d_ro_store[k];
}
int phys_batch_rollout_bind_storage(phys_batch_t *b, int s, void *device_ptr, long long step_stride, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_rollout_bind_storage: no batch"); return -1; }
    if (const char *why = ck::check_rollout_bind_storage(b->rollout, b->nenv, s, device_ptr, step_stride, row_stride)) return refuse("phys_batch_rollout_bind_storage", why);
    (void)hipSetDevice(b->device);
    int dim;
    ck::RolloutStore *st = ck::rollout_store_of(b->rollout, s, dim);
    DevBuf<unsigned> *buf = rollout_buf_of(b, s);
    /* (as phys_batch_bind: launches already queued keep the pointer they were given; hipFree waits for the device by itself) */
    if (device_ptr) { buf->borrow((unsigned *)device_ptr); st->step = step_stride; st->row = row_stride; }
    else if (!buf->owned()) {
        if (!buf->alloc((size_t)b->rollout.T * (size_t)b->nenv * (size_t)dim, true, "rollout store")) return -1;
        st->row = dim; st->step = (long long)b->nenv * dim;
    }
    return 0;
}
void *phys_batch_rollout_ptr(phys_batch_t *b, int s, long long *step_stride, long long *row_stride) {
    if (!b || b->rollout.nsrc < 1) return nullptr;
    int dim;
    const ck::RolloutStore *st = ck::rollout_store_of(b->rollout, s, dim);
    if (!st) return nullptr;
    if (step_stride) *step_stride = st->step;
    if (row_stride) *row_stride = st->row;
    return rollout_buf_of(b, s)->get();
}
int phys_batch_rollout_record(phys_batch_t *b, int t, int env0, int n, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_rollout_record: no batch"); return -1; }
    const ck::RolloutCfg c = rollout_cfg_of(b);
    const ck::RolloutLive L = rollout_live_of(b);
    if (const char *why = ck::check_rollout_record(c, L, b->nenv, t, env0, n)) return refuse("phys_batch_rollout_record", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    const ck::RolloutRecIO io = ck::make_rollout_rec_io(c, L, t, env0, n);
    hipLaunchKernelGGL(ck::cassie_rollout_record_kernel, dim3((unsigned)ck::rollout_record_grid(io)), dim3(WV_WAVE), 0, s, io);
    if (!hip_ok(hipGetLastError(), "cassie_rollout_record_kernel launch")) return -1;
    ++b->rollout_launches[0];
    return 0;
}
int phys_batch_rollout_finish(phys_batch_t *b, int env0, int n, const void *last_value_ptr, long long stride, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_rollout_finish: no batch"); return -1; }
    const ck::RolloutCfg c = rollout_cfg_of(b);
    const ck::RolloutLive L = rollout_live_of(b);
    if (const char *why = ck::check_rollout_finish(c, L, b->nenv, env0, n, last_value_ptr, stride)) return refuse("phys_batch_rollout_finish", why);
    (void)hipSetDevice(b->device);
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    hipLaunchKernelGGL(ck::cassie_rollout_finish_kernel, dim3((unsigned)ck::rollout_env_grid(n)), dim3(WV_WAVE), 0, s, ck::make_rollout_fin_io(c, L, env0, n, last_value_ptr, stride));
    if (!hip_ok(hipGetLastError(), "cassie_rollout_finish_kernel launch")) return -1;
    ++b->rollout_launches[1];
    return 0;
}
int phys_batch_rollout_normalise(phys_batch_t *b, double eps, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_rollout_normalise: no batch"); return -1; }
    (void)hipSetDevice(b->device);
    if (b->rollout.nsrc >= 1 && !b->d_ro_advn) {   /* (the first use: the batch's own ADVN, dense) */
        if (!b->d_ro_advn.alloc((size_t)b->rollout.T * (size_t)b->nenv, true, "rollout normalised advantages")) return -1;
        b->rollout.advn.row = 1; b->rollout.advn.step = b->nenv;
    }
    const ck::RolloutCfg c = rollout_cfg_of(b);
    if (const char *why = ck::check_rollout_normalise(c, b->nenv, eps)) return refuse("phys_batch_rollout_normalise", why);
    hipStream_t s = launch_stream(b, stream);
    const dim3 wave(WV_WAVE), envs((unsigned)ck::rollout_env_grid(b->nenv));
    hipLaunchKernelGGL(ck::cassie_rollout_reduce_kernel, dim3(1), wave, 0, s, ck::make_rollout_norm_io(c, b->nenv, eps, 0));
    hipLaunchKernelGGL(ck::cassie_rollout_square_kernel, envs, wave, 0, s, ck::make_rollout_norm_io(c, b->nenv, eps, 0));
    hipLaunchKernelGGL(ck::cassie_rollout_reduce_kernel, dim3(1), wave, 0, s, ck::make_rollout_norm_io(c, b->nenv, eps, 1));
    hipLaunchKernelGGL(ck::cassie_rollout_scale_kernel, dim3((unsigned)ck::rollout_scale_grid(b->nenv, c.T)), wave, 0, s, ck::make_rollout_norm_io(c, b->nenv, eps, 1));
    if (!hip_ok(hipGetLastError(), "rollout normalise launches")) return -1;
    b->rollout_launches[2] += 4;
    return 0;
}
int phys_batch_rollout_stats(phys_batch_t *b, double *mean_std_inv) {
    if (!b || !mean_std_inv || b->rollout.nsrc < 1 || !b->d_ro_q) return refuse("phys_batch_rollout_stats", ck::ROLLOUT_NOT_CONFIGURED);
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(mean_std_inv, b->d_ro_q + 2 * (size_t)b->nenv, sizeof(double) * 3, hipMemcpyDeviceToHost), "rollout stats download") ? 0 : -1;
}
int phys_batch_rollout_download(phys_batch_t *b, int s, void *host) {
    if (!b || !host || b->rollout.nsrc < 1) return refuse("phys_batch_rollout_download", ck::ROLLOUT_NOT_CONFIGURED);
    int dim;
    const ck::RolloutStore *st = ck::rollout_store_of(b->rollout, s, dim);
    const unsigned *base = st ? rollout_buf_of(b, s)->get() : nullptr;
    if (!base) return refuse("phys_batch_rollout_download", ck::ROLLOUT_NO_SUCH);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    const size_t row = sizeof(unsigned) * (size_t)dim, n = (size_t)b->nenv;
    for (int t = 0; t < b->rollout.T; ++t)
        if (!hip_ok(hipMemcpy2D((char *)host + (size_t)t * n * row, row, base + (size_t)t * (size_t)st->step, sizeof(unsigned) * (size_t)st->row, row, n, hipMemcpyDeviceToHost), "rollout download")) return -1;
    return 0;
}
int phys_batch_rollout_dim(const phys_batch_t *b, int *T, int *nsrcs, int *dims) {
    if (!b || b->rollout.nsrc < 1) return refuse("phys_batch_rollout_dim", ck::ROLLOUT_NOT_CONFIGURED);
    if (T) *T = b->rollout.T;
    if (nsrcs) *nsrcs = b->rollout.nsrc;
    if (dims) for (int s = 0; s < b->rollout.nsrc; ++s) dims[s] = b->rollout.dim[s];
    return 0;
}
int phys_batch_debug_rollout_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) for (int k = 0; k < 3; ++k) launches[k] = b->rollout_launches[k];
    return 0;
}

/* ------------------------------------------------ gradient rows ---- */
static_assert(PHYS_GRAD_DW == ck::GRAD_DW && PHYS_GRAD_DB == ck::GRAD_DB && PHYS_GRAD_DLS == ck::GRAD_DLS && PHYS_GRAD_ACT == ck::GRAD_ACT &&
              PHYS_GRAD_DELTA == ck::GRAD_DELTA && PHYS_GRAD_PARTIAL == ck::GRAD_PARTIAL && PHYS_GRAD_PACKT == ck::GRAD_PACKT &&
              PHYS_GRAD_MINCHUNK == ck::GRAD_MINCHUNK && PHYS_GRAD_MAXCHUNK == ck::GRAD_MAXCHUNK && PHYS_GRAD_NSTATS == ck::GRAD_NSTATS,
              "the header's numbers are grad_kernels.h's");
/* the record of a launch: what was configured and bound, with the pointers into the batch's buffers */
static ck::GradCfg grad_cfg_of(const phys_batch *b) {
    ck::GradCfg c = b->grad;
    c.act = b->d_grad_act; c.delta = b->d_grad_delta; c.packt = b->d_grad_packt; c.own = b->d_grad_own;
    c.part = b->d_grad_part; c.pos = b->d_grad_pos;
    c.stats = b->d_grad_pos ? b->d_grad_pos + (size_t)c.pos_doubles : nullptr;
    return c;
}
static void opt_release(phys_batch *b) {
    b->opt = {};
    b->d_opt_mom.reset(); b->d_opt_part.reset();
}
static void grad_release(phys_batch *b) {
    opt_release(b);              /* (the optimiser rows are laid out for the gradient rows that go away) */
    b->grad = {};
    b->grad_last_m = 0;
    b->d_grad_act.reset(); b->d_grad_delta.reset(); b->d_grad_packt.reset(); b->d_grad_own.reset(); b->d_grad_part.reset(); b->d_grad_pos.reset();
}
/* the transposed packing of a loaded layer from the policy's packed weights, behind whatever wrote them on s */
static bool grad_pack_layer(phys_batch *b, int net, int layer, hipStream_t s) {
    const ck::GradPackIO io = ck::make_grad_pack_io(grad_cfg_of(b), policy_cfg_of(b), net, layer);
    hipLaunchKernelGGL(ck::cassie_grad_pack_kernel, dim3((unsigned)ck::grad_pack_grid(io)), dim3(WV_WAVE), 0, s, io);
    if (!hip_ok(hipGetLastError(), "cassie_grad_pack_kernel launch")) return false;
    ++b->grad_launches[5];
    return true;
}
int phys_batch_grad_configure(phys_batch_t *b, int max_m, int chunk, double clip_eps, double c_v, double c_ent) {
    if (!b) return refuse("phys_batch_grad_configure", ck::GRAD_NEEDS);
    ck::GradCfg cfg;
    const long long total = b->rollout.nsrc >= 1 ? (long long)b->rollout.T * b->nenv : 0;
    if (const char *why = ck::grad_configure(b->policy, total, max_m, chunk, clip_eps, c_v, c_ent, cfg)) return refuse("phys_batch_grad_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be using the stores that go away) */
    if (max_m == 0) { grad_release(b); return 0; }
    DevBuf<float> act, delta, packt, own;
    DevBuf<double> part, pos;
    if (!act.alloc((size_t)cfg.act_floats, true, "gradient activations") || !delta.alloc((size_t)cfg.delta_floats, true, "gradient deltas") ||
        !packt.alloc((size_t)cfg.packt_floats, true, "transposed weights") || !own.alloc((size_t)cfg.own_floats, true, "gradients") ||
        !part.alloc((size_t)cfg.part_doubles, true, "gradient partials") || !pos.alloc((size_t)cfg.pos_doubles + ck::GRAD_NSTATS, true, "gradient head values")) return -1;
    grad_release(b);
    b->d_grad_act = std::move(act); b->d_grad_delta = std::move(delta); b->d_grad_packt = std::move(packt); b->d_grad_own = std::move(own);
    b->d_grad_part = std::move(part); b->d_grad_pos = std::move(pos);
    b->grad = cfg;   /* (nothing bound: every gradient is the batch's own) */
    /* the layers loaded before now: their transposed packing from the packed weights */
    hipStream_t s = launch_stream(b, nullptr);
    for (int a = 0; a < b->policy.nnets; ++a)
        for (int l = 0; l < b->policy.net[a].nlayers; ++l)
            if ((b->policy.loaded & ck::policy_layer_bit(a, l)) && !grad_pack_layer(b, a, l, s)) return -1;
    return quiesce(b) ? 0 : -1;
}
int phys_batch_grad_bind(phys_batch_t *b, int net, int layer, void *dw_ptr, long long dw_row_stride, void *db_ptr) {
    if (!b) { phys_set_last_error("phys_batch_grad_bind: no batch"); return -1; }
    if (const char *why = ck::check_grad_bind(b->grad, b->policy, net, layer, dw_ptr, dw_row_stride, db_ptr)) return refuse("phys_batch_grad_bind", why);
    const int s = ck::grad_slot(b->grad, net, layer);
    b->grad.dw[s] = (float *)dw_ptr; b->grad.sdw[s] = dw_ptr ? dw_row_stride : 0; b->grad.db[s] = (float *)db_ptr;
    return 0;
}
int phys_batch_grad_bind_log_std(phys_batch_t *b, void *ptr) {
    if (!b) { phys_set_last_error("phys_batch_grad_bind_log_std: no batch"); return -1; }
    if (b->grad.max_m < 1) return refuse("phys_batch_grad_bind_log_std", ck::GRAD_NOT_CONFIGURED);
    b->grad.dls = (float *)ptr;
    return 0;
}
int phys_batch_grad(phys_batch_t *b, const void *idx_ptr, int m, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_grad: no batch"); return -1; }
    const ck::GradCfg c = grad_cfg_of(b);
    const ck::PolicyCfg p = policy_cfg_of(b);
    if (c.max_m < 1) return refuse("phys_batch_grad", ck::GRAD_NOT_CONFIGURED);
    ck::GradSources S;
    if (const char *why = ck::grad_sources(rollout_cfg_of(b), p, b->nenv, S)) return refuse("phys_batch_grad", why);
    if (const char *why = ck::check_grad_call(c, p, idx_ptr, m)) return refuse("phys_batch_grad", why);
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    const ck::GradIO io = ck::make_grad_io(c, p, S, b->nenv, (const int *)idx_ptr, m);
    const dim3 wave(WV_WAVE), group(WV_WAVE * ck::POLICY_WAVES), tiles((unsigned)ck::grad_tile_grid(io));
    const unsigned lds = ck::grad_lds_bytes(p);
    const unsigned mask = b->grad_mask;
    if (mask & 1u) { hipLaunchKernelGGL(ck::cassie_grad_forward_kernel, tiles, group, lds, s, io); ++b->grad_launches[0]; }
    if ((mask & 2u) && ck::grad_has_backward(p)) { hipLaunchKernelGGL(ck::cassie_grad_backward_kernel, tiles, group, lds, s, io); ++b->grad_launches[1]; }
    if (mask & 4u) { hipLaunchKernelGGL(ck::cassie_grad_partial_kernel, dim3((unsigned)ck::grad_partial_grid(io)), wave, 0, s, io); ++b->grad_launches[2]; }
    if (mask & 8u) { hipLaunchKernelGGL(ck::cassie_grad_reduce_kernel, dim3((unsigned)ck::grad_reduce_grid(io)), wave, 0, s, io); ++b->grad_launches[3]; }
    if (mask & 16u) { hipLaunchKernelGGL(ck::cassie_grad_stats_kernel, dim3((unsigned)ck::grad_stats_grid(io)), wave, 0, s, io); ++b->grad_launches[4]; }
    if (!hip_ok(hipGetLastError(), "gradient launches")) return -1;
    b->grad_last_m = m;
    return 0;
}
int phys_batch_grad_stats(phys_batch_t *b, double *stats) {
    if (!b || !stats || b->grad.max_m < 1 || !b->d_grad_pos) return refuse("phys_batch_grad_stats", ck::GRAD_NOT_CONFIGURED);
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(stats, b->d_grad_pos + (size_t)b->grad.pos_doubles, sizeof(double) * ck::GRAD_NSTATS, hipMemcpyDeviceToHost), "gradient stats download") ? 0 : -1;
}
long long phys_batch_grad_count(const phys_batch_t *b, int what, int net, int layer) {
    if (!b || b->grad.max_m < 1) return -1;
    const ck::GradCfg &c = b->grad;
    if (what == ck::GRAD_DLS) return c.A;
    if (net < 0 || net >= b->policy.nnets) return -1;
    const ck::PolicyNet &N = b->policy.net[net];
    const long long m = b->grad_last_m;
    if (what == ck::GRAD_ACT) return layer >= 0 && layer <= N.nlayers ? m * (layer == 0 ? b->policy.in_dim : N.layer[layer - 1].out) : -1;
    if (layer < 0 || layer >= N.nlayers) return -1;
    const ck::PolicyLayer &L = N.layer[layer];
    switch (what) {
    case ck::GRAD_DW: return (long long)L.out * L.in;
    case ck::GRAD_DB: return L.out;
    case ck::GRAD_DELTA: return m * L.out;
    case ck::GRAD_PARTIAL: return (m + c.chunk - 1) / c.chunk * L.out * (L.in + 1);
    case ck::GRAD_PACKT: return (long long)c.g[net].hw[layer] * ((L.out + 3) & ~3);
    default: return -1;
    }
}
int phys_batch_grad_download(phys_batch_t *b, int what, int net, int layer, void *host) {
    if (!b || !host || b->grad.max_m < 1) return refuse("phys_batch_grad_download", ck::GRAD_NOT_CONFIGURED);
    if (phys_batch_grad_count(b, what, net, layer) < 0) return refuse("phys_batch_grad_download", "no such network, layer or kind (PHYS_GRAD_*)");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    const ck::GradCfg c = grad_cfg_of(b);
    const size_t m = (size_t)b->grad_last_m, f = sizeof(float);
    if (what == ck::GRAD_DLS) return hip_ok(hipMemcpy(host, c.dls ? c.dls : c.own + c.own_ls, f * (size_t)c.A, hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    const ck::GradNet &G = c.g[net];
    if (what == ck::GRAD_ACT) {
        const size_t w = (size_t)(layer == 0 ? b->policy.in_dim : b->policy.net[net].layer[layer - 1].out);
        if (m == 0) return 0;
        return hip_ok(hipMemcpy2D(host, f * w, c.act + G.h_off[layer], f * (size_t)G.hw[layer], f * w, m, hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    }
    const ck::PolicyLayer &L = b->policy.net[net].layer[layer];
    const int s = ck::grad_slot(c, net, layer);
    const size_t out = (size_t)L.out, in = (size_t)L.in;
    switch (what) {
    case ck::GRAD_DW:
        return hip_ok(hipMemcpy2D(host, f * in, c.dw[s] ? c.dw[s] : c.own + c.own_w[s], f * (size_t)(c.dw[s] ? c.sdw[s] : L.in), f * in, out, hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    case ck::GRAD_DB: return hip_ok(hipMemcpy(host, c.db[s] ? c.db[s] : c.own + c.own_b[s], f * out, hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    case ck::GRAD_DELTA:
        if (m == 0) return 0;
        return hip_ok(hipMemcpy2D(host, f * out, c.delta + G.d_off[layer], f * (size_t)L.out16, f * out, m, hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    case ck::GRAD_PARTIAL:
        if (m == 0) return 0;
        return hip_ok(hipMemcpy(host, c.part + G.p_off[layer], sizeof(double) * (size_t)phys_batch_grad_count(b, what, net, layer), hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    default:
        return hip_ok(hipMemcpy(host, c.packt + G.t_off[layer], f * (size_t)phys_batch_grad_count(b, what, net, layer), hipMemcpyDeviceToHost), "gradient download") ? 0 : -1;
    }
}
int phys_batch_debug_grad_mask(phys_batch_t *b, unsigned mask) {
    if (!b) return -1;
    b->grad_mask = mask & 31u;
    return 0;
}
int phys_batch_debug_grad_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) for (int k = 0; k < 6; ++k) launches[k] = b->grad_launches[k];
    return 0;
}

/* ------------------------------------------------ optimiser rows ---- */
static_assert(PHYS_OPT_M_W == ck::OPT_M_W && PHYS_OPT_M_B == ck::OPT_M_B && PHYS_OPT_V_W == ck::OPT_V_W && PHYS_OPT_V_B == ck::OPT_V_B &&
              PHYS_OPT_M_LS == ck::OPT_M_LS && PHYS_OPT_V_LS == ck::OPT_V_LS && PHYS_OPT_SCALARS == ck::OPT_SCALARS &&
              PHYS_OPT_PARTIALS == ck::OPT_PARTIALS && PHYS_OPT_SEG == ck::OPT_SEG && PHYS_OPT_NSTATS == ck::OPT_NSTATS,
              "the header's numbers are opt_kernels.h's");
/* the record of a launch: what was configured and bound, with the pointers into the batch's buffers */
static ck::OptCfg opt_cfg_of(const phys_batch *b) {
    ck::OptCfg c = b->opt;
    c.mom = b->d_opt_mom; c.part = b->d_opt_part;
    c.sc = b->d_opt_part ? b->d_opt_part + (size_t)c.nseg : nullptr;
    return c;
}
int phys_batch_opt_configure(phys_batch_t *b, double beta1, double beta2, double eps, double max_norm) {
    if (!b) return refuse("phys_batch_opt_configure", ck::OPT_NEEDS);
    ck::OptCfg cfg;
    if (const char *why = ck::opt_configure(b->grad, b->policy, beta1, beta2, eps, max_norm, cfg)) return refuse("phys_batch_opt_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be using the moments that go away) */
    if (!cfg.on) { opt_release(b); return 0; }
    DevBuf<float> mom;
    DevBuf<double> part;
    if (!mom.alloc(2 * (size_t)cfg.Q, true, "optimiser moments") || !part.alloc((size_t)cfg.nseg + ck::OPT_SC_COUNT, true, "optimiser partials")) return -1;
    double sc[ck::OPT_SC_COUNT];
    ck::opt_initial_scalars(sc);
    if (!hip_ok(hipMemcpy(part.get() + (size_t)cfg.nseg, sc, sizeof sc, hipMemcpyHostToDevice), "optimiser scalars upload")) return -1;
    opt_release(b);
    b->d_opt_mom = std::move(mom); b->d_opt_part = std::move(part);
    b->opt = cfg;   /* (nothing bound) */
    return 0;
}
int phys_batch_opt_bind_param(phys_batch_t *b, int net, int layer, void *w_ptr, long long w_row_stride, void *b_ptr) {
    if (!b) { phys_set_last_error("phys_batch_opt_bind_param: no batch"); return -1; }
    if (const char *why = ck::check_opt_bind_param(b->opt, b->policy, net, layer, w_ptr, w_row_stride, b_ptr)) return refuse("phys_batch_opt_bind_param", why);
    const int s = ck::grad_slot(b->grad, net, layer);
    b->opt.w[s] = (float *)w_ptr; b->opt.sw[s] = w_row_stride; b->opt.b[s] = (float *)b_ptr;
    return 0;
}
int phys_batch_opt_bind_log_std(phys_batch_t *b, void *ptr) {
    if (!b) { phys_set_last_error("phys_batch_opt_bind_log_std: no batch"); return -1; }
    if (const char *why = ck::check_opt_bind_log_std(b->opt, b->policy, ptr)) return refuse("phys_batch_opt_bind_log_std", why);
    b->opt.ls = (float *)ptr;
    return 0;
}
int phys_batch_opt_step(phys_batch_t *b, double lr, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_opt_step: no batch"); return -1; }
    const ck::OptCfg c = opt_cfg_of(b);
    const ck::GradCfg g = grad_cfg_of(b);
    const ck::PolicyCfg p = policy_cfg_of(b);
    if (const char *why = ck::check_opt_step(c, g, p, lr, b->grad_last_m > 0)) return refuse("phys_batch_opt_step", why);
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    const ck::OptIO io = ck::make_opt_io(c, g, p, lr);
    const dim3 wave(WV_WAVE);
    const unsigned mask = b->opt_mask;
    if (mask & 1u) { hipLaunchKernelGGL(ck::cassie_opt_sq_kernel, dim3((unsigned)ck::opt_sq_grid(io)), wave, 0, s, io); ++b->opt_launches[0]; }
    if (mask & 2u) { hipLaunchKernelGGL(ck::cassie_opt_scalars_kernel, dim3(1), wave, 0, s, io); ++b->opt_launches[1]; }
    if (mask & 4u) { hipLaunchKernelGGL(ck::cassie_opt_step_kernel, dim3((unsigned)ck::opt_step_grid(io)), wave, 0, s, io); ++b->opt_launches[2]; }
    return hip_ok(hipGetLastError(), "optimiser launches") ? 0 : -1;
}
int phys_batch_opt_stats(phys_batch_t *b, double *stats) {
    if (!b || !stats || !b->opt.on || !b->d_opt_part) return refuse("phys_batch_opt_stats", ck::OPT_NOT_CONFIGURED);
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(stats, b->d_opt_part + (size_t)b->opt.nseg, sizeof(double) * ck::OPT_NSTATS, hipMemcpyDeviceToHost), "optimiser stats download") ? 0 : -1;
}
long long phys_batch_opt_count(const phys_batch_t *b, int what, int net, int layer) {
    if (!b) return -1;
    ck::OptRegion R;
    return ck::opt_region(b->opt, b->grad, b->policy, what, net, layer, R) ? R.rows * R.width : -1;
}
/* a download (up false) or an upload of a region: dense host rows against the region's pitch */
static int opt_transfer(phys_batch_t *b, const char *fn, int what, int net, int layer, void *host, bool up) {
    if (!b || !host || !b->opt.on) return refuse(fn, ck::OPT_NOT_CONFIGURED);
    ck::OptRegion R;
    if (!ck::opt_region(opt_cfg_of(b), b->grad, b->policy, what, net, layer, R) || !R.ptr || (up && what == ck::OPT_PARTIALS))
        return refuse(fn, "no such network, layer or kind (PHYS_OPT_*)");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    const size_t e = R.doubles ? sizeof(double) : sizeof(float);
    const hipError_t rc = up ? hipMemcpy2D(R.ptr, e * (size_t)R.pitch, host, e * (size_t)R.width, e * (size_t)R.width, (size_t)R.rows, hipMemcpyHostToDevice)
                             : hipMemcpy2D(host, e * (size_t)R.width, R.ptr, e * (size_t)R.pitch, e * (size_t)R.width, (size_t)R.rows, hipMemcpyDeviceToHost);
    return hip_ok(rc, up ? "optimiser upload" : "optimiser download") ? 0 : -1;
}
int phys_batch_opt_download(phys_batch_t *b, int what, int net, int layer, void *host) {
    return opt_transfer(b, "phys_batch_opt_download", what, net, layer, host, false);
}
int phys_batch_opt_upload(phys_batch_t *b, int what, int net, int layer, const void *host) {
    return opt_transfer(b, "phys_batch_opt_upload", what, net, layer, (void *)host, true);
}
int phys_batch_debug_opt_mask(phys_batch_t *b, unsigned mask) {
    if (!b) return -1;
    b->opt_mask = mask & 7u;
    return 0;
}
int phys_batch_debug_opt_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) for (int k = 0; k < 3; ++k) launches[k] = b->opt_launches[k];
    return 0;
}

/* ------------------------------------------------ normaliser rows ---- */
static_assert(PHYS_NORM_N == ck::NORM_N && PHYS_NORM_MEAN == ck::NORM_MEAN && PHYS_NORM_M2 == ck::NORM_M2 && PHYS_NORM_SKIPPED == ck::NORM_SKIPPED &&
              PHYS_NORM_EXCLUDED == ck::NORM_EXCLUDED && PHYS_NORM_MB == ck::NORM_MB && PHYS_NORM_COUNTS == ck::NORM_COUNTS &&
              PHYS_NORM_PARTIALS == ck::NORM_PARTIALS && PHYS_NORM_MINBLOCK == ck::NORM_MINBLOCK && PHYS_NORM_MAXBLOCK == ck::NORM_MAXBLOCK &&
              PHYS_NORM_MAXROWS == ck::NORM_MAXROWS && PHYS_NORM_NSTATS == ck::NORM_NSTATS && PHYS_POL_MAXDIM == ck::NORM_MAXDIM,
              "the header's numbers are norm_kernels.h's");
/* the record of a launch: what was configured and bound, with the pointers into the batch's buffers */
static ck::NormCfg norm_cfg_of(const phys_batch *b) {
    ck::NormCfg c = b->norm;
    c.state = b->d_norm_state; c.part = b->d_norm_part; c.cnt = b->d_norm_cnt;
    return c;
}
static void norm_release(phys_batch *b) {
    b->norm = {};
    b->d_norm_state.reset(); b->d_norm_part.reset(); b->d_norm_cnt.reset();
}
int phys_batch_norm_configure(phys_batch_t *b, int dim, int block, long long max_rows, double eps) {
    if (!b) { phys_set_last_error("phys_batch_norm_configure: no batch"); return -1; }
    ck::NormCfg cfg;
    if (const char *why = ck::norm_configure(dim, block, max_rows, eps, cfg)) return refuse("phys_batch_norm_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be using the state that goes away) */
    if (!cfg.on) { norm_release(b); return 0; }
    DevBuf<double> state, part;
    DevBuf<int> cnt;
    const size_t words = (size_t)cfg.max_blocks * (size_t)cfg.D;
    if (!state.alloc((size_t)ck::NORM_STATE_ROWS * (size_t)cfg.D, true, "normaliser state") || !part.alloc(2 * words, true, "normaliser partials") ||
        !cnt.alloc(words, true, "normaliser counts")) return -1;
    norm_release(b);
    b->d_norm_state = std::move(state); b->d_norm_part = std::move(part); b->d_norm_cnt = std::move(cnt);
    b->norm = cfg;   /* (nothing bound: n, mean and m2 +0.0) */
    return 0;
}
int phys_batch_norm_bind_source(phys_batch_t *b, const void *ptr, int steps, int rows, long long step_stride, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_norm_bind_source: no batch"); return -1; }
    if (const char *why = ck::check_norm_bind_source(b->norm, ptr, steps, rows, step_stride, row_stride)) return refuse("phys_batch_norm_bind_source", why);
    ck::NormCfg &c = b->norm;
    c.src = (const float *)ptr;
    c.steps = ptr ? steps : 0; c.rows = ptr ? rows : 0; c.step_stride = ptr ? step_stride : 0; c.row_stride = ptr ? row_stride : 0;
    return 0;
}
int phys_batch_norm_bind_output(phys_batch_t *b, void *mean_ptr, void *inv_ptr) {
    if (!b) { phys_set_last_error("phys_batch_norm_bind_output: no batch"); return -1; }
    if (const char *why = ck::check_norm_bind_output(b->norm, mean_ptr, inv_ptr)) return refuse("phys_batch_norm_bind_output", why);
    b->norm.out_mean = (float *)mean_ptr; b->norm.out_inv = (float *)inv_ptr;
    return 0;
}
int phys_batch_norm_update(phys_batch_t *b, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_norm_update: no batch"); return -1; }
    const ck::NormCfg c = norm_cfg_of(b);
    ck::NormSource S;
    ck::NormOutput O;
    if (const char *why = ck::check_norm_update(c, rollout_cfg_of(b), b->policy, b->nenv, S, O)) return refuse("phys_batch_norm_update", why);
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    const ck::NormIO io = ck::make_norm_io(c, S, O);
    const dim3 wave(WV_WAVE), pass((unsigned)ck::norm_pass_grid(io)), cols((unsigned)ck::norm_column_grid(io));
    const unsigned mask = b->norm_mask;
    if (mask & 1u) { hipLaunchKernelGGL(ck::cassie_norm_sum_kernel, pass, wave, 0, s, io); ++b->norm_launches[0]; }
    if (mask & 2u) { hipLaunchKernelGGL(ck::cassie_norm_mean_kernel, cols, wave, 0, s, io); ++b->norm_launches[1]; }
    if (mask & 4u) { hipLaunchKernelGGL(ck::cassie_norm_sq_kernel, pass, wave, 0, s, io); ++b->norm_launches[2]; }
    if (mask & 8u) { hipLaunchKernelGGL(ck::cassie_norm_merge_kernel, cols, wave, 0, s, io); ++b->norm_launches[3]; }
    b->norm.last_R = io.R; b->norm.last_blocks = io.blocks; ++b->norm.calls;
    return hip_ok(hipGetLastError(), "normaliser launches") ? 0 : -1;
}
int phys_batch_norm_write(phys_batch_t *b, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_norm_write: no batch"); return -1; }
    const ck::NormCfg c = norm_cfg_of(b);
    ck::NormOutput O;
    if (const char *why = ck::check_norm_write(c, b->policy, O)) return refuse("phys_batch_norm_write", why);
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    const ck::NormIO io = ck::make_norm_io(c, ck::NormSource{}, O);
    hipLaunchKernelGGL(ck::cassie_norm_write_kernel, dim3((unsigned)ck::norm_column_grid(io)), dim3(WV_WAVE), 0, s, io);
    ++b->norm_launches[4];
    return hip_ok(hipGetLastError(), "cassie_norm_write_kernel launch") ? 0 : -1;
}
int phys_batch_norm_stats(phys_batch_t *b, double *stats) {
    if (!b || !stats || !b->norm.on || !b->d_norm_state) return refuse("phys_batch_norm_stats", ck::NORM_NOT_CONFIGURED);
    (void)hipSetDevice(b->device);
    const size_t D = (size_t)b->norm.D;
    std::vector<double> n(D), counts(D);
    if (!quiesce(b) || !hip_ok(hipMemcpy(n.data(), b->d_norm_state + ck::NORM_N * D, sizeof(double) * D, hipMemcpyDeviceToHost), "normaliser stats download") ||
        !hip_ok(hipMemcpy(counts.data(), b->d_norm_state + ck::NORM_COUNTS * D, sizeof(double) * D, hipMemcpyDeviceToHost), "normaliser stats download")) return -1;
    ck::norm_stats_host(b->norm, n.data(), counts.data(), stats);
    return 0;
}
long long phys_batch_norm_count(const phys_batch_t *b, int what) {
    if (!b) return -1;
    ck::NormRegion R;
    return ck::norm_region(b->norm, what, false, R) ? R.rows * R.width : -1;
}
/* a download (up false) or an upload of a region: dense host doubles against the region's pitch */
static int norm_transfer(phys_batch_t *b, const char *fn, int what, void *host, bool up) {
    if (!b || !host || !b->norm.on) return refuse(fn, ck::NORM_NOT_CONFIGURED);
    ck::NormRegion R;
    if (!ck::norm_region(norm_cfg_of(b), what, up, R) || !R.ptr) return refuse(fn, "no such kind (PHYS_NORM_*; an upload takes N, MEAN, M2, SKIPPED and EXCLUDED)");
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (R.width == 0) return 0;
    const size_t e = sizeof(double);
    const hipError_t rc = up ? hipMemcpy2D(R.ptr, e * (size_t)R.pitch, host, e * (size_t)R.width, e * (size_t)R.width, (size_t)R.rows, hipMemcpyHostToDevice)
                             : hipMemcpy2D(host, e * (size_t)R.width, R.ptr, e * (size_t)R.pitch, e * (size_t)R.width, (size_t)R.rows, hipMemcpyDeviceToHost);
    return hip_ok(rc, up ? "normaliser upload" : "normaliser download") ? 0 : -1;
}
int phys_batch_norm_download(phys_batch_t *b, int what, void *host) { return norm_transfer(b, "phys_batch_norm_download", what, host, false); }
int phys_batch_norm_upload(phys_batch_t *b, int what, const void *host) { return norm_transfer(b, "phys_batch_norm_upload", what, (void *)host, true); }
int phys_batch_debug_norm_mask(phys_batch_t *b, unsigned mask) {
    if (!b) return -1;
    b->norm_mask = mask & 15u;
    return 0;
}
int phys_batch_debug_norm_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) for (int k = 0; k < 5; ++k) launches[k] = b->norm_launches[k];
    return 0;
}

/* ------------------------------------------------ draw rows ---- */
static_assert(PHYS_DRAW_MAXA == ck::DRAW_MAXA && PHYS_DRAW_MAXPERM == ck::DRAW_MAXPERM, "the header's numbers are draw_kernels.h's");
/* the record of a launch: what was configured and bound, with the pointers into the batch's buffers */
static ck::DrawCfg draw_cfg_of(const phys_batch *b) {
    ck::DrawCfg c = b->draw;
    c.counts = b->d_draw_counts; c.perm = b->d_draw_perm;
    return c;
}
static void draw_release(phys_batch *b) {
    b->draw = {};
    b->d_draw_counts.reset(); b->d_draw_perm.reset();
}
int phys_batch_draw_configure(phys_batch_t *b, int A, long long perm_n, unsigned long long seed, unsigned env_base) {
    if (!b) { phys_set_last_error("phys_batch_draw_configure: no batch"); return -1; }
    ck::DrawCfg cfg;
    if (const char *why = ck::draw_configure(A, perm_n, seed, env_base, cfg)) return refuse("phys_batch_draw_configure", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;  /* (launches in flight may be using the buffers that go away) */
    if (!cfg.on) { draw_release(b); return 0; }
    DevBuf<unsigned> counts;
    DevBuf<int> perm;
    if (!counts.alloc((size_t)b->nenv, true, "draw call counts") || (cfg.perm_n > 0 && !perm.alloc((size_t)cfg.perm_n, true, "draw permutation"))) return -1;
    draw_release(b);
    b->d_draw_counts = std::move(counts); b->d_draw_perm = std::move(perm);
    b->draw = cfg;   /* (nothing bound: the counts 0) */
    return 0;
}
int phys_batch_draw_bind(phys_batch_t *b, void *ptr, long long row_stride) {
    if (!b) { phys_set_last_error("phys_batch_draw_bind: no batch"); return -1; }
    if (const char *why = ck::check_draw_bind(b->draw, ptr, row_stride)) return refuse("phys_batch_draw_bind", why);
    b->draw.dst = (float *)ptr; b->draw.sdst = ptr ? row_stride : 0;
    return 0;
}
int phys_batch_draw_bind_perm(phys_batch_t *b, void *ptr) {
    if (!b) { phys_set_last_error("phys_batch_draw_bind_perm: no batch"); return -1; }
    if (const char *why = ck::check_draw_bind_perm(b->draw, ptr)) return refuse("phys_batch_draw_bind_perm", why);
    b->draw.perm_dst = (int *)ptr;
    return 0;
}
int phys_batch_draw(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_draw: no batch"); return -1; }
    const ck::DrawCfg c = draw_cfg_of(b);
    ck::DrawDst D;
    if (const char *why = ck::check_draw(c, b->policy, b->nenv, env0, n, D)) return refuse("phys_batch_draw", why);
    if (n == 0) return 0;
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    const ck::DrawIO io = ck::make_draw_io(c, D, env0, n);
    hipLaunchKernelGGL(ck::cassie_draw_kernel, dim3((unsigned)ck::draw_grid(io)), dim3(WV_WAVE), 0, s, io);
    ++b->draw_launches[0];
    return hip_ok(hipGetLastError(), "cassie_draw_kernel launch") ? 0 : -1;
}
int phys_batch_draw_perm(phys_batch_t *b, unsigned epoch, void *stream) {
    if (!b) { phys_set_last_error("phys_batch_draw_perm: no batch"); return -1; }
    const ck::DrawCfg c = draw_cfg_of(b);
    if (const char *why = ck::check_draw_perm(c)) return refuse("phys_batch_draw_perm", why);
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    const ck::DrawPermIO io = ck::make_draw_perm_io(c, epoch);
    hipLaunchKernelGGL(ck::cassie_draw_perm_kernel, dim3((unsigned)ck::draw_perm_grid(io)), dim3(WV_WAVE), 0, s, io);
    ++b->draw_launches[1];
    return hip_ok(hipGetLastError(), "cassie_draw_perm_kernel launch") ? 0 : -1;
}
void *phys_batch_draw_perm_ptr(const phys_batch_t *b) {
    if (!b || !b->draw.on || b->draw.perm_n < 1) return nullptr;
    return b->draw.perm_dst ? (void *)b->draw.perm_dst : (void *)b->d_draw_perm.get();
}
int phys_batch_draw_dim(const phys_batch_t *b, int *A, long long *perm_n) {
    if (!b || !b->draw.on) return refuse("phys_batch_draw_dim", ck::DRAW_NOT_CONFIGURED);
    if (A) *A = b->draw.A;
    if (perm_n) *perm_n = b->draw.perm_n;
    return 0;
}
int phys_batch_draw_rows(phys_batch_t *b, float *host) {
    if (!b || !host) return refuse("phys_batch_draw_rows", ck::DRAW_NOT_CONFIGURED);
    ck::DrawDst D;
    if (const char *why = ck::check_draw(draw_cfg_of(b), b->policy, b->nenv, 0, b->nenv, D)) return refuse("phys_batch_draw_rows", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    const size_t e = sizeof(float), A = (size_t)b->draw.A;
    return hip_ok(hipMemcpy2D(host, e * A, D.ptr, e * (size_t)D.stride, e * A, (size_t)b->nenv, hipMemcpyDeviceToHost), "draw rows download") ? 0 : -1;
}
int phys_batch_draw_perm_rows(phys_batch_t *b, int *host) {
    if (!b || !host) return refuse("phys_batch_draw_perm_rows", ck::DRAW_NOT_CONFIGURED);
    const ck::DrawCfg c = draw_cfg_of(b);
    if (const char *why = ck::check_draw_perm(c)) return refuse("phys_batch_draw_perm_rows", why);
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    return hip_ok(hipMemcpy(host, c.perm_dst ? c.perm_dst : c.perm, sizeof(int) * (size_t)c.perm_n, hipMemcpyDeviceToHost), "draw permutation download") ? 0 : -1;
}
int phys_batch_draw_download(phys_batch_t *b, unsigned *counts_host) {
    if (!b || !counts_host || !b->draw.on || !b->d_draw_counts) return refuse("phys_batch_draw_download", ck::DRAW_NOT_CONFIGURED);
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(counts_host, b->d_draw_counts, sizeof(unsigned) * (size_t)b->nenv, hipMemcpyDeviceToHost), "draw call counts download") ? 0 : -1;
}
int phys_batch_draw_upload(phys_batch_t *b, const unsigned *counts_host) {
    if (!b || !counts_host || !b->draw.on || !b->d_draw_counts) return refuse("phys_batch_draw_upload", ck::DRAW_NOT_CONFIGURED);
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(b->d_draw_counts, counts_host, sizeof(unsigned) * (size_t)b->nenv, hipMemcpyHostToDevice), "draw call counts upload") ? 0 : -1;
}
int phys_batch_debug_draw_launches(const phys_batch_t *b, long long *launches) {
    if (!b) return -1;
    if (launches) { launches[0] = b->draw_launches[0]; launches[1] = b->draw_launches[1]; }
    return 0;
}

int phys_batch_sync(phys_batch_t *b) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    return quiesce(b) ? 0 : -1; /* the batch's stream and the callers' streams of the recent launches (step_range / reset_envs) */
}

int phys_batch_enable_ext(phys_batch_t *b, int on) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (on && !b->d_ext) {
        if (!b->d_ext.alloc((size_t)b->nenv, false, "ext")) return -1;
        if (!hip_ok(hipMemsetAsync(b->d_ext, 0, sizeof(cm_ext_t) * (size_t)b->nenv, b->stream), "hipMemset(ext)") ||
            !hip_ok(hipStreamSynchronize(b->stream), "ext sync")) return -1;
    } else if (!on) b->d_ext.reset();
    return 0;
}

int phys_batch_download_ext(phys_batch_t *b, cm_ext_t *host, int env0, int n) {
    if (!b || !host || !b->d_ext || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    return hip_ok(hipMemcpyAsync(host, b->d_ext + env0, sizeof(cm_ext_t) * (size_t)n, hipMemcpyDeviceToHost, b->stream), "ext download") &&
                   hip_ok(hipStreamSynchronize(b->stream), "ext sync")
               ? 0 : -1;
}

int phys_batch_download_ext_async(phys_batch_t *b, cm_ext_t *host, int env0, int n) {
    if (!b || !host || !b->d_ext || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    return hip_ok(hipMemcpyAsync(host, b->d_ext + env0, sizeof(cm_ext_t) * (size_t)n, hipMemcpyDeviceToHost, b->stream), "ext download") ? 0 : -1;
}

int phys_batch_derive(phys_batch_t *b, const int ids[6], void *stream) {
    if (!b || !ids) return -1;
    (void)hipSetDevice(b->device);
    hipStream_t s = launch_stream(b, stream);
    for (int f : {PHYS_F_DERIVED, PHYS_F_QM}) {
        if (b->d_field[f]) continue;
        const size_t count = (size_t)b->nenv * b->dim[f];
        if (!b->d_field[f].alloc(count, false, "derived")) return -1;
        if (!hip_ok(hipMemsetAsync(b->d_field[f], 0, sizeof(double) * count, s), "hipMemset(derived)")) return -1;
    }
    const bool had_ext = b->d_ext != nullptr;
    if (!had_ext && phys_batch_enable_ext(b, 1) != 0) return -1;
    int rc = launch(b, 1, 0, s); /* forward: the read-out of the current state */
    hipLaunchKernelGGL(ck::cassie_derive_kernel, dim3(b->nenv), dim3(WV_WAVE), 0, s,
                       ck::make_derive_io(view_of(b), b->nenv, b->d_ext, b->d_field[PHYS_F_DERIVED], b->d_field[PHYS_F_QM], ids));
    rc |= hip_ok(hipGetLastError(), "cassie_derive_kernel launch") ? 0 : -1;
    if (!had_ext) {
        /* the read-out buffer is 20 KB per env and makes every step write it: keep it only for the caller who asked for it */
        if (!hip_ok(hipStreamSynchronize(s), "derive sync")) rc = -1;
        rc |= phys_batch_enable_ext(b, 0);
    }
    return rc;
}

/* ------------------------------------------------ per-env physical parameters ---- */
static const struct { size_t off; int per; } PARAM_TABLE[CM_P_COUNT] = {
    {offsetof(cm_envparams_t, body_mass), 1}, {offsetof(cm_envparams_t, body_ipos), 3}, {offsetof(cm_envparams_t, body_inertia), 3},
    {offsetof(cm_envparams_t, dof_damping), 1}, {offsetof(cm_envparams_t, geom_friction), 3},
    {offsetof(cm_envparams_t, geom_pos), 3}, {offsetof(cm_envparams_t, geom_quat), 4}, {offsetof(cm_envparams_t, jnt_stiffness), 1},
    {offsetof(cm_envparams_t, qpos_spring), 1}};
static int param_count(const phys_batch *b, int param) {
    const cm_model_t &m = b->host_model;
    switch (param) {
        case CM_P_DOF_DAMPING: return m.nv;
        case CM_P_GEOM_FRICTION: case CM_P_GEOM_POS: case CM_P_GEOM_QUAT: return m.ngeom;
        case CM_P_JNT_STIFFNESS: return m.njnt;
        case CM_P_QPOS_SPRING: return m.nq;
        default: return m.nbody;
    }
}
int phys_batch_param_dim(const phys_batch_t *b, int param) {
    return (b && param >= 0 && param < CM_P_COUNT) ? param_count(b, param) * PARAM_TABLE[param].per : 0;
}
/* the per-env blocks, created on first use: every env starts from the shared model's own block */
static bool ensure_envparams(phys_batch *b) {
    if (b->d_envparams) return true;
    if (b->model_stride != 0) { phys_set_last_error("per-env parameter blocks and per-env models (phys_batch_set_model with env >= 0) do not mix"); return false; }
    if (!quiesce(b)) return false;
    DevBuf<cm_envparams_t> all;
    if (!all.alloc((size_t)b->nenv, false, "env parameters")) return false;
    std::vector<cm_envparams_t> tmp((size_t)b->nenv, b->host_model.params);
    if (!hip_ok(hipMemcpy(all, tmp.data(), sizeof(cm_envparams_t) * tmp.size(), hipMemcpyHostToDevice), "hipMemcpy(env parameters)")) return false;
    b->d_envparams = std::move(all);
    return true;
}
static int launch_setconst(phys_batch *b, int env0, int n, int derive_inertial, hipStream_t s) {
    hipLaunchKernelGGL(ck::cassie_setconst_kernel, dim3((unsigned)ck::setconst_grid(n)), dim3(WV_WAVE), 0, s,
                       ck::make_setconst_io(b->d_models, b->d_envparams, env0, n, derive_inertial));
    return hip_ok(hipGetLastError(), "cassie_setconst_kernel launch") ? 0 : -1;
}
/* the shared model's cm_model_t::env_geom / env_springs word (at `off`): from now on the step kernel reads that group from the blocks
 * (in order on `s`, behind the rows and their re-derive) */
static int read_from_blocks(phys_batch *b, int *host_word, size_t off, hipStream_t s) {
    static const int one = 1;
    if (*host_word) return 0;
    *host_word = 1;
    return hip_ok(hipMemcpyAsync((char *)b->d_models.get() + off, &one, sizeof one, hipMemcpyHostToDevice, s), "hipMemcpy(model word)") ? 0 : -1;
}
int phys_batch_randomize(phys_batch_t *b, int param, const double *values, int on_device, int env0, int n, void *stream) {
    if (!b || !values || param < 0 || param >= CM_P_COUNT || !range_ok(b, env0, n)) { phys_set_last_error("phys_batch_randomize: bad arguments"); return -1; }
    (void)hipSetDevice(b->device);
    if (!ensure_envparams(b)) return -1;
    if (n == 0) return 0;
    hipStream_t s = launch_stream(b, stream);
    const int dim = phys_batch_param_dim(b, param);
    const double *src = values;
    DevBuf<double> staged;
    if (!on_device) {
        const size_t count = (size_t)n * dim;
        if (!staged.alloc(count, false, "parameter rows")) return -1;
        if (!hip_ok(hipMemcpyAsync(staged, values, sizeof(double) * count, hipMemcpyHostToDevice, s), "hipMemcpy(parameter rows)")) return -1;
        src = staged;
    }
    hipLaunchKernelGGL(ck::cassie_param_scatter_kernel, dim3((unsigned)ck::param_scatter_grid(n)), dim3(WV_WAVE), 0, s, b->d_envparams.get(),
                       (int)(PARAM_TABLE[param].off / sizeof(double)), dim, src, env0, n);
    int rc = hip_ok(hipGetLastError(), "cassie_param_scatter_kernel launch") ? 0 : -1;
    /* friction needs no set_const in the reference (mj_contactParam mixes the geoms' values at every step): the pairs' mixed
     * values are refreshed right away; so are geometry (MuJoCo's kinematics reads geom_pos / geom_quat at every step) and springs
     * (mj_passive reads jnt_stiffness / qpos_spring): their derived records follow at once, and the step kernel reads those of
     * the blocks from now on; nothing else is -- masses, inertial offsets and inertias wait for phys_batch_set_const like
     * mjModel edits wait for mj_setConst, damping takes effect as it is */
    if (rc == 0 && param == CM_P_GEOM_FRICTION) rc = launch_setconst(b, env0, n, ck::SETCONST_FRICTION, s);
    if (rc == 0 && (param == CM_P_GEOM_POS || param == CM_P_GEOM_QUAT)) {
        rc = launch_setconst(b, env0, n, ck::SETCONST_GEOMETRY, s);
        if (rc == 0) rc = read_from_blocks(b, &b->host_model.env_geom, offsetof(cm_model_t, env_geom), s);
    }
    if (rc == 0 && (param == CM_P_JNT_STIFFNESS || param == CM_P_QPOS_SPRING)) {
        rc = launch_setconst(b, env0, n, ck::SETCONST_SPRINGS, s);
        if (rc == 0) rc = read_from_blocks(b, &b->host_model.env_springs, offsetof(cm_model_t, env_springs), s);
    }
    if (staged && !hip_ok(hipStreamSynchronize(s), "randomize sync")) rc = -1;
    return rc;
}
int phys_batch_set_const(phys_batch_t *b, int env0, int n, void *stream) {
    if (!b || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    if (!ensure_envparams(b)) return -1;
    if (n == 0) return 0;
    return launch_setconst(b, env0, n, ck::SETCONST_ALL, launch_stream(b, stream));
}
int phys_batch_download_params(phys_batch_t *b, cm_envparams_t *host, int env0, int n) {
    if (!b || !host || !range_ok(b, env0, n)) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    if (!b->d_envparams) { for (int e = 0; e < n; ++e) host[e] = b->host_model.params; return 0; }
    return hip_ok(hipMemcpy(host, b->d_envparams + env0, sizeof(cm_envparams_t) * (size_t)n, hipMemcpyDeviceToHost), "parameter download") ? 0 : -1;
}
int phys_batch_uses_env_params(const phys_batch_t *b) { return b && b->d_envparams ? 1 : 0; }
size_t phys_sizeof_envparams(void) { return sizeof(cm_envparams_t); }

int phys_batch_set_all_outputs_every_substep(phys_batch_t *b, int on) {
    if (!b) return -1;
    b->all_outputs = on != 0;
    return 0;
}

int phys_batch_download_progress(phys_batch_t *b, int *host) {
    if (!b || !host || !b->d_progress) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    return hip_ok(hipMemcpy(host, b->d_progress, sizeof(int) * (size_t)b->nenv, hipMemcpyDeviceToHost), "progress download") ? 0 : -1;
}

int phys_batch_enable_kernel_timing(phys_batch_t *b, int on) {
    if (!b) return -1;
    b->timing = on != 0;
    b->ev_used = 0;
    return 0;
}

int phys_batch_kernel_timing(phys_batch_t *b, int *launches, double *total_ms) {
    if (!b || !launches || !total_ms) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    double sum = 0;
    int n = 0;
    for (size_t i = 0; i < b->ev_used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, b->ev_pool[i].first, b->ev_pool[i].second) == hipSuccess) { sum += ms; ++n; }
    }
    b->ev_used = 0;
    *launches = n; *total_ms = sum;
    return 0;
}

int phys_batch_set_fast_rows(phys_batch_t *b, int on) {
    if (!b) return -1;
    b->fast_rows = on != 0;
    return 0;
}

int phys_batch_debug_inplace_ranges(const phys_batch_t *b) {
    if (!b) return -1;
    int k = 0;
    for (const auto &r : b->ranges.ranges) k += r.inplace ? 1 : 0;
    return k;
}

int phys_batch_debug_form_launches(const phys_batch_t *b, long long *plain, long long *inplace) {
    if (!b) return -1;
    if (plain) *plain = b->form_launches[0];
    if (inplace) *inplace = b->form_launches[1];
    return 0;
}

int phys_batch_set_inplace(phys_batch_t *b, int mode) {
    if (!b || mode < 0 || mode > 2) return -1;
    b->inplace_mode = mode;
    return 0;
}

int phys_batch_step_sums_enable(phys_batch_t *b, int on) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    /* (first use: the batch's own block, zeroed -- unless a caller's tensor is bound to the field) */
    if (on && !b->d_field[PHYS_F_STEP_SUMS] && !b->d_field[PHYS_F_STEP_SUMS].alloc((size_t)b->nenv * CM_SUM_DIM, true, "step sums")) return -1;
    b->step_sums = on != 0;
    return 0;
}

int phys_batch_set_chunks(phys_batch_t *b, int chunks) {
    if (!b || chunks < 1 || chunks > 7) return -1;
    b->chunks = b->chunks_range = chunks;
    b->chunks_default = false;
    return 0;
}

int phys_batch_set_waves_per_env(phys_batch_t *b, int waves) {
    if (!b || (waves != 1 && waves != 2)) return -1;
    b->waves_per_env = waves;
    b->waves_per_env_tray = waves;
    return 0;
}

int phys_batch_download_cost(phys_batch_t *b, unsigned *host) {
    if (!b || !host || !b->d_cost) return -1;
    (void)hipSetDevice(b->device);
    return quiesce(b) && hip_ok(hipMemcpy(host, b->d_cost, sizeof(unsigned) * (size_t)b->nenv, hipMemcpyDeviceToHost), "cost download") ? 0 : -1;
}

int phys_batch_measured_shader_clock(phys_batch_t *b, double *hz) {
    if (!b || !hz || !b->d_cost || !b->d_cost_wall) return -1;
    (void)hipSetDevice(b->device);
    std::vector<unsigned> c((size_t)b->nenv), w((size_t)b->nenv);
    if (!quiesce(b) || !hip_ok(hipMemcpy(c.data(), b->d_cost, sizeof(unsigned) * c.size(), hipMemcpyDeviceToHost), "cost download") ||
        !hip_ok(hipMemcpy(w.data(), b->d_cost_wall, sizeof(unsigned) * w.size(), hipMemcpyDeviceToHost), "cost download")) return -1;
    double sc = 0, sw = 0;
    for (size_t i = 0; i < c.size(); ++i) if (w[i] > 1000u) { sc += 64.0 * c[i]; sw += w[i]; } /* (envs that spanned at least 10 us) */
    if (sw <= 0) return -1;
    *hz = sc / sw * 1e8;
    return 0;
}

int phys_batch_debug_handover_pending(phys_batch_t *b) {
    if (!b) return -1;
    if (!b->d_handover_count) return 0;
    (void)hipSetDevice(b->device);
    std::vector<int> h(2 * (size_t)b->nenv);
    long total = 0;
    if (!quiesce(b)) return -1;
    for (int *d : {b->d_handover_count.get(), b->d_handover_count2.get()}) {
        if (!d) continue;
        if (!hip_ok(hipMemcpy(h.data(), d, sizeof(int) * h.size(), hipMemcpyDeviceToHost), "hand-over count download")) return -1;
        /* (a range in the in-place form keeps other things in its first list's words: the in-place count since the order kernel's last
         * report and the run of quiet reports) */
        if (d == b->d_handover_count) for (const auto &r : b->ranges.ranges) if (r.inplace) h[2 * (size_t)r.env0] = h[2 * (size_t)r.env0 + 1] = 0;
        for (int v : h) total += v < 0 ? -(long)v : v;
    }
    return total > 0x7fffffff ? 0x7fffffff : (int)total;
}

/* envs the 63-row pass of the last stepping launch over [env0, ...) handed on to the 127-row pass (what that pass reported) */
int phys_batch_wide_pass_envs(phys_batch_t *b, int env0) {
    if (!b || env0 < 0 || env0 >= b->nenv || !b->handover_seen2.host()) return -1;
    (void)hipSetDevice(b->device);
    if (!quiesce(b)) return -1;
    return *(volatile int *)(b->handover_seen2.host() + env0);
}

int phys_batch_set_balance(phys_batch_t *b, int on) {
    if (!b) return -1;
    b->balance = on != 0;
    return 0;
}

/* validation aid: fills the LDS of every CU with NaN bit patterns (LDS is not cleared between kernels), so that a step
 * kernel that reads LDS it has not written shows up in the results on any box, not only on a freshly booted one */
__global__ void __launch_bounds__(64) cassie_poison_lds_kernel(int *sink) {
    __shared__ unsigned long long blob[4975];   /* 39 800 B: the step kernel's footprint, so four of these fill a CU */
    for (int i = threadIdx.x; i < 4975; i += 64) blob[i] = 0xffffffffffffffffull;
    __syncthreads();
    if (sink && blob[(threadIdx.x * 77) % 4975] == 1ull) sink[0] = 1; /* keeps the stores alive */
}
int phys_batch_debug_poison_lds(phys_batch_t *b) {
    if (!b) return -1;
    (void)hipSetDevice(b->device);
    hipLaunchKernelGGL(cassie_poison_lds_kernel, dim3(8192), dim3(64), 0, b->stream, (int *)nullptr);
    return hip_ok(hipGetLastError(), "poison launch") && hip_ok(hipStreamSynchronize(b->stream), "poison sync") ? 0 : -1;
}

int phys_batch_set_generic_kernel(phys_batch_t *b, int on) {
    if (!b) return -1;
    b->generic_kernel = on != 0;
    return 0;
}

int phys_batch_profile_step(phys_batch_t *b, long long *host_stamps) { return phys_batch_profile_substeps(b, 1, host_stamps); }

int phys_batch_profile_substeps(phys_batch_t *b, int nsub, long long *host_stamps) {
    if (!b || !host_stamps || nsub < 1) return -1;
    (void)hipSetDevice(b->device);
    const size_t bytes = sizeof(long long) * ck::NSTAMP * (size_t)b->nenv;
    if (!b->d_prof.alloc(ck::NSTAMP * (size_t)b->nenv, false, "prof")) return -1;
    (void)hipMemsetAsync(b->d_prof, 0, bytes, b->stream);
    int rc = launch(b, nsub, 1, b->stream);
    bool ok = rc == 0 && hip_ok(hipStreamSynchronize(b->stream), "sync") &&
              hip_ok(hipMemcpy(host_stamps, b->d_prof, bytes, hipMemcpyDeviceToHost), "prof download");
    b->d_prof.reset();
    return ok ? 0 : -1;
}

int phys_batch_time_steps(phys_batch_t *b, int nsub, int reps, float *mean_ms) {
    if (!b || nsub <= 0 || reps <= 0 || !mean_ms) return -1;
    (void)hipSetDevice(b->device);
    if (!hip_ok(hipEventRecord(b->ev0, b->stream), "hipEventRecord")) return -1;
    for (int r = 0; r < reps; ++r)
        if (launch(b, nsub, 1, b->stream) != 0) return -1;
    if (!hip_ok(hipEventRecord(b->ev1, b->stream), "hipEventRecord")) return -1;
    if (!hip_ok(hipEventSynchronize(b->ev1), "hipEventSynchronize")) return -1;
    float ms = 0;
    if (!hip_ok(hipEventElapsedTime(&ms, b->ev0, b->ev1), "hipEventElapsedTime")) return -1;
    *mean_ms = ms / reps;
    return 0;
}

}  // extern "C"
