"""Locates and loads the product shared library and derives the ctypes layout of cm_model_t."""
import ctypes
import os

from . import cstruct

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # .../cassie-mujoco-sim_amd
REPO_DIR = os.path.dirname(PKG_DIR)
# CASSIE_LIB selects another build of the same library (tools/build_variant.sh: compiler-option experiments)
LIB_PATH = os.environ.get("CASSIE_LIB") or os.path.join(PKG_DIR, "lib", "libcassiemujoco.so")
MODEL_DIR = os.path.join(REPO_DIR, "models")

# (a variant built from an older source tree comes with its own header: <variant>.so.cm_model.h next to it)
_variant_hdr = LIB_PATH + ".cm_model.h"
with open(_variant_hdr if os.path.exists(_variant_hdr) else os.path.join(PKG_DIR, "csrc", "cm_model.h")) as _f:
    _hdr = _f.read()
MACROS = cstruct.parse_defines(_hdr)
_structs = cstruct.parse_structs(_hdr, MACROS)
CmModel = _structs["cm_model_t"]
CmDriveState = _structs["cm_drive_state_t"]
CmEnvParams = _structs["cm_envparams_t"]
CmEpisodeRules = _structs.get("cm_episode_rules_t")   # (None with the header of an older variant build)

_lib = None


def lib():
    """The product library.  Raises (loudly) if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s is missing: build it with `make` (or __graft_entry__.build()); "
                "this package has no pure-Python or CPU fallback" % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        _declare(_lib)
        if _lib.phys_sizeof_model() != ctypes.sizeof(CmModel):
            raise RuntimeError("cm_model_t layout mismatch between cm_model.h and the built library")
        if hasattr(_lib, "phys_sizeof_envparams") and _lib.phys_sizeof_envparams() != ctypes.sizeof(CmEnvParams):
            raise RuntimeError("cm_envparams_t layout mismatch between cm_model.h and the built library")
        if hasattr(_lib, "phys_sizeof_episode_rules") and _lib.phys_sizeof_episode_rules() != ctypes.sizeof(CmEpisodeRules):
            raise RuntimeError("cm_episode_rules_t layout mismatch between cm_model.h and the built library")
    return _lib


def _declare(L):
    c = ctypes
    vp, ip, dp = c.c_void_p, c.POINTER(c.c_int), c.POINTER(c.c_double)
    L.phys_sizeof_model.restype = c.c_size_t
    L.phys_last_error.restype = c.c_char_p
    L.phys_model_load.restype = vp
    L.phys_model_load.argtypes = [c.c_char_p, c.c_char_p, c.c_int]
    L.phys_model_copy.restype = vp
    L.phys_model_copy.argtypes = [vp]
    L.phys_model_free.argtypes = [vp]
    L.phys_model_save.argtypes = [vp, c.c_char_p]
    L.phys_model_set_const.argtypes = [vp]
    if hasattr(L, "phys_model_set_flag"):
        L.phys_model_set_flag.argtypes = [vp, c.c_uint, c.c_int]
        L.phys_model_flags.argtypes = [vp]
        L.phys_model_flags.restype = c.c_uint
    L.phys_model_compile.argtypes = [vp, c.POINTER(CmModel), c.c_char_p, c.c_int]
    L.phys_model_name2id.argtypes = [vp, c.c_int, c.c_char_p]
    L.phys_model_id2name.restype = c.c_char_p
    L.phys_model_id2name.argtypes = [vp, c.c_int, c.c_int]
    L.phys_model_size.argtypes = [vp, c.c_int]
    L.phys_model_array.restype = dp
    L.phys_model_array.argtypes = [vp, c.c_int]
    L.phys_model_iarray.restype = ip
    L.phys_model_iarray.argtypes = [vp, c.c_int]
    L.phys_model_geom_rgba.restype = c.POINTER(c.c_float)
    L.phys_model_geom_rgba.argtypes = [vp]
    L.phys_model_hfield_data.restype = c.POINTER(c.c_float)
    L.phys_model_hfield_data.argtypes = [vp]
    L.phys_batch_create.restype = vp
    L.phys_batch_create.argtypes = [c.POINTER(CmModel), c.c_int, c.c_int]
    L.phys_batch_free.argtypes = [vp]
    L.phys_batch_nenv.argtypes = [vp]
    L.phys_batch_field_dim.argtypes = [vp, c.c_int]
    L.phys_batch_set_model.argtypes = [vp, c.POINTER(CmModel), c.c_int]
    L.phys_batch_set_hfield.argtypes = [vp, c.POINTER(c.c_float), c.c_int]
    if hasattr(L, "phys_batch_randomize"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_param_dim.argtypes = [vp, c.c_int]
        L.phys_batch_randomize.argtypes = [vp, c.c_int, vp, c.c_int, c.c_int, c.c_int, vp]
        L.phys_batch_set_const.argtypes = [vp, c.c_int, c.c_int, vp]
        L.phys_batch_download_params.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_uses_env_params.argtypes = [vp]
        L.phys_sizeof_envparams.restype = c.c_size_t
    L.phys_batch_set_hfield_env.argtypes = [vp, c.c_int, c.POINTER(c.c_float), c.c_int]
    L.phys_batch_upload.argtypes = [vp, c.c_int, vp, c.c_int, c.c_int]
    L.phys_batch_download.argtypes = [vp, c.c_int, vp, c.c_int, c.c_int]
    L.phys_batch_download_warn.argtypes = [vp, vp, vp]
    L.phys_batch_device_ptr.restype = vp
    L.phys_batch_device_ptr.argtypes = [vp, c.c_int]
    L.phys_batch_bind.argtypes = [vp, c.c_int, vp]
    L.phys_batch_bind_strided.argtypes = [vp, c.c_int, vp, c.c_int]
    L.phys_batch_clear_warn.argtypes = [vp, c.c_int, c.c_int]
    L.phys_batch_step.argtypes = [vp, c.c_int, vp]
    L.phys_batch_forward.argtypes = [vp, vp]
    L.phys_batch_forward_kinematics.argtypes = [vp, vp]
    L.phys_batch_sync.argtypes = [vp]
    L.phys_batch_set_pd_mode.argtypes = [vp, c.c_int]
    L.phys_batch_set_drive_mode.argtypes = [vp, c.c_int]
    L.phys_batch_upload_drive_state.argtypes = [vp, vp, c.c_int, c.c_int]
    L.phys_batch_download_drive_state.argtypes = [vp, vp, c.c_int, c.c_int]
    L.phys_batch_uses_applied.argtypes = [vp]
    L.phys_batch_drive_pass.argtypes = [vp, c.c_int, vp]
    L.phys_batch_mark.argtypes = [vp]
    L.phys_batch_debug_poison_lds.argtypes = [vp]
    L.phys_batch_set_balance.argtypes = [vp, c.c_int]
    L.phys_batch_set_fast_rows.argtypes = [vp, c.c_int]
    L.phys_batch_set_waves_per_env.argtypes = [vp, c.c_int]
    L.phys_batch_set_inplace.argtypes = [vp, c.c_int]
    L.phys_batch_debug_inplace_ranges.argtypes = [vp]
    L.phys_batch_debug_form_launches.argtypes = [vp, c.POINTER(c.c_longlong), c.POINTER(c.c_longlong)]
    L.phys_batch_download_cost.argtypes = [vp, vp]
    L.phys_batch_measured_shader_clock.argtypes = [vp, vp]
    L.phys_batch_wide_pass_envs.argtypes = [vp, c.c_int]
    L.phys_batch_set_chunks.argtypes = [vp, c.c_int]
    L.phys_batch_debug_handover_pending.argtypes = [vp]
    L.phys_batch_debug_handover_pending.restype = c.c_int
    if hasattr(L, "phys_batch_kernel_timing"):
        L.phys_batch_enable_kernel_timing.argtypes = [vp, c.c_int]
        L.phys_batch_kernel_timing.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_double)]
    if hasattr(L, "phys_batch_step_range"):
        L.phys_batch_step_range.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
    if hasattr(L, "phys_batch_reset_envs"):
        L.phys_batch_reset_envs.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp, vp, vp]
    if hasattr(L, "phys_batch_end_episodes"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_episodes_enable.argtypes = [vp, c.POINTER(CmEpisodeRules)]
        L.phys_batch_episodes_set_bank.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_episode_row_dim.argtypes = [vp]
        L.phys_batch_episode_ptr.restype = vp
        L.phys_batch_episode_ptr.argtypes = [vp, c.c_int]
        L.phys_batch_episode_bind.argtypes = [vp, c.c_int, vp]
        L.phys_batch_end_episodes.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp, vp, vp]
        L.phys_batch_download_episodes.argtypes = [vp, c.c_int, vp]
        L.phys_sizeof_episode_rules.restype = c.c_size_t
    if hasattr(L, "phys_batch_place_configure"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_place_configure.argtypes = [vp, c.c_int, vp, c.c_int, c.c_double]
        L.phys_batch_place_ptr.restype = vp
        L.phys_batch_place_ptr.argtypes = [vp, c.c_int]
        L.phys_batch_place_bind.argtypes = [vp, c.c_int, vp]
        L.phys_batch_place_upload.argtypes = [vp, c.c_int, vp, c.c_int, c.c_int]
        L.phys_batch_place_download.argtypes = [vp, c.c_int, vp]
    if hasattr(L, "phys_batch_state_save"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_state_configure.argtypes = [vp, c.c_int, c.c_int]
        L.phys_batch_state_bind.argtypes = [vp, vp, c.c_int]
        L.phys_batch_state_ptr.restype = vp
        L.phys_batch_state_ptr.argtypes = [vp]
        for f in ("nslots", "groups", "row_dim"):
            getattr(L, "phys_batch_state_" + f).argtypes = [vp]
        L.phys_batch_state_layout.argtypes = [vp, ip]
        L.phys_batch_state_signature.restype = c.c_ulonglong
        L.phys_batch_state_signature.argtypes = [vp]
        L.phys_batch_state_save.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_state_restore.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_state_stage_slots.restype = vp
        L.phys_batch_state_stage_slots.argtypes = [vp, vp, c.c_int]
        L.phys_batch_state_download.argtypes = [vp, c.c_int, c.c_int, vp]
        L.phys_batch_state_upload.argtypes = [vp, c.c_int, c.c_int, vp, c.c_ulonglong]
    if hasattr(L, "phys_batch_set_hfield_bank"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_set_hfield_bank.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int]
        L.phys_batch_nterrain.argtypes = [vp]
        L.phys_batch_terrain_index_ptr.restype = vp
        L.phys_batch_terrain_index_ptr.argtypes = [vp]
        L.phys_batch_bind_terrain_index.argtypes = [vp, vp]
        L.phys_batch_set_terrain.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, vp]
        L.phys_batch_scan_configure.argtypes = [vp, vp, c.c_int, c.c_int, c.c_double]
        L.phys_batch_height_scan.argtypes = [vp, c.c_int, c.c_int, vp]
    if hasattr(L, "phys_batch_depth_image"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_depth_configure.argtypes = [vp, c.c_int, vp, vp, c.c_int, c.c_int, c.c_double, c.c_double, c.c_double]
        L.phys_batch_depth_bind_pose.argtypes = [vp, vp]
        L.phys_batch_depth_image.argtypes = [vp, c.c_int, c.c_int, vp]
    if hasattr(L, "phys_batch_depth_set_geoms"):   # (likewise)
        L.phys_batch_depth_set_geoms.argtypes = [vp, c.c_uint]
        L.phys_batch_depth_default_geoms.argtypes = [vp]
        L.phys_batch_depth_default_geoms.restype = c.c_uint
        L.phys_batch_depth_all_geoms.argtypes = [vp]
        L.phys_batch_depth_all_geoms.restype = c.c_uint
        L.phys_batch_depth_bind_ids.argtypes = [vp, vp]
        L.phys_batch_debug_depth_launches.argtypes = [vp, c.POINTER(c.c_longlong), c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_rays_cast"):   # (likewise)
        L.phys_batch_rays_configure.argtypes = [vp, vp, c.c_int, c.c_double, c.c_double]
        L.phys_batch_rays_set_geoms.argtypes = [vp, c.c_uint]
        L.phys_batch_rays_bind_ids.argtypes = [vp, vp]
        L.phys_batch_rays_bind_normals.argtypes = [vp, vp]
        L.phys_batch_rays_cast.argtypes = [vp, c.c_int, c.c_int, vp]
        L.phys_batch_debug_ray_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_probe"):   # (likewise)
        L.phys_batch_probes_configure.argtypes = [vp, vp, c.c_int, c.c_uint]
        L.phys_batch_probe_geom_classes.argtypes = [vp, vp]
        L.phys_batch_probe.argtypes = [vp, c.c_int, c.c_int, vp]
        L.phys_batch_probe_row_dim.argtypes = [vp]
        L.phys_batch_probe_layout.argtypes = [vp, vp, vp]
        L.phys_batch_probe_contacts_ptr.argtypes = [vp]
        L.phys_batch_probe_contacts_ptr.restype = vp
        L.phys_batch_probe_bind_contacts.argtypes = [vp, vp]
        L.phys_batch_probe_download_contacts.argtypes = [vp, vp]
        L.phys_batch_debug_probe_launches.argtypes = [vp, c.POINTER(c.c_longlong), c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_obs"):   # (likewise)
        L.phys_batch_obs_configure.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, c.c_ulonglong, c.c_uint]
        L.phys_batch_obs_bind.argtypes = [vp, vp, c.c_longlong]
        L.phys_batch_obs_bind_input.argtypes = [vp, vp, c.c_int, c.c_longlong, c.c_int]
        L.phys_batch_obs.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_obs_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]
        L.phys_batch_obs_layout.argtypes = [vp, vp]
        L.phys_batch_obs_download.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_obs_frames.argtypes = [vp, vp]
        L.phys_batch_obs_set_frames.argtypes = [vp, vp]
        L.phys_batch_debug_obs_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_reward"):   # (likewise)
        L.phys_batch_reward_configure.argtypes = [vp, vp, c.c_int, c.c_int, c.c_double, c.c_double]
        L.phys_batch_reward_bind.argtypes = [vp, vp, c.c_longlong]
        L.phys_batch_reward_bind_terms.argtypes = [vp, vp, c.c_longlong, c.c_int]
        L.phys_batch_reward_bind_input.argtypes = [vp, vp, c.c_int, c.c_longlong, c.c_int]
        L.phys_batch_reward.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_reward_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]
        L.phys_batch_reward_download.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_reward_download_terms.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_reward_returns.argtypes = [vp, vp]
        L.phys_batch_reward_set_returns.argtypes = [vp, vp]
        L.phys_batch_reward_final.argtypes = [vp, vp]
        L.phys_batch_debug_reward_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_act"):   # (likewise)
        L.phys_batch_act_configure.argtypes = [vp, vp, c.c_int, c.c_int, c.c_int, c.c_ulonglong, c.c_uint]
        L.phys_batch_act_bind_actions.argtypes = [vp, vp, c.c_longlong, c.c_int]
        L.phys_batch_act_bind_rows.argtypes = [vp, vp, c.c_longlong]
        L.phys_batch_act_bind_input.argtypes = [vp, vp, c.c_int, c.c_longlong, c.c_int]
        L.phys_batch_act_bind_delay.argtypes = [vp, vp]
        L.phys_batch_act.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_act_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_int)]
        L.phys_batch_act_download.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_act_state.argtypes = [vp, vp, vp]
        L.phys_batch_act_set_state.argtypes = [vp, vp, vp]
        L.phys_batch_debug_act_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_task"):   # (likewise)
        L.phys_batch_task_configure.argtypes = [vp, vp, c.c_int, c.c_int, c.c_ulonglong, c.c_uint]
        L.phys_batch_task_set_table.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_task_bind_rows.argtypes = [vp, vp, c.c_longlong]
        L.phys_batch_task.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_task_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_int)]
        L.phys_batch_task_download.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_task_state.argtypes = [vp, vp, vp, vp]
        L.phys_batch_task_set_state.argtypes = [vp, vp, vp, vp]
        L.phys_batch_debug_task_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_events"):   # (likewise)
        L.phys_batch_events_configure.argtypes = [vp, vp, c.c_int, c.c_int, c.c_ulonglong]
        L.phys_batch_events_bind_rows.argtypes = [vp, vp, c.c_longlong]
        L.phys_batch_events_bind_input.argtypes = [vp, vp, c.c_int, c.c_longlong, c.c_int]
        L.phys_batch_events_bind_flags.argtypes = [vp, vp]
        L.phys_batch_events_flags_ptr.argtypes = [vp]
        L.phys_batch_events_flags_ptr.restype = vp
        L.phys_batch_events.argtypes = [vp, c.c_int, c.c_int, vp, vp]
        L.phys_batch_events_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), c.POINTER(c.c_ulonglong)]
        L.phys_batch_events_download.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_events_download_flags.argtypes = [vp, vp]
        L.phys_batch_events_state.argtypes = [vp, vp, vp, vp]
        L.phys_batch_events_set_state.argtypes = [vp, vp, vp, vp]
        L.phys_batch_debug_events_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_policy"):   # (likewise)
        L.phys_batch_policy_configure.argtypes = [vp, vp, c.c_int, c.c_int]
        L.phys_batch_policy_load.argtypes = [vp, c.c_int, c.c_int, vp, c.c_longlong, vp, vp]
        L.phys_batch_policy_load_host.argtypes = [vp, c.c_int, c.c_int, vp, c.c_longlong, vp]
        L.phys_batch_policy_bind_input.argtypes = [vp, vp, c.c_int, c.c_longlong, c.c_int]
        L.phys_batch_policy_bind_norm.argtypes = [vp, vp, vp, c.c_double]
        L.phys_batch_policy_bind_output.argtypes = [vp, c.c_int, vp, c.c_longlong]
        L.phys_batch_policy_bind_sample.argtypes = [vp, vp, c.c_longlong, vp, vp, c.c_longlong, vp]
        L.phys_batch_policy.argtypes = [vp, c.c_int, c.c_int, vp]
        L.phys_batch_policy_download.argtypes = [vp, c.c_int, vp]
        L.phys_batch_policy_download_packed.argtypes = [vp, vp, c.POINTER(c.c_longlong)]
        L.phys_batch_debug_policy_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_rollout_record"):   # (likewise)
        L.phys_batch_rollout_configure.argtypes = [vp, c.c_int, vp, c.c_int, c.c_double, c.c_double, c.c_uint]
        L.phys_batch_rollout_bind_source.argtypes = [vp, c.c_int, vp, c.c_longlong]
        L.phys_batch_rollout_bind_storage.argtypes = [vp, c.c_int, vp, c.c_longlong, c.c_longlong]
        L.phys_batch_rollout_ptr.argtypes = [vp, c.c_int, c.POINTER(c.c_longlong), c.POINTER(c.c_longlong)]
        L.phys_batch_rollout_ptr.restype = vp
        L.phys_batch_rollout_record.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
        L.phys_batch_rollout_finish.argtypes = [vp, c.c_int, c.c_int, vp, c.c_longlong, vp]
        L.phys_batch_rollout_normalise.argtypes = [vp, c.c_double, vp]
        L.phys_batch_rollout_stats.argtypes = [vp, vp]
        L.phys_batch_rollout_download.argtypes = [vp, c.c_int, vp]
        L.phys_batch_rollout_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_int), vp]
        L.phys_batch_debug_rollout_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_grad"):   # (likewise)
        L.phys_batch_grad_configure.argtypes = [vp, c.c_int, c.c_int, c.c_double, c.c_double, c.c_double]
        L.phys_batch_grad_bind.argtypes = [vp, c.c_int, c.c_int, vp, c.c_longlong, vp]
        L.phys_batch_grad_bind_log_std.argtypes = [vp, vp]
        L.phys_batch_grad.argtypes = [vp, vp, c.c_int, vp]
        L.phys_batch_grad_stats.argtypes = [vp, vp]
        L.phys_batch_grad_count.argtypes = [vp, c.c_int, c.c_int, c.c_int]
        L.phys_batch_grad_count.restype = c.c_longlong
        L.phys_batch_grad_download.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
        L.phys_batch_debug_grad_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
        L.phys_batch_debug_grad_mask.argtypes = [vp, c.c_uint]
    if hasattr(L, "phys_batch_opt_step"):   # (likewise)
        L.phys_batch_opt_configure.argtypes = [vp, c.c_double, c.c_double, c.c_double, c.c_double]
        L.phys_batch_opt_bind_param.argtypes = [vp, c.c_int, c.c_int, vp, c.c_longlong, vp]
        L.phys_batch_opt_bind_log_std.argtypes = [vp, vp]
        L.phys_batch_opt_step.argtypes = [vp, c.c_double, vp]
        L.phys_batch_opt_stats.argtypes = [vp, vp]
        L.phys_batch_opt_count.argtypes = [vp, c.c_int, c.c_int, c.c_int]
        L.phys_batch_opt_count.restype = c.c_longlong
        L.phys_batch_opt_download.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
        L.phys_batch_opt_upload.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
        L.phys_batch_debug_opt_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
        L.phys_batch_debug_opt_mask.argtypes = [vp, c.c_uint]
    if hasattr(L, "phys_batch_norm_update"):   # (likewise)
        L.phys_batch_norm_configure.argtypes = [vp, c.c_int, c.c_int, c.c_longlong, c.c_double]
        L.phys_batch_norm_bind_source.argtypes = [vp, vp, c.c_int, c.c_int, c.c_longlong, c.c_longlong]
        L.phys_batch_norm_bind_output.argtypes = [vp, vp, vp]
        L.phys_batch_norm_update.argtypes = [vp, vp]
        L.phys_batch_norm_write.argtypes = [vp, vp]
        L.phys_batch_norm_stats.argtypes = [vp, vp]
        L.phys_batch_norm_count.argtypes = [vp, c.c_int]
        L.phys_batch_norm_count.restype = c.c_longlong
        L.phys_batch_norm_download.argtypes = [vp, c.c_int, vp]
        L.phys_batch_norm_upload.argtypes = [vp, c.c_int, vp]
        L.phys_batch_debug_norm_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
        L.phys_batch_debug_norm_mask.argtypes = [vp, c.c_uint]
    if hasattr(L, "phys_batch_draw"):   # (likewise)
        L.phys_batch_draw_configure.argtypes = [vp, c.c_int, c.c_longlong, c.c_ulonglong, c.c_uint]
        L.phys_batch_draw_bind.argtypes = [vp, vp, c.c_longlong]
        L.phys_batch_draw_bind_perm.argtypes = [vp, vp]
        L.phys_batch_draw.argtypes = [vp, c.c_int, c.c_int, vp]
        L.phys_batch_draw_perm.argtypes = [vp, c.c_uint, vp]
        L.phys_batch_draw_perm_ptr.argtypes = [vp]
        L.phys_batch_draw_perm_ptr.restype = vp
        L.phys_batch_draw_dim.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(c.c_longlong)]
        L.phys_batch_draw_rows.argtypes = [vp, vp]
        L.phys_batch_draw_perm_rows.argtypes = [vp, vp]
        L.phys_batch_draw_download.argtypes = [vp, vp]
        L.phys_batch_draw_upload.argtypes = [vp, vp]
        L.phys_batch_debug_draw_launches.argtypes = [vp, c.POINTER(c.c_longlong)]
    if hasattr(L, "phys_batch_step_sums_enable"):   # (likewise)
        L.phys_batch_step_sums_enable.argtypes = [vp, c.c_int]
    if hasattr(L, "phys_batch_download_progress"):   # (absent from older variant builds selected with CASSIE_LIB)
        L.phys_batch_download_progress.argtypes = [vp, vp]
    L.phys_batch_set_all_outputs_every_substep.argtypes = [vp, c.c_int]
    L.phys_batch_derive.argtypes = [vp, c.POINTER(c.c_int), vp]
    L.phys_batch_clear_drive_state.argtypes = [vp, c.c_int, c.c_int, c.c_int, vp]
    L.phys_batch_wait_mark.argtypes = [vp]
    L.phys_batch_set_generic_kernel.argtypes = [vp, ctypes.c_int]
    L.phys_batch_profile_step.argtypes = [vp, vp]
    L.phys_batch_profile_substeps.argtypes = [vp, ctypes.c_int, vp]
    L.phys_batch_time_steps.argtypes = [vp, c.c_int, c.c_int, c.POINTER(c.c_float)]
