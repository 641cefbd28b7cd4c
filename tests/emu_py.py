"""ctypes access to the CPU wave emulator running the real physics_kernel.h -- test infrastructure only.  The one binding of
tests/emu/libcassie_emu.so (tests/wave_check.py loads it besides, for the wc_* entries it shares with the device's library).

A call is handed everything it reads in one block (tests/emu/emu_api.h) -- the arrays and the emulator's settings; the library keeps
nothing from call to call.  `with settings(fast_rows=1, chunks=3) as run:` changes what the calls inside the block are handed, and
`run` adds up what they report (fast_bails, wide_envs, chunk_fault)."""
import contextlib
import ctypes
import os

import numpy as np

from cassie_amd._lib import CmDriveState, CmEpisodeRules, CmModel, REPO_DIR

_lib = None
_vp, _ci, _ul = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong


class Settings(ctypes.Structure):
    _fields_ = [(f, _ci) for f in ("two_waves", "fast_rows", "inplace", "inplace_stay_rows", "chunks", "resume_grid", "wave_schedule",
                                   "force_runtime_topology", "force_guarded_pgs", "poison_lds")] + \
               [("poison_lo", _ul), ("poison_hi", _ul), ("skip_com_init", _ci), ("producer_xcc", _ci)]


class StepArgs(ctypes.Structure):
    _fields_ = [("model", ctypes.POINTER(CmModel)), ("nenv", _ci), ("nsub", _ci), ("integrate", _ci)] + \
               [(f, _vp) for f in ("qpos", "qvel", "qacc_warmstart", "time", "ctrl", "qfrc_applied", "xfrc_applied", "qacc", "sensordata",
                                   "actuator_velocity", "warn", "info", "xpos", "xquat", "pd_ptarget", "pd_kp", "pd_kd")] + \
               [("drive_mode", _ci)] + [(f, _vp) for f in ("drive_state", "drive_cmd", "meas", "pd_dtarget", "pd_torque", "envparams", "hfield")] + \
               [("hfield_stride", _ul), ("hfield_index", _vp), ("nterrain", _ci), ("settings", Settings)]


class StepResult(ctypes.Structure):
    _fields_ = [(f, _ci) for f in ("fast_bails", "wide_envs", "chunk_fault")]


API = (Settings, StepArgs, StepResult)          # by emu_sizeof_api's / emu_offsetof_api's `which`
DEFAULTS = dict(resume_grid=2, chunks=1)        # the settings that are not zero by default


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(os.path.join(REPO_DIR, "tests", "emu", "libcassie_emu.so"))
        L.emu_sizeof_api.restype, L.emu_offsetof_api.restype = _ul, ctypes.c_long
        for which, T in enumerate(API):
            assert ctypes.sizeof(T) == L.emu_sizeof_api(which), T
            offsets = [L.emu_offsetof_api(which, k) for k in range(len(T._fields_) + 1)]
            assert offsets == [getattr(T, f).offset for f, _ in T._fields_] + [-1], T
        L.emu_phys_run.argtypes = [ctypes.POINTER(StepArgs), ctypes.POINTER(StepResult)]
        L.emu_derive.argtypes = [ctypes.POINTER(StepArgs), _vp, _vp, _vp, ctypes.POINTER(StepResult)]
        L.emu_pick_family.argtypes = [ctypes.POINTER(CmModel), _ci]
        L.emu_launch_forms.argtypes, L.emu_launch_forms.restype = [_ci] * 11 + [_vp], None
        L.emu_pass_grids.argtypes, L.emu_pass_grids.restype = [_ci] * 4 + [_vp], None
        L.emu_policy_defaults.argtypes, L.emu_policy_defaults.restype = [_vp], None
        L.emu_ranges_claim.argtypes = [_vp, _vp, _ci, _ci, _vp, _vp]
        L.emu_set_const.argtypes = [ctypes.POINTER(CmModel), _vp, _ci, _ci]
        L.emu_sizeof_envparams.restype = _ul
        L.emu_end_episodes.argtypes = ([ctypes.POINTER(CmModel), ctypes.POINTER(CmEpisodeRules)] + [_ci] * 4 + [_vp, _ci] * 3 + [_vp] * 13 +
                                       [_vp, _ci] + [_vp] * 2)
        L.emu_sizeof_episode_rules.restype, L.emu_offsetof_episode_rules.restype = _ul, ctypes.c_long
        L.emu_height_scan.argtypes = [ctypes.POINTER(CmModel), _vp, _ci, _ci, _ci, _vp, _ci, _ci, ctypes.c_double, _vp, _ci, _vp, _ci, _vp, _ul, _vp, _ci, _vp]
        L.emu_core_safety.argtypes, L.emu_core_safety.restype = [_ci] + [_vp] * 7, None
        L.emu_depth_geoms.argtypes, L.emu_depth_geoms.restype = [ctypes.POINTER(CmModel), _ci], ctypes.c_uint
        L.emu_depth_scene_kernel.argtypes = [ctypes.POINTER(CmModel), ctypes.c_uint, _ci]
        L.emu_scan_check.argtypes, L.emu_scan_check.restype = [ctypes.POINTER(CmModel), _ci, _vp, _ci, _ci, ctypes.c_double], ctypes.c_char_p
        L.emu_depth_check.argtypes = [ctypes.POINTER(CmModel), _ci, _ci, _vp, _vp, _ci, _ci] + [ctypes.c_double] * 3
        L.emu_depth_check.restype = ctypes.c_char_p
        L.emu_depth_geoms_check.argtypes, L.emu_depth_geoms_check.restype = [ctypes.POINTER(CmModel), ctypes.c_uint], ctypes.c_char_p
        _lib = L
    return _lib


class Counters:
    """What emulated step calls reported, added up."""

    def __init__(self):
        self.fast_bails = self.wide_envs = self.chunk_fault = 0

    def add(self, r):
        self.fast_bails += r.fast_bails
        self.wide_envs += r.wide_envs
        self.chunk_fault |= r.chunk_fault


_active = []    # the settings() blocks we are inside: (overrides, counters), outermost first


@contextlib.contextmanager
def settings(**kw):
    """The emulator's settings (emu_api.h: emu_settings) of the calls made inside the block, on top of those of the blocks around it;
    yields the Counters of those calls."""
    assert all(hasattr(Settings, k) for k in kw), kw
    run = Counters()
    _active.append((kw, run))
    try:
        yield run
    finally:
        _active.pop()


def _ptr(a):
    return None if a is None else a.ctypes.data if isinstance(a, np.ndarray) else ctypes.addressof(a)


class EmuBatch:
    """Same state arrays as cassie_amd.Batch, stepped by the emulated kernel."""

    def __init__(self, pod, nenv):
        self.pod, self.nenv = pod, nenv
        z = lambda n: np.zeros((nenv, n))
        self.qpos = np.tile(np.array(pod.qpos0[: pod.nq]), (nenv, 1))
        self.qvel, self.qacc_warmstart, self.qacc = z(pod.nv), z(pod.nv), z(pod.nv)
        self.ctrl, self.actuator_velocity = z(pod.nu), z(pod.nu)
        self.sensordata = z(pod.nsensordata)
        self.time = np.zeros(nenv)
        self.qfrc_applied, self.xfrc_applied = None, None
        self.warn = np.zeros(nenv, dtype=np.int32)
        self.info = np.zeros((nenv, 4), dtype=np.int32)
        self.xpos = z(pod.nbody * 3)
        self.xquat = z(pod.nbody * 4)
        self.pd_ptarget = self.pd_kp = self.pd_kd = None
        # the height field, float32: one grid [nrow * ncol] shared by all envs; with hfield_stride (floats between the grids) every env's
        # own (hfield_index None) or a bank of nterrain grids that hfield_index [nenv] (int32) picks from
        self.hfield, self.hfield_stride, self.hfield_index, self.nterrain = None, 0, None, 0
        # drive-level I/O (mode 0 = off): filter histories / delay lines, commands [nenv][nu + 1], measurement block
        self.drive_mode = 0
        self.drive_state = (CmDriveState * nenv)()
        self.drive_cmd = z(pod.nu + 1)
        self.meas = z(56)
        self.pd_dtarget = self.pd_torque = None
        self.envparams = None       # [nenv] cm_envparams_t (a ctypes array), or None: the model's own
        self.settings = {}          # this batch's own settings, on top of the settings() blocks around the call
        self.counters = Counters()  # what this batch's calls reported so far

    def _args(self, nsub, integrate):
        a = StepArgs(model=ctypes.pointer(self.pod), nenv=self.nenv, nsub=nsub, integrate=integrate, drive_mode=self.drive_mode,
                     hfield_stride=self.hfield_stride, nterrain=self.nterrain)
        for f in ("qpos", "qvel", "qacc_warmstart", "time", "ctrl", "qfrc_applied", "xfrc_applied", "qacc", "sensordata", "actuator_velocity",
                  "warn", "info", "xpos", "xquat", "pd_ptarget", "pd_kp", "pd_kd", "drive_state", "drive_cmd", "meas", "pd_dtarget",
                  "pd_torque", "envparams", "hfield", "hfield_index"):
            setattr(a, f, _ptr(getattr(self, f)))
        for kw in [DEFAULTS] + [k for k, _ in _active] + [self.settings]:
            for k, v in kw.items():
                setattr(a.settings, k, v)
        return a

    def _report(self, result):
        for c in [self.counters] + [run for _, run in _active]:
            c.add(result)
        return result

    def _run(self, nsub, integrate):
        result = StepResult()
        rc = lib().emu_phys_run(ctypes.byref(self._args(nsub, integrate)), ctypes.byref(result))
        assert rc == 0
        return self._report(result)

    def derive(self, ids):
        """phys_batch_derive on the emulator: -> (derived [nenv][CM_DRV_DIM], qM [nenv][nv][nv])."""
        from cassie_amd import phys as P
        derived = np.zeros((self.nenv, P.DRV_DIM))
        qM = np.zeros((self.nenv, self.pod.nv, self.pod.nv))
        idarr = np.asarray(ids, dtype=np.int32)
        result = StepResult()
        lib().emu_derive(ctypes.byref(self._args(1, 0)), _ptr(idarr), _ptr(derived), _ptr(qM), ctypes.byref(result))
        self._report(result)
        return derived, qM

    def step(self, nsub=1):
        return self._run(nsub, 1)

    def forward(self):
        return self._run(1, 0)


def pick_family(pod, generic_only=False):
    """ck::pick_family (csrc/step_plan.h) -> the index of the family in ck::StepFamily."""
    return lib().emu_pick_family(ctypes.byref(pod), 1 if generic_only else 0)


def launch_forms(fam, has_inplace=True, maxefc=63, integrate=1, ext=False, n=4096, nsub=50, fast_rows=True, waves_per_env=2,
                 waves_per_env_tray=2, inplace=False):
    """ck::launch_forms (csrc/step_policy.h) -> (first, mid, wide, stay_rows), the forms as indices in ck::StepForm."""
    out = np.zeros(4, dtype=np.int32)
    lib().emu_launch_forms(fam, int(has_inplace), maxefc, integrate, int(ext), n, nsub, int(fast_rows), waves_per_env, waves_per_env_tray,
                           int(inplace), _ptr(out))
    return int(out[0]), int(out[1]), bool(out[2]), int(out[3])


def launch_chunks(n, nenv, nsub, chunks=None):
    """ck::launch_chunks; chunks: what phys_batch_set_chunks was given, None: nobody asked (the defaults)."""
    d = np.zeros(2, dtype=np.int32)
    lib().emu_policy_defaults(_ptr(d))
    whole, rng = (int(d[0]), int(d[1])) if chunks is None else (chunks, chunks)
    return lib().emu_launch_chunks(n, nenv, nsub, whole, rng, 1 if chunks is None else 0)


def pass_grids(n, seen1, seen2, wide):
    """ck::pass_grids -> (mid, wide): the workgroups of the passes that walk the first / the second list."""
    out = np.zeros(3, dtype=np.uint32)
    lib().emu_pass_grids(n, seen1, seen2, int(wide), _ptr(out))
    assert out[0] == n
    return int(out[1]), int(out[2])


def next_inplace(was, seen, mode, auto_ok=True):
    return bool(lib().emu_next_inplace(int(was), seen, mode, int(auto_ok)))


def order_kernel_due(nsub, launches_since_sort):
    return bool(lib().emu_order_kernel_due(nsub, launches_since_sort))


class RangeTable:
    """ck::RangeTable: `records` are lists [env0, n, inplace, launches_since_sort], the caller's to edit between claims."""

    def __init__(self):
        self.records = []

    def claim(self, env0, n):
        """-> (the claimed record: one of self.records, the retired records)"""
        k = len(self.records)
        rec, gone = np.zeros((k + 1, 4), dtype=np.int32), np.zeros((k + 1, 4), dtype=np.int32)
        rec[:k] = np.asarray(self.records, dtype=np.int32).reshape(k, 4)
        nrec, ngone = ctypes.c_int(k), ctypes.c_int(0)
        at = lib().emu_ranges_claim(_ptr(rec), ctypes.addressof(nrec), env0, n, _ptr(gone), ctypes.addressof(ngone))
        kept = {(r[0], r[1]): r for r in self.records}             # (a record that survives stays the same list)
        self.records = [kept.get((int(r[0]), int(r[1])), [int(v) for v in r]) for r in rec[: nrec.value]]
        return self.records[at], [tuple(int(v) for v in g) for g in gone[: ngone.value]]


SCAN, EPISODES, DEPTH, RESET, SET_CONST, PARAM_SCATTER = range(6)      # emu_small_grid's `which`


def small_grid(which, n, width=0, height=0):
    """The workgroups phys_batch.hip launches kernel `which` with over n envs (csrc/small_launch.h: scan_grid, episode_grid, ...)."""
    return lib().emu_small_grid(which, n, width, height)


def depth_geoms(pod, every=False):
    """ck::depth_default_geoms / ck::depth_all_geoms."""
    return lib().emu_depth_geoms(ctypes.byref(pod), int(every))


def depth_scene_kernel(pod, mask, ids_bound=False):
    """ck::depth_scene_kernel: does a depth image of these geoms, with or without a hit-id image bound, take the scene kernel?"""
    return bool(lib().emu_depth_scene_kernel(ctypes.byref(pod), mask, int(ids_bound)))


def _message(m):
    return None if m is None else m.decode()


def scan_check(pod, npoints, body, scan_range, model_stride=0, offsets=True):
    """ck::scan_configure -> the message of its refusal, None where it accepts."""
    off = np.zeros((max(npoints, 1), 2)) if offsets else None
    return _message(lib().emu_scan_check(ctypes.byref(pod), model_stride, _ptr(off), npoints, body, scan_range))


def depth_check(pod, body, width, height, fovy, near, far, cam_quat=(1.0, 0.0, 0.0, 0.0), model_stride=0):
    """ck::depth_configure (fovy in radians) -> the message of its refusal, None where it accepts."""
    pos, quat = np.zeros(3), np.ascontiguousarray(cam_quat, dtype=np.float64)
    return _message(lib().emu_depth_check(ctypes.byref(pod), model_stride, body, _ptr(pos), _ptr(quat), width, height, fovy, near, far))


def depth_geoms_check(pod, mask):
    """ck::check_depth_geoms -> the message of its refusal, None where it accepts."""
    return _message(lib().emu_depth_geoms_check(ctypes.byref(pod), mask))


def set_const(pod, blocks, nenv, mode):
    """phys_batch_set_const on the emulator: the device's set_const kernel on the [nenv] parameter blocks (a ctypes array), in place."""
    assert lib().emu_set_const(ctypes.byref(pod), ctypes.addressof(blocks), nenv, mode) == 0


def end_episodes(state, pod, r, env0, n, restart, bank=None, pick=None, force=None, grid=0, block=None):
    """The emulated episode kernel on `state` (in place); r: the rules, as tests/episode_check.py's dict.  block: a
    [nenv][nq + nv + nsd] array whose column blocks ARE the state's qpos / qvel / sensordata (strided binding); otherwise the three
    are dense."""
    for k, a in state.items():
        assert a is None or a.flags.c_contiguous or block is not None, k
    if block is not None:
        w = block.shape[1]
        qp, qv, sd = block.ctypes.data, block.ctypes.data + 8 * pod.nq, block.ctypes.data + 8 * (pod.nq + pod.nv)
        sq = sqv = ssd = w
    else:
        qp, qv, sd = _ptr(state["qpos"]), _ptr(state["qvel"]), _ptr(state["sensordata"])
        sq, sqv, ssd = pod.nq, pod.nv, pod.nsensordata
    pick = None if pick is None else np.ascontiguousarray(pick, dtype=np.int32)
    force = None if force is None else np.ascontiguousarray(force, dtype=np.int32)
    rules = CmEpisodeRules(min_height=r["min_height"], min_upright=r["min_upright"], max_steps=r["max_steps"],
                           warn_mask=r["warn_mask"], nonfinite=1 if r["nonfinite"] else 0)
    rc = lib().emu_end_episodes(ctypes.byref(pod), ctypes.byref(rules), env0, n, 1 if restart else 0, grid,
                                qp, sq, qv, sqv, sd, ssd, _ptr(state["qacc_warmstart"]), _ptr(state["ctrl"]), _ptr(state["qacc"]), _ptr(state["time"]),
                                _ptr(state["actuator_velocity"]), _ptr(state["meas"]), _ptr(state["drive"]), _ptr(state["warn"]),
                                _ptr(state["done"]), _ptr(state["reason"]), _ptr(state["steps"]), _ptr(state["count"]), _ptr(state["terminal"]),
                                _ptr(bank), 0 if bank is None else bank.shape[0], _ptr(pick), _ptr(force))
    assert rc == 0


def height_scan(pod, qpos, offsets, body, scan_range, blocks=None, hfield=None, stride=0, index=None, nterrain=0, env0=0, n=None, grid=0,
                out=None, warn=None):
    """The emulated scan kernel -> (values [nenv][P], warn [nenv]).  hfield: float32, one grid / nenv grids / a bank; blocks: per-env
    parameter blocks whose geometry the scan reads (the model is then told to, like a batch that has randomised geometry)."""
    nenv, npts = qpos.shape[0], offsets.shape[0]
    n = nenv - env0 if n is None else n
    offsets = np.ascontiguousarray(offsets, dtype=np.float64)
    qpos = np.ascontiguousarray(qpos, dtype=np.float64)
    out = np.full((nenv, npts), np.nan) if out is None else out
    warn = np.zeros(nenv, dtype=np.int32) if warn is None else warn
    model = CmModel.from_buffer_copy(pod)
    model.env_geom = 1 if blocks is not None else 0
    index = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc = lib().emu_height_scan(ctypes.byref(model), _ptr(blocks), env0, n, grid, _ptr(offsets), npts, body, scan_range, _ptr(qpos),
                               qpos.shape[1], _ptr(out), out.shape[1], _ptr(hfield), stride, _ptr(index), nterrain, _ptr(warn))
    assert rc == 0
    return out, warn


def core_safety(n, u, q, w, L, sto, tau, msg):
    """cassie_core_sim's safety layer as the step kernel computes it (csrc/pk_safety.h): n samples, into tau [n][10] and msg [n]."""
    lib().emu_core_safety(n, _ptr(u), _ptr(q), _ptr(w), _ptr(L), _ptr(sto), _ptr(tau), _ptr(msg))
