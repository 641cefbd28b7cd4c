"""ctypes access to phys_batch_end_episodes with placed restarts on the CPU wave emulator (tests/emu/emu_placement.cpp) -- test
infrastructure only.  The library is the one tests/emu_py.py loads; this module declares the entry points it adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd._lib import CmEpisodeRules, CmModel

_vp, _ci, _cd, _ul = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_ulong
_declared = False


class PlaceArgs(ctypes.Structure):
    """emu_place_args of tests/emu/emu_placement.cpp."""
    _fields_ = [("model", ctypes.POINTER(CmModel)), ("rules", ctypes.POINTER(CmEpisodeRules))] + \
               [(f, _ci) for f in ("env0", "n", "restart", "grid", "sq", "sqv", "ssd", "nrows")] + \
               [(f, _vp) for f in ("qpos", "qvel", "sensordata", "qacc_warmstart", "ctrl", "qacc", "time", "actuator_velocity", "meas", "drive",
                                   "warn", "done", "reason", "steps", "count", "terminal", "bank", "pick", "force")] + \
               [("anchor", _ci), ("npoints", _ci), ("ground_ref", _cd)] + \
               [(f, _vp) for f in ("offsets", "pose", "next", "ground", "envparams", "hfield")] + \
               [("hfield_stride", _ul), ("hfield_index", _vp), ("nterrain", _ci)]


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        L.emu_place_sizeof.restype = _ul
        assert L.emu_place_sizeof() == ctypes.sizeof(PlaceArgs)
        L.emu_place_end_episodes.argtypes = [ctypes.POINTER(PlaceArgs), ctypes.POINTER(ctypes.c_char_p)]
        _declared = True
    return L


def end_episodes(state, pod, r, env0, n, restart, bank, anchor, pose, ground, footprint=None, ground_ref=0.0, nxt=None, pick=None, force=None,
                 grid=0, block=None, blocks=None, hfield=None, stride=0, index=None, nterrain=0, expect_error=False):
    """The emulated placed episode kernel on `state` (in place; tests/emu_py.end_episodes's conventions for state, r, block).  pose
    [nenv][4] and ground [nenv] are PHYS_PLACE_POSE / PHYS_PLACE_GROUND (ground is written), nxt [nenv] int32 the next terrains or None,
    footprint [P][2] or None; blocks: per-env parameter blocks whose geometry the surface reads (the model is then told to, like a batch
    that has randomised geometry); hfield / stride / index / nterrain as emu_py.height_scan's -- index is written where nxt is given.
    expect_error: -> the message with which the configure call would fail (nothing is run)."""
    _ptr = emu_py._ptr
    for k, a in state.items():
        assert a is None or a.flags.c_contiguous or block is not None, k
    if block is not None:
        qp, qv, sd = block.ctypes.data, block.ctypes.data + 8 * pod.nq, block.ctypes.data + 8 * (pod.nq + pod.nv)
        sq = sqv = ssd = block.shape[1]
    else:
        qp, qv, sd = _ptr(state["qpos"]), _ptr(state["qvel"]), _ptr(state["sensordata"])
        sq, sqv, ssd = pod.nq, pod.nv, pod.nsensordata
    pick = None if pick is None else np.ascontiguousarray(pick, dtype=np.int32)
    force = None if force is None else np.ascontiguousarray(force, dtype=np.int32)
    footprint = None if footprint is None or len(footprint) == 0 else np.ascontiguousarray(footprint, dtype=np.float64)
    assert pose.dtype == np.float64 and pose.flags.c_contiguous and ground.dtype == np.float64
    assert nxt is None or (nxt.dtype == np.int32 and index is not None and index.dtype == np.int32)
    rules = CmEpisodeRules(min_height=r["min_height"], min_upright=r["min_upright"], max_steps=r["max_steps"],
                           warn_mask=r["warn_mask"], nonfinite=1 if r["nonfinite"] else 0)
    model = CmModel.from_buffer_copy(pod)
    model.env_geom = 1 if blocks is not None else 0
    a = PlaceArgs(model=ctypes.pointer(model), rules=ctypes.pointer(rules), env0=env0, n=n, restart=1 if restart else 0, grid=grid,
                  sq=sq, sqv=sqv, ssd=ssd, nrows=0 if bank is None else bank.shape[0],
                  qpos=qp, qvel=qv, sensordata=sd, anchor=anchor, npoints=0 if footprint is None else footprint.shape[0],
                  ground_ref=float(ground_ref), hfield_stride=stride, nterrain=nterrain)
    for f, v in (("qacc_warmstart", state["qacc_warmstart"]), ("ctrl", state["ctrl"]), ("qacc", state["qacc"]), ("time", state["time"]),
                 ("actuator_velocity", state["actuator_velocity"]), ("meas", state["meas"]), ("drive", state["drive"]), ("warn", state["warn"]),
                 ("done", state["done"]), ("reason", state["reason"]), ("steps", state["steps"]), ("count", state["count"]),
                 ("terminal", state["terminal"]), ("bank", bank), ("pick", pick), ("force", force), ("offsets", footprint), ("pose", pose),
                 ("next", nxt), ("ground", ground), ("envparams", blocks), ("hfield", hfield), ("hfield_index", index)):
        setattr(a, f, _ptr(v))
    why = ctypes.c_char_p()
    rc = lib().emu_place_end_episodes(ctypes.byref(a), ctypes.byref(why))
    if expect_error:
        assert rc == -1
        return (why.value or b"").decode()
    assert rc == 0, (why.value or b"").decode()
