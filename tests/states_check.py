"""The row of the bank of full states, restated in numpy from the plain per-field arrays (test infrastructure only): what
cassie_state_save_kernel must leave in a slot and what cassie_state_restore_kernel must put back, following a layout
name -> (offset, count, dtype) as Batch.state_layout() / states_emu_py.layout() report it -- nothing here knows the order or the sizes of
the sections.  Also the hand-placed states of the emulator tests (every word distinct) and the snapshot of a batch the GPU tests compare."""
import ctypes

import numpy as np

from cassie_amd import phys as P
from cassie_amd._lib import CmDriveState, CmEnvParams

CORE = ("time", "qpos", "qvel", "qacc_warmstart", "ctrl", "qacc", "sensordata", "actuator_velocity", "meas", "drive_state", "xpos", "xquat", "warn")
FIELD_OF = {"time": P.F_TIME, "qpos": P.F_QPOS, "qvel": P.F_QVEL, "qacc_warmstart": P.F_QACC_WARMSTART, "ctrl": P.F_CTRL, "qacc": P.F_QACC,
            "sensordata": P.F_SENSORDATA, "actuator_velocity": P.F_ACTUATOR_VELOCITY, "meas": P.F_MEAS, "xpos": P.F_XPOS, "xquat": P.F_XQUAT,
            "pd_ptarget": P.F_PD_PTARGET, "pd_kp": P.F_PD_KP, "pd_kd": P.F_PD_KD, "pd_dtarget": P.F_PD_DTARGET, "pd_torque": P.F_PD_TORQUE,
            "drive_cmd": P.F_DRIVE_CMD, "qfrc_applied": P.F_QFRC_APPLIED, "xfrc_applied": P.F_XFRC_APPLIED}


def words(entry, dtype):
    """An env's entry of a section as the int64 words a row holds: the entry's bytes, or the 32-bit value zero-extended."""
    if np.dtype(dtype) == np.int32:
        return np.array([int(entry) & 0xffffffff], dtype=np.int64)
    raw = np.ascontiguousarray(entry).view(np.uint8).reshape(-1)
    assert raw.size % 8 == 0
    return raw.view(np.int64)


def row(layout, row_dim, fields, env):
    """The row a save of `env` leaves: every section's words at its offset, zeros where the batch has no such array, zero padding."""
    r = np.zeros(row_dim, dtype=np.int64)
    for name, (off, count, dt) in layout.items():
        a = fields.get(name)
        if a is None:
            continue
        w = words(a[env], dt)
        assert w.size == count, (name, w.size, count)
        r[off:off + count] = w
    return r


def apply(layout, r, fields, env):
    """What a restore of row `r` into `env` leaves in `fields` (in place): the sections of arrays the batch has, nothing else."""
    for name, (off, count, dt) in layout.items():
        a = fields.get(name)
        if a is None:
            continue
        w = np.ascontiguousarray(r[off:off + count])
        if np.dtype(dt) == np.int32:
            a[env] = np.array([w[0] & 0xffffffff], dtype=np.uint32).view(np.int32)[0]
        else:
            a[env] = w.view(a.dtype).reshape(a[env].shape)


def check_layout(layout, row_dim):
    """Sections start on 16-byte boundaries, are disjoint, and the row dim is the sum of their padded counts."""
    spans = sorted((off, count) for off, count, _ in layout.values())
    at = 0
    for off, count in spans:
        assert off % 2 == 0 and count >= 1, (off, count)
        assert off == at, "a gap or an overlap at word %d (expected %d)" % (off, at)
        at = off + count + (count & 1)
    assert row_dim == at and row_dim % 2 == 0


def section_shapes(pod):
    """name -> (shape of an env's entry, numpy dtype) of every section's per-env array"""
    nq, nv, nu, nsd, nb = pod.nq, pod.nv, pod.nu, pod.nsensordata, pod.nbody
    f, i = np.float64, np.int32
    return {"time": ((1,), f), "qpos": ((nq,), f), "qvel": ((nv,), f), "qacc_warmstart": ((nv,), f), "ctrl": ((nu,), f), "qacc": ((nv,), f),
            "sensordata": ((nsd,), f), "actuator_velocity": ((nu,), f), "meas": ((P.MEAS_DIM,), f),
            "drive_state": ((ctypes.sizeof(CmDriveState),), np.uint8), "xpos": ((3 * nb,), f), "xquat": ((4 * nb,), f), "warn": ((), i),
            "pd_ptarget": ((nu,), f), "pd_kp": ((nu,), f), "pd_kd": ((nu,), f), "pd_dtarget": ((nu,), f), "pd_torque": ((nu,), f),
            "drive_cmd": ((nu + 1,), f), "qfrc_applied": ((nv,), f), "xfrc_applied": ((6 * nb,), f),
            "ep_steps": ((), i), "ep_count": ((), i), "terrain": ((), i), "params": ((ctypes.sizeof(CmEnvParams),), np.uint8)}


def distinct_fields(pod, nenv, names, start=1):
    """Hand-placed arrays [nenv][...] for `names`, every 8-byte word (every int32 value) of every env distinct and non-zero."""
    shapes = section_shapes(pod)
    out, at = {}, start
    for name in names:
        shape, dt = shapes[name]
        if dt == np.int32:
            out[name] = (at + np.arange(nenv)).astype(np.int32)
            at += nenv
            continue
        nwords = int(np.prod(shape)) * np.dtype(dt).itemsize // 8
        w = (at + np.arange(nenv * nwords, dtype=np.int64)).reshape(nenv, nwords)
        at += nenv * nwords
        out[name] = (w.astype(np.float64) * 0.5 if dt == np.float64 else w.view(np.uint8)).reshape((nenv,) + shape).copy()
    return out


def copy_fields(fields):
    return {k: None if v is None else v.copy() for k, v in fields.items()}


def fields_bytes(fields):
    return {k: None if v is None else v.tobytes() for k, v in fields.items()}


def snapshot(b, names=CORE, drive=True):
    """The named sections' arrays of every env of a batch, downloaded: name -> bytes-comparable numpy array [nenv][...] (the drive-level
    state as the bytes of cm_drive_state_t, safety_msg included; drive=False: the batch has no drive mode in use, and the measurement
    block and the drive-level state are None -- asking for the latter would allocate it)."""
    out = {}
    for name in names:
        if name == "warn":
            out[name] = b.warnings()[0].copy()
        elif name == "drive_state":
            out[name] = None
            if drive:
                s = b.get_drive_state()
                out[name] = np.frombuffer(bytes(s), dtype=np.uint8).reshape(b.nenv, ctypes.sizeof(CmDriveState)).copy()
        elif name == "meas":
            out[name] = b.get(P.F_MEAS) if drive else None
        elif name == "params":
            out[name] = np.frombuffer(bytes(b.params()), dtype=np.uint8).reshape(b.nenv, ctypes.sizeof(CmEnvParams)).copy()
        elif name in ("ep_steps", "ep_count"):
            out[name] = b.episodes()[2 if name == "ep_steps" else 3].copy()
        else:
            out[name] = b.get(FIELD_OF[name])
    return out


def assert_equal(got, want, what="", envs=None):
    """tobytes() equality of two snapshots over every env (or `envs`), section by section."""
    assert got.keys() == want.keys()
    for name in got:
        g, w = got[name], want[name]
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        if envs is not None:
            g, w = g[envs], w[envs]
        assert g.tobytes() == w.tobytes(), "%s: section %s differs" % (what, name)
