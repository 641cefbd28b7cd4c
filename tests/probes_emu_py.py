"""ctypes access to the probe kernel on the CPU wave emulator (tests/emu/emu_probes.cpp) -- test infrastructure only.  The library is the
one tests/emu_py.py loads; this module declares the entry points emu_probes.cpp adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import _lib as plib
from cassie_amd import phys as P
from cassie_amd._lib import CmModel

CmExt = plib._structs["cm_ext_t"]
_vp, _ci, _cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
_declared = False
PROBE_GRID = None          # ck::PROBE_GRID, once the library is loaded (lib())
NAMES = tuple(name for name, _ in P.PQ_ROW)


def lib():
    global _declared, PROBE_GRID
    L = emu_py.lib()
    if not _declared:
        L.emu_probe_last_refusal.restype = ctypes.c_char_p
        L.emu_probe_constants.argtypes, L.emu_probe_constants.restype = [_vp], None
        L.emu_probe_grid.argtypes = [_ci]
        L.emu_probe_layout.argtypes = [_ci, _cu, _ci, _vp, _vp]
        L.emu_probe_check.argtypes, L.emu_probe_check.restype = [ctypes.POINTER(CmModel), _vp, _ci, _cu, _vp], ctypes.c_char_p
        L.emu_probe_call_check.argtypes, L.emu_probe_call_check.restype = [_ci] * 4, ctypes.c_char_p
        L.emu_probe_classify.argtypes, L.emu_probe_classify.restype = [_vp, _ci, _vp, _ci, _vp], None
        L.emu_probe_record.argtypes, L.emu_probe_record.restype = [ctypes.POINTER(CmModel), _ci, _cu] + [_ci] * 8 + [_vp, _vp], None
        L.emu_probe.argtypes = [ctypes.POINTER(emu_py.StepArgs), _ci, _ci, _ci, _vp, _ci, _cu, _vp, _ci, _vp, _ci, _vp, _ci, _vp,
                                ctypes.POINTER(emu_py.StepResult)]
        L.emu_probe_reduce.argtypes = [ctypes.POINTER(CmModel), _ci, _ci, _ci, _ci, _vp, _ci, _cu, _vp, _ci, _vp, _ci] + [_vp] * 7 + [_ci, _vp]
        c = np.zeros(6, dtype=np.int64)
        L.emu_probe_constants(c.ctypes.data)
        assert (int(c[1]), int(c[2]), int(c[3])) == (P.PROBES_MAX, P.PROBE_DTYPE.itemsize, len(P.PQ_ROW)) and int(c[5]) == ctypes.sizeof(CmExt)
        PROBE_GRID = int(c[0])
        _declared = True
    return L


def table_of(probes):
    """A list of (kind, id, offset) or a structured array -> PROBE_DTYPE entries, as Batch.configure_probes makes them."""
    if isinstance(probes, np.ndarray) and probes.dtype.names:
        return np.ascontiguousarray(probes.astype(P.PROBE_DTYPE, copy=False)).reshape(-1)
    probes = list(probes)
    table = np.zeros(len(probes), dtype=P.PROBE_DTYPE)
    for k, (kind, ident, offset) in enumerate(probes):
        table[k] = (int(kind), int(ident), np.asarray(offset, dtype=np.float64))
    return table


def grid(n):
    """ck::probe_grid."""
    return lib().emu_probe_grid(n)


def layout(nprobes, quantities, nv):
    """ck::probe_layout -> (row length, offsets [PQ_COUNT], dims [PQ_COUNT])."""
    off, dims = np.zeros(len(P.PQ_ROW), dtype=np.int32), np.zeros(len(P.PQ_ROW), dtype=np.int32)
    row = lib().emu_probe_layout(nprobes, quantities, nv, off.ctypes.data, dims.ctypes.data)
    return row, [int(v) for v in off], [int(v) for v in dims]


def check(pod, probes, quantities, nprobes=None):
    """ck::probes_configure -> the message of its refusal, None where it accepts (nprobes: what the caller claims, default: all)."""
    table = table_of(probes)
    cfg = np.zeros(2, dtype=np.int64)
    n = table.size if nprobes is None else nprobes
    why = lib().emu_probe_check(ctypes.byref(pod), table.ctypes.data if table.size else None, n, quantities, cfg.ctypes.data)
    if why is None and n > 0:
        assert (int(cfg[0]), int(cfg[1])) == (n, quantities)
    return None if why is None else why.decode()


def call_check(configured, nenv, env0, n):
    """ck::check_probe_call -> the message of its refusal, None where it accepts."""
    why = lib().emu_probe_call_check(int(configured), nenv, env0, n)
    return None if why is None else why.decode()


def classify(geom_user, nuser_geom, geom_group):
    """ck::probe_classify_geoms -> the table [ngeom] (int32)."""
    group = np.ascontiguousarray(geom_group, dtype=np.int32)
    user = None if geom_user is None else np.ascontiguousarray(geom_user, dtype=np.float64)
    table = np.zeros(group.size, dtype=np.int32)
    lib().emu_probe_classify(emu_py._ptr(user), nuser_geom, group.ctypes.data, group.size, table.ctypes.data)
    return table


def record(pod, nprobes, quantities, sout, sq, sqv, env0, n, classes=True, ngeom=0, contacts=True):
    """What ck::make_probe_io makes of a configuration and an env range -> (dict of the record's integer fields, the offsets)."""
    ints, off = np.zeros(14, dtype=np.int64), np.zeros(len(P.PQ_ROW), dtype=np.int32)
    lib().emu_probe_record(ctypes.byref(pod), nprobes, quantities, sout, sq, sqv, env0, n, int(classes), ngeom, int(contacts), ints.ctypes.data, off.ctypes.data)
    names = ("env0", "n", "nprobes", "quantities", "sout", "sxp", "sxq", "sq", "sqv", "sv", "row_dim", "classes", "ngeom", "contacts")
    return dict(zip(names, (int(v) for v in ints))), [int(v) for v in off]


def geom_classes(model):
    """(geom_user [ngeom][nuser_geom] or None, nuser_geom, geom_group [ngeom]) of a cassie_amd.Model's full geom list: what
    phys_batch_probe_geom_classes reads of the host model."""
    L = plib.lib()
    ngeom, nug = model.size(P.SIZE_NGEOM), model.size(16)      # PHYS_NGEOM, PHYS_NUSER_GEOM
    group = np.ctypeslib.as_array(L.phys_model_iarray(model._h, 4), shape=(ngeom,)).astype(np.int32)   # PHYS_MI_GEOM_GROUP
    user = model.array(P.M_GEOM_USER, ngeom * nug).copy() if nug >= 1 else None
    return user, nug, group


def split(rows, nprobes, quantities, nv):
    """Rows [n][>= row length] -> {name: [n][nprobes][*shape]} of the quantities in the mask."""
    _, off, dims = layout(nprobes, quantities, nv)
    out = {}
    for k, (name, shape) in enumerate(P.PQ_ROW):
        if off[k] >= 0:
            shape = tuple(nv if d == "nv" else d for d in shape)
            out[name] = rows[:, off[k]: off[k] + nprobes * dims[k]].reshape((rows.shape[0], nprobes) + shape)
    return out


def probe(emu, probes, quantities, classes=None, env0=0, n=None, grid=0, out=None, contacts=None):
    """phys_batch_probe on the emulator for an EmuBatch -> ({name: array} of the whole batch's rows, the contact words [nenv], the raw
    rows).  classes: geom_classes(model), None: no contact word is written.  out / contacts: pre-filled arrays to write into."""
    pod, nenv = emu.pod, emu.nenv
    table = table_of(probes)
    n = nenv - env0 if n is None else n
    row, _, _ = layout(table.size, quantities, pod.nv)
    out = np.full((nenv, max(row, 1)), np.nan) if out is None else out
    contacts = np.full(nenv, -1, dtype=np.int32) if contacts is None else contacts
    user, nug, group = classes if classes is not None else (None, 0, None)
    result = emu_py.StepResult()
    rc = lib().emu_probe(ctypes.byref(emu._args(1, 0)), env0, n, grid, table.ctypes.data, table.size, quantities, emu_py._ptr(user), nug,
                         emu_py._ptr(group), 0 if group is None else group.size, out.ctypes.data, out.shape[1], contacts.ctypes.data, ctypes.byref(result))
    assert rc == 0, (lib().emu_probe_last_refusal() or b"").decode()
    emu._report(result)
    return split(out, table.size, quantities, pod.nv), contacts, out


def reduce(pod, probes, quantities, ext, xpos, xquat, qpos, qvel, qacc, classes=None, env0=0, n=None, grid=0):
    """cassie_probe_kernel alone on hand-made read-out blocks: ext a (CmExt * nenv) array, the others [nenv] dense rows
    -> ({name: array}, the contact words [nenv])."""
    table = table_of(probes)
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (xpos, xquat, qpos, qvel, qacc)]
    nenv = arrs[2].shape[0]
    n = nenv - env0 if n is None else n
    row, _, _ = layout(table.size, quantities, pod.nv)
    out = np.full((nenv, max(row, 1)), np.nan)
    contacts = np.full(nenv, -1, dtype=np.int32)
    user, nug, group = classes if classes is not None else (None, 0, None)
    rc = lib().emu_probe_reduce(ctypes.byref(pod), nenv, env0, n, grid, table.ctypes.data, table.size, quantities, emu_py._ptr(user), nug,
                                emu_py._ptr(group), 0 if group is None else group.size, ctypes.addressof(ext), *[a.ctypes.data for a in arrs],
                                out.ctypes.data, out.shape[1], contacts.ctypes.data)
    assert rc == 0, (lib().emu_probe_last_refusal() or b"").decode()
    return split(out, table.size, quantities, pod.nv), contacts
