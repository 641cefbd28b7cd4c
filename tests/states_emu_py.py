"""ctypes access to the bank of full states on the CPU wave emulator (tests/emu/emu_states.cpp) -- test infrastructure only.  The
library is the one tests/emu_py.py loads; this module declares the entry points it adds."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import phys as P
from cassie_amd._lib import CmModel

_vp, _ci, _ul = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong
NSECT = len(P.STATE_SECTIONS)
NAMES = tuple(name for name, _ in P.STATE_SECTIONS)
_declared = False


class StateArgs(ctypes.Structure):
    """emu_state_args of tests/emu/emu_states.cpp."""
    _fields_ = [("model", ctypes.POINTER(CmModel))] + \
               [(f, _ci) for f in ("nenv", "env0", "n", "grid", "nslots", "groups", "sq", "sqv", "ssd", "nterrain")] + \
               [("env", _vp * NSECT), ("bank", _vp), ("slots", _vp)]


def lib():
    global _declared
    L = emu_py.lib()
    if not _declared:
        L.emu_state_sizeof.restype = _ul
        assert L.emu_state_sizeof() == ctypes.sizeof(StateArgs)
        assert L.emu_state_nsections() == NSECT
        L.emu_state_layout.argtypes = [_ci] * 6 + [_vp]
        L.emu_state_signature.argtypes, L.emu_state_signature.restype = [ctypes.POINTER(CmModel), _ci], ctypes.c_ulonglong
        L.emu_state_configure.argtypes, L.emu_state_configure.restype = [ctypes.POINTER(StateArgs)], ctypes.c_char_p
        L.emu_state_call.argtypes = [ctypes.POINTER(StateArgs), _ci, ctypes.POINTER(ctypes.c_char_p)]
        _declared = True
    return L


def layout(pod, groups):
    """(name -> (offset, count, dtype), row_dim) for the model's sizes and these groups: ck::state_layout, as Batch.state_layout()
    reports it for a configured batch."""
    return layout_of_sizes(pod.nq, pod.nv, pod.nu, pod.nsensordata, pod.nbody, groups)


def layout_of_sizes(nq, nv, nu, nsd, nbody, groups):
    oc = np.zeros((NSECT, 2), dtype=np.int32)
    row_dim = lib().emu_state_layout(nq, nv, nu, nsd, nbody, groups, oc.ctypes.data)
    return {name: (int(oc[s, 0]), int(oc[s, 1]), dt) for s, (name, dt) in enumerate(P.STATE_SECTIONS) if oc[s, 0] >= 0}, row_dim


def grid(n):
    return lib().emu_state_grid(n)


def signature(pod, groups):
    return int(lib().emu_state_signature(ctypes.byref(pod), groups))


def section_bytes():
    """sizeof(cm_drive_state_t), sizeof(cm_envparams_t)"""
    return lib().emu_state_section_bytes(0), lib().emu_state_section_bytes(1)


def _args(pod, arrays, bank, groups, env0, n, slots, nslots, grid, block, nterrain, nenv):
    """arrays: name -> numpy array [nenv][...] (or None / missing: the batch has none); block: an [nenv][W] float64 array whose columns
    hold qpos | qvel | sensordata (the arrays' entries of those names are then ignored)."""
    a = StateArgs(model=ctypes.pointer(CmModel.from_buffer_copy(pod)), nenv=nenv, env0=env0, n=n, grid=grid,
                  nslots=nslots, groups=groups, sq=pod.nq, sqv=pod.nv, ssd=pod.nsensordata, nterrain=nterrain)
    for s, name in enumerate(NAMES):
        v = arrays.get(name)
        assert v is None or v.flags.c_contiguous, name
        a.env[s] = emu_py._ptr(v)
    if block is not None:
        a.sq = a.sqv = a.ssd = block.shape[1]
        a.env[NAMES.index("qpos")] = block.ctypes.data
        a.env[NAMES.index("qvel")] = block.ctypes.data + 8 * pod.nq
        a.env[NAMES.index("sensordata")] = block.ctypes.data + 8 * (pod.nq + pod.nv)
    a.bank = emu_py._ptr(bank)
    a.slots = emu_py._ptr(slots)
    return a


def call(pod, arrays, bank, restore, groups=P.STATE_CORE, env0=0, n=None, slots=None, nslots=None, grid=0, block=None, nterrain=0,
         nenv=None, expect_error=False):
    """The emulated save (restore False) or restore kernel on `arrays` / `bank` (int64 [nslots][row_dim]) in place, checked and launched
    as phys_batch_state_save / _restore.  slots: int32 [n] or None.  expect_error: -> the refusal's message (nothing is run)."""
    nenv = arrays["time"].shape[0] if nenv is None else nenv
    n = nenv - env0 if n is None else n
    assert bank is None or (bank.dtype == np.int64 and bank.flags.c_contiguous)
    slots = None if slots is None else np.ascontiguousarray(slots, dtype=np.int32)
    ns = nslots if nslots is not None else 0 if bank is None else bank.shape[0]
    a = _args(pod, arrays, bank, groups, env0, n, slots, ns, grid, block, nterrain, nenv)
    why = ctypes.c_char_p()
    rc = lib().emu_state_call(ctypes.byref(a), 1 if restore else 0, ctypes.byref(why))
    if expect_error:
        assert rc == -1
        return (why.value or b"").decode()
    assert rc == 0, (why.value or b"").decode()


def configure_refusal(pod, arrays, nslots, groups, nterrain=0):
    """What phys_batch_state_configure answers for a batch that has `arrays` ('' : fine)."""
    a = _args(pod, arrays, None, groups, 0, 0, None, nslots, 0, None, nterrain, 1)
    return (lib().emu_state_configure(ctypes.byref(a)) or b"").decode()
