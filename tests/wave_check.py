"""ctypes access to the bodies of tests/device/wave_bodies.h on either backend -- test infrastructure only.

    WaveCheck("emu")     the CPU wave emulator (tests/emu/libcassie_emu.so)
    WaveCheck("device")  the gfx950 build (tests/device/libwave_check.so), one workgroup of one wave per trial

run(name, inputs) takes the inputs as [ntrial][nin][64] (or [nin][64] for one trial) and returns the outputs as
[ntrial][nout][64] (or [nout][64]), float64 throughout.  A body that reads an auxiliary block (the factor_* bodies: a model and the
step, factor_aux) takes it as `aux`: bytes every trial of the call shares.  Outputs a body does not write come back NaN."""
import ctypes
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"emu": os.path.join(REPO, "tests", "emu", "libcassie_emu.so"),
        "device": os.path.join(REPO, "tests", "device", "libwave_check.so")}


class WaveCheck:
    def __init__(self, backend):
        self.backend = backend
        self.lib = ctypes.CDLL(LIBS[backend])
        self.lib.wc_shape.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]

    def shape(self, name):
        nin, nout = ctypes.c_int(), ctypes.c_int()
        if self.lib.wc_shape(name.encode(), ctypes.byref(nin), ctypes.byref(nout)) != 0:
            raise KeyError(name)
        return nin.value, nout.value

    def factor_aux(self, pod, h):
        """The auxiliary block of the factor_* bodies: a copy of the model `pod` (a CmModel: nv, dof_ancmask, dof_armature and
        params.dof_damping are read) followed by the step h."""
        from cassie_amd._lib import CmModel
        self.lib.wc_sizeof_factor_aux.restype = self.lib.wc_offsetof_factor_aux_h.restype = ctypes.c_ulong
        size, at = self.lib.wc_sizeof_factor_aux(), self.lib.wc_offsetof_factor_aux_h()
        assert at >= ctypes.sizeof(CmModel) and size >= at + 8
        buf = ctypes.create_string_buffer(size)
        ctypes.memmove(buf, ctypes.byref(pod), ctypes.sizeof(CmModel))
        ctypes.c_double.from_buffer(buf, at).value = h
        return buf

    def tree(self, which):
        """A dof tree the bodies are instantiated for (0: run-time at 40 dofs, 1: Cassie-32, 2: the packed tray model): the padded
        size, nv and the ancestor masks (0 and None for the run-time tree: the model's own), the words of a packed factor and
        slot[k][i] of entry (k, i) in it (-1 where the row keeps none)."""
        nvp, nv, count = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if self.lib.wc_tree_size(which, ctypes.byref(nvp), ctypes.byref(nv), ctypes.byref(count)) != 0:
            raise KeyError(which)
        self.lib.wc_tree_mask.restype = ctypes.c_ulonglong
        n = nvp.value
        mask = [int(self.lib.wc_tree_mask(which, k)) for k in range(n)] if which else None
        slot = np.array([[self.lib.wc_tree_slot(which, k, i) for i in range(n)] for k in range(n)])
        return n, nv.value, mask, count.value, slot

    def run(self, name, inputs, aux=None):
        nin, nout = self.shape(name)
        x = np.ascontiguousarray(inputs, dtype=np.float64)
        single = x.ndim == 2
        if single:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (nin, 64):
            raise ValueError("%s takes [ntrial][%d][64] inputs, got %s" % (name, nin, x.shape))
        out = np.full((x.shape[0], nout, 64), np.nan)
        f = getattr(self.lib, "wc_" + name)
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + ([] if aux is None else [ctypes.c_void_p, ctypes.c_ulong])
        err = f(x.ctypes.data, out.ctypes.data, x.shape[0], *(() if aux is None else (ctypes.addressof(aux), ctypes.sizeof(aux))))
        if err != 0:
            raise RuntimeError("wc_%s on the %s failed: HIP error %d" % (name, self.backend, err))
        return out[0] if single else out

    def lanes(self, name, values, fill=1.0):
        """Independent per-lane work: values [nin][n] (or [n] for one input) spread over as many trials as they need,
        the last one padded with `fill`; returns the outputs as [nout][n]."""
        v = np.atleast_2d(np.asarray(values, dtype=np.float64))
        n = v.shape[1]
        v = np.concatenate([v, np.full((v.shape[0], -n % 64), fill)], axis=1)
        out = self.run(name, v.reshape(v.shape[0], -1, 64).transpose(1, 0, 2))
        return out.transpose(1, 0, 2).reshape(out.shape[1], -1)[:, :n]
