"""ctypes access to the bodies of tests/device/wave_bodies.h on either backend -- test infrastructure only.

    WaveCheck("emu")     the CPU wave emulator (tests/emu/libcassie_emu.so)
    WaveCheck("device")  the gfx950 build (tests/device/libwave_check.so), one workgroup of one wave per trial

run(name, inputs) takes the inputs as [ntrial][nin][64] (or [nin][64] for one trial) and returns the outputs as
[ntrial][nout][64] (or [nout][64]), float64 throughout."""
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

    def run(self, name, inputs):
        nin, nout = self.shape(name)
        x = np.ascontiguousarray(inputs, dtype=np.float64)
        single = x.ndim == 2
        if single:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (nin, 64):
            raise ValueError("%s takes [ntrial][%d][64] inputs, got %s" % (name, nin, x.shape))
        out = np.empty((x.shape[0], nout, 64))
        f = getattr(self.lib, "wc_" + name)
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        err = f(x.ctypes.data, out.ctypes.data, x.shape[0])
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
