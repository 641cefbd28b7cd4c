"""ctypes access to tests/emu/emu_sums.cpp -- stepping launches that accumulate the step-sums block (csrc/cm_model.h: CM_SUM_*) on the
CPU wave emulator -- and the numpy reference every step-sums test compares against: the EXISTING one-substep path (sums off, read-out
block on, one substep per launch), summed in substep order.  Test infrastructure only."""
import ctypes

import numpy as np

import emu_py
from cassie_amd import _lib as plib
from cassie_amd import phys as P

CmExt = plib._structs["cm_ext_t"]
_vp, _ci, _ul = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulong


class SumsArgs(ctypes.Structure):
    _fields_ = [("step", emu_py.StepArgs), ("sums", _vp), ("body_cfrc", _vp), ("ext", _vp), ("fast", _ci)]


_ready = False


def lib():
    global _ready
    L = emu_py.lib()
    if not _ready:
        L.emu_sizeof_sums_args.restype, L.emu_offsetof_sums_args.restype = _ul, _ul
        assert ctypes.sizeof(SumsArgs) == L.emu_sizeof_sums_args()
        assert [L.emu_offsetof_sums_args(k) for k in range(4)] == [getattr(SumsArgs, f).offset for f in ("sums", "body_cfrc", "ext", "fast")]
        assert ctypes.sizeof(CmExt) == L.emu_sizeof_ext()
        L.emu_sums_run.argtypes = [ctypes.POINTER(SumsArgs), ctypes.POINTER(emu_py.StepResult)]
        L.emu_sums_layout.argtypes, L.emu_sums_layout.restype = [_vp], None
        L.emu_physio_sums_offsets.argtypes, L.emu_physio_sums_offsets.restype = [_vp], None
        L.emu_launch_forms_sums.argtypes, L.emu_launch_forms_sums.restype = [_ci] * 13 + [_vp], None
        L.emu_step_sums_refuses.argtypes = [_ci] * 6
        lay = np.zeros(11, dtype=np.int32)
        L.emu_sums_layout(lay.ctypes.data)
        # cassie_amd.phys mirrors the header's layout
        assert list(lay) == [P.SUM_COUNT, P.SUM_BODY_CFRC, P.SUM_BODY_TOUCH, P.SUM_BODY_CFRC_MAX2, P.SUM_ACT_FORCE, P.SUM_ACT_FORCE2, P.SUM_ACT_POWER,
                             P.SUM_ACT_POSPOWER, P.SUM_DIM, P.MAXBODY, P.MAXU], lay
        _ready = True
    return L


def launch_forms(fam, has_inplace=True, maxefc=63, integrate=1, ext=False, n=4096, nsub=50, fast_rows=True, waves_per_env=2, waves_per_env_tray=2,
                 inplace=False, prof=False, sums=False):
    """ck::launch_forms (csrc/step_policy.h) with its two trailing arguments -> (first, mid, wide, stay_rows)."""
    out = np.zeros(4, dtype=np.int32)
    lib().emu_launch_forms_sums(fam, int(has_inplace), maxefc, integrate, int(ext), n, nsub, int(fast_rows), waves_per_env, waves_per_env_tray, int(inplace),
                                int(prof), int(sums), out.ctypes.data)
    return tuple(int(v) for v in out)


def step_sums_refuses(form, ext=False, integrate=1, prof=False, sums=False, sums_inst=False):
    return bool(lib().emu_step_sums_refuses(form, int(ext), integrate, int(prof), int(sums), int(sums_inst)))


class SumsBatch(emu_py.EmuBatch):
    """An EmuBatch whose launches go through emu_sums_run: with `accumulate` they zero and fill self.sums; without, they are launches as
    ever that also fill self.body_cfrc and (read_out) self.ext -- the twin."""

    def __init__(self, pod, nenv):
        super().__init__(pod, nenv)
        self.sums = np.full((nenv, P.SUM_DIM), np.nan)          # (a launch must zero its rows itself)
        self.body_cfrc = np.zeros((nenv, pod.nbody, 3))
        self.ext = (CmExt * nenv)()

    def run(self, nsub, accumulate, fast=False, read_out=False, integrate=1):
        lib()
        a = SumsArgs(step=self._args(nsub, integrate), sums=self.sums.ctypes.data if accumulate else None, body_cfrc=self.body_cfrc.ctypes.data,
                     ext=ctypes.addressof(self.ext) if read_out else None, fast=1 if fast else 0)
        result = emu_py.StepResult()
        rc = lib().emu_sums_run(ctypes.byref(a), ctypes.byref(result))
        assert rc == 0, "emu_sums_run refused the launch"
        return self._report(result)


def views(pod, raw):
    """The rows of the block as named views, as cassie_amd.Batch.step_sums returns them."""
    nb, nu = pod.nbody, pod.nu
    per_body = lambda at, w=1: raw[:, at:at + w * P.MAXBODY].reshape(raw.shape[0], P.MAXBODY, w)[:, :nb]
    out = dict(raw=raw, count=raw[:, P.SUM_COUNT], body_cfrc=per_body(P.SUM_BODY_CFRC, 3), body_touch=per_body(P.SUM_BODY_TOUCH)[:, :, 0],
               body_cfrc_max2=per_body(P.SUM_BODY_CFRC_MAX2)[:, :, 0])
    for name, at in (("act_force", P.SUM_ACT_FORCE), ("act_force2", P.SUM_ACT_FORCE2), ("act_power", P.SUM_ACT_POWER), ("act_pospower", P.SUM_ACT_POSPOWER)):
        out[name] = raw[:, at:at + nu]
    return out


class Reference:
    """The sums of the existing one-substep path, in numpy: add() after every one-substep launch of the twin, in substep order."""

    def __init__(self, pod, nenv):
        self.pod = pod
        self.raw = np.zeros((nenv, P.SUM_DIM))
        self.lo = np.array([pod.act_ctrlrange[u][0] for u in range(pod.nu)])
        self.hi = np.array([pod.act_ctrlrange[u][1] for u in range(pod.nu)])
        self.gear = np.array([pod.act_gear[u] for u in range(pod.nu)])
        self.dof = [pod.act_dofid[u] for u in range(pod.nu)]

    def add(self, ctrl, actuator_velocity, body_cfrc, contacts, done=None):
        """ctrl, actuator_velocity [n][nu], body_cfrc [n][nbody][3] as the launch left them; contacts: per env the list of (body1, body2)
        of the substep's contact list; done [n] bool: envs that take no part any more (None: all do)."""
        v = views(self.pod, self.raw)
        n, nb = self.raw.shape[0], self.pod.nbody
        F = np.clip(ctrl, self.lo, self.hi)
        F2 = F * F
        pw = F * actuator_velocity
        pp = np.maximum(pw, 0.0)
        cf = np.asarray(body_cfrc).reshape(n, nb, 3)
        m2 = (cf[:, :, 0] * cf[:, :, 0] + cf[:, :, 1] * cf[:, :, 1]) + cf[:, :, 2] * cf[:, :, 2]
        for e in range(n):
            if done is not None and done[e]:
                continue
            v["count"][e] += 1.0
            v["body_cfrc"][e] += cf[e]
            for b in set(b for pair in contacts[e] for b in pair):
                v["body_touch"][e, b] += 1.0
            v["body_cfrc_max2"][e] = np.maximum(v["body_cfrc_max2"][e], m2[e])
            v["act_force"][e] += F[e]
            v["act_force2"][e] += F2[e]
            v["act_power"][e] += pw[e]
            v["act_pospower"][e] += pp[e]


def ext_contacts(ext, nenv):
    """Per env the (body1, body2) pairs of the read-out block's contact list."""
    return [[(ext[e].con_body1[c], ext[e].con_body2[c]) for c in range(ext[e].ncon)] for e in range(nenv)]


BITWISE = ("count", "body_cfrc", "body_touch", "act_force", "act_force2", "act_power", "act_pospower")


def compare(pod, got_raw, ref_raw, label=""):
    """The issue's comparison: everything bitwise but the largest squared force, which takes three roundings the device may fuse (1e-14 relative)."""
    got, ref = views(pod, np.ascontiguousarray(got_raw)), views(pod, ref_raw)
    for k in BITWISE:
        assert got[k].tobytes() == ref[k].tobytes(), (label, k, np.abs(got[k] - ref[k]).max())
    assert np.allclose(got["body_cfrc_max2"], ref["body_cfrc_max2"], rtol=1e-14, atol=0.0), (label, "body_cfrc_max2")
    # entries past the model's nbody / nu stay 0
    mask = np.ones(P.SUM_DIM, dtype=bool)
    for at, w, used in ((P.SUM_BODY_CFRC, 3, pod.nbody), (P.SUM_BODY_TOUCH, 1, pod.nbody), (P.SUM_BODY_CFRC_MAX2, 1, pod.nbody)):
        mask[at:at + w * used] = False
    for at in (P.SUM_ACT_FORCE, P.SUM_ACT_FORCE2, P.SUM_ACT_POWER, P.SUM_ACT_POSPOWER):
        mask[at:at + pod.nu] = False
    mask[P.SUM_COUNT] = False
    assert not np.asarray(got_raw)[:, mask].any(), (label, "entries past nbody / nu")
