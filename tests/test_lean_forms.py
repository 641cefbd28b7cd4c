"""The lean fast forms of the step kernel (csrc/pk_stages.h: FEAT_READOUT / FEAT_PROF; csrc/step_plan.h: is_lean_form) on the CPU: the
emulator runs the same template, so a lean fast form + the pass behind it must leave the bytes the generic kernel alone leaves, the
profiled form the bytes of the lean one; and the launcher's policy (csrc/step_policy.h) never hands a lean form a launch it has no
code for -- launch_forms by its answers, lean_form_refuses as the launcher's last check."""
import ctypes
import itertools

import numpy as np
import pytest

import emu_py
from emu_py import EmuBatch

# ck::StepForm / ck::StepFamily (csrc/step_plan.h)
(FORM_ALONE, FORM_ALONE_2W, FORM_WIDE, FORM_FAST, FORM_FAST_2W, FORM_FAST_INPLACE, FORM_MID_WALK, FORM_MID_WALK_2W, FORM_WIDE_WALK,
 FORM_FAST_PROF, FORM_FAST_2W_PROF) = range(11)
CASSIE, CASSIE_HFIELD, CASSIE_ALL, TRAY, TRAY_HFIELD, GENERIC32, GENERIC40 = range(7)
LEAN = (FORM_FAST, FORM_FAST_2W, FORM_FAST_INPLACE)
PROF = (FORM_FAST_PROF, FORM_FAST_2W_PROF)


def _lib():
    L = emu_py.lib()
    L.emu_phys_run_lean.argtypes = [ctypes.POINTER(emu_py.StepArgs), ctypes.POINTER(emu_py.StepResult), ctypes.c_void_p]
    L.emu_launch_forms_prof.argtypes, L.emu_launch_forms_prof.restype = [ctypes.c_int] * 12 + [ctypes.c_void_p], None
    L.emu_form_kinds.argtypes, L.emu_form_kinds.restype = [ctypes.c_void_p], None
    return L


class LeanEmuBatch(EmuBatch):
    """An EmuBatch whose stepping launches with fast_rows set take the LEAN fast forms (tests/emu/emu_lean.cpp; EmuBatch's own fast
    bodies carry both feature bits); every other call is EmuBatch's."""
    profiled = False

    def __init__(self, pod, nenv):
        super().__init__(pod, nenv)
        self.stamps = np.zeros((nenv, _lib().emu_nstamp()), dtype=np.int64)

    def _run(self, nsub, integrate):
        args = self._args(nsub, integrate)
        if not (integrate and args.settings.fast_rows):
            return super()._run(nsub, integrate)
        result = emu_py.StepResult()
        self.stamps[:] = -1     # (the emulator's clocks read 0: a slot the kernel stamped is a cleared slot)
        rc = _lib().emu_phys_run_lean(ctypes.byref(args), ctypes.byref(result), self.stamps.ctypes.data if self.profiled else None)
        assert rc == 0
        return self._report(result)


class ProfiledEmuBatch(LeanEmuBatch):
    """... with the stage stamps on (PhysIO::prof): the fast forms' _PROF instantiations."""
    profiled = True


NENV, NSUB, NLAUNCH = 4, 12, 2
# how far below its initial height each model's pelvis starts: the envs land within the first launch -- which so starts in the fast code
# and ends above its rows -- and the second launch's last substep fits the fast code again (the tray model: see the test)
DROP = {"cassie": 0.06, "cassie_hfield": 0.16, "cassie_tray_box": 0.03}


def _workload(model, settings, batch=LeanEmuBatch, before_launch=None):
    """NLAUNCH fused launches of NSUB substeps over NENV envs of the benchmark's drive-level PD workload, the first with the benchmark's
    targets and the others with the +-10 rad stress targets (rows past the fast code's: hand-overs, the in-place code) -> everything a launch leaves behind as bytes, the solver
    statistics [launch][env][4], the batch."""
    import bench
    from cassie_amd import phys as P
    from hostchain_py import device_state_bytes
    pod = model.pod
    with emu_py.settings(**settings):
        emu = batch(pod, NENV)
        emu.qpos[:] = model.qpos_init()
        emu.qpos[:, 2] -= DROP[model.name]
        if pod.nhfpair > 0:
            import test_hfield
            emu.hfield = test_hfield.terrain()
        emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (NENV, 1)), np.tile(bench.PD_KD, (NENV, 1))
        emu.forward()
        emu.drive_mode = P.DRIVE_PD
        rows = []
        for p in range(NLAUNCH):
            amp = 0.3 if p == 0 else 10.0       # (the first launch stays in the fast code, the stress targets behind it leave it)
            emu.pd_ptarget = np.array([bench.PD_OFFSET + np.random.default_rng(977 + 31 * p + e).uniform(-amp, amp, 10) for e in range(NENV)])
            if before_launch:
                before_launch(p)
            emu.step(NSUB)
            rows.append(emu.info.copy())
    rows = np.array(rows)
    state = {f: getattr(emu, f).tobytes() for f in ("qpos", "qvel", "qacc_warmstart", "qacc", "sensordata", "actuator_velocity", "ctrl", "meas", "warn",
                                                     "time", "xpos", "xquat")}
    state["info"] = rows.tobytes()
    state["drive_state"] = [device_state_bytes(emu.drive_state[e]) for e in range(NENV)]
    return state, rows, emu


def _same(got, ref, what):
    for f in ref:
        assert got[f] == ref[f], (what, f)


@pytest.mark.parametrize("name", ["cassie", "cassie_hfield", "cassie_tray_box"])
def test_lean_fast_forms_leave_the_bytes_of_the_generic_kernel_alone(name, built):
    from cassie_amd import Model
    model = Model(name)
    tray = name == "cassie_tray_box"
    fast_rows, hook = 31, None
    if tray:
        # (the stress targets alone do not take this model past the 47 rows of its fast code: from the second launch on every limited
        # joint is inside its limit's margin -- 16 more rows, as tests/test_emu_parity.py has it -- so that the first launch stays in
        # the fast code and the later ones are handed over)
        fast_rows, margins = 47, [model.pod.jnt_margin[j] for j in range(model.pod.njnt)]

        def hook(p):
            for j in range(model.pod.njnt):
                model.pod.jnt_margin[j] = 10.0 if p > 0 and model.pod.jnt_limited[j] else margins[j]
    ref, rows, _ = _workload(model, dict(fast_rows=0), before_launch=hook)
    assert rows[:, :, 1].max() > fast_rows and rows[:, :, 1].min() <= fast_rows, "the workload must cross the fast code's row count"
    # the lean forms: one wave + the pass behind it, two waves + the list-walking pass, the in-place form (which stays in the 63-row code
    # until a substep fits the fast code again, as the launcher has it)
    forms = [dict(fast_rows=1), dict(fast_rows=1, two_waves=1, wave_schedule=1)]
    if not tray:
        forms += [dict(fast_rows=1, two_waves=1, inplace=1, inplace_stay_rows=27, wave_schedule=2)]
    for i, s in enumerate(forms):
        got, _, emu = _workload(model, s, before_launch=hook)
        _same(got, ref, s)
        if i < 2:
            assert emu.counters.fast_bails > 0, s      # (hand-overs happened; the in-place form finishes them itself)
        if i == (0 if tray else 1):
            # the profiled form of the same launch: the bytes of the lean one, and it did stamp (the lean one cannot: it is refused the buffer)
            gotp, _, emup = _workload(model, s, batch=ProfiledEmuBatch, before_launch=hook)
            _same(gotp, got, ("profiled", s))
            assert (emup.stamps[:, :16] == 0).any(axis=1).all(), "every env's last launch left stage stamps"
            assert (emu.stamps == -1).all(), "the lean form stamps nothing"


def _forms(fam, prof, **kw):
    a = dict(has_inplace=True, maxefc=63, integrate=1, ext=False, n=4096, nsub=50, fast_rows=True, waves_per_env=2, waves_per_env_tray=2, inplace=False)
    a.update(kw)
    out = np.zeros(4, dtype=np.int32)
    _lib().emu_launch_forms_prof(fam, int(a["has_inplace"]), a["maxefc"], a["integrate"], int(a["ext"]), a["n"], a["nsub"], int(a["fast_rows"]),
                                 a["waves_per_env"], a["waves_per_env_tray"], int(a["inplace"]), int(prof), out.ctypes.data)
    return int(out[0]), int(out[1])


def test_form_kinds_are_what_this_file_says(built):
    out = np.zeros(3, dtype=np.int32)
    _lib().emu_form_kinds(out.ctypes.data)
    assert out[0] == 11
    assert out[1] == sum(1 << f for f in LEAN) and out[2] == sum(1 << f for f in PROF)


def test_policy_never_answers_a_lean_form_with_ext_forward_or_prof(built):
    seen = set()
    for fam, integrate, ext, prof, inplace, has_inplace, w, wt, fast_rows, maxefc, (n, nsub) in itertools.product(
            range(7), (0, 1), (False, True), (False, True), (False, True), (False, True), (1, 2), (1, 2), (False, True), (63, 127),
            ((64, 1), (64, 12), (512, 4), (513, 4), (4096, 1), (4096, 50))):
        first, mid = _forms(fam, prof, integrate=integrate, ext=ext, inplace=inplace, has_inplace=has_inplace, waves_per_env=w, waves_per_env_tray=wt,
                            fast_rows=fast_rows, maxefc=maxefc, n=n, nsub=nsub)
        where = (fam, integrate, ext, prof, inplace, has_inplace, w, wt, fast_rows, maxefc, n, nsub)
        if ext or not integrate or prof:
            assert first not in LEAN, where
        if ext or not integrate:
            assert first not in PROF, where
        if not prof:
            assert first not in PROF, where
            # (without the buffer the answer is the one the rule gave before it had the argument)
            assert (first, mid) == emu_py.launch_forms(fam, has_inplace=has_inplace, maxefc=maxefc, integrate=integrate, ext=ext, n=n, nsub=nsub, fast_rows=fast_rows,
                                                       waves_per_env=w, waves_per_env_tray=wt, inplace=inplace)[:2], where
        assert mid not in LEAN + PROF, where
        assert not _lib().emu_lean_form_refuses(first, int(ext), integrate, int(prof)), where
        seen.add(first)
    assert set(LEAN + PROF) <= seen     # (every one of them is an answer somewhere)


@pytest.mark.parametrize("inplace", [False, True])
def test_policy_with_prof_answers_the_profiled_plain_form_whatever_inplace_says(inplace, built):
    for fam in (CASSIE, CASSIE_HFIELD):
        assert _forms(fam, True, inplace=inplace) == (FORM_FAST_2W_PROF, FORM_MID_WALK_2W)
        assert _forms(fam, True, inplace=inplace, waves_per_env=1) == (FORM_FAST_PROF, FORM_ALONE)
        assert _forms(fam, False, inplace=inplace)[0] == (FORM_FAST_INPLACE if inplace else FORM_FAST_2W)
    assert _forms(TRAY, True, inplace=inplace) == (FORM_FAST_2W_PROF, FORM_MID_WALK_2W)
    assert _forms(TRAY, True, inplace=inplace, waves_per_env_tray=1) == (FORM_FAST_PROF, FORM_MID_WALK)
    # where the launch takes no fast form the buffer changes nothing: the forms alone carry the stamps
    for kw in (dict(n=64, nsub=1), dict(fast_rows=False), dict(ext=True), dict(integrate=0)):
        for fam in (CASSIE, CASSIE_HFIELD) + ((TRAY,) if "n" not in kw else ()):   # (the tray model has no small-batch rule)
            assert _forms(fam, True, inplace=inplace, **kw) == _forms(fam, False, inplace=inplace, **kw)


def test_refusal_rule_fires_for_every_lean_form_and_each_condition(built):
    refuses = lambda form, ext, integrate, prof: bool(_lib().emu_lean_form_refuses(form, int(ext), integrate, int(prof)))
    for form in LEAN:
        assert not refuses(form, False, 1, False)
        assert refuses(form, True, 1, False) and refuses(form, False, 0, False) and refuses(form, False, 1, True)
    for form in PROF:       # (stamps, but no read-out code and no forward mode either)
        assert not refuses(form, False, 1, False) and not refuses(form, False, 1, True)
        assert refuses(form, True, 1, True) and refuses(form, False, 0, True)
    for form in (FORM_ALONE, FORM_ALONE_2W, FORM_WIDE, FORM_MID_WALK, FORM_MID_WALK_2W, FORM_WIDE_WALK):
        for ext, integrate, prof in itertools.product((False, True), (0, 1), (False, True)):
            assert not refuses(form, ext, integrate, prof)
