"""The launcher's rules about launches that accumulate the step sums (csrc/step_policy.h: launch_forms' trailing argument `sums`,
step_sums_refuses), run on the CPU through the emulator library -- pure functions, no launch."""
import itertools

import emu_py
import sums_emu_py as S

# ck::StepForm / ck::StepFamily (csrc/step_plan.h)
(FORM_ALONE, FORM_ALONE_2W, FORM_WIDE, FORM_FAST, FORM_FAST_2W, FORM_FAST_INPLACE, FORM_MID_WALK, FORM_MID_WALK_2W, FORM_WIDE_WALK, FORM_FAST_PROF,
 FORM_FAST_2W_PROF, FORM_COUNT) = range(12)
LEAN = (FORM_FAST, FORM_FAST_2W, FORM_FAST_INPLACE)
PROF = (FORM_FAST_PROF, FORM_FAST_2W_PROF)
CASSIE, CASSIE_HFIELD, CASSIE_ALL, TRAY, TRAY_HFIELD, GENERIC32, GENERIC40 = range(7)

# the argument grid tests/test_launch_policy.py sweeps, over every family
GRID = list(itertools.product(range(7), (True, False), (63, 127), (0, 1), (False, True), (64, 4096), (1, 4, 50), (False, True), (1, 2), (1, 2), (False, True)))


def _kw(g):
    fam, has_inplace, maxefc, integrate, ext, n, nsub, fast_rows, waves, waves_tray, inplace = g
    return dict(fam=fam, has_inplace=has_inplace, maxefc=maxefc, integrate=integrate, ext=ext, n=n, nsub=nsub, fast_rows=fast_rows, waves_per_env=waves,
                waves_per_env_tray=waves_tray, inplace=inplace)


def test_the_form_table_is_what_it_was(built):
    import ctypes
    import numpy as np
    kinds = np.zeros(3, dtype=np.int32)
    emu_py.lib().emu_form_kinds(ctypes.c_void_p(kinds.ctypes.data))
    assert kinds[0] == FORM_COUNT == 11             # no new StepForm value: whether a launch accumulates is a second axis
    assert kinds[1] == sum(1 << f for f in LEAN) and kinds[2] == sum(1 << f for f in PROF)


def test_with_the_sums_off_the_forms_are_todays(built):
    for g in GRID:
        kw = _kw(g)
        first, mid, wide, stay = emu_py.launch_forms(**kw)
        for prof in (False, True):
            got = S.launch_forms(prof=prof, sums=False, **kw)
            if not prof:
                assert got == (first, mid, int(wide), stay), kw
        # a forward pass is never an accumulating launch, whatever the flag says
        if not kw["integrate"]:
            assert S.launch_forms(sums=True, **kw) == (first, mid, int(wide), stay), kw


def test_an_accumulating_launch_takes_the_plain_two_wave_fast_form_or_a_full_form(built):
    fast2w = 0
    for g in GRID:
        kw = _kw(g)
        if not kw["integrate"]:
            continue
        for prof in (False, True):
            first, mid, wide, _ = S.launch_forms(prof=prof, sums=True, **kw)
            assert first != FORM_FAST_INPLACE and first not in (FORM_FAST, FORM_FAST_PROF, FORM_FAST_2W_PROF), (kw, prof, first)
            if first == FORM_FAST_2W:
                # ... the form it would have taken with the range in the plain form and the sums off, + the pass that walks the list
                assert mid == FORM_MID_WALK_2W and not prof and not kw["ext"]
                assert (first, mid, wide) == S.launch_forms(sums=False, **dict(kw, inplace=False))[:3]
                fast2w += 1
            else:
                assert first in (FORM_ALONE, FORM_ALONE_2W, FORM_WIDE), (kw, prof, first)
    assert fast2w > 0
    # whatever the range's in-place state says
    for fam in (CASSIE, CASSIE_HFIELD):
        assert S.launch_forms(fam, inplace=True, sums=False)[0] == FORM_FAST_INPLACE
        assert S.launch_forms(fam, inplace=True, sums=True)[:2] == (FORM_FAST_2W, FORM_MID_WALK_2W)
    assert S.launch_forms(TRAY, sums=True)[:2] == (FORM_FAST_2W, FORM_MID_WALK_2W)
    # the documented fall-back: one wave per env -> the full form alone
    assert S.launch_forms(CASSIE, waves_per_env=1, sums=True)[0] == FORM_ALONE
    assert S.launch_forms(CASSIE, waves_per_env=1, maxefc=127, sums=True)[0] == FORM_WIDE
    assert S.launch_forms(TRAY, waves_per_env_tray=1, sums=True)[0] == FORM_ALONE


def test_a_lean_or_profiled_instantiation_is_never_launched_with_the_block(built):
    for form in range(FORM_COUNT):
        for ext, integrate, prof in itertools.product((False, True), (0, 1), (False, True)):
            old = bool(emu_py.lib().emu_lean_form_refuses(form, int(ext), integrate, int(prof)))
            # the block off, an instantiation of the first table: the rule is lean_form_refuses
            assert S.step_sums_refuses(form, ext, integrate, prof, sums=False, sums_inst=False) == old
            # the block set: every lean and every profiled instantiation is refused, and every forward pass
            got = S.step_sums_refuses(form, ext, integrate, prof, sums=True, sums_inst=False)
            if form in LEAN or form in PROF or not integrate:
                assert got, (form, ext, integrate, prof)
            else:
                assert got == old
    # the FEAT_SUMS instantiations: the lean forms' siblings, for plain accumulating launches alone
    for form in range(FORM_COUNT):
        assert S.step_sums_refuses(form, sums=True, sums_inst=True) == (form not in LEAN)
        assert S.step_sums_refuses(form, sums=False, sums_inst=True)
        for ext, integrate, prof in ((True, 1, False), (False, 0, False), (False, 1, True)):
            assert S.step_sums_refuses(form, ext, integrate, prof, sums=True, sums_inst=True)
