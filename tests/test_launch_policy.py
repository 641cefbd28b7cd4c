"""The launcher's rules (csrc/step_policy.h) on the CPU, through the emulator library: which forms a stepping launch takes, in how many
chunks, with which grids behind it, when a range's fast kernel changes its form, when the order kernel is due -- and the table of env
ranges the launcher keeps its per-range facts in.  The expected values are the ones the launcher applied before the rules had a
header of their own (each is a measured choice: profiles/round4 .. round6)."""
import itertools

import pytest

import emu_py

ALONE, ALONE_2W, WIDE, FAST, FAST_2W, FAST_INPLACE, MID_WALK, MID_WALK_2W, WIDE_WALK = range(9)      # ck::StepForm
CASSIE, CASSIE_HFIELD, CASSIE_ALL, TRAY, TRAY_HFIELD, GENERIC32, GENERIC40 = range(7)                 # ck::StepFamily
STAY_ROWS = 31 - 4


def forms(fam=CASSIE, **kw):
    kw.setdefault("has_inplace", fam in (CASSIE, CASSIE_HFIELD))
    return emu_py.launch_forms(fam, **kw)


@pytest.mark.parametrize("fam", [CASSIE, CASSIE_HFIELD])
def test_forms_of_the_cassie_families(built, fam):
    assert forms(fam, n=4096, nsub=50) == (FAST_2W, MID_WALK_2W, False, STAY_ROWS)
    assert forms(fam, n=4096, nsub=50, inplace=True) == (FAST_INPLACE, MID_WALK_2W, False, STAY_ROWS)
    assert forms(fam, n=4096, nsub=50, inplace=True, has_inplace=False)[0] == FAST_2W
    # a small batch stepping a few substeps per launch: one instantiation alone
    assert forms(fam, n=512, nsub=4)[0] == ALONE_2W
    assert forms(fam, n=512, nsub=5)[:2] == (FAST_2W, MID_WALK_2W)
    assert forms(fam, n=513, nsub=4)[:2] == (FAST_2W, MID_WALK_2W)
    # forward / read-out passes, the fast kernel switched off: alone, one wave per env where the grid is large
    for kw in (dict(integrate=0, nsub=1), dict(ext=True), dict(fast_rows=False)):
        assert forms(fam, n=4096, **kw)[0] == ALONE, kw
        assert forms(fam, n=64, **kw)[0] == ALONE_2W, kw
        assert forms(fam, n=512, **kw)[0] == ALONE_2W and forms(fam, n=513, **kw)[0] == ALONE, kw
        assert forms(fam, n=4096, inplace=True, **kw)[0] == ALONE, kw
    # one wave per env: the 63-row pass behind the fast kernel looks records up
    assert forms(fam, waves_per_env=1)[:2] == (FAST, ALONE)
    assert forms(fam, waves_per_env=1, inplace=True)[:2] == (FAST, ALONE)
    # the wide caps: a third tier behind the fast kernel, the 127-row instantiation where one steps every env alone
    assert forms(fam, maxefc=127) == (FAST_2W, MID_WALK_2W, True, STAY_ROWS)
    assert forms(fam, maxefc=127, inplace=True) == (FAST_INPLACE, MID_WALK_2W, True, STAY_ROWS)
    assert forms(fam, maxefc=127, waves_per_env=1)[:3] == (FAST, ALONE, True)
    for kw in (dict(integrate=0, nsub=1), dict(ext=True), dict(fast_rows=False), dict(n=64, nsub=4)):
        assert forms(fam, maxefc=127, **kw)[0] == WIDE, kw
    assert forms(fam, maxefc=63)[2] is False and forms(fam, maxefc=64)[2] is True


def test_forms_of_the_tray_family(built):
    assert forms(TRAY)[:3] == (FAST_2W, MID_WALK_2W, False)
    for kw in itertools.product((True, False), (63, 127), (4096, 64), (50, 4), (1, 2)):
        first = forms(TRAY, inplace=True, has_inplace=kw[0], maxefc=kw[1], n=kw[2], nsub=kw[3], waves_per_env=kw[4])
        assert first[:3] == (FAST_2W, MID_WALK_2W, False), kw          # never in place, never wide, no small-batch rule
    assert forms(TRAY, waves_per_env_tray=1)[:2] == (FAST, MID_WALK)
    assert forms(TRAY, integrate=0, nsub=1)[0] == ALONE and forms(TRAY, ext=True)[0] == ALONE
    assert forms(TRAY, fast_rows=False)[0] == ALONE_2W
    assert forms(TRAY, fast_rows=False, waves_per_env_tray=1)[0] == ALONE


@pytest.mark.parametrize("fam", [CASSIE_ALL, TRAY_HFIELD, GENERIC32, GENERIC40])
def test_the_other_families_have_one_instantiation(built, fam):
    for integrate, ext, n, nsub, fast_rows, waves, inplace, maxefc in itertools.product((0, 1), (False, True), (64, 4096), (4, 50), (False, True),
                                                                                        (1, 2), (False, True), (63, 127)):
        got = emu_py.launch_forms(fam, has_inplace=False, maxefc=maxefc, integrate=integrate, ext=ext, n=n, nsub=nsub, fast_rows=fast_rows,
                                  waves_per_env=waves, waves_per_env_tray=waves, inplace=inplace)
        assert got[0] == ALONE and got[2] is False


@pytest.mark.parametrize("n,nenv,nsub,asked,expect", [
    (4096, 4096, 50, None, 7), (4096, 4096, 20, None, 4), (4096, 4096, 10, None, 2), (4096, 4096, 9, None, 1),
    (2048, 4096, 20, None, 3), (2048, 4096, 15, None, 3), (2048, 4096, 12, None, 2), (2048, 4096, 26, None, 2), (2048, 4096, 50, None, 2),
    (2048, 4096, 25, None, 3), (2048, 4096, 10, None, 2), (2048, 4096, 9, None, 1),
    (2040, 4096, 50, None, 1), (2052, 4096, 50, None, 1), (2040, 4096, 20, None, 1), (2052, 4096, 20, None, 1),
    (2040, 2040, 50, None, 1), (2048, 2048, 50, None, 7),
    (2048, 4096, 20, 4, 4), (4096, 4096, 50, 4, 4), (2048, 4096, 50, 4, 4), (2048, 4096, 15, 4, 3), (4096, 4096, 50, 1, 1), (2048, 4096, 20, 1, 1),
    (4096, 4096, 50, 2, 2), (2048, 4096, 20, 2, 2), (4096, 4096, 30, 7, 6),
])
def test_chunks_of_a_launch(built, n, nenv, nsub, asked, expect):
    assert emu_py.launch_chunks(n, nenv, nsub, asked) == expect


def test_grids_of_the_list_walking_passes(built):
    assert emu_py.pass_grids(4096, 0, 0, True) == (16, 8)
    assert emu_py.pass_grids(4096, 100, 0, True) == (216, 8)
    assert emu_py.pass_grids(4096, 10, 40, True) == (96, 88)       # (the first pass feeds the second: never the smaller)
    assert emu_py.pass_grids(4096, 10, 40, False) == (36, 8)       # (without the wide caps the second word is not read)
    assert emu_py.pass_grids(20, 100, 0, True) == (20, 8)
    assert emu_py.pass_grids(20, 100, 100, True) == (20, 20)
    assert emu_py.pass_grids(4, 0, 0, True) == (4, 4)
    assert emu_py.pass_grids(4096, -3, -5, True) == (16, 8)        # (the in-place form's run of quiet reports is not a length)
    assert emu_py.pass_grids(1 << 30, 1 << 30, 1 << 30, True) == (1 << 30, 1 << 30)


def test_form_of_a_ranges_fast_kernel(built):
    for was, seen, auto_ok in itertools.product((False, True), (-9, -8, -7, -1, 0, 1, 500), (False, True)):
        assert emu_py.next_inplace(was, seen, 0, auto_ok) is False
        assert emu_py.next_inplace(was, seen, 1, auto_ok) is True
    for was, seen in itertools.product((False, True), (-9, -8, -7, -1, 0, 1, 500)):
        assert emu_py.next_inplace(was, seen, 2, auto_ok=False) is False     # (without the order kernel nobody reports the in-place count)
    assert emu_py.next_inplace(False, 1, 2) is True and emu_py.next_inplace(False, 500, 2) is True
    assert emu_py.next_inplace(False, 0, 2) is False and emu_py.next_inplace(False, -8, 2) is False
    assert [emu_py.next_inplace(True, seen, 2) for seen in (3, 0, -1, -7, -8, -9)] == [True, True, True, True, False, False]


def test_order_kernel_cadence(built):
    assert emu_py.order_kernel_due(26, 1) and emu_py.order_kernel_due(50, 1)
    assert [k for k in range(1, 20) if emu_py.order_kernel_due(20, k)] == [16, 17, 18, 19]
    assert [k for k in range(1, 20) if emu_py.order_kernel_due(25, k)] == [16, 17, 18, 19]


def _disjoint(records):
    return all(a[0] + a[1] <= b[0] or b[0] + b[1] <= a[0] for a, b in itertools.combinations(records, 2))


def test_range_table_retires_what_a_new_range_overlaps(built):
    t = emu_py.RangeTable()
    whole, gone = t.claim(0, 4096)
    assert whole == [0, 4096, 0, 0] and gone == []
    whole[2], whole[3] = 1, 5                                        # (the launcher's: in place, five launches since a sort)
    again, gone = t.claim(0, 4096)
    assert again is whole and again == [0, 4096, 1, 5] and gone == [] and len(t.records) == 1
    lo, gone = t.claim(0, 2048)
    assert lo == [0, 2048, 0, 0] and gone == [(0, 4096, 1, 5)]      # (the retired record's form is reported: its words start over)
    hi, gone = t.claim(2048, 2048)
    assert hi == [2048, 2048, 0, 0] and gone == [] and t.records == [lo, hi]
    lo[3], hi[2], hi[3] = 3, 1, 9                                     # (launches_since_sort is per record)
    assert t.claim(0, 2048) == (lo, []) and t.claim(2048, 2048) == (hi, []) and (lo[3], hi[3]) == (3, 9)
    a, gone = t.claim(0, 1500)
    assert a == [0, 1500, 0, 0] and gone == [(0, 2048, 0, 3)] and t.records == [hi, a]
    c, gone = t.claim(1000, 2000)
    assert c == [1000, 2000, 0, 0] and sorted(gone) == [(0, 1500, 0, 0), (2048, 2048, 1, 9)] and t.records == [c]
    # neighbours that only touch do not overlap; a range inside another retires it
    assert t.claim(0, 1000)[1] == [] and t.claim(3000, 1096)[1] == [] and len(t.records) == 3
    assert t.claim(1500, 10)[1] == [(1000, 2000, 0, 0)]


def test_range_table_stays_disjoint(built):
    import numpy as np
    rng = np.random.default_rng(7)
    t = emu_py.RangeTable()
    for _ in range(300):
        env0 = int(rng.integers(0, 64))
        n = int(rng.integers(1, 65 - env0))
        before = [list(r) for r in t.records]
        rec, gone = t.claim(env0, n)
        assert rec[:2] == [env0, n] and _disjoint(t.records)
        if [env0, n] in [r[:2] for r in before]:
            assert gone == [] and t.records == before
        else:
            overlapping = [tuple(r) for r in before if r[0] < env0 + n and env0 < r[0] + r[1]]
            assert sorted(gone) == sorted(overlapping) and rec == [env0, n, 0, 0]
            assert sorted(map(tuple, t.records)) == sorted([tuple(r) for r in before if tuple(r) not in overlapping] + [(env0, n, 0, 0)])
        rec[2], rec[3] = int(rng.integers(0, 2)), int(rng.integers(0, 16))
