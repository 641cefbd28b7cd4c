"""The bank of full states on the CPU wave emulator (tests/emu/emu_states.cpp: the kernels of csrc/state_kernels.h, laid out, checked and
launched as phys_batch.hip does it) against the numpy restatement (tests/states_check.py), on hand-placed states in which every word is
distinct: a saved row, a restore that writes its sections and nothing else, skipped and out-of-range slots, strided qpos | qvel |
sensordata, a fan-out, all three models' sizes.  The GPU counterpart is tests/test_states_gpu.py."""
import numpy as np
import pytest

import states_check as sc
import states_emu_py as se
from cassie_amd import Model
from cassie_amd import phys as P

ALL = P.STATE_CORE | P.STATE_COMMANDS | P.STATE_EPISODE | P.STATE_PARAMS
NAMES = [n for n, _ in P.STATE_SECTIONS]
POISON = np.int64(-0x0123456789abcdef)


@pytest.fixture(scope="module")
def models(built):
    return {name: Model(name) for name in ("cassie", "cassie_hfield", "cassie_tray_box")}


def poisoned_bank(nslots, row_dim):
    return np.full((nslots, row_dim), POISON, dtype=np.int64)


@pytest.mark.parametrize("name,groups", [("cassie", P.STATE_CORE), ("cassie", ALL), ("cassie_hfield", P.STATE_CORE | P.STATE_EPISODE),
                                         ("cassie_tray_box", ALL), ("cassie_tray_box", P.STATE_CORE | P.STATE_PARAMS)])
def test_saved_rows_equal_the_restatement(models, name, groups):
    """7 envs to a permutation of 9 slots on 3 workgroups (every workgroup walks): each slot's row is states_check.row() of its env,
    padding words zero, the two slots nobody saved to untouched, the envs' arrays unchanged.  cassie has nq = 35, the tray model
    nq = 42 / nv = 40; the sections' lengths lie on both sides of a wave's 64 lanes (time 1, qpos 35, meas 56, sensordata, xpos 3 nbody,
    the drive-level state 150, the parameter block ~2000 words)."""
    pod = models[name].pod
    nenv, nslots = 7, 9
    lay, row_dim = se.layout(pod, groups)
    assert min(c for _, c, _ in lay.values()) == 1 and any(c < 64 for _, c, _ in lay.values()) and any(64 < c < 128 for _, c, _ in lay.values()) and \
        any(c > 128 for _, c, _ in lay.values())
    fields = sc.distinct_fields(pod, nenv, NAMES)
    before = sc.fields_bytes(fields)
    slots = np.array([4, 0, 8, 1, 6, 2, 5], dtype=np.int32)
    bank = poisoned_bank(nslots, row_dim)
    se.call(pod, fields, bank, False, groups=groups, slots=slots, grid=3, nterrain=2)
    for e in range(nenv):
        assert bank[slots[e]].tobytes() == sc.row(lay, row_dim, fields, e).tobytes(), e
    assert (bank[[3, 7]] == POISON).all() and sc.fields_bytes(fields) == before
    # the default slots (NULL): env e to slot e, over a sub-range, on the launcher's own grid
    bank2 = poisoned_bank(nslots, row_dim)
    se.call(pod, fields, bank2, False, groups=groups, env0=2, n=4, nterrain=2)
    for s in range(nslots):
        want = sc.row(lay, row_dim, fields, s) if 2 <= s < 6 else np.full(row_dim, POISON)
        assert bank2[s].tobytes() == want.tobytes(), s


def test_absent_arrays_are_zeros_and_are_skipped(models):
    """Before a drive mode is selected the batch has no measurement block and no drive-level state, without a bank of terrains no terrain
    index: their sections are saved as zeros, and a restore leaves the (later) arrays alone."""
    pod = models["cassie"].pod
    groups = P.STATE_CORE | P.STATE_EPISODE
    lay, row_dim = se.layout(pod, groups)
    full = sc.distinct_fields(pod, 3, NAMES)
    absent = dict(full, meas=None, drive_state=None)
    bank = poisoned_bank(3, row_dim)
    se.call(pod, absent, bank, False, groups=groups, nterrain=0)          # (terrain given, but no bank of terrains: not the env's)
    for e in range(3):
        want = sc.row(lay, row_dim, dict(absent, terrain=None), e)
        assert bank[e].tobytes() == want.tobytes()
        for sect in ("meas", "drive_state", "terrain"):
            off, count, _ = lay[sect]
            assert not want[off:off + count].any()
    # restored into a batch that still has none of them: the other sections arrive, the three arrays (not the batch's) are not touched
    other = sc.distinct_fields(pod, 3, NAMES, start=10 ** 6)
    held = {sect: other[sect].copy() for sect in ("meas", "drive_state", "terrain")}
    se.call(pod, dict(other, meas=None, drive_state=None), bank, True, groups=groups, nterrain=0, slots=[2, 0, 1])
    assert other["qpos"].tobytes() == full["qpos"][[2, 0, 1]].tobytes() and other["warn"].tobytes() == full["warn"][[2, 0, 1]].tobytes()
    assert all(other[sect].tobytes() == held[sect].tobytes() for sect in held)
    # restored after a drive mode was selected and a bank of terrains set: the zeros of the row -- what selecting the mode left
    se.call(pod, other, bank, True, groups=groups, nterrain=2, slots=[2, 0, 1])
    assert not other["meas"].any() and not other["drive_state"].any() and not other["terrain"].any()


@pytest.mark.parametrize("name,groups", [("cassie", P.STATE_CORE), ("cassie_tray_box", ALL)])
def test_restore_writes_its_sections_and_nothing_else(models, name, groups):
    """Envs 2 .. 5 of 8 take slots of a bank whose padding words are poisoned: they hold what states_check.apply() leaves, the
    neighbouring envs (0, 1, 6, 7), the sections of groups that are not in the row, and the bank itself are untouched."""
    pod = models[name].pod
    nenv, nslots = 8, 6
    lay, row_dim = se.layout(pod, groups)
    src = sc.distinct_fields(pod, nslots, NAMES, start=1)
    bank = np.stack([sc.row(lay, row_dim, src, s) for s in range(nslots)])
    covered = np.zeros(row_dim, dtype=bool)
    for off, count, _ in lay.values():
        covered[off:off + count] = True
    assert (~covered).sum() == sum(c & 1 for _, c, _ in lay.values()) > 0
    bank[:, ~covered] = POISON
    fields = sc.distinct_fields(pod, nenv, NAMES, start=10 ** 7)
    want = sc.copy_fields(fields)
    slots = np.array([5, 0, 3, 3], dtype=np.int32)
    for i, s in enumerate(slots):
        sc.apply(lay, bank[s], want, 2 + i)
    kept = bank.copy()
    se.call(pod, fields, bank, True, groups=groups, env0=2, n=4, slots=slots, grid=2, nterrain=3)
    assert sc.fields_bytes(fields) == sc.fields_bytes(want) and bank.tobytes() == kept.tobytes()
    for sect in NAMES:
        if sect not in lay:
            assert fields[sect].tobytes() == sc.distinct_fields(pod, nenv, NAMES, start=10 ** 7)[sect].tobytes(), sect
    # and a save of the restored envs gives the rows back (with clean padding)
    again = poisoned_bank(nslots, row_dim)
    se.call(pod, fields, again, False, groups=groups, env0=2, n=4, slots=[0, 1, 2, 4], nterrain=3)
    for i, s in enumerate(slots):
        got = again[[0, 1, 2, 4][i]]
        assert got[covered].tobytes() == bank[s][covered].tobytes() and not got[~covered].any()


@pytest.mark.parametrize("restore", [False, True])
def test_negative_and_out_of_range_slots(models, restore):
    """A negative slot skips the env; a slot >= nslots skips it and raises WARN_STATE_SLOT in its warning word, on top of the bits it
    holds; everybody else is served.  Nothing outside the bank is touched: the bank sits in the middle of a poisoned buffer."""
    pod = models["cassie"].pod
    assert se.lib().emu_state_warn_bit() == P.WARN_STATE_SLOT == 256
    nenv, nslots = 6, 3
    lay, row_dim = se.layout(pod, P.STATE_CORE)
    src = sc.distinct_fields(pod, nslots, NAMES, start=5 * 10 ** 6)
    buf = poisoned_bank(nslots + 2, row_dim)
    bank = buf[1:1 + nslots]
    bank[:] = np.stack([sc.row(lay, row_dim, src, s) for s in range(nslots)])
    fields = sc.distinct_fields(pod, nenv, NAMES)
    fields["warn"][:] = [0, 8, 1, 2, 0, 4]
    want, want_bank = sc.copy_fields(fields), bank.copy()
    slots = np.array([2, -1, nslots, 0, 1 << 30, -(1 << 31)], dtype=np.int32)
    for e, s in enumerate(slots):
        if 0 <= s < nslots:
            if restore:
                sc.apply(lay, bank[s], want, e)
            else:
                want_bank[s] = sc.row(lay, row_dim, fields, e)
        elif s >= nslots:
            want["warn"][e] |= P.WARN_STATE_SLOT
    se.call(pod, fields, bank, restore, slots=slots)
    assert sc.fields_bytes(fields) == sc.fields_bytes(want) and bank.tobytes() == want_bank.tobytes()
    assert (buf[[0, -1]] == POISON).all()
    assert list(fields["warn"][[2, 4]]) == [1 | 256, 256]


def test_strided_qpos_qvel_sensordata(models):
    """qpos | qvel | sensordata as columns of one [nenv][W] observation block with extra columns behind them: a save reads the columns,
    a restore writes them and leaves the other columns alone; the rows are those of dense arrays."""
    pod = models["cassie"].pod
    nenv = 5
    lay, row_dim = se.layout(pod, P.STATE_CORE)
    fields = sc.distinct_fields(pod, nenv, NAMES)
    w = pod.nq + pod.nv + pod.nsensordata
    block = np.full((nenv, w + 3), -7.25)
    block[:, :w] = np.concatenate([fields["qpos"], fields["qvel"], fields["sensordata"]], axis=1)
    bank = poisoned_bank(nenv, row_dim)
    hidden = dict(fields, qpos=None, qvel=None, sensordata=None)
    se.call(pod, hidden, bank, False, block=block)
    for e in range(nenv):
        assert bank[e].tobytes() == sc.row(lay, row_dim, fields, e).tobytes()
    slots = np.array([3, 4, -1, 0, 0], dtype=np.int32)
    want = sc.copy_fields(fields)
    for e, s in enumerate(slots):
        if s >= 0:
            sc.apply(lay, bank[s], want, e)
    se.call(pod, hidden, bank, True, block=block, slots=slots)
    assert block[:, :w].tobytes() == np.concatenate([want["qpos"], want["qvel"], want["sensordata"]], axis=1).tobytes()
    assert (block[:, w:] == -7.25).all()
    for sect in lay:
        if hidden[sect] is not None:
            assert hidden[sect].tobytes() == want[sect].tobytes(), sect


def test_fan_out_of_one_slot(models):
    """A fork: env 5 saved to slot 0, slot 0 restored into a scattered set of envs, slot -1 for everybody else."""
    pod = models["cassie_tray_box"].pod
    nenv = 12
    lay, row_dim = se.layout(pod, ALL)
    fields = sc.distinct_fields(pod, nenv, NAMES)
    start = sc.copy_fields(fields)
    bank = poisoned_bank(1, row_dim)
    save = np.full(nenv, -1, dtype=np.int32)
    save[5] = 0
    se.call(pod, fields, bank, False, groups=ALL, slots=save, nterrain=4)
    takers = [0, 3, 4, 9, 11]
    take = np.full(nenv, -1, dtype=np.int32)
    take[takers] = 0
    se.call(pod, fields, bank, True, groups=ALL, slots=take, nterrain=4)
    for sect in lay:
        for e in range(nenv):
            want = start[sect][5] if e in takers else start[sect][e]
            assert fields[sect][e].tobytes() == want.tobytes(), (sect, e)
