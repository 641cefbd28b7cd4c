"""The bank of full states, host side (csrc/small_launch.h: state_layout, state_grid, state_configure, check_state_call), through the
emulator's entry points, which go through the same functions as phys_batch.hip: the row's layout for all three models and every
combination of groups, the grid, and every refusal with its message.  No GPU."""
import ctypes
import itertools

import numpy as np
import pytest

import states_check as sc
import states_emu_py as se
from cassie_amd import Model
from cassie_amd import phys as P
from cassie_amd._lib import CmDriveState, CmEnvParams

MODELS = ("cassie", "cassie_hfield", "cassie_tray_box")
OPTIONAL = (P.STATE_COMMANDS, P.STATE_EPISODE, P.STATE_PARAMS)
GROUP_SETS = [P.STATE_CORE | sum(c) for k in range(4) for c in itertools.combinations(OPTIONAL, k)]
COMMANDS = ("pd_ptarget", "pd_kp", "pd_kd", "pd_dtarget", "pd_torque", "drive_cmd", "qfrc_applied", "xfrc_applied")
EPISODE = ("ep_steps", "ep_count", "terrain")


@pytest.fixture(scope="module")
def models(built):
    return {name: Model(name) for name in MODELS}


@pytest.mark.parametrize("name", MODELS)
def test_layout_of_every_group_combination(models, name):
    """Sections are 16-byte aligned and disjoint, the row dim is their (padded) sum, each group brings exactly its sections, and the
    counts are the per-env arrays' sizes in 8-byte words."""
    pod = models[name].pod
    shapes = sc.section_shapes(pod)
    assert len(GROUP_SETS) == 8
    assert se.section_bytes() == (ctypes.sizeof(CmDriveState), ctypes.sizeof(CmEnvParams))
    for groups in GROUP_SETS:
        lay, row_dim = se.layout(pod, groups)
        sc.check_layout(lay, row_dim)
        want = set(sc.CORE) | (set(COMMANDS) if groups & P.STATE_COMMANDS else set()) | (set(EPISODE) if groups & P.STATE_EPISODE else set()) | \
            ({"params"} if groups & P.STATE_PARAMS else set())
        assert set(lay) == want, groups
        for sect, (off, count, dt) in lay.items():
            shape, adt = shapes[sect]
            nbytes = int(np.prod(shape)) * np.dtype(adt).itemsize
            assert count == (1 if adt == np.int32 else nbytes // 8) and (adt == np.int32 or nbytes % 8 == 0), sect
            assert np.dtype(dt) == np.dtype(adt), sect
        # CORE is there whether named or not, and lies first: the optional groups only append
        core, core_dim = se.layout(pod, 0)
        assert core == se.layout(pod, P.STATE_CORE)[0] and all(lay[k] == core[k] for k in core) and row_dim >= core_dim
    # the order of the sections is the order of P.STATE_SECTIONS
    lay, _ = se.layout(pod, sum(OPTIONAL))
    offs = [lay[n][0] for n, _ in P.STATE_SECTIONS]
    assert offs == sorted(offs) and offs[0] == 0


def test_layout_sizes_beyond_the_models():
    """Odd counts everywhere (nq = 35, nv = 33, nu = 11, nsd = 67, nbody = 27): every section still starts on an even word."""
    for groups in GROUP_SETS:
        lay, row_dim = se.layout_of_sizes(35, 33, 11, 67, 27, groups)
        sc.check_layout(lay, row_dim)
        assert lay["qpos"][1] == 35 and lay["qvel"][0] == lay["qpos"][0] + 36


def test_signature(models):
    """The signature tells the models and the groups apart and is a function of them alone."""
    sigs = {(m, g): se.signature(models[m].pod, g) for m in MODELS for g in GROUP_SETS}
    assert len(set(sigs.values())) == len(sigs) and 0 not in sigs.values()
    assert se.signature(Model("cassie").pod, P.STATE_CORE) == sigs[("cassie", P.STATE_CORE)]
    assert se.signature(models["cassie"].pod, 0) == sigs[("cassie", P.STATE_CORE)]


def test_grid():
    """One workgroup per env up to 256, which then walk the range."""
    assert [se.grid(n) for n in (1, 2, 63, 64, 255, 256, 257, 4096, 1 << 20)] == [1, 2, 63, 64, 255, 256, 256, 256, 256]


def _fields(pod, nenv, names):
    return sc.distinct_fields(pod, nenv, names)


def test_refusals(models):
    """Every refusal and its message: of the configure call (nslots < 1, unknown group bits, EPISODE without episodes, PARAMS without
    parameter blocks, COMMANDS without applied forces) and of a save / restore (not configured, range out of bounds)."""
    pod = models["cassie"].pod
    nenv = 4
    core = _fields(pod, nenv, sc.CORE)
    every = _fields(pod, nenv, [n for n, _ in P.STATE_SECTIONS])
    ok = se.configure_refusal
    assert ok(pod, core, 1, P.STATE_CORE) == "" and ok(pod, every, 3, sum(OPTIONAL), nterrain=2) == ""
    assert "at least one slot" in ok(pod, core, 0, P.STATE_CORE) and "at least one slot" in ok(pod, core, -5, P.STATE_CORE)
    assert "PHYS_STATE_CORE, PHYS_STATE_COMMANDS" in ok(pod, every, 1, 16)
    msg = ok(pod, core, 1, P.STATE_EPISODE)
    assert "PHYS_STATE_EPISODE" in msg and "phys_batch_episodes_enable" in msg
    msg = ok(pod, core, 1, P.STATE_PARAMS)
    assert "PHYS_STATE_PARAMS" in msg and "phys_batch_randomize" in msg
    no_applied = dict(every, qfrc_applied=None, xfrc_applied=None)
    msg = ok(pod, no_applied, 1, P.STATE_COMMANDS)
    assert "qfrc_applied / xfrc_applied" in msg and "restored into nothing" in msg
    assert ok(pod, dict(every, xfrc_applied=None), 1, P.STATE_COMMANDS) == msg
    assert ok(pod, no_applied, 1, P.STATE_EPISODE | P.STATE_PARAMS) == ""

    lay, row_dim = se.layout(pod, P.STATE_CORE)
    bank = np.zeros((2, row_dim), dtype=np.int64)
    for restore in (False, True):
        assert "not configured" in se.call(pod, core, None, restore, expect_error=True)
        assert "not configured" in se.call(pod, core, bank, restore, nslots=0, expect_error=True)
        for env0, n in ((-1, 2), (0, nenv + 1), (nenv, 1), (2, 3), (0, -1)):
            assert se.call(pod, core, bank, restore, env0=env0, n=n, expect_error=True) == "env range out of bounds", (env0, n)
        # (a group's needs are checked again at the call: a new shared model may have dropped the parameter blocks since)
        assert "PHYS_STATE_PARAMS" in se.call(pod, core, bank, restore, groups=P.STATE_PARAMS, expect_error=True)
    before = sc.fields_bytes(core)
    se.call(pod, core, bank, False, env0=nenv, n=0)         # an empty range at the end is fine and does nothing
    assert not bank.any() and sc.fields_bytes(core) == before
