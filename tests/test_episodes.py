"""Episodes that end and restart on the device (phys_batch_end_episodes), on the CPU: the device's episode kernel
(csrc/episode_kernels.h: cassie_episode_kernel) executed by the wave emulator on hand-placed states, byte for byte against the numpy
restatement of the call in tests/episode_check.py.  The GPU counterpart is tests/test_episodes_gpu.py.

Every rule test asserts on its inputs that NO env lies within 1e-9 of min_height / min_upright (episode_check.
assert_clear_of_thresholds) before it compares; the comparison is then exact equality."""
import ctypes

import numpy as np
import pytest

import emu_py
import episode_check as ec
from cassie_amd import Model
from cassie_amd import phys as P
from cassie_amd._lib import CmModel, LIB_PATH

MODELS = ["cassie", "cassie_hfield", "cassie_tray_box"]
RULES = ec.rules(min_height=0.4, min_upright=0.5, max_steps=7, warn_mask=P.WARN_DIVERGED, nonfinite=True)
NROWS = 5


emu_end_episodes = emu_py.end_episodes


# hand-placed envs: (name, what to do to the upright, mid-episode env, reason bits expected under RULES)
def _tilt_x(a):
    return np.array([np.cos(a / 2), np.sin(a / 2), 0.0, 0.0])


def _tilt_y(a):
    return np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0])


CASES = [
    ("upright", lambda s, e: None, 0),
    ("below the height", lambda s, e: s["qpos"].__setitem__((e, 2), 0.39), ec.DONE_HEIGHT),
    ("just below the height", lambda s, e: s["qpos"].__setitem__((e, 2), 0.4 - 1e-6), ec.DONE_HEIGHT),
    ("just above the height", lambda s, e: s["qpos"].__setitem__((e, 2), 0.4 + 1e-6), 0),
    ("tilted 50 deg about x (within)", lambda s, e: s["qpos"].__setitem__((e, slice(3, 7)), _tilt_x(np.radians(50))), 0),
    ("tilted 70 deg about x (past)", lambda s, e: s["qpos"].__setitem__((e, slice(3, 7)), _tilt_x(np.radians(70))), ec.DONE_UPRIGHT),
    ("tilted 50 deg about y (within)", lambda s, e: s["qpos"].__setitem__((e, slice(3, 7)), _tilt_y(np.radians(-50))), 0),
    ("tilted 70 deg about y (past)", lambda s, e: s["qpos"].__setitem__((e, slice(3, 7)), _tilt_y(np.radians(-70))), ec.DONE_UPRIGHT),
    ("yawed 170 deg (upright)", lambda s, e: s["qpos"].__setitem__((e, slice(3, 7)), np.array([np.cos(1.48), 0, 0, np.sin(1.48)])), 0),
    ("NaN in qpos", lambda s, e: s["qpos"].__setitem__((e, 11), np.nan), ec.DONE_NONFINITE),
    ("NaN in the last qpos entry", lambda s, e: s["qpos"].__setitem__((e, -1), np.nan), ec.DONE_NONFINITE),
    ("1e11 in qvel", lambda s, e: s["qvel"].__setitem__((e, 9), 1e11), ec.DONE_NONFINITE),
    ("-1e11 in the last qvel entry", lambda s, e: s["qvel"].__setitem__((e, -1), -1e11), ec.DONE_NONFINITE),
    ("9e9 in qvel (finite enough)", lambda s, e: s["qvel"].__setitem__((e, 3), 9e9), 0),
    ("inf in qvel", lambda s, e: s["qvel"].__setitem__((e, 0), np.inf), ec.DONE_NONFINITE),
    ("warn word with the masked bit", lambda s, e: s["warn"].__setitem__(e, P.WARN_DIVERGED | P.WARN_CONTACT_FULL), ec.DONE_WARN),
    ("warn word without it", lambda s, e: s["warn"].__setitem__(e, P.WARN_CONTACT_FULL | P.WARN_CONSTRAINT_FULL), 0),
    ("steps one short of max_steps", lambda s, e: s["steps"].__setitem__(e, RULES["max_steps"] - 2), 0),
    ("steps at max_steps", lambda s, e: s["steps"].__setitem__(e, RULES["max_steps"] - 1), ec.DONE_TIME),
    ("steps past max_steps", lambda s, e: s["steps"].__setitem__(e, RULES["max_steps"] + 3), ec.DONE_TIME),
    ("forced", "force", ec.DONE_FORCED),
    ("forced and fallen", "force+height", ec.DONE_FORCED | ec.DONE_HEIGHT),
    ("low and tilted", lambda s, e: (s["qpos"].__setitem__((e, 2), 0.2), s["qpos"].__setitem__((e, slice(3, 7)), _tilt_x(2.0))),
     ec.DONE_HEIGHT | ec.DONE_UPRIGHT),
    ("diverged: NaN height, warn bit", lambda s, e: (s["qpos"].__setitem__((e, 2), np.nan), s["warn"].__setitem__(e, P.WARN_DIVERGED)),
     ec.DONE_NONFINITE | ec.DONE_WARN),
    ("NaN quaternion", lambda s, e: s["qpos"].__setitem__((e, 4), np.nan), ec.DONE_NONFINITE),
    ("out of time and low", lambda s, e: (s["steps"].__setitem__(e, 40), s["qpos"].__setitem__((e, 2), -3.0)), ec.DONE_TIME | ec.DONE_HEIGHT),
]


def make_state(model, nenv, seed, drive=True):
    """nenv envs somewhere in mid-episode: every array of the state holds non-trivial values, all envs upright and high."""
    pod = model.pod
    rng = np.random.default_rng(seed)
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape)
    qpos = np.tile(model.qpos_init(), (nenv, 1)) + 0.01 * u(nenv, pod.nq)
    qpos[:, 2] = 0.9 + 0.05 * u(nenv)
    qpos[:, 3:7] = [1.0, 0.0, 0.0, 0.0]
    s = dict(qpos=qpos, qvel=u(nenv, pod.nv), sensordata=u(nenv, pod.nsensordata), actuator_velocity=u(nenv, pod.nu),
             qacc=u(nenv, pod.nv), qacc_warmstart=u(nenv, pod.nv), ctrl=u(nenv, pod.nu), time=0.5 + np.abs(u(nenv)),
             warn=np.zeros(nenv, dtype=np.int32),
             meas=u(nenv, P.MEAS_DIM) if drive else None,
             drive=rng.integers(1, 255, (nenv, ec.DRIVE_BYTES), dtype=np.uint8) if drive else None,
             done=rng.integers(0, 2, nenv).astype(np.int32), reason=rng.integers(0, 64, nenv).astype(np.int32),
             steps=rng.integers(0, RULES["max_steps"] - 2, nenv).astype(np.int32), count=rng.integers(0, 9, nenv).astype(np.int32),
             terminal=u(nenv, pod.nq + pod.nv))
    return s


def placed_state(model, drive=True, pad=3):
    """The hand-placed cases, `pad` untouched envs before and after them and one between any two: -> (state, force, expected bits)."""
    nenv = 2 * pad + 2 * len(CASES)
    s = make_state(model, nenv, seed=len(model.name), drive=drive)
    force = np.zeros(nenv, dtype=np.int32)
    want = np.zeros(nenv, dtype=np.int32)
    for i, (_, place, bits) in enumerate(CASES):
        e = pad + 2 * i
        if isinstance(place, str):
            force[e] = 1 + i
            if "height" in place:
                s["qpos"][e, 2] = 0.1
        else:
            place(s, e)
        want[e] = bits
    return s, force, want


def make_bank(pod, nrows, seed=3):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (nrows, ec.row_dim(pod)))


@pytest.mark.parametrize("name", MODELS)
def test_rules_on_hand_placed_states(built, name):
    """done / reason / steps / count / terminal of every env equal the numpy restatement byte for byte, the reason words are the ones
    the cases were placed for, every CM_DONE_* bit occurs and some env has two; the state arrays are not touched (restart = 0)."""
    model = Model(name)
    s, force, want = placed_state(model)
    nenv = len(want)
    ec.assert_clear_of_thresholds(s["qpos"], RULES)
    ref, before = ec.copy_state(s), ec.copy_state(s)
    ec.end_episodes(ref, model.pod, RULES, 0, nenv, False, force=force)
    emu_end_episodes(s, model.pod, RULES, 0, nenv, False, force=force)
    ec.assert_states_equal(s, ref, name)
    assert np.array_equal(s["reason"], want), [(CASES[(e - 3) // 2][0], s["reason"][e], want[e]) for e in np.nonzero(s["reason"] != want)[0]]
    assert np.array_equal(s["done"], (want != 0).astype(np.int32))
    for bit in ec.ALL_BITS:
        assert (s["reason"] & bit).any(), bit
    assert any(bin(int(w)).count("1") >= 2 for w in s["reason"])
    for k in ec.STATE_ARRAYS:                                 # restart = 0: no state array changes at all
        assert s[k].tobytes() == before[k].tobytes(), k
    ended = s["done"] != 0
    assert np.array_equal(s["count"], before["count"] + ended) and np.array_equal(s["steps"], before["steps"] + 1)
    assert s["terminal"][~ended].tobytes() == before["terminal"][~ended].tobytes()
    assert s["terminal"][ended].tobytes() == np.concatenate([before["qpos"], before["qvel"]], axis=1)[ended].tobytes()


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("picked", [False, True])
@pytest.mark.parametrize("drive", [True, False])
def test_restart_takes_the_bank_row_and_leaves_the_others_alone(built, name, picked, drive):
    model = Model(name)
    pod = model.pod
    s, force, want = placed_state(model, drive=drive)
    nenv = len(want)
    bank = make_bank(pod, NROWS)
    pick = None
    if picked:                                                # (some outside [0, nrows): taken modulo nrows)
        pick = np.random.default_rng(5).integers(-2 * NROWS, 3 * NROWS, nenv).astype(np.int32)
    ec.assert_clear_of_thresholds(s["qpos"], RULES)
    ref, before = ec.copy_state(s), ec.copy_state(s)
    ec.end_episodes(ref, pod, RULES, 0, nenv, True, bank=bank, pick=pick, force=force)
    emu_end_episodes(s, pod, RULES, 0, nenv, True, bank=bank, pick=pick, force=force)
    ec.assert_states_equal(s, ref, name)
    ended = want != 0
    assert np.array_equal(s["done"], ended.astype(np.int32)) and np.array_equal(s["reason"], want)
    # written out once more, independently of episode_check.end_episodes: the row and the zeros of step 4
    rows = np.mod(pick.astype(np.int64), NROWS) if picked else (np.arange(nenv) + before["count"] + 1) % NROWS
    for e in np.nonzero(ended)[0]:
        got = np.concatenate([s[f][e] for f in ("qpos", "qvel", "sensordata", "actuator_velocity", "qacc")])
        assert got.tobytes() == bank[rows[e]].tobytes(), e
        for f in ("qacc_warmstart", "ctrl", "time", "warn", "steps") + (("meas", "drive") if drive else ()):
            assert not np.any(s[f][e]), (f, e)
        assert s["count"][e] == before["count"][e] + 1
    for k in ec.STATE_ARRAYS:                                 # every other env's every array is as before
        if s[k] is not None:
            assert s[k][~ended].tobytes() == before[k][~ended].tobytes(), k
    assert s["terminal"][~ended].tobytes() == before["terminal"][~ended].tobytes()
    assert np.array_equal(s["count"][~ended], before["count"][~ended]) and np.array_equal(s["steps"][~ended], before["steps"][~ended] + 1)


@pytest.mark.parametrize("grid", [1, 3, 32])
def test_a_range_of_the_batch_under_any_grid(built, grid):
    """Envs outside [env0, env0 + n) keep every array, done / reason included; pick / force are indexed from the range's start; the
    result does not depend on how many workgroups walk the range."""
    model = Model("cassie")
    pod = model.pod
    s, force, want = placed_state(model)
    nenv = len(want)
    env0, n = 5, nenv - 12
    bank = make_bank(pod, NROWS)
    pick = np.random.default_rng(9).integers(0, NROWS, n).astype(np.int32)
    ref, before = ec.copy_state(s), ec.copy_state(s)
    ec.end_episodes(ref, pod, RULES, env0, n, True, bank=bank, pick=pick, force=force[env0:env0 + n])
    emu_end_episodes(s, pod, RULES, env0, n, True, bank=bank, pick=pick, force=force[env0:env0 + n], grid=grid)
    ec.assert_states_equal(s, ref, "grid %d" % grid)
    outside = np.ones(nenv, dtype=bool)
    outside[env0:env0 + n] = False
    for k in s:
        assert s[k][outside].tobytes() == before[k][outside].tobytes(), k
    assert s["done"][env0:env0 + n].sum() == (want[env0:env0 + n] != 0).sum() > 10


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("restart", [False, True])
def test_strided_observation_block(built, name, restart):
    """qpos / qvel / sensordata as column blocks of one [nenv][nq + nv + nsd (+ 3 more)] block: same results as dense arrays, the
    block's other columns untouched."""
    model = Model(name)
    pod = model.pod
    s, force, want = placed_state(model)
    nenv = len(want)
    bank = make_bank(pod, NROWS)
    ref = ec.copy_state(s)
    ec.end_episodes(ref, pod, RULES, 0, nenv, restart, bank=bank, force=force)
    w = pod.nq + pod.nv + pod.nsensordata
    block = np.full((nenv, w + 3), 12345.678)
    block[:, :w] = np.concatenate([s["qpos"], s["qvel"], s["sensordata"]], axis=1)
    s["qpos"], s["qvel"], s["sensordata"] = block[:, :pod.nq], block[:, pod.nq:pod.nq + pod.nv], block[:, pod.nq + pod.nv:w]
    emu_end_episodes(s, pod, RULES, 0, nenv, restart, bank=bank, force=force, block=block)
    assert np.all(block[:, w:] == 12345.678)
    got = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in s.items()}
    ec.assert_states_equal(got, ref, name)
    assert (got["done"] != 0).sum() > 10


def test_rules_off_at_their_neutral_values(built):
    """With every rule at its neutral value nothing ends, whatever the state; each rule alone ends only its own cases."""
    model = Model("cassie")
    s, force, want = placed_state(model)
    nenv = len(want)
    off = ec.rules()
    a = ec.copy_state(s)
    emu_end_episodes(a, model.pod, off, 0, nenv, False)
    assert not a["done"].any() and not a["reason"].any()
    for key, bit in (("min_height", ec.DONE_HEIGHT), ("min_upright", ec.DONE_UPRIGHT), ("max_steps", ec.DONE_TIME),
                     ("warn_mask", ec.DONE_WARN), ("nonfinite", ec.DONE_NONFINITE)):
        one = ec.rules(**{key: RULES[key]})
        a, ref = ec.copy_state(s), ec.copy_state(s)
        emu_end_episodes(a, model.pod, one, 0, nenv, False)
        ec.end_episodes(ref, model.pod, one, 0, nenv, False)
        ec.assert_states_equal(a, ref, key)
        assert np.array_equal(a["reason"], want & bit) and a["reason"].any(), key


def test_rules_struct_layout_and_exported_symbols(built):
    """cm_episode_rules_t as ctypes derives it from cm_model.h against the compiled layout, and the new entry points in the product."""
    from cassie_amd._lib import CmEpisodeRules
    L = emu_py.lib()
    assert ctypes.sizeof(CmEpisodeRules) == L.emu_sizeof_episode_rules() == 32
    for which, f in enumerate(("min_height", "min_upright", "max_steps", "warn_mask", "nonfinite")):
        assert getattr(CmEpisodeRules, f).offset == L.emu_offsetof_episode_rules(which), f
    assert L.emu_offsetof_episode_rules(5) == -1
    product = ctypes.CDLL(LIB_PATH)
    for sym in ("phys_batch_episodes_enable", "phys_batch_episodes_set_bank", "phys_batch_episode_row_dim", "phys_batch_episode_ptr",
                "phys_batch_episode_bind", "phys_batch_end_episodes", "phys_batch_download_episodes", "phys_sizeof_episode_rules"):
        assert hasattr(product, sym), sym
    product.phys_sizeof_episode_rules.restype = ctypes.c_size_t
    assert product.phys_sizeof_episode_rules() == ctypes.sizeof(CmEpisodeRules)
    assert (P.DONE_HEIGHT, P.DONE_UPRIGHT, P.DONE_TIME, P.DONE_WARN, P.DONE_NONFINITE, P.DONE_FORCED) == ec.ALL_BITS
