"""The lean fast forms of the step kernel on the device (csrc/pk_stages.h: FEAT_READOUT / FEAT_PROF; csrc/step_plan.h: is_lean_form): the
fast kernels carry neither the read-out stores, nor the forward-mode exits, nor the stage stamps.  What they leave must be, to the last
bit, what the generic 63-row kernel alone leaves (set_fast_rows(False): FORM_ALONE*, both bits); a profiled launch takes the fast
kernel's _PROF form and leaves the same state with stamps in its buffer; a stepping launch with the read-out block on goes where the
read-out code is."""
import ctypes

import numpy as np
import pytest

import bench
import golden_physics as G
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd._lib import lib
from hostchain_py import device_state_bytes

pytestmark = pytest.mark.gpu

NLAUNCH = 4


def _targets(n, nlaunch):
    """reference example/cassietest_jac.py:106: pTarget = offset + U(-10, 10) -- every joint slammed into its limit."""
    return np.array([[bench.PD_OFFSET + np.random.default_rng(9100 + 53 * p + e).uniform(-10, 10, 10) for e in range(n)] for p in range(nlaunch)])


def _rollout(model, n, nsub, fast, inplace=2, drop=0.0):
    """NLAUNCH fused launches of nsub substeps of the drive-level PD workload under the stress targets -> everything the launches left,
    env-launches the fast kernel handed over (or finished in place), substeps the fast code completed itself, (plain, in place) launches"""
    name = model.name
    hf = G.terrain(name)
    q0 = np.tile(model.qpos_init(), (n, 1))
    q0[:, 2] -= drop
    if name == "cassie_hfield":
        for e in range(n):
            q0[e, 0], q0[e, 1] = G.start_xy(name, e)
    tg = _targets(n, NLAUNCH)
    b = Batch(model, n)
    try:
        b.set_fast_rows(fast)
        b.set_inplace(inplace)
        if hf is not None:
            b.set_hfield(hf)
        b.set(P.F_QPOS, q0)
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.forward()
        b.set_drive_mode(P.DRIVE_PD)
        rows, handed, done = [], 0, 0
        for p in range(NLAUNCH):
            b.set(P.F_PD_PTARGET, tg[p])
            b.step(nsub)
            rows.append(b.warnings()[1].copy())
            if fast and inplace == 0:
                prog = b.fast_rows_progress()
                handed += int(np.count_nonzero(prog < nsub))
                done += int(prog.sum())
        w, _ = b.warnings()
        rec = {f: b.get(getattr(P, "F_" + f)).tobytes() for f in ("QPOS", "QVEL", "QACC_WARMSTART", "QACC", "SENSORDATA", "ACTUATOR_VELOCITY", "TIME",
                                                                     "MEAS", "CTRL", "XPOS", "XQUAT")}
        rec["warn"], rec["info"] = w.tobytes(), np.array(rows).tobytes()
        rec["drive_state"] = b"".join(b"".join(device_state_bytes(s)) for s in b.get_drive_state(0, min(n, 64)))
        return rec, handed, done, (b.form_launches() if fast else (0, 0)), np.array(rows)
    finally:
        b.close()


def _same(got, ref, what):
    for f in ref:
        assert got[f] == ref[f], (what, f)


@pytest.mark.parametrize("n,nsub", [(64, 12), (2048, 10)])
def test_lean_fast_kernels_equal_the_generic_kernel_bit_for_bit_on_cassie(built, n, nsub):
    """64 envs x 12 substeps: the fast form in one piece (more than SMALL_BATCH_NSUB substeps); 2048 envs x 10: the smallest launch in
    chunks, two of 5.  The envs land from 6 cm within the first launch and the stress targets take them past the 31 rows of the
    fast code: hand-overs (plain form + list-walking pass), the in-place form (forced, and as the range chooses it)."""
    model = Model("cassie")
    assert bench.launch_chunks(n, nsub, True) == (2 if n == 2048 else 1)
    ref, _, _, _, rows = _rollout(model, n, nsub, fast=False, drop=0.06)
    assert rows[:, :, 1].max() > 31, "the workload must leave the fast code's rows"
    got, handed, done, forms, _ = _rollout(model, n, nsub, fast=True, inplace=0, drop=0.06)
    print("cassie %d x %d: %d of %d env-launches handed over, the fast code completed %d of %d substeps itself; launches (plain, in place) %s"
          % (n, nsub, handed, n * NLAUNCH, done, n * NLAUNCH * nsub, forms))
    assert handed > 0 and done > 0 and forms == (NLAUNCH, 0)
    _same(got, ref, "plain form")
    got, _, _, forms, _ = _rollout(model, n, nsub, fast=True, inplace=1, drop=0.06)
    assert forms == (0, NLAUNCH)
    _same(got, ref, "in-place form")
    if n == 64:
        got, _, _, forms, _ = _rollout(model, n, nsub, fast=True, inplace=2, drop=0.06)    # (the default: per range)
        assert sum(forms) == NLAUNCH
        _same(got, ref, "form by range")


@pytest.mark.parametrize("name", ["cassie_hfield", "cassie_tray_box"])
def test_lean_fast_kernels_equal_the_generic_kernel_bit_for_bit_on_the_other_models(built, name):
    model = Model(name)
    ref, _, _, _, _ = _rollout(model, 64, 12, fast=False)
    got, handed, done, forms, _ = _rollout(model, 64, 12, fast=True, inplace=0)
    print("%s 64 x 12: %d env-launches handed over, the fast code completed %d of %d substeps" % (name, handed, done, 64 * NLAUNCH * 12))
    assert done > 0
    _same(got, ref, "plain form")
    if name == "cassie_hfield":
        got, _, _, forms, _ = _rollout(model, 64, 12, fast=True, inplace=1)
        assert forms == (0, NLAUNCH)
        _same(got, ref, "in-place form")


# the stamps a two-wave fast kernel leaves, in program order per wave (tools/stage_profile.py names them)
WAVE0 = [0, 1, 17, 33, 5, 24, 34, 8, 9, 10, 11, 37]
WAVE1 = [35, 36, 2, 3, 38, 4, 6, 7, 47, 39, 12, 13, 14]


def _standing(model, n, drop=0.0):
    b = Batch(model, n)
    q0 = np.tile(model.qpos_init(), (n, 1))
    q0[:, 2] -= drop
    b.set(P.F_QPOS, q0)
    hi = np.array([model.pod.act_ctrlrange[u][1] for u in range(model.pod.nu)])
    b.set(P.F_CTRL, 0.3 * hi * np.random.default_rng(5).uniform(-1, 1, (n, model.pod.nu)))
    return b


def _state(b):
    return {f: b.get(getattr(P, "F_" + f)).tobytes() for f in ("QPOS", "QVEL", "QACC_WARMSTART", "QACC", "SENSORDATA", "ACTUATOR_VELOCITY", "TIME", "XPOS", "XQUAT")}


def test_profiled_launch_leaves_the_state_of_an_unprofiled_one_and_its_stamps(cassie):
    n, nsub = 64, 6
    a, b = _standing(cassie, n), _standing(cassie, n)
    try:
        a.step(nsub)
        st = b.profile_step(nsub)
        _same(_state(b), _state(a), "profiled")
        assert b.form_launches() == (1, 0) and a.form_launches()[0] + a.form_launches()[1] == 1    # (both took a fast kernel; the profiled one its plain form)
        for wave, chain in (("wave 0", WAVE0), ("wave 1", WAVE1)):
            s = st[:, chain]
            assert (s != 0).all(), (wave, np.argwhere(s == 0)[:4].tolist())
            assert (np.diff(s, axis=1) >= 0).all(), wave
        # ... and the next, unprofiled launch goes back to a lean form and goes on from the same state
        a.step(nsub)
        b.step(nsub)
        _same(_state(b), _state(a), "behind the profiled launch")
    finally:
        a.close()
        b.close()


def test_stepping_launch_with_the_read_out_block_on_fills_it_like_a_forward_pass(cassie, built):
    """The read-out block on: the launcher takes the instantiation that has the read-out code (never a lean form).  Its block is the
    read-out of the launch's last substep -- what a forward read-out pass writes on the state that substep started from."""
    import emu_py
    L, h = lib(), ctypes.c_void_p
    E = emu_py.lib()
    E.emu_sizeof_ext.restype = ctypes.c_ulong
    size = int(E.emu_sizeof_ext())
    n, nsub = 1024, 6      # (more than SMALL_BATCH envs: without the block a launch of any length takes the fast kernel)

    def read_out(b):
        buf = (ctypes.c_char * (size * n))()
        assert L.phys_batch_download_ext(h(b._h), buf, 0, n) == 0
        return bytes(buf)

    # (6 cm into the ground: contacts, so the block's contact records and forces are not empty)
    a, b, c = _standing(cassie, n, 0.06), _standing(cassie, n, 0.06), _standing(cassie, n, 0.06)
    try:
        for x in (a, b, c):
            x.set_inplace(0)
            x.step(nsub - 1)                            # a lean fast kernel
            assert x.form_launches() == (1, 0)
        assert L.phys_batch_enable_ext(h(a._h), 1) == 0 and L.phys_batch_enable_ext(h(b._h), 1) == 0    # (both blocks start cleared)
        a.step(1)                                       # the read-out block on: the stepping launch takes the generic kernel ...
        assert a.form_launches() == (1, 0)
        b.forward()                                     # ... and fills the block like the forward read-out pass on the same state
        ext_a, ext_b = read_out(a), read_out(b)
        assert np.frombuffer(ext_a, dtype=np.uint8).any()
        assert ext_a == ext_b
        assert L.phys_batch_enable_ext(h(b._h), 0) == 0
        b.step(1)
        c.step(1)                                       # (no block: a lean fast kernel again)
        assert c.form_launches() == (2, 0) and b.form_launches() == (2, 0)
        _same(_state(a), _state(c), "read-out launch against the lean one")
        _same(_state(b), _state(c), "behind the forward pass")
    finally:
        a.close()
        b.close()
        c.close()
