"""Wave 1's sensor stage behind the barrier J (csrc/env_step_wave1.inc, env_step: sensors_behind_j): in the two-wave forms of the plain
32-dof kernels (and, in the emulator's build, of its height-field-capable bodies: Makefile, EMU_FLAGS) the stage runs beside wave 0's
half solve and tells wave 0 through cmd[6] when it is done with the body tiles, in front of whose
region's first store -- the staging store of Y, csrc/env_step_solve.inc -- wave 0 waits.  Only the place of one stage and of one wait
differs from the one-wave form: every byte a launch leaves must be the one-wave form's, whichever wave the scheduler prefers (the
emulator's wave_schedule: 1 = wave 0 runs until it is blocked, so wave 1's sensor stage starts as late as it can, with wave 0 already
at the new wait; 2 = wave 1 does, so the stage starts the moment J opens), with the env's LDS block poisoned, through hand-overs, the
in-place code and a diverged env.  A wait on a flag nobody publishes would not fail an assertion here: the emulated launch would not end."""
import numpy as np
import pytest

import emu_py
from test_lean_forms import LeanEmuBatch, ProfiledEmuBatch

ONE_WAVE = dict(fast_rows=1)
TWO_WAVES = dict(fast_rows=1, two_waves=1)
IN_PLACE = dict(fast_rows=1, two_waves=1, inplace=1)
DIVERGED = 8                                    # WARN_DIVERGED (csrc/pk_types.h)


def _launch(model, settings, nenv, nsub, drop, amp, batch=LeanEmuBatch, nan_env=None):
    """One fused launch of nsub substeps of the benchmark's workload (config 2: drive-level PD with the safety layer) from the init pose,
    env e's pelvis lowered by drop[e] and its targets spread by amp[e] rad about the benchmark's -> the bytes the launch left, info, the batch."""
    import bench
    from cassie_amd import phys as P
    from hostchain_py import device_state_bytes
    pod = model.pod
    with emu_py.settings(**settings):
        emu = batch(pod, nenv)
        emu.qpos[:] = model.qpos_init()
        emu.qpos[:, 2] -= np.asarray(drop)
        if pod.nhfpair > 0:
            import test_hfield
            emu.hfield = test_hfield.terrain()
        emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (nenv, 1)), np.tile(bench.PD_KD, (nenv, 1))
        emu.forward()
        emu.drive_mode = P.DRIVE_PD_SAFE
        emu.pd_ptarget = np.array([bench.PD_OFFSET + np.random.default_rng(4100 + e).uniform(-amp[e], amp[e], 10) for e in range(nenv)])
        if nan_env is not None:
            emu.qvel[nan_env, 7] = np.nan
        emu.step(nsub)
    got = {f: getattr(emu, f).tobytes() for f in ("sensordata", "meas", "qpos", "qvel", "qacc_warmstart", "qacc", "actuator_velocity", "ctrl", "warn", "info")}
    got["drive_state"] = [device_state_bytes(emu.drive_state[e]) for e in range(nenv)]
    return got, emu.info.copy(), emu


def _same(got, ref, what):
    for f in ref:
        assert got[f] == ref[f], (what, f)


# 8 envs x 12 substeps: env e starts 3 e mm lower, so that some stand in the air and the others on their feet (four contacts: 28 rows)
N, NSUB = 8, 12
DROPS = [0.003 * e for e in range(N)]
CALM = [0.3] * N

_refs = {}


def _ref(model, key, *a, **kw):
    """the one-wave fast form's bytes of a workload, computed once"""
    if key not in _refs:
        _refs[key] = _launch(model, ONE_WAVE, *a, **kw)
    return _refs[key]


def test_two_wave_fast_form_equals_the_one_wave_form_bit_for_bit(cassie, built):
    from cassie_amd import phys as P
    ref, info, emu = _ref(cassie, "cassie", N, NSUB, DROPS, CALM)
    assert (info[:, 0] > 0).any() and info[:, 1].max() <= 31, "an env in contact, every env inside the fast code's rows"
    assert emu.counters.fast_bails <= N // 2, "most envs ran the substeps nsub - 2 and nsub - 1 in the fast code: the IMU words"
    assert np.abs(emu.meas[:, P.MEAS_ORIENTATION:P.MEAS_ORIENTATION + 4]).sum(axis=1).all() and np.abs(emu.meas[:, P.MEAS_LINACC:P.MEAS_LINACC + 3]).sum(axis=1).all()
    got, _, _ = _launch(cassie, TWO_WAVES, N, NSUB, DROPS, CALM)
    _same(got, ref, "two waves")


def test_in_place_form_with_an_env_over_its_rows_equals_the_one_wave_form(cassie, built):
    amp = [10.0] + CALM[1:]                         # (env 0: the stress targets -- every joint slammed into its limit)
    drops = [0.06] + DROPS[1:]
    ref, info, emu = _ref(cassie, "cassie_over", N, NSUB, drops, amp)
    assert info[0, 1] > 31 or emu.counters.fast_bails > 0, "env 0 must leave the fast code's rows"
    assert emu.counters.fast_bails > 0
    got, _, _ = _launch(cassie, IN_PLACE, N, NSUB, drops, amp)
    _same(got, ref, "in place")
    got, _, _ = _launch(cassie, dict(IN_PLACE, inplace_stay_rows=27, wave_schedule=1, poison_lds=1), N, NSUB, drops, amp)
    _same(got, ref, "in place, staying")


def test_height_field_two_wave_fast_form_equals_the_one_wave_form(built):
    from cassie_amd import Model
    model = Model("cassie_hfield")
    n, drops = 4, [0.0, 0.05, 0.10, 0.16]
    ref, info, _ = _ref(model, "hfield", n, NSUB, drops, CALM[:n])
    assert (info[:, 0] > 0).any()
    for s in (TWO_WAVES, dict(TWO_WAVES, wave_schedule=1, poison_lds=1)):
        got, _, _ = _launch(model, s, n, NSUB, drops, CALM[:n])
        _same(got, ref, s)


@pytest.mark.parametrize("schedule", [1, 2])
def test_order_of_the_sensor_stage_and_the_staging_store_holds_under_either_wave_held(cassie, built, schedule):
    """schedule 1 holds wave 1 right behind J for as long as the scheduler allows: wave 0 runs its half solve and is AT the new wait
    before the sensor stage has read one tile -- past it, the staged matrix would be what the stage reads.  schedule 2 holds wave 0 at
    J: the sensor stage runs at once, on this substep's tiles (wave 0 wrote them in front of J), never on what the substep before left
    of Y and the Gram matrix there.  LDS poisoned: a tile read before anybody wrote it is a NaN pattern in the results."""
    ref, _, _ = _ref(cassie, "cassie", N, NSUB, DROPS, CALM)
    got, _, emu = _launch(cassie, dict(TWO_WAVES, wave_schedule=schedule, poison_lds=1), N, NSUB, DROPS, CALM, batch=ProfiledEmuBatch)
    _same(got, ref, schedule)
    # (the profiled form of the same launch: wave 0 went through the wait and wave 1 through the stage behind J -- both halves of slot 15,
    # lengths on the emulator's clock, which reads 0)
    assert (emu.stamps[:, 15] == 0).all(), emu.stamps[:, 15]
    assert not np.isnan(emu.sensordata).any() and not np.isnan(emu.meas).any()


@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_hand_over_and_divergence_end_the_launch_with_nobody_at_the_new_flag(cassie, built, schedule):
    """env 0 is handed over in the middle of the launch (the plain form: to the pass behind the kernel), env 3 starts with a NaN in qvel:
    both waves leave through cmd[0], in front of J -- the launch ends, and leaves what the one-wave form leaves."""
    amp = [10.0] + CALM[1:]
    drops = [0.06] + DROPS[1:]
    ref, info, emu = _ref(cassie, "cassie_exits", N, NSUB, drops, amp, nan_env=3)
    assert emu.counters.fast_bails > 0 and emu.warn[3] & DIVERGED and not emu.warn[[0, 1, 2, 4, 5, 6, 7]].any()
    got, _, emu2 = _launch(cassie, dict(TWO_WAVES, wave_schedule=schedule, poison_lds=1), N, NSUB, drops, amp, nan_env=3)
    assert emu2.counters.fast_bails == emu.counters.fast_bails
    # (NaN bytes compare like any others)
    _same(got, ref, schedule)


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [0, 1])
def test_two_wave_fast_kernel_equals_the_one_wave_kernel_bit_for_bit_on_the_device(cassie, built, inplace):
    """64 envs x 10 substeps, drive-pd-safe: the two-wave fast kernel (plain, and with the in-place form forced) against
    set_waves_per_env(1).  The envs land from 0 .. 6 cm; the last eight get the stress targets and leave the fast code's rows."""
    import bench
    from cassie_amd import Batch
    from cassie_amd import phys as P
    from hostchain_py import device_state_bytes
    n, nsub = 64, 10
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.06 * (np.arange(n) % 8) / 7.0
    tg = np.array([bench.PD_OFFSET + np.random.default_rng(5200 + e).uniform(-1, 1, 10) * (10.0 if e >= n - 8 else 0.3) for e in range(n)])

    def rollout(waves):
        b = Batch(cassie, n)
        try:
            b.set_waves_per_env(waves)
            b.set_inplace(inplace)
            b.set(P.F_QPOS, q0)
            b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
            b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
            b.forward()
            b.set_drive_mode(P.DRIVE_PD_SAFE)
            b.set(P.F_PD_PTARGET, tg)
            rows = []
            for _ in range(2):
                b.step(nsub)
                rows.append(b.warnings()[1].copy())
            rec = {f: b.get(getattr(P, "F_" + f)).tobytes() for f in ("SENSORDATA", "MEAS", "QPOS", "QVEL", "QACC_WARMSTART", "QACC", "ACTUATOR_VELOCITY", "CTRL")}
            rec["warn"], rec["info"] = b.warnings()[0].tobytes(), np.array(rows).tobytes()
            rec["drive_state"] = b"".join(b"".join(device_state_bytes(s)) for s in b.get_drive_state(0, n))
            return rec, np.array(rows), b.form_launches()
        finally:
            b.close()

    ref, rows, _ = rollout(1)
    assert rows[:, :, 0].max() > 0 and rows[:, :, 1].max() > 31 and rows[:, :, 1].min() <= 31
    got, _, forms = rollout(2)
    assert forms == ((0, 2) if inplace else (2, 0))
    _same(got, ref, "two waves, in place" if inplace else "two waves")
