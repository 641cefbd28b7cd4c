"""The real kernel source (physics_kernel.h), executed lane-by-lane on the CPU wave
emulator, against the scalar oracle.  Catches kernel logic errors without a GPU."""
import numpy as np
import pytest

from emu_py import EmuBatch
from oracle_py import Oracle


def _drive(cassie, nsteps, teacher, seed, ctrl_scale=1.0, nenv=1):
    pod = cassie.pod
    rng = np.random.default_rng(seed)
    q0 = cassie.qpos_init()
    orcs = [Oracle(pod, q0) for _ in range(nenv)]
    emu = EmuBatch(pod, nenv)
    emu.qpos[:] = q0
    v0 = rng.uniform(-0.3, 0.3, (nenv, pod.nv))
    emu.qvel[:] = v0
    for e, o in enumerate(orcs):
        o.qvel[:] = v0[e]
    hi = np.array([pod.act_ctrlrange[u][1] for u in range(pod.nu)])
    worst = dict(q=0.0, v=0.0, s=0.0)
    for s in range(nsteps):
        if s % 10 == 0:
            c = ctrl_scale * hi * rng.uniform(-1, 1, (nenv, pod.nu))
            emu.ctrl[:] = c
            for e, o in enumerate(orcs):
                o.ctrl[:] = c[e]
        emu.step()
        for e, o in enumerate(orcs):
            o.step()
            assert (emu.info[e, 0], emu.info[e, 1], emu.info[e, 2]) == (o.d.ncon, o.d.nefc, o.d.solver_iter)
            worst["q"] = max(worst["q"], np.max(np.abs(emu.qpos[e] - o.qpos)))
            worst["v"] = max(worst["v"], np.max(np.abs(emu.qvel[e] - o.qvel)))
            worst["s"] = max(worst["s"], np.max(np.abs(emu.sensordata[e] - o.sensordata)))
            if teacher:
                emu.qpos[e], emu.qvel[e], emu.qacc_warmstart[e] = o.qpos, o.qvel, o.qacc_warmstart
    assert not emu.warn.any()
    return worst


def test_teacher_forced_steps(cassie):
    w = _drive(cassie, 300, True, seed=1, nenv=2)
    assert w["q"] < 1e-14 and w["v"] < 1e-10 and w["s"] < 1e-9, w


def test_free_running_600_steps_with_contacts(cassie):
    w = _drive(cassie, 600, False, seed=2)
    # north_star bar is 1e-6 relative over 1000 steps; the emulated kernel is far inside it
    assert w["q"] < 1e-9 and w["v"] < 1e-7, w


def test_forward_only_matches_and_leaves_state(cassie):
    pod = cassie.pod
    o = Oracle(pod, cassie.qpos_init())
    o.forward()
    emu = EmuBatch(pod, 1)
    emu.qpos[:] = cassie.qpos_init()
    q_before = emu.qpos.copy()
    emu.forward()
    assert np.array_equal(q_before, emu.qpos)
    assert np.allclose(emu.qacc[0], o.qacc, rtol=1e-9, atol=1e-9)
    assert np.allclose(emu.sensordata[0], o.sensordata, atol=1e-10)


def test_multi_substep_launch_equals_single_steps(cassie):
    pod = cassie.pod
    a, b = EmuBatch(pod, 1), EmuBatch(pod, 1)
    for x in (a, b):
        x.qpos[:] = cassie.qpos_init()
        x.ctrl[:] = 0.5
    a.step(nsub=25)
    for _ in range(25):
        b.step()
    assert np.abs(a.qpos - b.qpos).max() < 1e-11 and np.abs(a.qvel - b.qvel).max() < 1e-9
    assert abs(a.time[0] - 25 * pod.timestep) < 1e-15


def test_applied_forces(cassie):
    pod = cassie.pod
    rng = np.random.default_rng(5)
    o = Oracle(pod, cassie.qpos_init())
    emu = EmuBatch(pod, 1)
    emu.qpos[:] = cassie.qpos_init()
    emu.qfrc_applied = rng.uniform(-5, 5, (1, pod.nv))
    emu.xfrc_applied = np.zeros((1, pod.nbody * 6))
    emu.xfrc_applied[0, 6 * 1: 6 * 1 + 6] = [10, -5, 30, 1, 2, -1]       # pelvis
    emu.xfrc_applied[0, 6 * 13: 6 * 13 + 3] = [0, 0, 20]                  # left foot
    o.qfrc_applied[:] = emu.qfrc_applied[0]
    o.xfrc_applied[:] = emu.xfrc_applied.reshape(pod.nbody, 6)
    for _ in range(20):
        emu.step()
        o.step()
    assert np.max(np.abs(emu.qpos[0] - o.qpos)) < 1e-12
    assert np.max(np.abs(emu.qvel[0] - o.qvel)) < 1e-10


@pytest.mark.parametrize("two_waves", [0, 1])
def test_divergence_flag_is_sticky_and_state_untouched(cassie, two_waves):
    """A NaN in the state (caught at the top of the substep) and a diverged qacc (caught behind the solve -- in the two-wave form
    by wave 1, which tells wave 0 at the substep's last barrier): sticky flag, state left as it is."""
    import emu_py
    with emu_py.settings(two_waves=two_waves, fast_rows=two_waves):
        emu = EmuBatch(cassie.pod, 1)
        emu.qpos[:] = cassie.qpos_init()
        emu.qvel[0, 3] = np.nan
        q = emu.qpos.copy()
        emu.step(3)
        assert emu.warn[0] & 8
        assert np.array_equal(q, emu.qpos)
        # a finite state whose acceleration is not: a torque of 1e300 passes the state check and overflows qacc
        emu = EmuBatch(cassie.pod, 1)
        emu.qpos[:] = cassie.qpos_init()
        emu.qfrc_applied = np.zeros((1, cassie.pod.nv)); emu.xfrc_applied = np.zeros((1, cassie.pod.nbody, 6))
        emu.qfrc_applied[0, 8] = 1e306
        q, v = emu.qpos.copy(), emu.qvel.copy()
        emu.step(3)
        assert emu.warn[0] & 8
        assert np.array_equal(q, emu.qpos) and np.array_equal(v, emu.qvel)
        emu.forward()                                     # (a forward pass over the same state: same verdict, no hang)
        assert emu.warn[0] & 8


def test_on_device_pd_mode(cassie):
    """PD targets instead of torques: kernel-side PD + motor speed-torque limit vs the oracle's co_pd_ctrl."""
    pod = cassie.pod
    rng = np.random.default_rng(9)
    offset = np.array([0.0045, 0, 0.4973, -1.1997, -1.5968] * 2)
    kp = np.array([70, 70, 100, 100, 50] * 2, dtype=float)
    kd = np.array([7, 7, 8, 8, 5] * 2, dtype=float)
    pt = offset + rng.uniform(-0.3, 0.3, 10)
    o = Oracle(pod, cassie.qpos_init())
    emu = EmuBatch(pod, 1)
    emu.qpos[:] = cassie.qpos_init()
    emu.pd_ptarget, emu.pd_kp, emu.pd_kd = pt[None].copy(), kp[None].copy(), kd[None].copy()
    for _ in range(120):
        o.pd_ctrl(pt, kp, kd)
        o.step()
        emu.step()
    assert np.max(np.abs(emu.qpos[0] - o.qpos)) < 1e-11
    assert o.qpos[2] > 0.8          # still standing-ish under PD after 60 ms


def test_runtime_topology_instantiation_matches_static_one(cassie):
    """The generic kernel (dof-tree masks read from the model at run time) must agree with the
    compile-time-topology instantiation used for the in-scope models.  The static one eliminates the mass matrix
    height by height, the generic one dof by dof: the same updates in another order, so the agreement is to
    rounding, not bitwise."""
    import emu_py
    pod = cassie.pod
    a, b = EmuBatch(pod, 1), EmuBatch(pod, 1)
    for x in (a, b):
        x.qpos[:] = cassie.qpos_init()
        x.ctrl[:] = [1.0, -2.0, 3.0, -4.0, 0.5, -1.0, 2.0, -3.0, 4.0, -0.5]
    a.step(40)
    with emu_py.settings(force_runtime_topology=1):
        b.step(40)
    assert np.abs(a.qpos - b.qpos).max() < 1e-11 and np.abs(a.qvel - b.qvel).max() < 1e-9


def test_guarded_pgs_sweep_agrees_with_the_speculative_one(cassie):
    """The kernel runs PGS sweeps with the cost guard evaluated after the sweep and falls back to the row-by-row
    guarded sweep only when a guard would have fired (rare).  Forcing the fallback on every sweep must give the same
    trajectory to rounding."""
    import emu_py
    pod = cassie.pod
    a, b = EmuBatch(pod, 1), EmuBatch(pod, 1)
    for x in (a, b):
        x.qpos[:] = cassie.qpos_init()
        x.ctrl[:] = [1.0, -2.0, 3.0, -4.0, 0.5, -1.0, 2.0, -3.0, 4.0, -0.5]
    a.step(60)
    with emu_py.settings(force_guarded_pgs=1):
        b.step(60)
    assert np.abs(a.qpos - b.qpos).max() < 1e-11 and np.abs(a.qvel - b.qvel).max() < 1e-9


def test_joint_limit_rows_and_deep_penetration_from_qpos0(cassie):
    """qpos0 is not a rest pose: four limit rows are active and the feet start below the floor, so
    the first steps exercise limit rows, many simultaneous contacts and large corrective forces."""
    pod = cassie.pod
    q0 = np.array([pod.qpos0[i] for i in range(pod.nq)])
    o = Oracle(pod, q0)
    emu = EmuBatch(pod, 1)
    emu.qpos[:] = q0
    saw_limits = False
    for s in range(60):
        emu.step()
        o.step()
        assert (emu.info[0, 0], emu.info[0, 1], emu.info[0, 2]) == (o.d.ncon, o.d.nefc, o.d.solver_iter), s
        saw_limits |= o.d.nefc > 12 + 4 * o.d.ncon
        assert np.max(np.abs(emu.qpos[0] - o.qpos)) < 1e-9 and np.max(np.abs(emu.qvel[0] - o.qvel)) < 1e-6, s
    assert saw_limits


@pytest.mark.parametrize("caps", [(16, 63), (32, 127), (20, 70)])
def test_contact_and_row_caps_drop_the_same_rows_as_the_oracle(cassie, caps):
    """Sunk into the floor, every collision geom touches it.  With the caps of a model WITHOUT a 127-row instantiation (16 contacts /
    63 rows: cm_model_t::maxcon / maxefc, here set by hand) that is more contacts and more rows than fit; with the 32 / 127 of the
    Cassie models everything fits -- 17 contacts, 80 rows: the solve spread over both wavefronts; with 20 / 70 the 127-row
    instantiation itself drops rows (first pose).  Oracle and kernel must raise the same warning bits and keep the same (first) contacts and rows;
    a second pose (on its back, 13 contacts) overflows the rows only."""
    pod = cassie.pod
    keep = (pod.maxcon, pod.maxefc)
    pod.maxcon, pod.maxefc = caps
    try:
        for z, quat, want_bits in ((0.0, [1.0, 0.0, 0.0, 0.0], 3), (-0.2, [np.cos(np.pi / 4), 0.0, np.sin(np.pi / 4), 0.0], 2)):
            q0 = cassie.qpos_init().copy()
            q0[2] = z
            q0[3:7] = quat
            o = Oracle(pod, q0)
            emu = EmuBatch(pod, 1)
            emu.qpos[:] = q0
            seen, rows = 0, 0
            for s in range(12):
                emu.step()
                o.step()
                assert (emu.info[0, 0], emu.info[0, 1], emu.info[0, 2]) == (o.d.ncon, o.d.nefc, o.d.solver_iter), s
                want = (1 if o.d.warn_contact_full else 0) | (2 if o.d.warn_constraint_full else 0) | (4 if o.d.warn_unsupported_pair else 0)
                assert int(emu.warn[0]) & 7 == want, (s, int(emu.warn[0]), want)
                seen |= want
                rows = max(rows, o.d.nefc)
                assert np.max(np.abs(emu.qpos[0] - o.qpos)) < 1e-8, s
            if caps == (16, 63):
                assert seen & want_bits == want_bits
            elif caps == (32, 127):
                # (first pose: 17 contacts, 80 rows -- the rows past 64 are wave 1's; second pose: 13 contacts, exactly 64 rows -- every lane
                # of wave 0 a row, none on wave 1)
                assert seen == 0 and (rows > 64 if want_bits == 3 else rows == 64), (seen, rows)
            else:
                assert (seen == 2 and 64 < rows <= 70) if want_bits == 3 else (seen == 0 and rows == 64), (seen, rows)   # (limit rows come and go: 68 .. 70 of the 80)
    finally:
        pod.maxcon, pod.maxefc = keep


def test_kernel_never_reads_lds_it_has_not_written(cassie):
    """LDS is not initialised on the device: whatever a previous kernel left there -- possibly NaN bit patterns on a fresh
    box -- must not reach the results.  The emulator fills the whole EnvShared block with 0xff bytes (NaNs) at the start of
    every launch; trajectories through free fall, first contacts and standing must be identical to the un-poisoned run.
    (Round 2 regression: the centre-of-mass row of the static world body was read -- under an all-zero mask, by
    multiplication -- without ever being written.)"""
    import bench
    import emu_py
    pod = cassie.pod
    out = []
    for poison in (0, 1):
        with emu_py.settings(poison_lds=poison):
            emu = EmuBatch(pod, 2)
            emu.qpos[:] = cassie.qpos_init()
            emu.qpos[1, 2] -= 0.02
            emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (2, 1)), np.tile(bench.PD_KD, (2, 1))
            emu.pd_ptarget = np.ascontiguousarray(bench.pd_targets([3, 4], 1)[0])
            emu.step(50)
            emu.step(1)
            emu.step(40)
            out.append((emu.qpos.copy(), emu.qvel.copy(), emu.sensordata.copy(), emu.warn.copy(), emu.info.copy()))
    assert not out[1][3].any() and out[1][4][:, 0].max() >= 1          # no divergence flag, contacts happened
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    # the check is not vacuous: with the round-2 bug reinstated (the emulator's test hook skips the once-per-launch
    # initialisation of the centre-of-mass rows) the poisoned run differs from the clean one or raises the divergence flag
    def fifty(poison, skip):
        with emu_py.settings(skip_com_init=skip, poison_lds=poison):
            emu = EmuBatch(pod, 2)
            emu.qpos[:] = cassie.qpos_init()
            emu.qpos[1, 2] -= 0.02
            emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (2, 1)), np.tile(bench.PD_KD, (2, 1))
            emu.pd_ptarget = np.ascontiguousarray(bench.pd_targets([3, 4], 1)[0])
            emu.step(50)
            return emu.qpos.copy(), emu.warn.copy()
    clean, buggy = fifty(0, 0), fifty(1, 1)
    assert buggy[1].any() or not np.array_equal(clean[0], buggy[0])


@pytest.mark.parametrize("name,steps,drive", [("cassie_tray_box", 260, False), ("cassie_hfield", 120, False), ("cassie", 90, True)])
def test_lds_poison_on_the_other_models_and_modes(name, steps, drive, built):
    """Same check for the 40-dof instantiation with box pairs (the cube lands on the tray), the height-field pre-pass and
    the drive-level mode."""
    import bench
    import emu_py
    from cassie_amd import Model
    from cassie_amd import phys as P
    model = Model(name)
    pod = model.pod
    hf = None
    if name == "cassie_hfield":
        hf = np.random.default_rng(99).random((200, 200)).astype(np.float32).ravel()
    out = []
    for poison in (0, 1):
        with emu_py.settings(poison_lds=poison):
            emu = EmuBatch(pod, 1)
            emu.qpos[:] = model.qpos_init()
            if hf is not None:
                emu.hfield = hf
                emu.qpos[0, 0] = 0.6
            if name == "cassie_tray_box":
                emu.qpos[0, 37] = 1.20                      # the cube starts just above the tray
            emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (1, 1)), np.tile(bench.PD_KD, (1, 1))
            emu.pd_ptarget = np.ascontiguousarray(bench.pd_targets([5], 1)[0])
            if drive:
                emu.forward()
                emu.drive_mode = P.DRIVE_PD
            for _ in range(steps // 10):
                emu.step(10)
            out.append((emu.qpos.copy(), emu.qvel.copy(), emu.sensordata.copy(), emu.meas.copy(), emu.warn.copy(), emu.info.copy()))
    assert not out[1][4].any() and out[1][5][0, 0] >= 1
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_packed_factor_rows_address_the_same_slots_from_every_side(built):
    """The 40-dof tray kernel keeps its two factors in block-dense rows (ck::LPack, 392 slots instead of 820) so that four of
    its workgroups fit a CU.  The slot of entry (k, i) is computed three ways in the kernel -- at compile time, from the
    storing lane i of row k, and from the lane that owns row k / column i -- and all must agree, for the packed layout and
    for the dense one."""
    import emu_py
    lib = emu_py.lib()
    assert lib.emu_lpack_check() == 0
    assert lib.emu_lpack_count(0) == 32 * 33 // 2          # cassie.xml keeps the full triangle (index = base + immediate)
    assert lib.emu_lpack_count(1) == 392                   # 15 trunk + 2 x 156 leg + 51 cube + 13 padding + 1 dump slot


@pytest.mark.parametrize("drive", [False, True])
def test_row_capped_fast_kernel_hands_over_mid_launch_and_changes_nothing(cassie, drive):
    """The row-capped fast instantiation (31 rows) ahead of the full one, as phys_batch.hip launches them: an env that
    meets a substep with more rows in the MIDDLE of a fused launch is handed over through PhysIO::progress and finished by
    the full instantiation.  State, outputs, solver statistics and (drive mode) filter histories / delay lines must be bit
    for bit those of the full instantiation alone.  Workload: the +-10 rad stress targets, which push joints into their
    limits within the first launches (rows pass 31 while the robot is still on its feet)."""
    import bench
    import emu_py
    from cassie_amd import phys as P
    from hostchain_py import device_state_bytes
    pod = cassie.pod
    n = 3
    tg = np.empty((6, n, 10))
    for e in range(n):
        tg[:, e, :] = bench.PD_OFFSET + np.random.default_rng(4321 + e).uniform(-10, 10, (6, 10))
    out, bails = [], 0
    for fast in (0, 1):
        with emu_py.settings(fast_rows=fast) as run:
            emu = EmuBatch(pod, n)
            emu.qpos[:] = cassie.qpos_init()
            emu.qpos[:, 2] -= 0.2                               # start in contact so that rows are plenty from the first step
            emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (n, 1)), np.tile(bench.PD_KD, (n, 1))
            if drive:
                emu.forward()
                emu.drive_mode = P.DRIVE_PD
            rows = []
            for p in range(6):
                emu.pd_ptarget = np.ascontiguousarray(tg[p])
                emu.step(25)
                rows.append(emu.info[:, 1].copy())
            out.append((emu.qpos.copy(), emu.qvel.copy(), emu.qacc_warmstart.copy(), emu.sensordata.copy(), emu.meas.copy(), emu.info.copy(),
                        emu.warn.copy(), emu.time.copy(), [device_state_bytes(emu.drive_state[e]) for e in range(n)], np.array(rows)))
        if fast:
            bails = run.fast_bails
    assert out[0][9].max() > 31 and out[0][9].min() <= 31          # launches on both sides of the fast kernel's capacity
    assert bails > 0                                                # and the hand-over really happened
    for a, b in zip(out[0], out[1]):
        if isinstance(a, list):
            assert a == b
        else:
            assert a.tobytes() == b.tobytes()


# ---- the two-wave form (NW = 2): wave 1 runs the mass-matrix stage group beside wave 0's collision / velocity / row stages ----
def _two_wave_workload(model, drive, fast, two_waves, schedule, poison=False, nlaunch=5, nsub=12, stress=True):
    """A few fused launches of the benchmark's PD workload (optionally with the +-10 rad stress targets, which force hand-overs
    between the row-capped and the full instantiation); returns everything a launch leaves behind, as bytes, the solver statistics of
    every launch and the number of envs the workload's launches handed over."""
    import bench
    import emu_py
    from cassie_amd import phys as P
    from hostchain_py import device_state_bytes
    pod, n = model.pod, 2
    with emu_py.settings(fast_rows=1 if fast else 0, two_waves=1 if two_waves else 0, wave_schedule=schedule, poison_lds=1 if poison else 0):
        emu = EmuBatch(pod, n)
        emu.qpos[:] = model.qpos_init()
        emu.qpos[:, 2] -= 0.15
        if pod.nhfpair > 0:
            import test_hfield
            emu.hfield = test_hfield.terrain()
        emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (n, 1)), np.tile(bench.PD_KD, (n, 1))
        if drive:
            emu.forward()
            emu.drive_mode = P.DRIVE_PD
        rows = []
        amp = (10.0 if stress else 0.3) if isinstance(stress, bool) else float(stress)   # (a number: the targets' amplitude in rad)
        for p in range(nlaunch):
            tg = np.empty((n, 10))
            for e in range(n):
                tg[e] = bench.PD_OFFSET + np.random.default_rng(977 + 31 * p + e).uniform(-amp, amp, 10)
            emu.pd_ptarget = tg
            emu.step(nsub)
            rows.append(emu.info.copy())
        emu.forward()                                    # a forward-only pass goes through the same kernel (integrate = 0)
        return [emu.qpos.tobytes(), emu.qvel.tobytes(), emu.qacc_warmstart.tobytes(), emu.qacc.tobytes(), emu.sensordata.tobytes(),
                emu.actuator_velocity.tobytes(), emu.meas.tobytes(), emu.warn.tobytes(), emu.time.tobytes(), emu.xpos.tobytes(), emu.xquat.tobytes(),
                np.array(rows).tobytes(), [device_state_bytes(emu.drive_state[e]) for e in range(n)]], np.array(rows), emu.counters.fast_bails


@pytest.mark.parametrize("drive", [False, True])
def test_two_wave_form_is_bit_for_bit_the_one_wave_form_under_every_wave_schedule(cassie, drive):
    """NW = 2 computes every value by the same instructions from the same operands: state, outputs, solver statistics and the
    drive-level state must equal the one-wave form's bit for bit -- with the waves taking turns, with wave 0 running ahead
    to every barrier and with wave 1 doing so (an LDS race between the waves would show as a difference between schedules),
    on a workload that hands envs over from the row-capped to the full instantiation in the middle of fused launches."""
    ref, rows, _ = _two_wave_workload(cassie, drive, fast=True, two_waves=False, schedule=0)
    assert rows[:, :, 1].max() > 31 and rows[:, :, 1].min() <= 31
    import emu_py
    for schedule in (0, 1, 2):
        with emu_py.settings(resume_grid=(2, 1, 3)[schedule]):      # workgroups of the pass that walks the hand-over list
            got, _, bails = _two_wave_workload(cassie, drive, fast=True, two_waves=True, schedule=schedule)
        assert bails > 0
        assert got == ref, schedule
    # the full instantiation alone, two waves
    got, _, _ = _two_wave_workload(cassie, drive, fast=False, two_waves=True, schedule=2)
    assert got == ref


def test_two_wave_form_never_reads_lds_it_has_not_written(cassie):
    """LDS filled with NaN patterns at the start of every launch: same bits (wave 1 reads only what wave 0 -- or itself -- has
    written in this launch)."""
    ref, _, _ = _two_wave_workload(cassie, True, fast=True, two_waves=False, schedule=0, nlaunch=3, stress=False)
    for schedule in (1, 2):
        got, _, _ = _two_wave_workload(cassie, True, fast=True, two_waves=True, schedule=schedule, poison=True, nlaunch=3, stress=False)
        assert got == ref


@pytest.mark.parametrize("name", ["cassie_hfield", "cassie_tray_box"])
def test_two_wave_form_on_the_other_models(name, built):
    from cassie_amd import Model
    model = Model(name)
    ref, _, _ = _two_wave_workload(model, True, fast=True, two_waves=False, schedule=0, nlaunch=2, nsub=8, stress=False)
    for schedule in (1, 2):
        got, _, _ = _two_wave_workload(model, True, fast=True, two_waves=True, schedule=schedule, poison=True, nlaunch=2, nsub=8, stress=False)
        assert got == ref


def test_tray_fast_instantiation_is_bit_for_bit_the_full_one(built):
    """cassie_tray_box.xml: the 47-row instantiation forms its Gram matrix on the matrix core through the staged tile's own LDS
    (physics_kernel.h, gram_in_place) and hands substeps with more rows over to the full instantiation, which forms the same
    chains on the vector unit: state, outputs and solver statistics must be those of the full instantiation alone, bit for
    bit -- at rest on the tray (32 .. 40 rows) and under the stress targets (rows past 47: hand-overs), LDS poisoned."""
    from cassie_amd import Model
    import emu_py
    model = Model("cassie_tray_box")
    margins = [model.pod.jnt_margin[j] for j in range(model.pod.njnt)]
    for stress in (False, True):
        # (the second round: every limited joint inside its limit's margin all the time -- 16 more rows while the robot still stands)
        for j in range(model.pod.njnt):
            model.pod.jnt_margin[j] = 10.0 if stress and model.pod.jnt_limited[j] else margins[j]
        ref, rows, _ = _two_wave_workload(model, True, fast=False, two_waves=False, schedule=0, nlaunch=3, nsub=10, stress=stress)
        got, _, bails = _two_wave_workload(model, True, fast=True, two_waves=False, schedule=0, poison=True, nlaunch=3, nsub=10, stress=stress)
        assert got == ref, stress
        if stress:
            assert rows[:, :, 1].max() > 47 and bails > 0, (rows[:, :, 1].max(), bails)
        else:
            assert 16 < rows[:, :, 1].max() <= 47 and bails == 0, (rows[:, :, 1].max(), bails)
    # the walking pass in its two-wave form (what phys_batch.hip launches behind the fast kernel)
    with emu_py.settings(resume_grid=1):
        got, _, bails = _two_wave_workload(model, True, fast=True, two_waves=True, schedule=1, nlaunch=3, nsub=10, stress=True)
    assert got == ref and bails > 0


@pytest.mark.parametrize("name", ["cassie", "cassie_hfield", "cassie_tray_box"])
def test_launch_in_chunks_is_bit_for_bit_the_launch_in_one_piece(name, built):
    """PhysIO::nchunk: the fast instantiation's launch as chunks of substeps, one workgroup per (env, chunk), a chunk loading what
    the chunk before it stored and ending like a launch of its own -- state, outputs, solver statistics and drive-level state must
    be those of the launch in one piece, with envs handed over to the full instantiation in the middle of chunks (stress
    targets), in both wave forms, with chunk counts that do and do not divide the substep count."""
    from cassie_amd import Model
    import emu_py
    model = Model(name)
    for stress in ((False, True) if name != "cassie_tray_box" else (False,)):   # (the 40-dof model's 47-row instantiation is not left under these targets: covered above)
        ref, rows, _ = _two_wave_workload(model, True, fast=True, two_waves=False, schedule=0, nlaunch=3, nsub=11, stress=stress)
        for chunks, two_waves in ((4, False), (3, True), (2, True)):
            with emu_py.settings(chunks=chunks):
                got, _, bails = _two_wave_workload(model, True, fast=True, two_waves=two_waves, schedule=1, poison=True, nlaunch=3, nsub=11, stress=stress)
            assert got == ref, (chunks, two_waves, stress)
            if stress:
                assert bails > 0
    # more chunks than substeps (the trailing chunks have nothing to do), and a chunk of a single substep
    if name == "cassie":
        for nsub in (2, 5):
            ref, _, _ = _two_wave_workload(model, True, fast=True, two_waves=True, schedule=0, nlaunch=4, nsub=nsub, stress=False)
            with emu_py.settings(chunks=4):
                got, _, _ = _two_wave_workload(model, True, fast=True, two_waves=True, schedule=2, nlaunch=4, nsub=nsub, stress=False)
            assert got == ref, nsub


def test_a_chunk_that_finds_its_producer_on_another_xcd_flags_the_env_and_tells_the_launcher(cassie):
    """A launch in chunks hands an env's state over through the L2 of ONE XCD (csrc/wave.h: publish_global at workgroup scope): the
    word carries the producer's XCD and the consumer checks it.  With the emulator's producers publishing from "XCD 3" (consumers
    run on 0) every env must carry WARN_CHUNK_PLACEMENT (16) and the launcher's fault word must be set; with producers on 0 neither."""
    import emu_py
    with emu_py.settings(chunks=3, producer_xcc=0) as run:
        got, _, _ = _two_wave_workload(cassie, True, fast=True, two_waves=True, schedule=1, nlaunch=2, nsub=9, stress=False)
    warn = np.frombuffer(got[7], dtype=np.int32)
    assert not (warn & 16).any() and run.chunk_fault == 0
    with emu_py.settings(chunks=3, producer_xcc=3) as run:
        got, _, _ = _two_wave_workload(cassie, True, fast=True, two_waves=True, schedule=1, nlaunch=2, nsub=9, stress=False)
    warn = np.frombuffer(got[7], dtype=np.int32)
    assert (warn & 16).all() and run.chunk_fault == 1


def test_127_row_instantiation_is_the_63_row_one_bit_for_bit_where_both_hold_the_substep(cassie):
    """The 127-row instantiation parks every row in LDS, picks it up again, and runs a substep of at most 64 rows on wave 0 alone
    through the 63-row instantiation's chain of operations (physics_kernel.h, wide_solve): a workload that never needs more than
    63 rows must come out of it bit for bit as out of the 63-row instantiation -- which is what lets an env move between the tiers
    in the middle of a launch, and a launch go in chunks, without a trace in the results."""
    pod = cassie.pod
    keep = (pod.maxcon, pod.maxefc)
    try:
        pod.maxcon, pod.maxefc = 32, 127       # (the caps CM_FLAG_HFPRISM gives a model: the 127-row instantiation steps it)
        wide, rows, _ = _two_wave_workload(cassie, True, fast=False, two_waves=True, schedule=1, poison=True, nlaunch=3)
        assert 31 < rows[:, :, 1].max() <= 63
        pod.maxcon, pod.maxefc = 16, 63
        for two_waves in (True, False):
            mid, _, _ = _two_wave_workload(cassie, True, fast=False, two_waves=two_waves, schedule=2, nlaunch=3)
            assert mid == wide, two_waves
    finally:
        pod.maxcon, pod.maxefc = keep


def test_three_tiers_equal_the_127_row_instantiation_alone_bit_for_bit(built):
    """fast (31 rows) -> mid (63 rows, walks the first hand-over list, hands on to the second) -> wide (127 rows, walks the second):
    on the rough terrain with one contact per penetrated grid triangle (CM_FLAG_HFPRISM) robots dropped into the ground pass through
    all three in the middle of fused launches.  State, outputs, solver statistics and drive-level state must be those of the 127-row
    instantiation stepping every env alone -- under all three wave schedules, with NaN-poisoned LDS, in one-wave and two-wave form of
    the first two tiers, and with the launch in chunks."""
    from cassie_amd import Model
    from cassie_amd import phys as P
    import emu_py
    model = Model("cassie_hfield")
    model.set_flag(P.FLAG_HFPRISM, True)
    ref, rows, _ = _two_wave_workload(model, True, fast=False, two_waves=True, schedule=0, nlaunch=3, nsub=12, stress=False)
    assert rows[:, :, 1].max() > 63 and rows[:, :, 1].min() <= 31, (rows[:, :, 1].min(), rows[:, :, 1].max())
    for schedule, two_waves, chunks in ((0, True, 1), (1, True, 1), (2, True, 1), (1, False, 1), (2, True, 3)):
        with emu_py.settings(resume_grid=(2, 1, 3)[schedule], chunks=chunks) as run:
            got, _, _ = _two_wave_workload(model, True, fast=True, two_waves=two_waves, schedule=schedule, poison=True, nlaunch=3, nsub=12, stress=False)
        assert run.wide_envs > 0, "no env reached the 127-row pass"
        assert got == ref, (schedule, two_waves, chunks)


def test_guarded_sweeps_across_both_waves_reproduce_the_fast_ones(cassie):
    """The guard (never accept a cost increase) of a sweep that crosses the waves is local to each wave's half: forcing every half
    through its guarded form must give the trajectory of the unguarded sweeps to rounding, on the pose that needs 80 rows."""
    import emu_py
    pod = cassie.pod
    keep = (pod.maxcon, pod.maxefc)
    pod.maxcon, pod.maxefc = 32, 127           # (the caps CM_FLAG_HFPRISM gives a model)
    q0 = cassie.qpos_init().copy()
    q0[2] = 0.0
    try:
        a, b = EmuBatch(pod, 1), EmuBatch(pod, 1)
        for x in (a, b):
            x.qpos[:] = q0
        a.step(10)
        with emu_py.settings(force_guarded_pgs=1):
            b.step(10)
    finally:
        pod.maxcon, pod.maxefc = keep
    assert a.info[0, 1] > 64 and a.info[0, 3] == 0 and b.info[0, 3] > 0
    assert tuple(a.info[0, :3]) == tuple(b.info[0, :3])
    assert np.abs(a.qpos - b.qpos).max() < 1e-11 and np.abs(a.qvel - b.qvel).max() < 1e-9


# ---- round 6: the fast kernel that finishes the substeps it cannot hold in place (cassie_step_kernel's INROWS) ----
@pytest.mark.parametrize("drive", [False, True])
def test_in_place_form_equals_the_pass_behind_the_kernel_bit_for_bit(cassie, drive):
    """A substep that needs more than 31 rows is run by the 63-row code INSIDE the fast kernel's workgroup, and the env returns to the
    fast code for the next one -- instead of taking all its remaining substeps to the list-walking pass.  Every substep is computed by
    the same instructions either way, so everything a launch leaves must be identical: under the stress targets (hand-overs in the
    middle of fused launches), all three wave schedules, NaN-poisoned LDS, and with the launch in chunks."""
    import emu_py
    ref, rows, bails0 = _two_wave_workload(cassie, drive, fast=True, two_waves=True, schedule=0)
    assert rows[:, :, 1].max() > 31, "the workload never left the 31-row tier"
    # (stay: PhysIO::inplace_stay_rows -- 0 = back to the fast code after every substep, r = the env stays in the 63-row code until a
    # substep needs at most r rows again: 27 is what the product launches with, 31 the narrowest margin, 12 practically never back)
    for schedule, chunks, stay in ((0, 1, 0), (1, 1, 27), (2, 1, 31), (1, 3, 27), (0, 2, 12)):
        with emu_py.settings(inplace=1, chunks=chunks, inplace_stay_rows=stay):
            got, _, _ = _two_wave_workload(cassie, drive, fast=True, two_waves=True, schedule=schedule, poison=True)
        assert got == ref, (schedule, chunks, stay)
    # ... and the one-wave form of the full kernel alone agrees too (the yardstick of every form)
    alone, _, _ = _two_wave_workload(cassie, drive, fast=False, two_waves=False, schedule=0)
    assert alone == ref


def test_in_place_form_hands_on_to_the_127_row_pass(built):
    """With the wide caps (CM_FLAG_HFPRISM) the in-place 63-row call hands a substep of more than 63 rows on to the second list, which
    the 127-row pass walks: same results as the 127-row instantiation alone."""
    from cassie_amd import Model
    from cassie_amd import phys as P
    import emu_py
    model = Model("cassie_hfield")
    model.set_flag(P.FLAG_HFPRISM, True)
    ref, rows, _ = _two_wave_workload(model, True, fast=False, two_waves=True, schedule=0, nlaunch=3, nsub=12, stress=False)
    assert rows[:, :, 1].max() > 63 and rows[:, :, 1].min() <= 31
    for schedule, chunks, stay in ((0, 1, 0), (2, 3, 27), (1, 1, 31)):
        with emu_py.settings(inplace=1, chunks=chunks, resume_grid=(2, 1, 3)[schedule], inplace_stay_rows=stay) as run:
            got, _, _ = _two_wave_workload(model, True, fast=True, two_waves=True, schedule=schedule, poison=True, nlaunch=3, nsub=12, stress=False)
        assert run.wide_envs > 0, "no env reached the 127-row pass"
        assert got == ref, (schedule, chunks, stay)
