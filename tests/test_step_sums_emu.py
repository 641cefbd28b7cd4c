"""The step-sums block (csrc/cm_model.h: CM_SUM_*; include/cassie_phys.h: phys_batch_step_sums_enable) on the CPU wave emulator, which
runs the same template as the device.

THE REFERENCE IS THE EXISTING ONE-SUBSTEP PATH, not the new code: a twin state with the sums off and the read-out block on is stepped
nsub times, one substep per launch; after every launch ctrl (clipped to ctrlrange), actuator_velocity, the body contact forces
(PhysIO::body_cfrc, the value PHYS_F_BODY_CFRC holds) and the contact list's bodies are read and summed in numpy in substep order
(sums_emu_py.Reference).  Against it the accumulating launch's COUNT, BODY_CFRC, BODY_TOUCH and the four actuator sums must be equal
BIT FOR BIT, BODY_CFRC_MAX2 to 1e-14 relative (three roundings the device may fuse), and its final qpos / qvel bitwise the twin's.
That N one-substep launches reproduce a fused launch's state bitwise in the drive modes is what the existing fused-launch tests hold
(test_core_safety.py, test_emu_parity.py); every case below asserts it again on its own data."""
import numpy as np
import pytest

import sums_emu_py as S
from cassie_amd import phys as P

# forms of the accumulating launch: (label, fast, settings)
FORMS = (("alone", False, dict()),
         ("alone, two waves", False, dict(two_waves=1)),
         ("two-wave fast", True, dict(two_waves=1)),
         ("two-wave fast, 2 chunks", True, dict(two_waves=1, chunks=2)),
         ("one-wave fast: falls back to the full form alone", True, dict(two_waves=0)))


def _start(model, n, setup):
    """n envs of model, set up by setup(batch), as a SumsBatch."""
    b = S.SumsBatch(model.pod, n)
    b.qpos[:] = model.qpos_init()
    if model.pod.nhfpair > 0:
        import test_hfield
        b.hfield = test_hfield.terrain()
    setup(b)
    return b


def _twin_reference(model, n, setup, nsub, before_launch=None):
    """The twin: sums off, read-out on, one substep per launch -> (Reference, twin)."""
    twin = _start(model, n, setup)
    if before_launch:
        before_launch(twin)
    ref = S.Reference(model.pod, n)
    for _ in range(nsub):
        twin.run(1, accumulate=False, read_out=True)
        ref.add(twin.ctrl, twin.actuator_velocity, twin.body_cfrc, S.ext_contacts(twin.ext, n))
    assert np.isnan(twin.sums).all()            # (a launch that does not accumulate leaves the block alone)
    return ref, twin


def _check(model, n, setup, nsub, forms=FORMS, before_launch=None):
    """Every form's accumulating launch of nsub substeps against the twin; -> (reference views, {label: counters})."""
    import emu_py
    ref, twin = _twin_reference(model, n, setup, nsub, before_launch)
    assert not twin.warn.any()
    runs = {}
    for label, fast, settings in forms:
        with emu_py.settings(**settings) as run:
            b = _start(model, n, setup)
            if before_launch:
                before_launch(b)
            b.run(nsub, accumulate=True, fast=fast)
        assert not b.warn.any(), label
        S.compare(model.pod, b.sums, ref.raw, label)
        assert (b.sums[:, P.SUM_COUNT] == nsub).all(), label
        for f in ("qpos", "qvel", "qacc_warmstart", "time", "ctrl", "actuator_velocity", "sensordata"):
            assert getattr(b, f).tobytes() == getattr(twin, f).tobytes(), (label, f)
        runs[label] = run
    return S.views(model.pod, ref.raw), runs


def _drop(heights, vz):
    """qpos_init lifted / lowered by heights[e], falling at vz: feet that make (and, pushed back up by the contact, break) contact."""
    def setup(b):
        b.qpos[:, 2] += np.asarray(heights)
        b.qvel[:, 2] = vz
    return setup


def _constant_ctrl(model, n):
    hi = np.array([model.pod.act_ctrlrange[u][1] for u in range(model.pod.nu)])
    # (some entries past ctrlrange: F is the CLAMPED torque)
    return hi * np.random.default_rng(3).uniform(-1.3, 1.3, (n, model.pod.nu))


def _safe_mode(b):
    import bench
    n = b.nenv
    b.forward()
    b.drive_mode = P.DRIVE_PD_SAFE
    b.pd_kp, b.pd_kd = np.tile(bench.PD_KP, (n, 1)), np.tile(bench.PD_KD, (n, 1))
    b.pd_ptarget = bench.PD_OFFSET + np.random.default_rng(8).uniform(-0.4, 0.4, (n, 10))


# the drop of test 1: at qpos_init the feet stand 4 mm above the floor's contact margin; envs lowered by these offsets and falling at
# 1 m/s (the speed a 5 cm drop lands with: half a millimetre per substep) meet it in substep 7, 5, 3, 2, 1, 0 of the 8 -- the test itself
# checks that a foot's touch count lies strictly between 0 and the launch's substeps
DROP_HEIGHTS = np.array([-0.0005, -0.0015, -0.0025, -0.003, -0.0035, -0.005])
DROP_VZ = -1.0


@pytest.mark.parametrize("mode", ["off", "pd_safe"])
def test_cassie_dropped_feet_make_and_break_contact(cassie, mode):
    n, nsub = 6, 8
    feet = [cassie.name2id(1, "left-foot"), cassie.name2id(1, "right-foot")]
    if mode == "off":
        ctrl = _constant_ctrl(cassie, n)

        def setup(b):
            _drop(DROP_HEIGHTS, DROP_VZ)(b)
            b.ctrl[:] = ctrl
        ref, _ = _check(cassie, n, setup, nsub)
    else:
        def setup(b):
            _drop(DROP_HEIGHTS, DROP_VZ)(b)
        ref, _ = _check(cassie, n, setup, nsub, before_launch=_safe_mode)
    touch = ref["body_touch"][:, feet]
    print(mode, "foot touches per env:", touch.tolist())
    assert ((touch > 0) & (touch < nsub)).any(), touch          # a foot made or broke contact in the middle of the launch
    assert (ref["act_force2"] > 0).all() and (ref["act_power"] != 0).any()


def _stress(model):
    """The hand-over workload of tests/test_emu_parity.py (_two_wave_workload), unchanged: the benchmark's PD law in contact, targets
    that push joints into their limits."""
    import bench

    def setup(b):
        n = b.nenv
        b.qpos[:, 2] -= 0.15
        b.pd_kp, b.pd_kd = np.tile(bench.PD_KP, (n, 1)), np.tile(bench.PD_KD, (n, 1))
    return setup


def _stress_launches(model, n, nlaunch, nsub, amp, fast, settings):
    """nlaunch launches of the workload, accumulating (fast / settings) against the twin stepping one substep per launch beside it."""
    import bench
    import emu_py
    setup = _stress(model)
    twin, b = _start(model, n, setup), _start(model, n, setup)
    for e in (twin, b):
        e.forward()
        e.drive_mode = P.DRIVE_PD
    total = emu_py.Counters()
    for p in range(nlaunch):
        tg = np.empty((n, 10))
        for e in range(n):
            tg[e] = bench.PD_OFFSET + np.random.default_rng(977 + 31 * p + e).uniform(-amp, amp, 10)
        twin.pd_ptarget, b.pd_ptarget = tg, tg.copy()
        ref = S.Reference(model.pod, n)
        for _ in range(nsub):
            twin.run(1, accumulate=False, read_out=True)
            ref.add(twin.ctrl, twin.actuator_velocity, twin.body_cfrc, S.ext_contacts(twin.ext, n))
        with emu_py.settings(**settings) as run:
            b.run(nsub, accumulate=True, fast=fast)
        total.fast_bails += run.fast_bails
        total.wide_envs += run.wide_envs
        # (the prism terrain fills the contact list: the caps' warning bits are the workload's, the same in both; nobody diverged)
        assert b.warn.tobytes() == twin.warn.tobytes() and not (b.warn & P.WARN_DIVERGED).any()
        S.compare(model.pod, b.sums, ref.raw, (p, settings))
        assert (b.sums[:, P.SUM_COUNT] == nsub).all()
        for f in ("qpos", "qvel", "qacc_warmstart", "ctrl", "meas"):
            assert getattr(b, f).tobytes() == getattr(twin, f).tobytes(), (p, f)
    return total


@pytest.mark.parametrize("settings", [dict(two_waves=1), dict(two_waves=1, chunks=3, resume_grid=1)])
def test_a_substep_handed_to_the_63_row_pass_is_counted_once(cassie, settings):
    total = _stress_launches(cassie, 2, nlaunch=3, nsub=12, amp=10.0, fast=True, settings=settings)
    assert total.fast_bails > 0, "no env left the fast tier"


def test_a_substep_handed_on_to_the_127_row_pass_is_counted_once(built):
    from cassie_amd import Model
    model = Model("cassie_hfield")
    model.set_flag(P.FLAG_HFPRISM, True)
    total = _stress_launches(model, 2, nlaunch=3, nsub=12, amp=0.3, fast=True, settings=dict(two_waves=1))
    assert total.fast_bails > 0 and total.wide_envs > 0, "no env reached the 127-row pass"
    # ... and the 127-row form alone
    _stress_launches(model, 2, nlaunch=1, nsub=6, amp=0.3, fast=False, settings=dict(two_waves=1))


def test_the_sums_mean_what_the_oracle_computes(cassie):
    """CM_DRIVE_OFF, the oracle stepped nsub times: per-body forces by the recipe of tests/derive_check.py (its rtol 1e-8 / atol 1e-7 per
    substep, hence nsub x 1e-7 on a sum); TOUCH and COUNT exact."""
    import emu_py
    from oracle_py import Oracle
    pod, n, nsub = cassie.pod, 3, 8
    ctrl = _constant_ctrl(cassie, n)
    heights = DROP_HEIGHTS[[0, 2, 5]]
    with emu_py.settings(two_waves=1):
        b = _start(cassie, n, _drop(heights, DROP_VZ))
        b.ctrl[:] = ctrl
        q0, v0 = b.qpos.copy(), b.qvel.copy()
        b.run(nsub, accumulate=True, fast=True)
    got = S.views(pod, b.sums)
    lo = np.array([pod.act_ctrlrange[u][0] for u in range(pod.nu)])
    hi = np.array([pod.act_ctrlrange[u][1] for u in range(pod.nu)])
    for e in range(n):
        o = Oracle(pod, q0[e])
        o.qvel[:] = v0[e]
        o.ctrl[:] = ctrl[e]
        F, touch, force, power = np.zeros((pod.nbody, 3)), np.zeros(pod.nbody), np.zeros(pod.nu), np.zeros(pod.nu)
        for _ in range(nsub):
            vel = np.array([pod.act_gear[u] * o.qvel[pod.act_dofid[u]] for u in range(pod.nu)])
            o.step(1)                       # (the oracle's contact list and constraint forces are those of the substep it just took)
            d = o.d
            hit = set()
            for c in range(d.ncon):
                con = d.contact[c]
                b1, b2 = pod.geom_bodyid[con.geom1], pod.geom_bodyid[con.geom2]
                hit |= {b1, b2}
                fr = np.array(con.frame).reshape(3, 3)
                a = con.efc_address
                if con.dim == 1:
                    fc = np.array([d.efc_force[a], 0, 0])
                else:
                    ef = np.array([d.efc_force[a + i] for i in range(4)])
                    fc = np.array([ef.sum(), con.friction[0] * (ef[0] - ef[1]), con.friction[0] * (ef[2] - ef[3])])
                F[b2] += fr.T @ fc
                F[b1] -= fr.T @ fc
            for bb in hit:
                touch[bb] += 1
            force += np.clip(ctrl[e], lo, hi)
            power += np.clip(ctrl[e], lo, hi) * vel
        assert got["count"][e] == nsub
        assert np.array_equal(got["body_touch"][e], touch), (e, got["body_touch"][e], touch)
        assert np.allclose(got["body_cfrc"][e], F, rtol=1e-8, atol=nsub * 1e-7), (e, np.abs(got["body_cfrc"][e] - F).max())
        assert np.allclose(got["act_force"][e], force, rtol=1e-13) and np.allclose(got["act_power"][e], power, rtol=1e-8, atol=1e-9)
    assert got["body_touch"].max() > 0


@pytest.mark.parametrize("name", ["cassie_tray_box", "cassie_hfield"])
def test_the_other_models(name, built):
    from cassie_amd import Model
    model = Model(name)
    n, nsub = 4, 6
    ctrl = _constant_ctrl(model, n)

    def setup(b):
        b.qpos[:, 2] -= np.linspace(0.09, 0.12, n)
        b.qvel[:, 2] = -0.5
        b.ctrl[:] = ctrl
    ref, _ = _check(model, n, setup, nsub, forms=FORMS[:1] + FORMS[2:4])
    assert ref["body_touch"].max() > 0 and np.abs(ref["body_cfrc"]).max() > 0


def test_a_forward_pass_leaves_the_block_alone(cassie):
    b = _start(cassie, 2, _drop([-0.1, -0.1], 0.0))
    b.run(3, accumulate=True)
    before = b.sums.copy()
    assert (before[:, P.SUM_COUNT] == 3).all()
    b.run(1, accumulate=True, integrate=0)
    assert b.sums.tobytes() == before.tobytes()


def test_the_descriptor_keeps_its_offsets_and_appends_the_block(built):
    """PhysIO::sums / sums_stride are the descriptor's last fields: what tests/test_lean_forms_resources.py reads stays where it was."""
    import ctypes
    import emu_py
    L = S.lib()
    mine = np.zeros(3, dtype=np.uint64)
    L.emu_physio_sums_offsets(mine.ctypes.data)
    old = np.zeros(5, dtype=np.uint64)
    emu_py.lib().emu_physio_offsets.argtypes, emu_py.lib().emu_physio_offsets.restype = [ctypes.c_void_p], None
    emu_py.lib().emu_physio_offsets(old.ctypes.data)
    sums, stride, size = (int(v) for v in mine)
    assert size == int(old[4]) and stride == sums + 8 and size - stride <= 8
    assert all(int(v) < sums for v in old[:4])
