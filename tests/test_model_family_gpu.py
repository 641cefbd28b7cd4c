"""The family of generated models of tests/model_family.py through `Batch` on the DEVICE: what tests/test_model_family.py holds the
emulated kernel to -- the longdouble kinematics and mass matrix, the oracle's teacher-forced single steps and fused substeps, under
the same bounds and the same conditioning rule (tests/family_check.py), the references computed from the oracle alone -- and what
only the device can show: one launch of 40 fused substeps gives the bits of 40 launches of one, and the members that stand at the
32-wide and the 40-wide instantiation are already on the run-time topology without being forced to it.  The models are generated
into a temporary directory; nothing outside the tree is read."""
import numpy as np
import pytest

import family_check as C
import model_family as F
from cassie_amd import Batch
from cassie_amd import phys as P

pytestmark = pytest.mark.gpu

MEMBERS = list(F.MEMBERS)


@pytest.fixture(scope="module")
def family(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("family")
    return lambda member: C.model(member, d)


@pytest.mark.parametrize("member", MEMBERS)
def test_teacher_forced_single_steps_on_the_device(family, member):
    """64 states per member, one step on the device and on the oracle from identical (qpos, qvel, ctrl): equal ncon / nefc / solver_iter,
    equal cap and divergence bits, q 1e-12, v 5e-12, a 1e-9, s 1e-9 on the states the conditioning rule keeps.

    Measured on an MI355X, worst error over its bound across the family: q 3.3e-4 (free_box), v 0.010 and a 8.9e-5 (dofchain32),
    s 2.5e-5 (sensed); rows 0 .. 63, no state of any member left out."""
    model = family(member)
    pod = model.pod
    q, v, ctrl, refs, usable = C.single_steps(member, pod)
    b = Batch(model, C.N_SINGLE)
    try:
        b.set(P.F_QPOS, q); b.set(P.F_QVEL, v)
        if pod.nu:
            b.set(P.F_CTRL, ctrl)
        b.step(1)
        qg, vg, ag = b.get(P.F_QPOS), b.get(P.F_QVEL), b.get(P.F_QACC)
        sg = b.get(P.F_SENSORDATA) if pod.nsensordata else np.zeros((C.N_SINGLE, 0))
        w, info = b.warnings()
    finally:
        b.close()
    C.check_single_steps(member, pod, qg, vg, ag, sg, w, info)


@pytest.mark.parametrize("member", MEMBERS)
def test_forward_kinematics_and_mass_matrix_on_the_device(family, member):
    """forward() leaves qpos and qvel untouched; xpos / xquat and the mass matrix of derive() hold against the longdouble reference under
    100 x the oracle's measured worst relative error (at least 64 u), 16 states per member.

    Measured on an MI355X, worst error over its bound: xpos 0.051 and xquat 0.041 (ball_chain), M 0.071 (chain26)."""
    model = family(member)
    pod = model.pod
    q = C.kin_reference(member, pod)[0]
    v = C.states(member, pod, C.N_SINGLE)[1][: C.N_KIN]
    b = Batch(model, C.N_KIN)
    try:
        b.set(P.F_QPOS, q); b.set(P.F_QVEL, v)
        b.forward()
        assert np.array_equal(b.get(P.F_QPOS), q) and np.array_equal(b.get(P.F_QVEL), v)
        xpos, xquat = b.get(P.F_XPOS), b.get(P.F_XQUAT)
        b.derive([-1] * 6)
        qM = b.get(P.F_QM).reshape(C.N_KIN, pod.nv, pod.nv)
        assert np.array_equal(b.get(P.F_QPOS), q) and np.array_equal(b.get(P.F_QVEL), v)
    finally:
        b.close()
    C.check_kin(member, pod, xpos, xquat, qM)


def _run(model, q, v, ctrl, launches, nsub, generic=None):
    pod = model.pod
    b = Batch(model, q.shape[0])
    try:
        if generic is not None:
            b.set_generic_kernel(generic)
        b.set(P.F_QPOS, q); b.set(P.F_QVEL, v)
        if pod.nu:
            b.set(P.F_CTRL, ctrl)
        for _ in range(launches):
            b.step(nsub)
        w, info = b.warnings()
        return b.get(P.F_QPOS), b.get(P.F_QVEL), b.get(P.F_QACC), w, info
    finally:
        b.close()


@pytest.mark.parametrize("member", MEMBERS)
def test_forty_fused_substeps_on_the_device(family, member):
    """8 envs: step(40) as one launch gives the bits of forty step(1) launches, follows the oracle within 100 x the spread of its eight
    one-ulp twins (at least 1e-13) where they agree on every count, and raises only the warning bits the oracle's cap flags predict.

    Measured on an MI355X: bit-equal on every member; worst error over its bound 0.033 (loops, actuated); no env left out."""
    model = family(member)
    pod = model.pod
    q, v, ctrl = C.fused_reference(member, pod)[:3]
    fused = _run(model, q, v, ctrl, 1, C.NSUB)
    single = _run(model, q, v, ctrl, C.NSUB, 1)
    for a, b_, what in zip(fused, single, ("qpos", "qvel", "qacc", "warn", "info")):
        assert np.array_equal(a, b_), (member, what)
    C.check_fused(member, pod, fused[0], fused[3], fused[4])


@pytest.mark.parametrize("member", ["bushy32", "nv38_other"])
def test_the_launcher_already_chose_the_run_time_topology(family, member):
    """nv = 32 on a tree that is not Cassie's, nv = 38 on one that is not the tray's: ck::pick_family must answer the run-time topology,
    so forcing it changes no bit."""
    model = family(member)
    q, v, ctrl = C.fused_reference(member, model.pod)[:3]
    free, forced = _run(model, q, v, ctrl, 1, 5, generic=False), _run(model, q, v, ctrl, 1, 5, generic=True)
    for a, b_ in zip(free, forced):
        assert np.array_equal(a, b_), member
