"""The run-time-topology instantiations of the step kernel (launch_step<32 / 40, TopoRuntime>) on the CPU wave emulator, over a family
of generated models that stand on the loader's limits (tests/model_family.py): the loader's facts and refusals, the oracle and the
emulator against an independent longdouble reference of kinematics and mass matrix (tests/family_ref.py), teacher-forced single steps
and fused substeps against the oracle where the oracle itself is well conditioned, and negative controls that show the bounds bite.
tests/test_model_family_gpu.py runs the same checks (tests/family_check.py) on the device."""
import numpy as np
import pytest

import emu_py
import family_check as C
import family_ref
import model_family as F
from cassie_amd import Model
from cassie_amd._lib import CmModel
from emu_py import EmuBatch
from oracle_py import Oracle

MEMBERS = list(F.MEMBERS)


@pytest.fixture(scope="module")
def family(built, tmp_path_factory):
    d = tmp_path_factory.mktemp("family")
    return lambda member: C.model(member, d)


def test_the_text_is_a_pure_function_of_member_and_seed(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    for member in ("bushy32", "sensed"):
        one, two = open(F.generate(member, a)).read(), open(F.generate(member, b)).read()
        assert one == two and one != open(F.generate(member, b, seed=1)).read()


@pytest.mark.parametrize("member", MEMBERS)
def test_loader_facts(family, member):
    """What the table of tests/model_family.py says of a member is what the loader compiles: sizes, depth, kin_simple, and the family and
    padded size ck::pick_family answers -- the run-time topology, without being forced to it."""
    pod, facts = family(member).pod, F.MEMBERS[member][1]
    for k in ("nv", "nq", "nbody", "maxdepth", "kin_simple", "ngeom", "nroot", "neq", "nu", "nsensor", "nsensordata"):
        if k in facts:
            assert getattr(pod, k) == facts[k], (member, k, getattr(pod, k))
    pad = 40 if facts["nv"] > 32 else 32
    assert emu_py.pick_family(pod) == {32: F.GENERIC32, 40: F.GENERIC40}[pad] == emu_py.pick_family(pod, generic_only=True)
    assert max(pod.body_depth[b] for b in range(pod.nbody)) == facts["maxdepth"]
    if "dofdepth" in facts:
        assert max(bin(pod.dof_ancmask[d]).count("1") for d in range(pod.nv)) == facts["dofdepth"]
    if "root_children" in facts:
        assert pod.body_nchild[pod.root_body[0]] == facts["root_children"] == 4
        assert all(3 <= pod.body_nchild[pod.body_child[pod.root_body[0]][c]] <= 4 for c in range(4))
    assert pod.npair <= 192 and pod.maxcon == 16 and pod.maxefc == 63
    if member == "bodies32":
        assert sum(1 for b in range(1, pod.nbody) if pod.body_jntnum[b] == 0) == 15
    if member == "multi_joint":
        kinds = {tuple(pod.jnt_type[pod.body_jntadr[b] + k] for k in range(pod.body_jntnum[b])) for b in range(1, pod.nbody)}
        assert {(3, 3), (2, 3), (3, 2, 3), (3, 3, 3)} <= kinds
    if member == "pelvis_like":
        assert tuple(pod.jnt_type[k] for k in range(4)) == (2, 2, 2, 1) and pod.body_jntnum[1] == 4
    if member == "actuated":
        assert len({pod.act_gear[u] for u in range(pod.nu)}) == 12
    if member == "sensed":
        assert {pod.sensor_type[s] for s in range(pod.nsensor)} == set(range(6))
        assert len({pod.site_bodyid[pod.sensor_objid[s]] for s in range(pod.nsensor) if pod.sensor_type[s] >= 2}) >= 6


@pytest.mark.parametrize("name", list(F.REFUSALS))
def test_loader_refuses(built, tmp_path, name):
    """One step past each limit, and the two placements of a free joint on which oracle and kernel disagreed (a free joint on a body
    whose parent is not the world: 5 contacts / 20 rows against 1 / 4 at the first step; a free joint beside a hinge: 0 contacts
    against 4): the loader refuses, and says why."""
    with pytest.raises(RuntimeError, match=F.REFUSALS[name][1]):
        Model(F.generate_refusal(name, tmp_path))


@pytest.mark.parametrize("member", MEMBERS)
def test_kinematics_and_mass_matrix_against_longdouble(family, member):
    """Oracle first, then the emulator, against plain longdouble kinematics and M = sum of J^T (m, I) J from explicit body Jacobians,
    16 states per member.  The emulator's bound is 100 x the oracle's measured worst relative error, at least 64 u (of max(1, the
    largest coordinate) for xpos, of the largest entry for M).

    The oracle against the reference, worst over the family (per member: printed): xpos 3.1e-16, xquat 6.6e-16, site frames 8.8e-16,
    M 1.7e-15.  The emulator, worst error over its bound: xpos 0.035 and xquat 0.044 (ball_chain), M 0.070 (chain26)."""
    pod = family(member).pod
    q, kins, Ms, base = C.kin_reference(member, pod)
    assert all(x < 1e-13 for x in base.values()), (member, base)       # the oracle itself holds to the reference
    emu = EmuBatch(pod, C.N_KIN)
    emu.qpos[:] = q
    emu.forward()
    _, qM = emu.derive([-1] * 6)
    assert np.array_equal(emu.qpos, q) and not emu.qvel.any()           # forward passes: the state is untouched
    C.check_kin(member, pod, emu.xpos, emu.xquat, qM)


@pytest.mark.parametrize("member", MEMBERS)
def test_teacher_forced_single_steps(family, member):
    """The emulator against the oracle from identical (qpos, qvel, ctrl), 64 states per member, in the protocol, metrics and bounds of
    test_derive_gpu.py: equal ncon / nefc / solver_iter, equal cap and divergence bits, q 1e-12, v 5e-12, a 1e-9, s 1e-9 -- on the
    states where the oracle's own one-ulp twin stays within 1/100 of each bound (at most 5 % may fail that).  Rows run from the
    fewest a member can have (0; 24 with the eight connects of `loops`) to more than 31, except where a member cannot have that many
    (one_hinge: 1, one_slide: 5, free_box: 16).  The emulator, worst error over its bound across the family: q 3.3e-4, v 0.010
    (dofchain32), a 7.6e-5 (chain27), s 4.7e-5 (sensed); no state of any member is left out."""
    pod = family(member).pod
    q, v, ctrl, refs, usable = C.single_steps(member, pod)
    emu = EmuBatch(pod, C.N_SINGLE)
    emu.qpos[:], emu.qvel[:], emu.ctrl[:] = q, v, ctrl
    emu.step(1)
    C.check_single_steps(member, pod, emu.qpos, emu.qvel, emu.qacc, emu.sensordata, emu.warn, emu.info)
    seen = set().union(*[r["pairs"] for r in refs])
    if member == "four_free":      # plane 0, sphere 2, capsule 3, box 6: the pair types between moving bodies, and all three plane pairs ...
        assert {(2, 3), (3, 3), (2, 6), (3, 6), (0, 2), (0, 3), (0, 6)} <= seen, seen
    if member == "nv38_other":     # ... and box against box, which takes two boxes: the roots of this member's two trees
        assert (6, 6) in seen, seen


@pytest.mark.parametrize("member", MEMBERS)
def test_fused_substeps(family, member):
    """8 envs, step(40) as one emulated launch: the counts of the last substep and the cap bits are the oracle's, the final qpos lies within
    100 x the spread of eight oracle runs started one ulp apart (at least 1e-13) -- for the envs whose eight runs agree on every
    count of every substep (all but 10 % must; none is left out).  Worst error over its bound: 0.029 (actuated); the oracle's spread
    reaches 4e-15 (loops)."""
    pod = family(member).pod
    q, v, ctrl = C.fused_reference(member, pod)[:3]
    emu = EmuBatch(pod, C.N_FUSED)
    emu.qpos[:], emu.qvel[:], emu.ctrl[:] = q, v, ctrl
    emu.step(C.NSUB)
    C.check_fused(member, pod, emu.qpos, emu.warn, emu.info)


# ---------------------------------------------------------------------------------------- negative controls: reference against reference
def _changed_oracle_leaves_the_bounds(member, pod, changed):
    q, v, ctrl, refs, usable = C.single_steps(member, pod)
    worst = dict(q=0.0, v=0.0, a=0.0, s=0.0)
    for e in range(C.N_SINGLE):
        if not usable[e] or refs[e]["diverged"]:
            continue
        t = C._oracle_step(changed, q[e], v[e], ctrl[e])
        err = C.step_errors(pod, refs[e], t["q"], t["v"], t["a"], t["s"])
        for k in worst:
            worst[k] = max(worst[k], err[k] / C.BOUNDS[k])
    return worst


def test_negative_controls_leave_the_bounds_by_more_than_100x(family):
    """The oracle on a pod copy with ONE thing changed, against the oracle on the pod: each change leaves the single-step bounds by more
    than 100 x, so the parity tests above would see a kernel that had it wrong.  (Measured, bushy32: armature x (1 + 1e-6): v 6.8e3, a 2.3e2 x
    the bound; a body hung on its grandparent: v 6.0e10; a joint's axis negated: v 1.7e11; the dropped anchor: xpos 4.9e11.)  And the longdouble kinematics without one joint's
    anchor offset leaves the xpos bound by more than 100 x."""
    member = "bushy32"
    pod = family(member).pod
    # one dof's armature scaled by 1 + 1e-6
    arm = CmModel.from_buffer_copy(pod)
    o = Oracle(pod)
    o.forward()
    d = max(range(pod.nv), key=lambda k: pod.dof_armature[k] / o.qM[k, k])       # the dof whose inertia is armature most of all
    arm.dof_armature[d] = pod.dof_armature[d] * (1 + 1e-6)
    # one body's parent moved to its grandparent
    par = CmModel.from_buffer_copy(pod)
    b = next(b for b in range(1, pod.nbody) if pod.body_depth[b] == 3)
    par.body_parentid[b] = pod.body_parentid[pod.body_parentid[b]]
    # one non-root joint's axis negated
    ax = CmModel.from_buffer_copy(pod)
    j = next(j for j in range(pod.njnt) if pod.jnt_type[j] == 3 and pod.body_depth[pod.jnt_bodyid[j]] == 2)
    for i in range(3):
        ax.jnt_axis[j][i] = -pod.jnt_axis[j][i]
    for what, changed in (("armature", arm), ("parent", par), ("axis", ax)):
        worst = _changed_oracle_leaves_the_bounds(member, pod, changed)
        print("negative control %-8s: worst error / bound %s" % (what, {k: "%.2g" % x for k, x in worst.items()}))
        assert max(worst.values()) > 100.0, (what, worst)
    # the reference's own control: a joint's anchor offset dropped
    q, kins, Ms, base = C.kin_reference(member, pod)
    dropped = family_ref.kinematics(pod, q[0], drop_anchor=j)
    err = float(np.abs(dropped["xpos"] - kins[0]["xpos"]).max() / max(1.0, np.abs(kins[0]["xpos"]).max()))
    print("negative control anchor  : xpos error / bound %.2g" % (err / C.kin_bound(base, "xpos")))
    assert err > 100.0 * C.kin_bound(base, "xpos")
