"""Probes (phys_batch_probe, include/cassie_phys.h: the reward-side getters for any body or site, for an env range) on the CPU wave
emulator: the emulator's forward pass with the read-out and cassie_probe_kernel, launched through the launcher's own records, grid and
checks (csrc/small_launch.h), against the definition restated from the oracle's state (tests/probes_check.py), against the older
derived block, and the launch rules one by one.  The GPU counterpart is tests/test_probes_gpu.py."""
import ctypes

import numpy as np
import pytest

import emu_py
import probes_check as pc
import probes_emu_py as pe
import randomise_check as rc
from cassie_amd import Model
from cassie_amd import phys as P
from cassie_amd._lib import CmDriveState
from derive_check import foot_ids
from emu_py import EmuBatch

BODY, SITE = P.PROBE_BODY, P.PROBE_SITE
ROWS = P.PQ_ALL & ~P.PQ_CONTACTS


def cassie_probes(cassie):
    """Eight probes: the pelvis, both feet, a foot with an offset, a heel and a toe site (the toe's with an offset), the imu site, the world."""
    body, site = (lambda s: cassie.name2id(1, s)), (lambda s: cassie.name2id(6, s))
    ids = [body("cassie-pelvis"), body("left-foot"), body("right-foot"), site("left-heel"), site("right-toe"), site("imu")]
    assert min(ids) >= 0
    return [(BODY, ids[0], [0, 0, 0]), (BODY, ids[1], [0, 0, 0]), (BODY, ids[2], [0, 0, 0]), (BODY, ids[1], [0.02, -0.03, 0.05]),
            (SITE, ids[3], [0, 0, 0]), (SITE, ids[4], [0.01, 0.02, -0.03]), (SITE, ids[5], [0, 0, 0]), (BODY, 0, [0, 0, 0])]


def cassie_states(cassie, seed=5):
    """Six envs: in the air, touching, pressed 2 cm into the floor, legs crossed (lifted, the hips rolled inwards), randomised joint
    angles, pelvis attitude and velocities, and -- for the env with its own masses -- pressed 1.5 cm.  -> q, v, ctrl."""
    pod = cassie.pod
    rng = np.random.default_rng(seed)
    n = 6
    q = np.tile(cassie.qpos_init(), (n, 1))
    q[:, 2] -= [0.0, 0.012, 0.02, -0.3, 0.005, 0.015]
    q[3, 7], q[3, 21] = -0.1, 0.1
    q[4, 7:] += 0.05 * rng.standard_normal(pod.nq - 7)
    q[4, 3:7] += 0.1 * rng.standard_normal(4)
    q[4, 3:7] /= np.linalg.norm(q[4, 3:7])
    v = rng.uniform(-0.5, 0.5, (n, pod.nv))
    ctrl = rng.uniform(-2.0, 2.0, (n, pod.nu))
    return q, v, ctrl


def own_masses(name, nenv, env, seed=3):
    """Parameter blocks [nenv] in which `env` alone has randomised masses, inertial offsets and inertias (set_const run on the emulator)
    -> (blocks, the per-env compiled models the oracle is handed, the parameter rows as Batch.randomize takes them)."""
    pod0 = Model(name).pod
    hosts = rc.HostEnvModels(name)
    params = rc.random_params(hosts.m, nenv, seed=seed, damping=0.0, friction=(1.0, 1.0))
    own = rc.params_as_arrays(pod0.params, pod0)
    for f in rc.INPUT_FIELDS:
        for e in range(nenv):
            if e != env or f in ("dof_damping", "geom_friction"):
                params[f][e] = own[f].reshape(-1)
    blocks = rc.new_blocks(pod0, nenv, params)
    emu_py.set_const(pod0, blocks, nenv, 1)
    return blocks, [hosts.pod(params, e) if e == env else pod0 for e in range(nenv)], params


@pytest.fixture(scope="module")
def cassie_case(cassie):
    """The six envs probed once with every quantity, one wave and two: shared by the tests below (and left unchanged)."""
    pod = cassie.pod
    q, v, ctrl = cassie_states(cassie)
    blocks, pods, _ = own_masses("cassie", len(q), 5)
    probes, classes = cassie_probes(cassie), pe.geom_classes(cassie)
    runs = {}
    for two_waves in (0, 1):
        emu = EmuBatch(pod, len(q))
        emu.qpos[:], emu.qvel[:], emu.ctrl[:] = q, v, ctrl
        emu.envparams = blocks
        with emu_py.settings(two_waves=two_waves):
            got, words, _ = pe.probe(emu, probes, P.PQ_ALL, classes=classes)
        assert np.array_equal(emu.qpos, q) and np.array_equal(emu.qvel, v)
        runs[two_waves] = (emu, got, words)
    return dict(q=q, v=v, ctrl=ctrl, pods=pods, probes=probes, classes=classes, runs=runs)


@pytest.mark.parametrize("two_waves", [0, 1])
def test_definition_on_cassie(cassie, cassie_case, two_waves):
    """Every quantity of eight probes on six envs against the numpy restatement from the oracle's forward state, the contact words included."""
    c = cassie_case
    _, got, words = c["runs"][two_waves]
    assert set(got) == set(pe.NAMES)
    orcs = pc.check_rows(c["pods"], c["q"], c["v"], c["probes"], got, ctrl=c["ctrl"], words=words, classes=c["classes"])
    # the states are what their names say: no contact in the air and with the legs crossed in the air, loaded feet when pressed
    assert orcs[0].d.ncon == 0 and orcs[2].d.ncon >= 2
    assert np.all(got["cfrc"][0] == 0) and got["cfrc"][2, 1, 2] > 50 and got["cfrc"][2, 2, 2] > 50
    assert np.array_equal(got["cfrc"][:, 1], got["cfrc"][:, 3])            # the same body: the same force, whatever the offset
    assert np.all(got["jacp"][:, 7] == 0) and np.all(got["vel"][:, 7] == 0)    # the world does not move
    assert np.allclose(got["acc"][:, 7, 3:], -np.array(cassie.pod.gravity[:3]), atol=0, rtol=0)
    assert not np.allclose(got["cfrc"][5], got["cfrc"][2], rtol=1e-3)      # the env with its own masses stands on its own forces


@pytest.mark.parametrize("two_waves", [0, 1])
def test_feet_probes_against_the_derived_block(cassie, cassie_case, two_waves):
    """POS (with the reference's mid-foot offset), CVEL, JACP / JACR and the contact force of the two foot bodies are the derived block's."""
    c = cassie_case
    emu, got, _ = c["runs"][two_waves]
    pod, ids = cassie.pod, foot_ids(cassie)
    with emu_py.settings(two_waves=two_waves):
        D, _ = emu.derive(ids)
    off = np.sqrt(0.01762 ** 2 + 0.05219 ** 2)
    for side, j in ((0, 1), (1, 2)):
        assert c["probes"][j][:2] == (BODY, ids[side])
        assert np.allclose(got["pos"][:, j] - [0, 0, off], D[:, P.DRV_FOOT_POS + 3 * side: P.DRV_FOOT_POS + 3 * side + 3], atol=pc.ATOL, rtol=0)
        assert np.allclose(got["cvel"][:, j], D[:, P.DRV_FOOT_VEL + 6 * side: P.DRV_FOOT_VEL + 6 * side + 6], atol=pc.ATOL, rtol=0)
        for name, at in (("jacp", P.DRV_FOOT_JACP), ("jacr", P.DRV_FOOT_JACR)):
            J = D[:, at + side * 3 * P.MAXV: at + (side + 1) * 3 * P.MAXV].reshape(-1, 3, P.MAXV)
            assert np.allclose(got[name][:, j], J[:, :, : pod.nv], atol=pc.ATOL, rtol=0) and np.all(J[:, :, pod.nv:] == 0)
        assert np.allclose(got["cfrc"][:, j], D[:, P.DRV_FOOT_FORCE + 6 * side: P.DRV_FOOT_FORCE + 6 * side + 3], **pc.FORCE_TOL)
    assert np.abs(D[:, P.DRV_FOOT_FORCE: P.DRV_FOOT_FORCE + 3]).max() > 50


def test_site_probe_equals_the_body_probe_of_the_same_point(cassie, cassie_case):
    """A probe on a site with offset d is the probe on the site's body with the site's local pose composed with d -- but for QUAT, which
    is the site's own frame."""
    c = cassie_case
    pod, d = cassie.pod, [0.01, 0.02, -0.03]
    toe = cassie.name2id(6, "right-toe")
    probes = [(SITE, toe, d), pc.site_as_body_probe(pod, toe, d), (SITE, toe, [0, 0, 0])]
    emu = EmuBatch(pod, 3)
    emu.qpos[:], emu.qvel[:], emu.ctrl[:] = c["q"][[1, 3, 4]], c["v"][[1, 3, 4]], c["ctrl"][[1, 3, 4]]
    got, _, _ = pe.probe(emu, probes, ROWS)
    for name in ("pos", "vel", "jacp"):
        assert np.allclose(got[name][:, 0], got[name][:, 1], atol=pc.ATOL, rtol=0), name
    for name in ("cvel", "acc", "jacr", "cfrc"):
        assert np.array_equal(got[name][:, 0], got[name][:, 1]), name
    assert np.array_equal(got["quat"][:, 0], got["quat"][:, 2]) and np.abs(got["pos"][:, 0] - got["pos"][:, 2]).max() > 0.01
    for e in range(3):
        pc.check_internal(pod, emu.qvel[e], probes, {k: a[e] for k, a in got.items()})


@pytest.mark.parametrize("two_waves", [0, 1])
def test_second_tree_root_on_the_tray_model(two_waves):
    """cassie_tray_box: the cube (a free joint, its own body_rootid) sits on the tray the pelvis carries.  VEL and the Jacobians of a
    probe on the cube use the cube's own subtree_com; CFRC is the cube's weight and more, opposite on the two bodies."""
    m = Model("cassie_tray_box")
    pod = m.pod
    tray, cube = m.name2id(1, "tray"), pod.nbody - 1
    assert tray >= 0 and pod.body_rootid[cube] == cube and pod.body_rootid[tray] != cube and pod.body_dofnum[cube] == 6
    rng = np.random.default_rng(9)
    q = np.tile(np.array(pod.qpos0[: pod.nq]), (2, 1))
    o = pc.oracle_forward(pod, q[0], np.zeros(pod.nv))
    top = np.array(o.d.geom_xpos[[g for g in range(pod.ngeom) if pod.geom_bodyid[g] == tray][0]])
    qa = pod.jnt_qposadr[pod.body_jntadr[cube]]
    q[:, qa: qa + 3] = top + [[0, 0, 0.054], [0.01, -0.02, 0.053]]          # half heights 0.005 + 0.05: pressed 1 and 2 mm into the tray
    v = rng.uniform(-0.3, 0.3, (2, pod.nv))
    probes = [(BODY, cube, [0, 0, 0]), (BODY, cube, [0.05, 0.05, -0.05]), (BODY, tray, [0, 0, 0]), (BODY, tray, [0.1, 0, 0.005])]
    classes = pe.geom_classes(m)
    emu = EmuBatch(pod, 2)
    emu.qpos[:], emu.qvel[:] = q, v
    with emu_py.settings(two_waves=two_waves):
        got, words, _ = pe.probe(emu, probes, P.PQ_ALL, classes=classes)
    orcs = pc.check_rows(pod, q, v, probes, got, words=words, classes=classes)
    for e in range(2):
        on_tray = [f for _, _, b1, b2, f in pc.contact_forces(pod, orcs[e].d) if {b1, b2} == {tray, cube}]
        assert len(on_tray) >= 3 and abs(sum(on_tray)[2]) > 50
        assert abs(got["cfrc"][e, 0, 2]) > 50 and np.allclose(got["cfrc"][e, 0], -got["cfrc"][e, 2], **pc.FORCE_TOL)
        assert words[e] & P.PC_OBSTACLE                                     # the cube is the model's one obstacle-class geom
        # the cube's columns are its own six dofs, about its own centre of mass
        dofs = [k for k in range(pod.nv) if (pod.body_dofmask[cube] >> k) & 1]
        assert len(dofs) == 6 and np.all(np.delete(got["jacp"][e, 1], dofs, axis=1) == 0) and np.abs(got["jacp"][e, 1][:, dofs]).max() > 0.5


def test_contact_word_flags_on_cassie_are_set_and_clear(cassie, cassie_case):
    """Each flag the shipped cassie.xml can raise -- a robot geom on the floor (group 1 on group 0), two robot geoms on each other (the
    self-collision class, group 1 on group 1) -- is, by the ORACLE's contact lists, set in one of the six envs and clear in another; the
    emulated words are those (test_definition_on_cassie compares every env's)."""
    c = cassie_case
    _, _, words = c["runs"][0]
    want = [pc.contact_word(c["pods"][e], pc.oracle_forward(c["pods"][e], c["q"][e], c["v"][e], c["ctrl"][e]).d, c["classes"]) for e in range(6)]
    for flag in (P.PC_SELF, P.PC_GROUP0 << 0, P.PC_GROUP0 << 1):
        assert any(w & flag for w in want) and any(not (w & flag) for w in want), hex(flag)
    assert [int(w) for w in words] == want
    assert want[3] == P.PC_SELF | P.PC_GROUP0 << 1 and want[0] == 0 and want[2] == P.PC_GROUP0


def test_contact_word_bit_by_bit_on_hand_made_contact_lists(cassie):
    """cassie_probe_kernel alone (emu_probe_reduce) on read-out blocks whose contact lists are made by hand, over a hand-made class table:
    every bit of the word on its own -- the obstacle class and the geom groups the shipped models offer no state for included -- then
    combinations, ids outside the table, and an empty list."""
    pod = cassie.pod
    # the full list: geom g has group g for g = 0 .. 5, then an obstacle (user 1), two robot geoms (user 2; group 1), a geom of group 7
    user = np.array([0, 0, 0, 0, 0, 0, 1, 2, 2, 0], dtype=np.float64)
    group = np.array([0, 1, 2, 3, 4, 5, 0, 1, 1, 7], dtype=np.int32)
    OB, SELF, G = P.PC_OBSTACLE, P.PC_SELF, (lambda g: P.PC_GROUP0 << g)
    cases = [([(6, 9)], OB), ([(9, 6)], OB), ([(7, 8)], SELF | G(1)), ([(1, 0)], G(0)), ([(0, 1)], G(0)), ([(1, 1)], G(1)), ([(2, 1)], G(2)),
             ([(1, 3)], G(3)), ([(4, 1)], G(4)), ([(1, 5)], G(5)), ([(1, 9)], 0), ([(9, 9)], 0), ([(2, 3)], 0), ([(7, 9)], 0),
             ([(6, 0)], OB), ([(6, 1)], OB | G(0)), ([(7, 6)], OB | G(0)), ([(1, 0), (7, 8), (6, 9), (5, 1)], G(0) | SELF | G(1) | OB | G(5)),
             ([(1, 10)], 0), ([(-1, 1)], 0), ([], 0)]
    n = len(cases)
    ext = (pe.CmExt * n)()
    for e, (pairs, _) in enumerate(cases):
        ext[e].ncon = len(pairs)
        for c_, (g1, g2) in enumerate(pairs):
            ext[e].con_geom1[c_], ext[e].con_geom2[c_] = g1, g2
    xquat = np.tile([1.0, 0, 0, 0], (n, pod.nbody))
    z = lambda k: np.zeros((n, k))
    got, words = pe.reduce(pod, [(BODY, 1, [0, 0, 0])], P.PQ_POS | P.PQ_CONTACTS, ext, z(3 * pod.nbody), xquat, z(pod.nq), z(pod.nv), z(pod.nv),
                           classes=(user, 1, group))
    assert [int(w) for w in words] == [w for _, w in cases]
    assert np.all(got["pos"] == 0)
    # the table itself: the class in the low byte, the group above it
    assert [int(t) for t in pe.classify(user, 1, group)] == [int(u) | (int(g) << 8) for u, g in zip(user, group)]
    assert [int(t) & 0xff for t in pe.classify(None, 0, group)] == [0] * 10       # no geom_user: no classes, as the reference answers
    # without classes no word is written, asked for or not
    _, untouched = pe.reduce(pod, [(BODY, 1, [0, 0, 0])], P.PQ_POS | P.PQ_CONTACTS, ext, z(3 * pod.nbody), xquat, z(pod.nq), z(pod.nv), z(pod.nv))
    assert np.all(untouched == -1)


@pytest.mark.parametrize("two_waves", [0, 1])
def test_a_range_leaves_the_other_rows_alone(cassie, two_waves):
    """PROBE_GRID + 3 envs, the rows and the words pre-filled: probe(env0 = 2, n = PROBE_GRID) writes exactly those rows -- with the
    launcher's grid and with five workgroups, the walk with a remainder.  The env in the middle has a NaN in qpos: its row is NaN, its
    word 0, its neighbours are right."""
    pod = cassie.pod
    pe.lib()
    G = pe.PROBE_GRID
    nenv, env0, mid = G + 3, 2, 2 + G // 2
    rng = np.random.default_rng(1)
    q = np.tile(cassie.qpos_init(), (nenv, 1))
    q[:, 2] -= 0.0003 * np.arange(nenv)
    v = rng.uniform(-0.2, 0.2, (nenv, pod.nv))
    q[mid, 9] = np.nan
    probes, classes = cassie_probes(cassie)[:4], pe.geom_classes(cassie)
    Q = P.PQ_POS | P.PQ_VEL | P.PQ_JACP | P.PQ_CFRC | P.PQ_CONTACTS
    row = pe.layout(len(probes), Q, pod.nv)[0]
    results = []
    for grid in (0, 5):
        emu = EmuBatch(pod, nenv)
        emu.qpos[:], emu.qvel[:] = q, v
        out, words = np.full((nenv, row + 2), -7.0), np.full(nenv, -5, dtype=np.int32)
        with emu_py.settings(two_waves=two_waves):
            got, _, _ = pe.probe(emu, probes, Q, classes=classes, env0=env0, n=G, grid=grid, out=out, contacts=words)
        outside = [0, 1, nenv - 1]
        assert np.all(out[outside] == -7.0) and np.all(words[outside] == -5) and np.all(out[:, row:] == -7.0)
        assert np.all(np.isnan(out[mid, :row])) and words[mid] == 0
        inside = [e for e in range(env0, env0 + G) if e != mid]
        assert np.all(np.isfinite(out[inside, :row])) and np.all(words[inside] >= 0)
        pc.check_rows(pod, q, v, probes, got, words=words, classes=classes, envs=[env0, mid - 1, mid + 1, env0 + G - 1])
        assert emu.warn[mid] == P.WARN_DIVERGED and not emu.warn[inside].any()      # (what a forward pass of a NaN state raises anyway)
        results.append((out.tobytes(), words.tobytes()))
    assert results[0] == results[1]
    assert pe.grid(G) == G and pe.grid(G + 3) == G


def test_record_grid_and_layout_of_a_launch(cassie):
    """make_probe_io, probe_grid and probe_layout against hand-computed values for two quantity masks."""
    pod = cassie.pod
    pe.lib()
    assert (pod.nv, pod.nbody) == (32, 26) and pe.PROBE_GRID == 64
    assert [pe.grid(n) for n in (1, 63, 64, 65, 2048, 4096)] == [1, 63, 64, 64, 64, 64]
    A = P.PQ_POS | P.PQ_VEL | P.PQ_CFRC
    assert pe.layout(8, A, 32) == (96, [0, -1, 24, -1, -1, -1, -1, 72], [3, 4, 6, 6, 6, 96, 96, 3])
    assert pe.layout(3, P.PQ_ALL, 32) == (660, [0, 9, 21, 39, 57, 75, 363, 651], [3, 4, 6, 6, 6, 96, 96, 3])
    assert pe.layout(3, P.PQ_ALL, 32) == pe.layout(3, ROWS, 32)                   # the contact word is not in the row
    assert pe.layout(5, P.PQ_CONTACTS, 32)[0] == 0 and pe.layout(2, P.PQ_JACR | P.PQ_QUAT, 38) == (236, [-1, 0, -1, -1, -1, -1, 8, -1], [3, 4, 6, 6, 6, 114, 114, 3])
    rec, off = pe.record(pod, 8, A | P.PQ_CONTACTS, sout=120, sq=100, sqv=100, env0=2048, n=2048, ngeom=50)
    assert rec == dict(env0=2048, n=2048, nprobes=8, quantities=A | P.PQ_CONTACTS, sout=120, sxp=78, sxq=104, sq=100, sqv=100, sv=32, row_dim=96,
                       classes=1, ngeom=50, contacts=1)
    assert off == [0, -1, 24, -1, -1, -1, -1, 72]
    # the contact word is written only where it was asked for AND the classes are there
    for Q, classes, want in ((A, True, 0), (A | P.PQ_CONTACTS, False, 0), (P.PQ_ALL, True, 1)):
        rec, _ = pe.record(pod, 3, Q, sout=700, sq=pod.nq, sqv=pod.nv, env0=0, n=7, classes=classes, ngeom=50)
        assert (rec["contacts"], rec["classes"]) == (want, want) and rec["ngeom"] == (50 if want else 0)
        assert rec["row_dim"] == (660 if Q & P.PQ_JACP else 96 * 3 // 8)


def test_every_refusal_of_the_configuration(cassie):
    pod = cassie.pod
    ok = [(BODY, 1, [0, 0, 0]), (SITE, 0, [0.1, 0, 0])]
    SIZE = "0 .. 32 probes (0 releases them)"
    assert pe.check(pod, ok, P.PQ_ALL) is None and pe.check(pod, [], 0) is None            # (0 probes: the release, whatever the mask)
    assert pe.check(pod, [ok[0]] * 32, P.PQ_POS) is None and pe.check(pod, [(BODY, 0, [0, 0, 0])], P.PQ_CONTACTS) is None
    assert pe.check(pod, ok, P.PQ_ALL, nprobes=-1) == SIZE and pe.check(pod, [ok[0]] * 33, P.PQ_ALL) == SIZE
    assert pe.check(pod, [ok[0], (2, 1, [0, 0, 0])], P.PQ_ALL) == "a probe's kind is PHYS_PROBE_BODY or PHYS_PROBE_SITE"
    assert pe.check(pod, [(-1, 1, [0, 0, 0])], P.PQ_ALL) == "a probe's kind is PHYS_PROBE_BODY or PHYS_PROBE_SITE"
    for bad in (-1, pod.nbody):
        assert pe.check(pod, [ok[0], (BODY, bad, [0, 0, 0])], P.PQ_ALL) == "a body probe's id must lie in [0, nbody)"
    assert pe.check(pod, [(BODY, pod.nbody - 1, [0, 0, 0])], P.PQ_ALL) is None
    SITE_MSG = "a site probe's id must lie in [0, nsite) and below CM_MAXSITE, the sites of the read-out"
    for bad in (-1, pod.nsite, 16):
        assert pe.check(pod, [(SITE, bad, [0, 0, 0])], P.PQ_ALL) == SITE_MSG
    assert pe.check(pod, [(SITE, pod.nsite - 1, [0, 0, 0])], P.PQ_ALL) is None
    many = type(pod).from_buffer_copy(pod)
    many.nsite = 20                                                                        # (more sites than the read-out holds)
    assert pe.check(many, [(SITE, 15, [0, 0, 0])], P.PQ_ALL) is None and pe.check(many, [(SITE, 16, [0, 0, 0])], P.PQ_ALL) == SITE_MSG
    for bad in (np.nan, np.inf, -np.inf):
        assert pe.check(pod, [(BODY, 1, [0, bad, 0])], P.PQ_ALL) == "a probe needs a finite offset"
    for bad in (0, P.PQ_CONTACTS << 1, P.PQ_POS | 1 << 31):
        assert pe.check(pod, ok, bad) == "quantities is a non-empty OR of PHYS_PQ_*"
    # a call
    assert pe.call_check(True, 8, 0, 8) is None and pe.call_check(True, 8, 8, 0) is None
    assert pe.call_check(False, 8, 0, 8) == "not configured (phys_batch_probes_configure first)"
    for env0, n in ((-1, 2), (0, 9), (7, 2), (0, -1), (2 ** 31 - 1, 2)):
        assert pe.call_check(True, 8, env0, n) == "env range out of bounds"
    # the emulator's entry point answers as the launcher does
    emu = EmuBatch(pod, 2)
    out = np.zeros((2, 8))
    res = emu_py.StepResult()
    bad = pe.table_of([(BODY, 99, [0, 0, 0])])
    assert pe.lib().emu_probe(ctypes.byref(emu._args(1, 0)), 0, 2, 0, bad.ctypes.data, 1, P.PQ_POS, None, 0, None, 0, out.ctypes.data, 8, None, ctypes.byref(res)) == -1
    assert pe.lib().emu_probe_last_refusal().decode() == "a body probe's id must lie in [0, nbody)"
    good = pe.table_of(ok[:1])
    assert pe.lib().emu_probe(ctypes.byref(emu._args(1, 0)), 1, 2, 0, good.ctypes.data, 1, P.PQ_POS, None, 0, None, 0, out.ctypes.data, 8, None, ctypes.byref(res)) == -1
    assert pe.lib().emu_probe_last_refusal().decode() == "env range out of bounds"


def _snapshot(emu):
    keep = ("qpos", "qvel", "qacc", "qacc_warmstart", "sensordata", "actuator_velocity", "ctrl", "time", "xpos", "xquat", "info", "meas", "drive_cmd")
    snap = {k: getattr(emu, k).tobytes() for k in keep}
    snap["drive_state"] = bytes(emu.drive_state)
    return snap


@pytest.mark.parametrize("mode", [P.DRIVE_OFF, P.DRIVE_PD_SAFE])
@pytest.mark.parametrize("two_waves", [0, 1])
def test_a_probe_call_leaves_the_state(cassie, mode, two_waves):
    """qpos, qvel, qacc, sensordata, actuator_velocity, the drive-level state (and ctrl, time, the warm start, the stored body poses, the
    solver statistics, the measurement block) are byte-identical before and after emu_probe, in DRIVE_OFF and in DRIVE_PD_SAFE -- where
    the forward pass applies the torques the last step applied and advances no filter history or delay line."""
    import bench
    pod = cassie.pod
    n = 3
    emu = EmuBatch(pod, n)
    emu.qpos[:] = cassie.qpos_init()
    emu.qpos[:, 2] -= [0.0, 0.01, 0.015]
    emu.forward()
    with emu_py.settings(two_waves=two_waves):
        if mode != P.DRIVE_OFF:
            emu.drive_mode = mode
            emu.pd_kp, emu.pd_kd = np.tile(bench.PD_KP, (n, 1)), np.tile(bench.PD_KD, (n, 1))
            emu.pd_ptarget = np.ascontiguousarray(bench.pd_targets(np.arange(n), 1)[0])
        else:
            emu.ctrl[:] = np.random.default_rng(2).uniform(-3, 3, (n, pod.nu))
        emu.step(30)
        emu.step(30)
        assert not emu.warn.any()
        if mode != P.DRIVE_OFF:
            assert np.abs(emu.ctrl).max() > 1.0 and any(bytes(emu.drive_state[e]) != bytes(CmDriveState()) for e in range(n))
        before = _snapshot(emu)
        probes, classes = cassie_probes(cassie), pe.geom_classes(cassie)
        got, words, _ = pe.probe(emu, probes, P.PQ_ALL, classes=classes)
        assert _snapshot(emu) == before and not emu.warn.any()
        # ... and the values are those of the state as it stands, under the torques last applied
        pc.check_rows(pod, emu.qpos, emu.qvel, probes, got, ctrl=emu.ctrl, words=words, classes=classes, warm=emu.qacc_warmstart)
        assert got["cfrc"][:, 1, 2].max() > 50
        # stepping on from there is what it would have been without the call
        twin = EmuBatch(pod, n)
        for k in ("qpos", "qvel", "qacc", "qacc_warmstart", "sensordata", "actuator_velocity", "ctrl", "time", "meas"):
            getattr(twin, k)[...] = getattr(emu, k)
        ctypes.memmove(twin.drive_state, emu.drive_state, ctypes.sizeof(emu.drive_state))
        twin.drive_mode, twin.pd_kp, twin.pd_kd, twin.pd_ptarget = emu.drive_mode, emu.pd_kp, emu.pd_kd, emu.pd_ptarget
        pe.probe(emu, probes, ROWS)
        emu.step(10)
        twin.step(10)
        assert emu.qpos.tobytes() == twin.qpos.tobytes() and emu.qvel.tobytes() == twin.qvel.tobytes() and bytes(emu.drive_state) == bytes(twin.drive_state)
