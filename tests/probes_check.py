"""Checks probe rows (phys_batch_probe: F_PROBES and the contact words) against the definition of include/cassie_phys.h restated in numpy
from the ORACLE's forward state, in the way of tests/derive_check.py: points from xpos / xquat or the site frames, VEL from cvel and
subtree_com, ACC from the oracle's cdof, cdof_dot, qvel and qacc, Jacobians by the oracle's co_jac at the probe's point, CFRC and the
contact word from the oracle's contact list and efc_force -- and checks that need no restatement.  Shared by the emulator test
(tests/test_probes.py) and the GPU test (tests/test_probes_gpu.py) -- test infrastructure."""
import ctypes

import numpy as np

from cassie_amd import phys as P
from oracle_py import Oracle, arr, lib as olib

# tests/derive_check.py's own: positions, velocities and Jacobians; products with qvel; contact forces
ATOL, ATOL_QVEL, FORCE_TOL = 1e-12, 1e-11, dict(rtol=1e-8, atol=1e-7)


def quat2mat(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def mat2quat(R):
    """The routine and sign convention of cassie_sim_site_xquat (csrc/cassiemujoco.c), R a 3 x 3 array."""
    m = np.asarray(R).reshape(9)
    tr = m[0] + m[4] + m[8]
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2
        return np.array([0.25 * s, (m[7] - m[5]) / s, (m[2] - m[6]) / s, (m[3] - m[1]) / s])
    if m[0] > m[4] and m[0] > m[8]:
        s = np.sqrt(1.0 + m[0] - m[4] - m[8]) * 2
        return np.array([(m[7] - m[5]) / s, 0.25 * s, (m[1] + m[3]) / s, (m[2] + m[6]) / s])
    if m[4] > m[8]:
        s = np.sqrt(1.0 + m[4] - m[0] - m[8]) * 2
        return np.array([(m[2] - m[6]) / s, (m[1] + m[3]) / s, 0.25 * s, (m[5] + m[7]) / s])
    s = np.sqrt(1.0 + m[8] - m[0] - m[4]) * 2
    return np.array([(m[3] - m[1]) / s, (m[2] + m[6]) / s, (m[5] + m[7]) / s, 0.25 * s])


def oracle_forward(pod, q, v, ctrl=None, warm=None):
    o = Oracle(pod, q)
    o.qvel[:] = v
    if ctrl is not None:
        o.ctrl[:] = ctrl
    if warm is not None:
        o.qacc_warmstart[:] = warm      # (the solve starts where the batch's does: a state that has been stepped)
    o.forward()
    return o


def contact_forces(pod, d):
    """The oracle's contacts as [(geom1, geom2 in the COMPILED list, body1, body2, force in world axes)], as tests/derive_check.py forms them."""
    out = []
    for c in range(d.ncon):
        con = d.contact[c]
        fr = np.array(con.frame).reshape(3, 3)
        a = con.efc_address
        if con.dim == 1:
            fc = np.array([d.efc_force[a], 0, 0])
        else:
            ef = np.array([d.efc_force[a + i] for i in range(4)])
            fc = np.array([ef.sum(), con.friction[0] * (ef[0] - ef[1]), con.friction[0] * (ef[2] - ef[3])])
        out.append((con.geom1, con.geom2, pod.geom_bodyid[con.geom1], pod.geom_bodyid[con.geom2], fr.T @ fc))
    return out


def contact_word(pod, d, classes):
    """The contact word of the oracle's contact list; classes = (geom_user [ngeom * nuser_geom] or None, nuser_geom, geom_group) of the
    host model's full geom list, the rules those of csrc/cassiemujoco.c's three collision checks."""
    user, nug, group = classes
    word = 0
    for c in range(d.ncon):
        g1, g2 = pod.geom_fullid[d.contact[c].geom1], pod.geom_fullid[d.contact[c].geom2]
        if user is not None and nug >= 1:
            u1, u2 = user[nug * g1], user[nug * g2]
            if u1 == 1 or u2 == 1:
                word |= P.PC_OBSTACLE
            if u1 == 2 and u2 == 2:
                word |= P.PC_SELF
        for g in range(6):
            if (group[g1] == 1 and group[g2] == g) or (group[g2] == 1 and group[g1] == g):
                word |= P.PC_GROUP0 << g
    return word


def expected(pod, o, probes):
    """The definition for one env from its oracle o (after forward()): {name: [nprobes][*shape]} of every quantity."""
    d = o.d
    nv, nb = pod.nv, pod.nbody
    xpos, xquat = arr(d.xpos)[:nb], arr(d.xquat)[:nb]
    cvel, com = arr(d.cvel)[:nb], arr(d.subtree_com)
    cdof, cdof_dot = arr(d.cdof)[:nv], arr(d.cdof_dot)[:nv]
    site_xpos, site_xmat = arr(d.site_xpos), arr(d.site_xmat)
    qvel, qacc = np.array(o.qvel), np.array(o.qacc)
    forces = contact_forces(pod, d)
    out = {name: [] for name, _ in P.PQ_ROW}
    for kind, ident, offset in probes:
        offset = np.asarray(offset, dtype=np.float64)
        if kind == P.PROBE_SITE:
            body, x, R = pod.site_bodyid[ident], site_xpos[ident], site_xmat[ident].reshape(3, 3)
            quat = mat2quat(R)
        else:
            body, x, quat = ident, xpos[ident], xquat[ident]
            R = quat2mat(quat)
        p = x + R @ offset
        w = cvel[body, :3]
        root = pod.body_rootid[body]
        out["pos"].append(p)
        out["quat"].append(quat)
        out["vel"].append(np.concatenate([w, cvel[body, 3:] + np.cross(w, p - com[root])]))
        out["cvel"].append(cvel[body].copy())
        acc = np.concatenate([np.zeros(3), -np.array(pod.gravity[:3])])
        for k in range(nv):
            if (pod.body_dofmask[body] >> k) & 1:
                acc = acc + cdof_dot[k] * qvel[k] + cdof[k] * qacc[k]
        out["acc"].append(acc)
        jp, jr = ((ctypes.c_double * 40) * 3)(), ((ctypes.c_double * 40) * 3)()
        olib().co_jac(ctypes.byref(pod), ctypes.byref(d), int(body), (ctypes.c_double * 3)(*p), jp, jr)
        out["jacp"].append(np.array(jp)[:, :nv])
        out["jacr"].append(np.array(jr)[:, :nv])
        F = np.zeros(3)
        for _, _, b1, b2, fw in forces:
            if body in (b1, b2):
                F += (-1.0 if b1 == body else 1.0) * fw
        out["cfrc"].append(F)
    return {k: np.array(v) for k, v in out.items()}


def check_rows(pods, q, v, probes, got, ctrl=None, words=None, classes=None, envs=None, hfields=None, warm=None):
    """got: {name: [n][nprobes][*shape]} for the states q, v [n] (pods: one compiled model, or one per env); words [n]: the contact
    words, checked when classes is given; envs: the rows to check (default all); hfields: per env the grid the oracle stands on; ctrl,
    warm [n]: the torques and the solver's warm start of the states, where they are not zero.
    -> the oracles, for what a test wants to look at besides."""
    import oracle_py
    n = len(q)
    oracles = {}
    for e in (range(n) if envs is None else envs):
        pod = pods[e] if isinstance(pods, (list, tuple)) else pods
        if hfields is not None:
            oracle_py.set_hfield(hfields[e])
        o = oracle_forward(pod, q[e], v[e], None if ctrl is None else ctrl[e], None if warm is None else warm[e])
        oracles[e] = o
        want = expected(pod, o, probes)
        for name, w in want.items():
            if name not in got:
                continue
            g = got[name][e]
            if name == "cfrc":
                assert np.allclose(g, w, **FORCE_TOL), (e, name, g, w)
            elif name == "acc":
                # (the issue names no bound for ACC.  It is a linear image of qacc -- motion axes of unit size, lever arms below
                # 1.5 m -- and qacc comes out of the constraint solve, whose two implementations agree as the contact forces do:
                # the contact forces' tolerance)
                assert np.allclose(g, w, **FORCE_TOL), (e, name, np.abs(g - w).max())
            else:
                assert np.allclose(g, w, atol=ATOL, rtol=0), (e, name, np.abs(g - w).max())
        if classes is not None:
            assert int(words[e]) == contact_word(pod, o.d, classes), (e, int(words[e]), contact_word(pod, o.d, classes))
        check_internal(pod, v[e], probes, {k: a[e] for k, a in got.items()})
    if hfields is not None:
        oracle_py.set_hfield(None)
    return oracles


def check_internal(pod, qvel, probes, row):
    """What needs no restatement, on one env's quantities {name: [nprobes][*shape]}: J qvel is the point's velocity, QUAT is unit and
    rotates offset onto POS - the frame's origin (the origin: the same probe's POS at offset 0, which a test supplies as another probe)."""
    if "jacp" in row and "vel" in row:
        assert np.allclose(row["jacp"] @ qvel, row["vel"][:, 3:], atol=ATOL_QVEL, rtol=0)
    if "jacr" in row and "vel" in row:
        assert np.allclose(row["jacr"] @ qvel, row["vel"][:, :3], atol=ATOL_QVEL, rtol=0)
    if "quat" in row:
        assert np.allclose(np.linalg.norm(row["quat"], axis=1), 1.0, atol=ATOL, rtol=0)
    if "quat" in row and "pos" in row:
        origin = {(kind, ident): j for j, (kind, ident, offset) in enumerate(probes) if not np.any(np.asarray(offset))}
        for j, (kind, ident, offset) in enumerate(probes):
            if np.any(np.asarray(offset)) and (kind, ident) in origin:
                R = quat2mat(row["quat"][j])
                assert np.allclose(R @ np.asarray(offset), row["pos"][j] - row["pos"][origin[(kind, ident)]], atol=ATOL, rtol=0)


def site_as_body_probe(pod, site, offset):
    """The probe on the site's BODY that is the same point: the site's local pose composed with the offset."""
    R = quat2mat(np.array(pod.site_quat[site][:4]))
    return (P.PROBE_BODY, pod.site_bodyid[site], np.array(pod.site_pos[site][:3]) + R @ np.asarray(offset, dtype=np.float64))
