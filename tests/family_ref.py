"""A plain numpy forward kinematics and joint-space inertia in `longdouble`, written from the definitions and from nothing the oracle
or the kernel share -- test infrastructure only.

Oracle and kernel were written by one author from one reading of the recursion, so a mistake they share is invisible to their parity.
This reference reads only the pod's body_pos / body_quat / body_ipos / body_iquat / body_mass / body_inertia, jnt_* and qpos, composes
rotation MATRICES (Rodrigues' formula for a hinge; no quaternion products, no pointer jumping, no kinematics records) and builds

    M = sum_b ( m_b Jp_b^T Jp_b  +  Jr_b^T R_b I_b R_b^T Jr_b )  +  diag(armature)

from explicit body Jacobians at the bodies' centres of mass -- not the composite-rigid-body recursion."""
import numpy as np

FREE, BALL, SLIDE, HINGE = range(4)
SPHERE, CAPSULE, BOX = 2, 3, 6


def _quat_mat(q, T):
    q = np.array([q[0], q[1], q[2], q[3]], dtype=T)
    w, x, y, z = q / np.sqrt((q * q).sum())
    one, two = T(1), T(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=T)


def _rodrigues(axis, angle, T):
    a = np.array([axis[0], axis[1], axis[2]], dtype=T)
    a = a / np.sqrt((a * a).sum())
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=T)
    return np.eye(3, dtype=T) + np.sin(T(angle)) * K + (T(1) - np.cos(T(angle))) * (K @ K)


def mat_quat(R):
    """A rotation matrix -> a unit quaternion (w, x, y, z) with w >= 0 (Shepperd's choice of the largest pivot)."""
    T = R.dtype.type
    t = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]]
    k = int(np.argmax(t))
    if k == 0:
        q = [T(1) + t[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]
    elif k == 1:
        q = [R[2, 1] - R[1, 2], T(1) + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]]
    elif k == 2:
        q = [R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], T(1) - R[0, 0] + R[1, 1] - R[2, 2], R[1, 2] + R[2, 1]]
    else:
        q = [R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], T(1) - R[0, 0] - R[1, 1] + R[2, 2]]
    q = np.array(q, dtype=T)
    q = q / np.sqrt((q * q).sum())
    return -q if q[0] < 0 else q


def kinematics(pod, qpos, dtype=np.longdouble, drop_anchor=None):
    """-> dict: xpos [nbody][3], xmat [nbody][3][3], xquat [nbody][4], site_xpos, site_xmat, jnt_axis / jnt_anchor (world, per joint),
    dofs: per dof (translational?, axis, anchor).  drop_anchor: a joint whose anchor offset (jnt_pos) is left out -- the negative
    control of the tests."""
    T = dtype
    nb = pod.nbody
    xpos, xmat = np.zeros((nb, 3), dtype=T), np.zeros((nb, 3, 3), dtype=T)
    xmat[0] = np.eye(3, dtype=T)
    jaxis, janchor = np.zeros((pod.njnt, 3), dtype=T), np.zeros((pod.njnt, 3), dtype=T)
    dofs = [None] * pod.nv
    vec = lambda a: np.array([a[0], a[1], a[2]], dtype=T)
    for b in range(1, nb):
        par = pod.body_parentid[b]
        p = xpos[par] + xmat[par] @ vec(pod.body_pos[b])
        R = xmat[par] @ _quat_mat(pod.body_quat[b], T)
        for j in range(pod.body_jntadr[b], pod.body_jntadr[b] + pod.body_jntnum[b]):
            t, qa, d = pod.jnt_type[j], pod.jnt_qposadr[j], pod.jnt_dofadr[j]
            off = vec(pod.jnt_pos[j]) if j != drop_anchor else np.zeros(3, dtype=T)
            if t == FREE:                                          # the body's frame in the world IS qpos
                p = np.array([qpos[qa + i] for i in range(3)], dtype=T)
                R = _quat_mat([qpos[qa + 3 + i] for i in range(4)], T)
                jaxis[j], janchor[j] = np.array([0, 0, 1], dtype=T), p
                for k in range(3):
                    e = np.zeros(3, dtype=T); e[k] = 1
                    dofs[d + k] = (True, e, None)
                    dofs[d + 3 + k] = (False, R[:, k].copy(), p.copy())
                continue
            anchor, axis = p + R @ off, R @ vec(pod.jnt_axis[j])
            jaxis[j], janchor[j] = axis, anchor
            if t == SLIDE:
                p = p + axis * (T(qpos[qa]) - T(pod.qpos0[qa]))
                dofs[d] = (True, axis, None)
            elif t == HINGE:
                R = R @ _rodrigues(pod.jnt_axis[j], T(qpos[qa]) - T(pod.qpos0[qa]), T)
                p = anchor - R @ off                               # the anchor is a point of the body that the joint leaves where it is
                dofs[d] = (False, axis, anchor)
            else:                                                  # ball: angular velocity in the body's own frame, behind the joint
                R = R @ _quat_mat([qpos[qa + i] for i in range(4)], T)
                p = anchor - R @ off
                for k in range(3):
                    dofs[d + k] = (False, R[:, k].copy(), anchor)
        xpos[b], xmat[b] = p, R
    out = dict(xpos=xpos, xmat=xmat, xquat=np.array([mat_quat(xmat[b]) for b in range(nb)]), jnt_axis=jaxis, jnt_anchor=janchor, dofs=dofs)
    ns = pod.nsite
    out["site_xpos"] = np.array([xpos[pod.site_bodyid[s]] + xmat[pod.site_bodyid[s]] @ vec(pod.site_pos[s]) for s in range(ns)], dtype=T).reshape(ns, 3)
    out["site_xmat"] = np.array([xmat[pod.site_bodyid[s]] @ _quat_mat(pod.site_quat[s], T) for s in range(ns)], dtype=T).reshape(ns, 3, 3)
    return out


def mass_matrix(pod, kin):
    """M(qpos) from explicit body Jacobians, in the dtype of `kin`."""
    T = kin["xpos"].dtype.type
    nv = pod.nv
    M = np.zeros((nv, nv), dtype=T)
    for b in range(1, pod.nbody):
        m = T(pod.body_mass[b])
        if m <= 0:
            continue
        c = kin["xpos"][b] + kin["xmat"][b] @ np.array([pod.body_ipos[b][i] for i in range(3)], dtype=T)
        Ri = kin["xmat"][b] @ _quat_mat(pod.body_iquat[b], T)
        Jp, Jr = np.zeros((3, nv), dtype=T), np.zeros((3, nv), dtype=T)
        a = b
        while a > 0:                                               # the dofs of the bodies from b up to the world move b
            for d in range(pod.body_dofadr[a], pod.body_dofadr[a] + pod.body_dofnum[a]) if pod.body_dofnum[a] else ():
                trans, axis, anchor = kin["dofs"][d]
                if trans:
                    Jp[:, d] = axis
                else:
                    Jr[:, d] = axis
                    Jp[:, d] = np.cross(axis, c - anchor)
            a = pod.body_parentid[a]
        Il = Ri.T @ Jr
        I = np.array([pod.body_inertia[b][i] for i in range(3)], dtype=T)
        M += m * (Jp.T @ Jp) + Il.T @ (I[:, None] * Il)
    for d in range(nv):
        M[d, d] += T(pod.dof_armature[d])
    return M


def lowest_points(pod, kin):
    """Per body: the lowest world z of the collision geoms of the body's subtree (inf where it has none)."""
    low = np.full(pod.nbody, np.inf)
    for g in range(pod.ngeom):
        b, t = pod.geom_bodyid[g], pod.geom_type[g]
        if b == 0 or t not in (SPHERE, CAPSULE, BOX):
            continue
        R = np.asarray(kin["xmat"][b], dtype=np.float64) @ _quat_mat(pod.geom_quat[g], np.float64)
        c = np.asarray(kin["xpos"][b], dtype=np.float64) + np.asarray(kin["xmat"][b], dtype=np.float64) @ np.array(pod.geom_pos[g][:3])
        s = pod.geom_size[g]
        z = c[2] - (s[0] if t == SPHERE else s[0] + abs(R[2, 2]) * s[1] if t == CAPSULE else sum(abs(R[2, k]) * s[k] for k in range(3)))
        a = b
        while a > 0:
            low[a] = min(low[a], z)
            a = pod.body_parentid[a]
    return low
