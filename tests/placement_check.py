"""Placed restarts (include/cassie_phys.h: "PLACED RESTARTS", the seven steps that replace step 4 of phys_batch_end_episodes) restated in
numpy FROM THE HEADER, not from the kernel's text -- shared by the emulator suite (tests/test_placement.py) and the GPU suite
(tests/test_placement_gpu.py).  Built on episode_check.end_episodes (steps 1 - 4 of the call, the restart unplaced) and
terrain_check.surface (the height scan's surface S).

A `place` dict holds what phys_batch_place_configure and the three per-env arrays hold, and what the surface reads:
  anchor, footprint [P][2] or None, ground_ref, pose [nenv][4], ground [nenv] (written), nxt [nenv] int32 or None,
  index [nenv] int32 or None (the terrain index: written where nxt is given), grids [T][nrow][ncol] or None (the bank of terrains),
  geom_pos / geom_quat [nenv][ngeom][3 / 4] or None (the model's own).
Like terrain_check.scan, end_episodes reports which envs have a footprint point within 1e-9 m of a border between surface pieces."""
import numpy as np

import episode_check as ec
import terrain_check as tc

JNT_FREE, JNT_BALL, JNT_SLIDE = 0, 1, 2
SENS_FRAMEQUAT, SENS_ACCELEROMETER, SENS_MAGNETOMETER = 2, 4, 5
WARN_TERRAIN_INDEX, WARN_SCAN_TILTED, WARN_PLACE_MISS = 32, 64, 128
REL_TOL = 1e-12          # transformed entries: within REL_TOL * max(1, |v|)
ABS_TOL = 1e-12          # the ground height and the z entries: the scan suite's own bound
MOST_NEAR = 0.05         # fewer than this share of the restarted envs may have a footprint point near a border


def quat_mul(a, b):
    w1, x1, y1, z1 = (a[..., k] for k in range(4))
    w2, x2, y2, z2 = (b[..., k] for k in range(4))
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def qz(yaw):
    yaw = np.asarray(yaw, dtype=np.float64)
    return np.stack([np.cos(yaw / 2), np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2)], axis=-1)


def moving_roots(pod):
    """Children of the world with at least one joint."""
    return [b for b in range(1, pod.nbody) if pod.body_parentid[b] == 0 and pod.body_jntnum[b] > 0]


def root_layout(pod, b):
    """Where a moving root's world pose sits in qpos / qvel: dict(free, qpos address of x, y, z, of the quaternion, dofs of x and y)."""
    joints = range(pod.body_jntadr[b], pod.body_jntadr[b] + pod.body_jntnum[b])
    types = [pod.jnt_type[j] for j in joints]
    if types == [JNT_FREE]:
        j = joints[0]
        qa, da = pod.jnt_qposadr[j], pod.jnt_dofadr[j]
        return dict(free=True, q=[qa, qa + 1, qa + 2], quat=qa + 3, v=[da, da + 1])
    assert types == [JNT_SLIDE] * 3 + [JNT_BALL], "a moving root outside the accepted forms"
    assert list(pod.body_quat[b]) == [1, 0, 0, 0] and list(pod.jnt_pos[joints[3]]) == [0, 0, 0]
    q, v = [None] * 3, [None] * 3
    for j in joints[:3]:
        k = [list(pod.jnt_axis[j]) == e for e in ([1, 0, 0], [0, 1, 0], [0, 0, 1])].index(True)
        q[k], v[k] = pod.jnt_qposadr[j], pod.jnt_dofadr[j]
    return dict(free=False, q=q, quat=pod.jnt_qposadr[joints[3]], v=v[:2])


def root_pose(pod, b, qpos):
    """World position [E][3] and unit quaternion [E][4] of a moving root from qpos [E][nq]: a free joint's entries, or the body's place
    plus its slides' travel from qpos0 and the ball's quaternion -- normalised, as the scan does."""
    L = root_layout(pod, b)
    quat = qpos[:, L["quat"]:L["quat"] + 4]
    quat = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    if L["free"]:
        return qpos[:, L["q"]].copy(), quat
    pos = np.stack([pod.body_pos[b][k] + (qpos[:, L["q"][k]] - pod.qpos0[L["q"][k]]) for k in range(3)], axis=1)
    return pos, quat


def placed_sensors(pod):
    out = []
    for s in range(pod.nsensor):
        if pod.sensor_type[s] in (SENS_FRAMEQUAT, SENS_MAGNETOMETER):
            assert pod.sensor_body[s] in moving_roots(pod)
            out.append(s)
    return out


def transformed_columns(pod):
    """Which columns of qpos / qvel (= qacc) / sensordata a placement may change, and which qpos columns are world z."""
    qc, vc, zc, sc = [], [], [], []
    for b in moving_roots(pod):
        L = root_layout(pod, b)
        qc += L["q"] + list(range(L["quat"], L["quat"] + 4))
        zc.append(L["q"][2])
        vc += L["v"]
    for s in placed_sensors(pod):
        sc += list(range(pod.sensor_adr[s], pod.sensor_adr[s] + pod.sensor_dim[s]))
    return dict(qpos=sorted(qc), qvel=sorted(vc), qacc=sorted(vc), sensordata=sorted(sc), z=sorted(zc))


def place_rows(pod, rows, place, envs):
    """Steps 1 - 6 for the envs `envs` (absolute ids) that restart from `rows` [E][row_dim]: -> (qpos, qvel, sensordata, qacc as the
    placed envs hold them, G [E], warning bits [E], near [E]); writes place["index"] (step 1)."""
    nq, nv, nsd, nu = pod.nq, pod.nv, pod.nsensordata, pod.nu
    E = len(envs)
    rq, rv, rs = rows[:, :nq].copy(), rows[:, nq:nq + nv].copy(), rows[:, nq + nv:nq + nv + nsd].copy()
    ra = rows[:, nq + nv + nsd + nu:].copy()
    pose = place["pose"][envs]
    dx, dy, dz, yaw = (pose[:, k] for k in range(4))
    gref = place["ground_ref"]
    bits = np.zeros(E, dtype=np.int32)
    fp = place.get("footprint")
    npoints = 0 if fp is None else len(fp)
    grids_all, index, nxt = place.get("grids"), place.get("index"), place.get("nxt")
    # 1. terrain
    idx = None
    if grids_all is not None and index is not None:
        nt = len(grids_all)
        want = nxt[envs] if nxt is not None else index[envs]
        idx = np.clip(want, 0, nt - 1)
        if nxt is not None:
            index[envs] = idx
            bits[want != idx] |= WARN_TERRAIN_INDEX
        elif npoints > 0:
            bits[want != idx] |= WARN_TERRAIN_INDEX
    # 2. anchor
    apos, aquat = root_pose(pod, place["anchor"], rq)
    ax, ay = apos[:, 0], apos[:, 1]
    psi = tc.yaw_of(aquat)
    # 3. ground
    G = np.full(E, float(gref))
    near = np.zeros(E, dtype=bool)
    if npoints > 0:
        o = np.asarray(fp, dtype=np.float64)
        a = (psi + yaw)[:, None]
        X = (ax + dx)[:, None] + np.cos(a) * o[None, :, 0] - np.sin(a) * o[None, :, 1]
        Y = (ay + dy)[:, None] + np.sin(a) * o[None, :, 0] + np.cos(a) * o[None, :, 1]
        gp, gq = place.get("geom_pos"), place.get("geom_quat")
        if gp is None:
            gp, gq = tc.model_geom_poses(pod, E)
        else:
            gp, gq = gp[envs], gq[envs]
        grids = None if idx is None else grids_all[idx]
        top, hit, pieces, tilted = tc.surface(pod, X, Y, gp, gq, grids)
        some = hit.any(axis=1)
        G = np.where(some, np.max(np.where(hit, top, -np.inf), axis=1), float(gref))
        bits[~some] |= WARN_PLACE_MISS
        bits[tilted] |= WARN_SCAN_TILTED
        for ex in (-tc.EPS, tc.EPS):
            for ey in (-tc.EPS, tc.EPS):
                _, _, pc, _ = tc.surface(pod, X + ex, Y + ey, gp, gq, grids)
                near |= np.any(pc != pieces, axis=(1, 2))
    # 4. rigid motion of every moving root
    h = dz + G - gref
    c, s = np.cos(yaw), np.sin(yaw)
    q_out = rq.copy()
    for b in moving_roots(pod):
        L = root_layout(pod, b)
        p, _ = root_pose(pod, b, rq)
        rx, ry = p[:, 0] - ax, p[:, 1] - ay
        T = np.stack([p[:, 0] + dx + ((c - 1) * rx - s * ry), p[:, 1] + dy + (s * rx + (c - 1) * ry), p[:, 2] + h], axis=1)
        for k in range(3):
            q_out[:, L["q"][k]] = T[:, k] if L["free"] else pod.qpos0[L["q"][k]] + (T[:, k] - pod.body_pos[b][k])
        q_out[:, L["quat"]:L["quat"] + 4] = quat_mul(qz(yaw), rq[:, L["quat"]:L["quat"] + 4])
    # 5. the roots' linear velocities and accelerations
    v_out, a_out = rv.copy(), ra.copy()
    for b in moving_roots(pod):
        vx, vy = root_layout(pod, b)["v"]
        for src, dst in ((rv, v_out), (ra, a_out)):
            dst[:, vx] = c * src[:, vx] - s * src[:, vy]
            dst[:, vy] = s * src[:, vx] + c * src[:, vy]
    # 6. framequat and magnetometer
    s_out = rs.copy()
    B = np.array(list(pod.magnetic))
    for sn in placed_sensors(pod):
        adr = pod.sensor_adr[sn]
        if pod.sensor_type[sn] == SENS_FRAMEQUAT:
            s_out[:, adr:adr + 4] = quat_mul(qz(yaw), rs[:, adr:adr + 4])
        else:
            _, bq = root_pose(pod, pod.sensor_body[sn], rq)
            sq = np.array(list(pod.sensor_squat[sn]))
            R = tc.quat2mat(quat_mul(qz(yaw), quat_mul(bq, sq[None, :])))
            val = np.einsum("eij,i->ej", R, B)
            cut = pod.sensor_cutoff[sn]
            if cut > 0:
                val = np.clip(val, -cut, cut)
            turned = yaw != 0.0
            s_out[turned, adr:adr + 3] = val[turned]
    return q_out, v_out, s_out, a_out, G, bits, near


def end_episodes(state, pod, r, env0, n, restart, bank, place, pick=None, force=None):
    """The whole call on `state` and `place`, in place -> (mask over the range of the envs that ended, absolute ids of the envs that
    restarted, near [those envs])."""
    done = ec.end_episodes(state, pod, r, env0, n, restart, bank=bank, pick=pick, force=force)
    envs = env0 + np.nonzero(done)[0]
    if not restart or len(envs) == 0:
        return done, envs[:0], np.zeros(0, dtype=bool)
    rows = bank[ec.bank_rows(env0, n, state["count"][env0:env0 + n], bank.shape[0], pick)[done]]
    q, v, s, a, G, bits, near = place_rows(pod, rows, place, envs)
    state["qpos"][envs], state["qvel"][envs], state["sensordata"][envs], state["qacc"][envs] = q, v, s, a
    state["warn"][envs] = bits                                                                # 7
    place["ground"][envs] = G
    return done, envs, near


def compare(got, want, got_place, want_place, pod, envs, near, what=""):
    """The comparison of the issue: entries the definition leaves alone are equal; transformed entries within REL_TOL * max(1, |v|);
    PHYS_PLACE_GROUND and the z entries within ABS_TOL, envs with a footprint point near a border left out of those two only (fewer
    than MOST_NEAR of the restarted envs, asserted first); episode words, the terrain index and the warning words equal."""
    assert len(envs) > 0
    frac = float(np.mean(near))
    assert frac < MOST_NEAR, "%s: %.2f %% of the restarted envs have a footprint point within 1e-9 m of a border" % (what, 100 * frac)
    cols = transformed_columns(pod)
    worst_rel = worst_abs = 0.0
    for k in got:
        if got[k] is None or want[k] is None:
            assert got[k] is None and want[k] is None, k
            continue
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, k
        if k not in cols:
            assert g.tobytes() == w.tobytes(), "%s: %s differs in envs %s" % (what, k, np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:16])
            continue
        changed = np.zeros(g.shape, dtype=bool)
        changed[np.ix_(envs, cols[k])] = True
        assert np.array_equal(g[~changed], w[~changed]), "%s: %s differs outside the transformed entries: %s" % (what, k, np.argwhere((g != w) & ~changed)[:8])
        zmask = np.zeros(g.shape, dtype=bool)
        if k == "qpos":
            zmask[np.ix_(envs, cols["z"])] = True
        rel = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        r = float(np.max(np.where(changed & ~zmask, rel, 0.0)))
        assert r <= REL_TOL, "%s: a transformed entry of %s differs by %.3g (relative) at %s" % (what, k, r, np.unravel_index(np.argmax(np.where(changed & ~zmask, rel, 0.0)), g.shape))
        worst_rel = max(worst_rel, r)
        if k == "qpos":
            zerr = np.abs(g - w)
            zerr[envs[near]] = 0.0
            a = float(np.max(np.where(zmask, zerr, 0.0)))
            assert a <= ABS_TOL, "%s: a z entry differs by %.3g m in env %s" % (what, a, np.unravel_index(np.argmax(np.where(zmask, zerr, 0.0)), g.shape))
            worst_abs = max(worst_abs, a)
    gerr = np.abs(got_place["ground"][envs] - want_place["ground"][envs])
    gerr[near] = 0.0
    assert float(gerr.max()) <= ABS_TOL, "%s: PHYS_PLACE_GROUND differs by %.3g m in env %d" % (what, float(gerr.max()), envs[int(np.argmax(gerr))])
    others = np.ones(len(got_place["ground"]), dtype=bool)
    others[envs] = False
    assert np.array_equal(got_place["ground"][others], want_place["ground"][others]), "PHYS_PLACE_GROUND changed for an env that did not restart"
    if want_place.get("index") is not None:
        assert np.array_equal(got_place["index"], want_place["index"]), "%s: the terrain index differs" % what
    print("%s: %d envs restarted, %d near a border; transformed entries within %.2g (relative), z within %.2g m, ground within %.2g m"
          % (what, len(envs), int(near.sum()), worst_rel, worst_abs, float(gerr.max())))
