"""The depth image (phys_batch_depth_image, include/cassie_phys.h) restated in numpy FROM ITS DEFINITION, not from the kernel's text --
test infrastructure shared by tests/test_depth.py (the emulated kernel) and tests/test_depth_gpu.py (the device).

Definition.  The camera sits at cam_pos, cam_quat in the frame of the body (the pelvis: tests/terrain_check.py pelvis_pose), looks
along -z of its own frame, +x right, +y up.  Pixel (r, c) of H x W has the camera-frame direction d = (a T (2 (c + 1/2) / W - 1),
T (1 - 2 (r + 1/2) / H), -1), T = tan(fovy / 2), a = W / H, not normalised; its value is the smallest t in [near, far] at which
o + t R d meets a static collision geom, `far` where there is none.

How this file computes it (the kernel: a slab test for boxes, a cell-by-cell walk for the height field):
  plane          t = -o_z / d_z in the geom's frame;
  box            the ray against each of the six face planes, kept where the point lies within the face: the entry is the smaller
                 of the (at most two) crossings, an origin between the two gives `near`;
  height field   the segment clipped to [near, far] and to the footprint (and to z in [-PAD, sz + PAD], which drops no point of a
                 surface of elevations 0 .. 1); EVERY parameter at which it crosses an x or a y grid line, sorted; the midpoint of
                 each interval names a cell; that cell's two triangles by a Moeller-Trumbore test; the smallest accepted t.
brute_force() pins that against every triangle of the grid (plane crossing + barycentric coordinates in the x-y projection).

near_mask flags the rays whose value is not well determined (EPS = 1e-9):
  * a barycentric coordinate (height field) or a face margin (box) of the winning hit within EPS of its threshold;
  * a rejected candidate in front of the winner that is within EPS of being accepted;
  * a candidate within EPS of `near` or `far` (what the clip to [near, far] decides);
  * a grazing ray, |n.d| / (|n| |d|) < GRAZE = 1e-3 on the winning surface (the depth's conditioning reaches 1e3 there).
"""
import numpy as np

import terrain_check as tc

EPS = 1e-9
GRAZE = 1e-3
PAD = 1e-6
TOL = 1e-11


def unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def pixel_dirs(W, H, fovy_deg):
    """[H * W][3] camera-frame directions, row-major, row 0 at the top."""
    T = np.tan(np.radians(fovy_deg) / 2)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = (W / H) * T * (2 * (c + 0.5) / W - 1)
    y = T * (1 - 2 * (r + 0.5) / H)
    return np.stack([x, y, -np.ones_like(x)], axis=-1).reshape(-1, 3)


def rays(qpos, cam_pos, cam_quat, W, H, fovy_deg, pose=None):
    """World rays of every env: origins [E][3], directions [E][P][3].  pose: [E][7] per-env extrinsics in the place of the shared ones."""
    qpos = np.asarray(qpos, dtype=np.float64)
    E = qpos.shape[0]
    bp, bq = tc.pelvis_pose(qpos)
    cp = np.tile(np.asarray(cam_pos, dtype=np.float64), (E, 1)) if pose is None else np.asarray(pose, dtype=np.float64)[:, 0:3]
    cq = np.tile(np.asarray(cam_quat, dtype=np.float64), (E, 1)) if pose is None else np.asarray(pose, dtype=np.float64)[:, 3:7]
    Rb = tc.quat2mat(bq)
    Rc = Rb @ tc.quat2mat(unit(cq))
    o = bp + np.einsum("eij,ej->ei", Rb, cp)
    D = np.einsum("eij,pj->epi", Rc, pixel_dirs(W, H, fovy_deg))
    return o, D


class _Best:
    """Per ray: the winning candidate so far, whether it is ill-determined, and the nearest almost-accepted candidate."""

    def __init__(self, n, far):
        self.t = np.full(n, np.inf)
        self.bad = np.zeros(n, dtype=bool)
        self.almost = np.full(n, np.inf)
        self.far = far

    def take(self, idx, t, bad):
        """candidates t (accepted) of rays idx, with their own flags"""
        order = np.lexsort((t, idx))
        idx, t, bad = idx[order], t[order], bad[order]
        first = np.ones(idx.size, dtype=bool)
        first[1:] = idx[1:] != idx[:-1]
        idx, t, bad = idx[first], t[first], bad[first]
        better = t < self.t[idx]
        self.t[idx[better]] = t[better]
        self.bad[idx[better]] = bad[better]

    def nearly(self, idx, t):
        np.minimum.at(self.almost, idx, t)

    def result(self):
        hit = np.isfinite(self.t)
        val = np.where(hit, self.t, self.far)
        return val, (hit & self.bad) | (self.almost < val)


def _range_flags(t, near, far):
    return (np.abs(t - near) < EPS) | (np.abs(t - far) < EPS)


def _plane(best, o, d, near, far):
    dz = np.where(d[:, 2] != 0, d[:, 2], 1.0)
    t = np.where(d[:, 2] != 0, -o[:, 2] / dz, np.inf)
    ok = (t >= near) & (t <= far)
    graze = np.abs(d[:, 2]) / np.linalg.norm(d, axis=1) < GRAZE
    idx = np.nonzero(ok)[0]
    best.take(idx, t[idx], (graze | _range_flags(t, near, far))[idx])
    al = np.nonzero(~ok & _range_flags(t, near, far))[0]
    best.nearly(al, np.minimum(t[al], far))


def _box(best, o, d, size, near, far):
    n = o.shape[0]
    t_in, t_out = np.full(n, np.inf), np.full(n, -np.inf)
    m_in, m_out = np.full(n, np.inf), np.full(n, np.inf)      # the face margins of the entry / the exit
    g_in = np.zeros(n)
    almost = np.full(n, np.inf)
    dn = np.linalg.norm(d, axis=1)
    for k in range(3):
        m1, m2 = (k + 1) % 3, (k + 2) % 3
        dk = np.where(d[:, k] != 0, d[:, k], 1.0)
        for sgn in (-1.0, 1.0):
            t = np.where(d[:, k] != 0, (sgn * size[k] - o[:, k]) / dk, np.inf)
            tt = np.where(np.isfinite(t), t, 0.0)
            margin = np.minimum(size[m1] - np.abs(o[:, m1] + tt * d[:, m1]), size[m2] - np.abs(o[:, m2] + tt * d[:, m2]))
            on = np.isfinite(t) & (margin >= 0)
            almost = np.where(np.isfinite(t) & ~on & (margin > -EPS), np.minimum(almost, t), almost)
            lo = on & (t < t_in)
            t_in, m_in, g_in = np.where(lo, t, t_in), np.where(lo, margin, m_in), np.where(lo, np.abs(d[:, k]) / dn, g_in)
            hi = on & (t > t_out)
            t_out, m_out = np.where(hi, t, t_out), np.where(hi, margin, m_out)
    crossed = np.isfinite(t_in) & (t_out >= t_in)
    front = crossed & (t_in >= near) & (t_in <= far)
    inside = crossed & (t_in < near) & (t_out >= near)
    t = np.where(front, t_in, near)
    bad = np.where(front, (m_in < EPS) | (g_in < GRAZE) | _range_flags(t_in, near, far),
                   (m_in < EPS) | (m_out < EPS) | (np.abs(t_in - near) < EPS) | (np.abs(t_out - near) < EPS))
    idx = np.nonzero(front | inside)[0]
    best.take(idx, t[idx], bad[idx])
    # a face nearly hit (the ray passes within EPS of the box's edge), or a box that ends within EPS of the near plane
    al = np.nonzero(np.isfinite(almost) & (almost >= near - EPS) & (almost <= far))[0]
    best.nearly(al, np.maximum(almost[al], near))
    al = np.nonzero(crossed & ~front & ~inside & ((np.abs(t_out - near) < EPS) | (np.abs(t_in - far) < EPS)))[0]
    best.nearly(al, np.full(al.size, near))


def _triangle(o, d, a, b, c):
    """Moeller-Trumbore: the ray o + t d against the triangle a b c -> t, u, v, |n.d| / (|n| |d|)  (t = inf where parallel)."""
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = np.einsum("ij,ij->i", e1, p)
    ok = det != 0
    inv = 1.0 / np.where(ok, det, 1.0)
    s = o - a
    u = np.einsum("ij,ij->i", s, p) * inv
    q = np.cross(s, e1)
    v = np.einsum("ij,ij->i", d, q) * inv
    t = np.where(ok, np.einsum("ij,ij->i", e2, q) * inv, np.inf)
    nrm = np.cross(e1, e2)
    cosine = np.abs(np.einsum("ij,ij->i", nrm, d)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d, axis=1))
    return t, u, v, cosine


def _hfield(best, o, d, env, grids, size, nr, nc, near, far):
    """o, d [n][3] in the geom's frame, env [n] the ray's env (row of grids [E][nr][nc])."""
    sx, sy, sz = size
    n = o.shape[0]
    t0, t1 = np.full(n, float(near)), np.full(n, float(far))
    alive = np.ones(n, dtype=bool)
    for k, (lo, hi) in enumerate(((-sx, sx), (-sy, sy), (-PAD, sz + PAD))):
        moving = d[:, k] != 0
        dk = np.where(moving, d[:, k], 1.0)
        ta, tb = (lo - o[:, k]) / dk, (hi - o[:, k]) / dk
        t0 = np.where(moving, np.maximum(t0, np.minimum(ta, tb)), t0)
        t1 = np.where(moving, np.minimum(t1, np.maximum(ta, tb)), t1)
        alive &= moving | ((o[:, k] >= lo) & (o[:, k] <= hi))
    alive &= t0 <= t1
    ray = np.nonzero(alive)[0]
    if ray.size == 0:
        return
    o, d, env, t0, t1 = o[ray], d[ray], env[ray], t0[ray], t1[ray]
    cx, cy = 2 * sx / (nc - 1), 2 * sy / (nr - 1)
    # every parameter at which the segment crosses a grid line: lines k with the coordinate between the segment's ends
    ids, ts = [np.arange(ray.size), np.arange(ray.size)], [t0, t1]
    for k, (half, cell, count) in enumerate(((sx, cx, nc), (sy, cy, nr))):
        ga, gb = (o[:, k] + t0 * d[:, k] + half) / cell, (o[:, k] + t1 * d[:, k] + half) / cell
        first = np.clip(np.ceil(np.minimum(ga, gb)), 0, count - 1).astype(np.int64)
        last = np.clip(np.floor(np.maximum(ga, gb)), 0, count - 1).astype(np.int64)
        cnt = np.where((d[:, k] != 0) & (last >= first), last - first + 1, 0)
        who = np.repeat(np.arange(ray.size), cnt)
        line = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(first, cnt)
        t = ((-half + line * cell) - o[who, k]) / d[who, k]
        ids.append(who)
        ts.append(np.clip(t, t0[who], t1[who]))
    ids, ts = np.concatenate(ids), np.concatenate(ts)
    order = np.lexsort((ts, ids))
    ids, ts = ids[order], ts[order]
    same = ids[1:] == ids[:-1]
    who, tm = ids[:-1][same], 0.5 * (ts[:-1][same] + ts[1:][same])
    # the cell under the midpoint of each interval
    j = np.clip(np.floor((o[who, 0] + tm * d[who, 0] + sx) / cx).astype(np.int64), 0, nc - 2)
    i = np.clip(np.floor((o[who, 1] + tm * d[who, 1] + sy) / cy).astype(np.int64), 0, nr - 2)
    # (an interval of length zero -- a crossing at a clip end, a ray through a corner -- names a cell twice: harmless)
    G = grids
    e = env[who]
    x0, y0 = -sx + j * cx, -sy + i * cy
    v = lambda ii, jj, xx, yy: np.stack([xx, yy, sz * G[e, ii, jj].astype(np.float64)], axis=-1)
    v00, v10, v01, v11 = v(i, j, x0, y0), v(i, j + 1, x0 + cx, y0), v(i + 1, j, x0, y0 + cy), v(i + 1, j + 1, x0 + cx, y0 + cy)
    for a, b, c in ((v00, v10, v01), (v11, v01, v10)):
        t, u, w, cosine = _triangle(o[who], d[who], a, b, c)
        margin = np.minimum(np.minimum(u, w), 1.0 - u - w)
        inrange = (t >= near) & (t <= far)
        ok = (margin >= 0) & inrange
        bad = (margin < EPS) | (cosine < GRAZE) | _range_flags(t, near, far)
        best.take(ray[who[ok]], t[ok], bad[ok])
        al = ~ok & np.isfinite(t) & (margin > -EPS) & (t > near - EPS) & (t < far + EPS)
        best.nearly(ray[who[al]], np.clip(t[al], near, far))


def depth(pod, qpos, cam_pos, cam_quat, W, H, fovy_deg, near, far, geom_pos=None, geom_quat=None, grids=None, pose=None):
    """-> (depth [E][H * W], near_mask [E][H * W]).  grids: [E][nrow][ncol] (every env's own) or None; geom_pos / geom_quat: per-env geom
    poses [E][ngeom][3 / 4] (default: the model's)."""
    qpos = np.asarray(qpos, dtype=np.float64)
    E = qpos.shape[0]
    if geom_pos is None:
        geom_pos, geom_quat = tc.model_geom_poses(pod, E)
    o, D = rays(qpos, cam_pos, cam_quat, W, H, fovy_deg, pose)
    P = D.shape[1]
    best = _Best(E * P, far)
    env = np.repeat(np.arange(E), P)
    for g, kind in tc.static_geoms(pod):
        R = tc.quat2mat(geom_quat[:, g])
        og = np.einsum("eji,ej->ei", R, o - geom_pos[:, g])                  # R^T (o - p)
        dg = np.einsum("eji,epj->epi", R, D).reshape(-1, 3)
        og = np.repeat(og, P, axis=0)
        if kind == tc.PLANE:
            _plane(best, og, dg, near, far)
        elif kind == tc.BOX:
            _box(best, og, dg, np.array(list(pod.geom_size[g])), near, far)
        elif grids is not None:
            _hfield(best, og, dg, env, np.asarray(grids), tuple(pod.hfield_size[k] for k in range(3)), pod.hfield_nrow, pod.hfield_ncol, near, far)
    val, mask = best.result()
    return val.reshape(E, P), mask.reshape(E, P)


def brute_force(pod, qpos, cam_pos, cam_quat, W, H, fovy_deg, near, far, geom_pos, geom_quat, grids, picks, pose=None):
    """The height field alone, for the rays picks = (env [n], pixel [n]), against EVERY triangle of the env's grid: the crossing of the
    triangle's plane, kept where its x-y projection lies in the triangle's -> t [n] (inf: none).  pose: per-env extrinsics, as for depth()."""
    o, D = rays(qpos, cam_pos, cam_quat, W, H, fovy_deg, pose)
    g = pod.hfield_geom
    sx, sy, sz = (pod.hfield_size[k] for k in range(3))
    nr, nc = pod.hfield_nrow, pod.hfield_ncol
    cx, cy = 2 * sx / (nc - 1), 2 * sy / (nr - 1)
    xs, ys = -sx + np.arange(nc) * cx, -sy + np.arange(nr) * cy
    out = np.full(len(picks[0]), np.inf)
    for e in np.unique(picks[0]):
        sel = np.nonzero(picks[0] == e)[0]
        R = tc.quat2mat(geom_quat[e, g])
        og = R.T @ (o[e] - geom_pos[e, g])
        dg = D[e, picks[1][sel]] @ R                                          # rows R^T d
        Z = sz * np.asarray(grids[e], dtype=np.float64)
        x0, y0 = np.meshgrid(xs[:-1], ys[:-1])                               # [nr - 1][nc - 1] cell corners
        z00, z10, z01, z11 = Z[:-1, :-1], Z[:-1, 1:], Z[1:, :-1], Z[1:, 1:]
        # lower triangles: z = z00 + (x - x0) (z10 - z00) / cx + (y - y0) (z01 - z00) / cy; upper ones from v11 likewise
        for zc, gx, gy, xc, yc, sgn in ((z00, (z10 - z00) / cx, (z01 - z00) / cy, x0, y0, 1.0),
                                        (z11, (z11 - z01) / cx, (z11 - z10) / cy, x0 + cx, y0 + cy, -1.0)):
            N = np.stack([-gx.ravel(), -gy.ravel(), np.ones(gx.size)], axis=1)            # plane: N . (p - corner) = 0
            cst = np.einsum("ij,ij->i", N, np.stack([xc.ravel(), yc.ravel(), zc.ravel()], axis=1))
            for lo in range(0, sel.size, 64):
                part = sel[lo:lo + 64]
                dd = dg[lo:lo + 64]
                den = N @ dd.T                                                            # [T][r]
                t = (cst[:, None] - (N @ og)[:, None]) / np.where(den != 0, den, np.nan)
                u = sgn * (og[0] + t * dd[:, 0][None, :] - xc.ravel()[:, None]) / cx
                w = sgn * (og[1] + t * dd[:, 1][None, :] - yc.ravel()[:, None]) / cy
                ok = (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= near) & (t <= far)
                out[part] = np.minimum(out[part], np.where(ok, t, np.inf).min(axis=0))
    return out


def compare(got, want, mask, what="depth image", tol=TOL):
    """Asserts got == want within tol wherever the ray is not masked; prints the largest difference seen."""
    err = np.where(mask, 0.0, np.abs(got - want))
    print("%s: %d rays, %.4f %% masked, largest difference %.3g m" % (what, got.size, 100 * float(np.mean(mask)), float(err.max())))
    assert float(err.max()) <= tol, "differs by %.3g m at %s" % (float(err.max()), np.unravel_index(np.argmax(err), err.shape))


def check_mask(mask, most=0.01):
    """The condition on a case, from the restatement alone: fewer than 1 % of its rays are ill-determined."""
    frac = float(np.mean(mask))
    assert frac < most, "%.3f %% of the rays are within 1e-9 of a threshold or grazing" % (100 * frac)


def ramp_noise_flat_bank(nrow, ncol, count, seed=0):
    """`count` grids of elevations in [0, 1] with no vertical faces: flat, a ramp along x, smooth bumps, noise, a ramp along y, ..."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, nrow), np.linspace(0, 1, ncol), indexing="ij")
    out = []
    for k in range(count):
        kind = k % 4
        if kind == 0:
            g = np.full((nrow, ncol), 0.25 + 0.125 * (k // 4))
        elif kind == 1:
            g = x if (k // 4) % 2 == 0 else y
        elif kind == 2:
            g = 0.5 + 0.25 * np.sin((9 + k) * x) * np.cos((7 + k) * y)
        else:
            g = rng.random((nrow, ncol))
        out.append(np.asarray(g, dtype=np.float32))
    return np.stack(out)


def pitched_down(deg):
    """The quaternion of a camera on a body whose x axis points ahead and z axis up: looking ahead, pitched `deg` degrees down.
    (At 0 the camera's -z is the body's +x, its +x the body's -y, its +y the body's +z.)"""
    level = np.array([0.5, 0.5, -0.5, -0.5])          # columns of its matrix: (0, -1, 0), (0, 0, 1), (-1, 0, 0)
    a = np.radians(deg) / 2
    pitch = np.array([np.cos(a), -np.sin(a), 0.0, 0.0])   # about the camera's own x (right): nose down
    w1, x1, y1, z1 = level
    w2, x2, y2, z2 = pitch
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def sample_rays(envs, per_env, npix, seed):
    """picks for brute_force: per_env distinct pixels of each env of `envs` -> (env [n], pixel [n])."""
    rng = np.random.default_rng(seed)
    return (np.repeat(np.asarray(envs), per_env), np.concatenate([rng.choice(npix, per_env, replace=False) for _ in envs]))


def compare_brute(t, want, mask, picks, far, what, tol=1e-12):
    """Asserts that brute_force's t agrees with the restatement's values at the rays `picks` within tol off the mask."""
    brute = np.where(np.isfinite(t), t, far)
    err = np.where(mask[picks], 0.0, np.abs(brute - want[picks]))
    print("%s: restatement against brute force, %d rays, %d hits, largest difference %.3g m" % (what, t.size, int(np.isfinite(t).sum()), float(err.max())))
    assert float(err.max()) <= tol
    return int(np.isfinite(t).sum())
