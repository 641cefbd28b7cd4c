"""The range sensors on any body (phys_batch_rays_configure / phys_batch_rays_cast, include/cassie_phys.h) restated in numpy FROM THEIR
DEFINITION, not from the kernel's text -- test infrastructure shared by tests/test_rays.py (the emulated kernel) and
tests/test_rays_gpu.py (the device).  The geoms' world poses, the plane, box, sphere, capsule and height-field values and their masks
are depth_check's and depth_scene_check's; this file adds the three frames of a ray, the self-exclusion, the range [rmin, rmax], the hit
ids and the normals.

How this file computes the normals (the kernel: once per ray behind its geom loop, from the hit point in the winning geom's frame):
  plane          -+ the geom's z axis, against the ray;
  box            per axis the parameter at which the ray enters the slab, the axis of the largest (the first of equals), against the ray;
  sphere         the hit point over its length;
  capsule        the hit point less its projection onto the segment;
  height field   the cell and the side of its diagonal the hit point lies on, the plane through that triangle's three vertices.
normal_by_difference() pins the solids' independently: the gradient of the solid's signed distance at the hit point by central finite
differences.

The masks: depth_scene_check's for the values and the ids; for the normals, besides the value's, a box hit within EPS of an edge and a
height-field hit within EPS of a cell edge or diagonal.  (A capsule's normal is continuous across the seam of side and cap: not flagged.)
"""
import numpy as np

import depth_check as dc
import depth_scene_check as sc
import terrain_check as tc

EPS, TOL = dc.EPS, dc.TOL
BODY, WORLD_DIR, HEADING = 0, 1, 2
RAY_DTYPE = np.dtype([("body", np.int32), ("frame", np.int32), ("origin", np.float64, 3), ("dir", np.float64, 3)])


def table_of(rays):
    """A list of (body, frame, origin, dir) -> the structured array phys_batch_rays_configure takes."""
    t = np.zeros(len(rays), dtype=RAY_DTYPE)
    for k, (body, frame, origin, direction) in enumerate(rays):
        t[k] = (body, frame, np.asarray(origin, dtype=np.float64), np.asarray(direction, dtype=np.float64))
    return t


def heading_matrix(q):
    """[..., 4] -> the rotation about world z by the heading atan2(2 (w z + x y), 1 - 2 (y y + z z)) of q (the identity where the body's x
    axis is vertical: atan2(0, 0) = 0; NaN where q is)."""
    w, x, y, z = (q[..., k] for k in range(4))
    a = np.arctan2(2 * (w * z + x * y), 1 - 2 * (y * y + z * z))
    c, s = np.cos(a), np.sin(a)
    R = np.zeros(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 1, 0], R[..., 1, 1], R[..., 2, 2] = c, -s, s, c, 1.0
    return R


def world_rays(table, xpos, xquat):
    """-> origins [E][N][3], directions [E][N][3]: the table's rays on the body poses AS STORED (xpos / xquat [E][nbody * 3 / 4])."""
    E = xpos.shape[0]
    xp, xq = np.asarray(xpos, dtype=np.float64).reshape(E, -1, 3), np.asarray(xquat, dtype=np.float64).reshape(E, -1, 4)
    body, frame = table["body"], table["frame"]
    u0 = table["dir"] / np.linalg.norm(table["dir"], axis=1, keepdims=True)
    p, q = xp[:, body], xq[:, body]                                       # [E][N][3 / 4]
    R, Rz = tc.quat2mat(q), heading_matrix(q)
    Ro = np.where((frame == HEADING)[None, :, None, None], Rz, R)
    o = p + np.einsum("enij,nj->eni", Ro, table["origin"])
    u = np.einsum("enij,nj->eni", Ro, u0)
    u = np.where((frame == WORLD_DIR)[None, :, None], u0[None], u)
    return o, u


def _unit(v):
    n = np.linalg.norm(v, axis=-1, keepdims=True)
    return np.where(n > 0, v / np.where(n > 0, n, 1.0), 0.0)


def _hfield_triangle(p, env, grids, size, nr, nc):
    """The triangle of the height field under the points p [n][3] (geom frame) -> its normal (up, not normalised) and how far, in
    metres, p lies from the nearest cell edge or diagonal."""
    sx, sy, sz = size
    cx, cy = 2 * sx / (nc - 1), 2 * sy / (nr - 1)
    gx, gy = (p[:, 0] + sx) / cx, (p[:, 1] + sy) / cy
    j = np.clip(np.floor(np.nan_to_num(gx)).astype(np.int64), 0, nc - 2)
    i = np.clip(np.floor(np.nan_to_num(gy)).astype(np.int64), 0, nr - 2)
    a, b = gx - j, gy - i
    G = np.asarray(grids)
    x0, y0 = -sx + j * cx, -sy + i * cy
    v = lambda ii, jj, xx, yy: np.stack([xx, yy, sz * G[env, ii, jj].astype(np.float64)], axis=-1)
    v00, v10, v01, v11 = v(i, j, x0, y0), v(i, j + 1, x0 + cx, y0), v(i + 1, j, x0, y0 + cy), v(i + 1, j + 1, x0 + cx, y0 + cy)
    lower = a + b <= 1.0
    nrm = np.where(lower[:, None], np.cross(v10 - v00, v01 - v00), np.cross(v01 - v11, v10 - v11))
    margin = np.minimum.reduce([a * cx, (1 - a) * cx, b * cy, (1 - b) * cy, np.abs(a + b - 1.0) * min(cx, cy)])
    return nrm, margin


def _normal(kind, size, og, dg, t, env, grids, pod):
    """The outward normal (geom frame, unit, against the ray) at the hit og + t dg, and whether it is ill-determined."""
    n = og.shape[0]
    p = og + np.where(np.isfinite(t), t, 0.0)[:, None] * dg
    ill = np.zeros(n, dtype=bool)
    if kind == sc.PLANE:
        nl = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif kind == sc.SPHERE:
        nl = p
    elif kind == sc.CAPSULE:
        nl = p.copy()
        nl[:, 2] -= np.clip(p[:, 2], -size[1], size[1])
    elif kind == sc.BOX:
        s = np.asarray(size, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            enter = np.where(dg != 0, np.minimum((-s - og) / dg, (s - og) / dg), -np.inf)
        axis = np.argmax(enter, axis=1)                                   # (the first of equals)
        nl = np.zeros((n, 3))
        nl[np.arange(n), axis] = 1.0
        ill = (np.abs(np.abs(p) - s) < EPS).sum(axis=1) >= 2              # on an edge
    else:
        nl, margin = _hfield_triangle(p, env, grids, tuple(pod.hfield_size[k] for k in range(3)), pod.hfield_nrow, pod.hfield_ncol)
        ill = margin < EPS
    nl = _unit(nl)
    flip = np.einsum("ij,ij->i", nl, dg) > 0
    return np.where(flip[:, None], -nl, nl), ill


def cast(pod, table, rmin, rmax, mask, xpos, xquat, geom_pos=None, geom_quat=None, grids=None):
    """-> dict(val [E][N], ids [E][N] int32, normals [E][N][3], mask, id_mask, normal_mask [E][N]).  mask: bit g = compiled geom g;
    xpos / xquat: [E][nbody * 3 / 4] as the fields hold them; geom_pos / geom_quat: per-env geom poses (default: the model's); grids:
    [E][nrow][ncol], every env's own."""
    xpos, xquat = np.asarray(xpos, dtype=np.float64), np.asarray(xquat, dtype=np.float64)
    E, N = xpos.shape[0], table.size
    if geom_pos is None:
        geom_pos, geom_quat = tc.model_geom_poses(pod, E)
    o, u = world_rays(table, xpos, xquat)
    n = E * N
    env = np.repeat(np.arange(E), N)
    ray_body = np.tile(table["body"], E)
    o, u = o.reshape(n, 3), u.reshape(n, 3)
    ray_ok = np.isfinite(o).all(axis=1) & np.isfinite(u).all(axis=1)      # a NaN pose of the ray's body: the ray sees nothing
    o, u = np.nan_to_num(o), np.where(ray_ok[:, None], np.nan_to_num(u), [0.0, 0.0, 1.0])
    GP, GR = sc.geom_world_poses(pod, geom_pos, geom_quat, xpos, xquat)
    best, second, almost = np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf)
    best_bad, best_id = np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int32)
    best_n, best_nill = np.zeros((n, 3)), np.zeros(n, dtype=bool)
    for g, kind in sc.rendered(pod, mask):
        R, p = GR[:, g], GP[:, g]
        seen = (np.isfinite(R).all(axis=(1, 2)) & np.isfinite(p).all(axis=1))[env] & ray_ok & (ray_body != pod.geom_bodyid[g])
        R, p = np.nan_to_num(R)[env], np.nan_to_num(p)[env]
        og, dg = np.einsum("nji,nj->ni", R, o - p), np.einsum("nji,nj->ni", R, u)
        size = [pod.geom_size[g][k] for k in range(3)]
        if kind in sc.SOLIDS:
            t, bad, al = sc.solid(kind, size, og, dg, rmin, rmax)
            inside = np.isfinite(t) & (t == rmin)                         # (an entry AT rmin is within EPS of it: masked)
        else:
            b = dc._Best(n, rmax)
            if kind == sc.PLANE:
                dc._plane(b, og, dg, rmin, rmax)
            elif grids is not None:
                dc._hfield(b, og, dg, env, np.asarray(grids), tuple(pod.hfield_size[k] for k in range(3)), pod.hfield_nrow, pod.hfield_ncol, rmin, rmax)
            t = np.where(b.t < rmax, b.t, np.inf)
            bad, al = b.bad & np.isfinite(t), b.almost
            inside = np.zeros(n, dtype=bool)
        t, bad, al = np.where(seen, t, np.inf), bad & seen, np.where(seen, al, np.inf)
        nl, nill = _normal(kind, size, og, dg, t, env, grids, pod)
        nw = np.where((np.isfinite(t) & ~inside)[:, None], np.einsum("nij,nj->ni", R, nl), 0.0)
        wins = t < best                                                   # (ties go to the lower index)
        second = np.where(wins, best, np.minimum(second, t))
        best_id = np.where(wins, g, best_id).astype(np.int32)
        best_bad = np.where(wins, bad, best_bad)
        best_n, best_nill = np.where(wins[:, None], nw, best_n), np.where(wins, nill & ~inside, best_nill)
        best = np.where(wins, t, best)
        almost = np.minimum(almost, al)
    hit = np.isfinite(best)
    val = np.where(hit, best, rmax)
    near_mask = (hit & best_bad) | (almost < val)
    id_mask = near_mask | (hit & (second < best + EPS)) | (almost <= val)
    normal_mask = id_mask | (hit & best_nill)
    r = lambda a: a.reshape((E, N) + a.shape[1:])
    return dict(val=r(val), ids=r(np.where(hit, best_id, -1).astype(np.int32)), normals=r(np.where(hit[:, None], best_n, 0.0)), mask=r(near_mask),
                id_mask=r(id_mask), normal_mask=r(normal_mask), o=r(o), u=r(u))


def normal_by_difference(kind, size, p, h=1e-6):
    """The gradient of the solid's signed distance at the points p [n][3] (geom frame) by central differences, normalised."""
    g = np.zeros_like(p)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        g[:, k] = (sc.signed_distance(kind, size, p + e) - sc.signed_distance(kind, size, p - e)) / (2 * h)
    return _unit(g)


def compare_normals(got, want, mask, tol, what="normals"):
    err = np.where(mask[..., None], 0.0, np.abs(got - want))
    print("%s: %d rays, %.4f %% masked, largest component difference %.3g" % (what, mask.size, 100 * float(np.mean(mask)), float(err.max())))
    assert float(err.max()) <= tol, "differs by %.3g at %s" % (float(err.max()), np.unravel_index(np.argmax(err), err.shape))
    return float(err.max())
