"""The depth image of a CHOSEN SET of geoms, moving bodies included (phys_batch_depth_set_geoms / phys_batch_depth_bind_ids,
include/cassie_phys.h), restated in numpy FROM ITS DEFINITION, not from the kernel's text -- test infrastructure shared by
tests/test_depth_scene.py (the emulated kernel) and tests/test_depth_scene_gpu.py (the device).  Rays, the plane, the box and the height
field are depth_check's; this file adds the sphere, the capsule, the poses of geoms on moving bodies, the mask and the hit ids.

How this file computes the solids (the kernel: the quadratic about the point of closest approach with the unnormalised direction; for
the capsule every root of the side with |z| <= h and every root of both spheres, smallest to largest):
  sphere    with the UNIT direction u: the foot of the perpendicular from the centre onto the ray, at distance tca along it; the
            perpendicular's squared length d2; half the chord sqrt(r^2 - d2); entry and exit (tca -+ half chord) / |d|;
  capsule   the distance function |p - clamp(p_z, -h, h) z| = r solved PIECEWISE: z along the ray is monotone, so the ray's parameter
            line splits at z = -h and z = h into at most three stretches, on each of which the distance is that to one sphere centre or
            to the axis; each stretch's quadratic is solved as for the sphere (in 3-D or in the x-y projection) and a root counts only
            inside its own stretch.  A convex solid is crossed twice: the interval runs from the smallest to the largest root;
  box       depth_check's face-by-face test, also on a moving body.
brute_force_solid() pins all three against the solids' signed distance functions: convex along a ray, so a dense search for the
smallest sample, a golden-section refinement of it and a bisection between `near` and it find the first sign change.

The mask flags, besides depth_check's rays, those whose value is not well determined:
  * an entry or exit within EPS of `near`, an entry within EPS of `far`;
  * a grazing ray: half chord / r < GRAZE on the piece that gives the value (the conditioning of the root reaches 1e3 there), or a
    ray that passes a piece within the same bound on the outside, in front of the value;
  * a root within EPS (in z) of the seam between a capsule's side and a cap;
and, for the id comparison only, a second geom within EPS of the nearest.
"""
import numpy as np

import depth_check as dc
import terrain_check as tc

EPS, GRAZE, TOL = dc.EPS, dc.GRAZE, dc.TOL
PLANE, HFIELD, SPHERE, CAPSULE, BOX = 0, 1, 2, 3, 6
SOLIDS = (SPHERE, CAPSULE, BOX)


# ------------------------------------------------------------------ which geoms, and where they are ----
def default_mask(pod):
    return sum(1 << g for g, _ in tc.static_geoms(pod))


def all_mask(pod):
    return (1 << pod.ngeom) - 1


def is_moving(pod, g):
    return pod.body_weldid[pod.geom_bodyid[g]] != 0


def moving_mask(pod):
    return sum(1 << g for g in range(pod.ngeom) if is_moving(pod, g))


def rendered(pod, mask):
    """(geom, type) of the geoms a mask shows: static planes, boxes, height field, spheres, capsules; moving spheres, capsules, boxes."""
    out = []
    for g in range(pod.ngeom):
        t = pod.geom_type[g]
        if (mask >> g) & 1 and (t in SOLIDS if is_moving(pod, g) else t in SOLIDS + (PLANE, HFIELD)):
            out.append((g, t))
    return out


def geom_world_poses(pod, geom_pos, geom_quat, xpos, xquat):
    """World position [E][ngeom][3] and rotation [E][ngeom][3][3] of every geom: its own pose (static bodies carry the identity:
    terrain_check.static_geoms asserts it for the geoms it lists), composed with xpos / xquat [E][nbody][3 / 4] AS STORED on a moving body."""
    E = geom_pos.shape[0]
    P, R = geom_pos.astype(np.float64).copy(), tc.quat2mat(np.asarray(geom_quat, dtype=np.float64))
    for g in range(pod.ngeom):
        b = pod.geom_bodyid[g]
        if is_moving(pod, g):
            RB = tc.quat2mat(np.asarray(xquat, dtype=np.float64).reshape(E, -1, 4)[:, b])
            P[:, g] = np.asarray(xpos, dtype=np.float64).reshape(E, -1, 3)[:, b] + np.einsum("eij,ej->ei", RB, geom_pos[:, g])
            R[:, g] = RB @ R[:, g]
        else:
            while b > 0:
                assert list(pod.body_pos[b]) == [0, 0, 0] and list(pod.body_quat[b]) == [1, 0, 0, 0], "a static body with a pose of its own"
                b = pod.body_parentid[b]
    return P, R


# ------------------------------------------------------------------ the solids, in the geom's frame ----
def _ball_roots(o, d, r):
    """The line o + t d (any dimension, rows) against |p| = r -> t_in, t_out (nan: none), half chord / r (negative: passes outside
    by that much, as a fraction of r, squared-scale), t of the closest approach."""
    dn = np.linalg.norm(d, axis=1)
    ok = dn > 0
    u = d / np.where(ok, dn, 1.0)[:, None]
    tca = -np.einsum("ij,ij->i", o, u)
    w = o + tca[:, None] * u
    gap = r * r - np.einsum("ij,ij->i", w, w)
    half = np.sqrt(np.maximum(gap, 0.0))
    hit = ok & (gap >= 0)
    dn1 = np.where(ok, dn, 1.0)
    t_in = np.where(hit, (tca - half) / dn1, np.nan)
    t_out = np.where(hit, (tca + half) / dn1, np.nan)
    rel = np.where(ok, np.sign(gap) * np.sqrt(np.abs(gap)) / r, -np.inf)         # (half chord / r where hit; minus the like where missed)
    return t_in, t_out, rel, np.where(ok, tca / dn1, np.nan)


def sphere_interval(o, d, r):
    """-> t0, t1 (nan: missed), ill (the entry / exit is ill-determined), nearly (t of a near miss, inf: none)"""
    t0, t1, rel, tc_ = _ball_roots(o, d, r)
    ill = np.abs(rel) < GRAZE
    nearly = np.where((rel < 0) & (rel > -GRAZE), tc_, np.inf)
    return t0, t1, ill & np.isfinite(t0), nearly


def capsule_interval(o, d, r, h):
    n = o.shape[0]
    dz = d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-h - o[:, 2]) / dz, (h - o[:, 2]) / dz          # where z = -h, z = +h
    lo = np.full(n, np.inf)
    hi = np.full(n, -np.inf)
    ill_lo, ill_hi = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    nearly = np.full(n, np.inf)
    flat = dz == 0
    for piece in (-1, 0, 1):
        # the stretch of t on which this piece is the nearest part of the segment
        if piece == 0:
            s0 = np.where(flat, np.where(np.abs(o[:, 2]) <= h, -np.inf, np.inf), np.minimum(ta, tb))
            s1 = np.where(flat, np.where(np.abs(o[:, 2]) <= h, np.inf, -np.inf), np.maximum(ta, tb))
            ti, to, rel, tcl = _ball_roots(o[:, 0:2], d[:, 0:2], r)
        else:
            edge = ta if piece < 0 else tb                        # beyond this end: z * piece > h
            beyond_up = (dz * piece) > 0                         # ... for t above the edge
            inside = (o[:, 2] * piece) > h
            s0 = np.where(flat, np.where(inside, -np.inf, np.inf), np.where(beyond_up, edge, -np.inf))
            s1 = np.where(flat, np.where(inside, np.inf, -np.inf), np.where(beyond_up, np.inf, edge))
            oc = o.copy()
            oc[:, 2] -= piece * h
            ti, to, rel, tcl = _ball_roots(oc, d, r)
        for t in (ti, to):
            on = np.isfinite(t) & (t >= s0) & (t <= s1)
            seam = np.isfinite(t) & (np.abs(np.abs(o[:, 2] + np.where(np.isfinite(t), t, 0.0) * dz) - h) < EPS)
            bad = (np.abs(rel) < GRAZE) | seam
            take = on & (t < lo)
            lo, ill_lo = np.where(take, t, lo), np.where(take, bad, ill_lo)
            take = on & (t > hi)
            hi, ill_hi = np.where(take, t, hi), np.where(take, bad, ill_hi)
            # a root just outside its stretch is a root at the seam: flag whichever end it would have been
            off = np.isfinite(t) & ~on & seam
            nearly = np.where(off, np.minimum(nearly, t), nearly)
        miss = (rel < 0) & (rel > -GRAZE) & np.isfinite(tcl) & (tcl >= s0) & (tcl <= s1)
        nearly = np.where(miss, np.minimum(nearly, tcl), nearly)
    hit = lo <= hi
    return np.where(hit, lo, np.nan), np.where(hit, hi, np.nan), hit & (ill_lo | ill_hi), nearly


def _solid_value(t0, t1, ill, nearly, near, far):
    """The convex-solid rule -> candidate t (inf: none), bad, almost (inf: none)."""
    hit = np.isfinite(t0)
    a, b = np.where(hit, t0, np.inf), np.where(hit, t1, -np.inf)
    front = hit & (a >= near) & (a < far)
    inside = hit & (a < near) & (b >= near)
    t = np.where(front, a, np.where(inside, near, np.inf))
    bad = (front | inside) & (ill | (np.abs(a - near) < EPS) | (np.abs(b - near) < EPS) | (np.abs(a - far) < EPS))
    almost = np.where(np.isfinite(nearly) & (nearly <= far), np.maximum(nearly, near), np.inf)
    almost = np.where(np.isfinite(nearly) & (nearly < near - EPS) & ~inside, np.inf, almost)   # (a near miss behind the near plane)
    almost = np.where(hit & ~front & ~inside & (np.abs(b - near) < EPS), near, almost)          # ends within EPS of the near plane
    return t, bad, almost


def solid(kind, size, o, d, near, far):
    """One solid in its own frame, rays o, d [n][3] -> candidate t [n] (inf: none), bad [n], almost [n] (inf: none)."""
    if kind == SPHERE:
        return _solid_value(*sphere_interval(o, d, size[0]), near, far)
    if kind == CAPSULE:
        return _solid_value(*capsule_interval(o, d, size[0], size[1]), near, far)
    assert kind == BOX
    b = dc._Best(o.shape[0], far)
    dc._box(b, o, d, np.asarray(size, dtype=np.float64), near, far)
    t = np.where(b.t < far, b.t, np.inf)                          # (depth_check accepts t == far: the value is `far` either way)
    return t, b.bad & np.isfinite(t), b.almost


# ------------------------------------------------------------------ the image ----
def depth(pod, qpos, cam_pos, cam_quat, W, H, fovy_deg, near, far, mask, xpos, xquat, geom_pos=None, geom_quat=None, grids=None, pose=None,
          with_id_mask=False):
    """-> (depth [E][H * W], ids [E][H * W] int32, near_mask [E][H * W]), and with_id_mask: the mask of the id comparison as a fourth.
    mask: bit g = compiled geom g; xpos / xquat: [E][nbody * 3 / 4] as the fields hold them; the rest as depth_check.depth."""
    qpos = np.asarray(qpos, dtype=np.float64)
    E = qpos.shape[0]
    if geom_pos is None:
        geom_pos, geom_quat = tc.model_geom_poses(pod, E)
    o, D = dc.rays(qpos, cam_pos, cam_quat, W, H, fovy_deg, pose)
    P = D.shape[1]
    n = E * P
    env = np.repeat(np.arange(E), P)
    GP, GR = geom_world_poses(pod, geom_pos, geom_quat, xpos, xquat)
    best, second, almost = np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf)
    best_bad, best_id = np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int32)
    for g, kind in rendered(pod, mask):
        R, p = GR[:, g], GP[:, g]
        seen = np.repeat(np.isfinite(R).all(axis=(1, 2)) & np.isfinite(p).all(axis=1), P)     # a NaN pose: the geom is unseen
        R, p = np.nan_to_num(R), np.nan_to_num(p)
        og = np.repeat(np.einsum("eji,ej->ei", R, o - p), P, axis=0)
        dg = np.einsum("eji,epj->epi", R, D).reshape(-1, 3)
        if kind in SOLIDS:
            t, bad, al = solid(kind, [pod.geom_size[g][k] for k in range(3)], og, dg, near, far)
        else:
            b = dc._Best(n, far)
            if kind == PLANE:
                dc._plane(b, og, dg, near, far)
            elif grids is not None:
                dc._hfield(b, og, dg, env, np.asarray(grids), tuple(pod.hfield_size[k] for k in range(3)), pod.hfield_nrow, pod.hfield_ncol, near, far)
            t = np.where(b.t < far, b.t, np.inf)
            bad, al = b.bad & np.isfinite(t), b.almost
        t, bad, al = np.where(seen, t, np.inf), bad & seen, np.where(seen, al, np.inf)
        wins = t < best                                           # (ties go to the lower index)
        second = np.where(wins, best, np.minimum(second, t))
        best_id = np.where(wins, g, best_id).astype(np.int32)
        best_bad = np.where(wins, bad, best_bad)
        best = np.where(wins, t, best)
        almost = np.minimum(almost, al)
    hit = np.isfinite(best)
    val = np.where(hit, best, far)
    near_mask = (hit & best_bad) | (almost < val)
    id_mask = near_mask | (hit & (second < best + EPS)) | (almost <= val)
    r = lambda a: a.reshape(E, P)
    out = (r(val), r(np.where(hit, best_id, -1).astype(np.int32)), r(near_mask))
    return out + (r(id_mask),) if with_id_mask else out


def compare_ids(got, want, id_mask, what="hit ids"):
    wrong = (got != want) & ~id_mask
    print("%s: %d rays, %.4f %% masked, %d differ" % (what, got.size, 100 * float(np.mean(id_mask)), int(wrong.sum())))
    assert not wrong.any(), "ids differ at %s" % (np.argwhere(wrong)[:5].tolist(),)


# ------------------------------------------------------------------ brute force ----
def signed_distance(kind, size, p):
    if kind == SPHERE:
        return np.linalg.norm(p, axis=-1) - size[0]
    if kind == CAPSULE:
        q = p.copy()
        q[..., 2] -= np.clip(p[..., 2], -size[1], size[1])
        return np.linalg.norm(q, axis=-1) - size[0]
    q = np.abs(p) - np.asarray(size, dtype=np.float64)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(axis=-1), 0.0)


def brute_force_solid(kind, size, o, d, near, far, samples=2001):
    """The convex-solid rule from the signed distance alone -> value [n] (inf: missed), margin [n] (how far inside the solid the
    ray's deepest sample in [near, far] lies: small = grazing).  The distance to a convex solid is convex along a ray: the smallest of
    `samples` samples brackets its minimum, a golden-section search refines it, and where that is inside the solid a bisection between
    `near` and it finds the first sign change, to well under 1e-12."""
    n = o.shape[0]
    f = lambda t: signed_distance(kind, size, o + t[:, None] * d)
    ts = np.linspace(near, far, samples)
    vals = signed_distance(kind, size, o[:, None, :] + ts[None, :, None] * d[:, None, :])
    k = np.argmin(vals, axis=1)
    a, b = ts[np.maximum(k - 1, 0)], ts[np.minimum(k + 1, samples - 1)]
    phi = (np.sqrt(5.0) - 1) / 2
    for _ in range(90):
        c, e = b - phi * (b - a), a + phi * (b - a)
        left = f(c) < f(e)
        a, b = np.where(left, a, c), np.where(left, e, b)
    tm = 0.5 * (a + b)
    fm, fn = f(tm), f(np.full(n, float(near)))
    out = np.full(n, np.inf)
    out[fn <= 0] = near                                           # the near plane cuts the solid (or the origin is inside)
    go = (fn > 0) & (fm < 0)
    lo, hi = np.full(n, float(near)), tm.copy()
    for _ in range(70):
        mid = 0.5 * (lo + hi)
        outside = f(mid) > 0
        lo, hi = np.where(outside, mid, lo), np.where(outside, hi, mid)
    out[go] = (0.5 * (lo + hi))[go]
    return out, -np.minimum(fm, fn)


def random_rays(rng, n, half, inside_frac=0.05):
    """Origins in a shell 0.3 .. 3 m around the solid (a few within its bounding box `half`, any direction), directions at a point of
    the box 1.5 x `half`, so that some rays hit and some pass by; unnormalised like the kernel's (|d| in 1 .. 1.6)."""
    half = np.asarray(half, dtype=np.float64)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = v * rng.uniform(0.3, 3.0, (n, 1))
    d = rng.uniform(-1.5, 1.5, (n, 3)) * half - o
    k = int(n * inside_frac)
    o[:k] = rng.uniform(-1.0, 1.0, (k, 3)) * half
    d[:k] = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d * rng.uniform(1.0, 1.6, (n, 1))
