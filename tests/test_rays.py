"""Range sensors on any body on the CPU: the device's ray kernel (csrc/ray_kernel.h: cassie_rays_kernel) executed by the wave emulator,
configured, checked and launched through csrc/small_launch.h as the launcher does it, against the numpy restatement of the definition
in tests/rays_check.py -- itself pinned by brute force on the solids' signed distance functions (the values) and by finite differences
of them (the normals).  The GPU counterpart is tests/test_rays_gpu.py.

Bounds.  Ranges: depth_check.TOL (1e-11 m) off the mask, the bound the depth tests hold on this geometry.  Ids: equal off the id mask.
Normals: NORMAL_TOL = 6.6e-13 per component off the normal mask = ten times the largest difference between emulator and restatement
seen on the cases of this file and of tests/test_rays_gpu.py (the same cases at 256 envs, run on the emulator), 6.6e-14: 8 envs cassie
9.7e-15, cassie_tray_box 2.1e-14, cassie_hfield 2.3e-16; 256 envs cassie 5.1e-14, cassie_tray_box 6.6e-14, cassie_hfield 3.4e-16.  (The
hit point of a ray of up to 4 m carries a few 1e-15 m of rounding, over a radius of 0.02 m on the toe capsule.)  The factor is for the
device's FMA contraction.  Fewer than 1 % of the rays of any case may be masked: asserted from the restatement alone, before a kernel
result is looked at (no ray of cases 1 and 2 is masked for the values; at 256 envs the id and normal masks hold 0.04 % of cassie's rays).
The finite-difference pin of the normals holds 1e-6: a central difference of step h = 1e-6 m on a surface whose smallest radius of
curvature is r = 0.02 m (the toe capsule) is off by about (h / r)^2 = 2.5e-9, and by the rounding of the distance over h, 1e-16 / 1e-6;
box hits within 1e-5 m of an edge, where the difference straddles two faces, are left out of that pin."""
import numpy as np
import pytest

import depth_check as dc
import depth_scene_check as sc
import emu_py
import rays_cases as cs
import rays_check as rc
import rays_emu_py as re_
import terrain_check as tc
from cassie_amd import Model
from cassie_amd import phys as P
from test_depth_scene import emu_forward
from test_terrain import _blocks, stairs_case

NORMAL_TOL = 6.6e-13
NENV = 8
RMIN, RMAX, NRAYS = cs.RMIN, cs.RMAX, cs.NRAYS
SIZE = "1 .. 1024 rays and 0 <= rmin < rmax"
BODY = "a ray's body must lie in [0, nbody)"
DIRECTION = "a ray needs a finite origin and a finite direction that is not zero"
FRAME = "a ray's frame is PHYS_RAY_BODY, PHYS_RAY_WORLD_DIR or PHYS_RAY_HEADING"
MASK = "the mask names a geom at or above ngeom"


def nominal_poses(model):
    x0, q0 = emu_forward(model.pod, np.tile(model.qpos_init(), (1, 1)))
    return x0.reshape(-1, 3), q0.reshape(-1, 4)


def definition_case(name, nenv, seed=5):
    """Case 1: 96 rays over nine bodies (the world among them) in the three frames, every geom in the mask, body poses from the
    emulator's forward pass, per-env geometry -> the case and the restatement's answer."""
    model = Model(name)
    pod = model.pod
    c = cs.robot_case(model, nenv, seed, stairs=stairs_case if name == "cassie" else None)
    c["xpos"], c["xquat"] = emu_forward(pod, c["qpos"])
    c["table"] = cs.aimed_table(pod, *nominal_poses(model), NRAYS, seed)
    c["every"] = sc.all_mask(pod)
    c["want"] = rc.cast(pod, c["table"], RMIN, RMAX, c["every"], c["xpos"], c["xquat"], c["gp"], c["gq"])
    for k in ("mask", "id_mask", "normal_mask"):
        dc.check_mask(c["want"][k])
    return c


def compare(got, ids, normals, want, what, tol=NORMAL_TOL):
    dc.compare(got, want["val"], want["mask"], what + ", ranges")
    sc.compare_ids(ids, want["ids"], want["id_mask"], what + ", ids")
    return rc.compare_normals(normals, want["normals"], want["normal_mask"], tol, what + ", normals")


@pytest.fixture(scope="module", params=["cassie", "cassie_tray_box"])
def definition_result(built, request):
    c = definition_case(request.param, NENV)
    c["name"] = request.param
    c["blocks"] = _blocks(c["pod"], c["gp"], c["gq"])
    c["got"] = re_.cast(c["pod"], c["table"], RMIN, RMAX, c["xpos"], c["xquat"], mask=c["every"], blocks=c["blocks"])
    return c


# ------------------------------------------------------------------ 1. the definition on the emulator ----
def test_ranges_ids_and_normals_match_the_definition(definition_result):
    c = definition_result
    pod, want = c["pod"], c["want"]
    got, ids, normals, warn = c["got"]
    assert len(set(c["table"]["body"])) >= 6 and 0 in c["table"]["body"] and set(c["table"]["frame"]) == {rc.BODY, rc.WORLD_DIR, rc.HEADING}
    hit = want["ids"][want["ids"] >= 0]
    seen = {(pod.geom_type[g], bool(sc.is_moving(pod, g))) for g in np.unique(hit)}
    every_kind = {(pod.geom_type[g], bool(sc.is_moving(pod, g))) for g in range(pod.ngeom)}
    print("kinds hit (type, moving): %s; %.1f %% miss, %d at rmin" % (sorted(seen), 100 * (want["ids"] < 0).mean(), (want["val"] == RMIN).sum()))
    assert seen == every_kind and (want["ids"] < 0).any() and (want["val"] == RMIN).any()
    compare(got, ids, normals, want, "%s, emulator" % c["name"])
    assert not warn.any()
    # unit normals against the ray on a hit from outside, zero on a miss and from inside a solid
    length = np.linalg.norm(normals, axis=2)
    inside = (got == RMIN) & (ids >= 0)
    assert np.all(length[(ids < 0) | inside] == 0.0) and np.max(np.abs(length[(ids >= 0) & ~inside] - 1.0)) < 1e-14
    assert np.all(np.einsum("enk,enk->en", normals, want["u"]) <= 0.0)
    assert np.all((ids == -1) == (got == RMAX))
    # env 2's capsules have a pose of their own in its block: the kernel reads it
    gp0, gq0 = tc.model_geom_poses(pod, NENV)
    plain, _, _, _ = re_.cast(pod, c["table"], RMIN, RMAX, c["xpos"], c["xquat"], mask=c["every"], blocks=_blocks(pod, gp0, gq0))
    assert (plain[2] != got[2]).any()


def test_a_range_through_a_small_grid_leaves_the_other_rows_alone(definition_result):
    c = definition_result
    got, ids, normals, _ = c["got"]
    part, part_ids, part_n = np.full_like(got, -7.0), np.full_like(ids, -7), np.full_like(normals, -7.0)
    re_.cast(c["pod"], c["table"], RMIN, RMAX, c["xpos"], c["xquat"], mask=c["every"], blocks=c["blocks"], env0=2, n=5, grid=3, out=part, ids=part_ids,
             normals=part_n)
    for a, b in ((part, got), (part_ids, ids), (part_n, normals)):
        assert np.array_equal(a[2:7], b[2:7]) and np.all(a[:2] == -7) and np.all(a[7:] == -7)
    # values alone: no ids, no normals bound
    alone, none_ids, none_n, _ = re_.cast(c["pod"], c["table"], RMIN, RMAX, c["xpos"], c["xquat"], mask=c["every"], blocks=c["blocks"], want_ids=False,
                                          want_normals=False)
    assert none_ids is None and none_n is None and alone.tobytes() == got.tobytes()


def test_the_default_mask_is_the_depth_images_and_a_mask_hides_its_geoms(definition_result):
    c = definition_result
    pod = c["pod"]
    assert re_.check(pod, c["table"], RMIN, RMAX)[2] == sc.default_mask(pod) == emu_py.depth_geoms(pod)
    got, ids, _, _ = re_.cast(pod, c["table"], RMIN, RMAX, c["xpos"], c["xquat"], blocks=c["blocks"])
    static = [g for g, _ in tc.static_geoms(pod)]
    assert set(np.unique(ids)) <= set(static) | {-1}
    want = rc.cast(pod, c["table"], RMIN, RMAX, sc.default_mask(pod), c["xpos"], c["xquat"], c["gp"], c["gq"])
    dc.compare(got, want["val"], want["mask"], "default mask, emulator")


def test_nan_body_poses_blind_the_ray_and_hide_the_geoms(definition_result):
    c = definition_result
    pod = c["pod"]
    body = int(cs.feet(pod)[0])
    for field in ("xpos", "xquat"):
        bad = {k: c[k].copy().reshape(NENV, pod.nbody, -1) for k in ("xpos", "xquat")}
        bad[field][1, body] = np.nan
        xp, xq = bad["xpos"].reshape(NENV, -1), bad["xquat"].reshape(NENV, -1)
        got, ids, normals, warn = re_.cast(pod, c["table"], RMIN, RMAX, xp, xq, mask=c["every"], blocks=c["blocks"])
        want = rc.cast(pod, c["table"], RMIN, RMAX, c["every"], xp, xq, c["gp"], c["gq"])
        compare(got, ids, normals, want, "NaN %s, emulator" % field)
        own = c["table"]["body"] == body
        assert own.any() and np.all(got[1, own] == RMAX) and np.all(ids[1, own] == -1) and np.all(normals[1, own] == 0.0)
        assert not np.isin(ids[1], [g for g in range(pod.ngeom) if pod.geom_bodyid[g] == body]).any()
        assert np.array_equal(np.delete(got, 1, axis=0), np.delete(c["got"][0], 1, axis=0))


# ------------------------------------------------------------------ 2. the height field ----
@pytest.fixture(scope="module")
def hfield_result(built):
    hf = Model("cassie_hfield")
    pod = hf.pod
    c = cs.hfield_case(hf, NENV, seed=2)
    c["xpos"], c["xquat"] = emu_forward(pod, c["qpos"])
    c["table"] = cs.foot_probe_table(pod)
    c["every"] = sc.all_mask(pod)
    c["want"] = rc.cast(pod, c["table"], RMIN, RMAX, c["every"], c["xpos"], c["xquat"], c["gp"], c["gq"], c["bank"][c["index"]])
    for k in ("mask", "id_mask", "normal_mask"):
        dc.check_mask(c["want"][k])
    c["kw"] = dict(mask=c["every"], blocks=_blocks(pod, c["gp"], c["gq"]), hfield=c["bank"].reshape(-1), stride=pod.hfield_nrow * pod.hfield_ncol,
                   nterrain=len(c["bank"]))
    c["got"] = re_.cast(pod, c["table"], RMIN, RMAX, c["xpos"], c["xquat"], index=c["index"], **c["kw"])
    return c


def test_height_field_values_and_triangle_normals(hfield_result):
    c = hfield_result
    pod, want = c["pod"], c["want"]
    got, ids, normals, warn = c["got"]
    on_field = want["ids"] == pod.hfield_geom
    tilted = np.abs(tc.quat2mat(c["gq"][:, pod.hfield_geom])[:, 2, 2] - 1.0) > 1e-6
    assert tilted[0::2].all() and not tilted[1::2].any() and set(c["index"]) == {0, 1, 2}
    assert on_field.mean() > 0.3 and on_field[tilted].any() and on_field[~tilted].any() and (want["ids"] < 0).any()
    probes = c["table"]["frame"] == rc.WORLD_DIR
    assert on_field[:, probes].any() and on_field[:, ~probes].any()
    assert len(np.unique(np.round(want["normals"][on_field], 9), axis=0)) > 20          # (many triangles, not one slope)
    compare(got, ids, normals, want, "cassie_hfield, emulator")
    assert not warn.any()


def test_index_outside_the_bank_is_clamped_and_flagged(hfield_result):
    c = hfield_result
    bad = c["index"].copy()
    bad[[0, 5]] = [-1, len(c["bank"])]
    got, ids, normals, warn = re_.cast(c["pod"], c["table"], RMIN, RMAX, c["xpos"], c["xquat"], index=bad, **c["kw"])
    want = re_.cast(c["pod"], c["table"], RMIN, RMAX, c["xpos"], c["xquat"], index=np.clip(bad, 0, len(c["bank"]) - 1), **c["kw"])
    assert list(np.nonzero(warn)[0]) == [0, 5] and np.all(warn[[0, 5]] == P.WARN_TERRAIN_INDEX) and not want[3].any()
    assert got.tobytes() == want[0].tobytes() and normals.tobytes() == want[2].tobytes() and ids.tobytes() == want[1].tobytes()


# ------------------------------------------------------------------ 3. self-exclusion ----
def test_a_ray_reads_through_its_own_body_and_not_through_another(cassie):
    pod = cassie.pod
    rmin = 0.005                                                          # (inside the toe capsule, whose radius is 0.02)
    foot = int(cs.feet(pod)[0])
    toe = [g for g in range(pod.ngeom) if pod.geom_bodyid[g] == foot][0]
    pelvis = int(pod.root_body[0])
    assert pod.geom_type[toe] == sc.CAPSULE
    qpos = np.tile(cassie.qpos_init(), (1, 1))
    qpos[0, 2] = 1.5                                                      # (the feet half a metre over the floor)
    xpos, xquat = emu_forward(pod, qpos)
    xp, xq = xpos.reshape(-1, 3), xquat.reshape(-1, 4)
    lp = np.array(list(pod.geom_pos[toe]))
    centre = xp[foot] + tc.quat2mat(xq[foot]) @ lp                        # the middle of the toe capsule, in the world
    R1 = tc.quat2mat(xq[pelvis])
    table = rc.table_of([(foot, rc.WORLD_DIR, lp, [0, 0, -1]),           # from inside its own body's capsule
                         (pelvis, rc.BODY, R1.T @ (centre - xp[pelvis]), R1.T @ np.array([0.0, 0.0, -1.0]))])   # the same ray on another body
    got, ids, normals, _ = re_.cast(pod, table, rmin, RMAX, xpos, xquat, mask=sc.all_mask(pod))
    floor = [g for g, t in tc.static_geoms(pod) if t == tc.PLANE][0]
    assert ids[0, 0] == floor and abs(got[0, 0] - (centre[2] - pod.geom_pos[floor][2])) < 1e-12 and np.allclose(normals[0, 0], [0, 0, 1], atol=1e-15)
    assert got[0, 0] > 10 * rmin
    assert got[0, 1] == rmin and ids[0, 1] == toe and np.all(normals[0, 1] == 0.0)
    want = rc.cast(pod, table, rmin, RMAX, sc.all_mask(pod), xpos, xquat)
    assert want["ids"][0].tolist() == [floor, toe] and want["val"][0, 1] == rmin


# ------------------------------------------------------------------ 4. foot probes and the scan's surface ----
def test_a_vertical_probe_reads_the_height_over_the_scans_surface(cassie):
    pod = cassie.pod
    c = cs.robot_case(cassie, NENV, 5, stairs=stairs_case)
    xpos, xquat = emu_forward(pod, c["qpos"])
    rays = [(b, rc.WORLD_DIR, [0.05 * k - 0.1, 0.03 * k - 0.05, 0.0], [0, 0, -1]) for k in range(5) for b in cs.feet(pod) + [int(pod.root_body[0])]]
    table = rc.table_of(rays)
    got, ids, _, _ = re_.cast(pod, table, 1e-3, RMAX, xpos, xquat, blocks=_blocks(pod, c["gp"], c["gq"]))          # the default mask
    o, _ = rc.world_rays(table, xpos, xquat)
    top, hit, _, _ = tc.surface(pod, o[..., 0], o[..., 1], c["gp"], c["gq"], None)
    want = o[..., 2] - top
    ok = hit & (want > 1e-3) & (want < RMAX)
    print("probes over the surface: %d of %d, over boxes %d, largest difference %.3g m" % (ok.sum(), ok.size, (ids[ok] > 0).sum(), np.abs(got - want)[ok].max()))
    assert ok.mean() > 0.8 and (ids[ok] > 0).sum() > 10 and (ids[ok] == 0).sum() > 10
    assert np.abs(got - want)[ok].max() <= dc.TOL


# ------------------------------------------------------------------ 5. brute force ----
def test_values_by_brute_force_and_normals_by_finite_differences(definition_result):
    c = definition_result
    pod, want = c["pod"], c["want"]
    got, ids, normals, _ = c["got"]
    GP, GR = sc.geom_world_poses(pod, c["gp"], c["gq"], c["xpos"], c["xquat"])
    seen = set()
    for kind in sc.SOLIDS:
        pick = np.isin(want["ids"], [g for g in range(pod.ngeom) if pod.geom_type[g] == kind]) & ~want["normal_mask"]
        e, j = np.nonzero(pick)
        if e.size == 0:
            continue
        e, j = e[:60], j[:60]
        g = want["ids"][e, j]
        og = np.einsum("nji,nj->ni", GR[e, g], want["o"][e, j] - GP[e, g])
        dg = np.einsum("nji,nj->ni", GR[e, g], want["u"][e, j])
        worst_t = worst_n = 0.0
        for k in range(e.size):
            size = [pod.geom_size[g[k]][a] for a in range(3)]
            brute, _ = sc.brute_force_solid(kind, size, og[k:k + 1], dg[k:k + 1], RMIN, RMAX, samples=4001)
            worst_t = max(worst_t, abs(brute[0] - want["val"][e[k], j[k]]), abs(brute[0] - got[e[k], j[k]]))
            if want["val"][e[k], j[k]] == RMIN:
                assert np.all(normals[e[k], j[k]] == 0.0)
                continue
            p = og[k:k + 1] + brute[0] * dg[k:k + 1]
            if kind == sc.BOX and (np.abs(np.abs(p[0]) - size) < 1e-5).sum() >= 2:
                continue
            n_fd = GR[e[k], g[k]] @ rc.normal_by_difference(kind, size, p)[0]
            worst_n = max(worst_n, np.abs(n_fd - want["normals"][e[k], j[k]]).max(), np.abs(n_fd - normals[e[k], j[k]]).max())
        print("solid %d: %d rays, brute force within %.3g m, finite-difference normals within %.3g" % (kind, e.size, worst_t, worst_n))
        assert worst_t <= 1e-11 and worst_n <= 1e-6
        seen.add(kind)
    assert seen == {pod.geom_type[g] for g in range(pod.ngeom) if pod.geom_type[g] in sc.SOLIDS}


# ------------------------------------------------------------------ 6. the launch records and the refusals ----
def test_the_grid_and_the_record_of_a_launch(cassie):
    pod = cassie.pod
    assert [re_.grid(n, r) for n, r in ((1, 1), (1, 64), (1, 65), (8, 96), (256, 96), (1024, 96), (1025, 96), (4096, 1024), (3, 1024))] == \
        [1, 1, 2, 16, 512, 2048, 2048, 2048, 48]
    ints, reals = re_.record(pod, 96, 0.03, 4.0, 0x1234, 130, 128, 64, ids=True, normals=False)
    assert ints == dict(env0=128, n=64, nrays=96, sout=130, sxp=3 * pod.nbody, sxq=4 * pod.nbody, geoms=0x1234, ids=1, normals=0, index=0, nterrain=0)
    assert reals == (0.03, 4.0)
    ints, _ = re_.record(pod, 5, 0.0, 1.0, 1, 5, 0, 7, ids=False, normals=True, nterrain=3)
    assert (ints["ids"], ints["normals"], ints["index"], ints["nterrain"], ints["sout"]) == (0, 1, 1, 3, 5)
    # configure normalises the directions and leaves the rest of the table
    table = rc.table_of([(3, rc.HEADING, [0.1, 0.2, 0.3], [0.0, 3.0, -4.0]), (0, rc.BODY, [0, 0, 1], [1e-3, 0, 0])])
    why, out, mask = re_.check(pod, table, 0.0, 2.0)
    assert why is None and mask == sc.default_mask(pod)
    assert np.allclose(out["dir"], [[0.0, 0.6, -0.8], [1.0, 0.0, 0.0]], atol=1e-16) and np.array_equal(out["origin"], table["origin"])
    assert out["body"].tolist() == [3, 0] and out["frame"].tolist() == [rc.HEADING, rc.BODY]


def refusals(pod):
    """Every refused configuration once: (what, rays, rmin, rmax, mask, message)."""
    ok = [(1, rc.BODY, [0, 0, 0], [0, 0, -1])]
    return [
        ("no rays", [], 0.0, 1.0, None, SIZE),
        ("1025 rays", ok * 1025, 0.0, 1.0, None, SIZE),
        ("rmin >= rmax", ok, 1.0, 1.0, None, SIZE),
        ("a negative rmin", ok, -0.1, 1.0, None, SIZE),
        ("a body at nbody", [(pod.nbody, rc.BODY, [0, 0, 0], [0, 0, -1])], 0.0, 1.0, None, BODY),
        ("a negative body", [(-1, rc.BODY, [0, 0, 0], [0, 0, -1])], 0.0, 1.0, None, BODY),
        ("a zero direction", [(1, rc.BODY, [0, 0, 0], [0, 0, 0])], 0.0, 1.0, None, DIRECTION),
        ("a NaN direction", [(1, rc.BODY, [0, 0, 0], [0, np.nan, 1])], 0.0, 1.0, None, DIRECTION),
        ("an infinite origin", [(1, rc.BODY, [np.inf, 0, 0], [0, 0, 1])], 0.0, 1.0, None, DIRECTION),
        ("a frame of 3", [(1, 3, [0, 0, 0], [0, 0, 1])], 0.0, 1.0, None, FRAME),
        ("a mask bit at ngeom", ok, 0.0, 1.0, 1 << pod.ngeom, MASK),
    ]


def test_every_refusal_has_its_message(cassie):
    pod = cassie.pod
    assert pod.ngeom < 32
    for what, rays, rmin, rmax, mask, message in refusals(pod):
        why, _, _ = re_.check(pod, rc.table_of(rays), rmin, rmax, mask)
        assert why == message, what
    assert re_.check(pod, rc.table_of([(0, rc.WORLD_DIR, [0, 0, 1], [0, 0, -2])] * 1024), 0.0, 1.0, sc.all_mask(pod))[0] is None
    # the launch refuses likewise, and says why
    x = np.zeros((1, 3 * pod.nbody))
    with pytest.raises(AssertionError, match="1 .. 1024 rays"):
        re_.cast(pod, rc.table_of([]), 0.0, 1.0, x, np.zeros((1, 4 * pod.nbody)))
