"""Range sensors on any body on the MI355X: cassie_rays_kernel against the numpy restatement of its definition (tests/rays_check.py, the
bounds and the cap of tests/test_rays.py: ranges depth_check.TOL, normals NORMAL_TOL, fewer than 1 % of the rays masked), against the wave
emulator on the same case, queued behind stepping launches with nothing synchronised, on a bank of height fields, and what a batch
that never asks, or asks again, keeps.  256 envs and 96 rays: more jobs than one workgroup, a block of rays that is half empty, and
two env ranges.

Largest differences seen off the mask, device against restatement (ranges / normal components): cassie 9.3e-15 m / 7.4e-14,
cassie_tray_box 3.6e-15 m / 6.9e-14, cassie_hfield 2.2e-15 m / 4.4e-16, behind three step launches 1.4e-15 m / 3.7e-14; device against
emulator 4.0e-15 m / 1.2e-14.  No id differs; at most 0.04 % of a case's rays are masked.  (NORMAL_TOL, 6.6e-13, was fixed from the
emulator's differences before the device was run: tests/test_rays.py.)"""
import numpy as np
import pytest

import bench
import depth_check as dc
import depth_scene_check as sc
import rays_cases as cs
import rays_check as rc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from test_episodes_gpu import make
from test_rays import (BODY, DIRECTION, MASK, NORMAL_TOL, NRAYS, RMAX, RMIN, SIZE, compare, nominal_poses)
from test_rays import definition_result  # noqa: F401  (the module-scoped fixture: CPU case 1, its restatement and the emulator's answer)
from test_terrain import stairs_case

pytestmark = pytest.mark.gpu

NENV = 256
LEFT, RIGHT, FILL = 3, 6, -3.25


def _device_cast(model, c, table, mask, forward, bank=None):
    """The case on the device: per-env geometry through randomize; body poses from Batch.forward() on the uploaded qpos (forward=True)
    or uploaded as the case has them; the cast on two ranges and two streams, the ranges written through a strided binding into the
    middle columns of a wider tensor, ids and normals into bound tensors -> (ranges, ids, normals, warning words, xpos, xquat as the
    device holds them)."""
    import torch
    n, N = c["qpos"].shape[0], table.size
    b = Batch(model, n)
    try:
        b.set(P.F_QPOS, c["qpos"])
        b.randomize(P.P_GEOM_POS, c["gp"].reshape(n, -1))
        b.randomize(P.P_GEOM_QUAT, c["gq"].reshape(n, -1))
        if bank is not None:
            b.set_hfield_bank(bank)
            b.set_terrain(c["index"])
        if forward:
            b.forward()
            b.sync()
            b.clear_warnings()          # (the forward pass's own: drawn hinges may fill its contact and row buffers)
        else:
            b.set(P.F_XPOS, c["xpos"])
            b.set(P.F_XQUAT, c["xquat"])
        b.configure_rays(table, RMIN, RMAX)
        assert b.dim(P.F_RAYS) == N and b.ray_geoms(mask) == mask
        obs = torch.full((n, LEFT + N + RIGHT), FILL, dtype=torch.float64, device="cuda")
        b.bind(P.F_RAYS, obs.data_ptr() + 8 * LEFT, row_stride=LEFT + N + RIGHT)
        ids = torch.full((n, N), -9, dtype=torch.int32, device="cuda")
        normals = torch.full((n, N, 3), 7.5, dtype=torch.float64, device="cuda")
        b.bind_ray_ids(ids.data_ptr())
        b.bind_ray_normals(normals.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        half = n // 2
        for (e0, cnt), st in zip([(0, half), (half, n - half)], streams):
            b.cast_rays(e0, cnt, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        assert b.ray_launches() == 2
        o = obs.cpu().numpy()
        assert np.all(o[:, :LEFT] == FILL) and np.all(o[:, LEFT + N:] == FILL)
        assert np.array_equal(b.get(P.F_RAYS), o[:, LEFT:LEFT + N])
        return o[:, LEFT:LEFT + N].copy(), ids.cpu().numpy(), normals.cpu().numpy(), b.warnings()[0], b.get(P.F_XPOS), b.get(P.F_XQUAT)
    finally:
        b.close()


# ------------------------------------------------------------------ 1. the device against the definition ----
@pytest.mark.parametrize("name", ["cassie", "cassie_tray_box"])
def test_the_device_against_the_definition_256_envs(built, name):
    model = Model(name)
    pod = model.pod
    c = cs.robot_case(model, NENV, 5, stairs=stairs_case if name == "cassie" else None)
    table = cs.aimed_table(pod, *nominal_poses(model), NRAYS, 5)
    every = sc.all_mask(pod)
    got, ids, normals, warn, xpos, xquat = _device_cast(model, c, table, every, forward=True)
    assert np.abs(xpos.reshape(NENV, -1, 3)[:, pod.root_body[0]] - c["qpos"][:, 0:3]).max() < 1e-12       # the forward pass ran on this qpos
    want = rc.cast(pod, table, RMIN, RMAX, every, xpos, xquat, c["gp"], c["gq"])
    for k in ("mask", "id_mask", "normal_mask"):
        dc.check_mask(want[k])
    hit = want["ids"][want["ids"] >= 0]
    assert {(pod.geom_type[g], bool(sc.is_moving(pod, g))) for g in np.unique(hit)} == {(pod.geom_type[g], bool(sc.is_moving(pod, g))) for g in range(pod.ngeom)}
    compare(got, ids, normals, want, "%s, device" % name)
    assert not warn.any()


# ------------------------------------------------------------------ 2. the device against the emulator ----
def test_the_device_equals_the_emulator(definition_result):
    """Case 1 of tests/test_rays.py with the body poses the emulator's forward pass gave it: within the bounds, not bit for bit (the
    device contracts FMAs where the emulator's build does not)."""
    c = definition_result
    want = c["want"]
    e_got, e_ids, e_normals, _ = c["got"]
    got, ids, normals, warn, _, _ = _device_cast(Model(c["name"]), c, c["table"], c["every"], forward=False)
    dc.compare(got, e_got, want["mask"], "device against emulator, ranges")
    sc.compare_ids(ids, e_ids, want["id_mask"], "device against emulator, ids")
    rc.compare_normals(normals, e_normals, want["normal_mask"], NORMAL_TOL, "device against emulator, normals")
    assert not warn.any()


# ------------------------------------------------------------------ 3. nothing synchronised ----
def test_the_cast_follows_the_step_launches_with_nothing_synchronised(cassie):
    """Three policy steps of step_range(..., 50), then cast_rays with all geoms, on one stream with no synchronisation between them: the
    result is that of the xpos and xquat the launches in front of it left, and equals a cast after a full synchronisation."""
    import torch
    pod, n = cassie.pod, NENV
    rng = np.random.default_rng(23)
    qpos = np.tile(cassie.qpos_init(), (n, 1))
    qpos[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    yaw = rng.uniform(-np.pi, np.pi, n)
    qpos[:, 3:7] = np.stack([np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)], axis=-1)
    table = cs.aimed_table(pod, *nominal_poses(cassie), NRAYS, 7)
    tg = bench.pd_targets(np.arange(n), 3)
    b = make(cassie, n, P.DRIVE_PD_SAFE, qpos=qpos)
    try:
        b.configure_rays(table, RMIN, RMAX)
        every = b.ray_geoms(sc.all_mask(pod))
        ids_d = torch.full((n, NRAYS), -9, dtype=torch.int32, device="cuda")
        nrm_d = torch.full((n, NRAYS, 3), 7.5, dtype=torch.float64, device="cuda")
        b.bind_ray_ids(ids_d.data_ptr())
        b.bind_ray_normals(nrm_d.data_ptr())
        tg_d = torch.from_numpy(tg).cuda()
        ptarget = torch.zeros((n, 10), dtype=torch.float64, device="cuda")
        b.bind(P.F_PD_PTARGET, ptarget.data_ptr())
        b.sync()
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for p in range(3):
                ptarget.copy_(tg_d[p])
                b.step_range(0, n, 50, st.cuda_stream)
            b.cast_rays(0, n, stream=st.cuda_stream)
        torch.cuda.synchronize()
        xpos, xquat, got = b.get(P.F_XPOS), b.get(P.F_XQUAT), b.get(P.F_RAYS)
        ids, normals = ids_d.cpu().numpy(), nrm_d.cpu().numpy()
        assert np.abs(b.get(P.F_QPOS) - qpos).max() > 1e-3                     # the envs have moved on
        want = rc.cast(pod, table, RMIN, RMAX, every, xpos, xquat)
        dc.check_mask(want["mask"])
        compare(got, ids, normals, want, "behind three step launches")
        assert (want["ids"] >= 0).mean() > 0.3 and np.isin(want["ids"], [g for g in range(pod.ngeom) if sc.is_moving(pod, g)]).any()
        b.cast_rays()
        b.sync()
        torch.cuda.synchronize()
        assert b.get(P.F_RAYS).tobytes() == got.tobytes() and ids_d.cpu().numpy().tobytes() == ids.tobytes() and nrm_d.cpu().numpy().tobytes() == normals.tobytes()
        assert not b.warnings()[0].any()
    finally:
        b.close()


# ------------------------------------------------------------------ 4. the height field with a bank ----
def test_height_field_with_a_bank_256_envs(built):
    hf = Model("cassie_hfield")
    pod = hf.pod
    c = cs.hfield_case(hf, NENV, seed=2)
    table = cs.foot_probe_table(pod)
    every = sc.all_mask(pod)
    got, ids, normals, warn, xpos, xquat = _device_cast(hf, c, table, every, forward=True, bank=c["bank"])
    want = rc.cast(pod, table, RMIN, RMAX, every, xpos, xquat, c["gp"], c["gq"], c["bank"][c["index"]])
    for k in ("mask", "id_mask", "normal_mask"):
        dc.check_mask(want[k])
    on_field = want["ids"] == pod.hfield_geom
    assert on_field.mean() > 0.3 and len(np.unique(np.round(want["normals"][on_field], 9), axis=0)) > 100
    compare(got, ids, normals, want, "cassie_hfield, device")
    assert not warn.any()
    # an index outside the bank is clamped and flagged
    import torch
    b = Batch(hf, 8)
    try:
        b.set(P.F_QPOS, c["qpos"][:8])
        b.set_hfield_bank(c["bank"])
        b.forward()
        b.sync()
        b.clear_warnings()
        b.configure_rays(table, RMIN, RMAX)
        bad = torch.tensor([0, 1, 2, 3, -1, 1, 2, 0], dtype=torch.int32, device="cuda")
        b.bind_terrain_index(bad.data_ptr())
        b.cast_rays()
        b.sync()
        flagged = b.get(P.F_RAYS)
        w = b.warnings()[0]
        assert list(np.nonzero(w)[0]) == [3, 4] and np.all(w[[3, 4]] == P.WARN_TERRAIN_INDEX)
        bad.copy_(torch.tensor([0, 1, 2, 2, 0, 1, 2, 0], dtype=torch.int32))
        b.cast_rays()
        b.sync()
        assert b.get(P.F_RAYS).tobytes() == flagged.tobytes()
    finally:
        b.close()


# ------------------------------------------------------------------ 5. nothing changes for a batch that does not ask ----
def test_a_batch_that_never_configures_rays_runs_as_before(cassie):
    import torch
    pod, n = cassie.pod, 64
    rng = np.random.default_rng(3)
    qpos = np.tile(cassie.qpos_init(), (n, 1))
    qpos[:, 0:2] = rng.uniform(-1, 1, (n, 2))
    ctrl = rng.uniform(-1, 1, (n, pod.nu))
    table = cs.foot_probe_table(pod)
    out = []
    for ask in (False, True):
        b = Batch(cassie, n)
        try:
            b.set(P.F_QPOS, qpos)
            b.set(P.F_CTRL, ctrl)
            if not ask:
                assert b.dim(P.F_RAYS) == 0 and b.ray_launches() == 0
                with pytest.raises(RuntimeError, match="phys_batch_rays_configure"):
                    b.get(P.F_RAYS)
                t = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
                with pytest.raises(RuntimeError, match="configure the rays first"):
                    b.bind(P.F_RAYS, t.data_ptr())
                for call in (b.cast_rays, lambda: b.bind_ray_ids(t.data_ptr()), lambda: b.bind_ray_normals(t.data_ptr())):
                    with pytest.raises(RuntimeError, match="phys_batch_rays_configure first"):
                        call()
                with pytest.raises(ValueError, match="phys_batch_rays_configure first"):
                    b.ray_geoms()
            else:
                b.configure_rays(table, RMIN, RMAX)
                b.ray_geoms(sc.all_mask(pod))
            for _ in range(10):
                b.step(1)
                if ask:
                    b.cast_rays()
            b.sync()
            out.append(b.get(P.F_QPOS))
            if ask:
                assert b.ray_launches() == 10 and (b.get(P.F_RAYS) < RMAX).any()
        finally:
            b.close()
    assert out[0].tobytes() == out[1].tobytes() and np.abs(out[0] - qpos).max() > 1e-6


# ------------------------------------------------------------------ 6. lifetime ----
def test_reconfiguring_drops_the_callers_tensors(cassie):
    """Another table while a caller's tensors are bound: the bindings are dropped, the batch's own buffer of the new size is back, and
    the old tensors see no further write."""
    import torch
    pod, n = cassie.pod, 32
    sizes = (12, 20)
    tables = [cs.foot_probe_table(pod, nfan=k // 2, nprobe=k - k // 2) for k in sizes]

    def wide(dim):
        return torch.full((n, LEFT + dim + RIGHT), FILL, dtype=torch.float64, device="cuda")

    first, second = wide(sizes[0]), wide(sizes[1])
    ids0 = torch.full((n, sizes[0]), -9, dtype=torch.int32, device="cuda")
    nrm0 = torch.full((n, sizes[0], 3), 7.5, dtype=torch.float64, device="cuda")
    b = Batch(cassie, n)
    try:
        qpos = np.tile(cassie.qpos_init(), (n, 1))
        qpos[:, 2] = 1.3
        b.set(P.F_QPOS, qpos)
        b.forward()
        b.configure_rays(tables[0], RMIN, RMAX)
        b.bind(P.F_RAYS, first.data_ptr() + 8 * LEFT, row_stride=LEFT + sizes[0] + RIGHT)
        b.bind_ray_ids(ids0.data_ptr())
        b.bind_ray_normals(nrm0.data_ptr())
        b.configure_rays(tables[1], RMIN, RMAX)
        assert b.device_ptr(P.F_RAYS) not in (None, first.data_ptr() + 8 * LEFT) and b.dim(P.F_RAYS) == sizes[1]
        b.cast_rays()
        b.sync()
        torch.cuda.synchronize()
        own = b.get(P.F_RAYS)
        assert own.shape == (n, sizes[1]) and (own < RMAX).any()
        assert bool((first == FILL).all()) and bool((ids0 == -9).all()) and bool((nrm0 == 7.5).all())       # no use of the old pointers
        b.bind(P.F_RAYS, second.data_ptr() + 8 * LEFT, row_stride=LEFT + sizes[1] + RIGHT)
        b.cast_rays()
        b.sync()
        torch.cuda.synchronize()
        s = second.cpu().numpy()
        assert np.array_equal(s[:, LEFT:LEFT + sizes[1]], own) and np.all(s[:, :LEFT] == FILL) and np.all(s[:, LEFT + sizes[1]:] == FILL)
    finally:
        b.close()
    torch.cuda.synchronize()
    assert bool((first == FILL).all()) and np.array_equal(second.cpu().numpy(), s)      # the caller's tensors outlive the batch


# ------------------------------------------------------------------ 7. the launcher's refusals ----
def test_the_launcher_refuses_with_the_shared_messages(cassie):
    pod = cassie.pod
    ok = (1, P.RAY_BODY, [0, 0, 0], [0, 0, -1])
    b = Batch(cassie, 4)
    try:
        for rays, rmin, rmax, message in (([], 0.0, 1.0, SIZE), ([ok] * 1025, 0.0, 1.0, SIZE), ([ok], 1.0, 1.0, SIZE),
                                          ([(pod.nbody, P.RAY_BODY, [0, 0, 0], [0, 0, -1])], 0.0, 1.0, BODY),
                                          ([(1, P.RAY_BODY, [0, 0, 0], [0, 0, 0])], 0.0, 1.0, DIRECTION),
                                          ([(1, P.RAY_BODY, [0, 0, 0], [np.nan, 0, 1])], 0.0, 1.0, DIRECTION)):
            with pytest.raises(ValueError) as err:
                b.configure_rays(rays, rmin, rmax)
            assert str(err.value).endswith("phys_batch_rays_configure: " + message)
        assert b.dim(P.F_RAYS) == 0
        b.configure_rays(np.array([ok[:2] + (ok[2], ok[3])], dtype=P.RAY_DTYPE), 0.0, 1.0)          # a structured array
        assert b.dim(P.F_RAYS) == 1 and b.ray_geoms() == sc.default_mask(pod)
        with pytest.raises(ValueError) as err:
            b.ray_geoms(1 << pod.ngeom)
        assert str(err.value).endswith("phys_batch_rays_set_geoms: " + MASK)
    finally:
        b.close()
