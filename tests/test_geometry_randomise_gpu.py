"""Per-env geometry and springs on the GPU through the C ABI: phys_batch_randomize of CM_P_GEOM_POS / CM_P_GEOM_QUAT /
CM_P_JNT_STIFFNESS / CM_P_QPOS_SPRING, together with the five other parameters and phys_batch_set_const, against (a) the host model
compiler -- the blocks bit for bit -- and (b) the oracle stepping each env's own compiled model.  Writing the model's own values
must leave trajectories bit for bit those of an unrandomised batch in every form of the step kernel."""
import numpy as np
import pytest

import bench
import geometry_randomise_check as gc
import randomise_check as rc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from oracle_py import Oracle

pytestmark = pytest.mark.gpu
N = 4096


def _stairs_tilt_springs(pod, n, seed):
    """Per env: one stair box under the robot at its own height / offset, the floor tilted up to 3 degrees about a random
    horizontal axis, every spring's stiffness x U(0.8, 1.2) -- with the five other parameters randomised too."""
    rng = np.random.default_rng(seed)
    params = gc.own_params(pod, n)
    gp = params["geom_pos"].reshape(n, pod.ngeom, 3)
    gq = params["geom_quat"].reshape(n, pod.ngeom, 4)
    box = 1 + np.arange(n) % 15
    gp[np.arange(n), box] = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-1.03, -0.97, n)], 1)
    ang = np.radians(rng.uniform(0, 3, n)) / 2
    phi = rng.uniform(0, 2 * np.pi, n)
    gq[:, 0] = np.stack([np.cos(ang), np.sin(ang) * np.cos(phi), np.sin(ang) * np.sin(phi), np.zeros(n)], 1)
    params["geom_pos"], params["geom_quat"] = gp.reshape(n, -1), gq.reshape(n, -1)
    params["jnt_stiffness"] = params["jnt_stiffness"] * rng.uniform(0.8, 1.2, params["jnt_stiffness"].shape)
    params.update(rc.random_params(Model("cassie"), n, seed=seed + 1))
    return params


def _randomised_batch(model, params, n, torch_fields=()):
    b = Batch(model, n)
    keep = []
    for f, pid in gc.ALL_IDS.items():
        if f in torch_fields:
            import torch
            t = torch.from_numpy(np.ascontiguousarray(params[f])).to("cuda:0")
            torch.cuda.synchronize()
            keep.append(t)
            b.randomize(pid, None, device_ptr=t.data_ptr(), n=n)
        else:
            b.randomize(pid, params[f])
    b.set_const()
    b.sync()
    return b


def test_blocks_after_randomize_equal_the_host_compile(built):
    """512 envs: geometry / spring rows (two through a torch device pointer, two from host arrays) and no set_const -- the
    derived records follow the rows at once; then set_const re-derives them to the same bits."""
    name, n = "cassie", 512
    model = Model(name)
    pod = model.pod
    params = gc.own_params(pod, n)
    params.update(gc.random_geometry(pod, n, seed=23))
    import torch
    b = Batch(model, n)
    try:
        keep = []
        for f in gc.GEO_INPUTS:
            if f in ("geom_pos", "jnt_stiffness"):
                t = torch.from_numpy(np.ascontiguousarray(params[f])).to("cuda:0")
                torch.cuda.synchronize()
                keep.append(t)
                b.randomize(gc.GEO_IDS[f], None, device_ptr=t.data_ptr(), n=n)
            else:
                b.randomize(gc.GEO_IDS[f], params[f])
        b.sync()
        blocks = b.params()
        hosts = gc.HostGeomEnvModels(name)
        for e in range(0, n, 8):
            gc.assert_geo_equal(blocks[e], hosts.pod(params, e, set_const=False), pod, "env %d" % e)
        b.set_const()
        b.sync()
        again = b.params()
        for e in range(0, n, 64):
            gc.assert_geo_equal(again[e], hosts.pod(params, e), pod, "env %d after set_const" % e)
    finally:
        b.close()


def test_all_4096_envs_own_stairs_tilt_and_springs_follow_the_oracle(built):
    """Every env its own stair layout, floor tilt and spring stiffness, with the five other fields + set_const; one launch of 50
    substeps; every env against the oracle on its own compiled model: counts equal, qpos to rounding."""
    name, nsub = "cassie", 50
    model = Model(name)
    params = _stairs_tilt_springs(model.pod, N, seed=41)
    b = _randomised_batch(model, params, N, torch_fields=("geom_quat", "body_mass"))
    try:
        q0 = model.qpos_init()
        rng = np.random.default_rng(6)
        hi = np.array([model.pod.act_ctrlrange[u][1] for u in range(model.pod.nu)])
        ctrl = 0.5 * hi * rng.uniform(-1, 1, (N, model.pod.nu))
        b.set(P.F_QPOS, np.tile(q0, (N, 1)))
        b.set(P.F_CTRL, ctrl)
        b.step(nsub)
        q = b.get(P.F_QPOS)
        w, info = b.warnings()
        assert not w.any()
        hosts = gc.HostGeomEnvModels(name)
        worst, box_envs = 0.0, 0
        for e in range(N):
            o = Oracle(hosts.pod(params, e), q0)
            o.ctrl[:] = ctrl[e]
            o.step(nsub)
            assert (info[e, 0], info[e, 1], info[e, 2]) == (o.d.ncon, o.d.nefc, o.d.solver_iter), (e, info[e].tolist(), (o.d.ncon, o.d.nefc, o.d.solver_iter))
            worst = max(worst, float(np.max(np.abs(q[e] - o.qpos))))
            box_envs += any(1 <= o.d.contact[i].geom1 <= 15 or 1 <= o.d.contact[i].geom2 <= 15 for i in range(o.d.ncon))
        print("4096 envs with their own stairs / tilt / springs x %d steps: worst |qpos - oracle| %.2e, %d envs on their box" % (nsub, worst, box_envs))
        assert worst < 1e-10
        assert box_envs > N // 4
    finally:
        b.close()


def test_benchmarked_mode_two_ranges_on_two_streams_1000_steps(built):
    """CM_DRIVE_PD_SAFE, the batch stepped as two env ranges on two streams, 1000 steps in 50-substep launches; 64 sampled envs
    replayed through oracle (their own models) + host chain + safety block, compared at every policy step."""
    import torch
    name, nsteps = "cassie", 1000
    model = Model(name)
    params = _stairs_tilt_springs(model.pod, N, seed=57)
    b = _randomised_batch(model, params, N)
    sample = np.unique(np.linspace(0, N - 1, 64).astype(int))
    hosts = gc.HostGeomEnvModels(name)
    pods = [hosts.pod(params, int(e)) for e in sample]
    npol = nsteps // bench.HOLD
    tg = bench.pd_targets(sample, npol)
    rng = np.random.default_rng(78)
    tg_all = np.tile(bench.PD_OFFSET, (npol, N, 1)) + rng.uniform(-0.3, 0.3, (npol, N, 10))
    tg_all[:, sample, :] = tg
    ref = bench.SafeHostChainEnvs(model, sample, None, pods=pods)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    half = N // 2
    try:
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (N, 1)))
        b.forward()
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (N, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (N, 1)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        b.sync()
        worst = 0.0
        for p in range(npol):
            b.set(P.F_PD_PTARGET, tg_all[p])
            b.sync()
            for k, st in enumerate(streams):
                b.step_range(k * half, half, bench.HOLD, st.cuda_stream)
            for st in streams:
                st.synchronize()
            ref.step(bench.HOLD, tg[p])
            q = b.get(P.F_QPOS)[sample]
            w, info = b.warnings()
            qr, cnt = ref.qpos(), ref.counts()
            assert np.array_equal(info[sample][:, :3], cnt), (p, info[sample][:4].tolist(), cnt[:4].tolist())
            err = np.max(np.abs(q - qr) / np.maximum(1.0, np.abs(qr)), axis=1)
            safe = ref.flip_margin > 1e-6
            assert np.all(err[safe] <= 1e-9), (p, float(err[safe].max()))
            assert np.all(np.max(np.abs(q - qr), axis=1)[~safe] < 2e-4)
            worst = max(worst, float(err[safe].max()) if safe.any() else 0.0)
        assert not w.any()
        print("geometry-randomised drive-pd-safe on two streams: worst rel err %.2e over 64 envs x %d policy steps" % (worst, npol))
    finally:
        b.close()
        for hc in ref.chains:
            hc.close()


def _stress_rollout(name, n, params, inplace, flags=0):
    """Stress targets (every joint slammed into its limit: envs leave the 31-row tier), the given form of the fast kernel; params =
    None: an unrandomised batch.  Returns state, outputs, warnings and counts."""
    import test_drive_parity_gpu as D
    model = Model(name)
    for bit in (P.FLAG_HFPRISM,):
        if flags & bit:
            model.set_flag(bit, True)
    hf = None
    if name == "cassie_hfield":
        hf = np.random.default_rng(99).random((200, 200)).astype(np.float32)
        hf[95:105, 95:105] = 0
    b = Batch(model, n)
    try:
        if hf is not None:
            b.set_hfield(hf)
        if params is not None:
            for f in gc.GEO_INPUTS:
                b.randomize(gc.GEO_IDS[f], params[f])
        b.set_inplace(inplace)
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set_drive_mode(P.DRIVE_PD)
        tg = D._stress_targets(np.arange(n), 12)
        rows = 0
        for p in range(12):
            b.set(P.F_PD_PTARGET, tg[p])
            b.step((bench.HOLD, 20, 11)[p % 3])
            rows = max(rows, int(b.warnings()[1][:, 1].max()))
        w, info = b.warnings()
        return [b.get(P.F_QPOS), b.get(P.F_QVEL), b.get(P.F_QACC_WARMSTART), b.get(P.F_SENSORDATA), b.get(P.F_MEAS), w, info[:, :3].copy()], rows
    finally:
        b.close()


@pytest.mark.parametrize("name,flags,inplace,min_rows", [("cassie", 0, 0, 32), ("cassie", 0, 1, 32),
                                                         ("cassie_hfield", P.FLAG_HFPRISM, 2, 64)])
def test_the_models_own_geometry_and_springs_change_no_bit(built, name, flags, inplace, min_rows):
    """The plain and the in-place form of the fast kernel, and (height field with CM_FLAG_HFPRISM) the 127-row instantiation: a
    batch whose blocks hold the model's own geometry / springs -- read from the blocks -- steps to the bits of an unrandomised one."""
    n = 4096
    pod = Model(name).pod
    a, rows = _stress_rollout(name, n, None, inplace, flags)
    b, _ = _stress_rollout(name, n, gc.own_params(pod, n), inplace, flags)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert rows >= min_rows, rows


def test_device_pointer_without_n_is_a_value_error(built):
    model = Model("cassie")
    b = Batch(model, 4)
    try:
        with pytest.raises(ValueError):
            b.randomize(P.P_GEOM_POS, None, device_ptr=1, n=None)
    finally:
        b.close()
