"""Per-env terrains from a device bank and the height scan, on the MI355X: a batch on a bank of terrains with a per-env index against
a batch that holds the same grids as per-env grids (bit for bit) and against the CPU replay of sampled envs; terrain changes made
inside the stream behind phys_batch_end_episodes against a host loop; the scan kernel against the numpy restatement of its definition
(tests/terrain_check.py).  The CPU counterpart -- the same kernels on the wave emulator, the clamp of an index outside the bank
included -- is tests/test_terrain.py.  No test here hands the device an index outside the bank."""
import numpy as np
import pytest

import bench
import golden_physics as G
import oracle_py
import terrain_check as tc
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from test_drive_parity_gpu import FLIP_SAFE_COUNTS, REL_TOL
from test_episodes_gpu import STATE_FIELDS, bank_states, drive_bytes, stress_targets
from test_terrain import RANGE, hfield_case, stairs_case

pytestmark = pytest.mark.gpu


def start_bank(pod, count, seed=40):
    """`count` rough terrains that agree on the flat start patch of config 4's workload (golden_physics.terrain): start states do not
    follow the terrain."""
    out = []
    for k in range(count):
        h = np.random.default_rng(seed + k).random((pod.hfield_nrow, pod.hfield_ncol)).astype(np.float32) * np.float32(0.3 + 0.1 * k)
        h[95:105, 95:105] = 0
        out.append(h)
    return np.stack(out)


def make(model, n, q0, bank=None, index=None, own=None):
    """A fresh batch in CM_DRIVE_PD_SAFE on its terrain(s): a bank + index, or per-env grids through the old call."""
    b = Batch(model, n)
    if bank is not None:
        b.set_hfield_bank(bank)
        b.set_terrain(index)
    if own is not None:
        for e in range(n):
            b.set_hfield(own[e], env=e)
    b.set(P.F_QPOS, q0)
    b.forward()
    b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
    b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
    b.set_drive_mode(P.DRIVE_PD_SAFE)
    return b


def snapshot(b):
    out = {f: b.get(f) for f in (P.F_QPOS, P.F_QVEL, P.F_SENSORDATA)}
    out["warn"], info = b.warnings()
    out["info"] = info[:, :3].copy()
    return out


def test_bank_with_an_index_equals_per_env_grids_and_the_cpu_replay(built):
    """cassie_hfield, CM_DRIVE_PD_SAFE, 50-substep launches on two ranges and two streams: a bank of 8 terrains with a random index
    against the same grids handed in env by env -- qpos, qvel, sensordata, warning words and (ncon, nefc, sweeps) equal bit for bit
    after every policy step; sampled envs against the oracle + host chain on that env's grid within test_drive_parity_gpu's bounds."""
    import torch
    model = Model("cassie_hfield")
    pod, n, npol = model.pod, 2048, 6
    rng = np.random.default_rng(6)
    bank = start_bank(pod, 8)
    index = rng.integers(0, 8, n).astype(np.int32)
    sample = np.unique(np.linspace(0, n - 1, 16).astype(int))
    q0 = np.tile(model.qpos_init(), (n, 1))
    for e in range(n):
        q0[e, 0], q0[e, 1] = G.start_xy("cassie_hfield", e)
    tg_all = np.tile(bench.PD_OFFSET, (npol, n, 1)) + rng.uniform(-0.3, 0.3, (npol, n, 10))
    tg = bench.pd_targets(sample, npol)
    tg_all[:, sample, :] = tg
    refs = []
    for e in sample:
        oracle_py.set_hfield(bank[index[e]])
        r = bench.SafeHostChainEnvs(model, [int(e)])
        r.orcs[0].qpos[:] = q0[e]
        r.orcs[0].forward()
        refs.append(r)
    a = make(model, n, q0, bank=bank, index=index)
    b = make(model, n, q0, own=bank[index])
    try:
        assert a.nterrain == 8 and b.nterrain == 0
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        half = n // 2
        worst = 0.0
        for p in range(npol):
            for x in (a, b):
                x.set(P.F_PD_PTARGET, tg_all[p])
                for (e0, cnt), st in zip([(0, half), (half, n - half)], streams):
                    x.step_range(e0, cnt, 50, st.cuda_stream)
            sa, sb = snapshot(a), snapshot(b)
            for key in sa:
                assert sa[key].tobytes() == sb[key].tobytes(), (p, key)
            for i, e in enumerate(sample):
                oracle_py.set_hfield(bank[index[e]])
                refs[i].step(50, tg[p][i:i + 1])
                qr, cnt = refs[i].qpos()[0], refs[i].counts()[0]
                assert list(sa["info"][e]) == list(cnt), (p, int(e), sa["info"][e], cnt)
                q = sa[P.F_QPOS][e]
                if refs[i].flip_margin[0] > FLIP_SAFE_COUNTS:
                    err = float(np.max(np.abs(q - qr) / np.maximum(1.0, np.abs(qr))))
                    assert err <= REL_TOL, (p, int(e), err)
                    worst = max(worst, err)
                else:
                    assert np.max(np.abs(q - qr)) < 2e-4
        assert not sa["warn"].any()
        assert sa["info"][:, 0].max() >= 2                      # the robots stand on their terrains
        assert len({sa[P.F_QPOS][e].tobytes() for e in range(0, 64, 8)}) > 1
        print("bank of 8 terrains, %d envs x %d policy steps: equal bits with per-env grids; worst rel err of %d replayed envs %.2e" % (n, npol, len(sample), worst))
    finally:
        a.close(); b.close()
        for r in refs:
            for hc in r.chains:
                hc.close()
        oracle_py.set_hfield(None)


def test_terrain_changes_inside_the_stream_equal_a_host_loop(built):
    """A device loop -- two ranges on two streams; behind every end_episodes one torch statement on the range's stream gives the envs
    it restarted their next terrain, nothing synchronises -- against a host loop that synchronises after every policy step, reads
    `done` and sets the terrains one env at a time: every state array, the drive state, the warning words, the terrain index and the
    episode counters equal bit for bit at the end."""
    import torch
    model = Model("cassie_hfield")
    pod, n, npol, k, nt = model.pod, 2048, 8, 4, 8
    bank = start_bank(pod, nt)
    rng = np.random.default_rng(12)
    index0 = rng.integers(0, nt, n).astype(np.int32)
    nxt = rng.integers(0, nt, (npol, n)).astype(np.int32)
    pick = rng.integers(0, k, (npol, n)).astype(np.int32)
    tg = stress_targets(n, npol)
    q0 = np.tile(model.qpos_init(), (n, 1))
    bq, bv = bank_states(model, k)
    rules = dict(min_height=0.8, min_upright=0.7, max_steps=3, warn_mask=P.WARN_DIVERGED, nonfinite=True)
    tgd, pick_d, nxt_d = torch.from_numpy(tg).cuda(), torch.from_numpy(pick).cuda(), torch.from_numpy(nxt).cuda()
    half = n // 2
    ranges = [(0, half), (half, n - half)]

    def final(b, idx):
        out = {f: b.get(f) for f in STATE_FIELDS}
        out["warn"] = b.warnings()[0]
        out["drive"] = drive_bytes(b)
        _, _, out["steps"], out["count"], _ = b.episodes()
        out["index"] = idx
        return out

    def prepare(b):
        b.enable_episodes(**rules)
        b.set_reset_bank(b.make_reset_bank(bq, bv))
        b.sync()

    a = make(model, n, q0, bank=bank, index=index0)
    try:
        prepare(a)
        idx_d = torch.from_numpy(index0.copy()).cuda()
        done_d = torch.zeros(n, dtype=torch.int32, device="cuda")
        a.bind_terrain_index(idx_d.data_ptr())
        a.bind_episode(P.EP_DONE, done_d.data_ptr())
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for p in range(npol):
            a.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
            for (e0, cnt), st in zip(ranges, streams):
                a.step_range(e0, cnt, 50, st.cuda_stream)
                a.end_episodes(e0, cnt, True, pick_ptr=pick_d[p].data_ptr() + 4 * e0, stream=st.cuda_stream)
                with torch.cuda.stream(st):
                    sl = slice(e0, e0 + cnt)
                    idx_d[sl] = torch.where(done_d[sl] != 0, nxt_d[p, sl], idx_d[sl])
        a.sync()
        torch.cuda.synchronize()
        got = final(a, idx_d.cpu().numpy())
    finally:
        a.close()

    b = make(model, n, q0, bank=bank, index=index0)
    try:
        prepare(b)
        index = index0.copy()
        changed = 0
        for p in range(npol):
            b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
            b.step(50)
            b.end_episodes(0, n, True, pick_ptr=pick_d[p].data_ptr())
            b.sync()
            done = b.episodes()[0]
            for e in np.nonzero(done)[0]:
                changed += int(index[e] != nxt[p, e])
                index[e] = nxt[p, e]
                b.set_terrain(np.array([index[e]], dtype=np.int32), env0=int(e))
        want = final(b, index)
    finally:
        b.close()
    for key in want:
        if key == "drive":
            assert got[key] == want[key], key
        else:
            assert got[key].tobytes() == want[key].tobytes(), (key, np.nonzero((got[key] != want[key]).reshape(n, -1).any(axis=1))[0][:16])
    print("%d envs, %d policy steps: %d terrain changes at restarts, episodes per env %s" % (n, npol, changed, np.bincount(want["count"])))
    assert changed > n and want["count"].min() >= 2 and not (want["warn"] & P.WARN_TERRAIN_INDEX).any()


def _device_scan(model, c, offsets, bank=None, index=None):
    """The case on the device: per-env geometry through randomize, the scan on two ranges and two streams, written through a strided
    binding into the middle columns of a wider tensor."""
    import torch
    pod, n, npts = model.pod, c["qpos"].shape[0], offsets.shape[0]
    left, right = 5, 8
    b = Batch(model, n)
    try:
        if bank is not None:
            b.set_hfield_bank(bank)
            b.set_terrain(index)
        b.set(P.F_QPOS, c["qpos"])
        b.randomize(P.P_GEOM_POS, c["gp"].reshape(n, -1))
        b.randomize(P.P_GEOM_QUAT, c["gq"].reshape(n, -1))
        b.configure_scan(offsets, pod.root_body[0], RANGE)
        assert b.dim(P.F_HEIGHT_SCAN) == npts
        obs = torch.full((n, left + npts + right), -3.25, dtype=torch.float64, device="cuda")
        b.bind(P.F_HEIGHT_SCAN, obs.data_ptr() + 8 * left, row_stride=left + npts + right)
        b.sync()
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        half = n // 2
        for (e0, cnt), st in zip([(0, half), (half, n - half)], streams):
            b.height_scan(e0, cnt, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        o = obs.cpu().numpy()
        assert np.all(o[:, :left] == -3.25) and np.all(o[:, left + npts:] == -3.25)
        assert np.array_equal(b.get(P.F_HEIGHT_SCAN), o[:, left:left + npts])
        return o[:, left:left + npts].copy(), b.warnings()[0]
    finally:
        b.close()


def test_scan_on_the_device_4096_envs_height_field(built):
    hf = Model("cassie_hfield")
    c = hfield_case(hf, 4096, seed=21, nbank=8)
    offsets = tc.grid_pattern()
    got, warn = _device_scan(hf, c, offsets, c["bank"], c["index"])
    want, near, tilted = tc.scan(hf.pod, c["qpos"], offsets, RANGE, c["gp"], c["gq"], c["bank"][c["index"]])
    tc.compare(got, want, near)
    assert not warn.any() and not tilted.any()
    assert 0.3 < (np.abs(got) < RANGE).mean() < 0.95


def test_scan_on_the_device_4096_envs_stairs(cassie):
    c = stairs_case(cassie, 4096, seed=22)
    offsets = tc.grid_pattern()
    got, warn = _device_scan(cassie, c, offsets)
    want, near, _ = tc.scan(cassie.pod, c["qpos"], offsets, RANGE, c["gp"], c["gq"])
    tc.compare(got, want, near)
    assert not warn.any()


def test_python_layer_rejects_wrong_sizes(built):
    hf = Model("cassie_hfield")
    b = Batch(hf, 8)
    try:
        n = hf.pod.hfield_nrow * hf.pod.hfield_ncol
        with pytest.raises(ValueError):
            b.set_hfield_bank(np.zeros(n + 1, dtype=np.float32))
        with pytest.raises(ValueError):
            b.set_terrain(np.zeros(8, dtype=np.int32))          # no bank yet
        b.set_hfield_bank(np.zeros((3, n), dtype=np.float32))
        with pytest.raises(ValueError):
            b.set_terrain(np.array([0, 3], dtype=np.int32))     # outside the bank: refused on the host, never sent
        with pytest.raises(ValueError):
            b.set_terrain(np.zeros(9, dtype=np.int32))
        with pytest.raises(ValueError):
            b.configure_scan(np.zeros((1025, 2)), hf.pod.root_body[0], 1.0)
        with pytest.raises(ValueError):
            b.configure_scan(np.zeros((4, 2)), hf.pod.root_body[0] + 1, 1.0)   # not a child of the world
        with pytest.raises(RuntimeError):
            b.height_scan()                                      # not configured
        b.set_hfield(np.zeros(n, dtype=np.float32))
        assert b.nterrain == 0
    finally:
        b.close()
