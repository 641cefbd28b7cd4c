"""The bank of full states on the GPU (phys_batch_state_save / _restore, include/cassie_phys.h: "a bank of full states"): after a
restore an env continues byte for byte as the saved env did.  "Equal" below is tobytes() equality over EVERY env of every CORE section --
time, qpos, qvel, warm start, ctrl, qacc, sensordata, actuator_velocity, the measurement block, the bytes of cm_drive_state_t
(safety_msg included), xpos, xquat and the warning words (states_check.snapshot / assert_equal).  64 envs or fewer, a few step(50)
launches, bench.pd_targets; batches as in test_episodes_gpu.  The CPU counterparts: tests/test_states_launch.py, tests/test_states_emu.py."""
import numpy as np
import pytest

import bench
import golden_physics as G
import states_check as sc
import states_emu_py as se
from cassie_amd import Batch, Model
from cassie_amd import phys as P
from cassie_amd.distributed import ObservationBlock
from test_episodes_gpu import make, stress_targets
from test_terrain_gpu import start_bank

pytestmark = pytest.mark.gpu

N = 64
FORK_SRC = 5
FORK_DST = np.array([0, 3, 4, 9, 17, 31, 32, 40, 51, 62, 63])      # a scattered set of 11 envs


def policy_steps(b, tg, first, last):
    for p in range(first, last):
        b.set(P.F_PD_PTARGET, tg[p])
        b.step(50)


def device_slots(slots):
    import torch
    return torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int32)).cuda()


def make_on_terrain(model, n, nbank=0, index=None):
    """cassie_hfield in DRIVE_PD_SAFE on the flat start patch of rough terrain: one shared grid, or a bank with an index."""
    pod = model.pod
    q0 = np.tile(model.qpos_init(), (n, 1))
    for e in range(n):
        q0[e, 0], q0[e, 1] = G.start_xy("cassie_hfield", e)
    grids = start_bank(pod, max(nbank, 1))
    b = Batch(model, n)
    if nbank:
        b.set_hfield_bank(grids)
        b.set_terrain(index)
    else:
        b.set_hfield(grids[0])
    b.set(P.F_QPOS, q0)
    b.forward()
    b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
    b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
    b.set_drive_mode(P.DRIVE_PD_SAFE)
    return b


def make_model_batch(name, model, n):
    return make_on_terrain(model, n) if name == "cassie_hfield" else make(model, n, P.DRIVE_PD_SAFE)


def rewind(b, tg, before=2, window=2, left_fast=None):
    """`before` policy steps, a save to a device permutation of the slots, `window` more steps (recorded), a restore, the same steps again.
    left_fast: a list that collects, per recorded step, how many envs left the fast code, and the warning words."""
    perm = np.random.default_rng(17).permutation(b.nenv).astype(np.int32)
    slots_d = device_slots(perm)
    policy_steps(b, tg, 0, before)
    b.save_states(slots_ptr=slots_d.data_ptr())
    at_save = sc.snapshot(b)
    for p in range(before, before + window):
        policy_steps(b, tg, p, p + 1)
        if left_fast is not None:
            left_fast.append((int((b.fast_rows_progress() < 50).sum()), b.wide_pass_envs(), b.warnings()[0].copy()))
    record = sc.snapshot(b)
    assert record["qpos"].tobytes() != at_save["qpos"].tobytes()
    b.restore_states(slots_ptr=slots_d.data_ptr())
    sc.assert_equal(sc.snapshot(b), at_save, "right after the restore")
    policy_steps(b, tg, before, before + window)
    sc.assert_equal(sc.snapshot(b), record, "after the replayed steps")
    return perm, at_save


def test_rewind(cassie):
    """a. cassie, 64 envs, DRIVE_PD_SAFE: right after the restore every CORE section is what it was at the save, after the same two
    policy steps what the first pass recorded.  The saved rows are the numpy restatement's and the emulator's for the same inputs."""
    b = make(cassie, N, P.DRIVE_PD_SAFE)
    try:
        b.configure_states(N)
        lay, row_dim = b.state_layout(), b.state_row_dim()
        assert (lay, row_dim) == se.layout(cassie.pod, P.STATE_CORE) and b.state_signature() == se.signature(cassie.pod, P.STATE_CORE)
        perm, at_save = rewind(b, bench.pd_targets(np.arange(N), 4))
        rows, sig = b.states()
        assert rows.dtype == np.int64 and rows.shape == (N, row_dim) and sig == b.state_signature()
        for e in range(N):
            assert rows[perm[e]].tobytes() == sc.row(lay, row_dim, at_save, e).tobytes(), e
        emu_bank = np.zeros_like(rows)
        se.call(cassie.pod, at_save, emu_bank, False, slots=perm)
        assert emu_bank.tobytes() == rows.tobytes()
    finally:
        b.close()


@pytest.mark.parametrize("name", ["cassie", "cassie_hfield"])
def test_rewind_through_the_tiers(cassie, name):
    """b. The same with the +-10 rad stress targets: in the recorded window envs leave the fast code (the row-capped kernel hands them
    to the 63-row pass, and that to the 127-row pass) and none diverges -- asserted on the recorded run itself.  Whatever word a
    launch leaves per env beside the CORE list and a later launch reads would show here.

    The window, chosen on the MI355X from a run of these targets over 30 policy steps (1024 envs; an env's run does not depend on the
    batch around it): under the safety layer the robots take 15 policy steps to fall far enough for more than 31 rows, no env of the
    first 64 diverges within 30 steps, and the fast kernel hands over env-launches of these 64 envs in steps 16, 19 and 20 on cassie
    (1, 2, 1 envs) and 16, 17, 18 on cassie_hfield (1, 4, 3).  So: 16 steps, the save, steps 16 .. 19 recorded and replayed."""
    model = cassie if name == "cassie" else Model(name)
    b = make_model_batch(name, model, N)
    try:
        b.configure_states(N)
        seen = []
        forms0 = b.form_launches()
        rewind(b, stress_targets(N, 20), before=16, window=4, left_fast=seen)
        left = sum(s[0] for s in seen)
        forms1 = b.form_launches()
        print("%s: envs that left the fast code per recorded step %s, to the 127-row pass %s, fast-form launches %s -> %s" %
              (name, [s[0] for s in seen], [s[1] for s in seen], forms0, forms1))
        assert left > 0 or any(s[1] > 0 for s in seen) or forms1[1] > forms0[1]
        assert not any((s[2] & P.WARN_DIVERGED).any() for s in seen)
    finally:
        b.close()


def test_fork(cassie):
    """c. Env 5 saved to slot 0 and slot 0 restored into 11 scattered envs, slot -1 for everybody else: the others are byte-equal to a
    twin batch that never made the calls; after two policy steps with env 5's targets the 11 envs equal env 5, section by section;
    rewound once more and given their own targets they do not."""
    tg = bench.pd_targets(np.arange(N), 4)
    a, twin = make(cassie, N, P.DRIVE_PD_SAFE), make(cassie, N, P.DRIVE_PD_SAFE)
    try:
        a.configure_states(2)
        for x in (a, twin):
            policy_steps(x, tg, 0, 2)
        save = np.full(N, -1, dtype=np.int32)
        save[FORK_SRC] = 0
        take = np.full(N, -1, dtype=np.int32)
        take[FORK_DST] = 0
        save_d, take_d = device_slots(save), device_slots(take)
        a.save_states(slots_ptr=save_d.data_ptr())
        a.restore_states(slots_ptr=take_d.data_ptr())
        others = np.setdiff1d(np.arange(N), FORK_DST)
        got, want = sc.snapshot(a), sc.snapshot(twin)
        sc.assert_equal(got, want, "envs outside the fork", envs=others)
        for sect in got:
            assert got[sect][FORK_DST].tobytes() == np.repeat(want[sect][FORK_SRC][None], len(FORK_DST), axis=0).tobytes(), sect
        forked = tg.copy()
        forked[:, FORK_DST] = tg[:, FORK_SRC][:, None]
        policy_steps(a, forked, 2, 4)
        policy_steps(twin, tg, 2, 4)
        got, want = sc.snapshot(a), sc.snapshot(twin)
        sc.assert_equal(got, want, "envs outside the fork, two steps on", envs=others)
        for sect in got:
            assert got[sect][FORK_DST].tobytes() == np.repeat(want[sect][FORK_SRC][None], len(FORK_DST), axis=0).tobytes(), sect
        take[FORK_SRC] = 0                                   # once more from the fork point, env 5 included, each with its own targets
        a.restore_states(slots=take)
        policy_steps(a, tg, 2, 4)
        got = sc.snapshot(a)
        assert got["qpos"][FORK_SRC].tobytes() == want["qpos"][FORK_SRC].tobytes()
        assert all(got["qpos"][e].tobytes() != got["qpos"][FORK_SRC].tobytes() for e in FORK_DST)
    finally:
        a.close(); twin.close()


@pytest.mark.parametrize("name", ["cassie", "cassie_hfield", "cassie_tray_box"])
def test_all_models_with_the_episode_group(cassie, name):
    """d. Rewind on every model (cassie_tray_box: the cube's free joint is part of qpos / qvel; cassie_hfield: a bank of 4 terrains and an
    index) with STATE_EPISODE: EP_STEPS, EP_COUNT and the terrain index come back with the state; an env restored onto an env of
    another terrain index takes the source's terrain and continues equal to it."""
    import torch
    model = cassie if name == "cassie" else Model(name)
    n, nbank = 32, 4 if name == "cassie_hfield" else 0
    index = (np.arange(n) % 4).astype(np.int32)
    b = make_on_terrain(model, n, nbank, index) if nbank else make(model, n, P.DRIVE_PD_SAFE)
    try:
        tg = bench.pd_targets(np.arange(n), 5)
        if name == "cassie_tray_box":
            assert model.pod.nq > cassie.pod.nq
        index_d = None
        if nbank:
            index_d = torch.from_numpy(index).cuda()
            b.bind_terrain_index(index_d.data_ptr())
        b.enable_episodes(max_steps=3)                      # (steps count up, the third call ends every episode: count moves too)
        b.configure_states(n + 1, P.STATE_CORE | P.STATE_EPISODE)
        lay = b.state_layout()
        assert {"ep_steps", "ep_count", "terrain"} <= set(lay)

        def step_and_count(p):
            policy_steps(b, tg, p, p + 1)
            b.end_episodes(restart=False)

        def episode_words():
            _, _, steps, count, _ = b.episodes()
            return steps.copy(), count.copy(), None if index_d is None else index_d.cpu().numpy().copy()

        for p in range(3):
            step_and_count(p)
        b.save_states()
        at_save, ep_save = sc.snapshot(b), episode_words()
        assert ep_save[0].tolist() == [3] * n and ep_save[1].tolist() == [1] * n
        rows, _ = b.states(0, n)
        off = lay["terrain"][0]
        assert rows[:, off].tolist() == (index.tolist() if nbank else [0] * n)
        assert rows[:, lay["ep_steps"][0]].tolist() == [3] * n and rows[:, lay["ep_count"][0]].tolist() == [1] * n
        step_and_count(3)
        record, ep_record = sc.snapshot(b), episode_words()
        if nbank:
            index_d[:] = 3 - index_d                          # everybody elsewhere meanwhile
            torch.cuda.synchronize()
        b.restore_states()
        sc.assert_equal(sc.snapshot(b), at_save, "right after the restore")
        ep_now = episode_words()
        assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(ep_now, ep_save))
        step_and_count(3)
        sc.assert_equal(sc.snapshot(b), record, "after the replayed step")
        assert all(x is None or x.tobytes() == y.tobytes() for x, y in zip(episode_words(), ep_record))
        # env 1 (terrain 1) onto env 2 (terrain 2), from the saved state: env 2 stands on terrain 1 and follows env 1
        take = np.full(n, -1, dtype=np.int32)
        take[1], take[2] = 1, 1
        b.restore_states(slots=take)
        b.sync()
        if nbank:
            assert index_d.cpu().numpy()[[1, 2]].tolist() == [1, 1]
        tg2 = tg.copy()
        tg2[:, 2] = tg[:, 1]
        policy_steps(b, tg2, 3, 5)
        got = sc.snapshot(b)
        for sect in got:
            assert got[sect][2].tobytes() == got[sect][1].tobytes(), sect
        assert got["qpos"][3].tobytes() != got["qpos"][1].tobytes()
    finally:
        b.close()


def test_params_group(cassie):
    """e. Masses and friction randomised per env.  A fork with STATE_PARAMS carries the source's parameter block: the copy continues
    equal to the source.  Without the group the copy keeps its own physics: it differs from the source and equals a twin batch into
    whose env the source's CORE sections were copied through get / set on the host."""
    n, src, dst = 16, 3, 12
    tg = bench.pd_targets(np.arange(n), 4)
    tg[:, dst] = tg[:, src]
    pod = cassie.pod

    def randomised():
        b = make(cassie, n, P.DRIVE_PD_SAFE)
        blk = b.params(0, 1)[0]
        mass = np.ctypeslib.as_array(blk.body_mass)[:pod.nbody].copy()
        fric = np.ctypeslib.as_array(blk.geom_friction)[:pod.ngeom].copy().reshape(-1)
        r = np.random.default_rng(9)
        b.randomize(P.P_BODY_MASS, mass * r.uniform(0.8, 1.25, (n, pod.nbody)))
        b.randomize(P.P_GEOM_FRICTION, fric * r.uniform(0.5, 1.2, (n, fric.size)))
        b.set_const()
        return b

    plain = make(cassie, 2, P.DRIVE_PD_SAFE)
    try:
        with pytest.raises(ValueError, match="PHYS_STATE_PARAMS needs per-env parameter blocks"):
            plain.configure_states(1, P.STATE_PARAMS)
    finally:
        plain.close()
    a, c, twin = randomised(), randomised(), randomised()
    try:
        a.configure_states(n, P.STATE_CORE | P.STATE_PARAMS)
        c.configure_states(n)
        assert "params" in a.state_layout() and "params" not in c.state_layout()
        for x in (a, c, twin):
            policy_steps(x, tg, 0, 2)
        take = np.full(n, -1, dtype=np.int32)
        take[dst] = src
        for x in (a, c):
            x.save_states()
            x.restore_states(slots=take)
        # the host-side copy of the CORE sections into the twin's env
        for sect in sc.CORE:
            if sect in sc.FIELD_OF:
                arr = twin.get(sc.FIELD_OF[sect])
                arr[dst] = arr[src]
                twin.set(sc.FIELD_OF[sect], arr)
        ds = twin.get_drive_state()
        ds[dst] = ds[src]
        twin.set_drive_state(ds)
        assert not twin.warnings()[0].any()
        pa, pc = sc.snapshot(a, ("params",))["params"], sc.snapshot(c, ("params",))["params"]
        assert pa[dst].tobytes() == pa[src].tobytes() and pc[dst].tobytes() != pc[src].tobytes()
        for x in (a, c, twin):
            policy_steps(x, tg, 2, 4)
        ga, gc_, gt = sc.snapshot(a), sc.snapshot(c), sc.snapshot(twin)
        for sect in ga:
            assert ga[sect][dst].tobytes() == ga[sect][src].tobytes(), sect
        assert gc_["qpos"][dst].tobytes() != gc_["qpos"][src].tobytes()
        sc.assert_equal(gc_, gt, "without STATE_PARAMS: the destination's own physics")
    finally:
        a.close(); c.close(); twin.close()


def test_poses_come_back(cassie):
    """f. After a restore and NO step, the range sensors (ranges, hit ids, normals) and the depth image with the moving geoms (depths,
    hit ids) are what they were at the save: xpos / xquat are part of a row."""
    import torch
    n = 16
    pod = cassie.pod
    tg = bench.pd_targets(np.arange(n), 4)
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    try:
        pelvis = pod.root_body[0]
        w, h = 24, 16
        # 1.5 m in front of the pelvis, looking back at the robot (the camera looks along its -z, +y up: z_cam = body x, y_cam = body z)
        b.configure_depth(pelvis, [1.5, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5], w, h, 60.0, 0.05, 5.0)
        b.depth_geoms(moving=True)
        depth_ids = torch.full((n, w * h), -9, dtype=torch.int32, device="cuda")
        b.bind_depth_ids(depth_ids.data_ptr())
        rays = [(body, P.RAY_BODY, [0.0, 0.0, 0.0], d) for body in range(1, pod.nbody) for d in ([0.0, 0.0, -1.0], [1.0, 0.0, 0.0])]
        b.configure_rays(rays, 0.0, 4.0)
        b.ray_geoms(b.depth_all_geoms())
        ray_ids = torch.full((n, len(rays)), -9, dtype=torch.int32, device="cuda")
        normals = torch.full((n, len(rays), 3), 7.5, dtype=torch.float64, device="cuda")
        b.bind_ray_ids(ray_ids.data_ptr())
        b.bind_ray_normals(normals.data_ptr())
        b.configure_states(n)

        def look():
            b.cast_rays()
            b.depth_image()
            b.sync()
            return [b.get(P.F_RAYS).tobytes(), ray_ids.cpu().numpy().tobytes(), normals.cpu().numpy().tobytes(),
                    b.get(P.F_DEPTH).tobytes(), depth_ids.cpu().numpy().tobytes()]

        policy_steps(b, tg, 0, 2)
        b.save_states()
        at_save = look()
        assert (ray_ids.cpu().numpy() >= 0).any() and (depth_ids.cpu().numpy() >= 0).any()
        policy_steps(b, tg, 2, 4)
        moved = look()
        assert moved[0] != at_save[0] and moved[3] != at_save[3]
        b.restore_states()
        assert look() == at_save
    finally:
        b.close()


def test_two_ranges_on_two_streams(cassie):
    """g. Two env ranges on two streams, device slots, no host read between the save, the steps and the restore: the result equals
    the one-stream run of the whole batch."""
    import torch
    tg = bench.pd_targets(np.arange(N), 4)
    tgd = torch.from_numpy(tg).cuda()
    perm = np.random.default_rng(23).permutation(N).astype(np.int32)
    slots_d = device_slots(perm)
    half = N // 2
    ranges = [(0, half), (half, N - half)]

    def run(streams):
        b = make(cassie, N, P.DRIVE_PD_SAFE)
        try:
            b.configure_states(N)
            b.sync()
            torch.cuda.synchronize()
            lanes = [(e0, cnt, st.cuda_stream) for (e0, cnt), st in zip(ranges, streams)] if streams else [(0, N, None)]
            for first, last, call in ((0, 2, b.save_states), (2, 4, b.restore_states), (2, 3, None)):
                for p in range(first, last):
                    b.bind(P.F_PD_PTARGET, tgd[p].data_ptr())
                    for e0, cnt, st in lanes:
                        b.step_range(e0, cnt, 50, st)
                for e0, cnt, st in lanes:
                    if call:
                        call(env0=e0, n=cnt, slots_ptr=slots_d.data_ptr() + 4 * e0, stream=st)
            b.sync()
            torch.cuda.synchronize()
            return sc.snapshot(b), b.states()[0]
        finally:
            b.close()

    one, rows_one = run(None)
    two, rows_two = run([torch.cuda.Stream(), torch.cuda.Stream()])
    sc.assert_equal(two, one, "two streams against one")
    assert rows_two.tobytes() == rows_one.tobytes()


def test_bound_and_strided(cassie):
    """h. qpos | qvel | sensordata bound as the columns of an ObservationBlock and the bank bound to a torch int64 tensor: the rewind
    holds, the tensor's rows are states(), and they are the rows a batch with dense fields and its own bank saves."""
    import torch
    tg = bench.pd_targets(np.arange(N), 4)
    a, d = make(cassie, N, P.DRIVE_PD_SAFE), make(cassie, N, P.DRIVE_PD_SAFE)
    try:
        init = torch.from_numpy(np.concatenate([a.get(P.F_QPOS)[0], a.get(P.F_QVEL)[0], a.get(P.F_SENSORDATA)[0]]))
        obs = ObservationBlock(a, cassie.pod, torch.device("cuda", 0), init)
        a.configure_states(1)
        bank_d = torch.full((N, a.state_row_dim()), -1, dtype=torch.int64, device="cuda")
        assert bank_d.data_ptr() % 16 == 0
        a.bind_states(bank_d.data_ptr(), N)
        assert a.state_ptr() == bank_d.data_ptr()
        d.configure_states(N)
        perm, at_save = rewind(a, tg)
        rewind(d, tg)
        assert bank_d.cpu().numpy().tobytes() == a.states()[0].tobytes() == d.states()[0].tobytes()
        got = sc.snapshot(a)
        assert obs.tensor.cpu().numpy().tobytes() == np.concatenate([got["qpos"], got["qvel"], got["sensordata"]], axis=1).tobytes()
        a.bind_states(None, 0)                               # the batch's own bank again: one slot
        assert a.states()[0].shape[0] == 1
    finally:
        a.close(); d.close()


def test_across_batches(cassie):
    """i. states() of one batch, set_states() into a fresh batch of the same model, restore: it continues equal to the first.  Rows with
    the signature of another model or of another group set are refused, with the message; a slot outside the bank raises
    WARN_STATE_SLOT and leaves the env alone; the calls' own refusals."""
    tg = bench.pd_targets(np.arange(N), 4)
    a, b = make(cassie, N, P.DRIVE_PD_SAFE), make(cassie, N, P.DRIVE_PD_SAFE)
    try:
        with pytest.raises(RuntimeError, match="phys_batch_state_save: not configured"):
            a.save_states()
        with pytest.raises(ValueError, match="at least one slot"):
            a.configure_states(0)
        with pytest.raises(ValueError, match="PHYS_STATE_EPISODE needs the episode arrays"):
            a.configure_states(4, P.STATE_EPISODE)
        with pytest.raises(ValueError, match="restored into nothing"):
            a.configure_states(4, P.STATE_COMMANDS)
        a.configure_states(N)
        b.configure_states(N)
        with pytest.raises(RuntimeError, match="phys_batch_state_restore: env range out of bounds"):
            a.restore_states(env0=N - 1, n=2)
        policy_steps(a, tg, 0, 2)
        a.save_states()
        rows, sig = a.states()
        policy_steps(a, tg, 2, 4)
        want = sc.snapshot(a)
        b.set_states(rows, signature=sig)
        b.restore_states()
        policy_steps(b, tg, 2, 4)
        sc.assert_equal(sc.snapshot(b), want, "the fresh batch")
        # foreign rows
        other = Model("cassie_tray_box")
        with pytest.raises(ValueError, match="the rows' signature is not this batch's"):
            b.set_states(rows, signature=se.signature(other.pod, P.STATE_CORE))
        with pytest.raises(ValueError, match="the rows' signature is not this batch's"):
            b.set_states(rows, signature=se.signature(cassie.pod, P.STATE_CORE | P.STATE_EPISODE))
        # slots outside the bank, in both directions
        before = sc.snapshot(b)
        bank_before = b.states()[0]
        slots = np.arange(N, dtype=np.int32)
        slots[[7, 40]] = [N, 1 << 20]
        b.save_states(slots=slots)
        b.restore_states(slots=slots)
        after = sc.snapshot(b)
        want_warn = before["warn"].copy()
        want_warn[[7, 40]] |= P.WARN_STATE_SLOT
        assert after["warn"].tobytes() == want_warn.tobytes()
        sc.assert_equal({k: v for k, v in after.items() if k != "warn"}, {k: v for k, v in before.items() if k != "warn"}, "envs with a slot outside the bank")
        assert b.states()[0][[7, 40]].tobytes() == bank_before[[7, 40]].tobytes()
    finally:
        a.close(); b.close()
