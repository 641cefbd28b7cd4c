"""Normaliser rows (phys_batch_norm_*) on the device against the wave emulator and the definition restated in numpy (tests/norm_check.py),
BIT FOR BIT on every word: the cases tests/test_norm.py runs on the emulator, with the batch's own OBS store, with a bound, padded torch
tensor as the store, and with a caller's tensor as the source.  Also: a live loop that acts and differentiates with the updated words, update
and write back to back on one stream, that a call changes nothing else of the batch, the launch counters, and the refusals that need a
batch."""
import numpy as np
import pytest

import bench
import grad_cases as gcs
import grad_check as gc
import norm_cases as cases
import norm_check as nc
import norm_emu_py as ne
import policy_check as pc
from cassie_amd import phys as P
from test_episodes_gpu import make
from test_grad_gpu import Dev, fence, up

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32
NENV, T, BLOCK = 256, 3, 80              # 768 samples: ten blocks, the last short, every third astride a step
NAMES = ("n", "mean", "m2", "skipped", "excluded", "mb", "counts")


@pytest.fixture(scope="module")
def batch(cassie, built):
    b = make(cassie, NENV, P.DRIVE_PD_SAFE)
    yield b
    b.close()


def snapshot(b, mean_d, inv_d):
    """Every word in norm_cases' form (waits for the streams)."""
    fence(b)
    snap = {k: b.norm_download(i) for i, k in enumerate(NAMES)}
    a12 = b.norm_download(P.NORM_PARTIALS)
    snap.update(a1=a12[0], a2=a12[1], out_mean=mean_d.cpu().numpy(), out_inv=inv_d.cpu().numpy(), stats=b.norm_stats()["all"])
    return snap


@pytest.mark.parametrize("mode", ("own", "bound", "shifted"))
@pytest.mark.parametrize("D", cases.DIMS)
def test_shared_cases_on_the_device(batch, D, mode):
    """Three updates in a row.  own: the batch's own OBS store, filled by rollout_record; bound: a padded torch tensor as the store, NaN in
    the padding; shifted: no rollout at all, a caller's tensor one word behind a 16-byte boundary as the source (the word path on every D)."""
    import torch
    b = batch
    src = cases.Source(D, T, NENV, shift=1 if mode == "shifted" else 0)
    e, r = ne.Norm(D, BLOCK), cases.Ref(D, BLOCK)
    e.bind_source(*src.bind_args(), keep=src)
    mean_d, inv_d = up(np.full(D, ne.FILL, dtype=F32)), up(np.full(D, ne.FILL, dtype=F32))
    b.configure_rollout(T, [] if mode == "shifted" else [("obs", D)])
    b.configure_norm(D, BLOCK, max_rows=T * NENV, eps=cases.EPS)
    b.bind_norm_output(mean_d.data_ptr(), inv_d.data_ptr())
    row_d = torch.zeros((NENV, D), dtype=torch.float32, device="cuda")
    dev = torch.full((len(src.buf) + 4,), float("nan"), dtype=torch.float32, device="cuda")
    if mode == "own":
        b.bind_rollout_source("obs", row_d.data_ptr(), D)
    elif mode == "bound":
        b.bind_rollout_storage("obs", dev.data_ptr(), src.step_stride, src.row_stride)
    else:
        b.bind_norm_source(dev.data_ptr() + 4, T, NENV, src.step_stride, src.row_stride)
    before = b.norm_launches()
    for k, x in enumerate(cases.datasets(D, T, NENV)):
        src.fill(x)
        fence(b)
        if mode == "own":
            for t in range(T):
                row_d.copy_(torch.from_numpy(np.array(x[t])))            # (a writable copy)
                fence(b)
                b.rollout_record(t)
                fence(b)
        else:
            at = 1 if mode == "shifted" else 0
            dev[at: at + len(src.buf)].copy_(torch.from_numpy(src.buf))
            fence(b)
        b.norm_update()
        got = snapshot(b, mean_d, inv_d)
        assert cases.differing(got, r.update(src.dense())) == [], (D, mode, k)
        assert cases.differing(got, e.update()) == [], (D, mode, k)
    assert e.info["vec"] == (D % 4 == 0 and mode != "shifted")
    after = b.norm_launches()
    assert tuple(x - y for x, y in zip(after, before)) == (3, 3, 3, 3, 0)
    b.bind_norm_source(None)
    b.bind_norm_output(None, None)


def test_update_and_write_back_to_back(batch):
    """update, the outputs overwritten, write: all on one stream with no fence; write puts the very words back."""
    import torch
    b, D = batch, 67
    src = cases.Source(D, T, NENV)
    src.fill(cases.datasets(D, T, NENV)[0])
    dev, mean_d, inv_d = up(src.buf), up(np.full(D, ne.FILL, dtype=F32)), up(np.full(D, ne.FILL, dtype=F32))
    b.configure_norm(D, BLOCK, max_rows=T * NENV, eps=cases.EPS)
    b.bind_norm_source(dev.data_ptr(), T, NENV, src.step_stride, src.row_stride)
    b.bind_norm_output(mean_d.data_ptr(), inv_d.data_ptr())
    st = torch.cuda.Stream()
    fence(b)
    before = b.norm_launches()
    b.norm_update(st.cuda_stream)
    with torch.cuda.stream(st):
        mean_d.fill_(7.0)
        inv_d.fill_(7.0)
    b.norm_write(st.cuda_stream)
    fence(b)
    want = cases.Ref(D, BLOCK).update(src.dense())
    dead = np.arange(D) == cases.COL_DEAD
    got_mean, got_inv = mean_d.cpu().numpy(), inv_d.cpu().numpy()
    assert nc.same_bits(got_mean[~dead], want["out_mean"][~dead]) and nc.same_bits(got_inv[~dead], want["out_inv"][~dead])
    assert got_mean[dead] == 7.0 and got_inv[dead] == 7.0                       # (n = 0: write leaves the words alone)
    assert tuple(x - y for x, y in zip(b.norm_launches(), before)) == (1, 1, 1, 1, 1)
    # a checkpoint: everything downloaded, the rows configured anew, uploaded, written
    saved = {what: b.norm_download(what) for what in (P.NORM_N, P.NORM_MEAN, P.NORM_M2, P.NORM_SKIPPED, P.NORM_EXCLUDED)}
    b.configure_norm(D, BLOCK, max_rows=T * NENV, eps=cases.EPS)
    assert not b.norm_download(P.NORM_N).any()
    b.bind_norm_output(mean_d.data_ptr(), inv_d.data_ptr())
    for what, values in saved.items():
        b.norm_upload(what, values)
    mean_d.fill_(0.0)
    inv_d.fill_(0.0)
    fence(b)
    b.norm_write()
    fence(b)
    assert nc.same_bits(mean_d.cpu().numpy()[~dead], want["out_mean"][~dead]) and nc.same_bits(inv_d.cpu().numpy()[~dead], want["out_inv"][~dead])
    assert all(nc.same_bits(b.norm_download(what), v) for what, v in saved.items())
    with pytest.raises(ValueError, match="no such kind"):
        b.norm_upload(P.NORM_MB, np.zeros(D))
    assert b.norm_count(99) == -1 and b.norm_count(P.NORM_PARTIALS) == 0
    b.configure_norm(0, release=True)


def test_a_call_changes_nothing_else(cassie, built):
    """update and write with the rollout's bound OBS store as the source and two tensors of the caller's as the outputs: the states, the
    gradient rows' result, every rollout array, the policy's own normalisation and its packed weights keep every word."""
    case = gcs.shared_case()
    d = Dev(cassie, case, 16)
    try:
        b, p = d.b, case.p
        d.bind()
        b.configure_states(case.nenv, P.STATE_CORE)
        m = 37
        d.grad(case.idx(m))

        def everything_else():
            fence(b)
            b.save_states()
            res = d.result(m)
            own = [d.mean, d.inv] if p.norm is not None else []
            return [b.states()[0].tobytes(), gc.words(res).tobytes(), b.policy_packed().tobytes()] + [d.arr[k].cpu().numpy().tobytes() for k in gcs.KINDS] + \
                [t.cpu().numpy().tobytes() for t in d.dummy + own] + [t.cpu().numpy().tobytes() for per in d.dw + d.db for t in per]

        D = p.in_dim
        mean_d, inv_d = up(np.full(D, ne.FILL, dtype=F32)), up(np.full(D, ne.FILL, dtype=F32))
        b.configure_norm(D, 64, max_rows=case.T * case.nenv, eps=cases.EPS)
        b.bind_norm_output(mean_d.data_ptr(), inv_d.data_ptr())
        before = everything_else()
        b.norm_update()
        b.norm_write()
        assert everything_else() == before
        want = cases.Ref(D, 64).update(case.dense["obs"].reshape(case.T * case.nenv, D))   # (the rows of the padded store)
        assert nc.same_bits(mean_d.cpu().numpy(), want["out_mean"]) and nc.same_bits(inv_d.cpu().numpy(), want["out_inv"])
        assert b.norm_launches() == (1, 1, 1, 1, 1)
    finally:
        d.close()


NOBS, NACT, NPOL, CLIP = 12, 3, 3, 5.0


def test_live_loop_acts_with_the_updated_words(cassie, built):
    """256 envs on cassie.xml, every stage in place for three policy steps: observe, policy, act, step, reward, end_episodes, and
    rollout_record in two ranges on two streams that the caller orders; then norm_update with nothing bound -- the rollout's own OBS store
    into the policy's bound normalisation -- and a policy() call.  mean and inv are the restatement's for the downloaded store, the policy's
    outputs are policy_check's with them, and a grad call behind it keeps as h_0 the rows normalised with the new words."""
    import policy_cases
    import torch
    n, half = NENV, NENV // 2
    rng = np.random.default_rng(37)
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * rng.random(n)
    nets = [policy_cases.dense(rng, (NOBS, 16, NACT), (P.POL_ELU, P.POL_TANH)), policy_cases.dense(rng, (NOBS, 16, 1), (P.POL_TANH, P.POL_IDENTITY))]
    proto = policy_cases.Case("live", nets, np.zeros((n, NOBS), dtype=F32), pad=0, wpad=0)
    eps = np.clip(rng.normal(size=(NPOL + 2, n, NACT)), -4, 4).astype(F32)
    log_std = np.full(NACT, -1.5, dtype=F32)
    b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
    try:
        dev = "cuda"
        b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
        b.enable_episodes(max_steps=3, min_height=0.4)
        b.set_reset_bank(b.make_reset_bank(cassie.qpos_init()[None]))
        obs_d = torch.zeros((n, NOBS + 2), dtype=torch.float32, device=dev)
        act_d = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
        mu_d = torch.zeros((n, NACT + 1), dtype=torch.float32, device=dev)
        val_d = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        logp_d = torch.zeros(n, dtype=torch.float32, device=dev)
        mean0, inv0 = rng.normal(size=NOBS).astype(F32) * F32(0.1), rng.uniform(0.5, 2.0, size=NOBS).astype(F32)
        mean_d, inv_d = up(mean0), up(inv0)
        eps_d, ls_d = torch.from_numpy(eps).cuda(), torch.from_numpy(log_std).cuda()
        b.configure_obs([P.obs_copy(P.F_QPOS, 7, 10, scale=1.0), P.obs_copy(P.F_QVEL, 0, 2, scale=0.1)], history=1, dtype=np.float32)
        b.bind_obs(obs_d.data_ptr(), NOBS + 2)
        b.configure_actions([P.act_col(P.F_PD_PTARGET, j, lo=-1.5, hi=1.5, offset=float(bench.PD_OFFSET[j]), scale=0.2) for j in range(NACT)], dtype=np.float32)
        b.bind_actions(act_d.data_ptr(), NACT, torch.float32)
        b.configure_rewards([P.rew_vec(P.F_QPOS, 2, 1, target=0.9, norm=P.REW_SUMABS, shape=P.REW_EXP, k=10.0, weight=0.5),
                             P.rew_vec(P.F_QVEL, 0, 3, weight=-0.05)], dtype=np.float32, lo=-1.0, hi=1.0)
        b.configure_norm(NOBS, BLOCK, max_rows=NPOL * n, eps=cases.EPS)                        # (before the policy and the rollout: it holds no pointer of theirs)
        b.configure_policy(proto.defs, NOBS)
        for a, layers in enumerate(proto.weights):
            b.load_policy(a, layers)
        b.bind_policy_input(obs_d.data_ptr(), NOBS, NOBS + 2, torch.float32)
        b.bind_policy_norm(mean_d.data_ptr(), inv_d.data_ptr(), CLIP)
        b.bind_policy_output(0, mu_d.data_ptr(), NACT + 1)
        b.bind_policy_output(1, val_d.data_ptr(), 2)
        srcs = [("obs", NOBS), ("action", NACT), ("logp", 1), ("mu", NACT), ("value", 1), ("reward", 1), ("done", 1), ("reason", 1)]
        b.configure_rollout(NPOL, srcs, 0.99, 0.95, timeout_mask=P.DONE_TIME)
        b.configure_grad(NPOL * n, 32, 0.2, 0.5, 0.01)
        assert b.norm_count(P.NORM_N) == NOBS                               # (still configured)
        fence(b)
        st, st2 = torch.cuda.Stream(), torch.cuda.Stream()

        def forward(p):
            b.observe(stream=st.cuda_stream)
            b.bind_policy_sample(eps_d[p].data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
            b.policy(stream=st.cuda_stream)
            b.act(stream=st.cuda_stream)
            b.step_range(0, n, 50, st.cuda_stream)
            b.reward(stream=st.cuda_stream)

        forward(0)
        for t in range(NPOL):
            b.end_episodes(0, n, True, stream=st.cuda_stream)
            st2.wait_stream(st)                                             # the second range's record behind this step's stages ...
            b.rollout_record(t, 0, half, stream=st.cuda_stream)
            b.rollout_record(t, half, n - half, stream=st2.cuda_stream)
            st.wait_stream(st2)                                             # ... and everything that follows behind both records
            forward(t + 1)
        b.rollout_finish(stream=st.cuda_stream)
        b.rollout_normalise(1e-8, stream=st.cuda_stream)
        b.norm_update(st.cuda_stream)
        b.observe(stream=st.cuda_stream)
        b.bind_policy_sample(eps_d[NPOL + 1].data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
        b.policy(stream=st.cuda_stream)
        idx = np.random.default_rng(5).permutation(NPOL * n).astype(I32)[:200]
        idx_d = up(idx)
        st.synchronize()
        b.grad(idx_d.data_ptr(), len(idx), st.cuda_stream)
        fence(b)
        store = b.rollout("obs")
        assert np.all(np.isfinite(store))
        ref = cases.Ref(NOBS, BLOCK)
        ref.mean[:], ref.inv[:] = mean0, inv0
        want = ref.update(store.reshape(NPOL * n, NOBS))
        mean1, inv1 = mean_d.cpu().numpy(), inv_d.cpu().numpy()
        assert nc.same_bits(mean1, want["out_mean"]) and nc.same_bits(inv1, want["out_inv"])
        assert not np.any(mean1 == mean0) and not np.any(inv1 == inv0)
        stats = b.norm_stats()
        assert (stats["rows"], stats["blocks"], stats["updated"], stats["skipped"], stats["excluded"], stats["calls"], stats["n_max"]) == \
            (NPOL * n, -(-NPOL * n // BLOCK), NOBS, 0, 0, 1, NPOL * n)
        assert b.norm_launches() == (1, 1, 1, 1, 0)
        obs = obs_d.cpu().numpy()[:, :NOBS]
        res = pc.policy(obs, nets, (mean1, inv1, CLIP), eps[NPOL + 1], log_std)
        assert gc.same_bits(mu_d.cpu().numpy()[:, :NACT], res["out"][0]) and gc.same_bits(val_d.cpu().numpy()[:, :1], res["out"][1])
        assert gc.same_bits(act_d.cpu().numpy(), res["action"]) and gc.same_bits(logp_d.cpu().numpy(), res["logp"])
        old = pc.policy(obs, nets, (mean0, inv0, CLIP), eps[NPOL + 1], log_std)
        assert not gc.same_bits(old["out"][0], res["out"][0])
        h0 = b.grad_download(P.GRAD_ACT, 0, 0).reshape(len(idx), NOBS)
        rows = store.reshape(NPOL * n, NOBS)[idx]
        assert gc.same_bits(h0, pc.normalise(rows, mean1, inv1, CLIP)) and not gc.same_bits(h0, pc.normalise(rows, mean0, inv0, CLIP))
    finally:
        b.close()


def test_refusals_with_a_batch(cassie, built):
    import policy_cases
    from cassie_amd import Batch
    D, n = 12, 64
    b = Batch(cassie, n)
    try:
        for call in (b.norm_update, b.norm_write, b.norm_stats):
            with pytest.raises(RuntimeError, match="not configured"):
                call()
        with pytest.raises(ValueError, match="not configured"):
            b.bind_norm_output(None, None)
        for kw, msg in ((dict(dim=513), "dim lies in 1 .. 512"), (dict(block=24), "block is a multiple of 16"), (dict(max_rows=0), "max_rows lies in"),
                        (dict(eps=0.0), "eps is finite and > 0"), (dict(eps=float("nan")), "eps is finite and > 0")):
            with pytest.raises(ValueError, match=msg):
                b.configure_norm(**dict(dict(dim=D, block=64, max_rows=n), **kw))
        b.configure_norm(D, 64, max_rows=2 * n)
        with pytest.raises(RuntimeError, match="no rollout is configured"):
            b.norm_update()
        b.configure_rollout(3, [("action", 3)])
        with pytest.raises(RuntimeError, match="no OBS source"):
            b.norm_update()
        b.configure_rollout(3, [("obs", D + 1)])
        with pytest.raises(RuntimeError, match="does not have dim words"):
            b.norm_update()
        b.configure_rollout(3, [("obs", D)])
        with pytest.raises(RuntimeError, match="more samples than max_rows"):
            b.norm_update()
        b.configure_rollout(2, [("obs", D)])
        with pytest.raises(RuntimeError, match="no normalisation bound"):
            b.norm_update()
        with pytest.raises(RuntimeError, match="no normalisation bound"):
            b.norm_write()
        rng = np.random.default_rng(1)
        wide = policy_cases.Case("wide", [policy_cases.dense(rng, (D + 4, 8, 2), (P.POL_ELU, P.POL_TANH))], np.zeros((n, D + 4), dtype=F32), pad=0, wpad=0)
        b.configure_policy(wide.defs, D + 4)
        with pytest.raises(RuntimeError, match="no normalisation bound"):
            b.norm_update()
        mean_d, inv_d = up(np.zeros(D + 4, dtype=F32)), up(np.ones(D + 4, dtype=F32))
        b.bind_policy_norm(mean_d.data_ptr(), inv_d.data_ptr())
        with pytest.raises(RuntimeError, match="in_dim is not dim"):
            b.norm_update()
        with pytest.raises(ValueError, match="both or neither"):
            b.bind_norm_output(mean_d.data_ptr(), None)
        with pytest.raises(ValueError, match="strides of at least dim words"):
            b.bind_norm_source(mean_d.data_ptr(), 1, 1, 0, D - 1)
        b.bind_norm_output(mean_d.data_ptr(), inv_d.data_ptr())
        b.norm_update()                                                     # (the zeroed store: every column constant)
        fence(b)
        assert b.norm_stats()["updated"] == D and np.all(mean_d.cpu().numpy()[:D] == 0)
        b.configure_norm(0, release=True)
        with pytest.raises(RuntimeError, match="not configured"):
            b.norm_update()
    finally:
        b.close()
