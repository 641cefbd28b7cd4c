"""Optimiser rows (phys_batch_opt_*) on the device against the wave emulator and the definition restated in numpy (tests/opt_check.py), BIT
FOR BIT on every word: the cases tests/test_opt.py runs on the emulator, with the master tensors bound with a row stride, the gradients in
bound tensors and in the batch's own.  Also: two grad + opt_step pairs on one stream with no fence, the packings against a following
load_policy, the pack-launch counters, that a call changes nothing else of the batch, the skip of a NaN gradient, a checkpoint through
download and upload, a live loop that acts with the updated weights, and the refusals that need a batch."""
import copy

import numpy as np
import pytest

import bench
import grad_cases as gcs
import grad_check as gc
import opt_cases as cases
import opt_check as oc
import opt_emu_py as oe
import policy_check as pc
from cassie_amd import phys as P
from test_episodes_gpu import make
from test_grad_gpu import Dev, fence, up

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32


class DevOpt:
    """test_grad_gpu.Dev (the policy loaded from device tensors with a row stride, the rollout, the gradient rows) with the optimiser rows
    configured and those device tensors bound as the master tensors."""

    def __init__(self, cassie, case, max_norm=np.inf, bound=True, chunk=16, bind=True, **hyper):
        self.case, self.d = case, Dev(cassie, case, chunk)
        self.b = b = self.d.b
        if bound:
            self.d.bind()
        self.slots = [(n, l) for n, layers in enumerate(case.p.weights) for l in range(len(layers))]
        self.shapes = [(w.shape[0], w.shape[1] - case.p.wpad) for layers in case.p.weights for w, _ in layers]
        b.configure_opt(**dict(cases.HYPER, max_norm=max_norm, **hyper))
        if bind:
            self.bind()

    def bind(self):
        for n, l in self.slots:
            w, bias = self.d.keep[n][l]
            self.b.bind_opt_param(n, l, w.data_ptr(), w.shape[1], bias.data_ptr())
        self.b.bind_opt_log_std(self.d.ls.data_ptr())

    def moments(self):
        b = self.b
        get = lambda ww, wb, wl: oc.flat([b.opt_download(ww, n, l).reshape(s) for (n, l), s in zip(self.slots, self.shapes)],
                                         [b.opt_download(wb, n, l) for n, l in self.slots], b.opt_download(wl))
        return get(P.OPT_M_W, P.OPT_M_B, P.OPT_M_LS), get(P.OPT_V_W, P.OPT_V_B, P.OPT_V_LS)

    def snapshot(self):
        """Every word in opt_cases' form (waits for the streams)."""
        fence(self.b)
        b = self.b
        wfull = [self.d.keep[n][l][0].cpu().numpy() for n, l in self.slots]
        m, v = self.moments()
        return {"wfull": wfull, "w": [np.ascontiguousarray(w[:, :kin]) for w, (_, kin) in zip(wfull, self.shapes)],
                "b": [self.d.keep[n][l][1].cpu().numpy() for n, l in self.slots], "ls": self.d.ls.cpu().numpy(), "packed": b.policy_packed(),
                "packt": np.concatenate([b.grad_download(P.GRAD_PACKT, n, l) for n, l in self.slots]), "m": m, "v": v,
                "part": b.opt_download(P.OPT_PARTIALS), "scalars": b.opt_download(P.OPT_SCALARS), "stats": b.opt_stats()["all"]}

    def close(self):
        self.d.close()


def middle(name):
    ns = cases.norms(cases.setup(name)[1])
    return float(np.sqrt(min(ns) * max(ns)))


@pytest.mark.parametrize("name,bound", [("shared", True), ("shared", False), ("four layers", True), ("one layer", False), ("actor only", True),
                                        ("limits", False)])
def test_three_steps_on_the_device(cassie, built, name, bound):
    """grad + opt_step three times, each grad with the weights the step before it left and no load_policy: every word after every step
    is the emulator's and the restatement's, fed the gradients the device's grad call left."""
    case, _ = cases.setup(name)
    max_norm = middle(name)
    o = DevOpt(cassie, case, max_norm, bound, chunk=cases.CASES[name][1][0][1])
    try:
        e, r = oe.Opt(case, max_norm=max_norm, **cases.HYPER), cases.Ref(case, max_norm=max_norm)
        for k, ((m, chunk, seed), lr) in enumerate(zip(cases.CASES[name][1], cases.LRS)):
            g = cases.slots(o.d.grad(case.idx(m, seed=seed)))
            o.b.opt_step(lr)
            got = o.snapshot()
            e.set_grads(*g)
            assert cases.differing(got, r.step(g, lr)) == [], (name, k)
            assert cases.differing(got, e.step(lr)) == [], (name, k)
            assert cases.padding_kept(got, o.shapes)
        assert o.b.opt_launches() == (3, 3, 3) and got["stats"][3] == 3 and got["stats"][4] == 0
    finally:
        o.close()


def with_params(case, ws, bs, ls):
    """The grad case with other weights and log_std (the restatement reads p.nets and log_std alone)."""
    c = copy.copy(case)
    c.p = copy.copy(case.p)
    it = iter(zip(ws, bs))
    c.p.nets = [([next(it) for _ in layers], acts) for layers, acts in case.p.nets]
    c.log_std = ls
    return c


def test_two_pairs_back_to_back_on_one_stream(cassie, built):
    """grad, opt_step, grad, opt_step on one stream with no fence between them: the second grad reads the packings the first step wrote.
    The second gradient is the restatement's for the restatement's updated weights, the final words are the restatement's."""
    import torch
    case, grads = cases.setup("shared")
    (m1, c1, s1), (m2, _, s2) = cases.CASES["shared"][1][:2]
    o = DevOpt(cassie, case, 1e15, True, chunk=c1)
    try:
        i1, i2 = case.idx(m1, seed=s1), case.idx(m2, seed=s2)
        d1, d2 = up(i1), up(i2)
        st = torch.cuda.Stream()
        before = o.b.grad_launches()
        fence(o.b)
        o.b.grad(d1.data_ptr(), m1, st.cuda_stream)
        o.b.opt_step(cases.LRS[0], st.cuda_stream)
        o.b.grad(d2.data_ptr(), m2, st.cuda_stream)
        o.b.opt_step(cases.LRS[1], st.cuda_stream)
        got = o.snapshot()
        assert o.b.grad_launches()[5] == before[5]                           # (no transposed packing was made)
        r = cases.Ref(case, max_norm=1e15)
        r.step(grads[0], cases.LRS[0])
        res2 = o.d.result(m2)
        want2 = with_params(case, *r.params()).reference(i2, c1)
        assert gc.differing(res2, want2) == []
        assert cases.differing(got, r.step(cases.slots(want2), cases.LRS[1])) == []
    finally:
        o.close()


def test_a_following_load_policy_changes_no_packed_word(cassie, built):
    """After opt_step the packed weights and the transposed packing are what load_policy makes of the updated master tensors; the
    pack-launch counter does not move during opt_step and moves with the load; nothing else of the batch changes in an opt_step."""
    case, _ = cases.setup("shared")
    o = DevOpt(cassie, case, 1e15, True)
    try:
        b, d = o.b, o.d
        b.configure_states(case.nenv, P.STATE_CORE)
        m, chunk, seed = cases.CASES["shared"][1][0]
        d.grad(case.idx(m, seed=seed))

        def everything_else():
            fence(b)
            b.save_states()
            res = d.result(m)
            return [b.states()[0].tobytes(), gc.words(res).tobytes()] + [d.arr[k].cpu().numpy().tobytes() for k in gcs.KINDS] + \
                [t.cpu().numpy().tobytes() for t in d.dummy + [d.mean, d.inv]] + [t.cpu().numpy().tobytes() for per in d.dw + d.db for t in per]

        before, packs, packed0 = everything_else(), b.grad_launches()[5], b.policy_packed()
        b.opt_step(1e-3)
        assert everything_else() == before
        assert b.grad_launches()[5] == packs and b.opt_launches() == (1, 1, 1)
        packed = b.policy_packed()
        packt = [b.grad_download(P.GRAD_PACKT, n, l) for n, l in o.slots]
        assert not gc.same_bits(packed, packed0)
        for n in range(len(case.p.weights)):
            b.load_policy(n, [(w.data_ptr(), w.shape[1], bias.data_ptr()) for w, bias in d.keep[n]])
        fence(b)
        assert b.grad_launches()[5] == packs + len(o.slots)
        assert gc.same_bits(b.policy_packed(), packed)
        assert all(gc.same_bits(b.grad_download(P.GRAD_PACKT, n, l), t) for (n, l), t in zip(o.slots, packt))
    finally:
        o.close()


def test_a_nan_gradient_skips_the_call_on_the_device(cassie, built):
    """Step 1, then a call whose bound gradient holds one NaN word: every word stays, skipped = 1, t = 1; the next clean pair goes on."""
    case, grads = cases.setup("shared")
    runs = cases.CASES["shared"][1]
    o = DevOpt(cassie, case, 1e15, True, chunk=16)
    try:
        r = cases.Ref(case, max_norm=1e15)
        g = cases.slots(o.d.grad(case.idx(runs[0][0], seed=runs[0][2])))
        o.b.opt_step(cases.LRS[0])
        one = o.snapshot()
        assert cases.differing(one, r.step(g, cases.LRS[0])) == []
        g = cases.slots(o.d.grad(case.idx(runs[1][0], seed=runs[1][2])))
        o.d.dw[0][1][2, 3] = float("nan")
        g[0][1][2, 3] = np.nan
        fence(o.b)
        o.b.opt_step(cases.LRS[1])
        two = o.snapshot()
        assert cases.differing(two, r.step(g, cases.LRS[1])) == []
        assert cases.differing(two, one, keys=("w", "b", "ls", "packed", "packt", "m", "v")) == []
        assert all(gc.same_bits(a, b) for a, b in zip(two["wfull"], one["wfull"]))
        assert two["stats"][2] == 1 and list(two["scalars"]) == [1, F64(0.9), F64(0.999), 1]
        g = cases.slots(o.d.grad(case.idx(runs[1][0], seed=runs[1][2])))
        o.b.opt_step(cases.LRS[2])
        three = o.snapshot()
        assert cases.differing(three, r.step(g, cases.LRS[2])) == []
        assert three["stats"][2] == 0 and three["scalars"][0] == 2 and three["scalars"][3] == 1
    finally:
        o.close()


def test_a_checkpoint_through_download_and_upload(cassie, built):
    """Two steps; the moments and scalars downloaded; the optimiser rows configured anew (moments +0.0, t = 0), everything uploaded: the
    downloads are the same words again, and the third step equals the restatement's uninterrupted run."""
    case, _ = cases.setup("four layers")
    runs = cases.CASES["four layers"][1]
    o = DevOpt(cassie, case, np.inf, False)
    try:
        b, r = o.b, cases.Ref(case)
        for (m, chunk, seed), lr in zip(runs[:2], cases.LRS):
            g = cases.slots(o.d.grad(case.idx(m, seed=seed)))
            b.opt_step(lr)
            r.step(g, lr)
        kinds = [(what, n, l) for n, l in o.slots for what in (P.OPT_M_W, P.OPT_M_B, P.OPT_V_W, P.OPT_V_B)] + \
            [(what, 0, 0) for what in (P.OPT_M_LS, P.OPT_V_LS, P.OPT_SCALARS)]
        saved = {k: b.opt_download(*k) for k in kinds}
        b.configure_opt(**cases.HYPER)
        o.bind()
        assert not b.opt_download(P.OPT_M_W, 0, 0).any() and list(b.opt_download(P.OPT_SCALARS)) == [0, 1, 1, 0]
        for (what, n, l), values in saved.items():
            b.opt_upload(what, values, n, l)
        assert all(gc.same_bits(b.opt_download(*k), v) for k, v in saved.items())
        m, chunk, seed = runs[2]
        g = cases.slots(o.d.grad(case.idx(m, seed=seed)))
        b.opt_step(cases.LRS[2])
        assert cases.differing(o.snapshot(), r.step(g, cases.LRS[2])) == []
        with pytest.raises(ValueError, match="no such network, layer or kind"):
            b.opt_upload(P.OPT_PARTIALS, np.zeros(b.opt_count(P.OPT_PARTIALS)))
        assert b.opt_count(P.OPT_M_W, 0, 9) == -1 and b.opt_count(99) == -1
    finally:
        o.close()


NOBS, NACT, NPOL, NLIVE = 12, 3, 3, 130


def test_live_loop_acts_with_the_updated_weights(cassie, built):
    """The live loop of test_grad_gpu.py -- 130 envs on cassie.xml, every stage in place for T = 3 policy steps, finish, normalise, one
    grad over all 390 samples with chunk 32 -- with opt_step behind grad and then a policy() call with no load_policy: its outputs,
    actions and log-probabilities are the restatement's policy evaluated with the restatement's updated weights, bit for bit."""
    import policy_cases
    import torch
    n = NLIVE
    rng = np.random.default_rng(31)
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
        eps_d, ls_d = torch.from_numpy(eps).cuda(), torch.from_numpy(log_std).cuda()
        b.configure_obs([P.obs_copy(P.F_QPOS, 7, 10, scale=1.0), P.obs_copy(P.F_QVEL, 0, 2, scale=0.1)], history=1, dtype=np.float32)
        b.bind_obs(obs_d.data_ptr(), NOBS + 2)
        b.configure_actions([P.act_col(P.F_PD_PTARGET, j, lo=-1.5, hi=1.5, offset=float(bench.PD_OFFSET[j]), scale=0.2) for j in range(NACT)], dtype=np.float32)
        b.bind_actions(act_d.data_ptr(), NACT, torch.float32)
        b.configure_rewards([P.rew_vec(P.F_QPOS, 2, 1, target=0.9, norm=P.REW_SUMABS, shape=P.REW_EXP, k=10.0, weight=0.5),
                             P.rew_vec(P.F_QVEL, 0, 3, weight=-0.05)], dtype=np.float32, lo=-1.0, hi=1.0)
        b.configure_policy(proto.defs, NOBS)
        for a, layers in enumerate(proto.weights):
            b.load_policy(a, layers)
        b.bind_policy_input(obs_d.data_ptr(), NOBS, NOBS + 2, torch.float32)
        b.bind_policy_output(0, mu_d.data_ptr(), NACT + 1)
        b.bind_policy_output(1, val_d.data_ptr(), 2)
        srcs = [("obs", NOBS), ("action", NACT), ("logp", 1), ("mu", NACT), ("value", 1), ("reward", 1), ("done", 1), ("reason", 1)]
        b.configure_rollout(NPOL, srcs, 0.99, 0.95, timeout_mask=P.DONE_TIME)
        b.configure_grad(NPOL * n, 32, 0.2, 0.5, 0.01)
        b.configure_opt(max_norm=0.5)
        fence(b)
        st = torch.cuda.Stream()

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
            b.rollout_record(t, stream=st.cuda_stream)
            forward(t + 1)
        b.rollout_finish(stream=st.cuda_stream)
        b.rollout_normalise(1e-8, stream=st.cuda_stream)
        idx = np.random.default_rng(5).permutation(NPOL * n).astype(I32)
        idx_d = up(idx)
        # the weights move a little after the rollout, as after an earlier update: the ratios leave 1.  They are the master tensors
        moved = [([((w * F32(1.02)).astype(F32), bb) for w, bb in layers], acts) for layers, acts in nets]
        masters = [[(up(w), up(bb)) for w, bb in layers] for layers, _ in moved]
        fence(b)
        for a, layers in enumerate(masters):
            b.load_policy(a, [(w.data_ptr(), w.shape[1], bb.data_ptr()) for w, bb in layers], st.cuda_stream)
            for l, (w, bb) in enumerate(layers):
                b.bind_opt_param(a, l, w.data_ptr(), w.shape[1], bb.data_ptr())
        b.bind_opt_log_std(ls_d.data_ptr())
        packs = b.grad_launches()[5]
        b.grad(idx_d.data_ptr(), len(idx), st.cuda_stream)
        b.opt_step(3e-3, st.cuda_stream)
        b.observe(stream=st.cuda_stream)
        b.bind_policy_sample(eps_d[NPOL + 1].data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
        b.policy(stream=st.cuda_stream)
        fence(b)
        assert b.grad_launches()[5] == packs and b.opt_launches() == (1, 1, 1)
        S = NPOL * n
        stores = {"obs": b.rollout("obs").reshape(S, NOBS), "action": b.rollout("action").reshape(S, NACT), "logp": b.rollout("logp").reshape(S),
                  "advn": b.rollout("advn").reshape(S), "ret": b.rollout("ret").reshape(S)}
        want = gc.grad(moved, stores, idx, 32, 0.2, 0.5, 0.01, None, log_std)
        ws, bs = [w for layers, _ in moved for w, _ in layers], [bb for layers, _ in moved for _, bb in layers]
        state = oc.State(sum(w.size + bb.size for w, bb in zip(ws, bs)) + NACT)
        new, stats, _ = oc.step(oc.flat(ws, bs, log_std), oc.flat(*cases.slots(want)), state, 3e-3, max_norm=0.5, **cases.HYPER)
        assert gc.same_bits(b.opt_stats()["all"], stats) and stats[2] == 0 and stats[3] == 1
        ws, bs, ls = oc.unflat(new, [w.shape for w in ws], NACT)
        assert gc.same_bits(ls_d.cpu().numpy(), ls) and not gc.same_bits(ls, log_std)
        assert all(gc.same_bits(t.cpu().numpy(), w) for (t, _), w in zip([p for layers in masters for p in layers], ws))
        it = iter(zip(ws, bs))
        new_nets = [([next(it) for _ in layers], acts) for layers, acts in moved]
        obs = obs_d.cpu().numpy()[:, :NOBS]
        ref = pc.policy(obs, new_nets, None, eps[NPOL + 1], ls)
        assert gc.same_bits(mu_d.cpu().numpy()[:, :NACT], ref["out"][0]) and gc.same_bits(val_d.cpu().numpy()[:, :1], ref["out"][1])
        assert gc.same_bits(act_d.cpu().numpy(), ref["action"]) and gc.same_bits(logp_d.cpu().numpy(), ref["logp"])
        old = pc.policy(obs, moved, None, eps[NPOL + 1], log_std)
        assert not gc.same_bits(old["action"], ref["action"])
    finally:
        b.close()


def test_refusals_with_a_batch(cassie, built):
    from cassie_amd import Batch
    case, _ = cases.setup("shared")
    b = Batch(cassie, case.nenv)
    try:
        with pytest.raises(ValueError, match="needs configured gradient rows"):
            b.configure_opt()
        with pytest.raises(RuntimeError, match="not configured"):
            b.opt_step(1e-3)
        with pytest.raises(RuntimeError, match="not configured"):
            b.opt_stats()
    finally:
        b.close()
    o = DevOpt(cassie, case, bind=False)
    try:
        b, d = o.b, o.d
        with pytest.raises(ValueError, match="beta1 lies in"):
            b.configure_opt(beta1=1.0)
        with pytest.raises(ValueError, match="max_norm is > 0"):
            b.configure_opt(max_norm=0.0)
        with pytest.raises(RuntimeError, match="a master tensor is not bound"):
            b.opt_step(1e-3)
        w, bias = d.keep[0][0]
        with pytest.raises(ValueError, match="W row stride"):
            b.bind_opt_param(0, 0, w.data_ptr(), 2, bias.data_ptr())
        with pytest.raises(ValueError, match="no such network or layer"):
            b.bind_opt_param(0, 3, w.data_ptr(), 64, bias.data_ptr())
        with pytest.raises(ValueError, match="both needed"):
            b.bind_opt_param(0, 0, w.data_ptr(), w.shape[1], None)
        with pytest.raises(ValueError, match="must be the one phys_batch_policy_bind_sample names"):
            b.bind_opt_log_std(d.dummy[2].data_ptr())
        for n, l in o.slots:
            w, bias = d.keep[n][l]
            b.bind_opt_param(n, l, w.data_ptr(), w.shape[1], bias.data_ptr())
        with pytest.raises(RuntimeError, match="master log_std is not bound"):
            b.opt_step(1e-3)
        b.bind_opt_log_std(d.ls.data_ptr())
        with pytest.raises(RuntimeError, match="no gradient yet"):
            b.opt_step(1e-3)
        d.grad(case.idx(16))
        for lr in (float("nan"), -1e-3, float("inf")):
            with pytest.raises(RuntimeError, match="lr is finite and >= 0"):
                b.opt_step(lr)
        b.opt_step(1e-3)
        # the sample bound anew with another log_std: the step refuses until the optimiser's is that one
        other = up(np.asarray(case.log_std, dtype=F32))
        b.bind_policy_sample(d.dummy[0].data_ptr(), other.data_ptr(), d.dummy[1].data_ptr(), d.dummy[2].data_ptr())
        with pytest.raises(RuntimeError, match="must be the one phys_batch_policy_bind_sample names"):
            b.opt_step(1e-3)
        # the release form; gradient rows configured anew release the optimiser rows too
        b.configure_opt(release=True)
        with pytest.raises(RuntimeError, match="not configured"):
            b.opt_step(1e-3)
        b.configure_opt()
        b.configure_grad(32, 16)
        with pytest.raises(RuntimeError, match="not configured"):
            b.opt_step(1e-3)
        with pytest.raises(ValueError, match="not configured"):
            b.bind_opt_log_std(other.data_ptr())
    finally:
        o.close()
