"""Gradient rows (phys_batch_grad_*) on the device against the wave emulator and the definition restated in numpy (tests/grad_check.py),
BIT FOR BIT on every word: the cases tests/test_grad.py runs on the emulator, with weights loaded from device pointers and from host
arrays, the gradients in bound tensors with a row stride and in the batch's own.  Also: bindings read at the call, weights loaded anew,
two calls on one stream, that a call changes nothing of the batch, a live loop with every stage in place, and the refusals that need a
batch."""
import numpy as np
import pytest

import bench
import grad_cases as cases
import grad_check as gc
import grad_emu_py as ge
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import make

pytestmark = pytest.mark.gpu
F32, F64, I32 = np.float32, np.float64, np.int32


def fence(b):
    import torch
    b.sync()
    torch.cuda.synchronize()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Dev:
    """A batch with the policy, the rollout (its stores the case's padded arrays, bound) and the gradient rows of a case configured."""

    def __init__(self, cassie, case, chunk, max_m=None, host=False, load_first=True):
        p = case.p
        self.case, self.chunk, self.keep = case, chunk, {}
        self.b = b = Batch(cassie, case.nenv)
        b.configure_policy(p.defs, p.in_dim)
        if p.norm is not None:
            self.mean, self.inv = up(np.asarray(p.norm[0], dtype=F32)), up(np.asarray(p.norm[1], dtype=F32))
            b.bind_policy_norm(self.mean.data_ptr(), self.inv.data_ptr(), p.norm[2])
        A = case.A
        self.ls = up(np.asarray(case.log_std, dtype=F32))
        self.dummy = [up(np.zeros((case.nenv, A), dtype=F32)), up(np.zeros((case.nenv, A), dtype=F32)), up(np.zeros(case.nenv, dtype=F32))]
        b.bind_policy_sample(self.dummy[0].data_ptr(), self.ls.data_ptr(), self.dummy[1].data_ptr(), self.dummy[2].data_ptr())
        srcs = [("obs", p.in_dim), ("action", A), ("logp", 1), ("value", 1)]
        b.configure_rollout(case.T, srcs)
        self.arr = {k: up(case.arr[k]) for k in cases.KINDS}
        for k in cases.KINDS:
            b.bind_rollout_storage(k, self.arr[k].data_ptr(), case.step[k], case.row[k])
        fence(b)
        if load_first:
            self.load(host)
        b.configure_grad(case.S if max_m is None else max_m, chunk, case.eps, case.c_v, case.c_ent)
        if not load_first:
            self.load(host)

    def load(self, host=False, weights=None):
        p = self.case.p
        for n, layers in enumerate(weights or p.weights):
            if host:
                self.b.load_policy(n, [(w[:, : w.shape[1] - p.wpad], bias) for w, bias in layers])
            else:
                dev = [(up(w), up(bias)) for w, bias in layers]
                self.keep[n] = dev
                fence(self.b)
                self.b.load_policy(n, [(w.data_ptr(), w.shape[1], bias.data_ptr()) for w, bias in dev])

    def bind(self):
        """Padded gradient tensors of the caller's, FILL everywhere."""
        dw, db, dls = cases.result_tensors(self.case)
        self.dw, self.db, self.dls = [[up(a) for a in per] for per in dw], [[up(a) for a in per] for per in db], up(dls)
        fence(self.b)
        for n in range(len(dw)):
            for l in range(len(dw[n])):
                self.b.bind_grad(n, l, self.dw[n][l].data_ptr(), dw[n][l].shape[1], self.db[n][l].data_ptr())
        self.b.bind_grad_log_std(self.dls.data_ptr())

    def grad(self, idx, stream=None):
        self.idx = up(np.asarray(idx, dtype=I32))
        fence(self.b)
        self.b.grad(self.idx.data_ptr(), len(idx), stream)
        fence(self.b)
        return self.result(len(idx))

    def result(self, m):
        b = self.b
        get = lambda what, n, l, dt: b.grad_stats()["all"] if what == ge.NSTATS else b.grad_download(what, n, l)
        return ge.fetch_all(self.case, m, self.chunk, get)

    def close(self):
        self.b.close()


CASES = {"four layers": (cases.four_layer_case, ((38, 16),)), "one layer": (cases.one_layer_case, ((20, 32),)),
         "actor only": (cases.actor_only_case, ((37, 32),)), "limits": (cases.limits_case, ((16, 16),))}


@pytest.fixture(scope="module")
def shared():
    return cases.shared_case()


@pytest.mark.parametrize("chunk", cases.CHUNKS)
def test_shared_case(cassie, built, shared, chunk):
    """Every M of the shared case: weights from device pointers, gradients in bound tensors with a row stride -- the sentinel between the
    rows stays -- against the restatement and the emulator."""
    d = Dev(cassie, shared, chunk)
    try:
        d.bind()
        for m in cases.COUNTS:
            idx = shared.idx(m)
            got, want = d.grad(idx), shared.reference(idx, chunk)
            assert gc.differing(got, want) == [], (m, chunk)
            assert gc.differing(got, ge.Call(shared, chunk).grad(idx)) == [], (m, chunk)
            for n in range(len(d.dw)):
                for l, t in enumerate(d.dw[n]):
                    full = t.cpu().numpy()
                    assert gc.same_bits(full[:, :-3], want["dw"][n][l]) and np.all(full[:, -3:] == cases.FILL)
                    assert gc.same_bits(d.db[n][l].cpu().numpy(), want["db"][n][l])
            assert gc.same_bits(d.dls.cpu().numpy(), want["dls"])
        assert d.b.grad_launches()[:5] == (len(cases.COUNTS),) * 5
    finally:
        d.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_other_cases_from_host_weights_into_own_tensors(cassie, built, name):
    mk, runs = CASES[name]
    case = mk()
    for m, chunk in runs:
        d = Dev(cassie, case, chunk, host=True, load_first=False)
        try:
            idx = case.idx(m)
            got = d.grad(idx)
            assert gc.differing(got, case.reference(idx, chunk)) == [], (name, m, chunk)
            assert gc.differing(got, ge.Call(case, chunk).grad(idx)) == [], (name, m, chunk)
            for n, (layers, _) in enumerate(case.p.nets):
                for l, (w, _) in enumerate(layers):
                    assert gc.same_bits(d.b.grad_download(P.GRAD_PACKT, n, l), gc.pack_t(w))
        finally:
            d.close()


def test_bindings_and_weights_act_at_once_and_calls_do_not_disturb_each_other(cassie, built, shared):
    """log_std and the normalisation vectors changed in place between two calls act at once; weights loaded anew after a call give the
    new gradients; two calls on one stream with different idx give what each gives in a fresh batch."""
    import copy
    import torch
    chunk = 16
    d = Dev(cassie, shared, chunk)
    try:
        ia, ib = shared.idx(37), shared.idx(17, seed=9)
        st = torch.cuda.Stream()
        d.idx2 = up(ib)
        d.idx = up(ia)
        fence(d.b)
        d.b.grad(d.idx.data_ptr(), len(ia), st.cuda_stream)
        d.b.grad(d.idx2.data_ptr(), len(ib), st.cuda_stream)
        fence(d.b)
        assert gc.differing(d.result(len(ib)), shared.reference(ib, chunk)) == []
        assert gc.differing(d.grad(ia), shared.reference(ia, chunk)) == []
        # the vectors change in place
        case = copy.copy(shared)
        case.p = copy.copy(shared.p)
        case.log_std = (shared.log_std + F32(0.25)).astype(F32)
        case.p.norm = ((shared.p.norm[0] + F32(0.125)).astype(F32), (shared.p.norm[1] * F32(0.75)).astype(F32), shared.p.norm[2])
        d.ls.copy_(up(case.log_std)); d.mean.copy_(up(case.p.norm[0])); d.inv.copy_(up(case.p.norm[1]))
        want = case.reference(ia, chunk)
        assert gc.differing(d.grad(ia), want) == [] and gc.differing(want, shared.reference(ia, chunk)) != []
        # weights loaded anew
        rng = np.random.default_rng(77)
        case.p.nets = [([((w * F32(1.0 + 0.01 * rng.normal())).astype(F32), (b_ + F32(0.01)).astype(F32)) for w, b_ in layers], acts) for layers, acts in shared.p.nets]
        case.p.weights = [[(case.p.padded(w, case.p.wpad), b_) for w, b_ in layers] for layers, _ in case.p.nets]
        d.load(weights=case.p.weights)
        want2 = case.reference(ia, chunk)
        assert gc.differing(d.grad(ia), want2) == [] and gc.differing(want2, want) != []
    finally:
        d.close()


def test_a_call_changes_nothing_else(cassie, built, shared):
    d = Dev(cassie, shared, 32)
    try:
        b = d.b

        b.configure_states(shared.nenv, P.STATE_CORE)

        def everything():
            fence(b)
            b.save_states()
            return [b.states()[0].tobytes(), b.policy_packed().tobytes()] + [d.arr[k].cpu().numpy().tobytes() for k in cases.KINDS] + \
                [t.cpu().numpy().tobytes() for t in d.dummy + [d.ls, d.mean, d.inv]]

        before = everything()
        d.grad(shared.idx(130))
        assert everything() == before
    finally:
        d.close()


NOBS, NACT, NPOL, NLIVE = 12, 3, 3, 130


def test_live_loop_then_one_grad_over_every_sample(cassie, built):
    """130 envs on cassie.xml, every stage in place for T = 3 policy steps (end_episodes, record, observe, policy, act, step, reward), then
    rollout_finish, rollout_normalise and one grad over a permutation of all 390 samples with chunk 32: equal to the restatement fed the
    downloaded stores, bit for bit."""
    import policy_cases
    import torch
    n = NLIVE
    rng = np.random.default_rng(31)
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * rng.random(n)
    nets = [policy_cases.dense(rng, (NOBS, 16, NACT), (P.POL_ELU, P.POL_TANH)), policy_cases.dense(rng, (NOBS, 16, 1), (P.POL_TANH, P.POL_IDENTITY))]
    proto = policy_cases.Case("live", nets, np.zeros((n, NOBS), dtype=F32), pad=0, wpad=0)
    eps = np.clip(rng.normal(size=(NPOL + 1, n, NACT)), -4, 4).astype(F32)
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
        # the weights move a little after the rollout, as after an optimiser step: the ratios leave 1
        moved = [([((w * F32(1.02)).astype(F32), bb) for w, bb in layers], acts) for layers, acts in nets]
        for a, (layers, _) in enumerate(moved):
            b.load_policy(a, layers)
        fence(b)
        b.grad(idx_d.data_ptr(), len(idx), st.cuda_stream)
        fence(b)
        S = NPOL * n
        stores = {"obs": b.rollout("obs").reshape(S, NOBS), "action": b.rollout("action").reshape(S, NACT), "logp": b.rollout("logp").reshape(S),
                  "advn": b.rollout("advn").reshape(S), "ret": b.rollout("ret").reshape(S)}
        want = gc.grad(moved, stores, idx, 32, 0.2, 0.5, 0.01, None, log_std)
        case = type("C", (), {"p": type("Pc", (), {"nets": moved, "in_dim": NOBS})()})()
        got = ge.fetch_all(case, len(idx), 32, lambda what, nn, l, dt: b.grad_stats()["all"] if what == ge.NSTATS else b.grad_download(what, nn, l))
        assert gc.differing(got, want) == []
        assert want["stats"][5] == 0 and want["stats"][6] == S and np.all(np.isfinite(want["stats"])) and np.abs(want["ratio"] - 1).max() > 1e-3
        assert all(np.abs(w).max() > 0 for per in want["dw"] for w in per)
        assert b.grad_launches() == (1, 1, 1, 1, 1, 8)
    finally:
        b.close()


def test_refusals_with_a_batch(cassie, built, shared):
    import torch
    b = Batch(cassie, shared.nenv)
    try:
        idx = up(shared.idx(16))
        with pytest.raises(RuntimeError, match="not configured"):
            b.grad(idx.data_ptr(), 16)
        with pytest.raises(ValueError, match="configured policy and rollout"):
            b.configure_grad(16, 16)
    finally:
        b.close()
    d = Dev(cassie, shared, 16, max_m=32, load_first=False)
    try:
        b = d.b
        with pytest.raises(RuntimeError, match="m lies in 1 .. max_m"):
            b.grad(idx.data_ptr(), 33)
        with pytest.raises(ValueError, match="chunk is a multiple of 16"):
            b.configure_grad(32, 24)
        with pytest.raises(ValueError, match="c_v is finite"):
            b.configure_grad(32, 16, 0.2, -1.0)
        with pytest.raises(ValueError, match="max_m lies in"):
            b.configure_grad(shared.S + 1, 16)
        with pytest.raises(ValueError, match="row stride"):
            b.bind_grad(0, 0, idx.data_ptr(), 2, idx.data_ptr())
        with pytest.raises(ValueError, match="no such network or layer"):
            b.bind_grad(0, 3, idx.data_ptr(), 64, idx.data_ptr())
        b.grad(idx.data_ptr(), 16)
        # a policy configured anew releases the gradient rows; a layer never loaded refuses the call
        b.configure_policy(shared.p.defs, shared.p.in_dim)
        with pytest.raises(RuntimeError, match="not configured"):
            b.grad(idx.data_ptr(), 16)
        b.configure_grad(32, 16)
        with pytest.raises(RuntimeError, match="never loaded"):
            b.grad(idx.data_ptr(), 16)
        d.load()
        with pytest.raises(RuntimeError, match="no log_std"):
            b.grad(idx.data_ptr(), 16)
        b.configure_grad(0, 16)
        with pytest.raises(RuntimeError, match="not configured"):
            b.grad_stats()
        # a rollout configured anew releases them too; a missing role and a missing ADVN refuse the call
        b.configure_grad(32, 16)
        b.configure_rollout(shared.T, [("obs", shared.p.in_dim), ("action", shared.A)])
        with pytest.raises(RuntimeError, match="not configured"):
            b.grad(idx.data_ptr(), 16)
        b.configure_grad(32, 16)
        with pytest.raises(RuntimeError, match="sources of role OBS, ACTION and LOGP"):
            b.grad(idx.data_ptr(), 16)
        b.configure_rollout(shared.T, [("obs", shared.p.in_dim), ("action", shared.A), ("logp", 1), ("value", 1)])
        b.configure_grad(32, 16)
        with pytest.raises(RuntimeError, match="no ADVN"):
            b.grad(idx.data_ptr(), 16)
    finally:
        d.close()
