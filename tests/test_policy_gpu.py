"""Policy rows (phys_batch_policy) on the device against the definition restated in numpy (tests/policy_check.py) and against the wave
emulator, BIT FOR BIT on float32 words: the cases tests/test_policy.py runs on the emulator, loaded from device pointers and from host
arrays.  Also: that vectors read at every call act at once, weights loaded anew, two ranges on two streams, the loop observe -> policy ->
act -> step against the restatement's actions uploaded in between, that a call changes nothing of the batch, and the refusals that need a
batch."""
import numpy as np
import pytest

import bench
import policy_cases as cases
import policy_check as pc
import policy_emu_py as pe
from cassie_amd import Batch
from cassie_amd import phys as P
from test_episodes_gpu import make

pytestmark = pytest.mark.gpu
F32 = np.float32


def fence(b):
    import torch
    b.sync()
    torch.cuda.synchronize()


class Device:
    """A case's policy on a batch: the tensors of the case in torch tensors with the case's row strides, bound; `load`: "device" (the
    weights from torch tensors' data_ptr()) or "host" (numpy arrays)."""

    def __init__(self, model, case, load="device", batch=None):
        import torch
        self.case, self.own = case, batch is None
        self.b = b = Batch(model, case.nenv) if batch is None else batch
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        b.configure_policy(case.defs, case.in_dim)
        self.w = [[(up(w), up(bias)) for w, bias in layers] for layers in case.weights]
        self.load(load)
        self.x = up(case.x)
        b.bind_policy_input(self.x.data_ptr(), case.in_dim, case.x.shape[1], torch.float32)
        if case.norm is not None:
            self.mean, self.inv = up(np.asarray(case.norm[0], dtype=F32)), up(np.asarray(case.norm[1], dtype=F32))
            b.bind_policy_norm(self.mean.data_ptr(), self.inv.data_ptr(), case.norm[2])
        self.fresh()
        fence(b)

    def load(self, how, stream=None):
        case = self.case
        for n, layers in enumerate(self.w):
            if how == "device":
                self.b.load_policy(n, [(w.data_ptr(), w.shape[1], bias.data_ptr()) for w, bias in layers], stream=stream)
            else:
                self.b.load_policy(n, [(w[:, : w.shape[1] - case.wpad], bias) for w, bias in case.weights[n]])

    def fresh(self):
        """Output tensors of FILL, bound."""
        import torch
        case, b = self.case, self.b
        self.res = {k: ([torch.from_numpy(a).cuda() for a in v] if k == "out" else torch.from_numpy(v).cuda()) for k, v in case.fresh().items()}
        for n in range(len(case.widths)):
            b.bind_policy_output(n, self.res["out"][n].data_ptr(), self.res["out"][n].shape[1])
        if case.eps is not None:
            self.eps, self.log_std = torch.from_numpy(case.eps).cuda(), torch.from_numpy(case.log_std).cuda()
            b.bind_policy_sample(self.eps.data_ptr(), self.log_std.data_ptr(), self.res["action"].data_ptr(), self.res["logp"].data_ptr(),
                                 eps_stride=case.eps.shape[1], action_stride=self.res["action"].shape[1])
        fence(b)

    def download(self):
        fence(self.b)
        return {"out": [a.cpu().numpy() for a in self.res["out"]], "action": self.res["action"].cpu().numpy(), "logp": self.res["logp"].cpu().numpy()}

    def run(self, env0=0, n=None, stream=None):
        self.b.policy(env0, n, stream=stream)
        return self.download()

    def close(self):
        if self.own:
            self.b.close()


def emulated(case, env0=0, n=None):
    res = case.fresh()
    pe.Call.of_case(case, res).policy(env0, n)
    return res


@pytest.fixture(scope="module")
def shared():
    return cases.shared_case()


@pytest.mark.parametrize("load", ["device", "host"])
def test_shared_case_on_the_device(cassie, shared, load):
    """Every range of the emulator's test, on the device: the restatement's and the emulator's bits, sentinels untouched; the packed
    bytes of either way of loading are the numpy packing's; the output download and the launch counter."""
    d = Device(cassie, shared, load)
    try:
        assert np.array_equal(d.b.policy_packed().view(np.uint32), shared.packed().view(np.uint32))
        for k, n in enumerate(cases.COUNTS):
            d.fresh()
            got, want = d.run(cases.ENV0, n), shared.expected(cases.ENV0, n)
            assert cases.same(got, want), n
            assert np.array_equal(cases.words(got), cases.words(emulated(shared, cases.ENV0, n))), n
            assert d.b.policy_launches() == k + 1
        assert pc.same_bits(d.b.policy_outputs(0), got["out"][0][:, :3]) and pc.same_bits(d.b.policy_outputs(1), got["out"][1][:, :1])
        # a call over a range equals the calls over its halves
        d.fresh()
        whole = d.run(3, 37)
        d.fresh()
        d.b.policy(3, 20)
        assert cases.same(d.run(23, 17), whole)
        d.b.policy(5, 0)
        assert d.b.policy_launches() == len(cases.COUNTS) + 3
    finally:
        d.close()


@pytest.mark.parametrize("make_case", [cases.four_layer_case, cases.one_layer_case, cases.limits_case])
def test_depths_and_limits_on_the_device(cassie, make_case):
    case = make_case()
    d = Device(cassie, case)
    try:
        got = d.run()
        assert np.array_equal(d.b.policy_packed().view(np.uint32), case.packed().view(np.uint32))
        assert cases.same(got, case.expected()) and np.array_equal(cases.words(got), cases.words(emulated(case)))
    finally:
        d.close()


def test_special_values_on_the_device(cassie):
    """z on both sides of +-2^-10, +-0, +-40, +-400, +-inf, float32 subnormal outputs, a bias of -0.0, and a NaN that stays in its env."""
    for case in cases.special_cases() + cases.bias_cases():
        d = Device(cassie, case, "host")
        try:
            got = d.run()
            assert cases.same(got, case.expected()), case.name
            emu = emulated(case)
            finite = [~np.isnan(a) for a in emu["out"]]
            assert all(np.array_equal(g[f].view(np.uint32), e[f].view(np.uint32)) for g, e, f in zip(got["out"], emu["out"], finite)), case.name
        finally:
            d.close()
    case, bad = cases.nan_case()
    d = Device(cassie, case)
    try:
        got, emu = d.run(), emulated(case)
        assert cases.same(got, case.expected())
        keep = np.arange(case.nenv) != bad
        for g, e in zip(got["out"] + [got["action"], got["logp"]], emu["out"] + [emu["action"], emu["logp"]]):
            assert np.array_equal(g[keep].view(np.uint32), e[keep].view(np.uint32))
        assert np.all(np.isnan(got["action"][bad, :3]))
    finally:
        d.close()


def test_vectors_and_weights_read_at_every_call(cassie, shared):
    """mean, inv and log_std changed IN PLACE between two calls, then the weights loaded anew on the call's stream: each call's outputs are
    what the restatement says of what the memory held at the call."""
    import torch
    d = Device(cassie, shared)
    try:
        first = d.run()
        assert cases.same(first, shared.expected())
        mean, inv, clip = shared.norm
        mean2, inv2, ls2 = (mean + F32(0.25)).astype(F32), (inv * F32(0.5)).astype(F32), (shared.log_std - F32(0.5)).astype(F32)
        d.mean.copy_(torch.from_numpy(mean2))
        d.inv.copy_(torch.from_numpy(inv2))
        d.log_std.copy_(torch.from_numpy(ls2))
        changed = cases.Case("changed", shared.nets, shared.rows(shared.x), (mean2, inv2, clip), shared.rows(shared.eps), ls2)
        second = d.run()
        assert cases.same(second, changed.expected()) and not cases.same(second, first)
        # new weights: an "optimiser step" on the device, packed on the stream the call follows on
        nets2 = [([((w * F32(0.75)).astype(F32), (b + F32(0.125)).astype(F32)) for w, b in layers], acts) for layers, acts in shared.nets]
        moved = cases.Case("moved", nets2, shared.rows(shared.x), (mean2, inv2, clip), shared.rows(shared.eps), ls2)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            for layers, new in zip(d.w, moved.weights):
                for (w, b), (w2, b2) in zip(layers, new):
                    w.copy_(torch.from_numpy(w2), non_blocking=False)
                    b.copy_(torch.from_numpy(b2), non_blocking=False)
        d.load("device", stream=st.cuda_stream)
        third = d.run(stream=st.cuda_stream)
        assert cases.same(third, moved.expected()) and not cases.same(third, second)
        assert np.array_equal(d.b.policy_packed().view(np.uint32), moved.packed().view(np.uint32))
    finally:
        d.close()


def test_two_ranges_on_two_streams(cassie, shared):
    import torch
    d = Device(cassie, shared)
    try:
        whole = d.run()
        d.fresh()
        s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
        d.b.policy(0, 21, stream=s0.cuda_stream)
        d.b.policy(21, 27, stream=s1.cuda_stream)
        assert cases.same(d.download(), whole) and cases.same(whole, shared.expected())
    finally:
        d.close()


NOBS = 20


def loop_policy():
    rng = np.random.default_rng(12)
    actor = cases.dense(rng, (NOBS, 32, 10), (P.POL_ELU, P.POL_TANH))
    critic = cases.dense(rng, (NOBS, 16, 1), (P.POL_TANH, P.POL_IDENTITY))
    return [actor, critic]


def test_observe_policy_act_step(cassie):
    """64 envs, 3 policy steps of observe -> policy -> act -> step (50 substeps) on one stream, nothing in between, against the same
    loop with the observation downloaded, the restatement's action computed on the host and uploaded: every bit of qpos, of the actions
    and of the values."""
    import torch
    n, npol = 64, 3
    rng = np.random.default_rng(13)
    nets = loop_policy()
    q0 = np.tile(cassie.qpos_init(), (n, 1))
    q0[:, 2] -= 0.002 * rng.random(n)
    terms = [P.obs_copy(P.F_QPOS, 7, 10, scale=1.0), P.obs_copy(P.F_QVEL, 0, 10, scale=0.1)]
    cols = [P.act_col(P.F_PD_PTARGET, j, lo=-1.5, hi=1.5, offset=float(bench.PD_OFFSET[j]), scale=0.2) for j in range(10)]
    eps = np.clip(rng.normal(size=(npol, n, 10)), -4, 4).astype(F32)
    log_std = np.full(10, -1.5, dtype=F32)
    mean, inv = rng.normal(size=NOBS).astype(F32) * F32(0.1), rng.uniform(0.5, 2, NOBS).astype(F32)
    proto = cases.Case("loop", nets, np.zeros((n, NOBS), dtype=F32), pad=0, wpad=0)

    def run(on_device):
        b = make(cassie, n, P.DRIVE_PD_SAFE, q0)
        try:
            b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
            b.configure_obs(terms, history=1, dtype=np.float32)
            obs_d = torch.zeros((n, NOBS), dtype=torch.float32, device="cuda")
            act_d = torch.zeros((n, 10), dtype=torch.float32, device="cuda")
            val_d, logp_d = torch.zeros((n, 1), dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
            eps_d, ls_d = torch.from_numpy(eps).cuda(), torch.from_numpy(log_std).cuda()
            mean_d, inv_d = torch.from_numpy(mean).cuda(), torch.from_numpy(inv).cuda()
            b.bind_obs(obs_d.data_ptr(), NOBS)
            b.configure_actions(cols, dtype=np.float32)
            b.bind_actions(act_d.data_ptr(), 10, torch.float32)
            if on_device:
                b.configure_policy(proto.defs, NOBS)
                for a, layers in enumerate(proto.weights):
                    b.load_policy(a, layers)
                b.bind_policy_input(obs_d.data_ptr(), NOBS, NOBS, torch.float32)
                b.bind_policy_norm(mean_d.data_ptr(), inv_d.data_ptr(), 5.0)
                b.bind_policy_output(1, val_d.data_ptr(), 1)
            fence(b)
            st = torch.cuda.Stream()
            acts, vals = [], []
            for p in range(npol):
                b.observe(stream=st.cuda_stream)
                if on_device:
                    b.bind_policy_sample(eps_d[p].data_ptr(), ls_d.data_ptr(), act_d.data_ptr(), logp_d.data_ptr())
                    b.policy(stream=st.cuda_stream)
                else:
                    fence(b)
                    res = pc.policy(obs_d.cpu().numpy(), nets, (mean, inv, 5.0), eps[p], log_std)
                    act_d.copy_(torch.from_numpy(res["action"]))
                    val_d.copy_(torch.from_numpy(res["out"][1]))
                    fence(b)
                b.act(stream=st.cuda_stream)
                b.step_range(0, n, 50, st.cuda_stream)
                fence(b)
                acts.append(act_d.cpu().numpy().copy())
                vals.append(val_d.cpu().numpy().copy())
            assert not on_device or b.policy_launches() == npol
            return b.get(P.F_QPOS), np.array(acts), np.array(vals)
        finally:
            b.close()

    (q_dev, a_dev, v_dev), (q_ref, a_ref, v_ref) = run(True), run(False)
    assert pc.same_bits(a_dev, a_ref) and pc.same_bits(v_dev, v_ref)
    assert q_dev.tobytes() == q_ref.tobytes() and np.abs(q_dev - q0).max() > 1e-3
    assert np.abs(a_dev[1] - a_dev[0]).max() > 1e-3


def test_a_call_leaves_the_batch_alone(cassie, shared):
    """A save_states row of every env before and after a policy call in the middle of a loop: byte for byte the same."""
    n = shared.nenv
    b = make(cassie, n, P.DRIVE_PD_SAFE)
    d = None
    try:
        b.set(P.F_PD_PTARGET, np.tile(bench.PD_OFFSET, (n, 1)))
        b.configure_states(n, P.STATE_CORE)
        b.step(20)
        d = Device(cassie, shared, batch=b)
        b.save_states()
        before = b.states()[0].copy()
        got = d.run()
        b.save_states()
        after = b.states()[0]
        assert cases.same(got, shared.expected())
        assert before.tobytes() == after.tobytes() and before.size > 0
    finally:
        b.close()


def test_refusals_with_a_batch(cassie):
    import torch
    case = cases.one_layer_case()
    b = Batch(cassie, case.nenv)
    try:
        with pytest.raises(RuntimeError, match="not configured"):
            b.policy()
        b.configure_policy(case.defs, case.in_dim)
        x = torch.from_numpy(case.x).cuda()
        with pytest.raises(RuntimeError, match="never loaded"):
            b.policy()
        b.load_policy(0, [(w[:, :4], bias) for w, bias in case.weights[0]])
        with pytest.raises(RuntimeError, match="no input bound"):
            b.policy()
        with pytest.raises(ValueError, match="float64 input is refused"):
            b.bind_policy_input(x.data_ptr(), 4, case.x.shape[1], torch.float64)
        b.bind_policy_input(x.data_ptr(), 4, case.x.shape[1], torch.float32)
        with pytest.raises(RuntimeError, match="env range out of bounds"):
            b.policy(1, case.nenv)
        with pytest.raises(ValueError, match="last layer has at most 64 units"):
            b.configure_policy([[P.pol_layer(65)]], 4)
        b.policy()                                # (the refused configure call left the policy as it was)
        b.configure_policy([], 0)
        with pytest.raises(RuntimeError, match="not configured"):
            b.policy()
        assert b.policy_launches() == 1
    finally:
        b.close()
