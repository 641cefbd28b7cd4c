"""Policy rows (csrc/policy_kernels.h) on the wave emulator against the definition restated in numpy (tests/policy_check.py), BIT FOR BIT on
float32 words: weights and activations are float32, every product is exact in a double and every fma one rounding, so the order of a sum
is the only freedom -- and the definition fixes it.  Also: the negative controls that show the inputs can tell orders apart, the
activations against mpmath, the layout against torch's linear, the sample against torch's Normal, every refusal, the packed bytes."""
import numpy as np
import pytest

import policy_cases as cases
import policy_check as pc
import policy_emu_py as pe
from cassie_amd import phys as P

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    pe.lib()


@pytest.fixture(scope="module")
def shared():
    return cases.shared_case()


def run(case, env0=0, n=None, grid=0, res=None):
    res = case.fresh() if res is None else res
    pe.Call.of_case(case, res).policy(env0, n, grid)
    return res


@pytest.mark.parametrize("n", cases.COUNTS)
def test_shared_case(shared, n):
    """n envs from env0 = 3 of a batch of 48: the outputs, the action and logp are the restatement's, and every row outside the range
    and every word between two rows still holds the sentinel."""
    got, want = run(shared, cases.ENV0, n), shared.expected(cases.ENV0, n)
    assert cases.same(got, want)
    assert np.all(got["logp"][: cases.ENV0] == cases.FILL) and np.all(got["out"][0][cases.ENV0 + n:] == cases.FILL)
    assert np.all(got["action"][:, shared.widths[0]:] == cases.FILL) and np.all(got["out"][1][:, 1:] == cases.FILL)
    written = got["out"][0][cases.ENV0: cases.ENV0 + n, :3]
    assert not np.any(written == cases.FILL) and np.all(np.isfinite(written))


def test_a_call_equals_the_calls_over_its_halves_on_any_grid(shared):
    whole = run(shared, 3, 37)
    halves = run(shared, 23, 17, res=run(shared, 3, 20))
    one = run(shared, 3, 37, grid=1)
    assert pe.grid(37) == 3 and pe.grid(37, 2) == 6 and pe.grid(16) == 1 and pe.grid(0, 2) == 0 and pe.grid(16 * 5000) == pe.POLICY_GRID
    assert cases.same(whole, halves) and cases.same(whole, one) and cases.same(whole, run(shared, 3, 37, grid=2))


@pytest.mark.parametrize("make", [cases.four_layer_case, cases.one_layer_case, cases.limits_case])
def test_depths_and_limits(make):
    case = make()
    assert cases.same(run(case), case.expected())


def test_special_values():
    """z on both sides of +-2^-10, +-0, +-40, +-400, +-inf, values whose outputs are float32 subnormals; a bias of -0.0."""
    for case in cases.special_cases():
        got, want = run(case), case.expected()
        assert cases.same(got, want), case.name
    tanh_elu = run(cases.special_cases()[0])
    z = cases.Z_VALUES
    t, e = tanh_elu["out"][0][:, 0], tanh_elu["out"][1][:, 0]
    assert t[z == 400][0] == 1 and t[z == -400][0] == -1 and e[z == -400][0] == -1 and e[z == 400][0] == 400
    assert np.signbit(e[7]) and e[7] == 0 and z[7] == 0 and np.signbit(z[7])          # ELU(-0.0) = -0.0
    ident = run(cases.special_cases()[1])["out"][1]
    sub = ident[z == F32(2.0 ** -30)][0, 1]                                           # 2^-30 * 2^-100: a float32 subnormal
    assert 0 < sub < np.finfo(F32).tiny and sub == F32(2.0 ** -130) and ident[z == F32(1e-40)][0, 0] == F32(1e-40)
    assert ident[z == F32(-1.5 * 2.0 ** -33)][0, 1] == F32(-1.5 * 2.0 ** -133)
    b5, b8 = (run(c)["out"][0][:, :2] for c in cases.bias_cases())
    assert np.all(b5 == 0) and not np.any(np.signbit(b5)) and np.all(b8 == 0) and np.all(np.signbit(b8))
    for c in cases.bias_cases():
        assert cases.same(run(c), c.expected())


def test_a_nan_stays_in_its_env():
    case, bad = cases.nan_case()
    clean = cases.Case("clean", case.nets, np.where(np.isfinite(case.rows(case.x)), case.rows(case.x), F32(1.0)), None, case.rows(case.eps), case.log_std)
    got, ref = run(case), run(clean)
    assert cases.same(got, case.expected())
    keep = np.arange(case.nenv) != bad
    for a, b in zip(got["out"] + [got["action"]], ref["out"] + [ref["action"]]):
        assert np.array_equal(a[keep].view(np.uint32), b[keep].view(np.uint32))
        assert np.any(np.isnan(a[bad, : a.shape[1] - case.pad]))
    assert np.array_equal(got["logp"].view(np.uint32), ref["logp"].view(np.uint32))    # (logp reads eps and log_std alone)


def test_negative_controls(shared):
    """Another order of k, or float32 accumulation, changes more than a tenth of the words the shared case writes: its inputs can tell
    the definition from its neighbours."""
    env0, n = cases.ENV0, 37
    got = run(shared, env0, n)
    rows = lambda r: np.concatenate([a[env0: env0 + n, : a.shape[1] - shared.pad].reshape(-1) for a in r["out"] + [r["action"]]] + [r["logp"][env0: env0 + n]]).view(np.uint32)
    for kw in (dict(descending=True), dict(acc32=True)):
        other = shared.expected(env0, n, **kw)
        assert np.mean(rows(got) != rows(other)) > 0.1, kw
    assert np.array_equal(rows(got), rows(shared.expected(env0, n)))


def activation_points():
    edge = 2.0 ** -10
    near = np.concatenate([edge * (1 + np.linspace(-0.01, 0.01, 401)), np.linspace(-4 * edge, 4 * edge, 801)])
    wide = np.concatenate([np.linspace(-50, 50, 1001), np.linspace(-2, 2, 801), 10.0 ** np.linspace(-30, -3, 200), -(10.0 ** np.linspace(-30, -3, 200))])
    return np.unique(np.concatenate([near, -near, wide, [0.0]]).astype(F32))


def test_activations_against_mpmath():
    """TANH and ELU of a few thousand float32 points, dense around +-2^-10 and 0, out to +-50: within 1 float32 ulp of the exact value
    (the fp64 value is within 2^-34 relative by the definition's branches and expn's 1.06 ulp; the conversion adds half an ulp)."""
    import mpmath
    mpmath.mp.dps = 60
    z = activation_points()
    assert 3000 < z.size < 6000
    w, b = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=F32), np.zeros(1, dtype=F32)
    x = np.zeros((z.size, 4), dtype=F32)
    x[:, 0] = z
    case = cases.Case("activations", [([(w, b)], [P.POL_TANH]), ([(w, b)], [P.POL_ELU])], x)
    got = run(case)
    assert cases.same(got, case.expected())
    exact = {0: lambda v: mpmath.tanh(v), 1: lambda v: v if v >= 0 else mpmath.expm1(v)}
    for net in (0, 1):
        worst = 0.0
        for zi, gi in zip(z, got["out"][net][:, 0]):
            t = exact[net](mpmath.mpf(float(zi)))
            ulp = mpmath.mpf(2) ** max(int(mpmath.floor(mpmath.log(abs(t), 2))) - 23, -149) if t != 0 else mpmath.mpf(2) ** -149
            worst = max(worst, float(abs(mpmath.mpf(float(gi)) - t) / ulp))
        assert worst <= 1.0, (net, worst)


def test_layout_against_torch_linear():
    """One IDENTITY layer 37 -> 19 against torch.nn.functional.linear on the CPU in float32: within fp32 summation's own error bound,
    (in + 2) 2^-24 (|b| + sum |w| |x|) -- so [out][in] is read as torch writes it."""
    import torch
    rng = np.random.default_rng(8)
    w, b, x = rng.normal(size=(19, 37)).astype(F32), rng.normal(size=19).astype(F32), rng.normal(size=(21, 37)).astype(F32)
    lin = torch.nn.Linear(37, 19)
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(w))
        lin.bias.copy_(torch.from_numpy(b))
        ref = torch.nn.functional.linear(torch.from_numpy(x), lin.weight, lin.bias).numpy()
    case = cases.Case("layout", [([(lin.weight.detach().numpy(), lin.bias.detach().numpy())], [P.POL_IDENTITY])], x)
    got = run(case)["out"][0][:, :19]
    bound = (37 + 2) * 2.0 ** -24 * (np.abs(b)[None, :].astype(F64) + np.abs(x).astype(F64) @ np.abs(w).astype(F64).T)
    assert np.all(np.abs(got.astype(F64) - ref.astype(F64)) <= bound)
    assert not np.all(np.abs(run(cases.Case("t", [([(np.ascontiguousarray(w.T[:19, :19]), b)], [P.POL_IDENTITY])], x[:, :19]))["out"][0][:, :19].astype(F64)
                             - ref.astype(F64)) <= bound)     # (the bound can tell a transposed reading apart)


def test_sample_against_torch_normal(shared):
    """a and logp are the restatement's bits (test_shared_case); logp is also torch's Normal(mu, exp(log_std)).log_prob(a).sum(-1) within
    A 2^-20, the float32 arithmetic of torch's own formula, for |eps| <= 4 and |log_std| <= 2."""
    import torch
    got = run(shared)
    A = shared.widths[0]
    mu, a, logp = (torch.from_numpy(v.copy()) for v in (got["out"][0][:, :A], got["action"][:, :A], got["logp"]))
    assert np.abs(shared.rows(shared.eps)).max() <= 4 and np.abs(shared.log_std).max() <= 2
    ref = torch.distributions.Normal(mu, torch.exp(torch.from_numpy(shared.log_std))).log_prob(a).sum(-1)
    assert float((ref - logp).abs().max()) <= A * 2.0 ** -20
    std = np.exp(shared.log_std.astype(F64))
    assert np.allclose(a.numpy(), mu.numpy() + std * shared.rows(shared.eps), rtol=1e-6, atol=1e-6)


def test_packed_weights(shared):
    """The pack kernel's bytes are the numpy packing's: per block of 16 units and k-step of 4, the 64 words in lane order, zero-padded."""
    got, offs = pe.Call.of_case(shared).packed()
    want = shared.packed()
    assert got.size == want.size == sum(((o + 15) & ~15) * (((i + 3) & ~3) + 1) for i, o in ((5, 17), (17, 33), (33, 3), (5, 16), (16, 1)))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert tuple(offs[0]) == (0, 32 * 8, 8, 32) and tuple(offs[4]) == (int(offs[2][1]) + 16, int(offs[4][0]) + 16 * 8, 8, 16)
    w0 = shared.nets[0][0][0][0]
    assert got[0] == w0[0, 0] and got[1] == w0[1, 0] and got[16] == w0[0, 1] and got[64] == w0[0, 4] and got[64 + 16] == 0   # k = 5: padding


def test_lds_follows_the_widths():
    """A workgroup's two buffers hold what the widest input and outputs need, 64 bytes a row: 64 KiB at the limits, under the 40 KiB of
    a step workgroup for 340 -> 256 -> 256 -> 10 beside 340 -> 256 -> 256 -> 1."""
    L = P.pol_layer
    assert pe.Call([[L(512), L(512), L(512), L(64)]], 512, 16).lds_bytes() == 65536
    assert pe.Call([[L(256), L(256), L(10)], [L(256), L(256), L(1)]], 340, 16).lds_bytes() == (340 + 256) * 64 < 40960
    assert pe.Call([[L(17), L(33), L(3)], [L(16), L(1)]], 5, 16).lds_bytes() == (48 + 32) * 64
    assert pe.Call([[L(1)]], 4, 16).lds_bytes() == (4 + 16) * 64


def refusal(defs, in_dim=5, **kw):
    return pe.Call(defs, in_dim, 8, **kw).check()


def test_refusals():
    L = P.pol_layer
    ok = [[L(7, P.POL_TANH), L(3)], [L(1)]]
    assert refusal(ok) is None
    assert "1 or 2 networks" in refusal(ok + [[L(1)]])
    assert "1 .. 4 layers" in refusal([[L(4)] * 5])
    assert "1 .. 4 layers" in refusal([[]])
    assert "in_dim lies in 1 .. 512" in refusal(ok, in_dim=0) and "in_dim lies in 1 .. 512" in refusal(ok, in_dim=513)
    assert "width lies in 1 .. 512" in refusal([[L(513), L(3)]]) and "width lies in 1 .. 512" in refusal([[L(0), L(3)]])
    assert "activation is PHYS_POL_IDENTITY" in refusal([[L(7, 4)]]) and "activation" in refusal([[L(7, -1)]])
    assert "first layer reads in_dim" in refusal([[(6, 7, 0), (7, 3, 0)]])
    assert "as many elements as the layer before it has units" in refusal([[(5, 7, 0), (8, 3, 0)]])
    assert "last layer has at most 64 units" in refusal([[L(7), L(65)]])
    assert refusal([[L(512), L(64)]], in_dim=512) is None
    # the loads
    c = pe.Call(ok, 5, 8)
    w, b = np.zeros((7, 5), dtype=F32), np.zeros(7, dtype=F32)
    assert c.load_check(0, 0, w, 5, b) is None
    assert "row stride of at least the layer's in" in c.load_check(0, 0, w, 4, b)
    assert "no such network or layer" in c.load_check(0, 2, w, 5, b) and "no such network or layer" in c.load_check(2, 0, w, 5, b)
    assert "needs its weights and its biases" in c.load_check(0, 0, w, 5, None)
    assert "not configured" in pe.Call([], 5, 8).load_check(0, 0, w, 5, b)
    # the bindings
    x = np.zeros((8, 7), dtype=F32)

    def bound(f):
        c = pe.Call(ok, 5, 8)
        f(c)
        return c.check()
    assert bound(lambda c: c.bind_input(x[:, :5])) is None
    assert "float64 input is refused" in bound(lambda c: c.bind_input(x[:, :5], dtype=8))
    assert "PHYS_OBS_F32" in bound(lambda c: c.bind_input(x[:, :5], dtype=2))
    assert "hold in_dim elements" in bound(lambda c: c.bind_input(x[:, :6]))
    assert "row stride of at least the row" in bound(lambda c: c.bind_input(x[:, :5], stride=4))
    m = np.zeros(5, dtype=F32)
    assert bound(lambda c: c.bind_norm(m, m, np.inf)) is None and bound(lambda c: c.bind_norm(m, m, 0.0)) is None
    assert "clip is >= 0 or +inf" in bound(lambda c: c.bind_norm(m, m, -1.0)) and "clip is >= 0" in bound(lambda c: c.bind_norm(m, m, np.nan))
    assert "needs its mean and its inv" in bound(lambda c: c.bind_norm(m, None, 1.0))
    assert "at least the network's output width" in bound(lambda c: c.bind_output(0, x[:, :3], stride=2))
    assert bound(lambda c: c.bind_output(1, x[:, :1])) is None
    lp = np.zeros(8, dtype=F32)
    assert bound(lambda c: c.bind_sample(x[:, :3], m, x[:, :3], lp)) is None
    assert "at least the actor's output width" in bound(lambda c: c.bind_sample(x[:, :3], m, x[:, :3], lp, eps_stride=2))
    assert "at least the actor's output width" in bound(lambda c: c.bind_sample(x[:, :3], m, x[:, :3], lp, action_stride=2))
    assert "needs eps, log_std, the action tensor and logp" in bound(lambda c: c.bind_sample(x[:, :3], m, None, lp))
    assert "not configured" in pe.Call([], 5, 8).check(call=True, configured=False)
    # the call
    case = cases.one_layer_case()
    full = pe.Call.of_case(case, case.fresh())
    assert full.check(call=True, env0=0, n=case.nenv) is None and full.check(call=True, env0=2, n=0) is None
    assert "env range out of bounds" in full.check(call=True, env0=1, n=case.nenv) and "env range" in full.check(call=True, env0=-1, n=1)
    assert "never loaded" in pe.Call.of_case(case, case.fresh(), load=False).check(call=True, n=1)
    assert "no input bound" in pe.Call.of_case(case, None, bind=False).check(call=True, n=1)
    two = cases.shared_case()
    part = pe.Call.of_case(two, two.fresh(), load=False)
    for n, layers in enumerate(two.weights):
        for l, (w2, b2) in enumerate(layers):
            if (n, l) != (1, 1):
                part.load(n, l, w2[:, : w2.shape[1] - two.wpad], b2)
    assert "never loaded" in part.check(call=True, n=1)
