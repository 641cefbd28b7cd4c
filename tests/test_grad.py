"""Gradient rows (csrc/grad_kernels.h) on the wave emulator against the definition restated in numpy (tests/grad_check.py), BIT FOR BIT on
every word: the gradients, dls, the statistics, the kept activations, the deltas and the fp64 partials.  Also: the negative controls that
show the inputs can tell orders apart, the kept activations against the policy's own outputs, the selects of void positions and a NaN
sample, every branch of the head, the gradients against torch's autograd, the transposed packing, the refusals that need no batch."""
import numpy as np
import pytest

import grad_cases as cases
import grad_check as gc
import grad_emu_py as ge
import policy_cases as pcs
import policy_check as pc
from cassie_amd import phys as P

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    ge.lib()


@pytest.fixture(scope="module")
def shared():
    return cases.shared_case()


@pytest.fixture(scope="module")
def shared_runs(shared):
    """The restatement of the shared case, once per (M, chunk)."""
    return {(m, c): shared.reference(shared.idx(m), c) for m in cases.COUNTS for c in cases.CHUNKS}


@pytest.mark.parametrize("chunk", cases.CHUNKS)
@pytest.mark.parametrize("m", cases.COUNTS)
def test_shared_case(shared, shared_runs, m, chunk):
    """M positions of T nenv = 144 samples, with a repeated, a negative and a too large index from M = 16 on: every word is the
    restatement's; the caller's gradient tensors keep the sentinel between their rows; the stores' padding columns hold +0.0 and the rows
    past the call's chunks are left alone."""
    idx, want = shared.idx(m), shared_runs[(m, chunk)]
    call = ge.Call(shared, chunk)
    dw, db, dls = cases.result_tensors(shared)
    call.bind([[a[:, :-3] for a in per] for per in dw], db, dls)
    got = call.grad(idx)
    assert gc.differing(got, want) == []
    for n in range(len(dw)):
        for l, a in enumerate(dw[n]):
            assert gc.same_bits(a[:, :-3], want["dw"][n][l]) and np.all(a[:, -3:] == cases.FILL) and gc.same_bits(db[n][l], want["db"][n][l])
    assert gc.same_bits(dls, want["dls"])
    mcap = (m + chunk - 1) // chunk * chunk
    for n, (layers, _) in enumerate(shared.p.nets):
        for l in range(len(layers) + 1):
            raw, width = ge.fetch_raw(P.GRAD_ACT, n, l), want["act"][n][l].shape[1]
            assert not raw[:mcap, width:].any() and not np.signbit(raw[:mcap, width:]).any() and np.all(raw[mcap:] == cases.FILL)
            assert not raw[m:mcap].any() and not np.signbit(raw[m:mcap]).any()
        for l in range(len(layers)):
            raw, width = ge.fetch_raw(P.GRAD_DELTA, n, l), want["delta"][n][l].shape[1]
            assert not raw[:mcap, width:].any() and not raw[m:mcap].any() and np.all(raw[mcap:] == cases.FILL)
    assert want["stats"][5] == (2 if m >= 16 else 0) and want["stats"][6] == m and want["stats"][7] == 0
    assert np.all(np.isfinite(want["stats"])) and all(np.all(np.isfinite(a)) for per in want["dw"] for a in per)


def test_any_grid_gives_the_same_words(shared, shared_runs):
    idx = shared.idx(130)
    assert gc.differing(ge.Call(shared, 32).grad(idx, grid=1), shared_runs[(130, 32)]) == []
    assert gc.differing(ge.Call(shared, 32).grad(idx, grid=3), shared_runs[(130, 32)]) == []
    # a larger max_m lays the stores out differently and changes nothing
    assert gc.differing(ge.Call(shared, 32, max_m=130).grad(idx), shared_runs[(130, 32)]) == []


@pytest.mark.parametrize("make,m,chunk", [(cases.four_layer_case, 38, 16), (cases.one_layer_case, 20, 32), (cases.actor_only_case, 37, 32),
                                          (cases.limits_case, 16, 16)])
def test_depths_and_limits(make, m, chunk):
    case = make()
    idx = case.idx(m)
    got, want = ge.Call(case, chunk).grad(idx), case.reference(idx, chunk)
    assert gc.differing(got, want) == []
    assert want["stats"][1] == 0 and np.all(np.isfinite(want["stats"]))          # (no critic in these)


def test_the_order_is_visible(shared, shared_runs):
    """Each wrong reading of the definition differs from the right one on the shared case, in the fp64 partials or in a float32 word:
    otherwise the case could not tell them apart."""
    idx, right = shared.idx(130), shared_runs[(130, 16)]
    words = ("part", "act", "delta", "dw", "db", "dls")
    diff = {}
    for wrong in ("p_desc", "chunk_tree", "u_desc", "prod32"):
        diff[wrong] = [d for d in gc.differing(shared.reference(idx, 16, **{wrong: True}), right) if d.startswith(words)]
        assert diff[wrong] != [], wrong
    assert any(d.startswith("part") for d in diff["p_desc"])                 # the chain over p: in the partials' last bits
    assert any(d.startswith("dw") for d in diff["chunk_tree"])               # the planted pair of opposite samples: in float32 words
    assert "delta[0][1]" in diff["u_desc"]                                   # the twin rows of the actor's last layer: in float32 words
    assert any(d.startswith("part") for d in diff["prod32"])


def test_kept_activations_are_the_policy_outputs(shared, shared_runs):
    """The kept h of every live position is what the policy's restatement gives for that observation row; h_0 is the normalised input."""
    idx, res = shared.idx(130), shared_runs[(130, 32)]
    live = (idx >= 0) & (idx < shared.S)
    x = shared.dense["obs"][np.where(live, idx, 0)]
    out = pc.policy(x, shared.p.nets, shared.p.norm)["out"]
    for n in range(2):
        assert gc.same_bits(res["act"][n][-1][live], out[n][live])
        assert gc.same_bits(res["act"][n][0][live], pc.normalise(x, *shared.p.norm)[live])
        assert all(not a[~live].any() for a in res["act"][n]) and all(not a[~live].any() for a in res["delta"][n])


def with_weights(case, nets):
    import copy
    c = copy.copy(case)
    c.p = copy.copy(case.p)
    c.p.nets = nets
    c.p.weights = [[(c.p.padded(w, c.p.wpad), np.ascontiguousarray(b, dtype=F32)) for w, b in layers] for layers, _ in nets]
    return c


def test_a_void_position_changes_no_sum():
    """One weight of the actor's first layer is +inf: a live sample's unit saturates TANH at +-1 and its delta is exactly 0, while a void
    position's +0.0 input makes NaN of its own sums -- which a select drops.  Every word stays finite, the void rows hold +0.0, and the
    single chunk's partials are those of the same minibatch without the void positions."""
    base = cases.actor_only_case()
    nets = [([(w.copy(), b.copy()) for w, b in layers], acts) for layers, acts in base.p.nets]
    nets[0][0][0][0][3, 2] = np.inf
    case = with_weights(base, nets)
    idx = case.idx(37)
    void = (idx < 0) | (idx >= case.S)
    assert void.sum() == 2
    got, want = ge.Call(case, 48).grad(idx), case.reference(idx, 48)
    assert gc.differing(got, want) == []
    assert np.all(np.isfinite(got["stats"])) and np.all(np.isfinite(got["dls"]))
    for l in range(3):
        assert np.all(np.isfinite(got["dw"][0][l])) and np.all(np.isfinite(got["part"][0][l])) and np.all(np.isfinite(got["delta"][0][l]))
        assert not got["delta"][0][l][void].any() and not got["act"][0][l + 1][void].any()
    assert np.all(np.abs(got["act"][0][1][~void, 3]) == 1)
    dense = ge.Call(case, 48).grad(idx[~void])
    for l in range(3):
        assert gc.same_bits(dense["part"][0][l], got["part"][0][l])
    assert got["stats"][5] == 2 and dense["stats"][5] == 0


def test_a_nan_sample_stays_in_its_rows():
    """A sample with a NaN observation: NaN in its own kept activations and deltas and in the sums it enters -- its chunk's partials, the
    gradients, the statistics -- and in no other position's rows, nor in another chunk's partials."""
    pcase, _ = pcs.nan_case()
    clean = cases.Case(pcs.Case("clean", pcase.nets, pcs.shared_case().rows(pcs.shared_case().x), None, pcase.rows(pcase.eps), pcase.log_std))
    bad = cases.Case(pcs.Case("clean", pcase.nets, pcs.shared_case().rows(pcs.shared_case().x), None, pcase.rows(pcase.eps), pcase.log_std))
    idx = clean.idx(37, special=False)
    victim = int(idx[20])                                     # position 20: chunk 1 of chunks of 16
    bad.dense["obs"][victim] = np.nan
    bad.build()
    got, want, ok = ge.Call(bad, 16).grad(idx), bad.reference(idx, 16), clean.reference(idx, 16)
    assert gc.differing(got, want) == []
    others = np.arange(37) != 20
    for n in range(2):
        for a, c in zip(got["act"][n] + got["delta"][n], ok["act"][n] + ok["delta"][n]):
            assert gc.same_bits(a[others], c[others])
        # (RELU's D selects on h > 0, so a NaN h gives a delta of +0.0 below it: the top delta and every activation are NaN)
        assert all(np.all(np.isnan(a[20])) for a in got["act"][n]) and np.all(np.isnan(got["delta"][n][-1][20]))
        for l in range(len(got["part"][n])):
            pg, pk = got["part"][n][l], ok["part"][n][l]
            assert gc.same_bits(pg[0], pk[0]) and gc.same_bits(pg[2], pk[2]) and np.isnan(pg[1]).any()
            assert np.isnan(got["dw"][n][l]).any()
    assert np.all(np.isnan(got["stats"][:3])) and np.isfinite(got["stats"][4]) and got["stats"][5] == 0


def test_every_branch_of_the_head_occurs(shared, shared_runs):
    """Checked on the restatement's own doubles: the ratio below the clip with both signs of the advantage, above it with both, inside
    it; a RELU unit at exactly 0; an ELU output <= 0 -- and the emulator agrees on that minibatch (test_shared_case)."""
    res = shared_runs[(130, 32)]
    idx = shared.idx(130)
    live = (idx >= 0) & (idx < shared.S)
    ratio, adv = res["ratio"][live], res["adv"][live]
    lo, hi = 1.0 - shared.eps, 1.0 + shared.eps
    assert np.any((ratio < lo) & (adv > 0)) and np.any((ratio < lo) & (adv < 0))
    assert np.any((ratio > hi) & (adv > 0)) and np.any((ratio > hi) & (adv < 0))
    assert np.any((ratio >= lo) & (ratio <= hi))
    assert shared.p.nets[1][1][0] == P.POL_RELU and np.any(res["act"][1][1][live] == 0) and np.any(res["act"][1][1][live] > 0)
    assert shared.p.nets[0][1][1] == P.POL_ELU and np.any(res["act"][0][2][live] <= 0) and np.any(res["act"][0][2][live] > 0)
    inactive = res["s2"][live] < res["s1"][live]
    assert inactive.any() and not inactive.all()
    assert 0 < res["stats"][3] < 1 and res["stats"][2] > 0


def autograd_case(seed):
    rng = np.random.default_rng(seed)
    actor = pcs.dense(rng, (5, 17, 33, 3), (P.POL_TANH, P.POL_ELU, P.POL_IDENTITY))
    critic = pcs.dense(rng, (5, 16, 1), (P.POL_RELU, P.POL_IDENTITY))
    x = rng.normal(size=(cases.NENV, 5)).astype(F32)
    return cases.Case(pcs.Case("autograd", [actor, critic], x, None, None, rng.uniform(-1, 0.5, 3).astype(F32)), seed=seed, lr_noise=0.25)


AUTOGRAD_SEED = 9      # the first seed from 1 up whose float64 reference has no sample on a kink (on_a_kink)
AUTOGRAD_FACTOR = 2.0      # the restatement's error against float64 is at most twice the float32 module's (the issue's bound)


def torch_grads(case, idx, dtype):
    """The same loss as torch.nn.Sequential in `dtype`, gradients by autograd -> (the gradients in the restatement's order as float64
    arrays, the RELU layer's pre-activations, ratio, s1, s2)."""
    import torch
    acts = {P.POL_TANH: torch.nn.Tanh, P.POL_ELU: torch.nn.ELU, P.POL_RELU: torch.nn.ReLU, P.POL_IDENTITY: torch.nn.Identity}
    st = case.stores()
    nets = []
    for layers, kinds in case.p.nets:
        mods = []
        for (w, b), k in zip(layers, kinds):
            lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(dtype)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(w).to(dtype))
                lin.bias.copy_(torch.from_numpy(b).to(dtype))
            mods += [lin, acts[k]()]
        nets.append(torch.nn.Sequential(*mods))
    t = lambda a: torch.from_numpy(np.asarray(a)[idx]).to(dtype)
    ls = torch.from_numpy(case.log_std).to(dtype).requires_grad_(True)
    x, a, logp_old, adv, ret = t(st["obs"]), t(st["action"]), t(st["logp"]), t(st["advn"]), t(st["ret"])
    pre = nets[1][0](x)                                    # the RELU layer's pre-activations
    mu, v = nets[0](x), nets[1](x)[:, 0]
    A = mu.shape[1]
    logp = (-0.5 * (((a - mu) * torch.exp(-ls)) ** 2).sum(1) - ls.sum()) - A * float(gc.H)
    ratio = torch.exp(logp - logp_old)
    s1, s2 = ratio * adv, torch.clamp(ratio, 1.0 - case.eps, 1.0 + case.eps) * adv
    ent = (ls + 0.5 + float(gc.H)).sum()
    loss = -torch.minimum(s1, s2).mean() + case.c_v * 0.5 * ((v - ret) ** 2).mean() - case.c_ent * ent
    loss.backward()
    grads = [p.grad.numpy().astype(F64) for net in nets for m in net if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
    return grads + [ls.grad.numpy().astype(F64)], pre.detach().numpy(), ratio.detach().numpy(), s1.detach().numpy(), s2.detach().numpy()


def on_a_kink(case, pre, ratio, s1, s2):
    """What would make the float64 gradient itself ill-defined: a RELU pre-activation within 1e-3 of 0, a ratio within 1e-3 of a clip
    bound, an s1 == s2 tie outside the clip -> the count of such samples."""
    lo, hi = 1.0 - case.eps, 1.0 + case.eps
    outside = (ratio < lo) | (ratio > hi)
    return int((np.abs(pre) <= 1e-3).sum() + (np.abs(ratio - lo) <= 1e-3).sum() + (np.abs(ratio - hi) <= 1e-3).sum() + (outside & (s1 == s2)).sum())


def test_against_autograd():
    """The same loss as torch.nn.Sequential in float64; autograd gives the gradients.  The yardstick is the same module in float32: its
    largest error against float64, per tensor and relative to the tensor's largest magnitude.  The restatement accumulates in fp64 and
    rounds only activations and deltas to float32, so its error is at most AUTOGRAD_FACTOR times the yardstick.  The seed is chosen on the
    float64 reference alone so that no sample lies on a kink: asserted with zero samples excluded."""
    import torch
    case = autograd_case(AUTOGRAD_SEED)
    idx = np.random.default_rng(2).permutation(case.S).astype(np.int32)
    g64, pre, ratio, s1, s2 = torch_grads(case, idx, torch.float64)
    g32 = torch_grads(case, idx, torch.float32)[0]
    assert on_a_kink(case, pre, ratio, s1, s2) == 0            # on the float64 values, zero samples excluded
    res = case.reference(idx, 32)
    mine = [g.astype(F64) for n in range(2) for l in range(len(res["dw"][n])) for g in (res["dw"][n][l], res["db"][n][l])] + [res["dls"].astype(F64)]
    assert gc.differing(ge.Call(case, 32).grad(idx), res) == []
    worst_y = worst_e = 0.0
    for a, b, c in zip(g64, g32, mine):
        scale = np.abs(a).max()
        yard, err = np.abs(b - a).max() / scale, np.abs(c - a).max() / scale
        print("tensor %s: float32 module %.3e, restatement %.3e" % (a.shape, yard, err))
        worst_y, worst_e = max(worst_y, yard), max(worst_e, err)
        assert err <= AUTOGRAD_FACTOR * yard, (a.shape, err, yard)
    print("largest: float32 module %.3e, restatement %.3e" % (worst_y, worst_e))


def test_transposed_packing(shared):
    for case in (shared, cases.four_layer_case()):
        ge.Call(case, 16).grad(case.idx(16))
        for n, (layers, _) in enumerate(case.p.nets):
            for l, (w, _) in enumerate(layers):
                assert gc.same_bits(ge.fetch(P.GRAD_PACKT, n, l), gc.pack_t(w)), (n, l)
    w = np.arange(5 * 18, dtype=F32).reshape(5, 18) + 1
    t = gc.pack_t(w)
    assert t.shape == (8 * 32,) and t[0] == w[0, 0] and t[1] == w[0, 1] and t[16] == w[1, 0] and t[64] == w[4, 0] and t[80] == 0
    assert t[128] == w[0, 16] and t[130] == 0                       # block 1: k = 16, 17, then the padding


def test_refusals(shared):
    ok = lambda **kw: ge.Call(shared, kw.pop("chunk", 16), **kw)
    idx = shared.idx(16)
    assert ok().check(idx) is None
    for chunk in (0, 8, 24, 4112, 8192):
        assert "chunk is a multiple of 16" in ok(chunk=chunk).check(idx)
    assert ok(chunk=4096).check(idx) is None
    for kw, msg in (({"eps": -0.1}, "clip_eps is finite"), ({"eps": np.inf}, "clip_eps is finite"), ({"c_v": np.nan}, "c_v is finite"),
                    ({"c_v": -1.0}, "c_v is finite"), ({"c_ent": -1e-3}, "c_ent is finite"), ({"c_ent": np.inf}, "c_ent is finite")):
        assert msg in ok(**kw).check(idx), kw
    assert "max_m lies in" in ok(max_m=shared.S + 1).check(idx) and "max_m lies in" in ok(max_m=-1).check(idx)
    assert "not configured" in ok(max_m=0).check(idx)
    assert "m lies in 1 .. max_m" in ok(max_m=16).check(shared.idx(17)) and "m lies in 1 .. max_m" in ok().check(idx, m=0)
    assert "never loaded" in ok(load=False).check(idx)
    for name in ("obs", "action", "logp"):
        assert "OBS, ACTION and LOGP" in ok(skip=(name,)).check(idx)
    assert "no ADVN" in ok(skip=("advn",)).check(idx) and "no RET" in ok(skip=("ret",)).check(idx)
    c = ok()
    c.a.log_std = None
    assert "no log_std" in c.check(idx)
    c = ok()
    dw, db, dls = cases.result_tensors(shared)
    c.bind([[a[:, :-3] for a in per] for per in dw], db, dls)
    c.a.sdw[1] = 3
    assert "dW row stride" in c.check(idx)
    c.a.sdw[1], c.a.db[1] = 64, None
    assert "bound together" in c.check(idx)
    wide = pcs.shared_case()
    two = cases.Case(pcs.Case("wide critic", [wide.nets[0], wide.nets[0]], wide.rows(wide.x), wide.norm, wide.rows(wide.eps), wide.log_std))
    assert "critic's last layer has one unit" in ge.Call(two, 16).check(idx)
