"""The policy cases the CPU tests (tests/test_policy.py: the wave emulator) and the GPU tests (tests/test_policy_gpu.py: the device) share,
each against the restatement (tests/policy_check.py) -- test infrastructure only."""
import numpy as np

import policy_check as pc
from cassie_amd import phys as P

F32 = np.float32
FILL = F32(-7.25)                      # the sentinel of rows and padding no call may touch
NENV, ENV0, COUNTS = 48, 3, (1, 15, 16, 17, 37)


def spread(rng, shape):
    """float32 values whose products span many binades (as test_wave_primitives.mfma_inputs)."""
    return (rng.normal(size=shape) * 2.0 ** rng.integers(-4, 5, shape)).astype(F32)


class Case:
    """A policy and its inputs.  nets: [(layers [(W float32 [out][in], b float32 [out])], acts [POL_*])]; x float32 [nenv][in_dim];
    norm: (mean, inv, clip) or None; eps float32 [nenv][A] with log_std float32 [A], or None.  Every bound tensor gets a row stride larger
    than its row (pad), and the weights a row stride larger than `in` (wpad); what lies between the rows holds FILL."""

    def __init__(self, name, nets, x, norm=None, eps=None, log_std=None, pad=2, wpad=3):
        self.name, self.nets, self.norm, self.log_std = name, nets, norm, None if log_std is None else np.asarray(log_std, dtype=F32)
        self.in_dim, self.nenv, self.pad, self.wpad = int(x.shape[1]), int(x.shape[0]), pad, wpad
        self.x = self.padded(x, pad)
        self.eps = None if eps is None else self.padded(eps, pad)
        self.widths = [int(layers[-1][0].shape[0]) for layers, _ in nets]
        self.defs = [[P.pol_layer(w.shape[0], a) for (w, _), a in zip(layers, acts)] for layers, acts in nets]
        # the weights as a caller holds them: rows with a stride
        self.weights = [[(self.padded(w, wpad), np.ascontiguousarray(b, dtype=F32)) for w, b in layers] for layers, _ in nets]

    @staticmethod
    def padded(a, pad):
        a = np.asarray(a, dtype=F32)
        full = np.full((a.shape[0], a.shape[1] + pad), FILL, dtype=F32)
        full[:, : a.shape[1]] = a
        return full

    def rows(self, a):
        """The rows proper of a padded tensor."""
        return a[:, : a.shape[1] - self.pad]

    def fresh(self):
        """The output tensors before a call: FILL everywhere.  {"out": [per network], "action", "logp"}."""
        A = self.widths[0]
        return {"out": [np.full((self.nenv, w + self.pad), FILL, dtype=F32) for w in self.widths],
                "action": np.full((self.nenv, A + self.pad), FILL, dtype=F32), "logp": np.full(self.nenv, FILL, dtype=F32)}

    def expected(self, env0=0, n=None, **kw):
        """What a call over [env0, env0 + n) leaves in fresh() tensors, by the restatement.  kw: policy_check.layer's wrong readings."""
        n = self.nenv - env0 if n is None else n
        res, want = self.reference(env0, n, **kw), self.fresh()
        for a, w in enumerate(self.widths):
            want["out"][a][env0: env0 + n, :w] = res["out"][a]
        if self.eps is not None:
            want["action"][env0: env0 + n, : self.widths[0]] = res["action"]
            want["logp"][env0: env0 + n] = res["logp"]
        return want

    def reference(self, env0, n, **kw):
        x = self.rows(self.x)[env0: env0 + n]
        eps = None if self.eps is None else self.rows(self.eps)[env0: env0 + n]
        return pc.policy(x, self.nets, self.norm, eps, self.log_std, **kw)

    def packed(self):
        """The packed floats of the whole policy, by the numpy packing."""
        return np.concatenate([pc.pack(w, b) for layers, _ in self.nets for w, b in layers])


def words(res):
    """Every float32 word a call writes or leaves, as one uint32 array."""
    return np.concatenate([a.reshape(-1) for a in res["out"]] + [res["action"].reshape(-1), res["logp"]]).view(np.uint32)


def same(got, want):
    """Bit for bit on every float32 word (a NaN equal to any NaN), sentinels included."""
    return all(pc.same_bits(g, w) for g, w in zip(got["out"], want["out"])) and pc.same_bits(got["action"], want["action"]) and \
        pc.same_bits(got["logp"], want["logp"])


def dense(rng, widths, acts):
    """(layers, acts) of a network in -> widths[1:] with spread weights scaled to keep the activations of order one."""
    layers = []
    for i, o in zip(widths[:-1], widths[1:]):
        layers.append(((spread(rng, (o, i)) / F32(4.0 * np.sqrt(i))).astype(F32), spread(rng, (o,)) / F32(8.0)))
    return layers, list(acts)


def shared_case():
    """in_dim 5; actor 5 -> 17 -> 33 -> 3 (TANH, ELU, IDENTITY); critic 5 -> 16 -> 1 (RELU, IDENTITY); a normalisation whose clip bites;
    sampling.  So that the ORDER of a sum shows in float32 words (fp64 sums differ in their last bit only, which a conversion to float32
    hides): input elements 0 and 1 of most envs lie beyond the clip on the same side -- both become exactly c -- and the first layers'
    weights of the two are +-B with B around 2^28: the two products cancel exactly, and what is summed in between is rounded at B c's
    unit, 2^-22 of the result or so."""
    rng = np.random.default_rng(20261021)
    actor = dense(rng, (5, 17, 33, 3), (P.POL_TANH, P.POL_ELU, P.POL_IDENTITY))
    critic = dense(rng, (5, 16, 1), (P.POL_RELU, P.POL_IDENTITY))
    for layers, _ in (actor, critic):
        w = layers[0][0]
        w[:, 0] = (spread(rng, (w.shape[0],)) * F32(2.0 ** 28)).astype(F32)
        w[:, 1] = -w[:, 0]
    mean, std = rng.normal(size=5).astype(F32), rng.uniform(0.5, 2.0, 5).astype(F32)
    inv, clip = (F32(1.0) / std).astype(F32), 2.5
    x = (mean + std * rng.normal(size=(NENV, 5)) * 1.5).astype(F32)           # elements 2 .. 4: the clip bites now and then
    side = np.where(rng.random(NENV) < 0.5, -1.0, 1.0)
    x[:, 0] = mean[0] + std[0] * side * rng.uniform(4.0, 9.0, NENV)
    x[:, 1] = mean[1] + std[1] * side * rng.uniform(4.0, 9.0, NENV)
    x[::6, 1] = mean[1] - std[1] * side[::6] * 5.0                            # every sixth env: opposite sides, nothing cancels
    eps = np.clip(rng.normal(size=(NENV, 3)), -4, 4).astype(F32)
    log_std = rng.uniform(-2, 2, 3).astype(F32)
    return Case("shared", [actor, critic], x, (mean, inv, clip), eps, log_std)


def four_layer_case():
    rng = np.random.default_rng(4)
    net = dense(rng, (9, 20, 7, 50, 5), (P.POL_ELU, P.POL_TANH, P.POL_RELU, P.POL_TANH))
    return Case("four layers", [net], spread(rng, (19, 9)) / F32(4))


def one_layer_case():
    rng = np.random.default_rng(5)
    return Case("one layer", [dense(rng, (4, 1), (P.POL_IDENTITY,))], spread(rng, (5, 4)))


def limits_case():
    """512 -> 512 -> 512 -> 512 -> 64 on 16 envs."""
    rng = np.random.default_rng(6)
    net = dense(rng, (512, 512, 512, 512, 64), (P.POL_ELU, P.POL_TANH, P.POL_ELU, P.POL_IDENTITY))
    return Case("limits", [net], spread(rng, (16, 512)) / F32(4), pad=1, wpad=1)


Z_VALUES = np.array([2.0 ** -10, -2.0 ** -10, np.nextafter(F32(2.0 ** -10), F32(1)), np.nextafter(F32(2.0 ** -10), F32(0)),
                     -np.nextafter(F32(2.0 ** -10), F32(1)), -np.nextafter(F32(2.0 ** -10), F32(0)), 0.0, -0.0, 40.0, -40.0, 400.0, -400.0,
                     1e-30, -1e-30, 1e-40, -1e-40, 2.0 ** -30, -1.5 * 2.0 ** -33, 0.3, -0.3, 9.0, -9.0, 18.5, -18.5, np.inf, -np.inf], dtype=F32)


def special_cases():
    """One-layer networks of `in` 4 whose z IS the env's input element 0 (w = (1, -0, -0, -0) with a bias of -0.0: every other product
    is -0.0, so that z = -0.0 arrives), through every activation; unit 1 scales by 2^-100 into the float32 subnormals and below."""
    w = np.array([[1.0, -0.0, -0.0, -0.0], [2.0 ** -100, -0.0, -0.0, -0.0]], dtype=F32)
    b = np.array([-0.0, -0.0], dtype=F32)
    x = np.zeros((len(Z_VALUES), 4), dtype=F32)
    x[:, 0] = Z_VALUES
    net = lambda a: ([(w.copy(), b.copy())], [a])
    return [Case("tanh, elu", [net(P.POL_TANH), net(P.POL_ELU)], x), Case("relu, identity", [net(P.POL_RELU), net(P.POL_IDENTITY)], x)]


def bias_cases():
    """A bias of -0.0 with in 5 (the padding's +0.0 products turn it into +0.0) and with in 8 (products of -0.0 alone: it stays)."""
    out = []
    for kin in (5, 8):
        w, b = np.full((2, kin), -1.0, dtype=F32), np.array([-0.0, -0.0], dtype=F32)
        out.append(Case("bias -0.0, in %d" % kin, [([(w, b)], [P.POL_IDENTITY])], np.zeros((3, kin), dtype=F32)))
    return out


def nan_case():
    """The shared case without the cancelling columns' clip (no normalisation), env 5's input NaN, +inf, -inf, 1, NaN."""
    c = shared_case()
    x = c.rows(c.x).copy()
    x[5] = [np.nan, np.inf, -np.inf, 1.0, np.nan]
    return Case("nan", c.nets, x, None, c.rows(c.eps), c.log_std), 5
