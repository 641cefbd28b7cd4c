"""The gradient cases the CPU tests (tests/test_grad.py: the wave emulator) and the GPU tests (tests/test_grad_gpu.py: the device) share, each
against the restatement (tests/grad_check.py) -- test infrastructure only."""
import numpy as np

import grad_check as gc
import policy_cases as pcs
import policy_check as pc
from cassie_amd import phys as P

F32, F64 = np.float32, np.float64
FILL = pcs.FILL
T, NENV = 3, 48
COUNTS = (1, 15, 16, 17, 37, 130)
CHUNKS = (16, 32)
EPS, C_V, C_ENT = 0.2, 0.5, 0.01
KINDS = ("obs", "action", "logp", "value", "advn", "ret")


class Case:
    """A policy (a policy_cases.Case: networks, weights with a row stride, normalisation, log_std) and the arrays of a rollout of T steps
    of nenv envs: per kind [T][nenv][dim] float32 with a row stride larger than the row and a step stride larger than a step's rows, FILL
    between them.  The actions are the policy's own samples, logp_old its log-probabilities moved by lr_noise, so that the ratios spread
    around the clip bounds."""

    def __init__(self, pcase, steps=T, seed=11, lr_noise=0.3, eps=EPS, c_v=C_V, c_ent=C_ENT, twin_actions=False, pair=None):
        rng = np.random.default_rng(seed)
        self.pair = pair
        self.p, self.T, self.nenv = pcase, steps, pcase.nenv
        self.eps, self.c_v, self.c_ent = eps, c_v, c_ent
        self.S = S = steps * self.nenv
        self.A = A = pcase.widths[0]
        self.log_std = pcase.log_std if pcase.log_std is not None else rng.uniform(-1, 0.5, A).astype(F32)
        x0 = pcase.rows(pcase.x)
        # step 0 is the policy case's own rows; the later steps mix them so that the activations stay of the same kind
        obs = np.concatenate([x0] + [(x0[rng.permutation(self.nenv)] * F32(1.0 + 0.25 * t)).astype(F32) for t in range(1, steps)])
        draws = np.clip(rng.normal(size=(S, A)), -3, 3).astype(F32)
        if twin_actions:
            draws[:, 1] = draws[:, 0]
        fwd = pc.policy(obs, pcase.nets, pcase.norm, draws, self.log_std)
        logp = (fwd["logp"].astype(F64) + lr_noise * rng.normal(size=S)).astype(F32)
        self.dense = {"obs": obs, "action": fwd["action"], "logp": logp[:, None], "value": rng.normal(size=(S, 1)).astype(F32),
                      "advn": rng.normal(size=(S, 1)).astype(F32), "ret": rng.normal(size=(S, 1)).astype(F32)}
        if pair is not None:
            # two samples alike in everything but the sign of a large advantage, their ratio inside the clip: their deltas are exact
            # opposites, and idx() puts them into different chunks -- the order the chunks are added in then shows in float32 words
            sa, sb = pair
            for k in ("obs", "action", "value", "ret"):
                self.dense[k][sb] = self.dense[k][sa]
            self.dense["logp"][sa] = self.dense["logp"][sb] = fwd["logp"][sa]
            self.dense["advn"][sa], self.dense["advn"][sb] = F32(2.0 ** 40), F32(-2.0 ** 40)
        self.build()

    def build(self):
        """The padded arrays from self.dense: self.arr[kind] [T][nenv + 1][dim + 2], of which [:, :nenv, :dim] are the rows."""
        self.arr, self.row, self.step = {}, {}, {}
        for k in KINDS:
            d = self.dense[k]
            dim = d.shape[1]
            a = np.full((self.T, self.nenv + 1, dim + 2), FILL, dtype=F32)
            a[:, : self.nenv, :dim] = d.reshape(self.T, self.nenv, dim)
            self.arr[k], self.row[k], self.step[k] = a, dim + 2, (self.nenv + 1) * (dim + 2)

    def stores(self):
        return {k: (v if v.shape[1] > 1 else v[:, 0]) for k, v in self.dense.items()}

    def idx(self, m, seed=3, special=True):
        """m positions: a slice of a permutation of the samples that -- from m = 16 on -- also holds one repeated index, one negative index
        and one index equal to T nenv."""
        rng = np.random.default_rng(seed)
        idx = rng.permutation(self.S)[np.arange(m) % self.S].astype(np.int32)
        if special and m >= 16:
            idx[7], idx[11], idx[13] = idx[2], -1, self.S
        if self.pair is not None:                   # the pair's samples occur at positions 0 and 80 alone
            idx[np.isin(idx, self.pair)] = min(k for k in range(self.S) if k not in self.pair and k not in idx)
            if special and m > 80:
                idx[0], idx[80] = self.pair
        return idx

    def reference(self, idx, chunk, **kw):
        return gc.grad(self.p.nets, self.stores(), idx, chunk, self.eps, self.c_v, self.c_ent, self.p.norm, self.log_std, **kw)


TWIN_UNIT, TWIN_B = 7, F32(2.0 ** 30)


def shared_policy():
    """policy_cases.shared_case with what makes the ORDER of the backward sum over u show in a float32 word: unit TWIN_UNIT of the actor's
    second layer (ELU) has no weights and no bias, so its h is exactly +0.0; the last layer's rows 0 and 1 are equal but for that
    column, where they hold +B and -B; log_std 0 and 1 are equal (and Case draws equal actions for the two).  Then mu_0 = mu_1 and
    gmu_0 = gmu_1 exactly, the two products cancel exactly when they are added first, and whatever is added in between is rounded at
    B gmu's unit."""
    c = pcs.shared_case()
    nets = [([(w.copy(), b.copy()) for w, b in layers], acts) for layers, acts in c.nets]
    (w2, b2), (w3, b3) = nets[0][0][1], nets[0][0][2]
    w2[TWIN_UNIT, :], b2[TWIN_UNIT] = 0.0, 0.0
    w3[1, :], b3[1] = w3[0, :], b3[0]
    w3[0, TWIN_UNIT], w3[1, TWIN_UNIT] = TWIN_B, -TWIN_B
    log_std = c.log_std.copy()
    log_std[1] = log_std[0]
    return pcs.Case("shared", nets, c.rows(c.x), c.norm, c.rows(c.eps), log_std)


def shared_case():
    return Case(shared_policy(), twin_actions=True, pair=(5, 77))


def four_layer_case():
    return Case(pcs.four_layer_case(), steps=2, seed=12)


def one_layer_case():
    return Case(pcs.one_layer_case(), steps=4, seed=13)


def actor_only_case():
    c = shared_policy()
    return Case(pcs.Case("actor only", c.nets[:1], c.rows(c.x), c.norm, c.rows(c.eps), c.log_std), seed=14)


def limits_case():
    return Case(pcs.limits_case(), steps=1, seed=15)


def result_tensors(case):
    """Per network and layer (dW padded [out][in + 3], db [out]) full of FILL, and dls [A]: what a caller binds."""
    dw = [[np.full((w.shape[0], w.shape[1] + 3), FILL, dtype=F32) for w, _ in layers] for layers, _ in case.p.nets]
    db = [[np.full(w.shape[0], FILL, dtype=F32) for w, _ in layers] for layers, _ in case.p.nets]
    return dw, db, np.full(case.A, FILL, dtype=F32)
