"""What tests/test_model_family.py (the emulator) and tests/test_model_family_gpu.py (the device) share: the family's models and states,
the oracle's results for them -- computed once per member and handed out unchanged --, the conditioning rule that says where the
oracle itself is a usable reference, and the comparisons in the metrics of test_derive_gpu.py's teacher-forced single steps."""
import numpy as np

import family_ref
import model_family as F
from oracle_py import Oracle, arr

BOUNDS = dict(q=1e-12, v=5e-12, a=1e-9, s=1e-9)      # test_derive_gpu.py::test_teacher_forced_single_steps_over_randomised_states
U = 2.0 ** -53
N_SINGLE, N_KIN, N_FUSED, NSUB, TWINS = 64, 16, 8, 40, 8

_cache = {}


def model(member, directory):
    """The member's Model, generated into `directory` and loaded once."""
    from cassie_amd import Model
    key = ("model", member)
    if key not in _cache:
        _cache[key] = Model(F.generate(member, directory))
    return _cache[key]


def states(member, pod, n):
    key = ("states", member, n)
    if key not in _cache:
        _cache[key] = F.sample_states(pod, n, seed=n)
    return _cache[key]


def row_capacity(pod):
    """(fewest, most) constraint rows a state of the model can have: the active connects are always there; the limits, and four rows per
    contact its pairs can give (up to the model's caps), may all be."""
    per = {(0, 2): 1, (0, 3): 2, (0, 6): 4, (2, 2): 1, (2, 3): 1, (2, 6): 1, (3, 3): 1, (3, 6): 2, (6, 6): 4}
    ncon = sum(per[(pod.pair_type[i] & 255, pod.pair_type[i] >> 8)] for i in range(pod.npair))
    lo = 3 * sum(1 for e in range(pod.neq) if pod.eq_active[e])
    return lo, min(pod.maxefc, lo + sum(1 for j in range(pod.njnt) if pod.jnt_limited[j]) + 4 * min(ncon, pod.maxcon))


# ----------------------------------------------------------------------------------------------------- the oracle, one step
def _oracle_step(pod, q, v, ctrl):
    o = Oracle(pod, q)
    o.qvel[:] = v
    o.ctrl[:] = ctrl
    o.step()
    d = o.d
    return dict(q=o.qpos.copy(), v=o.qvel.copy(), a=o.qacc.copy(), s=o.sensordata.copy(), counts=(d.ncon, d.nefc, d.solver_iter),
                caps=(bool(d.warn_contact_full), bool(d.warn_constraint_full)), diverged=bool(d.diverged),
                pairs={(pod.geom_type[d.contact[c].geom1], pod.geom_type[d.contact[c].geom2]) for c in range(d.ncon)})


def _ulp_apart(rng, x):
    x = np.asarray(x, dtype=np.float64)
    return np.nextafter(x, np.where(rng.random(x.shape) < 0.5, -np.inf, np.inf))


def step_errors(pod, ref, q, v, a, s):
    """The four figures of test_derive_gpu.py for one env: (q, v, a, s) of a result against the oracle's `ref`."""
    h = pod.timestep
    return dict(q=float(np.abs(q - ref["q"]).max()),
                v=float(np.abs(v - ref["v"]).max() / max(1.0, np.abs(ref["v"]).max(), h * np.abs(ref["a"]).max())),
                a=float(np.abs(a - ref["a"]).max() / max(1.0, np.abs(ref["a"]).max())),
                s=float((np.abs(s - ref["s"]) / np.maximum(1.0, np.abs(ref["s"]))).max()) if pod.nsensordata else 0.0)


def single_steps(member, pod):
    """-> (q, v, ctrl, refs [n], usable [n]): the member's states, the oracle's step from each, and where the oracle is well conditioned:
    a twin started one ulp away in every component of qvel and ctrl has the same counts and stays within 1/100 of every bound."""
    key = ("single", member)
    if key not in _cache:
        q, v, ctrl = states(member, pod, N_SINGLE)
        rng = np.random.default_rng(5)
        refs, usable = [], np.ones(N_SINGLE, dtype=bool)
        for e in range(N_SINGLE):
            r = _oracle_step(pod, q[e], v[e], ctrl[e])
            t = _oracle_step(pod, q[e], _ulp_apart(rng, v[e]), _ulp_apart(rng, ctrl[e]))
            refs.append(r)
            if r["diverged"]:
                continue
            err = step_errors(pod, r, t["q"], t["v"], t["a"], t["s"])
            usable[e] = t["counts"] == r["counts"] and all(err[k] < BOUNDS[k] / 100 for k in BOUNDS)
        _cache[key] = (q, v, ctrl, refs, usable)
    return _cache[key]


def check_single_steps(member, pod, qg, vg, ag, sg, warn, info):
    """The assertions of the teacher-forced single steps, on the emulator's or the device's results; -> worst error / bound per figure."""
    q, v, ctrl, refs, usable = single_steps(member, pod)
    worst = dict(q=0.0, v=0.0, a=0.0, s=0.0)
    for e, r in enumerate(refs):
        assert tuple(int(x) for x in info[e, :3]) == r["counts"], (member, e, info[e], r["counts"])
        assert (bool(warn[e] & 1), bool(warn[e] & 2)) == r["caps"], (member, e)
        assert bool(warn[e] & 8) == r["diverged"], (member, e)
        if r["diverged"] or not usable[e]:
            continue
        err = step_errors(pod, r, qg[e], vg[e], ag[e], sg[e])
        for k in worst:
            worst[k] = max(worst[k], err[k] / BOUNDS[k])
    rows = [r["counts"][1] for r in refs]
    lo, hi = row_capacity(pod)
    print("%-12s single steps: rows %d .. %d (mean %.1f), %d of %d states left out, worst error / bound %s"
          % (member, min(rows), max(rows), np.mean(rows), int((~usable).sum()), len(refs), {k: "%.2g" % x for k, x in worst.items()}))
    assert (~usable).sum() <= 0.05 * len(refs), (member, int((~usable).sum()))
    # from no row at all to more than half a wavefront of them -- where the model can have that few / that many
    assert min(rows) == lo and (max(rows) > 31 or hi <= 31), (member, min(rows), max(rows), lo, hi)
    assert all(x < 1.0 for x in worst.values()), (member, worst)
    return worst


# ----------------------------------------------------------------------------------------------------- kinematics and M
def kin_reference(member, pod):
    """-> (q [N_KIN], per state the longdouble kinematics and M, the oracle's worst relative errors against them: the baseline)."""
    key = ("kin", member)
    if key not in _cache:
        q = states(member, pod, N_SINGLE)[0][:N_KIN]
        kins = [family_ref.kinematics(pod, q[e]) for e in range(N_KIN)]
        Ms = [family_ref.mass_matrix(pod, k) for k in kins]
        base = dict(xpos=0.0, xquat=0.0, site=0.0, M=0.0)
        for e in range(N_KIN):
            o = Oracle(pod, q[e])
            o.forward()
            err = kin_errors(pod, kins[e], Ms[e], arr(o.d.xpos)[: pod.nbody], arr(o.d.xquat)[: pod.nbody], o.qM)
            if pod.nsite:
                sp, sm = arr(o.d.site_xpos)[: pod.nsite], arr(o.d.site_xmat)[: pod.nsite].reshape(pod.nsite, 3, 3)
                err["site"] = max(float(np.abs(sp - kins[e]["site_xpos"]).max() / max(1.0, np.abs(kins[e]["site_xpos"]).max())),
                                  float(np.abs(sm - kins[e]["site_xmat"]).max()))
            for k, x in err.items():
                base[k] = max(base[k], x)
        _cache[key] = (q, kins, Ms, base)
    return _cache[key]


def kin_errors(pod, kin, M, xpos, xquat, qM):
    """Relative errors against the longdouble reference: xpos over max(1, the largest coordinate), xquat up to its sign, M over its
    largest entry."""
    xq = np.asarray(xquat).reshape(pod.nbody, 4)
    dq = np.minimum(np.abs(xq - kin["xquat"]).max(axis=1), np.abs(xq + kin["xquat"]).max(axis=1))
    return dict(xpos=float(np.abs(np.asarray(xpos).reshape(pod.nbody, 3) - kin["xpos"]).max() / max(1.0, np.abs(kin["xpos"]).max())),
                xquat=float(dq.max()), M=float(np.abs(np.asarray(qM) - M).max() / np.abs(M).max()))


def kin_bound(base, k):
    """100 x the oracle's measured worst (the kernel orders its sums differently and uses the 2-ulp reciprocal), at least 64 u."""
    return max(100.0 * base[k], 64 * U)


def check_kin(member, pod, xpos, xquat, qM):
    """xpos / xquat / M [N_KIN] of the emulator or the device against the longdouble reference; -> worst error / bound per figure."""
    q, kins, Ms, base = kin_reference(member, pod)
    worst = dict(xpos=0.0, xquat=0.0, M=0.0)
    for e in range(N_KIN):
        err = kin_errors(pod, kins[e], Ms[e], xpos[e], xquat[e], qM[e])
        for k in worst:
            worst[k] = max(worst[k], err[k] / kin_bound(base, k))
    print("%-12s kinematics: oracle against longdouble %s, worst error / bound %s"
          % (member, {k: "%.2g" % x for k, x in base.items()}, {k: "%.2g" % x for k, x in worst.items()}))
    assert all(x < 1.0 for x in worst.values()), (member, worst, base)
    return worst


# ----------------------------------------------------------------------------------------------------- fused substeps
def fused_reference(member, pod):
    """-> (q, v, ctrl [N_FUSED], final qpos [N_FUSED] of the oracle after NSUB steps, the last substep's counts, the cap flags any
    substep raised, usable [N_FUSED], spread [N_FUSED]).  Per env TWINS oracle runs, the first from the state itself and the others one
    ulp away in qvel and ctrl: an env is usable where all of them agree on every count of every substep; the spread is the furthest
    any twin's final qpos lies from the first's."""
    key = ("fused", member)
    if key not in _cache:
        q, v, ctrl = states(member, pod, N_FUSED)
        rng = np.random.default_rng(6)
        final, counts, caps = np.zeros_like(q), [], []
        usable, spread = np.ones(N_FUSED, dtype=bool), np.zeros(N_FUSED)
        for e in range(N_FUSED):
            runs = []
            for t in range(TWINS):
                o = Oracle(pod, q[e])
                o.qvel[:] = v[e] if t == 0 else _ulp_apart(rng, v[e])
                o.ctrl[:] = ctrl[e] if t == 0 else _ulp_apart(rng, ctrl[e])
                trace, cap = [], [False, False, False]
                for _ in range(NSUB):
                    o.step()
                    trace.append((o.d.ncon, o.d.nefc, o.d.solver_iter))
                    cap = [cap[0] or bool(o.d.warn_contact_full), cap[1] or bool(o.d.warn_constraint_full), cap[2] or bool(o.d.diverged)]
                runs.append((trace, o.qpos.copy(), cap))
            final[e] = runs[0][1]
            counts.append(runs[0][0][-1])
            caps.append(tuple(runs[0][2]))
            usable[e] = all(r[0] == runs[0][0] for r in runs) and not runs[0][2][2]
            spread[e] = max(float(np.abs(r[1] - runs[0][1]).max()) for r in runs[1:])
        _cache[key] = (q, v, ctrl, final, counts, caps, usable, spread)
    return _cache[key]


def check_fused(member, pod, qg, warn, info):
    """The result of one launch of NSUB fused substeps against the oracle; -> the worst error over its bound."""
    q, v, ctrl, final, counts, caps, usable, spread = fused_reference(member, pod)
    worst = 0.0
    for e in range(N_FUSED):
        # a cap bit only where the oracle raised the flag in some substep (and, where the twins agree, exactly there)
        for bit, k in ((1, 0), (2, 1), (8, 2)):
            assert not (warn[e] & bit) or caps[e][k], (member, e, int(warn[e]), caps[e])
        if not usable[e]:
            continue
        assert (bool(warn[e] & 1), bool(warn[e] & 2)) == caps[e][:2], (member, e, int(warn[e]), caps[e])
        assert tuple(int(x) for x in info[e, :3]) == counts[e], (member, e, info[e], counts[e])
        worst = max(worst, float(np.abs(qg[e] - final[e]).max()) / max(100.0 * spread[e], 1e-13))
    print("%-12s %d fused substeps: %d of %d envs left out, oracle spread up to %.2g, worst error / bound %.2g"
          % (member, NSUB, int((~usable).sum()), N_FUSED, spread.max(), worst))
    assert (~usable).sum() <= 0.1 * N_FUSED, (member, int((~usable).sum()))
    assert worst < 1.0, (member, worst)
    return worst
