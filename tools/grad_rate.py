#!/usr/bin/env python3
"""What the gradient rows cost -- nothing here is a condition, all of it is written down.  One MI355X, one process, the measured networks
(tools/policy_rate.py: actor 340 -> 256 -> 256 -> 10, critic 340 -> 256 -> 256 -> 1, ELU), T = 24 policy steps of 4096 envs by config 2's loop
with every stage in place (tools/rollout_rate.py's rollout leg), then minibatches of M = T nenv / 4 = 24 576 samples, chunk 512.

  grad alone     phys_batch_grad on an idle device, fenced regions; then each of its launches alone (phys_batch_debug_grad_mask: the
                 stores keep what a full call left), the FMAs of the three matrix launches and the fraction of the fp64 matrix rate
                 the measured time amounts to.
  torch          the same loss and backward() in torch fp32 on the same tensors (what a user does today), timed the same way; the
                 largest difference between the two legs' gradients, relative to each tensor's largest magnitude.
  iteration      one whole PPO iteration's device work: the rollout of T steps, finish and normalise, then 5 epochs x 4 minibatches of
                 grad + load_policy of every layer (the optimiser step itself is torch's and is left out of both); the share of it the
                 gradient calls take.
  --parent-lib   the loop ALONE in fresh child processes, parent commit's library and this one, in the order parent, this, this,
                 parent (tools/rollout_rate.py's bare leg): unused, the feature should cost nothing.

Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/grad_rate.py [--envs 4096] [--repeats 10] [--chunk 512] [--out profiles/grad_rate.json] [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import rollout_rate  # noqa: E402  (sets the other paths)
import policy_rate  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

T, NOBS, NACT = rollout_rate.T, rollout_rate.NOBS, rollout_rate.NACT
EPS, C_V, C_ENT, EPOCHS, MINIBATCHES = 0.2, 0.5, 0.01, 5, 4
LAUNCHES = ("forward_and_head", "backward_deltas", "weight_partials", "reduce", "statistics")
H64 = 0.91893853320467267


def stat(us):
    return {"median_us": float(np.median(us)), "min_us": float(min(us)), "max_us": float(max(us)), "regions_us": [float(v) for v in us]}


def timed(call, repeats, reps=3, stream=None):
    """Microseconds of a call on an idle device: `repeats` fenced regions of `reps` calls between two device events on the call's stream."""
    stream = stream or torch.cuda.current_stream()
    out = []
    call()
    torch.cuda.synchronize()
    for _ in range(repeats):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        ev0.record(stream)
        for _ in range(reps):
            call()
        ev1.record(stream)
        torch.cuda.synchronize()
        out.append(1000.0 * ev0.elapsed_time(ev1) / reps)
    return out


def fma_counts(widths_per_net, m):
    """FMAs of the three matrix launches for m positions (padding left out): forward, backward (layers above the first), weight partials
    with the bias column."""
    fwd = sum(m * i * o for w in widths_per_net for i, o in zip(w[:-1], w[1:]))
    bwd = sum(m * i * o for w in widths_per_net for i, o in list(zip(w[:-1], w[1:]))[1:])
    part = sum(m * (i + 1) * o for w in widths_per_net for i, o in zip(w[:-1], w[1:]))
    return fwd, bwd, part


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    n = a.envs
    S, M = T * n, T * n // MINIBATCHES
    out = {"tool": "grad_rate", "model": "cassie", "envs": n, "rollout_steps": T, "minibatch": M, "chunk": a.chunk, "regions": a.repeats,
           "networks": "actor 340-256-256-10, critic 340-256-256-1, ELU", "clip_eps": EPS, "c_v": C_V, "c_ent": C_ENT}
    if a.parent_lib:
        def alone(lib):
            cmd = [sys.executable, os.path.join(REPO, "tools", "rollout_rate.py"), "--only", "bare", "--envs", str(n), "--repeats", str(a.repeats)]
            env = dict(os.environ, CASSIE_LIB=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != "CASSIE_LIB"}
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("a child leg failed:\n" + r.stderr[-2000:])
            return json.loads(r.stdout.strip().splitlines()[-1])["bare"]

        def pooled(runs):
            r = [v for run in runs for v in run["regions"]]
            return {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
                    "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r}

        runs = [alone(lib) for lib in (a.parent_lib, None, None, a.parent_lib)]
        par, own = pooled([runs[0], runs[3]]), pooled([runs[1], runs[2]])
        out["parent_loop"], out["loop_alone"] = par, own
        out["loop_median_over_parent_median"] = own["env_steps_per_s_median"] / par["env_steps_per_s_median"]
        out["loop_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= own["env_steps_per_s_median"] <= par["env_steps_per_s_max"])
    model = Model("cassie")
    leg = rollout_rate.Leg(model, n, "rollout")
    b = leg.b
    try:
        def rollout():
            for _ in range(T):
                leg.launch()

        rollout()
        rollout()
        torch.cuda.synchronize()
        b.configure_grad(M, a.chunk, EPS, C_V, C_ENT)
        perm = torch.from_numpy(np.random.default_rng(3).permutation(S).astype(np.int32)).cuda()
        torch.cuda.synchronize()
        st = leg.streams[0]
        grad = lambda k=0: b.grad(perm.data_ptr() + 4 * M * k, M, st.cuda_stream)
        out["grad_alone"] = stat(timed(grad, a.repeats, stream=st))
        widths = [(NOBS, policy_rate.HIDDEN, policy_rate.HIDDEN, NACT), (NOBS, policy_rate.HIDDEN, policy_rate.HIDDEN, 1)]
        fmas = fma_counts(widths, M)
        per = {}
        for k, name in enumerate(LAUNCHES):
            b.grad_launch_mask(1 << k)
            per[name] = stat(timed(grad, a.repeats, stream=st))
        b.grad_launch_mask(31)
        for name, f in zip(LAUNCHES[:3], fmas):
            per[name]["fma"] = int(f)
            per[name]["fp64_TFLOP_per_s"] = 2.0 * f / (per[name]["median_us"] * 1e-6) / 1e12
        out["launches"] = per
        out["fma_total"] = int(sum(fmas))
        out["fp64_TFLOP_per_s_of_the_call"] = 2.0 * sum(fmas) / (out["grad_alone"]["median_us"] * 1e-6) / 1e12
        out["fp64_matrix_peak_TFLOP_per_s"] = 78.6
        out["fraction_of_the_fp64_matrix_rate"] = out["fp64_TFLOP_per_s_of_the_call"] / 78.6
        grad()
        torch.cuda.synchronize()
        stats = b.grad_stats()
        out["stats"] = {k: float(v) for k, v in stats.items() if k != "all"}
        mine = [b.grad_download(w, net, l) for net in range(2) for l in range(3) for w in (P.GRAD_DW, P.GRAD_DB)] + [b.grad_download(P.GRAD_DLS)]

        # ---- the torch leg: the same loss, fp32, on the same tensors ----
        dev = torch.device("cuda")
        wrng = np.random.default_rng(2)
        Hd = policy_rate.HIDDEN
        nets_np = [policy_rate.weights(wrng, (NOBS, Hd, Hd, NACT)), policy_rate.weights(wrng, (NOBS, Hd, Hd, 1))]
        nets = []
        for net in nets_np:
            mods = []
            for i, (w, bias) in enumerate(net):
                lin = torch.nn.Linear(w.shape[1], w.shape[0], device=dev)
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(w))
                    lin.bias.copy_(torch.from_numpy(bias))
                mods += [lin] + ([torch.nn.ELU()] if i < 2 else [])
            nets.append(torch.nn.Sequential(*mods))
        ls = leg.log_std.clone().requires_grad_(True)
        tens = {k: torch.from_numpy(b.rollout(k).reshape(S, -1)).to(dev) for k in ("obs", "action", "logp", "advn", "ret")}
        params = [p for net in nets for p in net.parameters()] + [ls]
        idx = perm[:M].long()

        def torch_grad():
            for p in params:
                p.grad = None
            x = torch.clamp((tens["obs"][idx] - leg.mean) * leg.inv, -policy_rate.CLIP, policy_rate.CLIP)
            mu, v = nets[0](x), nets[1](x)[:, 0]
            logp = (-0.5 * (((tens["action"][idx] - mu) * torch.exp(-ls)) ** 2).sum(1) - ls.sum()) - NACT * H64
            ratio = torch.exp(logp - tens["logp"][idx, 0])
            adv = tens["advn"][idx, 0]
            loss = -torch.minimum(ratio * adv, torch.clamp(ratio, 1 - EPS, 1 + EPS) * adv).mean() + \
                C_V * 0.5 * ((v - tens["ret"][idx, 0]) ** 2).mean() - C_ENT * (ls + 0.5 + H64).sum()
            loss.backward()

        out["torch_fp32_alone"] = stat(timed(torch_grad, a.repeats))
        torch_grad()
        torch.cuda.synchronize()
        theirs = [p.grad.detach().cpu().numpy().reshape(-1) for net in nets for m in net if isinstance(m, torch.nn.Linear) for p in (m.weight, m.bias)]
        theirs.append(ls.grad.detach().cpu().numpy())
        out["largest_difference_relative_to_each_tensors_largest_magnitude"] = float(max(
            np.abs(x.astype(np.float64) - y.astype(np.float64)).max() / max(np.abs(y).max(), 1e-30) for x, y in zip(mine, theirs)))
        out["grad_over_torch"] = out["grad_alone"]["median_us"] / out["torch_fp32_alone"]["median_us"]

        # ---- the share of an iteration ----
        dw = [[(torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev)) for w, bias in net] for net in nets_np]

        def update():
            for _ in range(EPOCHS):
                for k in range(MINIBATCHES):
                    grad(k)
                    for net, layers in enumerate(dw):
                        b.load_policy(net, [(w.data_ptr(), w.shape[1], bias.data_ptr()) for w, bias in layers], st.cuda_stream)

        def region(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0)

        ro, it = [], []
        for _ in range(a.repeats):
            ro.append(region(rollout))
            it.append(region(lambda: (rollout(), update())))
        out["rollout_region"], out["iteration_region"] = stat(ro), stat(it)
        out["share_of_an_iteration_percent"] = 100.0 * (1.0 - out["rollout_region"]["median_us"] / out["iteration_region"]["median_us"])
        out["grad_launches"] = list(b.grad_launches())
        out["envs_with_warnings"] = int(b.warnings()[0].astype(bool).sum())
    finally:
        leg.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
