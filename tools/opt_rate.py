#!/usr/bin/env python3
"""What the optimiser rows cost -- nothing here is a condition, all of it is written down.  One MI355X, one process, tools/grad_rate.py's
method and set-up: the measured networks (actor 340 -> 256 -> 256 -> 10, critic 340 -> 256 -> 256 -> 1, ELU), T = 24 policy steps of 4096
envs with every stage in place, minibatches of M = T nenv / 4 samples, chunk 512; fenced regions between device events on the call's stream.

  opt_step alone   phys_batch_opt_step on an idle device behind one grad call, lr = 0 (the weights stay, every launch does its whole
                   work); then each of its launches alone (phys_batch_debug_opt_mask: the doubles keep what a full call left).
  torch            on the same tensors: clip_grad_norm_ + torch.optim.Adam.step() with torch's default path, the same with fused=True
                   where this torch build accepts it, each alone and followed by load_policy of all six layers with the gradient rows
                   configured (what a user does today); the largest relative difference between the two legs' weights after 20 steps.
  iteration        one PPO iteration's device work, 5 epochs x 4 minibatches: grad + optimizer.step() + load_policy (the parent's way)
                   against grad + opt_step; the share of the iteration the update takes in both.
  --parent-lib     the loop ALONE in fresh child processes, parent commit's library and this one, in the order parent, this, this,
                   parent (tools/rollout_rate.py's bare leg): unused, the feature should cost nothing.

Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/opt_rate.py [--envs 4096] [--repeats 10] [--chunk 512] [--out profiles/opt_rate.json] [--parent-lib PATH]
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

import grad_rate  # noqa: E402  (sets the other paths)
import rollout_rate  # noqa: E402
import policy_rate  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Model  # noqa: E402

T, NOBS, NACT = rollout_rate.T, rollout_rate.NOBS, rollout_rate.NACT
EPS, C_V, C_ENT, EPOCHS, MINIBATCHES = grad_rate.EPS, grad_rate.C_V, grad_rate.C_ENT, grad_rate.EPOCHS, grad_rate.MINIBATCHES
BETA1, BETA2, ADAM_EPS, MAX_NORM, LR = 0.9, 0.999, 1e-8, 0.5, 3e-4
stat, timed = grad_rate.stat, grad_rate.timed


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
    out = {"tool": "opt_rate", "model": "cassie", "envs": n, "rollout_steps": T, "minibatch": M, "chunk": a.chunk, "regions": a.repeats,
           "networks": "actor 340-256-256-10, critic 340-256-256-1, ELU", "beta1": BETA1, "beta2": BETA2, "eps": ADAM_EPS, "max_norm": MAX_NORM,
           "lr": LR}
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
        dev = torch.device("cuda")
        Hd = policy_rate.HIDDEN
        wrng = np.random.default_rng(2)
        nets_np = [policy_rate.weights(wrng, (NOBS, Hd, Hd, NACT)), policy_rate.weights(wrng, (NOBS, Hd, Hd, 1))]
        slots = [(net, l) for net in range(2) for l in range(3)]
        out["parameters"] = int(sum(w.size + bias.size for net in nets_np for w, bias in net) + NACT)
        # the master tensors of the library's leg, and torch's own copies: torch.nn.Parameter, .grad the tensors grad() writes
        mine = [[(torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev)) for w, bias in net] for net in nets_np]
        params = [torch.nn.Parameter(t.clone()) for net in mine for pair in net for t in pair] + [torch.nn.Parameter(leg.log_std.clone())]
        for p in params:
            p.grad = torch.zeros_like(p)
        b.configure_grad(M, a.chunk, EPS, C_V, C_ENT)
        for k, (net, l) in enumerate(slots):
            b.bind_grad(net, l, params[2 * k].grad.data_ptr(), params[2 * k].shape[1], params[2 * k + 1].grad.data_ptr())
        b.bind_grad_log_std(params[-1].grad.data_ptr())
        perm = torch.from_numpy(np.random.default_rng(3).permutation(S).astype(np.int32)).cuda()
        st = leg.streams[0]
        grad = lambda k=0: b.grad(perm.data_ptr() + 4 * M * k, M, st.cuda_stream)

        def load(tensors):
            for net in range(2):
                b.load_policy(net, [(w.data_ptr(), w.shape[1], bias.data_ptr()) for w, bias in tensors[net]], st.cuda_stream)

        theirs = [[(params[2 * (3 * net + l)].data, params[2 * (3 * net + l) + 1].data) for l in range(3)] for net in range(2)]
        load(mine)
        b.configure_opt(BETA1, BETA2, ADAM_EPS, MAX_NORM)
        for net, l in slots:
            w, bias = mine[net][l]
            b.bind_opt_param(net, l, w.data_ptr(), w.shape[1], bias.data_ptr())
        b.bind_opt_log_std(leg.log_std.data_ptr())
        grad()
        torch.cuda.synchronize()

        # ---- opt_step alone (lr 0: the weights stay, every launch does its whole work) ----
        step = lambda lr=0.0: b.opt_step(lr, st.cuda_stream)
        out["opt_step_alone"] = stat(timed(step, a.repeats, stream=st))
        out["opt_stats"] = {k: float(v) for k, v in b.opt_stats().items() if k != "all"}
        per = {}
        for k, name in enumerate(("squares", "scalars", "step")):
            b.opt_launch_mask(1 << k)
            per[name] = stat(timed(step, a.repeats, stream=st))
        b.opt_launch_mask(7)
        out["launches"] = per

        # ---- the torch leg on the same gradients ----
        def torch_leg(fused):
            kw = {"fused": True} if fused else {}
            opt = torch.optim.Adam(params, lr=0.0, betas=(BETA1, BETA2), eps=ADAM_EPS, **kw)

            def update():
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()

            def update_and_load():
                update()
                load(theirs)

            with torch.cuda.stream(st):
                return {"clip_and_adam": stat(timed(update, a.repeats, stream=st)), "with_load_policy": stat(timed(update_and_load, a.repeats, stream=st))}

        out["torch_default"] = torch_leg(False)
        try:
            out["torch_fused"] = torch_leg(True)
        except (RuntimeError, TypeError, ValueError) as e:
            out["torch_fused"] = {"refused": str(e)[:200]}
        out["load_policy_six_layers"] = stat(timed(lambda: load(mine), a.repeats, stream=st))
        out["opt_step_over_torch_default_with_load"] = out["opt_step_alone"]["median_us"] / out["torch_default"]["with_load_policy"]["median_us"]

        # ---- 20 steps of both legs from the same weights on the same gradient sequence ----
        b.configure_opt(BETA1, BETA2, ADAM_EPS, MAX_NORM)
        for net, l in slots:
            w, bias = mine[net][l]
            b.bind_opt_param(net, l, w.data_ptr(), w.shape[1], bias.data_ptr())
        b.bind_opt_log_std(leg.log_std.data_ptr())
        ls0 = leg.log_std.clone()
        opt = torch.optim.Adam(params, lr=LR, betas=(BETA1, BETA2), eps=ADAM_EPS)
        with torch.cuda.stream(st):
            for k in range(20):
                grad(k % MINIBATCHES)
                step(LR)                            # (reads the gradients before torch's clip scales them in place)
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
        torch.cuda.synchronize()
        a_ = [t for net in mine for pair in net for t in pair] + [leg.log_std]
        out["largest_relative_difference_of_the_weights_after_20_steps"] = float(max(
            ((x.double() - p.data.double()).abs().max() / p.data.double().abs().max()).item() for x, p in zip(a_, params)))
        out["opt_stats_after_20_steps"] = {k: float(v) for k, v in b.opt_stats().items() if k != "all"}
        leg.log_std.copy_(ls0)

        # ---- the share of an iteration ----
        opt0 = torch.optim.Adam(params, lr=0.0, betas=(BETA1, BETA2), eps=ADAM_EPS)

        def update_parent():
            with torch.cuda.stream(st):
                for _ in range(EPOCHS):
                    for k in range(MINIBATCHES):
                        grad(k)
                        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                        opt0.step()
                        load(theirs)

        def update_this():
            for _ in range(EPOCHS):
                for k in range(MINIBATCHES):
                    grad(k)
                    step(0.0)

        def grads_only():
            for _ in range(EPOCHS):
                for k in range(MINIBATCHES):
                    grad(k)

        def region(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0)

        load(mine)
        ro, gr, it_p, it_t = [], [], [], []
        for _ in range(a.repeats):
            ro.append(region(rollout))
            gr.append(region(lambda: (rollout(), grads_only())))
            it_p.append(region(lambda: (rollout(), update_parent())))
            load(mine)
            it_t.append(region(lambda: (rollout(), update_this())))
        out["rollout_region"], out["rollout_and_grads_region"] = stat(ro), stat(gr)
        out["iteration_region_torch_step_and_load"], out["iteration_region_opt_step"] = stat(it_p), stat(it_t)
        g = out["rollout_and_grads_region"]["median_us"]
        for key, name in (("iteration_region_torch_step_and_load", "update_share_percent_torch_step_and_load"), ("iteration_region_opt_step", "update_share_percent_opt_step")):
            out[name] = 100.0 * (out[key]["median_us"] - g) / out[key]["median_us"]
        out["grad_launches"], out["opt_launches"] = list(b.grad_launches()), list(b.opt_launches())
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
