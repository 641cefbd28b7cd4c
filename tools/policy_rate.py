#!/usr/bin/env python3
"""What the policy network per policy step costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch,
the batch as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- with the stages around it in
place: per range and policy step task (tools/task_rate.py's 21 columns), observe (tools/obs_rate.py's 85 columns x 4 frames = 340 float32,
its input the task row's first 12 columns), [the policy], act (ten columns from the action tensor onto the task row's reference pose into
F_PD_PTARGET), the step launch.  Three legs ALTERNATE in one process on one box, fenced timed regions, ten each:

  loop          the loop with the action tensor held constant.  THE YARDSTICK.
  policy        the same plus one phys_batch_policy per range and policy step between observe and act: actor 340 -> 256 -> 256 -> 10 and
                critic 340 -> 256 -> 256 -> 1, ELU, the input normalised and clipped, the action sampled from the caller's draws with its
                log-probability, written into the tensor act reads.
  torch         the same networks as torch.nn.Sequential under no_grad on the same streams, with the normalisation, the sampling and the
                log-probability in torch operations, written into the same tensors.  What a user does today, in fp32.

--parent-lib PATH runs the loop ALONE (no task, observe or act: the parent has no policy either way, and this is the loop every earlier
measurement of "unused, it costs nothing" timed) in child processes, in the order parent, this build, this build, parent: like against
like, one batch in a fresh process of its own, the regions of a build's two runs pooled.  No stepping kernel changes with the policy rows,
so this build's median should lie inside the parent's regions.

Also times the policy call alone over the whole batch on an idle device, and compares the policy leg's outputs with the torch networks'
on the same rows.  Every region is recorded.  Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/policy_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/policy_rate.json]
                                [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cassie-mujoco-sim_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

import bench  # noqa: E402
import obs_rate  # noqa: E402
import task_rate  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

NSUB = bench.HOLD
LEGS = ("loop", "policy", "torch")
NACT, HIDDEN, CLIP, LOG_STD, SCALE, OUT_HALF = 10, 256, 5.0, -1.0, 0.3, 0.6
NOBS = 85 * obs_rate.HISTORY
H = 0.9189385332046727


def act_columns():
    return [P.act_col(P.F_PD_PTARGET, j, lo=-1.0, hi=1.0, bfield=P.ACT_INPUT, bindex=task_rate.REF + j, scale=SCALE,
                      out_lo=float(bench.PD_OFFSET[j]) - OUT_HALF, out_hi=float(bench.PD_OFFSET[j]) + OUT_HALF) for j in range(NACT)]


def weights(rng, widths):
    return [((rng.normal(size=(o, i)) / np.sqrt(i)).astype(np.float32), (0.1 * rng.normal(size=o)).astype(np.float32)) for i, o in zip(widths[:-1], widths[1:])]


def sequential(layers, dev):
    mods = []
    for k, (w, b) in enumerate(layers):
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
        mods += [lin] + ([torch.nn.ELU()] if k < len(layers) - 1 else [])
    return torch.nn.Sequential(*mods).to(dev)


class Leg:
    """One batch running config 2's loop with task, observe and act in place, and what its leg puts between observe and act.
    leg "bare": the loop alone (what --parent-lib compares)."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.b = b = Batch(model, n)
        dev = torch.device("cuda")
        rng = np.random.default_rng(1)
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + rng.uniform(-0.3, 0.3, (n, NACT)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        if leg != "bare":
            self.xfrc = torch.zeros((n, 6 * pod.nbody), dtype=torch.float64, device=dev)
            self.task_rows = torch.zeros((n, task_rate.NCOLS), dtype=torch.float32, device=dev)
            self.obs = torch.zeros((n, NOBS), dtype=torch.float32, device=dev)
            self.actions = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, NACT)).astype(np.float32)).to(dev)
            self.value = torch.zeros((n, 1), dtype=torch.float32, device=dev)
            self.mu = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
            self.logp = torch.zeros(n, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            b.bind(P.F_XFRC_APPLIED, self.xfrc.data_ptr())
            b.set_task_table(task_rate.reference_table())
            b.configure_task(task_rate.task_columns(pod), dtype=np.float32, seed=1)
            b.bind_task_rows(self.task_rows.data_ptr(), task_rate.NCOLS)
            b.configure_obs(obs_rate.obs_terms(pod), history=obs_rate.HISTORY, dtype=np.float32, seed=1)
            assert b.obs_dim()[2] == NOBS
            b.bind_obs(self.obs.data_ptr())
            b.bind_obs_input(self.task_rows.data_ptr(), obs_rate.NINPUT, task_rate.NCOLS, torch.float32)
            b.configure_actions(act_columns(), dtype=np.float32, seed=1)
            b.bind_actions(self.actions.data_ptr(), NACT, torch.float32)
            b.bind_action_input(self.task_rows.data_ptr(), task_rate.NCOLS, task_rate.NCOLS, torch.float32)
            # the policy of the two network legs: the same weights, statistics and draws
            wrng = np.random.default_rng(2)
            self.nets = [weights(wrng, (NOBS, HIDDEN, HIDDEN, NACT)), weights(wrng, (NOBS, HIDDEN, HIDDEN, 1))]
            self.mean = torch.from_numpy((0.1 * wrng.normal(size=NOBS)).astype(np.float32)).to(dev)
            self.inv = torch.from_numpy(wrng.uniform(0.5, 2.0, NOBS).astype(np.float32)).to(dev)
            self.log_std = torch.full((NACT,), LOG_STD, dtype=torch.float32, device=dev)
            self.eps = torch.from_numpy(np.clip(wrng.normal(size=(4, n, NACT)), -4, 4).astype(np.float32)).to(dev)
        if leg == "policy":
            acts = [P.POL_ELU, P.POL_ELU, P.POL_IDENTITY]
            b.configure_policy([[P.pol_layer(w.shape[0], a) for (w, _), a in zip(net, acts)] for net in self.nets], NOBS)
            self.wdev = [[(torch.from_numpy(w).to(dev), torch.from_numpy(bias).to(dev)) for w, bias in net] for net in self.nets]
            torch.cuda.synchronize()
            for k, net in enumerate(self.wdev):
                b.load_policy(k, [(w.data_ptr(), w.shape[1], bias.data_ptr()) for w, bias in net])
            b.bind_policy_input(self.obs.data_ptr(), NOBS, NOBS, torch.float32)
            b.bind_policy_norm(self.mean.data_ptr(), self.inv.data_ptr(), CLIP)
            b.bind_policy_output(0, self.mu.data_ptr(), NACT)
            b.bind_policy_output(1, self.value.data_ptr(), 1)
        if leg in ("policy", "torch"):
            self.actor, self.critic = sequential(self.nets[0], dev), sequential(self.nets[1], dev)
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def torch_policy(self, e0, cnt, p):
        """The actions, values and log-probabilities of the range as a user makes them today (on the current stream)."""
        s = slice(e0, e0 + cnt)
        with torch.no_grad():
            x = ((self.obs[s] - self.mean) * self.inv).clamp(-CLIP, CLIP)
            mu, eps = self.actor(x), self.eps[p % 4, s]
            self.value[s] = self.critic(x)
            self.mu[s] = mu
            self.actions[s] = mu + torch.exp(self.log_std) * eps
            self.logp[s] = (-0.5 * eps * eps - self.log_std).sum(-1) - NACT * H

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        if self.leg == "policy":
            b.bind_policy_sample(self.eps[p % 4].data_ptr(), self.log_std.data_ptr(), self.actions.data_ptr(), self.logp.data_ptr())
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            if self.leg != "bare":
                b.task(first, cnt, stream=st.cuda_stream)
                b.observe(first, cnt, stream=st.cuda_stream)
                if self.leg == "policy":
                    b.policy(first, cnt, stream=st.cuda_stream)
                elif self.leg == "torch":
                    with torch.cuda.stream(st):
                        self.torch_policy(first, cnt, p)
                b.act(first, cnt, stream=st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)

    def region(self, launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            self.launch()
        torch.cuda.synchronize()
        self.rates.append(self.n * NSUB * launches / (time.perf_counter() - t0))

    def report(self):
        r = self.rates
        out = {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
               "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r,
               "envs_with_warnings": int(self.b.warnings()[0].astype(bool).sum())}
        if self.leg in ("policy", "torch"):
            out["finite_action_rows"] = int(torch.isfinite(self.actions).all(dim=1).sum())
            out["finite_values"] = int(torch.isfinite(self.value).sum())
        if self.leg == "policy":
            b = self.b
            out["policy_launches"] = b.policy_launches()
            out["networks"] = {"actor": [NOBS, HIDDEN, HIDDEN, NACT], "critic": [NOBS, HIDDEN, HIDDEN, 1], "activation": "ELU",
                               "fma_per_env": int(sum(w.size for net in self.nets for w, _ in net))}
            # the torch networks on the rows the last call read: what fp32 GEMMs make of the same function
            with torch.no_grad():
                x = ((self.obs - self.mean) * self.inv).clamp(-CLIP, CLIP)
                out["largest_difference_of_mu_against_torch"] = float((self.actor(x) - self.mu).abs().max())
                out["largest_difference_of_value_against_torch"] = float((self.critic(x) - self.value).abs().max())
            # the call alone over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            b.policy(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    b.policy(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["policy_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
        if self.leg == "torch":
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            with torch.cuda.stream(st):
                self.torch_policy(0, self.n, 0)
                torch.cuda.synchronize()
                ev0.record()
                for _ in range(20):
                    self.torch_policy(0, self.n, 0)
                ev1.record()
            torch.cuda.synchronize()
            out["torch_policy_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
        return out

    def close(self):
        self.b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=list(LEGS) + ["bare"], default=None, help="one leg only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): the loop alone, in child processes")
    a = ap.parse_args()
    out = {"tool": "policy_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "task, observe (340 float32) and act in place; the legs alternate region by region in one process; the policy of a range "
                   "between its observe and its act",
           "yardstick": "loop"}
    if a.parent_lib:
        # (first, in fresh processes of their own: one library per process; this process has not touched the GPU yet)
        def alone(lib):
            cmd = [sys.executable, os.path.abspath(__file__), "--only", "bare", "--envs", str(a.envs), "--launches", str(a.launches),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            env = dict(os.environ, CASSIE_LIB=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != "CASSIE_LIB"}
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("a child leg failed:\n" + r.stderr[-2000:])
            return json.loads(r.stdout.strip().splitlines()[-1])["bare"]

        def pooled(runs):
            r = [v for run in runs for v in run["regions"]]
            return {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
                    "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r,
                    "run_medians": [run["env_steps_per_s_median"] for run in runs], "envs_with_warnings": sum(run["envs_with_warnings"] for run in runs)}

        runs = [alone(lib) for lib in (a.parent_lib, None, None, a.parent_lib)]
        out["parent_loop"], out["loop_alone"] = pooled([runs[0], runs[3]]), pooled([runs[1], runs[2]])
    model = Model("cassie")
    names = ["bare"] if a.only == "bare" else [name for name in LEGS if a.only in (None, name)]
    legs = [Leg(model, a.envs, name) for name in names]
    try:
        for leg in legs:
            for _ in range(a.warmup):
                leg.launch()
        for _ in range(a.repeats):
            for leg in legs:
                leg.region(a.launches)
        for leg in legs:
            out[leg.leg] = leg.report()
    finally:
        for leg in legs:
            leg.close()
    if "loop" in out:
        base = out["loop"]["env_steps_per_s_median"]
        for name in LEGS[1:]:
            if name in out:
                out[name]["cost_of_the_loop_percent"] = 100.0 * (1.0 - out[name]["env_steps_per_s_median"] / base)
        out["loop_spread_percent"] = out["loop"]["spread_percent_of_median"]
    if "policy" in out and "torch" in out:
        one, many = out["policy"]["env_steps_per_s_median"], out["torch"]["env_steps_per_s_median"]
        out["cheaper_network_leg"] = "policy" if one > many else "torch"
        out["largest_spread_of_a_leg_percent"] = max(out[name]["spread_percent_of_median"] for name in LEGS if name in out)
    if "parent_loop" in out:
        par, own = out["parent_loop"], out["loop_alone"]
        out["loop_median_over_parent_median"] = own["env_steps_per_s_median"] / par["env_steps_per_s_median"]
        out["loop_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= own["env_steps_per_s_median"] <= par["env_steps_per_s_max"])
        out["difference_of_medians_percent"] = 100.0 * abs(out["loop_median_over_parent_median"] - 1.0)
        out["parents_spread_percent"] = par["spread_percent_of_median"]
        out["unused_the_feature_costs_less_than_the_parents_spread"] = bool(out["difference_of_medians_percent"] < par["spread_percent_of_median"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
