#!/usr/bin/env python3
"""What the draw rows cost -- nothing here is a condition, all of it is written down.  One MI355X, one process, tools/norm_rate.py's
method: fenced regions between device events on the call's stream.

  alone            phys_batch_draw (4096 envs x 10 columns) and phys_batch_draw_perm (n = 98 304) on an idle device, against torch.randn
                   into the same tensor and torch.randperm(dtype=int32) on the same stream.
  bits             the device's rows and permutation against the numpy restatement (tests/draw_check.py).
  loop             config 2's loop with every stage of a policy step in place (tools/rollout_rate.py's "loop" leg), three legs of one
                   process that alternate region by region: a constant eps, draw() per range in front of policy(), torch.randn per range.
                   Each difference against the legs' own spread.
  --parent-lib     the loop ALONE in fresh child processes, parent commit's library and this one, in the order parent, this, this,
                   parent (tools/rollout_rate.py's bare leg): unused, the feature should cost nothing.

Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/draw_rate.py [--envs 4096] [--repeats 10] [--perm 98304] [--out profiles/draw_rate.json] [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import grad_rate  # noqa: E402  (sets the other paths)
import rollout_rate  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402

T, NACT, NSUB = rollout_rate.T, rollout_rate.NACT, rollout_rate.NSUB
SEED = 1
MODES = ("constant", "draw", "randn")
stat, timed = grad_rate.stat, grad_rate.timed


class Leg(rollout_rate.Leg):
    """rollout_rate's loop leg with the eps of its mode in front of every range's policy call."""

    def __init__(self, model, n, mode):
        super().__init__(model, n, "loop")
        self.mode = mode
        self.live = torch.zeros((n, NACT), dtype=torch.float32, device="cuda")
        if mode == "draw":
            self.b.configure_draws(NACT, 0, seed=SEED)
        torch.cuda.synchronize()

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        eps = self.eps[p % 4] if self.mode == "constant" else self.live
        b.bind_policy_sample(eps.data_ptr(), self.log_std.data_ptr(), self.actions.data_ptr(), self.logp.data_ptr())
        for (first, cnt), st in zip(self.ranges, self.streams):
            done = self.done.data_ptr() + 4 * first
            b.end_episodes(first, cnt, True, force_ptr=self.flags.data_ptr() + 4 * first, stream=st.cuda_stream)
            b.task(first, cnt, reset_ptr=done, stream=st.cuda_stream)
            b.observe(first, cnt, refill_ptr=done, stream=st.cuda_stream)
            if self.mode == "draw":
                b.draw(first, cnt, stream=st.cuda_stream)
            elif self.mode == "randn":
                with torch.cuda.stream(st):
                    self.live[first: first + cnt].normal_()
            b.policy(first, cnt, stream=st.cuda_stream)
            b.act(first, cnt, reset_ptr=done, stream=st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            b.events(first, cnt, reset_ptr=done, stream=st.cuda_stream)
            b.reward(first, cnt, reset_ptr=done, stream=st.cuda_stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--perm", type=int, default=98304)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    n = a.envs
    out = {"tool": "draw_rate", "model": "cassie", "envs": n, "columns": NACT, "perm_n": a.perm, "regions": a.repeats, "loop_steps_a_region": T}
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

    # ---- alone on an idle device ----
    import draw_check as dc
    b = Batch(model, n)
    try:
        dev = torch.device("cuda")
        rows = torch.zeros((n, NACT), dtype=torch.float32, device=dev)
        perm = torch.zeros(a.perm, dtype=torch.int32, device=dev)
        b.configure_draws(NACT, a.perm, seed=SEED)
        b.bind_draws(rows.data_ptr(), NACT)
        b.bind_draw_perm(perm.data_ptr())
        st = torch.cuda.Stream()
        b.draw(stream=st.cuda_stream)
        b.draw_perm(7, stream=st.cuda_stream)
        b.sync()
        torch.cuda.synchronize()
        want = dc.normal_rows(SEED, 0, np.arange(n), np.zeros(n, dtype=np.uint64), NACT)
        out["device_equals_restatement_bit_for_bit"] = bool(rows.cpu().numpy().tobytes() == want.tobytes() and
                                                            perm.cpu().numpy().tobytes() == dc.perm(a.perm, 7, SEED).tobytes())
        out["draw_alone"] = stat(timed(lambda: b.draw(stream=st.cuda_stream), a.repeats, stream=st))
        out["draw_perm_alone"] = stat(timed(lambda: b.draw_perm(7, stream=st.cuda_stream), a.repeats, stream=st))
        with torch.cuda.stream(st):
            out["torch_randn"] = stat(timed(lambda: rows.normal_(), a.repeats, stream=st))
            out["torch_randperm_int32"] = stat(timed(lambda: torch.randperm(a.perm, dtype=torch.int32, device=dev), a.repeats, stream=st))
        out["draw_over_torch_randn"] = out["draw_alone"]["median_us"] / out["torch_randn"]["median_us"]
        out["draw_perm_over_torch_randperm"] = out["draw_perm_alone"]["median_us"] / out["torch_randperm_int32"]["median_us"]
        out["values_per_s"] = {"draw": n * NACT / (1e-6 * out["draw_alone"]["median_us"]), "draw_perm": a.perm / (1e-6 * out["draw_perm_alone"]["median_us"])}
        out["draw_launches"] = list(b.draw_launches())
    finally:
        b.close()

    # ---- in config 2's loop: three legs of one process, region by region in turn ----
    legs = {mode: Leg(model, n, mode) for mode in MODES}
    try:
        for leg in legs.values():
            leg.region(T)
            leg.rates.clear()
        for _ in range(a.repeats):
            for leg in legs.values():
                leg.region(T)
        out["loop"] = {mode: leg.report() for mode, leg in legs.items()}
        med = {mode: out["loop"][mode]["env_steps_per_s_median"] for mode in MODES}
        out["loop_draw_over_constant"] = med["draw"] / med["constant"]
        out["loop_randn_over_constant"] = med["randn"] / med["constant"]
        out["loop_draw_over_randn"] = med["draw"] / med["randn"]
        out["loop_spread_percent"] = {mode: out["loop"][mode]["spread_percent_of_median"] for mode in MODES}
    finally:
        for leg in legs.values():
            leg.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
