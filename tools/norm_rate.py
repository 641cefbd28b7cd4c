#!/usr/bin/env python3
"""What the normaliser rows cost -- nothing here is a condition, all of it is written down.  One MI355X, one process, tools/grad_rate.py's
method and set-up: T = 24 policy steps of 4096 envs with every stage in place, the rollout's OBS store (340 float32 columns, a torch
tensor bound as the store) as the source, block 256; fenced regions between device events on the call's stream.

  norm_update      phys_batch_norm_update on an idle device; each of its launches alone (phys_batch_debug_norm_mask: the partials and the
                   state keep what a full call left), the sum pass alone behind a write of 1 GiB that empties the Infinity Cache, and
                   phys_batch_norm_write.  Bytes moved per second: both passes read the store once.
  torch            on the same tensor: torch.var_mean(dim=(0, 1)), the Chan merge, rsqrt and the two copy_.
  bits             the device's state against the numpy restatement (tests/norm_check.py) for the downloaded store, and the restatement
                   against numpy's own float64 mean / var of the same values.
  iteration        the rollout alone and the rollout with norm_update behind it; the update's share of an iteration, also against the
                   iteration profiles/grad_rate.json describes.
  --parent-lib     the loop ALONE in fresh child processes, parent commit's library and this one, in the order parent, this, this,
                   parent (tools/rollout_rate.py's bare leg): unused, the feature should cost nothing.

Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/norm_rate.py [--envs 4096] [--repeats 10] [--block 256] [--out profiles/norm_rate.json] [--parent-lib PATH]
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import grad_rate  # noqa: E402  (sets the other paths)
import rollout_rate  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

T, NOBS = rollout_rate.T, rollout_rate.NOBS
EPS = 1e-8
COPY_RATE = 6.29e12                      # the measured copy rate of the device, bytes read + written per second
LAUNCHES = ("sum", "mean", "sq", "merge")
stat, timed = grad_rate.stat, grad_rate.timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    n = a.envs
    R = T * n
    out = {"tool": "norm_rate", "model": "cassie", "envs": n, "rollout_steps": T, "dim": NOBS, "block": a.block, "rows": R, "regions": a.repeats,
           "store_bytes": 4 * R * NOBS, "eps": EPS}
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
        dev = torch.device("cuda")
        store = torch.zeros((T, n, NOBS), dtype=torch.float32, device=dev)
        b.bind_rollout_storage("obs", store.data_ptr())

        def rollout():
            for _ in range(T):
                leg.launch()

        rollout()
        rollout()
        torch.cuda.synchronize()
        # the outputs are two tensors of the tool's: the loop's own normalisation stays as it is, so every region runs the same loop
        mean_d, inv_d = torch.zeros(NOBS, dtype=torch.float32, device=dev), torch.ones(NOBS, dtype=torch.float32, device=dev)
        b.configure_norm(NOBS, a.block, max_rows=R, eps=EPS)
        b.bind_norm_output(mean_d.data_ptr(), inv_d.data_ptr())
        st = leg.streams[0]
        update = lambda: b.norm_update(st.cuda_stream)

        # ---- bits: one update against the restatement, the restatement against numpy's float64 mean / var ----
        import norm_check as nc
        update()
        b.sync()
        torch.cuda.synchronize()
        x = store.cpu().numpy().reshape(R, NOBS)
        ref, rmean, rinv = nc.State(NOBS), np.zeros(NOBS, dtype=np.float32), np.ones(NOBS, dtype=np.float32)
        nc.update(x, ref, a.block, EPS, rmean, rinv)
        same = all(nc.same_bits(b.norm_download(w), v) for w, v in zip((P.NORM_N, P.NORM_MEAN, P.NORM_M2), (ref.n, ref.mean, ref.m2)))
        out["device_equals_restatement_bit_for_bit"] = bool(same and nc.same_bits(mean_d.cpu().numpy(), rmean) and nc.same_bits(inv_d.cpu().numpy(), rinv))
        out["values_not_finite"] = int((~np.isfinite(x)).sum())
        x64 = x.astype(np.float64)
        m64, v64 = x64.mean(axis=0), x64.var(axis=0)
        out["restatement_vs_numpy_float64"] = {
            "mean_largest_difference_relative_to_the_largest_mean": float(np.max(np.abs(ref.mean - m64)) / np.max(np.abs(m64))),
            "var_largest_relative_difference": float(np.max(np.abs(ref.m2 / ref.n - v64) / np.maximum(v64, 1e-300))),
            "var_largest_difference_relative_to_the_largest_var": float(np.max(np.abs(ref.m2 / ref.n - v64)) / np.max(v64))}
        out["norm_stats"] = {k: float(v) for k, v in b.norm_stats().items() if k != "all"}

        # ---- norm_update alone, launch by launch ----
        out["norm_update_alone"] = stat(timed(update, a.repeats, stream=st))
        per = {}
        for k, name in enumerate(LAUNCHES):
            b.norm_launch_mask(1 << k)
            per[name] = stat(timed(update, a.repeats, stream=st))
        # the sum pass behind a write that empties the Infinity Cache: one call a region, the write outside the events
        flush = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        b.norm_launch_mask(1)
        cold = []
        for k in range(a.repeats):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                flush.fill_(float(k))
            ev0.record(st)
            update()
            ev1.record(st)
            torch.cuda.synchronize()
            cold.append(1000.0 * ev0.elapsed_time(ev1))
        per["sum_behind_a_1GiB_write"] = stat(cold)
        del flush
        b.norm_launch_mask(15)
        out["launches"] = per
        out["norm_write_alone"] = stat(timed(lambda: b.norm_write(st.cuda_stream), a.repeats, stream=st))
        bytes_pass = 4.0 * R * NOBS
        out["bytes_per_s"] = {"update_two_passes": 2 * bytes_pass / (1e-6 * out["norm_update_alone"]["median_us"]),
                              "sum_warm": bytes_pass / (1e-6 * per["sum"]["median_us"]), "sq_warm": bytes_pass / (1e-6 * per["sq"]["median_us"]),
                              "sum_cold": bytes_pass / (1e-6 * per["sum_behind_a_1GiB_write"]["median_us"]), "measured_copy_rate": COPY_RATE}
        out["update_over_copy_rate"] = out["bytes_per_s"]["update_two_passes"] / COPY_RATE
        out["warm_pass_over_cold_pass_time"] = per["sum"]["median_us"] / per["sum_behind_a_1GiB_write"]["median_us"]

        # ---- the torch chain on the same tensor ----
        rn, rm, rv = torch.zeros((), device=dev), torch.zeros(NOBS, device=dev), torch.ones(NOBS, device=dev)
        tmean, tinv = torch.zeros(NOBS, device=dev), torch.ones(NOBS, device=dev)

        def torch_chain():
            var, mean = torch.var_mean(store, dim=(0, 1), correction=0)
            tot = rn + R
            delta = mean - rm
            m2 = rv * rn + var * R + delta * delta * (rn * R / tot)
            rm.add_(delta * (R / tot))
            rv.copy_(m2 / tot)
            rn.fill_(0.0)                      # (every call merges into the same state: the work of a call stays the same)
            tmean.copy_(rm)
            tinv.copy_(torch.rsqrt(rv + EPS))

        with torch.cuda.stream(st):
            out["torch_chain"] = stat(timed(torch_chain, a.repeats, stream=st))
            out["torch_var_mean_alone"] = stat(timed(lambda: torch.var_mean(store, dim=(0, 1), correction=0), a.repeats, stream=st))
        out["bytes_per_s"]["torch_var_mean"] = bytes_pass / (1e-6 * out["torch_var_mean_alone"]["median_us"])
        out["norm_update_over_torch_chain"] = out["norm_update_alone"]["median_us"] / out["torch_chain"]["median_us"]

        # ---- the share of an iteration ----
        def region(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e6 * (time.perf_counter() - t0)

        ro, ru = [], []
        for _ in range(a.repeats):
            ro.append(region(rollout))
            ru.append(region(lambda: (rollout(), update())))
        out["rollout_region"], out["rollout_and_update_region"] = stat(ro), stat(ru)
        out["update_share_percent_of_rollout_plus_update"] = 100.0 * out["norm_update_alone"]["median_us"] / (out["rollout_region"]["median_us"] + out["norm_update_alone"]["median_us"])
        try:
            with open(os.path.join(REPO, "profiles", "grad_rate.json")) as f:
                it = json.load(f)["iteration_region"]["median_us"]
            out["update_share_percent_of_the_iteration_of_grad_rate_json"] = 100.0 * out["norm_update_alone"]["median_us"] / (it + out["norm_update_alone"]["median_us"])
        except (OSError, KeyError, ValueError):
            pass
        out["norm_launches"] = list(b.norm_launches())
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
