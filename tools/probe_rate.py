#!/usr/bin/env python3
"""What probes per policy step cost config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the batch
as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- in four legs that ALTERNATE in one
process on one box, fenced timed regions, ten each:

  loop          the loop alone.  THE YARDSTICK.
  probes        the same plus one phys_batch_probe per range and policy step, on the range's stream: 8 probes (pelvis, both feet, a foot
                point, two heel / toe sites, the imu site, a tarsus), POS | VEL | CFRC | CONTACTS.
  probes_jac    the same with JACP | JACR added.
  derive        for comparison the older call, phys_batch_derive once per policy step: it takes the whole batch, quiesces every stream
                and allocates and frees the read-out block, i.e. it stops the loop.

--parent-lib PATH runs the `loop` leg once more in a child process against another build of the library (the parent commit's): no
stepping kernel changes with the probes, so this build's `loop` median should differ from the parent's by no more than the spread of a
leg's own regions.

Also times the probe call alone (forward pass + reduction) over the whole batch on an idle device, and records the bytes the
configuration holds.  Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/probe_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/probe_rate.json]
                               [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cassie-mujoco-sim_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

import bench  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402
from cassie_amd._lib import _structs  # noqa: E402

NSUB = bench.HOLD
LEGS = ("loop", "probes", "probes_jac", "derive")


def probe_list(model):
    body, site = (lambda s: model.name2id(1, s)), (lambda s: model.name2id(6, s))
    return [(P.PROBE_BODY, body("cassie-pelvis"), [0, 0, 0]), (P.PROBE_BODY, body("left-foot"), [0, 0, 0]), (P.PROBE_BODY, body("right-foot"), [0, 0, 0]),
            (P.PROBE_BODY, body("left-foot"), [0.02, -0.03, 0.05]), (P.PROBE_SITE, site("left-heel"), [0, 0, 0]), (P.PROBE_SITE, site("right-toe"), [0, 0, 0]),
            (P.PROBE_SITE, site("imu"), [0, 0, 0]), (P.PROBE_BODY, body("right-tarsus"), [0, 0, 0])]


def quantities_of(leg):
    q = P.PQ_POS | P.PQ_VEL | P.PQ_CFRC | P.PQ_CONTACTS
    return q | P.PQ_JACP | P.PQ_JACR if leg == "probes_jac" else q


class Leg:
    """One batch running config 2's loop, with what its leg adds behind every range's step launch."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.b = b = Batch(model, n)
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + np.random.default_rng(1).uniform(-0.3, 0.3, (n, 10)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        self.held = 0
        if leg in ("probes", "probes_jac"):
            probes = probe_list(model)
            b.configure_probes(probes, quantities_of(leg))
            row = b.dim(P.F_PROBES)
            scratch = 2 * pod.nv + pod.nsensordata + pod.nu + 7 * pod.nbody
            self.held = {"rows": 8 * row * n, "contact_words": 4 * n, "read_out_block": ctypes.sizeof(_structs["cm_ext_t"]) * n,
                         "scratch_outputs": 8 * scratch * n, "row_doubles": row, "probes": len(probes)}
        self.ids = [model.name2id(1, "left-foot"), model.name2id(1, "right-foot"), model.name2id(6, "left-heel"), model.name2id(6, "right-heel"),
                    model.name2id(6, "left-toe"), model.name2id(6, "right-toe")]
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            if self.leg in ("probes", "probes_jac"):
                b.probe(first, cnt, stream=st.cuda_stream)
        if self.leg == "derive":
            b.derive(self.ids)

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
        if self.held:
            out["bytes_held"] = self.held
            out["probe_launches"] = list(self.b.probe_launches())
            # the call alone (forward pass + reduction) over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            self.b.probe(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    self.b.probe(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["probe_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
            vals = self.b.probes()
            out["finite_rows"] = int(np.isfinite(vals["pos"]).all(axis=(1, 2)).sum())
            out["envs_with_a_loaded_foot"] = int((np.abs(vals["cfrc"][:, 1:3]).max(axis=(1, 2)) > 1.0).sum())
        return out

    def close(self):
        self.b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=list(LEGS), default=None, help="one leg only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): its `loop` leg, in a child process")
    a = ap.parse_args()
    out = {"tool": "probe_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "the legs alternate region by region in one process; a probe per range behind its step launch",
           "probes_per_env": 8, "quantities": {"probes": "POS | VEL | CFRC | CONTACTS", "probes_jac": "POS | VEL | CFRC | CONTACTS | JACP | JACR"},
           "yardstick": "loop"}
    if a.parent_lib:
        # (first, in a process of its own: one library per process; this process has not touched the GPU yet)
        cmd = [sys.executable, os.path.abspath(__file__), "--only", "loop", "--envs", str(a.envs), "--launches", str(a.launches),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, env=dict(os.environ, CASSIE_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit("the --parent-lib leg failed:\n" + r.stderr[-2000:])
        out["parent_loop"] = json.loads(r.stdout.strip().splitlines()[-1])["loop"]
    model = Model("cassie")
    legs = [Leg(model, a.envs, name) for name in LEGS if a.only in (None, name)]
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
    if "parent_loop" in out and "loop" in out:
        par, own = out["parent_loop"], out["loop"]
        out["loop_median_over_parent_median"] = own["env_steps_per_s_median"] / par["env_steps_per_s_median"]
        out["loop_median_within_the_parents_regions"] = bool(par["env_steps_per_s_min"] <= own["env_steps_per_s_median"] <= par["env_steps_per_s_max"])
        out["difference_of_medians_percent"] = 100.0 * abs(out["loop_median_over_parent_median"] - 1.0)
        out["larger_spread_of_the_two_legs_percent"] = max(par["spread_percent_of_median"], own["spread_percent_of_median"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
