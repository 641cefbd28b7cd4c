#!/usr/bin/env python3
"""What the event row per policy step costs config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the
batch as two env ranges on two streams with nothing joining them, restarts on bench.py's schedule -- in three legs that ALTERNATE in one
process on one box, fenced timed regions, ten each:

  loop          the loop alone, F_PD_PTARGET bound as the benchmark binds it and F_BODY_CFRC bound to a torch tensor (in every leg, so
                that the legs differ in what follows a step launch alone).  THE YARDSTICK.
  events        the same plus one phys_batch_events per range and policy step, on the range's stream BEHIND its step launch: a biped's
                chain of 21 columns (float32) on F_BODY_CFRC -- the force on two feet and the pelvis, contact flags with hysteresis,
                on- and off-timers, touchdown and lift-off edges, the air time paid at touchdown, the peak force of a stance, "both feet
                off for 0.15 s" and "the pelvis took a force" as done columns -- with the done words written.
  torch         the same row and done words made with torch operations on the same streams: norms, thresholds with hysteresis, masked
                timers, where chains, previous-contact tensors.  What a user does today.

--parent-lib PATH runs the `loop` leg alone in child processes, in the order parent, this build, this build, parent, against another
build of the library (the parent commit's) and against this one: like against like, one batch in a fresh process of its own, the regions
of a build's two runs pooled.  No stepping kernel changes with the event rows, so this build's median should lie inside the parent's
regions.

Also times the events call alone over the whole batch on an idle device.  Every region is recorded.  Prints one JSON line; `--out` also
writes it to a file.  Needs a GPU.

    python tools/event_rate.py [--envs 4096] [--launches 20] [--warmup 10] [--repeats 10] [--only NAME] [--out profiles/event_rate.json]
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
sys.path.insert(0, REPO)

import bench  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

NSUB = bench.HOLD
LEGS = ("loop", "events", "torch")
DT, ON_THR, OFF_THR, PEL_THR, K_OFF = NSUB * 0.0005, 20.0, 5.0, 1.0, 6
# the row: three forces | two contact flags | on-timers | off-timers | touchdowns | lift-offs | air times | peaks | neither, flight, fly | pelvis
(FL, FR, FP, CL, CR, ONL, ONR, OFFL, OFFR, TDL, TDR, LOL, LOR, AIRL, AIRR, PEAKL, PEAKR, NEITHER, FLIGHT, FLY, PEL) = range(21)
NCOLS = 21


def event_columns(lf, rf, pel):
    force = lambda body: P.ev_measure(P.F_BODY_CFRC, 3 * body, 3, norm=P.EV_SUMSQ, root=True)
    cols = [force(lf), force(rf), force(pel), P.ev_level(FL, ON_THR, OFF_THR), P.ev_level(FR, ON_THR, OFF_THR),
            P.ev_timer(CL, DT, 1), P.ev_timer(CR, DT, 1), P.ev_timer(CL, DT, 0), P.ev_timer(CR, DT, 0),
            P.ev_edge(CL, P.EV_RISING), P.ev_edge(CR, P.EV_RISING), P.ev_edge(CL, P.EV_FALLING), P.ev_edge(CR, P.EV_FALLING),
            P.ev_latch(OFFL, TDL, lag=1), P.ev_latch(OFFR, TDR, lag=1), P.ev_accum(FL, P.EV_MAX, clear=TDL), P.ev_accum(FR, P.EV_MAX, clear=TDR),
            P.ev_logic([CL, CR], P.EV_NONE), P.ev_timer(NEITHER, DT, 1), P.ev_level(FLIGHT, K_OFF * DT), P.ev_level(FP, PEL_THR)]
    assert len(cols) == NCOLS
    return cols


class Leg:
    """One batch running config 2's loop, with what its leg adds behind every range's step launch."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.bodies = [model.name2id(1, name) for name in ("left-foot", "right-foot", "cassie-pelvis")]
        self.b = b = Batch(model, n)
        dev = torch.device("cuda")
        rng = np.random.default_rng(1)
        self.tgt = torch.from_numpy(bench.PD_OFFSET + rng.uniform(-0.3, 0.3, (n, 10))).to(dev)
        self.cfrc = torch.zeros((n, 3 * pod.nbody), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        b.bind(P.F_PD_PTARGET, self.tgt.data_ptr())
        b.bind(P.F_BODY_CFRC, self.cfrc.data_ptr())
        b.set(P.F_QPOS, np.tile(model.qpos_init(), (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([model.qpos_init(), sens0])).cuda()
        self.rows = torch.zeros((n, NCOLS), dtype=torch.float32, device=dev)
        self.flags = torch.zeros(n, dtype=torch.int32, device=dev)
        if leg == "events":
            b.configure_events(event_columns(*self.bodies), dtype=np.float32, done_mask=[FLY, PEL])
            b.bind_event_rows(self.rows.data_ptr(), NCOLS)
            b.bind_event_flags(self.flags.data_ptr())
        if leg == "torch":
            self.contact = torch.zeros((n, 2), dtype=torch.bool, device=dev)     # the previous contact flags
            self.on_t = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            self.off_t = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            self.peak = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            self.flight = torch.zeros(n, dtype=torch.int32, device=dev)
            self.pelvis = torch.zeros(n, dtype=torch.bool, device=dev)
            self.first = torch.ones(n, dtype=torch.bool, device=dev)
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.policy_step = 0
        self.rates = []

    def torch_events(self, e0, cnt):
        """The row and the done words of the range as a user makes them today (on the current stream)."""
        s = slice(e0, e0 + cnt)
        lf, rf, pel = self.bodies
        f = self.cfrc[s]
        force = torch.stack([f[:, 3 * k:3 * k + 3].norm(dim=1) for k in (lf, rf, pel)], dim=1)
        feet, first = force[:, :2], self.first[s]
        was = self.contact[s] & ~first[:, None]
        now = torch.where(was, feet > OFF_THR, feet >= ON_THR)
        prev = torch.where(first[:, None], now, was)
        off_before = self.off_t[s].clone()
        on_t = torch.where(now, self.on_t[s] + 1, torch.zeros_like(self.on_t[s]))
        off_t = torch.where(now, torch.zeros_like(off_before), off_before + 1)
        down, up = now & ~prev, ~now & prev
        air = torch.where(down, DT * off_before.double(), torch.zeros_like(force[:, :2]))
        peak = torch.maximum(torch.where(down, torch.zeros_like(feet), self.peak[s]), feet)
        neither = ~now.any(dim=1)
        flight = torch.where(neither, self.flight[s] + 1, torch.zeros_like(self.flight[s]))
        fly = DT * flight.double() >= K_OFF * DT
        pelvis = force[:, 2] >= PEL_THR
        self.contact[s], self.on_t[s], self.off_t[s], self.peak[s], self.flight[s], self.pelvis[s] = now, on_t, off_t, peak, flight, pelvis
        self.first[s] = False
        row = torch.cat([force, now.double(), DT * on_t.double(), DT * off_t.double(), down.double(), up.double(), air, peak, neither.double()[:, None],
                         (DT * flight.double())[:, None], fly.double()[:, None], pelvis.double()[:, None]], dim=1)
        self.rows[s] = row.float()
        self.flags[s] = (fly | pelvis).int()

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        for (first, cnt), st in zip(self.ranges, self.streams):
            r0, k = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
            if k:
                b.reset_envs(r0, bench.NGROUP, k, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            if self.leg == "events":
                b.events(first, cnt, stream=st.cuda_stream)
            elif self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_events(first, cnt)

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
        if self.leg != "loop":
            rows = self.rows.cpu().numpy()
            out["columns"] = NCOLS
            out["finite_rows"] = int(np.isfinite(rows).all(axis=1).sum())
            out["envs_with_a_foot_on_the_ground"] = int((rows[:, CL:CR + 1] > 0).any(axis=1).sum())
            out["envs_done_now"] = int(self.flags.cpu().numpy().astype(bool).sum())
        if self.leg == "events":
            out["event_launches"] = self.b.event_launches()
            out["row"] = {"columns": NCOLS, "dtype": "float32", "bytes_per_env": 4 * NCOLS, "state_bytes_per_env": (16 + 4) * NCOLS + 4}
            # the call alone over the whole batch on an idle device: device events round 20 calls
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = self.streams[0]
            self.b.events(0, self.n, stream=st.cuda_stream)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev0.record()
                for _ in range(20):
                    self.b.events(0, self.n, stream=st.cuda_stream)
                ev1.record()
            torch.cuda.synchronize()
            out["events_call_alone_us"] = 1000.0 * ev0.elapsed_time(ev1) / 20
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
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): its `loop` leg, in child processes")
    a = ap.parse_args()
    out = {"tool": "event_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams, restarts on the benchmark's schedule (config 2); "
                   "the legs alternate region by region in one process; the event row of a range behind its step launch",
           "yardstick": "loop"}
    if a.parent_lib:
        # (first, in fresh processes of their own: one library per process; this process has not touched the GPU yet)
        def alone(lib):
            cmd = [sys.executable, os.path.abspath(__file__), "--only", "loop", "--envs", str(a.envs), "--launches", str(a.launches),
                   "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
            env = dict(os.environ, CASSIE_LIB=os.path.abspath(lib)) if lib else {k: v for k, v in os.environ.items() if k != "CASSIE_LIB"}
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                sys.exit("a child leg failed:\n" + r.stderr[-2000:])
            return json.loads(r.stdout.strip().splitlines()[-1])["loop"]

        def pooled(runs):
            r = [v for run in runs for v in run["regions"]]
            return {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
                    "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r,
                    "run_medians": [run["env_steps_per_s_median"] for run in runs], "envs_with_warnings": sum(run["envs_with_warnings"] for run in runs)}

        runs = [alone(lib) for lib in (a.parent_lib, None, None, a.parent_lib)]
        out["parent_loop"], out["loop_alone"] = pooled([runs[0], runs[3]]), pooled([runs[1], runs[2]])
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
        out["loop_spread_percent"] = out["loop"]["spread_percent_of_median"]
    if "events" in out and "torch" in out:
        one, many = out["events"]["env_steps_per_s_median"], out["torch"]["env_steps_per_s_median"]
        out["cheaper_event_leg"] = "events" if one > many else "torch"
        out["events_lose_less_than_torch"] = bool(one > many)
        out["largest_spread_of_a_leg_percent"] = max(out[name]["spread_percent_of_median"] for name in LEGS if name in out)
        if "loop" in out:
            out["events_cost_no_more_than_the_loops_spread"] = bool(out["events"]["cost_of_the_loop_percent"] <= out["loop_spread_percent"])
            out["difference_of_the_event_legs_percent_of_loop"] = 100.0 * abs(one - many) / out["loop"]["env_steps_per_s_median"]
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
