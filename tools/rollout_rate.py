#!/usr/bin/env python3
"""What the rollout rows cost config 2's loop -- 4096 cassie.xml envs, CM_DRIVE_PD_SAFE, 50 fused substeps per launch, the batch as two env
ranges on two streams -- with EVERY link of a policy step in place: per range and policy step end_episodes (a time limit of
bench.NGROUP policy steps, the counters started apart, and the events' done words as `force`), task (tools/task_rate.py's 21 columns),
observe (340 float32), policy (tools/policy_rate.py's actor and critic), act, the step launch, events (tools/event_rate.py's 21 columns),
reward (tools/reward_rate.py's 12 terms, float32).  Three legs ALTERNATE in one process on one box, fenced timed regions, ten each:

  loop          the loop alone.  THE YARDSTICK.
  rollout       the same plus one phys_batch_rollout_record per range and policy step behind end_episodes -- obs (340), action (10), logp,
                mu (10), value, reward, done, reason, every one resolved from the batch's bindings -- and every T = 24 policy steps one
                phys_batch_rollout_finish per range behind its policy call (the NULL last value) and one phys_batch_rollout_normalise
                behind both.
  torch         the same written in torch on the same streams: a copy_ per tensor per range per policy step into [T][nenv][dim] tensors,
                every T steps the backward loop with (1 - done) products per range and mean() / std() over the batch.  What a user
                does today, in fp32.

--parent-lib PATH runs the loop ALONE (no stage of a policy step: the loop every earlier measurement of "unused, it costs nothing"
timed) in child processes, in the order parent, this build, this build, parent: like against like, one batch in a fresh process of its
own, the regions of a build's two runs pooled.  No stepping kernel changes with the rollout rows, so this build's median should lie
inside the parent's regions.

Also times the three calls alone over the whole batch on an idle device; for record it states the bytes moved and the achieved GB/s.
Every region is recorded.  Prints one JSON line; `--out` also writes it to a file.  Needs a GPU.

    python tools/rollout_rate.py [--envs 4096] [--launches 24] [--warmup 24] [--repeats 10] [--only NAME] [--out profiles/rollout_rate.json]
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
import event_rate  # noqa: E402
import obs_rate  # noqa: E402
import policy_rate  # noqa: E402
import reward_rate  # noqa: E402
import task_rate  # noqa: E402
import torch  # noqa: E402
from cassie_amd import Batch, Model  # noqa: E402
from cassie_amd import phys as P  # noqa: E402

NSUB = bench.HOLD
LEGS = ("loop", "rollout", "torch")
T, GAMMA, LAMBDA, EPS = 24, 0.99, 0.95, 1e-8
NACT, NOBS = policy_rate.NACT, policy_rate.NOBS
SOURCES = (("obs", NOBS), ("action", NACT), ("logp", 1), ("mu", NACT), ("value", 1), ("reward", 1), ("done", 1), ("reason", 1))
WORDS = sum(d for _, d in SOURCES)


class Leg:
    """One batch running config 2's loop with every stage of a policy step in place, and what its leg adds.  leg "bare": the loop alone
    (what --parent-lib compares)."""

    def __init__(self, model, n, leg):
        pod = model.pod
        self.leg, self.n, self.pod = leg, n, pod
        self.b = b = Batch(model, n)
        dev = torch.device("cuda")
        rng = np.random.default_rng(1)
        q0 = model.qpos_init()
        if leg != "bare":
            self.cfrc = torch.zeros((n, 3 * pod.nbody), dtype=torch.float64, device=dev)
            self.xfrc = torch.zeros((n, 6 * pod.nbody), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            b.bind(P.F_BODY_CFRC, self.cfrc.data_ptr())
        b.set(P.F_QPOS, np.tile(q0, (n, 1)))
        b.forward()
        sens0 = b.get(P.F_SENSORDATA, 0, 1)[0]
        b.set(P.F_PD_KP, np.tile(bench.PD_KP, (n, 1)))
        b.set(P.F_PD_KD, np.tile(bench.PD_KD, (n, 1)))
        b.set(P.F_PD_PTARGET, bench.PD_OFFSET + rng.uniform(-0.3, 0.3, (n, NACT)))
        b.set_drive_mode(P.DRIVE_PD_SAFE)
        self.init_row = torch.from_numpy(np.concatenate([q0, sens0])).cuda()
        if leg != "bare":
            f32 = dict(dtype=torch.float32, device=dev)
            self.task_rows, self.obs = torch.zeros((n, task_rate.NCOLS), **f32), torch.zeros((n, NOBS), **f32)
            self.actions = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, NACT)).astype(np.float32)).to(dev)
            self.value, self.mu, self.logp = torch.zeros((n, 1), **f32), torch.zeros((n, NACT), **f32), torch.zeros(n, **f32)
            self.rew, self.ev_rows = torch.zeros(n, **f32), torch.zeros((n, event_rate.NCOLS), **f32)
            self.flags = torch.zeros(n, dtype=torch.int32, device=dev)
            self.done, self.reason = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
            self.steps0 = torch.from_numpy((np.arange(n) % bench.NGROUP).astype(np.int32)).cuda()
            torch.manual_seed(1)
            self.rew_in = torch.rand((n, reward_rate.NINPUT), **f32)
            torch.cuda.synchronize()
            b.bind(P.F_XFRC_APPLIED, self.xfrc.data_ptr())
            b.enable_episodes(max_steps=bench.NGROUP)
            b.set_reset_bank(b.make_reset_bank(q0[None]))
            b.bind_episode(P.EP_STEPS, self.steps0.data_ptr())
            b.bind_episode(P.EP_DONE, self.done.data_ptr())
            b.bind_episode(P.EP_REASON, self.reason.data_ptr())
            b.set_task_table(task_rate.reference_table())
            b.configure_task(task_rate.task_columns(pod), dtype=np.float32, seed=1)
            b.bind_task_rows(self.task_rows.data_ptr(), task_rate.NCOLS)
            b.configure_obs(obs_rate.obs_terms(pod), history=obs_rate.HISTORY, dtype=np.float32, seed=1)
            b.bind_obs(self.obs.data_ptr())
            b.bind_obs_input(self.task_rows.data_ptr(), obs_rate.NINPUT, task_rate.NCOLS, torch.float32)
            b.configure_actions(policy_rate.act_columns(), dtype=np.float32, seed=1)
            b.bind_actions(self.actions.data_ptr(), NACT, torch.float32)
            b.bind_action_input(self.task_rows.data_ptr(), task_rate.NCOLS, task_rate.NCOLS, torch.float32)
            bodies = [model.name2id(1, name) for name in ("left-foot", "right-foot", "cassie-pelvis")]
            b.configure_events(event_rate.event_columns(*bodies), dtype=np.float32, done_mask=[event_rate.FLY, event_rate.PEL])
            b.bind_event_rows(self.ev_rows.data_ptr(), event_rate.NCOLS)
            b.bind_event_flags(self.flags.data_ptr())
            b.configure_rewards(reward_rate.reward_terms(), dtype=np.float32, lo=reward_rate.LO, hi=reward_rate.HI)
            b.bind_rewards(self.rew.data_ptr())
            b.bind_reward_input(self.rew_in.data_ptr(), reward_rate.NINPUT, reward_rate.NINPUT, torch.float32)
            wrng = np.random.default_rng(2)
            H = policy_rate.HIDDEN
            nets = [policy_rate.weights(wrng, (NOBS, H, H, NACT)), policy_rate.weights(wrng, (NOBS, H, H, 1))]
            self.mean = torch.from_numpy((0.1 * wrng.normal(size=NOBS)).astype(np.float32)).to(dev)
            self.inv = torch.from_numpy(wrng.uniform(0.5, 2.0, NOBS).astype(np.float32)).to(dev)
            self.log_std = torch.full((NACT,), policy_rate.LOG_STD, **f32)
            self.eps = torch.from_numpy(np.clip(wrng.normal(size=(4, n, NACT)), -4, 4).astype(np.float32)).to(dev)
            acts = [P.POL_ELU, P.POL_ELU, P.POL_IDENTITY]
            b.configure_policy([[P.pol_layer(w.shape[0], a) for (w, _), a in zip(net, acts)] for net in nets], NOBS)
            for k, net in enumerate(nets):
                b.load_policy(k, net)
            b.bind_policy_input(self.obs.data_ptr(), NOBS, NOBS, torch.float32)
            b.bind_policy_norm(self.mean.data_ptr(), self.inv.data_ptr(), policy_rate.CLIP)
            b.bind_policy_output(0, self.mu.data_ptr(), NACT)
            b.bind_policy_output(1, self.value.data_ptr(), 1)
        if leg == "rollout":
            b.configure_rollout(T, SOURCES, GAMMA, LAMBDA, timeout_mask=P.DONE_TIME)
        if leg == "torch":
            self.live = {"obs": self.obs, "action": self.actions, "logp": self.logp, "mu": self.mu, "value": self.value[:, 0], "reward": self.rew,
                         "done": self.done, "reason": self.reason}
            self.store = {name: torch.zeros((T,) + tuple(t.shape), dtype=t.dtype, device=dev) for name, t in self.live.items()}
            self.adv, self.ret, self.advn = (torch.zeros((T, n), **f32) for _ in range(3))
        b.sync()
        torch.cuda.synchronize()
        self.streams, half = [torch.cuda.Stream(), torch.cuda.Stream()], n // 2
        self.ranges = [(0, half), (half, n - half)]
        self.joined, self.normalised = torch.cuda.Event(), torch.cuda.Event()
        self.policy_step = 0
        self.rates = []

    def torch_record(self, t, e0, cnt):
        s = slice(e0, e0 + cnt)
        for name, live in self.live.items():
            self.store[name][t, s].copy_(live[s])

    def torch_finish(self, e0, cnt):
        """The usual backward loop, as a user writes it (on the current stream)."""
        s = slice(e0, e0 + cnt)
        val, rew, done, reason = (self.store[k][:, s] for k in ("value", "reward", "done", "reason"))
        nv, a = self.value[s, 0], torch.zeros(cnt, dtype=torch.float32, device=val.device)
        for t in range(T - 1, -1, -1):
            live = 1.0 - (done[t] != 0).float()
            r = torch.where((done[t] != 0) & (reason[t] == P.DONE_TIME), rew[t] + GAMMA * val[t], rew[t])
            delta = r + GAMMA * nv * live - val[t]
            a = delta + GAMMA * LAMBDA * live * a
            self.adv[t, s] = a
            self.ret[t, s] = a + val[t]
            nv = val[t]

    def launch(self):
        b, p = self.b, self.policy_step
        self.policy_step += 1
        t = p % T
        if self.leg != "bare":
            b.bind_policy_sample(self.eps[p % 4].data_ptr(), self.log_std.data_ptr(), self.actions.data_ptr(), self.logp.data_ptr())
        for k, ((first, cnt), st) in enumerate(zip(self.ranges, self.streams)):
            if self.leg == "bare":
                r0, m = bench.rows_of_group_in_range(bench.restart_group(p), 0, first, cnt)
                if m:
                    b.reset_envs(r0, bench.NGROUP, m, self.init_row.data_ptr(), self.init_row.data_ptr() + 8 * self.pod.nq, st.cuda_stream)
                b.step_range(first, cnt, NSUB, st.cuda_stream)
                continue
            done = self.done.data_ptr() + 4 * first
            b.end_episodes(first, cnt, True, force_ptr=self.flags.data_ptr() + 4 * first, stream=st.cuda_stream)
            if self.leg == "rollout":
                b.rollout_record(t, first, cnt, stream=st.cuda_stream)
            elif self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_record(t, first, cnt)
            b.task(first, cnt, reset_ptr=done, stream=st.cuda_stream)
            b.observe(first, cnt, refill_ptr=done, stream=st.cuda_stream)
            b.policy(first, cnt, stream=st.cuda_stream)
            if t == T - 1 and self.leg == "rollout":
                b.rollout_finish(first, cnt, stream=st.cuda_stream)
            elif t == T - 1 and self.leg == "torch":
                with torch.cuda.stream(st):
                    self.torch_finish(first, cnt)
            b.act(first, cnt, reset_ptr=done, stream=st.cuda_stream)
            b.step_range(first, cnt, NSUB, st.cuda_stream)
            b.events(first, cnt, reset_ptr=done, stream=st.cuda_stream)
            b.reward(first, cnt, reset_ptr=done, stream=st.cuda_stream)
        if t == T - 1 and self.leg in ("rollout", "torch"):
            # the normalisation behind both ranges' finish, on the first range's stream; the second range's next finish behind it
            s0, s1 = self.streams
            self.joined.record(s1)
            s0.wait_event(self.joined)
            if self.leg == "rollout":
                b.rollout_normalise(EPS, stream=s0.cuda_stream)
            else:
                with torch.cuda.stream(s0):
                    self.advn.copy_((self.adv - self.adv.mean()) / (self.adv.std() + EPS))
            self.normalised.record(s0)
            s1.wait_event(self.normalised)

    def region(self, launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(launches):
            self.launch()
        torch.cuda.synchronize()
        self.rates.append(self.n * NSUB * launches / (time.perf_counter() - t0))

    def timed(self, call, reps=20):
        """Microseconds of a call alone on an idle device: device events round `reps` calls on one stream."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = self.streams[0]
        with torch.cuda.stream(st):
            call(st)
            torch.cuda.synchronize()
            ev0.record()
            for _ in range(reps):
                call(st)
            ev1.record()
        torch.cuda.synchronize()
        return 1000.0 * ev0.elapsed_time(ev1) / reps

    def report(self):
        r = self.rates
        out = {"env_steps_per_s_median": float(np.median(r)), "env_steps_per_s_min": float(min(r)), "env_steps_per_s_max": float(max(r)),
               "spread_percent_of_median": 100.0 * (max(r) - min(r)) / float(np.median(r)), "regions": r,
               "envs_with_warnings": int(self.b.warnings()[0].astype(bool).sum())}
        if self.leg == "bare":
            return out
        out["episodes_ended"] = int(self.b.episodes()[3].sum())
        n, b = self.n, self.b
        if self.leg == "rollout":
            out["rollout_launches_record_finish_normalise"] = list(b.rollout_launches())
            adv, advn, done = b.rollout("adv"), b.rollout("advn"), b.rollout("done")
            mean, std, inv = b.rollout_stats()
            out.update(finite_advantages=int(np.isfinite(adv).sum()), advantages=int(adv.size), done_steps_in_store=int((done != 0).sum()),
                       mean=mean, std=std, normalised_mean=float(advn.astype(np.float64).mean()), normalised_std=float(advn.astype(np.float64).std(ddof=1)))
            out["record_alone_us"] = self.timed(lambda st: b.rollout_record(0, 0, n, stream=st.cuda_stream))
            out["record_bytes_moved"] = 2 * 4 * WORDS * n
            out["record_GB_per_s"] = out["record_bytes_moved"] / (out["record_alone_us"] * 1e-6) / 1e9
            out["finish_alone_us"] = self.timed(lambda st: b.rollout_finish(0, n, stream=st.cuda_stream))
            out["normalise_alone_us"] = self.timed(lambda st: b.rollout_normalise(EPS, stream=st.cuda_stream))
        if self.leg == "torch":
            out["finite_advantages"], out["advantages"] = int(torch.isfinite(self.adv).sum()), int(self.adv.numel())
            out["mean"], out["std"] = float(self.adv.mean()), float(self.adv.std())
            out["record_alone_us"] = self.timed(lambda st: self.torch_record(0, 0, n))
            out["finish_alone_us"] = self.timed(lambda st: self.torch_finish(0, n), reps=5)
            out["normalise_alone_us"] = self.timed(lambda st: self.advn.copy_((self.adv - self.adv.mean()) / (self.adv.std() + EPS)))
        return out

    def close(self):
        self.b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=T)
    ap.add_argument("--warmup", type=int, default=T)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--only", choices=list(LEGS) + ["bare"], default=None, help="one leg only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's): the loop alone, in child processes")
    a = ap.parse_args()
    out = {"tool": "rollout_rate", "model": "cassie", "envs": a.envs, "substeps_per_launch": NSUB, "launches_per_region": a.launches,
           "warmup_launches": a.warmup, "regions_per_leg": a.repeats, "rollout_steps": T, "words_per_env_and_step": WORDS,
           "mode": "CM_DRIVE_PD_SAFE, 50 fused substeps per launch, two env ranges on two streams (config 2); end_episodes (time limit, the events' "
                   "done words as force), task, observe (340 float32), policy, act, events and reward in place; the legs alternate region by "
                   "region in one process; a region is one rollout of T policy steps, so every region of the two rollout legs holds one finish "
                   "per range and one normalise",
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
    if "rollout" in out and "torch" in out:
        one, many = out["rollout"]["env_steps_per_s_median"], out["torch"]["env_steps_per_s_median"]
        out["cheaper_rollout_leg"] = "rollout" if one > many else "torch"
        out["largest_spread_of_a_leg_percent"] = max(out[name]["spread_percent_of_median"] for name in LEGS if name in out)
        out["rollout_ahead_of_torch_percent_of_the_loop"] = 100.0 * (one - many) / out["loop"]["env_steps_per_s_median"] if "loop" in out else None
        out["rollout_ahead_by_more_than_the_largest_spread"] = bool(out["rollout_ahead_of_torch_percent_of_the_loop"] is not None and
                                                                    out["rollout_ahead_of_torch_percent_of_the_loop"] > out["largest_spread_of_a_leg_percent"])
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
