"""Replica exchange between the rungs of a plain-HMC toy-target temperature ladder, the rounds INSIDE the launch
(`DynamicsSampler.run_hmc_exchange`, l2hmc_small_hmc_run_exchange), against the ladder run it is built on (`run_hmc`)
and against the loop a caller would write without it (`run_hmc(k)`, `swap_replicas`), in the manner of
tools/hmc_replica_exchange_bench.py.  8 rungs (chain c at TEMPS[c % 8], temperature 1.0 .. 4.5), `steps_per_launch` = 256,
keep_samples=False, ms per MCMC step:
  (a) no exchange : `run_hmc` of the ladder (`--plain-only` times just this, and also works on a tree that has no
                    exchange: `--tree PATH` imports the package of another, built, tree -- the parent commit);
  (b) in launch   : `run_hmc_exchange(..., replicas=8, swap_every=k)` for k = 1, 4, 16;
  (c) loop        : `run_hmc(k, ...)` then `swap_replicas(...)`, the same values with 1 + 1 launches per k steps
                    (its rounds' histories stay on the device and are dropped, which (b) copies to the host);
  and per row the launches of (a) and (b) alone (l2hmc_profile class 7), from which a round's cost inside the launch.
    python tools/small_hmc_exchange_bench.py > table.txt
    python tools/small_hmc_exchange_bench.py --stats      (the sampling figures below instead of the timings)
profiles/small_hmc_replica_exchange.txt is made of two passes of each, and of (a) on the parent commit.

Shapes: BASELINE config 1 (SCG, 128 chains, 5 LF) and config 2 (the 2-D mixture, 4096 chains, 10 LF).

A window is `steps` MCMC steps between two device synchronisations on the host clock, `steps` a multiple of 256 chosen
per row so that a window of (c) at swap_every = 1 lasts about `--window` seconds, after a warm-up window of the same
length; the variants of a row alternate, REPS windows each.  Reported: median (min .. max).  Every variant includes what
its caller pays for: the histories' copy to the host and the mean accept probability.

--stats: ONE seeded run (seed 11) of the README's mixture (sigma^2 = 0.025) at temperatures (1, 1.5, 2, 3), 2048 chains =
512 groups, eps 0.1, 10 leapfrog steps, from the target's own samples, `--stats-steps` steps after `--therm` steps,
without exchange and with swap_every = 1 and 4: the swap rate per neighbouring pair of rungs, the tunnelling rate of the
T = 1 columns (`stats.calc_tunneling_rate`), and the completed round trips (lowest rung -> highest -> lowest,
`stats.replica_round_trips`) per group and 1000 steps."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of (c, swap_every = 1) per timed window")
ap.add_argument("--label", default="this tree")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="root of the (built) tree whose l2hmc_amd is measured")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--steps", type=int, default=None,
                help="steps per window instead of the count --window gives (with --plain-only: the count of the full table)")
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-steps", type=int, default=4096)
ap.add_argument("--therm", type=int, default=512)
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
import l2hmc_amd as la  # noqa: E402

SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
SHAPES = [("cfg 1", "scg", 128, 5), ("cfg 2", "mog", 4096, 10)]       # rows of profiles/small_hmc_run.txt
RUNGS = 8
TEMPS = np.linspace(1.0, 4.5, RUNGS)
SWAP_EVERY = (1, 4, 16)


def mixture():
    return la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])


def sampler(target, N, seed=None):
    np.random.seed(0)
    torch.manual_seed(0)
    dist = la.Gaussian(np.zeros(2), SCG_SIGMA) if target == "scg" else mixture()
    kw = {} if seed is None else {"seed": seed}
    dyn = la.Dynamics(2, dist.get_energy_function(), trajectory_length=N, eps=0.1, hmc=True, use_temperature=True, **kw)
    return la.DynamicsSampler(dyn, distribution=dist)


class Run:
    """`run_hmc` of the ladder (swap_every None), `run_hmc_exchange` with a round every `swap_every` steps, or
    (`loop`) the same run as `run_hmc(swap_every)`, `swap_replicas`"""

    def __init__(self, target, B, N, swap_every=None, loop=False):
        self.smp = sampler(target, N)
        assert self.smp.steps_per_launch == 256
        self.x = la._lib.as_dev(self.smp.distribution.get_samples(B))
        t = TEMPS[np.arange(B) % RUNGS].astype(np.float32)
        self.temps, self.temps_dev = t[None, :], la._lib.as_dev(t)
        self.k, self.loop, self.done = swap_every, loop, 0

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.k is None:
            self.x = self.smp.run_hmc(steps, self.x, keep_samples=False, temperature=self.temps)["samples_out"]
        elif not self.loop:
            out = self.smp.run_hmc_exchange(steps, self.x, keep_samples=False, temperature=self.temps, replicas=RUNGS,
                                            swap_every=self.k, first_parity=self.done % 2)
            self.x, self.done = out["samples_out"], self.done + steps // self.k
        else:
            px = []
            for _ in range(steps // self.k):
                out = self.smp.run_hmc(self.k, self.x, keep_samples=False, temperature=self.temps)
                self.x = out["samples_out"]
                px.append(out["px"])
                self.smp.swap_replicas(self.x, self.temps_dev, RUNGS, self.done % 2)
                self.done += 1
            float(np.concatenate(px).mean(dtype=np.float64))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


med = statistics.median


def timings():
    fmt = lambda v: f"{med(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
    print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; Dynamics(hmc=True), x_dim 2, eps 0.1, {RUNGS} rungs of "
          f"temperature {TEMPS[0]} .. {TEMPS[-1]}, 256 steps per launch, keep_samples=False; ms per MCMC step: median "
          f"(min .. max) of {args.reps} alternating windows")
    for name, target, B, N in SHAPES:
        var = {"(a) no exchange": Run(target, B, N)}
        if not args.plain_only:
            for k in SWAP_EVERY:
                var[f"(b) in launch, swap_every = {k}"] = Run(target, B, N, k)
                var[f"(c) loop,      swap_every = {k}"] = Run(target, B, N, k, loop=True)
        slowest = list(var)[-1 if args.plain_only else 2]              # (c) at swap_every = 1, or (a) alone
        var[slowest].window(256)                                       # first touch, and the step count
        dt = var[slowest].window(256)
        steps = args.steps or max(2, round(args.window / (dt * 1e-3) / 256)) * 256
        for c in var:                                                  # warm-up at the windows' own size
            var[c].window(steps)
        times = {c: [] for c in var}
        for _ in range(args.reps):
            for c in var:
                times[c].append(var[c].window(steps))
        print(f"  {name}: {target}, {B} chains, {N} LF, {steps} steps per window")
        a = med(times["(a) no exchange"])
        for c in var:
            rel = "" if c.startswith("(a)") else f"/ (a) = {med(times[c]) / a:6.3f}"
            if c.startswith("(c)"):
                b = c.replace("(c) loop,     ", "(b) in launch,")
                gap = "disjoint" if max(times[b]) < min(times[c]) else "OVERLAPPING"
                rel += f"   (c) / (b) = {med(times[c]) / med(times[b]):6.2f}x, ranges {gap}"
            print(f"    {c:>32} | {fmt(times[c]):>30} | {rel}", flush=True)
        # the launches alone (l2hmc_profile class 7: HIP events around every launch of the run kernel), one window each
        L = la._lib.lib()
        dev = {}
        for c in var:
            if c.startswith("(c)"):
                continue
            la._lib.check(L.l2hmc_profile_begin(7))
            var[c].window(steps)
            ms, n = C.c_double(), C.c_int64()
            la._lib.check(L.l2hmc_profile_end(C.byref(ms), C.byref(n)))
            dev[c] = (ms.value / steps, n.value)
        a_dev = dev["(a) no exchange"][0]
        print("    the run kernel alone, ms per MCMC step (launches): "
              + "; ".join(f"{c.split(',')[0][:3]}{c.split('=')[1] if '=' in c else ''} {v:.4f} ({n})"
                          + ("" if c.startswith("(a)") else f" = (a) + {(v - a_dev) * 1e3 * int(c.split('=')[1]):.2f} us per round")
                          for c, (v, n) in dev.items()), flush=True)
        del var


def sampling_figures():
    temps4 = np.array([1.0, 1.5, 2.0, 3.0], dtype=np.float32)
    G, B, N = 4, 2048, 10
    n, therm = args.stats_steps, args.therm
    temps = temps4[np.arange(B) % G][None, :]
    cold = np.arange(B) % G == 0
    print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; one seeded run (seed 11) of the 2-D mixture (means (1, 0), "
          f"(0, 1), sigma^2 0.025), {B} chains = {B // G} groups of {G} rungs at temperatures {tuple(float(t) for t in temps4)}, "
          f"eps 0.1, {N} leapfrog steps, from the target's samples, {therm} steps first (with the same exchange), then {n} steps")
    print("# T = 1 columns: tunnelling rate per step (stats.calc_tunneling_rate, mean over the columns) and accept; round "
          "trips: completed lowest -> highest -> lowest per group and 1000 steps")
    for k in (None,) + SWAP_EVERY[:2]:
        smp = sampler("mog", N, seed=11)
        x = la._lib.as_dev(smp.distribution.get_samples(B))
        kw = dict(temperature=temps) if k is None else dict(temperature=temps, replicas=G, swap_every=k)
        run = smp.run_hmc if k is None else smp.run_hmc_exchange
        out = run(therm, x, keep_samples=False, **kw)
        if k is not None:
            kw.update(first_parity=(therm // k) % 2, replica0=out["replica"][-1])
        t0 = time.perf_counter()
        out = run(n, out["samples_out"], keep_samples=True, **kw)
        dt = time.perf_counter() - t0
        rate = la.stats.calc_tunneling_rate(out["samples"][:, cold], np.stack(smp.distribution.mus)).mean()
        line = (f"  {'no exchange' if k is None else f'swap_every = {k:<2}':<16} T = 1 tunnelling rate {rate:.5f}  "
                f"accept(T = 1) {out['px'][:, cold].mean():.3f}")
        if k is not None:
            trips, groups = la.stats.replica_round_trips(out["replica"], G)
            line += (f"  round trips {groups.mean() / n * 1000:.3f}  swap_rate per pair "
                     + " ".join(f"{r:.3f}" for r in out["swap_rate"]))
        print(line + f"   ({dt:.1f} s)", flush=True)


if args.stats:
    sampling_figures()
else:
    timings()
