"""A RUN of toy-target L2HMC steps (`DynamicsSampler.run`), ms per MCMC step:
  (a) loop : `steps_per_launch = 1`, one l2hmc_small_propose launch and one round of host work per step (the path
             before the run kernel; this change leaves its code alone);
  (b) run  : l2hmc_small_run, `steps_per_launch` = 256.
    python tools/small_run_bench.py > profiles/small_run.txt

Shapes: BASELINE config 1 (SCG, 128 chains, 5 LF, 10 nodes), config 2 (MoG, 4096 chains, 10 LF, 50 nodes) and the
reference's evaluation shape (mog_model.py:394: MoG, 500 chains, 100 steps per call).

A window is `run(STEPS, x)` between two device synchronisations on the host clock, in the same process for both
variants.  STEPS is chosen per row so that a window of the loop lasts about `--window` seconds (a multiple of 256, the
same for both variants; the evaluation shape is also timed at its own 100 steps), after a warm-up window of the same
length; the variants alternate, REPS windows each.  Reported: median (min .. max).  `run` includes what a caller pays
for: the accept probabilities' copy to the host (and, with `--keep-samples`, the samples')."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import l2hmc_amd as la  # noqa: E402

SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
# name, target, chains, LF steps, nodes, fixed step count (None = by --window)
SHAPES = [("cfg 1", "scg", 128, 5, 10, None), ("cfg 2", "mog", 4096, 10, 50, None),
          ("eval", "mog", 500, 10, 50, None), ("eval, 100 steps", "mog", 500, 10, 50, 100)]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of the loop per timed window (sets the step count)")
ap.add_argument("--keep-samples", action="store_true")
ap.add_argument("--label", default="this tree")
args = ap.parse_args()


def sampler(target, N, nodes, spl):
    np.random.seed(0)
    torch.manual_seed(0)
    if target == "scg":
        dist = la.Gaussian(np.zeros(2), SCG_SIGMA)
    else:
        dist = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
    dyn = la.Dynamics(2, dist.get_energy_function(), trajectory_length=N, eps=0.1,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    smp = la.DynamicsSampler(dyn, distribution=dist)
    smp.steps_per_launch = spl
    return smp


def run_window(smp, x, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = smp.run(steps, x, keep_samples=args.keep_samples)["samples_out"]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, x


fmt = lambda v: f"{statistics.median(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; DynamicsSampler.run, x_dim 2, eps 0.1, keep_samples="
      f"{args.keep_samples}; ms per MCMC step: median (min .. max) of {args.reps} alternating windows")
cols = ["(a) loop, 1 / launch", "(b) run, 256 / launch"]
print(f"# {'shape':>16} {'target':>6} {'chains':>6} {'LF':>3} {'nodes':>5} {'steps':>6} | "
      + " | ".join(f"{c:>26}" for c in cols) + " | (a) / (b)")
for name, target, B, N, nodes, fixed in SHAPES:
    var = {cols[0]: sampler(target, N, nodes, 1), cols[1]: sampler(target, N, nodes, 256)}
    x0 = la._lib.as_dev(var[cols[0]].distribution.get_samples(B))
    xs = {k: x0.clone() for k in var}
    dt, xs[cols[0]] = run_window(var[cols[0]], xs[cols[0]], 256)              # first touch, and the step count
    dt, xs[cols[0]] = run_window(var[cols[0]], xs[cols[0]], 256)
    steps = fixed or max(2, round(args.window / (dt * 1e-3) / 256)) * 256
    for k in var:                                              # warm-up at the windows' own size
        _, xs[k] = run_window(var[k], xs[k], steps)
    times = {c: [] for c in cols}
    for _ in range(args.reps):
        for k in var:
            dt, xs[k] = run_window(var[k], xs[k], steps)
            times[k].append(dt)
    ratio = statistics.median(times[cols[0]]) / statistics.median(times[cols[1]])
    print(f"  {name:>16} {target:>6} {B:6d} {N:3d} {nodes:5d} {steps:6d} | "
          + " | ".join(f"{fmt(times[c]):>26}" for c in cols) + f" | {ratio:6.2f}x", flush=True)
    del var, xs
