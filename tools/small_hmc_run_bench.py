"""A RUN of plain-HMC toy-target steps (`Dynamics(..., hmc=True)`), ms per MCMC step:
  (a) loop : `DynamicsSampler.run`, which takes an hmc dynamics through the loop over `propose` -- fill_normal,
             l2hmc_small_trajectory, ones_like, fill_uniform, l2hmc_mix_accept and the host work between them per step
             (the path before the run kernel; this change leaves its code alone);
  (b) run  : `DynamicsSampler.run_hmc`, l2hmc_small_hmc_run at `steps_per_launch` = 256;
  and, at config 2, (b) with a three-value ladder of step sizes and (b) with a three-value ladder of temperatures.
    python tools/small_hmc_run_bench.py > profiles/small_hmc_run.txt

Shapes: BASELINE config 1 (SCG, 128 chains, 5 LF), config 2 (MoG, 4096 chains, 10 LF) and the reference's evaluation
shape (mog_model.py:394: MoG, 500 chains, 100 steps per call).

A window is `run(STEPS, x)` / `run_hmc(STEPS, x)` between two device synchronisations on the host clock, in the same
process for all variants.  STEPS is chosen per row so that a window of the loop lasts about `--window` seconds (a
multiple of 256, the same for all variants; the evaluation shape is also timed at its own 100 steps), after a warm-up
window of the same length; the variants alternate, REPS windows each.  Reported: median (min .. max).  A window includes
what a caller pays for: the accept probabilities' copy to the host (and, with `--keep-samples`, the samples')."""
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
EPS_LADDER = (0.05, 0.1, 0.2)
TEMP_LADDER = (1.0, 2.0, 4.0)
# name, target, chains, LF steps, fixed step count (None = by --window), with the ladders
SHAPES = [("cfg 1", "scg", 128, 5, None, False), ("cfg 2", "mog", 4096, 10, None, True),
          ("eval", "mog", 500, 10, None, False), ("eval, 100 steps", "mog", 500, 10, 100, False)]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of the loop per timed window (sets the step count)")
ap.add_argument("--keep-samples", action="store_true")
ap.add_argument("--label", default="this tree")
args = ap.parse_args()


def sampler(target, N):
    np.random.seed(0)
    torch.manual_seed(0)
    if target == "scg":
        dist = la.Gaussian(np.zeros(2), SCG_SIGMA)
    else:
        dist = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
    dyn = la.Dynamics(2, dist.get_energy_function(), trajectory_length=N, eps=0.1, hmc=True, use_temperature=True)
    return la.DynamicsSampler(dyn, distribution=dist)


def window(call, x, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = call(steps, x)["samples_out"]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, x


fmt = lambda v: f"{statistics.median(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
LOOP, RUN, EPS, TEMP = "(a) loop", "(b) run_hmc, 256 / launch", "(b) + eps ladder", "(b) + temperature ladder"
print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; plain HMC (hmc=True), x_dim 2, eps 0.1, keep_samples="
      f"{args.keep_samples}; ms per MCMC step: median (min .. max) of {args.reps} alternating windows")
print(f"# eps ladder {EPS_LADDER}, temperature ladder {TEMP_LADDER}: chain c takes entry c % 3")
for name, target, B, N, fixed, ladders in SHAPES:
    ks = args.keep_samples
    smp = {k: sampler(target, N) for k in ((LOOP, RUN, EPS, TEMP) if ladders else (LOOP, RUN))}
    assert all(s.steps_per_launch == 256 for s in smp.values())
    eps = np.array(EPS_LADDER, dtype=np.float32)[np.arange(B) % 3]
    temps = np.array(TEMP_LADDER, dtype=np.float32)[np.arange(B) % 3][None]
    calls = {LOOP: lambda n, x: smp[LOOP].run(n, x, keep_samples=ks),
             RUN: lambda n, x: smp[RUN].run_hmc(n, x, keep_samples=ks)}
    if ladders:
        calls[EPS] = lambda n, x: smp[EPS].run_hmc(n, x, keep_samples=ks, eps=eps)
        calls[TEMP] = lambda n, x: smp[TEMP].run_hmc(n, x, keep_samples=ks, temperature=temps)
    x0 = la._lib.as_dev(smp[LOOP].distribution.get_samples(B))
    xs = {k: x0.clone() for k in calls}
    dt, xs[LOOP] = window(calls[LOOP], xs[LOOP], 256)            # first touch, and the step count
    dt, xs[LOOP] = window(calls[LOOP], xs[LOOP], 256)
    steps = fixed or max(2, round(args.window / (dt * 1e-3) / 256)) * 256
    for k in calls:                                              # warm-up at the windows' own size
        _, xs[k] = window(calls[k], xs[k], steps)
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k in calls:
            dt, xs[k] = window(calls[k], xs[k], steps)
            times[k].append(dt)
    print(f"  {name}: {target}, {B} chains, {N} LF, {steps} steps per window")
    base = statistics.median(times[RUN])
    for k in calls:
        rel = (f"(a) / (b) = {statistics.median(times[LOOP]) / base:6.2f}x" if k == RUN else
               "" if k == LOOP else f"/ (b) = {statistics.median(times[k]) / base:5.3f}")
        print(f"    {k:>26} | {fmt(times[k]):>30} | {rel}", flush=True)
    del smp, xs, calls
