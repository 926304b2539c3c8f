"""A RUN of plain-HMC MCMC steps (`GaugeSampler.run` with `GaugeDynamics(hmc=True)`), ms per MCMC step:
  (a) loop   : `steps_per_launch = 1`, one launch and one round of host work per step (the path before the run kernel;
               `--loop-only` times just this and also works on a tree that has no `steps_per_launch`);
  (b) graph  : a HIP-graph replay of one l2hmc_gauge_mcmc_step per step (the launch boundary without the host work);
  (c) run    : l2hmc_gauge_hmc_run, `steps_per_launch` = 16 and 256.
    python tools/hmc_run_bench.py > table.txt          (profiles/hmc_run.txt alternates this with --loop-only on the parent tree)

A window is `run(STEPS, beta, x)` (or STEPS replays) between two device synchronisations on the host clock.  STEPS is
chosen per row so that a window of the loop lasts about `--window` seconds (a multiple of 256, the same for every
variant of the row; short windows of 10-20 ms let one host hiccup decide a median), after a warm-up window of the
same length; the variants of a row alternate, REPS windows each.  Reported: median (min .. max).  `run` includes what a
caller pays for: the histories' copy to the host and the mean accept probability.  `--label` names the tree in the
table's header (e.g. the revision)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from l2hmc_amd import GaugeDynamics, GaugeLattice, GaugeSampler, _lib  # noqa: E402

SHAPES = [(8, 8, 2048, 10), (16, 16, 1024, 15), (32, 32, 2048, 25), (6, 6, 2048, 10)]     # T, X, chains, LF steps

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of the loop per timed window (sets the step count)")
ap.add_argument("--label", default="this tree")
ap.add_argument("--loop-only", action="store_true")
args = ap.parse_args()
BETA = 2.0


def sampler(T, X, B, N, both, spl):
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=0.1, hmc=True, num_steps=N, both_directions=both)
    smp = GaugeSampler(dyn)
    if spl is not None:
        smp.steps_per_launch = spl
    return smp


def run_window(smp, x, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = smp.run(steps, BETA, x)["samples_out"]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, x


class GraphStep:
    """One captured l2hmc_gauge_mcmc_step (in place), replayed per step: the draw index is frozen by the capture, so
    this is a timing of the launch boundary, not a sampler."""

    def __init__(self, smp, x):
        dyn, L = smp.dynamics, _lib.lib()
        B = x.shape[0]
        plan = dyn._plan()
        nb = L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
        self.keep = (torch.empty(nb, dtype=torch.uint8, device="cuda"), [torch.empty(B, device="cuda") for _ in range(5)], x)
        ws, outs, _ = self.keep
        self.g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(self.g, stream=side):
                _lib.check(L.l2hmc_gauge_mcmc_step(C.byref(plan), BETA, x.data_ptr(), B, dyn._seed, 7,
                                                   *(o.data_ptr() for o in outs), ws.data_ptr(), nb, _lib.stream_ptr()))
        torch.cuda.current_stream().wait_stream(side)

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.g.replay()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


fmt = lambda v: f"{statistics.median(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; GaugeSampler.run, GaugeDynamics(hmc=True), eps 0.1, "
      f"beta 2; ms per MCMC step: median (min .. max) of {args.reps} alternating windows of about {args.window} s of the loop")
cols = ["(a) loop"] if args.loop_only else ["(a) loop", "(b) graph replay", "(c) run, 16 / launch", "(c) run, 256 / launch"]
print(f"# {'lattice':>7} {'chains':>6} {'LF':>3} {'mode':>9} {'steps':>6} | " + " | ".join(f"{c:>26}" for c in cols) + " | (a) / (c256)")
for T, X, B, N in SHAPES:
    for both in (True, False):
        x0 = torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)
        var = {"(a) loop": sampler(T, X, B, N, both, None if args.loop_only else 1)}
        if not args.loop_only:
            var["(c) run, 16 / launch"] = sampler(T, X, B, N, both, 16)
            var["(c) run, 256 / launch"] = sampler(T, X, B, N, both, 256)
        xs = {k: x0.clone() for k in var}
        graph = None if args.loop_only else GraphStep(var["(a) loop"], x0.clone())
        dt, xs[cols[0]] = run_window(var[cols[0]], xs[cols[0]], 256)              # first touch, and the step count
        dt, xs[cols[0]] = run_window(var[cols[0]], xs[cols[0]], 256)
        steps = max(2, round(args.window / (dt * 1e-3) / 256)) * 256
        for k in var:                                              # warm-up at the windows' own size
            _, xs[k] = run_window(var[k], xs[k], steps)
        if graph:
            graph.window(steps)
        times = {c: [] for c in cols}
        for _ in range(args.reps):
            for k in var:
                dt, xs[k] = run_window(var[k], xs[k], steps)
                times[k].append(dt)
            if graph:
                times["(b) graph replay"].append(graph.window(steps))
        ratio = "" if args.loop_only else f"{statistics.median(times[cols[0]]) / statistics.median(times[cols[3]]):6.2f}x"
        print(f"  {T:>3}x{X:<3} {B:6d} {N:3d} {'both' if both else 'selected':>9} {steps:6d} | "
              + " | ".join(f"{fmt(times[c]):>26}" for c in cols) + f" | {ratio}", flush=True)
        del var, xs, graph
