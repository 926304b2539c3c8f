"""Plain-HMC MCMC step (`GaugeSampler.step` with `GaugeDynamics(hmc=True)`): the one-launch kernel of
l2hmc_amd/csrc/hmc_step.hip against the layer-by-layer path the same build keeps behind `fused=False`
(L2HMC_PLAN_LAYERED; leapfrog.hip's and mcmc_step.hip's general path, unchanged by the kernel's arrival).
    python tools/hmc_step_bench.py > profiles/hmc_step.txt

Per shape and mode the two paths are timed in the same process, alternating, REPS times each: a window of STEPS
steps between two device synchronisations on the host clock, after a warm-up of the same shape.  Reported is the
median window and the spread (min .. max) in ms per MCMC step.

Floors printed beside the times (per step, nothing of them is measured):
  * hbm: the state the step has to move, read x once and write x_next once, 8 B D bytes, at 6.3 TB/s (what a copy
    reaches on this part; 8 TB/s is the specification);
  * sincos: the kernel evaluates sin P / cos P once per plaquette for every force (num_steps + 1 per row) and for the
    step's observables (2 per chain), each a Cody-Waite reduction and two degree-7 / 8 polynomials, about 25 VALU
    instructions (common.h: fast_sincos), plus about 25 for the plaquette, the half-kicks and the two masked position
    sub-updates of the site: 50 lane-instructions per site and force.  256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz issue
    39.3 T lane-instructions per second.  A latency floor is not modelled: two barriers and two LDS round trips per
    leapfrog step are what the kernel waits on where a row has one site per thread.
"""
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
HBM, LANE_RATE, SITE_INSTR = 6.3e12, 256 * 4 * 16 * 2.4e9, 50.0

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window (sets the step count)")
args = ap.parse_args()


def build(T, X, B, N, both, fused):
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=0.1, hmc=True, num_steps=N, both_directions=both)
    dyn.fused = fused
    return GaugeSampler(dyn)


def window(smp, x, beta, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        x = smp.step(x, beta)[0]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, x


def launches(cls, smp, x, beta):
    L = _lib.lib()
    _lib.check(L.l2hmc_profile_begin(cls))
    smp.step(x, beta)
    ms, n = C.c_double(), C.c_int64()
    _lib.check(L.l2hmc_profile_end(C.byref(ms), C.byref(n)))
    return int(n.value)


print(f"# device {torch.cuda.get_device_name(0)}; library {os.path.relpath(_lib.LIB_PATH, ROOT)}")
print("# GaugeSampler.step, GaugeDynamics(hmc=True), eps 0.1, beta 2; old = fused=False (the layer-by-layer path,")
print("# unchanged in this build), new = the one-launch kernel; ms per MCMC step: median (min .. max) of "
      f"{args.reps} alternating windows")
print("# launches: new = class-5 launches counted by l2hmc_profile_begin/_end over one step; old = kernels the general")
print("#   path's dispatch issues (15 + 6 N in either mode, plus 4 device copies with both directions, 1 selected-only, and a")
print("#   memset), of which class 4 (u1_action_force) counted over one step is shown in brackets")
print("# floors per step (see the docstring): hbm = 8 B D bytes at 6.3 TB/s; sincos = 50 lane-instructions per site and")
print("#   force at 39.3 T/s; share = the larger floor over the new path's time")
print(f"# {'lattice':>7} {'chains':>6} {'LF':>3} {'mode':>9} | {'old ms':>24} | {'new ms':>24} | {'speed-up':>8} | "
      f"{'M chain-LF/s new':>16} | {'launches old / new':>18} | {'hbm us':>7} {'sincos us':>9} {'share':>6}")
for T, X, B, N in SHAPES:
    for both in (True, False):
        D = 2 * T * X
        beta = 2.0
        smp = {f: build(T, X, B, N, both, f) for f in (False, True)}
        x = {f: torch.rand(B, D, device="cuda") * (2 * np.pi) for f in (False, True)}
        steps = {}
        for f in (False, True):                                  # warm-up, and the step count of a window
            dt, x[f] = window(smp[f], x[f], beta, 20)
            dt, x[f] = window(smp[f], x[f], beta, 20)
            steps[f] = max(20, int(args.window / dt))
        times = {False: [], True: []}
        for _ in range(args.reps):
            for f in (False, True):
                dt, x[f] = window(smp[f], x[f], beta, steps[f])
                times[f].append(dt * 1e3)
        med = {f: statistics.median(times[f]) for f in times}
        n_new = launches(5, smp[True], x[True], beta)
        u1_old = launches(4, smp[False], x[False], beta)
        old_kernels = 15 + 6 * N
        rows = B * (2 if both else 1)
        hbm = 8.0 * B * D / HBM
        sincos = (rows * (N + 1) + 2 * B) * (T * X) * SITE_INSTR / LANE_RATE
        share = max(hbm, sincos) / (med[True] * 1e-3)
        fmt = lambda f: f"{med[f]:8.4f} ({min(times[f]):.4f} .. {max(times[f]):.4f})"
        print(f"  {T:>3}x{X:<3} {B:6d} {N:3d} {'both' if both else 'selected':>9} | {fmt(False):>24} | {fmt(True):>24} | "
              f"{med[False] / med[True]:7.1f}x | {B * N / (med[True] * 1e-3) / 1e6:16.1f} | "
              f"{old_kernels:5d} [{u1_old:3d}] / {n_new:<4d} | {hbm * 1e6:7.2f} {sincos * 1e6:9.2f} {share:6.2f}",
              flush=True)
        del smp, x
