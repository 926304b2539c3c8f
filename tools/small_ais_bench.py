"""Annealed importance sampling on the toy targets (`DynamicsSampler.ais`, l2hmc_small_ais_run), ms per annealing step:
  (a) run_hmc : `DynamicsSampler.run_hmc` on the same dynamics, l2hmc_small_hmc_run at `steps_per_launch` = 256 -- one
                target evaluation per force where an annealing step has two;
  (b) ais     : `ais` from N(0, I) on the reference's schedule, fresh momenta, 256 steps per launch;
  (c) ais + v : (b) with `refresh = 0.1` (a persistent momentum);
  (d) layered : the same anneal the only way the library could run it before this kernel -- per annealing step a fresh
                layer-by-layer `Dynamics(x_dim, curr_energy, hmc=True)` on a torch callable (1 - b) E0 + b E1 whose
                force is torch.autograd's, its `forward`, fill_uniform and the accept in torch (utils/ais.py:46-65 as
                written); a few steps timed.
    python tools/small_ais_bench.py > profiles/small_ais.txt      (section 1 of that file)

Shapes: BASELINE config 1 (SCG, 128 chains, 5 LF) and config 2 (MoG, 4096 chains, 10 LF).

A window is one call of STEPS steps between two device synchronisations on the host clock, in one process for all
variants; STEPS is chosen so that a window of (a) lasts about `--window` seconds (a multiple of 256, the same for (a),
(b), (c)), after a warm-up window of the same length; the variants alternate, REPS windows each.  Reported: median
(min .. max).  A window includes what a caller pays for: the schedule's copy to the device, the accept probabilities'
and the weights' copies to the host and the float64 finishing."""
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
from l2hmc_amd import ops  # noqa: E402

SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
MOG = ([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
SHAPES = [("cfg 1", "scg", 128, 5), ("cfg 2", "mog", 4096, 10)]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of run_hmc per timed window (sets the step count)")
ap.add_argument("--layered-steps", type=int, default=8, help="annealing steps per window of (d)")
ap.add_argument("--label", default="this tree")
args = ap.parse_args()


def distribution(target):
    return la.Gaussian(np.zeros(2), SCG_SIGMA) if target == "scg" else la.GMM(*MOG)


def sampler(target, N):
    np.random.seed(0)
    dyn = la.Dynamics(2, distribution(target).get_energy_function(), trajectory_length=N, eps=0.1, hmc=True,
                      use_temperature=True)
    return la.DynamicsSampler(dyn)


def torch_energies(target, dev):
    """(E0, E1) as torch callables on device tensors: N(0, I) and the target, as distributions.py writes them."""
    def gauss(mu, sigma):
        m, P = (torch.tensor(np.asarray(a, dtype=np.float32), device=dev) for a in (mu, np.linalg.inv(sigma)))
        return lambda z: 0.5 * (((z - m) @ P) * (z - m)).sum(1)
    E0 = gauss(np.zeros(2), np.eye(2))
    if target == "scg":
        return E0, gauss(np.zeros(2), SCG_SIGMA)
    mus, sigmas, pis = MOG
    comps = [gauss(m, s) for m, s in zip(mus, sigmas)]
    logc = [float(np.log(p / np.sqrt((2 * np.pi) ** 2 * np.linalg.det(s)))) for p, s in zip(pis, sigmas)]
    return E0, lambda z: -torch.logsumexp(torch.stack([c - e(z) for c, e in zip(logc, comps)], dim=1), dim=1)


def layered_anneal(E0, E1, x, N, betas, seed=42):
    """utils/ais.py:46-65 on the layer-by-layer path, fresh momenta: -> (x, w)."""
    w = torch.zeros(x.shape[0], device=x.device)
    b_prev, draws = 0.0, 0
    for b in betas:
        b = float(b)
        curr = lambda z, b=b: (1 - b) * E0(z) + b * E1(z)
        dyn = la.Dynamics(2, curr, trajectory_length=N, eps=0.1, hmc=True, seed=seed)
        dyn._draws = draws
        w = w + (b - b_prev) * (E0(x) - E1(x))
        Lx, _, px = dyn.forward(x)
        u = ops.fill_uniform((x.shape[0],), seed, dyn._draws, x.device)
        draws = dyn._draws + 1
        x = torch.where(((px - u) >= 0)[:, None], Lx, x)
        b_prev = b
    return x, w


def window(call, x, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x = call(steps, x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, x


fmt = lambda v: f"{statistics.median(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
RUN, AIS, AISV, LAY = "(a) run_hmc, 256 / launch", "(b) ais, 256 / launch", "(c) ais, refresh = 0.1", "(d) layered, callable energy"
print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; plain HMC transitions, x_dim 2, eps 0.1, init N(0, I); "
      f"ms per (annealing) step: median (min .. max) of {args.reps} alternating windows")
for name, target, B, N in SHAPES:
    smp = {k: sampler(target, N) for k in (RUN, AIS, AISV)}
    assert all(s.steps_per_launch == 256 for s in smp.values())
    init = la.Gaussian(np.zeros(2), np.eye(2))
    calls = {RUN: lambda n, x: smp[RUN].run_hmc(n, x, keep_samples=False)["samples_out"],
             AIS: lambda n, x: smp[AIS].ais(n, init, x)["samples_out"],
             AISV: lambda n, x: smp[AISV].ais(n, init, x, refresh=0.1)["samples_out"]}
    x0 = la._lib.as_dev(np.random.default_rng(0).standard_normal((B, 2)))
    xs = {k: x0.clone() for k in calls}
    dt, xs[RUN] = window(calls[RUN], xs[RUN], 256)               # first touch, and the step count
    dt, xs[RUN] = window(calls[RUN], xs[RUN], 256)
    steps = max(2, round(args.window / (dt * 1e-3) / 256)) * 256
    for k in calls:                                              # warm-up at the windows' own size
        _, xs[k] = window(calls[k], x0.clone(), steps)
    times = {k: [] for k in calls}
    for _ in range(args.reps):
        for k in calls:
            dt, xs[k] = window(calls[k], x0.clone(), steps)      # every anneal starts from the init's samples
            times[k].append(dt)
    print(f"  {name}: {target}, {B} chains, {N} LF, {steps} steps per window")
    base = statistics.median(times[RUN])
    for k in calls:
        rel = "" if k == RUN else f"/ (a) = {statistics.median(times[k]) / base:5.3f}"
        print(f"    {k:>30} | {fmt(times[k]):>30} | {rel}", flush=True)
    # (d): a few steps of the reference's schedule for `steps` steps
    E0, E1 = torch_energies(target, x0.device)
    betas = np.linspace(0., 1., steps + 1)[1:args.layered_steps + 1]
    lay = lambda n, x: layered_anneal(E0, E1, x, N, betas)[0]
    window(lay, x0.clone(), args.layered_steps)                  # warm-up
    t_lay = [window(lay, x0.clone(), args.layered_steps)[0] for _ in range(args.reps)]
    print(f"    {LAY:>30} | {fmt(t_lay):>30} | / (b) = {statistics.median(t_lay) / statistics.median(times[AIS]):7.1f}"
          f"   ({args.layered_steps} steps per window)", flush=True)
    del smp, xs, calls
