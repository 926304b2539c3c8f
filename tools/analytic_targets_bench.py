"""The rough-well and funnel targets on the one-launch path against the layered path, and the mixture / Gaussian
shapes of BASELINE configs 1 and 2 for a build-against-build comparison.
    python tools/analytic_targets_bench.py --part targets >> profiles/analytic_targets.txt
    L2HMC_LIB_PATH=<a build of the parent commit> python tools/analytic_targets_bench.py --part old --label parent
    python tools/analytic_targets_bench.py --part old --label "this tree"        (alternate the two, three times each)

--part targets: 2-D rough well (eps 0.5, easy) and 2-D funnel, 4096 chains, 10 leapfrog steps, 10 and 50 hidden units;
`propose` (one call), `DynamicsSampler.run` per step and `DynamicsTrainer.train_step`, once with the packed target
(one launch) and once with the same energy as a torch callable (layer by layer).
--part old: cfg 1 (SCG, 128 chains, 5 LF, 10 nodes) and cfg 2 (MoG, 4096 chains, 10 LF, 50 nodes), `propose` and `run`
per step, plus a digest of their outputs (propose, run, train_step) for a bit-for-bit comparison of two builds.

A window is a fixed number of calls between two device synchronisations on the host clock, after a warm-up window;
reported: median (min .. max) of --reps windows, ms per call (per MCMC step for `run`)."""
import argparse
import hashlib
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import l2hmc_amd as la  # noqa: E402
from l2hmc_amd.dynamics_trainer import DynamicsTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["targets", "old"], required=True)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="this tree")
args = ap.parse_args()
SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
CLIP = 8.0


def rough_well_fn(x, eps=0.5):
    return 0.5 * (x * x).sum(1) + eps * torch.cos(x / eps).sum(1)


def funnel_fn(x):
    v, n = x[:, 0], x.shape[1] - 1
    hi, lo = v > CLIP, -CLIP > v
    s = torch.where(hi, torch.full_like(v, math.exp(CLIP)),
                    torch.where(lo, torch.full_like(v, math.exp(-CLIP)), torch.exp(torch.where(hi | lo, 0 * v, v))))
    return 0.5 * ((v / 2.0) ** 2 + (x[:, 1:] ** 2).sum(1) / s + n * torch.log(2 * math.pi * s))


def dynamics(fn, N, nodes):
    np.random.seed(0)
    torch.manual_seed(0)
    return la.Dynamics(2, fn, trajectory_length=N, eps=0.1,
                       net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))


def window(call, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def timed(call, n):
    window(call, max(2, n // 4))
    window(call, n)
    return [window(call, n) for _ in range(args.reps)]


fmt = lambda v: f"{statistics.median(v):8.4f} ({min(v):.4f} .. {max(v):.4f})"  # noqa: E731
dev = torch.cuda.get_device_name(0)

if args.part == "targets":
    print(f"# device {dev}; {args.label}; 2-D targets, 4096 chains, 10 LF, eps 0.1; ms per call (run: per MCMC step), "
          f"median (min .. max) of {args.reps} windows")
    print(f"# {'target':>10} {'nodes':>5} {'path':>10} | {'propose':>28} | {'run, per step':>28} | {'train_step':>28}")
    for tname, dist, torch_fn in (("rough well", la.RoughWell(2, 0.5, easy=True), rough_well_fn),
                                  ("funnel", la.GaussianFunnel(2), funnel_fn)):
        for nodes in (10, 50):
            np.random.seed(1)
            x0 = la._lib.as_dev(dist.get_samples(4096))
            for path, fn in (("one launch", dist.get_energy_function()), ("layered", torch_fn)):
                dyn = dynamics(fn, 10, nodes)
                assert dyn.layered == (path == "layered")
                n = 200 if path == "one launch" else 5
                t_prop = timed(lambda: la.propose(x0, dyn, do_mh_step=True), n)
                smp = la.DynamicsSampler(dyn)
                steps = 256 if path == "one launch" else 4
                t_run = timed(lambda: smp.run(steps, x0), 4 if path == "one launch" else 1)
                t_run = [t / steps for t in t_run]
                tr = DynamicsTrainer(dynamics(fn, 10, nodes))
                t_train = timed(lambda: tr.train_step(x0), 50 if path == "one launch" else 3)
                print(f"  {tname:>10} {nodes:5d} {path:>10} | {fmt(t_prop):>28} | {fmt(t_run):>28} | {fmt(t_train):>28}", flush=True)
else:
    print(f"# device {dev}; {args.label}; ms per call (run: per MCMC step), median (min .. max) of {args.reps} windows")
    for name, B, N, nodes in (("cfg 1", 128, 5, 10), ("cfg 2", 4096, 10, 50)):
        if name == "cfg 1":
            dist = la.Gaussian(np.zeros(2), SCG_SIGMA)
        else:
            dist = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
        np.random.seed(1)
        x0 = la._lib.as_dev(dist.get_samples(B))
        dyn = dynamics(dist.get_energy_function(), N, nodes)
        h = hashlib.sha256()
        dyn._draws = 0
        Lx, _, px, (out,) = la.propose(x0, dyn, do_mh_step=True)
        r = la.DynamicsSampler(dyn).run(16, x0, keep_samples=True)
        trd = dynamics(dist.get_energy_function(), N, nodes)
        tr = DynamicsTrainer(trd)
        loss, xo, pxt = tr.calc_loss_and_grads(x0)[:3]
        for a in (Lx, px, out, r["px"], r["samples"], loss, xo, pxt, tr.grads):
            h.update(np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
        t_prop = timed(lambda: la.propose(x0, dyn, do_mh_step=True), 300)
        smp = la.DynamicsSampler(dyn)
        t_run = [t / 256 for t in timed(lambda: smp.run(256, x0), 4)]
        print(f"  {name} {args.label:>10} | propose {fmt(t_prop)} | run per step {fmt(t_run)} | "
              f"outputs sha256 {h.hexdigest()[:16]}", flush=True)
