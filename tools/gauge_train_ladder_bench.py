"""Training GaugeDynamics on a ladder of beta in one step (`GaugeTrainer.train_step` with beta [B]; the `_ladder`
training entries) against the uniform training step it is built from and against what it replaces; ms per training step
at the cfg 3 shape (8x8, GenericNet H = 512, 10 leapfrog steps, 2048 + 2048 chains):
  (a) uniform  : `train_step` of all the chains at one beta;
  (b) ladder   : `train_step` of all the chains on 8 rungs (chain c at betas[c % 8], 1.0 .. 4.5);
  (c) 8 steps  : what the ladder replaces -- 8 trainers of chains / 8 chains each, one `train_step` after the other;
  (x) train    : `train(..., replicas=8, swap_every=1)` on the 8 rungs: (b) + wrap, observables and a round per step.
    python tools/gauge_train_ladder_bench.py > table.txt
A window is `steps` training steps between two device synchronisations on the host clock, after a warm-up window of the
same length; the variants alternate, REPS windows each.  Reported: median (min .. max).
Behind the table, a short seeded demonstration (--demo-steps, 0 to skip): 300 training steps on the ladder against 300
annealed at a single beta, then `GaugeSampler.run_exchange` on the ladder with each set of weights: mean accept
probability per rung and swap_rate per pair, reported as found."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--steps", type=int, default=8, help="training steps per timed window")
ap.add_argument("--chains", type=int, default=2048)
ap.add_argument("--lf", type=int, default=10)
ap.add_argument("--demo-steps", type=int, default=300, help="training steps of the demonstration (0: timings only)")
ap.add_argument("--demo-run", type=int, default=400, help="run_exchange steps after each training")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from l2hmc_amd import GaugeDynamics, GaugeLattice  # noqa: E402
from l2hmc_amd.gauge_trainer import GaugeTrainer  # noqa: E402

T = X = 8
RUNGS, BETA, EPS = 8, 2.0, 0.1
BETAS = np.linspace(1.0, 4.5, RUNGS)
B = args.chains


def trainer(chains):
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=chains, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=EPS, hmc=False, num_steps=args.lf, eps_trainable=True,
                        network_arch='generic', seed=5)
    return GaugeTrainer(dyn, lr_init=1e-4)


class Steps:
    """`parts` trainers of B / parts chains, trainer i at beta[i] (a float, or a device tensor [chains])."""

    def __init__(self, parts, beta, train=False):
        self.tr = [trainer(B // parts) for _ in range(parts)]
        self.x = [torch.rand(B // parts, 2 * T * X, device="cuda") * (2 * np.pi) for _ in range(parts)]
        self.beta, self.train, self.rates = beta, train, []

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, tr in enumerate(self.tr):
            if self.train:
                out = tr.train(steps, samples_init=self.x[i], beta_init=self.beta[i], beta_final=self.beta[i],
                               replicas=RUNGS, swap_every=1)
                self.x[i] = out["samples"]
                self.rates.append(out["swap_rate"])
            else:
                for _ in range(steps):
                    tr.train_step(self.x[i], self.beta[i])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


ladder = BETAS[np.arange(B) % RUNGS]
ladder_dev = torch.as_tensor(ladder, dtype=torch.float32, device="cuda")
var = {"(a) uniform": Steps(1, [BETA]), "(b) 8-rung ladder": Steps(1, [ladder_dev]),
       "(c) 8 steps of chains / 8": Steps(RUNGS, [float(b) for b in BETAS]),
       "(x) train, a round per step": Steps(1, [ladder], train=True)}
cols = list(var)
med = statistics.median
fmt = lambda v: f"{med(v):8.3f} ({min(v):.3f} .. {max(v):.3f})"      # noqa: E731
for k in cols:                                                     # first touch and warm-up at the windows' own size
    var[k].window(args.steps)
    var[k].rates = []
times = {k: [] for k in cols}
for _ in range(args.reps):
    for k in cols:
        times[k].append(var[k].window(args.steps))
print(f"# device {torch.cuda.get_device_name(0)}; GaugeTrainer on GaugeDynamics(GenericNet), {T}x{X}, {B} + {B} chains, "
      f"{args.lf} LF, eps {EPS}; ms per training step: median (min .. max) of {args.reps} alternating windows of "
      f"{args.steps} steps")
for k in cols:
    print(f"  {k:<28} {fmt(times[k])}")
a, b, c, x = (med(times[k]) for k in cols)
print(f"  (b)/(a) = {b / a:.3f}   (a)'s own spread: {min(times[cols[0]]) / a:.3f} .. {max(times[cols[0]]) / a:.3f}")
print(f"  (c)/(b) = {c / b:.2f}")
print(f"  (x)/(b) = {x / b:.3f}   swap_rate per pair of rungs (betas {BETAS.tolist()}): "
      + " ".join(f"{v:.3f}" for v in np.mean(var[cols[3]].rates, axis=0)))

# ---- a short seeded demonstration (not a test, reported as found): networks trained ON the ladder against networks
# annealed at one beta, both then sampling the ladder with `GaugeSampler.run_exchange`
if args.demo_steps:
    del var
    from l2hmc_amd import GaugeSampler  # noqa: E402
    n, run = args.demo_steps, args.demo_run
    print(f"# demonstration: {n} training steps (seed 5, lr 1e-4, {B} + {B} chains), then run_exchange of {run} steps on "
          f"the 8 rungs (replicas 8, a round every 4th step); per rung: mean accept probability of the last "
          f"{run // 2} steps; swap_rate per pair of rungs")
    for name, kw in (("trained on the ladder (a round every 4th step)",
                      dict(beta_init=ladder, beta_final=ladder, replicas=RUNGS, swap_every=4)),
                     ("annealed at one beta, 2.0 -> 4.5", dict(beta_init=float(BETA), beta_final=float(BETAS[-1])))):
        tr = trainer(B)
        torch.manual_seed(5)
        x0 = torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)
        out = tr.train(n, samples_init=x0, **kw)
        smp = GaugeSampler(tr.dynamics)
        res = smp.run_exchange(run, ladder[None, :], out["samples"], replicas=RUNGS, swap_every=4)
        px = res["px"][run // 2:].reshape(-1, B // RUNGS, RUNGS).mean(axis=(0, 1))
        print(f"  {name}: final training loss {float(out['loss'][-1]):.2f}, eps {float(tr.dynamics.eps):.4f}")
        print("    mean accept prob per rung: " + " ".join(f"{v:.3f}" for v in px))
        print("    swap_rate per pair:        " + " ".join(f"{v:.3f}" for v in res["swap_rate"]))
