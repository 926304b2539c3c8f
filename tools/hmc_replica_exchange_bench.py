"""Replica exchange between the rungs of a plain-HMC lattice ladder (`GaugeSampler.run_hmc_exchange`,
`swap_replicas`, l2hmc_gauge_replica_swap) against the ladder run it is built on (`GaugeSampler.run_hmc`), with the
method of tools/hmc_run_ladder_bench.py, 8 rungs (chain c at betas[c % 8], beta 1.0 .. 4.5), `steps_per_launch` = 256:
  (a) no exchange : `run_hmc` of the ladder (`--plain-only` times just this, and also works on a tree that has no
                    exchange: `--tree PATH` imports the package of another, built, tree -- the parent commit);
  (b) exchange    : `run_hmc_exchange(..., replicas=8, swap_every=k)` for k = 1, 4, 16, ms per MCMC step;
  (c) the round   : `swap_replicas` alone, us per round: the call on the host clock (`--rounds` calls of alternating
                    parity between two synchronisations) and the kernel alone (l2hmc_profile class 8).
    python tools/hmc_replica_exchange_bench.py > table.txt
    python tools/hmc_replica_exchange_bench.py --stats      (the sampling figures below instead of the timings)
    python tools/hmc_replica_exchange_bench.py --in-launch      (the rounds inside the run's launches)
profiles/hmc_replica_exchange.txt is made of all three, and of (a) on the parent commit.

--in-launch times, per row and swap_every, the round between launches (b) next to the round inside the launch
(`run_hmc_exchange` on a sampler with `in_launch = True`, l2hmc_gauge_hmc_run_exchange), alternating with (a), at 8x8 with 8 rungs and
at 16x16 with 2 (the most that shape is served with); a fifth field of --shape is the row's number of rungs.

A window is `steps` MCMC steps between two device synchronisations on the host clock, `steps` a multiple of 256 chosen
per row so that a window of (a) lasts about `--window` seconds, after a warm-up window of the same length; the variants
of a row alternate, REPS windows each.  Reported: median (min .. max).  Every variant includes what its caller pays for:
the histories' copy to the host and the mean accept probability.

--stats: ONE seeded run at 8x8 (2048 chains = 256 groups of the 8 rungs, eps 0.1, 10 leapfrog steps, from the ordered
start, `--stats-steps` steps after `--therm` steps of thermalisation), without exchange and with swap_every = 1 and 4:
the swap rate per neighbouring pair of rungs, the top rung's mean |dQ| per step (`charge_diff`), the top rung's
integrated autocorrelation time of the plaquette (`stats.integrated_time`), and the completed round trips (lowest rung
-> highest -> lowest, `stats.replica_round_trips`) per group and 1000 steps."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of (a) per timed window (sets the step count)")
ap.add_argument("--label", default="this tree")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="root of the (built) tree whose l2hmc_amd is measured")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--in-launch", action="store_true", help="(b) between launches against the rounds in the launch")
ap.add_argument("--shape", action="append", metavar="T,X,CHAINS,LF[,RUNGS]",
                help="time this row instead of the two of profiles/hmc_run.txt (may be given more than once)")
ap.add_argument("--rounds", type=int, default=2000, help="calls of swap_replicas per window of (c)")
ap.add_argument("--stats", action="store_true")
ap.add_argument("--stats-steps", type=int, default=4096)
ap.add_argument("--therm", type=int, default=512)
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from l2hmc_amd import GaugeDynamics, GaugeLattice, GaugeSampler, _lib, stats  # noqa: E402

RUNGS, EPS = 8, 0.1
SHAPES = [(8, 8, 2048, 10), (32, 32, 2048, 25)]          # T, X, chains, LF steps: rows of profiles/hmc_run.txt
if args.in_launch:
    SHAPES = [(8, 8, 2048, 10, 8), (16, 16, 2048, 15, 2)]
if args.shape:
    SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.shape]
SHAPES = [(s + (RUNGS,))[:5] for s in SHAPES]            # the rungs of a row: 8 unless it says otherwise
BETAS = np.linspace(1.0, 4.5, RUNGS)
SWAP_EVERY = (1, 4, 16)


def sampler(T, X, B, N, both, seed=None):
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    kw = {} if seed is None else {"seed": seed}
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=EPS, hmc=True, num_steps=N, both_directions=both, **kw)
    return GaugeSampler(dyn), lat


class Run:
    """`run_hmc` of the ladder (swap_every None) or `run_hmc_exchange` with a round every `swap_every` steps"""

    def __init__(self, T, X, B, N, both, swap_every=None, rungs=RUNGS, in_launch=False):
        self.smp, _ = sampler(T, X, B, N, both)
        self.x = torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)
        self.beta = np.linspace(BETAS[0], BETAS[-1], rungs)[np.arange(B) % rungs][None, :]
        self.k, self.done, self.rungs = swap_every, 0, rungs
        if in_launch:                                                # (set only where asked for: other trees have none)
            self.smp.in_launch = True

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.k is None:
            self.x = self.smp.run_hmc(steps, self.beta, self.x)["samples_out"]
        else:
            out = self.smp.run_hmc_exchange(steps, self.beta, self.x, replicas=self.rungs, swap_every=self.k,
                                            first_parity=self.done % 2)
            self.x, self.done = out["samples_out"], self.done + steps // self.k
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


def round_alone(T, X, B, N, reps, rounds):
    """us per round: (host clock between two synchronisations, kernel time of l2hmc_profile class 8), `reps` windows"""
    smp, _ = sampler(T, X, B, N, True)
    x = torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)
    beta = torch.as_tensor(BETAS[np.arange(B) % RUNGS], dtype=torch.float32, device="cuda")
    L = _lib.lib()
    host, dev = [], []
    for rep in range(reps + 1):                                    # the first window warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for r in range(rounds):
            smp.swap_replicas(x, beta, RUNGS, r % 2)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) / rounds * 1e6)
        n_prof = min(rounds, 200)                                  # (200 launches are enough for the kernel's own time)
        _lib.check(L.l2hmc_profile_begin(8))
        for r in range(n_prof):
            smp.swap_replicas(x, beta, RUNGS, r % 2)
        ms, n = C.c_double(), C.c_int64()
        _lib.check(L.l2hmc_profile_end(C.byref(ms), C.byref(n)))
        dev.append(ms.value / max(1, n.value) * 1e3)
    return host[1:], dev[1:]


med = statistics.median


def timings():
    fmt = lambda v: f"{med(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
    fmu = lambda v: f"{med(v):6.2f} ({min(v):.2f} .. {max(v):.2f})"
    print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; GaugeDynamics(hmc=True), eps {EPS}, rungs of "
          f"beta {BETAS[0]} .. {BETAS[-1]}, 256 steps per launch; ms per MCMC step: median (min .. max) of {args.reps} "
          f"alternating windows of about {args.window} s of (a)")
    # (b): the round between launches; (c), with --in-launch: the rounds inside the run's launches
    kinds = [("b", False), ("c", True)] if args.in_launch else [("b", False)]
    variants = [] if args.plain_only else [(f"({n}) swap_every = {k}", k, inl) for k in SWAP_EVERY for n, inl in kinds]
    cols = ["(a) no exchange"] + [v[0] for v in variants]
    print(f"# {'lattice':>7} {'chains':>6} {'LF':>3} {'rungs':>5} {'mode':>9} {'steps':>6} | "
          + " | ".join(f"{c:>26}" for c in cols)
          + ("" if args.plain_only else " | " + " ".join(f"({n} {k})/(a)" for k in SWAP_EVERY for n, _ in kinds)))
    for T, X, B, N, G in SHAPES:
        for both in (True, False):
            var = {cols[0]: Run(T, X, B, N, both, rungs=G)}
            for c, k, inl in variants:
                var[c] = Run(T, X, B, N, both, k, G, inl)
            var[cols[0]].window(256)                                   # first touch, and the step count
            dt = var[cols[0]].window(256)
            steps = max(2, round(args.window / (dt * 1e-3) / 256)) * 256
            for c in cols:                                             # warm-up at the windows' own size
                var[c].window(steps)
            times = {c: [] for c in cols}
            for _ in range(args.reps):
                for c in cols:
                    times[c].append(var[c].window(steps))
            a = med(times[cols[0]])
            ratios = "" if args.plain_only else " | " + " ".join(f"{med(times[c]) / a:9.3f}" for c in cols[1:])
            print(f"  {T:>3}x{X:<3} {B:6d} {N:3d} {G:5d} {'both' if both else 'selected':>9} {steps:6d} | "
                  + " | ".join(f"{fmt(times[c]):>26}" for c in cols) + ratios, flush=True)
            del var
    if args.plain_only or args.in_launch:
        return
    print(f"# (c) one round alone (swap_replicas, {RUNGS} rungs): us per round, median (min .. max) of {args.reps} windows "
          f"of {args.rounds} calls of alternating parity; the kernel alone over 200 calls (l2hmc_profile class 8)")
    print(f"# {'lattice':>7} {'chains':>6} | {'the call, host clock':>26} | {'the kernel':>26}")
    for T, X, B, N, _ in SHAPES:
        host, dev = round_alone(T, X, B, N, args.reps, args.rounds)
        print(f"  {T:>3}x{X:<3} {B:6d} | {fmu(host):>26} | {fmu(dev):>26}", flush=True)


def sampling_figures():
    T, X, B, N = 8, 8, 2048, 10
    n, therm = args.stats_steps, args.therm
    beta = BETAS[np.arange(B) % RUNGS][None, :]
    top = np.arange(B) % RUNGS == RUNGS - 1
    print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; one seeded run (seed 11) at {T}x{X}, {B} chains = "
          f"{B // RUNGS} groups of {RUNGS} rungs of beta {BETAS[0]} .. {BETAS[-1]}, eps {EPS}, {N} leapfrog steps, ordered "
          f"start, {therm} steps of thermalisation (with the same exchange), then {n} steps")
    print("# top rung (beta 4.5): mean |dQ| per step and chain; tau_int of the plaquette in steps (stats.integrated_time "
          "over the rung's chains); round trips: completed lowest -> highest -> lowest per group and 1000 steps")
    for k in (None,) + SWAP_EVERY[:2]:
        smp, lat = sampler(T, X, B, N, True, seed=11)
        x = lat.samples.reshape(B, -1)
        kw = {} if k is None else dict(replicas=RUNGS, swap_every=k)
        run = smp.run_hmc if k is None else smp.run_hmc_exchange
        out = run(therm, beta, x, **kw)
        if k is not None:
            kw.update(first_parity=(therm // k) % 2, replica0=out["replica"][-1])
        t0 = time.perf_counter()
        out = run(n, beta, out["samples_out"], **kw)
        dt = time.perf_counter() - t0
        try:
            tau = float(stats.integrated_time(out["plaqs"][:, top, None], quiet=True)[0][0])
        except Exception:      # noqa: BLE001 -- too short a run for the estimator
            tau = float("nan")
        line = (f"  {'no exchange' if k is None else f'swap_every = {k:<2}':<16} top rung <|dQ|> "
                f"{out['charge_diff'][:, top].mean():.5f}  tau_int(plaq) {tau:7.2f}  accept(top) {out['px'][:, top].mean():.3f}")
        if k is not None:
            trips, groups = stats.replica_round_trips(out["replica"], RUNGS)
            line += (f"  round trips {groups.mean() / n * 1000:.3f}  swap_rate per pair "
                     + " ".join(f"{r:.3f}" for r in out["swap_rate"]))
        print(line + f"   ({dt:.1f} s)", flush=True)


if args.stats:
    sampling_figures()
else:
    timings()
