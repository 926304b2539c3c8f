"""A ladder of beta or of step sizes in one plain-HMC lattice launch (`GaugeSampler.run_hmc`,
l2hmc_gauge_hmc_run_ladder) against the uniform run it is built from (`GaugeSampler.run`, l2hmc_gauge_hmc_run) and
against what it replaces, ms per MCMC step at `steps_per_launch` = 256:
  (a) uniform  : `run` of all the chains at one beta (`--uniform-only` times just this, and also works on a tree
                 that has no `run_hmc`: `--tree PATH` imports the package of another, built, tree -- the parent commit);
  (b) ladder   : `run_hmc` of all the chains with an 8-rung beta ladder (chain c at betas[c % 8]), with an 8-rung eps
                 ladder, and with all entries equal (beta [1, B] and eps [B] of one value each);
  (c) 8 runs   : what the ladder replaces -- 8 samplers of chains / 8 chains each, one `run` after the other.
    python tools/hmc_run_ladder_bench.py > table.txt
    python tools/hmc_run_ladder_bench.py --resources     (no GPU: the register table of hmc_step.hip's kernels)
profiles/hmc_run_ladder.txt is made of both, and of both again on the parent commit.

A window is `steps` MCMC steps between two device synchronisations on the host clock, `steps` a multiple of 256 chosen
per row so that a window of (a) lasts about `--window` seconds, after a warm-up window of the same length; the variants
of a row alternate, REPS windows each.  Reported: median (min .. max).  Every variant includes what its caller pays for:
the histories' copy to the host and the mean accept probability."""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of (a) per timed window (sets the step count)")
ap.add_argument("--label", default="this tree")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="root of the (built) tree whose l2hmc_amd is measured")
ap.add_argument("--uniform-only", action="store_true")
ap.add_argument("--shape", action="append", metavar="T,X,CHAINS,LF",
                help="time this row instead of the two of profiles/hmc_run.txt (may be given more than once)")
ap.add_argument("--resources", action="store_true",
                help="compile csrc/hmc_step.hip of --tree for gfx950 and print every kernel's registers, scratch, LDS "
                     "and occupancy as the compiler reports them")
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)


def resources():
    sys.path.insert(0, ROOT)
    from l2hmc_amd import build as B
    hipcc = B._hipcc()
    ver = subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, *B.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "hmc_step.hip"),
               "-o", os.path.join(tmp, "hmc_step.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: \s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = subprocess.run([filt, val], capture_output=True, text=True).stdout.strip() or val
            name = re.sub(r"^void l2hmc::|\(.*$", "", name)
            cur = {"name": name}
            rows.append(cur)
        elif cur is not None:
            cur[key] = val
    print(f"# {args.label}: {' '.join(B.FLAGS)}; {ver[0] if ver else hipcc}" + (f"; {ver[1]}" if len(ver) > 1 else ""))
    print(f"# {'kernel':<32} {'VGPRs':>5} {'AGPRs':>5} {'SGPRs':>5} {'scratch B/lane':>14} {'waves/SIMD':>10} "
          f"{'static LDS':>10}")
    for r in sorted(rows, key=lambda r: r["name"]):
        print(f"  {r['name']:<32} {r.get('VGPRs', '?'):>5} {r.get('AGPRs', '?'):>5} {r.get('TotalSGPRs', '?'):>5} "
              f"{r.get('ScratchSize', '?'):>14} {r.get('Occupancy', '?'):>10} {r.get('LDS Size', '?'):>10}")


if args.resources:
    resources()
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
from l2hmc_amd import GaugeDynamics, GaugeLattice, GaugeSampler  # noqa: E402

SHAPES = [(8, 8, 2048, 10), (32, 32, 2048, 25)]          # T, X, chains, LF steps: rows of profiles/hmc_run.txt
if args.shape:
    SHAPES = [tuple(int(v) for v in s.split(",")) for s in args.shape]
RUNGS, BETA, EPS = 8, 2.0, 0.1
BETAS = np.linspace(1.0, 4.5, RUNGS)
EPSS = np.linspace(0.05, 0.19, RUNGS)


def sampler(T, X, B, N, both):
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=EPS, hmc=True, num_steps=N, both_directions=both)
    return GaugeSampler(dyn)


class Uniform:
    def __init__(self, T, X, B, N, both, parts=1, **_):
        self.smp = [sampler(T, X, B // parts, N, both) for _ in range(parts)]
        self.x = [torch.rand(B // parts, 2 * T * X, device="cuda") * (2 * np.pi) for _ in range(parts)]
        self.beta = [BETA] if parts == 1 else [float(b) for b in BETAS]

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, smp in enumerate(self.smp):
            self.x[i] = smp.run(steps, self.beta[i], self.x[i])["samples_out"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


class Ladder:
    def __init__(self, T, X, B, N, both, beta, eps):
        self.smp = sampler(T, X, B, N, both)
        self.x = torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)
        self.beta, self.eps = beta, eps

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.x = self.smp.run_hmc(steps, self.beta, self.x, eps=self.eps)["samples_out"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


med = statistics.median
fmt = lambda v: f"{med(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; GaugeDynamics(hmc=True), eps {EPS}, beta {BETA}, "
      f"256 steps per launch; ms per MCMC step: median (min .. max) of {args.reps} alternating windows of about "
      f"{args.window} s of (a)")
cols = ["(a) uniform"]
if not args.uniform_only:
    cols += ["(b) beta ladder", "(b) eps ladder", "(b) all equal", "(c) 8 runs of chains / 8"]
print(f"# {'lattice':>7} {'chains':>6} {'LF':>3} {'mode':>9} {'steps':>6} | " + " | ".join(f"{c:>26}" for c in cols)
      + ("" if args.uniform_only else " | (b beta)/(a) (b eps)/(a) (b equal)/(a) (c)/(b beta)"))
for T, X, B, N in SHAPES:
    for both in (True, False):
        c = np.arange(B)
        var = {"(a) uniform": Uniform(T, X, B, N, both)}
        if not args.uniform_only:
            var["(b) beta ladder"] = Ladder(T, X, B, N, both, BETAS[c % RUNGS][None, :], None)
            var["(b) eps ladder"] = Ladder(T, X, B, N, both, BETA, EPSS[c % RUNGS])
            var["(b) all equal"] = Ladder(T, X, B, N, both, np.full((1, B), BETA), np.full(B, EPS))
            var["(c) 8 runs of chains / 8"] = Uniform(T, X, B, N, both, parts=RUNGS)
        var[cols[0]].window(256)                                   # first touch, and the step count
        dt = var[cols[0]].window(256)
        steps = max(2, round(args.window / (dt * 1e-3) / 256)) * 256
        for k in cols:                                             # warm-up at the windows' own size
            var[k].window(steps)
        times = {k: [] for k in cols}
        for _ in range(args.reps):
            for k in cols:
                times[k].append(var[k].window(steps))
        a = med(times[cols[0]])
        ratios = "" if args.uniform_only else (
            f" | {med(times[cols[1]]) / a:12.3f} {med(times[cols[2]]) / a:11.3f} {med(times[cols[3]]) / a:13.3f} "
            f"{med(times[cols[4]]) / med(times[cols[1]]):13.2f}")
        print(f"  {T:>3}x{X:<3} {B:6d} {N:3d} {'both' if both else 'selected':>9} {steps:6d} | "
              + " | ".join(f"{fmt(times[k]):>26}" for k in cols) + ratios, flush=True)
        del var
