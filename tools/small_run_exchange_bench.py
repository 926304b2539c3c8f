"""Replica exchange between the rungs of an L2HMC toy-target temperature ladder, the rounds INSIDE the launch
(`DynamicsSampler.run_exchange` with `in_launch = True`, l2hmc_small_run_exchange), against the ladder run it is built
on (`run(temperature=)`) and against the same call with the rounds between launches (`in_launch = False`:
l2hmc_small_run_tempered cut at the rounds, l2hmc_small_replica_swap after each), in the manner of
tools/small_hmc_exchange_bench.py.  8 rungs (chain c at TEMPS[c % 8], temperature 1.0 .. 4.5), `steps_per_launch` = 256,
keep_samples=False, ms per MCMC step:
  (a) no exchange : `run(temperature=ladder)` (`--plain-only` times just this, and also works on a tree that has no
                    in-launch exchange: `--tree PATH` imports the package of another, built, tree -- the parent commit);
  (b) in launch   : `run_exchange(..., replicas=8, swap_every=k)` with `in_launch = True` for k = 1, 4, 16;
  (c) between     : the same call with `in_launch = False`: 1 + 1 launches per k steps;
  and per row the launches of (a) and (b) alone (l2hmc_profile class 7), from which a round's cost inside the launch.
`--packed`: groups of 3 and of 5 rungs at config 2's shape (4095 chains) and at a quarter of it (1020 chains), whose
placement leaves 2 and 3 of a wave's eight places idle and launches 4/3 and 8/5 as many waves: (a), and (b) and (c) at
swap_every = 1 and 16.
    python tools/small_run_exchange_bench.py > table.txt
    python tools/small_run_exchange_bench.py --packed > packed.txt
    python tools/small_run_exchange_bench.py --plain-only --tree PARENT --label "parent commit" > parent.txt
    python tools/small_run_exchange_bench.py --instances PARENT.log TREE.log > instances.txt
profiles/small_run_replica_exchange.txt is made of these.

Shapes: BASELINE config 1 (SCG, 128 chains, 5 LF, 10 nodes) and config 2 (the 2-D mixture, 4096 chains, 10 LF, 50 nodes).

A window is `steps` MCMC steps between two device synchronisations on the host clock, `steps` a multiple of 256 chosen
per row so that a window of (c) at swap_every = 1 lasts about `--window` seconds, after a warm-up window of the same
length; the variants of a row alternate, REPS windows each.  Reported: median (min .. max).  Every variant includes what
its caller pays for: the histories' copy to the host and the mean accept probability.

`--instances`: registers, scratch and waves per SIMD of the run instances of small_traj_mfma_kernel from two logs of
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=on -Rpass-analysis=kernel-resource-usage \\
        -c l2hmc_amd/csrc/small_mlp.hip
(the parent commit's and this tree's), and whether every instance the parent has kept its figures.  Needs no GPU."""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of (c, swap_every = 1) per timed window")
ap.add_argument("--label", default="this tree")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="root of the (built) tree whose l2hmc_amd is measured")
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--packed", action="store_true")
ap.add_argument("--steps", type=int, default=None,
                help="steps per window instead of the count --window gives (with --plain-only: the count of the full table)")
ap.add_argument("--instances", nargs=2, metavar=("PARENT_LOG", "TREE_LOG"), default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)


# ------------------------------------------------------------------------------------------------ --instances
def _remarks(path):
    """{template arguments of small_traj_mfma_kernel, ten of them: {VGPRs, AGPRs, ScratchSize, Occupancy}}"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True, check=True).stdout
            t = re.search(r"small_traj_mfma_kernel<(.*?)>\(", name)
            cur = None
            if t:
                a = [{"true": "1", "false": "0"}.get(v.strip().replace("(bool)", ""), v.strip())
                     for v in t.group(1).split(",")]
                cur = tuple(a + ["0"] * (10 - len(a)))
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            out[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def instances(parent_log, tree_log):
    P, N = _remarks(parent_log), _remarks(tree_log)
    moved = [k for k in P if N.get(k) != P[k]]
    print(f"# small_traj_mfma_kernel, gfx950 cross-compile: {len(P)} instances in the parent, {len(N)} in this tree; "
          f"instances of the parent whose VGPRs, AGPRs, scratch or waves per SIMD differ in this tree: {len(moved)}"
          + "".join(f"\n#   <{','.join(k)}>: {P[k]} -> {N.get(k)}" for k in moved))
    cell = lambda r: (f"{r['VGPRs']:3d}+{r['AGPRs']:3d} v+a, {r['ScratchSize']:3d} B, occ {r['Occupancy']}"
                      if r else "-").ljust(28)
    forms = sorted({k[:6] for k in N}, key=lambda k: (int(k[1]), int(k[0]), int(k[2]), -int(k[4]), -int(k[5])))
    print("# v+a: VGPRs + AGPRs per lane; B: scratch bytes per lane; occ: waves per SIMD the register count allows")
    for an in ("0", "1"):
        print(f"# AN = {an}: {'rough well, funnel' if an == '1' else 'mixture, Gaussian'}")
        heads = ["TEMPERED, parent", "TEMPERED, this tree", "EXCHANGE, this tree"]
        print(f"# {'<HP,MD,KS,KSH,L1M,TW>':21} | " + " | ".join(h.ljust(28) for h in heads))
        for f in forms:
            cells = [P.get(f + ("1", an, "1", "0")), N.get(f + ("1", an, "1", "0")), N.get(f + ("1", an, "1", "1"))]
            print(f"  <{','.join(f)}>".ljust(23) + " | " + " | ".join(cell(c) for c in cells))


if args.instances:
    instances(*args.instances)
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ timings
import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, ROOT)
import l2hmc_amd as la  # noqa: E402

SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
# name, target, chains, LF steps, nodes, rungs, swap_every
SHAPES = [("cfg 1", "scg", 128, 5, 10, 8, (1, 4, 16)), ("cfg 2", "mog", 4096, 10, 50, 8, (1, 4, 16))]
PACKED = [("cfg 2, 3 rungs", "mog", 4095, 10, 50, 3, (1, 16)), ("cfg 2, 5 rungs", "mog", 4095, 10, 50, 5, (1, 16)),
          ("a quarter of cfg 2, 3 rungs", "mog", 1020, 10, 50, 3, (1, 16)),
          ("a quarter of cfg 2, 5 rungs", "mog", 1020, 10, 50, 5, (1, 16))]


def sampler(target, N, nodes):
    np.random.seed(0)
    torch.manual_seed(0)
    if target == "scg":
        dist = la.Gaussian(np.zeros(2), SCG_SIGMA)
    else:
        dist = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
    dyn = la.Dynamics(2, dist.get_energy_function(), trajectory_length=N, eps=0.1, use_temperature=True,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    return la.DynamicsSampler(dyn, distribution=dist)


class Run:
    """`run` of the ladder (swap_every None), or `run_exchange` with a round every `swap_every` steps, inside the
    launches (`in_launch`) or between them"""

    def __init__(self, target, B, N, nodes, G, swap_every=None, in_launch=False):
        self.smp = sampler(target, N, nodes)
        assert self.smp.steps_per_launch == 256
        self.smp.in_launch = in_launch
        self.x = la._lib.as_dev(self.smp.distribution.get_samples(B))
        self.temps = np.linspace(1.0, 4.5, G)[np.arange(B) % G].astype(np.float32)[None, :]
        self.G, self.k, self.done = G, swap_every, 0

    def window(self, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.k is None:
            self.x = self.smp.run(steps, self.x, keep_samples=False, temperature=self.temps)["samples_out"]
        else:
            out = self.smp.run_exchange(steps, self.x, keep_samples=False, temperature=self.temps, replicas=self.G,
                                        swap_every=self.k, first_parity=self.done % 2)
            self.x, self.done = out["samples_out"], self.done + steps // self.k
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3


med = statistics.median


def timings(shapes):
    fmt = lambda v: f"{med(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
    print(f"# device {torch.cuda.get_device_name(0)}; {args.label}; Dynamics(hmc=False), x_dim 2, eps 0.1, rungs of "
          f"temperature 1.0 .. 4.5, 256 steps per launch, keep_samples=False; ms per MCMC step: median "
          f"(min .. max) of {args.reps} alternating windows")
    for name, target, B, N, nodes, G, ks in shapes:
        var = {"(a) no exchange": Run(target, B, N, nodes, G)}
        if not args.plain_only:
            for k in ks:
                var[f"(b) in launch, swap_every = {k}"] = Run(target, B, N, nodes, G, k, in_launch=True)
                var[f"(c) between,   swap_every = {k}"] = Run(target, B, N, nodes, G, k)
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
        print(f"  {name}: {target}, {B} chains, {N} LF, {nodes} nodes, {G} rungs, {steps} steps per window")
        a = med(times["(a) no exchange"])
        for c in var:
            rel = "" if c.startswith("(a)") else f"/ (a) = {med(times[c]) / a:6.3f}"
            if c.startswith("(c)"):
                b = c.replace("(c) between,  ", "(b) in launch,")
                gap = ("disjoint" if max(times[b]) < min(times[c]) or max(times[c]) < min(times[b]) else "OVERLAPPING")
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


timings(PACKED if args.packed else SHAPES)
