"""A tempered RUN of toy-target L2HMC steps (`DynamicsSampler.run(..., temperature=)`, l2hmc_small_run_tempered), ms per
MCMC step:
  (a0) parent run : l2hmc_small_run of the PARENT commit's library (`--parent-lib`, a build of the parent commit), through
                    this tree's `DynamicsSampler.run` (whose untempered path is the parent's);
  (a)  run        : l2hmc_small_run of this tree, no temperature keyword;
  (b1) schedule   : temperature = [steps], an anneal from 3 to 1;
  (b2) ladder     : temperature = [1, chains], 1 .. 3 across the chains;
  (c)  loop       : `steps_per_launch = 1` with the same schedule: `dynamics.temperature` set before every `propose`, the
                    way to anneal before this entry.
    python tools/small_run_tempered_bench.py --parent-lib PARENT/libl2hmc_hip.so > timings.txt
    python tools/small_run_tempered_bench.py --instances PARENT.log TREE.log > table.txt
profiles/small_run_tempered.txt is the two outputs, one after the other.

Shapes, windows and reporting as tools/small_run_bench.py: BASELINE config 1 (SCG, 128 chains, 5 LF, 10 nodes), config 2
(MoG, 4096 chains, 10 LF, 50 nodes) and the reference's evaluation shape (mog_model.py:394: MoG, 500 chains, 100 steps).
A window is `run(STEPS, x)` between two device synchronisations on the host clock, all variants in one process and
alternating, REPS windows each after a warm-up window; median (min .. max).

`--instances`: the table of registers, scratch and waves per SIMD of every small_traj_mfma_kernel instance from two logs of
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=on -Rpass-analysis=kernel-resource-usage \\
        -c l2hmc_amd/csrc/small_mlp.hip
(the parent commit's and this tree's).  Needs no GPU."""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--window", type=float, default=0.3, help="seconds of the loop per timed window (sets the step count)")
ap.add_argument("--parent-lib", default=None, help="libl2hmc_hip.so built from the parent commit: adds column (a0)")
ap.add_argument("--instances", nargs=2, metavar=("PARENT_LOG", "TREE_LOG"), default=None)
args = ap.parse_args()


# ------------------------------------------------------------------------------------------------ --instances
def _remarks(path):
    """{template arguments of small_traj_mfma_kernel, nine of them: (VGPRs, AGPRs, scratch bytes, waves per SIMD)}"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True, check=True).stdout
            t = re.search(r"small_traj_mfma_kernel<(.*?)>\(", name)
            cur = None
            if t:
                a = [{"true": "1", "false": "0"}.get(v.strip().replace("(bool)", ""), v.strip()) for v in t.group(1).split(",")]
                cur = tuple(a + ["0"] * (9 - len(a)))
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            out[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def instances(parent_log, tree_log):
    P, N = _remarks(parent_log), _remarks(tree_log)
    cell = lambda r: (f"{r['VGPRs']:3d}+{r['AGPRs']:3d} v+a, {r['ScratchSize']:3d} B, occ {r['Occupancy']}"
                      if r else "-").ljust(28)
    forms = sorted({k[:6] for k in N}, key=lambda k: (int(k[1]), int(k[0]), int(k[2]), -int(k[4]), -int(k[5])))
    print("# Compiler figures of every small_traj_mfma_kernel instance, gfx950 cross-compile (v+a: VGPRs + AGPRs per lane; B: "
          "scratch bytes per lane;\n# occ: waves per SIMD the register count allows)")
    for an in ("0", "1"):
        print(f"# AN = {an}: {'rough well, funnel' if an == '1' else 'mixture, Gaussian'}")
        heads = ["single pass, parent", "single pass, this tree", "RUN, parent", "RUN, this tree", "TEMPERED, this tree"]
        print(f"# {'<HP,MD,KS,KSH,L1M,TW>':21} | " + " | ".join(h.ljust(28) for h in heads))
        for f in forms:
            cells = [P.get(f + ("0", an, "0")), N.get(f + ("0", an, "0")), P.get(f + ("1", an, "0")),
                     N.get(f + ("1", an, "0")), N.get(f + ("1", an, "1"))]
            print(f"  <{','.join(f)}>".ljust(23) + " | " + " | ".join(cell(c) for c in cells))


if args.instances:
    instances(*args.instances)
    sys.exit(0)

# ------------------------------------------------------------------------------------------------ timings
import numpy as np  # noqa: E402
import torch  # noqa: E402

import l2hmc_amd as la  # noqa: E402
from l2hmc_amd import _lib  # noqa: E402

SCG_SIGMA = np.array([[50.05, -49.95], [-49.95, 50.05]])
# name, target, chains, LF steps, nodes, fixed step count (None = by --window)
SHAPES = [("cfg 1", "scg", 128, 5, 10, None), ("cfg 2", "mog", 4096, 10, 50, None),
          ("eval, 100 steps", "mog", 500, 10, 50, 100)]

TREE = _lib.lib()
PARENT = None
if args.parent_lib:
    PARENT = C.CDLL(os.path.abspath(args.parent_lib))
    for name, (res, argtypes) in _lib._PROTOS.items():
        if hasattr(PARENT, name):
            fn = getattr(PARENT, name)
            fn.restype, fn.argtypes = res, argtypes
    assert not hasattr(PARENT, "l2hmc_small_run_tempered"), "--parent-lib already has the tempered entry"


def sampler(target, N, nodes, spl):
    np.random.seed(0)
    torch.manual_seed(0)
    if target == "scg":
        dist = la.Gaussian(np.zeros(2), SCG_SIGMA)
    else:
        dist = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])
    dyn = la.Dynamics(2, dist.get_energy_function(), trajectory_length=N, eps=0.1, use_temperature=True,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    smp = la.DynamicsSampler(dyn, distribution=dist)
    smp.steps_per_launch = spl
    return smp


def run_window(smp, x, steps, temperature, handle):
    _lib._lib = handle                      # the library `DynamicsSampler.run` calls into
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = smp.run(steps, x, keep_samples=False, temperature=temperature)["samples_out"]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, x
    finally:
        _lib._lib = TREE


fmt = lambda v: f"{statistics.median(v):7.4f} ({min(v):.4f} .. {max(v):.4f})"
print(f"# device {torch.cuda.get_device_name(0)}; DynamicsSampler.run, x_dim 2, eps 0.1, use_temperature=True, "
      f"keep_samples=False; ms per MCMC step: median (min .. max) of {args.reps} alternating windows")
cols = (["(a0) parent run"] if PARENT else []) + ["(a) run", "(b1) schedule", "(b2) ladder", "(c) loop, T per step"]
print(f"# {'shape':>16} {'target':>6} {'chains':>6} {'LF':>3} {'nodes':>5} {'steps':>6} | "
      + " | ".join(f"{c:>26}" for c in cols) + " | (b1)/(a) (b2)/(a) (c)/(b1)")
for name, target, B, N, nodes, fixed in SHAPES:
    one, loop = sampler(target, N, nodes, 256), sampler(target, N, nodes, 1)
    x0 = la._lib.as_dev(one.distribution.get_samples(B))
    dt, _ = run_window(loop, x0, 256, None, TREE)                       # first touch, and the step count
    dt, _ = run_window(loop, x0, 256, None, TREE)
    steps = fixed or max(2, round(args.window / (dt * 1e-3) / 256)) * 256
    schedule = np.geomspace(3.0, 1.0, steps).astype(np.float32)
    ladder = np.linspace(1.0, 3.0, B, dtype=np.float32)[None]
    # variant: (sampler, temperature, library)
    var = {"(a0) parent run": (one, None, PARENT), "(a) run": (one, None, TREE), "(b1) schedule": (one, schedule, TREE),
           "(b2) ladder": (one, ladder, TREE), "(c) loop, T per step": (loop, schedule, TREE)}
    var = {k: var[k] for k in cols}
    xs = {k: x0.clone() for k in var}
    for k, (smp, t, h) in var.items():                                  # warm-up at the windows' own size
        _, xs[k] = run_window(smp, xs[k], steps, t, h)
    times = {c: [] for c in cols}
    for _ in range(args.reps):
        for k, (smp, t, h) in var.items():
            dt, xs[k] = run_window(smp, xs[k], steps, t, h)
            times[k].append(dt)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"  {name:>16} {target:>6} {B:6d} {N:3d} {nodes:5d} {steps:6d} | "
          + " | ".join(f"{fmt(times[c]):>26}" for c in cols)
          + f" | {med['(b1) schedule'] / med['(a) run']:8.3f} {med['(b2) ladder'] / med['(a) run']:8.3f} "
            f"{med['(c) loop, T per step'] / med['(b1) schedule']:9.2f}x", flush=True)
    del var, xs
