"""Builds libl2hmc_hip.so (the C-ABI library of include/l2hmc_hip.h) in-tree
with hipcc for gfx950.  No GPU is needed to build (hipcc cross-compiles)."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libl2hmc_hip.so")
SOURCES = ["capi.hip", "u1_lattice.hip", "stq_dense.hip", "leapfrog.hip", "small_mlp.hip", "small_hmc.hip", "small_ais.hip", "fused_traj.hip", "fused_traj4.hip", "fused_traj32.hip", "fused_traj_ncp.hip", "hmc_step.hip", "replica_swap.hip",
           "conv3d_front.hip", "mcmc_step.hip", "loss.hip", "train.hip", "small_train.hip", "fused_train.hip",
           "layered_train.hip"]
# every header is a dependency of every object (coarse, but never stale)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "l2hmc_hip.h")]
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function",
         "-ffp-contract=on"]


def _hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libl2hmc_hip.so")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, extra_flags=()):
    hipcc = _hipcc()
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in HEADERS] + [os.path.abspath(__file__)]
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc, *FLAGS, *extra_flags, "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
    if force or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
