"""The one-launch training forward of the torus-exact mode (`GaugeDynamics(periodic=True, tiled_train=True,
fused_forward=True)`, L2HMC_PLAN_PERIODIC_TAPE) against the layer-by-layer forward it replaces and against the reference
mode; the tables of profiles/periodic_train_forward.txt (a), (b) and (d).  Shape: 8x8, GenericNet H = 512, 10 leapfrog
steps, 2048 + 2048 chains, beta 2, eps0 0.25.
    python tools/periodic_train_forward_bench.py > table.txt
(a) `calc_loss_and_grads` and `train_step` of four trainers living in one process: three warm-up steps each, then
    `--reps` rounds in which every trainer in turn runs a window of `--steps` steps between two device synchronisations
    on the host clock.  Reported: median (min .. max) of the windows, ms per step.
(b) the forward alone: kernel time of profile class 5 (HIP events on the launch stream, `l2hmc_profile_begin` / `_end`)
    of the taped launch and of the untaped `l2hmc_gauge_trajectory` on the same 4096 rows, and the host-clock window of
    `l2hmc_gauge_train_forward` with and without the flag (what the launch replaces).
(d) `--q10`: the recipe of profiles/periodic_train.txt (c), trained with the flag."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
ap.add_argument("--chains", type=int, default=2048)
ap.add_argument("--lf", type=int, default=10)
ap.add_argument("--q10", action="store_true", help="also train and sample the Q10 recipe (about a minute)")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from l2hmc_amd import GaugeDynamics, GaugeLattice, GaugeSampler, _lib  # noqa: E402
from l2hmc_amd.gauge_trainer import GaugeTrainer  # noqa: E402

T = X = 8
D, B, BETA, EPS = 2 * T * X, args.chains, 2.0, 0.25
med = statistics.median
fmt = lambda v: f"{med(v):8.3f} ms   (windows {min(v):.3f} - {max(v):.3f})"      # noqa: E731


def dynamics(chains=B, **kw):
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=chains, rand=False)
    return GaugeDynamics(lat, lat.get_energy_function(), eps=EPS, hmc=False, num_steps=args.lf, eps_trainable=True,
                         network_arch='generic', seed=5, **kw)


def windows(cands, run):
    """cands: {name: object}; run(object): one step.  Warm-up, then alternating windows -> {name: [ms per step]}."""
    for c in cands.values():
        for _ in range(3):
            run(c)
    times = {k: [] for k in cands}
    for _ in range(args.reps):
        for k, c in cands.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(c)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.steps * 1e3)
    return times


print(f"# device {torch.cuda.get_device_name(0)}; {T}x{X}, {B} + {B} chains, H = 512, {args.lf} LF, beta {BETA}, eps0 {EPS}; "
      f"{args.reps} alternating windows of {args.steps} steps after 3 warm-up steps")

# ---- (a) the training step -----------------------------------------------------------------------------------------
KINDS = {"periodic, one-launch forward (fused_forward=True)": dict(periodic=True, tiled_train=True, fused_forward=True),
         "periodic, tiled entries (tiled_train=True)": dict(periodic=True, tiled_train=True),
         "reference mode, tiled entries (fused=False)": dict(fused=False),
         "reference mode, fused training kernels": dict()}
trainers = {k: GaugeTrainer(dynamics(**kw), lr_init=1e-4) for k, kw in KINDS.items()}
x = torch.rand(B, D, device="cuda") * (2 * np.pi)
for what, run in (("GaugeTrainer.calc_loss_and_grads", lambda tr: tr.calc_loss_and_grads(x, BETA)),
                  ("GaugeTrainer.train_step (+ Adam)", lambda tr: tr.train_step(x, BETA))):
    print(f"(a) {what}")
    t = windows(trainers, run)
    for k in KINDS:
        print(f"    {k:<52} {fmt(t[k])}")
    ks = list(KINDS)
    lo, hi = t[ks[0]], t[ks[1]]
    print(f"    flagged / unflagged = {med(lo) / med(hi):.3f}; ranges {'disjoint' if max(lo) < min(hi) else 'OVERLAP'}")
del trainers

# ---- (b) the forward alone -----------------------------------------------------------------------------------------
L = _lib.lib()
R = 2 * B
x0 = torch.rand(R, D, device="cuda") * (2 * np.pi)
v0 = torch.randn(R, D, device="cuda")
dirs = torch.cat([torch.zeros(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32)]).cuda()
outs = [torch.empty_like(x0), torch.empty_like(x0), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")]


def forward_of(dyn, train):
    plan = dyn._plan()
    nb = int((L.l2hmc_gauge_train_ws_bytes if train else L.l2hmc_gauge_ws_bytes)(C.byref(plan), R))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda")
    name = "l2hmc_gauge_train_forward" if train else "l2hmc_gauge_trajectory"
    return lambda: _lib.call(name, C.byref(plan), BETA, x0, v0, dirs, R, *outs, ws, nb, device=x0.device)


def class5_ms(run):
    _lib.check(L.l2hmc_profile_begin(5))
    for _ in range(args.steps):
        run()
    ms, n = C.c_double(), C.c_int64()
    _lib.check(L.l2hmc_profile_end(C.byref(ms), C.byref(n)))
    assert n.value == args.steps, n.value
    return ms.value / n.value


fw = {"taped launch (l2hmc_gauge_train_forward, flagged)": forward_of(dynamics(periodic=True, tiled_train=True,
                                                                              fused_forward=True), True),
      "untaped launch (l2hmc_gauge_trajectory, whole_step)": forward_of(dynamics(periodic=True, whole_step=True), False),
      "layer-by-layer taped forward (unflagged)": forward_of(dynamics(periodic=True, tiled_train=True), True)}
for f in fw.values():
    for _ in range(3):
        f()
torch.cuda.synchronize()
ks = list(fw)
kt = {k: [] for k in ks[:2]}
for _ in range(args.reps):
    for k in ks[:2]:
        kt[k].append(class5_ms(fw[k]))
print(f"(b) the forward alone, {R} rows: class-5 kernel time")
for k in ks[:2]:
    print(f"    {k:<52} {fmt(kt[k])}")
print(f"    taped / untaped = {med(kt[ks[0]]) / med(kt[ks[1]]):.3f}")
print("    host-clock windows of the whole entry (copies, mask inversion and all launches)")
t = windows({k: fw[k] for k in (ks[0], ks[2])}, lambda f: f())
for k in (ks[0], ks[2]):
    print(f"    {k:<52} {fmt(t[k])}")
del fw

# ---- (d) the Q10 recipe --------------------------------------------------------------------------------------------
if args.q10:
    dyn = dynamics(periodic=True, tiled_train=True, fused_forward=True, whole_step=True)
    tr = GaugeTrainer(dyn, lr_init=3e-4, lr_decay_steps=100, lr_decay_rate=0.96)
    torch.manual_seed(5)
    xs = torch.rand(B, D, device="cuda") * (2 * np.pi)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = tr.train(1000, samples_init=xs, beta_init=BETA, beta_final=BETA)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    print(f"(d) Q10 recipe with the flag: trained 1000 steps in {secs:.1f} s; accept {float(np.mean(out['accept_prob'][-50:])):.3f}, "
          f"eps {float(dyn.eps):.4f} at the end of training")
    smp = GaugeSampler(dyn)
    xs = smp.run(500, BETA, x=out["samples"])["samples_out"]
    blocks, px, dq = [], [], []
    for _ in range(4):
        res = smp.run(500, BETA, x=xs)
        xs = res["samples_out"]
        blocks.append(res["plaqs"])
        px.append(res["px"].mean())
        dq.append(res["charge_diff"].mean())
    per_chain = np.concatenate(blocks).mean(axis=0)
    mean, err = per_chain.mean(), per_chain.std(ddof=1) / np.sqrt(per_chain.size)
    exact = 0.69777
    print(f"    <plaquette> {mean:.5f} +- {err:.5f}  ({(mean - exact) / err:+.1f} standard errors from {exact})   blocks "
          + " ".join(f"{b.mean():.4f}" for b in blocks))
    print(f"    accept {np.mean(px):.3f}, |dQ| per step {np.mean(dq):.3f}")
