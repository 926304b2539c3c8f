"""Are the training steps of two source trees the same bits, and the same speed, on ONE library build?

    python tools/train_step_bits.py dump OUT.npz [--tree DIR]     every case below, three train_steps each, fixed seeds
    python tools/train_step_bits.py compare A.npz B.npz           numpy.array_equal per array; exit 1 on a difference
    python tools/train_step_bits.py time OUT.json [--tree DIR]    ms per train_step of the five timing cases
    python tools/train_step_bits.py run PARENT_TREE OUT_DIR       dump(parent), dump(this tree), compare (dumps in
                                                                  a temporary directory), then time parent / this
                                                                  tree alternating, three rounds (JSON in OUT_DIR)

`--tree` is the checkout whose `l2hmc_amd` package is imported (default: the one this file lies in); the library is
always this checkout's libl2hmc_hip.so (L2HMC_LIB_PATH), so only the host Python differs.  `run` starts every dump and
every timing in a fresh child process under its own `timeout` and stops at the first one that fails."""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3


def _import(tree):
    os.environ["L2HMC_LIB_PATH"] = os.path.join(HERE, "l2hmc_amd", "libl2hmc_hip.so")
    sys.path.insert(0, os.path.abspath(tree))
    import l2hmc_amd as la
    assert os.path.dirname(os.path.dirname(os.path.abspath(la.__file__))) == os.path.abspath(tree), la.__file__
    return la


# ---- cases: name -> (trainer, step(i) -> outputs of train_step) -------------------------------------------------
def _gauge(la, T, X, B, N=3, arch='generic', layered=None, inject=False, seed=42, eps=0.2, **kw):
    import numpy as np
    import torch
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    np.random.seed(seed)
    lat = la.GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=True)
    dyn = la.GaugeDynamics(lat, lat.get_energy_function(), eps=eps, hmc=False, network_arch=arch, num_steps=N,
                           eps_trainable=kw.pop("eps_trainable", True))
    tr = GaugeTrainer(dyn, lr_init=1e-3, **kw)
    tr.layered = layered
    x = torch.as_tensor(lat.samples.reshape(B, -1), dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(seed + 1)
    D = x.shape[1]

    def step(i):
        draws = {}
        if inject:
            mk = lambda: (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B),   # noqa: E731
                          rng.uniform(size=B))
            draws = dict(z=rng.standard_normal((B, D)), draws_x=mk(), draws_z=mk())
        return tr.train_step(x, 2.0 + 0.25 * i, **draws)
    return tr, step


def _quartic(x):
    import torch
    return ((x * x - 1.) ** 2).sum(dim=1) / 4. + 0.3 * (x * torch.roll(x, -1, dims=1)).sum(dim=1)


def _toy(la, kind, B, nodes=50, N=5, inject=False, seed=42, layered=False):
    import numpy as np
    import torch
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    np.random.seed(seed)
    if kind == "mog":
        dim, eps = 2, 0.1
        fn = la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5]).get_energy_function()
    elif kind == "gaussian":
        dim, eps = 2, 0.1
        fn = la.Gaussian(np.zeros(2), np.array([[50.05, -49.95], [-49.95, 50.05]])).get_energy_function()
    elif kind == "icg50":
        dim, eps = 50, 0.05
        prec = torch.tensor((1. / np.logspace(-2, 2, 50)).astype(np.float32), device="cuda")
        fn = lambda x: 0.5 * (x * x * prec).sum(dim=1)   # noqa: E731
    else:
        dim, eps, fn = 20, 0.05, _quartic
    dyn = la.Dynamics(dim, fn, trajectory_length=N, eps=eps,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    if layered:
        dyn.layered = True
    tr = DynamicsTrainer(dyn, scale=0.1)
    rng = np.random.default_rng(seed + 1)
    state = {"x": torch.as_tensor(rng.normal(0, 0.8, (B, dim)), dtype=torch.float32, device="cuda")}

    def step(i):
        draws = {}
        if inject:
            mk = lambda: (rng.standard_normal((B, dim)), rng.standard_normal((B, dim)),   # noqa: E731
                          rng.integers(0, 2, B).astype(np.float64), rng.uniform(size=B))
            draws = dict(z=rng.standard_normal((B, dim)), draws_x=mk(), draws_z=mk())
        out = tr.train_step(state["x"], **draws)
        state["x"] = out[1]
        return out
    return tr, step


def bit_cases(la):
    """name -> builder; every case once with injected draws (`/inj`) and once with the trainer's own (`/own`)."""
    base = {
        "gauge/tiled8x8": lambda j: _gauge(la, 8, 8, 48, inject=j),
        "gauge/tiled8x8_clip": lambda j: _gauge(la, 8, 8, 48, inject=j, clip_value=0.5),
        "gauge/tiled8x8_eager": lambda j: _gauge(la, 8, 8, 48, inject=j, eager_variables=True, eps_trainable=False),
        "gauge/tiled8x8_clip_eager": lambda j: _gauge(la, 8, 8, 48, inject=j, clip_value=0.5, eager_variables=True,
                                                      eps_trainable=False),
        "gauge/conv3D8x8": lambda j: _gauge(la, 8, 8, 32, arch='conv3D', inject=j),
        "gauge/layered6x6": lambda j: _gauge(la, 6, 6, 37, inject=j),
        "gauge/layered3x5": lambda j: _gauge(la, 3, 5, 19, N=2, inject=j),
        "gauge/layered8x8_forced": lambda j: _gauge(la, 8, 8, 24, layered=True, inject=j),
        "toy/mog": lambda j: _toy(la, "mog", 64, inject=j),
        "toy/gaussian": lambda j: _toy(la, "gaussian", 64, inject=j),
        "toy/layered_icg50": lambda j: _toy(la, "icg50", 33, nodes=100, inject=j),
        "toy/layered_quartic": lambda j: _toy(la, "quartic", 9, nodes=100, N=10, inject=j),
    }
    return {f"{k}/{'inj' if j else 'own'}": (lambda b=b, j=j: b(j)) for k, b in base.items() for j in (True, False)}


def time_cases(la):
    return {
        "gauge cfg-3 GenericNet 8x8, 2048 chains, 10 LF": lambda: _gauge(la, 8, 8, 2048, N=10, eps=0.25),
        "gauge ConvNet3D 8x8, 2048 chains, 10 LF": lambda: _gauge(la, 8, 8, 2048, N=10, eps=0.25, arch='conv3D'),
        "gauge layered 6x6, 512 chains, 5 LF": lambda: _gauge(la, 6, 6, 512, N=5),
        "toy layered x_dim 50 / 100 nodes, 512 chains, 10 LF": lambda: _toy(la, "icg50", 512, nodes=100, N=10),
        "toy one-launch mog, 512 chains, 10 LF": lambda: _toy(la, "mog", 512, N=10),
    }


# ---- modes ------------------------------------------------------------------------------------------------------
def dump(out, tree):
    import numpy as np
    import torch
    la = _import(tree)
    arrays = {}
    for name, build in bit_cases(la).items():
        tr, step = build()
        for i in range(STEPS):
            res = step(i)
            torch.cuda.synchronize()
            rec = dict(zip(("loss", "x_out", "px", "x_dq"), res))
            rec.update(grads=tr.grads, m=tr._m, v=tr._v, xnet=tr._nets[0].flat_params()[0],
                       vnet=tr._nets[1].flat_params()[0],
                       step_size=tr.dynamics.alpha if name.startswith("toy") else tr.dynamics.eps,
                       draws=tr.dynamics._draws, last_bucket_count=getattr(tr, "last_bucket_count", 0))
            for k, v in rec.items():
                arrays[f"{name}/step{i}/{k}"] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
        layered = tr._walk is not None if name.startswith("gauge") else tr._layered is not None
        assert layered == ("layered" in name), name
        print(f"{name}: loss {float(rec['loss']):.6g}  mean px {float(rec['px'].mean()):.4f}", flush=True)
    np.savez(out, **arrays)
    print(f"dump: {len(arrays)} arrays of {len(bit_cases(la))} cases -> {out}")


def compare(a, b):
    import numpy as np
    with np.load(a) as fa, np.load(b) as fb:
        if sorted(fa.files) != sorted(fb.files):
            print("compare: the dumps hold different arrays:", sorted(set(fa.files) ^ set(fb.files))[:10])
            return 1
        bad = [k for k in fa.files if not (fa[k].dtype == fb[k].dtype and np.array_equal(fa[k], fb[k]))]
        finite = sum(bool(np.isfinite(fa[k]).all()) for k in fa.files)
        print(f"compare: {len(fa.files)} arrays compared ({finite} all-finite), {len(bad)} differ")
        for k in bad[:20]:
            print("  differs:", k)
    return 1 if bad else 0


def time_steps(out, tree):
    import torch
    la = _import(tree)
    res = {}
    for name, build in time_cases(la).items():
        tr, step = build()
        for i in range(3):
            step(i)
        iters = 20
        while True:                      # at least a second of steps: the one-launch trainer's step is under a ms
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                step(i)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= 1.0:
                break
            iters = int(1.2 * iters / dt) + 1
        res[name] = 1e3 * dt / iters
        print(f"{name}: {res[name]:.3f} ms per train_step", flush=True)
    with open(out, "w") as f:
        json.dump(res, f)


def run(parent, outdir):
    import tempfile
    os.makedirs(outdir, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    o = lambda n: os.path.join(outdir, n)   # noqa: E731
    tmp = tempfile.TemporaryDirectory()      # the dumps hold every weight and moment of every step: not kept
    d = lambda n: os.path.join(tmp.name, n)   # noqa: E731

    def child(limit, *args):             # a fresh process under its own time limit; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(limit), *me, *args]).returncode
        if rc != 0:
            sys.exit(f"run: {' '.join(args)} ended with status {rc}; nothing more is started")
    child(300, "dump", d("bits_parent.npz"), "--tree", parent)
    child(300, "dump", d("bits_new.npz"), "--tree", HERE)
    child(60, "compare", d("bits_parent.npz"), d("bits_new.npz"))
    tmp.cleanup()
    rounds = {"parent": [], "new": []}
    for r in range(3):
        for who, tree in (("parent", parent), ("new", HERE)):
            child(200, "time", o(f"time_{who}_{r}.json"), "--tree", tree)
            with open(o(f"time_{who}_{r}.json")) as f:
                rounds[who].append(json.load(f))
    print(f"{'case':<54} {'parent repeats (ms)':<24} {'new repeats':<24} spread   med P   med N     N-P  ok")
    for name in rounds["parent"][0]:
        p, n = ([r[name] for r in rounds[w]] for w in ("parent", "new"))
        spread, mp, mn = max(p) - min(p), statistics.median(p), statistics.median(n)
        print(f"{name:<54} {' '.join(f'{v:.3f}' for v in p):<24} {' '.join(f'{v:.3f}' for v in n):<24} "
              f"{spread:6.3f} {mp:7.3f} {mn:7.3f} {mn - mp:+7.3f}  {'yes' if mn <= mp + spread else 'NO'}")


if __name__ == "__main__":
    mode, args = sys.argv[1], sys.argv[2:]
    tree = HERE
    if "--tree" in args:
        i = args.index("--tree")
        tree = args[i + 1]
        del args[i:i + 2]
    if mode == "dump":
        dump(args[0], tree)
    elif mode == "compare":
        sys.exit(compare(*args))
    elif mode == "time":
        time_steps(args[0], tree)
    elif mode == "run":
        run(*args)
    else:
        sys.exit(__doc__)
