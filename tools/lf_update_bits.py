"""Does every path through the leapfrog sub-update arithmetic (csrc/lf_update.h) give the bits of the parent commit?

    python tools/lf_update_bits.py build PARENT_TREE OUT_DIR      the parent's library -> OUT_DIR/libl2hmc_hip_parent.so
    python tools/lf_update_bits.py dump GROUP OUT.npz             one group of cases with the library L2HMC_LIB_PATH names
    python tools/lf_update_bits.py run PARENT_TREE OUT_DIR [GROUP]
                                                                  build (unless OUT_DIR already holds the library), then per
                                                                  group (or for GROUP alone): dump(parent), dump(this
                                                                  tree), compare
    python tools/lf_update_bits.py time OUT.json [ONLY]           ms per call of every timing case (or of those whose name
                                                                  holds ONLY), one after another in this process,
                                                                  library as for dump
    python tools/lf_update_bits.py timing PARENT_TREE OUT_DIR [ONLY]
                                                                  build, then time(parent), time(this tree) alternating,
                                                                  three rounds (one child process per library and
                                                                  round), and the table with the bound

The Python package is this checkout's for both dumps; only the library differs.  `run` starts every dump in a fresh
child process under its own `timeout`, one after another, and stops at the first child that fails.  Seeds and draws are
fixed; every output array must be numpy.array_equal with the same dtype.  `timing` does the same with one child per
library and round: a child runs all timing cases in turn (at least a second of calls each), so a case starts from the
allocator and clock state the cases before it left; bound: new median <= parent median + the parent's spread."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
PARENT_LIB = "libl2hmc_hip_parent.so"


# ---- inputs -----------------------------------------------------------------------------------------------------
def _dev(a, dtype=None):
    import numpy as np
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float32, device="cuda")


def _gauge_dyn(la, T, X, B, N=2, seed=42, **kw):
    import numpy as np
    np.random.seed(seed)
    lat = la.GaugeLattice(T, X, 2, 'U1', num_samples=B, rand=True)
    dyn = la.GaugeDynamics(lat, lat.get_energy_function(), eps=0.2, num_steps=N, **kw)
    rng = np.random.default_rng(seed + 1)
    D = 2 * T * X
    x = _dev(rng.uniform(0, 2 * np.pi, (B, D)))
    v = _dev(rng.standard_normal((B, D)))
    return dyn, x, v, rng


def _trajectory(dyn, x, v, beta, dirs):
    """l2hmc_gauge_trajectory with a per-row direction array."""
    import ctypes as C
    import torch
    from l2hmc_amd import _lib
    rows = x.shape[0]
    xo, vo = torch.empty_like(x), torch.empty_like(x)
    sld = torch.empty(rows, dtype=torch.float32, device=x.device)
    p = torch.empty_like(sld)
    plan, L = dyn._plan(), _lib.lib()
    ws, nb = dyn._ws.get(L.l2hmc_gauge_ws_bytes(C.byref(plan), rows), x.device)
    _lib.call("l2hmc_gauge_trajectory", C.byref(plan), float(beta), x, v, dirs, rows, xo, vo, sld, p, ws, nb,
              device=dyn._device)
    return xo, vo, sld, p


def _form_rows():
    """{rows per workgroup: a ragged row count that selects that form of the whole-trajectory launch on THIS device}
    (launch_fused_trajectory: at most 4 / 8 / 12 rows per CU -> sub-tile form, up to 16 per CU -> 16-row form, more ->
    32-row form), cross-checked against the library's own cut of a step wherever that is one launch."""
    import ctypes as C
    import torch
    from l2hmc_amd import _lib
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    forms = {4: 4 * cus - 3, 8: 8 * cus - 3, 12: 12 * cus - 3, 16: 16 * cus - 3, 32: 16 * cus + 5}
    rows_out, rpw_out = (C.c_int64 * 3)(), (C.c_int32 * 3)()
    for form in (4, 8, 12):
        n = _lib.lib().l2hmc_gauge_step_plan(forms[form], cus, rows_out, rpw_out)
        assert n == 1 and rpw_out[0] == form, (form, forms[form], cus, n, list(rpw_out))
    return forms


def _mixed_dirs(rng, rows):
    import torch
    return _dev(rng.integers(0, 2, rows), torch.int32)


def _fractional_masks(rng, N, D):
    import numpy as np
    return rng.choice(np.array([0., 0.25, 1.], dtype=np.float32), size=(N, D))


def _train_steps(tr, x, beta, out, name, steps=2):
    for i in range(steps):
        res = tr.train_step(x, beta + 0.25 * i)
        for k, a in zip(("loss", "x_out", "px", "x_dq"), res):
            out[f"{name}/step{i}/{k}"] = a
        out[f"{name}/step{i}/grads"] = tr.grads.clone()


# ---- groups: name -> {array name: tensor} -----------------------------------------------------------------------
def group_ops(la, out):
    """the standalone sub-updates and their reverses at 5 x 70 (ragged waves), fractional keep, NULL S/T/Q."""
    import numpy as np
    import torch
    from l2hmc_amd import _lib, ops
    rng = np.random.default_rng(5)
    R, D, eps = 5, 70, 0.17
    x, v, g, S, T, Q, u = (_dev(rng.standard_normal((R, D))) for _ in range(7))
    keep = _dev(rng.choice(np.array([0., 0.25, 1.], dtype=np.float32), size=D))
    dld = _dev(rng.standard_normal(R))
    for d in (0, 1):
        for tag, stq in (("stq", (S, T, Q)), ("null", (None, None, None))):
            out[f"ops/v/{tag}/dir{d}/out"], out[f"ops/v/{tag}/dir{d}/ld"] = ops.lf_update_v(v, g, *stq, eps, d)
            out[f"ops/x/{tag}/dir{d}/out"], out[f"ops/x/{tag}/dir{d}/ld"] = ops.lf_update_x(x, v, keep, *stq, eps, d)
        o = {k: torch.empty_like(x) for k in ("dv", "dg", "dS", "dT", "dQ")}
        de = torch.empty(R, dtype=torch.float32, device="cuda")
        _lib.call("l2hmc_lf_update_v_vjp", v, g, S, T, Q, eps, d, R, D, u, dld, o["dv"], o["dg"], o["dS"], o["dT"], o["dQ"],
                  de, device=x.device)
        out.update({f"ops/v_vjp/dir{d}/{k}": a for k, a in o.items()})
        out[f"ops/v_vjp/dir{d}/deps"] = de
        o = {k: torch.empty_like(x) for k in ("dx", "dv", "dS", "dT", "dQ")}
        de = torch.empty(R, dtype=torch.float32, device="cuda")
        _lib.call("l2hmc_lf_update_x_vjp", x, v, keep, S, T, Q, eps, d, R, D, u, dld, o["dx"], o["dv"], o["dS"], o["dT"],
                  o["dQ"], de, device=x.device)
        out.update({f"ops/x_vjp/dir{d}/{k}": a for k, a in o.items()})
        out[f"ops/x_vjp/dir{d}/deps"] = de


def group_layered(la, out):
    """layer-by-layer lattice plans: 4 x 6, 33 rows, 2 leapfrog steps, mixed per-row directions."""
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    beta = 2.0
    # heads_element (active columns, binary masks; every column, fractional masks)
    dyn, x, v, rng = _gauge_dyn(la, 4, 6, 33, fused=False)
    dirs = _mixed_dirs(rng, 33)
    for k, a in zip(("x", "v", "sld", "p"), _trajectory(dyn, x, v, beta, dirs)):
        out[f"layered/traj4x6/{k}"] = a
    dyn.all_columns = True
    dyn.set_masks(_fractional_masks(rng, 2, 48))
    for k, a in zip(("x", "v", "sld", "p"), _trajectory(dyn, x, v, beta, dirs)):
        out[f"layered/traj4x6_fractional/{k}"] = a
    # lf_update_{v,x}_kernel with a per-row direction array and NULL S/T/Q: the plain-HMC plan, fractional masks
    dyn, x, v, rng = _gauge_dyn(la, 4, 6, 33, fused=False, hmc=True)
    dyn.set_masks(_fractional_masks(rng, 2, 48))
    for k, a in zip(("x", "v", "sld", "p"), _trajectory(dyn, x, v, beta, _mixed_dirs(rng, 33))):
        out[f"layered/hmc4x6_fractional/{k}"] = a
    # layered-training entries (l2hmc_lf_update_{v,x}_vjp through GaugeTrainer's layered walk) on the 4 x 6 plan
    dyn, x, v, rng = _gauge_dyn(la, 4, 6, 33)
    _train_steps(GaugeTrainer(dyn, lr_init=1e-3), x, beta, out, "layered/train4x6_walk")
    # l2hmc_gauge_train_forward / _backward on a layered plan (train_update_kernel, update_bwd_kernel): those entries
    # take widths that are multiples of 32, so 4 x 8
    dyn, x, v, rng = _gauge_dyn(la, 4, 8, 33, fused=False)
    tr = GaugeTrainer(dyn, lr_init=1e-3)
    tr.layered = False
    _train_steps(tr, x, beta, out, "layered/train4x8_tiled")


def group_fused(la, out):
    """whole-trajectory kernels at 8 x 8, 2 leapfrog steps, binary masks; the row counts select each form of the
    trajectory launch from the device's CU count (_form_rows)."""
    from l2hmc_amd import GaugeSampler
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    beta = 2.0
    for form, B in _form_rows().items():
        dyn, x, v, rng = _gauge_dyn(la, 8, 8, B)
        for k, a in zip(("x", "v", "sld", "p"), _trajectory(dyn, x, v, beta, _mixed_dirs(rng, B))):
            out[f"fused/traj_{form}row/{k}"] = a
    dyn, x, v, rng = _gauge_dyn(la, 8, 8, 200)
    dirs = _mixed_dirs(rng, 200)
    for tag, flags in (("tiles16", {}), ("tiles16_all_columns", {"all_columns": True}), ("tiles16_full_l1", {"full_l1": True})):
        dyn.tiles16_only, dyn.all_columns, dyn.full_l1 = True, False, False
        for k_, v_ in flags.items():
            setattr(dyn, k_, v_)
        for k, a in zip(("x", "v", "sld", "p"), _trajectory(dyn, x, v, beta, dirs)):
            out[f"fused/{tag}/{k}"] = a
    # one whole MCMC step (l2hmc_gauge_mcmc_step: the active-column position update with and without the kept-column
    # first layer, every column, the sub-tile form) and a transition with both directions in one launch (dir_split)
    for tag, flags in (("tiles16", {"tiles16_only": True}), ("tiles16_full_l1", {"tiles16_only": True, "full_l1": True}),
                       ("tiles16_all_columns", {"tiles16_only": True, "all_columns": True}), ("subtile", {})):
        dyn, x, v, rng = _gauge_dyn(la, 8, 8, 200)
        for k_, v_ in flags.items():
            setattr(dyn, k_, v_)
        dyn._draws = 40
        xn, px, obs, dq = GaugeSampler(dyn).step(x, beta)
        out[f"fused/mcmc_step_{tag}/x"], out[f"fused/mcmc_step_{tag}/px"] = xn, px
        out[f"fused/mcmc_step_{tag}/action"], out[f"fused/mcmc_step_{tag}/dq"] = obs["action"], dq
        inj = dyn.apply_transition(x, beta, momentum_f=v, momentum_b=v.flip(0), coin=_dev(rng.uniform(size=200)),
                                   u=_dev(rng.uniform(size=200)))
        for k, a in zip(("x_prop", "v_prop", "p", "x_out"), inj):
            out[f"fused/transition_{tag}/{k}"] = a
    # ConvNet3D plan
    dyn, x, v, rng = _gauge_dyn(la, 8, 8, 40, network_arch='conv3D')
    for k, a in zip(("x", "v", "sld", "p"), _trajectory(dyn, x, v, beta, _mixed_dirs(rng, 40))):
        out[f"fused/conv3D/{k}"] = a
    # taped run and its reverse (l2hmc_gauge_train_forward, not layered; fused_train.hip)
    dyn, x, v, rng = _gauge_dyn(la, 8, 8, 48)
    _train_steps(GaugeTrainer(dyn, lr_init=1e-3), x, beta, out, "fused/train8x8")


def _toy_dyn(la, dim, nodes, form, target="gmm", N=3, seed=42, hmc=False, use_temperature=False):
    import numpy as np
    np.random.seed(seed)
    if target == "gmm":
        mus = [np.eye(dim)[0], np.eye(dim)[1]]
        fn = la.GMM(mus, [0.1 * np.eye(dim)] * 2, [0.5, 0.5]).get_energy_function()
    elif target == "gmm3":          # K = 3: more components than TargetRegs holds, so energy_grad from LDS
        mus = [np.eye(dim)[0], np.eye(dim)[1], -np.eye(dim)[0]]
        fn = la.GMM(mus, [0.1 * np.eye(dim)] * 3, [0.5, 0.25, 0.25]).get_energy_function()
    elif target == "funnel":
        fn = la.GaussianFunnel(dim).get_energy_function()
    else:
        fn = la.RoughWell(dim, 0.1).get_energy_function()
    dyn = la.Dynamics(dim, fn, trajectory_length=N, eps=0.1, hmc=hmc, use_temperature=use_temperature,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=nodes))
    dyn.first_layer_form = form
    assert not dyn.layered
    return dyn


def _toy_more(la, out):
    """the paths the cases below leave out: plain-HMC runs, tempered runs, the hmc plan, K = 3, the analytic kinds above
    x_dim 2, training above x_dim 2 / 10 nodes.  3 leapfrog steps, 3 MCMC steps."""
    import numpy as np
    import torch
    from l2hmc_amd.dynamics_sampler import DynamicsSampler
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    from l2hmc_amd.sampler import propose
    rng = np.random.default_rng(11)

    def keep(name, run):
        out[f"{name}/px"], out[f"{name}/samples"], out[f"{name}/x"] = run["px"], run["samples"], run["samples_out"]

    # run_hmc at 70 chains: one full 64-thread workgroup and a part-full one
    B = 70
    sched = np.linspace(2.0, 1.0, 3)
    for dim, target in ((2, "gmm"), (2, "gmm3"), (2, "rough"), (5, "funnel")):
        smp = DynamicsSampler(_toy_dyn(la, dim, 10, 0, target, hmc=True, use_temperature=True))
        x = _dev(rng.normal(0, 0.8, (B, dim)))
        ladder = np.linspace(1.0, 3.0, B)[None, :]
        keep(f"toy/run_hmc/{target}_d{dim}/plain", smp.run_hmc(3, x=x))
        keep(f"toy/run_hmc/{target}_d{dim}/schedule", smp.run_hmc(3, x=x, temperature=sched))
        keep(f"toy/run_hmc/{target}_d{dim}/ladder", smp.run_hmc(3, x=x, temperature=ladder))
        keep(f"toy/run_hmc/{target}_d{dim}/eps_chain", smp.run_hmc(3, x=x, eps=np.linspace(0.05, 0.15, B)))
    # run with a schedule and with a ladder, 40 chains
    B = 40
    ladder = np.linspace(1.0, 3.0, B)[None, :]
    for dim, nodes in ((2, 10), (5, 64)):
        for form in (1, 2, 3):
            smp = DynamicsSampler(_toy_dyn(la, dim, nodes, form, use_temperature=True))
            x = _dev(rng.normal(0, 0.8, (B, dim)))
            keep(f"toy/run_tempered/d{dim}_n{nodes}_form{form}/schedule", smp.run(3, x=x, temperature=sched))
            keep(f"toy/run_tempered/d{dim}_n{nodes}_form{form}/ladder", smp.run(3, x=x, temperature=ladder))
    # the P.hmc path of small_traj_mfma_kernel
    dyn = _toy_dyn(la, 2, 10, 0, hmc=True)
    x, v = _dev(rng.normal(0, 0.8, (B, 2))), _dev(rng.standard_normal((B, 2)))
    for tag, res in (("fwd", dyn.forward(x, init_v=v, log_jac=True)), ("bwd", dyn.backward(x, init_v=v, log_jac=True)),
                     ("fwd_p", dyn.forward(x, init_v=v))):
        for k, a in zip(("x", "v", "third"), res):
            out[f"toy/hmc_plan/{tag}/{k}"] = a
    Lx, _, px, outs = propose(x, dyn, do_mh_step=True)
    out["toy/hmc_plan/propose/Lx"], out["toy/hmc_plan/propose/px"], out["toy/hmc_plan/propose/out"] = Lx, px, outs[0]
    # run on the three-component mixture
    keep("toy/run/gmm3_d2", DynamicsSampler(_toy_dyn(la, 2, 10, 0, "gmm3")).run(3, x=x))
    # training: x_dim 5 / 64 nodes on the mixture (2 leapfrog steps: the tape fits the LDS), the AN instance on the rough well
    for dim, nodes, target, N in ((5, 64, "gmm", 2), (2, 10, "rough", 3)):
        name = f"toy/train/{target}_d{dim}_n{nodes}"
        x = _dev(rng.normal(0, 0.8, (B, dim)))
        tr = DynamicsTrainer(_toy_dyn(la, dim, nodes, 0, target, N=N), scale=0.1)
        res = tr.train_step(x)
        for k, a in zip(("loss", "x_out", "px"), res):
            out[f"{name}/train_step/{k}"] = a
        out[f"{name}/train_step/grads"] = tr.grads.clone()
        dyn = _toy_dyn(la, dim, nodes, 0, target, N=N)
        for t in dyn.variables:
            t.requires_grad_()
        xg, vg = x.clone().requires_grad_(), _dev(rng.standard_normal((B, dim))).requires_grad_()
        for tag, fn in (("fwd", dyn.forward), ("bwd", dyn.backward)):
            X, V, lj = fn(xg, init_v=vg, log_jac=True)
            (X.sum() + 0.5 * (V * V).sum() + 0.25 * lj.sum()).backward()
            for i, t in enumerate([xg, vg, *dyn.variables]):
                if t.grad is not None:
                    out[f"{name}/vjp/{tag}/grad{i}"] = t.grad.clone()
                    t.grad = None


def group_toy(la, out):
    """one-launch toy kernels: 40 chains (a 16-row group part full), 3 leapfrog steps."""
    import numpy as np
    from l2hmc_amd.dynamics_sampler import DynamicsSampler
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    from l2hmc_amd.sampler import propose
    B = 40
    shapes = [(2, 10, "gmm"), (2, 50, "gmm"), (5, 64, "gmm"), (2, 10, "rough")]
    for dim, nodes, target in shapes:
        for form in (1, 2, 3):
            name = f"toy/{target}_d{dim}_n{nodes}_form{form}"
            dyn = _toy_dyn(la, dim, nodes, form, target)
            rng = np.random.default_rng(3)
            x, v = _dev(rng.normal(0, 0.8, (B, dim))), _dev(rng.standard_normal((B, dim)))
            for tag, res in (("fwd", dyn.forward(x, init_v=v, log_jac=True)), ("bwd", dyn.backward(x, init_v=v, log_jac=True)),
                             ("fwd_p", dyn.forward(x, init_v=v))):
                for k, a in zip(("x", "v", "third"), res):
                    out[f"{name}/trajectory/{tag}/{k}"] = a
            Lx, _, px, outs = propose(x, dyn, do_mh_step=True)
            out[f"{name}/propose/Lx"], out[f"{name}/propose/px"], out[f"{name}/propose/out"] = Lx, px, outs[0]
            run = DynamicsSampler(dyn).run(3, x=x)
            out[f"{name}/run/px"], out[f"{name}/run/samples"] = run["px"], run["samples"]
    # l2hmc_small_train_step and l2hmc_small_vjp at x_dim 2 / 10 nodes / 40 chains
    dyn = _toy_dyn(la, 2, 10, 0)
    tr = DynamicsTrainer(dyn, scale=0.1)
    rng = np.random.default_rng(3)
    x = _dev(rng.normal(0, 0.8, (B, 2)))
    for i in range(2):
        res = tr.train_step(x)
        for k, a in zip(("loss", "x_out", "px"), res):
            out[f"toy/train_step/step{i}/{k}"] = a
        out[f"toy/train_step/step{i}/grads"] = tr.grads.clone()
        x = res[1]
    dyn = _toy_dyn(la, 2, 10, 0)
    for t in dyn.variables:
        t.requires_grad_()
    x, v = _dev(rng.normal(0, 0.8, (B, 2))).requires_grad_(), _dev(rng.standard_normal((B, 2))).requires_grad_()
    for tag, fn in (("fwd", dyn.forward), ("bwd", dyn.backward)):
        X, V, lj = fn(x, init_v=v, log_jac=True)
        (X.sum() + 0.5 * (V * V).sum() + 0.25 * lj.sum()).backward()
        for i, t in enumerate([x, v, *dyn.variables]):
            if t.grad is not None:
                out[f"toy/vjp/{tag}/grad{i}"] = t.grad.clone()
                t.grad = None
    _toy_more(la, out)


# ---- timing cases: name -> builder of a callable that runs one call --------------------------------------------
def time_cases(la):
    """The training steps at the shapes of tools/train_configs.py (cfg 3 / 4 / 5: whole-trajectory tape + reverse,
    ConvNet3D, tiled layer by layer) and of tools/train_step_bits.py (ConvNet3D 8 x 8, layered walk, both toy trainers),
    the toy trainer at x_dim 8 / 64 nodes, and 10-LF trajectories at the batches that select the sub-tile forms, the
    32-row form and the ConvNet3D plan (tools/perf_configs.py's cfg-3 networks)."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(HERE, "tools"))
    import bench
    import train_step_bits as tsb
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    from l2hmc_amd.gauge_trainer import GaugeTrainer

    def train_cfg(cfg):
        c = bench.CONFIGS[cfg]
        dyn = bench.build_gauge(cfg, c["per_gpu"])
        x = torch.rand(c["per_gpu"], 2 * c["L"] ** 2, device="cuda") * (2 * np.pi)
        tr = GaugeTrainer(dyn, lr_init=1e-5)
        return lambda: tr.train_step(x, c["beta"])

    def tsb_case(build):
        tr, step = build()
        return lambda: step(0)

    def toy8():
        np.random.seed(42)
        fn = la.GMM([np.eye(8)[0], np.eye(8)[1]], [0.1 * np.eye(8)] * 2, [0.5, 0.5]).get_energy_function()
        dyn = la.Dynamics(8, fn, trajectory_length=4, eps=0.1,       # (the tape of a longer one does not fit the LDS)
                          net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=64))
        tr = DynamicsTrainer(dyn, scale=0.1)
        x = _dev(np.random.default_rng(3).normal(0, 0.8, (512, 8)))
        return lambda: tr.train_step(x)

    def traj(B, arch=None):
        dyn = bench.build_gauge(3, B, arch=arch)
        rng = np.random.default_rng(7)
        x, v = _dev(rng.uniform(0, 2 * np.pi, (B, 128))), _dev(rng.standard_normal((B, 128)))
        dirs = _mixed_dirs(rng, B)
        return lambda: _trajectory(dyn, x, v, 2.0, dirs)

    cases = {f"train_step cfg {c} (tools/train_configs.py)": (lambda c=c: train_cfg(c)) for c in (3, 4, 5)}
    cases.update({f"train_step {k}": (lambda b=b: tsb_case(b)) for k, b in tsb.time_cases(la).items() if "cfg-3" not in k})
    cases["train_step toy one-launch x_dim 8 / 64 nodes, 512 chains, 4 LF"] = toy8
    forms = _form_rows()
    for form in (4, 8, 12, 32):
        B = forms[form] + 3 if form != 32 else 2 * (forms[16] + 3)      # full tiles: 4, 8, 12 rows on every CU; two rounds
        cases[f"trajectory 8x8 GenericNet 10 LF, {B} rows ({form}-row form)"] = (lambda B=B: traj(B))
    cases["trajectory 8x8 ConvNet3D 10 LF, 2048 rows"] = lambda: traj(2048, "conv3D")
    return cases


GROUPS = {"ops": (group_ops, 120), "layered": (group_layered, 240), "fused": (group_fused, 300), "toy": (group_toy, 300)}


# ---- modes ------------------------------------------------------------------------------------------------------
def build(parent, outdir):
    """The parent's sources with this tree's compiler flags -> OUT_DIR (objects in OUT_DIR/obj)."""
    from concurrent.futures import ThreadPoolExecutor
    from l2hmc_amd import build as B
    lib = os.path.join(outdir, PARENT_LIB)
    if os.path.exists(lib):
        print("build: found", lib)
        return lib
    obj = os.path.join(outdir, "obj")
    os.makedirs(obj, exist_ok=True)
    hipcc, csrc = B._hipcc(), os.path.join(os.path.abspath(parent), "l2hmc_amd", "csrc")
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    objs = [os.path.join(obj, s.replace(".hip", ".o")) for s in srcs]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(lambda so: subprocess.run([hipcc, *B.FLAGS, "-c", os.path.join(csrc, so[0]), "-o", so[1]], check=True),
                    zip(srcs, objs)))
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", lib], check=True)
    print("build:", lib)
    return lib


def dump(group, path):
    import numpy as np
    import torch
    import l2hmc_amd as la
    from l2hmc_amd import _lib
    out = {}
    GROUPS[group][0](la, out)
    torch.cuda.synchronize()
    arrays = {k: (a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)) for k, a in out.items()}
    np.savez(path, **arrays)
    print(f"dump {group}: {len(arrays)} arrays with {_lib.LIB_PATH} -> {path}", flush=True)


def time_calls(path, only=""):
    """`only`: substring of the names of the cases to time (all when empty)."""
    import json
    import time
    import torch
    import l2hmc_amd as la
    from l2hmc_amd import _lib
    res = {}
    for name, build in time_cases(la).items():
        if only not in name:
            continue
        call = build()
        for _ in range(2):
            call()
        iters = 1
        while True:                      # at least a second of calls per figure
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                call()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= 1.0:
                break
            iters = int(1.2 * iters / dt) + 1
        res[name] = 1e3 * dt / iters
        print(f"{name}: {res[name]:.4f} ms ({iters} calls, {_lib.LIB_PATH})", flush=True)
        del call
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        json.dump(res, f)


def timing(parent, outdir, only=""):
    import json
    import statistics
    os.makedirs(outdir, exist_ok=True)
    libs = {"parent": build(parent, outdir), "new": os.path.join(HERE, "l2hmc_amd", "libl2hmc_hip.so")}
    rounds = {"parent": [], "new": []}
    for r in range(3):
        for who, lib in libs.items():
            path = os.path.join(outdir, f"time_{who}_{r}.json")
            rc = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "time", path, only],
                                env=dict(os.environ, L2HMC_LIB_PATH=lib)).returncode
            if rc != 0:
                sys.exit(f"timing: round {r} ({who}) ended with status {rc}; nothing more is started")
            with open(path) as f:
                rounds[who].append(json.load(f))
    print(f"{'case (ms per call)':<76} {'parent rounds':<30} {'new rounds':<30} spread    med P    med N  ok")
    bad = 0
    for name in rounds["parent"][0]:
        p, n = ([r[name] for r in rounds[w]] for w in ("parent", "new"))
        spread, mp, mn = max(p) - min(p), statistics.median(p), statistics.median(n)
        bad += mn > mp + spread
        print(f"{name:<76} {' '.join(f'{v:.4f}' for v in p):<30} {' '.join(f'{v:.4f}' for v in n):<30} {spread:7.4f} "
              f"{mp:8.4f} {mn:8.4f}  {'yes' if mn <= mp + spread else 'NO'}")
    return 1 if bad else 0


def compare(a, b):
    import numpy as np
    with np.load(a) as fa, np.load(b) as fb:
        if sorted(fa.files) != sorted(fb.files):
            sys.exit(f"compare: the dumps hold different arrays: {sorted(set(fa.files) ^ set(fb.files))[:10]}")
        bad = [k for k in fa.files if not (fa[k].dtype == fb[k].dtype and np.array_equal(fa[k], fb[k]))]
        nonfinite = [k for k in fa.files if not np.isfinite(fa[k]).all()]
        for k in bad[:20]:
            print("  differs:", k)
        for k in nonfinite[:20]:
            print("  not finite:", k)
        return len(fa.files), len(bad), len(nonfinite)


def run(parent, outdir, only=None):
    os.makedirs(outdir, exist_ok=True)
    libs = {"parent": build(parent, outdir), "new": os.path.join(HERE, "l2hmc_amd", "libl2hmc_hip.so")}
    total = [0, 0, 0]
    for group, (_, limit) in GROUPS.items():
        if only and group != only:
            continue
        for who, lib in libs.items():
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "dump", group,
                                 os.path.join(outdir, f"bits_{group}_{who}.npz")],
                                env=dict(os.environ, L2HMC_LIB_PATH=lib)).returncode
            if rc != 0:
                sys.exit(f"run: dump {group} ({who}) ended with status {rc}; nothing more is started")
        res = compare(os.path.join(outdir, f"bits_{group}_parent.npz"), os.path.join(outdir, f"bits_{group}_new.npz"))
        print(f"compare {group}: {res[0]} arrays compared, {res[1]} differ, {res[2]} hold a non-finite value", flush=True)
        total = [t + r for t, r in zip(total, res)]
    print(f"lf_update_bits: {total[0]} arrays compared, {total[1]} differ, {total[2]} hold a non-finite value")
    return 1 if total[1] or total[2] else 0


if __name__ == "__main__":
    mode, args = (sys.argv[1], sys.argv[2:]) if len(sys.argv) > 1 else ("", [])
    if mode == "build" and len(args) == 2:
        build(*args)
    elif mode == "dump" and len(args) == 2:
        dump(*args)
    elif mode == "run" and len(args) in (2, 3):
        sys.exit(run(*args))
    elif mode == "time" and len(args) in (1, 2):
        time_calls(*args)
    elif mode == "timing" and len(args) in (2, 3):
        sys.exit(timing(*args))
    else:
        sys.exit(__doc__)
