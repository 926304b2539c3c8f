"""Cases, inputs and float64 references for the one-launch toy-target kernels at the limits include/l2hmc_hip.h states
(x_dim <= 8, <= 8 mixture components, <= 64 hidden units), in one place for tests/test_toy_limits_host.py (which
validates them without a GPU) and tests/test_gpu_toy_limits.py (which compares the kernels with them).

Targets.  `target(dim, K, kind)` builds the oracle object and the library object from the same arrays: means uniform in
[-1, 1], every covariance Q diag(ev) Q^T with Q a random orthogonal matrix and ev uniform in [0.05, 0.3] (full, not
diagonal), unequal weights.  kind "gaussian" is the Gaussian class (K = 1), kind "mixture" the GMM class, K = 1 included.

Everything a case hands out holds float32-representable numbers (start states, momenta, weights), so the float64
oracle, the float32 oracle and the kernels start from the same numbers.

Bars.  `fp32_equivalent` and `p_bar` restate `assert_fp32_equivalent` and the accept-probability rule of
tests/test_gpu_parity.py with its constants; they also return the figures so that a caller can print them.

A seed in a table below is one at which the input conditions of tests/test_toy_limits_host.py hold (for `vjp_seed`,
the seed of the cotangents of the l2hmc_small_vjp test: the condition on `cancellation`)."""
import collections
import copy
import functools

import numpy as np
import torch

from oracle import dynamics as od
from oracle.torch_ref import TorchDynamicsModel
from tests import helpers as H
from tests.test_gpu_parity import MAX_RATIO, P_RATIO, Q999_RATIO, RMS_RATIO, TOL_OP, TOL_P, rmserr

TOL_G = 2e-4
EPS = 0.1
MH_MARGIN = 1e-4          # chains with |p - u| within it are left out of the MH comparison; none may be
RELU_MARGIN = 1e-5        # no float64 hidden pre-activation of a training case lies this close to zero
MIN_MARGIN = 1e-4         # ... and no H0 - H1 + logdet this close to zero, where p = exp(min(., 0)) changes branch
SEES = 100.0              # a perturbed oracle differs from the oracle by this many times the bar of an output

SamplingCase = collections.namedtuple("SamplingCase", "dim K kind H N regime seed")
TrainCase = collections.namedtuple("TrainCase", "dim K kind H N B regime temperature seed vjp_seed")

G, M = "gaussian", "mixture"
# A covering set: dims 4, 5, 7, 8, each with a width of each instance class of small_launch (H <= 16, 17..50, 51..64);
# K = 1 of both kinds, 4 and 8; H = 1, 16, 17, 50, 51, 63, 64; (8, 8, 64) and (8, 8, 1); both weight regimes.
SAMPLING_CASES = [
    SamplingCase(4, 4, M, 16, 4, "stress", 1),
    SamplingCase(4, 1, G, 17, 5, "mild", 1),
    SamplingCase(4, 8, M, 63, 4, "stress", 1),
    SamplingCase(5, 1, M, 1, 4, "stress", 1),
    SamplingCase(5, 8, M, 17, 4, "stress", 1),
    SamplingCase(5, 4, M, 51, 3, "mild", 1),
    SamplingCase(7, 8, M, 16, 3, "mild", 1),
    SamplingCase(7, 4, M, 50, 4, "stress", 1),
    SamplingCase(7, 1, G, 51, 4, "stress", 1),
    SamplingCase(8, 8, M, 1, 4, "stress", 1),
    SamplingCase(8, 1, M, 50, 5, "stress", 1),
    SamplingCase(8, 1, G, 64, 4, "mild", 1),
    SamplingCase(8, 8, M, 64, 4, "stress", 1),
]
SAMPLING_BATCHES = (37, 1)          # three 16-row groups with the last ragged; one chain
PIECEWISE_CASES = [c for c in SAMPLING_CASES if (c.dim, c.K, c.H) in ((5, 8, 17), (8, 8, 64), (7, 1, 51))]
LAYERED_CASES = [c for c in SAMPLING_CASES if (c.dim, c.K, c.H) in ((8, 8, 64), (5, 8, 17))]

TRAIN_CASES = [
    TrainCase(4, 4, M, 16, 4, 21, "stress", 1.0, 4, 1),
    TrainCase(5, 8, M, 17, 3, 9, "stress", 1.0, 1, 0),
    TrainCase(7, 1, G, 50, 4, 19, "stress", 1.0, 14, 0),
    TrainCase(8, 1, G, 51, 3, 17, "mild", 1.0, 2, 0),
    TrainCase(8, 8, M, 64, 3, 37, "stress", 1.0, 6, 1),
    TrainCase(8, 4, M, 1, 3, 9, "stress", 1.0, 3, 5),
    TrainCase(4, 8, M, 64, 5, 16, "mild", 2.5, 18, 0),
]

TARGET_CASES = [(4, 4, M), (5, 8, M), (7, 1, G), (8, 8, M), (8, 1, M)]
TARGET_ROWS = (1, 255, 257)
TARGET_TEMPERATURES = (1.0, 2.5)


def case_id(c):
    tail = f"-T{c.temperature}" if hasattr(c, "temperature") and c.temperature != 1.0 else ""
    return f"d{c.dim}-K{c.K}{c.kind[0]}-H{c.H}-N{c.N}-{c.regime}{tail}"


def forms(H_nodes):
    """The first_layer_form values a width allows: 3 (two waves per group) exists in the 64-unit instances only."""
    return (1, 2, 3) if H_nodes > 16 else (1, 2)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------- builders
@functools.lru_cache(maxsize=None)
def target_arrays(dim, K, seed=0):
    rng = np.random.default_rng(1000 * dim + 10 * K + seed)
    mus = [rng.uniform(-1., 1., dim) for _ in range(K)]
    covs = []
    for _ in range(K):
        Q, R = np.linalg.qr(rng.standard_normal((dim, dim)))
        Q = Q * np.sign(np.diag(R))
        covs.append(Q @ np.diag(rng.uniform(0.05, 0.3, dim)) @ Q.T)
    pis = rng.uniform(0.5, 1.5, K)
    return mus, covs, pis / pis.sum()


def target(dim, K, kind, seed=0):
    """-> (oracle.dynamics object, l2hmc_amd object) from the same arrays."""
    import l2hmc_amd as la
    mus, covs, pis = target_arrays(dim, K, seed)
    if kind == G:
        assert K == 1
        return od.Gaussian(mus[0], covs[0]), la.Gaussian(mus[0], covs[0])
    return od.GMM(mus, covs, list(pis)), la.GMM(list(mus), list(covs), list(pis))


def oracle_packing(tgt_o):
    """(mu [K, dim], precision [K, dim, dim], log_const [K]) of an oracle target, as its energy uses them."""
    if isinstance(tgt_o, od.Gaussian):
        return (tgt_o.mu.astype('float32')[None], tgt_o.i_sigma.astype('float32')[None], np.zeros(1, np.float32))
    return (np.stack([m.astype('float32') for m in tgt_o.mus]), np.stack(tgt_o.i_sigmas),
            np.stack([np.log(c) for c in tgt_o.constants]))


def nets(dim, H_nodes, regime, seed):
    xp, vp = H.mlp_weights(dim, H_nodes, seed=106 + seed, regime=regime)
    return {k: f32(v) for k, v in xp.items()}, {k: f32(v) for k, v in vp.items()}


def masks(N, dim, seed):
    return od.make_masks(N, dim, np.random.RandomState(5 + seed))


def library_dynamics(la, c, tgt, xp, vp, m, temperature=1.0):
    dyn = la.Dynamics(c.dim, tgt.get_energy_function(), trajectory_length=c.N, eps=EPS,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=c.H),
                      use_temperature=True)
    dyn.temperature = temperature
    dyn.set_masks(m)
    dyn.XNet.load_state(xp)
    dyn.VNet.load_state(vp)
    return dyn


# --------------------------------------------------------------------------------------------------------- bars
def relerr(got, want):
    return H.relerr(got, want)


def fp32_equivalent(got, want64, want32):
    """-> (failures, figures): `assert_fp32_equivalent` of tests/test_gpu_parity.py, figures handed back."""
    got, want64, want32 = (np.asarray(a, dtype=np.float64) for a in (got, want64, want32))
    emax, imax = H.relerr(got, want64), H.relerr(want32, want64)
    erms, irms = rmserr(got, want64), rmserr(want32, want64)
    fails = []
    if not emax < max(TOL_OP, MAX_RATIO * imax):
        fails.append(f"max err {emax:.2e} vs intrinsic fp32 {imax:.2e}")
    if not erms < max(TOL_OP / 3, RMS_RATIO * irms):
        fails.append(f"rms err {erms:.2e} vs intrinsic fp32 {irms:.2e}")
    if np.size(want64) >= 4000:
        scale = max(1.0, np.max(np.abs(want64)))
        eq = np.quantile(np.abs(got - want64), 0.999) / scale
        iq = np.quantile(np.abs(want32 - want64), 0.999) / scale
        if not eq < max(TOL_OP / 2, Q999_RATIO * iq):
            fails.append(f"99.9 % quantile {eq:.2e} vs intrinsic fp32 {iq:.2e}")
    return fails, dict(max=emax, rms=erms, fp32_max=imax, fp32_rms=irms)


def max_bar(want64, want32):
    """The bar `fp32_equivalent` puts on the max error of an output."""
    return max(TOL_OP, MAX_RATIO * H.relerr(want32, want64))


def p_bar(want64, want32):
    """max(TOL_P, P_RATIO * the fp32 oracle's own error): the accept-probability rule of tests/test_gpu_parity.py."""
    return max(TOL_P, P_RATIO * float(np.abs(np.asarray(want32, dtype=np.float64) - want64).max()))


P_OUTPUTS = ("pf", "pb", "px", "p")


def check_output(name, got, want64, want32):
    """-> (failures, figures) of one sampling output under the bar its kind takes."""
    if name in P_OUTPUTS:
        got, want64, want32 = (np.asarray(a, dtype=np.float64) for a in (got, want64, want32))
        err, bar = float(np.abs(got - want64).max()), p_bar(want64, want32)
        fig = dict(max=err, rms=float(np.sqrt(np.mean((got - want64) ** 2))),
                   fp32_max=float(np.abs(want32 - want64).max()), fp32_rms=float(np.sqrt(np.mean((want32 - want64) ** 2))))
        return ([] if err < bar else [f"abs err {err:.2e} vs bar {bar:.2e}"]), fig
    return fp32_equivalent(got, want64, want32)


def report(case, B, what, name, fig):
    """One line of profiles/toy_limits_parity.txt."""
    return (f"toy_limits {case:<28s} B={B:<3d} {what:<10s} {name:<6s} max {fig['max']:.2e} rms {fig['rms']:.2e}"
            f" | fp32 oracle max {fig['fp32_max']:.2e} rms {fig['fp32_rms']:.2e}")


# ----------------------------------------------------------------------------------------------------- sampling
@functools.lru_cache(maxsize=None)
def sampling_inputs(c, B):
    """-> dict: start states drawn from the target, both momenta, direction bits (1 = forward), MH uniforms."""
    tgt_o, _ = target(c.dim, c.K, c.kind)
    rng = np.random.default_rng(100 * c.seed + B)
    x = f32(tgt_o.get_samples(B, rng))
    v0f, v0b = f32(rng.standard_normal((B, c.dim))), f32(rng.standard_normal((B, c.dim)))
    bits, u = rng.integers(0, 2, B).astype(np.float64), f32(rng.uniform(size=B))
    if B > 1:
        bits[:2] = (1., 0.)              # both directions in every batch of more than one chain
    return dict(x=x, v0f=v0f, v0b=v0b, bits=bits, u=u)


def _perturbed_target(tgt_o, how):
    t = copy.copy(tgt_o)
    if how == "drop_component":                       # component K - 1 is not there (the weights of the rest stay)
        t.mus, t.sigmas = t.mus[:-1], t.sigmas[:-1]
        t.i_sigmas, t.constants = t.i_sigmas[:-1], t.constants[:-1]
        t.nb_mixtures -= 1
        return t
    dim = (t.mu if isinstance(t, od.Gaussian) else t.mus[0]).shape[0]          # precision entry [dim-1][dim-2] is zero
    if isinstance(t, od.Gaussian):
        t.i_sigma = t.i_sigma.copy()
        t.i_sigma[dim - 1, dim - 2] = 0.
    else:
        t.i_sigmas = [s.copy() for s in t.i_sigmas]
        t.i_sigmas[0][dim - 1, dim - 2] = 0.
    return t


def _without_last_unit(p):
    """Hidden unit H - 1 of both hidden layers gives 0 whatever comes in."""
    p = {k: v.copy() for k, v in p.items()}
    for k in ("embed_1", "embed_2", "embed_3", "linear_1"):
        p[k + "/W"][:, -1] = 0.
        p[k + "/b"][-1] = 0.
    return p


PERTURBATIONS = ("last_unit", "last_component_or_precision_entry", "last_coordinate")


def sampling_outputs(c, B, dtype=np.float64, perturb=None):
    """Every output the GPU test compares, from DynamicsOracle in `dtype`.  `perturb` (host test): the oracle with
    hidden unit H - 1 zeroed in both nets; with component K - 1 removed (K > 1) or precision entry [dim-1][dim-2]
    zeroed (K = 1); with coordinate dim - 1 of the start state held at zero."""
    tgt_o, _ = target(c.dim, c.K, c.kind)
    xp, vp = nets(c.dim, c.H, c.regime, c.seed)
    i = sampling_inputs(c, B)
    x = i["x"]
    if perturb == "last_unit":
        xp, vp = _without_last_unit(xp), _without_last_unit(vp)
    elif perturb == "last_component_or_precision_entry":
        tgt_o = _perturbed_target(tgt_o, "drop_component" if c.K > 1 else "precision_entry")
    elif perturb == "last_coordinate":
        x = x.copy()
        x[:, c.dim - 1] = 0.
    else:
        assert perturb is None
    orc = od.DynamicsOracle(c.dim, tgt_o, c.N, EPS, masks(c.N, c.dim, c.seed), xp, vp, dtype=dtype)
    out = {}
    out["Xf"], out["Vf"], out["pf"] = orc.forward(x, i["v0f"])
    out["Xb"], out["Vb"], out["pb"] = orc.backward(x, i["v0b"])
    out["ljf"], out["ljb"] = orc.forward(x, i["v0f"], log_jac=True)[2], orc.backward(x, i["v0b"], log_jac=True)[2]
    Lx, _, px, outs, Lv = od.propose(x, orc, i["v0f"], i["v0b"], i["bits"], u=i["u"].astype(dtype), do_mh_step=True)
    out.update(Lx=Lx, Lv=Lv, px=px, x_out=outs[0])
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def sampling_reference(c, B):
    """-> (float64 outputs, float32-oracle outputs), computed once and shared; callers leave them unchanged."""
    return sampling_outputs(c, B), sampling_outputs(c, B, dtype=np.float32)


def mh_safe(c, B):
    """Chains whose accept decision is not within rounding of a tie in float64."""
    w64, _ = sampling_reference(c, B)
    return np.abs(w64["px"] - sampling_inputs(c, B)["u"]) > MH_MARGIN


# ----------------------------------------------------------------------------------------------------- training
class MarginModel(TorchDynamicsModel):
    """TorchDynamicsModel that also notes, per row, the smallest |hidden pre-activation| its nets have seen (both hidden
    layers of utils/network.py:89-114, restated) since `reset_margin`."""

    def reset_margin(self, rows):
        self.margin = np.full(rows, np.inf)

    def _net(self, p, inputs):
        a, b, t = inputs
        with torch.no_grad():
            h1 = (a @ p['embed_1/W'] + p['embed_1/b']) + (b @ p['embed_2/W'] + p['embed_2/b']) \
                + (t @ p['embed_3/W'] + p['embed_3/b'])
            h2 = torch.relu(h1) @ p['linear_1/W'] + p['linear_1/b']
            m = torch.minimum(h1.abs().min(dim=1).values, h2.abs().min(dim=1).values).numpy()
            if getattr(self, "margin", None) is not None and m.shape == self.margin.shape:
                self.margin = np.minimum(self.margin, m)
        return super()._net(p, inputs)


def t64(a):
    return torch.tensor(np.asarray(a, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def train_inputs(c):
    """-> dict: x from the target, z normal, and (v forward, v backward, direction bits, uniforms) for each."""
    tgt_o, _ = target(c.dim, c.K, c.kind)
    rng = np.random.default_rng(100 * c.seed + 11)
    x = f32(tgt_o.get_samples(c.B, rng))
    z = f32(rng.standard_normal((c.B, c.dim)))

    def mk():
        return (f32(rng.standard_normal((c.B, c.dim))), f32(rng.standard_normal((c.B, c.dim))),
                rng.integers(0, 2, c.B).astype(np.float64), f32(rng.uniform(size=c.B)))
    return dict(x=x, z=z, dx=mk(), dz=mk())


def train_model(c, cls=TorchDynamicsModel):
    """A fresh float64 model of a training case (its leaves collect gradients, so nobody shares it)."""
    tgt_o, _ = target(c.dim, c.K, c.kind)
    xp, vp = nets(c.dim, c.H, c.regime, c.seed)
    return cls(tgt_o, c.N, EPS, masks(c.N, c.dim, c.seed), xp, vp, temperature=c.temperature)


def train_margins(c):
    """-> (relu margin, min margin): over the x and the z chains in the direction each one's bit picks, the smallest
    |hidden pre-activation| of either net and the smallest |H0 - H1 + logdet| of the float64 model."""
    tm = train_model(c, MarginModel)
    i = train_inputs(c)
    relu, arg = np.inf, np.inf
    with torch.no_grad():
        for start, d in ((i["x"], i["dx"]), (i["z"], i["dz"])):
            for bwd, v0 in ((False, d[0]), (True, d[1])):
                rows = d[2] < 0.5 if bwd else d[2] > 0.5
                if not rows.any():
                    continue
                x0, v = t64(start[rows]), t64(v0[rows])
                tm.reset_margin(int(rows.sum()))
                xN, vN, _, ld = tm.trajectory(x0, v, None, bwd)
                relu = min(relu, float(tm.margin.min()))
                h0 = tm._energy(x0, None) + 0.5 * (v ** 2).sum(1)
                h1 = tm._energy(xN, None) + 0.5 * (vN ** 2).sum(1)
                arg = min(arg, float((h0 - h1 + ld).abs().min()))
    return relu, arg


def train_reference(c):
    """-> (model with gradients, loss, proposals [2B, dim], p [2B]) of mog_model.py:336-355 in float64."""
    tm = train_model(c)
    i = train_inputs(c)
    loss, Lx, px, Lz, pz = tm.mog_loss(t64(i["x"]), t64(i["z"]), tuple(map(t64, i["dx"])), tuple(map(t64, i["dz"])), 0.1)
    loss.backward()
    return (tm, float(loss.detach()), np.concatenate([Lx.detach().numpy(), Lz.detach().numpy()]),
            np.concatenate([px.detach().numpy(), pz.detach().numpy()]))


def vjp_cotangents(c):
    """Cotangents of (x_out, v_out, logdet, p) for the l2hmc_small_vjp test: all four non-zero, float32 numbers."""
    x0, _, _ = train_rows(c)
    R, D = x0.shape
    rng = np.random.default_rng(23 + c.vjp_seed)
    return [f32(rng.standard_normal(s)) for s in ((R, D), (R, D), R, R)]


def vjp_reference(c):
    """-> (model, x0 leaf, v0 leaf, per-row functional [2B]) of the float64 trajectory of the stacked chains, each in
    its direction, contracted with `vjp_cotangents`.  Its sum is what l2hmc_small_vjp differentiates."""
    tm = train_model(c)
    x0, v0, dirs = train_rows(c)
    g = vjp_cotangents(c)
    x64, v64 = t64(x0).requires_grad_(), t64(v0).requires_grad_()
    fw = torch.tensor(dirs == 0)
    res = [tm.trajectory(x64, v64, None, bwd) for bwd in (False, True)]
    X, V, P, LD = (torch.where(fw[:, None] if res[0][j].dim() == 2 else fw, res[0][j], res[1][j]) for j in range(4))
    rows = (t64(g[0]) * X).sum(1) + (t64(g[1]) * V).sum(1) + t64(g[2]) * LD + t64(g[3]) * P
    return tm, x64, v64, rows


def mog_loss_rows(c):
    """-> (model, per-row terms [2B]) whose sum is the loss of mog_model.py:336-355."""
    tm = train_model(c)
    i = train_inputs(c)
    x, z = t64(i["x"]), t64(i["z"])
    Lx, px = tm.propose(x, *map(t64, i["dx"][:3]))
    Lz, pz = tm.propose(z, *map(t64, i["dz"][:3]))
    v = torch.cat([((x - Lx) ** 2).sum(1) * px, ((z - Lz) ** 2).sum(1) * pz]) + 1e-4
    return tm, (0.1 / v - v / 0.1) / c.B


CANCELLATION = 10.0


def cancellation(tm, rows):
    """-> {tensor: sum over chains of |the chain's share| / |the sum|, at the tensor's largest gradient entry}.
    The gradient tests measure a tensor's error against that entry.  A kernel sums the chains' shares in float32, each
    share good to some 1e-5 of itself; where the shares cancel, the sum's relative error grows by this factor, so a
    case whose factor exceeds CANCELLATION (which leaves TOL_G = 2e-4 at twice the expected error) tests the inputs'
    conditioning, not the kernel."""
    leaves = {"alpha": tm.alpha, **{f"xnet.{k}": v for k, v in tm.xnet.items()}, **{f"vnet.{k}": v for k, v in tm.vnet.items()}}
    # one batched reverse pass: gs[k][r] is chain r's share of leaf k's gradient
    gs = torch.autograd.grad(rows, list(leaves.values()), grad_outputs=torch.eye(rows.shape[0], dtype=rows.dtype),
                             is_grads_batched=True, allow_unused=True)
    tot = {k: g.sum(0) for k, g in zip(leaves, gs)}
    mag = {k: g.abs().sum(0) for k, g in zip(leaves, gs)}
    out = {}
    for k in leaves:
        j = int(tot[k].abs().argmax())
        out[k] = float(mag[k].reshape(-1)[j] / tot[k].abs().reshape(-1)[j])
    return out


def train_rows(c):
    """-> (x0, v0, dirs): the 2B stacked x and z chains as the training step runs them, each with the momentum of the
    direction its bit picks; dirs is 1 for a backward chain."""
    i = train_inputs(c)
    bits = np.concatenate([i["dx"][2], i["dz"][2]])
    x0 = np.concatenate([i["x"], i["z"]])
    v0 = np.where(bits[:, None] > 0.5, np.concatenate([i["dx"][0], i["dz"][0]]), np.concatenate([i["dx"][1], i["dz"][1]]))
    return x0, v0, (bits < 0.5).astype(np.int32)


@functools.lru_cache(maxsize=None)
def train_forward_reference(c):
    """-> (float64, float32) dicts x, v, logdet, p of the stacked chains from DynamicsOracle: the yardstick of the
    forward outputs a training entry hands out."""
    tgt_o, _ = target(c.dim, c.K, c.kind)
    xp, vp = nets(c.dim, c.H, c.regime, c.seed)
    x0, v0, dirs = train_rows(c)
    out = []
    for dtype in (np.float64, np.float32):
        orc = od.DynamicsOracle(c.dim, tgt_o, c.N, EPS, masks(c.N, c.dim, c.seed), xp, vp, temperature=c.temperature,
                                dtype=dtype)
        f, b = orc.forward(x0, v0), orc.backward(x0, v0)
        lf, lb = orc.forward(x0, v0, log_jac=True)[2], orc.backward(x0, v0, log_jac=True)[2]
        sel = dirs == 0
        out.append({k: np.asarray(np.where(sel[:, None] if a.ndim == 2 else sel, a, b_), dtype=np.float64)
                    for k, a, b_ in (("x", f[0], b[0]), ("v", f[1], b[1]), ("p", f[2], b[2]), ("logdet", lf, lb))})
    return tuple(out)


# ------------------------------------------------------------------------------------------- standalone target entries
@functools.lru_cache(maxsize=None)
def target_points(dim, K, kind, rows):
    """-> (x, u) float32: rows drawn from the target; the last few (where there is room) 3 sigma away from EVERY mean
    along the first mean's widest axis and beyond, so that one component dominates the logsumexp."""
    tgt_o, _ = target(dim, K, kind)
    mus, covs, _ = target_arrays(dim, K)
    rng = np.random.default_rng(rows + 7 * dim + K)
    x = tgt_o.get_samples(rows, rng)
    far = min(4, rows - 1)
    for j in range(far):
        k = j % K
        w, Q = np.linalg.eigh(covs[k])
        step = Q[:, -1] * np.sqrt(w[-1])
        s = 3.0
        pt = mus[k] + s * step
        while min(float((pt - m) @ np.linalg.inv(S) @ (pt - m)) for m, S in zip(mus, covs)) < 9.0:
            s += 0.5
            pt = mus[k] + s * step
        x[rows - 1 - j] = pt
    u = rng.standard_normal((rows, dim))
    return x.astype(np.float32), u.astype(np.float32)


def target_reference(dim, K, kind, rows, temperature):
    """-> (energy, gradient, Hessian . u) per row from float64 torch autograd (a double backward for the last)."""
    tgt_o, _ = target(dim, K, kind)
    tm = TorchDynamicsModel(tgt_o, 1, EPS, np.zeros((1, dim)), {}, {}, temperature=temperature)
    x, u = target_points(dim, K, kind, rows)
    X = torch.tensor(x.astype(np.float64), requires_grad=True)
    e = tm._energy(X, None)
    (g,) = torch.autograd.grad(e.sum(), X, create_graph=True)
    (hv,) = torch.autograd.grad(g, X, grad_outputs=torch.tensor(u.astype(np.float64)))
    return e.detach().numpy(), g.detach().numpy(), hv.detach().numpy()
