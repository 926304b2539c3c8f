"""Shared by the toy-target ladder-training tests (tests/test_gpu_small_train_ladder.py,
tests/test_small_train_ladder_host.py): the float64 reference of a training step on a ladder of temperatures, the fixed
assignment of temperatures to chains, and the cases with their inputs.  It mirrors tests/ladder_ref.py.

The reference is oracle/torch_ref.py's TorchDynamicsModel, unedited, with the two methods through which the temperature
enters overridden so that `temperature` may be a [B] tensor: chain i of the x batch and chain i of the z batch run at
temperature[i] (the model integrates each batch on its own, so a row of either is chain i).  With a scalar the overrides
are the parent's methods.  Its per-chain terms equal the unmodified oracle's run rung by rung on that rung's chains, and
its gradients the B_g / B-weighted sum of those runs (checked on the CPU in test_small_train_ladder_host.py).

Batches: a workgroup of the training kernel holds 16 chains, so B = 37 is 74 rows in five workgroups, the last ragged,
with a chain's x row and z row in different slots ((37 + i) % 16 != i % 16); B = 9 is the small batch and B = 16 fills
its workgroups exactly.

A seed of a gradient case below is one at which the input conditions of tests/toy_cases.py hold for the ladder (no hidden pre-activation
within RELU_MARGIN of 0, no H0 - H1 + logdet within MIN_MARGIN of 0, cancellation factors within CANCELLATION), checked
on the CPU in test_small_train_ladder_host.py: no row is left out of any comparison."""
import collections
import functools

import numpy as np
import torch

from oracle import dynamics as od
from oracle.torch_ref import TorchDynamicsModel
from tests import helpers as H
from tests.ladder_ref import rung_of
from tests.toy_cases import MarginModel, f32, t64

# 1.7 is not a float32 number on purpose: the plan's scalar and the ladder's entry must round alike
RUNGS = (1.0, 1.7, 2.5)
SCALE = 0.1

Case = collections.namedtuple("Case", "kind H N eps B regime seed layered")
# the float64 gradient cases (the mixture and the Gaussian; the analytic kinds have no float64 model here: they are held
# bit for bit to the scalar entry, which their own tests hold to float64)
MOG = Case("mog", 50, 5, 0.1, 37, "stress", 56, False)            # cfg 2 widths, five workgroups, the last ragged
SCG = Case("scg", 10, 5, 0.1, 21, "stress", 21, False)           # HP 16, Gaussian
MOG3_16 = Case("mog3", 12, 3, 0.1, 9, "mild", 0, False)          # HP 16, run-time dimension
MOG3_64 = Case("mog3", 50, 4, 0.1, 19, "stress", 24, False)      # HP 64, run-time dimension
MOG_16 = Case("mog", 50, 5, 0.1, 16, "stress", 1, False)         # exact fill: 32 rows, two full workgroups
GRADIENT_CASES = [MOG, SCG, MOG3_16, MOG3_64]
# the analytic instances (no float64 model)
ROUGH_WELL = Case("rough_well", 10, 3, 0.1, 9, "mild", 0, False)
FUNNEL = Case("funnel", 50, 3, 0.05, 16, "mild", 0, False)
ONE_LAUNCH_CASES = GRADIENT_CASES + [MOG_16, ROUGH_WELL, FUNNEL]
# the layered path: the mixture with `dyn.layered = True`, and a callable energy at x_dim 10
MOG_LAYERED = MOG._replace(layered=True)
QUARTIC = Case("quartic10", 20, 2, 0.05, 9, "mild", 0, True)
LAYERED_CASES = [MOG_LAYERED, QUARTIC]


def case_id(c):
    return f"{c.kind}-H{c.H}-N{c.N}-B{c.B}-{c.regime}{'-layered' if c.layered else ''}"


def ladder(B, rungs=RUNGS):
    """temperature [B] float64 holding float32 numbers: the three values laid on the chains by ladder_ref's fixed,
    non-periodic pattern."""
    return f32(np.asarray(rungs, dtype=np.float64))[rung_of(B)]


# ---------------------------------------------------------------------------------------------------- the reference
class LadderDynamicsModel(TorchDynamicsModel):
    """TorchDynamicsModel whose `temperature` may be a [B] tensor (one value per chain of the batch it is handed):
    energy and force of the parent at temperature 1, over the row's temperature."""

    def _on_ladder(self):
        return torch.is_tensor(self.temperature) and self.temperature.ndim == 1

    def _at_one(self, fn, x):
        t, self.temperature = self.temperature, 1.0
        try:
            return fn(x, None)
        finally:
            self.temperature = t

    def _energy(self, x, beta):
        if self._on_ladder():
            return self._at_one(super()._energy, x) / self.temperature
        return super()._energy(x, beta)

    def _force(self, x, beta):
        if self._on_ladder():
            return self._at_one(super()._force, x) / self.temperature[:, None]
        return super()._force(x, beta)


class _DummyGaussian:
    mu = np.zeros(1)
    i_sigma = np.eye(1)


class QuarticModel(TorchDynamicsModel):
    """E(x) = sum_d (x_d^2 - 1)^2 / 4 + 0.3 sum_d x_d x_{d+1} (periodic), float64: the callable energy of the layered
    case (tests/test_gpu_train_layered.py's, at x_dim 10)."""

    def __init__(self, _target, *a, **k):
        super().__init__(_DummyGaussian(), *a, **k)

    def _energy(self, x, beta):
        return (((x * x - 1.) ** 2).sum(1) / 4. + 0.3 * (x * torch.roll(x, -1, dims=1)).sum(1)) / self.temperature

    def _force(self, x, beta):
        return ((x * x - 1.) * x + 0.3 * (torch.roll(x, -1, dims=1) + torch.roll(x, 1, dims=1))) / self.temperature


class LadderQuarticModel(LadderDynamicsModel, QuarticModel):
    pass


class LadderMarginModel(LadderDynamicsModel, MarginModel):
    pass


class LadderQuarticMarginModel(LadderDynamicsModel, MarginModel, QuarticModel):
    pass


def quartic_fn(x):
    return ((x * x - 1.) ** 2).sum(dim=1) / 4. + 0.3 * (x * torch.roll(x, -1, dims=1)).sum(dim=1)


MOG3 = ([np.array([1., 0., 0.5]), np.array([0., 1., -0.5]), np.array([-1., -1., 0.])],
        [np.diag([0.05, 0.08, 0.1]), 0.07 * np.eye(3) + 0.02, np.diag([0.1, 0.05, 0.06])], [0.3, 0.5, 0.2])


def oracle_target(kind):
    """-> (x_dim, oracle.dynamics target or None, start states (n, rng) -> [n, x_dim])."""
    if kind == "mog":
        o = H.mog_target_oracle()
        return 2, o, o.get_samples
    if kind == "scg":
        o = H.scg_target_oracle()
        return 2, o, o.get_samples
    if kind == "mog3":
        o = od.GMM(*MOG3)
        return 3, o, o.get_samples
    if kind == "quartic10":
        return 10, None, lambda n, rng: rng.normal(0, 0.8, (n, 10))
    if kind in ("rough_well", "funnel"):
        return 2, None, lambda n, rng: rng.normal(0, 0.7, (n, 2))
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> dict (shared, left unchanged): weights, masks, x, z and (v forward, v backward, direction bits, uniforms) of
    each transition, all float32 numbers; both directions run in each batch."""
    dim, _, samples = oracle_target(c.kind)
    xp, vp = H.mlp_weights(dim, c.H, regime=c.regime)
    xp, vp = {k: f32(v) for k, v in xp.items()}, {k: f32(v) for k, v in vp.items()}
    masks = od.make_masks(c.N, dim, np.random.RandomState(3))
    rng = np.random.default_rng(1000 + c.seed)
    x, z = f32(samples(c.B, rng)), f32(rng.standard_normal((c.B, dim)))

    def mk():
        bits = rng.integers(0, 2, c.B).astype(np.float64)
        bits[:2] = (1., 0.)
        return (f32(rng.standard_normal((c.B, dim))), f32(rng.standard_normal((c.B, dim))), bits,
                f32(rng.uniform(size=c.B)))
    return dict(dim=dim, xp=xp, vp=vp, masks=masks, x=x, z=z, dx=mk(), dz=mk())


def model(c, temperature, margin=False):
    """A fresh float64 model of a case at `temperature` (a float, or [B]: the ladder)."""
    i = inputs(c)
    _, o, _ = oracle_target(c.kind)
    if c.kind == "quartic10":
        cls = LadderQuarticMarginModel if margin else LadderQuarticModel
    else:
        cls = LadderMarginModel if margin else LadderDynamicsModel
    tm = cls(o, c.N, c.eps, i["masks"], i["xp"], i["vp"])
    tm.temperature = t64(temperature) if np.ndim(temperature) else float(temperature)
    return tm


def loss_rows(tm, i, B):
    """-> (per-row terms [2B] whose sum is the loss of mog_model.py:336-355, proposals [2B, dim], p [2B])."""
    x, z = t64(i["x"]), t64(i["z"])
    Lx, px = tm.propose(x, *map(t64, i["dx"][:3]))
    Lz, pz = tm.propose(z, *map(t64, i["dz"][:3]))
    v = torch.cat([((x - Lx) ** 2).sum(1) * px, ((z - Lz) ** 2).sum(1) * pz]) + 1e-4
    return (SCALE / v - v / SCALE) / B, torch.cat([Lx, Lz]), torch.cat([px, pz])


@functools.lru_cache(maxsize=None)
def reference(c):
    """-> (model with gradients, loss, per-row terms [2B] (undivided), proposals, p) of the ladder step in float64;
    computed once and shared, left unchanged."""
    tm = model(c, ladder(c.B))
    rows, L, p = loss_rows(tm, inputs(c), c.B)
    loss = rows.sum()
    loss.backward()
    return tm, float(loss.detach()), rows.detach().numpy() * c.B, L.detach().numpy(), p.detach().numpy()


def margins(c, temperature):
    """-> (relu margin, min margin) of the case at `temperature` as tests/toy_cases.py::train_margins takes them: over
    the x and the z chains in the direction each one's bit picks."""
    tm = model(c, temperature, margin=True)
    i = inputs(c)
    relu, arg = np.inf, np.inf
    with torch.no_grad():
        for start, d in ((i["x"], i["dx"]), (i["z"], i["dz"])):
            for bwd, v0 in ((False, d[0]), (True, d[1])):
                rows = d[2] < 0.5 if bwd else d[2] > 0.5
                x0, v = t64(start), t64(v0)
                tm.reset_margin(c.B)
                xN, vN, _, ld = tm.trajectory(x0, v, None, bwd)
                relu = min(relu, float(tm.margin[rows].min()))
                h0 = tm._energy(x0, None) + 0.5 * (v ** 2).sum(1)
                h1 = tm._energy(xN, None) + 0.5 * (vN ** 2).sum(1)
                arg = min(arg, float((h0 - h1 + ld).abs()[torch.tensor(rows)].min()))
    return relu, arg


# ------------------------------------------------------------------------------------------------------ the library
def library_energy(la, kind):
    if kind == "mog":
        return la.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5]).get_energy_function()
    if kind == "scg":
        return la.Gaussian(np.zeros(2), np.array([[50.05, -49.95], [-49.95, 50.05]])).get_energy_function()
    if kind == "mog3":
        return la.GMM(*MOG3).get_energy_function()
    if kind == "rough_well":
        return la.RoughWell(2, 0.5, easy=True).get_energy_function()
    if kind == "funnel":
        return la.GaussianFunnel(2).get_energy_function()
    assert kind == "quartic10"
    return quartic_fn


def trainer(c, temperature=1.0):
    """-> a fresh DynamicsTrainer on a Dynamics of the case (use_temperature=True, `temperature` on the dynamics)."""
    import l2hmc_amd as la
    from l2hmc_amd.dynamics_trainer import DynamicsTrainer
    i = inputs(c)
    dyn = la.Dynamics(i["dim"], library_energy(la, c.kind), trajectory_length=c.N, eps=c.eps,
                      net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=c.H),
                      use_temperature=True)
    dyn.temperature = temperature
    dyn.set_masks(i["masks"])
    dyn.XNet.load_state(i["xp"])
    dyn.VNet.load_state(i["vp"])
    if c.layered:
        dyn.layered = True
    return DynamicsTrainer(dyn, scale=SCALE)
