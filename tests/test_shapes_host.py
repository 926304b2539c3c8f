"""Host-side checks that a wrongly SHAPED caller tensor is refused at the Python boundary (`_lib.expect_shape`) before
any kernel could read it: the C ABI takes raw pointers and sizes a launch from one argument, so a short tensor would
be read past its end.  Every tensor argument of every stateless operator (ops, ops_periodic, torch_ops) and of every
method that takes caller tensors (GaugeDynamics, Dynamics, propose, tf_accept, both trainers, both samplers, the
networks) is offended in turn among good arguments; the call must raise ValueError naming it and both shapes, with
nothing reached: the library and torch.cuda raise AssertionError (`no_backend`), the objects are stubs whose draws and
plans raise, and their draw counter must not move.  The accepted forms must get as far as that backend.  No GPU, no
library: the refusals are proved here because on a device a missing check IS the out-of-bounds access."""
import inspect
import types

import numpy as np
import pytest
import torch

import l2hmc_amd as la
from l2hmc_amd import _lib, autograd, ops, ops_periodic, sampler, torch_ops
from l2hmc_amd.dynamics import Dynamics
from l2hmc_amd.dynamics_sampler import DynamicsSampler
from l2hmc_amd.dynamics_trainer import DynamicsTrainer
from l2hmc_amd.gauge_dynamics import GaugeDynamics
from l2hmc_amd.gauge_sampler import GaugeSampler
from l2hmc_amd.gauge_trainer import GaugeTrainer
from l2hmc_amd.network import ConvNet3D, GenericNet, MLPNet
from tests.test_autograd_ladder_host import _gauge_stub, _toy_stub
from tests.test_ops_host import CASES, no_backend  # noqa: F401  (the fixture)

T, X, B = 4, 6, 3
D = 2 * T * X
CPU = torch.device("cpu")


def text(shape):
    """A shape as the messages print it: a tuple, with * for an extent that is free."""
    return "(" + ", ".join("*" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"


@pytest.fixture
def wave(monkeypatch):
    """CPU tensors pass `dev_ptr` as good GPU tensors would: what is left to refuse them is their shape."""
    real = _lib.dev_ptr
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor":
                        1 if isinstance(t, torch.Tensor) else real(t, dtype, name))


def offenders(shape):
    """{kind: shape}: one row fewer, one column fewer, one extra trailing dimension, 0-D, a single element for a
    per-row vector, and the transpose of a non-square matrix (the good tensor's element count)."""
    out = {"row": (shape[0] - 1,) + shape[1:], "extra": shape + (2,), "0d": ()}
    if len(shape) >= 2:
        out["col"] = shape[:1] + (shape[1] - 1,) + shape[2:]
    if len(shape) == 1:
        out["one"] = (1,)
    if len(shape) == 2 and shape[0] != shape[1]:
        out["T"] = shape[::-1]
    return out


def fits(shape, constraint, fold=False):
    if fold and len(shape) > 2:
        shape = (shape[0], int(np.prod(shape[1:])))
    return len(shape) == len(constraint) and all(c is None or c == s for c, s in zip(constraint, shape))


def blamed(args, anchor, constraint, arg, bad, fold=False):
    """The argument the error must name.  The FIRST tensor (`anchor`) fixes rows and width for the others: offended in a
    way its own rule (`constraint`; None: any shape) allows, it makes the NEXT tensor the one that does not fit (None
    if there is none: a valid call)."""
    if arg != anchor:
        return arg
    if constraint is not None and not fits(bad, constraint, fold):
        return anchor
    names = list(args)
    i = names.index(anchor)
    return names[i + 1] if i + 1 < len(names) else None


def check_refusal(excinfo, prefix, bad, expected=None):
    msg = str(excinfo.value)
    assert msg.startswith(prefix), msg
    assert "expected" in msg and text(bad) in msg, msg
    if expected is not None:
        assert text(expected) in msg, msg


# ================================================================================================ stateless operators
H_, K_, D_ = 5, 4, 3           # stq_dense: hidden width, Ka = Kb, output width
PERIODIC = {
    "lf_update_x_ncp": (dict(x=(B, D), v=(B, D), keep=(D,), S=(B, D), T=(B, D), Q=(B, D)), (0.1, 1)),
    "lf_update_x_ncp_vjp": (dict(x=(B, D), v=(B, D), keep=(D,), S=(B, D), T=(B, D), Q=(B, D), dx_out=(B, D),
                                 dlogdet=(B,)), (0.1, 1)),
    "u1_angle_features": (dict(x=(B, D), out=(B, 2 * D)), ()),
    "u1_angle_features_vjp": (dict(x=(B, D), dfeat=(B, 2 * D), dx=(B, D)), ()),
}
WEIGHTS = dict(w1_t=(H_, 2 * K_), wt=(2, H_), b1=(H_,), wh_t=(H_, H_), bh=(H_,), whd_t=(3, D_, H_), bhd=(3, D_),
               coeff_s=(D_,), coeff_q=(D_,))
TORCH = {
    "u1_action_force": (dict(x=(B, D)), (T, X, 2.0)),
    "stq_dense": (dict(a=(B, K_), b=(B, K_), **WEIGHTS), (0, 1.0, 0.0)),
    "lf_update_v": CASES["lf_update_v"],
    "lf_update_x": CASES["lf_update_x"],
    "accept_prob": CASES["accept_prob"],
    "mix_accept": CASES["mix_accept"],
    "kinetic_energy": CASES["kinetic_energy"],
    "wrap_angle": (dict(x=(B, D)), ()),
}
MODULES = {"ops": (ops, CASES), "ops_periodic": (ops_periodic, PERIODIC), "torch_ops": (torch_ops, TORCH)}
# the first tensor's own rule (None: any shape); where absent: 2-D
ANCHOR_RULE = {"accept_prob": None, "wrap_angle": None, "fill_normal": None, "fill_uniform": None,
               "u1_action_force": (None, D), "u1_force_hvp": (None, D), "stq_dense": (None, K_),
               }
# stq_dense: w1_t gives H, whd_t gives D -- offended within their own rules they make the next weight the misfit
OVERRIDE = {("stq_dense", "w1_t", "row"): "whd_t", ("stq_dense", "whd_t", "col"): "bhd"}


def run_op(mod, fn, tensors):
    """`fn` of `mod` on {argument: tensor or None} and the case's scalars, bound by the signature."""
    module, cases = MODULES[mod]
    scalars = list(cases[fn][1])
    if fn.startswith("fill_"):
        return getattr(module, fn)(None, 1, 0, out=tensors["out"])
    if fn == "stq_dense":
        return module.stq_dense(tensors["a"], tensors["b"], [tensors[k] for k in WEIGHTS], *scalars)
    f = getattr(module, fn)
    params = list(inspect.signature(getattr(f, "_init_fn", f)).parameters)
    kw = dict(tensors)
    for p in params:
        if p not in kw and scalars:
            kw[p] = scalars.pop(0)
    return f(**kw)


def test_cases_cover_every_function_of_ops_periodic():
    public = {n for n, f in vars(ops_periodic).items()
              if callable(f) and not n.startswith("_") and f.__module__ == ops_periodic.__name__}
    assert public == set(PERIODIC)


def test_cases_cover_every_torch_op():
    assert set(torch_ops.OPS) == set(TORCH)
    registered = {n for n, f in vars(torch_ops).items() if isinstance(f, torch.library.CustomOpDef)}
    assert registered == set(TORCH)


# (torch.ops.l2hmc.u1_action_force reshapes its x to [-1, 2 T X] as it always did: torch refuses a count that is no
#  whole number of rows, and any other is a batch of configurations)
OP_OFFENCES = [(mod, fn, arg, kind) for mod, (_, cases) in MODULES.items() for fn, (shapes, _) in cases.items()
               for arg, shape in shapes.items() for kind in offenders(shape)
               if (mod, fn) != ("torch_ops", "u1_action_force")]


@pytest.mark.parametrize("mod,fn,arg,kind", OP_OFFENCES, ids=lambda v: str(v))
def test_each_operator_argument_of_the_wrong_shape_is_refused_and_named(no_backend, wave, mod, fn, arg,  # noqa: F811
                                                                        kind):
    shapes = MODULES[mod][1][fn][0]
    bad = offenders(shapes[arg])[kind]
    anchor = "w1_t" if arg in WEIGHTS and arg != "whd_t" else arg if arg == "whd_t" else next(iter(shapes))
    rule = ANCHOR_RULE.get((mod, fn), ANCHOR_RULE.get(fn, (None, None)))
    if arg in WEIGHTS:
        rule = (None, None) if arg == "w1_t" else (3, None, H_)
    who = OVERRIDE.get((fn, arg, kind)) or blamed(shapes, anchor, rule, arg, bad)
    tensors = {a: torch.zeros(bad if a == arg else s) for a, s in shapes.items()}
    if who is None:                  # the only tensor, in a shape its rule allows: nothing to refuse
        with pytest.raises(AssertionError, match="must not reach the library"):
            run_op(mod, fn, tensors)
        return
    if fn == "stq_dense" and arg == "w1_t" and kind in ("col", "T"):     # Ka + Kb odd: no Ka = Kb
        with pytest.raises(ValueError, match=r"^w1_t: expected shape \(H, Ka \+ Kb\) with Ka = Kb, got"):
            run_op(mod, fn, tensors)
        return
    with pytest.raises(ValueError) as e:
        run_op(mod, fn, tensors)
    # (an anchor's own rule has free extents: the message has them as `*`, and only the offender's shape is compared)
    check_refusal(e, f"{who}: expected shape ", bad if who == arg else shapes[who],
                  shapes[arg] if who == arg != anchor else None)


@pytest.mark.parametrize("mod,fn", [(m, f) for m, (_, cases) in MODULES.items() for f in cases])
def test_good_operator_arguments_get_as_far_as_the_library(no_backend, wave, mod, fn):  # noqa: F811
    shapes = MODULES[mod][1][fn][0]
    with pytest.raises(AssertionError, match="must not reach the library"):
        run_op(mod, fn, {a: torch.zeros(s) for a, s in shapes.items()})


@pytest.mark.parametrize("mod,fn,arg", [("ops", "mix_accept", "u"), ("ops", "wrap_angle", "out"),
                                        ("ops_periodic", "lf_update_x_ncp_vjp", "dlogdet"),
                                        ("ops_periodic", "u1_angle_features", "out"),
                                        ("ops", "lf_update_v", "S"), ("ops", "lf_update_x", "Q")])
def test_an_optional_operator_argument_may_stay_none(no_backend, wave, mod, fn, arg):  # noqa: F811
    shapes = MODULES[mod][1][fn][0]
    with pytest.raises(AssertionError, match="must not reach the library"):
        run_op(mod, fn, {a: None if a == arg else torch.zeros(s) for a, s in shapes.items()})


def test_expect_shape_is_host_arithmetic_on_shape_tuples(no_backend):  # noqa: F811
    class OnlyShape:                 # no data, no device, no dtype: the helper may read nothing else
        shape = (B, D)
    t = OnlyShape()
    assert _lib.expect_shape(t, (B, D), "t") is t and _lib.expect_shape(t, (None, D), "t") is t
    assert _lib.expect_shape(None, (B,), "t") is None
    assert _lib.expect_shape([[0.0] * D] * B, (B, D), "t") is not None                # a nested list has a shape too
    OnlyShape.shape = (B, T, X, 2)
    assert _lib.expect_shape(t, (B, D), "t", "C.m", fold=True) is t
    with pytest.raises(ValueError, match=r"^t: expected shape \(3, 48\), got \(3, 4, 6, 2\)$"):
        _lib.expect_shape(t, (B, D), "t")
    with pytest.raises(ValueError, match=r"^C\.m: t of shape \(3, 4, 6, 2\): expected \(\*, 47\)"):
        _lib.expect_shape(t, (None, D - 1), "t", "C.m", fold=True)
    OnlyShape.shape = (B,)
    with pytest.raises(ValueError, match=r"^C\.m: u of shape \(3,\): expected \(1,\)$"):
        _lib.expect_shape(t, (1,), "u", "C.m")


# ================================================================================================ the objects
def reached(*_a, **_k):
    raise AssertionError("reached the backend")


REACHED = "reached the backend|a draw was taken|must not build a plan|must not reach the library"


def gauge(T_=T, X_=X, B_=B, hmc=False):
    """`_gauge_stub` at a lattice of this file: draws and plans raise, everything behind the gates is `reached`."""
    GD, dyn = _gauge_stub(hmc=hmc)
    dyn.lattice = types.SimpleNamespace(time_size=T_, space_size=X_, grad_action=reached)
    dyn.x_dim, dyn.batch_size, dyn.periodic = 2 * T_ * X_, B_, False
    for name in ("potential", "hamiltonian", "grad_potential", "_stq", "position_fn", "momentum_fn"):
        setattr(dyn, name, reached)
    return dyn


def toy(B_=6, D_=2, hmc=False):
    _, dyn, _ = _toy_stub(B=B_, D=D_, hmc=hmc)
    for name in ("_trajectory", "hamiltonian", "_layered_run", "forward", "both"):
        setattr(dyn, name, reached)
    dyn.XNet = dyn.VNet = types.SimpleNamespace(state_dict=reached)
    return dyn


def gauge_trainer():
    tr = types.SimpleNamespace(dynamics=gauge())
    tr._chain_betas = lambda *a: GaugeTrainer._chain_betas(tr, *a)
    return tr


def toy_trainer():
    tr = types.SimpleNamespace(dynamics=toy())
    tr._chain_temperatures = lambda *a: DynamicsTrainer._chain_temperatures(tr, *a)
    return tr


def _rows(x):
    return x.shape[0] if np.ndim(x) else 1


def _draws(kw, name):
    d = tuple(kw.pop(f"{name}[{i}]", None) for i in range(4))
    return None if all(t is None for t in d) else d


GB, GD_ = (B, D), (B,)                      # lattice 4x6, 3 chains
TB, TR = (6, 2), (6,)                       # toy target: x_dim 2, 6 chains
DRAWS = {f"{n}[{i}]": s for n in ("draws_x", "draws_z") for i, s in enumerate((None, None, None, None))}


def _with_draws(full, rows):
    return {f"{n}[{i}]": s for n in ("draws_x", "draws_z") for i, s in enumerate((full, full, rows, rows))}


# (label, owner of the signature, `who` of the messages, {tensor argument: good shape} in the order they are checked,
#  the first tensor's own rule (fold: trailing extents may carry the width) or None, call(obj, **tensors), obj factory)
METHODS = [
    ("apply_transition", GaugeDynamics.apply_transition, "GaugeDynamics.apply_transition",
     dict(position=GB, momentum_f=GB, momentum_b=GB, coin=GD_, u=GD_), (None, D),
     lambda d, **t: GaugeDynamics.apply_transition(d, t.pop("position"), 2.0, **t), gauge),
    ("apply_transition/ladder", GaugeDynamics.apply_transition, "GaugeDynamics.apply_transition",
     dict(position=GB, momentum_f=GB, momentum_b=GB, coin=GD_, u=GD_), (None, D),
     lambda d, **t: GaugeDynamics.apply_transition(d, t.pop("position"), np.ones(B), **t), gauge),
    ("apply_transition/grad", GaugeDynamics.apply_transition, "GaugeDynamics.apply_transition",
     dict(position=GB, momentum_f=GB, momentum_b=GB, coin=GD_, u=GD_), (None, D),
     lambda d, **t: GaugeDynamics.apply_transition(
         d, torch.as_tensor(t.pop("position"), dtype=torch.float32).requires_grad_(), 2.0, **t), gauge),
    ("autograd.draws", autograd.draws, "GaugeDynamics.apply_transition",
     dict(momentum_f=GB, momentum_b=GB, coin=GD_, u=GD_), None,
     lambda d, **t: autograd.draws(d, B, D, torch.device("cpu"), **t), gauge),
    ("transition_kernel", GaugeDynamics.transition_kernel, "GaugeDynamics.transition_kernel",
     dict(position=GB, momentum=GB), (None, D),
     lambda d, **t: GaugeDynamics.transition_kernel(d, t["position"], 2.0, momentum=t["momentum"]), gauge),
    ("_lf", GaugeDynamics._lf, "GaugeDynamics._lf", dict(position=GB, momentum=GB), (None, D),
     lambda d, **t: GaugeDynamics._lf(d, t["position"], t["momentum"], 2.0, 0, False), gauge),
    ("_update_momentum", GaugeDynamics._update_momentum, "GaugeDynamics._update_momentum",
     dict(position=GB, momentum=GB), (None, D),
     lambda d, **t: GaugeDynamics._update_momentum(d, t["position"], t["momentum"], 2.0, None, False), gauge),
    ("_update_position", GaugeDynamics._update_position, "GaugeDynamics._update_position",
     dict(position=GB, momentum=GB), (None, D),
     lambda d, **t: GaugeDynamics._update_position(d, t["position"], t["momentum"], None, np.zeros(D), None, False),
     gauge),
    ("_compute_accept_prob", GaugeDynamics._compute_accept_prob, "GaugeDynamics._compute_accept_prob",
     dict(position=GB, momentum=GB, position_post=GB, momentum_post=GB, sumlogdet=GD_), (None, D),
     lambda d, **t: GaugeDynamics._compute_accept_prob(d, beta=2.0, **t), gauge),
    ("kinetic_energy", GaugeDynamics.kinetic_energy, "GaugeDynamics.kinetic_energy", dict(v=GB), (None, D),
     lambda d, **t: GaugeDynamics.kinetic_energy(d, t["v"]), gauge),
    ("potential_energy", GaugeDynamics.potential_energy, "GaugeDynamics.potential_energy", dict(position=GB), (None, D),
     lambda d, **t: GaugeDynamics.potential_energy(d, t["position"], 2.0), gauge),
    ("grad_potential", GaugeDynamics.grad_potential, "GaugeDynamics.grad_potential", dict(position=GB), (None, D),
     lambda d, **t: GaugeDynamics.grad_potential(d, t["position"], 2.0), gauge),
    ("GaugeTrainer", GaugeTrainer.calc_loss_and_grads, "GaugeTrainer.calc_loss_and_grads",
     dict(x=GB, z=GB, **_with_draws(GB, GD_)), (None, D),
     lambda tr, **t: GaugeTrainer.calc_loss_and_grads(tr, t.pop("x"), 2.0, z=t.pop("z"), draws_x=_draws(t, "draws_x"),
                                                      draws_z=_draws(t, "draws_z")), gauge_trainer),
    ("GaugeSampler.step", GaugeSampler.step, "GaugeSampler.step", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).step(t["x"], 2.0), gauge),
    ("GaugeSampler.step/ladder", GaugeSampler.step, "GaugeSampler.step", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).step(t["x"], np.ones(_rows(t["x"]))), gauge),
    ("GaugeSampler.calc_loss", GaugeSampler.calc_loss, "GaugeSampler.calc_loss", dict(x=GB, z=GB), (None, D),
     lambda d, **t: GaugeSampler(d).calc_loss(t["x"], 2.0, z=t["z"]), gauge),
    ("GaugeSampler.run", GaugeSampler.run, "GaugeSampler.run", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).run(2, 2.0, t["x"]), gauge),
    ("GaugeSampler.run/chains", GaugeSampler.run, "GaugeSampler.run", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).run(2, np.ones((1, _rows(t["x"]))), t["x"]), gauge),
    ("GaugeSampler.run_exchange", GaugeSampler.run_exchange, "GaugeSampler.run_exchange", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).run_exchange(2, np.ones((1, _rows(t["x"]))), t["x"],
                                                 replicas=max(2, _rows(t["x"]))), gauge),
    ("GaugeSampler.run_hmc", GaugeSampler.run_hmc, "GaugeSampler.run_hmc", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).run_hmc(2, 2.0, t["x"]), lambda: gauge(hmc=True)),
    ("GaugeSampler.run_hmc_exchange", GaugeSampler.run_hmc_exchange, "GaugeSampler.run_hmc", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).run_hmc_exchange(2, 2.0, t["x"], replicas=max(2, _rows(t["x"]))),
     lambda: gauge(hmc=True)),
    ("GaugeSampler.swap_replicas", GaugeSampler.swap_replicas, "GaugeSampler.swap_replicas", dict(x=GB), (None, D),
     lambda d, **t: GaugeSampler(d).swap_replicas(t["x"], np.ones(_rows(t["x"])), max(2, _rows(t["x"])), 0), gauge),
    ("Dynamics.forward", Dynamics.forward, "Dynamics.forward", dict(x=TB, init_v=TB), None,
     lambda d, **t: Dynamics.forward(d, t["x"], init_v=t["init_v"]), toy),
    ("Dynamics.backward", Dynamics.backward, "Dynamics.backward", dict(x=TB, init_v=TB), None,
     lambda d, **t: Dynamics.backward(d, t["x"], init_v=t["init_v"], log_jac=True), toy),
    ("Dynamics.both", Dynamics.both, "Dynamics.both", dict(x=TB, init_v_forward=TB, init_v_backward=TB), None,
     lambda d, **t: Dynamics.both(d, **t), toy),
    ("Dynamics.p_accept", Dynamics.p_accept, "Dynamics.p_accept", dict(x0=TB, v0=TB, x1=TB, v1=TB, log_jac=TR), None,
     lambda d, **t: Dynamics.p_accept(d, **t), toy),
    ("propose", sampler.propose, "propose", dict(x=TB, init_v=TB, init_v_backward=TB, dir_bits=TR, u=TR), None,
     lambda d, **t: la.propose(t.pop("x"), d, do_mh_step=True, **t), toy),
    ("propose/hmc", sampler.propose, "propose", dict(x=TB, init_v=TB, init_v_backward=TB, dir_bits=TR, u=TR), None,
     lambda d, **t: la.propose(t.pop("x"), d, do_mh_step=True, **t), lambda: toy(hmc=True)),
    ("_propose_grad", sampler._propose_grad, "propose", dict(x=TB, init_v=TB, init_v_backward=TB, dir_bits=TR, u=TR),
     None, lambda d, **t: sampler._propose_grad(torch.as_tensor(t["x"], dtype=torch.float32), d, t["init_v"], True,
                                                False, t["init_v_backward"], t["dir_bits"], t["u"]), toy),
    ("tf_accept", sampler.tf_accept, "tf_accept", dict(x=TB, Lx=TB, px=TR, u=TR), (None, None),
     lambda d, **t: sampler.tf_accept(dynamics=d, **t), toy),
    ("DynamicsTrainer", DynamicsTrainer.calc_loss_and_grads, "DynamicsTrainer.calc_loss_and_grads",
     dict(x=TB, z=TB, **_with_draws(TB, TR)), None,
     lambda tr, **t: DynamicsTrainer.calc_loss_and_grads(tr, t.pop("x"), z=t.pop("z"), draws_x=_draws(t, "draws_x"),
                                                         draws_z=_draws(t, "draws_z")), toy_trainer),
    ("DynamicsSampler.run", DynamicsSampler.run, "DynamicsSampler.run", dict(x=TB), (None, 2),
     lambda d, **t: DynamicsSampler(d).run(2, t["x"]), toy),
    ("DynamicsSampler.run_hmc", DynamicsSampler.run_hmc, "DynamicsSampler.run_hmc", dict(x=TB), (None, 2),
     lambda d, **t: DynamicsSampler(d).run_hmc(2, t["x"]), lambda: toy(hmc=True)),
    ("DynamicsSampler.run_exchange", DynamicsSampler.run_exchange, "DynamicsSampler.run_exchange", dict(x=TB),
     (None, 2), lambda d, **t: DynamicsSampler(d).run_exchange(2, t["x"], temperature=np.ones((1, _rows(t["x"]))),
                                                              replicas=max(2, _rows(t["x"]))), toy),
    ("DynamicsSampler.run_hmc_exchange", DynamicsSampler.run_hmc_exchange, "DynamicsSampler.run_hmc_exchange",
     dict(x=TB), (None, 2),
     lambda d, **t: DynamicsSampler(d).run_hmc_exchange(2, t["x"], temperature=np.ones((1, _rows(t["x"]))),
                                                        replicas=max(2, _rows(t["x"]))), lambda: toy(hmc=True)),
    ("DynamicsSampler.ais", DynamicsSampler.ais, "DynamicsSampler.ais", dict(x=TB), (None, 2),
     lambda d, **t: DynamicsSampler(d).ais(4, la.Gaussian(np.zeros(2), np.eye(2)), t["x"]), lambda: toy(hmc=True)),
    ("DynamicsSampler.swap_replicas", DynamicsSampler.swap_replicas, "DynamicsSampler.swap_replicas", dict(x=TB),
     (None, 2), lambda d, **t: DynamicsSampler(d).swap_replicas(t["x"], 1.0, max(2, _rows(t["x"])), 0), toy),
    ("DynamicsSampler.generate_trajectories", DynamicsSampler.generate_trajectories,
     "DynamicsSampler.generate_trajectories", dict(x=TB), (None, 2),
     lambda d, **t: DynamicsSampler(d).generate_trajectories(num_steps=2, x=t["x"]), toy),
]
BY_LABEL = {m[0]: m for m in METHODS}
# a toy-side x is reshaped to [-1, x_dim] as it always was: any whole number of rows is a start, so it is only
# offended by a row, which makes the next tensor the misfit
TOY_X = {"Dynamics.forward", "Dynamics.backward", "Dynamics.both", "Dynamics.p_accept", "propose", "propose/hmc",
         "_propose_grad", "DynamicsTrainer"}
FOLD = {m[0] for m in METHODS if m[0].split("/")[0].split(".")[0] in
        ("apply_transition", "transition_kernel", "_lf", "_update_momentum", "_update_position", "_compute_accept_prob",
         "kinetic_energy", "potential_energy", "grad_potential", "GaugeTrainer", "GaugeSampler", "DynamicsSampler",
         "autograd")} - {"GaugeSampler.swap_replicas", "DynamicsSampler.swap_replicas"}


def test_every_named_tensor_argument_is_a_parameter_of_its_method():
    for label, owner, _, args, *_ in METHODS:
        params = inspect.signature(owner).parameters
        for a in args:
            assert a.split("[")[0] in params, (label, a)


def _folds(label, arg):
    """Whether `arg` of the method goes through a position gate (trailing extents may carry the width)."""
    if label not in FOLD:
        return False
    return arg in ("position", "momentum", "momentum_f", "momentum_b", "position_post", "momentum_post", "v", "x", "z")


METHOD_OFFENCES = [(label, arg, kind) for label, _, _, args, *_ in METHODS for arg, shape in args.items()
                   for kind in offenders(shape)
                   if not (label in TOY_X and arg == next(iter(args)) and kind != "row")]


@pytest.mark.parametrize("label,arg,kind", METHOD_OFFENCES, ids=lambda v: str(v))
def test_each_method_argument_of_the_wrong_shape_is_refused_before_anything_is_reached(no_backend, wave,  # noqa: F811
                                                                                       label, arg, kind):
    _, _, who, args, rule, call, make = BY_LABEL[label]
    bad = offenders(args[arg])[kind]
    anchor = next(iter(args))
    name = blamed(args, anchor, rule, arg, bad, fold=_folds(label, anchor)) if label != "autograd.draws" else arg
    obj = make()
    dyn = getattr(obj, "dynamics", obj)
    draws = dyn._draws
    tensors = {a: torch.zeros(bad if a == arg else s) for a, s in args.items()}
    if name is None:                 # the only tensor, one row fewer: another batch, and a good one
        with pytest.raises(AssertionError, match=REACHED):
            with torch.no_grad():
                call(obj, **tensors)
        return
    with pytest.raises(ValueError) as e:
        call(obj, **tensors)
    check_refusal(e, f"{who}: {name} of shape ", bad if name == arg else args[name],
                  args[arg] if name == arg != anchor else None)
    assert dyn._draws == draws, "a refused call must not take a draw"


def test_a_position_of_the_wrong_width_never_reaches_a_4x4_dynamics():
    """The case of the issue: [B, 30] handed to a 4x4 dynamics (D = 32) used to go to the kernels with the plan's D."""
    dyn = gauge(4, 4, 4)
    for call in (lambda x: GaugeDynamics.apply_transition(dyn, x, 2.0),
                 lambda x: GaugeDynamics.transition_kernel(dyn, x, 2.0),
                 lambda x: GaugeDynamics._lf(dyn, x, np.zeros((4, 32)), 2.0, 0, False),
                 lambda x: GaugeSampler(dyn).step(x, 2.0)):
        for x in (torch.zeros(4, 30), np.zeros((4, 30)), np.zeros((4, 4, 4, 3)), np.zeros(32), np.zeros((32, 4))):
            with pytest.raises(ValueError, match=r": (position|x) of shape \(.*\): expected \(\*, 32\)"):
                call(x)
    assert dyn._draws == 4


# ------------------------------------------------------------------------------------------------ accepted forms
def _forms(shape, rng=np.random.default_rng(5)):
    """A good tensor as float32 torch, float64 numpy and float64 torch."""
    a = rng.standard_normal(shape)
    return torch.as_tensor(a, dtype=torch.float32), a, torch.as_tensor(a)


# (left out: `calc_loss` calls the dynamics, which a stub is not; the in-place `swap_replicas` take a device tensor
#  only; `autograd.draws` with all four injected has no backend to reach, see below)
ELSEWHERE = {"GaugeSampler.calc_loss", "GaugeSampler.swap_replicas", "DynamicsSampler.swap_replicas", "autograd.draws"}


@pytest.mark.parametrize("label", [m[0] for m in METHODS if m[0] not in ELSEWHERE])
@pytest.mark.parametrize("form", [0, 1, 2], ids=["float32", "numpy64", "torch64"])
def test_accepted_forms_get_as_far_as_the_backend(no_backend, wave, label, form):  # noqa: F811
    _, _, _, args, _, call, make = BY_LABEL[label]
    with pytest.raises(AssertionError, match=REACHED):
        with torch.no_grad():
            call(make(), **{a: _forms(s)[form] for a, s in args.items()})


@pytest.mark.parametrize("label", sorted(FOLD - ELSEWHERE))
def test_a_position_may_carry_its_width_as_trailing_extents(no_backend, wave, label):  # noqa: F811
    _, _, _, args, _, call, make = BY_LABEL[label]
    lattice = (T, X, 2) if args[next(iter(args))] == GB else (1, 2)
    tensors = {a: np.zeros(s[:1] + lattice) if _folds(label, a) else np.zeros(s) for a, s in args.items()}
    with pytest.raises(AssertionError, match=REACHED):
        with torch.no_grad():
            call(make(), **tensors)


@pytest.mark.parametrize("label,given", [("apply_transition", ("position",)),
                                         ("apply_transition", ("position", "coin")),
                                         ("apply_transition/ladder", ("position", "momentum_b")),
                                         ("transition_kernel", ("position",)), ("Dynamics.forward", ("x",)),
                                         ("Dynamics.both", ("x", "init_v_backward")), ("propose", ("x", "dir_bits")),
                                         ("propose/hmc", ("x",)), ("GaugeTrainer", ("x",)),
                                         ("GaugeTrainer", ("x", "z")), ("DynamicsTrainer", ("x",))])
def test_optional_draws_may_stay_none(no_backend, wave, label, given):  # noqa: F811
    _, _, _, args, _, call, make = BY_LABEL[label]
    with pytest.raises(AssertionError, match=REACHED):
        with torch.no_grad():
            call(make(), **{a: np.zeros(s) if a in given else None for a, s in args.items()})


def test_injected_draws_of_the_right_shape_come_back_as_float32_tensors(no_backend, wave):  # noqa: F811
    dyn = gauge()
    got = autograd.draws(dyn, B, D, CPU, np.zeros((B, T, X, 2)), torch.zeros(GB, dtype=torch.float64), np.zeros(B),
                         [0.5] * B)
    assert [tuple(t.shape) for t in got] == [GB, GB, GD_, GD_] and all(t.dtype == torch.float32 for t in got)
    assert dyn._draws == 4
    for x in (torch.zeros(GB), torch.zeros(B, T, X, 2)):
        with pytest.raises(AssertionError, match=REACHED):
            GaugeSampler(dyn).swap_replicas(GaugeDynamics._x(dyn, x), np.ones(B), 3, 0)


@pytest.mark.parametrize("draws", [(np.zeros(GB),) * 3, (np.zeros(GB),) * 5, ()])
def test_trainer_draws_are_exactly_four_tensors(draws):
    tr = gauge_trainer()
    with pytest.raises(ValueError,
                       match=rf"^GaugeTrainer.calc_loss_and_grads: draws_z of {len(draws)} tensors: expected 4"):
        GaugeTrainer.calc_loss_and_grads(tr, np.zeros(GB), 2.0, draws_z=draws)
    assert tr.dynamics._draws == 4


# ------------------------------------------------------------------------------------------------ energy callables
def _callable_dynamics(fn):
    dyn = toy()
    dyn._target, dyn._fn, dyn._temp = None, fn, lambda: 2.0
    return dyn


@pytest.mark.parametrize("method,who", [(Dynamics.energy, "Dynamics.energy"),
                                        (Dynamics.grad_energy, "Dynamics.grad_energy")])
@pytest.mark.parametrize("fn", [lambda x: (x * x).sum(1, keepdim=True), lambda x: (x * x).sum(), lambda x: x * x,
                                lambda x: (x * x).sum(1)[:-1]], ids=["column", "0d", "matrix", "short"])
def test_an_energy_callable_of_the_wrong_shape_is_refused_on_both_paths(method, who, fn):
    with pytest.raises(ValueError, match=rf"^{who}: energy_function\(x\) of shape \(.*\): expected \(6,\)$"):
        method(_callable_dynamics(fn), np.ones(TB))


def test_an_energy_callable_is_coerced_to_contiguous_float32():
    wide = lambda x: (x.double() * x.double()).sum(1).repeat_interleave(2)[::2]      # noqa: E731  float64, strided
    e = Dynamics.energy(_callable_dynamics(wide), np.full(TB, 3.0))
    assert e.dtype == torch.float32 and e.is_contiguous() and tuple(e.shape) == (6,)
    assert torch.equal(e, torch.full((6,), 9.0))                                     # 2 * 3^2 / temperature 2
    g = Dynamics.grad_energy(_callable_dynamics(wide), np.full(TB, 3.0))
    assert g.dtype == torch.float32 and g.is_contiguous() and torch.equal(g, torch.full(TB, 3.0))


# ------------------------------------------------------------------------------------------------ the networks
def _generic():
    return GenericNet(model_name="XNet", device=CPU, x_dim=D, num_hidden=8, factor=2., links_shape=(T, X, 2))


def _conv():
    return ConvNet3D(model_name="XNet", device=CPU, x_dim=64, num_hidden=8, factor=2., links_shape=(4, 8, 2),
                     num_filters=2, spatial_size=8)


def _mlp():
    return MLPNet(2, "XNet", 2.0, num_nodes=5, device=CPU)


NETS = {"GenericNet": (_generic, D), "ConvNet3D": (_conv, 64), "MLPNet": (_mlp, 2)}
T1 = torch.tensor([[0.5, -0.5]])


@pytest.mark.parametrize("net", list(NETS))
@pytest.mark.parametrize("arg", ["a", "b"])
@pytest.mark.parametrize("kind", ["row", "col", "extra", "0d", "T"])
def test_a_network_input_of_the_wrong_shape_is_refused_before_the_weights_are_packed(no_backend, net, arg,  # noqa: F811
                                                                                     kind):
    make, K = NETS[net]
    good = (B, K)
    bad = offenders(good)[kind]
    name = "b" if (arg, kind) == ("a", "row") else arg          # a fixes the rows
    inputs = [torch.zeros(bad if n == arg else good) for n in "ab"] + [T1]
    with pytest.raises(ValueError) as e:
        make()(inputs)
    check_refusal(e, f"{net}.__call__: {name} of shape ", bad if name == arg else good)


@pytest.mark.parametrize("net", list(NETS))
def test_network_time_inputs(no_backend, wave, net):  # noqa: F811
    make, K = NETS[net]
    a = b = torch.zeros(B, K)
    for t in (T1, T1.repeat(B, 1), [0.5, -0.5], np.asarray([[0.5, -0.5]])):           # one row, or `rows` equal rows
        with pytest.raises(AssertionError, match="must not reach the library"):
            make()([a, b, t])
    with pytest.raises(AssertionError, match="must not reach the library"):
        make()([np.zeros((B, K)), torch.zeros(B, K, dtype=torch.float64), T1])
    differ = T1.repeat(B, 1)
    differ[1, 0] = 0.25
    with pytest.raises(ValueError, match=rf"^{net}.__call__: t of shape \(3, 2\) has rows that differ"):
        make()([a, b, differ])
    for bad in (T1.repeat(B - 1, 1), T1.repeat(B + 1, 1), torch.zeros(B, 3), torch.zeros(B, 2, 2)):
        with pytest.raises(ValueError) as e:
            make()([a, b, bad])
        check_refusal(e, f"{net}.__call__: t of shape ", tuple(bad.shape), (B, 2))


def test_network_inputs_may_carry_their_width_as_trailing_extents(no_backend, wave):  # noqa: F811
    with pytest.raises(AssertionError, match="must not reach the library"):
        _generic()([np.zeros((B, T, X, 2)), torch.zeros(B, T, X, 2), T1])
    with pytest.raises(AssertionError, match="must not reach the library"):
        _conv()([np.zeros((B, 4, 8, 2)), torch.zeros(B, 64), T1])
