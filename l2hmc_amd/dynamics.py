"""`Dynamics` with the reference's surface (l2hmc/utils/dynamics.py:34-319).

Two paths behind it, chosen per instance (`Dynamics.layered`):
  * one launch per trajectory (l2hmc_small_trajectory / l2hmc_small_propose): the packed toy targets of
    l2hmc_amd.distributions (GMM / Gaussian / RoughWell / GaussianFunnel, x_dim <= 8, <= 8 components) with `network`-style nets of at most 64
    hidden units -- BASELINE configs 1 and 2;
  * layer by layer, for everything else the reference's constructor accepts (:35-43: ANY `energy_function`, any x_dim,
    `net_factory` of any `num_nodes`): per sub-update of utils/dynamics.py:120-225 one S/T/Q evaluation through
    l2hmc_stq_dense (any width) and one ops.lf_update_v / _x launch; the energy gradient comes from the packed target's
    kernel or, for an arbitrary callable on torch tensors, from torch.autograd (the reference's tf.gradients, :241-242)."""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib, _runs, ops
from . import autograd_toy as _autograd


class Dynamics(object):
    def __init__(self, x_dim, energy_function, trajectory_length=10, eps=0.1, hmc=False, net_factory=None,
                 eps_trainable=True, use_temperature=False, device=None, seed=42):
        self.x_dim = x_dim
        self.use_temperature = use_temperature
        self.temperature = 1.0             # the reference feeds a placeholder (:48)
        self.first_layer_form = 0          # 0 by batch size; 1 / 2 force the toy kernel's matrix-pipe / VALU first layer
        self._device = device or torch.device("cuda", torch.cuda.current_device())
        # quirk Q2: eps = exp(alpha), alpha = log(eps) (:51-60)
        self.alpha = torch.log(torch.tensor(float(eps), dtype=torch.float32))
        self.eps_trainable = eps_trainable
        if not callable(energy_function):
            raise TypeError("energy_function must be callable: x [B, x_dim] -> energies [B]")
        self._fn = energy_function
        # packed toy target (l2hmc_amd.distributions) or None = an arbitrary callable on torch tensors
        self._target = getattr(energy_function, "target", None)
        if self._target is not None:
            if self._target.dim != x_dim:
                raise ValueError(f"x_dim={x_dim} but the target has dimension {self._target.dim}")
            self._target.to(self._device)
        self.trajectory_length = int(trajectory_length)
        self.hmc = hmc
        self._init_mask()
        if hmc:                             # :75-78
            self.XNet = lambda inp: [torch.zeros_like(inp[0]) for _ in range(3)]
            self.VNet = lambda inp: [torch.zeros_like(inp[0]) for _ in range(3)]
        else:
            self.XNet = net_factory(x_dim, scope='XNet', factor=2.0)
            self.VNet = net_factory(x_dim, scope='VNet', factor=1.0)
        self._seed, self._draws = int(seed), 0
        # the one-launch kernels hold x_dim <= 8 and 64 hidden units, and evaluate the packed targets only
        wide = (not hmc) and int(getattr(self.XNet, "num_nodes", 0)) > _lib.MAX_SMALL_NODES
        self.layered = self._target is None or int(x_dim) > _lib.MAX_SMALL_DIM or wide

    @property
    def eps(self):
        return torch.exp(self.alpha)

    @property
    def variables(self):
        """alpha (eps = exp(alpha)), then XNet's and VNet's reference-layout tensors (layer order, kernel before bias,
        then the two scale vectors): what a torch optimiser takes.  Each may take requires_grad_(); the one-launch
        kernels then record an autograd graph (l2hmc_amd/autograd_toy.py)."""
        out = [self.alpha]
        if not self.hmc:
            out += list(self.XNet.variables) + list(self.VNet.variables)
        return out

    @property
    def trainable_variables(self):
        """`variables`, without alpha unless eps_trainable (:51-60)."""
        v = self.variables
        return v if self.eps_trainable else v[1:]

    def _init_mask(self):
        """:85-96 (legacy global NumPy stream)."""
        mask_per_step = []
        for _ in range(self.trajectory_length):
            ind = np.random.permutation(np.arange(self.x_dim))[:int(self.x_dim / 2)]
            m = np.zeros((self.x_dim,))
            m[ind] = 1
            mask_per_step.append(m)
        self.set_masks(np.stack(mask_per_step))

    def set_masks(self, masks):
        masks = np.asarray(masks, dtype=np.float32)
        if masks.shape != (self.trajectory_length, self.x_dim):
            raise ValueError(f"masks: expected {(self.trajectory_length, self.x_dim)}, got {masks.shape}")
        self.mask = _lib.as_dev(masks, self._device)

    def _get_mask(self, step):
        m = self.mask[int(step)]
        return m, 1. - m

    def _format_time(self, t, tile=1):
        """:105-110."""
        arg = np.float32(2 * np.pi) * np.float32(t) / np.float32(self.trajectory_length)
        return torch.tensor([[np.cos(arg), np.sin(arg)]], dtype=torch.float32).repeat(tile, 1)

    def _temp(self):
        return float(self.temperature) if self.use_temperature else 1.0

    def _chain_temperatures(self, temperature, B, who):
        """`temperature=` of a call -> (scalar or None, ladder or None): None for the dynamics' own; a number or a 0-d
        array / tensor -> its float32 value as a float; [B] or [1, B] -> the ladder as a float32 device tensor [B]
        (`_runs.per_chain`: a float32 tensor of that shape on the device stays there, unchecked).  ValueError for
        another shape, for a value that in float32 is not finite or not > 0, for a ladder tensor that requires grad
        (its values are not differentiated) and for any temperature on a dynamics built with use_temperature=False.
        Host-side: a caller runs it before it takes a draw."""
        if temperature is None:
            return None, None
        if not self.use_temperature:
            raise ValueError(f"{who}: temperature= on a Dynamics built with use_temperature=False, which ignores "
                             "temperatures (Dynamics._temp): build it with use_temperature=True")
        if isinstance(temperature, torch.Tensor) and temperature.requires_grad:
            raise ValueError(f"{who}: temperature requires grad; temperatures are not differentiated (detach it)")
        if _runs.ndim(temperature) == 0:
            t32 = np.float32(float(temperature))
            if not (np.isfinite(t32) and t32 > 0):
                raise ValueError(f"{who}: every temperature must be finite and > 0 (in float32)")
            return float(temperature), None
        return None, _runs.per_chain(temperature, B, self._device, who=who, name="temperature", sign="> 0")[0]

    def _call_temperature(self, temperature, B, who):
        """`temperature=` of forward / backward / both / propose -> what autograd_toy and `_plan` take: None, a float,
        or the ladder [B] on the device.  `_chain_temperatures`' refusals, and NotImplementedError for a ladder on a
        layer-by-layer Dynamics (DynamicsTrainer trains one on a ladder)."""
        t_scalar, t_ladder = self._chain_temperatures(temperature, B, who)
        if t_ladder is not None and self.layered:
            raise NotImplementedError(f"{who}: a temperature per chain on a Dynamics that runs layer by layer; only the "
                                      "one-launch toy targets take a ladder here (DynamicsTrainer trains a "
                                      "layer-by-layer Dynamics on one)")
        return t_scalar if t_ladder is None else t_ladder

    @contextlib.contextmanager
    def _at(self, temp):
        """A layer-by-layer call at the scalar `temp` (None: as it is): the layered stages read `self.temperature`,
        which is set for the call and put back (DynamicsTrainer's rule)."""
        saved = self.temperature
        if temp is not None:
            self.temperature = temp
        try:
            yield
        finally:
            self.temperature = saved

    def kinetic(self, v):
        return ops.kinetic_energy(_lib.as_dev(v, self._device))

    def energy(self, x, aux=None):
        """:227-236."""
        if self._target is None:
            x = _lib.as_dev(x, self._device).reshape(-1, self.x_dim)
            e = _lib.expect_shape(self._fn(x), (x.shape[0],), "energy_function(x)", "Dynamics.energy")
            # (one contiguous float32 per row, whatever the callable returned: p_accept hands its address to a kernel)
            return e.to(torch.float32).contiguous() / self._temp()
        return self._target.energy_grad(x, self._temp(), want_grad=False)[0]

    def hamiltonian(self, x, v, aux=None):
        return self.energy(x) + self.kinetic(v)

    def grad_energy(self, x, aux=None):
        """:241-242 -- closed form of the reference's tf.gradients for the packed targets, torch.autograd of the
        caller's function otherwise."""
        if self._target is None:
            with torch.enable_grad():
                xg = _lib.as_dev(x, self._device).reshape(-1, self.x_dim).detach().clone().requires_grad_(True)
                e = _lib.expect_shape(self._fn(xg), (xg.shape[0],), "energy_function(x)", "Dynamics.grad_energy")
                (g,) = torch.autograd.grad(e.sum(), xg)
            return (g / self._temp()).to(torch.float32).contiguous()
        return self._target.energy_grad(x, self._temp())[1]

    # ---- layer-by-layer path (utils/dynamics.py:120-225 sub-update by sub-update) ------------------------------------
    def _sub_v(self, x, v, t, d, logdet):
        """:123-132 / :158-166 (d = 0), :175-185 / :213-223 (d = 1): half-kick with VNet([x, grad, t])."""
        g = self.grad_energy(x)
        S, T, Q = self.VNet([x, g, t])
        out, ld = ops.lf_update_v(v, g, S, T, Q, self.eps, d)
        logdet += ld
        return out

    def _sub_x(self, x, v, keep, t, d, logdet):
        """:134-156 (d = 0), :187-211 (d = 1): XNet([v, keep * x, t]); the kept coordinates pass through."""
        S, T, Q = self.XNet([v, keep * x, t])
        out, ld = ops.lf_update_x(x, v, keep, S, T, Q, self.eps, d)
        logdet += ld
        return out

    def _layered_run(self, x, v, backward, log_jac):
        """forward (:255-281) or backward (:283-310) through the public sub-update operators."""
        x0, v0 = x, v
        lj = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
        N = self.trajectory_length
        for i in range(N):
            step = N - i - 1 if backward else i
            t = self._format_time(step)
            m, mb = self._get_mask(step)
            if not backward:                                   # :120-170
                v = self._sub_v(x, v, t, 0, lj)
                x = self._sub_x(x, v, m, t, 0, lj)
                x = self._sub_x(x, v, mb, t, 0, lj)
                v = self._sub_v(x, v, t, 0, lj)
            else:                                              # :172-225
                v = self._sub_v(x, v, t, 1, lj)
                x = self._sub_x(x, v, mb, t, 1, lj)
                x = self._sub_x(x, v, m, t, 1, lj)
                v = self._sub_v(x, v, t, 1, lj)
        return (x, v, lj) if log_jac else (x, v, self.p_accept(x0, v0, x, v, lj))

    def _plan(self, temperature=None):
        """The plan struct of the one-launch kernels; `temperature` (a float) goes into this struct alone, where
        `self.temperature` stays as it was."""
        if self.layered:
            raise NotImplementedError(
                "this Dynamics runs layer by layer (arbitrary energy function, x_dim > 8 or more than 64 hidden units): "
                "the one-launch kernels (l2hmc_small_*) and the one-launch training step do not hold it")
        p = _lib.SmallPlan(x_dim=self.x_dim, trajectory_length=self.trajectory_length, hmc=int(bool(self.hmc)),
                           eps=float(self.eps.detach()), first_layer_form=int(self.first_layer_form), masks=self.mask.data_ptr(),
                           target=self._target.struct(self._temp()), num_nodes=0)
        if not self.hmc:
            p.xnet, p.vnet = self.XNet.pack(), self.VNet.pack()
            p.num_nodes = p.xnet.H
        if temperature is not None:
            p.target.temperature = temperature
        return p

    def _normal(self, shape):
        out = ops.fill_normal(shape, self._seed, self._draws, self._device)
        self._draws += 1
        return out

    def _run(self, x, init_v, backward, log_jac, temperature=None):
        x = _lib.as_dev(x, self._device).reshape(-1, self.x_dim)
        who = "Dynamics.backward" if backward else "Dynamics.forward"
        temp = self._call_temperature(temperature, x.shape[0], who)
        _lib.expect_shape(init_v, tuple(x.shape), "init_v", who)
        if _autograd.wants_grad(self, x, init_v):
            _autograd.check_differentiable(self)          # before any draw
            v = _lib.as_dev(init_v, self._device) if init_v is not None else self._normal(tuple(x.shape))
            return _autograd.run(self, x, v, backward, log_jac, temp)
        v = _lib.as_dev(init_v, self._device) if init_v is not None else self._normal(tuple(x.shape))
        if self.layered:
            with self._at(temp):
                return self._layered_run(x, v, backward, log_jac)
        rows = x.shape[0]
        X, V = torch.empty_like(x), torch.empty_like(x)
        lj = torch.empty(rows, dtype=torch.float32, device=x.device)
        p = torch.empty_like(lj)
        dirs = torch.full((rows,), 1, dtype=torch.int32, device=x.device) if backward else None
        self._trajectory(temp, x, v, dirs, rows, X, V, lj, p)
        return (X, V, lj) if log_jac else (X, V, p)

    def _trajectory(self, temp, x, v, dirs, rows, X, V, lj, p):
        """l2hmc_small_trajectory at `temp` (None or a float: on the plan), or with the ladder `temp` [C], rows a
        multiple of C, l2hmc_small_trajectory_tempered: row r at temp[r % C]."""
        if isinstance(temp, torch.Tensor):
            plan = self._plan()
            _lib.call("l2hmc_small_trajectory_tempered", C.byref(plan), temp, 1, temp.numel(), x, v, dirs, rows, X, V,
                      lj, p, device=self._device)
        else:
            plan = self._plan(temp)
            _lib.call("l2hmc_small_trajectory", C.byref(plan), x, v, dirs, rows, X, V, lj, p, device=self._device)

    def both(self, x, init_v_forward=None, init_v_backward=None, log_jac=False, temperature=None):
        """forward(x) and backward(x) of the same chains in ONE launch (rows stacked, per-row direction):
        what `propose` needs (sampler.py:38-39).  Returns ((Xf, Vf, pf), (Xb, Vb, pb)).  temperature: as `forward`'s;
        a ladder [B] runs chain i at temperature[i] in both directions.  No graph is recorded here."""
        x = _lib.as_dev(x, self._device).reshape(-1, self.x_dim)
        B = x.shape[0]
        temp = self._call_temperature(temperature, B, "Dynamics.both")
        for name, v in (("init_v_forward", init_v_forward), ("init_v_backward", init_v_backward)):     # before any draw
            _lib.expect_shape(v, tuple(x.shape), name, "Dynamics.both")
        vf = _lib.as_dev(init_v_forward, self._device) if init_v_forward is not None else self._normal(tuple(x.shape))
        vb = _lib.as_dev(init_v_backward, self._device) if init_v_backward is not None else self._normal(tuple(x.shape))
        if self.layered:
            with self._at(temp):
                return self._layered_run(x, vf, False, log_jac), self._layered_run(x, vb, True, log_jac)
        xx, vv = torch.cat([x, x]), torch.cat([vf, vb])
        dirs = torch.cat([torch.zeros(B, dtype=torch.int32, device=x.device),
                          torch.ones(B, dtype=torch.int32, device=x.device)])
        X, V = torch.empty_like(xx), torch.empty_like(xx)
        lj = torch.empty(2 * B, dtype=torch.float32, device=x.device)
        p = torch.empty_like(lj)
        self._trajectory(temp, xx, vv, dirs, 2 * B, X, V, lj, p)
        third = lj if log_jac else p
        return (X[:B], V[:B], third[:B]), (X[B:], V[B:], third[B:])

    def forward(self, x, init_v=None, aux=None, log_path=False, log_jac=False, temperature=None):
        """:255-281.  Differentiable (torch.autograd, l2hmc_amd/autograd_toy.py) when grad mode is on and x, init_v,
        alpha or a network weight requires grad.

        temperature: None = the call as it is, at the dynamics' own temperature; a scalar = this call at that
        temperature, on a copy of the plan (`self.temperature` stays as it was: DynamicsTrainer's rule); [B] or [1, B]
        = a ladder, chain i at temperature[i] (l2hmc_small_trajectory_tempered, and l2hmc_small_vjp_tempered under
        grad) with the bits of the scalar call at that value.  The temperatures are NOT differentiated.  Refused before
        any draw is taken: ValueError for another shape, for a value that in float32 is not finite or not > 0, for a
        ladder tensor that requires grad and for any temperature on use_temperature=False; NotImplementedError for a
        ladder on a layer-by-layer Dynamics."""
        if aux is not None:
            raise NotImplementedError("aux inputs are only used by the out-of-scope VAE scripts")
        return self._run(x, init_v, False, log_jac, temperature)

    def backward(self, x, init_v=None, aux=None, log_jac=False, temperature=None):
        """:283-310.  Differentiable as `forward`; temperature: as `forward`'s."""
        if aux is not None:
            raise NotImplementedError("aux inputs are only used by the out-of-scope VAE scripts")
        return self._run(x, init_v, True, log_jac, temperature)

    def p_accept(self, x0, v0, x1, v1, log_jac, aux=None):
        """:312-319."""
        who = "Dynamics.p_accept"
        x0 = _lib.as_dev(x0, self._device).reshape(-1, self.x_dim)
        for name, t in (("v0", v0), ("x1", x1), ("v1", v1)):
            _lib.expect_shape(t, tuple(x0.shape), name, who)
        _lib.expect_shape(log_jac, (x0.shape[0],), "log_jac", who)
        e_new, e_old = self.hamiltonian(x1, v1), self.hamiltonian(x0, v0)
        return ops.accept_prob(e_old, e_new, _lib.as_dev(log_jac, self._device))
