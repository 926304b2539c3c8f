"""`GaugeDynamics` with the reference's operator surface
(l2hmc/dynamics/gauge_dynamics.py:42-709), backed by the HIP kernels of
libl2hmc_hip.so.  `dynamics(position, beta)` returns
(position_post, momentum_post, accept_prob, position_out) exactly as
`apply_transition` (:195-259) does; the random draws the reference takes from
the TF graph seed (momenta :269, direction coin :223, MH uniform :246) are
generated on the device by the library's Philox stream, or injected through
keyword arguments so a caller (or a parity test) can replay given draws.

Tensors are contiguous fp32 CUDA tensors [batch, x_dim]; NumPy inputs are
copied to the current device.  There is no CPU path."""
import ctypes as C

import numpy as np
import numpy.random as npr
import torch

from . import _lib, _runs, ops, ops_periodic
from . import autograd as _autograd
from .network import ConvNet3D, GenericNet


def _gate(dyn, a, name, who, rows=None):
    """`dyn._x(a)` for the argument `name` of the method `who`: the same rule, worded for the caller, and with `rows`
    the rows it must have (a momentum: its position's)."""
    _lib.expect_shape(a, (rows, dyn.x_dim), name, who, fold=True)
    return dyn._x(a)


class GaugeDynamics:
    """Dynamics engine of the L2HMC sampler on the 2D U(1) lattice."""

    def __init__(self, lattice, potential_fn, **kwargs):
        self.name = 'GaugeDynamics'
        self.lattice = lattice
        self.potential = potential_fn
        self.batch_size = self.lattice.samples.shape[0]
        self.x_dim = self.lattice.num_links
        # defaults of the reference's caller (gauge_model.py:596-603)
        self.hmc, self.network_arch, self.num_steps = False, 'generic', 5
        self.eps_trainable, self.data_format = True, 'channels_last'
        self.both_directions = True      # integrate fwd AND bwd like :211-218; False = selected only
        self.fused = True                # whole-trajectory kernel where the plan has one (hmc=True: up to 1024 sites)
        self.check_numerics = False      # True: raise on a non-finite trajectory like tf.check_numerics (:26-28)
        self.recompute = False           # True: layer-by-layer path forms every first-layer product anew (diagnostic)
        self.tiles16_only = False        # True: whole-step kernel on its 16-row form for every batch (A/B, bit-identity test)
        self.all_columns = False         # True: layer-by-layer path forms S/T/Q for every column of a position sub-update
        self.full_l1 = False             # True: whole-step kernel forms XNet's first-layer x product over all D columns (A/B)
        self.single_kicks = False        # True: whole-step kernel runs every momentum half-kick as a network call of its own (A/B)
        # True: the torus-exact mode (no reference counterpart).  The networks read every link angle as
        # [cos x | sin x] and the position sub-update scales on the circle (ops_periodic.lf_update_x_ncp), so the
        # proposal commutes with 2 pi shifts of any link and Metropolis-Hastings makes the wrapped chain exact for any
        # weights.  GenericNet only; runs layer by layer unless `whole_step` is set; with hmc=True there are no networks
        # and nothing changes.
        self.periodic = False
        # True (with periodic=True): the torus-exact mode's whole-step kernel (L2HMC_PLAN_PERIODIC_STEP) -- one launch
        # per trajectory or MCMC step where the plan has it (x_dim = 128 with a power-of-two space extent: 8x8, 4x16,
        # ...); any other lattice carries the flag and runs layer by layer.  Sampling only: training is unchanged.
        self.whole_step = False
        # True (with periodic=True): the tiled training entries take the torus-exact plan (L2HMC_PLAN_PERIODIC_TRAIN) --
        # GaugeTrainer and torch.autograd then run on l2hmc_gauge_train_* where every network width is a multiple of 32
        # (T * X a multiple of 16); any other lattice carries the flag and trains on the layered walk.  Training only:
        # every sampling entry ignores it, and it composes with `whole_step`.
        self.tiled_train = False
        # True (with periodic=True and tiled_train=True): the forward half of a training step is ONE launch of the
        # mode's whole-trajectory kernel, which writes the tape the tiled reverse pass reads (L2HMC_PLAN_PERIODIC_TAPE)
        # -- where the plan has the kernel (x_dim = 128 with a power-of-two space extent, H = 512); any other lattice
        # carries the flag and trains as without it.  Same arithmetic as `whole_step`'s kernel, so it differs from the
        # layer-by-layer forward in rounding.  Training only; it does not need `whole_step` and composes with it.
        self.fused_forward = False
        for key, val in kwargs.items():
            if key != 'eps':             # :73-75
                setattr(self, key, val)
        self.periodic = bool(self.periodic)
        self.whole_step = bool(self.whole_step)
        self.tiled_train = bool(self.tiled_train)
        self.fused_forward = bool(self.fused_forward)
        if self.fused_forward and not self.hmc and not (self.periodic and self.tiled_train):
            missing = [f"{k}=True" for k, on in (("periodic", self.periodic), ("tiled_train", self.tiled_train)) if not on]
            raise ValueError("fused_forward=True selects the taped whole-trajectory kernel of the torus-exact mode's "
                             "tiled training and needs " + " and ".join(missing) + " with it (the reference mode's "
                             "training forward is one launch already)")
        if self.tiled_train and not self.periodic and not self.hmc:
            raise ValueError("tiled_train=True opens the tiled training entries to the torus-exact mode and needs "
                             "periodic=True (the reference mode trains on them already)")
        if self.whole_step and not self.periodic and not self.hmc:
            raise ValueError("whole_step=True selects the whole-step kernel of the torus-exact mode and needs "
                             "periodic=True (the reference mode's one-launch step is `fused`, on by default)")
        if self.periodic and not self.hmc and self.network_arch == 'conv3D':
            raise NotImplementedError("periodic=True takes network_arch='generic' only: ConvNet3D has no front-end "
                                      "over [cos x | sin x]")
        self._device = kwargs.get('device') or torch.device("cuda", torch.cuda.current_device())
        if getattr(potential_fn, "u1_lattice", None) is None:
            raise NotImplementedError(
                "the fused trajectory integrates the 2D U(1) action; pass lattice.get_energy_function()")
        self.eps = torch.tensor(float(kwargs.get('eps', 0.4)), dtype=torch.float32)   # :91-96
        self._construct_time()
        self._construct_masks_while()
        if self.hmc:                     # :102-108
            self.position_fn = lambda inp: [torch.zeros_like(inp[0]) for _ in range(3)]
            self.momentum_fn = lambda inp: [torch.zeros_like(inp[0]) for _ in range(3)]
        elif self.network_arch == 'generic':
            self._build_generic_nets()
        elif self.network_arch == 'conv3D':
            self._build_conv_nets_3D()
        elif self.network_arch == 'conv2D':
            raise NotImplementedError(
                "network_arch='conv2D' is out of scope (SURVEY.md section 2: not named by any benchmark "
                "config, and its 4-D outputs break the reference's own reduce_sum(axis=1))")
        else:                            # :117-119
            raise AttributeError("`self._network_arch` must be one of `'conv3D', 'conv2D', 'generic'.`")
        self._ws = _lib.Workspace()
        self._seed = int(kwargs.get('seed', 42))
        self._draws = 0

    # ---- construction ------------------------------------------------------
    def _build_generic_nets(self):
        """:169-187."""
        kwargs = {'x_dim': self.x_dim, 'links_shape': self.lattice.links.shape,
                  'num_hidden': int(4 * self.x_dim), 'name_scope': 'position', 'factor': 2.}
        if self.periodic:                # XNet([v, m . x, t]): x is the second input; VNet([x, force, t]): the first
            kwargs['angle_input'] = 'second'
        self.position_fn = GenericNet(model_name='XNet', device=self._device, **kwargs)
        kwargs['factor'] = 1.
        kwargs['name_scope'] = 'momentum'
        if self.periodic:
            kwargs['angle_input'] = 'first'
        self.momentum_fn = GenericNet(model_name='VNet', device=self._device, **kwargs)

    def _build_conv_nets_3D(self):
        """:121-143."""
        kwargs = {
            '_input_shape': (self.batch_size, *self.lattice.links.shape),
            'links_shape': self.lattice.links.shape,
            'x_dim': self.lattice.num_links,
            'factor': 2.,
            'spatial_size': self.lattice.space_size,
            'num_hidden': 2 * self.lattice.num_links,
            'num_filters': int(self.lattice.space_size),
            'filter_sizes': [(3, 3, 2), (2, 2, 2)],
            'name_scope': 'position',
            'data_format': self.data_format,
        }
        self.position_fn = ConvNet3D(model_name='XNet', device=self._device, **kwargs)
        kwargs['name_scope'] = 'momentum'
        kwargs['factor'] = 1.
        self.momentum_fn = ConvNet3D(model_name='VNet', device=self._device, **kwargs)

    def _construct_time(self):
        """:611-619."""
        self.ts = [torch.tensor([[np.cos(2 * np.pi * i / self.num_steps),
                                  np.sin(2 * np.pi * i / self.num_steps)]], dtype=torch.float32)
                   for i in range(self.num_steps)]

    def _construct_masks_while(self):
        """:651-661 -- legacy global NumPy stream, like the reference."""
        mask_per_step = []
        for _ in range(self.num_steps):
            idx = npr.permutation(np.arange(self.x_dim))[:self.x_dim // 2]
            mask = np.zeros((self.x_dim,))
            mask[idx] = 1
            mask_per_step.append(mask)
        self.set_masks(np.stack(mask_per_step))

    def set_masks(self, masks):
        masks = np.asarray(masks, dtype=np.float32)
        if masks.shape != (self.num_steps, self.x_dim):
            raise ValueError(f"masks: expected {(self.num_steps, self.x_dim)}, got {masks.shape}")
        self.mask = _lib.as_dev(masks, self._device)

    @property
    def variables(self):
        v = [self.eps]
        if not self.hmc:
            v += self.position_fn.variables + self.momentum_fn.variables
        return v

    @property
    def trainable_variables(self):
        v = [self.eps] if self.eps_trainable else []
        if not self.hmc:
            v += self.position_fn.trainable_variables + self.momentum_fn.trainable_variables
        return v

    # ---- plumbing ----------------------------------------------------------
    def _plan(self):
        p = _lib.GaugePlan(T=self.lattice.time_size, X=self.lattice.space_size, num_steps=self.num_steps,
                           hmc=int(bool(self.hmc)), eps=float(self.eps.detach()),
                           flags=(0 if self.fused else _lib.PLAN_LAYERED)
                           | (0 if self.both_directions else _lib.PLAN_SELECTED_ONLY)
                           | (_lib.PLAN_RECOMPUTE if self.recompute else 0)
                           | (_lib.PLAN_TILES16_ONLY if self.tiles16_only else 0)
                           | (_lib.PLAN_ALL_COLUMNS if self.all_columns else 0)
                           | (_lib.PLAN_FULL_L1 if self.full_l1 else 0)
                           | (_lib.PLAN_SINGLE_KICKS if self.single_kicks else 0)
                           | (_lib.PLAN_PERIODIC if self.periodic and not self.hmc else 0)
                           | (_lib.PLAN_PERIODIC_STEP if self.whole_step and self.periodic and not self.hmc else 0)
                           | (_lib.PLAN_PERIODIC_TRAIN if self.tiled_train and self.periodic and not self.hmc else 0)
                           | (_lib.PLAN_PERIODIC_TAPE if self.fused_forward and self.tiled_train and self.periodic
                              and not self.hmc else 0),
                           masks=_lib.dev_ptr(self.mask, name="mask"))
        if not self.hmc:
            p.xnet = self.position_fn.pack()
            p.vnet = self.momentum_fn.pack()
            if self.network_arch == 'conv3D':
                p.flags |= _lib.PLAN_CONV3D
                p.xfront = self.position_fn.pack_front()
                p.vfront = self.momentum_fn.pack_front()
            elif self.fused:
                p.heads = self._heads_image(p)
        return p

    def _heads_image(self, plan):
        """l2hmc_gauge_pack_heads image of the plan's masks and XNet heads (the whole-step kernel's position
        sub-updates form S / T / Q on the columns they move), packed again whenever the masks or the weights change
        (set_masks, a rebuilt or refreshed XNet image: trainer steps, load_state, broadcasts); None if the plan has
        no such form."""
        L = _lib.lib()
        nbytes = L.l2hmc_gauge_pack_heads_bytes(C.byref(plan))
        if not nbytes:
            return None
        key = (plan.xnet.whd_t, getattr(self.position_fn, "_pack_serial", 0))
        h = getattr(self, "_heads", None)
        if h is None or h[0] is not self.mask or h[1] != key or h[2].numel() * 4 < nbytes:
            buf = torch.empty(nbytes // 4, dtype=torch.float32, device=self._device)
            _lib.call("l2hmc_gauge_pack_heads", C.byref(plan), buf, device=self._device)
            self._heads = h = (self.mask, key, buf)
        return h[2].data_ptr()

    def _x(self, a):
        """The ONE gate for positions and momenta -> a float32 device tensor [rows, x_dim].  [B, x_dim] passes, and so
        does any [B, ...] whose trailing extents multiply to x_dim ([B, T, X, 2]).  ValueError otherwise
        (`_lib.expect_shape`), before the value is copied anywhere: every kernel behind this object reads x_dim floats
        per row, whatever the tensor holds.  The methods come through `_gate`, which names the argument and its method
        and fixes a momentum's rows to its position's."""
        _lib.expect_shape(a, (None, self.x_dim), "position", "GaugeDynamics", fold=True)
        a = _lib.as_dev(a, self._device)
        return a if a.ndim == 2 else a.reshape(a.shape[0], -1)

    def _normal(self, shape):
        out = ops.fill_normal(shape, self._seed, self._draws, self._device)
        self._draws += 1
        return out

    def _uniform(self, shape):
        out = ops.fill_uniform(shape, self._seed, self._draws, self._device)
        self._draws += 1
        return out

    def _beta(self, beta, B):
        """`beta` of a transition -> (beta, None) for one value (untouched: the scalar call reads float(beta) as it
        always did), or (None, the ladder as a float32 device tensor [B]) for [B] / [1, B] (`_runs.per_chain`: a
        float32 tensor of that shape on the device stays there, unchecked).  Host-side, before any draw."""
        size = beta.numel() if isinstance(beta, torch.Tensor) else np.size(beta)
        if _runs.ndim(beta) == 0 or (size == 1 and B != 1):      # (one value in brackets: float() takes it, as before)
            return beta, None
        who = "GaugeDynamics.apply_transition"
        if isinstance(beta, torch.Tensor) and beta.requires_grad:
            raise ValueError(f"{who}: the beta ladder requires grad; its values are not differentiated (detach it)")
        if self.hmc:
            raise NotImplementedError(f"{who}: a beta per chain on hmc=True dynamics: GaugeSampler.run_hmc runs plain "
                                      "HMC on a ladder (l2hmc_gauge_hmc_run_ladder)")
        return None, _runs.per_chain(beta, B, self._device, who=who, name="beta", sign="not negative")[0]

    def _dir(self, rows, backward):
        return torch.full((rows,), int(backward), dtype=torch.int32, device=self._device)

    # ---- public operator surface -------------------------------------------
    def __call__(self, position, beta, **draws):
        return self.apply_transition(position, beta, **draws)

    call = __call__

    def apply_transition(self, position, beta, momentum_f=None, momentum_b=None, coin=None, u=None):
        """:195-259 -> (position_post, momentum_post, accept_prob, position_out).  Differentiable (torch.autograd,
        l2hmc_amd/autograd.py) when grad mode is on and the position, eps or a weight requires grad.

        beta: a scalar, or one value per chain, [B] or [1, B] (a ladder of a replica-exchange run): chain i runs, and
        is differentiated, at beta[i], with the bits of the scalar call at that value; draws and the draw counter are
        the scalar call's.  The ladder's values are NOT differentiated.  Without a graph the ladder call takes the
        draws of `l2hmc_gauge_transition_draw` with fill_normal / fill_uniform and runs LAYER BY LAYER
        (l2hmc_gauge_transition_ladder) whatever `fused` says: `GaugeSampler.step` is the one-launch ladder step.
        Refused before any draw is taken: ValueError for a ladder of another shape, with an entry that in float32 is
        not finite or is negative, or that requires grad; NotImplementedError for a ladder on hmc=True."""
        who = "GaugeDynamics.apply_transition"
        x = _gate(self, position, "position", who)
        _autograd.check_draws(self, x.shape[0], momentum_f, momentum_b, coin, u, who)     # all three branches below
        beta, ladder = self._beta(beta, x.shape[0])
        if _autograd.wants_grad(self, x):
            return _autograd.transition(self, x, float(beta) if ladder is None else ladder, momentum_f, momentum_b,
                                        coin, u)
        B, D = x.shape
        if ladder is not None:
            v0f, v0b, coin, u = _autograd.draws(self, B, D, x.device, momentum_f, momentum_b, coin, u)
            x_prop, v_prop, x_out = (torch.empty_like(x) for _ in range(3))
            p = torch.empty(B, dtype=torch.float32, device=x.device)
            plan, L = self._plan(), _lib.lib()
            both = int(bool(self.both_directions))
            ws, nb = self._ws.get(L.l2hmc_gauge_transition_ws_bytes(C.byref(plan), B, both), x.device)
            _lib.call("l2hmc_gauge_transition_ladder", C.byref(plan), ladder, 1, x, v0f.contiguous(), v0b.contiguous(),
                      coin, u, B, both, x_prop, v_prop, p, x_out, ws, nb, device=self._device)
            if self.check_numerics and not bool(torch.isfinite(x_prop).all() & torch.isfinite(v_prop).all()):
                raise FloatingPointError("check_numerics: non-finite value in the proposed configuration")
            return x_prop, v_prop, p, x_out
        if momentum_f is None and momentum_b is None and coin is None and u is None:
            # no draw injected: the library draws for itself (one stream pair from this object's counter, the
            # layout of the native MCMC step) -- one kernel launch where the plan has a whole-trajectory kernel
            # (GenericNet / ConvNet3D on 8x8-site lattices; hmc=True on any lattice of up to 1024 sites)
            x_prop, v_prop, x_out = (torch.empty_like(x) for _ in range(3))
            p = torch.empty(B, dtype=torch.float32, device=x.device)
            plan, L = self._plan(), _lib.lib()
            ws, nb = self._ws.get(L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B), x.device)
            draw, self._draws = _lib.step_draw_index(self._draws)
            _lib.call("l2hmc_gauge_transition_draw", C.byref(plan), float(beta), x, B, self._seed, draw, x_prop,
                      v_prop, p, x_out, ws, nb, device=self._device)
            if self.check_numerics and not bool(torch.isfinite(x_prop).all() & torch.isfinite(v_prop).all()):
                raise FloatingPointError("check_numerics: non-finite value in the proposed configuration")
            return x_prop, v_prop, p, x_out
        v0f = _gate(self, momentum_f, "momentum_f", who, B) if momentum_f is not None else self._normal((B, D))
        v0b = _gate(self, momentum_b, "momentum_b", who, B) if momentum_b is not None else self._normal((B, D))
        coin = _lib.as_dev(coin, self._device) if coin is not None else self._uniform((B,))
        u = _lib.as_dev(u, self._device) if u is not None else self._uniform((B,))
        x_prop, v_prop, x_out = (torch.empty_like(x) for _ in range(3))
        p = torch.empty(B, dtype=torch.float32, device=x.device)
        plan, L = self._plan(), _lib.lib()
        both = int(bool(self.both_directions))
        ws, nb = self._ws.get(L.l2hmc_gauge_transition_ws_bytes(C.byref(plan), B, both), x.device)
        _lib.call("l2hmc_gauge_transition", C.byref(plan), float(beta), x, v0f, v0b, coin, u, B, both, x_prop, v_prop,
                  p, x_out, ws, nb, device=self._device)
        if self.check_numerics and not bool(torch.isfinite(x_prop).all() & torch.isfinite(v_prop).all()):
            # the reference wraps every exp of the sub-updates in tf.check_numerics and aborts the step;
            # the kernels propagate NaN / inf instead, and this opt-in check (one host sync) reports it
            raise FloatingPointError("check_numerics: non-finite value in the proposed configuration")
        return x_prop, v_prop, p, x_out

    def transition_kernel(self, position, beta, forward=True, momentum=None, return_logdet=False):
        """:261-313 -> (position_post, momentum_post, accept_prob)."""
        who = "GaugeDynamics.transition_kernel"
        x = _gate(self, position, "position", who)
        rows, D = x.shape
        v0 = _gate(self, momentum, "momentum", who, rows) if momentum is not None else self._normal((rows, D))
        x_out, v_out = torch.empty_like(x), torch.empty_like(x)
        sld = torch.empty(rows, dtype=torch.float32, device=x.device)
        p = torch.empty_like(sld)
        plan, L = self._plan(), _lib.lib()
        dirs = None if forward else self._dir(rows, True)
        ws, nb = self._ws.get(L.l2hmc_gauge_ws_bytes(C.byref(plan), rows), x.device)
        _lib.call("l2hmc_gauge_trajectory", C.byref(plan), float(beta), x, v0, dirs, rows, x_out, v_out, sld, p, ws, nb,
                  device=self._device)
        if return_logdet:
            return x_out, v_out, p, sld
        return x_out, v_out, p

    def _lf(self, position, momentum, beta, step, backward, step_end=None):
        """Leapfrog step `step` (or the steps [step, step_end) in one call) -> (x, v, log-det)."""
        x = _gate(self, position, "position", "GaugeDynamics._lf")
        rows = x.shape[0]
        x, v = x.clone(), _gate(self, momentum, "momentum", "GaugeDynamics._lf", rows).clone()
        logdet = torch.zeros(rows, dtype=torch.float32, device=x.device)
        plan, L = self._plan(), _lib.lib()
        dirs = self._dir(rows, True) if backward else None
        ws, nb = self._ws.get(L.l2hmc_gauge_ws_bytes(C.byref(plan), rows), x.device)
        _lib.call("l2hmc_gauge_leapfrog_steps", C.byref(plan), float(beta), int(step),
                  int(step + 1 if step_end is None else step_end), x, v, dirs, rows, logdet, ws, nb, device=self._device)
        return x, v, logdet

    def _forward_lf(self, position, momentum, beta, step):
        """:412-445."""
        return self._lf(position, momentum, beta, step, backward=False)

    def _backward_lf(self, position, momentum, beta, step):
        """:447-483 -- the time/mask index is num_steps - step - 1, reversed inside as there."""
        return self._lf(position, momentum, beta, step, backward=True)

    # sub-updates on materialised S/T/Q (the fused trajectory never materialises them)
    def _stq(self, fn, a, b, t):
        return fn([a, b, t])

    def _update_momentum(self, position, momentum, beta, t, backward):
        x = _gate(self, position, "position", "GaugeDynamics._update_momentum")
        v = _gate(self, momentum, "momentum", "GaugeDynamics._update_momentum", x.shape[0])
        grad = self.grad_potential(x, beta)
        S, T, Q = self._stq(self.momentum_fn, self._net_x(x), grad, t)           # :493-495
        return ops.lf_update_v(v, grad, self._x(S), self._x(T), self._x(Q), self.eps, backward)

    def _update_momentum_forward(self, position, momentum, beta, t):
        """:486-508."""
        return self._update_momentum(position, momentum, beta, t, False)

    def _update_momentum_backward(self, position, momentum, beta, t):
        """:537-561."""
        return self._update_momentum(position, momentum, beta, t, True)

    def _update_position(self, position, momentum, t, mask, mask_inv, backward):
        who = "GaugeDynamics._update_position"
        x = _gate(self, position, "position", who)
        v = _gate(self, momentum, "momentum", who, x.shape[0])
        keep = _lib.as_dev(mask, self._device).reshape(-1)       # (its length: ops.lf_update_x checks `keep`)
        if self.periodic and not self.hmc:
            S, T, Q = self._stq(self.position_fn, v, keep.repeat(2)[None, :] * self._net_x(x), t)
            return ops_periodic.lf_update_x_ncp(x, v, keep, self._x(S), self._x(T), self._x(Q), self.eps, backward)
        S, T, Q = self._stq(self.position_fn, v, keep[None, :] * x, t)   # :515-517
        return ops.lf_update_x(x, v, keep, self._x(S), self._x(T), self._x(Q), self.eps, backward)

    def _net_x(self, x):
        """A configuration as the networks read it: x itself, or [cos x | sin x] on a periodic dynamics."""
        return ops_periodic.u1_angle_features(x) if self.periodic and not self.hmc else x

    def _update_position_forward(self, position, momentum, t, mask, mask_inv):
        """:511-534."""
        return self._update_position(position, momentum, t, mask, mask_inv, False)

    def _update_position_backward(self, position, momentum, t, mask, mask_inv):
        """:565-590."""
        return self._update_position(position, momentum, t, mask, mask_inv, True)

    def _compute_accept_prob(self, position, momentum, position_post, momentum_post, sumlogdet, beta):
        """:592-609."""
        who = "GaugeDynamics._compute_accept_prob"
        x = _gate(self, position, "position", who)
        rows = x.shape[0]
        v = _gate(self, momentum, "momentum", who, rows)
        x1 = _gate(self, position_post, "position_post", who, rows)
        v1 = _gate(self, momentum_post, "momentum_post", who, rows)
        _lib.expect_shape(sumlogdet, (rows,), "sumlogdet", who)
        old = self.hamiltonian(x, v, beta)
        new = self.hamiltonian(x1, v1, beta)
        return ops.accept_prob(old, new, _lib.as_dev(sumlogdet, self._device))

    def _get_time(self, i):
        return self.ts[i]

    def _format_time(self, i, tile=1):
        """:625-633 -> [tile, 2] (cos, sin) of 2 pi i / num_steps in fp32."""
        arg = np.float32(2 * np.pi) * np.float32(i) / np.float32(self.num_steps)
        t = torch.tensor([[np.cos(arg), np.sin(arg)]], dtype=torch.float32)
        return t.repeat(tile, 1)

    def _get_mask_while(self, step):
        """:671-673."""
        m = self.mask[int(step)]
        return m, 1. - m

    def potential_energy(self, position, beta):
        """:675-681."""
        return float(beta) * self.potential(_gate(self, position, "position", "GaugeDynamics.potential_energy"))

    def kinetic_energy(self, v):
        """:683-689."""
        return ops.kinetic_energy(_gate(self, v, "v", "GaugeDynamics.kinetic_energy"))

    def hamiltonian(self, position, momentum, beta):
        """:691-696."""
        return self.potential_energy(position, beta) + self.kinetic_energy(momentum)

    def grad_potential(self, position, beta, check_numerics=True):
        """:698-709 -- closed form of the autodiff the reference runs."""
        return self.lattice.grad_action(_gate(self, position, "position", "GaugeDynamics.grad_potential"), beta)
