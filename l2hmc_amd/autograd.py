"""torch.autograd through a GaugeDynamics transition: what tf.gradients(loss,
dynamics.variables) gives the reference for ANY loss its caller writes around `dynamics(x, beta)`
(gauge_model.py:799-832), on the HIP training entries of include/l2hmc_hip.h:

  forward   l2hmc_gauge_train_forward     each chain in the direction its coin picks, every intermediate taped
            x_out = where(p > u, x_N, x)  the Metropolis-Hastings select (gauge_dynamics.py:244-257)
  backward  l2hmc_gauge_accept_backward   cotangents of (x_prop, v_prop, p, x_out) -> d(x_N, v_N, sumlogdet)
                                          and the direct part of d(x)
            l2hmc_gauge_train_backward    -> weight, step-size and start-state gradients through the trajectory

With a beta per chain (`dyn(x, ladder)`, ladder [B]) the same three steps run on the `_ladder` entries
(l2hmc_gauge_train_forward_ladder, l2hmc_gauge_accept_backward_ladder, l2hmc_gauge_train_backward_ladder; chains = B,
stride 1): chain i is differentiated at ladder[i], with the bits of the scalar call at that value.  The ladder's values
are not differentiated.

A torus-exact dynamics (`periodic=True`) is differentiated only with `tiled_train=True` (L2HMC_PLAN_PERIODIC_TRAIN), where
the same entries take its plan; without the flag, or at widths that are no multiples of 32, it is refused.  With
`fused_forward=True` (L2HMC_PLAN_PERIODIC_TAPE) the forward of step 1 is one taped launch where the plan has the kernel.

Every call owns its tape (a train workspace), the plan and the packed weight buffers it ran with, so several
transitions may be differentiated by one backward (the reference loss runs two: x and z).  The tape is freed
after the backward; a second backward through the same graph is an error."""
import ctypes as C

import torch

from . import _lib, ops


def _nets(dyn):
    return (("position_fn", dyn.position_fn), ("momentum_fn", dyn.momentum_fn))


def wants_grad(dyn, x):
    """True when `dyn(x, beta)` has to record a graph: grad mode is on and the position, the step size or a
    reference-layout weight requires grad.  Host-side only."""
    if not torch.is_grad_enabled():
        return False
    if x.requires_grad or dyn.eps.requires_grad:
        return True
    if dyn.hmc:
        return False
    return any(getattr(net, "_flat", None) is None and any(t.requires_grad for t in net._ref_tensors())
               for _, net in _nets(dyn))


def check_differentiable(dyn):
    """Refuse, before any launch, what the training entries do not take."""
    if dyn.hmc:
        raise NotImplementedError("autograd through GaugeDynamics: hmc=True dynamics have no networks; the "
                                  "training entries take L2HMC plans only")
    # (tiled_train=True -- L2HMC_PLAN_PERIODIC_TRAIN -- lets the mode through to the width check below)
    if getattr(dyn, "periodic", False) and not getattr(dyn, "tiled_train", False):
        raise NotImplementedError("autograd through GaugeDynamics: periodic=True dynamics have no tiled training "
                                  "entries; they would need the layered reverse walk, which torch.autograd is refused "
                                  "at today for every shape whose widths are no multiples of 32 (GaugeTrainer trains "
                                  "them)")
    for name, net in _nets(dyn):
        if getattr(net, "_flat", None) is not None:
            raise ValueError(f"autograd through GaugeDynamics: a GaugeTrainer owns the weights of {name} (flat master "
                             "copy); differentiate a dynamics object of your own (load_state(state_dict()))")
        la, lb, _, lh, ls = net._layers()[:5]
        widths = dict(D=ls.kernel.shape[1], H=lh.kernel.shape[0], Ka=la.kernel.shape[0], Kb=lb.kernel.shape[0])
        if any(w % 32 for w in widths.values()):
            raise ValueError(f"autograd through GaugeDynamics: {name} has widths {widths}; the training kernels need "
                             "multiples of 32 (a T x X lattice has D = 2*T*X)")


def check_draws(dyn, B, momentum_f=None, momentum_b=None, coin=None, u=None, who="GaugeDynamics.apply_transition"):
    """Refuse injected draws that do not fit B chains (None: not injected): the momenta go through the dynamics'
    position gate with the position's rows, coin and u are (B,).  Shapes only, on the host, before any draw."""
    for name, v in (("momentum_f", momentum_f), ("momentum_b", momentum_b)):
        _lib.expect_shape(v, (B, dyn.x_dim), name, who, fold=True)
    for name, c in (("coin", coin), ("u", u)):
        _lib.expect_shape(c, (B,), name, who)


def draws(dyn, B, D, dev, momentum_f=None, momentum_b=None, coin=None, u=None):
    """(v0_f, v0_b, coin, u) of a transition: the library's own where none is injected, else the injected ones and
    single streams of the counter for the rest."""
    check_draws(dyn, B, momentum_f, momentum_b, coin, u)
    if momentum_f is None and momentum_b is None and coin is None and u is None:
        # the draws of l2hmc_gauge_transition_draw: (seed, 2d) = [v0_f; v0_b], (seed, 2d+1) = coin | u
        d, dyn._draws = _lib.step_draw_index(dyn._draws)
        V = ops.fill_normal(2 * B * D, dyn._seed, 2 * d, dev)
        cu = ops.fill_uniform(2 * B, dyn._seed, 2 * d + 1, dev)
        v0f, v0b, coin, u = V[:B * D].view(B, D), V[B * D:].view(B, D), cu[:B], cu[B:]
    else:
        v0f = dyn._x(momentum_f) if momentum_f is not None else dyn._normal((B, D))
        v0b = dyn._x(momentum_b) if momentum_b is not None else dyn._normal((B, D))
        coin = _lib.as_dev(coin, dyn._device) if coin is not None else dyn._uniform((B,))
        u = _lib.as_dev(u, dyn._device) if u is not None else dyn._uniform((B,))
    return v0f, v0b, coin, u


def transition(dyn, x, beta, momentum_f=None, momentum_b=None, coin=None, u=None):
    """Differentiable apply_transition -> (x_prop, v_prop, p_accept, x_out).  `x`: [B, D] fp32 on dyn's device; `beta`:
    a float, or the ladder [B] as a float32 tensor on that device (chain i at beta[i]; not differentiated)."""
    check_differentiable(dyn)
    B, D = x.shape
    v0f, v0b, coin, u = draws(dyn, B, D, x.device, momentum_f, momentum_b, coin, u)
    xs, vs = dyn.position_fn.state_dict(), dyn.momentum_fn.state_dict()
    out = _Transition.apply(dyn, beta, list(xs), list(vs), x, v0f.detach(), v0b.detach(), coin.detach(),
                            u.detach(), dyn.eps, *xs.values(), *vs.values())
    if dyn.check_numerics and not bool(torch.isfinite(out[0]).all() & torch.isfinite(out[1]).all()):
        raise FloatingPointError("check_numerics: non-finite value in the proposed configuration")
    return out


def _grad_buffers(bufs, keys):
    return {k: torch.zeros_like(bufs[k]) for k in keys}


class _Transition(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dyn, beta, xnames, vnames, x, v0f, v0b, coin, u, eps, *weights):
        B = x.shape[0]
        x = x.contiguous()
        fwd = coin > 0.5                                  # gauge_dynamics.py:223-226
        v0 = torch.where(fwd[:, None], v0f, v0b).contiguous()
        dirs = (~fwd).to(torch.int32).contiguous()
        plan, L = dyn._plan(), _lib.lib()
        nets = [net for _, net in _nets(dyn)]
        nbytes = max(int(L.l2hmc_gauge_train_ws_bytes(C.byref(plan), B)), 256)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        xN, vN = torch.empty_like(x), torch.empty_like(x)
        sld, p = (torch.empty(B, dtype=torch.float32, device=x.device) for _ in range(2))
        ladder = isinstance(beta, torch.Tensor)           # [B] on the device: chain i at beta[i]
        if ladder:
            _lib.call("l2hmc_gauge_train_forward_ladder", C.byref(plan), beta, 1, B, x, v0, dirs, B, xN, vN, sld, p, ws,
                      nbytes, device=x.device)
        else:
            _lib.call("l2hmc_gauge_train_forward", C.byref(plan), beta, x, v0, dirs, B, xN, vN, sld, p, ws, nbytes,
                      device=x.device)
        x_out = torch.where((p > u)[:, None], xN, x)      # strict >, gauge_dynamics.py:244-257
        ctx.save_for_backward(x, v0, xN, vN, p, u, eps, *weights)
        ctx.set_materialize_grads(False)
        # the tape and what the plan points at stay alive until the backward
        ctx.dyn, ctx.beta, ctx.names, ctx.plan, ctx.ws, ctx.dirs = dyn, beta, (xnames, vnames), plan, ws, dirs
        ctx.mask = dyn.mask
        ctx.bufs = [net._packed[1] for net in nets]
        ctx.front = [getattr(net, "_front_bufs", None) if dyn.network_arch == 'conv3D' else None for net in nets]
        return xN, vN, p, x_out

    @staticmethod
    def backward(ctx, g_xprop, g_vprop, g_p, g_xout):
        if ctx.ws is None:
            raise RuntimeError("GaugeDynamics transition: backward ran twice through the same graph; the transition's "
                               "tape is freed by the first backward")
        saved = ctx.saved_tensors          # raises if a weight or input was modified in place since the forward
        x, v0, xN, vN, p, u, eps = saved[:7]
        dyn, plan = ctx.dyn, ctx.plan
        B = x.shape[0]
        dev = x.device
        T, X = dyn.lattice.time_size, dyn.lattice.space_size
        gs = [None if t is None else t.contiguous() for t in (g_xprop, g_vprop, g_p, g_xout)]
        dxN, dvN = torch.empty_like(x), torch.empty_like(x)
        dld = torch.empty(B, dtype=torch.float32, device=dev)
        dx0 = torch.empty_like(x) if ctx.needs_input_grad[4] else None
        ladder = isinstance(ctx.beta, torch.Tensor)
        if ladder:
            _lib.call("l2hmc_gauge_accept_backward_ladder", T, X, ctx.beta, 1, B, B, x, v0, xN, vN, p, u, *gs,
                      dxN, dvN, dld, dx0, None, device=dev)
        else:
            _lib.call("l2hmc_gauge_accept_backward", T, X, ctx.beta, B, x, v0, xN, vN, p, u, *gs, dxN, dvN, dld, dx0,
                      None, device=dev)
        nets = [net for _, net in _nets(dyn)]
        keys = _lib.DenseGrads._fields_
        dense = [_grad_buffers(b, [k for k, _ in keys]) for b in ctx.bufs]
        conv = [None if f is None else _grad_buffers(f, list(f)) for f in ctx.front]
        deps = torch.zeros(1, dtype=torch.float32, device=dev)
        if B > 0:
            gstruct = [_lib.DenseGrads(**{k: v.data_ptr() for k, v in g.items()}) for g in dense]
            cstruct = [None if g is None else _lib.Conv3DGrads(**{k: v.data_ptr() for k, v in g.items()}) for g in conv]
            tail = (C.byref(gstruct[0]), C.byref(gstruct[1]), *(None if c is None else C.byref(c) for c in cstruct),
                    deps, ctx.ws, ctx.ws.numel())
            if ladder:                     # (its bucket callback may be NULL)
                _lib.call("l2hmc_gauge_train_backward_ladder", C.byref(plan), ctx.beta, 1, B, ctx.dirs, B, dxN, dvN, dld,
                          *tail, device=dev, tail=(_lib.BUCKET_FN(), None))
            else:
                _lib.call("l2hmc_gauge_train_backward", C.byref(plan), ctx.beta, ctx.dirs, B, dxN, dvN, dld, *tail,
                          device=dev)
        else:
            dxN.zero_()
        ctx.ws = ctx.plan = ctx.bufs = ctx.front = ctx.mask = ctx.dyn = ctx.beta = None
        grad_x = dx0 + dxN if dx0 is not None else None
        wgrads = []
        for net, names, g, c in zip(nets, ctx.names, dense, conv):
            named = net.unpack_grads({**g, **(c or {})})
            wgrads += [named[n] for n in names]
        grad_eps = deps.reshape(eps.shape).to(eps.device)
        return (None, None, None, None, grad_x, None, None, None, None, grad_eps, *wgrads)
