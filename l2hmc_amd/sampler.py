"""Sampler glue with the reference's signatures (l2hmc/utils/sampler.py:28-59).
Random draws (direction bits, MH uniforms, momenta) come from the library's
Philox stream unless injected through the keyword-only arguments."""
import ctypes as C

import torch

from . import _lib, ops
from . import autograd_toy as _autograd


def _uniform(dynamics, n):
    out = ops.fill_uniform(n, dynamics._seed, dynamics._draws, dynamics._device)
    dynamics._draws += 1
    return out


def tf_accept(x, Lx, px, u=None, dynamics=None):
    """:57-59 -- accept iff px - u >= 0."""
    _lib.expect_shape(x, (None, None), "x", "tf_accept")
    _lib.expect_shape(Lx, tuple(x.shape), "Lx", "tf_accept")
    for name, t in (("px", px), ("u", u)):
        _lib.expect_shape(t, (x.shape[0],), name, "tf_accept")
    x, Lx, px = (_lib.as_dev(t) for t in (x, Lx, px))
    u = _lib.as_dev(u) if u is not None else _uniform(dynamics, px.numel())
    # forward slot carries Lx with coin=1; strict=0 selects the sampler.py comparison
    return ops.mix_accept(x, Lx, Lx, px, Lx, Lx, px, torch.ones_like(px), u, 0, want_proposal=False)[3]


def _check_draws(x, init_v, init_v_backward, dir_bits, u):
    """`propose`'s injected draws against x [rows, x_dim] (None: not injected): momenta [rows, x_dim], direction bits
    and uniforms (rows,).  ValueError (`_lib.expect_shape`), on the host, before any draw."""
    for name, v in (("init_v", init_v), ("init_v_backward", init_v_backward)):
        _lib.expect_shape(v, tuple(x.shape), name, "propose")
    for name, t in (("dir_bits", dir_bits), ("u", u)):
        _lib.expect_shape(t, (x.shape[0],), name, "propose")


def propose(x, dynamics, init_v=None, aux=None, do_mh_step=False, log_jac=False, *,
            init_v_backward=None, dir_bits=None, u=None, temperature=None):
    """:28-55 -> (Lx, Lv, px, outputs).  Differentiable (torch.autograd, l2hmc_amd/autograd_toy.py) when grad mode
    is on and x, init_v, init_v_backward, dynamics.alpha or a network weight requires grad: Lx, Lv, px and
    outputs[0] then carry a graph.  The draws are the ones the no-grad call takes.  Each chain's gradient flows
    through the direction its bit picks only; the other direction is multiplied by an exact 0 (:35-41).

    temperature: None = the call as it is; a scalar = this call at that temperature, on a copy of the plan
    (`dynamics.temperature` stays); [B] or [1, B] = a ladder: chain i at temperature[i] in both of its directions, with
    the bits of the scalar call at that value.  With a graph the ladder runs through l2hmc_small_trajectory_tempered
    and l2hmc_small_vjp_tempered; without one piecewise (`Dynamics.both` + mix_accept) on the Philox streams
    l2hmc_small_propose takes.  The temperatures are NOT differentiated.  Refused before any draw: what
    `Dynamics.forward` refuses."""
    x = _lib.as_dev(x, dynamics._device)
    _check_draws(x.reshape(-1, dynamics.x_dim), init_v, init_v_backward, dir_bits, u)
    temp = None
    if temperature is not None:
        temp = dynamics._call_temperature(temperature, x.reshape(-1, dynamics.x_dim).shape[0], "propose")
    ladder = isinstance(temp, torch.Tensor)
    if _autograd.wants_grad(dynamics, x, init_v, init_v_backward):
        _autograd.check_differentiable(dynamics)          # before any draw
        if aux is not None:
            raise NotImplementedError("aux inputs are only used by the out-of-scope VAE scripts")
        return _propose_grad(x, dynamics, init_v, do_mh_step, log_jac, init_v_backward, dir_bits, u, temp)
    if dynamics.hmc:
        Lx, Lv, px = dynamics.forward(x, init_v=init_v, aux=aux, temperature=temp)
        return Lx, Lv, px, [tf_accept(x, Lx, px, u, dynamics)]
    B = x.shape[0]
    if aux is not None:
        raise NotImplementedError("aux inputs are only used by the out-of-scope VAE scripts")
    if (init_v is None and init_v_backward is None and dir_bits is None and u is None and not log_jac
            and not dynamics.layered and not ladder):
        # every draw is the library's: ONE launch (direction bit, both momenta, both trajectories, mix, MH);
        # same Philox streams, same numbers as the piecewise path below
        x = x.reshape(-1, dynamics.x_dim).contiguous()
        Lx, px = torch.empty_like(x), torch.empty(B, dtype=torch.float32, device=x.device)
        out = torch.empty_like(x) if do_mh_step else None
        plan = dynamics._plan(temp)
        _lib.call("l2hmc_small_propose", C.byref(plan), x, B, dynamics._seed, dynamics._draws, Lx, None, px, out,
                  device=x.device)
        dynamics._draws += 4 if do_mh_step else 3
        return Lx, None, px, ([out] if do_mh_step else [])       # Lv is None without init_v (:43-45, quirk Q6)
    if dir_bits is None:
        mask = (_uniform(dynamics, B) >= 0.5).to(torch.float32)     # randint{0,1}
    else:
        mask = _lib.as_dev(dir_bits, dynamics._device)
    vb = init_v_backward if init_v_backward is not None else init_v
    (Lx1, Lv1, px1), (Lx2, Lv2, px2) = dynamics.both(x, init_v, vb, log_jac=log_jac,
                                                     temperature=temp)                # one launch, both directions
    if do_mh_step and u is None:
        u = _uniform(dynamics, B)
    u = None if u is None else _lib.as_dev(u, dynamics._device)
    Lx, Lvm, px, out = ops.mix_accept(x, Lx1, Lv1, px1, Lx2, Lv2, px2, mask, u, 0, want_out=do_mh_step)
    Lv = Lvm if init_v is not None else None       # :43-45 (quirk Q6)
    outputs = [out] if do_mh_step else []
    return Lx, Lv, px, outputs


def _propose_grad(x, dynamics, init_v, do_mh_step, log_jac, init_v_backward, dir_bits, u, temp=None):
    """The L2HMC branch with an autograd graph.  Draws in the order of the piecewise path below, which are the
    Philox streams of l2hmc_small_propose: direction bits (draw0), forward momenta (draw0 + 1), backward momenta
    (draw0 + 2), MH uniforms (draw0 + 3)."""
    dev = dynamics._device
    x = x.reshape(-1, dynamics.x_dim)
    B = x.shape[0]
    _check_draws(x, init_v, init_v_backward, dir_bits, u)
    mask = (_uniform(dynamics, B) >= 0.5).to(torch.float32) if dir_bits is None else _lib.as_dev(dir_bits, dev)
    vf = _lib.as_dev(init_v, dev) if init_v is not None else dynamics._normal(tuple(x.shape))
    vb = init_v_backward if init_v_backward is not None else init_v
    vb = _lib.as_dev(vb, dev) if vb is not None else dynamics._normal(tuple(x.shape))
    if do_mh_step and u is None:
        u = _uniform(dynamics, B)
    Lx, Lvm, px, out = _autograd.propose(dynamics, x, vf, vb, mask, _lib.as_dev(u, dev) if do_mh_step else None,
                                         log_jac, temp)
    Lv = Lvm if init_v is not None else None       # :43-45 (quirk Q6)
    return Lx, Lv, px, ([out] if do_mh_step else [])
