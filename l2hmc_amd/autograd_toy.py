"""torch.autograd through the one-launch toy-target trajectories: what
tf.gradients(loss, dynamics.variables) gives the reference for ANY loss its caller writes around
`dynamics.forward / .backward` or `propose` (mog_model.py:324-363), on the HIP entries of include/l2hmc_hip.h:

  forward   l2hmc_small_trajectory   the launch the no-grad path runs, so the values are the same bits
  backward  l2hmc_small_vjp          the forward recomputed on-chip, then the reverse pass seeded by the cotangents of
                                     (x_N, v_N, sumlogdet, p): weight, step-size and start-state gradients

With a temperature per chain (`temperature=` of Dynamics.forward / .backward / propose, a ladder [B]) the two
launches are l2hmc_small_trajectory_tempered and l2hmc_small_vjp_tempered: chain i, in both of its directions, runs and
is differentiated at temperature[i] with the bits of the scalar call at that value.  The ladder's values are not
differentiated.

`propose` integrates every chain in both directions and keeps one (sampler.py:35-41 multiplies the other by an
exact 0, as DynamicsTrainer does): the backward runs only the kept rows, and the unselected direction's start
state gets no gradient.  Each call keeps the packed weight buffers and the masks it ran with until its backward;
the reference-layout weights are saved, so an in-place edit between forward and backward raises."""
import ctypes as C

import torch

from . import _lib


def _nets(dyn):
    return (("XNet", dyn.XNet), ("VNet", dyn.VNet))


def wants_grad(dyn, *inputs):
    """True when a call on `dyn` has to record a graph: grad mode is on and one of `inputs` (the position, an
    initial momentum; None allowed), the step size or a reference-layout weight requires grad.  Host-side only."""
    if not torch.is_grad_enabled():
        return False
    if any(t is not None and isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
        return True
    if dyn.alpha.requires_grad:
        return True
    if dyn.hmc:
        return False
    return any(getattr(net, "_flat", None) is None and any(t.requires_grad for t in net._ref_tensors())
               for _, net in _nets(dyn))


def check_differentiable(dyn):
    """Refuse, before any launch (and before any draw), what l2hmc_small_vjp does not take."""
    if dyn.hmc:
        raise NotImplementedError("autograd through Dynamics: hmc=True dynamics have no networks and the step size "
                                  "is not differentiated; call it under torch.no_grad() or without requires_grad")
    if dyn.layered:
        raise NotImplementedError("autograd through Dynamics: this Dynamics runs layer by layer (arbitrary energy "
                                  "function, x_dim > 8 or more than 64 hidden units); only the one-launch toy targets "
                                  "(l2hmc_amd.GMM / Gaussian / RoughWell / GaussianFunnel, x_dim <= 8, num_nodes <= 64) are differentiable")
    for name, net in _nets(dyn):
        if getattr(net, "_flat", None) is not None:
            raise ValueError(f"autograd through Dynamics: a DynamicsTrainer owns the weights of {name} (flat master "
                             "copy); differentiate a dynamics object of your own (load_state(state_dict()))")


def trajectory(dyn, x0, v0, dirs=None, sel=None, temp=None):
    """Differentiable l2hmc_small_trajectory -> (X, V, sumlogdet, p) of the rows `sel` (LongTensor; None = all).
    x0, v0: [R, x_dim] fp32 on dyn's device; dirs: [R] int32 (1 = backward) or None (all forward).  temp: None (the
    dynamics' own temperature), a float (this call's, on a copy of the plan), or a ladder, a float32 device tensor [C]
    with R a multiple of C: row r at temp[r % C] (l2hmc_small_trajectory_tempered / l2hmc_small_vjp_tempered)."""
    check_differentiable(dyn)
    xs, vs = dyn.XNet.state_dict(), dyn.VNet.state_dict()
    return _Trajectory.apply(dyn, list(xs), list(vs), x0, v0, dirs, sel, temp, dyn.alpha, *xs.values(), *vs.values())


def vjp_grads(dyn, plan, x0, v0, dirs, cot, want_dx0=True, want_dv0=True, temps=None):
    """One l2hmc_small_vjp over the rows (x0, v0, dirs) with cotangents cot = (g_x, g_v, g_logdet, g_p) (each may be
    None) -> (grads [xnet | vnet | d/d eps], dx0, dv0).  temps: None, or the ladder [C] (row r at temps[r % C])."""
    L = _lib.lib()
    R = x0.shape[0]
    dev = x0.device
    gsize = [sum(t.numel() for t in _segments(net).values()) for _, net in _nets(dyn)]
    grads = torch.empty(sum(gsize) + 1, dtype=torch.float32, device=dev)
    dx0 = torch.empty_like(x0) if want_dx0 else None
    dv0 = torch.empty_like(x0) if want_dv0 else None
    nbytes = max(int(L.l2hmc_small_train_ws_bytes(C.byref(plan), R)), 256)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tail = (x0, v0, dirs, R, *cot, dx0, dv0, grads, None, None, None, None, ws, nbytes)
    if temps is None:
        _lib.call("l2hmc_small_vjp", C.byref(plan), *tail, device=dev)
    else:
        _lib.call("l2hmc_small_vjp_tempered", C.byref(plan), temps, 1, temps.numel(), *tail, device=dev)
    return grads, dx0, dv0


def _segments(net, bufs=None):
    """The packed buffers struct l2hmc_dense_net points at, in the flat gradient order of l2hmc_small_train_step."""
    bufs = bufs if bufs is not None else net._packed[1]
    return {k: bufs[k] for k in net.SEGMENTS}


def unpack(dyn, grads, bufs=None):
    """[xnet | vnet | d/d eps] -> ({state_dict name: gradient} of XNet, of VNet, d/d eps [1])."""
    out, off = [], 0
    for i, (_, net) in enumerate(_nets(dyn)):
        seg = {}
        for k, b in _segments(net, None if bufs is None else bufs[i]).items():
            seg[k] = grads[off:off + b.numel()].view(b.shape)
            off += b.numel()
        out.append(net.unpack_grads(seg))
    return out[0], out[1], grads[off:off + 1]


class _Trajectory(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dyn, xnames, vnames, x0, v0, dirs, sel, temp, alpha, *weights):
        x0, v0 = x0.contiguous(), v0.contiguous()
        R = x0.shape[0]
        temps = temp if isinstance(temp, torch.Tensor) else None
        plan = dyn._plan(None if temps is not None else temp)
        X, V = torch.empty_like(x0), torch.empty_like(x0)
        ld = torch.empty(R, dtype=torch.float32, device=x0.device)
        p = torch.empty_like(ld)
        if temps is None:
            _lib.call("l2hmc_small_trajectory", C.byref(plan), x0, v0, dirs, R, X, V, ld, p, device=dyn._device)
        else:
            _lib.call("l2hmc_small_trajectory_tempered", C.byref(plan), temps, 1, temps.numel(), x0, v0, dirs, R, X, V,
                      ld, p, device=dyn._device)
        ctx.temps = temps
        ctx.save_for_backward(x0, v0, alpha, *weights)
        ctx.set_materialize_grads(False)
        # what the plan points at stays alive until the backward
        ctx.dyn, ctx.plan, ctx.names, ctx.dirs, ctx.sel, ctx.eps = dyn, plan, (xnames, vnames), dirs, sel, plan.eps
        ctx.mask = dyn.mask
        ctx.target = dyn._target
        ctx.bufs = [net._packed[1] for _, net in _nets(dyn)]
        if sel is None:
            return X, V, ld, p
        return X[sel], V[sel], ld[sel], p[sel]

    @staticmethod
    def backward(ctx, g_X, g_V, g_ld, g_p):
        if ctx.plan is None:
            raise RuntimeError("Dynamics trajectory: backward ran twice through the same graph; retain_graph is not "
                               "supported (the packed weights are released by the first backward)")
        saved = ctx.saved_tensors          # raises if a weight or input was modified in place since the forward
        x0, v0, alpha = saved[:3]
        dyn, plan, sel, dirs = ctx.dyn, ctx.plan, ctx.sel, ctx.dirs
        if sel is not None:                # only the kept rows: the others' outputs are multiplied by an exact 0
            x0, v0 = x0[sel].contiguous(), v0[sel].contiguous()
            dirs = None if dirs is None else dirs[sel].contiguous()
        cot = [None if g is None else g.contiguous() for g in (g_X, g_V, g_ld, g_p)]
        want_x, want_v = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        # (a ladder with kept rows: `propose`'s, one row per chain -- row i of the kept ones is chain i)
        grads, dx0, dv0 = vjp_grads(dyn, plan, x0, v0, dirs, cot, want_x, want_v, ctx.temps)
        gx, gv, deps = unpack(dyn, grads, ctx.bufs)
        ctx.plan = ctx.bufs = ctx.mask = ctx.target = ctx.dyn = ctx.temps = None
        if sel is not None:
            R = saved[0].shape[0]
            dx0 = None if dx0 is None else dx0.new_zeros(R, dx0.shape[1]).index_copy_(0, sel, dx0)
            dv0 = None if dv0 is None else dv0.new_zeros(R, dv0.shape[1]).index_copy_(0, sel, dv0)
        xnames, vnames = ctx.names
        wgrads = [gx[n] for n in xnames] + [gv[n] for n in vnames]
        grad_alpha = (deps * ctx.eps).reshape(alpha.shape).to(alpha.device)    # d/d alpha = eps d/d eps (quirk Q2)
        return (None, None, None, dx0, dv0, None, None, None, grad_alpha, *wgrads)


def run(dyn, x, v, backward, log_jac, temp=None):
    """Differentiable Dynamics.forward / .backward -> (X, V, p) or (X, V, sumlogdet).  temp: as `trajectory`'s."""
    dirs = torch.ones(x.shape[0], dtype=torch.int32, device=x.device) if backward else None
    X, V, ld, p = trajectory(dyn, x, v, dirs, None, temp)
    return (X, V, ld) if log_jac else (X, V, p)


def propose(dyn, x, vf, vb, mask, u, log_jac, temp=None):
    """Differentiable L2HMC branch of sampler.propose: both directions of every chain in one 2B-row trajectory
    launch, the direction `mask` (> 0.5 = forward) picks; u: MH uniforms or None.  -> (Lx, Lv, px, x_out or None).
    temp: as `trajectory`'s; a ladder [B] puts chain i at temp[i] in both of its directions."""
    B = x.shape[0]
    xx, vv = torch.cat([x, x]), torch.cat([vf, vb])
    dirs = torch.cat([torch.zeros(B, dtype=torch.int32, device=x.device),
                      torch.ones(B, dtype=torch.int32, device=x.device)])
    fwd = mask != 0                        # ops.mix_accept(strict = 0)
    sel = torch.arange(B, device=x.device) + B * (~fwd).to(torch.int64)
    Lx, Lv, ld, p = trajectory(dyn, xx, vv, dirs, sel, temp)
    px = ld if log_jac else p
    out = None if u is None else torch.where(((px - u) >= 0)[:, None], Lx, x)     # sampler.py:57-59
    return Lx, Lv, px, out
