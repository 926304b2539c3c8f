"""The stateless operators of the torus-exact mode (`GaugeDynamics(periodic=True)`, L2HMC_PLAN_PERIODIC), one plain
function per C entry, with the checks of `ops`: every caller-supplied tensor goes through `_lib.dev_ptr` (a torch tensor,
on the GPU, fp32, contiguous) and `_lib.expect_shape` (the shape that follows from the first tensor: the state's for
v / S / T / Q / dx_out / dx, (D,) for keep, (rows,) for dlogdet, [rows, 2 D] for the angle features; either error names
the argument) before torch.cuda or the library is touched.  `ops` stays
the place of the reference's operators; these have no counterpart there."""
import torch

from . import _lib
from .ops import _ptrs, _rows, _shapes, _update_x_shapes


def lf_update_x_ncp(x, v, keep, S, T, Q, eps, direction):
    """Circle-preserving position sub-update; keep [D]: 1 = coordinate kept -> (x' (principal value, defined modulo
    2 pi), per-row log-det)."""
    ptrs = _ptrs(x=x, v=v, keep=keep, S=S, T=T, Q=Q)
    _update_x_shapes(x, v, keep, S, T, Q)
    out, ld = torch.empty_like(x), _rows(x)
    _lib.call("l2hmc_lf_update_x_ncp", *ptrs, float(eps), int(direction), x.shape[0], x.shape[1], out, ld,
              device=x.device)
    return out, ld


def lf_update_x_ncp_vjp(x, v, keep, S, T, Q, eps, direction, dx_out, dlogdet):
    """Reverse of `lf_update_x_ncp` from the cotangents of (x', log-det) -> (dx, dv through this update alone, dS, dT,
    dQ, per-row d/d eps)."""
    ptrs = _ptrs(x=x, v=v, keep=keep, S=S, T=T, Q=Q)
    tail = _ptrs(dx_out=dx_out, dlogdet=dlogdet)
    _update_x_shapes(x, v, keep, S, T, Q)
    _shapes(tuple(x.shape), dx_out=dx_out)
    _shapes((x.shape[0],), dlogdet=dlogdet)
    dx, dv, dS, dT, dQ = (torch.empty_like(x) for _ in range(5))
    deps = _rows(x)
    _lib.call("l2hmc_lf_update_x_ncp_vjp", *ptrs, float(eps), int(direction), x.shape[0], x.shape[1], *tail, dx, dv, dS,
              dT, dQ, deps, device=x.device)
    return dx, dv, dS, dT, dQ, deps


def u1_angle_features(x, out=None):
    """x [rows, D] -> [cos x | sin x] [rows, 2 D], into `out` if given."""
    px, _ = _ptrs(x=x, out=out)
    _shapes((None, None), x=x)
    rows, D = x.shape
    _shapes((rows, 2 * D), out=out)
    if out is None:
        out = torch.empty(rows, 2 * D, dtype=torch.float32, device=x.device)
    _lib.call("l2hmc_u1_angle_features", px, rows, D, out, device=x.device)
    return out


def u1_angle_features_vjp(x, dfeat, dx):
    """dx [rows, D] += -sin x * dfeat[:, :D] + cos x * dfeat[:, D:] (in place; returns dx).  dfeat [rows, 2 D]."""
    px, pf, pd = _ptrs(x=x, dfeat=dfeat, dx=dx)
    _shapes((None, None), x=x)
    _shapes((x.shape[0], 2 * x.shape[1]), dfeat=dfeat)
    _shapes(tuple(x.shape), dx=dx)
    _lib.call("l2hmc_u1_angle_features_vjp", px, pf, dfeat.shape[1], x.shape[0], x.shape[1], dx, device=x.device)
    return dx
