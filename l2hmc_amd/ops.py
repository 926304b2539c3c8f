"""The stateless operators of the C ABI (include/l2hmc_hip.h), one plain function per entry: the ONE place in the
package that calls them.  Each validates every caller-supplied tensor (`_lib.dev_ptr`: a torch tensor, on the GPU, fp32
or int32 as the entry reads it, contiguous; then `_lib.expect_shape`: the first tensor fixes rows and width, and every
other tensor -- inputs, per-row vectors, `keep`, a given `out` -- must have the shape that follows from it, since the C
entries take raw pointers and size their launch from one argument; either error names the argument) before it touches
torch.cuda or the library, allocates its outputs, launches on torch's current stream of the inputs' device and checks
the status.  `torch_ops`
registers these with PyTorch's dispatcher; the dynamics, samplers and trainers call them directly."""
import torch

from . import _lib


def _ptrs(**tensors):
    return [_lib.dev_ptr(t, name=n) for n, t in tensors.items()]


def _shapes(shape, **tensors):
    for n, t in tensors.items():
        _lib.expect_shape(t, shape, n)


def _rows(t):
    return torch.empty(t.shape[0], dtype=torch.float32, device=t.device)


def kinetic_energy(v):
    """0.5 * sum_d v^2 per row of v [rows, D]."""
    (pv,) = _ptrs(v=v)
    _shapes((None, None), v=v)
    out = _rows(v)
    _lib.call("l2hmc_kinetic_energy", pv, v.shape[0], v.shape[1], out, device=v.device)
    return out


def accept_prob(h_old, h_new, sumlogdet):
    """exp(min(h_old - h_new + sumlogdet, 0)), non-finite -> 0."""
    ptrs = _ptrs(h_old=h_old, h_new=h_new, sumlogdet=sumlogdet)
    _shapes(tuple(h_old.shape), h_new=h_new, sumlogdet=sumlogdet)
    p = torch.empty_like(h_old)
    _lib.call("l2hmc_accept_prob", *ptrs, p.numel(), p, device=p.device)
    return p


def wrap_angle(x, out=None):
    """x mod 2 pi in [0, 2 pi), into `out` (another tensor of x's shape) if given."""
    px, _ = _ptrs(x=x, out=out)
    _shapes(tuple(x.shape), out=out)
    if out is None:
        out = torch.empty_like(x)
    _lib.call("l2hmc_wrap_angle", px, x.numel(), out, device=x.device)
    return out


def lf_update_v(v, grad, S, T, Q, eps, direction):
    """Momentum half-kick (direction 0 forward, 1 backward) -> (v', per-row log-det)."""
    ptrs = _ptrs(v=v, grad=grad, S=S, T=T, Q=Q)
    _shapes((None, None), v=v)
    _shapes(tuple(v.shape), grad=grad, S=S, T=T, Q=Q)
    out, ld = torch.empty_like(v), _rows(v)
    _lib.call("l2hmc_lf_update_v", *ptrs, float(eps), int(direction), v.shape[0], v.shape[1], out, ld, device=v.device)
    return out, ld


def _update_x_shapes(x, v, keep, S, T, Q):
    _shapes((None, None), x=x)
    _shapes(tuple(x.shape), v=v)
    _shapes((x.shape[1],), keep=keep)
    _shapes(tuple(x.shape), S=S, T=T, Q=Q)


def lf_update_x(x, v, keep, S, T, Q, eps, direction):
    """Position sub-update; keep [D]: 1 = coordinate kept -> (x', per-row log-det)."""
    ptrs = _ptrs(x=x, v=v, keep=keep, S=S, T=T, Q=Q)
    _update_x_shapes(x, v, keep, S, T, Q)
    out, ld = torch.empty_like(x), _rows(x)
    _lib.call("l2hmc_lf_update_x", *ptrs, float(eps), int(direction), x.shape[0], x.shape[1], out, ld, device=x.device)
    return out, ld


def mix_accept(x, xf, vf, pf, xb, vb, pb, coin, u, strict, want_proposal=True, want_out=True):
    """Pick each chain's direction by `coin` and accept by `u` -> (x_prop, v_prop, p, x_out); the proposal triple and
    x_out are None unless wanted (u = None: no MH step, so no x_out).  strict = 1: p > u, 0: p - u >= 0."""
    ptrs = _ptrs(x=x, xf=xf, vf=vf, pf=pf, xb=xb, vb=vb, pb=pb, coin=coin, u=u)
    _shapes((None, None), x=x)
    full, rows = tuple(x.shape), (x.shape[0],)
    for n, t in dict(xf=xf, vf=vf, pf=pf, xb=xb, vb=vb, pb=pb, coin=coin, u=u).items():
        _lib.expect_shape(t, rows if n in ("pf", "pb", "coin", "u") else full, n)
    x_prop, v_prop, p = (torch.empty_like(x), torch.empty_like(x), torch.empty_like(pf)) if want_proposal else (None,) * 3
    x_out = torch.empty_like(x) if want_out else None
    _lib.call("l2hmc_mix_accept", *ptrs, int(strict), x.shape[0], x.shape[1], x_prop, v_prop, p, x_out, device=x.device)
    return x_prop, v_prop, p, x_out


def u1_action_force(x, T, X, beta, want_force=True, want_observables=True):
    """x [rows, 2*T*X] -> (action, beta * dS/dx, average plaquette, topological charge); None where not wanted."""
    (px,) = _ptrs(x=x)
    _shapes((None, 2 * T * X), x=x)
    action, plaq, charge = (_rows(x) for _ in range(3)) if want_observables else (None,) * 3
    force = torch.empty_like(x) if want_force else None
    _lib.call("l2hmc_u1_action_force", px, x.shape[0], T, X, float(beta), action, force, plaq, charge, device=x.device)
    return action, force, plaq, charge


def u1_force_hvp(x, u, T, X, beta):
    """d(beta * dS/dx)/dx . u per row."""
    ptrs = _ptrs(x=x, u=u)
    _shapes((None, 2 * T * X), x=x)
    _shapes(tuple(x.shape), u=u)
    out = torch.empty_like(x)
    _lib.call("l2hmc_u1_force_hvp", *ptrs, x.shape[0], T, X, float(beta), out, device=x.device)
    return out


def _fill(entry, shape, seed, draw, device, out):
    _ptrs(out=out)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
    _lib.call(entry, out, out.numel(), int(seed), int(draw), device=out.device)
    return out


def fill_normal(shape, seed, draw, device=None, out=None):
    """N(0, 1) of the Philox stream (seed, draw): a new tensor of `shape` on `device`, or all of `out`."""
    return _fill("l2hmc_fill_normal", shape, seed, draw, device, out)


def fill_uniform(shape, seed, draw, device=None, out=None):
    """U[0, 1) of the Philox stream (seed, draw): a new tensor of `shape` on `device`, or all of `out`."""
    return _fill("l2hmc_fill_uniform", shape, seed, draw, device, out)
