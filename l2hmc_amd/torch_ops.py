"""`torch.ops.l2hmc.*`: the stateless operators of the C ABI registered with PyTorch's dispatcher (SURVEY.md 8b names
`extern "C"` / `TORCH_LIBRARY(l2hmc)` as the boundary; the C ABI of include/l2hmc_hip.h is the boundary, this file makes
the same entry points visible to callers that compose torch operators).  Every op takes contiguous fp32 CUDA (ROCm)
tensors, launches on torch's current stream, allocates only its outputs and has NO CPU implementation: called with a CPU
tensor it raises like every other entry of this package.  Each validates every caller-supplied tensor before the library
is touched: device, dtype and contiguity (`_lib.dev_ptr`) and its shape (`_lib.expect_shape`, through `ops`; stq_dense
checks all nine weight shapes against (H, Ka + Kb) and D, and a [rows, Ka], b [rows, Kb] against them).  Networks travel
as the flat tuple of their packed device buffers (`_DenseSTQ.flat_tensors()` order: w1_t, wt, b1, wh_t, bh, whd_t, bhd,
coeff_s, coeff_q).

    import l2hmc_amd.torch_ops            # registers the library
    action, force, plaq, charge = torch.ops.l2hmc.u1_action_force(x, T, X, beta)
    S, T_, Q = torch.ops.l2hmc.stq_dense(a, b, weights, q_tanh, t_cos, t_sin)
    v1, logdet = torch.ops.l2hmc.lf_update_v(v, grad, S, T_, Q, eps, direction)
    x1, logdet = torch.ops.l2hmc.lf_update_x(x, v, keep, S, T_, Q, eps, direction)
    p = torch.ops.l2hmc.accept_prob(h_old, h_new, sumlogdet)
    x_prop, v_prop, p, x_out = torch.ops.l2hmc.mix_accept(x, xf, vf, pf, xb, vb, pb, coin, u, strict)
    k = torch.ops.l2hmc.kinetic_energy(v)
    y = torch.ops.l2hmc.wrap_angle(x)
"""
import ctypes as C
from typing import List, Tuple

import torch

from . import _lib, ops

_WEIGHT_FIELDS = ("w1_t", "wt", "b1", "wh_t", "bh", "whd_t", "bhd", "coeff_s", "coeff_q")


def _net_struct(weights, q_tanh):
    """struct l2hmc_dense_net over `weights` after their checks: all nine shapes follow from w1_t [H, Ka + Kb] (Ka = Kb)
    and the D of whd_t [3, D, H]."""
    if len(weights) != len(_WEIGHT_FIELDS):
        raise ValueError(f"weights: expected {len(_WEIGHT_FIELDS)} tensors {_WEIGHT_FIELDS}, got {len(weights)}")
    ptrs = [_lib.dev_ptr(t, name=f) for f, t in zip(_WEIGHT_FIELDS, weights)]
    w1_t, whd_t = weights[0], weights[5]
    _lib.expect_shape(w1_t, (None, None), "w1_t")
    H, K = w1_t.shape
    if K % 2:
        raise ValueError(f"w1_t: expected shape (H, Ka + Kb) with Ka = Kb, got {tuple(w1_t.shape)}")
    _lib.expect_shape(whd_t, (3, None, H), "whd_t")
    D = whd_t.shape[1]
    shapes = dict(wt=(2, H), b1=(H,), wh_t=(H, H), bh=(H,), bhd=(3, D), coeff_s=(D,), coeff_q=(D,))
    for f, t in zip(_WEIGHT_FIELDS, weights):
        if f in shapes:
            _lib.expect_shape(t, shapes[f], f)
    st = _lib.DenseNet(D=D, H=H, Ka=K // 2, Kb=K // 2, q_tanh=int(q_tanh), reserved=0, packed=None)
    for f, ptr in zip(_WEIGHT_FIELDS, ptrs):
        setattr(st, f, ptr)
    return st


@torch.library.custom_op("l2hmc::u1_action_force", mutates_args=())
def u1_action_force(x: torch.Tensor, time_size: int, space_size: int, beta: float) -> Tuple[torch.Tensor, torch.Tensor,
                                                                                             torch.Tensor, torch.Tensor]:
    """lattice.py:285-362, gauge_dynamics.py:698-709: (action, beta * dS/dx, average plaquette, topological charge)."""
    return ops.u1_action_force(x.reshape(-1, 2 * time_size * space_size), time_size, space_size, beta)


@torch.library.custom_op("l2hmc::stq_dense", mutates_args=())
def stq_dense(a: torch.Tensor, b: torch.Tensor, weights: List[torch.Tensor], q_tanh: int, t_cos: float,
              t_sin: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """generic_net.py:129-146 / utils/network.py:89-114 (q_tanh = 1): (S, T, Q) = net([a, b, t])."""
    st = _net_struct(weights, q_tanh)
    pa, pb = _lib.dev_ptr(a, name="a"), _lib.dev_ptr(b, name="b")
    _lib.expect_shape(a, (None, st.Ka), "a")
    rows = a.shape[0]
    _lib.expect_shape(b, (rows, st.Kb), "b")
    S, T, Q = (torch.empty(rows, st.D, dtype=torch.float32, device=a.device) for _ in range(3))
    nb = _lib.lib().l2hmc_stq_ws_bytes(rows, st.H)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=a.device)
    _lib.call("l2hmc_stq_dense", C.byref(st), pa, pb, None, float(t_cos), float(t_sin), rows, S, T, Q, ws, nb,
              device=a.device)
    return S, T, Q


@torch.library.custom_op("l2hmc::lf_update_v", mutates_args=())
def lf_update_v(v: torch.Tensor, grad: torch.Tensor, S: torch.Tensor, T: torch.Tensor, Q: torch.Tensor, eps: float,
                direction: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """gauge_dynamics.py:486-508 (direction 0), :537-561 (1): (v', per-row log-det)."""
    return ops.lf_update_v(v, grad, S, T, Q, eps, direction)


@torch.library.custom_op("l2hmc::lf_update_x", mutates_args=())
def lf_update_x(x: torch.Tensor, v: torch.Tensor, keep: torch.Tensor, S: torch.Tensor, T: torch.Tensor, Q: torch.Tensor,
                eps: float, direction: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """gauge_dynamics.py:511-534 (direction 0), :565-590 (1); keep [D]: 1 = coordinate kept."""
    return ops.lf_update_x(x, v, keep, S, T, Q, eps, direction)


@torch.library.custom_op("l2hmc::accept_prob", mutates_args=())
def accept_prob(h_old: torch.Tensor, h_new: torch.Tensor, sumlogdet: torch.Tensor) -> torch.Tensor:
    """gauge_dynamics.py:592-609: exp(min(h_old - h_new + sumlogdet, 0)), non-finite -> 0."""
    return ops.accept_prob(h_old, h_new, sumlogdet)


@torch.library.custom_op("l2hmc::mix_accept", mutates_args=())
def mix_accept(x: torch.Tensor, xf: torch.Tensor, vf: torch.Tensor, pf: torch.Tensor, xb: torch.Tensor, vb: torch.Tensor,
               pb: torch.Tensor, coin: torch.Tensor, u: torch.Tensor, strict: int) -> Tuple[torch.Tensor, torch.Tensor,
                                                                                              torch.Tensor, torch.Tensor]:
    """gauge_dynamics.py:221-257 (strict = 1) / utils/sampler.py:33-59 (0): (x_prop, v_prop, p, x_out)."""
    return ops.mix_accept(x, xf, vf, pf, xb, vb, pb, coin, u, strict)


@torch.library.custom_op("l2hmc::kinetic_energy", mutates_args=())
def kinetic_energy(v: torch.Tensor) -> torch.Tensor:
    """gauge_dynamics.py:683-689: 0.5 * sum_d v^2 per row."""
    return ops.kinetic_energy(v)


@torch.library.custom_op("l2hmc::wrap_angle", mutates_args=())
def wrap_angle(x: torch.Tensor) -> torch.Tensor:
    """gauge_model.py:1180, :1388: x mod 2 pi in [0, 2 pi)."""
    return ops.wrap_angle(x)


OPS = ("u1_action_force", "stq_dense", "lf_update_v", "lf_update_x", "accept_prob", "mix_accept", "kinetic_energy",
       "wrap_angle")
