"""Reference and inputs for the lattice loss kernels (`gauge_loss_kernel` in csrc/loss.hip, `loss_bwd_kernel` in
csrc/train.hip), in one place for tests/test_loss_ref_host.py (which validates both without a GPU) and
tests/test_gpu_loss_kernels.py (which compares the kernels with them).

`loss_ref` restates gauge_model.py:728-797 on the 2B stacked chains in plain torch: rows [0, B) start at x, rows
[B, 2B) at the auxiliary z.  The accept probability is p = exp(min(H0 - H1 + sld, 0)) with
H = beta * action + |v|^2 / 2; the metric table and the n = 1..4 projection series are those of
`oracle.torch_ref.TorchGaugeModel.loss`, and both auxiliary terms compare z with the proposal of x (quirk Q9).
loss = inv_count * sum(terms); autograd gives d loss / d (xN, vN, sld).  With dtype=torch.float64 it is the
yardstick; with dtype=torch.float32 (on the CPU) it is the fp32 evaluation in the reference's op order that
`assert_fp32_equivalent` measures a kernel against.

Every array of a case holds float32-representable numbers, and `loss_ref` rounds its scalars to float32 first, so
the float64 evaluation, the float32 evaluation and the kernels all start from the same numbers."""
import collections
import functools

import numpy as np
import torch

from oracle.torch_ref import TWO_PI, action, plaq

METRICS = ('l1', 'l2', 'cos', 'cos2', 'cos_diff')      # position = the C ABI's metric code
BETA = 1.7
WEIGHTS = dict(loss_scale=0.7, aux_weight=0.9, std_weight=1.1, charge_weight=1.3)

# (T, X, B, seed): what each shape is for is told in tests/test_gpu_loss_kernels.py.  A seed is one at which the input
# conditions of tests/test_loss_ref_host.py hold.
CASES = [
    (2, 3, 5, 1),
    (3, 5, 37, 1),
    (8, 8, 24, 1),
    (4, 16, 11, 1),
    (16, 4, 11, 2),
    (1, 6, 4, 2),
    (6, 1, 4, 1),
    (10, 10, 9, 1),
    (12, 24, 3, 2),
    (32, 32, 3, 2),
    (64, 64, 2, 2),
]
ALL_METRICS_AT = {(3, 5, 37), (10, 10, 9), (12, 24, 3)}     # the other shapes run cos_diff alone
BACKWARD_ONLY = {(64, 64, 2)}

LossRef = collections.namedtuple("LossRef", "terms p dxN dvN dsld")


def f32(s):
    """A Python float rounded to float32: what a kernel receives for a scalar argument."""
    return float(np.float32(s))


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _metric(name):
    return {'l1': lambda a, b: torch.abs(a - b), 'l2': lambda a, b: (a - b) ** 2,
            'cos': lambda a, b: torch.abs(torch.cos(a) - torch.cos(b)),
            'cos2': lambda a, b: (torch.cos(a) - torch.cos(b)) ** 2,
            'cos_diff': lambda a, b: 1. - torch.cos(a - b)}[name]


def charge_series(a, T, X):
    """sum over plaquettes of sum_{n=1}^{4} (-2/n)(-1)^n sin(n P), over 2 pi (gauge_model.py:94-108, :718-725)."""
    pq = plaq(a, T, X)
    y = torch.zeros_like(pq)
    for n in range(1, 5):
        y = y + (-2. / n) * ((-1.) ** n) * torch.sin(n * pq)
    return y.sum(dim=(1, 2)) / TWO_PI


def loss_ref(x, z, xN, vN, sld, x0v0_H, beta, T, X, metric, loss_scale, aux_weight, std_weight, charge_weight,
             inv_count, dtype, p_in=None):
    """x, z [B, D]: initial states;  xN, vN [2B, D], sld [2B]: proposals and summed log-determinants of the 2B chains;
    x0v0_H [2B]: the Hamiltonian of the initial state (x0, v0), a constant of the loss.  Returns LossRef(terms [B],
    p [2B], d loss / d xN, d loss / d vN, d loss / d sld) as NumPy arrays of `dtype`.
    p_in [2B]: take the VALUE of p from here, as `loss_bwd_kernel` does (p is one of its inputs), and only its
    derivative from the formula; the float32 evaluation then does not carry the rounding of H0 - H1 + sld, which at
    |H| of some thousands dwarfs everything a kernel adds."""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dtype)          # noqa: E731
    beta, ls, aw, sw, cw, w = map(f32, (beta, loss_scale, aux_weight, std_weight, charge_weight, inv_count))
    x, z, H0 = t(x), t(z), t(x0v0_H)
    xN, vN, sld = (t(a).requires_grad_() for a in (xN, vN, sld))
    B = x.shape[0]
    H1 = beta * action(xN, T, X) + 0.5 * (vN ** 2).sum(1)
    logp = torch.minimum(H0 - H1 + sld, torch.zeros((), dtype=dtype))
    p = torch.exp(logp) if p_in is None else t(p_in) * torch.exp(logp - logp.detach())
    px, pz, x_ = p[:B], p[B:], xN[:B]
    eps = 1e-3
    m = _metric(metric)
    x_std = m(x, x_).sum(1) * px + eps
    z_std = aw * (m(z, x_).sum(1) * pz + eps)
    std_loss = sw * (ls * (1. / x_std + 1. / z_std) - (x_std + z_std) / ls)
    q_ = charge_series(x_, T, X)
    xq = px * torch.abs(charge_series(x, T, X) - q_) + eps
    zq = aw * (pz * torch.abs(charge_series(z, T, X) - q_) + eps)
    terms = std_loss + cw * (xq + zq)
    (w * terms.sum()).backward()
    return LossRef(*(a.detach().numpy() for a in (terms, p, xN.grad, vN.grad, sld.grad)))


@functools.lru_cache(maxsize=None)
def loss_case(T, X, B, seed):
    """The inputs of one case, as read-only float64 arrays of float32-representable numbers: x, z [B, D]; xN, vN
    [2B, D]; sld, H0 [2B].  A = H0 - H1 + sld is N(0, 1) as in test_accept_backward_kernel_matches_float64, so there
    are chains with p == 1 and chains with 0 < p < 1; where A < 0 it is raised to log 0.06 so that p >= 0.05 (the range
    of test_loss_forward_matches_oracle, where 1 / x_std stays well conditioned), and |A| >= 0.02 keeps the side of
    the min the same in float32 and float64."""
    D = 2 * T * X
    rng = np.random.default_rng([seed, T, X, B])
    x, xN, zN = (_r32(rng.uniform(0, 2 * np.pi, (B, D))) for _ in range(3))
    z = _r32(rng.standard_normal((B, D)))
    vN, v0 = (_r32(rng.standard_normal((2 * B, D))) for _ in range(2))
    xN = np.concatenate([xN, zN])
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)          # noqa: E731
    h = lambda q, v: (f32(BETA) * action(t64(q), T, X) + 0.5 * (t64(v) ** 2).sum(1)).numpy()      # noqa: E731
    H0 = _r32(h(np.concatenate([x, z]), v0))
    A = rng.standard_normal(2 * B)
    A = np.where(A < 0, np.maximum(A, np.log(0.06)), A)
    A = np.where(A < 0, -1., 1.) * np.maximum(np.abs(A), 0.02)
    sld = _r32(h(xN, vN) - H0 + A)
    case = dict(x=x, z=z, xN=xN, vN=vN, sld=sld, H0=H0)
    for a in case.values():
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def reference(T, X, B, seed, metric, inv_count, dtype=torch.float64, given_p=False):
    """`loss_ref` of a committed case at the tests' weights, computed once and left unchanged.  given_p: with the
    float64 value of p, rounded to float32, handed in (what the tests hand the kernels)."""
    c = loss_case(T, X, B, seed)
    p_in = _r32(reference(T, X, B, seed, metric, inv_count).p) if given_p else None
    ref = loss_ref(c["x"], c["z"], c["xN"], c["vN"], c["sld"], c["H0"], BETA, T, X, metric, inv_count=inv_count,
                   dtype=dtype, p_in=p_in, **WEIGHTS)
    for a in ref:
        a.setflags(write=False)
    return ref


def case_metric_pairs(backward):
    """[(case, metric)] the GPU tests run: all five metrics at ALL_METRICS_AT, cos_diff elsewhere; the backward-only
    shape is left to the backward entry."""
    out = []
    for case in CASES:
        if case[:3] in BACKWARD_ONLY and not backward:
            continue
        for metric in (METRICS if case[:3] in ALL_METRICS_AT else ('cos_diff',)):
            out.append((case, metric))
    return out


def pair_id(pair):
    (T, X, B, _), metric = pair
    return f"{T}x{X}x{B}-{metric}"
