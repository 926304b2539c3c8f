"""float64 restatement of one replica-exchange round on a toy target (l2hmc_small_replica_swap,
DynamicsSampler.swap_replicas and the rounds inside l2hmc_small_hmc_run_exchange), in torch so that it runs on the host
and on the device alike, and the exact-sample fixture of the invariance checks.

Columns [g * G, (g + 1) * G) of x [B, dim] are one group, column c at temps[c].  A round of parity pi proposes the pairs
(a, a + 1), a = g * G + j, j = pi, pi + 2, ... with j + 1 < G (tests/replica_ref.lower_chains), and exchanges the two
rows iff p > u[a],
    p = min(1, exp((1 / T_a - 1 / T_b) (U_a - U_b))),   U = the target's energy at temperature 1
which is the Metropolis ratio exp(-U_b / T_a - U_a / T_b) / exp(-U_a / T_a - U_b / T_b) of the joint distribution.
`rule` selects the correct form or one of two deliberate defects (the power controls)."""
import numpy as np
import torch

from tests import invariance as I
from tests.replica_ref import RULES, lower_chains


def swap_round(x, temps, G, parity, u, energy, rule="correct"):
    """One round on x [B, dim] (any float dtype; a new tensor is returned) at temperatures temps [B] with uniforms
    u [B] (element a decides pair a); `energy(x)` -> U [B] float64 at temperature 1 (a torch tensor on x's device)
    -> (x_new, swap_p [B] float64 with NaN off the lower chains, swapped [B] bool, perm [B] int64: x_new = x[perm])."""
    assert rule in RULES
    B = x.shape[0]
    dev = x.device
    a = torch.as_tensor(lower_chains(B, G, parity), device=dev)
    b = a + 1
    U = torch.as_tensor(energy(x), dtype=torch.float64, device=dev)
    it = 1.0 / torch.as_tensor(temps, dtype=torch.float64, device=dev).reshape(-1)
    dh = (it[a] - it[b]) * (U[a] - U[b])
    if rule == "sign_flipped":
        dh = -dh
    p = torch.exp(torch.clamp(dh, max=0.0)).nan_to_num(0.0)
    if rule == "always_accept":
        p = torch.ones_like(p)
    acc = p > torch.as_tensor(u, dtype=torch.float64, device=dev)[a]
    perm = torch.arange(B, device=dev)
    perm[a[acc]], perm[b[acc]] = b[acc], a[acc]
    swap_p = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    swap_p[a] = p
    swapped = torch.zeros(B, dtype=torch.bool, device=dev)
    swapped[a] = acc
    return x[perm], swap_p, swapped, perm


# ------------------------------------------------------------------------------------- the ladder of the invariance checks
COV = np.array([[1.0, 0.6], [0.6, 1.0]])
MU = np.zeros(2)
LADDER = (1.0, 2.0, 4.0, 8.0)
GROUPS = 4096
CHECKPOINTS = (1, 4, 16)
HMC_EPS, HMC_N = 0.3, 5
_START = {}


def precision64():
    """The precision the library's Gaussian(MU, COV) evaluates: float32 inv(COV), as float64."""
    return np.linalg.inv(COV).astype(np.float32).astype(np.float64)


def energy64(x):
    """U(x) = (x - mu)^T P (x - mu) / 2 in float64, on the device x is on."""
    xt = torch.as_tensor(x).double()
    P = torch.as_tensor(precision64(), device=xt.device)
    P = 0.5 * (P + P.T)
    return 0.5 * torch.einsum("bi,ij,bj->b", xt, P, xt)


def ladder_start(groups=GROUPS, seed=1):
    """(x0 [groups * G, 2] float64: column g * G + r an exact sample at the r-th temperature; temps [groups * G];
    exact: per rung (ExactGMM, W, c) for `rung_zscores`).  Computed once per key and never changed by a caller."""
    if (groups, seed) not in _START:
        rng = np.random.default_rng(seed)
        G = len(LADDER)
        x0 = np.empty((groups, G, 2))
        exact = []
        for r, T in enumerate(LADDER):
            gmm = I.ExactGMM.of_library_gaussian(MU, COV, temperature=T)
            x0[:, r] = gmm.sample(groups, rng)
            exact.append((gmm, *gmm.halfspaces(np.random.default_rng(100 + r))))
        _START[(groups, seed)] = (x0.reshape(groups * G, 2), np.tile(np.asarray(LADDER), groups), exact)
    return _START[(groups, seed)]


def rung_zscores(x, exact, with_energy=False):
    """z [G, J] per rung (column % G) of the state x [B, 2] against `ladder_start`'s exact: ExactGMM.features (means,
    second moments, half-space indicators) and, `with_energy`, U, whose mean at temperature T is T dim / 2."""
    G = len(exact)
    xs = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)
    xs = xs.reshape(-1, G, xs.shape[-1])
    out = []
    for r, (gmm, W, c) in enumerate(exact):
        f, e = gmm.features(xs[:, r], W, c), gmm.expectations(W, c)
        if with_energy:
            f = np.concatenate([f, energy64(xs[:, r]).numpy()[:, None]], axis=1)
            e = np.concatenate([e, [LADDER[r] * gmm.dim / 2.0]])
        out.append(I.zscores(f, e))
    return np.stack(out)


def hmc_step64(x, temps, rng, eps=HMC_EPS, n=HMC_N):
    """One plain-HMC step with the Metropolis-Hastings decision on x [B, 2] (NumPy float64), column c at temps[c]."""
    P = precision64()
    P = 0.5 * (P + P.T)
    it = (1.0 / np.asarray(temps, dtype=np.float64))[:, None]
    grad = lambda y: (y @ P) * it
    ham = lambda y, w: 0.5 * np.einsum("bi,ij,bj->b", y, P, y) * it[:, 0] + 0.5 * (w ** 2).sum(1)
    v = rng.standard_normal(x.shape)
    y, w = x.copy(), v - 0.5 * eps * grad(x)
    for i in range(n):
        y = y + eps * w
        w = w - (eps if i + 1 < n else 0.5 * eps) * grad(y)
    acc = rng.uniform(size=x.shape[0]) < np.exp(np.minimum(ham(x, v) - ham(y, w), 0.0))
    return np.where(acc[:, None], y, x)
