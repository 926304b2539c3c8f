"""float64 restatement of one replica-exchange round (l2hmc_gauge_replica_swap, GaugeSampler.swap_replicas), in torch
so that it runs on the host and on the device alike, and the exact-sample fixture of the invariance checks.

Columns [g * G, (g + 1) * G) of x [B, 2TX] are one group, column c at betas[c].  A round of parity pi proposes the
pairs (a, a + 1), a = g * G + j, j = pi, pi + 2, ... with j + 1 < G, and exchanges the two rows iff p > u[a],
    p = min(1, exp((beta_a - beta_b) (S_a - S_b))),   S = sum_p (1 - cos P_p)
which is the Metropolis ratio exp(-beta_b S_a - beta_a S_b) / exp(-beta_a S_a - beta_b S_b) of the joint distribution.
`rule` selects the correct form or one of two deliberate defects (the power controls)."""
import numpy as np
import torch

from tests import invariance as I

RULES = ("correct", "sign_flipped", "always_accept")


def action64(x, T, X):
    """(action, average plaquette, real-valued charge) of x [B, 2TX] in float64, as oracle/lattice.py."""
    s = x.double().reshape(-1, T, X, 2)
    x0, x1 = s[..., 0], s[..., 1]
    P = x0 - x1 - torch.roll(x0, -1, dims=2) + torch.roll(x1, -1, dims=1)
    cs = torch.cos(P).sum(dim=(1, 2))
    proj = P - 2 * np.pi * torch.floor((P + np.pi) / (2 * np.pi))
    return T * X - cs, cs / (T * X), proj.sum(dim=(1, 2)) / (2 * np.pi)


def lower_chains(B, G, parity):
    """The lower chain a of every pair of the round, ascending (int64 NumPy)."""
    j = np.arange(parity, G - 1, 2)
    return (np.arange(B // G)[:, None] * G + j[None, :]).reshape(-1)


def swap_round(x, betas, G, parity, u, T, X, rule="correct"):
    """One round on x [B, 2TX] (any float dtype; a new tensor is returned) with uniforms u [B] (element a decides pair
    a) -> (x_new, swap_p [B] float64 with NaN off the lower chains, swapped [B] bool, perm [B] int64: x_new = x[perm])."""
    assert rule in RULES
    B = x.shape[0]
    dev = x.device
    a = torch.as_tensor(lower_chains(B, G, parity), device=dev)
    b = a + 1
    S = action64(x, T, X)[0]
    bt = torch.as_tensor(betas, dtype=torch.float64, device=dev).reshape(-1)
    dh = (bt[a] - bt[b]) * (S[a] - S[b])
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


# (T, X, betas of the rungs): the ladders of the invariance checks
LADDERS = {"4x4": (4, 4, (1.0, 2.0, 3.0, 4.0)), "2x4": (2, 4, (1.0, 1.5, 2.0, 3.0, 4.0)),
           "8x8": (8, 8, (2.0, 2.5, 3.0, 3.5))}
GROUPS = 4096
CHECKPOINTS = (1, 4, 16)
_START = {}


def ladder_start(name, groups=GROUPS, seed=1):
    """(x0 [groups * G, 2TX] float64: column g * G + r an exact sample at the r-th beta; betas [groups * G] float64;
    exact [G, 4]: I.u1_exact_vector at every rung).  Computed once per ladder and never changed by a caller."""
    if (name, groups, seed) not in _START:
        T, X, ladder = LADDERS[name]
        rng = np.random.default_rng(seed)
        G = len(ladder)
        x0 = np.empty((groups, G, 2 * T * X))
        for r, beta in enumerate(ladder):
            x0[:, r] = I.u1_samples(groups, T, X, beta, rng)
        x0 = x0.reshape(groups * G, -1)
        exact = np.stack([I.u1_exact_vector(T, X, beta) for beta in ladder])
        _START[(name, groups, seed)] = (x0, np.tile(np.asarray(ladder, dtype=np.float64), groups), exact)
    return _START[(name, groups, seed)]


def rung_zscores(x, T, X, G, exact):
    """z [G, 4] of I.U1_FEATURES per rung (column % G) of the state x [B, 2TX] against exact [G, 4]."""
    a, p, q = (v.cpu().numpy().reshape(-1, G) for v in action64(x, T, X))
    return np.stack([I.zscores(I.u1_features(p[:, r], a[:, r], q[:, r]), exact[r]) for r in range(G)])
