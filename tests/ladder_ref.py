"""Shared by the ladder-training tests (tests/test_gpu_gauge_train_ladder.py, tests/test_gauge_train_ladder_host.py):
the float64 reference of a training step on a ladder of beta, and the fixed assignment of betas to chains.

The reference is oracle/torch_ref.py's TorchGaugeModel, unedited, with the two methods through which beta enters
overridden so that `beta` may be a [B] tensor: chain i of the x batch and chain i of the z batch run at beta[i] (the
model integrates each batch on its own, so a row of either is chain i).  With a scalar the overrides are the parent's
methods.  Its per-chain terms equal the unmodified oracle's run rung by rung on that rung's chains, and its gradients
the B_g / B-weighted sum of those runs (checked on the CPU in test_gauge_train_ladder_host.py)."""
import numpy as np
import torch

from oracle.torch_ref import TorchGaugeModel, action, grad_action

RUNGS = (1.0, 2.0, 3.0)
# which rung a chain sits on: fixed and NOT periodic, so the rows of one 16-row workgroup differ and -- with B = 24 or
# 9 -- a chain's x row and z row sit at different places in their workgroups ((B + i) % 16 != i % 16)
_PATTERN = (0, 2, 1, 1, 0, 2, 2, 0, 1, 0, 0, 2, 1, 2, 2, 0, 1, 1, 0, 1, 2, 2, 1, 0, 0, 1, 2, 1, 0, 2, 0, 2, 1, 1, 2, 0, 1,
            0, 2, 2, 1, 0)


def rung_of(B):
    """The rung index (0, 1, 2) of each of B chains."""
    assert B <= len(_PATTERN)
    return np.asarray(_PATTERN[:B])


def ladder(B, rungs=RUNGS):
    """beta [B] float64: the three values laid on the chains by the fixed pattern."""
    return np.asarray(rungs, dtype=np.float64)[rung_of(B)]


class LadderGaugeModel(TorchGaugeModel):
    """TorchGaugeModel whose `beta` may be a [B] tensor (one value per chain of the batch it is handed)."""

    def _force(self, x, beta):
        if torch.is_tensor(beta) and beta.ndim == 1:
            return beta[:, None] * grad_action(x, self.T, self.X)
        return super()._force(x, beta)

    def _energy(self, x, beta):
        if torch.is_tensor(beta) and beta.ndim == 1:
            return beta * action(x, self.T, self.X)
        return super()._energy(x, beta)


def ref_grads(tm, x, z, dx, dz, beta, metric='cos_diff', **w):
    """loss.backward() of the float64 model at `beta` (a float, or [B]) -> (loss, per-chain terms)."""
    tt = lambda a: torch.tensor(a, dtype=torch.float64)      # noqa: E731
    b = tt(np.asarray(beta, dtype=np.float64)) if np.ndim(beta) else float(beta)
    for p in tm.parameters():
        p.grad = None
    loss, terms = tm.loss(tt(x), tt(z), b, tuple(map(tt, dx)), tuple(map(tt, dz)), metric=metric, **w)
    loss.backward()
    return float(loss.detach()), terms.detach().numpy()


def inputs(B, D, seed=7):
    """x, z and the two transitions' draws, as tests/test_gpu_train.py::_setup draws them."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 2 * np.pi, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    return x, z, dx, dz
