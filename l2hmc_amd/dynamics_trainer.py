"""Training step of the generic L2HMC sampler on the toy targets (second half):
  l2hmc/mog_model.py:324-355  _create_loss   (squared jump distance of the x and z chains)
  l2hmc/mog_model.py:357-363  _create_optimizer (AdamOptimizer.minimize)
  l2hmc/mog_model.py:183-192  exponential_decay learning rate
Forward, loss and the whole reverse pass run in ONE library call (l2hmc_small_train_step); a layer-by-layer dynamics
(`Dynamics.layered`: any x_dim, num_nodes or energy) runs a taped forward and a hand-written reverse pass through the
layered kernels instead (l2hmc_amd/layered_train.py), into the same gradient buffer.  The flat buffer, the stacking of
the x and z chains and the Adam step are the lattice trainer's (l2hmc_amd/_flat_trainer.py).  Chains run in the
direction `propose` picks for them (sampler.py:35-41 multiplies the other direction by an exact 0)."""
import ctypes as C

import torch

from . import _lib, ops
from . import layered_train as _layered_train
from ._flat_trainer import FlatTrainer, stack_chains
from .dist import active as _active_dist


class DynamicsTrainer(FlatTrainer):
    STEP_NAME = 'alpha'

    def __init__(self, dynamics, lr_init=1e-2, lr_decay_steps=2500, lr_decay_rate=0.96, scale=0.1, dist=None,
                 beta1=0.9, beta2=0.999, epsilon=1e-8):
        if dynamics.hmc:
            raise ValueError("hmc=True dynamics have no trainable networks")
        dyn = dynamics
        self.scale = float(scale)
        self.lr_init, self.lr_decay_steps, self.lr_decay_rate = float(lr_init), int(lr_decay_steps), float(lr_decay_rate)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.dist = _active_dist(dist)
        self.world = self.dist.get_world_size() if self.dist is not None else 1
        super().__init__(dyn, (dyn.XNet, dyn.VNet),                            # [xnet | vnet | alpha]
                         dyn.alpha.detach().to(dyn._device, torch.float32).reshape(1).clone())
        self._layered = None

    def _write_step(self):
        self.dynamics.alpha = self._step_dev.detach().cpu().reshape(())

    def _step_trainable(self):
        return bool(self.dynamics.eps_trainable)

    def learning_rate(self):
        return self.lr_init * self.lr_decay_rate ** (self.global_step // self.lr_decay_steps)

    def calc_loss_and_grads(self, x, z=None, draws_x=None, draws_z=None):
        """-> (loss, x_out, px).  draws_*: optional (init_v_forward, init_v_backward, dir_bits (1 = forward), u)."""
        dyn = self.dynamics
        dev = dyn._device
        x = _lib.as_dev(x, dev).reshape(-1, dyn.x_dim)
        B, D = x.shape
        z = dyn._normal((B, D)) if z is None else _lib.as_dev(z, dev).reshape(B, D)

        def uniform(n):
            out = ops.fill_uniform(n, dyn._seed, dyn._draws, dev)
            dyn._draws += 1
            return out

        def draw(d):
            if d is None:
                return dyn._normal((B, D)), dyn._normal((B, D)), (uniform(B) >= 0.5).to(torch.float32), uniform(B)
            return tuple(_lib.as_dev(a, dev) for a in d)
        x0, v0, fwd, dirs, u_x = stack_chains(x, z, draw(draws_x), draw(draws_z))
        R = 2 * B
        if dyn.layered:          # decided per call: a test (or a caller) may switch a dynamics to the layered path
            if self._layered is None:
                self._layered = _layered_train.LayeredStep(self)
            xN, p, terms = self._layered(x0, v0, fwd, 1.0 / (B * self.world))
        else:
            xN, vN = torch.empty_like(x0), torch.empty_like(x0)
            p, terms = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(2))
            plan, L = dyn._plan(), _lib.lib()
            ws, nb = self._ws.get(L.l2hmc_small_train_ws_bytes(C.byref(plan), R), dev)
            _lib.call("l2hmc_small_train_step", C.byref(plan), x0, v0, dirs, R, self.scale, 1.0 / (B * self.world), xN,
                      vN, p, terms, self.grads, ws, nb, device=dev)
        self.grads[-1] *= float(dyn.eps)              # d/d alpha = eps * d/d eps  (utils/dynamics.py:51-60)
        buf = torch.stack([terms.sum(dtype=torch.float32), torch.full((), float(B), dtype=torch.float32, device=dev)])
        if self.dist is not None:
            self.dist.all_reduce(buf, op=self.dist.ReduceOp.SUM)
            self.dist.all_reduce(self.grads, op=self.dist.ReduceOp.SUM)
        loss = buf[0] / buf[1]
        px, Lx = p[:B], xN[:B]
        x_out = torch.where(((px - u_x) >= 0)[:, None], Lx, x)       # sampler.py:57-59
        self.last_terms, self.last_proposals, self.last_p = terms, xN, p
        return loss, x_out, px
