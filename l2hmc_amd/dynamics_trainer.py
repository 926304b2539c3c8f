"""Training step of the generic L2HMC sampler on the toy targets (second half):
  l2hmc/mog_model.py:324-355  _create_loss   (squared jump distance of the x and z chains)
  l2hmc/mog_model.py:357-363  _create_optimizer (AdamOptimizer.minimize)
  l2hmc/mog_model.py:183-192  exponential_decay learning rate
Forward, loss and the whole reverse pass run in ONE library call (l2hmc_small_train_step); a layer-by-layer dynamics
(`Dynamics.layered`: any x_dim, num_nodes or energy) runs a taped forward and a hand-written reverse pass through the
layered kernels instead (l2hmc_amd/layered_train.py), into the same gradient buffer.  The flat buffer, the stacking of
the x and z chains and the Adam step are the lattice trainer's (l2hmc_amd/_flat_trainer.py).  Chains run in the
direction `propose` picks for them (sampler.py:35-41 multiplies the other direction by an exact 0).

Temperature (mog_model.py:917-943 feeds one per step and anneals it): `calc_loss_and_grads` / `train_step` take
`temperature=` -- None (the dynamics' own), a scalar, or a LADDER [B]: chain i of the x batch and chain i of the z batch
then train at temperature[i] in the same one launch (l2hmc_small_train_step_tempered, a LADDER instance of the kernel
that reads the row's temperature from a device array), so one pair of networks is trained for every rung of a
replica-exchange run.  `train` is the reference's annealed loop, rung by rung for a ladder, with exchange rounds between
the steps on the samplers' schedule (`replicas=`)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _runs, ops
from . import layered_train as _layered_train
from ._flat_trainer import FlatTrainer, check_draws, stack_chains
from .dist import active as _active_dist
from .dynamics_sampler import LAYERED_SWAP_MESSAGE, DynamicsSampler, replica_swap


def _anneal(temp, step, annealing_steps, annealing_factor):
    """One turn of mog_model.py:940-943 after the step with index `step`, elementwise (float64): -> (the new value,
    whether an update was due and no entry could fall further -- the reference's exit)."""
    if step % int(annealing_steps) != 0:
        return temp, False
    lower = temp * float(annealing_factor)
    falls = lower > 1.
    return np.where(falls, lower, temp), not bool(np.any(falls))


def temperature_schedule(step, temp_init, annealing_steps, annealing_factor):
    """The temperature the step with index `step` trains at when step 0 trains at `temp_init` (a scalar or an array:
    elementwise, float64) -- the reference's recurrence (mog_model.py:940-943): after every step s with
    s % annealing_steps == 0 the value is multiplied by annealing_factor, and keeps its old value wherever the product
    would not be > 1.  A ladder anneals rung by rung, and a rung at 1 stays at 1."""
    temp = np.asarray(temp_init, dtype=np.float64)
    for s in range(0, int(step), int(annealing_steps)):          # the steps before `step` an update follows
        temp, _ = _anneal(temp, s, annealing_steps, annealing_factor)
    return temp if temp.ndim else float(temp)


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

    def _chain_temperatures(self, temperature, B, who):
        """`temperature=` of a step -> (scalar or None, ladder or None): None for the dynamics' own; a number or a 0-d
        array / tensor -> its float32 value as a float; [B] or [1, B] -> the ladder as a float32 device tensor [B]
        (`_runs.per_chain`: a float32 tensor of that shape on the device stays there, unchecked).  ValueError for
        another shape, for a value that in float32 is not finite or not > 0, and for any temperature on a dynamics
        built with use_temperature=False."""
        if temperature is None:
            return None, None
        dyn = self.dynamics
        if not dyn.use_temperature:
            raise ValueError(f"{who}: temperature= on a Dynamics built with use_temperature=False, which ignores "
                             "temperatures (Dynamics._temp): build it with use_temperature=True")
        if _runs.ndim(temperature) == 0:
            t32 = np.float32(float(temperature))
            if not (np.isfinite(t32) and t32 > 0):
                raise ValueError(f"{who}: every temperature must be finite and > 0 (in float32)")
            return float(temperature), None
        return None, _runs.per_chain(temperature, B, dyn._device, who=who, name="temperature", sign="> 0")[0]

    def calc_loss_and_grads(self, x, z=None, draws_x=None, draws_z=None, temperature=None):
        """-> (loss, x_out, px).  draws_*: optional (init_v_forward, init_v_backward, dir_bits (1 = forward), u).
        temperature: None = the step at the dynamics' own temperature (`Dynamics._temp`); a scalar = that step at this
        temperature (on a copy of the plan: `dynamics.temperature` stays as it was); [B] or [1, B] = a LADDER: chain i
        of the x batch and chain i of the z batch train at temperature[i] (l2hmc_small_train_step_tempered; a
        layer-by-layer dynamics scales the temperature-1 force, energy and Hessian product per row).  Draws, the loss,
        its normalisation 1 / (B * world), the all-reduce and the outputs are the scalar step's.  ValueError before any
        draw is taken for another shape, a value that in float32 is not finite or not > 0, and any temperature on a
        dynamics built with use_temperature=False."""
        dyn = self.dynamics
        dev = dyn._device
        x = _lib.as_dev(x, dev).reshape(-1, dyn.x_dim)
        B, D = x.shape
        who = "DynamicsTrainer.calc_loss_and_grads"
        t_scalar, t_ladder = self._chain_temperatures(temperature, B, who)
        _lib.expect_shape(z, (B, D), "z", who)                           # (every shape, before the first draw)
        check_draws(draws_x, B, D, "draws_x", who)
        check_draws(draws_z, B, D, "draws_z", who)
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
            if t_scalar is not None:         # the layered stages read the dynamics' temperature: set, and put back
                saved, dyn.temperature = dyn.temperature, t_scalar
                try:
                    xN, p, terms = self._layered(x0, v0, fwd, 1.0 / (B * self.world))
                finally:
                    dyn.temperature = saved
            else:                            # rows i and B + i at temperature[i]
                xN, p, terms = self._layered(x0, v0, fwd, 1.0 / (B * self.world),
                                             None if t_ladder is None else t_ladder.repeat(2))
        else:
            xN, vN = torch.empty_like(x0), torch.empty_like(x0)
            p, terms = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(2))
            plan, L = dyn._plan(), _lib.lib()
            if t_scalar is not None:         # into this struct alone, as _runs.plan_with_step_sizes treats eps
                plan.target.temperature = t_scalar
            ws, nb = self._ws.get(L.l2hmc_small_train_ws_bytes(C.byref(plan), R), dev)
            tail = (x0, v0, dirs, R, self.scale, 1.0 / (B * self.world), xN, vN, p, terms, self.grads, ws, nb)
            if t_ladder is None:
                _lib.call("l2hmc_small_train_step", C.byref(plan), *tail, device=dev)
            else:
                _lib.call("l2hmc_small_train_step_tempered", C.byref(plan), t_ladder, 1, B, *tail, device=dev)
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

    temperature_schedule = staticmethod(temperature_schedule)

    def train(self, train_steps, x, temp_init=1.0, annealing_steps=200, annealing_factor=0.98, replicas=None,
              swap_every=1, stop_when_annealed=False, print_steps=0, log=print):
        """mog_model.py:917-943 without the file side effects: per step `train_step` at the current temperature, the
        Metropolis-Hastings output as the next x, an exchange round if one is due, then the annealing update
        (`temperature_schedule`'s recurrence).  temp_init: a scalar, or [B] -- a ladder, trained in one launch per step
        and annealed rung by rung.  Returns per-step NumPy histories 'loss', 'accept_prob', 'eps', 'lr' and
        'temperature' ([steps], or [steps, B] for a ladder) and 'samples', the final state on the device.
        stop_when_annealed=True ends the run after the first step at which an update is due and no entry of the
        temperature can fall further (the reference's exit); the default runs all steps.
        replicas=G: replica exchange between the rungs WHILE the networks train -- the samplers' schedule
        (`_runs.Exchange`, first parity 0): columns [g G, (g + 1) G) are one group; after every step s (from 1 within
        the call) with s % swap_every == 0 ONE round of l2hmc_small_replica_swap runs on the x chains at the
        temperatures that step ran with, taking one stream of the dynamics' counter (`DynamicsSampler.swap_replicas`'s
        round, bit for bit).  The dictionary gains 'swap_rate' [G - 1] and 'swapped' [rounds, B].  A group lives on
        one rank; the gradient all-reduce is what it was.  NotImplementedError for a layer-by-layer dynamics, before
        the first step."""
        dyn = self.dynamics
        dev = dyn._device
        x = _lib.as_dev(x, dev).reshape(-1, dyn.x_dim).clone()
        B = x.shape[0]
        temp = np.asarray(temp_init.detach().cpu().numpy() if isinstance(temp_init, torch.Tensor) else temp_init,
                          dtype=np.float64)
        if temp.shape not in ((), (B,)):
            raise ValueError(f"DynamicsTrainer.train: temp_init of shape {temp.shape}: expected a scalar or [{B}]")
        ladder = temp.ndim > 0
        # a dynamics built with use_temperature=False trains at 1, which the default schedule never leaves
        plain = not dyn.use_temperature and not ladder and float(temp) == 1.0
        if not plain:
            self._chain_temperatures(temp, B, "DynamicsTrainer.train")       # ValueError before the first step
        ex = None
        if replicas is not None:
            if dyn.layered:
                raise NotImplementedError(LAYERED_SWAP_MESSAGE)
            G, k, _, _ = _runs.check_replicas(replicas, B, swap_every, who="DynamicsTrainer.train",
                                               most=DynamicsSampler.MAX_REPLICAS)
            ex = _runs.Exchange(G, k, 0, None, B)
        hist = {k: [] for k in ("loss", "accept_prob", "eps", "lr", "temperature")}
        for step in range(int(train_steps)):
            lr = self.learning_rate()
            # (a ladder goes to the device once per step: the step and the round read the same float32 values)
            t_dev = self._chain_temperatures(temp, B, "DynamicsTrainer.train")[1] if ladder else None
            loss, x, px = self.train_step(x, temperature=None if plain else float(temp) if t_dev is None else t_dev)
            parity = ex.parity_after(step + 1) if ex is not None else None
            if parity is not None:
                if t_dev is None:
                    t_dev = torch.full((B,), float(temp), dtype=torch.float32, device=dev)
                _, swapped, _ = replica_swap(dyn, x, t_dev, 1, ex.G, parity)
                ex.rounds["swapped"].append(swapped)
            hist["loss"].append(loss)
            hist["accept_prob"].append(px.mean())
            hist["eps"].append(float(dyn.eps))
            hist["lr"].append(lr)
            hist["temperature"].append(temp if ladder else float(temp))
            if print_steps and step % print_steps == 0:
                log(f"{step:>5g}/{train_steps:<6g} loss {float(loss):^9.4g} acc {float(px.mean()):^9.4g} "
                    f"eps {float(dyn.eps):^9.4g} temp {float(np.mean(temp)):^9.4g} lr {lr:^9.4g}")
            temp, annealed = _anneal(temp, step, annealing_steps, annealing_factor)
            if stop_when_annealed and annealed:
                break
        out = {k: (torch.stack(v).cpu().numpy() if v and isinstance(v[0], torch.Tensor) else np.asarray(v))
               for k, v in hist.items()}
        out["samples"] = x
        if ex is not None:       # (the trainer keeps no labels: of the samplers' histories, `swapped` and its rate)
            ex.rounds["swap_p"], ex.rounds["replica"] = [], []
            rounds = ex.finish({})
            out["swapped"], out["swap_rate"] = rounds["swapped"], rounds["swap_rate"]
        return out
