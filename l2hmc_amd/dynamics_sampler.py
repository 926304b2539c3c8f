"""Device-resident sampling loop for the toy-target `Dynamics`: what l2hmc/mog_model.py:394-421
(`GaussianMixtureModel.generate_trajectories`) does with one `sess.run` per MCMC step -- chains started from the target's
own samples, positions and accept probabilities of every step kept -- and the tunnelling-rate / autocorrelation
evaluation of the paper is made of.

An L2HMC dynamics the one-launch kernel holds (packed target, x_dim <= 8, at most 64 hidden units) hands
`steps_per_launch` steps at a time to l2hmc_small_run: ONE launch per chunk, the chains in registers from step to step,
the weights, target, masks and time table staged once.  The values are those of the loop over
`propose(x, dynamics, do_mh_step=True)`, bit for bit, and that loop is what every other dynamics (`hmc`, `layered`) and
`steps_per_launch = 1` run.

`run(..., temperature=)` anneals or ladders the temperature inside such a run (l2hmc_small_run_tempered): one value per
step, per chain, or both, where `dynamics.temperature` is one value for the launch.

`run_hmc` is the plain-HMC baseline in one launch per chunk (l2hmc_small_hmc_run, a kernel of its own: one thread per
chain): the values of `run` on an `hmc=True` dynamics, bit for bit, and beyond them a temperature and a step size per
chain, so that "HMC at three eps" is one call."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _runs
from .sampler import propose


class DynamicsSampler:
    def __init__(self, dynamics, distribution=None, batch_size=None):
        """`distribution`: anything with `get_samples(n)` (l2hmc_amd.distributions), the start of
        `generate_trajectories`.  `batch_size`: the number of chains `run` starts when no `x` is given."""
        self.dynamics = dynamics
        self.distribution = distribution
        self.batch_size = batch_size
        # MCMC steps per launch of l2hmc_small_run (1 = one launch per step through `propose`, the cross-check)
        self.steps_per_launch = 256

    def _one_launch(self):
        dyn = self.dynamics
        return int(self.steps_per_launch) > 1 and not dyn.hmc and not dyn.layered

    def _temperatures(self, temperature, run_steps, B):
        """`run`'s `temperature` by `_runs.chain_axis` -> (flat float32 array, step_stride, chain_stride)."""
        if not self.dynamics.use_temperature:
            raise ValueError("run: temperature= on a Dynamics built with use_temperature=False, which ignores "
                             "temperatures (Dynamics._temp): build it with use_temperature=True")
        _, flat, strides = _runs.chain_axis(temperature, run_steps, B, who="run", name="temperature", positive=True)
        return (flat, *strides)

    def _start(self, who, run_steps, x, temperature):
        """What `run` and `run_hmc` (`who`) check alike -> (run_steps, start on the device, `_temperatures` or None)."""
        dyn, run_steps = self.dynamics, int(run_steps)
        if run_steps < 0:
            raise ValueError(f"run_steps={run_steps} must not be negative")
        if x is None:
            if self.batch_size is None:
                raise ValueError(f"{who}: pass the start `x`, or give the sampler a batch_size to start from N(0, 1)")
            x = np.random.randn(int(self.batch_size), dyn.x_dim)
        x = _lib.as_dev(x, dyn._device).reshape(-1, dyn.x_dim)
        temps = None if temperature is None else self._temperatures(temperature, run_steps, x.shape[0])
        return run_steps, x, temps

    @staticmethod
    def _finish(out):
        px = out["px"]
        out["mean_accept"] = float(px.mean(dtype=np.float64)) if px.size else float("nan")
        return out

    def run(self, run_steps, x=None, keep_samples=True, temperature=None):
        """`run_steps` MCMC steps (utils/sampler.py:28-59 with the Metropolis-Hastings step) from `x` [B, x_dim], or
        from N(0, 1) samples for `batch_size` chains.  Returns {"px": [steps, B] accept probabilities, "samples":
        [steps, B, x_dim] with samples[s] the OUTPUT of step s (if kept), "samples_out": the final state on the
        device, "mean_accept": the mean of this run's px (NaN for an empty run)}.  The caller's `x` is not advanced in
        place.  The draws come from the dynamics' own counter (`_draws`, 4 streams per L2HMC step) and the temperature
        is the dynamics' (`use_temperature` / `temperature`), or `temperature`: a scalar (the whole run), [run_steps]
        (a schedule: step s at temperature[s]), [1, B] (a ladder: chain c at temperature[0, c]) or [run_steps, B]
        (both).  Chains never interact, so the columns of a ladder are independent runs at their own temperatures.
        `dynamics.temperature` is left as it was.  Temperatures per chain need the one-launch path."""
        run_steps, x, temps = self._start("run", run_steps, x, temperature)
        if temps is not None and temps[2] and not self._one_launch():
            raise NotImplementedError(
                "run: temperatures per chain need the one-launch path (an L2HMC dynamics the one-launch kernel holds: "
                "not hmc, not layer by layer, and steps_per_launch > 1); the loop over `propose` has one "
                "`dynamics.temperature` for all chains")
        if run_steps == 0:
            out = _runs.empty_run(("px",), x, keep_samples)
        elif not self._one_launch():
            out = self._run_loop(run_steps, x, keep_samples, temps)
        else:
            plan = self.dynamics._plan()
            entry, middle = "l2hmc_small_run", lambda s0: ()
            if temps is not None:
                entry, middle = "l2hmc_small_run_tempered", self._temps_from(temps, x.device)
            out = self._run_launches(run_steps, x, keep_samples, plan, entry, middle, streams=4)
        return self._finish(out)

    def _run_loop(self, run_steps, x, keep_samples, temps=None):
        """One `propose` per step: any dynamics.  `temps` (one value or a schedule, as `_temperatures` returns it) is
        set on `dynamics.temperature` step by step, and what was there is put back."""
        dyn = self.dynamics
        px_hist, samples = [], []
        saved = dyn.temperature
        try:
            for s in range(run_steps):
                if temps is not None:
                    dyn.temperature = float(temps[0][s * temps[1]])
                _, _, px, (x,) = propose(x, dyn, do_mh_step=True)
                px_hist.append(px)
                if keep_samples:
                    samples.append(x)
        finally:
            dyn.temperature = saved
        out = {"px": torch.stack(px_hist).cpu().numpy(), "samples_out": x}
        if keep_samples:
            out["samples"] = torch.stack(samples).cpu().numpy()
        return out

    @staticmethod
    def _temps_from(temps, dev):
        """s0 -> (the temperatures from step s0 on, step_stride, chain_stride) as the tempered entries take them: the
        array goes to the device once and every chunk starts at its own row.  `temps` None: (NULL, 0, 0)."""
        if temps is None:
            return lambda s0: (None, 0, 0)
        flat, step_stride, chain_stride = temps
        temps_dev = _lib.as_dev(flat, dev)
        return lambda s0: (temps_dev[s0 * step_stride:], step_stride, chain_stride)

    def _run_launches(self, run_steps, x, keep_samples, plan, entry, middle, streams):
        """ONE launch of `entry` per chunk (`_runs.run_chunks`), `streams` per step: the same values as `_run_loop`, bit
        for bit.  `middle(s0)`: what the entry takes between n_steps and px for a chunk from step s0 on."""
        dyn = self.dynamics
        B = x.shape[0]
        px = torch.empty(run_steps, B, dtype=torch.float32, device=x.device)

        def launch(s0, n, x_in, x_next, samples_dev):
            # the chunk's first stream is the counter as it stands at this launch, and the counter moves only after
            # the entry returned: a failed launch leaves it where it was
            _lib.call(entry, C.byref(plan), x_in, x_next, B, dyn._seed, dyn._draws, n, *middle(s0), px[s0:],
                      samples_dev, device=dyn._device)
            dyn._draws += streams * n

        out = _runs.run_chunks(run_steps, x, self.steps_per_launch, keep_samples, launch)
        out["px"] = px.cpu().numpy()
        return out

    def run_hmc(self, run_steps, x=None, keep_samples=True, temperature=None, eps=None):
        """`run` for a plain-HMC dynamics (`hmc=True`) on a packed toy target, `steps_per_launch` steps per launch
        (l2hmc_small_hmc_run): the same dictionary, the same values as `run` gives for that dynamics, bit for bit, and
        the same draws (`_draws`, 2 streams per HMC step: momenta, Metropolis-Hastings uniforms).  The caller's `x` is
        not advanced in place.  `temperature` as in `run`, per chain included.  `eps`: None (the dynamics' own), a
        scalar, or [B], one step size per chain -- chains never interact, so "HMC at three eps" is one call whose
        columns are the runs at each eps.  `dynamics.alpha` and `dynamics.temperature` are left as they were.
        ValueError for an L2HMC dynamics and NotImplementedError for one that runs layer by layer (a callable energy,
        x_dim > 8): `run` takes both."""
        dyn = self.dynamics
        if not dyn.hmc:
            raise ValueError("run_hmc: the dynamics is an L2HMC sampler (hmc=False): `run` runs it, in one launch per "
                             "chunk where the one-launch kernel holds it")
        if dyn.layered:
            raise NotImplementedError(
                "run_hmc: this hmc dynamics runs layer by layer (arbitrary energy function or x_dim > 8), which the "
                "one-launch kernel does not hold: `run` takes it through the loop over `propose`")
        run_steps, x, temps = self._start("run_hmc", run_steps, x, temperature)
        step = None if eps is None else _runs.step_sizes(eps, x.shape[0])
        if run_steps == 0:
            return self._finish(_runs.empty_run(("px",), x, keep_samples))
        plan, eps_chain = _runs.plan_with_step_sizes(dyn, step, x.device)
        temps_from = self._temps_from(temps, x.device)
        return self._finish(self._run_launches(run_steps, x, keep_samples, plan, "l2hmc_small_hmc_run",
                                               lambda s0: (*temps_from(s0), eps_chain), streams=2))

    def generate_trajectories(self, temp=1., num_samples=500, num_steps=100, x=None):
        """mog_model.py:394-421 -> (trajectories [num_steps, num_samples, x_dim], px [num_steps, num_samples]).  As in
        the reference trajectories[s] is the INPUT of step s (:410), so trajectories[0] is the start: `x`, or
        `num_samples` samples of the sampler's distribution (:399).  `temp` is set on `dynamics.temperature` for the
        run and restored afterwards; it takes effect on a dynamics built with use_temperature=True, which is how the
        reference builds its own (:385-387).  The reference's third return value, the training loss of every step, is
        the trainer's business (DynamicsTrainer) and is not produced here.  `num_steps=None`: the trajectory length
        (:396-398)."""
        dyn = self.dynamics
        if num_steps is None:
            num_steps = int(dyn.trajectory_length)
        if x is None:
            if self.distribution is None:
                raise ValueError("generate_trajectories: pass the start `x`, or give the sampler a distribution")
            x = self.distribution.get_samples(int(num_samples))
        x = _lib.as_dev(x, dyn._device).reshape(-1, dyn.x_dim)
        saved = dyn.temperature
        dyn.temperature = temp
        try:
            out = self.run(num_steps, x, keep_samples=True)
        finally:
            dyn.temperature = saved
        start = x.cpu().numpy()[None]
        return np.concatenate([start, out["samples"]])[:int(num_steps)], out["px"]
