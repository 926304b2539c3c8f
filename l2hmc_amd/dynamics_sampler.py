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
chain, so that "HMC at three eps" is one call.

`ais` is the reference's annealed importance sampling (utils/ais.py) on such a dynamics, `steps_per_launch` annealing
steps per launch (l2hmc_small_ais_run, the geometry of the plain-HMC run): an estimate of a normalising constant.

`run_hmc_exchange` is `run_hmc` on a temperature ladder with replica exchange (parallel tempering) between the rungs,
the rounds inside the launch (l2hmc_small_hmc_run_exchange: a replica group sits in one wave); `swap_replicas` is one
round on its own (l2hmc_small_replica_swap).

`run_exchange` is `run(temperature=)` of an L2HMC dynamics on such a ladder with that round after every `swap_every`
steps: by default the host composition of the two (one launch per piece between two rounds and one per round, any
group of up to 64 rungs), and with `in_launch = True` the rounds inside the launches (l2hmc_small_run_exchange: groups
of 2..8 rungs, which sit in the eight chains of a wave), one launch per chunk whatever `swap_every` is.  The values are
the same, bit for bit."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _runs
from .sampler import propose


def replica_swap(dyn, x, temps_dev, chain_stride, G, parity, replica=None):
    """ONE replica-exchange round of l2hmc_small_replica_swap on device state x [B, x_dim], IN PLACE, at the float32
    device temperatures `temps_dev` (column c at temps_dev[c * chain_stride]); the uniforms are one stream of the
    dynamics' counter (`_draws`, then + 1); `replica` (int32 [B] on the device, or None) is exchanged too.  What
    `DynamicsSampler.swap_replicas` and `DynamicsTrainer.train` run.  -> (swap_p, swapped bool, energy), each [B]."""
    B = x.shape[0]
    plan = dyn._plan()
    swap_p = torch.empty(B, dtype=torch.float32, device=x.device)
    swapped = torch.empty(B, dtype=torch.uint8, device=x.device)
    energy = torch.full((B,), float("nan"), dtype=torch.float32, device=x.device)
    _lib.call("l2hmc_small_replica_swap", C.byref(plan), x, B, G, parity, temps_dev, chain_stride, dyn._seed,
              dyn._draws, replica, energy, swap_p, swapped, device=dyn._device)
    dyn._draws += 1
    return swap_p, swapped.view(torch.bool), energy


LAYERED_SWAP_MESSAGE = ("swap_replicas: this dynamics runs layer by layer (arbitrary energy function or "
                        "x_dim > 8): the round needs a packed target")


class DynamicsSampler:
    def __init__(self, dynamics, distribution=None, batch_size=None):
        """`distribution`: anything with `get_samples(n)` (l2hmc_amd.distributions), the start of
        `generate_trajectories`.  `batch_size`: the number of chains `run` starts when no `x` is given."""
        self.dynamics = dynamics
        self.distribution = distribution
        self.batch_size = batch_size
        # MCMC steps per launch of l2hmc_small_run (1 = one launch per step through `propose`, the cross-check)
        self.steps_per_launch = 256
        # `run_exchange`: False = one launch per round between the launches of the run (groups of up to MAX_REPLICAS
        # rungs); True = the rounds inside the run's launches (l2hmc_small_run_exchange), where `exchange_in_launch`
        # says so
        self.in_launch = False
        # int32 [B] labels on the device while an exchange run is followed (`run_hmc_exchange`, `run_exchange`)
        self.replica = None

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
        x = _runs.position(x, dyn.x_dim, dyn._device, f"DynamicsSampler.{who}")
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
        return _runs.rows_from(_lib.as_dev(temps[0], dev), temps[1:])

    def _run_launches(self, run_steps, x, keep_samples, plan, entry, middle, streams, cut_every=None, after=None):
        """ONE launch of `entry` per chunk (`_runs.run_chunks`, which takes `cut_every` and `after`), `streams` per
        step: the same values as `_run_loop`, bit for bit.  `middle(s0)`: what the entry takes between n_steps and px
        for a chunk from step s0 on."""
        dyn = self.dynamics
        B = x.shape[0]
        px = torch.empty(run_steps, B, dtype=torch.float32, device=x.device)

        def launch(s0, n, x_in, x_next, samples_dev):
            # the chunk's first stream is the counter as it stands at this launch, and the counter moves only after
            # the entry returned: a failed launch leaves it where it was
            _lib.call(entry, C.byref(plan), x_in, x_next, B, dyn._seed, dyn._draws, n, *middle(s0), px[s0:],
                      samples_dev, device=dyn._device)
            dyn._draws += streams * n

        out = _runs.run_chunks(run_steps, x, self.steps_per_launch, keep_samples, launch, cut_every, after)
        out["px"] = px.cpu().numpy()
        return out

    def _check_hmc(self, who):
        """What `run_hmc` and `run_hmc_exchange` (`who`) refuse of the dynamics."""
        dyn = self.dynamics
        if not dyn.hmc:
            raise ValueError(f"{who}: the dynamics is an L2HMC sampler (hmc=False): `run` runs it, in one launch per "
                             "chunk where the one-launch kernel holds it")
        if dyn.layered:
            raise NotImplementedError(
                f"{who}: this hmc dynamics runs layer by layer (arbitrary energy function or x_dim > 8), which the "
                "one-launch kernel does not hold: `run` takes it through the loop over `propose`")

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
        self._check_hmc("run_hmc")
        run_steps, x, temps = self._start("run_hmc", run_steps, x, temperature)
        step = None if eps is None else _runs.step_sizes(eps, x.shape[0])
        if run_steps == 0:
            return self._finish(_runs.empty_run(("px",), x, keep_samples))
        plan, eps_chain = _runs.plan_with_step_sizes(dyn, step, x.device)
        temps_from = self._temps_from(temps, x.device)
        return self._finish(self._run_launches(run_steps, x, keep_samples, plan, "l2hmc_small_hmc_run",
                                               lambda s0: (*temps_from(s0), eps_chain), streams=2))

    # ------------------------------------------------------------------------------------------ annealed importance sampling
    @staticmethod
    def ais_schedule(anneal_steps, betas=None, who="ais"):
        """`ais`'s `betas` -> the float32 array [anneal_steps] of b_1 .. b_n.  None: the reference's schedule
        (utils/ais.py:43: linspace(0, 1, n + 1)[1:]), formed in float32.  ValueError for another shape and for an entry
        that, in float32, is not finite, lies outside [0, 1] or is smaller than the one before."""
        n = int(anneal_steps)
        if n != anneal_steps or n < 1:
            raise ValueError(f"{who}: anneal_steps={anneal_steps} must be a whole number, 1 or more")
        if betas is None:
            return np.linspace(0., 1., n + 1, dtype=np.float32)[1:]
        v, b = _runs._float32(betas)
        if b.shape != (n,):
            raise ValueError(f"{who}: betas of shape {v.shape}: expected [{n}] (b_1 .. b_n; b_0 = 0)")
        if not (np.isfinite(b) & (b >= 0) & (b <= 1)).all() or (np.diff(b) < 0).any():
            raise ValueError(f"{who}: betas must be finite, in [0, 1] and non-decreasing (in float32)")
        return np.ascontiguousarray(b)

    def ais(self, anneal_steps, init, x, betas=None, refresh=None):
        """Annealed importance sampling (utils/ais.py:30-82, after Wu et al. 2016) from `init`, a `Gaussian`, to the
        dynamics' target at the dynamics' temperature, with the transitions of this plain-HMC dynamics (`hmc=True`: its
        masks, eps, trajectory_length), `steps_per_launch` annealing steps per launch (l2hmc_small_ais_run): an
        estimate of log(Z1 / Z0), Z = integral of exp(-E).  `x` [B, x_dim]: the chains' starts, drawn from `init` by the
        caller (the reference's `initial_x`); it is not advanced in place.  With b_0 = 0 and b_1 <= .. <= b_n = `betas`
        (None: linspace(0, 1, n + 1)[1:] in float32), step s adds (b_s - b_{s-1}) (E0(x) - E1(x)) to the chain's log
        weight, draws a momentum and runs one Metropolis-Hastings HMC step on (1 - b_s) E0 + b_s E1.
        `refresh`: None -- a fresh N(0, I) momentum every step; a float rho in (0, 1] -- the momentum persists as
        v sqrt(1 - rho) + n sqrt(rho), n ~ N(0, I), from a start v that is one `fill_normal` stream of the dynamics'
        counter; an accepted step keeps the proposed momentum and a rejected one its negative (DESIGN.md quirk list).
        Draws: `_draws` advances by 2 per step (momenta or noise, uniforms), plus 1 with `refresh`.  Any
        `steps_per_launch` gives the same bits.  Returns a dictionary:
          log_w [B] float64         the chains' log weights
          log_ratio                 logsumexp(log_w) - log(B): the estimate of log(Z1 / Z0)
          log_z                     log_ratio + 0.5 logdet(2 pi Sigma_init): the estimate of log Z1
          se                        the delta-method standard error of log_ratio, std(w~, ddof=1) / (sqrt(B) mean(w~))
                                    with w~ = exp(log_w - max log_w)
          ess                       (sum w~)^2 / sum w~^2
          px [n, B], mean_accept    every step's accept probabilities and their mean
          samples_out [B, x_dim]    the final state on the device;  v_out [B, x_dim] with `refresh`
        ValueError for an L2HMC dynamics, an `init` that is no `Gaussian` of the dynamics' dimension, a bad schedule or
        `refresh`, and a `dynamics.temperature` other than 1 on a dynamics built with use_temperature=False (which
        ignores it); NotImplementedError for a dynamics that runs layer by layer.  All before any draw."""
        from . import ops
        from .distributions import Gaussian
        who, dyn = "ais", self.dynamics
        self._check_hmc(who)
        if not dyn.use_temperature and float(dyn.temperature) != 1.0:
            raise ValueError(f"{who}: temperature={dyn.temperature} on a Dynamics built with use_temperature=False, "
                             "which ignores temperatures (Dynamics._temp): build it with use_temperature=True")
        if not isinstance(init, Gaussian) or np.shape(init.mu) != (dyn.x_dim,):
            raise ValueError(f"{who}: init must be a Gaussian of dimension {dyn.x_dim} (the chains start from its "
                             f"samples): got {type(init).__name__}"
                             + (f" of dimension {np.shape(init.mu)}" if isinstance(init, Gaussian) else ""))
        sched = self.ais_schedule(anneal_steps, betas, who)
        n = sched.shape[0]
        if refresh is not None:
            ok = not isinstance(refresh, bool) and np.ndim(refresh) == 0
            rho = float(np.float32(refresh)) if ok else float("nan")
            if not (0.0 < rho <= 1.0):
                raise ValueError(f"{who}: refresh={refresh}: expected None (fresh momenta) or a number in (0, 1]")
        if x is None:
            raise ValueError(f"{who}: pass the start `x` [B, {dyn.x_dim}], drawn from init")
        x = _runs.position(x, dyn.x_dim, dyn._device, "DynamicsSampler.ais")
        B, dev = x.shape[0], x.device
        plan = dyn._plan()
        init_target = init.get_energy_function().target.to(dev)      # (kept alive until the last launch returned)
        init_struct = init_target.struct(1.0)
        betas_dev = _lib.as_dev(np.concatenate([np.zeros(1, np.float32), sched]), dev)
        log_w = torch.zeros(B, dtype=torch.float64, device=dev)
        px = torch.empty(n, B, dtype=torch.float32, device=dev)
        # the start momentum is the stream at the counter; the counter moves only after a launch returned
        v = None if refresh is None else ops.fill_normal((B, dyn.x_dim), dyn._seed, dyn._draws, dev)
        taken = [0 if v is None else 1]                            # streams taken ahead of the next launch

        def launch(s0, m, x_in, x_next, _):
            _lib.call("l2hmc_small_ais_run", C.byref(plan), C.byref(init_struct), x_in, x_next, v,
                      0.0 if refresh is None else rho, B, dyn._seed, dyn._draws + taken[0], m, betas_dev[s0:],
                      log_w.data_ptr(), px[s0:], device=dyn._device)
            dyn._draws += taken[0] + 2 * m
            taken[0] = 0

        out = _runs.run_chunks(n, x, self.steps_per_launch, False, launch)
        out["px"] = px.cpu().numpy()
        out["log_w"] = lw = log_w.cpu().numpy()
        if refresh is not None:
            out["v_out"] = v
        with np.errstate(all="ignore"):
            top = lw.max() if B else np.float64("nan")
            wt = np.exp(lw - top)
            mean = wt.mean() if B else np.float64("nan")
            out["log_ratio"] = float(top + np.log(mean))
            out["se"] = float(wt.std(ddof=1) / (np.sqrt(B) * mean)) if B > 1 else float("nan")
            out["ess"] = float(wt.sum() ** 2 / np.square(wt).sum()) if B else float("nan")
        out["log_z"] = out["log_ratio"] + 0.5 * float(np.linalg.slogdet(2 * np.pi * np.asarray(init.sigma, np.float64))[1])
        return self._finish(out)

    # ------------------------------------------------------------------------------------------ replica exchange
    MAX_REPLICAS = 64               # a replica group sits in one wave (l2hmc_small_replica_swap)
    MAX_REPLICAS_IN_LAUNCH = 8       # ... in the eight chains of a wave of the L2HMC kernel (l2hmc_small_run_exchange)

    def exchange_in_launch(self, replicas):
        """Whether `run_exchange(..., replicas=replicas)` with `self.in_launch = True` is served: the dynamics is on the
        one-launch path (L2HMC, not layer by layer, steps_per_launch > 1) and a group has 2..8 rungs."""
        try:
            G = int(replicas)
        except (TypeError, ValueError):
            return False
        return self._one_launch() and G == replicas and 2 <= G <= self.MAX_REPLICAS_IN_LAUNCH

    def _exchange_args(self, who, run_steps, x, temperature, replicas, swap_every, first_parity, replica0):
        """What the two exchange runs (`who`) check alike, before any launch -> (run_steps, start on the device,
        `_temperatures`, the run's `_runs.Exchange`)."""
        if temperature is None:
            raise ValueError(f"{who}: replicas={replicas} without temperature=: the rungs of a replica group are the "
                             "columns of a temperature ladder")
        run_steps, x, temps = self._start(who, run_steps, x, temperature)
        B = x.shape[0]
        G, k, fp, _ = _runs.check_replicas(replicas, B, swap_every, first_parity, who=who, most=self.MAX_REPLICAS)
        return run_steps, x, temps, _runs.Exchange(G, k, fp, _runs.replica_labels(replica0, B, who), B)

    def run_hmc_exchange(self, run_steps, x=None, keep_samples=True, temperature=None, eps=None, replicas=None,
                         swap_every=1, first_parity=0, replica0=None):
        """`run_hmc` with replica exchange (parallel tempering) between the columns of a temperature ladder, the rounds
        INSIDE the launch (l2hmc_small_hmc_run_exchange): still one launch per chunk of `steps_per_launch` steps, with
        an exchange after every step if asked.  `replicas=None`: `run_hmc` itself, bit for bit (the other three
        arguments are then ignored).  `replicas=G` (2..64): columns [g * G, (g + 1) * G) are one group of G rungs and
        `temperature` is required, in any shape `run_hmc` takes (a scalar makes every exchange certain).  After every
        MCMC step s (counting from 1) with s % swap_every == 0 -- the last step of the call included -- ONE round runs
        on the state that step left, with parity (first_parity + s // swap_every - 1) % 2 and the temperatures step s
        ran with: the pairs (j, j + 1), j = parity, parity + 2, ... of every group trade places with probability
        min(1, exp((1 / T_a - 1 / T_b)(U_a - U_b))), U the target's energy at temperature 1.  Temperature and eps
        belong to the COLUMN: states move, rungs stay.  The run is the loop `run_hmc(swap_every, ...)`,
        `swap_replicas(...)`, bit for bit, and takes the same draws (2 streams per step, 1 per round).  `samples[s]` is
        what step s wrote, before any round; `samples_out` the state after the last round.  Added to `run_hmc`'s
        dictionary, named and shaped as `GaugeSampler.run_hmc_exchange`'s (n_r = run_steps // swap_every rounds):
          swap_p [n_r, B] float32   p at the lower chain of every proposed pair, NaN elsewhere
          swapped [n_r, B] bool
          replica [n_r, B] int32    the label of the state that sits in column c after the round; labels start as
                                    arange(B), or as `replica0` (the last row of an earlier call: a run continues with
                                    first_parity = (first_parity + n_r) % 2 of that call)
          swap_rate [G - 1]         the mean of `swapped` over rounds and groups for each neighbouring pair of rungs
        `self.replica` keeps the labels on the device; `stats.replica_round_trips` reads `replica`.  ValueError, on top
        of `run_hmc`'s, for replicas outside 2..64, a batch that is no multiple of it, swap_every < 1, first_parity
        not 0 or 1, a replica0 that is not int32 [B], and replicas without a temperature."""
        if replicas is None:
            return self.run_hmc(run_steps, x, keep_samples, temperature, eps)
        who, dyn = "run_hmc_exchange", self.dynamics
        self._check_hmc(who)
        run_steps, x, temps, exchange = self._exchange_args(who, run_steps, x, temperature, replicas, swap_every,
                                                            first_parity, replica0)
        B = x.shape[0]
        step = None if eps is None else _runs.step_sizes(eps, B, who)
        if run_steps == 0:
            return self._finish(exchange.finish(_runs.empty_run(("px",), x, keep_samples)))
        plan, eps_chain = _runs.plan_with_step_sizes(dyn, step, x.device)
        temps_from = self._temps_from(temps, x.device)
        self.replica = exchange.start(x.device)
        exchange.in_launch(run_steps, x.device)
        px = torch.empty(run_steps, B, dtype=torch.float32, device=x.device)

        def launch(s0, n, x_in, x_next, samples_dev):
            # a chunk may end inside a swap period: it passes where in the period it starts and its first round's
            # parity, and moves the counter by its steps' streams and its rounds'
            place, hist, n_rounds = exchange.chunk(s0, n)
            _lib.call("l2hmc_small_hmc_run_exchange", C.byref(plan), x_in, x_next, B, dyn._seed, dyn._draws, n,
                      *temps_from(s0), eps_chain, *place, self.replica, px[s0:], samples_dev, *hist, device=dyn._device)
            dyn._draws += 2 * n + n_rounds

        out = _runs.run_chunks(run_steps, x, self.steps_per_launch, keep_samples, launch)
        out["px"] = px.cpu().numpy()
        return self._finish(exchange.finish(out))

    def swap_replicas(self, x, temperature, replicas, parity):
        """ONE replica-exchange round on device state x [B, x_dim], IN PLACE (l2hmc_small_replica_swap), for a
        plain-HMC and an L2HMC dynamics on a packed target alike: columns [g * replicas, (g + 1) * replicas) are one
        group, column c at temperature[c] (`temperature`: a scalar, [B] or [1, B]); the round of `parity` 0 / 1
        proposes the pairs (j, j + 1), j = parity, parity + 2, ... of every group and exchanges two rows with
        probability min(1, exp((1 / T_a - 1 / T_b)(U_a - U_b))), U the target's energy at temperature 1.  The uniforms
        are one stream of the dynamics' counter (`_draws`, then + 1).  If the sampler keeps labels (`self.replica`,
        int32 [B] on the device) the round exchanges them too.  Returns (swap_p [B], NaN off the lower chain of a pair;
        swapped [B] bool; energy [B], U of the chains that were in a pair, NaN elsewhere) as tensors."""
        dyn = self.dynamics
        if dyn.layered:
            raise NotImplementedError(LAYERED_SWAP_MESSAGE)
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"swap_replicas: x: expected a device tensor [B, {dyn.x_dim}] (exchanged in place)")
        _lib.expect_shape(x, (None, dyn.x_dim), "x", "DynamicsSampler.swap_replicas")     # (in place: no other form)
        B = x.shape[0]
        G, _, _, parity = _runs.check_replicas(replicas, B, parity=parity, who="swap_replicas", most=self.MAX_REPLICAS)
        replica = getattr(self, "replica", None)
        if replica is not None and tuple(replica.shape) != (B,):
            raise ValueError(f"swap_replicas: the sampler's labels are {tuple(replica.shape)}: expected [{B}] (or None)")
        temps_dev, stride = _runs.per_chain(temperature, B, x.device, who="swap_replicas", name="temperature",
                                            scalar="a scalar", sign="> 0")
        return self._swap_round(x, temps_dev, stride, G, parity)

    def _swap_round(self, x, temps_dev, chain_stride, G, parity):
        return replica_swap(self.dynamics, x, temps_dev, chain_stride, G, parity, getattr(self, "replica", None))

    def run_exchange(self, run_steps, x=None, keep_samples=True, temperature=None, replicas=None, swap_every=1,
                     first_parity=0, replica0=None):
        """`run(..., temperature=)` of an L2HMC dynamics with replica exchange between the columns of the ladder: the
        loop `run(swap_every, temperature=)`, `swap_replicas(...)`, bit for bit, with its draws (4 streams per step, 1
        per round).  Arguments and the added entries of the dictionary as `run_hmc_exchange`; `replicas=None` is `run`
        itself.
        `self.in_launch = False` (the default): the run is cut at the multiples of `swap_every` steps (one launch of
        l2hmc_small_run_tempered per piece of at most `steps_per_launch` steps) and every round is a launch of its own
        (`swap_replicas`); groups of up to 64 rungs.
        `self.in_launch = True` (an attribute of the sampler, like `steps_per_launch`; the signature is what it was):
        the rounds run INSIDE the launches (l2hmc_small_run_exchange) -- chunks of `steps_per_launch` steps that are
        not cut at the rounds, no launch per round, the same dictionary and the same `self.replica`, bit for bit.
        Served for groups of 2..8 rungs (`exchange_in_launch(replicas)`): the L2HMC kernel gives a chain eight lanes
        and a wave eight chains, so a group of up to 8 rungs sits in one wave and a larger one does not;
        NotImplementedError for a larger group, before any launch.  A group size that does not divide 8 leaves some of
        a wave's eight places idle (3 rungs: 6 of 8 used) and launches more waves: on batches that fill the chip and
        with rounds many steps apart the round between launches can be the faster form (README).
        ValueError for a plain-HMC dynamics (`run_hmc_exchange` runs it); NotImplementedError where `run` has no
        one-launch path (layer by layer, steps_per_launch = 1)."""
        if replicas is None:
            return self.run(run_steps, x, keep_samples, temperature)
        who, dyn = "run_exchange", self.dynamics
        if dyn.hmc:
            raise ValueError(f"{who}: the dynamics is a plain-HMC sampler (hmc=True): `run_hmc_exchange` runs it, with "
                             "the rounds inside the launch")
        if not self._one_launch():
            raise NotImplementedError(
                f"{who}: temperatures per chain need the one-launch path (an L2HMC dynamics the one-launch kernel "
                "holds: not layer by layer, and steps_per_launch > 1)")
        run_steps, x, temps, exchange = self._exchange_args(who, run_steps, x, temperature, replicas, swap_every,
                                                            first_parity, replica0)
        in_launch = bool(self.in_launch)
        if in_launch and not self.exchange_in_launch(exchange.G):
            raise NotImplementedError(
                f"{who} with in_launch = True: replicas={exchange.G}: a replica group sits in the eight chains of one "
                f"wave of the L2HMC kernel, so it has {self.MAX_REPLICAS_IN_LAUNCH} rungs at the most "
                "(`exchange_in_launch(replicas)`); in_launch = False takes groups of up to "
                f"{self.MAX_REPLICAS} rungs")
        if run_steps == 0:
            return self._finish(exchange.finish(_runs.empty_run(("px",), x, keep_samples)))
        self.replica = exchange.start(x.device)
        temps_from = self._temps_from(temps, x.device)
        if in_launch:
            return self._finish(exchange.finish(self._run_exchange_launches(run_steps, x, keep_samples, temps_from,
                                                                            exchange)))
        # a round takes one stream of the dynamics' counter; the next chunk reads the counter when it is launched
        out = self._run_launches(run_steps, x, keep_samples, dyn._plan(), "l2hmc_small_run_tempered", temps_from,
                                 streams=4, cut_every=exchange.k, after=exchange.between(self._swap_round, temps_from))
        return self._finish(exchange.finish(out))

    def _run_exchange_launches(self, run_steps, x, keep_samples, temps_from, exchange):
        """`run_exchange` with the rounds inside the launches: ONE launch of l2hmc_small_run_exchange per chunk of
        `steps_per_launch` steps, as `run_hmc_exchange` launches its entry."""
        dyn = self.dynamics
        B = x.shape[0]
        plan = dyn._plan()
        exchange.in_launch(run_steps, x.device)
        px = torch.empty(run_steps, B, dtype=torch.float32, device=x.device)

        def launch(s0, n, x_in, x_next, samples_dev):
            # a chunk may end inside a swap period: it passes where in the period it starts and its first round's
            # parity, and moves the counter by its steps' streams and its rounds', after the entry returned
            place, hist, n_rounds = exchange.chunk(s0, n)
            _lib.call("l2hmc_small_run_exchange", C.byref(plan), x_in, x_next, B, dyn._seed, dyn._draws, n,
                      *temps_from(s0), *place, self.replica, px[s0:], samples_dev, *hist, device=dyn._device)
            dyn._draws += 4 * n + n_rounds

        out = _runs.run_chunks(run_steps, x, self.steps_per_launch, keep_samples, launch)
        out["px"] = px.cpu().numpy()
        return out

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
        x = _runs.position(x, dyn.x_dim, dyn._device, "DynamicsSampler.generate_trajectories")
        saved = dyn.temperature
        dyn.temperature = temp
        try:
            out = self.run(num_steps, x, keep_samples=True)
        finally:
            dyn.temperature = saved
        start = x.cpu().numpy()[None]
        return np.concatenate([start, out["samples"]])[:int(num_steps)], out["px"]
