"""Device-resident sampling loop: the step harness around the hot path
(l2hmc/gauge_model.py:1304-1460 `GaugeModel.run`, the inference half of SURVEY.md 8f/f3).

The reference runs one `sess.run` per MCMC step, copying the whole sample batch host<->device through
`feed_dict` and wrapping it with `np.mod(., 2*pi)` on the host (:1371-1388).  Here the chain state never
leaves HBM: transition -> wrap -> per-step observables are all library calls on device buffers, and the
per-step scalars of all ranks are combined by one small asynchronous all-reduce (l2hmc_amd/dist.py)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _runs, ops
from .dist import StepStats
from .lattice import replica_swap, u1_observables, u1_plaq_exact


class GaugeSampler:
    def __init__(self, dynamics, beta_init=2., beta_final=4., train_steps=10000, dist=None, reduce_every=16):
        self.dynamics = dynamics
        self.lattice = dynamics.lattice
        self.beta_init, self.beta_final, self.train_steps = beta_init, beta_final, train_steps
        # (reduce_every: MCMC steps whose scalar sums share one all-reduce when sharded; l2hmc_amd/dist.py)
        self.stats = StepStats(dynamics._device, dist, reduce_every=reduce_every)
        # [sum p, sum |dQ|, B, ticket] per step: the fused step kernel needs the ticket at 0 on entry and leaves it
        # at 0, so the rows of one zero-initialised ring are handed out in turn (longer than StepStats' backlog)
        self._sums_ring = torch.zeros(256, 4, dtype=torch.float32, device=dynamics._device)
        self._sums_next = 0
        # plain-HMC runs on a plan with the one-launch kernel: MCMC steps per launch of l2hmc_gauge_hmc_run
        # (1 = one launch per step through `step`, the cross-check)
        self.steps_per_launch = 256
        self._run_sums = None        # [steps][4] like _sums_ring: zeroed once, the kernel leaves the tickets at 0
        # int32 [B] on the device, or None: the label of the configuration that sits in every column.  Every
        # replica-exchange round (`swap_replicas`) exchanges it with the rows; `run_hmc_exchange` starts it anew
        self.replica = None
        # `run_hmc_exchange`: False = one launch per round between the launches of the run (every lattice and group);
        # True = the rounds inside the run's launches (l2hmc_gauge_hmc_run_exchange), where `exchange_in_launch` says so
        self.in_launch = False

    def update_beta(self, step):
        """gauge_model.py:1039-1046: linear annealing of 1/beta."""
        temp = ((1. / self.beta_init - 1. / self.beta_final) * (1. - step / float(self.train_steps))
                + 1. / self.beta_final)
        return 1. / temp

    def wrap(self, x):
        return ops.wrap_angle(x)

    def step(self, x, beta):
        """One MCMC step on device state x: [B, x_dim].  Returns (x_next, px, observables of x, |dQ|);
        as in the reference the action / plaquette / charge ops look at the step's INPUT samples
        (gauge_model.py:256-266) and dQ compares input and output (:718-725).  Runs as ONE library call
        (l2hmc_gauge_mcmc_step: draws + trajectories + mix/accept + observables + wrap).  With
        `dynamics.both_directions = False` the plan carries L2HMC_PLAN_SELECTED_ONLY: each chain is integrated
        only in the direction its coin picks -- same random streams, same chains, half the work.
        `beta`: a float, or for an L2HMC dynamics one value per chain -- [B] or [1, B] as a list / array (checked:
        finite and not negative in float32), or a float32 tensor [B] or [1, B] on x's device, which is used as it is
        (`_runs.per_chain`; l2hmc_gauge_mcmc_step_ladder: chain c has the bits of the step of the whole batch at beta[c])."""
        x = _runs.position(x, self.dynamics.x_dim, self.dynamics._device, "GaugeSampler.step")
        if _runs.ndim(beta) == 0:
            return self._step(x, beta)
        if self.dynamics.hmc:                              # (ValueErrors before any draw)
            raise ValueError("step: a beta per chain on a plain-HMC dynamics (hmc=True): `run_hmc` runs it")
        return self._step(x, None, _runs.per_chain(beta, x.shape[0], x.device, who="step", name="beta", scalar="a float",
                                                   sign="not negative", hint=" (one per chain)")[0])

    def _step(self, x, beta, beta_dev=None):
        """`step` on checked arguments: at the float `beta`, or with `beta_dev` (float32 [B] on the device, may be a
        view) at a beta per chain."""
        dyn = self.dynamics
        x_next = torch.empty_like(x)                       # written by the step (out of place: no copy of x)
        B = x.shape[0]
        outs = {k: torch.empty(B, dtype=torch.float32, device=x.device)
                for k in ("px", "action", "avg_plaq", "top_charge", "dq")}
        sums = self._sums_ring[self._sums_next]                  # [sum p, sum |dQ|, B, ticket], filled in-kernel
        self._sums_next = (self._sums_next + 1) % self._sums_ring.shape[0]
        plan, L = dyn._plan(), _lib.lib()
        ws, nb = dyn._ws.get(L.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B), x.device)
        # the step's random streams come from the dynamics' own draw counter (saved / restored with the state):
        # a sampler never replays noise the dynamics, a trainer or another sampler on the same dynamics used
        draw, dyn._draws = _lib.step_draw_index(dyn._draws)
        entry, front = (("l2hmc_gauge_mcmc_step_ex", (float(beta),)) if beta_dev is None else
                        ("l2hmc_gauge_mcmc_step_ladder", (beta_dev, 1)))
        _lib.call(entry, C.byref(plan), *front, x, x_next, B, dyn._seed, draw, outs["px"],
                  outs["action"], outs["avg_plaq"], outs["top_charge"], outs["dq"], sums, ws, nb, device=dyn._device)
        self.stats.push_sums(sums[:3])
        return x_next, outs["px"], outs, outs["dq"]

    def _step_composed(self, x, beta):
        """The same step from the separate public ops (used for selected-only mode and as a cross-check)."""
        T, X = self.lattice.time_size, self.lattice.space_size
        _, _, px, x_out = self.dynamics(x, beta)
        obs = u1_observables(x, T, X)
        x_next = self.wrap(x_out)
        dq = torch.abs(u1_observables(x_out, T, X)["top_charge"] - obs["top_charge"])
        self.stats.push(px, dq)
        return x_next, px, obs, dq

    METRICS = {'l1': 0, 'l2': 1, 'cos': 2, 'cos2': 3, 'cos_diff': 4}

    def calc_loss(self, x, beta, metric='cos_diff', loss_scale=1., z=None, **weights):
        """gauge_model.py:728-797 `_calc_loss`, forward value: (loss, x_out, px, x_dq).  Two transitions (on x
        and on the auxiliary z ~ N(0,1)), the per-chain terms in one kernel, and the mean over the chains of
        ALL ranks through one all-reduce of [sum, count] -- the collective north_star asks for."""
        if metric not in self.METRICS:        # :653-655
            raise AttributeError(f"metric={metric}. Expected one of: 'l1', 'l2', 'cos', 'cos2', or 'cos_diff'.")
        dyn = self.dynamics
        T, X = self.lattice.time_size, self.lattice.space_size
        x = _runs.position(x, dyn.x_dim, dyn._device, "GaugeSampler.calc_loss")
        if z is not None:                                  # (refused before the x transition takes its draws)
            z = _runs.position(z, dyn.x_dim, dyn._device, "GaugeSampler.calc_loss", "z", x.shape[0])
        x_prop, _, px, x_out = dyn(x, beta)
        z = dyn._normal(tuple(x.shape)) if z is None else z
        _, _, pz, _ = dyn(z, beta)
        terms = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        _lib.call("l2hmc_gauge_loss_terms", x, x_prop, px, z, pz, x.shape[0], T, X, self.METRICS[metric],
                  float(loss_scale), float(weights.get('aux_weight', 1.)), float(weights.get('std_weight', 1.)),
                  float(weights.get('charge_weight', 1.)), terms, device=dyn._device)
        buf = torch.stack([terms.sum(dtype=torch.float32),
                           torch.full((), float(terms.numel()), dtype=torch.float32, device=x.device)])
        if self.stats.dist is not None:
            self.stats.dist.all_reduce(buf, op=self.stats.dist.ReduceOp.SUM)
        loss = buf[0] / buf[1]
        q0 = u1_observables(x, T, X)["top_charge"]
        q1 = u1_observables(x_out, T, X)["top_charge"]
        x_dq = torch.abs(q0 - q1).to(torch.int32)          # :762-763
        self.last_loss_terms = terms
        return loss, x_out, px, x_dq

    def run(self, run_steps, beta, x=None, keep_samples=False):
        """:1304-1460 without the file/plot side effects.  Starts from N(0,1) samples like the reference
        (:1354) unless `x` is given.  Returns per-step histories as NumPy arrays [steps, B].  `beta`: a float, or a
        sequence of `run_steps` values (one per step; `plaq_exact` is then taken at the last).  Plain HMC on a plan
        with the one-launch kernel runs `steps_per_launch` steps per launch (`_run_chunks`): the same values.
        For an L2HMC dynamics `beta` may also have a chain axis, [1, B] (one per chain) or [run_steps, B]
        (`_runs.chain_axis`): a scan of the trained sampler over beta in ONE run (l2hmc_gauge_mcmc_step_ladder per
        step).  Chains never interact, so column c of every history is `run` of the whole batch at that column's betas,
        bit for bit; `plaq_exact` is then a [B] array at the last step's betas.  ValueError for such a beta of another
        shape, with an entry that is negative or not finite, and on a plain-HMC dynamics (`run_hmc` runs those)."""
        dyn = self.dynamics
        if _runs.ndim(beta) > 1:
            return self._exchange_run(*self._start("run", run_steps, beta, x)[:3], keep_samples)
        if x is None:
            x = _lib.as_dev(np.random.randn(dyn.batch_size, dyn.x_dim), dyn._device)
        else:
            x = _runs.position(x, dyn.x_dim, dyn._device, "GaugeSampler.run")
        per_step = _runs.ndim(beta) > 0
        betas = [float(b) for b in beta] if per_step else [beta] * run_steps
        if len(betas) != run_steps:
            raise ValueError(f"beta: expected a float or {run_steps} values, got {len(betas)}")
        if (run_steps > 0 and dyn.hmc and int(self.steps_per_launch) > 1
                and _lib.lib().l2hmc_gauge_plan_fused(C.byref(dyn._plan())) == 1):
            # l2hmc_gauge_hmc_run: the same draws, histories, sums and samples as the loop below, bit for bit
            beta_dev = torch.tensor(betas, dtype=torch.float32, device=x.device)
            out = self._run_chunks(run_steps, x, keep_samples, dyn._plan(), "l2hmc_gauge_hmc_run",
                                   lambda s0: (beta_dev[s0:],))
            out["plaq_exact"] = u1_plaq_exact(betas[-1])
            return out
        out = self._run_steps(run_steps, x, keep_samples, lambda i, x_now: self.step(x_now, betas[i]))
        out["plaq_exact"] = u1_plaq_exact(betas[-1] if per_step else beta)
        return out

    def _run_steps(self, run_steps, x, keep_samples, step, after=None):
        """The loop over `step(i, x) -> (x_next, px, obs, dq)`, a launch per step: `run`'s dictionary less
        `plaq_exact`.  `after(s, x)`, called behind step s (from 1) once its sample is kept, returns the state the
        next step starts from."""
        hist = {k: [] for k in ("px", "actions", "plaqs", "charges", "charge_diff")}
        samples = []
        for i in range(run_steps):
            x, px, obs, dq = step(i, x)
            hist["px"].append(px)
            hist["actions"].append(obs["action"])
            hist["plaqs"].append(obs["avg_plaq"])
            hist["charges"].append(obs["top_charge"])
            hist["charge_diff"].append(dq)
            if keep_samples:
                samples.append(x)
            if after is not None:
                x = after(i + 1, x)
        out = {k: torch.stack(v).cpu().numpy() for k, v in hist.items()}
        out["samples_out"] = x
        out["mean_accept"] = self.stats.mean_accept()
        if keep_samples:
            out["samples"] = torch.stack(samples).cpu().numpy()
        return out

    HISTORIES = ("px", "actions", "plaqs", "charges", "charge_diff")

    def _start(self, who, run_steps, beta, x, eps=None):
        """What `run` with a chain axis on beta, `run_exchange` and `run_hmc` (`who`; `run_hmc_exchange` checks as
        `run_hmc`) refuse, before any draw or plan -> (run_steps, start on the device, `_runs.chain_axis` of beta,
        `_runs.step_sizes` of eps or None)."""
        dyn = self.dynamics
        if who == "run_hmc" and not dyn.hmc:
            raise ValueError("run_hmc: the dynamics is an L2HMC sampler (hmc=False): `run` runs it")
        if who != "run_hmc" and dyn.hmc:
            raise ValueError(f"{who}: the dynamics is plain HMC (hmc=True): "
                             f"`{'run_hmc_exchange' if who == 'run_exchange' else 'run_hmc'}` runs its ladders")
        run_steps = int(run_steps)
        if run_steps < 0:
            raise ValueError(f"run_steps={run_steps} must not be negative")
        _lib.expect_shape(x, (None, dyn.x_dim), "x", f"GaugeSampler.{who}", fold=True)
        shape = (dyn.batch_size, dyn.x_dim) if x is None else (np.shape(x)[0], dyn.x_dim)
        betas = _runs.chain_axis(beta, run_steps, shape[0], who=who, name="beta", positive=False)
        step = None if eps is None else _runs.step_sizes(eps, shape[0])
        x = _runs.position(np.random.randn(*shape) if x is None else x, dyn.x_dim, dyn._device, f"GaugeSampler.{who}")
        return run_steps, x, betas, step

    def _ladder_frame(self, run_steps, x, betas, keep_samples, body):
        """What the runs at the betas of `_runs.chain_axis` share: the empty run; `body(rows)` for 1 step or more,
        `rows` the `_runs.rows_from` of the betas, which go to the device once; `plaq_exact` at the last step's beta, a
        float, or a [B] array where beta has a chain axis."""
        b64, b32, strides = betas
        if run_steps == 0:
            out = _runs.empty_run(self.HISTORIES, x, keep_samples)
            out["mean_accept"] = self.stats.mean_accept()
        else:
            out = body(_runs.rows_from(_lib.as_dev(b32, x.device), strides))
        last = _runs.last_step(b64)
        out["plaq_exact"] = u1_plaq_exact(float(last)) if last.ndim == 0 else u1_plaq_exact(last)
        return out

    def _exchange_run(self, run_steps, x, betas, keep_samples, exchange=None):
        """`run` at the betas of `_runs.chain_axis` on checked arguments, a launch per step, which takes its row view
        (or, without a chain axis, its float); with an `exchange` (`_runs.Exchange`) its rounds between the steps."""
        b32, (step_stride, chain_stride) = betas[1:]

        def body(rows):
            def step(i, x_now):
                if chain_stride:
                    return self._step(x_now, None, rows(i)[0])
                return self._step(x_now, float(b32[i * step_stride]))

            after = None
            if exchange is not None:
                self.replica = exchange.start(x.device)
                # (the round is in place: with `keep_samples` it gets a copy and the step's output stays the sample)
                after = exchange.between(self._swap_round, rows, clone=keep_samples)
            return self._run_steps(run_steps, x, keep_samples, step, after)

        return self._ladder_frame(run_steps, x, betas, keep_samples, body)

    def run_exchange(self, run_steps, beta, x=None, keep_samples=False, replicas=None, swap_every=1, first_parity=0,
                     replica0=None):
        """`run` of an L2HMC dynamics with replica exchange (parallel tempering) between the columns of a ladder: the
        trained sampler, tempered.  `beta` as `run` takes it -- usually [1, B], G rungs repeated B / G times.
        `replicas=None`: `run` itself, bit for bit (the other three arguments are then ignored).  `replicas=G`: columns
        [g * G, (g + 1) * G) are one group of G rungs.  After every MCMC step s (counting from 1) with
        s % swap_every == 0 -- the last step of the call included -- ONE round (`swap_replicas`) runs on the state that
        step left, with parity (first_parity + s // swap_every - 1) % 2 and the betas step s ran with.  Beta belongs to
        the COLUMN: configurations move, rungs stay.  The run is the loop `run(swap_every, ...)`,
        `swap_replicas(...)`, bit for bit, on the dynamics' one draw counter: a step takes the next even-aligned pair
        of streams, a round the next stream.  Every L2HMC step is a launch of its own anyway, so the rounds are launches
        of their own between them (l2hmc_gauge_replica_swap) -- there is no in-launch form here, and `in_launch` is not
        read.  `samples[s]` is what step s wrote, before any round; `samples_out` the state after the last round.
        Added to `run`'s dictionary, as in `run_hmc_exchange` (n_r = run_steps // swap_every rounds): swap_p [n_r, B]
        float32 (p at the lower chain of every proposed pair, NaN elsewhere), swapped [n_r, B] bool, replica [n_r, B]
        int32 (the label of the configuration in column c after the round; labels start as arange(B) or as `replica0`,
        the last row of an earlier call, which continues with first_parity = (first_parity + n_r) % 2 of that call;
        `self.replica` holds them on the device) and swap_rate [G - 1].  Nothing is exchanged between ranks.
        ValueError, before any draw or plan: a plain-HMC dynamics (`run_hmc_exchange` runs those), what `run` refuses,
        replicas < 2, a batch that is no multiple of it, swap_every < 1, first_parity not 0 or 1, a replica0 that is
        not int32 [B]."""
        if replicas is None and _runs.ndim(beta) <= 1:
            if self.dynamics.hmc:
                raise ValueError("run_exchange: the dynamics is plain HMC (hmc=True): `run_hmc_exchange` runs its "
                                 "ladders")
            return self.run(run_steps, beta, x, keep_samples)
        run_steps, x, betas, _ = self._start("run_exchange", run_steps, beta, x)
        if replicas is None:
            return self._exchange_run(run_steps, x, betas, keep_samples)
        exchange = self._exchange(x.shape[0], replicas, swap_every, first_parity, replica0, "run_exchange")
        return exchange.finish(self._exchange_run(run_steps, x, betas, keep_samples, exchange))

    @staticmethod
    def _exchange(B, replicas, swap_every, first_parity, replica0, who):
        """The checked replica-exchange arguments of a run (`who`) of B chains as its `_runs.Exchange`."""
        G, k, parity0, _ = _runs.check_replicas(replicas, B, swap_every, first_parity, who=who)
        return _runs.Exchange(G, k, parity0, _runs.replica_labels(replica0, B, who), B)

    def _run_chunks(self, run_steps, x, keep_samples, plan, entry, front, cut_every=None, after=None, exchange=None):
        """Plain-HMC steps through `_runs.run_chunks` (`cut_every`, `after`: see there), ONE launch of `entry` per
        chunk: l2hmc_gauge_hmc_run or l2hmc_gauge_hmc_run_ladder; `front(s0)` is what it takes between the plan and x_in
        for a chunk from step s0 on.  Histories, `_run_sums`, workspace: once per run.  `run`'s dictionary less
        `plaq_exact`.  With an `exchange` (`_runs.Exchange`, `in_launch`) the entry is l2hmc_gauge_hmc_run_exchange,
        whose chunks are not cut at the rounds: a round follows every k-th step of the run inside the launch, and
        `exchange.chunk` places every chunk in that schedule; the labels are `self.replica`."""
        dyn = self.dynamics
        B, dev = x.shape[0], x.device
        hist = {k: torch.empty(run_steps, B, dtype=torch.float32, device=dev) for k in self.HISTORIES}
        if self._run_sums is None or self._run_sums.shape[0] < run_steps or self._run_sums.device != dev:
            self._run_sums = torch.zeros(run_steps, 4, dtype=torch.float32, device=dev)
        sums = self._run_sums
        chunk = _runs.chunk_length(run_steps, self.steps_per_launch)
        ws, nb = dyn._ws.get(getattr(_lib.lib(), entry + "_ws_bytes")(C.byref(plan), B, chunk), dev)

        def launch(s0, n, x_in, x_next, samples_dev):
            # the draw index comes from the dynamics' counter as it stands when the chunk is launched: consecutive from
            # chunk to chunk unless `after` took a stream in between (then the next even-aligned pair).  The counter
            # moves only after the entry returned: a failed launch leaves it where it was
            if exchange is None:
                (draw, draws_after), mid, tail = _lib.run_draw_index(dyn._draws, n), (), ()
            else:
                place, tail, _ = exchange.chunk(s0, n)
                draw, _, draws_after = _lib.exchange_run_draw_index(dyn._draws, n, *place[1:3])
                mid = (*place, self.replica)
            _lib.call(entry, C.byref(plan), *front(s0), x_in, x_next, B, dyn._seed, draw, n, *mid,
                      *(hist[k][s0:] for k in self.HISTORIES), sums[s0:], samples_dev, *tail, ws, nb,
                      device=dyn._device)
            dyn._draws = draws_after
            for i in range(s0, s0 + n):
                self.stats.push_sums(sums[i, :3])

        out = _runs.run_chunks(run_steps, x, self.steps_per_launch, keep_samples, launch, cut_every, after)
        out.update((k, v.cpu().numpy()) for k, v in hist.items())
        out["mean_accept"] = self.stats.mean_accept()
        return out

    def run_hmc(self, run_steps, beta, x=None, eps=None, keep_samples=False):
        """`run` for a plain-HMC dynamics (`hmc=True`) with a chain axis on beta and on the step size: a scan over
        either, or a grid of both, in ONE launch per chunk of `steps_per_launch` steps (l2hmc_gauge_hmc_run_ladder).
        `beta`: a scalar, [run_steps] (one per step), [1, B] (one per chain) or [run_steps, B].  `eps`: None (the
        dynamics' own), a scalar, or [B].  Chains never interact, so column c of every history is the run of the whole
        batch at that column's beta and eps -- `run` on a dynamics with that eps -- bit for bit.  Returns the dictionary
        of `run`; `plaq_exact` is a float where beta has no chain axis and a [B] array (at the last step's beta)
        where it has one.  Draws from the dynamics' counter as `run` does; the caller's `x`, `dynamics.eps` and the
        dynamics' plan are left as they were.  ValueError for an L2HMC dynamics, a wrong shape, a beta that is negative
        or not finite and an eps that is not finite and > 0; NotImplementedError for an hmc dynamics whose plan has no
        one-launch kernel (more than 1024 sites, `fused = False`): `run` takes those, one beta at a time.
        `run_hmc_exchange` is this run with replica exchange between the columns of a ladder."""
        return self._ladder_run(*self._start("run_hmc", run_steps, beta, x, eps), keep_samples)

    def _ladder_run(self, run_steps, x, betas, step, keep_samples, exchange=None, in_launch=False):
        """What `run_hmc` means, on checked arguments; with an `exchange` (`_runs.Exchange`) its rounds, between the
        launches of the run or with `in_launch` inside them."""
        def body(rows):
            plan, eps_chain = _runs.plan_with_step_sizes(self.dynamics, step, x.device)
            if _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan)) != 1:
                raise NotImplementedError(
                    "run_hmc: this hmc dynamics has no one-launch kernel (more than 1024 sites, or fused = False): "
                    "`run` takes it through the loop over `step`, one beta at a time")
            args = (run_steps, x, keep_samples, plan)
            front = lambda s0: (*rows(s0), eps_chain)
            if exchange is None:
                return self._run_chunks(*args, "l2hmc_gauge_hmc_run_ladder", front)
            self.replica = exchange.start(x.device)        # stays on the device from chunk to chunk
            if in_launch:
                exchange.in_launch(run_steps, x.device)
                return self._run_chunks(*args, "l2hmc_gauge_hmc_run_exchange", front, exchange=exchange)
            # chunks cut at the multiples of k steps, one round after each of them: it takes one stream of the
            # dynamics' counter, and the next chunk reads the counter when it is launched
            return self._run_chunks(*args, "l2hmc_gauge_hmc_run_ladder", front, exchange.k,
                                    exchange.between(self._swap_round, rows))

        return self._ladder_frame(run_steps, x, betas, keep_samples, body)

    def swap_replicas(self, x, beta, replicas, parity):
        """ONE replica-exchange round on device state x [B, x_dim], IN PLACE (l2hmc_gauge_replica_swap): columns
        [g * replicas, (g + 1) * replicas) are one group, column c at beta[c] (`beta`: [B] or [1, B]); the round of
        `parity` 0 / 1 proposes the pairs (j, j + 1), j = parity, parity + 2, ... of every group and exchanges two rows
        with probability min(1, exp((beta_a - beta_b)(S_a - S_b))).  The uniforms are one stream of the dynamics'
        counter, taken as `GaugeDynamics._uniform` takes it.  If the sampler keeps labels (`self.replica`, int32 [B]
        on the device) the round exchanges them too.  Returns (swap_p [B], NaN off the lower chain of a pair;
        swapped [B] bool; action [B], sum (1 - cos P) of the chains that were in a pair, NaN elsewhere) as tensors."""
        dyn = self.dynamics
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"swap_replicas: x: expected a device tensor [B, {dyn.x_dim}] (exchanged in place)")
        _lib.expect_shape(x, (None, dyn.x_dim), "x", "GaugeSampler.swap_replicas")        # (in place: no other form)
        B = x.shape[0]
        G, _, _, parity = _runs.check_replicas(replicas, B, parity=parity, who="swap_replicas")
        beta_dev, _ = _runs.per_chain(beta, B, x.device, who="swap_replicas", name="beta")
        return self._swap_round(x, beta_dev, 1, G, parity)

    def _swap_round(self, x, beta_dev, chain_stride, G, parity):
        dyn = self.dynamics
        T, X = self.lattice.time_size, self.lattice.space_size
        out = replica_swap(x, T, X, G, parity, beta_dev, dyn._seed, dyn._draws, chain_stride, self.replica)
        dyn._draws += 1                                    # one stream, as GaugeDynamics._uniform
        return out

    def exchange_in_launch(self, replicas):
        """Whether `run_hmc_exchange(..., replicas=replicas)` with `self.in_launch = True` is served for this dynamics
        (l2hmc_gauge_hmc_run_exchange_served): a workgroup of at most 1024 threads has to hold whole groups."""
        try:
            G = int(replicas)
        except (TypeError, ValueError):
            return False
        if G != replicas or not self.dynamics.hmc:
            return False
        return _lib.lib().l2hmc_gauge_hmc_run_exchange_served(C.byref(self.dynamics._plan()), G) == 1

    def run_hmc_exchange(self, run_steps, beta, x=None, eps=None, keep_samples=False, replicas=None, swap_every=1,
                         first_parity=0, replica0=None):
        """`run_hmc` with replica exchange (parallel tempering) between the columns of a ladder.  `replicas=None`:
        `run_hmc` itself, bit for bit (the other three arguments are then ignored).  `replicas=G`: columns
        [g * G, (g + 1) * G) are one group of G rungs.  After every MCMC step s (counting from 1) with
        s % swap_every == 0 -- the last step of the call included -- ONE round (`swap_replicas`) runs on the state that
        step left, with parity (first_parity + s // swap_every - 1) % 2 and the betas step s ran with.  beta and eps
        belong to the COLUMN: configurations move, rungs stay.  A launch of the run kernel never spans a round and never
        exceeds `steps_per_launch` steps; the run is the loop `run_hmc(swap_every, ...)`, `swap_replicas(...)`, bit
        for bit.  `samples[s]` is what step s wrote, before any round; `samples_out` the state after the last round.
        Added to `run_hmc`'s dictionary (n_r = run_steps // swap_every rounds):
          swap_p [n_r, B] float32   p at the lower chain of every proposed pair, NaN elsewhere
          swapped [n_r, B] bool
          replica [n_r, B] int32    the label of the configuration that sits in column c after the round; labels start
                                    as arange(B), or as `replica0` (the last row of an earlier call: a run continues
                                    with first_parity = (first_parity + n_r) % 2 of that call)
          swap_rate [G - 1]         the mean of `swapped` over rounds and groups for each neighbouring pair of rungs (a
                                    pair is proposed in every other round)
        With `self.in_launch = True` (an attribute of the sampler, like `steps_per_launch`; the signature is what it was)
        the rounds run INSIDE the launches of the run (l2hmc_gauge_hmc_run_exchange) -- chunks of
        `steps_per_launch` steps that are not cut at the rounds, no launch per round, the same dictionary and the same
        `self.replica`, bit for bit.  Served where a workgroup of at most 1024 threads holds whole groups
        (`exchange_in_launch(replicas)`: e.g. up to 8 rungs at 8x8, 2 at 16x16, none at 32x32); NotImplementedError
        elsewhere.  The default stays the round between launches, which serves every lattice and group.
        Nothing is exchanged between ranks: a group lives on one rank.  ValueError, on top of `run_hmc`'s, for
        replicas < 2, a batch that is no multiple of it, swap_every < 1, first_parity not 0 or 1, and a replica0 that
        is not int32 [B]."""
        run_steps, x, betas, step = self._start("run_hmc", run_steps, beta, x, eps)
        if replicas is None:
            return self._ladder_run(run_steps, x, betas, step, keep_samples)
        exchange = self._exchange(x.shape[0], replicas, swap_every, first_parity, replica0, "run_hmc_exchange")
        in_launch = bool(self.in_launch)
        if in_launch and not self.exchange_in_launch(exchange.G):
            raise NotImplementedError(
                "run_hmc_exchange with in_launch = True: " + _lib.lib().l2hmc_last_error().decode()
                + ".  The rule: lcm(replicas, chains per workgroup of the ladder run) x rows per chain x threads per "
                "row must not exceed 1024, on a lattice of at most 512 sites whose plan has the one-launch kernel "
                "(`exchange_in_launch(replicas)`); in_launch = False takes every lattice and group")
        return exchange.finish(self._ladder_run(run_steps, x, betas, step, keep_samples, exchange, in_launch))

    @staticmethod
    def run_dicts(out, beta):
        """`run()` histories -> the four dicts the reference pickles per run (gauge_model.py:1409-1413, :1758-1822:
        actions / plaqs / charges / charge_diff keyed by (step, beta)), for a caller that wants the reference's
        in-memory layout; this package itself writes .npz (save_run)."""
        n = out["px"].shape[0]
        keys = [(i, beta) for i in range(n)]
        return tuple({k: out[name][i] for i, k in enumerate(keys)}
                     for name in ("actions", "plaqs", "charges", "charge_diff"))

    def save_run(self, out, out_dir, beta, therm_frac=10):
        """gauge_model.py:1758-2033 (`_save_run_info`) without pickles: the histories returned by `run` go to
        `observables_steps_{n}_beta_{beta}.npz` and a readable summary -- per-chain means and standard errors of
        action, plaquette, topological charge and susceptibility after dropping the first steps // therm_frac
        steps, the charge histogram, mean accept probability, plaquette vs the exact value, integrated
        autocorrelation time of the plaquette -- to `statistics_steps_{n}_beta_{beta}.txt`.  Returns both paths."""
        import os
        from . import stats
        os.makedirs(out_dir, exist_ok=True)
        n = int(out["px"].shape[0])
        arrays = {k: np.asarray(v) for k, v in out.items()
                  if k in ("px", "actions", "plaqs", "charges", "charge_diff", "samples")}
        arrays["samples_out"] = out["samples_out"].detach().cpu().numpy()
        arrays["beta"], arrays["plaq_exact"] = np.float64(beta), np.float64(out["plaq_exact"])
        npz = os.path.join(out_dir, f"observables_steps_{n}_beta_{beta}.npz")
        np.savez_compressed(npz, **arrays)
        (am, ae), (pm, pe), (qm, qe), (sm, se), probs = stats.calc_observables_stats(
            out["actions"], out["plaqs"], out["charges"], therm_frac=therm_frac)
        therm = n // therm_frac
        try:
            tau = float(stats.integrated_time(out["plaqs"][therm:, :, None], quiet=True)[0][0])
        except Exception:      # noqa: BLE001 -- too short a run for the estimator
            tau = float("nan")
        lines = [f"run of {n} steps, {out['px'].shape[1]} chains, beta = {beta}, thermalisation cut {therm} steps",
                 f"mean accept probability      : {float(np.mean(out['px'][therm:])):.6f}",
                 f"average plaquette            : {float(pm.mean()):.6f} +/- {float(np.sqrt(np.mean(pe ** 2) / len(pe))):.6f}"
                 f"   (exact {float(out['plaq_exact']):.6f}, difference {float(pm.mean() - out['plaq_exact']):+.6f})",
                 f"average action               : {float(am.mean()):.6f} +/- {float(np.sqrt(np.mean(ae ** 2) / len(ae))):.6f}",
                 f"topological charge           : {float(qm.mean()):+.6f} +/- {float(np.sqrt(np.mean(qe ** 2) / len(qe))):.6f}",
                 f"topological susceptibility   : {float(sm.mean()):.6f} +/- {float(np.sqrt(np.mean(se ** 2) / len(se))):.6f}",
                 f"tunnelling rate |dQ| / step  : {float(np.mean(out['charge_diff'][therm:])):.6f}",
                 f"tau_int(plaquette)           : {tau:.3f} steps",
                 "charge probabilities         : " + ", ".join(f"{k:+d}: {v:.4f}" for k, v in probs.items())]
        txt = os.path.join(out_dir, f"statistics_steps_{n}_beta_{beta}.txt")
        with open(txt, "w") as f:
            f.write("\n".join(lines) + "\n")
        return npz, txt
