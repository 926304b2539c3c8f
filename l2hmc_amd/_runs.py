"""What the "many MCMC steps in one launch" runs of GaugeSampler and DynamicsSampler share, host code only: the rule for
a value with an optional step axis and chain axis, the rule for one value per chain, the step-size rule, the ONE
replica-exchange schedule (`Exchange`), the empty run, and the ONE loop over chunks."""
import numpy as np
import torch

from . import _lib


def _float32(value):
    """tensor / array / list / scalar -> (float64 array as given, the float32 array the device takes)."""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    v = np.asarray(value, dtype=np.float64)
    with np.errstate(over="ignore"):
        return v, v.astype(np.float32)


def ndim(value):
    """Axes of a per-run value as it is given (tensor / array / list / scalar): 0 one value, 1 one per step (`step`: one
    per chain), 2 a chain axis."""
    return value.ndim if isinstance(value, torch.Tensor) else np.ndim(value)


def last_step(v):
    """The last step's entry of a `chain_axis` value (float64, as given): a 0-d array or a [B] array; NaN where an
    empty run has an empty schedule."""
    return v if v.ndim == 0 else v[-1] if v.shape[0] else np.full(v.shape[1:], np.nan)


def chain_axis(value, run_steps, B, *, who, name, positive):
    """A per-run value (beta, temperature) -> (float64 array as given, flat contiguous float32 array for the device,
    (step_stride, chain_stride)): step s of chain c reads flat[s * step_stride + c * chain_stride], the element strides
    of l2hmc_gauge_hmc_run_ladder, l2hmc_small_run_tempered and l2hmc_small_hmc_run.  ValueError for a shape that is
    not in the table and for an entry that, in float32, is not finite or is negative (`positive`: or is 0)."""
    v, v32 = _float32(value)
    # one value, a schedule, both, a ladder over the chains (last: [1, B] of a run of 1 step is read as a ladder)
    strides = {(): (0, 0), (run_steps,): (1, 0), (run_steps, B): (B, 1), (1, B): (0, 1)}
    if v.shape not in strides:
        raise ValueError(f"{who}: {name} of shape {v.shape}: expected a scalar, [{run_steps}] (one per step), "
                         f"[1, {B}] (one per chain) or [{run_steps}, {B}]")
    if not (np.isfinite(v32) & ((v32 > 0) if positive else (v32 >= 0))).all():
        raise ValueError(f"{who}: every {name} must be finite and {'> 0' if positive else 'not negative'} (in float32)")
    return v, np.ascontiguousarray(v32).reshape(-1), strides[v.shape]


def rows_from(flat_dev, strides):
    """s0 -> (the values from step s0's row on, step_stride, chain_stride) as the ladder entries and the rounds take
    them.  `flat_dev`: `chain_axis`' flat array on the device, where it goes once per run; every chunk starts at its own
    row, and the row step s (from 1) ran with is the one from s - 1 on."""
    step_stride, chain_stride = strides
    return lambda s0: (flat_dev[s0 * step_stride:], step_stride, chain_stride)


def position(x, x_dim, device, who, name="x", rows=None):
    """The samplers' gate for a caller's state (GaugeDynamics._x's rule) -> a float32 device tensor [B, x_dim]: [B, x_dim]
    passes, and so does any [B, ...] whose trailing extents multiply to x_dim; `rows`: the B it must have.  ValueError
    (`_lib.expect_shape`) otherwise, on the host, before the value is copied, a draw is taken or a plan is built."""
    _lib.expect_shape(x, (rows, x_dim), name, who, fold=True)
    x = _lib.as_dev(x, device)
    return x if x.ndim == 2 else x.reshape(x.shape[0], -1)


def per_chain(value, B, device, *, who, name, scalar=None, sign=None, hint=""):
    """One value per chain (`step`'s and `swap_replicas`' beta or temperature) -> (float32 device tensor, chain_stride):
    [B] or [1, B] -> ([B], 1); one value -> ([1], 0) where `scalar` (the word the message has for it) is given.  A
    float32 tensor [B] or [1, B] on `device` (not the CPU) stays there, unchecked.  ValueError for another shape, and
    with `sign` ("not negative" or "> 0") for an entry that, in float32, is not finite or not that."""
    if (isinstance(value, torch.Tensor) and value.device == device and device.type != "cpu"
            and value.dtype == torch.float32 and tuple(value.shape) in ((B,), (1, B))):
        return value.reshape(-1), 1                        # (a ladder that is on the device already stays there)
    v, v32 = _float32(value)
    if v.shape not in ((B,), (1, B)) and (scalar is None or v.ndim):
        raise ValueError(f"{who}: {name} of shape {v.shape}: expected {scalar + ', ' if scalar else ''}[{B}] or "
                         f"[1, {B}]{hint}")
    if sign is not None and not (np.isfinite(v32) & ((v32 > 0) if sign == "> 0" else (v32 >= 0))).all():
        raise ValueError(f"{who}: every {name} must be finite and {sign} (in float32)")
    return _lib.as_dev(np.ascontiguousarray(v32).reshape(-1), device), int(v.ndim > 0)


def step_sizes(eps, B, who="run_hmc"):
    """`run_hmc`'s `eps` as a float32 array [] or [B]; ValueError for another shape or an entry not > 0 in float32."""
    _, e = _float32(eps)
    if e.shape not in ((), (B,)):
        raise ValueError(f"{who}: eps of shape {e.shape}: expected a scalar or [{B}] (one per chain)")
    if not (np.isfinite(e) & (e > 0)).all():
        raise ValueError(f"{who}: every eps must be finite and > 0 (in float32)")
    return e


def plan_with_step_sizes(dyn, step, device):
    """(a fresh plan struct of `dyn`, eps_chain) for `step` = None or what `step_sizes` returned: a scalar goes into
    `plan.eps` of this struct alone (the dynamics' own plan and eps stay), a [B] array goes to the device."""
    plan, eps_chain = dyn._plan(), None
    if step is not None and step.ndim == 0:
        plan.eps = float(step)
    elif step is not None:
        eps_chain = _lib.as_dev(step, device)
    return plan, eps_chain


def check_replicas(replicas, B, swap_every=1, first_parity=0, parity=0, who="run_hmc_exchange", most=None):
    """The replica-exchange arguments of both samplers -> (G, swap_every, first_parity, parity) as ints; ValueError
    otherwise.  `most`: the largest group the entry behind `who` takes (the toy targets keep a group in one wave)."""
    try:
        G, k, fp, par = int(replicas), int(swap_every), int(first_parity), int(parity)
        whole = G == replicas and k == swap_every and fp == first_parity and par == parity
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError(f"{who}: replicas, swap_every and the parity must be whole numbers")
    if G < 2:
        raise ValueError(f"{who}: replicas={G}: a replica group has 2 rungs or more")
    if most is not None and G > most:
        raise ValueError(f"{who}: replicas={G}: a replica group has {most} rungs at the most (it sits in one wave)")
    if B % G != 0:
        raise ValueError(f"{who}: the {B} chains (of this rank) are no whole number of groups of replicas={G}")
    if k < 1:
        raise ValueError(f"{who}: swap_every={k} must be 1 or more")
    if fp not in (0, 1) or par not in (0, 1):
        raise ValueError(f"{who}: the parity of a round is 0 or 1")
    return G, k, fp, par


def replica_labels(replica0, B, who="run_hmc_exchange"):
    """The labels an exchange run starts with, int32 [B] on the host: arange(B), or `replica0` (ValueError unless it
    is int32 [B])."""
    if replica0 is None:
        return np.arange(B, dtype=np.int32)
    labels = replica0.detach().cpu().numpy() if isinstance(replica0, torch.Tensor) else np.asarray(replica0)
    if labels.dtype != np.int32 or labels.shape != (B,):
        raise ValueError(f"{who}: replica0 of dtype {labels.dtype} and shape {labels.shape}: expected int32 [{B}]")
    return labels


def exchange_histories(out, rounds, B, G):
    """Adds what an exchange run returns on top of its run's dictionary `out`: swap_p [n_r, B] float32, swapped bool,
    replica int32 -- from `rounds`, per name a list of [B] device tensors or one [n_r, B] device tensor -- and
    swap_rate [G - 1], the mean of `swapped` over rounds and groups for each neighbouring pair of rungs."""
    counts = None
    for name, dtype in (("swap_p", np.float32), ("swapped", np.bool_), ("replica", np.int32)):
        r = rounds[name]
        if isinstance(r, list):
            r = torch.stack(r) if r else None
        if r is not None and name == "swapped":
            # (uint8 from the run kernel: the same bytes.)  The exchanges are counted where the history lives: a run
            # with a round after every step has as many rows as steps, and the host would walk them all for G - 1 numbers
            r = r.view(torch.bool) if r.dtype == torch.uint8 else r
            counts = r.reshape(-1, B // G, G)[:, :, :G - 1].sum(dim=(0, 1), dtype=torch.int64).cpu().numpy()
        out[name] = np.empty((0, B), dtype=dtype) if r is None else r.cpu().numpy().astype(dtype, copy=False)
    n_r = out["swapped"].shape[0]
    # the mean of `swapped` over rounds and groups, as NumPy forms it: the exact count over the number of entries
    out["swap_rate"] = counts / np.float64(n_r * (B // G)) if n_r else np.full(G - 1, np.nan)
    return out


class Exchange:
    """The replica-exchange schedule of ONE run, for both samplers: groups of `G` columns, a round after every step s
    (from 1) with s % k == 0, of parity (parity0 + s // k - 1) % 2, on the values step s ran with; the labels start as
    `labels` (int32 [B] on the host).  The only place that knows which steps a round follows, how the rounds' results
    are collected and how they complete the run's dictionary.  A sampler hands it what differs: its `_swap_round` for
    rounds between the launches, its entry's arguments (`chunk`) for rounds inside them."""
    NAMES = ("swap_p", "swapped", "replica")

    def __init__(self, G, k, parity0, labels, B):
        self.G, self.k, self.parity0, self.labels, self.B = G, k, parity0, labels, B
        self.rounds = {name: [] for name in self.NAMES}    # per round a [B] device tensor; `in_launch`: [n_r, B] each
        self.replica = None

    def start(self, device):
        """A run of 1 step or more starts: the labels on the device, which the sampler keeps as its `replica`."""
        self.replica = _lib.as_dev(self.labels, device, torch.int32)
        return self.replica

    def parity_after(self, s):
        """The parity of the round that follows step s (from 1), or None where none does."""
        return (self.parity0 + s // self.k - 1) % 2 if s % self.k == 0 else None

    def between(self, swap_round, rows, clone=False):
        """Rounds as launches of their own: the `after(s, x)` of `run_chunks` (with `cut_every` = k) or of a loop over
        steps; it returns the state the next step starts from.  `swap_round(x, values, chain_stride, G, parity)` is the
        sampler's round, in place, taking one stream of its counter; `rows`: `rows_from`.  `clone`: the round gets a
        copy of x, where x itself is kept as the step's sample."""
        def after(s, x_now):
            parity = self.parity_after(s)
            if parity is not None:
                x_now = x_now.clone() if clone else x_now
                values, _, chain_stride = rows(s - 1)
                p, swapped, _ = swap_round(x_now, values, chain_stride, self.G, parity)
                for name, r in zip(self.NAMES, (p, swapped, self.replica.clone())):
                    self.rounds[name].append(r)
            return x_now
        return after

    def in_launch(self, run_steps, device):
        """Rounds inside the launches of a run of `run_steps` steps: the three device histories, allocated once."""
        self.rounds = {name: torch.empty(run_steps // self.k, self.B, dtype=dtype, device=device)
                       for name, dtype in zip(self.NAMES, (torch.float32, torch.uint8, torch.int32))}

    def place(self, s0, n):
        """Steps [s0, s0 + n) in the schedule -> (steps into the period at s0, parity of the chunk's first round, its
        row in the histories, rounds in the chunk)."""
        phase, row = s0 % self.k, s0 // self.k
        return phase, (self.parity0 + row) % 2, row, _lib.exchange_rounds(n, self.k, phase)

    def chunk(self, s0, n):
        """What an exchange entry takes for steps [s0, s0 + n) -> ((group, swap_every, swap_phase, first_parity), the
        chunk's slices of the three histories -- NULL for a chunk without a round --, rounds in the chunk)."""
        phase, parity, row, n_rounds = self.place(s0, n)
        hist = tuple(self.rounds[name][row:] if n_rounds else None for name in self.NAMES)
        return (self.G, self.k, phase, parity), hist, n_rounds

    def finish(self, out):
        """The run's dictionary `out` with the rounds' histories and swap_rate added (`exchange_histories`)."""
        return exchange_histories(out, self.rounds, self.B, self.G)


def empty_run(names, x, keep_samples):
    """The dictionary of a run of 0 steps from `x` [B, D]: empty histories, a copy of the start as the final state."""
    out = {k: np.empty((0, x.shape[0]), dtype=np.float32) for k in names}
    out["samples_out"] = x.clone()
    if keep_samples:
        out["samples"] = np.empty((0, *x.shape), dtype=np.float32)
    return out


def chunk_length(run_steps, steps_per_launch):
    """The most steps one launch of a run takes: what a caller sizes its workspace by."""
    return min(int(steps_per_launch), run_steps)


def run_chunks(run_steps, x, steps_per_launch, keep_samples, launch, cut_every=None, after=None):
    """`run_steps` > 0 steps from `x` [B, D] in chunks of at most `steps_per_launch`.  `launch(s0, n, x_in, x_next,
    samples_dev)` runs steps [s0, s0 + n) through the caller's entry: state from `x_in` to `x_next`, the n samples (if
    kept) to the head of `samples_dev`.  With `cut_every` = k no chunk spans a multiple of k steps.  `after(s, x_next)`
    is called after every chunk with the steps completed so far and the state they left, which it may change in place.
    Returns {"samples_out": the final state, "samples": host array [run_steps, B, D] (if kept)}; histories are the
    caller's.  Allocated once per run: `x_next`, and with `keep_samples` a device buffer ONE chunk long and the host
    array.  Per chunk: the launch and, with `keep_samples`, the one device-to-host copy -- nothing else allocates or
    synchronises.  A chunk's draw index is the caller's, read in `launch`: `after` may take streams in between."""
    B, D = x.shape
    chunk = chunk_length(run_steps, steps_per_launch)
    samples_dev = torch.empty(chunk, B, D, dtype=torch.float32, device=x.device) if keep_samples else None
    x_next = torch.empty_like(x)                           # the first chunk leaves the caller's x alone
    out = {"samples_out": x_next}
    if keep_samples:
        out["samples"] = np.empty((run_steps, B, D), dtype=np.float32)
    x_in = x
    s0 = 0
    while s0 < run_steps:
        n = min(chunk, run_steps - s0)
        if cut_every is not None:
            n = min(n, cut_every - s0 % cut_every)
        launch(s0, n, x_in, x_next, samples_dev)           # raises if the entry fails: nothing below has happened
        x_in = x_next                                      # later chunks advance the state in place
        if keep_samples:
            out["samples"][s0:s0 + n] = samples_dev[:n].cpu().numpy()
        s0 += n
        if after is not None:
            after(s0, x_next)
    return out
