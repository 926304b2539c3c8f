"""The replica-exchange layer both samplers' ladder runs share (l2hmc_amd/_runs.py: `Exchange`, `rows_from`, `per_chain`)
alone, against the plain loop it stands for: for s in 1..n a step, and behind every step with s % k == 0 a round of
parity (parity0 + s // k - 1) % 2 on the values step s ran with.  No GPU and no library: CPU tensors, a fake launch that
adds 1 to the state per step and a fake round that adds 100 in place and moves the labels on."""
import itertools

import numpy as np
import pytest
import torch

from l2hmc_amd import _lib, _runs

B, D, G = 4, 2, 2
GRID = list(itertools.product(range(8), range(1, 5), (0, 1)))                # n, k, parity0
LAUNCHES = (1, 2, 3, 256)                                                     # steps_per_launch
LABELS = np.array([3, 2, 1, 0], dtype=np.int32)


def _loop(n, k, parity0):
    """The plain loop -> [(the step s, from 1, a round follows; the round's parity)]."""
    rounds = []
    for s in range(1, n + 1):
        if s % k == 0:
            rounds.append((s, (parity0 + s // k - 1) % 2))
    return rounds


def _values(shape_kind, n):
    """A `chain_axis` value of each of its four shapes whose entry for step s (from 0), chain c is told apart."""
    grid = 10.0 * (np.arange(n)[:, None] + 1) + np.arange(B)[None, :]
    return {"scalar": 2.5, "schedule": grid[:, 0], "ladder": 1.0 + np.arange(B)[None, :], "both": grid}[shape_kind]


def _rows(value, n):
    """(s -> the B values step s, from 1, runs with, read off the value as given; `rows_from` of its flat form)."""
    v, flat, strides = _runs.chain_axis(value, n, B, who="f", name="beta", positive=False)

    def ran_with(s):
        if v.ndim == 2:
            return v[min(s, v.shape[0]) - 1].tolist()      # [1, B]: the one row
        return [float(v if v.ndim == 0 else v[s - 1])] * B
    return ran_with, _runs.rows_from(torch.from_numpy(flat), strides)


class FakeRound:
    """The sampler's `_swap_round`: records what it is given, adds 100 to x in place, moves every label on by 1."""

    def __init__(self, exchange):
        self.exchange, self.calls = exchange, []

    def __call__(self, x, values, chain_stride, group, parity):
        self.calls.append((x.clone(), [float(values[c * chain_stride]) for c in range(B)], group, parity))
        x.add_(100.0)
        self.exchange.replica.add_(1)
        j = len(self.calls)
        return torch.full((B,), float(j)), torch.tensor([j % 2 == 1, False] * (B // 2)), None


def _launch(calls):
    def launch(s0, n, x_in, x_next, samples_dev):
        calls.append((s0, n))
        start = x_in.clone()
        if samples_dev is not None:
            for i in range(n):
                samples_dev[i] = start + (i + 1)
        x_next.copy_(start + n)
    return launch


def _exchange(k, parity0):
    ex = _runs.Exchange(G, k, parity0, LABELS.copy(), B)   # (on the CPU the "upload" shares the array's memory)
    replica = ex.start(torch.device("cpu"))
    assert replica is ex.replica and replica.dtype == torch.int32 and replica.tolist() == LABELS.tolist()
    return ex


# ------------------------------------------------------------------------------------------ rounds between launches
@pytest.mark.parametrize("kind", ["scalar", "schedule", "ladder", "both"])
@pytest.mark.parametrize("n,k,parity0", GRID)
def test_rounds_between_the_steps_are_the_loops(n, k, parity0, kind):
    """`between` as the `after` of a loop over single steps (GaugeSampler.run_exchange)."""
    want = _loop(n, k, parity0)
    table, rows = _rows(_values(kind, n), n)
    ex = _exchange(k, parity0)
    fake = FakeRound(ex)
    after = ex.between(fake, rows)
    x = torch.zeros(B, D)
    for s in range(1, n + 1):
        x = x + 1                                          # the step
        assert after(s, x) is x                            # in place: the state goes on as it is
        assert ex.parity_after(s) == dict(want).get(s)
    assert [(int(c[0][0, 0]), c[3]) for c in fake.calls] == [(s + 100 * j, p) for j, (s, p) in enumerate(want)]
    assert [c[1] for c in fake.calls] == [table(s) for s, _ in want]      # the row step s ran with
    assert all(c[2] == G for c in fake.calls)
    # one snapshot of the labels per round, none of them the live tensor
    snaps = ex.rounds["replica"]
    assert [t.tolist() for t in snaps] == [(LABELS + j + 1).tolist() for j in range(len(want))]
    assert all(t is not ex.replica for t in snaps) and len({t.data_ptr() for t in snaps}) == len(snaps)
    out = ex.finish({})
    assert out["swap_p"].shape == out["swapped"].shape == out["replica"].shape == (n // k, B)
    assert out["swap_p"].tolist() == [[float(j + 1)] * B for j in range(n // k)]
    assert out["replica"].dtype == np.int32 and out["swapped"].dtype == np.bool_ and out["swap_p"].dtype == np.float32


@pytest.mark.parametrize("spl", LAUNCHES)
@pytest.mark.parametrize("n,k,parity0", [g for g in GRID if g[0] > 0])
def test_through_run_chunks_no_chunk_spans_a_round(n, k, parity0, spl):
    """`between` as the `after` of `run_chunks` with `cut_every` = k (run_hmc_exchange, DynamicsSampler.run_exchange)."""
    want = _loop(n, k, parity0)
    table, rows = _rows(_values("both", n), n)
    ex = _exchange(k, parity0)
    fake, chunks = FakeRound(ex), []
    out = _runs.run_chunks(n, torch.zeros(B, D), spl, True, _launch(chunks), cut_every=k, after=ex.between(fake, rows))
    assert sum(m for _, m in chunks) == n and all(m <= spl and s0 % k + m <= k for s0, m in chunks)
    assert [(int(c[0][0, 0]), c[3]) for c in fake.calls] == [(s + 100 * j, p) for j, (s, p) in enumerate(want)]
    assert [c[1] for c in fake.calls] == [table(s) for s, _ in want]
    assert len(ex.rounds["replica"]) == len(want)
    # samples[s - 1] is what step s wrote, before its round; samples_out the state after the last round
    assert out["samples"][:, 0, 0].tolist() == [s + 100.0 * ((s - 1) // k) for s in range(1, n + 1)]
    assert float(out["samples_out"][0, 0]) == n + 100.0 * (n // k)


def test_a_round_on_a_copy_leaves_the_steps_output():
    ex = _exchange(1, 0)
    after = ex.between(FakeRound(ex), _rows(2.5, 3)[1], clone=True)
    x = torch.ones(B, D)
    x_next = after(1, x)
    assert x_next is not x and torch.equal(x, torch.ones(B, D)) and torch.equal(x_next, x + 100)
    ex = _exchange(2, 0)
    assert ex.between(FakeRound(ex), _rows(2.5, 3)[1], clone=True)(1, x) is x          # no round: no copy


# ------------------------------------------------------------------------------------------ rounds inside the launches
@pytest.mark.parametrize("spl", LAUNCHES)
@pytest.mark.parametrize("n,k,parity0", GRID)
def test_chunks_of_an_in_launch_run_reproduce_the_loops_schedule(n, k, parity0, spl):
    want = _loop(n, k, parity0)
    ex = _exchange(k, parity0)
    ex.in_launch(n, torch.device("cpu"))
    assert [(tuple(ex.rounds[name].shape), ex.rounds[name].dtype) for name in ex.NAMES] == [
        ((n // k, B), torch.float32), ((n // k, B), torch.uint8), ((n // k, B), torch.int32)]
    for j in range(n // k):
        ex.rounds["replica"][j] = j                        # a row says which it is
    chunks = []
    if n:
        _runs.run_chunks(n, torch.zeros(B, D), spl, False, _launch(chunks))
    got, total, draws, ref = [], 0, 5, 5
    for s0, m in chunks:
        phase, parity, row, n_rounds = ex.place(s0, m)
        place, hist, n_rounds_again = ex.chunk(s0, m)
        assert place == (G, k, phase, parity) and n_rounds_again == n_rounds and 0 <= phase < k
        if n_rounds:
            assert all(h.data_ptr() == ex.rounds[name][row].data_ptr() for h, name in zip(hist, ex.NAMES))
            assert int(hist[2][0, 0]) == row and hist[2].shape[0] >= n_rounds
        else:
            assert hist == (None, None, None)              # NULL: the entries take it for a chunk without a round
        # the entry's rule: a round follows step i (from 0) of the chunk iff (swap_phase + i + 1) % swap_every == 0
        in_chunk = [s0 + i + 1 for i in range(m) if (phase + i + 1) % k == 0]
        assert len(in_chunk) == n_rounds
        got += [(s, (parity + j) % 2, row + j) for j, s in enumerate(in_chunk)]
        total += n_rounds
        # the draws: `step_draw_index` per step and + 1 per round, walked along the loop
        d0, rounds_drawn, draws = _lib.exchange_run_draw_index(draws, m, k, phase)
        for s in range(s0 + 1, s0 + m + 1):
            d, ref = _lib.step_draw_index(ref)
            assert s != s0 + 1 or d == d0
            ref += s % k == 0
        assert (rounds_drawn, draws) == (n_rounds, ref)
    assert got == [(s, p, j) for j, (s, p) in enumerate(want)] and total == n // k
    assert _lib.exchange_rounds(n, k, 0) == n // k


def test_in_launch_histories_complete_the_dictionary():
    ex = _exchange(2, 1)
    ex.in_launch(5, torch.device("cpu"))
    ex.rounds["swap_p"].copy_(torch.tensor([[0.5, float("nan")] * 2, [1.0, float("nan")] * 2]))
    ex.rounds["swapped"].copy_(torch.tensor([[1, 0, 0, 0], [1, 0, 1, 0]], dtype=torch.uint8))
    ex.rounds["replica"].copy_(torch.tensor([[1, 0, 2, 3], [0, 1, 3, 2]], dtype=torch.int32))
    out = ex.finish({"px": 1})
    assert out["px"] == 1 and out["swapped"].dtype == np.bool_ and out["swapped"].tolist() == [[True, False, False, False],
                                                                                              [True, False, True, False]]
    assert out["replica"].tolist() == [[1, 0, 2, 3], [0, 1, 3, 2]] and out["swap_rate"].tolist() == [0.75]
    assert np.array_equal(out["swap_p"], ex.rounds["swap_p"].numpy(), equal_nan=True)


# ------------------------------------------------------------------------------------------------ the empty run
@pytest.mark.parametrize("groups", [2, 4])
def test_an_empty_run_has_empty_histories_and_no_rate(groups):
    ex = _runs.Exchange(groups, 3, 1, LABELS, B)
    x = torch.ones(B, D)
    out = ex.finish(_runs.empty_run(("px",), x, True))
    assert out["px"].shape == (0, B) and out["samples"].shape == (0, B, D) and torch.equal(out["samples_out"], x)
    for name, dtype in (("swap_p", np.float32), ("swapped", np.bool_), ("replica", np.int32)):
        assert out[name].shape == (0, B) and out[name].dtype == dtype
    assert out["swap_rate"].shape == (groups - 1,) and np.isnan(out["swap_rate"]).all()
    assert ex.replica is None                              # nothing went to the device


# ------------------------------------------------------------------------------------------------ one value per chain
CPU = torch.device("cpu")
STEP = dict(who="step", name="beta", scalar="a float", sign="not negative", hint=" (one per chain)")      # GaugeSampler
SWAP = dict(who="swap_replicas", name="beta")                                                            # GaugeSampler
TOY_SWAP = dict(who="swap_replicas", name="temperature", scalar="a scalar", sign="> 0")                  # DynamicsSampler
EXPECTED = {"step": f"a float, [{B}] or [1, {B}] (one per chain)", "beta": f"[{B}] or [1, {B}]",
            "temperature": f"a scalar, [{B}] or [1, {B}]"}


def _expected(rule):
    return EXPECTED["step" if rule is STEP else rule["name"]]


@pytest.mark.parametrize("rule", [STEP, SWAP, TOY_SWAP], ids=["step", "swap", "toy_swap"])
def test_per_chain_takes_the_two_shapes_in_every_form(rule):
    ladder = [0.1, 1.0, 2.5, 4.0]
    want = np.float32(ladder).tolist()                     # float32 rounding is the device's: 0.1 arrives as float32(0.1)
    forms = [ladder, [ladder], np.array(ladder), np.array([ladder]), torch.tensor(ladder, dtype=torch.float64),
             torch.tensor([ladder]), np.float32(ladder),
             np.repeat(np.array(ladder), 2)[::2],                                      # strided: laid out anew
             torch.tensor(ladder, dtype=torch.float64).repeat_interleave(2)[::2][None]]  # [1, B], element stride 2
    assert not forms[-2].flags["C_CONTIGUOUS"] and not forms[-1].is_contiguous()
    for value in forms:
        dev, stride = _runs.per_chain(value, B, CPU, **rule)
        assert stride == 1 and dev.dtype == torch.float32 and dev.shape == (B,) and dev.is_contiguous()
        assert dev.tolist() == want and dev.tolist()[0] == float(np.float32(0.1)) != 0.1


@pytest.mark.parametrize("shape", [(B + 1,), (B - 1,), (2, B), (B, 1), (1, 1, B), (1, B + 1), (0,)])
@pytest.mark.parametrize("rule", [STEP, SWAP, TOY_SWAP], ids=["step", "swap", "toy_swap"])
def test_per_chain_refuses_other_shapes_with_the_accepted_ones_named(rule, shape):
    for value in (np.ones(shape), torch.ones(shape)):
        with pytest.raises(ValueError) as e:
            _runs.per_chain(value, B, CPU, **rule)
        assert str(e.value) == f"{rule['who']}: {rule['name']} of shape {shape}: expected {_expected(rule)}"


def test_one_value_is_refused_or_goes_over_with_stride_0():
    with pytest.raises(ValueError) as e:
        _runs.per_chain(2.0, B, CPU, **SWAP)
    assert str(e.value) == f"swap_replicas: beta of shape (): expected [{B}] or [1, {B}]"
    for value in (0.1, np.float64(0.1), torch.tensor(0.1, dtype=torch.float64)):
        dev, stride = _runs.per_chain(value, B, CPU, **TOY_SWAP)
        assert stride == 0 and dev.shape == (1,) and dev.dtype == torch.float32 and dev.tolist() == [float(np.float32(0.1))]


BAD = [float("nan"), float("inf"), -float("inf"), 1e60, -0.5, -1e-3]


def test_the_sign_rule_is_each_callers():
    def with_entry(v):
        return [1.0, v, 2.0, 3.0]
    # step: finite and not negative in float32; 0 passes, and so does what rounds to 0
    for ok in (0.0, 1e-50):
        assert _runs.per_chain(with_entry(ok), B, CPU, **STEP)[0].tolist() == [1.0, 0.0, 2.0, 3.0]
    for bad in BAD:
        with pytest.raises(ValueError, match=r"^step: every beta must be finite and not negative \(in float32\)$"):
            _runs.per_chain(with_entry(bad), B, CPU, **STEP)
    # the lattice round checks no sign: whatever float32 holds goes over
    for v in (-0.5, 0.0, float("inf")):
        assert _runs.per_chain(with_entry(v), B, CPU, **SWAP)[0].tolist() == [1.0, v, 2.0, 3.0]
    assert np.isnan(_runs.per_chain(with_entry(float("nan")), B, CPU, **SWAP)[0].tolist()[1])
    # the toy round: finite and > 0 in float32, a scalar included
    for bad in BAD + [0.0, 1e-50]:
        for value in (with_entry(bad), [with_entry(bad)], bad):
            with pytest.raises(ValueError,
                               match=r"^swap_replicas: every temperature must be finite and > 0 \(in float32\)$"):
                _runs.per_chain(value, B, CPU, **TOY_SWAP)
    # the shape is looked at first
    with pytest.raises(ValueError, match="of shape"):
        _runs.per_chain([-1.0] * (B + 1), B, CPU, **TOY_SWAP)


def test_a_float32_tensor_on_the_cpu_is_no_device_ladder():
    """The stay-where-it-is path is for the device of the state: a CPU tensor is checked and copied like an array."""
    t = torch.tensor([1.0, -2.0, 3.0, 4.0])
    with pytest.raises(ValueError, match="every beta"):
        _runs.per_chain(t, B, CPU, **STEP)
    dev, _ = _runs.per_chain(t.abs(), B, CPU, **STEP)
    assert dev.tolist() == [1.0, 2.0, 3.0, 4.0]
