"""The samplers' shared run driver (l2hmc_amd/_runs.py) alone: how `run_chunks` cuts a run into launches and hands the
state and the samples on, and how `chain_axis` maps a value's shape to its element strides.  No GPU and no library: CPU
tensors and a fake `launch` that records its arguments and writes x_in + n into x_next."""
import numpy as np
import pytest
import torch

from l2hmc_amd import _runs

B, D = 3, 2


class FakeLaunch:
    """Steps [s0, s0 + n): the state goes up by 1 per step, and sample i of the chunk is the state after step s0 + i."""

    def __init__(self):
        self.calls = []

    def __call__(self, s0, n, x_in, x_next, samples_dev):
        self.calls.append((s0, n, x_in, x_next, samples_dev))
        start = x_in.clone()                              # (x_in is x_next from the second chunk on)
        if samples_dev is not None:
            for i in range(n):
                samples_dev[i] = start + (i + 1)
        x_next.copy_(start + n)


def _drive(run_steps, spl, keep_samples=True, **kw):
    x = torch.arange(B * D, dtype=torch.float32).reshape(B, D)
    keep = x.clone()
    launch = FakeLaunch()
    out = _runs.run_chunks(run_steps, x, spl, keep_samples, launch, **kw)
    assert torch.equal(x, keep)                           # the caller's tensor is unchanged at the end
    assert set(out) == ({"samples_out", "samples"} if keep_samples else {"samples_out"})
    return x, launch.calls, out["samples_out"], out.get("samples")


@pytest.mark.parametrize("spl,cut,chunks,afters", [
    (3, None, [(0, 3), (3, 3), (6, 1)], [3, 6, 7]),
    (3, 2, [(0, 2), (2, 2), (4, 2), (6, 1)], [2, 4, 6, 7]),
    (3, 5, [(0, 3), (3, 2), (5, 2)], [3, 5, 7]),
    (256, None, [(0, 7)], [7]),
    (7, None, [(0, 7)], [7]),
    (256, 4, [(0, 4), (4, 3)], [4, 7]),
    (1, 3, [(s, 1) for s in range(7)], list(range(1, 8)))])
def test_run_chunks_cuts_the_run_and_calls_after_every_chunk(spl, cut, chunks, afters):
    seen = []
    x, calls, x_out, samples = _drive(7, spl, cut_every=cut, after=lambda s, x_now: seen.append((s, x_now)))
    assert [c[:2] for c in calls] == chunks
    assert [s for s, _ in seen] == afters and all(x_now is x_out for _, x_now in seen)
    # without `after` the chunks are the same
    assert [c[:2] for c in _drive(7, spl, cut_every=cut)[1]] == chunks


def test_run_chunks_hands_the_state_on_and_leaves_the_callers_tensor():
    x, calls, x_out, _ = _drive(7, 3)
    assert calls[0][2] is x and x_out is not x and x_out.shape == x.shape and x_out.dtype == x.dtype
    assert all(c[3] is x_out for c in calls) and all(c[2] is x_out for c in calls[1:])
    assert torch.equal(x_out, x + 7)


@pytest.mark.parametrize("spl,cut,length", [(3, None, 3), (3, 2, 3), (256, None, 7), (256, 2, 7)])
def test_run_chunks_keeps_one_sample_buffer_one_chunk_long_and_assembles_in_step_order(spl, cut, length):
    x, calls, _, samples = _drive(7, spl, cut_every=cut)
    assert all(c[4] is calls[0][4] for c in calls)
    assert calls[0][4].shape == (length, B, D) and calls[0][4].dtype == torch.float32
    assert samples.shape == (7, B, D) and samples.dtype == np.float32
    assert np.array_equal(samples, np.stack([x.numpy() + s + 1 for s in range(7)]))
    # not kept: no buffer, no host array
    _, calls, x_out, samples = _drive(7, spl, keep_samples=False, cut_every=cut)
    assert samples is None and all(c[4] is None for c in calls) and torch.equal(x_out, x + 7)


def test_after_may_change_the_state_in_place():
    def after(s, x_now):
        x_now.mul_(2.0)
    x, _, x_out, samples = _drive(4, 3, after=after)
    assert torch.equal(x_out, ((x + 3) * 2 + 1) * 2)
    assert np.array_equal(samples[3], ((x + 3) * 2 + 1).numpy())      # what step 4 wrote, before `after`


def test_a_failed_launch_ends_the_run_there():
    calls = []

    def launch(s0, n, *rest):
        calls.append(s0)
        if s0 == 3:
            raise RuntimeError("entry failed")
    seen = []
    with pytest.raises(RuntimeError, match="entry failed"):
        _runs.run_chunks(7, torch.zeros(B, D), 3, True, launch, after=lambda s, x: seen.append(s))
    assert calls == [0, 3] and seen == [3]


def test_empty_run():
    x = torch.ones(B, D)
    out = _runs.empty_run(("px", "actions"), x, True)
    assert set(out) == {"px", "actions", "samples_out", "samples"}
    assert out["px"].shape == out["actions"].shape == (0, B) and out["px"].dtype == np.float32
    assert out["samples"].shape == (0, B, D) and out["samples"].dtype == np.float32
    assert torch.equal(out["samples_out"], x) and out["samples_out"] is not x
    assert "samples" not in _runs.empty_run(("px",), x, False)


# ------------------------------------------------------------------------------------------------ chain_axis
def _axis(value, n=5, b=3, positive=False):
    return _runs.chain_axis(value, n, b, who="f", name="beta", positive=positive)


def test_the_four_shapes_map_to_their_stride_pairs():
    n, b = 5, 3
    v, flat, strides = _axis(2.5)
    assert strides == (0, 0) and flat.dtype == np.float32 and flat.tolist() == [2.5] and v.shape == ()
    sched = np.arange(1, n + 1, dtype=np.float64)
    v, flat, strides = _axis(sched)
    assert strides == (1, 0) and flat.tolist() == sched.tolist()
    lad = np.array([[1.0, 2.5, 4.0]])
    v, flat, strides = _axis(lad)
    assert strides == (0, 1) and flat.tolist() == [1.0, 2.5, 4.0]
    grid = sched[:, None] + 10 * np.arange(b)[None, :]
    v, flat, (ss, cs) = _axis(grid)
    assert (ss, cs) == (b, 1) and flat.shape == (n * b,) and flat.flags["C_CONTIGUOUS"]
    assert all(flat[s * ss + c * cs] == grid[s, c] for s in range(n) for c in range(b))
    assert v.dtype == np.float64 and np.array_equal(v, grid)
    # a Fortran-ordered view is laid out anew
    v, flat, (ss, cs) = _axis(np.asfortranarray(grid))
    assert flat.flags["C_CONTIGUOUS"] and all(flat[s * ss + c * cs] == grid[s, c] for s in range(n) for c in range(b))
    # [1, B] of a one-step run is [n, B] with n = 1 as well: either reading reads the same elements
    v, flat, (ss, cs) = _axis(lad, n=1)
    assert (ss, cs) in ((0, 1), (b, 1)) and [flat[0 * ss + c * cs] for c in range(b)] == [1.0, 2.5, 4.0]
    # float32 rounding is the device's
    assert _axis(0.1)[1][0] == np.float32(0.1) and _axis(0.1)[0] == 0.1


@pytest.mark.parametrize("shape", [(3,), (4,), (1,), (0,), (5, 1), (3, 5), (5, 2), (2, 3), (1, 4), (1, 1), (5, 3, 1),
                                   (1, 1, 3)])
def test_other_shapes_are_refused_with_the_accepted_ones_named(shape):
    with pytest.raises(ValueError) as e:
        _axis(np.ones(shape))
    assert str(e.value) == (f"f: beta of shape {shape}: expected a scalar, [5] (one per step), [1, 3] (one per chain) "
                            f"or [5, 3]")


def test_zero_is_accepted_unless_positive():
    assert _axis(0.0)[1].tolist() == [0.0]
    assert _axis([[1.0, 0.0, 2.0]])[1].tolist() == [1.0, 0.0, 2.0]
    for v in (0.0, [[1.0, 0.0, 2.0]], 1e-50):             # the last: 0 in float32
        with pytest.raises(ValueError, match=r"^f: every beta must be finite and > 0 \(in float32\)$"):
            _axis(v, positive=True)
    assert _axis(1e-50)[1].tolist() == [0.0]


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf"), 1e60, -0.5, -1e-3])
def test_entries_that_are_not_finite_or_negative_are_refused(bad, positive):
    word = "> 0" if positive else "not negative"
    for v in (bad, [1.0, 1.0, bad, 1.0, 1.0], [[1.0, bad, 1.0]], np.where(np.eye(5, 3) > 0, bad, 1.0)):
        with pytest.raises(ValueError) as e:
            _axis(v, positive=positive)
        assert str(e.value) == f"f: every beta must be finite and {word} (in float32)"


def test_a_tensor_a_list_and_an_array_give_the_same_result():
    rows = [[1.0, 2.5, 0.1], [4.0, 0.3, 7.0]]
    want = _runs.chain_axis(np.array(rows), 2, 3, who="f", name="t", positive=True)
    for value in (rows, torch.tensor(rows, dtype=torch.float64), torch.tensor(rows, dtype=torch.float64).t().t()):
        v, flat, strides = _runs.chain_axis(value, 2, 3, who="f", name="t", positive=True)
        assert v.dtype == np.float64 and np.array_equal(v, want[0])
        assert flat.dtype == np.float32 and np.array_equal(flat, want[1]) and strides == want[2] == (3, 1)
    # a float32 tensor is taken as given: its values are float32 already
    v, flat, _ = _runs.chain_axis(torch.tensor(rows), 2, 3, who="f", name="t", positive=True)
    assert np.array_equal(flat, want[1]) and v.dtype == np.float64


def test_step_sizes():
    assert _runs.step_sizes(0.25, 4).shape == () and _runs.step_sizes(0.25, 4).dtype == np.float32
    assert _runs.step_sizes([0.1, 0.2, 0.3, 0.4], 4).tolist() == np.float32([0.1, 0.2, 0.3, 0.4]).tolist()
    with pytest.raises(ValueError, match="^who: eps of shape"):
        _runs.step_sizes([0.1, 0.2], 4, who="who")
    for bad in (0.0, -0.1, float("nan"), 1e60, 1e-60):
        with pytest.raises(ValueError, match="^run_hmc: every eps must be finite and > 0"):
            _runs.step_sizes(bad, 4)
