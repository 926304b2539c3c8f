"""No result depends on what a workspace holds on entry, and no state is carried from one call or one graph replay
to the next (the table of tests/workspace_cases.py on the device).

Every comparison is bitwise, through `.view(torch.int32)` so that NaNs compare; there is no tolerance.

1. Content independence: every output of every operation is the same under the three byte patterns, and when the shared
   buffer was last used by another operation with a larger batch.  Control: two runs under 0x00 first.
2. Repetition: three eager calls with the buffer and step_sums untouched in between give the same bits, and every
   documented ticket word of step_sums is 0 after each.
3. Graph replay: every whole-step form (the cut batch and a ladder included), captured in place at a fixed draw and
   replayed three times from x0, equals three chained eager steps after each replay -- with the workspace left alone,
   and with it refilled with 0xFF between the replays.  Three replays, once.
4. Graph shape: a one-launch step form is captured as kernel nodes only, and the cut batch as a chain of at least three
   kernel nodes: no memset node stands between a step's kernels."""
import pytest
import torch

from tests import helpers as H
from tests import workspace_cases as W

pytestmark = pytest.mark.gpu

_BUILT = {}


def _op(name):
    if name not in _BUILT:
        _BUILT[name] = W.OPS[name].build()
    return _BUILT[name]


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        x, y = _bits(a[k]), _bits(b[k])
        assert x.shape == y.shape and torch.equal(x, y), \
            f"{what}: output {k!r} differs in {int((x != y).sum())} of {x.numel()} words"


def _run(name, monkeypatch, pattern, shared=None):
    with W.poisoned(monkeypatch, pattern, shared) as ws:
        gets = ws.gets
        out = _op(name).run(ws)
        torch.cuda.synchronize()
        assert ws.gets > gets, f"{name} never asked for a workspace: the pattern was not laid"
    return {k: v.clone() for k, v in out.items()}


def _tickets_are_zero(out, what):
    if "tickets" in out:
        assert not bool(out["tickets"].any()), f"{what}: ticket words {out['tickets'].flatten().tolist()}"


@pytest.mark.parametrize("name", list(W.OPS))
def test_content_independence(name, monkeypatch):
    ref = _run(name, monkeypatch, 0x00)
    _assert_same(ref, _run(name, monkeypatch, 0x00), f"{name} is not bit-reproducible with itself under 0x00 (control)")
    for pattern in W.PATTERNS[1:]:
        _assert_same(ref, _run(name, monkeypatch, pattern), f"{name}, workspace filled with {pattern:#04x}")
    other = W.OPS[name].stale_from
    assert other != name
    shared = W.SharedWorkspace()
    _run(other, monkeypatch, 0x7F, shared)
    _assert_same(ref, _run(name, monkeypatch, None, shared), f"{name}, workspace last used by {other}")


@pytest.mark.parametrize("name", list(W.OPS))
def test_repetition(name, monkeypatch):
    shared = W.SharedWorkspace()
    first = _run(name, monkeypatch, None, shared)
    _tickets_are_zero(first, f"{name}, call 1")
    for i in (2, 3):
        again = _run(name, monkeypatch, None, shared)
        _assert_same(first, again, f"{name}, call {i} against call 1")
        _tickets_are_zero(again, f"{name}, call {i}")


def _captured(form, ws, xg, outs):
    """(graph, shape before, shape after) of one in-place step captured on a side stream."""
    hip = H._hip()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            before = H._graph_shape(hip, side.cuda_stream)
            form.call(xg, xg, outs, ws.data_ptr(), ws.numel())
            after = H._graph_shape(hip, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    return g, before, after


def _eager_chain(form, ws, steps=3):
    x, want = form.x0.clone(), []
    for _ in range(steps):                         # (the first is also the warm-up: one-time function attributes)
        outs = form.outs()
        form.call(x, x, outs, ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        want.append(form.result(x, outs))
    return want


_IDS = [f"{k}{'_ladder' if lad else ''}" for k, lad in W.CAPTURED]


@pytest.mark.parametrize("refill", [False, True], ids=["left_alone", "refilled_0xff"])
@pytest.mark.parametrize("kind,ladder", W.CAPTURED, ids=_IDS)
def test_graph_replay(kind, ladder, refill):
    form = W._step(kind, ladder)()
    assert form.fused() == 1
    ws = torch.full((form.nbytes,), 0x7F, dtype=torch.uint8, device="cuda")
    want = _eager_chain(form, ws)
    moved = [int((a["x"] != b["x"]).any(dim=1).sum()) for a, b in zip([{"x": form.x0}] + want[:-1], want)]
    print(f"chains moved by the three eager steps: {moved} of {form.B}")
    xg, outs = form.x0.clone(), form.outs()
    g, _, _ = _captured(form, ws, xg, outs)
    xg.copy_(form.x0)
    for i in range(3):                             # three replays, once
        if refill:
            ws.fill_(0xFF)                         # on the stream the replay is launched on
        for o in outs:                             # a chain that a replay leaves unwritten must not pass as one that
            o.fill_(float("nan"))                  # rejected: its outputs of the replay before are taken away
        form.sums[:3].fill_(float("nan"))          # (the ticket word stays as the step left it)
        g.replay()
        torch.cuda.synchronize()
        got = form.result(xg, outs)
        _assert_same(want[i], got, f"{_IDS[W.CAPTURED.index((kind, ladder))]}, replay {i + 1} against eager step {i + 1}")
        _tickets_are_zero(got, f"replay {i + 1}")


# kernel nodes of a captured step: the split form clears its pair tickets in a kernel of its own ahead of the step
_KERNELS = {"subtile_b3": 1, "split16_b16": 2, "split16_b19": 2, "selected_only": 1, "conv3d": 1, "periodic_whole_8x8": 1}


@pytest.mark.parametrize("kind,ladder", W.CAPTURED, ids=_IDS)
def test_graph_shape(kind, ladder):
    form = W._step(kind, ladder)()
    ws = torch.full((form.nbytes,), 0x7F, dtype=torch.uint8, device="cuda")
    _eager_chain(form, ws, steps=1)
    _, before, (kernels, others, edges) = _captured(form, ws, form.x0.clone(), form.outs())
    assert before == (0, 0, 0)
    assert others == 0, f"{others} node(s) of the captured step are no kernel nodes (a memset?)"
    assert edges == kernels - 1, (kernels, edges)              # one stream: a chain
    if kind == "cut_batch":
        assert kernels >= 3, kernels
    else:
        assert kernels == _KERNELS[kind], kernels
