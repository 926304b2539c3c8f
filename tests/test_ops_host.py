"""Host-side checks of the Python boundary of the C ABI (l2hmc_amd/ops.py, _lib.call): a tensor that is not a
contiguous GPU tensor of the dtype the entry reads raises, with the argument's name, before the library or torch.cuda
is touched.  No GPU, no library."""
import numpy as np
import pytest
import torch

from l2hmc_amd import _lib, ops

T, X, B = 4, 6, 3
D = 2 * T * X


# per function: ({tensor argument: shape} in call order, the scalars that follow them)
CASES = {
    "kinetic_energy": (dict(v=(B, D)), ()),
    "accept_prob": (dict(h_old=(B,), h_new=(B,), sumlogdet=(B,)), ()),
    "wrap_angle": (dict(x=(B, D), out=(B, D)), ()),
    "lf_update_v": (dict(v=(B, D), grad=(B, D), S=(B, D), T=(B, D), Q=(B, D)), (0.1, 0)),
    "lf_update_x": (dict(x=(B, D), v=(B, D), keep=(D,), S=(B, D), T=(B, D), Q=(B, D)), (0.1, 1)),
    "mix_accept": (dict(x=(B, D), xf=(B, D), vf=(B, D), pf=(B,), xb=(B, D), vb=(B, D), pb=(B,), coin=(B,), u=(B,)), (1,)),
    "u1_action_force": (dict(x=(B, D)), (T, X, 2.0)),
    "u1_force_hvp": (dict(x=(B, D), u=(B, D)), (T, X, 2.0)),
    "fill_normal": (dict(out=(B, D)), ()),
    "fill_uniform": (dict(out=(B, D)), ()),
}


def _run(fn, tensors):
    if fn.startswith("fill_"):
        return getattr(ops, fn)(None, 1, 0, out=tensors[0])
    return getattr(ops, fn)(*tensors, *CASES[fn][1])


@pytest.fixture
def no_backend(monkeypatch):
    """The library and the torch.cuda entries the boundary uses raise: validation has to come first."""
    def boom(*a, **k):
        raise AssertionError("validation must not reach the library or torch.cuda")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "stream_ptr", boom)
    for name in ("current_stream", "current_device", "_lazy_init"):
        monkeypatch.setattr(torch.cuda, name, boom)


def test_cases_cover_every_function_of_ops():
    public = {n for n, f in vars(ops).items() if callable(f) and not n.startswith("_") and f.__module__ == ops.__name__}
    assert public == set(CASES)


@pytest.mark.parametrize("fn", list(CASES))
def test_cpu_tensors_and_numpy_arrays_raise_before_the_library(no_backend, fn):
    shapes = CASES[fn][0]
    first = next(iter(shapes))
    with pytest.raises(RuntimeError, match=f"^{first}: .*no CPU fallback"):
        _run(fn, [torch.zeros(s) for s in shapes.values()])
    with pytest.raises(TypeError, match=f"^{first}: expected a torch.Tensor, got ndarray"):
        _run(fn, [np.zeros(s, dtype=np.float32) for s in shapes.values()])


@pytest.mark.parametrize("fn,bad", [(fn, a) for fn, (shapes, _) in CASES.items() for a in shapes])
def test_each_argument_is_checked_and_named(no_backend, monkeypatch, fn, bad):
    """One offender among arguments that pass (stand-ins for good GPU tensors, waved through `dev_ptr`): the error
    names that argument."""
    shapes = CASES[fn][0]
    good = [torch.zeros(s) for s in shapes.values()]
    real = _lib.dev_ptr
    monkeypatch.setattr(_lib, "dev_ptr", lambda t, dtype=torch.float32, name="tensor":
                        1 if any(t is g for g in good) else real(t, dtype, name))
    i = list(shapes).index(bad)
    with pytest.raises(RuntimeError, match=f"^{bad}: .*no CPU fallback"):
        _run(fn, good[:i] + [torch.zeros(shapes[bad])] + good[i + 1:])
    with pytest.raises(TypeError, match=f"^{bad}: expected a torch.Tensor, got ndarray"):
        _run(fn, good[:i] + [np.zeros(shapes[bad], dtype=np.float32)] + good[i + 1:])


def test_lib_call_checks_tensors_and_passes_the_rest_through(monkeypatch):
    seen = []

    class Stub:
        @staticmethod
        def l2hmc_stub(*args):
            seen.append(args)
            return 0
    calls = {"lib": 0}

    def lib():
        calls["lib"] += 1
        return Stub
    monkeypatch.setattr(_lib, "lib", lib)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: 77)
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        _lib.call("l2hmc_stub", 3, torch.zeros(4), None)
    assert "l2hmc_stub" in str(e.value) and "argument 1" in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.call("l2hmc_stub", torch.zeros(4, dtype=torch.int32))
    assert calls["lib"] == 0 and not seen, "a bad tensor must not reach the library"
    plan = object()
    _lib.call("l2hmc_stub", plan, None, 5, 2.5, device="cuda", tail=("cb", None))
    assert seen == [(plan, None, 5, 2.5, 77, "cb", None)]
    Stub.l2hmc_stub = staticmethod(lambda *a: 1)
    Stub.l2hmc_last_error = staticmethod(lambda: b"bad rows")
    with pytest.raises(ValueError, match="bad argument: bad rows"):
        _lib.call("l2hmc_stub", 1)
