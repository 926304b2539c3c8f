"""torch.autograd through a GaugeDynamics transition with one beta per chain: `dyn(x, betas)`, betas [B] (l2hmc_amd/
autograd.py on l2hmc_gauge_train_forward_ladder, l2hmc_gauge_accept_backward_ladder, l2hmc_gauge_train_backward_ladder;
without a graph l2hmc_gauge_transition_ladder).

Three betas {1, 2, 3} lie on the chains in the fixed non-periodic pattern of tests/ladder_ref.py.
  1. the accept-backward kernel alone; 2. a rung's rows have the bits of the scalar call at its beta; 3. a ladder of
  equal values is the scalar call; 4., 5. float64 autograd (ladder_ref.LadderGaugeModel) at test_gpu_autograd.py's bars;
  6. the plumbing is exact; 7. the call without a graph; 8. a torch.optim loop.
Cases, inputs and betas are the ones tests/test_gpu_gauge_train_ladder.py holds to float64 at the same gate."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle.torch_ref import action
from tests import helpers as H
from tests import ladder_ref as LR
from tests.test_gpu_autograd import (TOL_G, _accept_vjp_ref, _calc_loss, _compare_to_oracle, _draw_kw, _rel,
                                     _requires_grad, _t64)
from tests.test_gpu_gauge_train_ladder import FUSED_C9, FUSED_G9, FUSED_G24, TILED_37, TILED_L8, ids

pytestmark = pytest.mark.gpu

CASES = [FUSED_G24, FUSED_G9, FUSED_C9, TILED_37, TILED_L8]
ONE_PER_PATH = [FUSED_G9, FUSED_C9, TILED_37]


def _setup(case):
    """A dynamics object that owns its weights (no trainer), the float64 ladder model, and LR.inputs."""
    T, X, N, eps, B, regime, arch, fused = case
    xp, vp = H.gauge_weights(T, X, regime=regime) if arch == 'generic' else H.conv_weights(T, X, regime=regime)
    orc = H.gauge_oracle(T, X, N, eps, xp, vp, arch=arch)
    dyn = H.gauge_hip(T, X, N, eps, xp, vp, orc.mask, B, arch=arch)
    dyn.fused = fused
    tm = LR.LadderGaugeModel(T, X, N, eps, orc.mask, xp, vp, arch=arch)
    return dyn, tm, LR.inputs(B, 2 * T * X)


def _dev(dyn, a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=dyn._device)


def _cotangents(dyn, B, D, seed=3):
    rng = np.random.default_rng(seed)
    return [_dev(dyn, rng.standard_normal(s)) for s in ((B, D), (B, D), (B,), (B, D))]


def _weight_grads(dyn):
    out = {f"{n}.{k}": t.grad.clone() for n, net in (("xnet", dyn.position_fn), ("vnet", dyn.momentum_fn))
           for k, t in net.state_dict().items()}
    out["eps"] = dyn.eps.grad.clone()
    return out


def _call_with_cotangents(dyn, x, beta, draws, cot):
    """dyn(x, beta) with x.requires_grad_() and the fixed cotangents -> (the four outputs, x.grad, weight gradients)."""
    _requires_grad(dyn)
    xg = _dev(dyn, x).requires_grad_()
    outs = dyn(xg, beta, **_draw_kw(draws))
    sum((c * o).sum() for c, o in zip(cot, outs)).backward()
    return [o.detach() for o in outs], xg.grad, _weight_grads(dyn)


# ---- 1. the accept-backward kernel alone -------------------------------------------------------------------------------
def _accept_inputs():
    """The inputs of test_gpu_autograd.py::test_accept_backward_kernel_matches_float64 with a beta per row."""
    T, X, R = 3, 5, 131                        # odd lattice, rows not a multiple of 64
    D = 2 * T * X
    betas = np.asarray(LR.RUNGS)[np.random.default_rng(17).integers(0, 3, R)]
    rng = np.random.default_rng(5)
    x0, xN = rng.uniform(0, 2 * np.pi, (R, D)), rng.uniform(0, 2 * np.pi, (R, D))
    v0, vN = rng.standard_normal((R, D)), rng.standard_normal((R, D))
    h = lambda x, v: (_t64(betas) * action(_t64(x), T, X) + 0.5 * (_t64(v) ** 2).sum(1)).numpy()  # noqa: E731
    sld = h(xN, vN) - h(x0, v0) + rng.standard_normal(R)      # A ~ N(0, 1): p = 1 and 0 < p < 1
    g = [rng.standard_normal((R, D)), rng.standard_normal((R, D)), rng.standard_normal(R), rng.standard_normal((R, D))]
    p0 = np.exp(np.minimum(h(x0, v0) - h(xN, vN) + sld, 0))
    u = np.where(rng.uniform(size=R) < 0.5, p0 * 0.5, np.minimum(p0 + 0.25, 1.5))   # accept / reject, far from p
    ref = _accept_vjp_ref(x0, v0, xN, vN, sld, u, g, _t64(betas), T, X)
    bad = np.arange(R) % 7 == 3                # non-finite proposals: p = 0
    xN_in = xN.copy()
    xN_in[bad, 0], xN_in[bad, 1] = np.nan, np.inf
    p_in = np.where(bad, 0., ref[0])
    return T, X, R, D, betas, (x0, v0, xN_in, vN, p_in, u), g, ref, bad


def _accept(T, X, head, rows, ins, gs):
    """The entry `head` selects (a float: the scalar one; (betas, stride, chains): the ladder) on the first `rows` rows
    -> [dxN, dvN, dlogdet, dx0, dv0], each filled with 7 beforehand."""
    from l2hmc_amd import _lib
    dev = ins[0].device
    D = 2 * T * X
    outs = [torch.full(s, 7., device=dev) for s in ((rows, D), (rows, D), (rows,), (rows, D), (rows, D))]
    args = [t[:rows].contiguous() for t in ins + gs] + outs
    if isinstance(head, float):
        _lib.call("l2hmc_gauge_accept_backward", T, X, head, rows, *args, device=dev)
    else:
        _lib.call("l2hmc_gauge_accept_backward_ladder", T, X, *head, rows, *args, device=dev)
    return outs


def test_accept_backward_ladder_kernel():
    from l2hmc_amd import _lib
    T, X, R, D, betas, ins, g, ref, bad = _accept_inputs()
    dev = torch.device("cuda", torch.cuda.current_device())
    ins = [_lib.as_dev(a, dev) for a in ins]
    gs = [_lib.as_dev(a, dev) for a in g]
    bt = _lib.as_dev(betas, dev)
    names = ("dxN", "dvN", "dlogdet", "dx0", "dv0")
    got = _accept(T, X, (bt, 1, R), R, ins, gs)
    # a rung's rows are the scalar entry's at that beta
    scalar = {b: _accept(T, X, float(b), R, ins, gs) for b in LR.RUNGS}
    for b in LR.RUNGS:
        rows = torch.as_tensor(np.nonzero(betas == b)[0], device=dev)
        assert rows.numel() > 20
        for name, a, w in zip(names, got, scalar[b]):
            assert torch.equal(a[rows], w[rows]), (name, b)
    # a ladder of equal values, stride 1 and stride 0
    for head in ((torch.full((R,), 2., device=dev), 1, R), (torch.full((1,), 2., device=dev), 0, R),
                 (torch.full((1,), 2., device=dev), 0, 1)):
        for name, a, w in zip(names, _accept(T, X, head, R, ins, gs), scalar[2.0]):
            assert torch.equal(a, w), (name, head[1:])
    # chains = rows / 2: row r and row r + chains read one value
    half = _accept(T, X, (bt, 1, 65), 130, ins, gs)
    for b in LR.RUNGS:
        ch = np.nonzero(betas[:65] == b)[0]
        rows = torch.as_tensor(np.concatenate([ch, 65 + ch]), device=dev)
        for name, a, w in zip(names, half, scalar[b]):
            assert torch.equal(a[rows], w[rows]), (name, b)
    # float64 autograd with a beta per row, at the scalar test's bar
    _, dxN, dvN, dld, dx0, dv0 = ref
    dxN[bad], dvN[bad], dld[bad], dx0[bad], dv0[bad] = g[0][bad], g[1][bad], 0., g[3][bad], 0.
    p = ref[0]
    assert ((p < 1) & ~bad).sum() > 20 and ((p == 1) & ~bad).sum() > 20
    out = [o.cpu().numpy() for o in got]
    for name, a, w in zip(names, out, (dxN, dvN, dld, dx0, dv0)):
        assert np.isfinite(a).all(), name
        assert H.relerr(a, w) <= 1e-5, (name, H.relerr(a, w))
    assert (out[2][bad] == 0).all() and (out[2][p == 1] == 0).all()


# ---- 2. rows have the scalar call's bits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_rows_of_a_rung_have_the_bits_of_the_scalar_call_at_its_beta(case):
    dyn, _, (x, _, dx, _) = _setup(case)
    B, D = x.shape
    rung, betas = LR.rung_of(B), LR.ladder(B)
    cot = _cotangents(dyn, B, D)
    outs, gx, _ = _call_with_cotangents(dyn, x, betas, dx, cot)
    assert float(gx.abs().max()) > 0
    for g, b in enumerate(LR.RUNGS):
        rows = torch.as_tensor(np.nonzero(rung == g)[0], device=dyn._device)
        ref, rgx, _ = _call_with_cotangents(dyn, x, float(b), dx, cot)
        for i, (a, w) in enumerate(zip(outs, ref)):
            assert torch.equal(a[rows], w[rows]), (i, b)
        assert torch.equal(gx[rows], rgx[rows]), b


# ---- 3. a ladder of equal values is the scalar call ----------------------------------------------------------------------
@pytest.mark.parametrize("case", ONE_PER_PATH, ids=ids)
def test_a_ladder_of_equal_values_is_the_scalar_call(case):
    dyn, _, (x, _, dx, _) = _setup(case)
    B, D = x.shape
    cot = _cotangents(dyn, B, D)
    want = _call_with_cotangents(dyn, x, 2.5, dx, cot)
    for ladder in (np.full(B, 2.5), torch.full((1, B), 2.5, device=dyn._device)):
        got = _call_with_cotangents(dyn, x, ladder, dx, cot)
        for a, w in zip(got[0], want[0]):
            assert torch.equal(a, w)
        assert torch.equal(got[1], want[1])
        for k, w in want[2].items():
            assert torch.equal(got[2][k], w), k


# ---- 4. float64, the reference loss ----------------------------------------------------------------------------------------
def _ladder_loss(dyn, x, z, dx, dz, betas):
    T, X = dyn.lattice.time_size, dyn.lattice.space_size
    x, z = dyn._x(x), dyn._x(z)
    x_prop, _, px, _ = dyn(x, betas, **_draw_kw(dx))
    _, _, pz, _ = dyn(z, betas, **_draw_kw(dz))
    return _calc_loss(x, x_prop, px, z, pz, T, X)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_reference_loss_on_a_ladder_matches_float64(case):
    dyn, tm, (x, z, dx, dz) = _setup(case)
    betas = LR.ladder(case[4])
    _requires_grad(dyn)
    loss = _ladder_loss(dyn, x, z, dx, dz, betas)
    assert loss.grad_fn is not None
    loss.backward()
    want, _ = tm.loss(_t64(x), _t64(z), _t64(betas), tuple(map(_t64, dx)), tuple(map(_t64, dz)))
    want.backward()
    worst = _compare_to_oracle(dyn, tm, tol=np.inf)
    print(f"ladder {ids(case)}: loss {float(loss.detach()):.6g} against {float(want.detach()):.6g}; worst gradient ratio "
          f"{max(worst.values()):.3g} ({max(worst, key=worst.get)})")
    assert abs(float(loss.detach()) - float(want.detach())) <= 2e-4 * max(1., abs(float(want.detach())))
    _compare_to_oracle(dyn, tm)


# ---- 5. float64, every output and the input -------------------------------------------------------------------------------
def test_every_output_and_the_input_match_float64_on_a_ladder():
    """The weighted-sum loss of test_gpu_autograd.py::test_every_output_and_the_input_match_float64, chain i at
    beta[i]: accepted and rejected chains, p < 1 and p == 1 on at least two rungs each, every chain compared."""
    T = X = 8
    N, eps, B = 3, 0.1, 96                     # smoke()'s regime
    case = (T, X, N, eps, B, "mild", "generic", True)
    dyn, tm, (_, _, dx, _) = _setup(case)
    D = 2 * T * X
    rung = np.random.default_rng(17).integers(0, 3, B)
    betas = np.asarray(LR.RUNGS)[rung]
    rng = np.random.default_rng(11)
    x = rng.normal(0, 0.3, (B, D))
    c = [rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.standard_normal(B), rng.standard_normal((B, D))]
    with torch.no_grad():                      # MH uniforms kept off p, where fp32 and fp64 could select apart
        p = tm.apply_transition(_t64(x), _t64(betas), *map(_t64, dx))[2].numpy()
    dx = (*dx[:3], np.where(np.abs(p - dx[3]) < 1e-3, 0.5 * p, dx[3]))
    _requires_grad(dyn)
    xg = _dev(dyn, x).requires_grad_()
    outs = dyn(xg, betas, **_draw_kw(dx))
    sum((_dev(dyn, ci) * o).sum() for ci, o in zip(c, outs)).backward()
    x64 = _t64(x).requires_grad_()
    want = tm.apply_transition(x64, _t64(betas), *map(_t64, dx))
    sum((_t64(ci) * o).sum() for ci, o in zip(c, want)).backward()
    p, u = want[2].detach().numpy(), dx[3]
    acc = p > u
    for name, mask in (("accepted", acc), ("rejected", ~acc), ("p < 1", p < 1), ("p == 1", p == 1)):
        assert len(set(rung[mask])) >= 2, (name, np.bincount(rung[mask], minlength=3))
    worst = _compare_to_oracle(dyn, tm)
    worst["x"] = _rel(xg.grad, x64.grad)
    assert worst["x"] <= TOL_G, worst


# ---- 6. plumbing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [FUSED_G24, TILED_37], ids=ids)
def test_ladder_plumbing_is_exact(case):
    """The autograd weight gradients are, bit for bit, those of l2hmc_gauge_train_forward_ladder +
    l2hmc_gauge_accept_backward_ladder + l2hmc_gauge_train_backward_ladder called directly with the same cotangents."""
    from l2hmc_amd import _lib
    dyn, _, (x, _, dx, _) = _setup(case)
    B, D = x.shape
    T, X = dyn.lattice.time_size, dyn.lattice.space_size
    dev = dyn._device
    betas = _dev(dyn, LR.ladder(B))
    cot = _cotangents(dyn, B, D)
    outs, gx, wg = _call_with_cotangents(dyn, x, betas, dx, cot)
    xt = _dev(dyn, x)
    vf, vb, coin, u = (_lib.as_dev(a, dev) for a in dx)
    fwd = coin > 0.5
    v0 = torch.where(fwd[:, None], vf, vb).contiguous()
    dirs = (~fwd).to(torch.int32).contiguous()
    plan, L = dyn._plan(), _lib.lib()
    nb = L.l2hmc_gauge_train_ws_bytes(C.byref(plan), B)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    xN, vN = torch.empty_like(xt), torch.empty_like(xt)
    sld, p = torch.empty(B, device=dev), torch.empty(B, device=dev)
    _lib.call("l2hmc_gauge_train_forward_ladder", C.byref(plan), betas, 1, B, xt, v0, dirs, B, xN, vN, sld, p, ws, nb,
              device=dev)
    assert torch.equal(xN, outs[0]) and torch.equal(vN, outs[1]) and torch.equal(p, outs[2])
    dxN, dvN, dx0 = torch.empty_like(xt), torch.empty_like(xt), torch.empty_like(xt)
    dld = torch.empty(B, device=dev)
    _lib.call("l2hmc_gauge_accept_backward_ladder", T, X, betas, 1, B, B, xt, v0, xN, vN, p, u, *cot, dxN, dvN, dld, dx0,
              None, device=dev)
    grads = []
    for net in (dyn.position_fn, dyn.momentum_fn):
        grads.append({k: torch.zeros_like(net._packed[1][k]) for k in net.SEGMENTS})
    structs = [_lib.DenseGrads(**{k: v.data_ptr() for k, v in g.items()}) for g in grads]
    deps = torch.zeros(1, device=dev)
    _lib.call("l2hmc_gauge_train_backward_ladder", C.byref(plan), betas, 1, B, dirs, B, dxN, dvN, dld,
              C.byref(structs[0]), C.byref(structs[1]), None, None, deps, ws, nb, device=dev,
              tail=(_lib.BUCKET_FN(), None))
    for name, net, g in zip(("xnet", "vnet"), (dyn.position_fn, dyn.momentum_fn), grads):
        ref = net.unpack_grads(g)
        for k in net.state_dict():
            assert torch.equal(wg[f"{name}.{k}"], ref[k]), k
    assert torch.equal(wg["eps"].reshape(1), deps.cpu())
    assert torch.equal(gx, dx0 + dxN)


# ---- 7. no grad ------------------------------------------------------------------------------------------------------
def test_ladder_call_without_a_graph_takes_the_same_draws():
    """Without injected draws, the grad-enabled and the no-grad ladder call take the same Philox streams."""
    from l2hmc_amd import _lib
    case = (8, 8, 3, 0.1, 42, "mild", "generic", True)
    dyn, _, (x, *_) = _setup(case)
    B = case[4]
    betas = LR.ladder(B)
    _requires_grad(dyn)
    x = np.random.default_rng(9).normal(0, 0.3, x.shape)
    dyn._draws = 5
    with torch.no_grad():
        a = dyn(x, betas)
    draws_a = dyn._draws
    dyn._draws = 5
    b = dyn(x, betas)
    assert b[0].grad_fn is not None and a[0].grad_fn is None
    assert dyn._draws == draws_a == _lib.step_draw_index(5)[1]
    a = [t.cpu().numpy() for t in a]
    b = [t.detach().cpu().numpy() for t in b]
    for i in range(3):
        assert H.relerr(b[i], a[i]) <= 2e-5, i
    cu = torch.empty(2 * B, device=dyn._device)
    d, _ = _lib.step_draw_index(5)
    _lib.call("l2hmc_fill_uniform", cu, 2 * B, dyn._seed, 2 * d + 1, device=dyn._device)
    u = cu.cpu().numpy()[B:]
    safe = np.abs(a[2] - u) > 1e-4
    assert safe.sum() > B - 8
    assert H.relerr(b[3][safe], a[3][safe]) <= 2e-5


@pytest.mark.parametrize("case", [FUSED_G24, FUSED_C9, TILED_37], ids=ids)
def test_ladder_call_without_a_graph_runs_layer_by_layer(case):
    """On the tiled plan a rung's rows are the scalar no-grad call's at that beta, and a fused plan's ladder call is the
    tiled plan's bit for bit: the ladder never reaches a kernel that holds one beta."""
    dyn, _, (x, _, dx, _) = _setup(case)
    B = case[4]
    rung, betas = LR.rung_of(B), LR.ladder(B)
    with torch.no_grad():
        dyn.fused = True
        fused = dyn(x, betas, **_draw_kw(dx))
        dyn.fused = False
        tiled = dyn(x, betas, **_draw_kw(dx))
        for a, w in zip(fused, tiled):
            assert torch.equal(a, w)
        for g, b in enumerate(LR.RUNGS):
            rows = torch.as_tensor(np.nonzero(rung == g)[0], device=dyn._device)
            ref = dyn(x, float(b), **_draw_kw(dx))
            for i, (a, w) in enumerate(zip(tiled, ref)):
                assert torch.equal(a[rows], w[rows]), (i, b)
        ref = dyn(x, 2.0, **_draw_kw(dx))
        for a, w in zip(dyn(x, np.full(B, 2.0), **_draw_kw(dx)), ref):
            assert torch.equal(a, w)


# ---- 8. a torch.optim loop -------------------------------------------------------------------------------------------
def test_torch_optim_loop_on_a_ladder():
    T = X = 8
    N, eps, B = 2, 0.15, 32
    case = (T, X, N, eps, B, "init", "generic", True)
    dyn, _, (x, z, dx, dz) = _setup(case)
    betas = _dev(dyn, LR.ladder(B))
    _requires_grad(dyn)
    opt = torch.optim.Adam(dyn.trainable_variables, lr=1e-4)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = _ladder_loss(dyn, x, z, dx, dz, betas)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] != losses[0], losses
    # the sampler runs the moved weights: equal, bit for bit, to a fresh object loaded with them
    orc_mask = dyn.mask.cpu().numpy()
    fresh = H.gauge_hip(T, X, N, float(dyn.eps.detach()), *H.gauge_weights(T, X, regime="init"), orc_mask, B)
    fresh.position_fn.load_state({k: v.detach().clone() for k, v in dyn.position_fn.state_dict().items()})
    fresh.momentum_fn.load_state({k: v.detach().clone() for k, v in dyn.momentum_fn.state_dict().items()})
    with torch.no_grad():
        got = dyn(x, betas, **_draw_kw(dx))
        want = fresh(x, betas, **_draw_kw(dx))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    w0 = H.gauge_weights(T, X, regime="init")[0]["h_layer/W"]
    assert not np.array_equal(dyn.position_fn.h_layer.kernel.detach().cpu().numpy(), np.float32(w0))
