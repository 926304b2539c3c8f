"""GaugeTrainer at lattice shapes the tiled training entries do not take (GenericNet widths that are not multiples of
32: 6x6, 3x5, 4x6, 10x10), through the layered-training entries and l2hmc_u1_force_hvp.

- l2hmc_u1_force_hvp against torch double-backward of the float64 action;
- gradients against float64 autograd (oracle/torch_ref.py) per tensor at 2e-4, as test_gpu_train.py;
- the forced-layered path against the tiled entries at 32-multiple shapes, with the same draws;
- bit-reproducible gradients, the data-parallel exchange (bucketed and single all-reduce), and a 200-step run that
  raises the acceptance and resumes bit for bit from its saved state."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.torch_ref import TorchGaugeModel, action
from tests import helpers as H
from tests.test_gpu_train import _compare, _ref_grads

pytestmark = pytest.mark.gpu


def _setup_tx(T, X, N, eps, B, regime, metric='cos_diff', seed=7):
    """test_gpu_train._setup for a T x X lattice."""
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    D = 2 * T * X
    xp, vp = H.gauge_weights(T, X, regime=regime)
    orc = H.gauge_oracle(T, X, N, eps, xp, vp)
    dyn = H.gauge_hip(T, X, N, eps, xp, vp, orc.mask, B)
    tr = GaugeTrainer(dyn, metric=metric, lr_init=1e-3)
    tm = TorchGaugeModel(T, X, N, eps, orc.mask, xp, vp)
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 2 * np.pi, (B, D))
    z = rng.standard_normal((B, D))
    dx = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    dz = (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B), rng.uniform(size=B))
    return tr, tm, x, z, dx, dz


# ---- l2hmc_u1_force_hvp ----------------------------------------------------------------------------------------
def _hvp(x, u, T, X, beta):
    from l2hmc_amd import _lib
    xd = torch.tensor(x, dtype=torch.float32, device="cuda")
    ud = torch.tensor(u, dtype=torch.float32, device="cuda")
    out = torch.full_like(xd, 7.0)
    rc = _lib.lib().l2hmc_u1_force_hvp(xd.data_ptr(), ud.data_ptr(), xd.shape[0], T, X, beta, out.data_ptr(),
                                       _lib.stream_ptr())
    return rc, out


@pytest.mark.parametrize("T,X", [(6, 6), (3, 5), (2, 4), (4, 6), (10, 10), (32, 32)])
@pytest.mark.parametrize("rows", [1, 37, 131])
def test_force_hvp_matches_float64_double_backward(T, X, rows):
    from l2hmc_amd import _lib
    beta = 2.5
    rng = np.random.default_rng(T * 1000 + X * 10 + rows)
    D = 2 * T * X
    x = rng.uniform(0, 2 * np.pi, (rows, D))
    u = rng.standard_normal((rows, D))
    rc, got = _hvp(x, u, T, X, beta)
    _lib.check(rc)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(action(xt, T, X).sum(), xt, create_graph=True)
    (hv,) = torch.autograd.grad(g, xt, grad_outputs=torch.tensor(u, dtype=torch.float64))
    want = beta * hv.detach().numpy()
    assert H.relerr(got.cpu().numpy(), want) <= 1e-5


def test_force_hvp_zero_rows_writes_nothing_and_large_lattice_is_refused():
    from l2hmc_amd import _lib
    L = _lib.lib()
    x = torch.zeros(2, 72, device="cuda")
    out = torch.full_like(x, 7.0)
    assert L.l2hmc_u1_force_hvp(x.data_ptr(), x.data_ptr(), 0, 6, 6, 1.0, out.data_ptr(), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    big = torch.zeros(1, 2 * 128 * 128, device="cuda")
    rc = L.l2hmc_u1_force_hvp(big.data_ptr(), big.data_ptr(), 1, 128, 128, 1.0, big.data_ptr(), _lib.stream_ptr())
    assert rc == 1 and b"does not fit LDS" in L.l2hmc_last_error()


# ---- gradients against float64 autograd ------------------------------------------------------------------------
@pytest.mark.parametrize("T,X,N,eps,B,regime", [
    (6, 6, 3, 0.2, 6, "mild"),
    (3, 5, 2, 0.15, 37, "stress"),          # ragged rows, strong S / Q
    (4, 6, 2, 0.2, 8, "mild"),              # T != X
    (10, 10, 2, 0.1, 9, "mild"),
])
def test_layered_gradients_match_autograd(T, X, N, eps, B, regime):
    tr, tm, x, z, dx, dz = _setup_tx(T, X, N, eps, B, regime)
    assert tr.layered is None
    beta = 2.5
    loss, x_out, px, x_dq = tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
    assert tr._walk is not None                  # decided by shape: the layered path ran
    want_loss, want_terms = _ref_grads(tm, x, z, dx, dz, beta, 'cos_diff')
    np.testing.assert_allclose(tr.last_loss_terms.cpu().numpy(), want_terms, rtol=2e-4,
                               atol=1e-5 * max(1., np.abs(want_terms).max()))
    assert abs(float(loss) - want_loss) <= 2e-4 * max(1., abs(want_loss))
    _compare(tr, tm)


@pytest.mark.parametrize("metric", ['l1', 'l2', 'cos', 'cos2'])
def test_layered_gradients_other_metrics_and_weights(metric):
    tr, tm, x, z, dx, dz = _setup_tx(6, 6, 2, 0.2, 9, "mild", metric=metric)
    tr.loss_scale = 0.7
    tr.weights = dict(aux_weight=0.5, std_weight=1.3, charge_weight=0.8)
    tr.calc_loss_and_grads(x, 3.0, z=z, draws_x=dx, draws_z=dz)
    _ref_grads(tm, x, z, dx, dz, 3.0, metric, loss_scale=0.7, aux_weight=0.5, std_weight=1.3, charge_weight=0.8)
    _compare(tr, tm)


# ---- forced layered against the tiled entries ------------------------------------------------------------------
@pytest.mark.parametrize("L,N,eps,B", [(4, 3, 0.15, 6), (8, 2, 0.1, 16)])
def test_forced_layered_matches_tiled(L, N, eps, B):
    tr, tm, x, z, dx, dz = _setup_tx(L, L, N, eps, B, "mild")
    # u = 0: x_out is the proposal wherever p > 0 (strict), so it shows x_prop
    dx = dx[:3] + (np.zeros(B),)
    tr.layered = False
    _, xa, pa, _ = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert tr._walk is None
    ga, pza = tr.grad_views(), tr.last_pz.clone()
    ga = {n: ({k: v.clone() for k, v in ga[n].items()} if n != "eps" else ga[n].clone()) for n in ga}
    xa, pa = xa.clone(), pa.clone()
    tr.layered = True
    _, xb, pb, _ = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert tr._walk is not None
    assert bool((pa > 0).all())
    gb = tr.grad_views()
    worst = {}
    for name in ("xnet", "vnet"):
        for k, want in ga[name].items():
            scale = float(want.abs().max())
            assert scale > 0, (name, k)
            worst[f"{name}.{k}"] = float((gb[name][k] - want).abs().max()) / scale
    worst["eps"] = abs(float(gb["eps"][0]) - float(ga["eps"][0])) / abs(float(ga["eps"][0]))
    assert max(worst.values()) <= 2e-5, worst
    assert H.relerr(xb.cpu().numpy(), xa.cpu().numpy()) <= 1e-5
    assert float((pb - pa).abs().max()) <= 1e-5
    # the z chains' H = beta S + |v|^2 / 2 is about 200 at 8x8, whose fp32 spacing is 1.5e-5: two summation orders of
    # H0 - H1 may differ by that much, and p = exp(H0 - H1 + sumlogdet) with them (the parity tests' 2e-5 for p)
    assert float((tr.last_pz - pza).abs().max()) <= 2e-5


def test_layered_gradients_are_reproducible():
    tr, tm, x, z, dx, dz = _setup_tx(6, 6, 3, 0.2, 11, "stress")
    tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    g1 = tr.grads.clone()
    tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    assert torch.equal(g1, tr.grads)


# ---- data-parallel ---------------------------------------------------------------------------------------------
def test_layered_data_parallel_gradients_equal_full_batch(tmp_path):
    """Two ranks on the test box's one GPU over gloo, each with half of the chains: the bucketed exchange (three
    ranges: xnet, vnet, eps) and one all-reduce of the whole buffer give the same bits, and the full-batch gradient."""
    B = 10
    tr, tm, x, z, dx, dz = _setup_tx(6, 6, 2, 0.2, B, "mild")
    loss, *_ = tr.calc_loss_and_grads(x, 2.5, z=z, draws_x=dx, draws_z=dz)
    full = tr.grads.cpu().numpy().copy()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "dp.npz")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(os.path.dirname(__file__),
                                                                    "dp_gauge_layered_worker.py"), out, str(B)],
                                      env=env))
    for p in procs:
        assert p.wait(timeout=300) == 0
    with np.load(out) as f:
        got, got_loss, lr = f["grads"], float(f["loss"]), float(f["lr"])
        np.testing.assert_array_equal(f["grads"], f["grads_single"])
        assert int(f["buckets"]) == 3
    assert abs(got_loss - float(loss)) <= 1e-5 * max(1., abs(float(loss)))
    assert np.abs(got - full).max() <= 2e-5 * np.abs(full).max()
    assert lr == pytest.approx(2 * tr.learning_rate())


# ---- end to end ------------------------------------------------------------------------------------------------
def _trainer_6x6(B, eps, seed=5):
    """A hot start with the settings of examples/train_and_sample_u1.py (eps 0.2, lr 3e-4 decaying every 100 steps)."""
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    from l2hmc_amd.gauge_trainer import GaugeTrainer
    np.random.seed(seed)
    lat = GaugeLattice(6, 6, 2, 'U1', num_samples=B, rand=True)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, num_steps=5, eps_trainable=True)
    return GaugeTrainer(dyn, lr_init=3e-4, lr_decay_steps=100, lr_decay_rate=0.96)


def test_layered_training_raises_acceptance_and_resumes_bit_for_bit(tmp_path):
    B = 512
    tr = _trainer_6x6(B, eps=0.2)
    eps0 = float(tr.dynamics.eps)
    out = tr.train(200, beta_init=2., beta_final=2.)
    assert tr._walk is not None
    for k in ("loss", "accept_prob", "eps"):
        assert np.isfinite(out[k]).all(), k
    assert float(tr.dynamics.eps) != eps0
    acc = out["accept_prob"]
    assert acc[-50:].mean() > acc[:50].mean(), (acc[:50].mean(), acc[-50:].mean())
    x = out["samples"]
    path = str(tmp_path / "state.npz")
    tr.save_state(path, samples=x, beta=2.0)
    a = tr.train_step(x, 2.0)
    wa = [n.flat_params()[0].clone() for n in tr._nets]
    tr2 = _trainer_6x6(B, eps=0.3, seed=11)      # other weights and masks: load_state must restore all of them
    extra = tr2.load_state(path)
    x2 = torch.as_tensor(extra["samples"], device="cuda")
    b = tr2.train_step(x2, float(extra["beta"]))
    assert float(a[0]) == float(b[0])
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for p, q in zip(wa, [n.flat_params()[0] for n in tr2._nets]):
        assert torch.equal(p, q)
    assert float(tr.dynamics.eps) == float(tr2.dynamics.eps) and tr.global_step == tr2.global_step
