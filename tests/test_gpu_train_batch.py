"""Training gradients at benchmark batch sizes, where the weight-gradient reductions split (train.hip
gemm_tn / colsum, the ConvNet3D filter partials, the toy-target partials) -- checks that relu flips cannot disturb.

test_gpu_train.py pins the gradients to float64 autograd at up to 37 chains.  At thousands of chains a direct
max-norm comparison with float64 is noise: a few relu pre-activations land within rounding of 0, fall on the other
side in fp32, and move one row of every gradient below that relu by a full term
(profiles/r01_train_gradient_parity_B8200_1LF.txt).  So each case here runs three checks:

1. Batch additivity.  The loss is a per-chain mean, so B * g(B) = sum_s B_s * g(shard_s) for the same chains and
   draws cut into shards small enough to sit in the regime that float64 autograd pins (one split, one column-sum
   chunk).  The taped forward pass is first shown to be bit-identical between the full batch and the shards (same
   relu gates), so the only difference left is the grouping of the fp32 sums.  Element-wise, per tensor:
       |B g(B) - sum_s B_s g_s| <= C_ADD * max(m, FLOOR_ADD * max(m)),   m = sum_s |B_s g_s|.
   The floor is for entries that cancel inside a single chain (m is then the cancelled sum, not the size of its
   terms): measured at ConvNet3D L=16, an entry of 4.9e-6 in a tensor whose largest is 1.2e4, fed by one chain,
   differs by 3e-9 = 6e-4 of m.
   The taped forward pass was bit-identical on every path here, the layered gemm_relu forms included, so no case
   needs to fall back to checks 2 and 3 alone.
2. Float64 autograd at the full batch.  Tensors no relu gates (whd_t, bhd, coeff_s, coeff_q, eps) and the loss in
   the max norm at TOL_U; the gated ones (w1_t, wt, b1, wh_t, bh, the Conv3D filters) in the Frobenius norm against
   float32 torch autograd of the same graph:  |g - g64|_F <= K_F * max(|g32 - g64|_F, FLOOR_F * |g64|_F).
   The floor is the relu-flip noise level: float32 torch itself sits at up to 4.7e-4 of the norm at these batches
   (generic B = 4100, vnet.w1_t), but at 4e-6 where it happens to flip almost nothing (B = 16384, vnet.wh_t, where
   the HIP path sits at 1.5e-4): without the floor that single draw would set K_F to 38.
3. Reproducibility.  A second call on the same inputs gives bit-equal gradients (train.hip: no float atomics).

Every case asserts that its batch lands in the reduction regime its comment names, through a mirror of the
library's heuristics (_tn_splits, _colsum_chunks, _bwd_data_form, _conv_cpw below): a change to them fails here
instead of silently moving coverage.

Measured on the MI355X (1 LF, "mild" weights; the checks are deterministic, so these are exact for these inputs):
  additivity, worst over all tensors:  generic fused 8.4e-6 (B = 1000), 1.3e-6 (4100), 5.1e-7 (16384); layered
      2.3e-6 (3000), 1.2e-6 (8200); ConvNet3D 1.7e-5 (L = 8), 6e-4 (L = 16) before the floor; toy 3.2e-7 (MoG),
      4.2e-7 (SCG).  With the floor: <= 8.4e-6 (ConvNet3D L = 16: 4.1e-6).
  |g - g64|_F / max(|g32 - g64|_F, 1e-4 |g64|_F), worst tensor:  2.4 (layered B = 3000, xnet.wt / b1);  <= 2.3 elsewhere.
  ungated tensors, max norm:  <= 2.3e-5 (ConvNet3D L = 16, xnet.bhd), toy <= 5.1e-5 (MoG vnet.coeff_q); loss <= 2e-6.
  wall time per case: <= 4 s, except generic B = 16384 (7.9 s) and ConvNet3D L = 16 (7.4 s; float64 graph 6 s on 16
  threads); 28 s for the module.
Injected faults (on a build that drops the last split-k partial of gemm_tn, the last column-sum chunk, the last
ConvNet3D filter partial, or the last toy-target partial) fail every case that runs the reduction concerned."""
import os
import time

import numpy as np
import pytest
import torch

from oracle.torch_ref import TorchGaugeModel
from tests import helpers as H
from tests.test_gpu_train import _mlp_packed_ref, _packed_ref, _ref_grads, _setup, _small_setup

pytestmark = pytest.mark.gpu

C_ADD = 5e-5        # additivity bound (measured <= 1e-5)
FLOOR_ADD = 1e-6    # ... below this fraction of the tensor's largest m, m is replaced by the floor
TOL_U = 1e-4        # ungated tensors and the loss against float64, max norm (measured <= 5.1e-5)
K_F = 5.0           # gated tensors: Frobenius distance from float64 in units of float32 torch's (measured <= 2.4)
FLOOR_F = 1e-4      # ... which is never taken below this fraction of the tensor's norm

UNGATED = ("whd_t", "bhd", "coeff_s", "coeff_q")
GATED = ("w1_t", "wt", "b1", "wh_t", "bh", "w1_a", "b1_a", "w2_a", "b2_a", "w1_b", "b1_b", "w2_b", "b2_b")


# ------------------------------------------------------------------ mirror of the library's reduction heuristics
def _cdiv(a, b):
    return -(-a // b)


def _tn_splits(M, N, R):
    """train.hip tn_splits + gemm_tn: (splits, chunk) of the split-k TN product P[R][M]^T . Q[R][N]."""
    mt, nt = _cdiv(M, 128), _cdiv(N, 128)
    s = min(max(1, 512 // (mt * nt)), max(1, _cdiv(R, 256)))
    return s, _cdiv(_cdiv(R, s), 16) * 16


def _colsum_chunks(Rt):
    """train.hip colsum_chunks (kColsumMaxS = 512) and colsum_args: (S, rows per chunk)."""
    S = min(512, max(1, Rt // 128))
    return S, _cdiv(Rt, S)


def _bwd_data_form(rows, N, K):
    """stq_dense.hip launch_gemm_relu, kind 3/4 (aligned widths): '128' = gemm_relu_kernel<128, k, 32>,
    '64' = <64, k, 32>, 'deep3' = <64, k, 64, 64>."""
    ntiles = _cdiv(N, 128)
    if _cdiv(rows, 128) * ntiles >= 512:
        return "128"
    return "deep3" if K % 64 == 0 and _cdiv(rows, 64) * ntiles <= 256 else "64"


def _conv_cpw(T, X, F):
    """conv3d_front.hip conv3d_cpw: chains per workgroup of the backward kernel (one filter partial each)."""
    return min(16, max(1, 512 // ((T // 2) * (X // 2) * F)))


def _toy_partials(rows):
    """small_train.hip: one gradient partial per 256-thread workgroup of 16-lane chains."""
    return _cdiv(rows, 256 // 16)


def _products(D, H, Kin, Rt):
    """(splits, chunk) of the three weight-gradient products of one network at contraction length Rt."""
    return {"w1": _tn_splits(H, Kin, Rt), "wh": _tn_splits(H, H, Rt), "whd": _tn_splits(3 * D, H, Rt)}


# ------------------------------------------------------------------ the three checks
def _shards(B, size):
    return [(a, min(B, a + size)) for a in range(0, B, size)]


def _cut(t, a, b):
    return tuple(d[a:b] for d in t)


def _segments(tr):
    """(name, start, stop) of every gradient tensor in the trainer's flat buffer."""
    base = tr.grads.storage_offset()
    out = []
    for name, g in tr.grad_views().items():
        for k, v in (g.items() if isinstance(g, dict) else [("", g)]):
            a = v.storage_offset() - base
            out.append((f"{name}.{k}" if k else name, a, a + v.numel()))
    return out


def _gauge_call(tr, x, z, dx, dz, beta):
    loss, x_out, px, _ = tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
    fwd = [t.cpu().numpy().copy() for t in (tr.last_loss_terms, x_out, px, tr.last_pz)]
    return float(loss), fwd, tr.grads.cpu().clone()


def _toy_call(tr, x, z, dx, dz):
    loss, x_out, px = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
    B = x.shape[0]
    p, prop = tr.last_p.cpu().numpy(), tr.last_proposals.cpu().numpy()
    fwd = [tr.last_terms.cpu().numpy()[:B].copy(), x_out.cpu().numpy().copy(), p[:B].copy(), p[B:].copy(),
           prop[:B].copy(), prop[B:].copy()]
    return float(loss), fwd, tr.grads.cpu().clone()


def _additivity(call, segs, B, shard, x, z, dx, dz):
    """Checks 1 and 3.  Returns the worst ratio of |B g(B) - sum B_s g_s| to its bound's scale, and the shard count."""
    loss, fwd, g = call(x, z, dx, dz)
    parts = [[] for _ in fwd]
    acc = torch.zeros(g.shape, dtype=torch.float64)
    mag = torch.zeros_like(acc)
    for a, b in _shards(B, shard):
        _, f, gs = call(x[a:b], z[a:b], _cut(dx, a, b), _cut(dz, a, b))
        for lst, t in zip(parts, f):
            lst.append(t)
        term = (b - a) * gs.double()
        acc += term
        mag += term.abs()
    # same chains, same draws: the taped forward pass (hence every relu gate) is bit-identical
    for i, (want, lst) in enumerate(zip(fwd, parts)):
        np.testing.assert_array_equal(np.concatenate(lst), want, err_msg=f"forward output {i} depends on the batch")
    # check 3: after the shard calls, the same full-batch call again gives the same bits
    loss2, fwd2, g2 = call(x, z, dx, dz)
    assert loss2 == loss and torch.equal(g2, g), "calc_loss_and_grads is not reproducible"
    diff = (B * g.double() - acc).abs()
    ratios = {}
    for name, a, b in segs:
        d, m = diff[a:b], mag[a:b]
        m = torch.clamp(m, min=FLOOR_ADD * float(m.max()))
        ratios[name] = float((d / m).max()) if float(m.max()) > 0 else (0. if float(d.max()) == 0 else float("inf"))
    bad = {k: f"{v:.2e}" for k, v in ratios.items() if not v <= C_ADD}
    assert not bad, f"batch additivity: {bad} > {C_ADD:.0e}"
    return max(ratios.values()), len(_shards(B, shard))


def _f64_check(tr, tm, t32, x, z, dx, dz, beta, loss):
    """Check 2 for the lattice trainer: ungated tensors in the max norm, gated ones in the Frobenius norm."""
    want_loss, _ = _ref_grads(tm, x, z, dx, dz, beta, 'cos_diff')
    f32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)   # noqa: E731
    l32, _ = t32.loss(f32(x), f32(z), beta, tuple(map(f32, dx)), tuple(map(f32, dz)))
    l32.backward()
    gv = tr.grad_views()
    ratios, bad = {"loss": abs(loss - want_loss) / max(1., abs(want_loss))}, []
    for name, net, n32 in (("xnet", tm.xnet, t32.xnet), ("vnet", tm.vnet, t32.vnet)):
        ref64, ref32 = _packed_ref(net), _packed_ref(n32)
        for k, w in ref64.items():
            got = gv[name][k].cpu().numpy().astype(np.float64).reshape(w.shape)
            if k in UNGATED:
                ratios[f"{name}.{k}"] = float(np.abs(got - w).max() / np.abs(w).max())
            else:
                assert k in GATED, k
                yard = max(np.linalg.norm(ref32[k] - w), FLOOR_F * np.linalg.norm(w))
                ratios[f"{name}.{k}/F"] = float(np.linalg.norm(got - w) / yard)
    ratios["eps"] = abs(float(gv["eps"][0]) - float(tm.eps.grad)) / abs(float(tm.eps.grad))
    for k, r in ratios.items():
        if not r <= (K_F if k.endswith("/F") else TOL_U):
            bad.append(k)
    assert not bad, f"float64 autograd: {[(k, f'{ratios[k]:.2e}') for k in bad]}\nall: {ratios}"
    return ratios


def _gauge_case(L, N, eps, B, regime, arch, fused, shard, beta=2.0):
    tr, tm, x, z, dx, dz = _setup(L, N, eps, B, regime, arch=arch)
    if fused is not None:
        tr.dynamics.fused = fused
    t0 = time.perf_counter()
    worst, nshards = _additivity(lambda *a: _gauge_call(tr, *a, beta), _segments(tr), B, shard, x, z, dx, dz)
    t1 = time.perf_counter()
    # check 2 at the full batch: the float64 graph takes at most 6 s on 16 threads (ConvNet3D L = 16)
    loss, *_ = _gauge_call(tr, x, z, dx, dz, beta)
    xp, vp = H.gauge_weights(L, L, regime=regime) if arch == 'generic' else H.conv_weights(L, L, regime=regime)
    t32 = TorchGaugeModel(L, L, N, eps, tm.mask.numpy(), xp, vp, arch=arch, dtype=torch.float32)
    with _threads(16):
        ratios = _f64_check(tr, tm, t32, x, z, dx, dz, beta, loss)
    t2 = time.perf_counter()
    return dict(additivity=worst, shards=nshards, ratios=ratios, t_add=t1 - t0, t_f64=t2 - t1)


class _threads:
    def __init__(self, n):
        self.n = min(n, os.cpu_count() or 1)

    def __enter__(self):
        self.old = torch.get_num_threads()
        torch.set_num_threads(self.n)

    def __exit__(self, *exc):
        torch.set_num_threads(self.old)


# ------------------------------------------------------------------ GenericNet, 8x8 lattice (D = 128, H = 512), 1 LF
D8, H8, KIN8 = 128, 512, 256


@pytest.mark.parametrize("B", [
    1000,       # Rt = 4000: 16 splits in every product (below the caps), last split ragged (160 of 256 rows);
                # 31 column-sum chunks, the last one short
    4100,       # Rt = 16400: W1 at its 64-split cap with splits 61-63 empty, head (whd) 42 splits with split 41 empty
    16384,      # Rt = 65536: the column sums reach their 512-chunk cap
])
def test_fused_gradients_at_large_batch(B):
    Rt = 4 * B          # 2 calls x (x and z chains)
    pr = _products(D8, H8, KIN8, Rt)
    S, _ = _colsum_chunks(Rt)
    if B == 1000:
        assert all(s == 16 and Rt % c and (s - 1) * c < Rt for s, c in pr.values()), pr
        assert S == 31 and Rt % S, S
    elif B == 4100:
        s, c = pr["w1"]
        assert (s, c) == (64, 272) and 60 * c < Rt <= 61 * c, pr
        s, c = pr["whd"]
        assert s == 42 and (s - 1) * c >= Rt, pr
    else:
        assert S == 512, S
    # the shards: 32 chains = 128 taped rows, one split and one column-sum chunk (the regime autograd pins)
    shard = 32
    assert all(s == 1 for s, _ in _products(D8, H8, KIN8, 4 * shard).values()) and _colsum_chunks(4 * shard)[0] == 1
    _gauge_case(8, 1, 0.1, B, "mild", "generic", True, shard)


@pytest.mark.parametrize("B", [
    3000,       # 6000 rows per call: d2 / d1 (kind 3, N = 512) in the 64-row form, din (kind 4, N = 256) in deep3
    8200,       # 16400 rows: kind 3 in the 128-row form, kind 4 in the 64-row form
])
def test_layered_gradients_at_large_batch(B):
    rows = 2 * B
    if B == 3000:
        assert _bwd_data_form(rows, H8, 3 * D8) == _bwd_data_form(rows, H8, H8) == "64"
        assert _bwd_data_form(rows, KIN8, H8) == "deep3"
    else:
        assert _bwd_data_form(rows, H8, 3 * D8) == _bwd_data_form(rows, H8, H8) == "128"
        assert _bwd_data_form(rows, KIN8, H8) == "64"
    shard = 32
    assert _bwd_data_form(2 * shard, H8, H8) == _bwd_data_form(2 * shard, KIN8, H8) == "deep3"
    _gauge_case(8, 1, 0.1, B, "mild", "generic", False, shard)


# ------------------------------------------------------------------ ConvNet3D (F = L, H = 2D), 1 LF
@pytest.mark.parametrize("L,B", [
    (16, 1024),     # cfg 4's shape (F = 16, H = 1024) at its per-GPU 1024 chains: 1 chain per filter partial, 2048 of them
    (8, 1024),      # 8x8, F = 8: 4 chains per partial, 512 of them
])
def test_conv3d_gradients_at_large_batch(L, B):
    cpw = _conv_cpw(L, L, L)
    nwg = _cdiv(2 * B, cpw)
    assert nwg >= 512, nwg          # hundreds of filter partials per network
    shard = 16
    _gauge_case(L, 1, 0.1, B, "mild", "conv3D", None, shard)


# ------------------------------------------------------------------ toy targets
@pytest.mark.parametrize("kind,H_nodes,N,regime,B", [
    ("mog", 50, 10, "mild", 4096),      # cfg 2: 8192 rows in 512 workgroup partials
    ("scg", 10, 5, "stress", 4096),     # cfg 1's 16-wide variant
])
def test_toy_target_gradients_at_large_batch(kind, H_nodes, N, regime, B):
    assert _toy_partials(2 * B) == 512
    _toy_case(kind, H_nodes, N, regime, B, 32)


def _toy_case(kind, H_nodes, N, regime, B, shard):
    assert _toy_partials(2 * shard) == 4
    tr, tm, x, z, dx, dz = _small_setup(kind, H_nodes, N, 0.1, B, regime)
    t0 = time.perf_counter()
    worst, nshards = _additivity(lambda *a: _toy_call(tr, *a), _segments(tr), B, shard, x, z, dx, dz)
    t1 = time.perf_counter()
    # check 2: float64 autograd on the tensors no relu gates (the toy graph has no float32 restatement)
    loss, *_ = _toy_call(tr, x, z, dx, dz)
    tt = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))   # noqa: E731
    with _threads(16):
        want, *_ = tm.mog_loss(tt(x), tt(z), tuple(map(tt, dx)), tuple(map(tt, dz)), 0.1)
        want.backward()
    want = want.item()
    gv = tr.grad_views()
    ratios = {"loss": abs(loss - want) / max(1., abs(want))}
    for name, net in (("xnet", tm.xnet), ("vnet", tm.vnet)):
        ref = _mlp_packed_ref(net)
        for k in UNGATED:
            w = ref[k]
            got = gv[name][k].cpu().numpy().astype(np.float64).reshape(w.shape)
            ratios[f"{name}.{k}"] = float(np.abs(got - w).max() / np.abs(w).max())
    ratios["alpha"] = abs(float(gv["alpha"][0]) - float(tm.alpha.grad)) / abs(float(tm.alpha.grad))
    t2 = time.perf_counter()
    bad = {k: v for k, v in ratios.items() if not v <= TOL_U}
    assert not bad, f"float64 autograd: {bad}\nall: {ratios}"
    return dict(additivity=worst, shards=nshards, ratios=ratios, t_add=t1 - t0, t_f64=t2 - t1)
