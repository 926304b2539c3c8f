"""Replica exchange INSIDE the one-launch L2HMC toy-target run: `DynamicsSampler.run_exchange` with
`in_launch = True` (l2hmc_small_run_exchange: the rounds between two steps of ONE launch of small_traj_mfma_kernel's
EXCHANGE instances).

The round is held to float64 in tests/test_gpu_small_replica_swap.py, the tempered run in
tests/test_gpu_small_run_tempered.py and their composition between launches -- today's `run_exchange` -- in
tests/test_gpu_small_hmc_exchange.py, whose building blocks are used here.  What is new is where the round runs, so the
yardstick is the same sampler with `in_launch = False`, and every comparison with it is an equality: group sizes that
divide the eight chains of a wave (2, 4, 8: the run's own placement) and that do not (3, 5, 6, 7: packed placements
with idle slots), every first-layer form, chunks that end inside a swap period, both parities.  The target is the
other yardstick: 4096 groups of exact samples of the tempered Gaussians at every rung stay exact under L2HMC steps with
untrained networks and a round after each (Metropolis-Hastings makes any weights exact).

Measured on the MI355X (`_report`'s line of test_exchange_run_leaves_every_rung_invariant):
  [invariance] toy L2HMC + replica exchange in the launch: max|z| = 2.71 (checkpoint 1, rung 2, f7) accept 0.939,
  exchanges per pair and round 0.671; the 56 tests of the file take 7.6 s.
The power controls of the round's rule (tests/test_gpu_small_hmc_exchange.py::test_exchange_power_controls) run the same
device function and are not repeated."""
import math
import time

import numpy as np
import pytest
import torch

from tests import toy_replica_ref as TR
from tests.replica_ref import lower_chains
from tests.run_cases import count_launches
from tests.test_gpu_small_hmc_exchange import HIST, ROUNDS, STEPS, TOYS, _assert_same, _loop, _report, _temps, _x0
from tests.test_gpu_small_hmc_exchange import _sampler as _hmc_exchange_sampler

pytestmark = pytest.mark.gpu

Z_PASS = 5.0                         # tests/test_gpu_invariance.py


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _sampler(la, kind, spl=256, in_launch=True, nodes=10, form=0):
    """The L2HMC sampler of tests/test_gpu_small_hmc_exchange.py (stress-regime nets, seed 7, draws at 4)"""
    smp = _hmc_exchange_sampler(la, kind, spl, hmc=False, nodes=nodes)
    smp.dynamics.first_layer_form = form
    smp.in_launch = in_launch
    return smp


def _same_run(out, ref, smp, ref_smp, what):
    """Everything `run_exchange` returns and leaves behind, bit for bit"""
    _assert_same(out, ref, smp, ref_smp, what)
    assert np.array_equal(out["swap_rate"], ref["swap_rate"], equal_nan=True), what
    assert out["mean_accept"] == ref["mean_accept"], what
    assert torch.equal(smp.replica, ref_smp.replica), what
    assert out["swapped"].dtype == np.bool_ and out["replica"].dtype == np.int32 and out["swap_p"].dtype == np.float32


def _batches(G):
    """72 chains: a partial last workgroup; a group size that does not divide 8: 8 groups (packed placement, more waves
    than the run without exchange has) and one group alone"""
    return (72,) if 8 % G == 0 else (8 * G, G)


def _check_against_between_launches(la, kind, G, batches, spls=(256, 3, 7), **kw):
    dim = TOYS[kind][0]
    exchanged = 0
    for B in batches:
        x0 = _x0(B, dim)
        keep = x0.clone()
        for k in (1, 5):
            temps = _temps(B, G) if k == 1 else _temps(B, G, STEPS)      # a ladder; a ladder with a schedule
            for fp in (0, 1):
                ref_smp = _sampler(la, kind, in_launch=False, **kw)
                ref = ref_smp.run_exchange(STEPS, x0, temperature=temps, replicas=G, swap_every=k, first_parity=fp)
                assert ref_smp.dynamics._draws == 4 + 4 * STEPS + STEPS // k
                for spl in spls:                                     # (3, 7: a chunk ends inside a swap period of 5)
                    what = f"{kind} B={B} G={G} swap_every={k} first_parity={fp} steps_per_launch={spl} {kw}"
                    smp = _sampler(la, kind, spl, **kw)
                    assert smp.exchange_in_launch(G)
                    out = smp.run_exchange(STEPS, x0, temperature=temps, replicas=G, swap_every=k, first_parity=fp)
                    assert out["swap_p"].shape == (STEPS // k, B) and out["px"].shape == (STEPS, B), what
                    assert out["samples"].shape == (STEPS, B, dim), what
                    _same_run(out, ref, smp, ref_smp, what)
                    assert np.array_equal(smp.replica.cpu().numpy(), out["replica"][-1]), what
                exchanged += int(ref["swapped"].sum())
        assert torch.equal(x0, keep)                                 # the caller's x is not advanced in place
    assert exchanged > 0
    return exchanged


# ----------------------------------------------------------------- 1. the values of the round between launches
@pytest.mark.parametrize("G", [2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("kind", list(TOYS))
def test_in_launch_is_the_round_between_launches(la, kind, G):
    _check_against_between_launches(la, kind, G, _batches(G))


# ----------------------------------------------------------------- 2. every form
@pytest.mark.parametrize("G", [4, 3])
@pytest.mark.parametrize("kind,nodes,form", [("mog", 10, 1), ("mog", 10, 2), ("mog", 10, 0), ("gmm5", 50, 1),
                                             ("gmm5", 50, 2), ("gmm5", 50, 0), ("gmm5", 50, 3), ("rw", 50, 3),
                                             ("rw", 10, 2)])
def test_every_form(la, kind, nodes, form, G):
    _check_against_between_launches(la, kind, G, _batches(G), nodes=nodes, form=form)


@pytest.mark.parametrize("nodes", [10, 50])
def test_the_form_follows_the_batch_and_not_the_packed_waves(la, nodes):
    """72 chains in groups of 3 are 9 groups of 16 rows and 12 packed waves: the run is that of the loop over single
    `propose` steps (steps_per_launch = 1), which knows nothing of the placement.  That loop has one temperature for
    all chains, so the ladder is a schedule here and every proposed exchange certain."""
    kind, B, G = "mog", 72, 3
    x0 = _x0(B, TOYS[kind][0])
    temps = 1.0 + 0.25 * np.arange(STEPS)
    for fp in (0, 1):
        ref_smp = _hmc_exchange_sampler(la, kind, 1, hmc=False, nodes=nodes)
        ref = _loop(ref_smp, STEPS, temps, x0, G, 1, first_parity=fp)
        smp = _sampler(la, kind, nodes=nodes)
        out = smp.run_exchange(STEPS, x0, temperature=temps, replicas=G, first_parity=fp)
        _assert_same(out, ref, smp, ref_smp, f"nodes={nodes} first_parity={fp}")
        assert out["swapped"].sum() == STEPS * (B // G)              # one pair per group and round, each certain


@pytest.mark.parametrize("nodes,B", [(50, 4092), (10, 8190)])
def test_the_form_at_the_batch_sizes_where_the_packed_waves_would_pick_another(la, nodes, B):
    """Groups of 3: 4092 chains are 512 groups of 16 rows (the twin form's last batch size) in 682 packed wave pairs,
    8190 chains 1024 groups (the matrix-pipe form's last) in 1365 packed waves."""
    kind, G = "mog", 3
    assert math.ceil(2 * B / 16) in (512, 1024) and math.ceil(B / 6) > math.ceil(2 * B / 16)
    x0, temps = _x0(B, TOYS[kind][0]), _temps(B, G)
    ref_smp, smp = _sampler(la, kind, in_launch=False, nodes=nodes), _sampler(la, kind, nodes=nodes)
    ref = ref_smp.run_exchange(STEPS, x0, temperature=temps, replicas=G)
    out = smp.run_exchange(STEPS, x0, temperature=temps, replicas=G)
    _same_run(out, ref, smp, ref_smp, f"nodes={nodes} B={B}")
    assert out["swapped"].sum() > 0


# ----------------------------------------------------------------- 3. a run continues
@pytest.mark.parametrize("kind,B,G", [("mog", 72, 3), ("gmm5", 8, 4), ("rw", 72, 2)])
def test_two_halves_are_the_whole(la, kind, B, G):
    x0, temps = _x0(B, TOYS[kind][0]), _temps(B, G)
    for k, n in ((1, 3), (2, 6), (5, 5)):
        for fp in (0, 1):
            whole_smp, smp = _sampler(la, kind), _sampler(la, kind, spl=4)
            whole = whole_smp.run_exchange(2 * n, x0, temperature=temps, replicas=G, swap_every=k, first_parity=fp)
            a = smp.run_exchange(n, x0, temperature=temps, replicas=G, swap_every=k, first_parity=fp)
            b = smp.run_exchange(n, a["samples_out"], temperature=temps, replicas=G, swap_every=k,
                                 first_parity=(fp + n // k) % 2, replica0=a["replica"][-1])
            both = {key: np.concatenate([a[key], b[key]]) for key in HIST + ("samples",) + ROUNDS}
            both["samples_out"] = b["samples_out"]
            _assert_same(whole, both, whole_smp, smp, f"{kind} G={G} swap_every={k} first_parity={fp}")


# ----------------------------------------------------------------- 4. launches
@pytest.mark.parametrize("kind,B,G", [("mog", 72, 2), ("mog", 72, 4), ("gmm5", 15, 5), ("rw", 72, 3)])
def test_one_launch_per_chunk_and_no_launch_per_round(la, kind, B, G):
    """Class 7: the toy-target run kernels, class 8: a round on its own."""
    x, n, temps = _x0(B, TOYS[kind][0]), STEPS, _temps(B, G)
    for k in (1, 5):
        for spl in (256, 3, 7):
            smp = _sampler(la, kind, spl)
            run = lambda: smp.run_exchange(n, x, temperature=temps, replicas=G, swap_every=k, first_parity=1)
            run()                                                    # warm-up
            assert count_launches(7, run) == math.ceil(n / spl), (G, k, spl)
            assert count_launches(8, run) == 0, (G, k, spl)


def test_the_entry_is_captured_as_one_kernel_node_and_replays_the_eager_bits(la):
    """No workspace, no host synchronisation, no second launch: one kernel node, rounds included."""
    import ctypes as C
    from l2hmc_amd import _lib
    from tests.test_gpu_small_run import _graph_shape, _hip
    L, n, B, G = _lib.lib(), 5, 66, 3
    smp = _sampler(la, "mog")                        # (kept: the plan points into its dynamics' tensors)
    plan = smp.dynamics._plan()
    x0 = _x0(B, 2)
    temps = torch.as_tensor(_temps(B, G)[0], dtype=torch.float32, device="cuda")
    label0 = torch.arange(B, dtype=torch.int32, device="cuda")
    out = dict(px=torch.empty(n, B, device="cuda"), samples=torch.empty(n, B, 2, device="cuda"),
               swap_p=torch.empty(n, B, device="cuda"), swapped=torch.empty(n, B, dtype=torch.uint8, device="cuda"),
               hist=torch.empty(n, B, dtype=torch.int32, device="cuda"), replica=label0.clone())

    def run(x_in, x_next):
        _lib.check(L.l2hmc_small_run_exchange(
            C.byref(plan), x_in.data_ptr(), x_next.data_ptr(), B, 77, 5, n, temps.data_ptr(), 0, 1, G, 1, 0, 1,
            out["replica"].data_ptr(), out["px"].data_ptr(), out["samples"].data_ptr(), out["swap_p"].data_ptr(),
            out["swapped"].data_ptr(), out["hist"].data_ptr(), _lib.stream_ptr()))
    eager = torch.empty_like(x0)
    run(x0, eager)
    torch.cuda.synchronize()
    want = {k: v.clone() for k, v in out.items()}
    assert want["swapped"].sum() > 0 and torch.equal(want["replica"], want["hist"][-1])
    hip = _hip()
    xin, xg = x0.clone(), torch.empty_like(x0)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            before = _graph_shape(hip, side.cuda_stream)
            run(xin, xg)
            after = _graph_shape(hip, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    assert before == (0, 0, 0) and after == (1, 0, 0), (before, after)
    for _ in range(2):
        for v in out.values():
            v.zero_()
        out["replica"].copy_(label0)
        xin.copy_(x0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(xg, eager)
        for k, v in out.items():
            assert torch.equal(v.view(torch.uint8), want[k].view(torch.uint8)), k        # (bytes: swap_p holds NaNs)


# ----------------------------------------------------------------- 5. labels and rates
@pytest.mark.parametrize("kind,B,G", [("mog", 72, 3), ("gmm5", 16, 8), ("rw", 72, 8), ("mog", 3, 3)])
def test_labels_are_permutations_and_the_rate_is_the_mean(la, kind, B, G):
    smp = _sampler(la, kind)
    start = np.arange(B, dtype=np.int32).reshape(-1, G)[:, ::-1].reshape(-1).copy()       # every group reversed
    out = smp.run_exchange(STEPS, _x0(B, TOYS[kind][0]), temperature=_temps(B, G), replicas=G, replica0=start)
    rep, sw = out["replica"], out["swapped"]
    assert rep.shape == (STEPS, B)
    prev = start
    for t in range(STEPS):
        assert np.array_equal(np.sort(rep[t].reshape(-1, G), axis=1), np.arange(B).reshape(-1, G)), t
        low = lower_chains(B, G, t % 2)
        lower = np.zeros(B, dtype=bool)
        lower[low] = True
        assert not sw[t][~lower].any() and np.isnan(out["swap_p"][t][~lower]).all()
        assert np.isfinite(out["swap_p"][t][lower]).all()
        perm = np.arange(B)
        a = low[sw[t][low]]
        perm[a], perm[a + 1] = a + 1, a
        assert np.array_equal(rep[t], prev[perm]), t
        prev = rep[t]
    assert out["swap_rate"].shape == (G - 1,)
    assert np.array_equal(out["swap_rate"], sw.reshape(STEPS, B // G, G)[:, :, :G - 1].mean(axis=(0, 1)))
    assert sw.any()


# ----------------------------------------------------------------- 6. the target stays invariant
def test_exchange_run_leaves_every_rung_invariant(la):
    t0 = time.time()
    G = len(TR.LADDER)
    x0, temps, exact = TR.ladder_start()
    state = np.random.get_state()
    with torch.random.fork_rng(devices=[]):          # the weights as built, the same ones in every run of the suite
        torch.manual_seed(5)
        np.random.seed(5)
        dyn = la.Dynamics(2, la.Gaussian(TR.MU, TR.COV).get_energy_function(), trajectory_length=TR.HMC_N,
                          eps=TR.HMC_EPS, use_temperature=True, seed=5,
                          net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=10))
    np.random.set_state(state)
    assert not dyn.hmc and not dyn.layered
    smp = la.DynamicsSampler(dyn)
    smp.in_launch = True
    x = torch.as_tensor(x0, dtype=torch.float32, device="cuda")
    zs, done, labels, rate, acc = [], 0, None, [], []
    for cp in TR.CHECKPOINTS:                                        # the run, continued from checkpoint to checkpoint
        run = lambda: smp.run_exchange(cp - done, x, keep_samples=False, temperature=temps[None, :], replicas=G,
                                       swap_every=1, first_parity=done % 2, replica0=labels)
        out = run()
        x, labels, done = out["samples_out"], out["replica"][-1], cp
        rate.append(out["swapped"].sum() / np.isfinite(out["swap_p"]).sum())        # per proposed pair
        acc.append(out["px"].mean())
        zs.append(TR.rung_zscores(x, exact))
    m = _report("toy L2HMC + replica exchange in the launch", zs,
                f"accept {np.mean(acc):.3f}, exchanges per pair and round {np.mean(rate):.3f}, {time.time() - t0:.1f} s")
    assert np.mean(rate) > 0.1
    assert m < Z_PASS, zs
