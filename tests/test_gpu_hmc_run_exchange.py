"""Replica exchange INSIDE the launches of a plain-HMC ladder run: `GaugeSampler.run_hmc_exchange` with `sampler.in_launch = True`
and l2hmc_gauge_hmc_run_exchange (hmc_run_exchange_kernel, l2hmc_amd/csrc/hmc_step.hip).

The yardstick is the path that exists already and is held to the loop a caller would write and to the target in
tests/test_gpu_replica_exchange.py: `in_launch = False`, the round between launches, on a second sampler of the same
seed.  Every comparison with it is an equality, at every served shape class of tests/test_hmc_run_exchange_host.py, at a
batch that fills the last workgroup and at one that does not.  N_LF 3 and 12 steps, as there."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.run_cases import count_launches

pytestmark = pytest.mark.gpu

N_LF, EPS, STEPS = 3, 0.1, 12
HIST = ("px", "actions", "plaqs", "charges", "charge_diff")
ROUNDS = ("swap_p", "swapped", "replica")
EPSS = (0.05, 0.1, 0.2)
# (T, X, B, G, both).  Chains per workgroup of the exchange run = lcm(G, chains per workgroup of the ladder run):
# 8x8 both 2 -> 6 at G = 3 (B = 72 fills 12 workgroups, B = 9 leaves the second half filled), 8 at G = 8;
# 3x5 both 8; 6x6 both 6; 8x16 both 1 -> 2, 4; 16x16 and 16x32 both 1 -> 2; selected-only twice as many
CASES = [(8, 8, 72, 3, True), (8, 8, 9, 3, True), (8, 8, 24, 8, True), (8, 8, 72, 2, True), (8, 8, 72, 4, True),
         (3, 5, 8, 4, True), (3, 5, 12, 4, True), (6, 6, 9, 3, True), (6, 6, 12, 3, True), (8, 16, 6, 2, True),
         (8, 16, 8, 4, True), (16, 16, 6, 2, True), (16, 32, 4, 2, True),
         (8, 8, 72, 3, False), (8, 8, 9, 3, False), (8, 8, 24, 8, False), (8, 8, 32, 16, False), (8, 8, 6, 2, False),
         (8, 8, 72, 4, False), (8, 8, 8, 4, False),
         (3, 5, 8, 4, False), (3, 5, 32, 4, False), (16, 16, 8, 4, False), (16, 16, 6, 2, False), (16, 32, 4, 4, False)]


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _sampler(la, T, X, B, both=True, spl=256, draws=4, in_launch=False):
    orc = H.gauge_oracle(T, X, N_LF, EPS, None, None, hmc=True)
    dyn = H.gauge_hip(T, X, N_LF, EPS, None, None, orc.mask, B, hmc=True, both_directions=both)
    dyn._draws = draws
    smp = la.GaugeSampler(dyn)
    smp.steps_per_launch = spl
    smp.in_launch = in_launch
    return smp


def _x0(T, X, B):
    torch.manual_seed(1234)
    return torch.rand(B, 2 * T * X, device="cuda") * (2 * np.pi)


def _betas(B, G, n=None):
    """[1, B] ladder from 1 to 4 over the rungs of every group, or [n, B]: the ladder scaled a little from step to step"""
    lad = np.tile(np.linspace(1.0, 4.0, G), B // G)[None, :]
    return lad if n is None else lad * (1.0 + 0.02 * np.arange(n))[:, None]


def _assert_same(a, b, sa, sb, what):
    for key in HIST + ("samples",) + ROUNDS:
        assert a[key].shape == b[key].shape and a[key].dtype == b[key].dtype, (what, key)
        assert np.array_equal(a[key], b[key], equal_nan=(key == "swap_p")), (what, key)
    assert np.array_equal(a["swap_rate"], b["swap_rate"], equal_nan=True), what
    assert torch.equal(a["samples_out"], b["samples_out"]), what
    assert a["mean_accept"] == b["mean_accept"], what
    assert torch.equal(sa.stats.total, sb.stats.total), what
    assert sa.dynamics._draws == sb.dynamics._draws, what
    assert torch.equal(sa.replica, sb.replica), what


# ----------------------------------------------------------------- 1. the run is the run with the round between launches
@pytest.mark.parametrize("T,X,B,G,both", CASES)
def test_in_launch_is_between_launches(la, T, X, B, G, both):
    x0 = _x0(T, X, B)
    keep = x0.clone()
    eps = np.array(EPSS)[np.arange(B) % 3]
    assert _sampler(la, T, X, B, both).exchange_in_launch(G) is True
    exchanged, mixed = 0, False
    for k in (1, 5):
        beta = _betas(B, G) if k == 1 else _betas(B, G, STEPS)           # a ladder; a ladder with a schedule
        for fp in (0, 1):
            ref_smp = _sampler(la, T, X, B, both)
            ref = ref_smp.run_hmc_exchange(STEPS, beta, x0, eps=eps, keep_samples=True, replicas=G, swap_every=k,
                                           first_parity=fp)
            # steps_per_launch = 5 at swap_every = 5: every chunk ends on a round; at 1: a round after every step of
            # every chunk; 12 steps in chunks of 5 at swap_every = 5 end between rounds.  256: one launch
            for spl in (256, 5):
                what = f"{T}x{X} B={B} both={both} G={G} swap_every={k} first_parity={fp} steps_per_launch={spl}"
                smp = _sampler(la, T, X, B, both, spl, in_launch=True)
                got = {}

                def run():
                    got["out"] = smp.run_hmc_exchange(STEPS, beta, x0, eps=eps, keep_samples=True, replicas=G,
                                                      swap_every=k, first_parity=fp)
                # the path taken is the in-launch one: no launch of the round on its own (the reference makes some)
                assert count_launches(8, run) == 0, what
                out = got["out"]
                assert out["swap_p"].shape == (STEPS // k, B) and out["swap_p"].dtype == np.float32, what
                assert out["swapped"].dtype == np.bool_ and out["replica"].dtype == np.int32, what
                _assert_same(out, ref, smp, ref_smp, what)
                assert np.array_equal(smp.replica.cpu().numpy(), out["replica"][-1]), what
            exchanged += int(ref["swapped"].sum())
            proposed = np.isfinite(ref["swap_p"])
            mixed = mixed or any((ref["swapped"][t] & proposed[t]).any() and (~ref["swapped"][t] & proposed[t]).any()
                                 for t in range(STEPS // k))
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    print(f"\n[exchange] {T}x{X} B={B} G={G} both={both}: {exchanged} exchanges, a round with both outcomes: {mixed}")
    if B >= 72:                                                      # 18 groups or more: pairs enough for both outcomes
        assert exchanged > 0 and mixed


@pytest.mark.parametrize("both", [True, False])
def test_chunks_start_at_every_phase(la, both):
    """swap_every = 3 in chunks of 5 and 7 steps: chunks start at phases 0, 2, 1 (and 0, 1), end on and between rounds."""
    T, X, B, G = 8, 8, 72, 3
    x0, beta = _x0(T, X, B), _betas(B, G, STEPS)
    ref_smp = _sampler(la, T, X, B, both)
    ref = ref_smp.run_hmc_exchange(STEPS, beta, x0, keep_samples=True, replicas=G, swap_every=3, first_parity=1)
    for spl in (5, 7, 1):
        smp = _sampler(la, T, X, B, both, spl, in_launch=True)
        out = smp.run_hmc_exchange(STEPS, beta, x0, keep_samples=True, replicas=G, swap_every=3, first_parity=1)
        _assert_same(out, ref, smp, ref_smp, f"both={both} steps_per_launch={spl}")


# ----------------------------------------------------------------- 2. a run continues
@pytest.mark.parametrize("T,X,B,G", [(3, 5, 8, 4), (8, 8, 72, 3), (16, 16, 6, 2)])
def test_two_halves_are_the_whole(la, T, X, B, G):
    x0, beta = _x0(T, X, B), _betas(B, G)
    for k, n in ((1, 3), (2, 6), (5, 5)):
        for fp in (0, 1):
            whole_smp, smp = _sampler(la, T, X, B, in_launch=True), _sampler(la, T, X, B, in_launch=True)
            whole = whole_smp.run_hmc_exchange(2 * n, beta, x0, keep_samples=True, replicas=G, swap_every=k,
                                               first_parity=fp)
            a = smp.run_hmc_exchange(n, beta, x0, keep_samples=True, replicas=G, swap_every=k, first_parity=fp)
            b = smp.run_hmc_exchange(n, beta, a["samples_out"], keep_samples=True, replicas=G, swap_every=k,
                                     first_parity=(fp + n // k) % 2, replica0=a["replica"][-1])
            what = f"{T}x{X} G={G} swap_every={k} first_parity={fp}"
            for key in HIST + ("samples",) + ROUNDS:
                both = np.concatenate([a[key], b[key]])
                assert np.array_equal(whole[key], both, equal_nan=(key == "swap_p")), (what, key)
            assert torch.equal(whole["samples_out"], b["samples_out"]), what
            assert whole["mean_accept"] == b["mean_accept"], what
            assert torch.equal(whole_smp.stats.total, smp.stats.total), what
            assert whole_smp.dynamics._draws == smp.dynamics._draws, what
            assert torch.equal(whole_smp.replica, smp.replica), what


# ----------------------------------------------------------------- 3. launches
def test_one_launch_per_chunk_and_none_per_round(la):
    """Class 5: the run kernel, class 8: the round on its own.  G = 2 at first_parity 1: every other round is pairless."""
    T, X, B, n = 8, 8, 72, STEPS
    x = _x0(T, X, B)
    for G in (2, 4):
        beta = _betas(B, G)
        for k in (1, 5):
            for spl in (256, 5):
                smp = _sampler(la, T, X, B, spl=spl, in_launch=True)
                run = lambda: smp.run_hmc_exchange(n, beta, x, replicas=G, swap_every=k, first_parity=1)
                run()                                                # warm-up
                assert count_launches(5, run) == math.ceil(n / spl), (G, k, spl)
                assert count_launches(8, run) == 0, (G, k, spl)
                assert count_launches(4, run) == 0


# ----------------------------------------------------------------- 4. the entry on its own
def _entry(la, plan, betas, x_in, x_next, B, n, G, k, phase, fp, replica, hist, sums, samples, rounds, ws, draw0=9):
    from l2hmc_amd import _lib
    nb = 0 if ws is None else ws.numel()
    _lib.call("l2hmc_gauge_hmc_run_exchange", C.byref(plan), betas, 0, 1, None, x_in, x_next, B, 42, draw0, n, G, k,
              phase, fp, replica, *hist, sums, samples, *rounds, ws, nb)


def test_entry_optional_outputs_aliasing_tickets_and_graph(la):
    from l2hmc_amd import _lib
    T, X, B, G, n, k = 8, 8, 24, 8, 7, 2
    D = 2 * T * X
    smp = _sampler(la, T, X, B)
    plan, L = smp.dynamics._plan(), _lib.lib()
    x0 = _x0(T, X, B)
    betas = torch.tensor(_betas(B, G)[0], dtype=torch.float32, device="cuda")
    n_r = (1 + n) // k                                               # swap_phase 1: rounds after steps 0, 2, 4, 6
    ws = torch.empty(L.l2hmc_gauge_hmc_run_exchange_ws_bytes(C.byref(plan), B, n), dtype=torch.uint8, device="cuda")

    def full():
        o = {"hist": [torch.zeros(n, B, device="cuda") for _ in HIST], "sums": torch.zeros(n, 4, device="cuda"),
             "samples": torch.zeros(n, B, D, device="cuda"),
             "rounds": [torch.zeros(n_r, B, device="cuda"), torch.zeros(n_r, B, dtype=torch.uint8, device="cuda"),
                        torch.zeros(n_r, B, dtype=torch.int32, device="cuda")],
             "replica": torch.arange(B, dtype=torch.int32, device="cuda"), "x": torch.empty_like(x0)}
        return o

    def call(o, x_in, x_next):
        _entry(la, plan, betas, x_in, x_next, B, n, G, k, 1, 1, o["replica"], o["hist"], o["sums"], o["samples"],
               o["rounds"], ws)

    a, b = full(), full()
    call(a, x0, a["x"])
    call(b, x0, b["x"])                                              # two calls give the same bits
    torch.cuda.synchronize()
    flat = lambda o: [o["x"], *o["hist"], o["sums"], o["samples"], *o["rounds"][1:], o["replica"]]
    for u, v in zip(flat(a), flat(b)):
        assert torch.equal(u, v)
    assert torch.equal(a["rounds"][0].isnan(), b["rounds"][0].isnan())
    assert torch.equal(a["rounds"][0].nan_to_num(-1.), b["rounds"][0].nan_to_num(-1.))
    assert a["rounds"][1].sum() > 0 and torch.equal(a["rounds"][2][-1], a["replica"])
    assert (a["sums"][:, 3] == 0).all() and (a["sums"][:, 2] == B).all()       # tickets left at 0
    assert torch.equal(a["samples"][-1].ne(a["x"]).any(dim=1), a["rounds"][2][-1].ne(
        a["rounds"][2][-2] if n_r > 1 else torch.arange(B, device="cuda")))     # samples[s]: BEFORE step s's round
    # x_next aliasing x_in
    c = full()
    c["x"].copy_(x0)
    call(c, c["x"], c["x"])
    torch.cuda.synchronize()
    for u, v in zip(flat(a), flat(c)):
        assert torch.equal(u, v)
    # every optional output NULL: the state alone, the same bits
    xn = torch.empty_like(x0)
    _entry(la, plan, betas, x0, xn, B, n, G, k, 1, 1, None, [None] * 5, None, None, [None] * 3, None)
    torch.cuda.synchronize()
    assert torch.equal(xn, a["x"])
    # captured into a graph and replayed
    g_out = full()
    xin = x0.clone()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            call(g_out, xin, g_out["x"])
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        g_out["x"].zero_(), g_out["samples"].zero_(), g_out["replica"].copy_(torch.arange(B, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(flat(a), flat(g_out)):
            assert torch.equal(u, v)


# ----------------------------------------------------------------- 5. not served
@pytest.mark.parametrize("T,X,B,G", [(8, 8, 16, 16), (32, 32, 4, 2)])
def test_unserved_raises_without_a_launch(la, T, X, B, G):
    smp = _sampler(la, T, X, B, in_launch=True)
    assert smp.exchange_in_launch(G) is False
    x0, beta = _x0(T, X, B), _betas(B, G)

    def run():
        with pytest.raises(NotImplementedError, match="exceed 1024"):
            smp.run_hmc_exchange(STEPS, beta, x0, replicas=G)
    assert count_launches(5, run) == 0 and count_launches(8, run) == 0
    assert smp.dynamics._draws == 4 and smp.replica is None
    smp.in_launch = False
    out = smp.run_hmc_exchange(STEPS, beta, x0, replicas=G)           # the round between launches takes it
    assert out["swap_p"].shape == (STEPS, B)
