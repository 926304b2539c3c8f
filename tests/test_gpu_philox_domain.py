"""Every Philox generator of the library at 64-bit seeds and stream indices.

The counter {block_lo, block_hi, stream_lo, stream_hi} and the key {seed_lo, seed_hi} are put together by hand in
fill_kernel (capi.hip), step_draws_kernel (mcmc_step.hip), stage_chains / philox_u01 (fused_step.h), the staging code of
hmc_step.hip, gauge_swap.h / replica_swap.hip, philox_block_at (small_mlp.h) and its callers, small_hmc.hip and
small_swap.h; three of them also form 2 * draw and 2 * draw + 1 on the device.  The rest of the suite runs them at seeds
below 2^32 and draw indices below 100, where both high words are 0.  Here they run at the corners of
tests/philox_cases.py, whose power to tell a dropped word from a kept one tests/test_philox_domain_host.py shows:

  a. the fill entries against the integer / float64 reference of tests/philox_ref.py;
  b. every in-kernel generator against the float64 oracle fed the fill entries' buffers of the same (seed, stream)
     (the pattern, tolerances and exclusion rule of test_native_mcmc_step_matches_oracle_on_its_own_draws and
     test_hmc_step_matches_oracle_on_its_own_draws);
  c. the index arithmetic of the runs: the equalities the suite holds at small draws, at the run corners;
  d. sensitivity with no reference: the outputs at (seed, draw) differ from those at each truncated twin;
  e. the Python samplers on a counter beyond 2^32.

Not covered: block indices of 2^32 or more (block_hi) would need more than 2^34 elements in one stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import lattice as olat
from tests import helpers as H
from tests import philox_cases as PC
from tests import philox_ref as R

pytestmark = pytest.mark.gpu

TOL_OP, TOL_P = 1e-5, 2e-5          # tests/test_gpu_parity.py
HIST = ("px", "actions", "plaqs", "charges", "charge_diff")
SEED = PC.SEED_HIGH


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def circle(a, b):
    d = np.mod(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)), 2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _fill(kind, n, seed, stream, unaligned=False):
    """l2hmc_fill_uniform / _normal into a fresh buffer; `unaligned`: into a view one float past a 16-byte boundary."""
    from l2hmc_amd import _lib
    buf = torch.full((n + 4,), float("nan"), device="cuda")
    out = buf[1:n + 1] if unaligned else buf[:n]
    assert out.data_ptr() % 16 == (4 if unaligned else 0)
    _lib.check(getattr(_lib.lib(), "l2hmc_fill_" + kind)(out.data_ptr(), n, seed, stream, None))
    torch.cuda.synchronize()
    assert torch.isnan(buf[n + 1 if unaligned else n:]).all() and (not unaligned or torch.isnan(buf[0]))
    return out.clone()


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")


# ================================================================= a. the fill entries
@pytest.mark.parametrize("stream", PC.FILL_STREAMS, ids=hex)
@pytest.mark.parametrize("seed", PC.SEEDS, ids=hex)
def test_fill_uniform_is_the_integer_reference_bit_for_bit(la, seed, stream):
    """Every element of 4099 (a ragged last block), through the float4 stores and, on an output that is not 16-byte
    aligned, through the scalar stores."""
    n = PC.FILL_N
    want = R.uniforms(seed, stream, n)
    for unaligned in (False, True):
        got = _fill("uniform", n, seed, stream, unaligned).cpu().numpy()
        assert got.dtype == want.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hex(seed), hex(stream), unaligned)


_NORMAL_MAX = {}


@pytest.mark.parametrize("stream", PC.FILL_STREAMS, ids=hex)
@pytest.mark.parametrize("seed", PC.SEEDS, ids=hex)
def test_fill_normal_matches_the_float64_reference(la, seed, stream):
    """Box-Muller in float64 on the device's own float32 uniforms (tests/philox_ref.normal) against l2hmc_fill_normal.
    The bound is derived: |z| <= 5.9 since u1 >= 2^-25; the angle is off by <= 2.4e-7 (the fp32 product 2 pi u2) +
    1.8e-7 (2 pi in fp32) + about 1e-7 (fast_sincos); the radius by about 2e-7 relative (logf, sqrtf, the product);
    5.9 * (5.2e-7 + 2e-7) is below 5e-6.  Asserted: < 1e-5.
    Measured on the MI355X: 1.402e-06 at the worst of the 15 corners (9.1e-07 .. 1.4e-06 over them, max |z| 3.4 .. 4.4
    in 4099 draws); aligned and unaligned outputs hold the same bits."""
    n = PC.FILL_N
    want = R.normals(seed, stream, n)
    got = _fill("normal", n, seed, stream)
    odd = _fill("normal", n, seed, stream, unaligned=True)
    assert torch.equal(got.view(torch.int32), odd.view(torch.int32))        # aligned and unaligned: the same bits
    err = float(np.abs(np_(got) - want).max())
    _NORMAL_MAX[(seed, stream)] = err
    print(f"fill_normal seed={seed:#x} stream={stream:#x}: max |device - float64| = {err:.3e}, max |z| = "
          f"{np.abs(want).max():.3f}; largest over {len(_NORMAL_MAX)} corners so far {max(_NORMAL_MAX.values()):.3e}")
    assert np.isfinite(np_(got)).all()
    assert err < 1e-5


# ================================================================= b. the in-kernel generators against the fill entries
def _lattice_dyn(c):
    orc = PC.lattice_oracle(c)
    xp, vp = PC.lattice_weights(c.arch, c.T, c.X)
    dyn = H.gauge_hip(c.T, c.X, PC.N_LF, PC.EPS, xp, vp, orc.mask, c.B, hmc=c.hmc, both_directions=c.both,
                      arch=c.arch or "generic")
    if c.layered:
        dyn.fused = False
    return orc, dyn


def _step(dyn, x0, seed, draw, betas=None, beta=PC.BETA):
    """l2hmc_gauge_mcmc_step_ex (or _ladder with `betas` [B]) from x0 -> dict of x_next, the five outputs, step_sums."""
    from l2hmc_amd import _lib
    B = x0.shape[0]
    plan, Lh = dyn._plan(), _lib.lib()
    nb = Lh.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws = _ws(nb)
    out = {k: torch.empty(B, device="cuda") for k in HIST}
    out["x_next"], out["sums"] = torch.empty_like(x0), torch.zeros(4, device="cuda")
    tail = ([out[k] for k in HIST], out["sums"], ws, nb)
    if betas is None:
        _lib.call("l2hmc_gauge_mcmc_step_ex", C.byref(plan), beta, x0, out["x_next"], B, seed, draw, *tail[0], *tail[1:])
    else:
        _lib.call("l2hmc_gauge_mcmc_step_ladder", C.byref(plan), betas, 1, x0, out["x_next"], B, seed, draw, *tail[0],
                  *tail[1:])
    torch.cuda.synchronize()
    return out


def _transition_draw(dyn, x0, seed, draw, beta=PC.BETA):
    from l2hmc_amd import _lib
    B = x0.shape[0]
    plan, Lh = dyn._plan(), _lib.lib()
    nb = Lh.l2hmc_gauge_mcmc_step_ws_bytes(C.byref(plan), B)
    ws = _ws(nb)
    outs = [torch.empty_like(x0), torch.empty_like(x0), torch.empty(B, device="cuda"), torch.empty_like(x0)]
    _lib.call("l2hmc_gauge_transition_draw", C.byref(plan), beta, x0, B, seed, draw, *outs, ws, nb)
    torch.cuda.synchronize()
    return outs


def _fill_step_draws(seed, draw, B, D):
    sv, su = R.lattice_step_streams(draw)
    V = np_(_fill("normal", 2 * B * D, seed, sv)).reshape(2 * B, D)
    cu = np_(_fill("uniform", 2 * B, seed, su))
    return V[:B], V[B:], cu[:B], cu[B:]


@pytest.mark.parametrize("case", PC.LATTICE_CASES, ids=lambda c: c.name)
def test_lattice_generators_match_the_oracle_on_the_fill_entries_draws(la, case):
    """The step (or l2hmc_gauge_transition_draw) draws for itself at (2^64 - 59, draw); the float64 oracle is fed what
    l2hmc_fill_normal(seed, 2 draw) and l2hmc_fill_uniform(seed, 2 draw + 1) write.  A generator that drops or
    misplaces a word integrates other momenta and misses by O(1)."""
    from l2hmc_amd import _lib
    c = case
    T, X, B, D = c.T, c.X, c.B, 2 * c.T * c.X
    orc, dyn = _lattice_dyn(c)
    plan = dyn._plan()
    fused = _lib.lib().l2hmc_gauge_plan_fused(C.byref(plan))
    assert bool(plan.flags & _lib.PLAN_LAYERED) == c.layered
    assert bool(plan.flags & _lib.PLAN_SELECTED_ONLY) == (not c.both)
    assert fused == (0 if c.layered or "step-draws" in c.name else 1), c.name      # the generator the case is named for
    x0 = PC.lattice_x0(c)
    x64 = x0.astype(np.float64)
    xd = torch.as_tensor(x0, device="cuda")
    for draw in PC.STEP_DRAWS:
        vf, vb, coin, u = _fill_step_draws(SEED, draw, B, D)
        want = orc.apply_transition(x64, PC.BETA, vf, vb, coin, u)
        safe = np.abs(want[2] - u) > PC.MARGIN_GPU
        if c.entry == "draw":
            got = [np_(g) for g in _transition_draw(dyn, xd, SEED, draw)]
            figs = dict(x_prop=H.relerr(got[0], want[0]), v_prop=H.relerr(got[1], want[1]),
                        px=np.abs(got[2] - want[2]).max(), x_out=H.relerr(got[3][safe], want[3][safe]),
                        excluded=int((~safe).sum()), accepted=int((want[2] > u).sum()))
            print(f"philox domain {c.name} draw={draw:#x}: {figs}")
            assert figs["excluded"] <= PC.excluded_cap(B)
            # test_dynamics_call_with_library_draws_matches_oracle's bars
            assert figs["x_prop"] < 2 * TOL_OP and figs["v_prop"] < 2 * TOL_OP and figs["px"] < TOL_P
            assert figs["x_out"] < 2 * TOL_OP
            continue
        o = _step(dyn, xd, SEED, draw)
        px, actions, plaqs, charges, dq = (np_(o[k]) for k in HIST)
        got = np_(o["x_next"])
        figs = dict(px=np.abs(px - want[2]).max(), action=H.relerr(actions, olat.total_action(x64, T, X)),
                    plaq=H.relerr(plaqs, olat.avg_plaq(x64, T, X)), charge=H.relerr(charges, olat.top_charge(x64, T, X)),
                    dq=H.relerr(dq[safe], olat.top_charge_diff(x64, want[3], T, X)[safe]),
                    x_next=circle(got, np.mod(want[3], 2 * np.pi))[safe].max(), excluded=int((~safe).sum()),
                    accepted=int((want[2] > u).sum()))
        print(f"philox domain {c.name} draw={draw:#x}: {figs}")
        assert figs["excluded"] <= PC.excluded_cap(B)
        assert figs["px"] < TOL_P
        assert figs["action"] < TOL_OP and figs["plaq"] < TOL_OP and figs["charge"] < 1e-4
        assert figs["dq"] < 1e-3
        assert figs["x_next"] < 5e-5
        assert got.min() >= 0 and got.max() < 2 * np.pi + 1e-6
        assert o["sums"][3].view(torch.int32).item() == 0 and o["sums"][2].item() == B


def test_ladder_instance_with_equal_betas_is_the_uniform_step(la):
    """The LADDER instance of the whole-step kernel stages its chains with the same code: bit for bit
    l2hmc_gauge_mcmc_step_ex, at the draw whose streams carry into the high word."""
    c = next(k for k in PC.LATTICE_CASES if k.name == "generic-8x8-transition-draw")
    _, dyn = _lattice_dyn(c)
    xd = torch.as_tensor(PC.lattice_x0(c), device="cuda")
    betas = torch.full((c.B,), PC.BETA, device="cuda")
    a, b = _step(dyn, xd, SEED, 2 ** 31), _step(dyn, xd, SEED, 2 ** 31, betas=betas)
    for k in HIST + ("x_next", "sums"):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["x_next"], xd)


# ----------------------------------------------------------------- toy targets
def _toy_oracle(kind):
    """The float64 DynamicsOracle of tests/test_gpu_small_run.py::_toy(kind): same target, nets, masks, eps."""
    from oracle import dynamics as od
    from tests.test_gpu_small_run import GMM3, TOYS
    dim, N, nodes, temp = TOYS[kind]
    tgt = H.mog_target_oracle() if kind == "mog" else od.GMM(*GMM3)
    xp, vp = H.mlp_weights(dim, nodes, seed=106, regime="stress")
    assert temp == 1.0
    return tgt, od.DynamicsOracle(dim, tgt, N, 0.1, od.make_masks(N, dim, np.random.RandomState(3)), xp, vp)


def _propose(dyn, x, seed, draw0):
    from l2hmc_amd import _lib
    B = x.shape[0]
    plan = dyn._plan()
    Lx, Lv, px, xo = torch.empty_like(x), torch.empty_like(x), torch.empty(B, device="cuda"), torch.empty_like(x)
    _lib.call("l2hmc_small_propose", C.byref(plan), x, B, seed, draw0, Lx, Lv, px, xo)
    torch.cuda.synchronize()
    return Lx, Lv, px, xo


@pytest.mark.parametrize("draw0", PC.TOY_PROPOSE_DRAW0, ids=hex)
@pytest.mark.parametrize("kind", ["mog", "gmm3"])
def test_small_propose_matches_the_oracle_on_the_fill_entries_draws(la, kind, draw0):
    """philox_block_at and its callers: l2hmc_small_propose on its own four streams against the float64 oracle's
    `propose` fed the fill entries' buffers, compared as test_generic_dynamics_and_propose compares (TOL_OP on Lx and
    Lv, TOL_P on px, x_out where the decision is clear of its uniform by 1e-4), and against the piecewise path on the
    same buffers bit for bit.  x_dim 3: a chain's components straddle Philox blocks.  37 chains: a ragged last group."""
    from oracle import dynamics as od
    from tests.test_gpu_small_run import _toy
    B = 37
    tgt_o, orc = _toy_oracle(kind)
    dyn = _toy(la, kind)
    dim = dyn.x_dim
    x = tgt_o.get_samples(B, np.random.default_rng(8)).astype(np.float32)
    xd = torch.as_tensor(x, device="cuda")
    Lx, Lv, px, xo = _propose(dyn, xd, SEED, draw0)
    ub = _fill("uniform", B, SEED, draw0)
    vf = _fill("normal", B * dim, SEED, draw0 + 1).reshape(B, dim)
    vb = _fill("normal", B * dim, SEED, draw0 + 2).reshape(B, dim)
    u = _fill("uniform", B, SEED, draw0 + 3)
    bits = (ub >= 0.5).float()
    want = od.propose(x.astype(np.float64), orc, np_(vf), np_(vb), np_(bits), u=np_(u), do_mh_step=True)
    wLx, wpx, wout, wLv = want[0], want[2], want[3][0], want[4]
    safe = np.abs(wpx - np_(u)) > 1e-4
    figs = dict(Lx=H.relerr(np_(Lx), wLx), Lv=H.relerr(np_(Lv), wLv), px=np.abs(np_(px) - wpx).max(),
                x_out=H.relerr(np_(xo)[safe], wout[safe]), excluded=int((~safe).sum()),
                forward=int(np_(bits).sum()), accepted=int((wpx > np_(u)).sum()))
    print(f"philox domain small_propose {kind} draw0={draw0:#x}: {figs}")
    assert figs["excluded"] == 0 and 0 < figs["forward"] < B
    assert figs["Lx"] < TOL_OP and figs["Lv"] < TOL_OP and figs["px"] < TOL_P and figs["x_out"] < TOL_OP
    pLx, pLv, ppx, pouts = la.propose(xd, dyn, init_v=vf, do_mh_step=True, init_v_backward=vb, dir_bits=bits, u=u)
    assert torch.equal(pLx, Lx) and torch.equal(pLv, Lv) and torch.equal(ppx, px) and torch.equal(pouts[0], xo)


# ================================================================= c. the index arithmetic of the runs
def _hmc_dyn(T, X, B, both=True):
    orc = H.gauge_oracle(T, X, PC.N_LF, PC.EPS, None, None, hmc=True)
    return H.gauge_hip(T, X, PC.N_LF, PC.EPS, None, None, orc.mask, B, hmc=True, both_directions=both)


def _lattice_x(T, X, B):
    g = torch.Generator(device="cpu").manual_seed(1234)
    return (torch.rand(B, 2 * T * X, generator=g) * (2 * np.pi)).to("cuda")


def _hmc_run(dyn, x0, seed, draw0, n, ladder):
    """l2hmc_gauge_hmc_run (or _ladder at one beta per step and the plan's eps) with every output."""
    from l2hmc_amd import _lib
    B, D = x0.shape
    plan, Lh = dyn._plan(), _lib.lib()
    query = Lh.l2hmc_gauge_hmc_run_ladder_ws_bytes if ladder else Lh.l2hmc_gauge_hmc_run_ws_bytes
    nb = query(C.byref(plan), B, n)
    ws = _ws(nb)
    betas = torch.full((n,), PC.BETA, device="cuda")
    out = {k: torch.empty(n, B, device="cuda") for k in HIST}
    out.update(x_next=torch.empty_like(x0), sums=torch.zeros(n, 4, device="cuda"), samples=torch.empty(n, B, D, device="cuda"))
    tail = (*[out[k] for k in HIST], out["sums"], out["samples"], ws, nb)
    if ladder:
        _lib.call("l2hmc_gauge_hmc_run_ladder", C.byref(plan), betas, 1, 0, None, x0, out["x_next"], B, seed, draw0, n,
                  *tail)
    else:
        _lib.call("l2hmc_gauge_hmc_run", C.byref(plan), betas, x0, out["x_next"], B, seed, draw0, n, *tail)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ladder", [False, True], ids=["run", "ladder"])
@pytest.mark.parametrize("draw0", PC.RUN_DRAW0, ids=hex)
@pytest.mark.parametrize("T,X,B", [(4, 4, 9), (16, 32, 3)])
def test_lattice_runs_equal_their_steps_at_the_run_corners(la, T, X, B, draw0, ladder):
    """hmc_run_kernel adds the step index to the draw index and doubles it on the device: four steps that straddle the
    carry of 2 * draw into the high word, and the four that end on the last draw index the entries take (2^63 - 1, the
    first execution of the kernel's bit-63 path at its boundary), against four calls of l2hmc_gauge_mcmc_step_ex.
    Every history, samples and step_sums, bit for bit; the tickets are left at 0."""
    n = PC.RUN_STEPS
    dyn = _hmc_dyn(T, X, B)
    x0 = _lattice_x(T, X, B)
    run = _hmc_run(dyn, x0, SEED, draw0, n, ladder)
    x = x0
    for s in range(n):
        one = _step(dyn, x, SEED, draw0 + s)
        for k in HIST:
            assert torch.equal(run[k][s], one[k]), (k, s)
        assert torch.equal(run["samples"][s], one["x_next"]) and torch.equal(run["sums"][s], one["sums"]), s
        assert not torch.equal(one["x_next"], x)
        x = one["x_next"]
    assert torch.equal(run["x_next"], x)
    assert torch.all(run["sums"].view(torch.int32)[:, 3] == 0) and torch.all(run["sums"][:, 2] == B)


@pytest.mark.parametrize("draw0", PC.EXCHANGE_DRAW0, ids=hex)
def test_lattice_exchange_run_equals_the_loop_on_one_stream_counter(la, draw0):
    """l2hmc_gauge_hmc_run_exchange (rounds inside the launch) against launches of l2hmc_gauge_hmc_run_ladder with
    l2hmc_gauge_replica_swap between them: a step takes the pair (2 d, 2 d + 1), the round after it the stream 2 d + 2.
    8 x 8, groups of 4, a round after every second step; the second start ends on stream 2^64 - 2."""
    from l2hmc_amd import _lib
    from tests.test_gpu_hmc_run_exchange import _assert_same, _betas, _sampler, _x0
    T, X, B, G, n, k = 8, 8, 8, 4, PC.RUN_STEPS, PC.EXCHANGE_EVERY
    x0, beta = _x0(T, X, B), _betas(B, G)
    outs = []
    for in_launch in (True, False):
        smp = _sampler(la, T, X, B, draws=2 * draw0, in_launch=in_launch)
        smp.dynamics._seed = SEED
        assert smp.exchange_in_launch(G) is True
        outs.append((smp.run_hmc_exchange(n, beta, x0, keep_samples=True, replicas=G, swap_every=k), smp))
    (a, sa), (b, sb) = outs
    _assert_same(a, b, sa, sb, f"draw0={draw0:#x}")
    assert a["swap_p"].shape == (PC.EXCHANGE_ROUNDS, B)
    assert sa.dynamics._draws == _lib.exchange_run_draw_index(2 * draw0, n, k, 0)[2] == R.lattice_run_draws(
        draw0, n, k)[1][-1] + 1
    # the rounds' decisions are those of the reference uniforms of their streams
    for j, st in enumerate(R.lattice_run_draws(draw0, n, k)[1]):
        low = np.isfinite(a["swap_p"][j])
        u = R.uniform(SEED, st, np.arange(B))
        assert low.sum() == B // G * len(range(j % 2, G - 1, 2))
        assert np.array_equal(a["swapped"][j][low], a["swap_p"][j][low] > u[low]), j


def _small_run(dyn, x0, seed, draw0, n, temps=None):
    from l2hmc_amd import _lib
    B, D = x0.shape
    plan = dyn._plan()
    px, samples, xn = torch.empty(n, B, device="cuda"), torch.empty(n, B, D, device="cuda"), torch.empty_like(x0)
    if temps is None:
        _lib.call("l2hmc_small_run", C.byref(plan), x0, xn, B, seed, draw0, n, px, samples)
    else:
        _lib.call("l2hmc_small_run_tempered", C.byref(plan), x0, xn, B, seed, draw0, n, temps, 0, 1, px, samples)
    torch.cuda.synchronize()
    return px, samples, xn


@pytest.mark.parametrize("tempered", [False, True], ids=["run", "tempered"])
@pytest.mark.parametrize("draw0,n", PC.TOY_RUN, ids=lambda v: hex(v) if v > 99 else str(v))
@pytest.mark.parametrize("kind", ["mog", "gmm3"])
def test_toy_runs_equal_chained_proposes_at_the_run_corners(la, kind, draw0, n, tempered):
    """The RUN and TEMPERED instances add 4 s to draw0 on the device: three steps whose twelve streams straddle 2^32,
    and the three that end at l2hmc_small_run's own limit, against l2hmc_small_propose at draw0 + 4 s chained through
    x_out.  (Tempered: a ladder whose entries all equal the plan's temperature, which has the bits of l2hmc_small_run.)"""
    from tests.test_gpu_small_run import _toy, _x0
    B = 37
    dyn = _toy(la, kind)
    x0 = _x0(B, dyn.x_dim)
    temps = torch.full((B,), float(dyn.temperature), device="cuda") if tempered else None
    px, samples, xn = _small_run(dyn, x0, SEED, draw0, n, temps)
    x = x0
    for s in range(n):
        _, _, p, xo = _propose(dyn, x, SEED, draw0 + 4 * s)
        assert torch.equal(p, px[s]) and torch.equal(xo, samples[s]), s
        x = xo
    assert torch.equal(x, xn)
    moved = (samples[0] != x0).any(dim=1)
    assert moved.any() and not moved.all()                            # accepts and rejects: px and u both matter


@pytest.mark.parametrize("draw0,n", PC.TOY_HMC_RUN, ids=lambda v: hex(v) if v > 99 else str(v))
@pytest.mark.parametrize("kind", ["mog", "gmm3"])
def test_toy_hmc_run_equals_the_loop_at_the_run_corners(la, kind, draw0, n):
    """small_hmc_run_kernel (momenta on stream draw0 + 2 s, uniforms on the next) against the loop over `propose` on
    the plain-HMC dynamics: l2hmc_fill_normal, l2hmc_small_trajectory, l2hmc_fill_uniform, l2hmc_mix_accept per step."""
    from tests.run_cases import assert_same_run
    from tests.test_gpu_small_hmc_run import _sampler, _x0
    B = 65
    new, old = _sampler(la, kind), _sampler(la, kind)
    for smp in (new, old):
        smp.dynamics._seed, smp.dynamics._draws = SEED, draw0
    x0 = _x0(B, new.dynamics.x_dim)
    a = new.run_hmc(n, x0, keep_samples=True)
    b = old.run(n, x0, keep_samples=True)
    assert_same_run(a, b, ("px", "samples"), f"{kind} draw0={draw0:#x}")
    assert new.dynamics._draws == old.dynamics._draws == draw0 + 2 * n
    # and the momenta are those of the reference: the first step's kinetic energy shows in nothing we can read, so
    # the decision is checked instead -- a chain moved iff px > u is not contradicted by the reference uniforms
    u = R.toy_hmc_step(SEED, draw0, 0, B, new.dynamics.x_dim)[1]
    moved = (a["samples"][0] != x0.cpu().numpy()).any(axis=1)
    clear = np.abs(a["px"][0] - u) > 1e-6
    assert np.array_equal(moved[clear], (a["px"][0] >= u)[clear])


@pytest.mark.parametrize("draw0", PC.TOY_EXCHANGE_DRAW0, ids=hex)
def test_toy_exchange_run_equals_the_loop_with_the_standalone_round(la, draw0):
    """l2hmc_small_hmc_run_exchange against run_hmc(2 steps), swap_replicas, ...: a step two streams, a round the next.
    The second start is the largest the entry takes (draw0 + 2 n_steps + rounds = 2^64 - 1)."""
    from tests.test_gpu_small_hmc_exchange import _assert_same, _loop, _sampler, _temps, _x0
    kind, B, G, n, k = "mog", 72, 3, PC.TOY_EXCHANGE_STEPS, PC.TOY_EXCHANGE_EVERY
    x0, temps = _x0(B, 2), _temps(B, G)
    ref_smp, smp = _sampler(la, kind, draws=draw0), _sampler(la, kind, draws=draw0)
    for s in (ref_smp, smp):
        s.dynamics._seed = SEED
    ref = _loop(ref_smp, n, temps, x0, G, k)
    out = smp.run_hmc_exchange(n, x0, keep_samples=True, temperature=temps, replicas=G, swap_every=k)
    _assert_same(out, ref, smp, ref_smp, f"draw0={draw0:#x}")
    assert smp.dynamics._draws == draw0 + 2 * n + n // k
    for j, st in enumerate(R.toy_hmc_run_streams(draw0, n, k)[1]):
        low = np.isfinite(out["swap_p"][j])
        u = R.uniform(SEED, st, np.arange(B))
        assert low.any() and np.array_equal(out["swapped"][j][low], out["swap_p"][j][low] > u[low]), j


@pytest.mark.parametrize("stream", PC.SWAP_STREAMS, ids=hex)
def test_lattice_replica_swap_decides_with_the_reference_uniforms(la, stream):
    """gauge_swap.h / replica_swap.hip: swap_p against the float64 round of tests/replica_ref.py, `swapped` against the
    kernel's own swap_p and tests/philox_ref.uniform, exactly.  The bound on swap_p is that of the action, which the
    suite holds to TOL_OP of its scale: |dp| <= |beta_a - beta_b| (|dS_a| + |dS_b|), plus one fp32 ulp of p."""
    from l2hmc_amd import lattice
    from tests import replica_ref as RR
    from tests.test_gpu_replica_swap import _input
    T, X, G, ng = 8, 8, 4, 7
    x, betas, labels, S64 = _input(T, X, G, ng)
    B = G * ng
    u = R.uniform(SEED, stream, np.arange(B))
    exchanged = pairs = 0
    for parity in (0, 1):
        xd = torch.as_tensor(x, device="cuda").clone()
        p, sw, act = lattice.replica_swap(xd, T, X, G, parity, torch.as_tensor(betas, device="cuda"), SEED, stream, 1,
                                          torch.as_tensor(labels, device="cuda").clone())
        torch.cuda.synchronize()
        p, sw = p.cpu().numpy(), sw.cpu().numpy()
        xr, pr, swr, perm = RR.swap_round(torch.as_tensor(x), betas.astype(np.float64), G, parity, u.astype(np.float64), T, X)
        low = RR.lower_chains(B, G, parity)
        # (2^-23: the fp32 difference of the betas, as the kernel forms it, times |S_a - S_b| <= 2 max S)
        bound = (np.abs(betas[low].astype(np.float64) - betas[low + 1]) * 2 * (TOL_OP + 2.0 ** -23)
                 * max(1.0, np.abs(S64).max()) + 1.2e-7)
        err = np.abs(p[low] - pr.numpy()[low])
        print(f"philox domain gauge_replica_swap stream={stream:#x} parity={parity}: swap_p err {err.max():.2e} "
              f"(bound {bound.min():.2e}..{bound.max():.2e}), {int(sw.sum())} of {low.size} exchanged")
        assert (err <= bound).all()
        assert np.array_equal(sw[low], p[low] > u[low]) and not np.delete(sw, low).any()
        clear = np.abs(pr.numpy()[low] - u[low]) > bound
        assert clear.sum() >= low.size - 1 and np.array_equal(sw[low][clear], swr.numpy()[low][clear])
        if clear.all():
            assert np.array_equal(xd.cpu().numpy(), xr.numpy())
        exchanged, pairs = exchanged + int(sw.sum()), pairs + low.size
    assert 0 < exchanged < pairs                                     # both outcomes: the uniforms decide


@pytest.mark.parametrize("stream", PC.SWAP_STREAMS, ids=hex)
def test_toy_replica_swap_decides_with_the_reference_uniforms(la, stream):
    """small_swap.h: the same for l2hmc_small_replica_swap on the 2-D mixture of tests/test_gpu_small_replica_swap.py,
    whose energies the suite holds to 2e-5 of their scale."""
    from tests import toy_replica_ref as TR
    from tests.replica_ref import lower_chains
    from tests.test_gpu_small_replica_swap import TOL_TARGET, _input, _sampler
    dim, K, kind, G, ng = 2, 2, "mixture", 3, 22
    x, temps, labels, U64 = _input(dim, K, kind, G, ng)
    B = G * ng
    smp = _sampler(la, dim, K, kind)
    smp.dynamics._seed = SEED
    u = R.uniform(SEED, stream, np.arange(B))
    exchanged = pairs = 0
    for parity in (0, 1):
        xd = torch.as_tensor(x, device="cuda").clone()
        smp.replica = torch.as_tensor(labels, device="cuda").clone()
        smp.dynamics._draws = stream
        p, sw, U = smp.swap_replicas(xd, torch.as_tensor(temps, device="cuda"), G, parity)
        torch.cuda.synchronize()
        p, sw = p.cpu().numpy(), sw.cpu().numpy()
        it = (np.float32(1) / temps).astype(np.float64)                # 1 / t in fp32, as every step forms it
        xr, pr, swr, perm = TR.swap_round(torch.as_tensor(x), 1.0 / it, G, parity, u.astype(np.float64),
                                          lambda _: torch.as_tensor(U64))
        low = lower_chains(B, G, parity)
        bound = np.abs(it[low] - it[low + 1]) * 2 * (TOL_TARGET + 2.0 ** -23) * max(1.0, np.abs(U64).max()) + 1.2e-7
        err = np.abs(p[low] - pr.numpy()[low])
        print(f"philox domain small_replica_swap stream={stream:#x} parity={parity}: swap_p err {err.max():.2e} "
              f"(bound {bound.min():.2e}..{bound.max():.2e}), {int(sw.sum())} of {low.size} exchanged")
        assert (err <= bound).all()
        assert np.array_equal(sw[low], p[low] > u[low]) and not np.delete(sw, low).any()
        clear = np.abs(pr.numpy()[low] - u[low]) > bound
        assert clear.sum() >= low.size - 1 and np.array_equal(sw[low][clear], swr.numpy()[low][clear])
        exchanged, pairs = exchanged + int(sw.sum()), pairs + low.size
    assert 0 < exchanged < pairs


# ================================================================= d. sensitivity, no reference involved
def _differs(a, b):
    """(px, state) pairs of two calls have nothing in common, chain by chain.  No accept probability that is not
    saturated (exactly 0 or 1: plain HMC from a hot start lowers the energy of every chain) has the same bits in both --
    a kernel that drops a word in ONE of its generators keeps the momenta or the direction coins of its chains and with
    them about half of the probabilities.  And no chain that certainly moved in both (px = 1; one step) has the same
    next state."""
    (pa, xa), (pb, xb) = a, b
    same_p = (pa == pb) & (pa > 0) & (pa < 1)
    same_x = (xa == xb).all(dim=-1) & (pa == 1) & (pb == 1) if pa.dim() == 1 else torch.zeros(1, dtype=torch.bool)
    return not torch.equal(xa, xb) and not bool(same_p.any()) and not bool(same_x.any())


@pytest.mark.parametrize("name", ["generic-8x8-subtile", "generic-8x8-16row", "conv3d-8x8", "generic-6x6-step-draws",
                                  "hmc-4x4", "hmc-16x32-two-sites", "hmc-32x32-selected"])
def test_lattice_steps_read_every_word_of_seed_and_draw(la, name):
    """px and the next state at (seed, draw) against those at the truncated twins: the seed without its high word, the
    draw in 31 bits (so that 2 * draw fits 32).  A kernel that ignores a high word makes them equal."""
    c = next(k for k in PC.LATTICE_CASES if k.name == name)
    _, dyn = _lattice_dyn(c)
    xd = torch.as_tensor(PC.lattice_x0(c), device="cuda")
    run = lambda seed, draw: [_step(dyn, xd, seed, draw)[k] for k in ("px", "x_next")]
    for draw in (2 ** 31, 2 ** 63 - 1):
        here = run(SEED, draw)
        assert all(torch.equal(x, y) for x, y in zip(here, run(SEED, draw)))          # the same call: the same bits
        twins = [(s2, draw) for s2 in PC.truncated_seeds(SEED)] + [(SEED, d2) for d2 in PC.truncated_draws(draw)]
        twins += [(PC.SEED_LOW_ZERO, draw), (SEED, draw ^ (1 << 32))]
        assert len(twins) == 4
        for seed2, draw2 in twins:
            assert _differs(here, run(seed2, draw2)), (name, hex(seed2), hex(draw2))


@pytest.mark.parametrize("kind", ["mog", "gmm3"])
def test_toy_kernels_read_every_word_of_seed_and_stream(la, kind):
    from tests.test_gpu_small_hmc_run import _toy as _toy_hmc
    from tests.test_gpu_small_run import _toy, _x0
    B = 37
    dyn, hmc = _toy(la, kind), _toy_hmc(la, kind)
    x0 = _x0(B, dyn.x_dim)

    def hmc_run(seed, draw0):
        from l2hmc_amd import _lib
        plan = hmc._plan()
        px, xn = torch.empty(2, B, device="cuda"), torch.empty_like(x0)
        _lib.call("l2hmc_small_hmc_run", C.byref(plan), x0, xn, B, seed, draw0, 2, None, 0, 0, None, px, None)
        torch.cuda.synchronize()
        return px, xn
    for fn, draw0 in ((lambda s, d: _propose(dyn, x0, s, d)[2:], 2 ** 64 - 4),
                      (lambda s, d: _small_run(dyn, x0, s, d, 2)[::2], 2 ** 64 - 13), (hmc_run, 2 ** 64 - 7)):
        here = fn(SEED, draw0)
        assert all(torch.equal(x, y) for x, y in zip(here, fn(SEED, draw0)))
        for seed2, draw2 in ((SEED & R.M32, draw0), (SEED, draw0 & R.M32), (PC.SEED_LOW_ZERO, draw0),
                             (SEED, draw0 ^ (1 << 32))):
            assert _differs(here, fn(seed2, draw2)), (kind, hex(seed2), hex(draw2))


# ================================================================= e. the Python layer on a counter beyond 2^32
def test_gauge_sampler_run_hmc_hands_the_entry_its_64_bit_counter(la):
    from l2hmc_amd import _lib
    T, X, B, n, draws = 4, 4, 9, 4, 2 ** 32 - 4
    dyn = _hmc_dyn(T, X, B)
    dyn._seed, dyn._draws = SEED, draws
    x0 = _lattice_x(T, X, B)
    out = la.GaugeSampler(dyn).run_hmc(n, PC.BETA, x0, keep_samples=True)
    draw0, after = _lib.run_draw_index(draws, n)
    assert draw0 == 2 ** 31 - 2 and dyn._draws == after == 2 ** 32 + 4
    want = _hmc_run(dyn, x0, SEED, draw0, n, ladder=True)
    for k in HIST:
        assert np.array_equal(out[k], want[k].cpu().numpy()), k
    assert np.array_equal(out["samples"], want["samples"].cpu().numpy())
    assert torch.equal(out["samples_out"], want["x_next"])


def test_dynamics_sampler_run_hands_the_entry_its_64_bit_counter(la):
    from tests.test_gpu_small_run import _toy, _x0
    B, n, draws = 37, 3, 2 ** 32 - 4
    dyn = _toy(la, "gmm3")
    dyn._seed, dyn._draws = SEED, draws
    x0 = _x0(B, dyn.x_dim)
    out = la.DynamicsSampler(dyn).run(n, x0, keep_samples=True)
    assert dyn._draws == draws + 4 * n
    px, samples, xn = _small_run(dyn, x0, SEED, draws, n)
    assert np.array_equal(out["px"], px.cpu().numpy()) and np.array_equal(out["samples"], samples.cpu().numpy())
    assert torch.equal(out["samples_out"], xn)
