"""Annealed importance sampling on the toy targets in one launch (l2hmc_small_ais_run, small_ais_run_kernel in
l2hmc_amd/csrc/small_ais.hip), `DynamicsSampler.ais` around it and `ais_estimate`.

1. At the ends of the schedule the kernel IS the plain-HMC run: every b = 1 gives the bits of `run_hmc` on the dynamics,
   every b = 0 those of `run_hmc` on a dynamics whose target is the init Gaussian at temperature 1.
2. On a real schedule the outputs are held against the float64 restatement of tests/ais_ref.py with
   `assert_fp32_equivalent`, the float32 restatement giving the intrinsic error, and px at max(TOL_P, P_RATIO x
   intrinsic).  No chain is left out: tests/test_ais_host.py holds every float64 |p - u| of these cases above MH_MARGIN
   on the draws of tests/philox_ref.py.  Here the restatements are fed the normals l2hmc_fill_normal writes for the same
   (seed, stream) -- which tests/test_gpu_philox_domain.py holds within 1e-5 of philox_ref.normal --, as that file feeds
   its oracles: float32 Box-Muller is up to 5e-6 away from the float64 one, an input error that is no part of the
   float32 restatement's own.  The uniforms are philox_ref's, which are bit exact.
3. Any chunking gives the same bits; the draws are counted; the caller's x is untouched.
4. The known-answer mixture case of the host file lands within 4 se of log Z1 = 0.
5. `ais_estimate` is `ais` on the dynamics it builds."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import dynamics as od
from tests import ais_ref as A
from tests import philox_ref as R
from tests import toy_cases as tc
from tests.run_cases import count_launches
from tests.test_gpu_parity import assert_fp32_equivalent
from tests.test_gpu_small_hmc_run import BATCHES, TOYS, _sampler, _x0

pytestmark = pytest.mark.gpu

END_KINDS = ["scg", "mog", "gmm3", "gauss8", "rw", "funnel"]
END_STEPS = 5


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _init(la, dim):
    return la.Gaussian(*A.init_arrays(dim))


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ----------------------------------------------------------------- 1. the ends of the schedule, bit for bit
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", END_KINDS)
def test_the_ends_of_the_schedule_are_plain_hmc_runs(la, kind, B):
    from l2hmc_amd import _lib
    dim, N, _ = TOYS[kind]
    init, x0 = _init(la, dim), _x0(B, dim)
    keep = x0.clone()
    # every b = 1: the run on the dynamics.  (Through `ais` b_0 = 0, so the first step adds E0 - E1 to the weights)
    want = _sampler(la, kind).run_hmc(END_STEPS, x0, keep_samples=False)
    smp = _sampler(la, kind)
    got = smp.ais(END_STEPS, init, x0, betas=np.ones(END_STEPS))
    assert smp.dynamics._draws == 4 + 2 * END_STEPS and torch.equal(x0, keep)
    assert got["px"].dtype == np.float32 and np.array_equal(got["px"], want["px"]), kind
    assert torch.equal(got["samples_out"], want["samples_out"]) and got["mean_accept"] == want["mean_accept"]
    one = _sampler(la, kind).ais(1, init, x0, betas=np.ones(1))
    assert np.array_equal(got["log_w"], one["log_w"]) and (got["log_w"] != 0).all()     # the later steps add exactly 0
    # ... and the entry itself with b_{s-1} = 1 as well: log_w is exactly 0
    dyn = _sampler(la, kind).dynamics
    init_target = init.get_energy_function().target                 # (owns the device arrays the struct points to)
    plan, st = dyn._plan(), init_target.struct(1.0)
    ones = torch.ones(END_STEPS + 1, device="cuda")
    x_next, log_w = torch.empty_like(x0), torch.zeros(B, dtype=torch.float64, device="cuda")
    px = torch.empty(END_STEPS, B, device="cuda")
    _lib.call("l2hmc_small_ais_run", C.byref(plan), C.byref(st), x0, x_next, None, 0.0, B, dyn._seed, 4, END_STEPS, ones,
              log_w.data_ptr(), px)
    assert torch.equal(x_next, want["samples_out"]) and np.array_equal(px.cpu().numpy(), want["px"])
    assert (log_w == 0).all()
    # every b = 0: the run on the init Gaussian at temperature 1, whatever the final target and its temperature
    dyn0 = la.Dynamics(dim, init.get_energy_function(), trajectory_length=N, eps=0.1, hmc=True, use_temperature=True,
                       seed=7)
    dyn0.set_masks(od.make_masks(N, dim, np.random.RandomState(3)))
    dyn0._draws = 4
    want0 = la.DynamicsSampler(dyn0).run_hmc(END_STEPS, x0, keep_samples=False)
    got0 = _sampler(la, kind, temperature=2.5).ais(END_STEPS, init, x0, betas=np.zeros(END_STEPS))
    assert np.array_equal(got0["px"], want0["px"]) and torch.equal(got0["samples_out"], want0["samples_out"]), kind
    assert got0["log_w"].dtype == np.float64 and (got0["log_w"] == 0).all()
    assert B == 1 or not torch.equal(got0["samples_out"], got["samples_out"])


# ----------------------------------------------------------------- 2. a real schedule against the restatement
def _parity_dynamics(la, kind, refresh, spl=256):
    dim, temperature, eps = A.KINDS[kind]
    dyn = la.Dynamics(dim, A.final_library(la, kind).get_energy_function(), trajectory_length=A.PARITY_LF, eps=eps,
                      hmc=True, use_temperature=True, seed=A.PARITY_SEEDS[(kind, refresh)])
    dyn.temperature = temperature
    dyn.set_masks(A.masks(A.PARITY_LF, dim))
    dyn._draws = A.DRAW0
    smp = la.DynamicsSampler(dyn)
    smp.steps_per_launch = spl
    return smp


def _device_normal(seed, stream, i):
    """Elements i of what l2hmc_fill_normal writes for (seed, stream)."""
    from l2hmc_amd import ops
    i = np.asarray(i)
    return np_(ops.fill_normal((int(i.max()) + 1,), seed, stream, torch.device("cuda")))[i]


def _parity_run(la, kind, refresh, B, spl=256):
    smp = _parity_dynamics(la, kind, refresh, spl)
    x0 = torch.from_numpy(A.start(A.KINDS[kind][0], B).astype(np.float32)).to("cuda")
    keep = x0.clone()
    out = smp.ais(A.PARITY_STEPS, _init(la, A.KINDS[kind][0]), x0, betas=A.PARITY_SCHEDULE,
                  refresh=A.REFRESH if refresh else None)
    assert torch.equal(x0, keep)                                     # the caller's x is not advanced in place
    assert smp.dynamics._draws == A.DRAW0 + 2 * A.PARITY_STEPS + (1 if refresh else 0)
    assert set(out) == {"log_w", "log_ratio", "log_z", "se", "ess", "px", "mean_accept", "samples_out"} | (
        {"v_out"} if refresh else set())
    return out


@pytest.mark.parametrize("B", A.PARITY_BATCHES)
@pytest.mark.parametrize("refresh", [False, True], ids=["fresh", "refresh"])
@pytest.mark.parametrize("kind", list(A.KINDS))
def test_a_real_schedule_matches_the_float64_restatement(la, kind, refresh, B):
    dim, temperature, eps = A.KINDS[kind]
    mu, sigma = A.init_arrays(dim)
    got = _parity_run(la, kind, refresh, B)
    args = (od.Gaussian(mu, sigma), A.final_oracle(kind), temperature, A.masks(A.PARITY_LF, dim), eps, A.start(dim, B),
            A.PARITY_SCHEDULE, A.PARITY_SEEDS[(kind, refresh)], A.DRAW0)
    w64, w32 = (A.anneal(*args, refresh=A.REFRESH if refresh else None, dtype=dt, draws=(_device_normal, R.uniform))
                for dt in (np.float64, np.float32))
    what = f"ais {kind} refresh={refresh} B={B}"
    # no chain is left out: no decision of the reference lies near a tie, on these draws as on philox_ref's
    assert w64["margin"].min() > tc.MH_MARGIN, (what, w64["margin"].min())
    assert np.array_equal(w64["accepted"], A.parity_reference(kind, refresh, B)[0]["accepted"]), what
    assert w64["accepted"].any() and not w64["accepted"].all(), what
    pairs = [("log_w", got["log_w"], "log_w"), ("samples_out", np_(got["samples_out"]), "x")]
    if refresh:
        pairs.append(("v_out", np_(got["v_out"]), "v"))
    for name, g, k in pairs:
        print(f"{what} {name}: max {tc.relerr(g, w64[k]):.2e} (fp32 restatement {tc.relerr(w32[k], w64[k]):.2e})")
    perr, pbar = float(np.abs(got["px"].astype(np.float64) - w64["px"]).max()), tc.p_bar(w64["px"], w32["px"])
    print(f"{what} px: max {perr:.2e} (bar {pbar:.2e})")
    for name, g, k in pairs:
        assert g.shape == w64[k].shape
        assert_fp32_equivalent(g, w64[k], w32[k], f"{what} {name}")
    assert got["px"].shape == (A.PARITY_STEPS, B) and perr < pbar, (what, perr, pbar)
    assert np.isclose(got["mean_accept"], w64["px"].mean(), atol=pbar)
    # the finishing is the restatement's, on the kernel's weights
    log_ratio, se, ess = A.estimate(got["log_w"]) if B > 1 else (float(got["log_w"][0]), float("nan"), 1.0)
    assert np.isclose(got["log_ratio"], log_ratio, rtol=1e-12, atol=1e-12) and np.isclose(got["ess"], ess, rtol=1e-12)
    assert (np.isnan(got["se"]) and B == 1) or np.isclose(got["se"], se, rtol=1e-12)
    assert np.isclose(got["log_z"], got["log_ratio"] + A.log_norm(sigma), rtol=1e-12, atol=1e-12)


# ----------------------------------------------------------------- 3. chunks, launches, the entry on its own
@pytest.mark.parametrize("refresh", [False, True], ids=["fresh", "refresh"])
@pytest.mark.parametrize("kind,B", [("mog", 130), ("gmm3", 65), ("funnel", 63)])
def test_any_chunking_gives_the_same_bits(la, kind, refresh, B):
    runs = [_parity_run(la, kind, refresh, B, spl) for spl in (256, 3, 1)]
    for other in runs[1:]:
        for k in ("log_w", "px"):
            assert runs[0][k].dtype == other[k].dtype and np.array_equal(runs[0][k], other[k]), (kind, k)
        for k in ("samples_out",) + (("v_out",) if refresh else ()):
            assert torch.equal(runs[0][k], other[k]), (kind, k)
        for k in ("log_ratio", "log_z", "se", "ess", "mean_accept"):
            assert runs[0][k] == other[k], (kind, k)
    assert np.isfinite(runs[0]["log_w"]).all() and (runs[0]["log_w"] != 0).all()


def test_ais_is_one_launch_per_chunk(la):
    x0 = torch.from_numpy(A.start(2, 65).astype(np.float32)).to("cuda")
    for spl in (256, 3):
        smp = _parity_dynamics(la, "mog", False, spl)
        run = lambda: smp.ais(A.PARITY_STEPS, _init(la, 2), x0, betas=A.PARITY_SCHEDULE)
        run()                                                        # warm-up
        assert count_launches(7, run) == math.ceil(A.PARITY_STEPS / spl)


@pytest.mark.parametrize("kind,B", [("mog", 70), ("gauss8", 33), ("rw", 65)])
def test_c_entry_outputs_are_optional_and_it_runs_in_place(la, kind, B):
    from l2hmc_amd import _lib
    smp = _parity_dynamics(la, kind, True)
    dyn, n = smp.dynamics, A.PARITY_STEPS
    D = dyn.x_dim
    init_target = _init(la, D).get_energy_function().target         # (owns the device arrays the struct points to)
    plan, st = dyn._plan(), init_target.struct(7.0)                  # the init's temperature is not read
    betas = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), A.PARITY_SCHEDULE])).to("cuda")
    x0 = torch.from_numpy(A.start(D, B).astype(np.float32)).to("cuda")
    v0 = torch.randn(B, D, generator=torch.Generator().manual_seed(5)).to("cuda")

    def call(x_in, x_next, v, s0, m, log_w, px):
        _lib.call("l2hmc_small_ais_run", C.byref(plan), C.byref(st), x_in, x_next, v, 0.1, B, 77, 5 + 2 * s0, m,
                  betas[s0:], log_w.data_ptr(), px)
        torch.cuda.synchronize()

    zeros = lambda: torch.zeros(B, dtype=torch.float64, device="cuda")
    full, v_full, w_full, px = torch.empty_like(x0), v0.clone(), zeros(), torch.empty(n, B, device="cuda")
    call(x0, full, v_full, 0, n, w_full, px)
    inplace, v_bare, w_bare = x0.clone(), v0.clone(), zeros()
    call(inplace, inplace, v_bare, 0, n, w_bare, None)               # no px, x_next aliases x_in
    assert torch.equal(full, inplace) and torch.equal(v_full, v_bare) and torch.equal(w_full, w_bare)
    assert not torch.equal(full, x0) and not torch.equal(v_full, v0)
    # the steps chain through x, v and log_w: 3 steps, then 5 from the same schedule at an offset
    x, v, w = x0.clone(), v0.clone(), zeros()
    call(x, x, v, 0, 3, w, None)
    call(x, x, v, 3, n - 3, w, None)
    assert torch.equal(x, full) and torch.equal(v, v_full) and torch.equal(w, w_full)
    # without v the momenta are fresh and refreshment is not read
    a, b, wa, wb = torch.empty_like(x0), torch.empty_like(x0), zeros(), zeros()
    _lib.call("l2hmc_small_ais_run", C.byref(plan), C.byref(st), x0, a, None, 0.1, B, 77, 5, n, betas, wa.data_ptr(), None)
    _lib.call("l2hmc_small_ais_run", C.byref(plan), C.byref(st), x0, b, None, -3.0, B, 77, 5, n, betas, wb.data_ptr(), None)
    assert torch.equal(a, b) and torch.equal(wa, wb) and not torch.equal(a, full)


# ----------------------------------------------------------------- 4. a known answer
def test_the_mixture_has_log_z_zero(la):
    """cfg 2's mixture from N(0, I): log(Z1 / Z0) = -log(2 pi).  The bar is 4 x the se of the float64 restatement of the
    same case, which tests/test_ais_host.py holds within 2 se of the exact value."""
    k = A.known("mixture")
    _, ref_ratio, ref_se, ref_ess = A.known_reference("mixture")
    m = k.final
    dyn = la.Dynamics(2, la.GMM(m.mus, m.sigmas, m.pis).get_energy_function(), trajectory_length=k.lf, eps=k.eps,
                      hmc=True, seed=k.seed)
    dyn.set_masks(A.masks(k.lf, 2))
    x0 = torch.from_numpy(A.known_start(k).astype(np.float32)).to("cuda")
    out = la.DynamicsSampler(dyn).ais(k.steps, la.Gaussian(np.zeros(2), k.init_sigma), x0)
    print(f"ais mixture on the GPU: log_ratio {out['log_ratio']:.4f} (restatement {ref_ratio:.4f}, exact {k.exact:.4f}) "
          f"se {out['se']:.4f} ({ref_se:.4f}) ess {out['ess']:.1f} ({ref_ess:.1f}) log_z {out['log_z']:.4f}")
    assert dyn._draws == 2 * k.steps and out["px"].shape == (k.steps, k.B)
    assert abs(out["log_ratio"] - k.exact) <= 4 * ref_se
    assert abs(out["log_z"]) <= 4 * ref_se and out["ess"] >= k.B / 8


# ----------------------------------------------------------------- 5. the reference-shaped function
@pytest.mark.parametrize("refresh", [False, True], ids=["fresh", "refresh"])
def test_ais_estimate_is_ais_on_the_dynamics_it_builds(la, refresh):
    m = A.final_oracle("mog")
    final, init = la.GMM(m.mus, m.sigmas, m.pis), la.Gaussian(np.zeros(2), np.eye(2))
    x0 = torch.from_numpy(A.start(2, 130).astype(np.float32)).to("cuda")
    log_ratio, mean_alpha = la.ais_estimate(init, final, 16, x0, step_size=0.2, leapfrogs=5, refresh=refresh,
                                            refreshment=0.25, seed=11)
    dyn = la.Dynamics(2, final.get_energy_function(), trajectory_length=5, eps=0.2, hmc=True, seed=11)
    out = la.DynamicsSampler(dyn).ais(16, init, x0, refresh=0.25 if refresh else None)
    assert dyn._draws == 32 + (1 if refresh else 0)
    assert log_ratio == out["log_ratio"] and mean_alpha == out["mean_accept"] and np.isfinite(log_ratio)
    other = la.ais_estimate(init, final, 16, x0, step_size=0.2, leapfrogs=5, refresh=not refresh, refreshment=0.25, seed=11)
    assert other[0] != log_ratio
