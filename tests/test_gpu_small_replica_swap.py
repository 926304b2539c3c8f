"""One replica-exchange round on a toy target on its own: l2hmc_small_replica_swap (small_swap_kernel in
l2hmc_amd/csrc/small_hmc.hip around small_swap.h's round) through `DynamicsSampler.swap_replicas` and the C entry.

No decision is compared across precisions.  The energy of every chain of a pair is held to float64 at the bar
tests/test_gpu_toy_limits.py holds l2hmc_mog_energy_grad's energy to (2e-5 of the largest energy); the probability is
the float64 formula of the round applied to the kernel's OWN returned energies and the fp32 1 / t, to one float32 ulp
(the only freedom is the double exp and one rounding); the decision is `swap_p > u` with u from `ops.fill_uniform`,
exactly; and the state and the labels after the call are the input with exactly the accepted pairs exchanged.

Targets: the three mixtures of toy_cases.TARGET_CASES whose parameters the kernel reads from LDS, a 2-D mixture of two
components (the register-held instance), a 7-D Gaussian, a 3-D rough well and a 2-D funnel (the analytic instances at
both widths).  Groups of 2, 3, 5, 8 and 64 rungs, one group and then enough for a second, partial workgroup: 3 rungs
give 63 chains per workgroup, a group of 5 straddles lanes 15 | 16, and 64 rungs at parity 1 pair the lanes (15, 16)
and (31, 32)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import toy_cases as tc
from tests.replica_ref import lower_chains
from tests.run_cases import count_launches

pytestmark = pytest.mark.gpu

TOL_TARGET = 2e-5                  # tests/test_gpu_toy_limits.py
M, G_ = tc.M, tc.G
TARGETS = [(4, 4, M), (5, 8, M), (8, 8, M), (2, 2, M), (7, 1, G_), (3, 1, "rough_well"), (2, 1, "funnel")]
assert all(t in tc.TARGET_CASES for t in TARGETS[:3] + TARGETS[4:5])
# (rungs, groups): one group; then a second workgroup that is not full
GROUPS = {2: (1, 33), 3: (1, 22), 5: (1, 13), 8: (1, 9), 64: (1, 2)}
SEED, STREAM = 7, 5
RW_EPS, RW_EASY = 0.5, True
FUNNEL_SIGMA, FUNNEL_CLIP = 2.0, 8.0


@pytest.fixture(scope="module")
def la():
    import l2hmc_amd
    from l2hmc_amd import _lib
    _lib.lib()
    return l2hmc_amd


def _library_target(la, dim, K, kind):
    if kind == "rough_well":
        return la.RoughWell(dim, RW_EPS, easy=RW_EASY)
    if kind == "funnel":
        return la.GaussianFunnel(dim)
    return tc.target(dim, K, kind)[1]


def _sampler(la, dim, K, kind, hmc=True):
    """A sampler whose next stream is STREAM; plain HMC or (hmc=False) an L2HMC dynamics: the round reads the target."""
    from oracle import dynamics as od
    kw = dict(hmc=True) if hmc else dict(net_factory=lambda d, scope, factor: la.network(d, scope, factor, num_nodes=10))
    dyn = la.Dynamics(dim, _library_target(la, dim, K, kind).get_energy_function(), trajectory_length=3, eps=0.1,
                      use_temperature=True, seed=SEED, **kw)
    dyn.set_masks(od.make_masks(3, dim, np.random.RandomState(3)))
    dyn._draws = STREAM
    assert not dyn.layered and dyn._seed == SEED
    return la.DynamicsSampler(dyn)


@functools.lru_cache(maxsize=None)
def _input(dim, K, kind, G, ng):
    """(x [B, dim] fp32, temps [B] fp32 in (0.5, 5) with two equal neighbours in groups 2 and 5, labels [B] int32, the
    float64 energies at temperature 1): NumPy, made once, read only."""
    B = G * ng
    rng = np.random.default_rng(1000 * dim + 10 * G + ng)
    if kind == "rough_well":
        x = rng.normal(0, 1.5, (B, dim)).astype(np.float32)
        x64 = x.astype(np.float64)
        U = 0.5 * (x64 ** 2).sum(1) + RW_EPS * np.cos(x64 / (RW_EPS if RW_EASY else RW_EPS ** 2)).sum(1)
    elif kind == "funnel":
        x = rng.normal(0, 1.0, (B, dim))
        x[:, 0] = np.resize(np.array([-9., -8., -7.5, 0., 7.5, 8., 9., 1.5, -2.]), B)      # both clipped branches too
        x[:, 1:] *= np.exp(np.clip(x[:, :1], -FUNNEL_CLIP, FUNNEL_CLIP) / 2)
        x = x.astype(np.float32)
        x64 = x.astype(np.float64)
        s = np.exp(np.clip(x64[:, 0], -FUNNEL_CLIP, FUNNEL_CLIP))
        U = 0.5 * ((x64[:, 0] / FUNNEL_SIGMA) ** 2 + (x64[:, 1:] ** 2).sum(1) / s + (dim - 1) * np.log(2 * np.pi * s))
    else:
        x = tc.target_points(dim, K, kind, B)[0]
        U = tc.target_reference(dim, K, kind, B, temperature=1.0)[0]
    temps = rng.uniform(0.5, 5, B).astype(np.float32)
    if ng > 2:
        temps[2 * G + 1] = temps[2 * G]                      # the pair (0, 1) of group 2: p = 1 exactly
    if ng > 5 and G > 2:
        temps[5 * G + 2] = temps[5 * G + 1]                  # the pair (1, 2) of group 5
    labels = rng.permutation(B).astype(np.int32)
    return x, temps, labels, np.asarray(U, dtype=np.float64)


def _round(smp, x, temps, labels, G, parity):
    xd = torch.as_tensor(x, device="cuda").clone()
    smp.replica = torch.as_tensor(labels, device="cuda").clone()
    smp.dynamics._draws = STREAM
    p, sw, U = smp.swap_replicas(xd, torch.as_tensor(temps, device="cuda"), G, parity)
    torch.cuda.synchronize()
    assert smp.dynamics._draws == STREAM + 1
    return xd, smp.replica, p, sw, U


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _masks(B, G, parity):
    low = lower_chains(B, G, parity)
    member, lower = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    member[low] = member[low + 1] = lower[low] = True
    return low, member, lower


@pytest.mark.parametrize("G", list(GROUPS))
@pytest.mark.parametrize("dim,K,kind", TARGETS)
def test_round_against_float64_and_its_own_energies(la, dim, K, kind, G):
    from l2hmc_amd import ops
    smp = _sampler(la, dim, K, kind)
    for ng in GROUPS[G]:
        x, temps, labels, U64 = _input(dim, K, kind, G, ng)
        B = G * ng
        u = ops.fill_uniform(B, SEED, STREAM, device="cuda").cpu().numpy()
        for parity in (0, 1):
            what = f"d{dim}-K{K}-{kind} G={G} groups={ng} parity={parity}"
            xd, rd, p, sw, U = _round(smp, x, temps, labels, G, parity)
            p, sw, U = p.cpu().numpy(), sw.cpu().numpy(), U.cpu().numpy()
            low, member, lower = _masks(B, G, parity)
            if G == 2 and parity == 1:
                # no pair: nothing changes
                assert low.size == 0
                assert np.isnan(p).all() and not sw.any() and np.isnan(U).all(), what
                assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(rd.cpu().numpy(), labels), what
                continue
            # energy: every member of a pair against float64; the chains that sit out keep the wrapper's NaN
            err = float(np.abs(U[member] - U64[member]).max() / max(np.abs(U64[member]).max(), 1e-30))
            print(f"small_replica_swap {what}: energy rel max {err:.2e}")
            assert err < TOL_TARGET, (what, err)
            assert np.isnan(U[~member]).all(), what
            # probability: the float64 formula on the kernel's own energies and the fp32 1 / t, to one float32 ulp
            it = (np.float32(1) / temps).astype(np.float64)
            with np.errstate(under="ignore"):
                p64 = np.exp(np.minimum((it[low] - it[low + 1]) * (U[low].astype(np.float64) - U[low + 1]), 0.0))
            ulp = np.spacing(np.maximum(p64.astype(np.float32), np.float32(0)))
            assert (np.abs(p[low].astype(np.float64) - p64) <= ulp).all(), (what, p[low], p64)
            assert np.isnan(p[~lower]).all(), what
            # decision: strict, with the uniforms of fill_uniform's stream
            assert np.array_equal(sw[low], p[low] > u[low]), what
            assert not sw[~lower].any(), what
            # state and labels: the input with exactly the accepted pairs exchanged
            perm = np.arange(B)
            a = low[sw[low]]
            perm[a], perm[a + 1] = a + 1, a
            assert np.array_equal(xd.cpu().numpy(), x[perm]), what
            assert np.array_equal(rd.cpu().numpy(), labels[perm]), what
            assert (perm[~member] == np.arange(B)[~member]).all()


def test_equal_temperatures_always_exchange_and_a_scalar_exchanges_every_pair(la):
    dim, K, kind, G, ng = 5, 8, M, 8, 9
    smp = _sampler(la, dim, K, kind)
    x, temps, labels, _ = _input(dim, K, kind, G, ng)
    _, _, p, sw, _ = _round(smp, x, temps, labels, G, 0)
    assert float(p[2 * G]) == 1.0 and bool(sw[2 * G])
    _, _, p, sw, _ = _round(smp, x, temps, labels, G, 1)
    assert float(p[5 * G + 1]) == 1.0 and bool(sw[5 * G + 1])
    seen = set()                                             # both outcomes occur
    for parity in (0, 1):
        sw = _round(smp, x, temps, labels, G, parity)[3].cpu().numpy()
        seen |= set(sw[lower_chains(G * ng, G, parity)].tolist())
    assert seen == {True, False}
    xd = torch.as_tensor(x, device="cuda").clone()
    p, sw, _ = smp.swap_replicas(xd, 2.5, G, 0)
    low = lower_chains(G * ng, G, 0)
    assert (p[low] == 1.0).all() and sw[low].all() and int(sw.sum()) == low.size


@pytest.mark.parametrize("dim,K,kind", [(2, 2, M), (8, 8, M), (3, 1, "rough_well")])
def test_a_nan_coordinate_gives_probability_zero_and_no_exchange(la, dim, K, kind):
    G, ng = 5, 13
    smp = _sampler(la, dim, K, kind)
    x, temps, labels, _ = _input(dim, K, kind, G, ng)
    x = x.copy()
    x[0, 0] = np.nan                       # the lower chain of pair (0, 1)
    x[G + 3, dim - 1] = np.nan             # the upper chain of pair (2, 3) of group 1
    xd, rd, p, sw, _ = _round(smp, x, temps, labels, G, 0)
    assert float(p[0]) == 0.0 and not bool(sw[0]) and float(p[G + 2]) == 0.0 and not bool(sw[G + 2])
    out = xd.cpu().numpy()
    assert np.array_equal(out[[0, 1, G + 2, G + 3]], x[[0, 1, G + 2, G + 3]], equal_nan=True)
    assert np.array_equal(rd.cpu().numpy()[[0, 1, G + 2, G + 3]], labels[[0, 1, G + 2, G + 3]])
    assert bool(sw.any())


@pytest.mark.parametrize("dim,K,kind,G", [(4, 4, M, 3), (2, 2, M, 5), (2, 1, "funnel", 8)])
def test_a_group_does_not_depend_on_the_rest_of_the_batch(la, dim, K, kind, G):
    """The stream element is the chain index, so the group is placed first: alone it gives the bits it gives as group 0
    of a batch that fills more than one workgroup."""
    smp = _sampler(la, dim, K, kind)
    x, temps, labels, _ = _input(dim, K, kind, G, GROUPS[G][1])
    for parity in (0, 1):
        full = _round(smp, x, temps, labels, G, parity)
        full = [t.clone() for t in full]
        alone = _round(smp, x[:G], temps[:G], labels[:G], G, parity)
        for f, a in zip(full, alone):
            assert torch.equal(_bits(f[:G]), _bits(a)), (dim, K, kind, G, parity)


def test_an_l2hmc_dynamics_gives_the_same_round(la):
    dim, K, kind, G, ng = 4, 4, M, 3, 22
    x, temps, labels, _ = _input(dim, K, kind, G, ng)
    a = _round(_sampler(la, dim, K, kind, hmc=True), x, temps, labels, G, 1)
    b = _round(_sampler(la, dim, K, kind, hmc=False), x, temps, labels, G, 1)
    for s, t in zip(a, b):
        assert torch.equal(_bits(s), _bits(t))
    assert bool(a[3].any())


def test_outputs_are_optional_untouched_entries_stay_and_a_round_without_a_pair_launches_nothing(la):
    from l2hmc_amd import _lib
    dim, K, kind, G, ng = 5, 8, M, 5, 13
    smp = _sampler(la, dim, K, kind)
    plan = smp.dynamics._plan()
    x, temps, labels, _ = _input(dim, K, kind, G, ng)
    B = G * ng
    td = torch.as_tensor(temps, device="cuda")
    ref = _round(smp, x, temps, labels, G, 1)
    xd = torch.as_tensor(x, device="cuda").clone()
    swap = lambda *a: _lib.call("l2hmc_small_replica_swap", C.byref(plan), *a)
    assert count_launches(8, lambda: swap(xd, B, G, 1, td, 1, SEED, STREAM, None, None, None, None)) == 1
    assert torch.equal(xd, ref[0])
    U = torch.full((B,), -3.0, device="cuda")
    xd = torch.as_tensor(x, device="cuda").clone()
    swap(xd, B, G, 1, td, 1, SEED, STREAM, None, U, None, None)
    assert torch.equal(xd, ref[0])
    assert (U[0::G] == -3.0).all() and torch.equal(U[1:G], ref[4][1:G])            # chain 0 of a group sits out
    # group 2, parity 1: the outputs are filled, nothing else is touched, nothing is launched
    pp, ss = torch.zeros(4, device="cuda"), torch.ones(4, dtype=torch.uint8, device="cuda")
    U = torch.full((4,), -3.0, device="cuda")
    xd = torch.as_tensor(x[:4], device="cuda").clone()
    assert count_launches(8, lambda: swap(xd, 4, 2, 1, td, 1, SEED, STREAM, None, U, pp, ss)) == 0
    assert torch.isnan(pp).all() and not ss.any() and np.array_equal(xd.cpu().numpy(), x[:4]) and (U == -3.0).all()
    smp.replica = None
    assert count_launches(8, lambda: smp.swap_replicas(xd, td[:4], 2, 1)) == 0
    assert count_launches(7, lambda: smp.swap_replicas(xd, td[:4], 2, 0)) == 0
