"""One replica-exchange round on its own: l2hmc_gauge_replica_swap (l2hmc_amd/csrc/replica_swap.hip) through
`lattice.replica_swap`.

No decision is compared across precisions.  The action of every chain of a pair is held to the float64 oracle at the
bar the project holds that sum to (TOL_OP); the probability is the float64 formula of the round applied to the kernel's
OWN returned actions, to one float32 ulp (the only freedom is the double exp and one rounding); the decision is
`swap_p > u` with u from `ops.fill_uniform`, exactly; and the state after the call is the input with exactly the
accepted pairs exchanged.  Shapes: 15 sites (a wave with dead lanes, rows that are no multiple of 16 bytes), 64 (one
wave per pair, four pairs per workgroup), 36, 320 and 1024 (four waves per pair, several plaquettes per thread) and
1056 sites -- more than the one-launch run kernel takes.  1 and 7 groups: a partial workgroup and more than one."""
import numpy as np
import pytest
import torch

from oracle import lattice as olat
from tests import helpers as H
from tests import replica_ref as R

pytestmark = pytest.mark.gpu

TOL_OP = 1e-5                      # tests/test_gpu_parity.py
SHAPES = [(3, 5), (8, 8), (6, 6), (16, 20), (32, 32), (33, 32)]
GROUP_SIZES = [2, 3, 4, 5]
SEED, STREAM = 77, 5


@pytest.fixture(scope="module")
def ops():
    from l2hmc_amd import _lib, ops
    _lib.lib()
    return ops


def replica_swap(*args, **kw):
    from l2hmc_amd import lattice
    return lattice.replica_swap(*args, **kw)


_INPUT = {}


def _input(T, X, G, ng):
    """(x [B, 2TX] fp32 uniform in (-7, 7) as test_u1_action_force_observables draws it, betas [B] fp32 in (0.5, 5)
    with two equal neighbours in groups 2 and 5, labels [B] int32, the float64 actions): NumPy, made once, read only."""
    key = (T, X, G, ng)
    if key not in _INPUT:
        B = G * ng
        rng = np.random.default_rng(1)
        x = rng.uniform(-7, 7, (B, 2 * T * X)).astype(np.float32)
        betas = rng.uniform(0.5, 5, B).astype(np.float32)
        if ng > 2:
            betas[2 * G + 1] = betas[2 * G]                      # the pair (0, 1) of group 2: p = 1 exactly
        if ng > 5 and G > 2:
            betas[5 * G + 2] = betas[5 * G + 1]                  # the pair (1, 2) of group 5
        labels = rng.permutation(B).astype(np.int32)
        _INPUT[key] = (x, betas, labels, olat.total_action(x.astype(np.float64), T, X))
    return _INPUT[key]


def _round(ops, x, betas, labels, T, X, G, parity):
    xd = torch.as_tensor(x, device="cuda").clone()
    rd = torch.as_tensor(labels, device="cuda").clone()
    p, sw, act = replica_swap(xd, T, X, G, parity, torch.as_tensor(betas, device="cuda"), SEED, STREAM, 1, rd)
    torch.cuda.synchronize()
    return xd, rd, p, sw, act


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("G", GROUP_SIZES)
@pytest.mark.parametrize("T,X", SHAPES)
def test_round_against_float64_and_its_own_actions(ops, T, X, G):
    for ng in (1, 7):
        x, betas, labels, S64 = _input(T, X, G, ng)
        B = G * ng
        u = ops.fill_uniform(B, SEED, STREAM, device="cuda").cpu().numpy()
        for parity in (0, 1):
            what = f"{T}x{X} G={G} groups={ng} parity={parity}"
            xd, rd, p, sw, act = _round(ops, x, betas, labels, T, X, G, parity)
            p, sw, act = p.cpu().numpy(), sw.cpu().numpy(), act.cpu().numpy()
            low = R.lower_chains(B, G, parity)
            member = np.zeros(B, dtype=bool)
            member[low] = member[low + 1] = True
            lower = np.zeros(B, dtype=bool)
            lower[low] = True
            if G == 2 and parity == 1:
                # no pair: nothing changes, nothing is launched
                assert low.size == 0
                assert np.isnan(p).all() and not sw.any() and np.isnan(act).all(), what
                assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(rd.cpu().numpy(), labels), what
                continue
            # action: every member of a pair against float64; the chains that sit out keep the wrapper's NaN
            assert H.relerr(act[member], S64[member]) < TOL_OP, what
            assert np.isnan(act[~member]).all(), what
            # probability: the float64 formula on the kernel's own actions, to one float32 ulp
            db = (betas[low] - betas[low + 1]).astype(np.float64)            # the fp32 difference, as the kernel forms it
            with np.errstate(under="ignore"):
                p64 = np.exp(np.minimum(db * (act[low].astype(np.float64) - act[low + 1].astype(np.float64)), 0.0))
            ulp = np.spacing(np.maximum(p64.astype(np.float32), np.float32(0)))
            assert (np.abs(p[low].astype(np.float64) - p64) <= ulp).all(), (what, p[low], p64)
            assert np.isnan(p[~lower]).all(), what
            # decision: strict, with the uniforms of fill_uniform's stream
            assert np.array_equal(sw[low], p[low] > u[low]), what
            assert not sw[~lower].any(), what
            # state: the input with exactly the accepted pairs exchanged (chains outside every pair untouched)
            perm = np.arange(B)
            a = low[sw[low]]
            perm[a], perm[a + 1] = a + 1, a
            assert np.array_equal(xd.cpu().numpy(), x[perm]), what
            assert np.array_equal(rd.cpu().numpy(), labels[perm]), what
            assert (perm[~member] == np.arange(B)[~member]).all()


def test_equal_betas_always_exchange_and_both_outcomes_occur(ops):
    T, X, G, ng = 8, 8, 4, 7
    x, betas, labels, _ = _input(T, X, G, ng)
    _, _, p, sw, _ = _round(ops, x, betas, labels, T, X, G, 0)
    assert float(p[2 * G]) == 1.0 and bool(sw[2 * G])
    _, _, p, sw, _ = _round(ops, x, betas, labels, T, X, G, 1)
    assert float(p[5 * G + 1]) == 1.0 and bool(sw[5 * G + 1])
    seen = set()
    for parity in (0, 1):
        sw = _round(ops, x, betas, labels, T, X, G, parity)[3].cpu().numpy()
        seen |= set(sw[R.lower_chains(G * ng, G, parity)].tolist())
    assert seen == {True, False}


@pytest.mark.parametrize("T,X,G", [(3, 5, 3), (8, 8, 4), (16, 20, 5), (33, 32, 2)])
def test_a_group_does_not_depend_on_the_rest_of_the_batch(ops, T, X, G):
    """The stream element is the chain index, so the group is placed first: alone it gives the bits it gives as group 0
    of 7."""
    x, betas, labels, _ = _input(T, X, G, 7)
    for parity in (0, 1):
        full = _round(ops, x, betas, labels, T, X, G, parity)
        alone = _round(ops, x[:G], betas[:G], labels[:G], T, X, G, parity)
        for f, a in zip(full, alone):
            assert torch.equal(_bits(f[:G]), _bits(a)), (T, X, G, parity)


def test_outputs_are_optional_and_untouched_entries_stay(ops):
    """The C entry with NULL outputs gives the same state; `action` entries of chains outside every pair are not
    written; a beta stride of 0 (one beta for all) exchanges every pair."""
    from l2hmc_amd import _lib
    T, X, G, ng = 6, 6, 5, 3
    x, betas, labels, _ = _input(T, X, G, ng)
    B = G * ng
    bd = torch.as_tensor(betas, device="cuda")
    ref = _round(ops, x, betas, labels, T, X, G, 1)
    xd = torch.as_tensor(x, device="cuda").clone()
    _lib.call("l2hmc_gauge_replica_swap", T, X, xd, B, G, 1, bd, 1, SEED, STREAM, None, None, None, None)
    assert torch.equal(xd, ref[0])
    act = torch.full((B,), -3.0, device="cuda")
    xd = torch.as_tensor(x, device="cuda").clone()
    _lib.call("l2hmc_gauge_replica_swap", T, X, xd, B, G, 1, bd, 1, SEED, STREAM, None, act, None, None)
    assert torch.equal(xd, ref[0])
    assert (act[0::G] == -3.0).all() and torch.equal(act[1:G], ref[4][1:G])          # chain 0 of a group sits out
    xd = torch.as_tensor(x, device="cuda").clone()
    p, sw, _ = replica_swap(xd, T, X, G, 0, bd[:1], SEED, STREAM, chain_stride=0)
    low = R.lower_chains(B, G, 0)
    assert (p[low] == 1.0).all() and sw[low].all() and int(sw.sum()) == low.size
    # group 2, parity 1 through the C entry: the outputs are filled, nothing else is touched
    pp, ss = torch.zeros(4, device="cuda"), torch.ones(4, dtype=torch.uint8, device="cuda")
    xd = torch.as_tensor(x[:4], device="cuda").clone()
    _lib.call("l2hmc_gauge_replica_swap", T, X, xd, 4, 2, 1, bd, 1, SEED, STREAM, None, None, pp, ss)
    assert torch.isnan(pp).all() and not ss.any() and np.array_equal(xd.cpu().numpy(), x[:4])


def test_rows_that_are_not_16_byte_aligned(ops):
    """x at an address that is 8 modulo 16: the exchange takes its 4-byte path and gives the same bits."""
    T, X, G, ng = 8, 8, 4, 2
    x, betas, labels, _ = _input(T, X, G, ng)
    B, D = x.shape
    ref = _round(ops, x, betas, labels, T, X, G, 0)
    buf = torch.empty(B * D + 4, device="cuda")
    off = 2 if buf.data_ptr() % 16 == 0 else 0
    xd = buf[off:off + B * D].view(B, D)
    assert xd.data_ptr() % 16 == 8
    xd.copy_(torch.as_tensor(x, device="cuda"))
    p, sw, act = replica_swap(xd, T, X, G, 0, torch.as_tensor(betas, device="cuda"), SEED, STREAM)
    assert torch.equal(xd, ref[0]) and torch.equal(sw, ref[3]) and torch.equal(_bits(p), _bits(ref[2]))
    assert bool(sw.any())
