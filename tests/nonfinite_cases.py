"""Case table, inputs and references of tests/test_gpu_nonfinite.py: a chain that holds an inf or a NaN, in every
reference-mode sampling kernel (its sibling for links far outside [0, 2 pi) is tests/unwrapped_cases.py).  Importable
without a GPU; tests/test_nonfinite_host.py proves the conditions below on the NumPy oracle alone.

A poisoned chain.  The oracle (oracle/gauge_dynamics.py, oracle/dynamics.py) is chain-local and does ordinary IEEE
arithmetic on a NaN: its relu is np.maximum, which hands a NaN on, so one NaN in a network input makes every hidden unit
and with it every S, T and Q of the row NaN: the chain comes back NaN in EVERY link, with p = 0, and no other chain moves
a bit.  A relu that drops a NaN (fmaxf: IEEE maxNum) keeps the hidden layer finite and the NaN then spreads only through
the element-wise arithmetic and the force's stencil: `relu_drops_nan()` swaps that relu into the oracle, and the host
test shows that every case marked `pattern` tells the two apart.  N is 1, 2 or 3 for the network cases: at N = 10 the
stencil alone has reached all 128 links and the case cannot discriminate.  The plain-HMC cases have no network: there
the oracle's pattern after N steps is itself a strict subset of the links (the stencil's reach), which is the sharp
check; the toy cases use a Gaussian with DIAGONAL covariance, whose force does not couple the coordinates.

Kinds of poison (chain `bad`): "inf" / "nanx": a link that the forward direction's first position sub-update moves
(mask 0 in row 0) holds inf / NaN; "nanv": momentum component 5 (toy: 1) of both directions is NaN, for the entries
that take their momenta as arguments.  The benign twin of a call has the bad chain replaced by its neighbour's values.
"""
import collections
import contextlib
import functools

import numpy as np

from oracle import dynamics as od
from oracle import lattice as olat
from oracle import nets as onets
from oracle.gauge_dynamics import GaugeDynamicsOracle, make_masks
from tests import helpers as H
from tests import hmc_geometry_cases as G
from tests import philox_ref

HOST_CUS = 256
TWO_PI = 2 * np.pi
SEED, DRAWS = 11, 40                 # step entries: the dynamics' Philox seed and draw counter (draw index DRAWS // 2)
KINDS_APPLY = ("inf", "nanx", "nanv")
KINDS_STEP = ("inf", "nanx")

# name; family (the kernel the case is there for); entry: "apply" = apply_transition with every draw injected, "step" =
# GaugeSampler.step and apply_transition on the library's own draws; arch; lattice; N, eps, beta; chains (0: from the
# launch plan, `chains()`); the bad chains (negative: from the end); both directions; dynamics attributes; pattern: the
# case tells np.maximum from a NaN-dropping relu (False: an isolation case, or one whose pattern no relu decides)
Case = collections.namedtuple("Case", "name family entry arch T X N eps beta B bad both flags pattern")


def case(name, family, entry, B=19, bad=(3,), arch="generic", T=8, X=8, N=3, eps=0.2, beta=2.0, both=True, pattern=True,
       **flags):
    return Case(name, family, entry, arch, T, X, N, eps, beta, B, tuple(bad), both, tuple(sorted(flags.items())), pattern)


T16 = dict(tiles16_only=True)
LATTICE_CASES = [
    # ---- whole-step kernel, GenericNet 8x8 (fused_traj.hip / fused_traj4.hip / fused_traj32.hip) -----------------------
    case("rows16-b19", "16-row", "apply", **T16),
    case("rows16-b19-n1", "16-row", "apply", N=1, **T16),
    case("rows16-b130", "16-row", "apply", B=130, bad=(3, 129), **T16),
    case("rows16-selected", "16-row", "apply", both=False, **T16),
    case("rows16-single-kicks", "16-row", "apply", single_kicks=True, **T16),
    case("rows16-4x16", "16-row", "apply", T=4, X=16, **T16),
    case("subtile-b19", "sub-tile", "apply"),
    case("subtile-b19-n1", "sub-tile", "apply", N=1),
    case("step-subtile-b19", "sub-tile", "step"),
    case("step-split-heads", "split", "step", **T16),
    case("step-split-heads-b130", "split", "step", B=130, bad=(3, 129), **T16),
    case("step-split-all-columns", "split", "step", all_columns=True, **T16),
    case("step-split-full-l1", "split", "step", full_l1=True, **T16),
    case("step-split-single-kicks", "split", "step", single_kicks=True, **T16),
    case("step-rows16-per-row", "16-row", "step", both=False, **T16),
    case("step-rows32", "32-row", "step", B=0, bad=(3, -1), N=1),
    case("step-ladder", "ladder", "step", B=21, bad=(4,), beta=(1.0, 2.0, 3.0)),
    case("step-ladder-rows16", "ladder", "step", B=21, bad=(4,), beta=(1.0, 2.0, 3.0), **T16),
    # ---- ConvNet3D: the whole-step kernel (8x8, F = 8) and the layered path (conv3d_front.hip + the dense kernels) ----
    case("conv-whole-step", "conv3d whole-step", "apply", arch="conv3D", N=2),
    case("conv-whole-step-selected", "conv3d whole-step", "apply", arch="conv3D", N=2, both=False),
    case("conv-step", "conv3d whole-step", "step", arch="conv3D", N=2),
    case("conv-layered", "conv3d layered", "apply", arch="conv3D", N=2, fused=False),
    case("conv-layered-4x16", "conv3d layered", "apply", arch="conv3D", T=4, X=16, N=2, B=9),
    # ---- the layered path (stq_dense.hip + leapfrog.hip) ---------------------------------------------------------
    case("layered-8x8", "layered", "apply", fused=False),
    case("layered-8x8-all-columns", "layered", "apply", fused=False, all_columns=True),
    case("layered-4x4", "layered", "apply", T=4, X=4),
    case("layered-4x4-all-columns", "layered", "apply", T=4, X=4, all_columns=True),
    case("layered-6x6", "layered", "apply", T=6, X=6),
    case("layered-6x6-all-columns", "layered", "apply", T=6, X=6, all_columns=True),
]
# ---- plain HMC (hmc_step.hip): one lattice per threads-per-row value 2^tsh of tests/hmc_geometry_cases.py, the batch of
# its both-directions case (a full workgroup and a chain: below tsh 6 the bad chain shares its wave with others), and
# 8x8, the lattice of the whole-step kernels.  No network: pattern = the stencil's reach, decided by no relu.
HMC_LATTICES = [(1, 1), (1, 2), (2, 2), (2, 4), (4, 4), (4, 8), (8, 8), (7, 9), (8, 16), (16, 16)]
_GEO = {(c.T, c.X): c for c in G.CASES}
for _T, _X in HMC_LATTICES:
    _B = _GEO[(_T, _X)].B if (_T, _X) in _GEO else 9
    for _entry in ("apply", "step"):
        LATTICE_CASES.append(case(f"hmc-{_entry}-{_T}x{_X}", "plain HMC", _entry, arch="hmc", T=_T, X=_X, B=_B, bad=(1,),
                                eps=0.1, pattern=False))
LATTICE_CASES.append(case("hmc-apply-8x8-selected", "plain HMC", "apply", arch="hmc", B=9, bad=(1,), eps=0.1, both=False,
                        pattern=False))
assert sorted({G.geom(T, X)[1] for T, X in HMC_LATTICES}) == sorted({G.geom(c.T, c.X)[1] for c in G.CASES})
HMC_RUN_STEPS = 3
HMC_RUN_LATTICES = [(2, 2), (4, 8), (8, 8), (16, 16)]

BY_NAME = {c.name: c for c in LATTICE_CASES}
assert len(BY_NAME) == len(LATTICE_CASES)
FAMILIES = ("16-row", "sub-tile", "32-row", "split", "ladder", "conv3d whole-step", "conv3d layered", "layered",
            "plain HMC", "toy")


def kinds(c):
    return KINDS_APPLY if c.entry == "apply" else KINDS_STEP


def step_plan(rows, cus):
    """l2hmc_gauge_step_plan (host logic only) -> [(rows, rows per workgroup), ...]."""
    import ctypes as C
    from l2hmc_amd import _lib
    rows_out, rpw = (C.c_int64 * 3)(), (C.c_int * 3)()
    n = _lib.lib().l2hmc_gauge_step_plan(rows, cus, rows_out, rpw)
    assert 1 <= n <= 3, n
    return [(int(rows_out[i]), int(rpw[i])) for i in range(n)]


@functools.lru_cache(maxsize=None)
def smallest_32_row_batch(cus):
    """The smallest batch of both-directions chains of which launch_fused_step gives a 32-row launch, from the plan query."""
    B = 8 * cus + 1
    while not any(w == 32 for _, w in step_plan(2 * B, cus)):
        B += 1
        assert B <= 64 * cus
    return B


def chains(c, cus=HOST_CUS):
    return c.B if c.B else smallest_32_row_batch(cus)


def bad_chains(c, cus=HOST_CUS):
    B = chains(c, cus)
    return tuple(b % B for b in c.bad)


def dim(c):
    return 2 * c.T * c.X


def masks(c):
    return make_masks(c.N, dim(c), np.random.RandomState(42))       # tests/helpers.py::gauge_oracle


@functools.lru_cache(maxsize=None)
def weights(c):
    if c.arch == "hmc":
        return None, None
    if c.arch == "conv3D":
        return H.conv_weights(c.T, c.X, regime="mild")
    return H.gauge_weights(c.T, c.X, regime="mild")


def moved_link(c):
    """A link that the first position sub-update of a forward row moves."""
    return int(np.flatnonzero(masks(c)[0] == 0)[0])


def betas(c, B):
    """None, or the ladder of a case whose beta is a tuple of rungs: chain i on rung i % len."""
    if not isinstance(c.beta, tuple):
        return None
    return np.asarray([c.beta[i % len(c.beta)] for i in range(B)], dtype=np.float32)


def beta_of(c, chain):
    return c.beta[chain % len(c.beta)] if isinstance(c.beta, tuple) else c.beta


def clean_inputs(c, cus=HOST_CUS, draws=None):
    """[x, v0f, v0b, coin, u] in float32.  "apply": tests/helpers.py::gauge_inputs.  "step": the same start, and the
    draws the step takes for itself, from `draws(B, D)` (the GPU test: the library's generators) or restated on the host
    (tests/philox_ref.py) for the given rows only."""
    B, D = chains(c, cus), dim(c)
    x, v0f, v0b, coin, u = H.gauge_inputs(B, D)
    if c.arch == "hmc":
        x = np.mod(np.random.default_rng(5).normal(0.0, G.START, (B, D)), TWO_PI)
    if c.entry == "step":
        v0f, v0b, coin, u = draws(B, D)
    return [np.asarray(a, dtype=np.float32) for a in (x, v0f, v0b, coin, u)]


def host_step_draws(rows):
    """-> draws(B, D) that restates the step's Philox draws on the host for `rows` only (the other rows: zeros)."""
    def draws(B, D):
        sv, su = philox_ref.lattice_step_streams(DRAWS // 2)
        V = np.zeros((2, B, D))
        cu = philox_ref.uniform(SEED, su, np.arange(2 * B))
        cols = np.arange(D)
        for r in rows:
            for d in (0, 1):
                V[d, r] = philox_ref.normal(SEED, sv, (d * B + r) * D + cols)
        return V[0], V[1], cu[:B], cu[B:]
    return draws


def poison(c, kind, clean, cus=HOST_CUS):
    """(inputs with the bad chains poisoned, inputs with them replaced by their neighbours' values)."""
    bad, benign = [a.copy() for a in clean], [a.copy() for a in clean]
    B = clean[0].shape[0]
    for b in bad_chains(c, cus):
        if kind == "nanv":
            assert c.entry == "apply"
            bad[1][b, min(5, dim(c) - 1)] = np.nan
            bad[2][b, min(5, dim(c) - 1)] = np.nan
        else:
            bad[0][b, moved_link(c)] = np.inf if kind == "inf" else np.nan
        twin = b + 1 if b + 1 < B else b - 1
        for a in benign[:3] if c.entry == "apply" else benign[:1]:     # (a step's draws belong to the chain's place)
            a[b] = a[twin]
    return bad, benign


@contextlib.contextmanager
def relu_drops_nan():
    """The oracle with the relu of fmaxf(h, 0): a NaN pre-activation gives 0."""
    keep = onets._relu
    onets._relu = lambda a: np.fmax(a, 0)
    try:
        yield
    finally:
        onets._relu = keep


def oracle(c, dtype=np.float32):
    xp, vp = weights(c)
    arch = "generic" if c.arch == "hmc" else c.arch
    return GaugeDynamicsOracle(c.T, c.X, c.N, c.eps, masks(c), xp, vp, arch, hmc=c.arch == "hmc", dtype=dtype)


APPLY_NAMES = ("x_prop", "v_prop", "p", "x_out")
STEP_NAMES = APPLY_NAMES + ("x_next", "action", "avg_plaq", "top_charge", "dq")


def reference(c, inputs, rows, dtype=np.float32):
    """The oracle's outputs for the chains `rows` of a call (it is chain-local: tests/test_nonfinite_host.py), in
    `dtype`: apply_transition's four and, for a step entry, x_next = np.mod(x_out, 2 pi), the observables of the step's
    INPUT and |dQ| between input and output (gauge_model.py:256-266, :718-725, :1388)."""
    rows = np.asarray(rows)
    x, v0f, v0b, coin, u = (np.asarray(a)[rows].astype(dtype) for a in inputs)
    out = {}
    with np.errstate(all="ignore"):
        groups = {}
        for i, r in enumerate(rows):
            groups.setdefault(beta_of(c, int(r)), []).append(i)
        parts = {}
        for beta, idx in groups.items():
            res = oracle(c, dtype).apply_transition(x[idx], beta, v0f[idx], v0b[idx], coin[idx], u[idx])
            for k, a in zip(APPLY_NAMES, res):
                parts.setdefault(k, {})[beta] = (idx, np.asarray(a))
        for k, by_beta in parts.items():
            first = next(iter(by_beta.values()))[1]
            full = np.empty((len(rows),) + first.shape[1:], dtype=first.dtype)
            for idx, a in by_beta.values():
                full[idx] = a
            out[k] = full
        if c.entry == "step":
            out["x_next"] = np.mod(out["x_out"], dtype(TWO_PI))
            out["action"] = olat.total_action(x, c.T, c.X)
            out["avg_plaq"] = olat.avg_plaq(x, c.T, c.X)
            out["top_charge"] = olat.top_charge(x, c.T, c.X)
            out["dq"] = olat.top_charge_diff(x, out["x_out"], c.T, c.X)
    return out


def nan_counts(ref, i=0):
    return {k: int(np.isnan(np.atleast_1d(ref[k][i])).sum()) for k in ref}


# ---- toy targets (small_mlp.hip, small_mlp.h) ----------------------------------------------------------------------
# dim, hidden units, leapfrog steps; a Gaussian with diagonal covariance; batches of tests/toy_cases.py
ToyCase = collections.namedtuple("ToyCase", "dim H N")
TOY_CASES = [ToyCase(4, 16, 1), ToyCase(8, 64, 1)]
TOY_BATCHES = (37, 1)
TOY_BAD = 3
TOY_EPS = 0.1


def toy_id(c):
    return f"d{c.dim}-H{c.H}-N{c.N}"


@functools.lru_cache(maxsize=None)
def toy_arrays(c):
    rng = np.random.default_rng(1000 * c.dim + c.H)
    return rng.uniform(-1., 1., c.dim), np.diag(rng.uniform(0.05, 0.3, c.dim))


def toy_nets(c):
    xp, vp = H.mlp_weights(c.dim, c.H, seed=107, regime="mild")
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # noqa: E731
    return {k: f32(v) for k, v in xp.items()}, {k: f32(v) for k, v in vp.items()}


def toy_masks(c):
    return od.make_masks(c.N, c.dim, np.random.RandomState(6))


def toy_oracle(c, dtype=np.float32):
    mu, cov = toy_arrays(c)
    xp, vp = toy_nets(c)
    return od.DynamicsOracle(c.dim, od.Gaussian(mu, cov), c.N, TOY_EPS, toy_masks(c), xp, vp, dtype=dtype)


def toy_inputs(c, B):
    """dict x, v0f, v0b, bits (1 = forward), u in float32-representable float64."""
    mu, cov = toy_arrays(c)
    rng = np.random.default_rng(100 + B)
    f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)      # noqa: E731
    x = f32(mu + rng.standard_normal((B, c.dim)) * np.sqrt(np.diag(cov)))
    bits = rng.integers(0, 2, B).astype(np.float64)
    if B > 1:
        bits[:2] = (1., 0.)
    return dict(x=x, v0f=f32(rng.standard_normal((B, c.dim))), v0b=f32(rng.standard_normal((B, c.dim))), bits=bits,
                u=f32(rng.uniform(0.01, 1.0, B)))


def toy_bad(B):
    return min(TOY_BAD, B - 1)


def toy_poison(c, kind, clean):
    B = clean["x"].shape[0]
    b = toy_bad(B)
    bad = {k: v.copy() for k, v in clean.items()}
    benign = {k: v.copy() for k, v in clean.items()}
    if kind == "nanv":
        bad["v0f"][b, 1] = bad["v0b"][b, 1] = np.nan
    else:
        bad["x"][b, 1] = np.inf if kind == "inf" else np.nan
    for k in ("x", "v0f", "v0b"):
        benign[k][b] = benign[k][b - 1] if B > 1 else 0.25
    return bad, benign


TOY_NAMES = ("Xf", "Vf", "pf", "Xb", "Vb", "pb", "Lx", "Lv", "px", "x_out")


def toy_reference(c, i, dtype=np.float32):
    orc = toy_oracle(c, dtype)
    out = {}
    with np.errstate(all="ignore"):
        out["Xf"], out["Vf"], out["pf"] = orc.forward(i["x"], i["v0f"])
        out["Xb"], out["Vb"], out["pb"] = orc.backward(i["x"], i["v0b"])
        Lx, _, px, outs, Lv = od.propose(i["x"], orc, i["v0f"], i["v0b"], i["bits"], u=i["u"].astype(dtype),
                                         do_mh_step=True)
    out.update(Lx=Lx, Lv=Lv, px=px, x_out=outs[0])
    return {k: np.asarray(v) for k, v in out.items()}


# ---- the toy run (l2hmc_small_run, `DynamicsSampler.run`): the chains stay in registers over the steps of one launch ----
# The run takes its own draws, so only a coordinate can be poisoned ("inf", "nanx").  Whatever the relu does, the
# proposal of such a chain is NaN in every coordinate, p = 0 and the chain is rejected in every step: the run cases are
# isolation cases -- the other chains keep their bits in every step, the bad chain keeps its input's bits and p = 0.
TOY_RUN_STEPS, TOY_RUN_DRAWS = 3, 20


def toy_host_draws(B, dim):
    """s -> (direction uniforms, forward momenta, backward momenta, MH uniforms) of step s of the run, restated on the host
    (tests/philox_ref.py::toy_step: streams TOY_RUN_DRAWS + 4 s + 0 .. 3 of seed SEED)."""
    return lambda s: philox_ref.toy_step(SEED, TOY_RUN_DRAWS, s, B, dim)


def toy_run_reference(c, x, draws, steps=TOY_RUN_STEPS, dtype=np.float32):
    """The oracle's run (utils/sampler.py:28-59 with the MH step, a chain forward iff its direction uniform >= 0.5) ->
    (px [steps, B], samples [steps, B, dim] with samples[s] the output of step s)."""
    orc = toy_oracle(c, dtype)
    x = np.asarray(x, dtype=dtype)
    px, samples = [], []
    with np.errstate(all="ignore"):
        for s in range(steps):
            du, v0f, v0b, u = draws(s)
            bits = (np.asarray(du) >= 0.5).astype(np.float64)
            _, _, p, outs, _ = od.propose(x, orc, np.asarray(v0f, dtype=dtype), np.asarray(v0b, dtype=dtype), bits,
                                          u=np.asarray(u, dtype=dtype), do_mh_step=True)
            x = np.asarray(outs[0], dtype=dtype)
            px.append(np.asarray(p))
            samples.append(x)
    return np.stack(px), np.stack(samples)


# ---- comparison of a poisoned chain's outputs with the reference's ---------------------------------------------------
def same_pattern(got, want):
    """NaN exactly where the reference has NaN, inf (of its sign) exactly where it has inf."""
    got, want = np.asarray(got), np.asarray(want)
    return bool(np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want))
                and np.array_equal(np.isneginf(got), np.isneginf(want)))
