"""Operations whose result must not depend on what their workspace holds on entry, in one place for
tests/test_workspace_cases_host.py (which checks the table against the header and the package without a GPU) and
tests/test_gpu_workspace_state.py (which runs it).  Importing this module touches neither the library nor the device.

The contract (include/l2hmc_hip.h, Conventions): a workspace's content on entry is arbitrary and is not preserved; only
the documented ticket words of step_sums must be zero on entry, and they are left at zero.  The package hands one
grow-only buffer (`_lib.Workspace`) to whichever entry comes next, so an entry normally finds there what the same call
on the same inputs left -- the right bytes.  `poisoned` takes that away: every `_lib.Workspace.get` returns ONE shared
buffer (`SharedWorkspace`), filled with a byte pattern on every call, or left as the previous operation left it.

An operation (`Op`) names what it covers and builds, on the device, an object with `run(ws) -> {name: tensor}`:
  - package-level operations go through the package's classes and reach the buffer through the patched `get`;
  - C-level operations call their entry with `ws.get(...)` themselves: the whole-step forms (`StepForm`, which the
    capture tests also drive), the plain-HMC runs, and the three entries whose package call sites allocate a workspace
    with a bare torch.empty (l2hmc_amd/autograd.py, autograd_toy.py, torch_ops.py).
A train_forward / train_backward pair shares one workspace (the tape): the pattern is laid before the forward only.

Shapes are the smallest that select each path; every operation is bit-reproducible with itself (the control of
tests/test_gpu_workspace_state.py::test_content_independence), so none takes the float64 route."""
import collections
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np

PATTERNS = (0x00, 0xFF, 0x7F)      # zeros; every float a NaN and every int -1; floats 3.39e38 and ints large positive
N_LF, EPS, BETA, SEED, DRAW = 3, 0.1, 2.0, 42, 7
TWO_PI = 2 * np.pi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the poisoning helper ------------------------------------------------------------------------------------------
class SharedWorkspace:
    """One grow-only byte buffer standing in for every workspace.  `pattern`: a byte laid over the WHOLE buffer on
    every `get`, or None = leave what the last user left."""

    def __init__(self, pattern=None):
        self.buf, self.pattern, self.gets = None, pattern, 0

    def get(self, nbytes, device):
        import torch
        device = torch.device(device)
        n = max(int(nbytes), 256)
        if self.buf is None or self.buf.numel() < n or self.buf.device != device:
            self.buf = torch.empty(n, dtype=torch.uint8, device=device)
        if self.pattern is not None:
            self.buf.fill_(self.pattern)
        self.gets += 1
        return self.buf.data_ptr(), self.buf.numel()


@contextlib.contextmanager
def poisoned(monkeypatch, pattern, shared=None):
    """Inside the block every `_lib.Workspace.get` of the package returns `shared` (a new SharedWorkspace by default)
    with `pattern` laid over it; -> shared.  C-level operations take the same object."""
    from l2hmc_amd import _lib
    shared = SharedWorkspace() if shared is None else shared
    shared.pattern = pattern
    with monkeypatch.context() as m:
        m.setattr(_lib.Workspace, "get", lambda self, nbytes, device: shared.get(nbytes, device))
        yield shared


# ---- host logic: the cut batch -------------------------------------------------------------------------------------
def step_plan(rows, cus):
    """l2hmc_gauge_step_plan -> [(rows, rows per workgroup), ...] (host logic only)."""
    from l2hmc_amd import _lib
    rows_out, rpw = (C.c_int64 * 3)(), (C.c_int32 * 3)()
    n = _lib.lib().l2hmc_gauge_step_plan(rows, cus, rows_out, rpw)
    return [(int(rows_out[i]), int(rpw[i])) for i in range(n)]


def is_cut_in_three(parts):
    return len(parts) == 3 and parts[0][1] == 32 and parts[1][1] == 16 and parts[2][1] in (4, 8, 12)


@functools.lru_cache(maxsize=None)
def cut_batch_chains(cus):
    """The smallest both-directions batch that `launch_fused_step` cuts into a 32-row part, a 16-row part and a
    sub-tile part on a device with `cus` compute units."""
    for B in range(1, 1 << 16):
        if is_cut_in_three(step_plan(2 * B, cus)):
            return B
    raise AssertionError(f"no batch below 65536 chains is cut in three on {cus} CUs")


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


# ---- builders ------------------------------------------------------------------------------------------------------
def _dev(a, dtype=None):
    import torch
    return torch.as_tensor(np.asarray(a), dtype=dtype or torch.float32).to("cuda").contiguous()


@functools.lru_cache(maxsize=None)
def _gauge(T, X, arch="generic", both=True, fused=True, tiles16=False, hmc=False, N=N_LF, eps=EPS):
    """A GaugeDynamics with the weights of the parity tests (tests/helpers.py, "mild")."""
    from tests import helpers as H
    if hmc:
        xp = vp = None
    else:
        xp, vp = (H.conv_weights if arch == "conv3D" else H.gauge_weights)(T, X, regime="mild")
    orc = H.gauge_oracle(T, X, N, eps, xp, vp, hmc=hmc, arch=arch)
    dyn = H.gauge_hip(T, X, N, eps, xp, vp, orc.mask, 8, hmc=hmc, both_directions=both, arch=arch)
    dyn.fused = fused
    dyn.tiles16_only = tiles16
    return dyn


@functools.lru_cache(maxsize=None)
def _periodic(T, X, whole_step):
    from tests.test_gpu_periodic import _hip
    return _hip(T, X, N_LF, 0.15, 8, "mild", whole_step=whole_step)[0]


def _x0(B, D, seed=3):
    """A hot start, uniform on [0, 2 pi): at the weights and step size used here the float64 reference accepts between
    a fifth and two fifths of such chains, so a step both accepts and rejects (a near-cold start is no use: wrapped, its
    links sit at both ends of [0, 2 pi), the networks read raw angles, and every proposal is rejected)."""
    return _dev(np.random.default_rng(seed + B).uniform(0, TWO_PI, (B, D)).astype(np.float32))


class StepForm:
    """l2hmc_gauge_mcmc_step_ex (or _ladder) on one plan and batch, with a workspace the caller hands in.  `sums` is
    zeroed ONCE, here: every call must leave its ticket word at 0 for the next."""
    OUTS = ("px", "actions", "plaqs", "charges", "dq")

    def __init__(self, dyn, B, ladder=False):
        import torch
        from l2hmc_amd import _lib
        self.dyn, self.B, self.D, self.ladder = dyn, int(B), int(dyn.x_dim), ladder
        self.plan = dyn._plan()
        self.nbytes = int(_lib.lib().l2hmc_gauge_mcmc_step_ws_bytes(C.byref(self.plan), self.B))
        self.x0 = _x0(self.B, self.D)
        self.betas = _dev(BETA + 0.5 * (np.arange(self.B) % 3)) if ladder else None
        self.sums = torch.zeros(4, dtype=torch.float32, device="cuda")

    def fused(self):
        from l2hmc_amd import _lib
        return _lib.lib().l2hmc_gauge_plan_fused(C.byref(self.plan))

    def outs(self):
        import torch
        return [torch.empty(self.B, dtype=torch.float32, device="cuda") for _ in self.OUTS]

    def call(self, x_in, x_next, outs, ws_ptr, nb, draw=DRAW):
        """Enqueue one step on torch's current stream (x_next may be x_in)."""
        from l2hmc_amd import _lib
        front = (self.betas, 1) if self.ladder else (BETA,)
        _lib.call("l2hmc_gauge_mcmc_step_ladder" if self.ladder else "l2hmc_gauge_mcmc_step_ex", C.byref(self.plan),
                  *front, x_in, x_next, self.B, SEED, draw, *outs, self.sums, ws_ptr, nb)

    def result(self, x_next, outs):
        import torch
        out = {"x": x_next.clone(), "sums": self.sums[:3].clone(), "tickets": self.sums[3:].view(torch.int32).clone()}
        out.update((k, o.clone()) for k, o in zip(self.OUTS, outs))
        return out

    def run(self, ws):
        import torch
        x_next, outs = torch.empty_like(self.x0), self.outs()
        self.call(self.x0, x_next, outs, *ws.get(self.nbytes, "cuda"))
        return self.result(x_next, outs)


def _step(kind, ladder):
    """The whole-step forms of launch_fused_step, the layer-by-layer step and the torus-exact plans."""
    def build():
        if kind == "subtile_b3":
            return StepForm(_gauge(8, 8), 3, ladder)
        if kind in ("split16_b16", "split16_b19"):                  # the 16-row split form, one pair full / two, one ragged
            return StepForm(_gauge(8, 8, tiles16=True), int(kind[-2:]), ladder)
        if kind == "selected_only":
            return StepForm(_gauge(8, 8, both=False, tiles16=True), 19, ladder)
        if kind == "conv3d":
            return StepForm(_gauge(8, 8, arch="conv3D"), 5, ladder)
        if kind == "layered_6x6":
            return StepForm(_gauge(6, 6), 7, ladder)
        if kind == "cut_batch":
            form = StepForm(_gauge(8, 8), cut_batch_chains(device_cus()), ladder)
            assert is_cut_in_three(step_plan(2 * form.B, device_cus()))
            return form
        if kind == "periodic_layered_3x5":
            return StepForm(_periodic(3, 5, False), 7, ladder)
        if kind == "periodic_whole_8x8":
            return StepForm(_periodic(8, 8, True), 19, ladder)
        raise ValueError(kind)
    return build


STEP_KINDS = ("subtile_b3", "split16_b16", "split16_b19", "selected_only", "conv3d", "layered_6x6", "cut_batch",
              "periodic_layered_3x5", "periodic_whole_8x8")
# the forms that take one launch (graph shape: kernel nodes only), and those a capture test replays
ONE_LAUNCH_KINDS = ("subtile_b3", "split16_b16", "split16_b19", "selected_only", "conv3d", "periodic_whole_8x8")
CAPTURED = tuple((k, False) for k in ONE_LAUNCH_KINDS + ("cut_batch",)) + (("split16_b19", True), ("cut_batch", True))


class _Fn:
    def __init__(self, run):
        self.run = run


def _net_call(which):
    def build():
        import torch
        import l2hmc_amd as la
        from tests import helpers as H
        t = torch.tensor([[float(np.float32(np.cos(0.7))), float(np.float32(np.sin(0.7)))]])
        if which == "d128":
            net, D, rows = _gauge(8, 8).position_fn, 128, 19
        elif which == "conv3d":
            net, D, rows = _gauge(8, 8, arch="conv3D").position_fn, 128, 5
        else:                                                    # the any-width path
            D, Hn, rows = 30, 120, 9
            net = la.network(D, "XNet", 2.0, num_nodes=Hn)
            net.load_state(H.mlp_weights(D, Hn, regime="stress", seed=D + Hn)[0])
        rng = np.random.default_rng(D + rows)
        a, b = _dev(rng.standard_normal((rows, D))), _dev(rng.uniform(0, TWO_PI, (rows, D)))
        return _Fn(lambda ws: dict(zip("STQ", net([a, b, t]))))
    return build


def _stq_dense_c():
    """l2hmc_stq_dense itself (the call of l2hmc_amd/torch_ops.py, which allocates its workspace with torch.empty)."""
    import torch
    import l2hmc_amd as la
    from l2hmc_amd import _lib
    from tests import helpers as H
    D, Hn, rows = 30, 120, 9
    net = la.network(D, "XNet", 2.0, num_nodes=Hn)
    net.load_state(H.mlp_weights(D, Hn, regime="stress", seed=D + Hn)[0])
    st = net.pack()
    rng = np.random.default_rng(5)
    a, b = _dev(rng.standard_normal((rows, D))), _dev(rng.standard_normal((rows, D)))
    nbytes = _lib.lib().l2hmc_stq_ws_bytes(rows, st.H)

    def run(ws):
        S, T, Q = (torch.empty(rows, D, device="cuda") for _ in range(3))
        _lib.call("l2hmc_stq_dense", C.byref(st), a, b, None, 0.76, 0.64, rows, S, T, Q, *ws.get(nbytes, "cuda"))
        return {"S": S, "T": T, "Q": Q}
    keep = (net, st)
    return _Fn(lambda ws, keep=keep: run(ws))


def _gauge_paths(T, X, arch, B, fused):
    """One leapfrog step, a backward trajectory and a transition with injected draws through GaugeDynamics."""
    def build():
        from tests import helpers as H
        dyn = _gauge(T, X, arch=arch, fused=fused)
        x, v0f, v0b, coin, u = (_dev(a) for a in H.gauge_inputs(B, 2 * T * X))

        def run(ws):
            out = dict(zip(("lf_x", "lf_v", "lf_logdet"), dyn._lf(x, v0f, BETA, 1, backward=False)))
            out.update(zip(("tr_x", "tr_v", "tr_p", "tr_logdet"),
                           dyn.transition_kernel(x, BETA, forward=False, momentum=v0b, return_logdet=True)))
            out.update(zip(("x_prop", "v_prop", "p", "x_out"),
                           dyn.apply_transition(x, BETA, momentum_f=v0f, momentum_b=v0b, coin=coin, u=u)))
            return out
        return _Fn(run)
    return build


def _hmc_run(entry, T, X):
    """l2hmc_gauge_hmc_run / _ladder / _exchange with step_sums, three steps, on a T x X lattice of
    tests/hmc_geometry_cases.py (B = 9 chains there: one workgroup and a partial one; the exchange takes 10, groups of
    two)."""
    def build():
        import torch
        from l2hmc_amd import _lib
        from tests import hmc_geometry_cases as G
        assert any((c.T, c.X) == (T, X) for c in G.CASES)
        n, B = 3, 10 if entry == "exchange" else 9
        dyn = _gauge(T, X, hmc=True, eps=0.3)
        plan, D = dyn._plan(), 2 * T * X
        x0 = _dev(np.mod(np.random.default_rng(B).normal(0, G.START, (B, D)), TWO_PI).astype(np.float32))
        name = "l2hmc_gauge_hmc_run" + ("" if entry == "run" else "_" + entry)
        nbytes = getattr(_lib.lib(), name + "_ws_bytes")(C.byref(plan), B, n)
        assert nbytes > 0
        sums = torch.zeros(n, 4, device="cuda")                    # zeroed once
        sched = _dev([1.5, 2.0, 2.5])
        ladder = _dev(1.5 + 0.5 * (np.arange(B) % 2))
        eps_chain = _dev(0.25 + 0.1 * (np.arange(B) % 3))

        def run(ws):
            hist = [torch.empty(n, B, device="cuda") for _ in range(5)]
            samples, x_next = torch.empty(n, B, D, device="cuda"), torch.empty_like(x0)
            out = dict(zip(StepForm.OUTS, hist), samples=samples, x=x_next)
            wsp = ws.get(nbytes, "cuda")
            if entry == "run":
                _lib.call(name, C.byref(plan), sched, x0, x_next, B, SEED, DRAW, n, *hist, sums, samples, *wsp)
            elif entry == "ladder":
                _lib.call(name, C.byref(plan), ladder, 0, 1, eps_chain, x0, x_next, B, SEED, DRAW, n, *hist, sums,
                          samples, *wsp)
            else:
                replica = torch.arange(B, dtype=torch.int32, device="cuda")          # read on entry, written on exit
                rounds = [torch.empty(n, B, device="cuda"), torch.empty(n, B, dtype=torch.uint8, device="cuda"),
                          torch.empty(n, B, dtype=torch.int32, device="cuda")]
                _lib.call(name, C.byref(plan), ladder, 0, 1, None, x0, x_next, B, SEED, DRAW, n, 2, 1, 0, 0, replica,
                          *hist, sums, samples, *rounds, *wsp)
                out.update(replica=replica, swap_p=rounds[0], swapped=rounds[1], replica_hist=rounds[2])
            out.update(sums=sums[:, :3].clone(), tickets=sums[:, 3].contiguous().view(torch.int32).clone())
            return out
        keep = (dyn, plan)
        return _Fn(lambda ws, keep=keep: run(ws))
    return build


def _gauge_trainer(kind):
    """GaugeTrainer.calc_loss_and_grads (the loss and reverse pass of a training step; Adam takes no workspace)."""
    def build():
        from l2hmc_amd.gauge_trainer import GaugeTrainer
        T, X, arch, B, N = {"fused": (8, 8, "generic", 5, 2), "tiled": (4, 4, "generic", 9, 2),
                            "walk_3x5": (3, 5, "generic", 7, 2), "conv3d": (8, 8, "conv3D", 5, 2),
                            "ladder": (8, 8, "generic", 5, 2)}[kind]
        from tests import helpers as H
        xp, vp = (H.conv_weights if arch == "conv3D" else H.gauge_weights)(T, X, regime="mild")
        orc = H.gauge_oracle(T, X, N, EPS, xp, vp, arch=arch)
        tr = GaugeTrainer(H.gauge_hip(T, X, N, EPS, xp, vp, orc.mask, B, arch=arch), lr_init=1e-3)
        assert tr._use_layered() == (kind == "walk_3x5")
        D = 2 * T * X
        rng = np.random.default_rng(7)
        x, z = rng.uniform(0, TWO_PI, (B, D)), rng.standard_normal((B, D))
        mk = lambda: (rng.standard_normal((B, D)), rng.standard_normal((B, D)), rng.uniform(size=B),   # noqa: E731
                      rng.uniform(size=B))
        dx, dz = mk(), mk()
        beta = _dev(2.0 + 0.5 * (np.arange(B) % 3)) if kind == "ladder" else 2.5

        def run(ws):
            loss, x_out, px, x_dq = tr.calc_loss_and_grads(x, beta, z=z, draws_x=dx, draws_z=dz)
            return {"loss": loss.reshape(1), "x_out": x_out, "px": px, "x_dq": x_dq, "grads": tr.grads.clone(),
                    "terms": tr.last_loss_terms.clone()}
        return _Fn(run)
    return build


def _dynamics_trainer(kind):
    """DynamicsTrainer.calc_loss_and_grads: the one-launch form, the layer-by-layer form, and the layer-by-layer form
    in the split-k regime of tests/test_gpu_train_layered.py::test_split_k_regime_matches_float64_and_is_reproducible
    at its smallest batch: 2 * 10 * 2 * 1640 = 65600 taped rows per network, so every weight-gradient product of
    l2hmc_dense_weight_grads runs split-k and its column sums run in 512 chunks, as there."""
    def build():
        from tests.test_gpu_train_layered import _colsum_chunks, _setup, _tn_splits
        if kind == "one_launch":
            tr, _, x, z, dx, dz = _setup("mog", 50, 5, 0.1, 37, "stress")
            assert not tr.dynamics.layered
        elif kind == "layered":
            tr, _, x, z, dx, dz = _setup("mog", 50, 5, 0.1, 37, "stress", force_layered=True)
        else:
            B, N, Hn = 1640, 10, 100
            R = 2 * N * 2 * B
            assert _tn_splits(Hn, 2 * 50, R) > 1 and _tn_splits(Hn, Hn, R) > 1 and _tn_splits(150, Hn, R) > 1
            assert _colsum_chunks(R) == 512
            tr, _, x, z, dx, dz = _setup("icg50", Hn, N, 0.02, B, "mild")
            assert tr.dynamics.layered

        def run(ws):
            loss, x_out, px = tr.calc_loss_and_grads(x, z=z, draws_x=dx, draws_z=dz)
            return {"loss": loss.reshape(1), "x_out": x_out, "px": px, "grads": tr.grads.clone(),
                    "terms": tr.last_terms.clone()}
        return _Fn(run)
    return build


def _toy_vjp():
    """l2hmc_small_vjp (the call of l2hmc_amd/autograd_toy.py, which allocates its workspace with torch.empty), on the
    rows of tests/test_gpu_autograd_toy.py::test_vjp_entry_matches_float64."""
    import torch
    from l2hmc_amd import _lib, autograd_toy
    from tests.test_gpu_autograd_toy import _setup
    dyn = _setup("mog", 50, 4, 0.1, 37, "stress")[0]
    R, D = 37, 2
    rng = np.random.default_rng(23)
    xt, vt = _dev(rng.normal(0.5, 0.4, (R, D))), _dev(rng.standard_normal((R, D)))
    dt = _dev((rng.uniform(size=R) < 0.5).astype(np.int32), torch.int32)
    gs = [_dev(rng.standard_normal(s)) for s in ((R, D), (R, D), (R,), (R,))]
    plan = dyn._plan()
    n_grads = sum(t.numel() for n in (dyn.XNet, dyn.VNet) for t in autograd_toy._segments(n).values()) + 1
    nbytes = _lib.lib().l2hmc_small_train_ws_bytes(C.byref(plan), R)

    def run(ws, keep=(dyn, plan)):
        grads = torch.full((n_grads,), 7., device="cuda")
        outs = [torch.full((R, D), 7., device="cuda") for _ in range(4)] + [torch.full((R,), 7., device="cuda")
                                                                             for _ in range(2)]
        _lib.call("l2hmc_small_vjp", C.byref(plan), xt, vt, dt, R, *gs, outs[0], outs[1], grads, *outs[2:],
                  *ws.get(nbytes, "cuda"))
        return dict(zip(("dx0", "dv0", "X", "V", "logdet", "p"), outs), grads=grads)
    return _Fn(run)


def _gauge_train_c():
    """l2hmc_gauge_train_forward + l2hmc_gauge_train_backward (the calls of l2hmc_amd/autograd.py, which allocates
    their workspace with torch.empty), as tests/test_gpu_autograd.py::test_plumbing_is_exact drives them.  The pair
    shares the workspace: the pattern is laid before the forward."""
    import torch
    from l2hmc_amd import _lib
    from tests import helpers as H
    dyn, B, D = _gauge(8, 8, N=2), 24, 128
    rng = np.random.default_rng(3)
    xt, v0 = _dev(rng.uniform(0, TWO_PI, (B, D))), _dev(rng.standard_normal((B, D)))
    dirs = _dev((rng.uniform(size=B) < 0.5).astype(np.int32), torch.int32)
    c1, c2 = _dev(rng.standard_normal((B, D))), _dev(rng.standard_normal((B, D)))
    plan = dyn._plan()
    nbytes = _lib.lib().l2hmc_gauge_train_ws_bytes(C.byref(plan), B)

    def run(ws, keep=(dyn, plan)):
        wsp = ws.get(nbytes, "cuda")
        xN, vN = torch.empty_like(xt), torch.empty_like(xt)
        sld, p = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        _lib.call("l2hmc_gauge_train_forward", C.byref(plan), BETA, xt, v0, dirs, B, xN, vN, sld, p, *wsp)
        grads = [{k: torch.full_like(net._packed[1][k], 7.) for k in net.SEGMENTS}
                 for net in (dyn.position_fn, dyn.momentum_fn)]
        structs = [_lib.DenseGrads(**{k: v.data_ptr() for k, v in g.items()}) for g in grads]
        dxN, dvN, dld, deps = c1.clone(), c2.clone(), torch.zeros(B, device="cuda"), torch.full((1,), 7., device="cuda")
        _lib.call("l2hmc_gauge_train_backward", C.byref(plan), BETA, dirs, B, dxN, dvN, dld, C.byref(structs[0]),
                  C.byref(structs[1]), None, None, deps, *wsp)
        out = {"xN": xN, "vN": vN, "logdet": sld, "p": p, "dx0": dxN, "dv0": dvN, "deps": deps}
        for name, g in zip(("gx", "gv"), grads):
            out.update((f"{name}.{k}", v) for k, v in g.items())
        return out
    assert H is not None
    return _Fn(run)


# ---- the table -----------------------------------------------------------------------------------------------------
# name; the *_ws_bytes queries whose workspace it fills; the package modules whose _lib.Workspace it reaches; build;
# stale_from = the operation (another one, with a larger batch) that uses the shared buffer right before it in the
# "last used by a different operation" run.  The cut batch is the largest batch of the table and dirties the buffer for
# every other operation; the cut batches themselves follow the split-k trainer step, the operation with the most
# workspace traffic (no operation has a larger batch).
Op = collections.namedtuple("Op", "name covers modules build stale_from")
_STEP_WS = ("l2hmc_gauge_mcmc_step_ws_bytes",)
_BIG = "step_cut_batch"


def _ops():
    ops = [
        Op("stq_dense_d128", ("l2hmc_stq_ws_bytes",), ("network",), _net_call("d128"), _BIG),
        Op("stq_dense_any_width", ("l2hmc_stq_ws_bytes",), ("network",), _net_call("any"), _BIG),
        Op("stq_dense_c_entry", ("l2hmc_stq_ws_bytes",), (), _stq_dense_c, _BIG),
        Op("stq_conv3d_l8", ("l2hmc_stq_conv3d_ws_bytes",), ("network",), _net_call("conv3d"), _BIG),
    ]
    both = ("l2hmc_gauge_ws_bytes", "l2hmc_gauge_transition_ws_bytes")
    ops += [Op("gauge_fused_8x8", both, ("gauge_dynamics",), _gauge_paths(8, 8, "generic", 19, True), _BIG),
            Op("gauge_layered_3x5", both, ("gauge_dynamics",), _gauge_paths(3, 5, "generic", 7, True), _BIG),
            Op("gauge_conv3d", both, ("gauge_dynamics",), _gauge_paths(8, 8, "conv3D", 5, True), _BIG)]
    for kind in STEP_KINDS:
        for ladder in (False, True):
            name = f"step_{kind}" + ("_ladder" if ladder else "")
            ops.append(Op(name, _STEP_WS, (), _step(kind, ladder),
                          "dynamics_trainer_split_k" if kind == "cut_batch" else _BIG))
    for T, X in ((5, 3), (4, 4)):                                  # a ragged and a full lattice (16 threads per row)
        for entry in ("run", "ladder", "exchange"):
            q = "l2hmc_gauge_hmc_run" + ("" if entry == "run" else "_" + entry) + "_ws_bytes"
            ops.append(Op(f"hmc_{entry}_{T}x{X}", (q,), (), _hmc_run(entry, T, X), _BIG))
    for kind in ("fused", "tiled", "walk_3x5", "conv3d", "ladder"):
        walk = kind == "walk_3x5"
        ops.append(Op(f"gauge_trainer_{kind}",
                      ("l2hmc_dense_backward_data_ws_bytes", "l2hmc_dense_weight_grads_ws_bytes") if walk
                      else ("l2hmc_gauge_train_ws_bytes",), ("layered_train",) if walk else ("_flat_trainer",),
                      _gauge_trainer(kind), _BIG))
    ops += [
        Op("gauge_train_c_entries", ("l2hmc_gauge_train_ws_bytes",), (), _gauge_train_c, _BIG),
        Op("dynamics_trainer_one_launch", ("l2hmc_small_train_ws_bytes",), ("_flat_trainer",),
           _dynamics_trainer("one_launch"), _BIG),
        Op("dynamics_trainer_layered", ("l2hmc_dense_backward_data_ws_bytes", "l2hmc_dense_weight_grads_ws_bytes"),
           ("layered_train",), _dynamics_trainer("layered"), _BIG),
        Op("dynamics_trainer_split_k", ("l2hmc_dense_backward_data_ws_bytes", "l2hmc_dense_weight_grads_ws_bytes"),
           ("layered_train",), _dynamics_trainer("split_k"), _BIG),
        Op("toy_vjp_entry", ("l2hmc_small_train_ws_bytes",), (), _toy_vjp, _BIG),
    ]
    return ops


OPS = {op.name: op for op in _ops()}
# the package call sites that allocate a workspace with a bare torch.empty, and the C-level operation that reaches
# their entry with a workspace the test owns
BARE_EMPTY_SITES = {"autograd": "gauge_train_c_entries", "autograd_toy": "toy_vjp_entry", "torch_ops": "stq_dense_c_entry"}


# ---- what the host test compares the table with --------------------------------------------------------------------
def declared_ws_queries():
    """Every l2hmc_*_ws_bytes function include/l2hmc_hip.h declares."""
    from l2hmc_amd import _lib
    return sorted(s for s in _lib.declared_symbols() if s.endswith("_ws_bytes"))


def modules_with_a_workspace():
    """The modules under l2hmc_amd/ that construct a `_lib.Workspace`."""
    pkg = os.path.join(ROOT, "l2hmc_amd")
    out = []
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py") and f != "_lib.py":
            with open(os.path.join(pkg, f)) as fh:
                if re.search(r"\bWorkspace\(\)", fh.read()):
                    out.append(f[:-3])
    return out
