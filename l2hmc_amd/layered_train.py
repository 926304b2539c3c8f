"""Training step of a layer-by-layer `Dynamics` (any x_dim, num_nodes or energy; `Dynamics.layered`): the loss of
mog_model.py:336-355 and its gradient with respect to both networks and eps (mog_model.py:357-363,
tf.gradients(loss, dynamics.variables)), by hand-written reverse mode over a tape.

Forward: the 2B stacked chains are split by the direction `propose` picked for them; each direction runs ONE taped
layered trajectory (step masks and the time input depend on the direction), through the same kernels as
`Dynamics.forward` / `.backward` -- l2hmc_stq_dense_taped is l2hmc_stq_dense with its activations kept --, so the
proposals and p are those bits.  Per sub-update the tape holds the network inputs [a | b] (VNet: x, grad E(x);
XNet: v, keep * x), h1, h2, S, T, Q, and references to the state the update consumed.

Reverse: sub-updates in reverse order.  l2hmc_lf_update_{v,x}_vjp give the cotangents of the input state, of S, T, Q
(and of grad E for a momentum update) and per-row d/d eps partials; l2hmc_dense_backward_data carries (dS, dT, dQ)
through the network to its inputs.  VNet's inputs are (x, grad E(x)), so d/dx gains d/da + Hess(E)(x) . (dg + d/db):
the closed form (l2hmc_mog_energy_hvp) for the packed targets, torch double-backward of the caller's energy
otherwise -- the reference's tf.gradients semantics, so a callable energy must be twice differentiable in torch.
The weight gradients are formed once per network, over all its calls' tapes stacked along rows
(l2hmc_dense_weight_grads), straight into the trainer's flat buffer [xnet | vnet | d/d eps].

Tape size per network: 2 N_LF calls x 2B rows x (Ka+Kb + 4H + 3D (S, T, Q) + 3D + 2D + 2) floats; with both
networks about 4 N_LF 2B (2D + 2H + 3D) 4 bytes for the forward part, and as much again for the reverse-pass
cotangents (at x_dim 50, H 100, N_LF 10, 2B = 8192: about 1.2 GB in all).

The two stages (LayeredWalk.forward: split by direction, taped trajectories, scatter into the stacked row order;
LayeredWalk.backward: reverse walk, weight gradients network by network, summed d/d eps) depend on no loss and no
trainer: a `Walk` gives them the networks, eps, the per-step masks and time input, and the energy gradient with its
Hessian-vector product; the caller gives the accept probability and, between the stages, the cotangents of
(x_N, v_N, sumlogdet).  `LayeredStep` is the toy targets' caller (squared-jump loss); `GaugeTrainer` runs the same
stages on the lattice (beta * force, ops.u1_force_hvp, l2hmc_gauge_loss_backward) where its tiled training entries
do not take the network widths."""
import collections
import ctypes as C

import torch

from . import _lib, ops, ops_periodic


class _NetTape:
    """Row-stacked tape of every call of one network: call c of a trajectory over n rows owns rows [off, off + n)."""

    def __init__(self, net, rows, dev):
        st = net.pack()
        self.D, self.H, self.Kin = st.D, st.H, st.Ka + st.Kb
        D, H = self.D, self.H
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)   # noqa: E731
        self.rows = rows
        self.inp, self.h1, self.h2 = f(rows, self.Kin), f(rows, H), f(rows, H)
        self.S, self.T, self.Q = f(rows, D), f(rows, D), f(rows, D)
        self.dz1, self.dz2, self.dpre, self.dsq = f(rows, H), f(rows, H), f(rows, 3 * D), f(rows, 2 * D)
        self.tcs = f(rows, 2)
        self.off = 0

    def take(self, n):
        sl = slice(self.off, self.off + n)
        self.off += n
        return sl


def energy_hvp(dyn, x, u, temperature=None):
    """Hess(energy / temperature)(x) . u per row: l2hmc_mog_energy_hvp for a packed target, torch double-backward of
    the caller's energy otherwise.  `temperature`: None = the dynamics' own (`_temp`)."""
    temp = dyn._temp() if temperature is None else float(temperature)
    if x.shape[0] == 0:
        return torch.zeros_like(x)
    if dyn._target is not None:
        out = torch.empty_like(x)
        st = dyn._target.struct(temp)
        _lib.call("l2hmc_mog_energy_hvp", C.byref(st), x, u.contiguous(), x.shape[0], out, device=dyn._device)
        return out
    with torch.enable_grad():
        xg = x.detach().clone().requires_grad_(True)
        e = dyn._fn(xg)
        if e.shape != (xg.shape[0],):
            raise ValueError(f"energy_function must return one energy per row: got {tuple(e.shape)}")
        (g,) = torch.autograd.grad(e.sum(), xg, create_graph=True)
        if not g.requires_grad:          # an energy linear in x: zero Hessian
            return torch.zeros_like(x)
        (hv,) = torch.autograd.grad(g, xg, grad_outputs=u, allow_unused=True)
    if hv is None:
        return torch.zeros_like(x)
    return (hv.to(torch.float32) / temp).contiguous()


class Walk:
    """What a taped layered trajectory and its reverse walk need of a target, and nothing of any loss or trainer:
    the two networks, eps, the trajectory length, per step the time input `format_time(step) -> [[t_cos, t_sin]]`
    (the dynamics' `_format_time`) and the masks `masks(step) -> (m, 1 - m)` ([D] device tensors), and the gradient
    that feeds the momentum update and VNet's second input, `grad(x)`, with its Hessian-vector product `hvp(x, u)`
    (toy targets: grad E / temperature and energy_hvp; the lattice: beta * force and ops.u1_force_hvp).
    `row_scale` ([R] device tensor over the stacked rows, or None): a factor per row on `grad` and `hvp` -- the
    lattice's beta on a ladder, where `grad` and `hvp` are those of beta = 1, and the toy targets' 1 / temperature,
    where they are those of temperature 1.
    `periodic`: the torus-exact lattice mode (GaugeDynamics(periodic=True)) -- x reaches the networks as
    [cos x | sin x] (VNet's first input, XNet's masked second one), the position sub-update is
    ops_periodic.lf_update_x_ncp, and the reverse walk carries the features' cotangents back into dx."""

    def __init__(self, xnet, vnet, eps, num_steps, format_time, masks, grad, hvp, row_scale=None, periodic=False):
        self.xnet, self.vnet, self.eps, self.num_steps = xnet, vnet, float(eps), int(num_steps)
        self.format_time, self.masks, self.grad, self.hvp = format_time, masks, grad, hvp
        self.row_scale, self.periodic = row_scale, bool(periodic)

    def time(self, step):
        t = self.format_time(step)
        return float(t[0, 0]), float(t[0, 1])

    def on_rows(self, idx):
        """The walk of the rows `idx` of the stacked batch (one direction's run): itself, or with `row_scale` the walk
        whose `grad` and `hvp` carry those rows' factors."""
        if self.row_scale is None:
            return self
        s = self.row_scale[idx][:, None]
        return Walk(self.xnet, self.vnet, self.eps, self.num_steps, self.format_time, self.masks,
                    lambda x: self.grad(x) * s, lambda x, u: self.hvp(x, u) * s, periodic=self.periodic)


# What LayeredWalk.forward hands to LayeredWalk.backward: the Walk, both tapes, per direction run (d, row indices,
# sub-updates), and x_N, v_N, sumlogdet, p in the stacked row order.
Forward = collections.namedtuple("Forward", "w tx tv runs xN vN sld p")


class LayeredWalk:
    """The target-independent stages of a layered training step (holds their workspaces): `forward`, taped
    trajectories of the stacked chains in the direction each runs, and `backward`, the reverse walk from given
    cotangents of (x_N, v_N, sumlogdet) with the weight gradients into caller-given l2hmc_dense_grads."""

    def __init__(self, device):
        self.device = device
        self._ws_bwd, self._ws_wg = _lib.Workspace(), _lib.Workspace()
        self.start_cotangents = None        # (d loss / d x_0, d loss / d v_0) of the last `backward`, stacked order

    def tapes(self, w, rows):
        """(XNet tape, VNet tape) for trajectories over `rows` rows in all."""
        n = 2 * w.num_steps * rows
        return _NetTape(w.xnet, n, self.device), _NetTape(w.vnet, n, self.device)

    # ---- forward ---------------------------------------------------------------------------------------------
    def _sub_v(self, w, x, v, tc, ts, d, lj, tape, subs):
        n, D = x.shape
        g = w.grad(x)
        sl = tape.take(n)
        a = ops_periodic.u1_angle_features(x) if w.periodic else x
        Ka = a.shape[1]
        tape.inp[sl, :Ka] = a
        tape.inp[sl, Ka:] = g
        tape.tcs[sl, 0], tape.tcs[sl, 1] = tc, ts
        S, T, Q = tape.S[sl], tape.T[sl], tape.Q[sl]
        _lib.call("l2hmc_stq_dense_taped", C.byref(w.vnet.pack()), a, g, None, tc, ts, n, S, T, Q, tape.h1[sl],
                  tape.h2[sl], device=self.device)
        out, ld = ops.lf_update_v(v, g, S, T, Q, w.eps, d)
        lj += ld
        subs.append(("v", sl, x, v, g, None))
        return out

    def _sub_x(self, w, x, v, keep, tc, ts, d, lj, tape, subs):
        n, D = x.shape
        b = keep.repeat(2) * ops_periodic.u1_angle_features(x) if w.periodic else keep * x
        sl = tape.take(n)
        tape.inp[sl, :D] = v
        tape.inp[sl, D:] = b
        tape.tcs[sl, 0], tape.tcs[sl, 1] = tc, ts
        S, T, Q = tape.S[sl], tape.T[sl], tape.Q[sl]
        _lib.call("l2hmc_stq_dense_taped", C.byref(w.xnet.pack()), v, b, None, tc, ts, n, S, T, Q, tape.h1[sl],
                  tape.h2[sl], device=self.device)
        out, ld = (ops_periodic.lf_update_x_ncp if w.periodic else ops.lf_update_x)(x, v, keep, S, T, Q, w.eps, d)
        lj += ld
        subs.append(("x", sl, x, v, None, keep))
        return out

    def trajectory(self, w, x0, v0, d, tx, tv):
        """One layered trajectory in direction d (0 forward, 1 backward) with every intermediate taped:
        -> (x_N, v_N, sumlogdet, subs)."""
        N = w.num_steps
        x, v = x0, v0
        lj = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
        subs = []
        for i in range(N):
            step = N - i - 1 if d else i
            tc, ts = w.time(step)
            m, mb = w.masks(step)
            first, second = (mb, m) if d else (m, mb)
            v = self._sub_v(w, x, v, tc, ts, d, lj, tv, subs)
            x = self._sub_x(w, x, v, first, tc, ts, d, lj, tx, subs)
            x = self._sub_x(w, x, v, second, tc, ts, d, lj, tx, subs)
            v = self._sub_v(w, x, v, tc, ts, d, lj, tv, subs)
        return x, v, lj, subs

    def forward(self, w, x0, v0, fwd, accept, accept_rows=False):
        """The stacked chains x0, v0 [R][D], each in the direction fwd [R] (bool, True = forward) gives it: one taped
        trajectory per direction over the rows that run it, scattered back into the stacked order, with
        p = accept(x_start, v_start, x_end, v_end, sumlogdet) of those rows (accept_rows: `accept` also takes the rows'
        indices in the stacked order, for a target whose energy depends on the row).  -> Forward."""
        R = x0.shape[0]
        tx, tv = self.tapes(w, R)
        xN, vN = torch.empty_like(x0), torch.empty_like(x0)
        sld, p = (torch.empty(R, dtype=torch.float32, device=self.device) for _ in range(2))
        runs = []
        for d, idx in ((0, torch.nonzero(fwd).reshape(-1)), (1, torch.nonzero(~fwd).reshape(-1))):
            if idx.numel() == 0:
                continue
            xs, vs = x0[idx].contiguous(), v0[idx].contiguous()
            xe, ve, lj, subs = self.trajectory(w.on_rows(idx), xs, vs, d, tx, tv)
            xN[idx], vN[idx], sld[idx] = xe, ve, lj
            p[idx] = accept(xs, vs, xe, ve, lj, idx) if accept_rows else accept(xs, vs, xe, ve, lj)
            runs.append((d, idx, subs))
        return Forward(w, tx, tv, runs, xN, vN, sld, p)

    # ---- reverse ---------------------------------------------------------------------------------------------
    def _backward_data(self, net, tape, sl, dS, dT, dQ):
        L, dev = _lib.lib(), self.device
        st = net.pack()
        n = dS.shape[0]
        din = torch.empty(n, tape.Kin, dtype=torch.float32, device=dev)
        ws, nb = self._ws_bwd.get(L.l2hmc_dense_backward_data_ws_bytes(C.byref(st)), dev)
        _lib.call("l2hmc_dense_backward_data", C.byref(st), tape.S[sl], tape.Q[sl], dS, dT, dQ, tape.h1[sl], tape.h2[sl],
                  n, tape.dpre[sl], tape.dsq[sl], tape.dz2[sl], tape.dz1[sl], din, ws, nb, device=dev)
        return din

    def reverse(self, w, subs, d, dx, dv, dld, tx, tv):
        """Walk one trajectory's sub-updates backwards from the cotangents of (x_N, v_N, sumlogdet); fills the tapes'
        cotangent slices and returns (the per-row d/d eps partials of every sub-update, d loss / d (x_0, v_0))."""
        eps = w.eps
        parts = []
        for kind, sl, xin, vin, g, keep in reversed(subs):
            tape = tv if kind == "v" else tx
            n, D = xin.shape
            S, T, Q = tape.S[sl], tape.T[sl], tape.Q[sl]
            dS, dT, dQ = torch.empty_like(S), torch.empty_like(S), torch.empty_like(S)
            de = torch.empty(n, dtype=torch.float32, device=xin.device)
            if kind == "v":
                dv_in, dg = torch.empty_like(dv), torch.empty_like(dv)
                _lib.call("l2hmc_lf_update_v_vjp", vin, g, S, T, Q, eps, d, n, D, dv, dld, dv_in, dg, dS, dT, dQ, de,
                          device=self.device)
                din = self._backward_data(w.vnet, tape, sl, dS, dT, dQ)
                if w.periodic:       # VNet read [cos x | sin x] (2 D wide) and the force
                    dx = (dx + w.hvp(xin, (dg + din[:, 2 * D:]).contiguous())).contiguous()
                    ops_periodic.u1_angle_features_vjp(xin, din[:, :2 * D].contiguous(), dx)
                else:
                    dx = dx + din[:, :D] + w.hvp(xin, (dg + din[:, D:]).contiguous())
                dv = dv_in
            else:
                dx_in, dv_part = torch.empty_like(dx), torch.empty_like(dx)
                _lib.call("l2hmc_lf_update_x_ncp_vjp" if w.periodic else "l2hmc_lf_update_x_vjp", xin, vin, keep, S, T,
                          Q, eps, d, n, D, dx, dld, dx_in, dv_part, dS, dT, dQ, de, device=self.device)
                din = self._backward_data(w.xnet, tape, sl, dS, dT, dQ)
                if w.periodic:       # XNet read keep . [cos x | sin x]
                    dx = ops_periodic.u1_angle_features_vjp(xin, (keep.repeat(2) * din[:, D:]).contiguous(), dx_in)
                else:
                    dx = (dx_in + keep * din[:, D:]).contiguous()
                dv = (dv + dv_part + din[:, :D]).contiguous()
            dx, dv = dx.contiguous(), dv.contiguous()
            parts.append(de)
        return parts, dx, dv

    def weight_grads(self, net, tape, g):
        """Weight gradients of `net` over every row of its tape into the l2hmc_dense_grads `g` (overwritten)."""
        L, dev = _lib.lib(), self.device
        st = net.pack()
        R = tape.off
        ws, nb = self._ws_wg.get(L.l2hmc_dense_weight_grads_ws_bytes(C.byref(st), R), dev)
        _lib.call("l2hmc_dense_weight_grads", C.byref(st), R, tape.inp, tape.h1, tape.h2, tape.dz1, tape.dz2, tape.dpre,
                  tape.dsq, tape.tcs, C.byref(g), ws, nb, device=dev)

    def backward(self, fw, dxN, dvN, dld, gx, gv, after_net=None):
        """From the cotangents of (x_N, v_N, sumlogdet) in the stacked row order: the reverse walk of every run of
        `fw`, then the weight gradients of XNet into the l2hmc_dense_grads `gx` and of VNet into `gv`;
        `after_net(k)` is called right after network k's products were enqueued.  -> d/d eps summed over all
        sub-updates (a device scalar).  `self.start_cotangents` keeps d loss / d (x_0, v_0) in the stacked row order (what
        the tiled entries leave in dx, dv)."""
        parts = []
        dx0, dv0 = torch.empty_like(dxN), torch.empty_like(dvN)
        for d, idx, subs in fw.runs:
            de, dx0[idx], dv0[idx] = self.reverse(fw.w.on_rows(idx), subs, d, dxN[idx].contiguous(),
                                                  dvN[idx].contiguous(), dld[idx].contiguous(), fw.tx, fw.tv)
            parts += de
        self.start_cotangents = (dx0, dv0)
        for k, (net, tape, g) in enumerate(((fw.w.xnet, fw.tx, gx), (fw.w.vnet, fw.tv, gv))):
            self.weight_grads(net, tape, g)
            if after_net is not None:
                after_net(k)
        return torch.cat(parts).sum() if parts else torch.zeros((), dtype=torch.float32, device=self.device)


class LayeredStep:
    """One `DynamicsTrainer.calc_loss_and_grads` of a layered dynamics (held by the trainer for its workspaces): the
    `Walk` over the toy target and the squared-jump loss with its cotangents."""

    def __init__(self, trainer):
        self.tr = trainer
        self.walk = LayeredWalk(trainer.dynamics._device)

    def __call__(self, x0, v0, fwd, inv_count, row_temps=None):
        """x0, v0 [2B][D] stacked start states, fwd [2B] bool (True = forward).  Writes the trainer's gradient buffer
        ([xnet | vnet | d/d eps]) and returns (x_N, p, terms) in the stacked row order.
        row_temps ([2B] float32 device tensor, or None = the dynamics' own temperature): a temperature per stacked row.
        Energy, its gradient and the Hessian-vector product are then formed at temperature 1 and multiplied by the
        row's 1 / temperature, formed as the scalar path forms it -- a packed target's kernels multiply by the float32
        quotient 1.f / temperature; torch, dividing a callable energy's values by a scalar, multiplies by the float64
        quotient rounded to float32 --, so a row has the bits of the scalar step at its (float32) temperature."""
        tr = self.tr
        dyn = tr.dynamics
        if row_temps is None:
            grad_energy, accept, accept_rows, inv = dyn.grad_energy, dyn.p_accept, False, None
            hvp = lambda x, u: energy_hvp(dyn, x, u)                      # noqa: E731
        else:
            inv = 1.0 / row_temps if dyn._target is not None else (1.0 / row_temps.double()).float()
            grad1, energy1 = self._at_temperature_one(dyn)
            grad_energy = grad1                                            # (Walk.on_rows lays the rows' factors on it)
            hvp = lambda x, u: energy_hvp(dyn, x, u, temperature=1.0)     # noqa: E731

            def accept(xs, vs, xe, ve, lj, idx):        # utils/dynamics.py:312-319 with the rows' temperatures
                old = energy1(xs) * inv[idx] + dyn.kinetic(vs)
                new = energy1(xe) * inv[idx] + dyn.kinetic(ve)
                return ops.accept_prob(old, new, lj)
            accept_rows = True
        w = Walk(dyn.XNet, dyn.VNet, dyn.eps, dyn.trajectory_length, dyn._format_time, dyn._get_mask, grad_energy, hvp,
                 row_scale=inv)
        fw = self.walk.forward(w, x0, v0, fwd, accept, accept_rows=accept_rows)
        xN, vN, p = fw.xN, fw.vN, fw.p
        # loss (mog_model.py:336-355) and its cotangents at (x_N, v_N, sumlogdet)
        scale = tr.scale
        sq = ((x0 - xN) ** 2).sum(1)
        vv = sq * p + 1e-4
        terms = scale / vv - vv / scale
        dvv = inv_count * (-scale / (vv * vv) - 1.0 / scale)
        # p = exp(min(H0 - H1 + sumlogdet, 0)): d p / d(H0 - H1 + sumlogdet) = p where p < 1, else 0
        dD = torch.where(p < 1, dvv * sq * p, torch.zeros_like(p))
        live = (p > 0)[:, None]
        zero = torch.zeros_like(x0)
        gE = torch.zeros_like(x0)
        if bool(live.any()):
            gE = dyn.grad_energy(xN) if inv is None else grad_energy(xN) * inv[:, None]
        dxN = torch.where(live, (dvv * p)[:, None] * 2.0 * (xN - x0) - dD[:, None] * gE, zero)
        dvN = torch.where(live, -dD[:, None] * vN, zero)
        dld = dD.contiguous()
        tr.grads[-1] = self.walk.backward(fw, dxN, dvN, dld, *tr._grad_structs)
        return xN, p, terms

    @staticmethod
    def _at_temperature_one(dyn):
        """(grad E, E) of the dynamics' target at temperature 1, whatever `dyn.temperature` is: `Dynamics.grad_energy`
        and `.energy` with their own expressions."""
        if dyn._target is not None:
            return (lambda x: dyn._target.energy_grad(x, 1.0)[1],
                    lambda x: dyn._target.energy_grad(x, 1.0, want_grad=False)[0])

        def grad1(x):
            with torch.enable_grad():
                xg = _lib.as_dev(x, dyn._device).reshape(-1, dyn.x_dim).detach().clone().requires_grad_(True)
                e = dyn._fn(xg)
                if e.shape != (xg.shape[0],):
                    raise ValueError(f"energy_function must return one energy per row: got {tuple(e.shape)}")
                (g,) = torch.autograd.grad(e.sum(), xg)
            return g.contiguous()
        return grad1, lambda x: dyn._fn(_lib.as_dev(x, dyn._device).reshape(-1, dyn.x_dim))
