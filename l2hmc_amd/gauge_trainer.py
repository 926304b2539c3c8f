"""Training step of the lattice sampler on the device:
  l2hmc/gauge_model.py:728-830  _calc_loss / _calc_loss_and_grads (loss + tf.gradients + clip_by_global_norm)
  l2hmc/gauge_model.py:925-970  exponential_decay schedule, AdamOptimizer (x hvd.size()), apply_gradients
  l2hmc/gauge_model.py:1160-1200 one `train_op` evaluation per step.

Everything between "samples in" and "weights updated" is library calls on device buffers
(include/l2hmc_hip.h, training section); the only host work per step is reading back the new step size,
which the plan passes by value.  Gradients of all ranks are combined by ONE all-reduce(SUM) of a flat buffer
[xnet | vnet | eps] -- the loss already divides by the global chain count, so the sum IS the gradient of the
global mean.  (The reference calls tf.gradients + apply_gradients, which bypasses
hvd.DistributedOptimizer.compute_gradients: its ranks never exchange gradients.  `allreduce_grads=False`
reproduces that; the default does what the Horovod wrapper is there for.)

Chains are integrated only in the direction their coin selects: the reference's mask multiplies the other
direction's outputs by exactly 0, so it contributes exactly 0 to every gradient.

The tiled training entries (l2hmc_gauge_train_*) need every network width to be a multiple of 32; GenericNet
networks of other widths (lattices whose T * X is not a multiple of 16: 6x6, 3x5, 4x6, ...) are trained through the
layered-training entries instead (the forward and backward stages of l2hmc_amd/layered_train.py), and so is a torus-exact
dynamics (`periodic=True`) unless `tiled_train=True` opens the tiled entries to it (`fused_forward=True` then makes
their forward one taped launch where the mode has its whole-trajectory kernel; nothing here changes for it).  Both are the
forward and the reverse of ONE step body (`calc_loss_and_grads`: stack, forward, loss reverse, reverse, exchange), so
they share the draws, the flat buffer, the data-parallel exchange and the optimiser (l2hmc_amd/_flat_trainer.py)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, _runs, ops
from . import layered_train as _layered_train
from ._flat_trainer import FlatTrainer, check_draws, stack_chains
from .dist import active as _active_dist
from .lattice import replica_swap, u1_observables

METRICS = {'l1': 0, 'l2': 1, 'cos': 2, 'cos2': 3, 'cos_diff': 4}


class GaugeTrainer(FlatTrainer):
    STEP_NAME = 'eps'

    def __init__(self, dynamics, lr_init=1e-3, lr_decay_steps=1000, lr_decay_rate=0.96, clip_value=None,
                 metric='cos_diff', loss_scale=1., aux_weight=1., std_weight=1., charge_weight=1., dist=None,
                 allreduce_grads=True, beta1=0.9, beta2=0.999, epsilon=1e-8, eager_variables=False,
                 bucketed=True):
        if metric not in METRICS:        # gauge_model.py:653-655
            raise AttributeError(f"metric={metric}. Expected one of: 'l1', 'l2', 'cos', 'cos2', or 'cos_diff'.")
        if dynamics.hmc:
            raise ValueError("hmc=True dynamics have no trainable networks (gauge_model.py:913-918 builds the "
                             "sampler only)")
        if dynamics.network_arch not in ('generic', 'conv3D'):
            raise NotImplementedError("training is implemented for network_arch 'generic' and 'conv3D'")
        dyn = dynamics
        self.metric, self.loss_scale = metric, float(loss_scale)
        self.weights = dict(aux_weight=float(aux_weight), std_weight=float(std_weight),
                            charge_weight=float(charge_weight))
        self.lr_init, self.lr_decay_steps, self.lr_decay_rate = float(lr_init), int(lr_decay_steps), float(lr_decay_rate)
        self.clip_value = None if clip_value is None else float(clip_value)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)
        self.dist = _active_dist(dist)
        self.world = self.dist.get_world_size() if self.dist is not None else 1
        self.allreduce_grads = bool(allreduce_grads)
        # bucketed: gradient groups go on the wire as soon as the reverse pass has produced them, on a side stream,
        # while the next group's products still run (what hvd.DistributedOptimizer does tensor by tensor,
        # gauge_model.py:942-943); False = one all-reduce of the whole buffer after the pass.  Same numbers.
        self.bucketed = bool(bucketed)
        # Which variable list the optimiser sees.  Graph mode -- the path the CLI runs -- differentiates and
        # applies over `dynamics.variables` (gauge_model.py:825, :965-968), which holds the step size even when
        # it was created with trainable=False (gauge_dynamics.py:91-96): eps moves and counts in the clip norm
        # REGARDLESS of `eps_trainable`.  Eager mode uses `trainable_variables` (:820) and respects the flag.
        # Default = graph mode, as the reference's sessions run; eager_variables=True = the eager branch.
        self.eager_variables = bool(eager_variables)
        self.last_bucket_count = 0       # gradient groups the last step put on the wire (0: nothing to exchange)
        dev = dyn._device
        # one bucket: [xnet | vnet | eps]
        super().__init__(dyn, (dyn.position_fn, dyn.momentum_fn),
                         torch.tensor([float(dyn.eps)], dtype=torch.float32, device=dev))
        self.broadcast_weights()
        self._buckets = self._bucket_ranges()
        self._side = torch.cuda.Stream(device=dev) if (self.dist is not None and dev.type == "cuda") else None
        # Which kernels a step runs through, decided per call: None = by shape (the tiled training entries where every
        # width of both GenericNets is a multiple of 32, the layered-training entries otherwise); True = the layered
        # path at any shape; False = the tiled entries (which refuse other widths).
        self.layered = None
        self._walk = None

    def _bucket_ranges(self):
        """{bucket id of l2hmc_gauge_train_backward_buckets: [(lo, hi), ...]} over the flat gradient buffer
        [xnet | vnet | eps]; a network's flat layout is SEGMENTS (+ Conv3D kernels), so groups 3k .. 3k+2 are
        single contiguous ranges and the rest (front-end gradients, eps) a few short ones."""
        out, rest, off = {}, [], 0
        for k, net in enumerate(self._nets):
            flat, _, offsets = net.flat_params()
            out[3 * k + 0] = [(off + offsets["w1_t"][0], off + offsets["b1"][1])]
            out[3 * k + 1] = [(off + offsets["wh_t"][0], off + offsets["bh"][1])]
            out[3 * k + 2] = [(off + offsets["whd_t"][0], off + offsets["coeff_q"][1])]
            extra = [n for n in offsets if n not in net.SEGMENTS]
            if extra:
                rest.append((off + min(offsets[n][0] for n in extra), off + max(offsets[n][1] for n in extra)))
            off += flat.numel()
        rest.append((off, off + 1))
        out[_lib.GRAD_BUCKET_REST] = rest
        return out

    def broadcast_weights(self, src=0):
        """hvd.BroadcastGlobalVariablesHook(0) (gauge_model.py:1008): every rank starts from rank `src`'s
        weights, step size and masks -- one broadcast per flat buffer."""
        if self.dist is None:
            return
        dyn = self.dynamics
        for net in self._nets:
            self.dist.broadcast(net.flat_params()[0], src=src)
            net.refresh_packed()
        self.dist.broadcast(self._step_dev, src=src)
        self._write_step()
        self.dist.broadcast(dyn.mask, src=src)
        dyn._heads = None                 # the masks changed in place: the active-column heads are packed again

    # ---- what the shared optimiser step asks of a trainer ---------------------------------------------------
    def _write_step(self):
        self.dynamics.eps = self._step_dev.detach().cpu().reshape(())      # the plan carries eps by value

    def _step_trainable(self):
        return bool(self.dynamics.eps_trainable) or not self.eager_variables

    def learning_rate(self):
        """tf.train.exponential_decay(staircase=True) times the rank count (gauge_model.py:934-942)."""
        return self.lr_init * self.lr_decay_rate ** (self.global_step // self.lr_decay_steps) * self.world

    # ---- loss + gradients ----------------------------------------------------------
    def calc_loss_and_grads(self, x, beta, z=None, draws_x=None, draws_z=None):
        """gauge_model.py:799-830 -> (loss, x_out, accept_prob, x_dq); gradients land in self.grads.
        draws_*: optional (momentum_f, momentum_b, coin, u) for the x and the z transition.
        beta: a scalar, or a LADDER [B] / [1, B] (`_runs.per_chain`; a float32 tensor on the device stays there):
        chain i of the x batch and chain i of the z batch then train at beta[i], through the `_ladder` training entries
        on every path (fused, tiled, layered); everything else -- draws, loss, its normalisation, the exchange -- is the
        scalar step's.  ValueError for another shape, a negative or a non-finite beta, before any draw is taken."""
        dyn = self.dynamics
        dev = dyn._device
        T, X = dyn.lattice.time_size, dyn.lattice.space_size
        who = "GaugeTrainer.calc_loss_and_grads"
        _lib.expect_shape(x, (None, 2 * T * X), "x", who, fold=True)
        x = dyn._x(x)
        B, D = x.shape
        betas = self._chain_betas(beta, B, "calc_loss_and_grads")      # None: one beta, today's entries
        _lib.expect_shape(z, (B, D), "z", who, fold=True)               # (every shape, before the first draw)
        check_draws(draws_x, B, D, "draws_x", who)
        check_draws(draws_z, B, D, "draws_z", who)
        z = dyn._normal((B, D)) if z is None else dyn._x(z)

        def draw(d):
            if d is None:
                return dyn._normal((B, D)), dyn._normal((B, D)), dyn._uniform((B,)), dyn._uniform((B,))
            return tuple(_lib.as_dev(a, dev) for a in d)
        x0, v0, fwd, dirs, u_x = stack_chains(x, z, draw(draws_x), draw(draws_z))
        R = 2 * B
        L, layered = _lib.lib(), self._use_layered()
        if layered:          # one taped layered trajectory per direction, on the rows that run it
            if self._walk is None:
                self._walk = _layered_train.LayeredWalk(dev)
            if betas is None:
                fw = self._walk.forward(self._lattice_walk(float(beta)), x0, v0, fwd,
                                        lambda *a: dyn._compute_accept_prob(*a, float(beta)))
            else:            # rows i and B + i at beta[i]: the beta = 1 force and its Hessian scaled per row
                rb = betas.repeat(2)

                def accept(xs, vs, xe, ve, lj, idx):        # gauge_dynamics.py:592-609 with the rows' betas
                    old = rb[idx] * dyn.potential(xs) + dyn.kinetic_energy(vs)
                    new = rb[idx] * dyn.potential(xe) + dyn.kinetic_energy(ve)
                    return ops.accept_prob(old, new, lj)
                fw = self._walk.forward(self._lattice_walk(1.0, rb), x0, v0, fwd, accept, accept_rows=True)
            xN, vN, p = fw.xN, fw.vN, fw.p
        else:
            xN, vN = torch.empty_like(x0), torch.empty_like(x0)
            sld, p = (torch.empty(R, dtype=torch.float32, device=dev) for _ in range(2))
            plan = dyn._plan()
            ws, nb = self._ws.get(L.l2hmc_gauge_train_ws_bytes(C.byref(plan), R), dev)
            if betas is None:
                _lib.call("l2hmc_gauge_train_forward", C.byref(plan), float(beta), x0, v0, dirs, R, xN, vN, sld, p, ws,
                          nb, device=dev)
            else:
                _lib.call("l2hmc_gauge_train_forward_ladder", C.byref(plan), betas, 1, B, x0, v0, dirs, R, xN, vN, sld,
                          p, ws, nb, device=dev)
        terms = torch.empty(B, dtype=torch.float32, device=dev)
        dxN, dvN = torch.empty_like(x0), torch.empty_like(x0)
        dld = torch.empty(R, dtype=torch.float32, device=dev)
        w = self.weights
        loss_tail = (x0, xN, vN, p, B, METRICS[self.metric], self.loss_scale, w['aux_weight'], w['std_weight'],
                     w['charge_weight'], 1.0 / (B * self.world), terms, dxN, dvN, dld)
        if betas is None:
            _lib.call("l2hmc_gauge_loss_backward", T, X, float(beta), *loss_tail, device=dev)
        else:
            _lib.call("l2hmc_gauge_loss_backward_ladder", T, X, betas, 1, *loss_tail, device=dev)
        buf = torch.stack([terms.sum(dtype=torch.float32),
                           torch.full((), float(B), dtype=torch.float32, device=dev)])
        # Bucketed exchange: `send(ranges)` puts ranges of the flat buffer on the wire as soon as the reverse has
        # enqueued their producers -- each network's range right after its products, the eps slot last.
        n0, n1 = self._sizes
        bucketed = self.dist is not None and self.allreduce_grads and self.bucketed
        works = []
        cur = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        send = (lambda ranges: self._all_reduce_ranges(ranges, works, cur)) if bucketed else None
        if layered:
            lo = (0, n0)
            self.grads[n0 + n1] = self._walk.backward(
                fw, dxN, dvN, dld, *self._grad_structs,
                (lambda k: send([(lo[k], lo[k] + self._sizes[k])])) if bucketed else None)
            if bucketed:
                send([(n0 + n1, n0 + n1 + 1)])
        else:
            bargs = (C.byref(plan), *((float(beta),) if betas is None else (betas, 1, B)), dirs, R, dxN, dvN, dld,
                     C.byref(self._grad_structs[0]), C.byref(self._grad_structs[1]),
                     *(C.byref(g) if g is not None else None for g in self._conv_grad_structs),
                     self.grads[n0 + n1:], ws, nb)
            errors = []

            def on_bucket(_user, b):           # host thread, right after bucket b's producers were enqueued
                try:
                    send(self._buckets[int(b)])
                except Exception as e:          # noqa: BLE001 -- a ctypes callback cannot raise: re-raised below
                    errors.append(e)
            cb = _lib.BUCKET_FN(on_bucket) if bucketed else _lib.BUCKET_FN()      # (not bucketed: a NULL callback)
            if betas is not None:               # one entry for both: its callback may be NULL
                _lib.call("l2hmc_gauge_train_backward_ladder", *bargs, device=dev, tail=(cb, None))
            elif bucketed:
                _lib.call("l2hmc_gauge_train_backward_buckets", *bargs, device=dev, tail=(cb, None))
            else:
                _lib.call("l2hmc_gauge_train_backward", *bargs, device=dev)
            if errors:
                raise errors[0]
        if bucketed:
            self.dist.all_reduce(buf, op=self.dist.ReduceOp.SUM)
            for wk in works:
                wk.wait()
            if self._side is not None:
                cur.wait_stream(self._side)
            self.last_bucket_count = len(works)
        elif self.dist is not None:
            self.dist.all_reduce(buf, op=self.dist.ReduceOp.SUM)
            if self.allreduce_grads:
                self.dist.all_reduce(self.grads, op=self.dist.ReduceOp.SUM)
        return self._step_outputs(x, u_x, xN, p, terms, buf)

    def _step_outputs(self, x, u_x, xN, p, terms, buf):
        """(loss, x_out, accept_prob, x_dq) of a step from its proposals, accept probabilities and loss sums."""
        T, X = self.dynamics.lattice.time_size, self.dynamics.lattice.space_size
        B = x.shape[0]
        loss = buf[0] / buf[1]
        px = p[:B]
        x_prop = xN[:B]
        x_out = torch.where((px > u_x)[:, None], x_prop, x)        # gauge_dynamics.py:244-257 (strict >)
        q0 = u1_observables(x, T, X)["top_charge"]
        q1 = u1_observables(x_out, T, X)["top_charge"]
        x_dq = torch.abs(q0 - q1).to(torch.int32)                  # gauge_model.py:762-763
        self.last_loss_terms, self.last_pz = terms, p[B:]
        return loss, x_out, px, x_dq

    def _use_layered(self):
        if getattr(self.dynamics, "periodic", False):
            # tiled_train=True (L2HMC_PLAN_PERIODIC_TRAIN) opens the tiled entries to the mode where the widths tile
            if getattr(self.dynamics, "tiled_train", False):
                if self.layered:                           # the walk, as the cross-check
                    return True
                packs = [net.pack() for net in self._nets]
                widths = [(st.D, st.H, st.Ka, st.Kb) for st in packs]
                if all(w % 32 == 0 for ws in widths for w in ws):
                    return False
                if self.layered is not None:               # layered = False where the widths do not tile
                    raise NotImplementedError(f"GaugeTrainer.layered = False on a periodic=True, tiled_train=True "
                                              f"dynamics whose network widths (D, H, Ka, Kb) = {widths} are not all "
                                              "multiples of 32: the tiled training entries refuse them; the layered "
                                              "walk trains them")
                return True
            if self.layered is not None and not self.layered:
                raise NotImplementedError("GaugeTrainer.layered = False on a periodic=True dynamics: the tiled "
                                          "training entries refuse L2HMC_PLAN_PERIODIC plans; the layered walk trains them")
            return True
        if self.layered is not None:
            use = bool(self.layered)
        else:
            packs = [net.pack() for net in self._nets]
            use = not all(w % 32 == 0 for st in packs for w in (st.D, st.H, st.Ka, st.Kb))
        if use and self.dynamics.network_arch != 'generic':
            raise NotImplementedError("the layered training path takes GenericNet networks only; ConvNet3D training "
                                      "needs network widths that are multiples of 32")
        return use

    def _all_reduce_ranges(self, ranges, works, cur):
        """Start async all-reduces(SUM) of the given ranges of the flat gradient buffer, on the side stream after
        everything enqueued so far on `cur`."""
        if self._side is not None:
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                for lo, hi in ranges:
                    works.append(self.dist.all_reduce(self.grads[lo:hi], op=self.dist.ReduceOp.SUM, async_op=True))
        else:
            for lo, hi in ranges:
                works.append(self.dist.all_reduce(self.grads[lo:hi], op=self.dist.ReduceOp.SUM, async_op=True))

    def _lattice_walk(self, beta, row_betas=None):
        """The lattice as l2hmc_amd/layered_train.py sees it: beta * force feeds the momentum update and VNet, with
        ops.u1_force_hvp as its Hessian-vector product.  A ladder is beta = 1 with `row_betas` [2B] as the walk's row
        factor: both kernels form beta * (a difference of sines), so the host's product has the bits of theirs."""
        dyn = self.dynamics
        T, X = dyn.lattice.time_size, dyn.lattice.space_size
        return _layered_train.Walk(dyn.position_fn, dyn.momentum_fn, dyn.eps, dyn.num_steps, dyn._format_time,
                                   dyn._get_mask_while,
                                   lambda x: ops.u1_action_force(x, T, X, beta, want_observables=False)[1],
                                   lambda x, u: ops.u1_force_hvp(x, u, T, X, beta), row_scale=row_betas,
                                   periodic=getattr(dyn, "periodic", False))

    def _chain_betas(self, beta, B, who):
        """None for one beta (a number or a 0-d array / tensor: the scalar entries, untouched); else the ladder as a
        float32 device tensor [B] (`_runs.per_chain`: ValueError for another shape or a value that is negative or not
        finite in float32; a float32 tensor [B] or [1, B] on the device stays there, unchecked)."""
        nd = beta.ndim if isinstance(beta, torch.Tensor) else np.ndim(beta)
        if nd == 0:
            return None
        return _runs.per_chain(beta, B, self.dynamics._device, who=f"GaugeTrainer.{who}", name="beta",
                               sign="not negative")[0]

    def update_beta(self, step, beta_init=2., beta_final=4., train_steps=10000):
        """gauge_model.py:1039-1046: linear annealing of 1/beta (elementwise: a ladder anneals rung by rung)."""
        temp = (1. / beta_init - 1. / beta_final) * (1. - step / float(train_steps)) + 1. / beta_final
        return 1. / temp

    @staticmethod
    def swap_schedule(n_steps, swap_every):
        """The exchange rounds of `train(..., replicas=G, swap_every=k)` over n_steps steps: {s: parity} for every
        step s (counting from 1 within the call) that a round follows -- the samplers' schedule, `_runs.Exchange`
        with first parity 0, read out step by step."""
        ex = _runs.Exchange(2, int(swap_every), 0, None, 2)
        return {s: ex.parity_after(s) for s in range(1, int(n_steps) + 1) if ex.parity_after(s) is not None}

    def train(self, train_steps, samples_init=None, beta_init=2., beta_final=4., initial_step=0, print_steps=0,
              log=print, replicas=None, swap_every=1):
        """gauge_model.py:1119-1300 without the file / TensorBoard side effects: per step anneal beta, run the
        train op on the current samples, wrap the new samples to [0, 2 pi) (device side), record loss, accept
        probability, step size, learning rate and the observables of the step's INPUT samples (:256-266).
        Returns {'loss', 'accept_prob', 'eps', 'lr', 'beta', 'actions', 'plaqs', 'charges', 'charge_diff',
        'samples'} with per-step NumPy histories; the chain state never leaves the device inside the loop.
        beta_init / beta_final: each a scalar or [B] (one per chain): with an array the step trains on the ladder
        update_beta gives it (`calc_loss_and_grads`) and out['beta'] is [steps, B] instead of [steps].
        replicas=G: replica exchange between the rungs WHILE the networks train -- the frozen high-beta rungs see what
        tunnelled at low beta.  Columns [g G, (g + 1) G) are one group; after the wrap of every step s (from 1 within
        the call) with s % swap_every == 0 ONE round of l2hmc_gauge_replica_swap runs on the x chains at that step's
        betas, with parity (s // swap_every - 1) % 2 and one stream of the dynamics' counter
        (`GaugeSampler.swap_replicas`'s round, bit for bit).  out gains 'swap_rate' [G - 1] and 'swapped' [rounds, B].
        A group lives on one rank; the gradient all-reduce is what it was.  replicas=None: no round."""
        dyn = self.dynamics
        T, X = dyn.lattice.time_size, dyn.lattice.space_size
        if samples_init is None:
            samples_init = np.asarray(dyn.lattice.samples, dtype=np.float32).reshape(dyn.batch_size, dyn.x_dim)
        _lib.expect_shape(samples_init, (None, dyn.x_dim), "samples_init", "GaugeTrainer.train", fold=True)
        x = dyn._x(samples_init).clone()
        B = x.shape[0]
        ladder = np.ndim(beta_init) > 0 or np.ndim(beta_final) > 0
        if ladder:
            beta_init, beta_final = (np.asarray(b, dtype=np.float64) for b in (beta_init, beta_final))
            for name, b in (("beta_init", beta_init), ("beta_final", beta_final)):
                if b.shape not in ((), (B,)):
                    raise ValueError(f"GaugeTrainer.train: {name} of shape {b.shape}: expected a scalar or [{B}]")
            beta_init, beta_final = np.broadcast_to(beta_init, (B,)), np.broadcast_to(beta_final, (B,))
        ex = None                # the samplers' exchange schedule and histories (_runs.Exchange), first parity 0
        if replicas is not None:
            G, k, _, _ = _runs.check_replicas(replicas, B, swap_every, who="GaugeTrainer.train")
            ex = _runs.Exchange(G, k, 0, None, B)
        hist = {k: [] for k in ("loss", "accept_prob", "eps", "lr", "beta", "actions", "plaqs", "charges",
                                "charge_diff")}
        for step in range(initial_step, train_steps):
            beta = self.update_beta(step, beta_init, beta_final, train_steps)
            lr = self.learning_rate()
            obs = u1_observables(x, T, X)
            # (a ladder goes to the device once per step: the step and the round read the same float32 values)
            beta_dev = self._chain_betas(beta, B, "train") if ladder else None
            loss, x_out, px, x_dq = self.train_step(x, beta if beta_dev is None else beta_dev)
            ops.wrap_angle(x_out, out=x)
            parity = ex.parity_after(step - initial_step + 1) if ex is not None else None
            if parity is not None:
                if beta_dev is None:
                    beta_dev = torch.full((B,), float(beta), dtype=torch.float32, device=x.device)
                swap_p, swapped, _ = replica_swap(x, T, X, G, parity, beta_dev, dyn._seed, dyn._draws)
                dyn._draws += 1                                # one stream, as GaugeSampler._swap_round takes it
                ex.rounds["swap_p"].append(swap_p)
                ex.rounds["swapped"].append(swapped)
            for k, v in (("loss", loss), ("accept_prob", px.mean()), ("actions", obs["action"].mean()),
                         ("plaqs", obs["avg_plaq"].mean()), ("charges", obs["top_charge"]),
                         ("charge_diff", x_dq.sum() / float(x_dq.numel()))):
                hist[k].append(v)
            hist["eps"].append(float(dyn.eps))
            hist["lr"].append(lr)
            hist["beta"].append(beta)
            if print_steps and step % print_steps == 0:
                log(f"{step:>5g}/{train_steps:<6g} loss {float(loss):^9.4g} acc {float(px.mean()):^9.4g} "
                    f"eps {float(dyn.eps):^9.4g} beta {float(np.mean(beta)):^9.4g} "
                    f"plaq {float(obs['avg_plaq'].mean()):^9.4g} lr {lr:^9.4g}")
        out = {k: (torch.stack(v).cpu().numpy() if v and isinstance(v[0], torch.Tensor) else np.asarray(v))
               for k, v in hist.items()}
        out["samples"] = x
        if ex is not None:       # (the trainer keeps no labels: of the samplers' histories, `swapped` and its rate)
            rounds = ex.finish({})
            out["swapped"], out["swap_rate"] = rounds["swapped"], rounds["swap_rate"]
        return out

    # ---- resumable state (gauge_model.py:519-556 `_current_state` + save_weights; .npz, never a pickle) ----
    def save_state(self, path, samples=None, beta=None):
        """Everything a resumed run needs: weights and Adam moments in the flat layout, step size, counters,
        masks, and optionally the chain state and beta (a scalar or a ladder [B]) of `_current_state`."""
        d = {"xnet": self._nets[0].flat_params()[0], "vnet": self._nets[1].flat_params()[0], "adam_m": self._m,
             "adam_v": self._v, "eps": self._step_dev, "masks": self.dynamics.mask}
        out = {k: v.detach().cpu().numpy() for k, v in d.items()}
        out.update(global_step=np.int64(self.global_step), step=np.int64(self.global_step),
                   adam_t=np.int64(self._adam_t),
                   lr=np.float64(self.learning_rate()), draws=np.int64(self.dynamics._draws))
        if samples is not None:
            out["samples"] = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
        if beta is not None:
            out["beta"] = np.asarray(beta, dtype=np.float64)       # a scalar, or a ladder [B] as given
        np.savez(path, **out)

    def load_state(self, path):
        """Inverse of save_state; returns {'samples', 'beta'} when they were stored."""
        dyn = self.dynamics
        with np.load(path if str(path).endswith(".npz") else str(path) + ".npz", allow_pickle=False) as f:
            for net, key in zip(self._nets, ("xnet", "vnet")):
                flat = net.flat_params()[0]
                if f[key].shape != tuple(flat.shape):
                    raise ValueError(f"{key}: stored {f[key].shape}, expected {tuple(flat.shape)}")
                flat.copy_(torch.from_numpy(f[key]))
                net.pack()
                net.refresh_packed()
            self._m.copy_(torch.from_numpy(f["adam_m"]))
            self._v.copy_(torch.from_numpy(f["adam_v"]))
            self._step_dev.copy_(torch.from_numpy(f["eps"]))
            self._write_step()
            dyn.set_masks(f["masks"])
            self.global_step, self._adam_t = int(f["global_step"]), int(f["adam_t"])
            dyn._draws = int(f["draws"])
            extra = {k: f[k] for k in ("samples", "beta") if k in f.files}
        self.sync_weights()
        return extra

    def current_state(self, samples=None, beta=None):
        """The reference's `_current_state` dict (gauge_model.py:370-376, :1190-1194) with its own keys --
        {'samples', 'eps', 'step', 'beta', 'lr'} -- from this trainer; `save_state` writes the same keys (plus the
        optimiser state the reference leaves to the TF checkpoint) into its .npz."""
        if isinstance(samples, torch.Tensor):
            samples = samples.detach().cpu().numpy()
        return {'samples': samples, 'eps': float(self.dynamics.eps), 'step': int(self.global_step),
                'beta': (None if beta is None else float(beta) if np.ndim(beta) == 0
                         else np.asarray(beta, dtype=np.float64)), 'lr': float(self.learning_rate() / self.world)}

    @staticmethod
    def train_data_dict(out, initial_step=0):
        """`train()` histories -> the reference's `train_data_dict` (gauge_model.py:362-369, :1196-1205):
        {'loss' | 'actions' | 'plaqs' | 'charges' | 'charge_diff' | 'accept_prob': {(step, beta): value}}."""
        keys = [(initial_step + i, float(b) if np.ndim(b) == 0 else tuple(float(v) for v in b))     # (a ladder: its
                for i, b in enumerate(out['beta'])]                                                   #  rungs)
        return {name: {k: out[name][i] for i, k in enumerate(keys)}
                for name in ('loss', 'actions', 'plaqs', 'charges', 'charge_diff', 'accept_prob')}
