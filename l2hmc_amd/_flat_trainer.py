"""What `GaugeTrainer` and `DynamicsTrainer` share: the flat buffer [xnet | vnet | step size] of gradients and Adam
moments with the per-network gradient structs over it, the stacking of the x and z chains into one batch, and the
optimiser step (optional clip_by_global_norm, Adam per network, the step-size update, repacking).  A subclass supplies
the device scalar of its step size (`_step_dev`) and the name of its slot (`STEP_NAME`), `_write_step` (what storing
a new step size in the dynamics means), `_step_trainable`, `clip_value` and `learning_rate`."""
import torch

from . import _lib


def check_draws(draws, B, D, name, who):
    """A trainer's `draws_x` / `draws_z` (None: not injected): exactly four tensors, [B, D], [B, D], (B,), (B,) --
    momentum forward, momentum backward, coin or direction bit, u.  ValueError on the host, before any draw."""
    if draws is None:
        return
    if len(draws) != 4:
        raise ValueError(f"{who}: {name} of {len(draws)} tensors: expected 4 (momentum forward, momentum backward, "
                         "coin or direction bit, u)")
    for i, (t, shape) in enumerate(zip(draws, ((B, D), (B, D), (B,), (B,)))):
        _lib.expect_shape(t, shape, f"{name}[{i}]", who)


def stack_chains(x, z, draws_x, draws_z):
    """The x and z chains as one batch of 2B rows, from the (momentum_f, momentum_b, coin / direction bit, u) draws
    of each: -> (x0, v0, fwd [2B] bool, dirs [2B] int32 (1 = backward), u of the x chains).  A chain starts from the
    momentum of the direction it runs in."""
    vf_x, vb_x, coin_x, u_x = draws_x
    vf_z, vb_z, coin_z, _ = draws_z
    fwd = torch.cat([coin_x, coin_z]) > 0.5
    x0 = torch.cat([x, z]).contiguous()
    v0 = torch.where(fwd[:, None], torch.cat([vf_x, vf_z]), torch.cat([vb_x, vb_z])).contiguous()
    dirs = (~fwd).to(torch.int32).contiguous()
    return x0, v0, fwd, dirs, u_x


class FlatTrainer:
    STEP_NAME = None         # name of the last slot in grad_views(): 'eps' / 'alpha'
    clip_value = None

    def __init__(self, dynamics, nets, step_dev):
        self.dynamics = dynamics
        self.global_step, self._adam_t = 0, 0
        self._nets = nets
        flats = [n.flat_params() for n in nets]
        self._sizes = [f[0].numel() for f in flats]
        self.grads = torch.zeros(sum(self._sizes) + 1, dtype=torch.float32, device=dynamics._device)
        self._m, self._v = torch.zeros_like(self.grads), torch.zeros_like(self.grads)
        self._step_dev = step_dev
        self._gnorm = torch.zeros(1, dtype=torch.float32, device=dynamics._device)
        self._ws = _lib.Workspace()
        # l2hmc_dense_grads (and, for a ConvNet3D, l2hmc_conv3d_grads) of each network over the flat buffer
        self._grad_structs, self._conv_grad_structs = [], []
        off = 0
        for net, (flat, _, offsets) in zip(nets, flats):
            at = lambda k: self.grads.data_ptr() + 4 * (off + offsets[k][0])     # noqa: E731
            self._grad_structs.append(_lib.DenseGrads(**{k: at(k) for k in net.SEGMENTS}))
            conv = [k for k in offsets if k not in net.SEGMENTS]
            self._conv_grad_structs.append(_lib.Conv3DGrads(**{k: at(k) for k in conv}) if conv else None)
            off += flat.numel()

    def grad_views(self):
        """{'xnet': {segment: tensor}, 'vnet': {...}, STEP_NAME: tensor} over the flat gradient buffer."""
        out, off = {}, 0
        for name, net in zip(("xnet", "vnet"), self._nets):
            flat, views, offsets = net.flat_params()
            out[name] = {k: self.grads[off + a:off + b].view(views[k].shape) for k, (a, b) in offsets.items()}
            off += flat.numel()
        out[self.STEP_NAME] = self.grads[off:off + 1]
        return out

    def apply_gradients(self):
        """clip_by_global_norm (if clip_value) + Adam on [xnet | vnet | step size]; bumps global_step."""
        dev = self.dynamics._device
        self._adam_t += 1
        t = self._adam_t
        lr_t = self.learning_rate() * (1. - self.beta2 ** t) ** 0.5 / (1. - self.beta1 ** t)
        g, m, v = self.grads, self._m, self._v
        segs, off = [], 0
        for net in self._nets:
            flat, _, offsets = net.flat_params()
            segs.append((flat, off, flat.numel(), offsets["b1"]))
            off += flat.numel()
        step = self._step_trainable()
        gnorm, clip = None, 0.
        if self.clip_value is not None:
            for i, (_, o, n, tri) in enumerate(segs):
                _lib.call("l2hmc_grad_sumsq", g[o:], n, tri[0], tri[1], self._gnorm, int(i > 0), device=dev)
            if step:
                _lib.call("l2hmc_grad_sumsq", g[off:], 1, 0, 0, self._gnorm, 1, device=dev)
            gnorm, clip = self._gnorm, self.clip_value
        for (w, o, n, tri) in segs:
            _lib.call("l2hmc_adam_step", w, g[o:], m[o:], v[o:], n, lr_t, self.beta1, self.beta2, self.epsilon, gnorm,
                      clip, tri[0], tri[1], device=dev)
        if step:
            _lib.call("l2hmc_adam_step", self._step_dev, g[off:], m[off:], v[off:], 1, lr_t, self.beta1, self.beta2,
                      self.epsilon, gnorm, clip, 0, 0, device=dev)
            self._write_step()
        for net in self._nets:
            net.refresh_packed()
        self.global_step += 1

    def train_step(self, x, *args, **kw):
        """calc_loss_and_grads, then apply_gradients: -> what calc_loss_and_grads returns."""
        out = self.calc_loss_and_grads(x, *args, **kw)
        self.apply_gradients()
        return out

    def sync_weights(self):
        """Bring the reference-layout layer tensors (state_dict / save_weights) up to date."""
        for net in self._nets:
            net.sync_reference_layout()
