"""Float64 reference of the torus-exact L2HMC mode (`GaugeDynamics(periodic=True)`), written from its formulas and from
nothing else of the package: NumPy for sampling parity (any dtype, so the same code in float32 is the yardstick for how
far a float32 implementation may sit from the float64 answer) and a torch float64 subclass of the gradient oracle.

A position sub-update with keep mask `keep`, omk = 1 - keep, direction d, es = exp(+-eps S), eq = exp(eps Q) and
S, T, Q = XNet(v, [keep cos x, keep sin x], t):
  d = 0:  y = 2 atan2(es sin(x/2), cos(x/2)) + eps (eq v + T),      x' = keep x + omk y
          log-det  omk (eps S - log(cos^2(x/2) + es^2 sin^2(x/2)))
  d = 1:  w = x' - eps (eq v + T),  x = keep x' + omk 2 atan2(es sin(w/2), cos(w/2)),   es = exp(-eps S)
          log-det  omk (-eps S - log(cos^2(w/2) + es^2 sin^2(w/2)))
The momentum sub-update is the reference's with VNet([cos x, sin x], beta force(x), t).  Positions are defined modulo
2 pi: compare them with `angdist`."""
import numpy as np
import torch

from oracle import nets
from oracle.torch_ref import TorchGaugeModel
from tests import helpers as H

TWO_PI = 2 * np.pi


def angdist(a, b):
    """|a - b| on the circle, element-wise, in [0, pi]."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs((d + np.pi) % TWO_PI - np.pi)


def periodic_weights(T, X, seed=106, regime="stress", hidden_mult=4):
    """(XNet, VNet) of a periodic dynamics: the draws of oracle.nets.init_generic_net in its order, with the layer that
    reads x twice as wide -- x_layer of XNet ([v, m x, t]), v_layer of VNet ([x, force, t])."""
    rng = np.random.default_rng(seed)
    D, Hn = 2 * T * X, hidden_mult * 2 * T * X
    kw = H.REGIMES[regime]
    hf, bs, cs = kw["head_factor"], kw["bias_std"], kw["coeff_std"]

    def net(factor, x_in, v_in):
        p = {}
        p['x_layer/W'], p['x_layer/b'] = nets._dense_init(rng, x_in, Hn, factor / 3., bs)
        p['v_layer/W'], p['v_layer/b'] = nets._dense_init(rng, v_in, Hn, 1. / 3., bs)
        p['t_layer/W'], p['t_layer/b'] = nets._dense_init(rng, 2, Hn, 1. / 3., bs)
        p['h_layer/W'], p['h_layer/b'] = nets._dense_init(rng, Hn, Hn, 1., bs)
        for name in ('scale_layer', 'translation_layer', 'transformation_layer'):
            p[name + '/W'], p[name + '/b'] = nets._dense_init(rng, Hn, D, hf, bs)
        p['coeff_scale'] = rng.standard_normal((1, D)) * cs
        p['coeff_transformation'] = rng.standard_normal((1, D)) * cs
        return p
    return net(2., 2 * D, D), net(1., D, 2 * D)


def masks_for(N, D, seed=42):
    from oracle.gauge_dynamics import make_masks
    return make_masks(N, D, np.random.RandomState(seed))


class NumpyPeriodic:
    """The periodic trajectory in NumPy at `dtype` (float64: the reference; float32: the yardstick)."""

    def __init__(self, T, X, N, eps, masks, xnet, vnet, dtype=np.float64):
        self.T, self.X, self.N, self.dtype = T, X, N, dtype
        self.eps = dtype(eps)
        self.mask = np.asarray(masks).astype(dtype)
        self.xnet = {k: np.asarray(v).astype(dtype) for k, v in xnet.items()}
        self.vnet = {k: np.asarray(v).astype(dtype) for k, v in vnet.items()}

    def plaq(self, x):
        s = x.reshape(x.shape[0], self.T, self.X, 2)
        return s[..., 0] - s[..., 1] - np.roll(s[..., 0], -1, 2) + np.roll(s[..., 1], -1, 1)

    def action(self, x):
        return np.sum(1 - np.cos(self.plaq(x)), axis=(1, 2))

    def force(self, x):
        sp = np.sin(self.plaq(x))
        return np.stack([sp - np.roll(sp, 1, 2), -sp + np.roll(sp, 1, 1)], axis=-1).reshape(x.shape[0], -1)

    @staticmethod
    def net(p, a, b, t):
        h = (a @ p['v_layer/W'] + p['v_layer/b']) + (b @ p['x_layer/W'] + p['x_layer/b']) \
            + (t @ p['t_layer/W'] + p['t_layer/b'])
        h = np.maximum(h, 0)
        h = np.maximum(h @ p['h_layer/W'] + p['h_layer/b'], 0)
        S = np.tanh(h @ p['scale_layer/W'] + p['scale_layer/b']) * np.exp(p['coeff_scale'])
        Tr = h @ p['translation_layer/W'] + p['translation_layer/b']
        Q = (h @ p['transformation_layer/W'] + p['transformation_layer/b']) * np.exp(p['coeff_transformation'])
        return S, Tr, Q

    @staticmethod
    def feats(x):
        return np.concatenate([np.cos(x), np.sin(x)], axis=1)

    def _time(self, i, B):
        arg = TWO_PI * i / self.N
        return np.tile(np.array([[np.cos(arg), np.sin(arg)]]).astype(self.dtype), (B, 1))

    def upd_v(self, x, v, beta, t, bwd):
        g = beta * self.force(x)
        S, Tr, Q = self.net(self.vnet, self.feats(x), g, t)
        eps, h = self.eps, self.dtype(0.5)
        if not bwd:
            s = S * (h * eps)
            return v * np.exp(s) - h * eps * (np.exp(Q * eps) * g - Tr), s.sum(1)
        s = S * (-h * eps)
        return np.exp(s) * (v + h * eps * (np.exp(Q * eps) * g - Tr)), s.sum(1)

    def upd_x(self, x, v, t, keep, bwd):
        omk = 1 - keep
        S, Tr, Q = self.net(self.xnet, v, np.concatenate([keep, keep]) * self.feats(x), t)
        eps, h, two = self.eps, self.dtype(0.5), self.dtype(2)
        drift = eps * (np.exp(Q * eps) * v + Tr)
        s = S * (-eps if bwd else eps)
        es = np.exp(s)
        w = x - drift if bwd else x
        sh, ch = np.sin(h * w), np.cos(h * w)
        y = two * np.arctan2(es * sh, ch)
        if not bwd:
            y = y + drift
        ld = omk * (s - np.log(ch * ch + es * es * sh * sh))
        return keep * x + omk * y, ld.sum(1)

    def leapfrog(self, x, v, beta, step, bwd):
        i = self.N - step - 1 if bwd else step
        t = self._time(i, x.shape[0])
        m = self.mask[i]
        mi = 1 - m
        v, l1 = self.upd_v(x, v, beta, t, bwd)
        x, l2 = self.upd_x(x, v, t, mi if bwd else m, bwd)
        x, l3 = self.upd_x(x, v, t, m if bwd else mi, bwd)
        v, l4 = self.upd_v(x, v, beta, t, bwd)
        return x, v, l1 + l2 + l3 + l4

    def trajectory(self, x0, v0, beta, bwd=False):
        """-> (x_N, v_N, p, sumlogdet); beta a number or one value per row."""
        dt = self.dtype
        x, v = np.asarray(x0).astype(dt), np.asarray(v0).astype(dt)
        x0, v0 = x, v
        beta = np.asarray(beta).astype(dt)
        bcol = beta[:, None] if beta.ndim else beta
        ld = np.zeros(x.shape[0], dtype=dt)
        for step in range(self.N):
            x, v, j = self.leapfrog(x, v, bcol, step, bwd)
            ld = ld + j
        h0 = beta * self.action(x0) + dt(0.5) * (v0 ** 2).sum(1)
        h1 = beta * self.action(x) + dt(0.5) * (v ** 2).sum(1)
        with np.errstate(over='ignore', invalid='ignore'):
            p = np.exp(np.minimum(h0 - h1 + ld, 0))
        return x, v, np.where(np.isfinite(p), p, 0).astype(dt), ld

    def apply_transition(self, x, beta, v0f, v0b, coin, u):
        xf, vf, pf, _ = self.trajectory(x, v0f, beta, False)
        xb, vb, pb, _ = self.trajectory(x, v0b, beta, True)
        fm = (np.asarray(coin) > 0.5).astype(self.dtype)
        bm = 1 - fm
        xp = fm[:, None] * xf + bm[:, None] * xb
        vp = fm[:, None] * vf + bm[:, None] * vb
        p = fm * pf + bm * pb
        am = (p > np.asarray(u)).astype(self.dtype)
        return xp, vp, p, am[:, None] * xp + (1 - am)[:, None] * np.asarray(x).astype(self.dtype)


def _feats_t(x):
    return torch.cat([torch.cos(x), torch.sin(x)], dim=1)


class TorchPeriodic(TorchGaugeModel):
    """oracle.torch_ref.TorchGaugeModel with the periodic sub-updates: float64 autograd of the same loss.  Records the
    smallest |pre-activation| of any relu and whether beta is a per-row tensor."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.min_preact = np.inf         # smallest |pre-activation| of any relu so far
        self.min_clamp = np.inf          # smallest |H0 - H1 + sumlogdet| so far: 0 is where p = exp(min(., 0)) kinks

    def trajectory(self, x0, v0, beta, bwd):
        x, v, p, ld = super().trajectory(x0, v0, beta, bwd)
        with torch.no_grad():
            dh = self._energy(x0, beta) + 0.5 * (v0 ** 2).sum(1) - self._energy(x, beta) - 0.5 * (v ** 2).sum(1) + ld
            self.min_clamp = min(self.min_clamp, float(dh.abs().min()))
        return x, v, p, ld

    def flip_free(self, margin=1e-5):
        """No relu pre-activation within `margin` of 0 and no accept probability within `margin` of its clamp at 1
        (p = exp(min(dH, 0)): |dH| > margin, so neither p in (1 - margin, 1) nor a clamped p that rounding could
        unclamp): float32 rounding cannot move a gradient by a whole row."""
        return self.min_preact > margin and self.min_clamp > margin

    def _net(self, p, inputs):
        v, x, t = inputs
        h1 = (v @ p['v_layer/W'] + p['v_layer/b']) + (x @ p['x_layer/W'] + p['x_layer/b']) \
            + (t @ p['t_layer/W'] + p['t_layer/b'])
        h2 = torch.relu(h1) @ p['h_layer/W'] + p['h_layer/b']
        self.min_preact = min(self.min_preact, float(h1.detach().abs().min()), float(h2.detach().abs().min()))
        h = torch.relu(h2)
        S = torch.tanh(h @ p['scale_layer/W'] + p['scale_layer/b']) * torch.exp(p['coeff_scale'])
        Tr = h @ p['translation_layer/W'] + p['translation_layer/b']
        Q = (h @ p['transformation_layer/W'] + p['transformation_layer/b']) * torch.exp(p['coeff_transformation'])
        return S, Tr, Q

    @staticmethod
    def _col(beta):
        return beta[:, None] if torch.is_tensor(beta) and beta.dim() else beta

    def _force(self, x, beta):
        return self._col(beta) * super()._force(x, 1.0)

    def _upd_v(self, x, v, beta, t, bwd):
        g = self._force(x, beta)
        S, Tr, Q = self._net(self.vnet, [_feats_t(x), g, t])
        eps = self.eps
        if not bwd:
            s = S * (0.5 * eps)
            return v * torch.exp(s) - 0.5 * eps * (torch.exp(Q * eps) * g - Tr), s.sum(1)
        s = S * (-0.5 * eps)
        return torch.exp(s) * (v + 0.5 * eps * (torch.exp(Q * eps) * g - Tr)), s.sum(1)

    def _upd_x(self, x, v, t, m, mi, bwd):
        S, Tr, Q = self._net(self.xnet, [v, torch.cat([m, m]) * _feats_t(x), t])
        eps = self.eps
        drift = eps * (torch.exp(Q * eps) * v + Tr)
        s = S * (-eps if bwd else eps)
        es = torch.exp(s)
        w = x - drift if bwd else x
        sh, ch = torch.sin(0.5 * w), torch.cos(0.5 * w)
        y = 2. * torch.atan2(es * sh, ch)
        if not bwd:
            y = y + drift
        ld = mi * (s - torch.log(ch * ch + es * es * sh * sh))
        return m * x + mi * y, ld.sum(1)
