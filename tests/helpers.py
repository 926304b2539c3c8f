"""Shared builders for the parity tests: an oracle and a HIP-backed dynamics
object holding the same weights, masks and step size."""
import ctypes as C

import numpy as np

from oracle import nets
from oracle import dynamics as ogen
from oracle.gauge_dynamics import GaugeDynamicsOracle, make_masks

REGIMES = {
    # reference initialisation (generic_net.py:39-90): heads factor 0.001, zero biases/coeffs
    "init": dict(head_factor=0.001, bias_std=0.0, coeff_std=0.0),
    # SURVEY.md 8d "stress": eps*S, eps*Q reach O(0.3) so exp / tanh / log-det paths matter
    "stress": dict(head_factor=0.1, bias_std=0.05, coeff_std=0.2),
    # same paths exercised, gentle enough to stay finite over 10+ leapfrog steps at D=128
    "mild": dict(head_factor=0.01, bias_std=0.02, coeff_std=0.1),
}


def relerr(got, want):
    """max |got - want| relative to the tensor's own scale (>= 1)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / max(1.0, np.max(np.abs(want)))) if want.size else 0.0


def gauge_weights(T, X, seed=106, regime="stress", hidden_mult=4):
    rng = np.random.default_rng(seed)
    D = 2 * T * X
    kw = REGIMES[regime]
    xp = nets.init_generic_net(rng, D, hidden_mult * D, 2., **kw)
    vp = nets.init_generic_net(rng, D, hidden_mult * D, 1., **kw)
    return xp, vp


def conv_weights(T, X, seed=106, regime="stress", F=None):
    """ConvNet3D as gauge_dynamics.py:121-143 builds it: F = space_size (unless given), H = 2 * x_dim."""
    rng = np.random.default_rng(seed)
    D = 2 * T * X
    F = X if F is None else F
    kw = REGIMES[regime]
    xp = nets.init_conv3d_net(rng, (T, X), D, 2 * D, F, 2., **kw)
    vp = nets.init_conv3d_net(rng, (T, X), D, 2 * D, F, 1., **kw)
    return xp, vp


def gauge_oracle(T, X, num_steps, eps, xp, vp, hmc=False, dtype=np.float64, mask_seed=42, arch='generic'):
    masks = make_masks(num_steps, 2 * T * X, np.random.RandomState(mask_seed))
    return GaugeDynamicsOracle(T, X, num_steps, eps, masks, xp, vp, arch, hmc=hmc, dtype=dtype)


def gauge_hip(T, X, num_steps, eps, xp, vp, masks, batch, hmc=False, both_directions=True, arch='generic'):
    from l2hmc_amd import GaugeLattice, GaugeDynamics
    lat = GaugeLattice(T, X, 2, 'U1', num_samples=batch, rand=False)
    dyn = GaugeDynamics(lat, lat.get_energy_function(), eps=eps, hmc=hmc, network_arch=arch,
                        num_steps=num_steps, eps_trainable=True, data_format='channels_last',
                        both_directions=both_directions)
    dyn.set_masks(masks)
    if not hmc:
        dyn.position_fn.load_state(xp)
        dyn.momentum_fn.load_state(vp)
    return dyn


def gauge_inputs(B, D, seed=103):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 2 * np.pi, (B, D))
    v0f = np.random.default_rng(seed + 1000).standard_normal((B, D))
    v0b = np.random.default_rng(seed + 1001).standard_normal((B, D))
    coin = np.random.default_rng(seed + 2000).uniform(size=B)
    u = np.random.default_rng(seed + 3000).uniform(size=B)
    return x, v0f, v0b, coin, u


def mog_target_oracle():
    """cfg 2: means on the axes, sigma^2 = 0.025 I, equal weights (mog_model.py:1063-1120)."""
    return ogen.GMM([np.array([1., 0.]), np.array([0., 1.])], [0.025 * np.eye(2)] * 2, [0.5, 0.5])


def scg_target_oracle():
    """cfg 1: strongly correlated Gaussian (SCGExperiment.ipynb cell 3)."""
    return ogen.Gaussian(np.zeros(2), np.array([[50.05, -49.95], [-49.95, 50.05]]))


def mlp_weights(x_dim, num_nodes, seed=106, regime="stress"):
    rng = np.random.default_rng(seed)
    kw = REGIMES[regime]
    return (nets.init_mlp_net(rng, x_dim, 2., num_nodes, **kw),
            nets.init_mlp_net(rng, x_dim, 1., num_nodes, **kw))


# ---- HIP graph capture (shared by the capture tests)
def _hip():
    """The HIP runtime this process already runs on (torch's own copy first, if it ships one)."""
    paths = sorted({l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l}, key=lambda p: "torch" not in p)
    assert paths, "the HIP runtime is not mapped into this process"
    return C.CDLL(paths[0])


def _graph_shape(hip, stream):
    """(kernel nodes, other nodes, edges) of the graph `stream` is capturing into."""
    status, gid, graph = C.c_int(), C.c_ulonglong(), C.c_void_p()
    deps, ndeps = C.c_void_p(), C.c_size_t()
    assert hip.hipStreamGetCaptureInfo_v2(C.c_void_p(stream), C.byref(status), C.byref(gid), C.byref(graph),
                                          C.byref(deps), C.byref(ndeps)) == 0
    assert status.value == 1 and graph.value                        # hipStreamCaptureStatusActive
    n = C.c_size_t()
    assert hip.hipGraphGetNodes(graph, None, C.byref(n)) == 0
    nodes = (C.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, C.byref(n)) == 0
    kernels = 0
    for i in range(n.value):
        kind = C.c_int()
        assert hip.hipGraphNodeGetType(C.c_void_p(nodes[i]), C.byref(kind)) == 0
        kernels += kind.value == 0                                  # hipGraphNodeTypeKernel
    e = C.c_size_t()
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(e)) == 0
    return kernels, n.value - kernels, e.value
