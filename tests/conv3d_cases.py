"""Shapes, inputs and launch-form mirrors shared by tests/test_conv3d_shapes_host.py (float64 references alone)
and tests/test_gpu_conv3d_shapes.py (the HIP kernels against them): ConvNet3D away from square lattices with
num_filters = extent, i.e. the run-time-shaped instances conv3d_front_kernel<0, 0> / conv3d_front_bwd_kernel<0, 0>
(csrc/conv3d_front.hip) and the host code that carves their buffers."""
import numpy as np

from oracle import nets as onets
from tests import helpers as H

# ---- stage 1: front-end + trunk alone.  (T, X, F, rows); the comments name what each row reaches
STQ_CASES = [
    (4, 16, 16, 9),      # T/4 = 1, default F = X, D = 128
    (16, 4, 4, 9),       # X/4 = 1, smallest F, nflat = 32
    (8, 16, 16, 5),      # two chains per workgroup with an odd row count: partial last workgroup
    (12, 8, 8, 3),       # T/4 = 3 (not a power of two)
    (8, 8, 12, 7),       # F not a power of two, nflat = 96, five chains per workgroup, partial last workgroup
    (8, 8, 20, 3),       # F = 20, nflat = 160
    (4, 12, 4, 5),       # nflat = 24: ragged first dense layer, D = 96
    (4, 4, 4, 300),      # smallest lattice, nflat = 8, eight chains per workgroup, 37 full workgroups + 4 rows
    (8, 16, 16, 1),      # a single row
]
# what the forward launcher must make of them: (chains per workgroup, full workgroups, rows of the partial one)
STQ_FORMS = {
    (4, 16, 16, 9): (4, 2, 1), (16, 4, 4, 9): (8, 1, 1), (8, 16, 16, 5): (2, 2, 1), (12, 8, 8, 3): (5, 0, 3),
    (8, 8, 12, 7): (5, 1, 2), (8, 8, 20, 3): (3, 1, 0), (4, 12, 4, 5): (8, 0, 5), (4, 4, 4, 300): (8, 37, 4),
    (8, 16, 16, 1): (2, 0, 1),
}

# ---- stage 3: training gradients.  (T, X, F, N, B) -> chains per workgroup of the backward kernel.
# D, H = 2 D and nflat are multiples of 32 (what the training entries stage).  16 x 4 / F = 4 has 64 pooled conv1
# cells per chain, i.e. 512 / 64 = 8 chains per workgroup; 16 needs <= 32 cells per chain = nflat <= 16, which no
# trainable shape has.
TRAIN_CASES = {
    (4, 16, 16, 2, 7): 2,       # T/4 = 1; 2 B = 14 rows in 7 workgroups of two chains
    (16, 4, 4, 2, 9): 8,        # X/4 = 1; 18 rows: 2 full workgroups + 2 rows
    (8, 16, 16, 1, 3): 1,       # D = 256, one chain per workgroup
    (8, 8, 20, 2, 5): 1,        # 3620 gradient entries per chain > 12 x 256: the wider-filter-set tail loop
    (4, 8, 8, 2, 37): 8,        # 74 rows: 9 full workgroups + 2 rows
    (12, 8, 8, 1, 5): 2,        # T/4 = 3, nflat = 96
    # not one of the shapes the run-time instances were promised for, but a path of its own: D = 128, H = 256 and
    # 2 nflat = 128 are the widths of the 8 x 8 / F = 8 benchmark shape, so the reverse pass takes the single-call trunk
    # kernel (fused_train.hip trunk_bwd_supported) IN FRONT OF conv3d_front_bwd_kernel<0, 0>; 14 rows: 3 workgroups + 2 rows
    (4, 16, 8, 2, 7): 4,
}


def single_call_trunk(T, X, F):
    """fused_train.hip trunk_bwd_supported for ConvNet3D as gauge_dynamics.py builds it (H = 2 D)."""
    return 2 * T * X == 128 and 2 * nflat(T, X, F) == 128


def cdiv(a, b):
    return -(-a // b)


def nflat(T, X, F):
    """csrc/conv3d_front.hip conv3d_nflat: features per input after two 2 x 2 pools (T, X multiples of 4)."""
    return (T // 4) * (X // 4) * 2 * F


def is_instance(T, X, F):
    """launch_conv3d_front / launch_conv3d_front_bwd: the shapes that have compile-time kernel instances."""
    return (T, X, F) in ((8, 8, 8), (16, 16, 16))


def front_cpw(T, X, F):
    """launch_conv3d_front, run-time form: chains per workgroup of the FORWARD kernel."""
    per_chain = (T // 2) * (X // 2) * F
    cpw = 1 if per_chain >= 1024 else min(8, 1024 // per_chain)
    return 2 if 1024 <= per_chain < 4096 else cpw


def front_form(T, X, F, rows):
    cpw = front_cpw(T, X, F)
    return cpw, rows // cpw, rows % cpw


def bwd_entries(F):
    """conv3d_front_bwd_kernel: compact gradient entries of one chain, w1 | b1 | w2 (dd = 0 slice) | b2."""
    return 19 * F + 8 * F * F + 2 * F


BWD_SLOT_ENTRIES = 12 * 256       # kSlotRegs * NTHR of the run-time instance: entries its register-held slot covers


def stq_inputs(T, X, rows, seed=5, angle=0.7):
    """The inputs of test_stq_conv3d_matches_oracle at another shape: a ~ N(0, 1), b ~ U(0, 6.3), one time."""
    D = 2 * T * X
    rng = np.random.default_rng(seed)
    a, b = rng.standard_normal((rows, D)), rng.uniform(0, 6.3, (rows, D))
    t = np.array([[np.cos(angle), np.sin(angle)]])
    return a, b, t


def f32(z):
    return np.asarray(z).astype(np.float32).astype(np.float64)


def stq_reference(T, X, F, rows, regime="stress", bmask=None):
    """(xp, a, b, t, (S, T, Q)): float64 oracle/nets.conv3d_net on fp32-rounded weights and inputs."""
    xp, _ = H.conv_weights(T, X, regime=regime, F=F)
    a, b, t = stq_inputs(T, X, rows)
    p32 = {k: f32(v) for k, v in xp.items()}
    b_in = f32(b) if bmask is None else f32(b) * f32(bmask)
    want = onets.conv3d_net(p32, [f32(a), b_in, np.tile(f32(t), (rows, 1))], (T, X, 2))
    return xp, a, b, t, want
