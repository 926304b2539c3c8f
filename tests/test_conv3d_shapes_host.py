"""ConvNet3D away from square lattices with num_filters = extent: the reference side of
tests/test_gpu_conv3d_shapes.py, float64 alone (no GPU).

1. The two float64 restatements of conv_net.py:247-280 -- NumPy shifted sums (oracle/nets.py) and
   torch.nn.functional.conv3d (oracle/torch_ref.py) -- agree to 1e-12 at every shape of the GPU comparisons.
2. Power controls.  A kernel that mixes T with X in an index is the identity on a square lattice; the GPU
   comparisons only mean something where such a mix-up moves the answer.  Three altered evaluations of the
   reference must each move S, T and Q by more than 100 x TOL_OP (relerr: max deviation over the tensor's scale):
     - links_shape transposed to (X, T, 2)             (the identity where T == X: not asked there);
     - the flattened features in (j, i, g) order        (the identity where T/4 == 1 or X/4 == 1, as is the index
                                                        mix-up it stands for, I2 * X4 + J2 against J2 * T4 + I2:
                                                        asked where both are > 1);
     - the conv taps di / dj swapped                    (every shape).
   Measured ("stress" weights): every movement lies between 0.20 and 0.60; the smallest is T at 8 x 16 / F = 16
   with links_shape transposed (0.197), i.e. 200 x the bar.
3. oracle.nets.init_conv3d_net takes a (T, X) pair; for a square lattice it returns, bit for bit, what it
   returned when it took the extent alone.
4. The launch forms the shapes are chosen for (chains per workgroup, partial last workgroup, ragged trunk, the
   wider-filter-set loop), through mirrors of the launchers' rules (tests/conv3d_cases.py)."""
import numpy as np
import pytest
import torch

from oracle import nets as onets, torch_ref
from tests import conv3d_cases as CC
from tests import helpers as H

TOL_OP = 1e-5                    # tests/test_gpu_parity.py (a GPU module: not imported here)
MOVE = 100 * TOL_OP
SHAPES = sorted({c[:3] for c in CC.STQ_CASES} | {c[:3] for c in CC.TRAIN_CASES})
ROWS = 3


@pytest.fixture(scope="module")
def refs():
    """shape -> (p, inputs, (S, T, Q)) of the unaltered float64 NumPy evaluation, computed once."""
    out = {}
    for T, X, F in SHAPES:
        xp, a, b, t, want = CC.stq_reference(T, X, F, ROWS)
        p = {k: CC.f32(v) for k, v in xp.items()}
        out[T, X, F] = (p, [CC.f32(a), CC.f32(b), np.tile(CC.f32(t), (ROWS, 1))], want)
    return out


@pytest.mark.parametrize("T,X,F", SHAPES)
def test_numpy_and_torch_restatements_agree(refs, T, X, F):
    p, inputs, want = refs[T, X, F]
    tt = lambda z: torch.tensor(z, dtype=torch.float64)   # noqa: E731
    got = torch_ref.conv3d_net({k: tt(v) for k, v in p.items()}, [tt(z) for z in inputs], T, X)
    for g, w in zip(got, want):
        assert H.relerr(g.numpy(), w) < 1e-12
    assert want[0].shape == (ROWS, 2 * T * X)
    assert p['x_layer/W'].shape[0] == CC.nflat(T, X, F) == onets.conv3d_flat_size((T, X), F)


def _net_flatten_ji(p, inputs, T, X, F):
    """conv3d_net with each input's features flattened over (j, i, g) instead of (i, j, g)."""
    v, x, t = inputs
    feats = []
    for z, which in ((v, 'v'), (x, 'x')):
        f = onets.conv3d_front(p, z, which, (T, X, 2)).reshape(z.shape[0], T // 4, X // 4, 2 * F)
        feats.append(f.transpose(0, 2, 1, 3).reshape(z.shape[0], -1))
    return onets.generic_net(p, [feats[0], feats[1], t])


def _moved(alt, want):
    return min(H.relerr(a, w) for a, w in zip(alt, want))


@pytest.mark.parametrize("T,X,F", [s for s in SHAPES if s[0] != s[1]])
def test_control_links_shape_transposed(refs, T, X, F):
    p, inputs, want = refs[T, X, F]
    assert _moved(onets.conv3d_net(p, inputs, (X, T, 2)), want) > MOVE


@pytest.mark.parametrize("T,X,F", [s for s in SHAPES if s[0] > 4 and s[1] > 4])
def test_control_flatten_order(refs, T, X, F):
    p, inputs, want = refs[T, X, F]
    assert _moved(_net_flatten_ji(p, inputs, T, X, F), want) > MOVE


def test_flatten_order_is_the_identity_on_one_row_or_column_of_cells(refs):
    """Why the control above is not asked at T/4 == 1 or X/4 == 1: there (i, j, g) and (j, i, g) are one order."""
    for T, X, F in [s for s in SHAPES if s[0] == 4 or s[1] == 4]:
        p, inputs, want = refs[T, X, F]
        for a, w in zip(_net_flatten_ji(p, inputs, T, X, F), want):
            np.testing.assert_array_equal(a, w)


@pytest.mark.parametrize("T,X,F", SHAPES)
def test_control_conv_taps_swapped(refs, T, X, F):
    p, inputs, want = refs[T, X, F]
    q = dict(p)
    for k in p:
        if k.startswith('conv_') and k.endswith('/W'):
            q[k] = np.ascontiguousarray(p[k].transpose(1, 0, 2, 3, 4))      # tap (di, dj) <-> (dj, di)
    assert _moved(onets.conv3d_net(q, inputs, (T, X, 2)), want) > MOVE


def _init_conv3d_net_square(rng, L, x_dim, num_hidden, num_filters, factor, head_factor=0.001, bias_std=0.0,
                            coeff_std=0.0, dtype=np.float64):
    """oracle.nets.init_conv3d_net as it was while it took a square lattice's extent only."""
    F = num_filters
    p = {}
    for s in ('x', 'v'):
        p[f'conv_{s}1/W'] = onets._glorot_uniform(rng, (3, 3, 2, 1, F), dtype)
        p[f'conv_{s}1/b'] = (rng.standard_normal(F) * bias_std).astype(dtype)
        p[f'conv_{s}2/W'] = onets._glorot_uniform(rng, (2, 2, 2, F, 2 * F), dtype)
        p[f'conv_{s}2/b'] = (rng.standard_normal(2 * F) * bias_std).astype(dtype)
    l2 = -(-(-(-L // 2)) // 2)
    nflat = l2 * l2 * 2 * F
    p['x_layer/W'], p['x_layer/b'] = onets._dense_init(rng, nflat, num_hidden, factor / 3., bias_std, dtype)
    p['v_layer/W'], p['v_layer/b'] = onets._dense_init(rng, nflat, num_hidden, 1. / 3., bias_std, dtype)
    p['t_layer/W'], p['t_layer/b'] = onets._dense_init(rng, 2, num_hidden, 1. / 3., bias_std, dtype)
    p['h_layer/W'], p['h_layer/b'] = onets._dense_init(rng, num_hidden, num_hidden, 1., bias_std, dtype)
    for name in ('scale_layer', 'translation_layer', 'transformation_layer'):
        p[name + '/W'], p[name + '/b'] = onets._dense_init(rng, num_hidden, x_dim, head_factor, bias_std, dtype)
    p['coeff_scale'] = (rng.standard_normal((1, x_dim)) * coeff_std).astype(dtype)
    p['coeff_transformation'] = (rng.standard_normal((1, x_dim)) * coeff_std).astype(dtype)
    return p


@pytest.mark.parametrize("L", [8, 16])
def test_square_lattices_keep_their_weights_bit_for_bit(L):
    D, kw = 2 * L * L, H.REGIMES["stress"]
    old_rng, int_rng = np.random.default_rng(106), np.random.default_rng(106)
    for factor, new in zip((2., 1.), H.conv_weights(L, L, regime="stress")):       # xp, then vp, from one stream
        old = _init_conv3d_net_square(old_rng, L, D, 2 * D, L, factor, **kw)
        as_int = onets.init_conv3d_net(int_rng, L, D, 2 * D, L, factor, **kw)
        assert list(old) == list(new) == list(as_int)
        for k in old:
            assert old[k].dtype == new[k].dtype and old[k].shape == new[k].shape
            assert old[k].tobytes() == new[k].tobytes() == as_int[k].tobytes(), k
    assert onets.conv3d_flat_size(L, L) == onets.conv3d_flat_size((L, L), L) == CC.nflat(L, L, L)


def test_non_square_weights_have_the_trunk_the_library_expects():
    for T, X, F in SHAPES:
        xp, vp = H.conv_weights(T, X, regime="mild", F=F)
        for p in (xp, vp):
            assert p['x_layer/W'].shape == p['v_layer/W'].shape == (CC.nflat(T, X, F), 4 * T * X)
            assert p['conv_x2/W'].shape == (2, 2, 2, F, 2 * F)
    assert H.conv_weights(4, 16)[0]['conv_x1/W'].shape[-1] == 16              # default F = X (gauge_dynamics.py:130)


def test_shapes_land_in_the_forms_they_are_chosen_for():
    assert set(CC.STQ_FORMS) == set(CC.STQ_CASES)
    for case in CC.STQ_CASES:
        T, X, F, rows = case
        assert T % 4 == 0 and X % 4 == 0 and F % 4 == 0 and not CC.is_instance(T, X, F)
        assert CC.front_form(*case) == CC.STQ_FORMS[case], case
    forms = CC.STQ_FORMS
    assert sum(1 for f in forms.values() if f[1] >= 1 and f[2] >= 1) >= 5      # full workgroups AND a partial one
    assert forms[8, 8, 20, 3][2] == 0                                          # ... and one with none
    assert CC.nflat(4, 12, 4) == 24 and CC.nflat(4, 4, 4) == 8                 # ragged trunk: Ka = Kb not 32 k
    assert CC.nflat(8, 8, 12) == 96 and CC.nflat(8, 8, 20) == 160 and CC.nflat(16, 4, 4) == 32
    for (T, X, F, N, B), cpw in CC.TRAIN_CASES.items():
        D, nf = 2 * T * X, CC.nflat(T, X, F)
        assert D % 32 == 0 and nf % 32 == 0 and not CC.is_instance(T, X, F)    # what the training entries stage
        assert min(16, max(1, 512 // ((T // 2) * (X // 2) * F))) == cpw        # conv3d_cpw
    # the loop behind the register-held slot of the backward kernel exists from F = 20 on
    assert CC.bwd_entries(16) <= CC.BWD_SLOT_ENTRIES < CC.bwd_entries(20) == 3620
    rows = {(T, X, F): 2 * B for T, X, F, N, B in CC.TRAIN_CASES}              # the x and the z chains
    assert divmod(rows[4, 8, 8], 8) == (9, 2) and divmod(rows[16, 4, 4], 8) == (2, 2)    # partial last workgroups
    assert divmod(rows[4, 16, 8], 4) == (3, 2) and divmod(rows[4, 16, 16], 2) == (7, 0)
    assert [s for s in rows if CC.single_call_trunk(*s)] == [(4, 16, 8)]
