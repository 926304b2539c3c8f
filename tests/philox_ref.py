"""The library's random streams in plain Python / NumPy: Philox4x32-10 (Salmon et al., SC'11) in integers, the word ->
float maps of l2hmc_amd/csrc/common.h, and the element layouts by which the kernels hand the draws to chains and steps
(include/l2hmc_hip.h).  One copy, for the host and the GPU tests alike; nothing here touches the library.

Block b of the stream (seed, stream) is philox(counter = {b_lo, b_hi, stream_lo, stream_hi}, key = {seed_lo, seed_hi});
element i of a stream is word i & 3 of block i >> 2.  seed and stream are taken over the full 64 bits and are never
reduced: a value outside [0, 2^64) is an error of the caller, not a wrap."""
import numpy as np

M32 = 0xFFFFFFFF
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox(block, offset, seed):
    """Philox4x32-10 in Python integers: the four words of block `block` of stream (seed, offset)."""
    c = [block & M32, block >> 32, offset & M32, offset >> 32]
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        p0, p1 = c[0] * _M0, c[2] * _M1
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return c


def philox_raw(counter, key):
    """The same function on a counter of four and a key of two 32-bit words (the form of Random123's known answers)."""
    return philox(counter[0] | counter[1] << 32, counter[2] | counter[3] << 32, key[0] | key[1] << 32)


def _u64(name, v):
    v = int(v)
    if not 0 <= v < 2 ** 64:
        raise ValueError(f"{name} = {v} is outside [0, 2^64)")
    return v


def blocks(seed, stream, block):
    """`philox` on an array of block indices: uint64 [..., 4] holding the 32-bit words."""
    seed, stream = _u64("seed", seed), _u64("stream", stream)
    b = np.asarray(block, dtype=np.uint64)
    m = np.uint64(M32)
    s32 = np.uint64(32)
    c = [b & m, b >> s32, np.full_like(b, stream & M32), np.full_like(b, stream >> 32)]
    k0, k1 = seed & M32, seed >> 32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)          # 32 x 32 bits: no overflow in 64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return np.stack(c, axis=-1)


def _index(i):
    i = np.asarray(i, dtype=np.int64)
    if i.size and i.min() < 0:
        raise ValueError("negative element index")
    return i


def word(seed, stream, i):
    """Word of element(s) i of the stream: uint64 holding 32 bits."""
    i = _index(i)
    w = blocks(seed, stream, i >> 2)
    return np.take_along_axis(w, (i & 3)[..., None], axis=-1)[..., 0]


def uniform(seed, stream, i):
    """Element(s) i of what l2hmc_fill_uniform writes for (seed, stream): float32 in [0, 1), bit exact."""
    return ((word(seed, stream, i) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def _u01_open(w):
    """u01_open of common.h, in float32 as the device forms it.  For w >> 8 >= 2^23 the sum with 0.5 is not
    representable and rounds to the even neighbour, so the top word gives exactly 1.0: that is what the device does, and
    it is reproduced here, not repaired."""
    return ((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def normal(seed, stream, i):
    """Element(s) i of what l2hmc_fill_normal writes for (seed, stream), in float64: Box-Muller on the word pairs (0, 1)
    -> elements 0, 1 and (2, 3) -> elements 2, 3 of a block, from the device's float32 uniforms."""
    i = _index(i)
    w = blocks(seed, stream, i >> 2)
    h = ((i & 3) >> 1)[..., None]
    u1 = np.take_along_axis(_u01_open(w), 2 * h, axis=-1)[..., 0].astype(np.float64)
    u2 = np.take_along_axis(_u01_open(w), 2 * h + 1, axis=-1)[..., 0].astype(np.float64)
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return np.where(i & 1, rad * np.sin(ang), rad * np.cos(ang))


def uniforms(seed, stream, n):
    return uniform(seed, stream, np.arange(n))


def normals(seed, stream, n):
    return normal(seed, stream, np.arange(n))


# ----------------------------------------------------------------- element layouts
def lattice_step_streams(draw):
    """A lattice step of draw index d takes the streams 2 d (momenta) and 2 d + 1 (coin | u); d < 2^63."""
    draw = int(draw)
    if not 0 <= draw < 2 ** 63:
        raise ValueError(f"draw = {draw} is outside [0, 2^63)")
    return 2 * draw, 2 * draw + 1


def lattice_step(seed, draw, B, D, draw_fn=(normal, uniform)):
    """(v0_f [B, D], v0_b [B, D], coin [B], u [B]) of l2hmc_gauge_mcmc_step: V[dir * B + chain][d] on stream 2 draw,
    coin[chain] | u[B + chain] on stream 2 draw + 1."""
    sv, su = lattice_step_streams(draw)
    V = draw_fn[0](seed, sv, np.arange(2 * B * D)).reshape(2, B, D)
    cu = draw_fn[1](seed, su, np.arange(2 * B))
    return V[0], V[1], cu[:B], cu[B:]


def lattice_run_draws(draw0, n_steps, swap_every=None, swap_phase=0):
    """The draw index of every step of a lattice run and the stream of every exchange round in it.  Without rounds step
    s draws with index draw0 + s.  With rounds (a round after step s iff (swap_phase + s + 1) % swap_every == 0) a step
    at index d leaves one stream counter at 2 d + 2, the round after it takes stream 2 d + 2, and the step after a round
    has index d + 2 (stream 2 d + 3 is skipped).  Returns (step draw indices, round streams)."""
    d, steps, rounds = int(draw0), [], []
    for s in range(n_steps):
        steps.append(d)
        lattice_step_streams(d)
        if swap_every is not None and (swap_phase + s + 1) % swap_every == 0:
            rounds.append(_u64("stream", 2 * d + 2))
            d += 2
        else:
            d += 1
    return steps, rounds


def toy_step(seed, draw0, s, B, x_dim, draw_fn=(normal, uniform)):
    """(direction uniforms [B], forward momenta [B, x_dim], backward momenta [B, x_dim], MH uniforms [B]) of step s of a
    toy L2HMC run (l2hmc_small_propose at draw0 + 4 s): the streams draw0 + 4 s + 0 .. 3."""
    st = [_u64("stream", int(draw0) + 4 * s + k) for k in range(4)]
    n = np.arange(B * x_dim)
    return (draw_fn[1](seed, st[0], np.arange(B)), draw_fn[0](seed, st[1], n).reshape(B, x_dim),
            draw_fn[0](seed, st[2], n).reshape(B, x_dim), draw_fn[1](seed, st[3], np.arange(B)))


def toy_hmc_run_streams(draw0, n_steps, swap_every=None, swap_phase=0):
    """The streams of a toy plain-HMC run in the order it takes them: a step two (momenta, MH uniforms), a round after
    step s iff (swap_phase + s + 1) % swap_every == 0 the next one.  Returns ([(momenta, uniforms) per step], [round
    streams])."""
    st, steps, rounds = int(draw0), [], []
    for s in range(n_steps):
        steps.append((_u64("stream", st), _u64("stream", st + 1)))
        st += 2
        if swap_every is not None and (swap_phase + s + 1) % swap_every == 0:
            rounds.append(_u64("stream", st))
            st += 1
    return steps, rounds


def toy_hmc_step(seed, draw0, s, B, x_dim, draw_fn=(normal, uniform)):
    """(momenta [B, x_dim], MH uniforms [B]) of step s of l2hmc_small_hmc_run: the streams draw0 + 2 s and + 1."""
    sv, su = toy_hmc_run_streams(draw0, s + 1)[0][s]
    return draw_fn[0](seed, sv, np.arange(B * x_dim)).reshape(B, x_dim), draw_fn[1](seed, su, np.arange(B))
