"""numpy restatement of the diffusion-noise contract (include/ovla.h "Diffusion noise") and of what `csrc/diffusion_noise.hip` computes.
Nothing here needs a GPU.  Box-Muller is evaluated in float64: the kernel's fp32 evaluation is compared against it with a derived bound.

    generator   Philox4x32-10 (tests/lora_dropout_reference.py): counter (c0, c1, c2, c3), key (seed_lo, seed_hi)
    timestep    o = philox(0, b, 1, call);  t_b = (o[0] * T) >> 32
    noise       elements 4 j .. 4 j + 3 of sample b from o = philox(j, b, stream, call); (o[0], o[1]) -> 4 j, 4 j + 1; (o[2], o[3]) -> 4 j + 2, 4 j + 3
                u1 = ((w_a >> 8) + 1) 2^-24,  u2 = (w_b >> 8) 2^-24,  r = sqrt(-2 ln u1),  z_even = r cos(2 pi u2),  z_odd = r sin(2 pi u2)
    noisy       bf16(ab[t][0] * float(actions) + ab[t][1] * float(bf16(z))) with fp32 operations rounded one by one
"""
import numpy as np

from lora_dropout_reference import MASK32, bf16_bits_to_f32, f32_to_bf16_bits, philox4x32_10, seed_words

STREAM_TRAIN, STREAM_TIMESTEP, STREAM_SAMPLER = 0, 1, 2
Z_MAX = float(np.sqrt(48.0 * np.log(2.0)))     # u1 = 2^-24: the largest |z| the construction can produce (5.77)


def words(c0, b, stream, call, seed):
    """The four output words (uint64 arrays of 32-bit values) for counter (c0, b, stream, call)."""
    lo, hi = seed_words(seed)
    c0, b = np.asarray(c0, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    c0, b = np.broadcast_arrays(c0, b)
    return philox4x32_10(c0, b, np.full(c0.shape, int(stream) & MASK32, np.uint64), np.full(c0.shape, int(call) & MASK32, np.uint64), lo, hi)


def timesteps(B, T, *, call, seed, b0=0):
    """int64 [B]: the training timestep of samples b0 .. b0 + B - 1."""
    o = words(np.zeros(B, np.uint64), np.arange(b0, b0 + B, dtype=np.uint64), STREAM_TIMESTEP, call, seed)
    return ((o[0] * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


def box_muller(wa, wb):
    """Two generator words -> (z_even, z_odd) in float64."""
    u1 = ((wa >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (wb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    c, s = cos_sin_2pi(u2)
    return r * c, r * s


def cos_sin_2pi(u):
    """(cos(2 pi u), sin(2 pi u)) in float64 for u in [0, 1) with an EXACT argument reduction (u is a multiple of 2^-24): 2 u = q / 2 + f with q
    an integer quadrant and |f| <= 1/4, both exact, so the zeros at u = 0, 1/4, 1/2, 3/4 are zeros and not 1e-16 (2 pi u rounded to float64)."""
    y = 2.0 * np.asarray(u, dtype=np.float64)
    q = np.rint(2.0 * y)
    f = y - 0.5 * q
    c0, s0 = np.cos(np.pi * f), np.sin(np.pi * f)
    q = q.astype(np.int64) & 3
    c = np.choose(q, [c0, -s0, -c0, s0])
    s = np.choose(q, [s0, c0, -s0, -c0])
    return c + 0.0, s + 0.0          # (-0.0 + 0.0 = +0.0: the sign of a zero is not part of the contract)


def normals(B, n, *, call, seed, stream=STREAM_TRAIN, b0=0):
    """float64 [B, n]: the unrounded N(0, 1) values of samples b0 .. b0 + B - 1."""
    assert stream != STREAM_TIMESTEP
    nq = (n + 3) // 4
    o = words(np.arange(nq, dtype=np.uint64)[None, :], np.arange(b0, b0 + B, dtype=np.uint64)[:, None], stream, call, seed)
    z = np.empty((B, nq, 4), dtype=np.float64)
    z[:, :, 0], z[:, :, 1] = box_muller(o[0], o[1])
    z[:, :, 2], z[:, :, 3] = box_muller(o[2], o[3])
    return z.reshape(B, nq * 4)[:, :n]


def add_noise_bits(actions_bits, noise_bits, ab, t):
    """uint16 [B, n]: bf16(ab[t][0] * actions + ab[t][1] * noise), two fp32 multiplies and one fp32 add (numpy float32 arithmetic never fuses)."""
    ab = np.asarray(ab, dtype=np.float32)
    a0, a1 = ab[t, 0][:, None], ab[t, 1][:, None]
    x = (a0 * bf16_bits_to_f32(actions_bits)).astype(np.float32)
    y = (a1 * bf16_bits_to_f32(noise_bits)).astype(np.float32)
    return f32_to_bf16_bits((x + y).astype(np.float32))


def bf16_bracket(z):
    """float64 z -> (lo, hi) float64: the adjacent bf16 values with lo <= z <= hi (lo == hi where z is a bf16 value)."""
    z = np.asarray(z, dtype=np.float64)
    bits = (z.astype(np.float32).view(np.uint32) >> 16).astype(np.int64)          # truncated toward zero, sign-magnitude
    order = np.where(bits & 0x8000, -(bits & 0x7FFF), bits & 0x7FFF)             # an integer that orders the bf16 values
    cand = np.stack([order - 1, order, order + 1])
    cbits = np.where(cand < 0, (-cand) | 0x8000, cand).astype(np.uint16)
    vals = bf16_bits_to_f32(cbits).astype(np.float64)
    lo = np.where(vals <= z, vals, -np.inf).max(0)
    hi = np.where(vals >= z, vals, np.inf).min(0)
    return lo, hi


def bf16_ulp(z):
    """Spacing of the bf16 values at |z| (normal range)."""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(z, dtype=np.float64)), 2.0 ** -126)))
    return 2.0 ** (e - 7)
