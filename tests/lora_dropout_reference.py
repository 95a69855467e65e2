"""numpy restatement of the LoRA-dropout mask contract (include/ovla.h "LoRA dropout") and of what the three kernels of
`csrc/lora_dropout.hip` compute.  Nothing here needs a GPU.

    generator   Philox4x32-10: counter (q_lo, q_hi, module, call), key (seed_lo, seed_hi), q = m * (K / 8) + (k >> 3)
    columns     output word w -> column 8 (k >> 3) + 2 w (low 16 bits) and + 2 w + 1 (high 16 bits)
    keep        u16 >= thr,  thr = floor(float32(p) * 65536)
    value       kept: bf16_rne(float32(x) * inv), inv = float32(1) / (float32(1) - float32(p));  dropped: +0
"""
import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF

# (counter, key) -> output
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((MASK32,) * 4, (MASK32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Four uint32 arrays (or scalars) of counter words and two of key words -> the four output words (uint64 arrays holding 32-bit values)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK32, int(k1) & MASK32
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def threshold(p):
    return int(np.floor(float(np.float32(p)) * 65536.0))


def inv_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def seed_words(seed):
    return int(seed) & MASK32, (int(seed) >> 32) & MASK32


def keep_mask(M, K, *, module, call, seed, p):
    """bool [M, K]: True where the element is kept."""
    assert K % 8 == 0 and 0.0 <= p < 1.0
    nv = K // 8
    q = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(nv) + np.arange(nv, dtype=np.uint64)[None, :]
    lo, hi = seed_words(seed)
    words = philox4x32_10(q & MASK32, q >> 32, np.full_like(q, int(module) & MASK32), np.full_like(q, int(call) & MASK32), lo, hi)
    u16 = np.empty((M, nv, 8), dtype=np.uint64)
    for w in range(4):
        u16[:, :, 2 * w] = words[w] & 0xFFFF
        u16[:, :, 2 * w + 1] = words[w] >> 16
    return (u16 >= threshold(p)).reshape(M, K)


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(x):
    """Round to nearest even; NaN stays NaN."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + 0x7FFF
    out = ((u.astype(np.uint64) + r) >> 16).astype(np.uint16)
    return np.where(np.isnan(np.asarray(x, dtype=np.float32)), np.uint16(0x7FC0), out)


def dropout_bits(x_bits, keep, p):
    """uint16 bf16 bit patterns of dropout(x): float32 multiply, round to nearest even, +0 where dropped."""
    with np.errstate(over="ignore"):          # (a dropped element may overflow here; its product is discarded)
        scaled = f32_to_bf16_bits(bf16_bits_to_f32(x_bits) * inv_scale(p))
    return np.where(keep, scaled, np.uint16(0))


# ---- torch conveniences (bf16 tensors in, bf16 tensors out) --------------------------------------------------------------------------------
def to_bits(t):
    import torch
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(bits):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def dropout(x, *, module, call, seed, p):
    """dropout_module(x) for a CPU / GPU bf16 tensor [M, K] -> CPU bf16 tensor."""
    M, K = x.shape
    return from_bits(dropout_bits(to_bits(x), keep_mask(M, K, module=module, call=call, seed=seed, p=p), p))
