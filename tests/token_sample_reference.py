"""numpy / float64 restatement of THE SAMPLING CONTRACT (include/ovla.h "Token sampling and the policy-gradient objective") and of what the two
kernels of `csrc/token_sample.hip` compute.  Nothing here needs a GPU.

    scale       invT = float32(1) / float32(T);  s_j = float32(z_j) * invT, one rounded fp32 product
    generator   Philox4x32-10 (tests/lora_dropout_reference.py): counter (j >> 2, row_key, 3, call), key (seed_lo, seed_hi), word j & 3,
                with j the ABSOLUTE token id
    uniform     u = (2 (w >> 9) + 1) 2^-24, exact
    Gumbel      g = -log(-log(u));  key_j = s_j + g;  token = lowest index of the maximum key over [lo, hi)
    logprob     s_token - logsumexp(s over the window);  entropy = logsumexp - sum_j p_j s_j

The reference evaluates g and the keys in float64 from the SAME fp32 s_j and reports, per row, the two largest keys and a bound `e` on the
error of a key computed in fp32 as the contract says:
    a = -logf(u):        |da| <= L ulp(a) <= L 2^-23 a            (L = LOGF_ULPS, the accurate logf)
    g = -logf(a):        |dg| <= |da| / a + L ulp(g) <= L 2^-23 (1 + |g|)
    key = s + g:         one rounded add, 2^-24 |key|;  the product s_j is part of the contract and is reproduced exactly (its rounding,
                         2^-24 |s_j|, is added all the same: a twin that rounded it otherwise would still be inside)
    e = L 2^-23 (1 + |g|) + 2^-24 |s| + 2^-24 |key|               (|g| <= 16.64: e <= 5e-6 + 2^-23 |key|, below 2e-5 for |key| < 32)
The kernel's token must equal the reference's wherever the two largest float64 keys are further apart than max(4 e, NEAR_TIE).
"""
import numpy as np
import torch

from tests.lora_dropout_reference import MASK32, philox4x32_10, seed_words
from tests.pointwise_reference import U32, token_ce_ref

LOGF_ULPS = 2.0           # logf in the HIP math tables (OpenCL's full-profile bound is 3; CUDA's table says 1)
NEAR_TIE = 1e-3
GUMBEL_MIN, GUMBEL_MAX = -2.812, 16.636
STREAM = 3


def inv_temperature(T):
    return np.float32(1.0) / np.float32(T)


def words(row_keys, lo, hi, *, seed, call, relative=False):
    """uint64 [rows, hi - lo]: the generator word of every (row key, token id) of the window.  relative=True is the planted mutant that counts
    token ids from the window's start."""
    j = np.arange(0, hi - lo, dtype=np.uint64) if relative else np.arange(lo, hi, dtype=np.uint64)
    keys = (np.asarray(row_keys, dtype=np.int64) & MASK32).astype(np.uint64)
    c0 = np.broadcast_to((j >> np.uint64(2))[None, :], (len(keys), len(j)))
    c1 = np.broadcast_to(keys[:, None], c0.shape)
    s_lo, s_hi = seed_words(seed)
    o = philox4x32_10(c0, c1, np.full(c0.shape, STREAM, dtype=np.uint64), np.full(c0.shape, int(call) & MASK32, dtype=np.uint64), s_lo, s_hi)
    sel = np.broadcast_to((j & np.uint64(3))[None, :], c0.shape)
    return np.choose(sel.astype(np.int64), o)


def uniform_int(w, shift=9):
    """The 23-bit integer the uniform is built from (shift=8: the planted mutant, a 24-bit one)."""
    return w >> np.uint64(shift)


def gumbel64(w, shift=9):
    u = (2.0 * uniform_int(w, shift).astype(np.float64) + 1.0) * 2.0 ** -24
    return -np.log(-np.log(u))


def flat_token_ref(row_keys, lo, hi, *, seed, call):
    """The draw of a row whose window logits are all equal: the lowest token id holding the largest 23-bit integer k = w >> 9 (g is increasing in k and
    the add keeps the order).  Integers only: no logarithm enters.  Returns (token int32 [rows], k int64 [rows, hi - lo])."""
    k = uniform_int(words(row_keys, lo, hi, seed=seed, call=call)).astype(np.int64)
    return (np.argmax(k, axis=1) + lo).astype(np.int32), k


def scaled(z, T):
    """s = float32(z) * invT as fp32 (numpy rounds each product once): z is a bf16 / fp32 torch tensor or array [rows, n]."""
    z32 = z.float().numpy() if isinstance(z, torch.Tensor) else np.asarray(z, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (z32 * inv_temperature(T)).astype(np.float32)


def sample_ref(z, lo, hi, T, *, seed, call, row_keys=None, relative=False, shift=9, last_max=False, g=None):
    """z [rows, >= hi] bf16 logits -> dict of per-row numpy arrays: token (absolute id; first maximum of the float64 keys), key1 >= key2 (the two largest
    keys), e (the fp32 key error bound at the winner's and runner-up's magnitude), gap = key1 - key2, decided = gap > max(4 e, NEAR_TIE)."""
    rows = z.shape[0]
    row_keys = np.arange(rows) if row_keys is None else np.asarray(row_keys)
    s = scaled(z[:, lo:hi], T).astype(np.float64)
    if g is None:
        g = gumbel64(words(row_keys, lo, hi, seed=seed, call=call, relative=relative), shift)
    with np.errstate(invalid="ignore"):
        key = s + g
    key = np.where(np.isnan(key), -np.inf, key)               # a NaN key never wins
    if last_max:
        tok = key.shape[1] - 1 - np.argmax(key[:, ::-1], axis=1)
    else:
        tok = np.argmax(key, axis=1)                          # numpy: the first occurrence of the maximum
    order = np.partition(key, -2, axis=1) if key.shape[1] > 1 else key
    key1, key2 = order[:, -1], (order[:, -2] if key.shape[1] > 1 else np.full(rows, -np.inf))
    r = np.arange(rows)
    # |g| <= GUMBEL_MAX for both the winner and the runner-up; |s| and |key| at the winner (the runner-up's differ by less than the gap in question)
    e = LOGF_ULPS * 2.0 ** -23 * (1.0 + GUMBEL_MAX) + U32 * np.abs(s[r, tok]) + U32 * np.abs(key1)
    with np.errstate(invalid="ignore"):
        gap = key1 - key2                                     # (a window of -inf: NaN, never "decided")
    return dict(token=(tok + lo).astype(np.int32), key1=key1, key2=key2, e=e, gap=gap, decided=gap > np.maximum(4.0 * e, NEAR_TIE))


def row_stats_ref(z, lo, hi, T, tokens):
    """float64 log-probability of `tokens` (absolute ids, clamped into the window) and entropy of softmax(s) over the window with their derived bounds.
    logprob = -loss of token_ce_ref on s, so its bound is token_ce_ref's loss_bound on s plus the product's rounding 2^-24 |s_token|.
    entropy = lse - N / S with N = sum_j e_j s_j evaluated like S (W = ceil(n / 256) + 8 adds per lane and tree):
        d lse <= loss_bound's first three terms;   d N / S <= sum_j p_j |s_j| (|s_j - m| + 3 + W) 2^-24   (__expf, the product e_j s_j, the sum)
        d (N / S) <= d N / S + |N / S| (ds / s + 2^-24);   the subtraction adds 2^-24 |entropy|."""
    s32 = torch.from_numpy(scaled(z[:, lo:hi], T))
    n = hi - lo
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long).clamp(lo, hi - 1) - lo
    ref = token_ce_ref(s32, tok, n, 1.0)
    x = s32.double()
    s_tok = x.gather(1, tok[:, None])[:, 0]
    m = x.max(-1).values
    e = torch.exp(x - m[:, None])
    S = e.sum(-1)
    p = e / S[:, None]
    lse = torch.log(S) + m
    xs = torch.where(p > 0, x, torch.zeros_like(x))
    mean_s = (p * xs).sum(-1)
    W = -(-n // 256) + 8
    dist = torch.where(torch.isfinite(x), (x - m[:, None]).abs(), torch.zeros_like(x))
    ds = ((p * (dist + 2)).sum(-1) + W) * U32
    d_lse = ds + 3 * U32 * torch.log(S).abs() + U32 * lse.abs()
    d_mean = (p * xs.abs() * (dist + 3 + W)).sum(-1) * U32 + mean_s.abs() * (ds + U32)
    entropy = lse - mean_s
    return dict(logprob=-ref["loss"], logprob_bound=ref["loss_bound"] + U32 * s_tok.abs(), entropy=entropy,
                entropy_bound=d_lse + d_mean + U32 * entropy.abs(), p=p, onehot_grad=ref["grad64"], grad_floor=ref["grad_floor"], token_rel=tok)


def gate_ref(adv, ratio, clip_lo, clip_hi, ignore_sign=False):
    """gate = 0 where the clipped surrogate is flat in the ratio, otherwise the ratio.  ignore_sign=True is the planted mutant (clips on either side
    whatever the advantage's sign)."""
    adv, ratio = np.asarray(adv, dtype=np.float64), np.asarray(ratio, dtype=np.float64)
    if ignore_sign:
        gated = (ratio > clip_hi) | (ratio < clip_lo)
    else:
        gated = ((adv >= 0) & (ratio > clip_hi)) | ((adv < 0) & (ratio < clip_lo))
    return np.where(gated, 0.0, ratio), gated


def pg_ref(z, vocab, lo, hi, T, tokens, adv, *, old_logprob=None, clip=(0.8, 1.2), grad_scale=1.0, minus_one=True, ignore_sign=False):
    """float64 ovla_token_pg: logprob / entropy (row_stats_ref), ratio, gate, clipped, and dlogits [rows, vocab] = (p - onehot) c inside the window, 0
    outside, with the floor of token_ce_ref's gradient times |c| plus the three roundings of c itself.  minus_one=False plants the gradient
    without its one-hot term."""
    st = row_stats_ref(z, lo, hi, T, tokens)
    rows = z.shape[0]
    adv64 = np.asarray(adv, dtype=np.float64)
    ratio = np.ones(rows) if old_logprob is None else np.exp(st["logprob"].numpy() - np.asarray(old_logprob, dtype=np.float64))
    gate, gated = gate_ref(adv64, ratio, clip[0], clip[1], ignore_sign)
    c = torch.from_numpy(adv64 * gate * float(grad_scale) * float(inv_temperature(T)))
    inner = st["onehot_grad"] if minus_one else st["p"]
    grad = torch.zeros((rows, vocab), dtype=torch.float64)
    floor = torch.zeros((rows, vocab), dtype=torch.float64)
    grad[:, lo:hi] = inner * c[:, None]
    floor[:, lo:hi] = st["grad_floor"] * c.abs()[:, None] + 3 * U32 * grad[:, lo:hi].abs()
    st.update(ratio=ratio, gate=gate, clipped=gated.astype(np.int32), c=c.numpy(), grad64=grad, grad_floor=floor)
    return st


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def eighths(g, shape):
    """bf16 logits that are multiples of 1/8 in [-8, 8] (exact in bf16)."""
    return (torch.randint(-64, 65, shape, generator=g).double() / 8.0).to(torch.bfloat16)


GENERAL_T = (0.5, 1.0, 1.6)
GENERAL_KEYS = 64            # distinct row keys per logits row
GENERAL_ROWS = 64            # distinct logits rows; 64 x 64 = 4096 (row, key) pairs


def general_rows(vocab, ld, lo, hi, seed=2024):
    """The general input set: 64 distinct logits rows [64, ld], each drawn under 64 row keys.  Returns (z [64, ld] bf16, keys int32 [64])."""
    g = torch.Generator().manual_seed(seed + vocab + 7 * lo + 13 * hi)
    z = eighths(g, (GENERAL_ROWS, ld))
    keys = (torch.arange(GENERAL_KEYS, dtype=torch.int32) * 7919 + 11)
    return z, keys


def general_ref(z, keys, lo, hi, T, *, seed, call):
    """sample_ref of every (logits row r, key k) pair, flat index r * len(keys) + k.  The Gumbel variates depend on (key, token id) only and are
    evaluated once."""
    g = gumbel64(words(keys.numpy(), lo, hi, seed=seed, call=call))
    parts = [sample_ref(z[r:r + 1].expand(len(keys), -1), lo, hi, T, seed=seed, call=call, g=g) for r in range(z.shape[0])]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
