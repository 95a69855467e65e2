"""CPU reference and checks for the attention-probability kernel (`csrc/attn_probs.hip`, `ops.attn_probs`).  Nothing here needs a GPU.

The reference P is `attn_reference.reference(...)[5]` (float64), gathered at the listed query rows.  Per element the allowed error is

    |P - P_ref| <= c * P_ref * E[b, h, s] + 2^-126,      E = LSE_U * (1 + |lse_ref| + scale * max over visible k of |q_s| . |k_k|)

E is `attn_reference.check_lse`'s own bound: P = exp(score - lse), so an absolute error e in the exponent is a relative error e in P, and
the exponent carries that bound once for the fp32 score and once for the lse that is fed in.  c = 1 when the lse fed in is lse_ref rounded
to fp32; c = 2 when it is the device forward's lse, which check_lse itself allows one unit.  2^-126 (the smallest normal fp32) covers a
result flushed to zero.  Where P_ref is 0 (masked keys) the output must be 0 exactly.  Row sums: |sum_k P - 1| <= c * E.

At gain 1 (unit-variance q, k) E is about 1.2e-4, so a P rounded to bf16 (2^-9 relative) fails: gain 1 is the deciding case, gain 3
(larger scores, smaller probabilities) only adds spread.  An fp32 evaluation of the formula on the CPU stays below 0.02 units on every
case (tests/test_attn_probs_reference.py), so the reference itself is far inside the bound.

Tensors are CPU tensors: q, k [B, H, S, hd]; lse [B, H, S]; P [B, H, S, S]; gathered P [R, H, S].
"""
import torch

from tests import attn_reference as ar

TINY = 2.0 ** -126

# the head_dim 64 / 128 cases of the attention suite (72 belongs to the towers, which this kernel refuses)
CPU_CASES = [c for c in ar.CASES if c[3] in (64, 128)]
# what the GPU test runs: the same without the 1159-token ALOHA context (its all-rows per-head P alone is 2 * 1159^2 fp32)
GPU_CASES = [
    (2, 2, 64, 128, [64, 1], False),
    (2, 1, 50, 128, [50, 17], True),
    (3, 3, 200, 128, [200, 128, 65], False),
    (2, 2, 257, 128, [257, 192], True),
    (3, 5, 130, 64, [130, 64, 1], False),
    (2, 3, 130, 64, [129, 63], True),
]
assert all(c in ar.CASES for c in GPU_CASES)


def inputs(case, gain=1.0, seed=0):
    """bf16-exact fp32 q, k, v [B, H, S, hd] with standard deviation `gain`."""
    B, H, S, hd, _, _ = case
    g = torch.Generator().manual_seed(seed * 1000 + B * 100 + S + hd)
    return tuple(ar._bf(torch.randn(B, H, S, hd, generator=g) * gain) for _ in range(3))


def reference(q, k, v, kv_len, causal, scale):
    """float64 (P [B, H, S, S], lse [B, H, S], E [B, H, S])."""
    B, H, S, hd = q.shape
    _, lse, _, _, _, P = ar.reference(q, k, v, torch.zeros_like(v), kv_len, causal, scale)
    a = q.double().abs() @ k.double().abs().transpose(-1, -2)
    a = a.masked_fill(~ar.mask(S, kv_len, causal, B), 0.0).amax(-1)
    return P, lse, ar.LSE_U * (1.0 + lse.abs() + scale * a)


def restate(q, k, lse, kv_len, causal, scale, visible=None):
    """fp32 restatement of the kernel: exp2(fp32(q . k) * (scale * log2e) - lse * log2e), masked keys 0 by select.  lse fp32 [B, H, S]."""
    q, k = q.float(), k.float()
    B, H, S, hd = q.shape
    vis = ar.mask(S, kv_len, causal, B) if visible is None else visible
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(ar.LOG2E, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    l2 = lse.float()[..., None] * torch.tensor(ar.LOG2E, dtype=torch.float32)
    return torch.exp2(s * sl2 - l2).masked_fill(~vis, 0.0)


def head_mean(P):
    """The kernel's P_mean from fp32 P [..., H, S]: acc summed over h = 0 .. H-1 in that order in fp32, times fp32(1 / H)."""
    P = P.float()
    H = P.shape[-2]
    acc = torch.zeros_like(P[..., 0, :])
    for h in range(H):
        acc = acc + P[..., h, :]
    return acc * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H), dtype=torch.float32)).to(P.device)


def row_list(B, S, R=21, seed=0):
    """A gathered list of R rows: a permutation sample of the valid rows with one repeat, a -1 and an index >= B*S (first one past the
    end, so that an off-by-one range check shows)."""
    g = torch.Generator().manual_seed(seed + B * S)
    rows = torch.randperm(B * S, generator=g)[: R - 3].tolist()
    rows = rows[:5] + [rows[2]] + rows[5:] + [-1]
    rows.insert(9, B * S)
    assert len(rows) == R
    return rows


def gather(T, rows):
    """[B, X, S, ...] -> [R, X, ...]: row b*S + s of every (b, s) listed; zeros for an index outside [0, B*S)."""
    B, S = T.shape[0], T.shape[2]
    out = torch.zeros((len(rows),) + tuple(T.shape[1:2]) + tuple(T.shape[3:]), dtype=T.dtype)
    for i, r in enumerate(rows):
        if 0 <= r < B * S:
            out[i] = T[r // S, :, r % S]
    return out


def check_probs(P, P_ref, E, c, what="P"):
    """P, P_ref [R, H, S]; E [R, H].  Returns the worst |err| / (P_ref * E) (in units; `c` are allowed)."""
    P, P_ref, E = P.double(), P_ref.double(), E.double()
    assert P.shape == P_ref.shape and E.shape == P.shape[:2], f"{what}: shapes {tuple(P.shape)} {tuple(P_ref.shape)} {tuple(E.shape)}"
    assert torch.isfinite(P).all(), f"{what}: non-finite output"
    zero = P_ref == 0
    nz = int((P[zero] != 0).sum())
    assert nz == 0, f"{what}: {nz} elements are non-zero where the exact result is 0 (masked keys), first at {ar._first(zero & (P != 0))}"
    err = (P - P_ref).abs()
    unit = P_ref * E[..., None]
    over = err > c * unit + TINY
    ratio = torch.where(zero, torch.zeros_like(err), (err - TINY).clamp_min(0.0) / unit.masked_fill(zero, 1.0))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert not over.any(), f"{what}: |err| = {worst:.3f} * P_ref * E (allowed {c}) at {ar._first(ratio == ratio.max())}, {int(over.sum())} elements over"
    return worst


def check_row_sums(P, E, valid, c, what="row sums"):
    """|sum_k P - 1| <= c * E for the valid rows, exactly 0 for the others.  P [R, H, S], E [R, H], valid bool [R]."""
    sums = P.double().sum(-1)
    assert not (sums[~valid] != 0).any(), f"{what}: a row with a bad index is not zero"
    ratio = (sums[valid] - 1.0).abs() / E.double()[valid]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= c, f"{what}: |sum - 1| = {worst:.3f} * E (allowed {c})"
    return worst


def counting_expected(B, S, kv_len, causal):
    """Exact P [B, 1, S, S] for `attn_reference.counting_inputs`: 1 / n(s) on the visible keys of row s."""
    vis = ar.mask(S, kv_len, causal, B).double()
    return vis / vis.sum(-1, keepdim=True)
