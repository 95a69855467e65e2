"""Plain CPU references and checks for the attention kernels (`csrc/attention.hip`).  Nothing here needs a GPU.

Two kinds of check, both per element (no normalisation by the largest element of the tensor):

* `check_elementwise`: |out - ref| <= c * 2^-8 * bound, where `bound` is the abs-weighted version of the product that forms
  the element (`bounds`), i.e. the quantity first-order rounding analysis scales with.  Each output passes two bf16
  roundings (unit roundoff 2^-8): one on the operand of the second MFMA (P for O and dV, dS for dQ and dK), one on the
  stored result, so the first-order bound is 2 * 2^-8 * bound; the third unit covers fp32 accumulation, the hardware
  exp2 / log and delta being formed from the bf16 O.  Hence c = 3.  Where `bound` is 0 (masked keys) the output must be 0.
* `check_counting`: with `counting_inputs` the exact answers are small rationals that count the visible keys of every row,
  so one key too many or too few anywhere is far outside the tolerance.

`emulate` restates the kernels in fp32 with the bf16 roundings where the kernels round; the CPU self-test uses it (with
correct and deliberately shifted masks) to show that the checks pass what is right and reject what is off by one.

All tensors are CPU tensors of shape [B, H, S, hd] (lse: [B, H, S]).
"""
import math

import torch

U = 2.0 ** -8            # unit roundoff of bf16 (8 significant bits, round to nearest)
LSE_U = 2.0 ** -17       # hd * 2^-24 with hd <= 128: worst-case fp32 dot-product bound
COUNT_LSE_TOL = 1e-4     # below n = 1200 adjacent counts differ by >= 8.3e-4 in the log; fp32 log error there is ~1e-6
COUNT_REL_TOL = 3 * U    # same two roundings + slack as check_elementwise; one key changes a non-zero element by >= 1/19
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453

# (B, H, S, hd, kv_len, causal): the smallest shapes that reach each block or tile edge of the kernels -- S on both sides of
# the 16-row / 32-row forward switch at 64, ragged last query and key blocks of 64 and 128 rows, kv_len on / inside / before
# a 64-key tile and at 1, causal diagonals inside a block, the ALOHA context (19 key tiles), and for head_dim 72 both backward
# branches: 4-wave (S = 50, 129), 8-wave with exact blocks (256) and 8-wave with a ragged last block (520).
CASES = [
    (2, 2, 64, 128, [64, 1], False),
    (2, 1, 50, 128, [50, 17], True),
    (3, 3, 200, 128, [200, 128, 65], False),
    (2, 2, 257, 128, [257, 192], True),
    (1, 2, 1159, 128, [1100], False),
    (3, 5, 130, 64, [130, 64, 1], False),
    (2, 3, 130, 64, [129, 63], True),
    (1, 2, 50, 72, None, False),
    (2, 3, 129, 72, [129, 77], True),
    (1, 2, 256, 72, [200], False),
    (1, 2, 520, 72, [515], False),
    (1, 2, 520, 72, None, True),
]


def case_id(case):
    B, H, S, hd, kvl, causal = case
    kv = "full" if kvl is None else "kv" + "-".join(str(x) for x in kvl)
    return f"B{B}H{H}S{S}hd{hd}-{kv}-{'causal' if causal else 'bidir'}"


def _kv_list(kv_len, B, S):
    if kv_len is None:
        return [S] * B
    kv = [int(x) for x in (kv_len.tolist() if torch.is_tensor(kv_len) else kv_len)]
    assert len(kv) == B
    return kv


def mask(S, kv_len, causal, B=None, causal_shift=0):
    """bool [B, 1, S, S]: key k is visible to query s iff k < kv_len[b] and (not causal or k <= s + causal_shift)."""
    if B is None:
        B = 1 if kv_len is None else len(kv_len)
    kv = torch.tensor(_kv_list(kv_len, B, S))
    idx = torch.arange(S)
    vis = (idx[None, None, None, :] < kv[:, None, None, None]).expand(B, 1, S, S).clone()
    if causal:
        vis &= (idx[None, :] <= idx[:, None] + causal_shift)[None, None]
    return vis


def shifted_masks(B, S, kv_len, causal):
    """The off-by-one variants of a case's mask, as (name, mask).  A shift is applied per batch entry where kv_len stays
    inside [1, S]; a variant that changes nothing, or leaves a row without a visible key, is not returned."""
    right = mask(S, kv_len, causal, B)
    kv = _kv_list(kv_len, B, S)
    out = []
    for d in (1, -1):
        new = [x + d if 1 <= x + d <= S else x for x in kv]
        out.append((f"kv_len{d:+d}", mask(S, new, causal, B)))
    if causal:
        for d in (1, -1):
            out.append((f"causal{d:+d}", mask(S, kv_len, True, B, causal_shift=d)))
    return [(n, m) for n, m in out if not torch.equal(m, right) and bool(m.any(-1).all())]


def reference(q, k, v, do, kv_len, causal, scale):
    """Textbook attention and its gradients in float64.  Returns O, lse, dQ, dK, dV, P."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    B, H, S, hd = q.shape
    vis = mask(S, kv_len, causal, B)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    O = P @ v
    dV = P.transpose(-1, -2) @ do
    dP = do @ v.transpose(-1, -2)
    delta = (O * do).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dQ = scale * (dS @ k)
    dK = scale * (dS.transpose(-1, -2) @ q)
    return O, lse, dQ, dK, dV, P


def bounds(q, k, v, do, O, P, scale):
    """Abs-weighted running-error references bO, bdQ, bdK, bdV (float64)."""
    q, k, v, do = (t.double().abs() for t in (q, k, v, do))
    bO = P @ v
    bdV = P.transpose(-1, -2) @ do
    T = P * (do @ v.transpose(-1, -2) + (O.abs() * do).sum(-1, keepdim=True))
    bdQ = scale * (T @ k)
    bdK = scale * (T.transpose(-1, -2) @ q)
    return bO, bdQ, bdK, bdV


def check_elementwise(out, ref, bound, c=3, what=""):
    """|out - ref| <= c * 2^-8 * bound for every element, and out == 0 exactly where bound == 0.  Returns the worst
    |err| / (2^-8 * bound)."""
    out, ref, bound = out.double(), ref.double(), bound.double()
    assert out.shape == ref.shape == bound.shape, f"{what}: shapes {tuple(out.shape)} {tuple(ref.shape)} {tuple(bound.shape)}"
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    zero = bound == 0
    nz = int((out[zero] != 0).sum())
    assert nz == 0, f"{what}: {nz} elements are non-zero where the exact result is 0 (masked keys), first at {_first(zero & (out != 0))}"
    err = (out - ref).abs()
    ratio = torch.where(zero, torch.zeros_like(err), err / (U * bound).masked_fill(zero, 1.0))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= c, f"{what}: |err| = {worst:.2f} * 2^-8 * bound (allowed {c}) at {_first(ratio == ratio.max())}, {int((ratio > c).sum())} elements over"
    return worst


def check_lse(out, ref, q, k, kv_len, causal, scale, what="lse"):
    """|lse - ref| <= 2^-17 * (1 + |ref| + scale * max over visible k of |q_s| . |k_k|).  Returns the worst ratio to that bound."""
    out, ref = out.double(), ref.double()
    B, H, S, hd = q.shape
    assert out.shape == ref.shape == (B, H, S), f"{what}: shape {tuple(out.shape)}"
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    a = q.double().abs() @ k.double().abs().transpose(-1, -2)
    a = a.masked_fill(~mask(S, kv_len, causal, B), 0.0).amax(-1)
    bound = LSE_U * (1.0 + ref.abs() + scale * a)
    ratio = (out - ref).abs() / bound
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |err| = {worst:.2f} * bound at {_first(ratio == ratio.max())}, err {float((out - ref).abs().max()):.3e}"
    return worst


def _first(cond):
    idx = cond.nonzero()
    return tuple(idx[0].tolist()) if len(idx) else None


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def emulate(q, k, v, do, kv_len, causal, scale, visible=None):
    """fp32 restatement of the kernels, bf16 roundings exactly where they round.  `visible` replaces the mask (the
    self-test passes the shifted ones).  Inputs are bf16-exact fp32.  Returns O, lse, dQ, dK, dV (O, dQ, dK, dV bf16-exact)."""
    q, k, v, do = (t.float() for t in (q, k, v, do))
    B, H, S, hd = q.shape
    vis = mask(S, kv_len, causal, B) if visible is None else visible
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    x = (s * sl2).masked_fill(~vis, float("-inf"))
    m = x.amax(-1, keepdim=True)
    p = torch.exp2(x - m)
    l = p.sum(-1, keepdim=True)
    O = _bf((_bf(p) @ v) * (1.0 / l))
    lse = (m * LN2 + torch.log(l))[..., 0]
    P = torch.exp2(s * sl2 - lse[..., None] * LOG2E).masked_fill(~vis, 0.0)
    delta = (O * do).sum(-1, keepdim=True)
    dS = _bf(P * (do @ v.transpose(-1, -2) - delta))
    dQ = _bf(scale * (dS @ k))
    dK = _bf(scale * (dS.transpose(-1, -2) @ q))
    dV = _bf(_bf(P).transpose(-1, -2) @ do)
    return O, lse, dQ, dK, dV


def counting_inputs(B, H, S, hd, seed=0):
    """Q = 0 (every visible score is 0, P is uniform over the visible keys), V[k, d] = [d == k % hd],
    dO[s, d] = [d == s % hd], K random (bf16-exact).  fp32 tensors q, k, v, do."""
    g = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, H, S, hd)
    k = _bf(torch.randn(B, H, S, hd, generator=g))
    onehot = (torch.arange(hd)[None, :] == (torch.arange(S) % hd)[:, None]).float()
    v = onehot.expand(B, H, S, hd).contiguous()
    return q, k, v, v.clone()


def counting_expected(B, S, hd, kv_len, causal):
    """Exact lse [B, S], O [B, S, hd], dV [B, S, hd] for `counting_inputs` (the same for every head)."""
    vis = mask(S, kv_len, causal, B)[:, 0].double()
    n = vis.sum(-1)                                                         # n(s) = min(kv_len, s + 1) or kv_len
    onehot = (torch.arange(hd)[None, :] == (torch.arange(S) % hd)[:, None]).double()
    O = (vis @ onehot) / n[..., None]                                       # #{visible k : k % hd == d} / n(s)
    dV = vis.transpose(-1, -2) @ (onehot / n[..., None])                    # sum over {s sees k, s % hd == d} of 1 / n(s)
    return n.log(), O, dV


def _check_rational(out, exact, what):
    out = out.double()
    exact = exact[:, None].expand_as(out)
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    zero = exact == 0
    bad = zero & (out != 0)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements non-zero where no visible key contributes, first at {_first(bad)}"
    rel = torch.where(zero, torch.zeros_like(out), (out - exact).abs() / exact.masked_fill(zero, 1.0))
    assert float(rel.max()) <= COUNT_REL_TOL, (
        f"{what}: relative error {float(rel.max()):.3e} (allowed {COUNT_REL_TOL:.3e}) at {_first(rel == rel.max())}: "
        f"a row sees the wrong set of keys")


def check_counting(O, lse, dK, dV, kv_len, causal, parts=("lse", "O", "dV", "dK")):
    """The outputs for `counting_inputs` against the exact answers.  `parts` selects the sub-checks (the self-test
    requires each of lse, O, dV to reject a shifted mask on its own)."""
    B, H, S, hd = O.shape
    e_lse, e_O, e_dV = counting_expected(B, S, hd, kv_len, causal)
    if "lse" in parts:
        err = (lse.double() - e_lse[:, None]).abs()
        assert torch.isfinite(lse).all() and float(err.max()) <= COUNT_LSE_TOL, (
            f"counting lse: |lse - log n| = {float(err.max()):.3e} (allowed {COUNT_LSE_TOL}) at {_first(err == err.max())}: wrong number of visible keys")
    if "O" in parts:
        _check_rational(O, e_O, "counting O")
    if "dV" in parts:
        _check_rational(dV, e_dV, "counting dV")
    if "dK" in parts:
        bad = dK != 0
        assert not bad.any(), f"counting dK: {int(bad.sum())} non-zero elements with Q = 0, first at {_first(bad)}"
