"""numpy / float64 restatement of ovla_token_pg_group (include/ovla.h "Token sampling and the policy-gradient objective", THE GROUP FORMS): G
given samples per row, the clipped surrogate, Schulman's k3 KL estimator to a reference policy and the entropy bonus.  Nothing here needs a GPU.

For one row with s = float32(z) * invT over the window, lse, p = softmax(s), H = lse - sum_j p_j s_j, and per sample g
    logprob_g = s[tok_g] - lse;  ratio_g = exp(logprob_g - old_g) (1 without);  gate_g as tests/token_sample_reference.gate_ref
    d_g = ref_g - logprob_g;  kl_g = expm1(d_g) - d_g
the loss is
    L = sum_g [ -min(ratio_g A_g, clip(ratio_g) A_g) + kl_coef kl_g ] grad_scale  -  ent_scale H
and its gradient with respect to the LOGITS z (one factor invT from s = z invT)
    dL/dz_j = sum_g (p_j - [j == tok_g]) w_g + ent_scale invT p_j (log p_j + H)
    w_g = (A_g gate_g + kl_coef expm1(d_g)) grad_scale invT
(d logprob_g / ds_j = [j == tok_g] - p_j;  d kl_g / d logprob_g = -expm1(d_g);  dH / ds_j = -p_j (log p_j + H)).

The floor of an element computed in fp32 as the header says, with U32 = 2^-24 and row_stats_ref's per-term floor F_j = d p_j + 2 U32 |p_j - onehot|:
    w_g      c_g carries 3 roundings and, with old log-probabilities, the ratio's error (the bound of the kernel's own logprob, expf's 2 ulps, the
             subtraction: logprob_bound + 5 U32, relative);  k_g carries expm1f of a d known to logprob_bound + U32 |d| (times e^d), its 2 ulps and 3
             roundings;  the add one more:  dw_g = |c_g| (3 U32 [+ lpb + 5 U32]) + kc e^(d + dd) dd + 7 U32 |k_g| + U32 |w_g|,  dd = lpb + U32 |d|
    term     t_g = (p - onehot) w_g:  F_j |w_g| + |p - onehot| dw_g + U32 |t_g|
    sum      one U32 per add, each on a partial sum no larger than sum_g |t_g| (+ |entropy term| for the last add)
    entropy  u = (ec p_j) a_j, a_j = (s_j - lse) + H:  ec (d p_j |a_j| + p_j (d lse + d H + 2 U32 (|s_j - lse| + |a_j|))) + 3 U32 |u|
"""
import numpy as np
import torch

from tests import token_sample_reference as R
from tests.pointwise_reference import U32

GROUP_MAX = 64            # ovla.h: OVLA_PG_GROUP_MAX


def row_loss64(s, tok_rel, adv, old, ref, *, kl_coef, ent_scale, clip, grad_scale):
    """float64 loss of ONE row as a function of its scaled window values: s [..., n] (leading dimensions are independent copies of the row, e.g. the
    perturbed copies of a finite difference), tok_rel int [G] relative to the window, adv / old / ref float [G] (old, ref may be None) -> [...]."""
    s = np.asarray(s, dtype=np.float64)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    S = e.sum(-1, keepdims=True)
    lse = (np.log(S) + m)[..., 0]
    p = e / S
    H = lse - (p * np.where(p > 0, s, 0.0)).sum(-1)
    total = -ent_scale * H
    for g in range(len(tok_rel)):
        lp = s[..., int(tok_rel[g])] - lse
        ratio = np.ones_like(lp) if old is None else np.exp(lp - old[g])
        surr = np.minimum(ratio * adv[g], np.clip(ratio, clip[0], clip[1]) * adv[g])
        total = total - surr * grad_scale
        if ref is not None:
            d = ref[g] - lp
            total = total + kl_coef * (np.expm1(d) - d) * grad_scale
    return total


def loss64(z, lo, hi, T, tokens, adv, *, old_logprob=None, ref_logprob=None, kl_coef=0.0, ent_scale=0.0, clip=(0.8, 1.2), grad_scale=1.0):
    """float64 loss per row [rows] of bf16 logits z [rows, >= hi] (the scaled values are the contract's fp32 products)."""
    s = R.scaled(z[:, lo:hi], T).astype(np.float64)
    tok = np.clip(np.asarray(tokens), lo, hi - 1) - lo
    return np.array([row_loss64(s[r], tok[r], np.asarray(adv, dtype=np.float64)[r], None if old_logprob is None else np.asarray(old_logprob, dtype=np.float64)[r],
                                None if ref_logprob is None else np.asarray(ref_logprob, dtype=np.float64)[r], kl_coef=kl_coef, ent_scale=ent_scale, clip=clip,
                                grad_scale=grad_scale) for r in range(s.shape[0])])


def group_ref(z, vocab, lo, hi, T, tokens, adv, *, old_logprob=None, ref_logprob=None, kl_coef=0.0, ent_scale=0.0, clip=(0.8, 1.2), grad_scale=1.0):
    """float64 ovla_token_pg_group.  z bf16 [rows, >= vocab], tokens int [rows, G], adv / old_logprob / ref_logprob float [rows, G] ->
    dict(logprob, logprob_bound, ratio, gate, clipped, kl, kl_bound, w [rows, G];  entropy, entropy_bound [rows];  grad64, grad_floor [rows, vocab])."""
    tokens = np.asarray(tokens)
    rows, G = tokens.shape
    assert 1 <= G <= GROUP_MAX
    adv64 = np.asarray(adv, dtype=np.float64)
    invT = float(R.inv_temperature(T))
    gs = float(grad_scale)
    kc = float(kl_coef) * gs * invT
    per = [R.row_stats_ref(z, lo, hi, T, tokens[:, g]) for g in range(G)]
    st0 = per[0]
    n = hi - lo
    lp = np.stack([s["logprob"].numpy() for s in per], 1)
    lpb = np.stack([s["logprob_bound"].numpy() for s in per], 1)
    ratio = np.ones((rows, G)) if old_logprob is None else np.exp(lp - np.asarray(old_logprob, dtype=np.float64))
    gate, gated = R.gate_ref(adv64, ratio, clip[0], clip[1])
    c = adv64 * gate * gs * invT
    dw = np.abs(c) * (3 * U32 + (0.0 if old_logprob is None else lpb + 5 * U32))
    kl = kl_bound = None
    w = c
    if ref_logprob is not None:
        d = np.asarray(ref_logprob, dtype=np.float64) - lp
        dd = lpb + U32 * np.abs(d)                              # what the kernel's d is known to
        kl = np.expm1(d) - d
        # kl = expm1f(d) - d: the function's slope |e^d - 1| on dd and its second-order remainder, expm1f's 2 ulps (4 U32), the subtraction
        kl_bound = np.abs(np.expm1(d)) * dd + np.exp(d + dd) * dd * dd + 4 * U32 * np.abs(np.expm1(d)) + U32 * np.abs(kl)
        k = kc * np.expm1(d)
        w = c + k
        dw = dw + kc * np.exp(d + dd) * dd + 7 * U32 * np.abs(k) + U32 * np.abs(w)
    p = st0["p"]
    grad = torch.zeros((rows, vocab), dtype=torch.float64)
    floor = torch.zeros((rows, vocab), dtype=torch.float64)
    acc = torch.zeros((rows, n), dtype=torch.float64)
    fl = torch.zeros((rows, n), dtype=torch.float64)
    mag = torch.zeros((rows, n), dtype=torch.float64)
    n_terms = torch.zeros(rows, dtype=torch.float64)
    for g in range(G):
        wg, dwg = torch.from_numpy(np.ascontiguousarray(w[:, g]))[:, None], torch.from_numpy(np.ascontiguousarray(dw[:, g]))[:, None]
        t = per[g]["onehot_grad"] * wg                           # a skipped sample (w == 0) contributes exactly nothing, as in the kernel
        acc += t
        fl += per[g]["grad_floor"] * wg.abs() + per[g]["onehot_grad"].abs() * dwg + U32 * t.abs()
        mag += t.abs()
        n_terms += (wg[:, 0] != 0).double()
    entropy = st0["entropy"]
    if ent_scale != 0.0:
        ec = float(ent_scale) * invT
        x = torch.from_numpy(R.scaled(z[:, lo:hi], T)).double()
        lse = (x.gather(1, st0["token_rel"][:, None])[:, 0] - st0["logprob"])
        logp = x - lse[:, None]
        a = logp + entropy[:, None]
        live = p > 0
        u = torch.where(live, ec * p * a, torch.zeros_like(a))
        dp = st0["grad_floor"] - 2 * U32 * st0["onehot_grad"].abs()           # row_stats_ref's d p_j
        d_lse = torch.from_numpy(lpb.max(1))
        da = (d_lse + st0["entropy_bound"])[:, None] + 2 * U32 * (logp.abs() + a.abs())
        fu = abs(ec) * (dp * a.abs() + p * da) + 3 * U32 * u.abs()
        acc += u
        fl += torch.where(live, fu, torch.zeros_like(fu))
        mag += u.abs()
        n_terms += 1
    fl += U32 * n_terms[:, None] * mag                           # one rounding per add, each partial sum at most `mag`
    grad[:, lo:hi], floor[:, lo:hi] = acc, fl
    return dict(logprob=torch.from_numpy(lp), logprob_bound=torch.from_numpy(lpb), ratio=ratio, gate=gate, clipped=gated.astype(np.int32),
                kl=None if kl is None else torch.from_numpy(kl), kl_bound=None if kl is None else torch.from_numpy(kl_bound), w=w,
                entropy=entropy, entropy_bound=st0["entropy_bound"], grad64=grad, grad_floor=floor, p=p)


def group_advantages_ref(rewards, eps=1e-6):
    """(r - mean_g) / (std_g + eps) per row of rewards [B, G] in float64, std the population standard deviation (openvla-oft_amd/rl.py)."""
    r = np.asarray(rewards, dtype=np.float64)
    return (r - r.mean(1, keepdims=True)) / (r.std(1, keepdims=True) + eps)
