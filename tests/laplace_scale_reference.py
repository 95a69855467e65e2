"""numpy restatement of the Laplace policy with a learned scale (include/ovla.h "Laplace policy with a learned scale") and of what the two kernels of
`csrc/laplace_scale.hip` compute, on top of tests/laplace_policy_reference.py (`L`: generator, variate, bounds' constants).  Nothing here needs a GPU.

    element     s bf16;  s_c = fmin(fmax(s, s_lo), s_hi) (NaN -> s_lo);  inside = s_lo <= s <= s_hi;  b = expf(s_c);  inv_b = 1.0f / b;
                log_norm = s_c + LN2F, LN2F = float32(ln 2)
    sampler     L's generator words, uniform, variate and noise;  a_d = mu_d + b_{r,d} e;  logprob by L's body with the element's inv_b / log_norm
    per sample  logprob, ratio, gate, clipped, c_g: L.pg_ref's rules
    per (r, d)  q_g = |a_{g,d} - mu_d| inv_b over the samples not skipped, ascending g, first term as it is:
                  acc_mu = sum (sgn(mu_d - a_{g,d}) inv_b) c_g          acc_s = sum (1 - q_g) c_g
                reference:  u = s_c - s_rc;  D = mu - ref;  q = |D| inv_b;  x = -expm1f(-q);  rho = expf(u)
                  kl_d   = (expm1f(u) - u) + rho (q - x);   kl[r] = kl_0 + kl_1 + ...
                  acc_mu = acc_mu + (((kl_coef x) kl_scale) (sgn(D) inv_b)) rho
                  acc_s  = acc_s + (kl_coef kl_scale) (((rho (1 - x)) (1 + q)) - 1)
                entropy[r] = (1 + log_norm_0) + (1 + log_norm_1) + ...;   if entropy_coef != 0: acc_s = acc_s - (entropy_coef ent_scale), last
                dpred = bf16(acc_mu);  dlog_scale = inside ? bf16(acc_s) : +0

What is IEEE is restated bit for bit in float32: s_c, inside, log_norm, the entropy, and -- GIVEN the kernel's inv_b bits (`inv_b_bits`) and its
ratio bits (`ratio_bits`) -- the log-probability of stored actions, the weights c_g, both surrogate sums, the entropy's term, and everything of
the KL term on policy (u = 0 and D = 0: rho = 1, x = kl_d = +0, both gradient terms +0; expf(0) = 1 and expm1f(0) = 0 are exact).  Without
`inv_b_bits` the twin takes b = float32(exp(s_c) in float64) and its own IEEE division.

How a test reads the kernel's inv_b bits through the public entry (probe_args / probe_inv_b): one more launch on [rows * adim, 1] with mu = 0, one
draw a = 2^30, no ratio.  q = 2^30 inv_b is exact (a power of two); inv_b >= 1 / e^{s_hi} makes ulp(q) >= 2^30 2^-24 / e^{s_hi} >= 23 for s_hi
<= 1, and |log_norm| <= max(|s_lo|, |s_hi|) + 0.7 < 8 for the bounds used here is below a quarter of it, so q + log_norm rounds back to q and
logprob = -(2^30 inv_b): inv_b = -logprob 2^-30 exactly.  (A row's bits do not depend on its position: the contract.)

Where a library function enters, the twin evaluates it in float64 from the SAME fp32 argument and reports a derived bound (L's constants: logf,
expf, expm1f known to LOGF_ULPS / EXPF_ULPS / EXPM1F_ULPS ulps; U32 = 2^-24 per rounded fp32 operation; SLACK for second-order products):

    action      b_hat = b (1 + EXPF_ULPS 2^-23), e_hat = e (1 + LOGF_ULPS 2^-23);  p = b_hat e_hat and a = mu + p rounded once each:
                |a_hat - a| <= (|b e| (EXPF_ULPS + LOGF_ULPS) 2^-23 + U32 |b e| + U32 |a|) SLACK.  Where s_c == 0, b = 1 is exact: L's bound.
    ratio       as L.pg_ref.
    kl          u and q are exact fp32 arguments.  x_hat: dx = EXPM1F_ULPS 2^-23 |x|;  rho_hat: drho = EXPF_ULPS 2^-23 rho, 0 where u == 0;
                m_hat = expm1f(u): dm = EXPM1F_ULPS 2^-23 |m|.  t1 = fl(m_hat - u): e1 = dm + U32 (|m - u| + dm), 0 where u == 0.
                t2 = fl(q - x_hat): e2 = dx + U32 (|q - x| + dx).  p = fl(rho_hat t2): ep = rho e2 + drho |t2| + [u != 0] U32 |rho t2|.
                kl_d = fl(t1 + p): e1 + ep + [u != 0] U32 (|kl_d| + e1 + ep).  At u == 0 this is L.pg_ref's kl_d bound.  The row sum as there.
    d/d mu      k = kl_coef x kl_scale sgn(D) inv_b rho: three rounded products, a fourth where u != 0, of factors known to dx / x and
                drho / rho: |k_hat - k| <= |k| (EXPM1F_ULPS 2^-23 + [u != 0] (EXPF_ULPS 2^-23 + U32) + 3 U32);  acc = fl(acc + k_hat) adds
                U32 |acc|.  At u == 0: L.pg_ref's floor.
    d/d s       A = rho (1 - x): eA = drho (1 - x) + rho (dx + U32 (1 - x)) + U32 A;  B = 1 + q: eB = U32 B;  P = A B: eP = eA B + A eB +
                U32 P;  gs = P - 1: eg = eP + U32 (|gs| + eP);  W = fl(kl_coef kl_scale) is IEEE;  term = fl(W gs): |W| eg + U32 |W gs|;
                acc = fl(acc + term) adds U32 |acc|;  the entropy's subtraction adds another U32 |acc|.
    As in L.pg_ref the stored bf16 lies between bf16(float32(v - fb)) and bf16(float32(v + fb)); on policy both are the IEEE value.
"""
import numpy as np

from tests import laplace_policy_reference as L
from tests.lora_dropout_reference import f32_to_bf16_bits
from tests.pointwise_reference import U32
from tests.token_sample_reference import LOGF_ULPS, gate_ref

F32 = np.float32
LN2F = F32(np.log(2.0))
BOUNDS = (-6.0, 1.0)          # engine default; a design choice
PROBE_A = 2.0 ** 30
EXPF_ULPS, EXPM1F_ULPS, SLACK, CLIP_MARGIN = L.EXPF_ULPS, L.EXPM1F_ULPS, L.SLACK, L.CLIP_MARGIN


def elem_ref(log_scale, bounds, inv_b_bits=None):
    """log_scale bf16 tensor / uint16 bits / bf16-exact floats [rows, adim] -> dict(s, s_c, inside, b64 (float64 exp of the fp32 s_c), b, inv_b,
    log_norm fp32).  `inv_b_bits`: the kernel's own inv_b (probe_inv_b)."""
    s = L.mu32(log_scale)
    lo, hi = F32(bounds[0]), F32(bounds[1])
    assert np.isfinite(lo) and np.isfinite(hi) and lo <= hi
    with np.errstate(invalid="ignore"):
        s_c = np.fmin(np.fmax(s, lo), hi).astype(F32)            # fmax / fmin ignore a NaN operand, as fmaxf / fminf
        inside = (s >= lo) & (s <= hi)
    b64 = np.exp(s_c.astype(np.float64))
    b = b64.astype(F32)
    inv_b = (F32(1.0) / b).astype(F32) if inv_b_bits is None else np.asarray(inv_b_bits, dtype=F32).reshape(s.shape)
    return dict(s=s, s_c=s_c, inside=inside, b64=b64, b=b, inv_b=inv_b, log_norm=(s_c + LN2F).astype(F32))


def fixed_elem(scale, rows, adim):
    """The element dict of a FIXED scale (L.scales) on a log-scale of 0: how the anchors on L.pg_ref reach scales other than 1."""
    b, inv_b, log_norm = L.scales(scale, adim)
    t = lambda v: np.broadcast_to(v[None, :], (rows, adim)).copy()
    return dict(s=np.zeros((rows, adim), F32), s_c=np.zeros((rows, adim), F32), inside=np.ones((rows, adim), bool), b64=t(b).astype(np.float64), b=t(b),
                inv_b=t(inv_b), log_norm=t(log_norm))


def probe_args(log_scale_bits_shape):
    """(pred float [n, 1], actions float [n, 1, 1], advantage [n, 1]) of the inv_b probe for a log-scale of `shape` flattened to [n, 1]."""
    n = int(np.prod(log_scale_bits_shape))
    return np.zeros((n, 1), F32), np.full((n, 1, 1), PROBE_A, F32), np.ones((n, 1), F32)


def probe_inv_b(logprob, shape, bounds=BOUNDS):
    """The probe launch's logprob fp32 [n, 1] -> the kernel's inv_b bits fp32 `shape` (module docstring)."""
    assert bounds[1] <= 1.0 and max(abs(bounds[0]), abs(bounds[1])) + 0.7 < 8.0, "the probe's absorption argument is written for these bounds"
    return (-np.asarray(logprob, dtype=F32).reshape(shape) * F32(2.0 ** -30)).astype(F32)


def entropy32(log_norm):
    h = (F32(1.0) + log_norm[:, 0]).astype(F32)
    for d in range(1, log_norm.shape[1]):
        h = (h + (F32(1.0) + log_norm[:, d]).astype(F32)).astype(F32)
    return h


def logprob32(mu, actions, inv_b, log_norm):
    """L.logprob32 with inv_b / log_norm per element [rows, adim]."""
    mu, a = np.asarray(mu, dtype=F32), np.asarray(actions, dtype=F32)
    acc = np.zeros(a.shape[:2], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(a.shape[2]):
            q = (np.abs((a[:, :, d] - mu[:, None, d]).astype(F32)) * inv_b[:, None, d]).astype(F32)
            acc = (acc - (q + log_norm[:, None, d]).astype(F32)).astype(F32)
    return acc


def sample_rows_ref(pred, log_scale, bounds, G, *, seed, call, row_keys=None, inv_b_bits=None):
    """float64 ovla_laplace_sample_rows -> dict(e, action, action_bound float64 [rows, G, adim], action32 (the twin's own fp32 actions), entropy fp32
    [rows] (exact), elem, keys)."""
    mu = L.mu32(pred)
    rows, adim = mu.shape
    assert 1 <= G <= L.GROUP_MAX and 1 <= adim <= L.MAX_ADIM
    el = elem_ref(log_scale, bounds, inv_b_bits)
    keys = L.default_keys(rows, G) if row_keys is None else np.asarray(row_keys).reshape(rows, G)
    e = L.noise64(L.words(keys, adim, seed=seed, call=call)).reshape(rows, G, adim)
    b64, mu64 = el["b64"][:, None, :], mu.astype(np.float64)[:, None, :]
    a = mu64 + b64 * e
    expf_term = np.where(el["s_c"] == 0, 0.0, EXPF_ULPS)[:, None, :]
    bound = (np.abs(b64 * e) * (expf_term + LOGF_ULPS) * 2.0 ** -23 + U32 * np.abs(b64 * e) + U32 * np.abs(a)) * SLACK
    e32 = e.astype(F32)
    a32 = (mu[:, None, :] + (el["b"][:, None, :] * e32).astype(F32)).astype(F32)
    return dict(e=e, action=a, action_bound=bound, action32=a32, entropy=entropy32(el["log_norm"]), elem=el, keys=keys)


def pg_rows_ref(pred, log_scale, bounds, actions, adv, *, old_logprob=None, ref_pred=None, ref_log_scale=None, kl_coef=0.0, clip=(0.8, 1.2), grad_scale=1.0,
                kl_scale=0.0, entropy_coef=0.0, ent_scale=0.0, ratio_bits=None, inv_b_bits=None, elem=None):
    """ovla_laplace_pg_rows.  -> dict(logprob fp32 (exact given inv_b_bits), ratio float64, ratio_bound, clipped int32, c fp32, entropy fp32 (exact),
    surrogate, surrogate_s fp32 [rows, adim] (the sample sums, exact given ratio_bits and inv_b_bits), and without a reference dpred_bits /
    dlog_scale_bits uint16 (exact, the entropy's term included); with one: kl, kl_bound float64 [rows], kl_on_policy bool [rows, adim], kl_d,
    kl_grad, kl_grad_s float64, dpred_lo / dpred_hi / dlog_scale_lo / dlog_scale_hi fp32 [rows, adim])."""
    mu, a = L.mu32(pred), np.asarray(actions, dtype=F32)
    rows, G, adim = a.shape
    assert mu.shape == (rows, adim) and 1 <= G <= L.GROUP_MAX and 1 <= adim <= L.MAX_ADIM
    assert (ref_pred is None) == (ref_log_scale is None) and entropy_coef >= 0 and kl_coef >= 0
    el = elem_ref(log_scale, bounds, inv_b_bits) if elem is None else elem
    inv_b, log_norm, inside = el["inv_b"], el["log_norm"], el["inside"]
    adv = np.asarray(adv, dtype=F32).reshape(rows, G)
    lp = logprob32(mu, a, inv_b, log_norm)
    with np.errstate(invalid="ignore", over="ignore"):
        if old_logprob is None:
            ratio, ratio_bound = np.ones((rows, G)), np.zeros((rows, G))
        else:
            arg = (lp - np.asarray(old_logprob, dtype=F32).reshape(rows, G)).astype(F32)
            ratio = np.exp(arg.astype(np.float64))
            ratio_bound = EXPF_ULPS * 2.0 ** -23 * ratio
        live = adv != 0
        for bound in clip:
            away = np.abs(ratio - float(F32(bound))) >= CLIP_MARGIN * float(F32(bound))
            assert bool(np.all(away | ~live | ~np.isfinite(ratio))), "a ratio lies within CLIP_MARGIN of a clip bound: choose other inputs"
        gate, gated = gate_ref(adv, ratio, float(F32(clip[0])), float(F32(clip[1])))
        r32 = ratio.astype(F32) if ratio_bits is None else np.asarray(ratio_bits, dtype=F32).reshape(rows, G)
        c = ((adv * r32).astype(F32) * F32(grad_scale)).astype(F32)
        c = np.where(gated | (adv == 0), F32(0.0), c)
        skip = c == 0
        acc = np.zeros((rows, adim), dtype=F32)
        acc_s = np.zeros((rows, adim), dtype=F32)
        started = np.zeros((rows, adim), dtype=bool)
        for g in range(G):
            sg = (np.sign(mu - a[:, g, :]) * 1.0).astype(F32)    # comparisons: a NaN action gives 0 ...
            sg = np.where(np.isnan(sg), F32(0.0), sg)
            t = ((sg * inv_b).astype(F32) * c[:, g, None]).astype(F32)
            q = (np.abs((a[:, g, :] - mu).astype(F32)) * inv_b).astype(F32)
            ts = ((F32(1.0) - q).astype(F32) * c[:, g, None]).astype(F32)
            use = ~skip[:, g, None] & np.ones((rows, adim), dtype=bool)
            acc = np.where(use, np.where(started, (acc + t).astype(F32), t), acc)
            acc_s = np.where(use, np.where(started, (acc_s + ts).astype(F32), ts), acc_s)
            started |= use
    E = F32(F32(entropy_coef) * F32(ent_scale))
    has_ent = float(F32(entropy_coef)) != 0.0
    out = dict(logprob=lp, ratio=ratio, ratio_bound=ratio_bound, clipped=gated.astype(np.int32), c=c, entropy=entropy32(log_norm), surrogate=acc,
               surrogate_s=acc_s, elem=el)
    if ref_pred is None:
        fin_s = (acc_s - E).astype(F32) if has_ent else acc_s
        out.update(dpred_bits=f32_to_bf16_bits(acc), dlog_scale_bits=np.where(inside, f32_to_bf16_bits(fin_s), np.uint16(0)).astype(np.uint16))
        return out
    ref = L.mu32(ref_pred)
    s_rc = elem_ref(ref_log_scale, bounds)["s_c"]
    u32 = (el["s_c"] - s_rc).astype(F32)
    u = u32.astype(np.float64)
    off = u32 != 0
    delta = (mu - ref).astype(F32)
    q32 = (np.abs(delta) * inv_b).astype(F32)
    q = q32.astype(np.float64)
    x = -np.expm1(-q)
    dx = EXPM1F_ULPS * 2.0 ** -23 * np.abs(x)
    rho = np.exp(u)
    drho = np.where(off, EXPF_ULPS * 2.0 ** -23 * rho, 0.0)
    m = np.expm1(u)
    dm = EXPM1F_ULPS * 2.0 ** -23 * np.abs(m)
    t1 = m - u
    e1 = np.where(off, dm + U32 * (np.abs(t1) + dm), 0.0)
    t2 = q - x
    e2 = dx + U32 * (np.abs(t2) + dx)
    p = rho * t2
    ep = rho * e2 + drho * np.abs(t2) + np.where(off, U32 * np.abs(p), 0.0)
    kl_d = t1 + p
    kl_d_bound = e1 + ep + np.where(off, U32 * (np.abs(kl_d) + e1 + ep), 0.0)
    kl = kl_d.sum(1)
    kl_bound = (kl_d_bound.sum(1) + (adim - 1) * U32 * (np.abs(kl_d).sum(1) + kl_d_bound.sum(1))) * SLACK
    sgn = np.sign(mu.astype(np.float64) - ref.astype(np.float64))
    k = float(F32(kl_coef)) * x * float(F32(kl_scale)) * sgn * inv_b.astype(np.float64) * rho
    v = acc.astype(np.float64) + k
    fb = (np.abs(k) * (EXPM1F_ULPS * 2.0 ** -23 + np.where(off, EXPF_ULPS * 2.0 ** -23 + U32, 0.0) + 3 * U32) + U32 * np.abs(v)) * SLACK
    on = (q32 == 0) & ~off
    exact = (acc + F32(0.0)).astype(F32)                          # on policy everything is IEEE: the term is +0 (-0 + +0 = +0)
    lo = np.where(on, L.bf16_round(exact), L.bf16_round((v - fb).astype(F32)))
    hi = np.where(on, L.bf16_round(exact), L.bf16_round((v + fb).astype(F32)))
    # the log-scale's gradient
    A = rho * (1.0 - x)
    eA = drho * (1.0 - x) + rho * (dx + U32 * (1.0 - x)) + U32 * A
    B = 1.0 + q
    P = A * B
    eP = eA * B + A * U32 * B + U32 * P
    gs = P - 1.0
    eg = eP + U32 * (np.abs(gs) + eP)
    W = float(F32(F32(kl_coef) * F32(kl_scale)))
    ks = W * gs
    vs = acc_s.astype(np.float64) + ks
    fbs = abs(W) * eg + U32 * np.abs(ks) + U32 * np.abs(vs)
    exact_s = (acc_s + F32(0.0)).astype(F32)
    if has_ent:
        vs = vs - float(E)
        fbs = fbs + U32 * np.abs(vs)
        exact_s = (exact_s - E).astype(F32)
    fbs = fbs * SLACK
    zero = np.zeros((rows, adim), dtype=F32)
    lo_s = np.where(inside, np.where(on, L.bf16_round(exact_s), L.bf16_round((vs - fbs).astype(F32))), zero)
    hi_s = np.where(inside, np.where(on, L.bf16_round(exact_s), L.bf16_round((vs + fbs).astype(F32))), zero)
    out.update(kl=kl, kl_bound=kl_bound, kl_d=kl_d, kl_on_policy=on, kl_grad=k, kl_grad_s=ks, dpred64=v, dpred_floor=fb, dpred_lo=lo, dpred_hi=hi,
               dlog_scale64=vs, dlog_scale_floor=fbs, dlog_scale_lo=lo_s, dlog_scale_hi=hi_s)
    return out


# ---- the float64 objective and its closed-form gradient (what the kernel's gradient is the gradient OF) -------------------------------------------
def objective64(mu, s, actions, adv, *, bounds=BOUNDS, old_logprob=None, ref_mu=None, ref_s=None, kl_coef=0.0, clip=(0.8, 1.2), grad_scale=1.0, kl_scale=0.0,
                entropy_coef=0.0, ent_scale=0.0):
    """sum_{r,g} -min(ratio A, clip(ratio) A) grad_scale + kl_coef kl_scale sum_r kl - entropy_coef ent_scale sum_r entropy, in float64, of float64
    mu, s [rows, adim], actions [rows, G, adim], adv (old_logprob) [rows, G] -> (total, dict(surrogate, kl, entropy))."""
    mu, s, a, adv = (np.asarray(t, dtype=np.float64) for t in (mu, s, actions, adv))
    s_c = np.clip(s, bounds[0], bounds[1])
    inv_b = np.exp(-s_c)
    lp = -(np.abs(a - mu[:, None, :]) * inv_b[:, None, :] + s_c[:, None, :] + np.log(2.0)).sum(2)
    ratio = np.ones_like(lp) if old_logprob is None else np.exp(lp - np.asarray(old_logprob, dtype=np.float64))
    surr = -(np.minimum(ratio * adv, np.clip(ratio, clip[0], clip[1]) * adv)).sum() * grad_scale
    kl = 0.0
    if ref_mu is not None:
        u = s_c - np.clip(np.asarray(ref_s, dtype=np.float64), bounds[0], bounds[1])
        q = np.abs(mu - np.asarray(ref_mu, dtype=np.float64)) * inv_b
        kl = kl_coef * kl_scale * ((np.expm1(u) - u) + np.exp(u) * (q + np.expm1(-q))).sum()
    ent = -entropy_coef * ent_scale * (1.0 + s_c + np.log(2.0)).sum()
    return surr + kl + ent, dict(surrogate=surr, kl=kl, entropy=ent)


def grad64(mu, s, actions, adv, *, bounds=BOUNDS, old_logprob=None, ref_mu=None, ref_s=None, kl_coef=0.0, clip=(0.8, 1.2), grad_scale=1.0, kl_scale=0.0,
           entropy_coef=0.0, ent_scale=0.0):
    """The contract's closed forms in float64, term by term -> dict(surrogate=(d mu, d s), kl=(d mu, d s), entropy=(0, d s)), each [rows, adim].
    (No clamp mask: for points strictly inside the bounds.)"""
    mu, s, a, adv = (np.asarray(t, dtype=np.float64) for t in (mu, s, actions, adv))
    inv_b = np.exp(-s)
    qg = np.abs(a - mu[:, None, :]) * inv_b[:, None, :]
    lp = -(qg + s[:, None, :] + np.log(2.0)).sum(2)
    ratio = np.ones_like(lp) if old_logprob is None else np.exp(lp - np.asarray(old_logprob, dtype=np.float64))
    gated = ((adv >= 0) & (ratio > clip[1])) | ((adv < 0) & (ratio < clip[0]))
    c = np.where(gated, 0.0, adv * ratio * grad_scale)
    d_mu = (np.sign(mu[:, None, :] - a) * inv_b[:, None, :] * c[:, :, None]).sum(1)
    d_s = ((1.0 - qg) * c[:, :, None]).sum(1)
    out = dict(surrogate=(d_mu, d_s), kl=(np.zeros_like(mu), np.zeros_like(mu)), entropy=(np.zeros_like(mu), np.full_like(mu, -entropy_coef * ent_scale)))
    if ref_mu is not None:
        D = mu - np.asarray(ref_mu, dtype=np.float64)
        u = s - np.asarray(ref_s, dtype=np.float64)
        q, rho = np.abs(D) * inv_b, np.exp(u)
        x = -np.expm1(-q)
        w = kl_coef * kl_scale
        out["kl"] = (w * np.sign(D) * x * inv_b * rho, w * (rho * (1.0 - x) * (1.0 + q) - 1.0))
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def log_scales(g, rows, adim, bounds=BOUNDS, edge=True):
    """bf16-exact log-scales fp32 [rows, adim]: multiples of 1/16 inside the bounds (0 among them); with `edge` and enough elements, one each below
    s_lo, above s_hi, exactly at both bounds, and one NaN, planted at fixed flat positions."""
    import torch
    lo, hi = int(np.ceil(bounds[0] * 16)), int(np.floor(bounds[1] * 16))
    s = (torch.randint(lo, hi + 1, (rows, adim), generator=g).double() / 16.0).numpy().astype(F32)
    flat = s.reshape(-1)
    if edge and flat.size >= 7:
        plant = [bounds[0] - 0.5, bounds[1] + 0.5, bounds[0], bounds[1], np.nan, 0.0]
        pos = np.linspace(0, flat.size - 1, len(plant)).astype(int)
        flat[pos] = np.asarray(plant, dtype=F32)
    return flat.reshape(rows, adim)


SEED, CALL = 0x9E3779B97F4A7C15, 43
PG_KW = dict(kl_coef=0.375, clip=(0.8, 1.2), grad_scale=1.0 / 24, kl_scale=1.0 / 3, entropy_coef=0.25, ent_scale=1.0 / 3)


def pg_inputs(rows, adim, G, seed=5, bounds=BOUNDS):
    """The inputs both test files use, as numpy arrays: dict(mu, s fp32 [rows, adim] (bf16-exact; s with the planted edge values), act fp32
    [rows, G, adim] (the twin's own draws), adv, old fp32 [rows, G], ref_mu, ref_s fp32 [rows, adim] (bf16-exact)).  Ratios e^(+-0.5) and e^(+-0.05):
    at least 4 % from the clip bounds 0.8 / 1.2 on either side of the gate.  Every third dimension is on policy (ref == live in mean and scale);
    elsewhere the reference is up to 1/4 off in the mean and a multiple of 1/8 up to 1 off in the log-scale."""
    import torch
    g = torch.Generator().manual_seed(1000 * adim + 10 * G + rows + seed)
    mu = L.means(g, rows, adim)
    s = log_scales(g, rows, adim, bounds)
    smp = sample_rows_ref(mu, s, bounds, G, seed=SEED, call=CALL)
    act, el = smp["action32"], smp["elem"]
    adv = (torch.randint(1, 9, (rows, G), generator=g).float() / 4.0 * torch.where(torch.rand((rows, G), generator=g) < 0.5, -1.0, 1.0)).numpy().astype(F32)
    idx = np.arange(rows * G).reshape(rows, G)
    shift = np.where(idx % 2 == 0, 0.5, -0.05) * np.where(idx % 3 == 0, -1.0, 1.0)
    old = (logprob32(mu, act, el["inv_b"], el["log_norm"]) + shift.astype(F32)).astype(F32)
    off = (torch.randint(-16, 17, (rows, adim), generator=g).float() / 64.0).numpy()
    off_s = (torch.randint(-8, 9, (rows, adim), generator=g).float() / 8.0).numpy()
    off[:, ::3], off_s[:, ::3] = 0.0, 0.0
    ref_mu = L.bf16_round((mu + off).astype(F32))
    with np.errstate(invalid="ignore"):
        ref_s = L.bf16_round((s + off_s).astype(F32))
    return dict(mu=mu, s=s, act=act, adv=adv, old=old, ref_mu=ref_mu, ref_s=ref_s)
