"""numpy restatement of the Laplace policy on the L1 head (include/ovla.h "Laplace policy on the L1 head") and of what the two kernels of
`csrc/laplace_policy.hip` compute.  Nothing here needs a GPU.

    scales      b_d fp32;  inv_b_d = float32(1) / b_d;  log_norm_d = float32(log(2 b_d)) formed in double
    generator   Philox4x32-10 (tests/lora_dropout_reference.py): counter (d >> 2, key, 4, call), key (seed_lo, seed_hi), word d & 3
    uniform     u = (2 (w >> 9) + 1) 2^-24;  x = u - 1/2;  t = 1 - 2 |x|: all exact in fp32 (checked over every 23-bit integer on the CPU)
    noise       e = copysign(-log t, x);  a_d = mu_d + b_d e
    logprob     q_d = |a_d - mu_d| inv_b_d;  acc = 0;  acc = acc - (q_d + log_norm_d) for ascending d, from the STORED fp32 a_d

What is IEEE is restated bit for bit in float32 (numpy rounds every operation once): the log-probability of stored actions, the weights c_g given
the kernel's own ratio bits, the gradient sum of the surrogate, and everything of the KL term on policy (q = 0: x = kl_d = k_d = +0).
Where a library function enters, the reference evaluates it in float64 from the SAME fp32 argument and reports a derived bound:

    action      e_hat = logf's result: |e_hat - e| <= LOGF_ULPS 2^-23 |e| =: de (ulp(e) <= 2^-23 |e|; the sign and t are exact).  Two rounded
                operations follow, p = b e_hat and a = mu + p:  |a_hat - a| <= b de + 2^-24 |b e| + 2^-24 |a|, times (1 + 2^-20) for the products
                of these small terms.
    ratio       the argument lp - old is one fp32 subtraction of exactly known operands: reproduced exactly.  expf: EXPF_ULPS 2^-23 relative.
    kl          q is exact.  x_hat = -expm1f(-q): |x_hat - x| <= EXPM1F_ULPS 2^-23 |x| =: dx.  kl_d = fl(q - x_hat): dx + 2^-24 (|kl_d| + dx).
                The row sum: one rounding per add, each on a partial sum no larger than the total (every term is >= 0 up to its own bound).
    kl gradient k_d = ((kl_coef x_hat) kl_scale) (sgn(D) inv_b): three rounded products of a factor known to dx / x (the product sgn inv_b is
                exact): |k_hat - k| <= |k| (EXPM1F_ULPS 2^-23 + 3 2^-24) (1 + 2^-20).  acc = fl(acc_surrogate + k_hat) adds 2^-24 |acc|.  The
                surrogate part of acc is exact, so the fp32 value before the bf16 store lies within `fb` of the float64 value v; rounding to
                bf16 is monotone and the kernel's value is an fp32 number, so its stored bits lie between bf16(float32(v - fb)) and
                bf16(float32(v + fb)), which differ (by one bf16 ulp) only where a rounding boundary lies within fb of v.

The HIP math library documents logf, expf and expm1f at 1 ulp; LOGF_ULPS follows tests/token_sample_reference.py, the other two its twin
tests/token_group_reference.py ("expf's 2 ulps", "expm1f ... its 2 ulps").

Clip margins: gate and `clipped` are compared exactly, so pg_ref ASSERTS that every float64 ratio is at least CLIP_MARGIN (relative) away from
both clip bounds -- three orders of magnitude above expf's bound -- and no sample is excluded from the comparison.
"""
import numpy as np

from tests.lora_dropout_reference import MASK32, bf16_bits_to_f32, f32_to_bf16_bits, philox4x32_10, seed_words
from tests.pointwise_reference import U32
from tests.token_sample_reference import LOGF_ULPS, gate_ref

STREAM = 4                # the token sampler uses 3 on the same seed
EXPF_ULPS = 2.0
EXPM1F_ULPS = 2.0
CLIP_MARGIN = 1e-3
GROUP_MAX = 64            # ovla.h: OVLA_PG_GROUP_MAX
MAX_ADIM = 16
E_MAX = 15.943            # -log(2^-23) = 15.9424
SLACK = 1.0 + 2.0 ** -20  # second-order products of the bounds' own terms
F32 = np.float32


def scales(scale, adim):
    """A scalar or per-dimension scale -> (b, inv_b, log_norm) fp32 [adim], as ops.laplace_scales and the launcher form them."""
    b = np.asarray(scale, dtype=np.float64).reshape(-1)
    b = np.repeat(b, adim) if b.size == 1 else b
    assert b.size == adim
    b32 = b.astype(F32)
    return b32, (F32(1.0) / b32).astype(F32), np.log(2.0 * b32.astype(np.float64)).astype(F32)


def words(keys, adim, *, seed, call, stream=STREAM, per_call=False):
    """uint64 [n, adim]: the generator word of every (draw key, dimension).  stream=3 and per_call=True (dimension d takes word 0 of counter
    d: `d` counted per Philox call instead of d >> 2 / d & 3) are the planted mutants."""
    d = np.arange(adim, dtype=np.uint64)
    k = (np.asarray(keys, dtype=np.int64).reshape(-1) & MASK32).astype(np.uint64)
    c0 = np.broadcast_to((d if per_call else d >> np.uint64(2))[None, :], (len(k), adim))
    c1 = np.broadcast_to(k[:, None], c0.shape)
    s_lo, s_hi = seed_words(seed)
    o = philox4x32_10(c0, c1, np.full(c0.shape, stream, dtype=np.uint64), np.full(c0.shape, int(call) & MASK32, dtype=np.uint64), s_lo, s_hi)
    sel = np.broadcast_to((np.zeros_like(d) if per_call else d & np.uint64(3))[None, :], c0.shape)
    return np.choose(sel.astype(np.int64), o)


def variate(k):
    """The 23-bit integer k = w >> 9 -> (u, x, t) as the contract's fp32 operations compute them."""
    u = ((2 * np.asarray(k, dtype=np.int64) + 1).astype(F32) * F32(2.0 ** -24)).astype(F32)
    x = (u - F32(0.5)).astype(F32)
    t = (F32(1.0) - (F32(2.0) * np.abs(x)).astype(F32)).astype(F32)
    return u, x, t


def noise64(w):
    """Generator words -> the unit Laplace variate in float64 (from the exact fp32 x and t)."""
    _, x, t = variate(np.asarray(w, dtype=np.uint64) >> np.uint64(9))
    return np.copysign(-np.log(t.astype(np.float64)), x.astype(np.float64))


def mu32(pred):
    """bf16 torch tensor or uint16 bit patterns or float array [rows, adim] -> fp32 values."""
    if hasattr(pred, "detach"):
        return pred.detach().float().cpu().numpy().astype(F32)
    pred = np.asarray(pred)
    return bf16_bits_to_f32(pred) if pred.dtype == np.uint16 else pred.astype(F32)


def default_keys(rows, G):
    return np.arange(rows * G, dtype=np.int64).reshape(rows, G)


def logprob32(mu, actions, inv_b, log_norm):
    """Bit-for-bit log-probability fp32 [rows, G] of STORED fp32 actions [rows, G, adim] around mu fp32 [rows, adim]."""
    mu, a = np.asarray(mu, dtype=F32), np.asarray(actions, dtype=F32)
    acc = np.zeros(a.shape[:2], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(a.shape[2]):
            q = (np.abs((a[:, :, d] - mu[:, None, d]).astype(F32)) * inv_b[d]).astype(F32)
            acc = (acc - (q + log_norm[d]).astype(F32)).astype(F32)
    return acc


def sample_ref(pred, scale, G, *, seed, call, row_keys=None, stream=STREAM, per_call=False):
    """float64 ovla_laplace_sample.  pred bf16 [rows, adim] -> dict(e [rows, G, adim] the unit variates, action, action_bound float64 [rows, G, adim],
    action32: the twin's own fp32 actions (mu + b float32(e), each operation rounded once -- the kernel's up to logf's error), and
    logprob_from_e: the planted mutant that takes q_d = |e| instead of recomputing it from the stored action)."""
    mu = mu32(pred)
    rows, adim = mu.shape
    assert 1 <= G <= GROUP_MAX and 1 <= adim <= MAX_ADIM
    b, inv_b, log_norm = scales(scale, adim)
    keys = default_keys(rows, G) if row_keys is None else np.asarray(row_keys).reshape(rows, G)
    e = noise64(words(keys, adim, seed=seed, call=call, stream=stream, per_call=per_call)).reshape(rows, G, adim)
    b64, mu64 = b.astype(np.float64)[None, None, :], mu.astype(np.float64)[:, None, :]
    a = mu64 + b64 * e
    bound = (b64 * LOGF_ULPS * 2.0 ** -23 * np.abs(e) + U32 * np.abs(b64 * e) + U32 * np.abs(a)) * SLACK
    e32 = e.astype(F32)
    a32 = (mu[:, None, :] + (b[None, None, :] * e32).astype(F32)).astype(F32)
    from_e = np.zeros((rows, G), dtype=F32)
    for d in range(adim):
        from_e = (from_e - (np.abs(e32[:, :, d]) + log_norm[d]).astype(F32)).astype(F32)
    return dict(e=e, action=a, action_bound=bound, action32=a32, logprob_from_e=from_e, keys=keys)


def bf16_round(x32):
    """fp32 -> the fp32 value of its bf16 rounding (nearest even)."""
    return bf16_bits_to_f32(f32_to_bf16_bits(np.asarray(x32, dtype=F32)))


def pg_ref(pred, actions, adv, scale, *, old_logprob=None, ref_pred=None, kl_coef=0.0, clip=(0.8, 1.2), grad_scale=1.0, kl_scale=0.0, ratio_bits=None,
           multiply_through=False, kl_sign=1.0):
    """ovla_laplace_pg.  pred (ref_pred) bf16 [rows, adim], actions fp32 [rows, G, adim], adv (old_logprob) fp32 [rows, G].  `ratio_bits`: the
    kernel's own fp32 ratio [rows, G], which the weights c_g are then formed from bit for bit (without it: float32 of the float64 ratio).
    -> dict(logprob fp32 (exact), ratio float64, ratio_bound, clipped int32 (exact: the margins are asserted), c fp32, surrogate fp32 [rows, adim]
    (the gradient sum before the KL term, exact given ratio_bits), dpred_bits uint16 (exact without ref_pred), and with ref_pred: kl, kl_bound
    float64 [rows], kl_on_policy bool [rows, adim], dpred_lo / dpred_hi fp32 [rows, adim] (the two bf16 values the stored gradient lies between)).
    multiply_through=True (a gated / zero-advantage sample multiplied through instead of skipped) and kl_sign=-1 are the planted mutants."""
    mu, a = mu32(pred), np.asarray(actions, dtype=F32)
    rows, G, adim = a.shape
    assert mu.shape == (rows, adim) and 1 <= G <= GROUP_MAX and 1 <= adim <= MAX_ADIM
    b, inv_b, log_norm = scales(scale, adim)
    adv = np.asarray(adv, dtype=F32).reshape(rows, G)
    lp = logprob32(mu, a, inv_b, log_norm)
    with np.errstate(invalid="ignore", over="ignore"):
        if old_logprob is None:
            ratio = np.ones((rows, G))
            ratio_bound = np.zeros((rows, G))
        else:
            arg = (lp - np.asarray(old_logprob, dtype=F32).reshape(rows, G)).astype(F32)
            ratio = np.exp(arg.astype(np.float64))
            ratio_bound = EXPF_ULPS * 2.0 ** -23 * ratio
        live = adv != 0                                           # a zero advantage is set to +0 whatever its ratio holds: no margin is needed
        for bound in clip:
            away = np.abs(ratio - float(F32(bound))) >= CLIP_MARGIN * float(F32(bound))
            assert bool(np.all(away | ~live | ~np.isfinite(ratio))), "a ratio lies within CLIP_MARGIN of a clip bound: choose other inputs"
        gate, gated = gate_ref(adv, ratio, float(F32(clip[0])), float(F32(clip[1])))
        r32 = ratio.astype(F32) if ratio_bits is None else np.asarray(ratio_bits, dtype=F32).reshape(rows, G)
        gs = F32(grad_scale)
        c = ((adv * r32).astype(F32) * gs).astype(F32)
        skip = gated | (adv == 0)
        if multiply_through:
            c = (c * np.where(skip, F32(0.0), F32(1.0))).astype(F32)       # NaN * 0 = NaN: what the skip exists to prevent
            skip = np.zeros_like(skip)
        else:
            c = np.where(skip, F32(0.0), c)
            skip = c == 0
        acc = np.zeros((rows, adim), dtype=F32)
        started = np.zeros((rows, adim), dtype=bool)
        for g in range(G):
            s = (np.sign(mu - a[:, g, :]) * 1.0).astype(F32)      # comparisons: a NaN action gives 0 ...
            s = np.where(np.isnan(s), F32(0.0), s)
            t = ((s * inv_b[None, :]).astype(F32) * c[:, g, None]).astype(F32)
            use = ~skip[:, g, None] & np.ones((rows, adim), dtype=bool)
            acc = np.where(use, np.where(started, (acc + t).astype(F32), t), acc)
            started |= use
    out = dict(logprob=lp, ratio=ratio, ratio_bound=ratio_bound, clipped=gated.astype(np.int32), c=c, surrogate=acc, dpred_bits=f32_to_bf16_bits(acc))
    if ref_pred is None:
        return out
    ref = mu32(ref_pred)
    delta = (mu - ref).astype(F32)
    q = (np.abs(delta) * inv_b[None, :]).astype(F32)
    q64 = q.astype(np.float64)
    x = -np.expm1(-q64)
    dx = EXPM1F_ULPS * 2.0 ** -23 * np.abs(x)
    kl_d = q64 - x
    kl_d_bound = dx + U32 * (np.abs(kl_d) + dx)
    kl = kl_d.sum(1)
    kl_bound = (kl_d_bound.sum(1) + (adim - 1) * U32 * (np.abs(kl_d).sum(1) + kl_d_bound.sum(1))) * SLACK
    sgn = np.sign(mu.astype(np.float64) - ref.astype(np.float64))
    k = float(kl_sign) * float(F32(kl_coef)) * x * float(F32(kl_scale)) * sgn * inv_b.astype(np.float64)[None, :]
    v = acc.astype(np.float64) + k
    fb = (np.abs(k) * (EXPM1F_ULPS * 2.0 ** -23 + 3 * U32) + U32 * np.abs(v)) * SLACK
    on = q == 0
    # on policy everything is IEEE: x = +0, kl_d = +0, k_d = +0 and acc + (+0) is acc (-0 + +0 = +0)
    exact = (acc + F32(0.0)).astype(F32)
    lo = np.where(on, bf16_round(exact), bf16_round((v - fb).astype(F32)))
    hi = np.where(on, bf16_round(exact), bf16_round((v + fb).astype(F32)))
    out.update(kl=kl, kl_bound=kl_bound, kl_on_policy=on, kl_grad=k, dpred64=v, dpred_floor=fb, dpred_lo=lo, dpred_hi=hi, dpred_bits=None)
    return out


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
SCALES = {1: [1.0], 4: [1.0, 0.3, 0.5, 2.0], 5: [0.7, 1.0, 0.125, 0.3, 1.5], 7: [1.0, 0.3, 0.05, 0.5, 0.7, 0.25, 1.3],
          14: [1.0, 0.3] * 7, 16: [0.3, 1.0, 0.5, 0.11] * 4}      # per dimension: 1.0 and non-powers-of-two in every set


def means(g, rows, adim):
    """bf16-exact predictions in [-1, 1]: multiples of 1/64 (torch generator g) -> fp32 numpy [rows, adim]."""
    import torch
    return (torch.randint(-64, 65, (rows, adim), generator=g).double() / 64.0).numpy().astype(F32)
