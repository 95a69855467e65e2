"""numpy restatement of preference optimisation on the Laplace policy (include/ovla.h "Preference optimisation on the Laplace policy") and of what
`csrc/laplace_dpo.hip` computes, on top of tests/laplace_policy_reference.py (`L`) and tests/laplace_scale_reference.py (`S`: the element rules, the
log-probability body and the group gradient sum).  Nothing here needs a GPU.

    per step c    lp_w, lp_l = S.logprob32 of the chosen / rejected chunk under (pred, scale);  rlp_w, rlp_l the same under (ref_pred, reference scale)
    per obs. b    h_w = (lp_w[0] - rlp_w[0]) + (lp_w[1] - rlp_w[1]) + ... ascending c, first term as it is;  h_l likewise;  m = h_w - h_l
    sigmoid       z = beta m;  az = |z|;  e = expf(-az);  den = 1 + e;  l = logf(den);  s_big = 1 / den;  s_small = e / den
                  softplus(-z) = (z < 0 ? az : 0) + l;  softplus(z) = (z > 0 ? az : 0) + l;  sigma(-z) = z >= 0 ? s_small : s_big;  sigma(z) the other
                  one_m = 1 - eps;  loss = (one_m softplus(-z)) + (eps softplus(z));  k = ((one_m sigma(-z)) - (eps sigma(z))) beta
    IPO           tau = 1 / (2 beta);  dm = m - tau;  loss = dm dm;  k = -2 dm
    coef          (k w) grad_scale;  c_0 = coef, or coef + ((nll_coef w) nll_scale) with nll_coef > 0;  c_1 = -coef
    gradient      S.pg_rows_ref's sample sums at G = 2 over (chosen, rejected) with c_g as they are (ratio 1, grad_scale 1, no reference):
                  dpred = bf16(acc_mu);  dlog_scale = inside ? bf16(acc_s) : +0
    w == 0        nothing of the observation is read; +0 to every output of it

What is IEEE is restated bit for bit in float32: the log-probabilities given inv_b, h and the margin given the log-probabilities
(`logprob_bits` / `ref_logprob_bits`: the kernel's own), everything of the IPO loss, the weights c_g and the gradient given `coef_bits`.

Where expf and logf enter (the sigmoid loss) the twin evaluates loss and k in float64 from the SAME fp32 z and reports a derived bound (L's
constants: expf known to EXPF_ULPS ulps, logf to LOGF_ULPS ulps, U32 = 2^-24 per rounded fp32 operation, SLACK for second-order products;
TINY = 2^-126 covers an e that underflows):

    e_hat         de = EXPF_ULPS 2^-23 e + TINY
    den_hat       fl(1 + e_hat):  dden = de + U32 den
    l_hat         logf(den_hat):  |log den_hat - log den| <= dden / den (den >= 1), and logf's own LOGF_ULPS 2^-23 |l|:  dl = dden / den + LOGF_ULPS 2^-23 l
                  (for e < 2^-24 den_hat = 1 and l_hat = 0 exactly; the true l = log1p(e) <= e <= dden: covered)
    softplus      fl(r + l_hat), r = max(-+z, 0) exact:  dsp = dl + U32 |sp|
    loss          p1 = fl(one_m sp-):  one_m dsp- + U32 |p1|;  p2 = fl(eps sp+) likewise;  loss = fl(p1 + p2):  dp1 + dp2 + U32 |loss|
    s_big         fl(1 / den_hat):  s_big (dden / den + U32);    s_small = fl(e_hat / den_hat):  de / den + s_small (dden / den + U32) + TINY
    k             a = fl(one_m sig-):  one_m dsig- + U32 a;  b = fl(eps sig+):  eps dsig+ + U32 b;  diff = fl(a - b):  da + db + U32 |diff|;
                  k = fl(diff beta):  beta ddiff + U32 |k|
    coef          two rounded products of k_hat with exactly known factors:  |w grad_scale| dk + 2 U32 |coef|
each times SLACK.  one_m = fl(1 - eps) is IEEE and enters both sides as the same fp32 number.

objective64 / grad64: the float64 definition of the stated total  grad_scale sum_b w_b loss_b + nll_coef nll_scale sum_{b,c} w_b (-lp_w[b, c])  and
its closed-form gradient with respect to (mu, s); the tests take central differences of the first.
"""
import numpy as np

from tests import laplace_policy_reference as L
from tests import laplace_scale_reference as S
from tests.pointwise_reference import U32
from tests.token_sample_reference import LOGF_ULPS

F32 = np.float32
EXPF_ULPS, SLACK = L.EXPF_ULPS, L.SLACK
TINY = 2.0 ** -126
CHUNK_MAX = 64            # ovla.h: OVLA_DPO_CHUNK_MAX
SIGMOID, IPO = 0, 1
TYPES = {"sigmoid": SIGMOID, "ipo": IPO}      # ops.DPO_LOSS_TYPES
MUTANTS = ("rejected_sign", "no_reference", "no_beta", "smoothing_sign", "wrong_axis", "nll_on_rejected")


def pair(chosen, rejected):
    """chosen, rejected [rows, adim] -> the group of two [rows, 2, adim] the Laplace kernels take."""
    return np.stack([np.asarray(chosen, dtype=F32), np.asarray(rejected, dtype=F32)], axis=1)


def chunk_sum32(t, B, chunk, wrong_axis=False):
    """fp32 [B * chunk] -> the sum over each observation's chunk steps in ascending c, the first term taken as it is -> fp32 [B].
    wrong_axis (planted mutant): the rows read as [chunk, B]."""
    t = np.asarray(t, dtype=F32)
    t = t.reshape(chunk, B).T if wrong_axis else t.reshape(B, chunk)
    acc = t[:, 0].copy()
    for c in range(1, chunk):
        acc = (acc + t[:, c]).astype(F32)
    return acc


def sigmoid_terms(z32, beta, eps):
    """The sigmoid loss and k of fp32 z [B] in float64 with the module docstring's bounds, and the twin's own fp32 evaluation (expf and logf
    correctly rounded) -> dict(loss, loss_bound, k, k_bound float64; loss32, k32 fp32)."""
    beta32, eps32 = F32(beta), F32(eps)
    one_m32 = F32(F32(1.0) - eps32)
    z = np.asarray(z32, dtype=F32).astype(np.float64)
    one_m, ep, bt = float(one_m32), float(eps32), float(beta32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        az = np.abs(z)
        e = np.exp(-az)
        den = 1.0 + e
        l = np.log1p(e)
        s_big, s_small = 1.0 / den, e / den
        r_neg, r_pos = np.where(z < 0, az, 0.0), np.where(z > 0, az, 0.0)
        sp_neg, sp_pos = r_neg + l, r_pos + l
        sig_neg, sig_pos = np.where(z >= 0, s_small, s_big), np.where(z >= 0, s_big, s_small)
        loss = one_m * sp_neg + ep * sp_pos
        k = (one_m * sig_neg - ep * sig_pos) * bt
        de = EXPF_ULPS * 2.0 ** -23 * e + TINY
        dden = de + U32 * den
        dl = dden / den + LOGF_ULPS * 2.0 ** -23 * l
        dsp_neg, dsp_pos = dl + U32 * np.abs(sp_neg), dl + U32 * np.abs(sp_pos)
        p1, p2 = one_m * sp_neg, ep * sp_pos
        loss_bound = (one_m * dsp_neg + U32 * np.abs(p1) + ep * dsp_pos + U32 * np.abs(p2) + U32 * np.abs(loss)) * SLACK
        ds_big = s_big * (dden / den + U32)
        ds_small = de / den + s_small * (dden / den + U32) + TINY
        dsig_neg, dsig_pos = np.where(z >= 0, ds_small, ds_big), np.where(z >= 0, ds_big, ds_small)
        a, b = one_m * sig_neg, ep * sig_pos
        ddiff = one_m * dsig_neg + U32 * a + ep * dsig_pos + U32 * b + U32 * np.abs(a - b)
        k_bound = (bt * ddiff + U32 * np.abs(k)) * SLACK
        # the twin's own fp32 chain, one rounding per operator
        z32 = np.asarray(z32, dtype=F32)
        az32 = np.abs(z32)
        e32 = np.exp(-az32.astype(np.float64)).astype(F32)
        den32 = (F32(1.0) + e32).astype(F32)
        l32 = np.log(den32.astype(np.float64)).astype(F32)
        sb32, ss32 = (F32(1.0) / den32).astype(F32), (e32 / den32).astype(F32)
        spn32 = (np.where(z32 < 0, az32, F32(0.0)) + l32).astype(F32)
        spp32 = (np.where(z32 > 0, az32, F32(0.0)) + l32).astype(F32)
        sgn32, sgp32 = np.where(z32 >= 0, ss32, sb32), np.where(z32 >= 0, sb32, ss32)
        loss32 = ((one_m32 * spn32).astype(F32) + (eps32 * spp32).astype(F32)).astype(F32)
        k32 = (((one_m32 * sgn32).astype(F32) - (eps32 * sgp32).astype(F32)).astype(F32) * beta32).astype(F32)
    return dict(loss=loss, loss_bound=loss_bound, k=k, k_bound=k_bound, loss32=loss32, k32=k32, parts32=dict(one_m=one_m32, sig_neg=sgn32, sig_pos=sgp32))


def ipo_terms32(m32, beta):
    """The IPO loss and k of the fp32 margin [B]: all IEEE -> (loss32, k32)."""
    tau = F32(F32(1.0) / F32(F32(2.0) * F32(beta)))
    with np.errstate(over="ignore", invalid="ignore"):
        dm = (np.asarray(m32, dtype=F32) - tau).astype(F32)
        return (dm * dm).astype(F32), (F32(-2.0) * dm).astype(F32)


def dpo_ref(mu, ref_mu, chosen, rejected, chunk, elem, ref_elem=None, *, weight=None, beta, eps=0.0, loss_type=SIGMOID, grad_scale=1.0, nll_coef=0.0,
            nll_scale=0.0, logprob_bits=None, ref_logprob_bits=None, coef_bits=None, mutant=None):
    """ovla_laplace_dpo.  mu, ref_mu bf16-exact floats (or bf16 tensors / bit patterns) [rows, adim]; chosen, rejected fp32 [rows, adim]; `elem`
    (`ref_elem`, default `elem`) the element dicts of S.elem_ref / S.fixed_elem; weight fp32 [B].  `logprob_bits` / `ref_logprob_bits` fp32
    [rows, 2]: the kernel's own log-probabilities, from which h and the margin are then formed bit for bit; `coef_bits` fp32 [B]: the kernel's own
    coef, from which the gradient is.  `mutant`: one of MUTANTS.
    -> dict(logprob, ref_logprob fp32 [rows, 2]; h fp32 [B, 2], margin fp32 [B] (exact given the log-probabilities); loss, coef float64 [B] with
    loss_bound, coef_bound (0 for IPO); loss32, coef32 fp32 (the twin's own; exact for IPO); c fp32 [B, 2]; acc_mu, acc_s fp32 [rows, adim] (the
    gradient sums before the bf16 store), dpred_bits, dlog_scale_bits uint16 [rows, adim] (exact given coef_bits); skipped bool [B])."""
    assert mutant is None or mutant in MUTANTS
    mu, ref = L.mu32(mu), L.mu32(ref_mu)
    rows, adim = mu.shape
    assert rows % chunk == 0 and 1 <= chunk <= CHUNK_MAX and 1 <= adim <= L.MAX_ADIM
    assert float(F32(beta)) >= 0 and 0 <= float(F32(eps)) < 0.5 and float(F32(nll_coef)) >= 0 and loss_type in (SIGMOID, IPO)
    B = rows // chunk
    ref_elem = elem if ref_elem is None else ref_elem
    w = np.ones(B, dtype=F32) if weight is None else np.asarray(weight, dtype=F32).reshape(B)
    skipped = w == 0
    row_skip = np.repeat(skipped, chunk)
    act = pair(chosen, rejected)
    lp = S.logprob32(mu, act, elem["inv_b"], elem["log_norm"]) if logprob_bits is None else np.asarray(logprob_bits, dtype=F32).reshape(rows, 2)
    rlp = S.logprob32(ref, act, ref_elem["inv_b"], ref_elem["log_norm"]) if ref_logprob_bits is None else np.asarray(ref_logprob_bits, dtype=F32).reshape(rows, 2)
    lp, rlp = np.where(row_skip[:, None], F32(0.0), lp), np.where(row_skip[:, None], F32(0.0), rlp)
    with np.errstate(over="ignore", invalid="ignore"):
        ratio_w = lp[:, 0] if mutant == "no_reference" else (lp[:, 0] - rlp[:, 0]).astype(F32)
        ratio_l = lp[:, 1] if mutant == "no_reference" else (lp[:, 1] - rlp[:, 1]).astype(F32)
        h_w = chunk_sum32(ratio_w, B, chunk, mutant == "wrong_axis")
        h_l = chunk_sum32(ratio_l, B, chunk, mutant == "wrong_axis")
        m = (h_w - h_l).astype(F32)
        beta32, gs32 = F32(beta), F32(grad_scale)
        if loss_type == SIGMOID:
            t = sigmoid_terms((beta32 * m).astype(F32), beta, eps)
            loss64, loss_bound, k64, k_bound, loss32, k32 = t["loss"], t["loss_bound"], t["k"], t["k_bound"], t["loss32"], t["k32"]
            if mutant == "no_beta":
                k32 = (k32 / beta32).astype(F32)
            if mutant == "smoothing_sign":
                p = t["parts32"]
                k32 = (((p["one_m"] * p["sig_neg"]).astype(F32) + (F32(eps) * p["sig_pos"]).astype(F32)).astype(F32) * beta32).astype(F32)
        else:
            loss32, k32 = ipo_terms32(m, beta)
            if mutant == "no_beta":
                k32 = (k32 * F32(0.5) / beta32).astype(F32)       # (the IPO form of the same slip: tau's factor lost from the slope)
            loss64, k64 = loss32.astype(np.float64), k32.astype(np.float64)
            loss_bound, k_bound = np.zeros(B), np.zeros(B)
        coef32 = ((k32 * w).astype(F32) * gs32).astype(F32)
        coef64 = k64 * w.astype(np.float64) * float(gs32)
        coef_bound = (np.abs(w.astype(np.float64) * float(gs32)) * k_bound + 2 * U32 * np.abs(coef64)) * SLACK
        if loss_type == IPO:                                       # IEEE throughout: the fp32 value is the value
            coef64, coef_bound = coef32.astype(np.float64), np.zeros(B)
        coef = coef32 if coef_bits is None else np.asarray(coef_bits, dtype=F32).reshape(B)
        nll32 = ((F32(nll_coef) * w).astype(F32) * F32(nll_scale)).astype(F32)
        on_nll = float(F32(nll_coef)) > 0
        c0 = (coef + nll32).astype(F32) if on_nll and mutant != "nll_on_rejected" else coef
        c1 = coef if mutant == "rejected_sign" else (-coef).astype(F32)
        if on_nll and mutant == "nll_on_rejected":
            c1 = (c1 + nll32).astype(F32)
    zero = F32(0.0)
    h = np.where(skipped[:, None], zero, np.stack([h_w, h_l], axis=1))
    m = np.where(skipped, zero, m)
    c = np.where(skipped[:, None], zero, np.stack([c0, c1], axis=1)).astype(F32)
    adv = np.repeat(c, chunk, axis=0)                              # [rows, 2]: every chunk step of the observation takes its pair of weights
    g = S.pg_rows_ref(mu, None, None, act, adv, grad_scale=1.0, elem=elem)
    assert np.array_equal(g["c"], adv, equal_nan=True), "ratio 1 and grad_scale 1: the group sum's weights are the pair's as they are"
    return dict(logprob=lp, ref_logprob=rlp, h=h.astype(F32), margin=m.astype(F32), loss=np.where(skipped, 0.0, loss64), loss_bound=np.where(skipped, 0.0, loss_bound),
                coef=np.where(skipped, 0.0, coef64), coef_bound=np.where(skipped, 0.0, coef_bound), loss32=np.where(skipped, zero, loss32).astype(F32),
                coef32=np.where(skipped, zero, coef32).astype(F32), c=c, acc_mu=g["surrogate"], acc_s=g["surrogate_s"], dpred_bits=g["dpred_bits"],
                dlog_scale_bits=g["dlog_scale_bits"], skipped=skipped)


# ---- the float64 objective and its closed-form gradient ---------------------------------------------------------------------------------------------
def _logprob64(mu, s, a):
    return -(np.abs(a - mu) * np.exp(-s) + s + np.log(2.0)).sum(-1)


def objective64(mu, s, ref_mu, ref_s, chosen, rejected, chunk, *, weight=None, beta, eps=0.0, loss_type=SIGMOID, grad_scale=1.0, nll_coef=0.0, nll_scale=0.0):
    """grad_scale sum_b w_b loss_b + nll_coef nll_scale sum_{b,c} w_b (-lp_w[b, c]) in float64, of float64 mu, s (log-scale, strictly inside any
    clamp), ref_mu, ref_s, chosen, rejected [rows, adim] -> (total, dict(margin [B], loss [B], preference, nll))."""
    mu, s, ref_mu, ref_s, aw, al = (np.asarray(t, dtype=np.float64) for t in (mu, s, ref_mu, ref_s, chosen, rejected))
    B = mu.shape[0] // chunk
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64)
    lp_w, lp_l = _logprob64(mu, s, aw), _logprob64(mu, s, al)
    h_w = (lp_w - _logprob64(ref_mu, ref_s, aw)).reshape(B, chunk).sum(1)
    h_l = (lp_l - _logprob64(ref_mu, ref_s, al)).reshape(B, chunk).sum(1)
    m = h_w - h_l
    if loss_type == SIGMOID:
        z = beta * m
        loss = (1.0 - eps) * np.logaddexp(0.0, -z) + eps * np.logaddexp(0.0, z)
    else:
        loss = (m - 1.0 / (2.0 * beta)) ** 2
    pref = grad_scale * (w * loss).sum()
    nll = nll_coef * nll_scale * (w[:, None] * -lp_w.reshape(B, chunk)).sum()
    return pref + nll, dict(margin=m, loss=loss, preference=pref, nll=nll)


def grad64(mu, s, ref_mu, ref_s, chosen, rejected, chunk, *, weight=None, beta, eps=0.0, loss_type=SIGMOID, grad_scale=1.0, nll_coef=0.0, nll_scale=0.0):
    """The contract's closed form in float64 -> (d mu, d s) [rows, adim] of objective64's total."""
    mu, s, aw, al = (np.asarray(t, dtype=np.float64) for t in (mu, s, chosen, rejected))
    B = mu.shape[0] // chunk
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64)
    _, parts = objective64(mu, s, ref_mu, ref_s, chosen, rejected, chunk, weight=weight, beta=beta, eps=eps, loss_type=loss_type)
    m = parts["margin"]
    if loss_type == SIGMOID:
        z = beta * m
        sig = lambda x: 1.0 / (1.0 + np.exp(-x))                  # noqa: E731
        k = ((1.0 - eps) * sig(-z) - eps * sig(z)) * beta
    else:
        k = -2.0 * (m - 1.0 / (2.0 * beta))
    coef = k * w * grad_scale
    c0 = np.repeat(coef + nll_coef * w * nll_scale, chunk)[:, None]
    c1 = np.repeat(-coef, chunk)[:, None]
    inv_b = np.exp(-s)
    d_mu = np.sign(mu - aw) * inv_b * c0 + np.sign(mu - al) * inv_b * c1
    d_s = (1.0 - np.abs(aw - mu) * inv_b) * c0 + (1.0 - np.abs(al - mu) * inv_b) * c1
    return d_mu, d_s


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
MIN_GAP = 2.0 ** -5        # every |a - mu| and |a - ref| of dpo_inputs is at least this: far above any difference step


def dpo_inputs(B, chunk, adim, seed=3, learned=True, bounds=S.BOUNDS):
    """The inputs both test files use, as numpy arrays: dict(mu, ref_mu fp32 [rows, adim] (bf16-exact, multiples of 1/64 in [-1, 1] and up to 1/32 apart),
    s, ref_s fp32 [rows, adim] (bf16-exact log-scales: multiples of 1/16 strictly inside `bounds`, the reference a multiple of 1/8 up to 1/2 off; all
    0 without `learned`), chosen, rejected fp32 [rows, adim] (mu + an offset of magnitude in [1/16, 1], so that every |a - mu| >= 1/16 and every
    |a - ref| >= 1/32 = MIN_GAP by construction), weight fp32 [B] in {0.5, 1, 2})."""
    import torch
    g = torch.Generator().manual_seed(100000 * B + 1000 * chunk + 10 * adim + seed)
    rows = B * chunk
    mu = L.means(g, rows, adim)
    roff = (torch.randint(-2, 3, (rows, adim), generator=g).float() / 64.0).numpy()
    ref_mu = L.bf16_round(np.clip(mu + roff, -1.0, 1.0).astype(F32))

    def offsets(lo):
        mag = (torch.randint(lo, 129, (rows, adim), generator=g).float() / 128.0).numpy()
        sgn = torch.where(torch.rand((rows, adim), generator=g) < 0.5, -1.0, 1.0).numpy()
        return (mag * sgn).astype(F32)

    chosen, rejected = (mu + 0.5 * offsets(16)).astype(F32), (mu + offsets(8)).astype(F32)    # the chosen chunk lies closer on average
    if learned:
        lo, hi = int(np.ceil(bounds[0] * 16)) + 9, int(np.floor(bounds[1] * 16)) - 9
        s = (torch.randint(max(lo, -24), min(hi, 0) + 1, (rows, adim), generator=g).float() / 16.0).numpy().astype(F32)
        ref_s = (s + (torch.randint(-4, 5, (rows, adim), generator=g).float() / 8.0).numpy()).astype(F32)
        assert bool(np.all((ref_s > bounds[0]) & (ref_s < bounds[1]) & (s > bounds[0]) & (s < bounds[1])))
        assert np.array_equal(L.bf16_round(s), s) and np.array_equal(L.bf16_round(ref_s), ref_s)
    else:
        s, ref_s = np.zeros((rows, adim), F32), np.zeros((rows, adim), F32)
    weight = np.asarray([0.5, 1.0, 2.0], dtype=F32)[torch.randint(0, 3, (B,), generator=g).numpy()]
    assert float(np.abs(chosen - mu).min()) >= 2 * MIN_GAP - 1e-6 and float(np.abs(rejected - mu).min()) >= 2 * MIN_GAP - 1e-6
    assert float(np.abs(chosen - ref_mu).min()) >= MIN_GAP - 1e-6 and float(np.abs(rejected - ref_mu).min()) >= MIN_GAP - 1e-6
    return dict(mu=mu, ref_mu=ref_mu, s=s, ref_s=ref_s, chosen=chosen, rejected=rejected, weight=weight)
