"""The numpy restatement of the Laplace policy with a learned scale (tests/laplace_scale_reference.py) against itself and against the fixed-scale
restatement it extends: its gradients are the derivatives of the float64 objective, it is tests/laplace_policy_reference.py bit for bit where the
scales coincide, the KL is +0 on policy and never negative, and a clamped log-scale takes no gradient.  No GPU."""
import numpy as np
import pytest
import torch

from tests import laplace_policy_reference as L
from tests import laplace_scale_reference as S

F32 = np.float32
H_STEP = 2.0 ** -13            # the finite-difference step on a mean or a log-scale (a power of two: exact in float64 on the 1/64 and 1/16 grids)
EPS64 = 2.0 ** -52
GROW = 1.02                    # what e^{h (|q - 1| + ...)}, e^{h inv_b} and (e^h)^3 can add to the third-derivative factors below over one step


def _fd_world(G):
    """A small world strictly inside the clamp, draws at least 8 h from the mean, the reference's mean off by a multiple of 1/64."""
    g = torch.Generator().manual_seed(770 + G)
    rows, adim = 2, 3
    mu = L.means(g, rows, adim).astype(np.float64)
    s = (torch.randint(-32, 9, (rows, adim), generator=g).double() / 16.0).numpy()            # b in [e^-2, e^0.5]
    e = L.noise64(L.words(L.default_keys(rows, G), adim, seed=S.SEED, call=3)).reshape(rows, G, adim)
    act = mu[:, None, :] + np.exp(s)[:, None, :] * e
    assert float(np.abs(act - mu[:, None, :]).min()) > 8 * H_STEP
    adv = (torch.randint(1, 9, (rows, G), generator=g).double() / 4.0 * torch.where(torch.rand((rows, G), generator=g) < 0.5, -1.0, 1.0)).numpy()
    lp = -(np.abs(e) + s[:, None, :] + np.log(2.0)).sum(2)
    idx = np.arange(rows * G).reshape(rows, G)
    old = lp + np.where(idx % 2 == 0, 0.5, -0.05) * np.where(idx % 3 == 0, -1.0, 1.0)
    ref_mu = mu + (torch.randint(1, 17, (rows, adim), generator=g).double() / 64.0).numpy() * np.where(np.arange(adim) % 2 == 0, 1.0, -1.0)
    ref_mu[0, 0] = mu[0, 0]                                                                    # one element on policy in the mean
    ref_s = np.minimum(s + (torch.randint(-8, 9, (rows, adim), generator=g).double() / 8.0).numpy(), 0.875)   # strictly inside the clamp too
    return mu, s, act, adv, old, ref_mu, ref_s


def _fd_bounds(mu, s, act, adv, old, ref_mu, ref_s, kw):
    """|central difference - derivative| <= h^2 / 6 max |f'''| + rounding, per element -> (bound for d mu, bound for d s) [rows, adim].
    Along mu_d the log-probability is linear away from a = mu (slope p = sgn(a - mu) inv_b): (A ratio)''' = A ratio p^3.  Along s_d, p = d logprob /
    d s = q - 1, p' = -q, p'' = q: (A ratio)''' = A ratio (p^3 + 3 p p' + p'').  kl_d = (e^u - 1 - u) + e^u g(q), g = q - 1 + e^-q: along mu its third
    derivative is rho e^-q inv_b^3 in magnitude (one-sided at D = 0, where kl_d is twice differentiable: Taylor's remainder holds on either side);
    along s, with q' = -q and T g = g - q g', (e^u g)''' = e^u T^3 g = e^u (-1 + (1 + q + q^3) e^-q), at most 4 e^u, and (e^u)''' = e^u: 5 rho.
    The entropy is linear.  GROW covers the movement of ratio, rho and q over the step.  Rounding: the float64 objective is a sum of a few hundred
    products and exponentials known to 64 eps of the magnitudes of its terms; the difference divides that by h."""
    inv_b = np.exp(-s)
    qg = np.abs(act - mu[:, None, :]) * inv_b[:, None, :]
    lp = -(qg + s[:, None, :] + np.log(2.0)).sum(2)
    ratio = np.exp(lp - old)
    gs, w, clip = kw["grad_scale"], kw["kl_coef"] * kw["kl_scale"], kw["clip"]
    Ar = (np.abs(adv) * ratio)[:, :, None]
    m3_mu = (Ar * inv_b[:, None, :] ** 3).sum(1) * gs
    p = np.abs(qg - 1.0)
    m3_s = (Ar * (p ** 3 + 3 * p * qg + qg)).sum(1) * gs
    mag = (np.abs(adv) * np.maximum(ratio, clip[1])).sum() * gs + kw["entropy_coef"] * kw["ent_scale"] * (1.0 + np.abs(s) + 1.0).sum()
    if ref_mu is not None:
        rho, q = np.exp(s - ref_s), np.abs(mu - ref_mu) * inv_b
        m3_mu = m3_mu + w * rho * inv_b ** 3
        m3_s = m3_s + w * 5.0 * rho
        mag += w * (rho * (2.0 + q) + np.abs(s - ref_s) + 1.0).sum()
    rounding = 64 * EPS64 * mag / H_STEP
    return H_STEP ** 2 / 6.0 * GROW * m3_mu + rounding, H_STEP ** 2 / 6.0 * GROW * m3_s + rounding


@pytest.mark.parametrize("terms", ("all", "surrogate", "kl", "entropy"))
@pytest.mark.parametrize("G", (1, 3, 8))
def test_gradient_is_the_derivative_of_the_objective(terms, G):
    mu, s, act, adv, old, ref_mu, ref_s = _fd_world(G)
    kw = dict(kl_coef=0.04, clip=(0.8, 1.2), grad_scale=1.0 / 7, kl_scale=1.0 / 3, entropy_coef=0.01, ent_scale=1.0 / 3)
    if terms == "surrogate":
        ref_mu, ref_s, kw["entropy_coef"] = None, None, 0.0
    elif terms == "kl":
        adv, kw["entropy_coef"] = np.zeros_like(adv), 0.0
    elif terms == "entropy":
        adv, ref_mu, ref_s = np.zeros_like(adv), None, None
    f = lambda m, t: S.objective64(m, t, act, adv, old_logprob=old, ref_mu=ref_mu, ref_s=ref_s, **kw)[0]
    g = S.grad64(mu, s, act, adv, old_logprob=old, ref_mu=ref_mu, ref_s=ref_s, **kw)
    want_mu = sum(g[k][0] for k in g)
    want_s = sum(g[k][1] for k in g)
    b_mu, b_s = _fd_bounds(mu, s, act, adv, old, ref_mu, ref_s, kw)
    if terms != "entropy":
        ratio = np.exp(-(np.abs(act - mu[:, None, :]) * np.exp(-s)[:, None, :] + s[:, None, :] + np.log(2.0)).sum(2) - old)
        assert float(np.minimum(np.abs(ratio / 0.8 - 1), np.abs(ratio / 1.2 - 1)).min()) > 0.04, "a ratio is near a clip bound"
    resolved = []
    for r in range(mu.shape[0]):
        for d in range(mu.shape[1]):
            one = np.zeros_like(mu)
            one[r, d] = H_STEP
            fd_mu = (f(mu + one, s) - f(mu - one, s)) / (2 * H_STEP)
            fd_s = (f(mu, s + one) - f(mu, s - one)) / (2 * H_STEP)
            print(f"{terms} G={G} ({r},{d}): d mu {want_mu[r, d]:+.6e} fd err {abs(fd_mu - want_mu[r, d]):.2e} / {b_mu[r, d]:.2e};  "
                  f"d s {want_s[r, d]:+.6e} fd err {abs(fd_s - want_s[r, d]):.2e} / {b_s[r, d]:.2e}")
            assert abs(fd_mu - want_mu[r, d]) <= b_mu[r, d], f"{terms} G={G} ({r},{d}): d mu"
            assert abs(fd_s - want_s[r, d]) <= b_s[r, d], f"{terms} G={G} ({r},{d}): d s"
            resolved += [abs(want_mu[r, d]) / b_mu[r, d], abs(want_s[r, d]) / b_s[r, d]]
    assert max(resolved) > 1e3, "the gradients do not stand above the bound: the comparison means nothing"
    # the fp32 restatement computes that gradient: its bf16 interval holds the float64 closed form to bf16 precision
    ref = S.pg_rows_ref(mu.astype(F32), s.astype(F32), S.BOUNDS, act.astype(F32), adv.astype(F32), old_logprob=None if terms == "entropy" else old.astype(F32),
                        ref_pred=None if ref_mu is None else ref_mu.astype(F32), ref_log_scale=None if ref_s is None else ref_s.astype(F32), **kw)
    assert ref["entropy"].shape == (mu.shape[0],)
    np.testing.assert_allclose(ref["entropy"], (1.0 + s + np.log(2.0)).sum(1), rtol=1e-6)


def _anchor_world(rows, adim, G, seed=0):
    g = torch.Generator().manual_seed(31 * adim + G + rows + seed)
    mu = L.means(g, rows, adim)
    keys = (np.arange(rows * G, dtype=np.int64).reshape(rows, G) * 7919 - 300000)
    adv = (torch.randint(1, 9, (rows, G), generator=g).float() / 4.0 * torch.where(torch.rand((rows, G), generator=g) < 0.5, -1.0, 1.0)).numpy().astype(F32)
    adv[0, 0] = 0.0
    off = (torch.randint(-16, 17, (rows, adim), generator=g).float() / 64.0).numpy()
    off[:, ::3] = 0.0
    return mu, keys, adv, L.bf16_round((mu + off).astype(F32))


def _old(lp, rows, G):
    idx = np.arange(rows * G).reshape(rows, G)
    return (lp + (np.where(idx % 2 == 0, 0.5, -0.05) * np.where(idx % 3 == 0, -1.0, 1.0)).astype(F32)).astype(F32)


@pytest.mark.parametrize("adim,G", ((1, 1), (7, 2), (14, 5), (16, 64)))
def test_zero_log_scale_is_the_fixed_scale_restatement_at_one(adim, G):
    rows = 5
    mu, keys, adv, ref_mu = _anchor_world(rows, adim, G)
    zero = np.zeros((rows, adim), F32)
    a = S.sample_rows_ref(mu, zero, S.BOUNDS, G, seed=S.SEED, call=9, row_keys=keys)
    b = L.sample_ref(mu, 1.0, G, seed=S.SEED, call=9, row_keys=keys)
    for k in ("e", "action", "action_bound", "action32"):
        assert np.array_equal(a[k], b[k]), k
    act = a["action32"]
    old = _old(L.logprob32(mu, act, *L.scales(1.0, adim)[1:]), rows, G)
    kw = dict(kl_coef=0.375, clip=(0.8, 1.2), grad_scale=1.0 / 24, kl_scale=1.0 / 3)
    got0 = S.pg_rows_ref(mu, zero, S.BOUNDS, act, adv, old_logprob=old, clip=kw["clip"], grad_scale=kw["grad_scale"])
    want0 = L.pg_ref(mu, act, adv, 1.0, old_logprob=old, clip=kw["clip"], grad_scale=kw["grad_scale"])
    for k in ("logprob", "ratio", "ratio_bound", "clipped", "c", "surrogate", "dpred_bits"):
        assert np.array_equal(got0[k], want0[k]), k
    got = S.pg_rows_ref(mu, zero, S.BOUNDS, act, adv, old_logprob=old, ref_pred=ref_mu, ref_log_scale=zero, **kw)
    want = L.pg_ref(mu, act, adv, 1.0, old_logprob=old, ref_pred=ref_mu, **kw)
    for k in ("kl", "kl_bound", "kl_on_policy", "kl_grad", "dpred64", "dpred_floor", "dpred_lo", "dpred_hi"):
        assert np.array_equal(got[k], want[k]), k


def test_equal_power_of_two_scales_are_the_fixed_scale_kl():
    """s_c = k ln 2 does not round-trip through expf, so the case is built from s = 0 and the fixed-scale twin's own (b, inv_b, log_norm)."""
    rows, adim, G = 5, 7, 3
    scale = [0.5, 2.0, 0.25, 1.0, 0.125, 4.0, 0.0625]
    mu, keys, adv, ref_mu = _anchor_world(rows, adim, G, seed=3)
    act = L.sample_ref(mu, scale, G, seed=S.SEED, call=2, row_keys=keys)["action32"]
    old = _old(L.logprob32(mu, act, *L.scales(scale, adim)[1:]), rows, G)
    kw = dict(kl_coef=0.375, clip=(0.8, 1.2), grad_scale=1.0 / 24, kl_scale=1.0 / 3)
    zero = np.zeros((rows, adim), F32)
    got = S.pg_rows_ref(mu, zero, S.BOUNDS, act, adv, old_logprob=old, ref_pred=ref_mu, ref_log_scale=zero, elem=S.fixed_elem(scale, rows, adim), **kw)
    want = L.pg_ref(mu, act, adv, scale, old_logprob=old, ref_pred=ref_mu, **kw)
    for k in ("logprob", "ratio", "clipped", "c", "surrogate", "kl", "kl_bound", "kl_grad", "dpred_lo", "dpred_hi"):
        assert np.array_equal(got[k], want[k]), k
    assert bool((want["kl"] > 0).any())


def test_kl_is_zero_on_policy_and_the_split_stays_rare():
    for rows, adim, G in ((24, 7, 2), (67, 16, 64), (1, 1, 1)):
        w = S.pg_inputs(rows, adim, G)
        on = S.pg_rows_ref(w["mu"], w["s"], S.BOUNDS, w["act"], w["adv"], old_logprob=w["old"], ref_pred=w["mu"], ref_log_scale=w["s"], **S.PG_KW)
        assert bool((on["kl"].astype(F32).view(np.int32) == 0).all()) and bool((on["kl_d"] == 0).all()) and bool(on["kl_on_policy"].all())
        assert np.array_equal(on["dpred_lo"], on["dpred_hi"]) and np.array_equal(on["dlog_scale_lo"], on["dlog_scale_hi"])
        assert np.array_equal(on["dpred_lo"], L.bf16_round((on["surrogate"] + F32(0.0)).astype(F32)))
        # the inputs of the GPU test: the one-ulp allowance is the exception in the restatement alone
        ref = S.pg_rows_ref(w["mu"], w["s"], S.BOUNDS, w["act"], w["adv"], old_logprob=w["old"], ref_pred=w["ref_mu"], ref_log_scale=w["ref_s"], **S.PG_KW)
        if rows * adim >= 100:
            for name in ("dpred", "dlog_scale"):
                split = ref[name + "_lo"] != ref[name + "_hi"]
                print(f"rows {rows} adim {adim} G {G}: {name} split on {split.mean():.4f} of the elements")
                assert split.mean() < 0.05, name
            assert ref["kl_on_policy"].any() and not ref["kl_on_policy"].all()
            assert 0 < int(ref["clipped"].sum()) < rows * G


def _bf16_values(lo, hi, full_above):
    """Every bf16 value in [lo, hi] of magnitude >= full_above, and below that two per binade and sign (smallest and largest mantissa), and 0."""
    bits = np.arange(0, 0x10000, dtype=np.uint32)
    v = (bits << 16).astype(np.uint32).view(F32)
    keep = np.isfinite(v) & (v >= lo) & (v <= hi)
    mant = bits & 0x7F
    keep &= (np.abs(v) >= full_above) | (mant == 0) | (mant == 0x7F)
    return np.unique(v[keep])


def test_kl_is_never_negative():
    """kl_d >= 0 for pairs of bf16 log-scales in the default bounds on a grid of D.  Every bf16 value of magnitude >= 2^-12 enters (below it two per
    binade and sign, and 0: 1.1e9 pairs of all 33 thousand values do not fit a test of seconds) -- about 3.9 thousand values, every pair of them.
    The twin's fp32 value is formed as the kernel forms it, from correctly rounded float64 library values: expm1(u) >= u and 1 - e^-q <= q
    survive one monotone rounding because u and q are fp32 numbers themselves."""
    v = _bf16_values(S.BOUNDS[0], S.BOUNDS[1], 2.0 ** -12)
    assert v.size > 3500 and 0.0 in v and F32(S.BOUNDS[0]) in v and F32(S.BOUNDS[1]) in v
    b = np.exp(v.astype(np.float64)).astype(F32)
    inv_b = (F32(1.0) / b).astype(F32)
    worst = np.inf
    for D in (0.0, 2.0 ** -8, 1.0 / 64, 0.25, 1.0, 2.0):
        q = (F32(D) * inv_b).astype(F32)                                        # [n]: depends on the live scale alone
        x = (-np.expm1(-q.astype(np.float64))).astype(F32)
        t2 = (q - x).astype(F32)
        for i in range(0, v.size, 256):
            u = (v[i:i + 256, None] - v[None, :]).astype(F32)                   # live rows i.., every reference
            m = np.expm1(u.astype(np.float64)).astype(F32)
            rho = np.exp(u.astype(np.float64)).astype(F32)
            kl = ((m - u).astype(F32) + (rho * t2[i:i + 256, None]).astype(F32)).astype(F32)
            worst = min(worst, float(kl.min()))
            assert bool((kl >= 0).all()) and bool(np.isfinite(kl).all()), f"D = {D}: kl_d = {kl.min()}"
    assert worst == 0.0


def test_a_clamped_log_scale_takes_no_gradient():
    rows, adim, G = 24, 7, 2
    w = S.pg_inputs(rows, adim, G)
    s = w["s"]
    with np.errstate(invalid="ignore"):
        out = np.isnan(s) | (s < S.BOUNDS[0]) | (s > S.BOUNDS[1])
    assert int(out.sum()) == 3 and bool((s == F32(S.BOUNDS[0])).any()) and bool((s == F32(S.BOUNDS[1])).any())
    el = S.elem_ref(s, S.BOUNDS)
    assert np.array_equal(el["inside"], ~out) and bool(np.isfinite(el["b"]).all())
    assert bool((el["s_c"][np.isnan(s)] == F32(S.BOUNDS[0])).all())
    ref0 = S.pg_rows_ref(w["mu"], s, S.BOUNDS, w["act"], w["adv"], old_logprob=w["old"], clip=(0.8, 1.2), grad_scale=1.0 / 24, entropy_coef=0.25, ent_scale=1.0 / 3)
    ref = S.pg_rows_ref(w["mu"], s, S.BOUNDS, w["act"], w["adv"], old_logprob=w["old"], ref_pred=w["ref_mu"], ref_log_scale=w["ref_s"], **S.PG_KW)
    assert bool((ref0["dlog_scale_bits"][out] == 0).all()) and bool((ref0["dlog_scale_bits"][~out] != 0).all())
    assert bool((ref["dlog_scale_lo"][out].view(np.int32) == 0).all()) and bool((ref["dlog_scale_hi"][out].view(np.int32) == 0).all())
    for k in ("logprob", "entropy", "surrogate", "surrogate_s"):
        assert bool(np.isfinite(ref[k]).all()), k
    for k in ("kl", "dpred_lo", "dpred_hi", "dlog_scale_lo", "dlog_scale_hi"):
        assert bool(np.isfinite(ref[k]).all()), k
    # a skipped draw full of NaN leaves the row finite
    act = w["act"].copy()
    adv = w["adv"].copy()
    act[:, 0], adv[:, 0] = np.nan, 0.0
    nan = S.pg_rows_ref(w["mu"], s, S.BOUNDS, act, adv, old_logprob=w["old"], clip=(0.8, 1.2), grad_scale=1.0 / 24)
    assert bool(np.isfinite(nan["surrogate"]).all()) and bool(np.isfinite(nan["surrogate_s"]).all())
