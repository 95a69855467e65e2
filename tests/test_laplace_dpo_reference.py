"""The numpy twin of ovla_laplace_dpo (tests/laplace_dpo_reference.py) against its own float64 definition, on the CPU: the twin's fp32 gradient sums
against central differences of objective64 in every term, planted mutants that the same comparison must catch, and the contract's exact identities.
(The twin against the kernel: tests/test_laplace_dpo_gpu.py.)"""
import itertools

import numpy as np
import pytest

from tests import laplace_dpo_reference as D
from tests import laplace_policy_reference as L
from tests import laplace_scale_reference as S

F32 = np.float32
B, CHUNK, ADIM = 3, 4, 3
STEP = 2.0 ** -20          # the difference step: MIN_GAP / 2^15, so no |a - mu| or |a - ref| changes sign inside it
# The twin's fp32 sums against the float64 derivative.  The margin is a sum of 4 * chunk * adim = 48 rounded terms of magnitude below 16 (adim = 3,
# q <= 4.5), so it carries at most 48 * 16 * 2^-24 < 5e-5 of absolute error; beta <= 0.1 turns that into 5e-6 in z, which moves k by at most that
# share of its size (|d log k / d z| <= 1); for IPO k = -2 (m - tau) with |m - tau| of order 5 takes 1e-4 / 5 relative.  The remaining operations
# add a few 2^-24 each.  RTOL = 1e-4 of the largest gradient element covers both with a factor of five to spare; a mutant is off by order 1.
RTOL = 1e-4
FIXED_SCALE = [0.7, 1.0, 0.3]


def setup(learned, weights, seed=3):
    w = D.dpo_inputs(B, CHUNK, ADIM, seed=seed, learned=learned)
    rows = B * CHUNK
    if learned:
        elem, ref_elem, s64, ref_s64 = S.elem_ref(w["s"], S.BOUNDS), S.elem_ref(w["ref_s"], S.BOUNDS), w["s"].astype(np.float64), w["ref_s"].astype(np.float64)
    else:
        elem = ref_elem = S.fixed_elem(FIXED_SCALE, rows, ADIM)
        s64 = ref_s64 = np.log(elem["b"].astype(np.float64))
    return w, elem, ref_elem, s64, ref_s64, (w["weight"] if weights else None)


def central(w, s64, ref_s64, kw):
    """Central differences of objective64 with respect to every element of mu and of s -> (d mu, d s) float64 [rows, adim]."""
    mu = w["mu"].astype(np.float64)
    f = lambda m_, s_: D.objective64(m_, s_, w["ref_mu"], ref_s64, w["chosen"], w["rejected"], CHUNK, **kw)[0]   # noqa: E731
    d_mu, d_s = np.zeros_like(mu), np.zeros_like(mu)
    for i, j in itertools.product(range(mu.shape[0]), range(mu.shape[1])):
        e = np.zeros_like(mu)
        e[i, j] = STEP
        d_mu[i, j] = (f(mu + e, s64) - f(mu - e, s64)) / (2 * STEP)
        d_s[i, j] = (f(mu, s64 + e) - f(mu, s64 - e)) / (2 * STEP)
    return d_mu, d_s


def gradient_errors(loss_type, eps, nll_coef, weights, learned, mutant=None):
    w, elem, ref_elem, s64, ref_s64, weight = setup(learned, weights)
    assert STEP * 2 ** 10 < D.MIN_GAP
    kw = dict(weight=weight, beta=0.1, eps=eps, loss_type=loss_type, grad_scale=1.0 / B, nll_coef=nll_coef, nll_scale=1.0 / (B * CHUNK))
    twin = D.dpo_ref(w["mu"], w["ref_mu"], w["chosen"], w["rejected"], CHUNK, elem, ref_elem, mutant=mutant, **kw)
    d_mu, d_s = central(w, s64, ref_s64, kw)
    c_mu, c_s = D.grad64(w["mu"], s64, w["ref_mu"], ref_s64, w["chosen"], w["rejected"], CHUNK, **kw)
    assert float(np.abs(d_mu).max()) > 1e-3 and float(np.abs(d_s).max()) > 1e-3, "the case has a gradient to check"
    closed = max(np.abs(c_mu - d_mu).max() / np.abs(d_mu).max(), np.abs(c_s - d_s).max() / np.abs(d_s).max())
    assert closed < 1e-6, f"grad64 is not the derivative of objective64: {closed:.3e}"
    return float(np.abs(twin["acc_mu"] - d_mu).max() / np.abs(d_mu).max()), float(np.abs(twin["acc_s"] - d_s).max() / np.abs(d_s).max()), twin


@pytest.mark.parametrize("learned", (False, True))
@pytest.mark.parametrize("weights", (False, True))
@pytest.mark.parametrize("nll_coef", (0.0, 0.5))
@pytest.mark.parametrize("eps", (0.0, 0.1))
@pytest.mark.parametrize("loss_type", (D.SIGMOID, D.IPO))
def test_gradient_against_central_differences(loss_type, eps, nll_coef, weights, learned):
    e_mu, e_s, twin = gradient_errors(loss_type, eps, nll_coef, weights, learned)
    print(f"relative error to the largest element: d mu {e_mu:.3e}, d s {e_s:.3e}")
    assert e_mu <= RTOL and e_s <= RTOL, f"the twin's gradient is not the derivative of the stated total: d mu {e_mu:.3e}, d s {e_s:.3e}"
    assert bool(np.all(twin["c"][:, 0] != 0)) and bool(np.all(twin["c"][:, 1] != 0)), "no sample of the case is skipped: every element is compared"
    if loss_type == D.SIGMOID:                                     # the twin's own fp32 chain lies inside its own bounds
        assert bool(np.all(np.abs(twin["loss32"] - twin["loss"]) <= twin["loss_bound"])) and bool(np.all(np.abs(twin["coef32"] - twin["coef"]) <= twin["coef_bound"]))
    else:
        assert not twin["loss_bound"].any() and not twin["coef_bound"].any(), "IPO is IEEE: exact"


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_planted_mutants_are_caught(mutant):
    for loss_type in (D.SIGMOID, D.IPO):
        if loss_type == D.IPO and mutant == "smoothing_sign":
            continue                                               # (IPO has no label smoothing)
        for learned in (False, True):
            e_mu, e_s, _ = gradient_errors(loss_type, 0.1, 0.5, True, learned, mutant=mutant)
            assert max(e_mu, e_s) > 100 * RTOL, f"{mutant} (loss_type {loss_type}, learned {learned}) passes the central-difference check: {e_mu:.3e}, {e_s:.3e}"


def test_sigmoid_bounds_hold_over_the_range_of_z():
    z = np.concatenate([np.linspace(-200, 200, 4001), [-1e-6, 0.0, 1e-6, 16.6, 17.0, 87.0, 88.0, 103.0, 104.0]]).astype(F32)
    for eps in (0.0, 0.1, 0.4375):
        t = D.sigmoid_terms(z, 0.25, eps)
        assert bool(np.isfinite(t["loss32"]).all()) and bool(np.isfinite(t["k32"]).all())
        assert bool(np.all(np.abs(t["loss32"] - t["loss"]) <= t["loss_bound"])) and bool(np.all(np.abs(t["k32"] - t["k"]) <= t["k_bound"]))
        assert bool(np.all(t["loss_bound"] <= 6e-7 * np.maximum(1.0, np.abs(z)))), "the bound stays a few ulps of the larger softplus (of 1 below it)"
        assert bool(np.all(t["k_bound"] <= 1e-6 * 0.25)), "k's bound stays a few ulps of beta"
        # the float64 values are the textbook forms
        z64 = z.astype(np.float64)
        assert np.allclose(t["loss"], float(F32(1.0) - F32(eps)) * np.logaddexp(0, -z64) + float(F32(eps)) * np.logaddexp(0, z64), rtol=1e-12, atol=1e-300)


def test_identities():
    for learned in (False, True):
        w, elem, ref_elem, _, _, weight = setup(learned, True)
        kw = dict(weight=weight, beta=0.1, grad_scale=1.0 / B)
        args = (w["mu"], w["ref_mu"])
        # chosen == rejected: m == 0 exactly, the sigmoid loss is float32(ln 2), every gradient element +0
        same = D.dpo_ref(*args, w["chosen"], w["chosen"], CHUNK, elem, ref_elem, **kw)
        assert not same["margin"].view(np.int32).any(), "chosen == rejected: the margin is not +0"
        assert np.array_equal(same["loss32"], np.full(B, F32(np.log(2.0)))) and bool(np.all(same["coef32"] != 0))
        assert not same["dpred_bits"].any() and not same["dlog_scale_bits"].any(), "chosen == rejected: x + (-x) is +0 in every element"
        # pred == ref_pred bitwise with equal scales: h == (0, 0) exactly
        on = D.dpo_ref(w["mu"], w["mu"], w["chosen"], w["rejected"], CHUNK, elem, elem, **kw)
        assert not on["h"].view(np.int32).any() and not on["margin"].view(np.int32).any()
        # swapping chosen and rejected negates the margin bit for bit
        fwd = D.dpo_ref(*args, w["chosen"], w["rejected"], CHUNK, elem, ref_elem, **kw)
        rev = D.dpo_ref(*args, w["rejected"], w["chosen"], CHUNK, elem, ref_elem, **kw)
        assert bool(np.all(fwd["margin"] != 0)) and np.array_equal((-fwd["margin"]).view(np.int32), rev["margin"].view(np.int32))
        assert np.array_equal(fwd["h"][:, ::-1].view(np.int32), rev["h"].view(np.int32))
        # |z| >= 200 on either side: finite loss and coef
        big = float(200.0 / np.abs(fwd["margin"]).min()) * 1.01
        for r in (D.dpo_ref(*args, w["chosen"], w["rejected"], CHUNK, elem, ref_elem, weight=weight, beta=big, eps=0.1, grad_scale=1.0 / B),
                  D.dpo_ref(*args, w["rejected"], w["chosen"], CHUNK, elem, ref_elem, weight=weight, beta=big, eps=0.1, grad_scale=1.0 / B)):
            assert bool(np.all(np.abs(F32(big) * r["margin"]) >= 200)) and all(bool(np.isfinite(r[k]).all()) for k in ("loss", "loss32", "coef", "coef32", "acc_mu", "acc_s"))
        # a weight == 0 observation filled with NaN leaves every output of it +0 and the others' bits unchanged
        wz = weight.copy()
        wz[1] = 0.0
        hole = {k: v.copy() for k, v in w.items()}
        sl = slice(CHUNK, 2 * CHUNK)
        for k in ("mu", "ref_mu", "chosen", "rejected"):
            hole[k][sl] = np.nan
        nan_kw = dict(weight=wz, beta=0.1, eps=0.1, grad_scale=1.0 / B, nll_coef=0.5, nll_scale=1.0 / (B * CHUNK))
        got = D.dpo_ref(hole["mu"], hole["ref_mu"], hole["chosen"], hole["rejected"], CHUNK, elem, ref_elem, **nan_kw)
        ref = D.dpo_ref(*args, w["chosen"], w["rejected"], CHUNK, elem, ref_elem, **nan_kw)
        for k in ("logprob", "ref_logprob", "dpred_bits", "dlog_scale_bits", "acc_mu", "acc_s"):
            assert not np.ascontiguousarray(got[k][sl]).view(np.uint8).any(), f"w == 0: {k} of the skipped observation is not +0"
            keep = np.r_[0:CHUNK, 2 * CHUNK:3 * CHUNK]
            assert np.array_equal(np.ascontiguousarray(got[k][keep]).view(np.uint8), np.ascontiguousarray(ref[k][keep]).view(np.uint8)), f"w == 0: {k} of the others changed"
        for k in ("h", "margin", "loss32", "coef32", "loss", "coef", "c"):
            assert not np.ascontiguousarray(got[k][1]).view(np.uint8).any(), f"w == 0: {k} of the skipped observation is not +0"
            assert np.array_equal(np.ascontiguousarray(got[k][[0, 2]]).view(np.uint8), np.ascontiguousarray(ref[k][[0, 2]]).view(np.uint8)), f"w == 0: {k} of the others changed"
        assert bool(got["skipped"][1]) and int(got["skipped"].sum()) == 1


def test_nll_alone_is_the_group_gradient_of_the_chosen_chunk():
    """beta = 0: k = 0, coef = +0, the rejected chunk is skipped and the gradient is S.pg_rows_ref's at G = 1 with adv = 1 and grad_scale = nll_scale."""
    w, elem, ref_elem, _, _, _ = setup(True, False)
    rows = B * CHUNK
    got = D.dpo_ref(w["mu"], w["ref_mu"], w["chosen"], w["rejected"], CHUNK, elem, ref_elem, beta=0.0, eps=0.1, nll_coef=1.0, nll_scale=1.0 / rows)
    assert not got["coef32"].view(np.int32).any() and not got["c"][:, 1].any()
    want = S.pg_rows_ref(w["mu"], None, None, w["chosen"][:, None, :], np.ones((rows, 1), F32), grad_scale=1.0 / rows, elem=elem)
    assert np.array_equal(got["dpred_bits"], want["dpred_bits"]) and np.array_equal(got["dlog_scale_bits"], want["dlog_scale_bits"])
    assert got["dpred_bits"].any() and got["dlog_scale_bits"].any()
