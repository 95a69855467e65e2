"""The float64 twin of ovla_token_pg_group (tests/token_group_reference.py) checked against itself on the CPU: its gradient is the derivative of its
loss (a central difference pins the signs of the surrogate, KL and entropy terms), it reduces to pg_ref, the entropy gradient sums to zero over a
row, and rl.group_advantages centres every group."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import token_group_reference as G
from tests import token_sample_reference as R
from tests.conftest import load_pkg

VOCAB, LD, LO, HI = 300, 304, 3, 261
H_STEP = 2.0 ** -13            # the finite-difference step on a logit (a power of two: z + h is exact in float64)
EPS64 = 2.0 ** -52


def _inputs(Gn, seed=0, T=1.6):
    g = torch.Generator().manual_seed(4100 + seed + Gn)
    rows = 3
    z = R.eighths(g, (rows, LD))
    tokens = torch.randint(LO, HI, (rows, Gn), generator=g).numpy()
    if Gn > 1:
        tokens[:, 1] = tokens[:, 0]                         # two samples share a token
    adv = (torch.randint(1, 9, (rows, Gn), generator=g).double() / 4.0 * torch.where(torch.rand((rows, Gn), generator=g) < 0.5, -1.0, 1.0)).numpy()
    lp = G.group_ref(z, VOCAB, LO, HI, T, tokens, adv)["logprob"].numpy()
    # ratios e^(+-0.5) and e^(+-0.05): far from the clip bounds 0.8 / 1.2 on either side, so the surrogate is smooth around the inputs
    shift = np.where(np.arange(rows * Gn).reshape(rows, Gn) % 2 == 0, 0.5, -0.05) * np.where(np.arange(Gn)[None, :] % 3 == 0, -1.0, 1.0)
    old = lp + shift
    ref = lp + np.where(np.arange(Gn)[None, :] % 2 == 0, 0.5, -0.5)
    return z, tokens, adv, old, ref


def _fd_bound(z, T, tokens, adv, old, ref, kw, r):
    """|central difference - derivative| <= h^2 / 6 max |L'''| + rounding.  With u = s_j, q = d logprob / du in [-1, 1], |q'| <= 1/4, |q''| < 0.1:
    (A ratio)''' = A ratio (q^3 + 3 q q' + q'') is at most 1.85 |A| ratio, the same for e^d, and d''' < 0.1;  H''' is at most 2.5 K + 0.65 with
    K = 1/e + log n (token_group_reference's dH/du = -p (log p + H) differentiated twice, every factor p |log p + H| <= K, p (1 - p) <= 1/4).  A step
    h on z is a step h invT on u: three factors invT.  The ratios move by at most e^h over the step (factor 1.01 below).  Rounding: the float64 loss
    is a sum of n exponentials, a logarithm and a few products, known to 64 eps of the magnitudes of its terms; the difference divides that by h."""
    invT = float(R.inv_temperature(T))
    n = HI - LO
    gs, klc, es, clip = kw["grad_scale"], kw["kl_coef"], kw["ent_scale"], kw["clip"]
    ref0 = G.group_ref(z, VOCAB, LO, HI, T, tokens, adv, old_logprob=old, ref_logprob=ref, **kw)
    ratio = ref0["ratio"][r]
    m3 = (1.85 * np.abs(adv[r]) * ratio * 1.01).sum() * gs
    mag = (np.abs(adv[r]) * np.maximum(ratio, clip[1])).sum() * gs
    if ref is not None:
        d = ref[r] - ref0["logprob"][r].numpy()
        m3 += klc * gs * (1.85 * np.exp(d) * 1.01 + 0.1).sum()
        mag += klc * gs * (np.exp(d) + np.abs(d) + 1).sum()
    K = 1.0 / math.e + math.log(n)
    m3 += abs(es) * (2.5 * K + 0.65)
    mag += abs(es) * math.log(n)
    return H_STEP ** 2 / 6.0 * invT ** 3 * m3 + 64 * EPS64 * mag / H_STEP


@pytest.mark.parametrize("terms", ("all", "surrogate", "kl", "entropy"))
@pytest.mark.parametrize("Gn", (1, 3, 8))
def test_gradient_is_the_derivative_of_the_loss(terms, Gn):
    T = 1.6
    z, tokens, adv, old, ref = _inputs(Gn, T=T)
    kw = dict(kl_coef=0.04, ent_scale=0.01, clip=(0.8, 1.2), grad_scale=1.0 / 7)
    if terms == "surrogate":
        ref, kw["ent_scale"] = None, 0.0
    elif terms == "kl":
        adv, kw["ent_scale"] = np.zeros_like(adv), 0.0
    elif terms == "entropy":
        adv, ref = np.zeros_like(adv), None
    twin = G.group_ref(z, VOCAB, LO, HI, T, tokens, adv, old_logprob=old, ref_logprob=ref, **kw)
    invT = float(R.inv_temperature(T))
    n = HI - LO
    tok_rel = np.clip(tokens, LO, HI - 1) - LO
    resolved = []
    for r in range(z.shape[0]):
        z64 = z[r, LO:HI].double().numpy()
        f = lambda zz: G.row_loss64(zz * invT, tok_rel[r], adv[r], old[r], None if ref is None else ref[r], **kw)
        fd = (f(z64[None, :] + H_STEP * np.eye(n)) - f(z64[None, :] - H_STEP * np.eye(n))) / (2 * H_STEP)
        got = twin["grad64"][r, LO:HI].numpy()
        bound = _fd_bound(z, T, tokens, adv, old, ref, kw, r)
        err = np.abs(fd - got).max()
        assert err <= bound, f"{terms} G={Gn} row {r}: |central difference - gradient| = {err:.3e} > {bound:.3e}"
        resolved.append(np.abs(got).max() / bound)
        assert bool((twin["grad64"][r, :LO] == 0).all()) and bool((twin["grad64"][r, HI:] == 0).all())
    # (a row whose only sample is gated has a zero gradient; the others must stand far above the bound for the comparison to mean anything)
    assert max(resolved) > 1e4, f"{terms} G={Gn}: the bound is not small against any row's gradient ({resolved})"


def test_signs():
    """More KL weight pulls the log-probability of a sample the reference likes better (ref > logprob) up; an entropy bonus pushes the likeliest
    column's logit down."""
    z, tokens, adv, old, ref = _inputs(1)
    zero = np.zeros_like(adv)
    lp = G.group_ref(z, VOCAB, LO, HI, 1.0, tokens, zero)["logprob"].numpy()
    g_kl = G.group_ref(z, VOCAB, LO, HI, 1.0, tokens, zero, ref_logprob=lp + 0.5, kl_coef=1.0)
    g_en = G.group_ref(z, VOCAB, LO, HI, 1.0, tokens, zero, ent_scale=1.0)
    for r in range(z.shape[0]):
        assert g_kl["grad64"][r, tokens[r, 0]] < 0            # descent raises the token's logit
        assert bool((g_kl["kl"][r] > 0).all())
        top = int(g_en["p"][r].argmax())
        assert g_en["grad64"][r, LO + top] > 0


@pytest.mark.parametrize("T", (0.5, 1.0, 1.6))
def test_reduces_to_pg_ref(T):
    z, tokens, adv, old, _ = _inputs(1, T=T)
    for o in (None, old):
        a = R.pg_ref(z, VOCAB, LO, HI, T, tokens[:, 0], adv[:, 0], old_logprob=None if o is None else o[:, 0], grad_scale=0.25)
        b = G.group_ref(z, VOCAB, LO, HI, T, tokens, adv, old_logprob=o, grad_scale=0.25)
        assert torch.equal(a["grad64"], b["grad64"]) and torch.equal(a["logprob"], b["logprob"][:, 0]) and torch.equal(a["entropy"], b["entropy"])
        assert np.array_equal(a["clipped"], b["clipped"][:, 0]) and np.array_equal(a["ratio"], b["ratio"][:, 0])
        assert bool((b["grad_floor"] >= a["grad_floor"]).all())
        if o is None:                                        # the same floor but for the term's and the add's rounding
            assert bool((b["grad_floor"] <= 2 * a["grad_floor"]).all())
        assert b["kl"] is None


def test_loss_values_by_hand():
    z, tokens, adv, _, _ = _inputs(1)
    one = np.ones_like(adv)
    lp = G.group_ref(z, VOCAB, LO, HI, 1.0, tokens, one)["logprob"].numpy()[:, 0]
    assert np.array_equal(G.loss64(z, LO, HI, 1.0, tokens, one), -one[:, 0])       # ratio = 1 without old log-probabilities: the value is -A
    # with old = logprob - log 2 the ratio is 2, clipped at 1.2 for A > 0: value -1.2 A
    assert np.allclose(G.loss64(z, LO, HI, 1.0, tokens, one, old_logprob=(lp - math.log(2.0))[:, None]), -1.2)
    # the KL value on its own: k3 of d = 0.5
    assert np.allclose(G.loss64(z, LO, HI, 1.0, tokens, 0 * one, ref_logprob=(lp + 0.5)[:, None], kl_coef=2.0), 2.0 * (math.expm1(0.5) - 0.5))


def test_entropy_gradient_sums_to_zero():
    """sum_j p_j (log p_j + H) = -H + H: the entropy cannot move the row's total logit mass."""
    z, tokens, adv, _, _ = _inputs(3)
    g = G.group_ref(z, VOCAB, LO, HI, 1.6, tokens, np.zeros_like(adv), ent_scale=0.7)
    tot = g["grad64"].sum(-1)
    scale = g["grad64"].abs().sum(-1)
    assert bool((scale > 0).all()) and bool((tot.abs() <= 64 * EPS64 * scale).all()), (tot, scale)


def test_group_advantages_on_the_host():
    load_pkg()
    rl = importlib.import_module("openvla-oft_amd.rl")
    g = torch.Generator().manual_seed(5)
    r = torch.randn((6, 8), generator=g)
    r[2] = 3.25                                              # a constant group
    a = rl.group_advantages(r)
    assert a.shape == (6, 8) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
    assert bool((a.mean(1).abs() <= 8 * 2.0 ** -23 * a.abs().max(1).values.clamp_min(1.0)).all())
    assert bool((a[2] == 0).all())
    assert bool((rl.group_advantages(torch.full((3, 1), 2.0)) == 0).all())
    want = G.group_advantages_ref(r.numpy())
    assert np.allclose(a.numpy(), want, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        rl.group_advantages(torch.zeros(4))
