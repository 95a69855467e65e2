"""The numpy restatement of the Laplace policy (tests/laplace_policy_reference.py) checked against itself on the CPU: the variate is exact and
symmetric over every 23-bit integer, the unit-Laplace moments follow from those integers, the closed-form KL and its gradient are what a
quadrature and a central difference give, the reference tells the planted mutants apart, and the two kernels' refusals fire before any launch."""
import importlib
import math

import numpy as np
import pytest
import torch

from tests import laplace_policy_reference as L
from tests.conftest import load_pkg

SEED, CALL = 0x1234ABCD5678EF01, 9
N23 = 1 << 23


def test_variate_is_exact_and_symmetric_over_every_integer():
    k = np.arange(N23, dtype=np.int64)
    u, x, t = L.variate(k)
    m = 2 * k + 1                                                # u = m 2^-24 with m odd below 2^24: exact in fp32
    assert np.array_equal(u.astype(np.float64), m * 2.0 ** -24)
    assert np.array_equal(x.astype(np.float64), (m - N23) * 2.0 ** -24)
    assert np.array_equal(t.astype(np.float64), 1.0 - np.abs(m - N23) * 2.0 ** -23)
    assert float(t.min()) == 2.0 ** -23 and float(t.max()) == 1.0 - 2.0 ** -23 and bool(np.all(x != 0))
    assert np.array_equal(x, -x[::-1]) and np.array_equal(t, t[::-1])          # k <-> 2^23 - 1 - k flips the sign and keeps the magnitude
    assert -math.log(2.0 ** -23) <= L.E_MAX


def test_unit_laplace_moments_from_the_integers():
    """|e| = -log t takes the values -log((2 j + 1) h / 2), h = 2^-22, j < 2^22, each twice (once per sign): the midpoint rule for the integrals
    of -log t and log^2 t over (0, 1), which are 1 and 2.  Both integrands are convex, so the rule errs low; on the first cell by exactly
    h (1 - log 2) and h (2 L (1 - log 2) + 2 - log^2 2) with L = -log h, on the others by at most h^3 / 24 max f'': summed, (pi^2 / 144) h and
    (pi^2 / 72) (1 + L) h.  The first moment of e is exactly 0 by symmetry."""
    h = 2.0 ** -22
    j = np.arange(1 << 22, dtype=np.float64)
    a = -np.log((2.0 * j + 1.0) * (h / 2.0))
    m1, m2 = float(a.mean()), float((a * a).mean())
    Lh, l2 = -math.log(h), math.log(2.0)
    e1 = h * ((1.0 - l2) + math.pi ** 2 / 144.0)
    e2 = h * ((2.0 * Lh * (1.0 - l2) + 2.0 - l2 * l2) + math.pi ** 2 / 72.0 * (1.0 + Lh))
    tiny = 1e-12                                                 # the float64 sums themselves
    assert -tiny <= 1.0 - m1 <= e1 + tiny, (1.0 - m1, e1)
    assert -tiny <= 2.0 - m2 <= e2 + tiny, (2.0 - m2, e2)
    # the same numbers through the reference's own path, on the full integer range
    e = L.noise64(np.arange(N23, dtype=np.uint64) << np.uint64(9))
    assert np.array_equal(e, -e[::-1]) and abs(float(np.abs(e).mean()) - m1) < 1e-12 and abs(float((e * e).mean()) - m2) < 1e-11
    assert float(np.abs(e).max()) <= L.E_MAX


def _inputs(rows=5, G=4, adim=7, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    mu = L.means(g, rows, adim)
    keys = (torch.arange(rows * G).view(rows, G) * 7919 - 40000).numpy()
    draw = L.sample_ref(mu, L.SCALES[adim], G, seed=SEED, call=CALL, row_keys=keys)
    adv = (torch.randint(1, 9, (rows, G), generator=g).double() / 4.0 * torch.where(torch.rand((rows, G), generator=g) < 0.5, -1.0, 1.0)).numpy()
    return mu, keys, draw, adv


def test_draws_are_laplace_around_the_mean():
    mu, keys, draw, _ = _inputs(rows=64, G=64)
    z = (draw["action"] - mu[:, None, :].astype(np.float64)) / L.scales(L.SCALES[7], 7)[0].astype(np.float64)[None, None, :]
    assert np.allclose(z, draw["e"], rtol=0, atol=1e-12)
    n = z.size                                                   # 28672 draws: mean 0 +- sqrt(2 / n), E|e| = 1 +- sqrt(1 / n); six sigma
    assert abs(z.mean()) < 6 * math.sqrt(2.0 / n) and abs(np.abs(z).mean() - 1.0) < 6 * math.sqrt(1.0 / n)
    assert len(np.unique(draw["e"])) > 0.99 * n
    # the twin's fp32 action is inside its own bound of the float64 one
    assert bool(np.all(np.abs(draw["action32"].astype(np.float64) - draw["action"]) <= draw["action_bound"]))


def test_logprob_is_the_laplace_density():
    mu, _, draw, _ = _inputs()
    b, inv_b, log_norm = L.scales(L.SCALES[7], 7)
    lp = L.logprob32(mu, draw["action32"], inv_b, log_norm)
    want = (-np.abs(draw["action32"].astype(np.float64) - mu[:, None, :]) / b[None, None, :] - np.log(2.0 * b.astype(np.float64))[None, None, :]).sum(-1)
    assert np.allclose(lp, want, rtol=0, atol=7 * 4 * 2.0 ** -24 * np.abs(want).max())


def test_kl_is_the_closed_form_and_its_gradient_the_derivative():
    """KL(Laplace(mu, b) || Laplace(ref, b)) = q - (1 - e^-q), q = |mu - ref| / b: against the integral of p log(p / p_ref) by quadrature, and
    the gradient term against a central difference."""
    b = 0.3
    for D in (0.0, 0.01, 0.25, 1.0, 3.0):
        zs = np.linspace(-60.0, 60.0, 2_400_001) * b
        p = np.exp(-np.abs(zs) / b) / (2 * b)
        integral = float((p * (np.abs(zs - D) - np.abs(zs)) / b).sum() * (zs[1] - zs[0]))
        q = D / b
        assert abs(integral - (q + math.expm1(-q))) < 1e-6, (D, integral, q + math.expm1(-q))
    mu = np.array([[0.5, -0.25, 0.125, 0.0]], dtype=np.float32)
    ref = np.array([[0.25, 0.5, 0.125, -1.0]], dtype=np.float32)
    acts = np.zeros((1, 1, 4), dtype=np.float32)
    out = L.pg_ref(mu, acts, np.zeros((1, 1)), [0.3, 1.0, 0.5, 0.7], ref_pred=ref, kl_coef=0.5, kl_scale=0.25)
    bs = np.array([0.3, 1.0, 0.5, 0.7], dtype=np.float32).astype(np.float64)
    kl = lambda m: float((np.abs(m - ref[0]) / bs + np.expm1(-np.abs(m - ref[0]) / bs)).sum())
    assert abs(out["kl"][0] - kl(mu[0].astype(np.float64))) <= out["kl_bound"][0] + 1e-15
    hstep = 2.0 ** -12
    for d in range(4):
        e = np.zeros(4)
        e[d] = hstep
        fd = 0.5 * 0.25 * (kl(mu[0] + e) - kl(mu[0] - e)) / (2 * hstep)
        if d == 2:                                               # on policy: exactly +0, and the kink's two one-sided slopes cancel
            assert out["kl_grad"][0, d] == 0.0 and bool(out["kl_on_policy"][0, d])
        else:                                                    # |f'''| = e^-q / b^3 <= 38: h^2 / 6 of it
            assert abs(fd - out["kl_grad"][0, d]) < 0.125 * hstep ** 2 / 6 * 38 + 1e-9, (d, fd, out["kl_grad"][0, d])
    assert out["kl_grad"][0, 0] > 0 and out["kl_grad"][0, 1] < 0  # descent moves mu towards the reference


def test_surrogate_gradient_is_the_derivative_of_the_loss():
    """d/dmu of -ratio A grad_scale with ratio = exp(logprob - old): -A ratio grad_scale dlogprob/dmu, dlogprob/dmu_d = sgn(a_d - mu_d) / b_d,
    against a central difference of the float64 loss (piecewise linear exponent: no kink within the step by construction)."""
    mu, _, draw, adv = _inputs(rows=3, G=3)
    b, inv_b, log_norm = L.scales(L.SCALES[7], 7)
    a = draw["action32"]
    lp0 = L.logprob32(mu, a, inv_b, log_norm)
    old = (lp0 + np.float32(0.05) * np.where(adv > 0, 1, -1)).astype(np.float32)       # ratios e^-0.05 / e^0.05: inside the clip range
    out = L.pg_ref(mu, a, adv, L.SCALES[7], old_logprob=old, grad_scale=0.125)

    def loss(m):
        lp = (-np.abs(a.astype(np.float64) - m[:, None, :]) / b[None, None, :] - log_norm.astype(np.float64)[None, None, :]).sum(-1)
        return float((-np.exp(lp - old) * adv * 0.125).sum())

    hstep = 2.0 ** -14
    assert float(np.abs(a - mu[:, None, :]).min()) > 4 * hstep
    for r in range(3):
        for d in range(7):
            e = np.zeros(mu.shape)
            e[r, d] = hstep
            fd = (loss(mu.astype(np.float64) + e) - loss(mu.astype(np.float64) - e)) / (2 * hstep)
            got = float(out["surrogate"][r, d])
            assert abs(fd - got) <= 1e-4 * max(1.0, abs(got)), (r, d, fd, got)


def test_reference_catches_the_planted_mutants():
    mu, keys, draw, adv = _inputs()
    scale = L.SCALES[7]
    b, inv_b, log_norm = L.scales(scale, 7)
    # stream word 3 instead of 4;  d counted per Philox call instead of d >> 2 / d & 3
    for kw in (dict(stream=3), dict(per_call=True)):
        m = L.sample_ref(mu, scale, 4, seed=SEED, call=CALL, row_keys=keys, **kw)
        far = np.abs(m["action"] - draw["action"]) > draw["action_bound"] + m["action_bound"]
        assert far[:, :, 1:].mean() > 0.99, (kw, far.mean())      # (dimension 0 is word 0 of counter 0 in both orders: the others tell)
    per_call = L.sample_ref(mu, scale, 4, seed=SEED, call=CALL, row_keys=keys, per_call=True)
    assert np.array_equal(per_call["e"][:, :, 0], draw["e"][:, :, 0])
    # the log-probability taken from e instead of the stored a: other bits wherever the rounding of mu + b e shows
    # (the kernel tests compare every draw's bits, so a mutant is caught as soon as ONE draw differs: a tenth of 4096 draws is far beyond that)
    mu_l, _, draw_l, _ = _inputs(rows=64, G=64)
    stored = L.logprob32(mu_l, draw_l["action32"], inv_b, log_norm)
    assert (stored != draw_l["logprob_from_e"]).mean() > 0.1
    # the KL gradient's sign flipped
    ref = (mu + np.float32(0.25) * np.where(np.arange(7) % 2 == 0, 1, -1).astype(np.float32)).astype(np.float32)
    zero = np.zeros_like(adv)
    good = L.pg_ref(mu, draw["action32"], zero, scale, ref_pred=ref, kl_coef=0.5, kl_scale=0.25)
    bad = L.pg_ref(mu, draw["action32"], zero, scale, ref_pred=ref, kl_coef=0.5, kl_scale=0.25, kl_sign=-1.0)
    assert bool(np.all(good["dpred_hi"] < bad["dpred_lo"]) or np.all((good["dpred_hi"] < bad["dpred_lo"]) | (bad["dpred_hi"] < good["dpred_lo"])))
    assert bool(np.all(np.sign(good["dpred64"]) == np.sign(mu - ref)))
    # a gated sample multiplied through instead of skipped: a padding draw full of NaN poisons the row
    a = draw["action32"].copy()
    a[:, 1, :] = np.nan
    adv2 = adv.astype(np.float32).copy()
    adv2[:, 1] = 0.0
    old = L.logprob32(mu, a, inv_b, log_norm)                     # NaN for the padding draw, as its ratio then is
    assert bool(np.all(np.isnan(old[:, 1]))) and bool(np.all(np.isfinite(old[:, [0, 2, 3]])))
    good = L.pg_ref(mu, a, adv2, scale, old_logprob=old, grad_scale=0.25)
    bad = L.pg_ref(mu, a, adv2, scale, old_logprob=old, grad_scale=0.25, multiply_through=True)
    assert bool(np.all(np.isfinite(good["surrogate"]))) and bool(np.all(good["surrogate"] != 0)) and bool(np.all(np.isnan(bad["surrogate"])))
    # ... and the duplicated-draw identity the kernel tests lean on holds in the reference: x + x and the halved scale are exact
    one = L.pg_ref(mu, draw["action32"][:, :1], adv[:, :1], scale, grad_scale=0.25)
    two = L.pg_ref(mu, np.repeat(draw["action32"][:, :1], 2, axis=1), np.repeat(adv[:, :1], 2, axis=1), scale, grad_scale=0.125)
    assert np.array_equal(one["dpred_bits"], two["dpred_bits"])


def test_clip_margin_is_asserted():
    mu, _, draw, adv = _inputs(rows=2, G=2)
    b, inv_b, log_norm = L.scales(L.SCALES[7], 7)
    lp = L.logprob32(mu, draw["action32"], inv_b, log_norm)
    old = (lp - np.float32(math.log(1.2))).astype(np.float32)                        # ratio = 1.2 to fp32 accuracy
    with pytest.raises(AssertionError, match="CLIP_MARGIN"):
        L.pg_ref(mu, draw["action32"], np.abs(adv), L.SCALES[7], old_logprob=old)


# ---- the kernels' refusals: OVLA_EINVAL before any launch, so they can be called without a device ------------------------------------------------
FAKE = 0x1000             # a non-null address nothing dereferences: every case below is refused on the host


def _struct(lib, name, **over):
    g = lib.STRUCTS[name]()
    ptrs = dict(ovla_laplace_sample_args=("pred", "action", "logprob"), ovla_laplace_pg_args=("pred", "actions", "advantage", "logprob", "ratio", "clipped"))[name]
    for p in ptrs:
        setattr(g, p, FAKE)
    g.rows, g.adim, g.G = 3, 7, 2
    for d in range(16):
        g.scale[d], g.log_norm[d] = 0.5, 0.0
    if name == "ovla_laplace_pg_args":
        g.clip_lo, g.clip_hi, g.grad_scale = 0.8, 1.2, 1.0
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(g, k)[v[0]] = v[1]
        else:
            setattr(g, k, v)
    return g


COMMON = [(dict(pred=0), "null pointer"), (dict(logprob=0), "null pointer"), (dict(rows=0), "rows=0"), (dict(rows=-2), "rows=-2"), (dict(adim=0), "adim=0"),
          (dict(adim=17), "adim=17"), (dict(G=0), "G = 0"), (dict(G=65), "G = 65"), (dict(scale=(0, 0.0)), "scale"), (dict(scale=(6, -1.0)), "scale"),
          (dict(scale=(3, float("inf"))), "scale"), (dict(scale=(2, float("nan"))), "scale")]


@pytest.mark.parametrize("over, phrase", COMMON + [(dict(action=0), "null pointer")])
def test_laplace_sample_refusals(over, phrase):
    load_pkg()
    lib = importlib.import_module("openvla-oft_amd._lib")
    with pytest.raises(lib.OvlaError, match="ovla_laplace_sample: .*" + phrase):
        lib.call("ovla_laplace_sample", _struct(lib, "ovla_laplace_sample_args", **over), 0)


@pytest.mark.parametrize("over, phrase", COMMON + [(dict(actions=0), "null pointer"), (dict(advantage=0), "null pointer"), (dict(ratio=0), "null pointer"),
                                                   (dict(clipped=0), "null pointer"), (dict(clip_lo=1.3), "clip_lo"), (dict(clip_hi=float("nan")), "clip_lo"),
                                                   (dict(clip_lo=float("nan")), "clip_lo"), (dict(kl_coef=-0.5), "kl_coef"), (dict(kl_coef=float("nan")), "kl_coef"),
                                                   (dict(ref_pred=FAKE), "come together"), (dict(kl=FAKE), "come together")])
def test_laplace_pg_refusals(over, phrase):
    load_pkg()
    lib = importlib.import_module("openvla-oft_amd._lib")
    with pytest.raises(lib.OvlaError, match="ovla_laplace_pg: .*" + phrase):
        lib.call("ovla_laplace_pg", _struct(lib, "ovla_laplace_pg_args", **over), 0)


def test_scales_binding():
    load_pkg()
    ops = importlib.import_module("openvla-oft_amd.ops")
    b, ln = ops.laplace_scales(0.3, 7)
    rb, _, rln = L.scales(0.3, 7)
    assert b.dtype == np.float32 and np.array_equal(b, rb) and np.array_equal(ln, rln)
    b, ln = ops.laplace_scales(torch.tensor(L.SCALES[7]), 7)
    rb, _, rln = L.scales(L.SCALES[7], 7)
    assert np.array_equal(b, rb) and np.array_equal(ln, rln) and ln[0] == np.float32(math.log(2.0))
    with pytest.raises(ValueError, match="scale"):
        ops.laplace_scales([0.1, 0.2], 7)
