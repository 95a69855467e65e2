"""The numpy twins of csrc/value_gae.hip (tests/value_gae_reference.py) against what they claim to be: GAE against its textbook definition in
float64 (bit for bit on dyadic data, where every intermediate is exact in fp32; within a bound derived from the operation count elsewhere), its
limits, four planted mistakes that must not survive, the value loss against central differences, and the normalisation's moments.  No GPU."""
import numpy as np
import pytest

from tests import value_gae_reference as V

F32, F64 = np.float32, np.float64


def _dones(rng, N, T, p=0.25):
    d = (rng.random((N, T)) < p).astype(np.uint8)
    if T >= 3:
        d[0, 0] = 1                       # at t = 0
        d[0, T - 1] = 1                   # at T - 1
        d[-1, 1:3] = 1                    # on consecutive steps
    return d


def _lengths(rng, N, T):
    ln = rng.integers(0, T + 1, size=N).astype(np.int32)
    ln[0] = T
    if N > 1:
        ln[1] = 0
    if N > 2:
        ln[2] = 1
    return ln


def _exact_case(kind, seed, N=6, T=8):
    rng = np.random.default_rng(seed)
    if kind == "integers":                # gamma = lambda = 1, integer rewards and values: every sum an integer below 2^24
        r, v, bs = rng.integers(-9, 10, (N, T)), rng.integers(-9, 10, (N, T)), rng.integers(-9, 10, N)
        gamma, lam, gl = 1.0, 1.0, 1.0
    else:                                 # gamma = 0.5, gamma lambda = 0.25, quarter-integers, T <= 8: at most 2 + 2 * 8 fractional bits
        r, v, bs = rng.integers(-12, 13, (N, T)) / 4.0, rng.integers(-12, 13, (N, T)) / 4.0, rng.integers(-12, 13, N) / 4.0
        gamma, lam, gl = 0.5, 0.5, 0.25
    return r.astype(F32), v.astype(F32), bs.astype(F32), _dones(rng, N, T), _lengths(rng, N, T), gamma, lam, gl


@pytest.mark.parametrize("kind", ["integers", "quarters"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gae_twin_is_exact_on_dyadic_data(kind, seed):
    r, v, bs, d, ln, gamma, lam, gl = _exact_case(kind, seed)
    assert float(V.gamma_lambda32(gamma, lam)) == gl
    adv, ret = V.gae_ref(r, v, bs, d, ln, gamma, lam)
    adv64, ret64 = V.gae_definition64(r, v, bs, d, ln, gamma, lam)
    assert adv.dtype == F32 and ret.dtype == F32
    assert np.array_equal(adv.astype(F64).view(np.int64), adv64.view(np.int64)), "adv: the fp32 recursion is not the float64 definition bit for bit"
    assert np.array_equal(ret.astype(F64).view(np.int64), ret64.view(np.int64)), "ret: the fp32 recursion is not the float64 definition bit for bit"
    assert np.any(adv64 != 0)


@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.9, 0.0), (1.0, 0.97), (0.0, 0.5)])
def test_gae_twin_within_the_derived_bound_on_general_data(gamma, lam):
    rng = np.random.default_rng(7)
    N, T = 9, 33
    r, v, bs = rng.standard_normal((N, T)).astype(F32), (3 * rng.standard_normal((N, T))).astype(F32), rng.standard_normal(N).astype(F32)
    d, ln = _dones(rng, N, T, 0.1), _lengths(rng, N, T)
    adv, ret = V.gae_ref(r, v, bs, d, ln, gamma, lam)
    adv64, ret64 = V.gae_definition64(r, v, bs, d, ln, gamma, lam)
    bound = V.gae_bound(r, v, bs, d, ln, gamma, lam)
    err = np.abs(adv.astype(F64) - adv64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"gamma {gamma} lam {lam}: max adv error / bound = {worst:.3f}")
    assert np.all(err <= bound)
    assert np.all(np.abs(ret.astype(F64) - ret64) <= bound + 2.0 ** -24 * np.abs(ret64) * 1.01)
    mask = V._valid_mask(N, T, ln)
    assert np.all(adv[~mask].view(np.int32) == 0) and np.all(ret[~mask].view(np.int32) == 0), "beyond the length: +0"


def test_gae_limits():
    rng = np.random.default_rng(3)
    N, T = 5, 9
    r, v, bs = rng.integers(-5, 6, (N, T)).astype(F32), rng.integers(-5, 6, (N, T)).astype(F32), rng.integers(-5, 6, N).astype(F32)
    d, ln = _dones(rng, N, T), _lengths(rng, N, T)
    # lambda = 0: the advantage is the one-step TD error
    adv, _ = V.gae_ref(r, v, bs, d, ln, 0.5, 0.0)
    for n in range(N):
        for t in range(ln[n]):
            vnext = bs[n] if t == ln[n] - 1 else v[n, t + 1]
            delta = F32(F32(r[n, t] + F32(F32(F32(0.5) * vnext) * F32(0.0 if d[n, t] else 1.0))) - v[n, t])
            assert adv[n, t].view(np.int32) == delta.view(np.int32)
    # gamma = lambda = 1 on integers: ret is the reward-to-go of the step's own episode plus the bootstrap if the buffer ends before the episode
    _, ret = V.gae_ref(r, v, bs, d, ln, 1.0, 1.0)
    for n in range(N):
        for t in range(ln[n]):
            togo, s = 0.0, t
            while True:
                togo += float(r[n, s])
                if d[n, s]:
                    break
                if s == ln[n] - 1:
                    togo += float(bs[n])
                    break
                s += 1
            assert float(ret[n, t]) == togo


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_gae_planted_mutants_are_killed(mutant):
    """Each planted mistake must change the result on the exact data (where the honest recursion equals the definition bit for bit)."""
    killed = False
    for kind in ("integers", "quarters"):
        for seed in (0, 1, 2):
            r, v, bs, d, ln, gamma, lam, _ = _exact_case(kind, seed)
            v = v.copy()
            v[~V._valid_mask(*v.shape, ln)] = 100.0          # what lies beyond the length must never matter
            adv64, ret64 = V.gae_definition64(r, v, bs, d, ln, gamma, lam)
            adv, ret = V.gae_ref(r, v, bs, d, ln, gamma, lam)
            assert np.array_equal(adv.astype(F64), adv64) and np.array_equal(ret.astype(F64), ret64)
            adv_m, ret_m = V.gae_ref(r, v, bs, d, ln, gamma, lam, mutant=mutant)
            killed |= not (np.array_equal(adv_m.astype(F64), adv64) and np.array_equal(ret_m.astype(F64), ret64))
    assert killed, f"{mutant}: the comparison with the definition does not notice it"


def test_value_loss_gradient_central_difference_on_both_branches():
    h = 1e-6
    cases = [  # (v, R, old, clip, clipped?)
        (0.75, 2.0, 0.5, 0.125, True),      # v ran past old + clip towards R: the clipped value is further from R, clipped branch
        (0.75, -1.0, 0.5, 0.125, False),    # v ran away from R: the unclipped error is the larger
        (0.5625, 2.0, 0.5, 0.125, False),   # inside the clip range: lc == l, the unclipped branch
        (-3.0, -3.5, -1.0, 0.25, True),
        (1.25, 0.25, 0.0, 0.0, False),      # no clipping
    ]
    for v, R, old, clip, want_clipped in cases:
        loss, dl, clipped = V.value_terms(v, R, old, clip)
        assert clipped == want_clipped, (v, R, old, clip)
        num = (V.value_loss64(v + h, R, old, clip) - V.value_loss64(v - h, R, old, clip)) / (2 * h)
        # the loss is piecewise quadratic with |second derivative| <= 1: the central difference is exact up to float64 rounding of terms of
        # magnitude <= 16, 2 * 16 * 2^-53 / 2e-6 < 2e-9; the fp32 dl = v - R is exact for these dyadic inputs
        assert abs(float(dl) - num) <= 2e-9, (v, R, old, clip, float(dl), num)
        assert abs(float(loss) - V.value_loss64(v, R, old, clip)) == 0.0
        if clipped:
            assert dl.view(np.int32) == 0, "the clipped branch's gradient is exactly +0"


def test_value_clip_zero_is_the_unclipped_loss_and_equality_is_unclipped():
    rng = np.random.default_rng(5)
    B, chunk = 9, 8
    u = V.bf16_round(rng.standard_normal(B * chunk).astype(F32))
    R, old = rng.standard_normal(B).astype(F32), rng.standard_normal(B).astype(F32)
    a = V.value_loss_ref(u, chunk, R, old, None, 0.0, 0.25)
    b = V.value_loss_ref(u, chunk, R, None, None, 0.0, 0.25)
    huge = V.value_loss_ref(u, chunk, R, old, None, 1e30, 0.25)         # a clip range nothing leaves: lc == l everywhere
    for k in ("value", "du_bits", "stats", "loss", "dl"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        assert np.array_equal(a[k].view(np.uint8), huge[k].view(np.uint8)), k
    assert not huge["clipped"].any() and huge["stats"][1] == 0
    want = (F32(0.5) * ((a["value"] - R).astype(F32) ** 2).astype(F32)).astype(F32)
    assert np.array_equal(a["loss"].view(np.int32), want.view(np.int32))
    loss, dl, clipped = V.value_terms(0.5625, 2.0, 0.5, 0.125)          # lc == l exactly
    assert not clipped and float(dl) == 0.5625 - 2.0


def test_value_loss_statistics_and_padding():
    rng = np.random.default_rng(11)
    B, chunk = 9, 25
    u = V.bf16_round(rng.standard_normal(B * chunk).astype(F32)).reshape(B, chunk)
    R, old = rng.standard_normal(B).astype(F32), rng.standard_normal(B).astype(F32)
    valid = np.ones(B, dtype=np.int32)
    valid[[2, 8]] = 0
    ref = V.value_loss_ref(u[valid == 1], chunk, R[valid == 1], old[valid == 1], None, 0.2, 0.125)
    u2, R2, old2 = u.copy(), R.copy(), old.copy()
    u2[valid == 0], R2[valid == 0], old2[valid == 0] = np.nan, np.nan, np.nan
    got = V.value_loss_ref(u2, chunk, R2, old2, valid, 0.2, 0.125)
    assert np.array_equal(got["stats"].view(np.int32), ref["stats"].view(np.int32)), "padding leaked into the statistics"
    assert np.all(got["du_bits"].reshape(B, chunk)[valid == 0] == 0)
    assert np.array_equal(got["du_bits"].reshape(B, chunk)[valid == 1].reshape(-1), ref["du_bits"])
    assert got["stats"][0] == 7 and 0 < got["stats"][1] < 7, "the case must hold clipped and unclipped observations"
    s = got["stats"].astype(F64)
    v, r = ref["value"].astype(F64), R[valid == 1].astype(F64)
    ev = 1.0 - s[5] / (s[6] - s[4] ** 2 / s[0])
    assert abs(ev - (1.0 - np.sum((r - v) ** 2) / np.sum((r - r.mean()) ** 2))) <= 1e-5


@pytest.mark.parametrize("N,T", [(1, 1), (1, 63), (1, 64), (5, 13), (17, 241)])
def test_normalize_moments(N, T):
    rng = np.random.default_rng(N * 1000 + T)
    adv = (5.0 + 3.0 * rng.standard_normal((N, T))).astype(F32)
    ln = None if N == 1 else _lengths(rng, N, T)
    mask = V._valid_mask(N, T, ln)
    src = adv.copy()
    src[~mask] = np.nan
    out = V.normalize_ref(src, ln, 1e-8)
    assert np.array_equal(out[~mask].view(np.int32), src[~mask].view(np.int32)), "padding must keep its bits"
    x = out[mask].astype(F64)
    n = x.size
    if n == 1:
        assert out[mask].view(np.int32)[0] == 0, "one valid element gives exactly +0"
        return
    # each output is ((x - m) / (s + eps)) with three rounded fp32 operations and fp32 roundings of m and s: a relative error of at most 5 * 2^-24
    # of |x - m| / s plus 2 * 2^-24 |m| / s from the subtraction's operands; z below is the standardised magnitude, c = |mean| / std of the input
    src64 = src[mask].astype(F64)
    c = abs(src64.mean()) / src64.std()
    z = np.abs(src64 - src64.mean()) / src64.std()
    e = 2.0 ** -24 * (5 * z + 2 * c) * 1.01 + 1e-8 / src64.std() * z
    assert abs(x.mean()) <= e.mean(), (x.mean(), e.mean())
    assert abs(x.var() - 1.0) <= 2 * float((z * e).mean()) + float((e * e).mean()) + e.mean() ** 2, x.var()


def test_normalize_with_no_valid_element_writes_nothing():
    adv = np.full((3, 4), np.nan, dtype=F32)
    out = V.normalize_ref(adv, np.zeros(3, dtype=np.int32))
    assert np.array_equal(out.view(np.int32), adv.view(np.int32))
