"""The GEMM checks of tests/gemm_reference.py discriminate (no GPU).

`emulate` restates a tiled GEMM in fp32 on the CPU -- tiles of BM x BN, K walked in tiles of BK, optionally cut into slabs that are summed in
slab order, the epilogue with the documented bf16 rounding points -- and takes one deliberate bug at a time (`MUTATIONS`).  The correct
emulation passes `assert_exact` against the float64 reference at every tile shape and split; every mutation is rejected by it.

What the earlier check would have said: `old_close` is the `close()` of tests/test_kernels_gpu.py (max|err| <= 1.5e-2 max|ref| and
mean|err| <= 2.5e-3 max|ref|), applied to the same mutations with `randn` operands at K = 4096 (operand scales 0.5 / 0.1, bias and residual
randn, as those tests draw them; max|ref| is 15.75 here).  test_old_check_accepts_what_the_exact_check_rejects pins this table:

    truncate         truncation instead of round-to-nearest-even          ACCEPTED  (max 4.0e-3, mean 3.8e-4 of max|ref|)
    double_round     an extra bf16 rounding ahead of the residual add     ACCEPTED  (max 7.9e-3, mean 2.3e-4)
    k_dropped        one k index dropped in one tile                      ON THE EDGE: the mean bound is blind (3.3e-4, an eighth of it); the max
    k_doubled        one k index doubled at a split boundary              bound is decided by the largest single product among the tile's 8192,
                                                                          1.6e-2 ... 2.8e-2 of max|ref| depending on WHICH k (2.1e-2 / 1.8e-2 for
                                                                          the ones planted here): it passes or fails by the draw, and passes the
                                                                          batch-invariance bound 2e-2 max|ref| + 2e-2 for half of the indices
    row_edge         tile edge shifted by one row                         rejected  (a whole tile row of unrelated values)
    col_edge         tile edge shifted by one column                      rejected
    k2_group         K-extension column group off by one group           rejected  (the K-extension operands are drawn at scale 1 / 0.2)
    bias_shift       bias shifted by one column                           rejected with a randn bias of scale 1; `close` accepts it as soon as
                                                                          neighbouring bias entries are alike
    rope_pos         RoPE position off by one                             rejected with independent table rows (real tables differ between
    rope_row         row itself instead of row % rope_S                   neighbouring positions in their first few columns only)

`double_round`: between colscale and the residual add the value is already bf16 (a documented rounding point), so a second rounding THERE is
the identity.  The extra rounding that can go wrong upstream of the residual add is of the raw accumulator, before alpha and bias are applied
(what a split-K reduce that stores bf16 slabs would do); that is the mutation.
"""
import pytest
import torch

from tests import gemm_reference as R

BF = torch.bfloat16
MUTATIONS = ["k_dropped", "k_doubled", "row_edge", "col_edge", "k2_group", "bias_shift", "rope_pos", "rope_row", "truncate", "double_round"]
OLD_CHECK_ACCEPTS = {"truncate", "double_round"}
OLD_CHECK_EDGE = {"k_dropped", "k_doubled"}      # decided by one product's tail: see the docstring


def _r(x):          # fp32 -> bf16 -> fp32, round to nearest even
    return x.to(BF).float()


def _t(x):          # fp32 -> bf16 by truncation
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(a, b, *, BM, BN, BK=64, splits=1, a2=None, b2=None, k2_group_n=0, alpha=1.0, bias=None, residual=None, rope=None, mut=None):
    """fp32 tiled GEMM with the documented rounding points; `mut` plants one bug (in tile (1, 1) where it is per tile)."""
    M, K = a.shape
    N = b.shape[0]
    af, bf_ = a.float(), b.float()
    out = torch.zeros((M, N), dtype=torch.float32)
    T = -(-K // BK)
    per = -(-T // splits)
    rnd_store = _t if mut == "truncate" else _r
    for ti, m0 in enumerate(range(0, M, BM)):
        for tj, n0 in enumerate(range(0, N, BN)):
            rows, cols = torch.arange(m0, min(m0 + BM, M)), torch.arange(n0, min(n0 + BN, N))
            hit = (ti, tj) == (1, 1)
            arows = rows - 1 if (mut == "row_edge" and ti == 1) else rows
            brows = cols - 1 if (mut == "col_edge" and tj == 1) else cols
            acc = torch.zeros((len(rows), len(cols)), dtype=torch.float32)
            for s in range(splits):                                            # slabs in slab order
                k0, k1 = s * per * BK, min((s + 1) * per * BK, K)
                if k0 >= k1:
                    continue
                ks = torch.arange(k0, k1)
                if mut == "k_doubled" and hit and s == splits - 1:
                    ks = torch.arange(k0 - 1, k1)                              # the boundary index belongs to both slabs
                if mut == "k_dropped" and hit and s == 0:
                    ks = ks[ks != k0 + 5]
                acc = acc + af[arows][:, ks] @ bf_[brows][:, ks].T
            if a2 is not None:
                K2 = b2.shape[1]
                G = a2.shape[1] // K2
                g = n0 // k2_group_n if k2_group_n else 0
                if mut == "k2_group":
                    g = (g + 1) % G
                acc = acc + a2.float()[rows][:, g * K2:(g + 1) * K2] @ b2.float()[cols].T
            if mut == "double_round":
                acc = _r(acc)
            v = acc * alpha
            if rope is not None:
                cos, sin, S, rcols = rope
                y = _r(v)
                pos = rows % S
                if mut == "rope_pos":
                    pos = (rows + 1) % S
                if mut == "rope_row":
                    pos = rows
                c, s_ = cos.float()[pos], sin.float()[pos]
                o = y.clone()
                for h0 in range(0, len(cols), 128):
                    if n0 + h0 >= rcols:
                        break
                    lo, hi = y[:, h0:h0 + 64], y[:, h0 + 64:h0 + 128]
                    o[:, h0:h0 + 64] = _r(lo * c) + _r(-hi * s_)
                    o[:, h0 + 64:h0 + 128] = _r(hi * c) + _r(lo * s_)
                out[m0:m0 + BM, n0:n0 + BN] = rnd_store(o)
                continue
            if bias is not None:
                bcols = (cols + 1) % N if mut == "bias_shift" else cols
                v = v + bias.float()[bcols][None, :]
            v = _r(v)
            if residual is not None:
                v = v + residual.float()[rows][:, cols]
            out[m0:m0 + BM, n0:n0 + BN] = rnd_store(v)
    return out.to(BF)


def exact_problem(seed, M, N, K, *, K2=0, G=1, rope_S=0):
    g = R.rng(seed)
    p = dict(a=R.operand(g, M, K), b=R.operand(g, N, K), alpha=0.5, bias=R.bias_like(g, N), residual=R.bias_like(g, M, N))
    if K2:
        p.update(a2=R.operand(g, M, G * K2), b2=R.operand(g, N, K2), k2_group_n=N // G if G > 1 else 0)
    if rope_S:
        cos, sin = R.rope_tables(g, M)          # M rows: the `rope_row` mutation indexes by the row itself
        p = dict(a=p["a"], b=p["b"], rope=(cos, sin, rope_S, 256), **{k: p[k] for k in ("a2", "b2", "k2_group_n") if k in p})
    return p


def randn_problem(seed, M, N, K, *, K2=0, G=1, rope_S=0):
    """What the tolerance tests draw: randn operands of scale 0.5 / 0.1, K-extension of scale 1 / 0.2, randn bias and residual."""
    torch.manual_seed(seed)
    rn = lambda *s, scale=1.0: (torch.randn(*s) * scale).to(BF)
    p = dict(a=rn(M, K, scale=0.5), b=rn(N, K, scale=0.1), bias=rn(N), residual=rn(M, N))
    if K2:
        p.update(a2=rn(M, G * K2), b2=rn(N, K2, scale=0.2), k2_group_n=N // G if G > 1 else 0)
    if rope_S:
        cos, sin = rn(M, 64), rn(M, 64)
        p = dict(a=p["a"], b=p["b"], rope=(cos, sin, rope_S, 256), **{k: p[k] for k in ("a2", "b2", "k2_group_n") if k in p})
    return p


def old_close(out, ref, tol=1.5e-2, mean_tol=2.5e-3):
    out, ref = out.float(), ref.float()
    scale = ref.abs().max().item() + 1e-12
    err = (out - ref).abs()
    return bool(torch.isfinite(out).all()) and err.max().item() / scale <= tol and err.mean().item() / scale <= mean_tol


def problem_for(mut, make, K):
    """The problem a mutation shows on: 2 x 2 tiles of 64 x 128 plus ragged edges, so tile (1, 1) is interior; RoPE on two heads of 128."""
    M, N = 2 * 64 + 37, 2 * 128 + 24 if not mut.startswith("rope") else 384
    kw = dict(K2=32, G=3 if mut == "k2_group" else 1) if mut in ("k2_group",) else {}
    if mut == "k2_group":
        N = 384
    if mut.startswith("rope"):
        kw["rope_S"] = 77
    return make(7, M, N, K, **kw)


# ---- the correct emulation passes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("BM,BN,BK,splits", [(64, 128, 64, 1), (128, 128, 64, 3), (256, 256, 64, 2), (128, 256, 32, 1), (128, 32, 64, 8), (32, 32, 32, 1)])
def test_emulation_passes_every_check(BM, BN, BK, splits):
    M, N, K = 2 * 64 + 37, 2 * 128 + 24, 520
    p = exact_problem(1, M, N, K)
    ref = R.reference(**p)
    R.assert_exact(emulate(BM=BM, BN=BN, BK=BK, splits=splits, **p), ref.out, "bias + residual", tile=(BM, BN))
    p = exact_problem(2, M, 384, K, K2=32, G=3)
    R.assert_exact(emulate(BM=BM, BN=128 if BN > 128 else BN, BK=BK, splits=splits, **p), R.reference(**p).out, "grouped K-extension")
    if BN % 128 == 0:
        p = exact_problem(3, M, 384, K, rope_S=77)
        R.assert_exact(emulate(BM=BM, BN=BN, BK=BK, splits=splits, **p), R.reference(**p).out, "rope")


def test_slab_order_does_not_matter_with_exact_operands():
    p = exact_problem(4, 165, 280, 520)
    outs = [emulate(BM=64, BN=128, splits=s, **p) for s in (1, 2, 3, 5, 8)]
    assert all(torch.equal(o, outs[0]) for o in outs)


# ---- every mutation is rejected ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", MUTATIONS)
def test_assert_exact_rejects(mut):
    p = problem_for(mut, exact_problem, 520)
    ref = R.reference(**p).out
    R.assert_exact(emulate(BM=64, BN=128, splits=3, **p), ref, "unmutated")
    got = emulate(BM=64, BN=128, splits=3, mut=mut, **p)
    with pytest.raises(AssertionError, match="elements differ") as e:
        R.assert_exact(got, ref, mut, tile=(64, 128))
    msg = str(e.value)
    assert "tile row" in msg and "in-tile offset" in msg
    if mut in ("k_dropped", "k_doubled"):      # one tile is wrong, and the report says which
        assert "first at (64, 128) = tile row 1, tile column 1, in-tile offset (0, 0)" in msg, msg


@pytest.mark.parametrize("mut", MUTATIONS)
def test_old_check_accepts_what_the_exact_check_rejects(mut):
    """randn operands at K = 4096 under the old `close()`: the docstring's table."""
    p = problem_for(mut, randn_problem, 4096)
    ref = R.reference(exact=False, **p).out
    assert old_close(emulate(BM=64, BN=128, splits=3, **p), ref), "the correct emulation passes the old check"
    got = emulate(BM=64, BN=128, splits=3, mut=mut, **p)
    assert not torch.equal(got, ref)
    if mut in OLD_CHECK_EDGE:
        scale = ref.float().abs().max().item()
        err = (got.float() - ref.float()).abs()
        assert err.mean().item() / scale <= 2.5e-3 / 5, "the mean bound does not see one wrong tile"
        assert 0.5 * 1.5e-2 <= err.max().item() / scale <= 2 * 1.5e-2, "the max bound is decided by the tail of one product"
        return
    assert old_close(got, ref) == (mut in OLD_CHECK_ACCEPTS), f"{mut}: old check {'accepts' if old_close(got, ref) else 'rejects'}"


# ---- the fold's single row factor -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", R.FOLD_ALPHAS)
@pytest.mark.parametrize("tile,BM,BN", [(1, 128, 128), (101, 128, 128), (22, 128, 256), (122, 128, 256)])
def test_fold_alpha_case_tells_the_two_multiplication_orders_apart(tile, BM, BN, alpha):
    """The inputs test_rmsnorm_fold feeds its alpha != 2^k consumer case: with the CPU's fp32 rstd at least 8 elements of the interior tile and
    8 of the edge tiles round differently under (acc * rstd) * alpha than under acc * (alpha * rstd), so assert_exact rejects the old order in
    either region; and with rstd one ulp either side (the GPU's rsqrt) both regions still tell them apart."""
    a, b, parts, eps = R.fold_alpha_case(tile, BM, BN, alpha)
    assert parts.shape == (BM + 37, 8) and float(parts.min()) >= 100 and float(parts.max()) <= 3000
    acc, r = R.accumulate(a, b)[0], R.rstd32(parts, eps)
    want, other = R.fold_orders(acc, r, alpha)
    inner, edge = R.fold_told_apart(want, other, BM, BN)
    assert inner >= 8 and edge >= 8, (inner, edge)
    for region in (want[:BM, :BN], want[BM:], want[:, BN:]):
        assert region.float().abs().max() > 0
    with pytest.raises(AssertionError, match="elements differ"):
        R.assert_exact(other[:BM, :BN], want[:BM, :BN], "interior tile, the other order", tile=(BM, BN))
    with pytest.raises(AssertionError, match="elements differ"):
        R.assert_exact(torch.cat([other[BM:].flatten(), other[:BM, BN:].flatten()])[None], torch.cat([want[BM:].flatten(), want[:BM, BN:].flatten()])[None], "edge tiles, the other order")
    for rr in (torch.nextafter(r, torch.zeros(())), torch.nextafter(r, torch.ones(()))):
        inner, edge = R.fold_told_apart(*R.fold_orders(acc, rr, alpha), BM, BN)
        assert inner >= 1 and edge >= 1, (inner, edge)
    ref = R.reference(a, b, rowscale=(parts, eps), alpha=alpha, exact=True)          # and the float64 reference agrees within its 1 ulp
    R.assert_ulps(want, ref.out64, R.ULPS["rowscale"], what="fold_orders against the float64 reference")


# ---- the helpers themselves ---------------------------------------------------------------------------------------------------------------------
def test_rbf_is_round_to_nearest_even_and_ulp_is_a_bf16_ulp():
    torch.manual_seed(0)
    x = torch.cat([torch.randn(20000) * 100, torch.tensor([1.00390625, 1.01171875, 257.0, 259.0, -3.0, 0.5, 2.0 ** -20])])   # incl. exact ties
    assert torch.equal(R.rbf(x.double()).float(), x.to(BF).float())
    assert torch.equal(R.tbf(x.double()).float(), _t(x))
    one = torch.tensor([1.0, 1.99, 2.0, 255.0, 256.0, -0.75], dtype=torch.float64)
    assert R.ulp_bf16(one).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0, 2.0 ** -8]


def test_reference_refuses_operands_outside_the_exact_regime():
    g = R.rng(5)
    a, b = R.operand(g, 16, 64), R.operand(g, 16, 64)
    with pytest.raises(AssertionError, match="exact regime"):
        R.reference(a * 2, b)
    with pytest.raises(AssertionError, match="exact regime"):
        R.reference(a, b, alpha=1.0 / 3.0)
    with pytest.raises(AssertionError, match="256"):
        R.reference(torch.full((8, 64), 3.0).to(BF), torch.full((64, 64), 3.0).to(BF), rowsq=True)
    r = R.reference(a, b.repeat(4, 1), rowsq=True)
    assert r.rowsq.shape == (16, 1) and torch.equal(r.rowsq[:, 0].double(), r.out.double().pow(2).sum(-1))


def test_generators_give_what_they_promise():
    g = R.rng(6)
    a = R.operand(g, 300, 520)
    assert a.dtype == BF and int(a.abs().min()) == 1 and int(a.abs().max()) == 3 and set(a.unique().tolist()) == {-3, -2, -1, 1, 2, 3}
    cos, sin = R.rope_tables(g, 77)
    assert set(cos.unique().tolist()) == {0, 0.5, -0.5, 1, -1} and not torch.equal(cos[0], cos[1]) and not torch.equal(cos[:, 0], cos[:, 1])
    gam, beta = R.film_like(g, 3, 64)
    assert set(gam.unique().tolist()) <= {-0.5, 0, 1, 3} and torch.equal(beta.float(), beta.float().round())
    assert torch.equal(R.operand(R.rng(9), 8, 8), R.operand(R.rng(9), 8, 8))


@pytest.mark.parametrize("align", [8, 4])
def test_embed_keeps_the_alignment_rules_and_sees_a_touched_guard(align):
    t = R.operand(R.rng(7), 37, 72 if align == 8 else 44)
    for fill in R.GUARD_FILLS + ("sentinel",):
        e = R.embed(t, align=align, fill=fill)
        assert torch.equal(e.view, t) and e.view.stride(0) % align == 0 and e.view.stride(0) > t.shape[1] and e.view.data_ptr() % (2 * align) == 0
        assert e.r0 > 0 and e.c0 > 0 and e.buf.shape[0] > e.r0 + 37
    nan = R.embed(t, align=align, fill="nan")
    assert torch.isnan(nan.buf.float()).sum() == nan.buf.numel() - t.numel()
    big = R.embed(t, align=align, fill="big").buf.float()
    assert big.max() > 2.9e38 and big.min() < -2.9e38 and torch.isfinite(big).all()
    e = R.embed(BF, shape=(37, 44), align=align, fill="sentinel", device="cpu")
    e.view.zero_()
    e.assert_guards("untouched")
    for r, c in [(e.r0 - 1, e.c0), (e.r0 + 37, e.c0 + 3), (e.r0 + 5, e.c0 - 1), (e.r0 + 5, e.c0 + 44)]:    # above, below, left, right (columns >= N up to ld)
        f = R.embed(BF, shape=(37, 44), align=align, fill="sentinel", device="cpu")
        f.buf[r, c] = 0.0
        with pytest.raises(AssertionError, match="guard elements overwritten"):
            f.assert_guards("touched")
    f32 = R.embed(torch.float32, shape=(5, 8), align=4, fill="sentinel", device="cpu")
    f32.assert_guards("fp32")
    f32.buf[0, 0] = 1.0
    with pytest.raises(AssertionError):
        f32.assert_guards("fp32 touched")


def test_assert_ulps_bounds():
    ref = torch.tensor([[1.0, 300.0, -0.0371, 5.0]], dtype=torch.float64)
    ulp = R.ulp_bf16(ref)
    assert R.assert_ulps((ref + 0.49 * ulp).float(), ref, 1) < 0.5
    R.assert_ulps(R.rbf(ref + 0.99 * ulp).to(BF), ref, 1.5)
    with pytest.raises(AssertionError, match="beyond 1 ulp"):
        R.assert_ulps((ref + 1.5 * ulp).float(), ref, 1)
    with pytest.raises(AssertionError, match="beyond 2 ulp"):
        R.assert_ulps((ref - 2.5 * ulp).float(), ref, 2)
    R.assert_ulps((ref + 1.5 * ulp).float(), ref, 1, abs_floor=0.6 * ulp)
    with pytest.raises(AssertionError, match="non-finite"):
        R.assert_ulps(torch.tensor([[float("nan"), 0, 0, 0]]), ref, 1)
    # a correctly rounded activation is within 1/2 ulp of the float64 value; one whose fp32 evaluation crossed a rounding boundary within 1
    z = torch.linspace(-6, 6, 4001, dtype=torch.float64)[None]
    for act in (R.ACT_GELU, R.ACT_SILU, R.ACT_GELU_TANH):
        assert R.assert_ulps(R.rbf(R.act64(z, act)).to(BF), R.act64(z, act), 1) <= 0.5
