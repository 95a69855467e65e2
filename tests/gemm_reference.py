"""Exact operands, a float64 reference and bit-level checks for the GEMM kernels (`csrc/gemm_nt.hip`, `gemm_tn.hip`).
Nothing here needs a GPU.

Why exact: bf16 x bf16 products of small integers are integers, and integers below 2^24 add exactly in fp32 in ANY order.  With the
operands of this module a correct kernel therefore matches a float64 reference bit for bit whatever its tile, split or reduction order,
and `assert_exact` (torch.equal on the bf16 bits) replaces a tolerance: one k index dropped or doubled in one tile, a bias read one
column off, a truncating store -- each changes bits.  `reference` asserts that every fp32 intermediate it forms is exactly representable
(`_exact32`), so an edit that leaves the exact regime fails here instead of silently turning the comparison into a tolerance test.

Epilogue order and rounding points are those of include/ovla.h ("Epilogue order") as the kernels implement them:

    z = bf16(alpha * acc + bias)            [C_pre = z]
    rowscale:  C = epilogue(acc * (alpha * rstd[m])): ONE fp32 factor ra = alpha * rstd[m], formed first and multiplied into the accumulator
               once, on every path a tile can take (z = bf16(ra * acc + bias); `fold_orders` below is that formula in fp32)
    v = bf16(act(z));  v = bf16(v * colscale[n]);  v = bf16(v + residual[m, n])
    FiLM:  [C_pre = v];  v = bf16(bf16(v * bf16(1 + gamma[m / film_rows, n])) + beta[...])
    RoPE (columns [0, rope_cols), head_dim 128, pos = m % rope_S, x = own column, y = partner column +-64, both bf16(acc)):
        low half   bf16(bf16(x cos) + bf16(-y sin))        high half   bf16(bf16(x cos) + bf16(y sin))
    rowsq_out[m, j] = sum of squares of the stored bf16 row's columns [64 j, 64 j + 64)   (fp32)
    OVLA_ACT_SWIGLU:  g | u = bf16(ra * acc) of B rows [0, F) | [F, 2F);  C = bf16(bf16(silu(g)) * u);  C_pre = [g | u]
    dact_mode 1:  C = bf16(bf16(alpha * acc) * act'(src))
    dact_mode 2:  d = bf16(alpha * acc), g | u = src[:, :N] | src[:, N:];  C[:, :N] = bf16(d * u * silu'(g)),  C[:, N:] = bf16(d * bf16(g * sigmoid(g)))

What cannot be exact (a transcendental, the fold's rsqrt) is checked by `assert_ulps` against the float64 value in units of the bf16 ulp of
the reference; the bounds are derived where they are used (`ULPS`).
"""
import functools
import math
from types import SimpleNamespace

import torch

BF = torch.bfloat16
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU, ACT_GELU_TANH, ACT_SWIGLU = 0, 1, 2, 3, 4, 5

# Derived bounds of assert_ulps, in bf16 ulps of the float64 reference.  A correctly rounded store is within 1/2 ulp.  An fp32 transcendental
# (relative error ~1e-7, four orders below the bf16 ulp 2^-8) can move a value across a rounding boundary, which costs the other 1/2: 1 ulp
# for one transcendental followed by one rounding.  Where that rounded value is multiplied and rounded again, the first ulp propagates
# (relative, so still 1 ulp of the product) and the second rounding adds its own 1/2 + 1/2: 2 ulps.
ULPS = {"silu": 1, "gelu_tanh": 1, "gelu": 1, "rowscale": 1, "dact1": 1, "swiglu": 2, "dact2": 2}
ERF_FLOOR = 2e-7          # * |z|: fast_erf's 1.5e-7 absolute bound (common.h) times the 0.5 |z| that multiplies it in GELU, rounded up


# ---- bf16 arithmetic in float64 ------------------------------------------------------------------------------------------------------------
def rbf(x):
    """float64 -> the nearest bf16 value (ties to even), as float64.  Done on the float64 itself: float64 -> float32 -> bf16 would round twice."""
    m, e = torch.frexp(x.double())
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def tbf(x):
    """float64 -> bf16 by truncation (the mutation `assert_exact` must reject)."""
    m, e = torch.frexp(x.double())
    return torch.ldexp(torch.trunc(m * 256.0) / 256.0, e)


def ulp_bf16(x):
    """One bf16 ulp at |x| (float64): 2^(floor(log2 |x|) - 7); the smallest normal's ulp at 0."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 8)


def _exact32(v, what):
    """The exact regime: `v` (float64, a value the kernel holds in fp32) must be representable in fp32 and below 2^24 in units of its own
    granularity -- then every order of fp32 additions that forms it is exact."""
    assert torch.equal(v.float().double(), v), f"{what}: left the exact regime (a value is not representable in fp32)"
    return v


# ---- operand generators --------------------------------------------------------------------------------------------------------------------
def rng(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, shape, lo, hi, nonzero=False, dtype=BF):
    """Integers in [lo, hi] from the seeded generator; `nonzero` redraws zeros as +-1 .. so that every k index changes every output."""
    x = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
        mag = torch.randint(1, max(abs(lo), abs(hi)) + 1, shape, generator=g)
        x = torch.where(x == 0, sign * mag, x)
    return x.to(dtype)


def operand(g, rows, cols):
    """A / B / A2 / B2: nonzero integers in [-3, 3]."""
    return ints(g, (rows, cols), -3, 3, nonzero=True)


def choice(g, shape, values, dtype=BF):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)].to(dtype)


ALPHAS = (1.0, 0.5, 2.0, 2.0 ** -4)


def bias_like(g, *shape):
    return ints(g, shape, -8, 8)


def colscale_like(g, n):
    return choice(g, (n,), (0.5, 1.0, 2.0))


def film_like(g, groups, n):
    return choice(g, (groups, n), (-0.5, 0.0, 1.0, 3.0)), ints(g, (groups, n), -8, 8)


def rope_tables(g, rows):
    """cos / sin [rows, 64] with entries from {0, +-0.5, +-1}, drawn independently per (position, column): a wrong position or a wrong
    half-head column index reads different values."""
    vals = (0.0, 0.5, -0.5, 1.0, -1.0)
    return choice(g, (rows, 64), vals), choice(g, (rows, 64), vals)


# ---- activations in float64 ----------------------------------------------------------------------------------------------------------------
def _sigmoid(z):
    return 1.0 / (1.0 + torch.exp(-z))


def act64(z, act):
    if act == ACT_GELU:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == ACT_RELU:
        return torch.clamp_min(z, 0.0)
    if act == ACT_SILU:
        return z * _sigmoid(z)
    if act == ACT_GELU_TANH:      # 0.5 z (1 + tanh u) = z sigmoid(2 u): the form that does not cancel for z << 0 (float64's 1 + tanh u is gone by z = -7)
        return z * _sigmoid(2.0 * 0.7978845608028654 * (z + 0.044715 * z ** 3))
    return z


def act_grad64(z, act):
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act == ACT_RELU:
        return (z > 0).double()
    if act == ACT_SILU:
        s = _sigmoid(z)
        return s * (1.0 + z * (1.0 - s))
    if act == ACT_GELU_TANH:
        k, c = 0.7978845608028654, 0.044715
        s = _sigmoid(2.0 * k * (z + c * z ** 3))      # 0.5 (1 + t) = s,  1 - t^2 = 4 s (1 - s)
        return s * (1.0 + 2.0 * z * (1.0 - s) * k * (1.0 + 3.0 * c * z * z))
    return torch.ones_like(z)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def accumulate(a, b, a2=None, b2=None, k2_group_n=0, a_group_n=0):
    """A . B^T (+ A2 . B2^T) in float64: block-diagonal mode (`a_group_n`) and the K-extension's column groups (`k2_group_n`) as ovla.h states them."""
    a, b = a.double(), b.double()
    N, K = b.shape
    if a_group_n:
        G = N // a_group_n
        assert a.shape[1] == G * K
        acc = torch.cat([a[:, g * K:(g + 1) * K] @ b[g * a_group_n:(g + 1) * a_group_n].T for g in range(G)], 1)
    else:
        acc = a @ b.T
    terms = a.shape[1] if not a_group_n else K
    if a2 is not None:
        a2, b2 = a2.double(), b2.double()
        K2 = b2.shape[1]
        if k2_group_n:
            for n0 in range(0, N, k2_group_n):
                c0 = (n0 // k2_group_n) * K2
                acc[:, n0:n0 + k2_group_n] += a2[:, c0:c0 + K2] @ b2[n0:n0 + k2_group_n].T
        else:
            acc = acc + a2[:, :K2] @ b2.T
        terms += K2
    return acc, terms


def reference(a, b, *, a2=None, b2=None, k2_group_n=0, a_group_n=0, alpha=1.0, bias=None, act=ACT_NONE, colscale=None, residual=None,
              film=None, rope=None, rowsq=False, rowscale=None, dact=None, exact=True):
    """float64 reference of ovla_gemm_bf16 (CPU tensors; bf16 operands).  Returns a namespace:
        out      bf16 [M, N] ([M, N / 2] for ACT_SWIGLU, [M, 2 N] for dact "swiglu")
        out64    float64: the value whose bf16 rounding is `out` (what assert_ulps compares with)
        c_pre    bf16 or None (the value ovla.h says C_pre receives for this epilogue)
        z64      float64 pre-activation (bf16-valued)
        rowsq    fp32 [M, N / 64] when `rowsq`;  rstd  float64 [M] when `rowscale` = (parts fp32 [M, K / 64], eps)
    `exact`: assert the exact regime on every intermediate that should be in it (off for the randn demonstrations of the self-test)."""
    chk = _exact32 if exact else (lambda v, what: v)
    acc, terms = accumulate(a, b, a2, b2, k2_group_n, a_group_n)
    if exact:
        assert float(max(a.abs().max(), b.abs().max())) <= 3 and 9 * terms < 2 ** 24, "operands outside the exact regime"
        assert torch.equal(acc, acc.round()), "accumulator is not an integer"
    M, N = acc.shape
    r = SimpleNamespace(c_pre=None, rowsq=None, rstd=None)
    v = acc * alpha
    if rowscale is not None:
        parts, eps = rowscale
        K = b.shape[1]
        assert parts.shape == (M, K // 64)
        r.rstd = 1.0 / torch.sqrt(parts.double().sum(-1) / K + eps)
        v = v * r.rstd[:, None]          # not exact: rsqrt
    else:
        chk(v, "alpha * acc")

    if rope is not None:
        cos, sin, S, cols = rope
        assert act == ACT_NONE and bias is None and residual is None and colscale is None and film is None and dact is None and cols % 128 == 0 and cols <= N
        y = rbf(v)
        out = y.clone()
        pos = torch.arange(M) % S
        c, s = cos.double()[pos], sin.double()[pos]                      # [M, 64]
        for h0 in range(0, cols, 128):
            lo, hi = y[:, h0:h0 + 64], y[:, h0 + 64:h0 + 128]
            out[:, h0:h0 + 64] = chk(rbf(lo * c) + rbf(-hi * s), "rope low half") if rowscale is None else rbf(lo * c) + rbf(-hi * s)
            out[:, h0 + 64:h0 + 128] = chk(rbf(hi * c) + rbf(lo * s), "rope high half") if rowscale is None else rbf(hi * c) + rbf(lo * s)
        r.z64 = y
        r.out64 = out
        r.out = rbf(out).to(BF)
        return r

    if act == ACT_SWIGLU:
        assert bias is None and residual is None and colscale is None and film is None and dact is None and N % 2 == 0
        gu = rbf(v)
        F = N // 2
        g_, u_ = gu[:, :F], gu[:, F:]
        r.c_pre = gu.to(BF)
        r.z64 = gu
        r.out64 = rbf(act64(g_, ACT_SILU)) * u_
        r.out = rbf(r.out64).to(BF)
        return r

    if dact is not None:
        assert bias is None and residual is None and colscale is None and film is None and act == ACT_NONE
        d = rbf(v)
        r.z64 = d
        if dact[0] == "swiglu":
            src = dact[1].double()
            g_, u_ = src[:, :N], src[:, N:]
            s = _sigmoid(g_)
            r.out64 = torch.cat([d * u_ * (s * (1.0 + g_ * (1.0 - s))), d * rbf(g_ * s)], 1)
        else:
            r.out64 = d * act_grad64(dact[1].double(), dact[2])
        r.out = rbf(r.out64).to(BF)
        return r

    if bias is not None:
        v = v + bias.double()[None, :]
        if rowscale is None:
            chk(v, "alpha * acc + bias")
    z = rbf(v)
    r.z64 = z
    if film is None:
        r.c_pre = z.to(BF)
    pre_round = v                       # the float64 value whose rounding is the running bf16 value
    v = z
    if act != ACT_NONE:
        pre_round = act64(v, act)
        if act == ACT_RELU:
            chk(pre_round, "relu")
        v = rbf(pre_round)
    if colscale is not None:
        pre_round = chk(v * colscale.double()[None, :], "colscale")
        v = rbf(pre_round)
    if residual is not None:
        pre_round = v + residual.double()
        if act in (ACT_NONE, ACT_RELU) and rowscale is None:
            chk(pre_round, "residual add")
        v = rbf(pre_round)
    if film is not None:
        gamma, beta, rows = film
        grp = torch.arange(M) // rows
        r.c_pre = v.to(BF)
        one_plus = rbf(1.0 + gamma.double())[grp]
        pre_round = rbf(chk(v * one_plus, "film scale")) + beta.double()[grp]
        chk(pre_round, "film shift")
        v = rbf(pre_round)
    r.out64 = pre_round
    r.out = v.to(BF)
    if rowsq:
        assert N % 64 == 0
        if exact:
            assert float(v.abs().max()) <= 256, "rowsq_out: |out| must stay <= 256 for exact fp32 sums of squares"
        r.rowsq = chk(v.view(M, N // 64, 64).pow(2).sum(-1), "rowsq_out").float()
    return r


# ---- the fold's single row factor ---------------------------------------------------------------------------------------------------------------
# With the RMSNorm fold the kernel multiplies the accumulator by ONE fp32 factor alpha * rstd[m].  The accumulator of exact operands is an
# exact fp32 integer, so given the kernel's own rstd (rowscale_r) the output is known to the bit: bf16(fp32(acc) * fp32(alpha * rstd[m])).
# The other order, (acc * rstd[m]) * alpha, gives other bf16 bits for about one element in 10^5 of random data when alpha is no power of two:
# too few to notice in one small launch.  `fold_alpha_problem` therefore picks the producer's row sums: for every row, the sum (among those a
# parts row can have) under which the most elements of that row's accumulators round differently under the two orders.  The GPU's rsqrt may
# differ from the CPU's in the last place, which moves every such element: rows take turns being picked for rstd as the CPU rounds it, one
# fp32 ulp below and one above, so a third of the rows tells the orders apart whichever way a row's rstd falls.
FOLD_ALPHAS = (0.3, 1.7)


def rstd32(parts, eps):
    """rstd as the kernel's prologue forms it in fp32: the slot sums are exact integers, then one division, one addition, rsqrt."""
    return torch.rsqrt(parts.float().sum(-1) / float(parts.shape[1] * 64) + torch.tensor(eps, dtype=torch.float32))


def fold_orders(acc, r32, alpha):
    """(bf16(acc * (alpha * r[m])), bf16((acc * r[m]) * alpha)) in fp32 arithmetic: the documented formula and the order it replaced."""
    x, r, al = acc.float(), r32.float().cpu()[:, None], torch.tensor(alpha, dtype=torch.float32)
    return (x * (al * r)).to(BF), ((x * r) * al).to(BF)


@functools.lru_cache(maxsize=None)
def _fold_table(K, alpha, eps):
    """sums [S] a parts row of integers in [1000, 2000] can have, and tells[3, S, 512]: |acc| = v rounds differently under the two orders with
    rstd of that sum one ulp below / as the CPU rounds it / one ulp above."""
    slots = K // 64
    sums, vals = torch.arange(1000 * slots, 2000 * slots + 1), torch.arange(512)[None, :].expand(1000 * slots + 1, -1)
    r = torch.rsqrt(sums.float() / float(K) + torch.tensor(eps, dtype=torch.float32))
    tells = []
    for rr in (torch.nextafter(r, torch.zeros(())), r, torch.nextafter(r, torch.ones(()))):
        one, two = fold_orders(vals, rr, alpha)
        tells.append((one != two).float())
    return sums, torch.stack(tells)


def fold_alpha_problem(g, M, N, K, alpha, eps):
    """a, b (exact operands) and parts fp32 [M, K / 64] (integers in [1000, 2000]) whose row sums tell the two orders apart (see above)."""
    a, b = operand(g, M, K), operand(g, N, K)
    sums, tells = _fold_table(K, alpha, eps)
    mag = accumulate(a, b)[0].abs().long().clamp_max(511)
    hist = torch.zeros((M, 512)).scatter_add_(1, mag, torch.ones((M, N)))          # how often row m's accumulators take each magnitude
    rows = torch.zeros(M, dtype=torch.long)
    for v in range(3):                                                             # rows 0, 3, ..: as the CPU rounds; 1, 4, ..: one ulp above; 2, 5, ..: below
        rows[v::3] = sums[(hist[v::3] @ tells[(v + 1) % 3].T).argmax(-1)]
    slots = K // 64
    parts = (rows // slots)[:, None] + (torch.arange(slots)[None, :] < (rows % slots)[:, None])
    assert torch.equal(parts.sum(-1), rows)
    return a, b, parts.float()


def fold_alpha_case(tile, BM, BN, alpha):
    """The non-power-of-two-alpha consumer case of test_rmsnorm_fold for one tile id: (a, b, parts, eps) at M = BM + 37, N = BN + 24, K = 512."""
    eps = 1e-5
    return (*fold_alpha_problem(rng(6500 + tile), BM + 37, BN + 24, 512, alpha, eps), eps)


def fold_told_apart(one, two, BM, BN):
    """How many elements of the interior tile [0, BM) x [0, BN) and of the edge tiles differ between the two outputs."""
    d = one.cpu() != two.cpu()
    inner = int(d[:BM, :BN].sum())
    return inner, int(d.sum()) - inner


# ---- embedding operands in larger allocations ------------------------------------------------------------------------------------------------
GUARD_FILLS = ("zero", "big", "nan")
SENTINEL = {2: 0x7FA5, 4: 0x7FA5A5A5}      # a NaN bit pattern no kernel produces (int16 / int32 view)


class Embedded:
    """`view` is a [rows, cols] strided view inside `buf` with guard rows above and below and guard columns left and right of every row."""

    def __init__(self, buf, r0, c0, rows, cols):
        self.buf, self.r0, self.c0, self.rows, self.cols = buf, r0, c0, rows, cols
        self.view = buf[r0:r0 + rows, c0:c0 + cols]
        self._guard = torch.ones(buf.shape, dtype=torch.bool)
        self._guard[r0:r0 + rows, c0:c0 + cols] = False

    def _bits(self, t):
        return t.view(torch.int16 if t.element_size() == 2 else torch.int32)

    def fill_guards(self, fill):
        """`fill`: "zero" | "big" (+-3e38, alternating) | "nan" | "sentinel" (SENTINEL bit pattern, for outputs)."""
        b = self.buf
        if fill == "sentinel":
            pat = torch.full(b.shape, SENTINEL[b.element_size()], dtype=self._bits(b).dtype, device=b.device)
            g = pat.view(b.dtype)
        elif fill == "big":
            sign = (torch.arange(b.shape[0], device=b.device)[:, None] + torch.arange(b.shape[1], device=b.device)[None, :]) % 2 * 2 - 1
            g = (sign * 3e38).to(b.dtype)
        else:
            g = torch.full(b.shape, {"zero": 0.0, "nan": float("nan")}[fill], dtype=b.dtype, device=b.device)
        mask = self._guard.to(b.device)
        self._bits(b)[mask] = self._bits(g)[mask]
        return self

    def assert_guards(self, what):
        """Every guard element still holds the sentinel bit pattern."""
        bits = self._bits(self.buf).cpu()
        bad = (bits != SENTINEL[self.buf.element_size()]) & self._guard
        if bad.any():
            idx = bad.nonzero()
            r, c = idx[0].tolist()
            raise AssertionError(f"{what}: {len(idx)} guard elements overwritten; first at buffer ({r}, {c}) = view ({r - self.r0}, {c - self.c0}) "
                                 f"of a [{self.rows}, {self.cols}] view")


def embed(t, *, align=8, top=3, bottom=5, left=1, right=1, fill="zero", device=None, shape=None):
    """Places `t` (2-D; or an uninitialised output of `shape` with `t` = a dtype) as a strided view inside a larger allocation.  `align` (elements):
    8 for A / B / A2 / B2 (lda % 8 == 0, 16-byte base), 4 for C / C_pre / residual / dact_src (ld % 4 == 0, 8-byte base); `left` / `right` count
    guard columns in units of `align`, so base and leading dimension keep the alignment the ABI asks for and no more than that."""
    if isinstance(t, torch.dtype):
        dtype, (rows, cols), src = t, shape, None
    else:
        dtype, (rows, cols), src = t.dtype, t.shape, t
        device = device if device is not None else t.device
    assert align * torch.empty((), dtype=dtype).element_size() in (8, 16) or dtype == torch.float32
    c0 = left * align
    ld = c0 + -(-cols // align) * align + right * align
    buf = torch.empty((top + rows + bottom, ld), dtype=dtype, device=device)
    assert buf.data_ptr() % 16 == 0
    e = Embedded(buf, top, c0, rows, cols).fill_guards(fill)
    if src is not None:
        e.view.copy_(src)
    return e


# ---- the two checkers ------------------------------------------------------------------------------------------------------------------------
def _where(r, c, tile):
    if not tile:
        return f"({r}, {c})"
    BM, BN = tile
    return f"({r}, {c}) = tile row {r // BM}, tile column {c // BN}, in-tile offset ({r % BM}, {c % BN}) of a {BM}x{BN} tile"


def assert_exact(out, ref, what="", tile=None):
    """Bit equality.  On failure: how many elements differ, the first and the worst (row, col), and where in the tile grid of the
    configuration under test (`tile` = (BM, BN)) they lie."""
    out, ref = out.detach().cpu(), ref.detach().cpu()
    assert out.shape == ref.shape and out.dtype == ref.dtype, f"{what}: {tuple(out.shape)} {out.dtype} vs {tuple(ref.shape)} {ref.dtype}"
    if torch.equal(out, ref):
        return
    bits = torch.int16 if out.element_size() == 2 else torch.int32
    bad = out.contiguous().view(bits) != ref.contiguous().view(bits)
    if not bad.any():      # +0 / -0 style differences that torch.equal hides never reach here; equal bits are equal
        return
    idx = bad.nonzero()
    err = (out.double() - ref.double()).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf"))) * bad
    w = int(err.argmax())
    wr, wc = w // out.shape[1], w % out.shape[1]
    fr, fc = idx[0].tolist()
    rows, cols = idx[:, 0].unique(), idx[:, 1].unique()
    raise AssertionError(f"{what}: {len(idx)} of {out.numel()} elements differ (rows {int(rows[0])}..{int(rows[-1])}, {len(rows)} distinct; columns "
                         f"{int(cols[0])}..{int(cols[-1])}, {len(cols)} distinct); first at {_where(fr, fc, tile)}: got {out[fr, fc].item()} want "
                         f"{ref[fr, fc].item()}; worst at {_where(wr, wc, tile)}: got {out[wr, wc].item()} want {ref[wr, wc].item()}")


def ulp_error(out, ref64, abs_floor=None):
    """|out - ref64| in bf16 ulps of ref64, after the absolute floor has been taken off (float64 tensor)."""
    err = (out.detach().cpu().double() - ref64).abs()
    if abs_floor is not None:
        err = (err - abs_floor).clamp_min(0.0)
    return err / ulp_bf16(ref64)


def assert_ulps(out, ref64, n, abs_floor=None, what="", tile=None):
    """|out - ref64| <= n bf16 ulps of ref64 (+ abs_floor) for every element; returns the worst observed |err| / ulp."""
    assert out.shape == ref64.shape, f"{what}: {tuple(out.shape)} vs {tuple(ref64.shape)}"
    o = out.detach().cpu()
    assert torch.isfinite(o.float()).all(), f"{what}: non-finite output"
    e = ulp_error(o, ref64, abs_floor)
    worst = float(e.max())
    if worst > n:
        w = int(e.argmax())
        r, c = w // o.shape[1], w % o.shape[1]
        raise AssertionError(f"{what}: {(e > n).sum().item()} of {o.numel()} elements beyond {n} ulp; worst {worst:.3f} ulp at {_where(r, c, tile)}: "
                             f"got {o[r, c].item()} want {ref64[r, c].item():.9g}")
    return worst


class Failures(list):
    """Collects the failures of a test that loops over shapes, so one run reports all of them."""

    def exact(self, out, ref, what, tile=None):
        """`ref`: bf16 on either device.  Compared on the GPU; the report (tile row / column / offset) is only built on a mismatch."""
        if out.shape == ref.shape and torch.equal(out, ref.to(out.device)):
            return
        try:
            assert_exact(out, ref, what, tile)
        except AssertionError as e:
            self.append(str(e))

    def ulps(self, out, ref64, n, what, abs_floor=None, tile=None):
        try:
            return assert_ulps(out, ref64, n, abs_floor, what, tile)
        except AssertionError as e:
            self.append(str(e))
            return float(ulp_error(out, ref64, abs_floor).max())

    def check(self, cond, what):
        if not cond:
            self.append(what)

    def done(self):
        assert not self, f"{len(self)} failures:\n" + "\n".join(self[:12])
