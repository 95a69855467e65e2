"""float64 references, derived error bounds, exact-regime generators and an op-by-op fp32 AdamW emulation for the kernels of
`csrc/elementwise.hip` and `csrc/head_optim.hip` (norms, RoPE, SwiGLU, activation backward, token cross-entropy, head output, FiLM backward,
masked mean, AdamW).  Nothing here needs a GPU.  The bf16 arithmetic, the checkers and the guard machinery are those of
tests/gemm_reference.py; this module adds what the row-wise kernels need.

Three kinds of comparison, none of them normalised by the largest element of a tensor:

* bit equality (`assert_exact`) wherever the kernel's result does not depend on the order of its fp32 sums: RoPE, the copies and casts,
  AdamW (a fixed sequence of IEEE fp32 operations and bf16 roundings), and every accumulating kernel fed from the exact-regime generators
  below (small integers and powers of two: every fp32 partial sum is an integer below 2^24 times one power of two, so any order is exact);
* bf16 ulps of the float64 value (`assert_ulps`): ONE rounding of an fp32 expression whose own error is far below the bf16 ulp is within 1 ulp
  (1/2 from the store, 1/2 for a value the fp32 error moved across a rounding boundary); a value that was rounded, multiplied by an exact factor
  and rounded again is within 2 (gemm_reference.ULPS).  The second bound is rigorous when the factor's mantissa is at most 1.5 -- the inner ulp
  times the factor is then at most 1.5 ulps of the product, plus 1/2 from the store -- which is why `mant15` draws such factors;
* an absolute floor where an fp32 reduction can cancel (`U32`-based, below): the forward error bound of a sum of n terms evaluated as
  sequential adds per lane plus a butterfly / tree is (adds per lane + tree levels) * 2^-24 * sum |terms| (Higham, Accuracy and Stability of
  Numerical Algorithms, 4.2, first order), and everything computed from that sum inherits it through its derivative.  Each floor below states
  its terms next to the code.

Hardware functions: rsqrtf, powf, sinf, cosf and the v_exp_f32 / v_log_f32 behind __expf / __logf are taken at 1 ulp (2^-23 relative), the
accuracy the HIP math tables and the CDNA ISA manual state; __expf(y) = exp2(y log2 e) adds |y| 2^-24 from the rounded product.
"""
import math

import torch

from tests.gemm_reference import (BF, ERF_FLOOR, SENTINEL, ULPS, Embedded, Failures, _exact32, _sigmoid, act64, act_grad64,  # noqa: F401
                                  assert_exact, assert_ulps, choice, embed, ints, rbf, rng, tbf, ulp_bf16, ulp_error)

U32 = 2.0 ** -24                 # unit roundoff of fp32
HW = 2.0 ** -23                  # one ulp of an fp32 hardware function, relative
BF_MAX = 3.3895313892515355e38   # largest finite bf16
ERF_GRAD_FLOOR = 1e-7            # * |dh|: fast_erf's 1.5e-7 absolute bound (common.h) times the 0.5 that multiplies it in the GELU derivative, rounded up
GRID_CAP_ITEMS = 4096 * 256      # grid_for(): work items one trip of a grid-stride loop covers
ADAMW_CAP_ITEMS = 8192 * 256

NORM_DIMS = (8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048, 2056, 4104)
NORM_ROWS = (1, 3, 4, 5, 9)


# ---- small helpers ---------------------------------------------------------------------------------------------------------------------------
def to_bf(x64):
    """float64 -> bf16 tensor, one rounding (ties to even), overflow to +-inf as the hardware convert does."""
    r = rbf(x64)
    r = torch.where(r.abs() > BF_MAX, torch.sign(r) * float("inf"), r)
    return r.to(BF)


def mant15(g, shape, exps=(-1, 0, 1), signed=True):
    """bf16 factors with mantissa in {1, 1.25, 1.5} times 2^e: products with them are exact in fp32 and the 2-ulp bound is rigorous."""
    v = choice(g, shape, (1.0, 1.25, 1.5)).double() * torch.pow(2.0, choice(g, shape, [float(e) for e in exps]).double())
    if signed:
        v = v * choice(g, shape, (1.0, -1.0)).double()
    return v.to(BF)


def pow2(g, shape, exps=(-1, 0, 1)):
    return torch.pow(2.0, choice(g, shape, [float(e) for e in exps]).double()).to(BF)


def randn_bf(g, shape, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(BF)


def all_finite_bf16():
    """Every finite bf16 bit pattern (65,280 values, both zeros included), padded with 1.0 to a multiple of 8."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    assert bits.numel() == 65280
    return bits.to(torch.int16).view(BF).contiguous()


def assert_abs(out, ref64, bound, what=""):
    """|out - ref64| <= bound per element (fp32 outputs with a derived absolute bound); returns the worst |err| / bound."""
    o = out.detach().cpu().double()
    assert o.shape == ref64.shape, f"{what}: {tuple(o.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    err = (o - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        w = int(ratio.argmax())
        raise AssertionError(f"{what}: {(ratio > 1).sum().item()} of {o.numel()} elements beyond their bound; worst |err| / bound = {worst:.3f} at flat index {w}: "
                             f"got {o.flatten()[w].item():.9g} want {ref64.flatten()[w].item():.9g} bound {bound.flatten()[w].item():.3g}")
    return worst


class Checks(Failures):
    """gemm_reference.Failures plus the absolute-bound check and a record of the worst observed |err| / bound per label."""
    worst = {}

    def note(self, label, ratio):
        if ratio is not None:
            Checks.worst[label] = max(Checks.worst.get(label, 0.0), float(ratio))
        return ratio

    def ulps(self, out, ref64, n, what, abs_floor=None, tile=None):
        """Failures.ulps, but what comes back (and is recorded) is the worst |err| / (n ulps + floor): a result that uses 99 % of its floor says so."""
        super().ulps(out, ref64, n, what, abs_floor, tile)
        o = out.detach().cpu().double()
        if o.shape != ref64.shape:
            return float("inf")
        err = torch.nan_to_num((o - ref64).abs(), nan=float("inf"))
        bound = n * ulp_bf16(ref64) + (abs_floor if abs_floor is not None else 0.0)
        return float((err / bound).max())

    def abs(self, out, ref64, bound, what):
        try:
            return assert_abs(out, ref64, bound, what)
        except AssertionError as e:
            self.append(str(e))
            return float("inf")


class Guarded:
    """A CONTIGUOUS output of `shape` inside a flat allocation with 64 sentinel elements before and after it (the kernels that take no leading
    dimension): `view` is what the kernel writes, `assert_guards` checks that nothing around it changed."""
    PAD = 64

    def __init__(self, dtype, shape, device="cpu"):
        n = math.prod(shape)
        self.n = n
        self.buf = torch.empty(n + 2 * self.PAD, dtype=dtype, device=device)
        self.ibits = torch.int16 if self.buf.element_size() == 2 else torch.int32
        self.buf.view(self.ibits).fill_(SENTINEL[self.buf.element_size()])
        self.view = self.buf[self.PAD:self.PAD + n].view(shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()

    def assert_guards(self, what):
        b = self.buf.view(self.ibits).cpu()
        g = torch.cat([b[:self.PAD], b[self.PAD + self.n:]])
        bad = (g != SENTINEL[self.buf.element_size()]).nonzero()
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{what}: {len(bad)} guard elements overwritten; first {self.PAD - i} before the view" if i < self.PAD
                                 else f"{what}: {len(bad)} guard elements overwritten; first {i - self.PAD} past the end of the view")


# ---- reductions ------------------------------------------------------------------------------------------------------------------------------
def norm_lanes(dim):
    """Threads that share one row: a wave for dim <= 1536 (norm_fwd_wave_kernel), the 256-thread workgroup above (norm_fwd_kernel).  The
    backward is always the workgroup kernel."""
    return 64 if dim <= 1536 else 256


def red_terms(n, lanes):
    """Rounding errors one term of an n-term fp32 sum can meet: sequential adds of its lane (8 per 16-byte chunk, chunks dealt round-robin) +
    6 butterfly levels (+ 3 adds of the four wave sums for a workgroup)."""
    chunks = -(-n // 8)
    return 8 * -(-chunks // lanes) + 6 + (3 if lanes == 256 else 0)


# ---- norms -----------------------------------------------------------------------------------------------------------------------------------
def norm_fwd_ref(x, w, b, eps, rms, lanes=None):
    """float64 RMSNorm  y = bf16(w * bf16(x * rstd))  /  LayerNorm  y = bf16((x - mean) * rstd * w + b)  of x [rows, dim] (bf16, CPU).
    Returns a dict: y64 (the value whose bf16 rounding is y), ulps, floor (None for RMS), mean, rstd, mean_bound (absolute), rstd_rel."""
    x64, w64 = x.double(), w.double()
    rows, dim = x64.shape
    T = red_terms(dim, lanes or norm_lanes(dim))
    mean = torch.zeros(rows, dtype=torch.float64) if rms else x64.mean(-1)
    # mean = fl(sum) / dim: T roundings on the sum weighted by sum |x|, one on the division
    mean_bound = torch.zeros(rows, dtype=torch.float64) if rms else (T + 1) * U32 * x64.abs().sum(-1) / dim
    var = ((x64 - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    # var: d = fl(x - mean) squared (2 roundings), T fma adds, the division, + eps; a mean off by D adds dim D^2 to the sum of squares (the first-order
    # term vanishes: sum (x - mean) = 0).  rstd = rsqrtf(var): half of var's relative error plus one ulp of rsqrtf.
    rstd_rel = 0.5 * ((T + 4) * U32 + mean_bound ** 2 / (var + eps)) + HW
    if rms:
        inner = rbf(x64 * rstd[:, None])
        return dict(y64=w64[None] * inner, ulps=2, floor=None, mean=mean, rstd=rstd, mean_bound=mean_bound, rstd_rel=rstd_rel)
    t = (x64 - mean[:, None]) * rstd[:, None] * w64[None]
    y64 = t + (b.double()[None] if b is not None else 0.0)
    # y = fma(fl(fl(x - mean) * rstd), w, b): the mean's error enters as |w| rstd D, rstd's and the two roundings of the factor relative to t, the
    # fma's single rounding relative to y.  Where b cancels t this floor, not the ulp of the small result, is what fp32 delivers.
    floor = w64.abs()[None] * rstd[:, None] * mean_bound[:, None] + t.abs() * (rstd_rel[:, None] + 2 * U32) + U32 * y64.abs()
    return dict(y64=y64, ulps=1, floor=floor, mean=mean, rstd=rstd, mean_bound=mean_bound, rstd_rel=rstd_rel)


def balanced_rows(g, rows, dim, k):
    """Rows holding +2^k and -2^k in equal numbers, shuffled: mean is exactly 0 and var exactly 4^k in any summation order."""
    assert dim % 2 == 0
    base = torch.cat([torch.full((dim // 2,), 2.0 ** k), torch.full((dim // 2,), -(2.0 ** k))])
    return torch.stack([base[torch.randperm(dim, generator=g)] for _ in range(rows)]).to(BF)


def norm_bwd_ref(x, dy, w, mean, rstd, rms, dx0=None, dw0=None, db0=None, exact=False):
    """float64 backward from GIVEN fp32 statistics (mean None for RMS):  g = dy w,  xhat = (x - mean) rstd,
    dx = bf16([dx0 +] rstd (g - mean(g) - xhat mean(g xhat)))  (mean(g) dropped for RMS),  dw += sum_r dy xhat,  db += sum_r dy.
    Returns dict(dx64, dx_floor, dw, dw_bound, db, db_bound); with `exact` the sums are asserted to be in the exact regime."""
    x64, dy64, w64 = x.double(), dy.double(), w.double()
    rows, dim = x64.shape
    T = red_terms(dim, 256)
    mu = torch.zeros(rows, dtype=torch.float64) if rms else mean.double()
    rs = rstd.double()
    g = dy64 * w64[None]
    xhat = (x64 - mu[:, None]) * rs[:, None]
    gx = g * xhat
    m1 = torch.zeros(rows, dtype=torch.float64) if rms else g.mean(-1)
    m2 = gx.mean(-1)
    v = rs[:, None] * (g - m1[:, None] - xhat * m2[:, None])
    # m1, m2: T roundings on the sum (+ 1 / + 3 for the division and the roundings inside each term) weighted by the abs-sum; dx inherits them
    # through rstd (d m1 + |xhat| d m2), plus four roundings of the final expression on its abs-weighted value, plus one for the accumulate add.
    d1 = torch.zeros(rows, dtype=torch.float64) if rms else (T + 1) * U32 * g.abs().sum(-1) / dim
    d2 = (T + 3) * U32 * gx.abs().sum(-1) / dim
    floor = rs[:, None] * (d1[:, None] + xhat.abs() * d2[:, None]) + 4 * U32 * rs[:, None] * (g.abs() + m1.abs()[:, None] + (xhat * m2[:, None]).abs())
    dx64 = v
    if dx0 is not None:
        dx64 = dx0.double() + v
        floor = floor + U32 * (dx0.double().abs() + v.abs())
    dw = (dy64 * xhat).sum(0)
    db = dy64.sum(0)
    # one thread per column, rows in order: `rows` adds, two roundings inside the term, one for the += onto the start value
    dw_bound = (rows + 3) * U32 * ((dy64 * xhat).abs().sum(0) + (dw0.double().abs() if dw0 is not None else 0.0))
    db_bound = (rows + 1) * U32 * (dy64.abs().sum(0) + (db0.double().abs() if db0 is not None else 0.0))
    if dw0 is not None:
        dw = dw + dw0.double()
    if db0 is not None:
        db = db + db0.double()
    if exact:
        _exact32(xhat, "xhat"), _exact32(dy64 * xhat, "dy xhat"), _exact32(dw, "dw"), _exact32(db, "db")
        assert float((dy64 * xhat).abs().sum(0).max()) < 2 ** 20, "dw: partial sums leave the exact regime"
    return dict(dx64=dx64, dx_floor=floor, dw=dw, dw_bound=dw_bound, db=db, db_bound=db_bound)


def norm_bwd_exact_inputs(g, rows, dim):
    """x - mean integer, mean small integers, rstd and w powers of two, dy integer: dw, db and every partial sum are exact."""
    mean = ints(g, (rows,), -2, 2, dtype=torch.float32)
    x = (ints(g, (rows, dim), -6, 6, dtype=torch.float32) + mean[:, None]).to(BF)
    rstd = pow2(g, (rows,), (-1, 0, 1)).float()
    return x, ints(g, (rows, dim), -4, 4, nonzero=True), pow2(g, (dim,), (-1, 0, 1)), mean, rstd


# ---- RoPE ------------------------------------------------------------------------------------------------------------------------------------
def rope_ref(qk, cos, sin, S, n_heads, hd, inverse=False):
    """bf16(bf16(a c) + bf16(-b s)) | bf16(bf16(b c) + bf16(a s)) on the first n_heads * hd columns of qk [rows, ld], pos = row % S; the other
    columns are returned as they are.  Every product is rounded to bf16 before the add and the add of two bf16 values is exact in fp32 up to its
    single rounding, so the kernel reproduces this bit for bit for ANY input."""
    out = qk.clone()
    rows, half = qk.shape[0], hd // 2
    pos = torch.arange(rows) % S
    c = cos.double()[pos][:, None, :]
    s = sin.double()[pos][:, None, :] * (-1.0 if inverse else 1.0)
    x = qk[:, :n_heads * hd].double().view(rows, n_heads, hd)
    a, b = x[..., :half], x[..., half:]
    lo = rbf(a * c) + rbf(-b * s)
    hi = rbf(b * c) + rbf(a * s)
    out[:, :n_heads * hd] = to_bf(torch.cat([lo, hi], -1)).view(rows, n_heads * hd)
    return out


def rope_table_ref(S, hd, theta):
    """cos / sin of the angle pos * (1 / theta^(2 i / hd)) in float64, from the fp32 exponent the kernel forms (an IEEE division), and the absolute
    floor of the fp32 evaluation: powf, the reciprocal and the product are 1 + 1/2 + 1/2 ulp = 2^-22 relative on the angle, and d cos = d sin <= d angle;
    cosf / sinf add one ulp of a result <= 1."""
    half = hd // 2
    e32 = (torch.arange(half, dtype=torch.float32) * 2.0) / torch.tensor(float(hd), dtype=torch.float32)
    inv = torch.pow(torch.tensor(float(theta), dtype=torch.float64), -e32.double())
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None]
    floor = ang.abs() * 2.0 ** -22 + HW
    return torch.cos(ang), torch.sin(ang), floor


# ---- SwiGLU and activation backward ------------------------------------------------------------------------------------------------------------
def swiglu_fwd_ref(gu):
    """h = bf16(bf16(silu(g)) * u), gu = [g | u].  float64 [rows, F]; 2 ulps."""
    F = gu.shape[1] // 2
    g, u = gu[:, :F].double(), gu[:, F:].double()
    return rbf(act64(g, 3)) * u


def swiglu_bwd_ref(gu, dh):
    """dgu = [bf16(dh u silu'(g)) | bf16(dh bf16(g sigmoid(g)))].  float64 [rows, 2 F]; 2 ulps."""
    F = gu.shape[1] // 2
    g, u, d = gu[:, :F].double(), gu[:, F:].double(), dh.double()
    s = _sigmoid(g)
    return torch.cat([d * u * (s * (1.0 + g * (1.0 - s))), d * rbf(g * s)], 1)


def act_bwd_ref(z, dh, act):
    """dz = bf16(dh * act'(z)): float64 value and the absolute floor (erf-GELU only)."""
    z64, d64 = z.double(), dh.double()
    out = d64 * act_grad64(z64, act)
    return out, (ERF_GRAD_FLOOR * d64.abs() if act == 1 else None)


def sigmoid_f32(y, tail=True):
    """common.h's sigmoidf_ op by op in fp32 (torch CPU; exp in float64 rounded to fp32 stands in for __expf: it overflows and flushes where fp32
    does): 1 / (1 + e), and exp(y) once e = exp(-y) has overflowed.  tail=False is the bare form, 0 from y = -88.7 on."""
    e = torch.exp(-y.double()).float()
    s = 1.0 / (1.0 + e)
    return torch.where(torch.isinf(e), torch.exp(y.double()).float(), s) if tail else s


def silu_f32(x, tail=True):
    e = torch.exp(-x.double()).float()
    s = x / (1.0 + e)
    return torch.where(torch.isinf(e), x * torch.exp(x.double()).float(), s) if tail else s


def gelu_tanh_grad_f32(z, clamp=True, tail=True):
    """common.h's gelu_tanh_grad op by op in fp32.  clamp=False leaves the polynomial factor unclamped: 0 * inf = NaN for z <= -2e13 and near the bf16
    maximum."""
    k, c = torch.tensor(0.7978845608028654).float(), torch.tensor(0.044715).float()
    x = z.float()
    s = sigmoid_f32(2.0 * k * (x + c * x * x * x), tail)
    xc = x.clamp(-16.0, 16.0) if clamp else x
    return s * (1.0 + 2.0 * xc * (1.0 - s) * k * (1.0 + 3.0 * c * xc * xc))


# ---- token cross-entropy ---------------------------------------------------------------------------------------------------------------------
def token_ce_ref(logits, targets, vocab, grad_scale=None):
    """float64 next-token cross entropy of logits[:, :vocab] (bf16) with targets clamped to [0, vocab): per-row loss, FIRST maximum, gradient
    (p - onehot) * grad_scale, and the derived bounds.  A row without a finite maximum (all -inf, or only NaN) has argmax 0.
    With p_j = exp(x_j - m) / s and T = ceil(vocab / 256) + 8 (adds per thread + butterfly + the four wave sums):
      ds / s  <= sum_j p_j (|x_j - m| + 2) 2^-24 + T 2^-24            (__expf: the rounded product y log2 e, v_exp_f32, and the sum)
      d loss  <= ds / s + 3 * 2^-24 |log s| + 2^-24 |log s + m| + 2^-24 |loss|      (v_log_f32 and the ln 2 product; the add; the subtraction)
      d p_j   <= p_j ((|x_j - m| + 4) 2^-24 + ds / s);   d grad_j <= grad_scale (d p_j + 2 * 2^-24 |p_j - onehot_j|)
    A confident row has loss ~ 1e-4 = log(1 + 1e-4): s is only known to 2^-24 T, so the loss is to about 5e-7 absolute -- 0.5 % of it, not 2e-5."""
    x = logits[:, :vocab].double()
    rows = x.shape[0]
    tgt = targets.clamp(0, vocab - 1)
    m = x.max(-1).values
    finite_max = torch.isfinite(m)
    am = torch.where(finite_max | (m == float("inf")), (x == m[:, None]).double().argmax(-1), torch.zeros(rows, dtype=torch.long))
    e = torch.exp(x - m[:, None])
    s = e.sum(-1)
    p = e / s[:, None]
    xt = x.gather(1, tgt[:, None])[:, 0]
    loss = (torch.log(s) + m) - xt
    T = -(-vocab // 256) + 8
    dist = torch.where(torch.isfinite(x), (x - m[:, None]).abs(), torch.zeros_like(x))
    ds = ((p * (dist + 2)).sum(-1) + T) * U32
    loss_bound = ds + 3 * U32 * torch.log(s).abs() + U32 * (torch.log(s) + m).abs() + U32 * loss.abs()
    r = dict(loss=loss, loss_bound=loss_bound, argmax=am.to(torch.int32), grad64=None, grad_floor=None)
    if grad_scale is not None:
        onehot = torch.zeros_like(x).scatter_(1, tgt[:, None], 1.0)
        dp = p * ((dist + 4) * U32 + ds[:, None])
        r["grad64"] = (p - onehot) * grad_scale
        r["grad_floor"] = abs(grad_scale) * (dp + 2 * U32 * (p - onehot).abs())
    return r


# ---- head output -----------------------------------------------------------------------------------------------------------------------------
def head_inputs(g, rows, dim, adim):
    """Integer x and W in [-3, 3], integer bias, and a target within a few bf16 steps of the prediction (some equal to it), so that pred, the loss
    terms and every gradient sum are integers far below 2^24."""
    x, W, b = ints(g, (rows, dim), -3, 3), ints(g, (adim, dim), -3, 3, nonzero=True), ints(g, (adim,), -8, 8)
    pred = rbf(x.double() @ W.double().T + b.double())
    k = ints(g, (rows, adim), -3, 3, dtype=torch.float64)
    k[::2, 0] = 0.0                                           # pred == target: the L1 gradient there is exactly 0
    target = to_bf(pred + k * ulp_bf16(pred).clamp_min(1.0))
    return x, W, b, target


def head_ref(x, W, b, target, mse, scale=None, loss0=0.0, dW0=None, db0=None, dpred=None):
    """pred = bf16(x . W^T + b);  loss_sum = loss0 + sum |bf16(target - pred)|  (MSE: bf16(d^2));  backward from dpred = bf16(sign(d') scale)
    (MSE: bf16(bf16(2 d' scale))), d' = bf16(pred - target), or from an explicit `dpred`:  dx = bf16(dpred . W),  dW += dpred^T . x,  db += sum_m dpred.
    Everything is asserted to stay in the exact regime."""
    x64, W64 = x.double(), W.double()
    acc = _exact32(x64 @ W64.T + (b.double() if b is not None else 0.0), "head accumulator")
    assert 9 * x.shape[1] < 2 ** 24
    pred = rbf(acc)
    r = dict(pred=pred.to(BF))
    if target is not None:
        d = rbf(target.double() - pred)
        terms = rbf(d * d) if mse else d.abs()
        assert float(terms.sum()) + abs(loss0) < 2 ** 24 and torch.equal(terms, terms.round()), "loss terms leave the exact regime"
        r["loss_sum"] = torch.tensor([loss0 + float(terms.sum())], dtype=torch.float32)
    if scale is not None or dpred is not None:
        if dpred is None:
            dd = rbf(pred - target.double())
            dp = rbf(rbf(2.0 * dd * scale)) if mse else torch.sign(dd) * rbf(torch.tensor(scale, dtype=torch.float64))
        else:
            dp = dpred.double()
        r["dpred"] = dp
        r["dx"] = to_bf(_exact32(dp @ W64 + 0.0, "head dx"))          # + 0.0: the kernel's sum starts from +0, so a sum of -0 terms is +0
        r["dW"] = _exact32(dp.T @ x64 + (dW0.double() if dW0 is not None else 0.0), "head dW").float()
        r["db"] = _exact32(dp.sum(0) + (db0.double() if db0 is not None else 0.0), "head db").float()
    return r


# ---- FiLM backward, masked mean ----------------------------------------------------------------------------------------------------------------
def film_bwd_ref(dy, x_pre, gamma, dgamma0, dbeta0, B, rows):
    """dy <- bf16(dy * bf16(1 + gamma[b]));  dgamma[b] += sum_r dy x_pre;  dbeta[b] += sum_r dy  (the incoming dy).  Exact regime asserted."""
    dim = dy.shape[1]
    d, xp = dy.double().view(B, rows, dim), x_pre.double().view(B, rows, dim)
    one_plus = rbf(1.0 + gamma.double())
    out = to_bf(_exact32(d * one_plus[:, None, :], "film dy")).view(B * rows, dim)
    dg = _exact32(dgamma0.double() + (d * xp).sum(1), "dgamma").float()
    db = _exact32(dbeta0.double() + d.sum(1), "dbeta").float()
    return out, dg, db


def masked_mean_ref(x, mask, B, L, dim):
    """bf16(fl32(sum) / fl32(max(count, 1))) with integer x (the sum is exact; the fp32 division is IEEE on both sides); all-zero mask: zeros."""
    xf = x.float().view(B, L, dim) * mask.view(B, L, 1).float()
    cnt = mask.view(B, L).float().sum(1).clamp_min(1.0)
    return (xf.sum(1) / cnt[:, None]).to(BF)


# ---- AdamW: the kernels' sequence of fp32 operations, one torch CPU op each ---------------------------------------------------------------------
def fma32(a, b, c):
    """Correctly rounded fp32 fma(a, b, c) on fp32 tensors: the product is exact in float64 (48 bits); the float64 sum is made round-to-odd with
    TwoSum (so the second rounding, to fp32, cannot double-round: 53 >= 24 + 2), then narrowed."""
    p = a.double() * b.double()
    c64 = c.double()
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)
    even = (s.view(torch.int64) & 1) == 0
    toward = torch.where(err > 0, torch.full_like(s, float("inf")), torch.full_like(s, float("-inf")))
    s = torch.where((err != 0) & even & torch.isfinite(s), torch.nextafter(s, toward), s)
    return s.float()


def adamw_scalars(step, lr, beta1, beta2, eps, weight_decay, grad_scale):
    """ovla_adamw's scalars: computed in double as torch/optim/adamw.py does, narrowed to fp32."""
    f = lambda v: torch.tensor(v, dtype=torch.float64).float()  # noqa: E731
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return dict(decay=f(1.0 - lr * weight_decay), w1=f(1.0 - beta1), beta2=f(beta2), w2=f(1.0 - beta2), bc2_sqrt=f(math.sqrt(bc2)), eps=f(eps),
                step_size=f(-(lr / bc1)), grad_scale=f(grad_scale))


def _aten_lerp(a, b, w):
    d = b - a
    return fma32(w.expand_as(a), d, a) if abs(float(w)) < 0.5 else fma32((w - 1.0).expand_as(a), d, b)


def sqrt32(x):
    """IEEE fp32 square root.  torch's vectorised CPU sqrt of fp32 is a 1-ulp routine (0.65 % of inputs differ from the correctly rounded
    result, which is what the kernels' sqrtf returns); through float64 the second rounding is innocuous (53 >= 2 * 24 + 2)."""
    return torch.sqrt(x.double()).float()


def adamw_emulate(p, m, v, g, *, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, mut=None):
    """adamw_bf16_kernel / adamw_f32_kernel (by p.dtype) on CPU tensors; returns new (p, m, v).  torch's CPU fp32 multiply, add, divide and sqrt are
    IEEE, sqrt goes through `sqrt32`, the kernels are compiled with fp contract(off) and correctly rounded division and sqrt: no tolerance is involved.
    `mut`: "fma" fuses (w2 grad) grad + v into one rounding; "no_grad_scale" drops the grad_scale product."""
    s = adamw_scalars(step, lr, beta1, beta2, eps, weight_decay, grad_scale)
    r = (lambda t: t.to(BF).float()) if p.dtype == BF else (lambda t: t)
    pf, mf, vf = p.float(), m.float(), v.float()
    grad = r(g if mut == "no_grad_scale" else g * s["grad_scale"])
    pp = r(pf * s["decay"])
    mm = r(_aten_lerp(mf, grad, s["w1"]))
    vv = r(vf * s["beta2"])
    vv = r(fma32(s["w2"] * grad, grad, vv)) if mut == "fma" else r(vv + (s["w2"] * grad) * grad)
    d = r(sqrt32(vv))
    d = r(d / s["bc2_sqrt"])
    d = r(d + s["eps"])
    pp = r(pp + (s["step_size"] * mm) / d)
    return pp.to(p.dtype), mm.to(p.dtype), vv.to(p.dtype)


ADAMW_GRID = [(lr, wd, gs, b2, eps) for lr in (5e-4, 1e-2) for wd in (0.0, 0.01) for gs in (1.0, 2.0 ** -7, 0.37) for b2 in (0.999, 0.95) for eps in (1e-8, 1e-6)]
ADAMW_STEPS = (1, 2, 3, 1000)


def adamw_inputs(g, n, dtype):
    """Parameters ~ 0.05, gradients with magnitudes spread over 1e-8 .. 1e2, a block of exact zeros with zero state (denominator = eps), and a block
    of large parameters with tiny gradients whose update is below half an ulp."""
    p = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * torch.pow(10.0, torch.randint(-8, 3, (n,), generator=g).float())
    m = torch.randn(n, generator=g) * 1e-2
    v = (torch.randn(n, generator=g) * 1e-2) ** 2
    q = n // 8
    grad[:q], m[:q], v[:q] = 0.0, 0.0, 0.0
    p[q:2 * q] = torch.randn(q, generator=g) * 50.0 + 100.0
    grad[q:2 * q] *= 1e-6
    m[q:2 * q] *= 1e-6
    return p.to(dtype), m.to(dtype), v.to(dtype), grad.float()


# ================================================================================================================================================
# The suites.  Each takes a `Checks` and an object K whose methods run one kernel on CPU tensors and return CPU tensors: the GPU files pass
# `GpuKernels` (below: the real launches, outputs in guarded buffers), tests/test_pointwise_reference.py passes an fp32 emulation of the same
# kernels, with and without planted bugs.  Shapes and data are decided here, once, for both.
# ================================================================================================================================================
def _sent(shape, dtype=BF):
    n = torch.empty(shape, dtype=dtype)
    n.view(torch.int16 if n.element_size() == 2 else torch.int32).fill_(SENTINEL[n.element_size()])
    return n


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(fails, out, ref, what):
    """Bit equality that also holds NaN payloads equal (guards and sentinel-filled regions are part of the comparison)."""
    ok = out.shape == ref.shape and out.dtype == ref.dtype and torch.equal(_bits(out.cpu()), _bits(ref.cpu()))
    if not ok and out.shape == ref.shape and out.dtype == ref.dtype:
        bad = (_bits(out.cpu()) != _bits(ref.cpu())).flatten().nonzero()[:, 0]
        i = int(bad[0])
        fails.append(f"{what}: {len(bad)} of {out.numel()} elements differ in bits (flat indices {i}..{int(bad[-1])}); first: got {out.flatten()[i].item()} want {ref.flatten()[i].item()}")
    elif not ok:
        fails.append(f"{what}: {tuple(out.shape)} {out.dtype} vs {tuple(ref.shape)} {ref.dtype}")


def suite_norm_fwd(fails, K, dims=NORM_DIMS, rows_list=NORM_ROWS):
    for dim in dims:
        g = rng(100 + dim)
        w, bias = mant15(g, (dim,)), randn_bf(g, (dim,))
        for rows in rows_list:
            x = randn_bf(g, (rows, dim), 2.0, 0.5)
            for rms in (True, False):
                eps = 1e-5 if rms else 1e-6
                for b in ((None,) if rms else (None, bias)):
                    ref = norm_fwd_ref(x, w, b, eps, rms)
                    for save in (True, False):
                        y, mean, rstd = K.norm_fwd(x, w, b, eps, rms, save)
                        what = f"norm_fwd {'rms' if rms else 'ln'} {rows}x{dim} bias {b is not None} stats {save}"
                        fails.note("norm_fwd rms y" if rms else "norm_fwd ln y", fails.ulps(y, ref["y64"], ref["ulps"], what, ref["floor"]))
                        fails.check((rstd is not None) == save and (mean is not None) == (save and not rms), what + ": which statistics came back")
                        if save:
                            fails.note("norm_fwd rstd", fails.abs(rstd, ref["rstd"], ref["rstd_rel"] * ref["rstd"], what + " rstd"))
                            if not rms:
                                fails.note("norm_fwd mean", fails.abs(mean, ref["mean"], ref["mean_bound"], what + " mean"))
    # one exact case per kernel variant (one live lane, <2>, <3>, workgroup with a second chunk for thread 0): mean is exactly 0, var exactly 4^k
    g = rng(99)
    for dim in (8, 512, 1536, 2056):
        w = mant15(g, (dim,))
        for k in (-3, 0, 5):
            x = balanced_rows(g, 5, dim, k)
            for rms in (True, False):
                eps = 1e-5 if rms else 1e-6
                _, mean, rstd = K.norm_fwd(x, w, None, eps, rms, True)
                what = f"norm_fwd exact {'rms' if rms else 'ln'} 5x{dim} +-2^{k}"
                if not rms:
                    fails.exact(mean.view(1, -1), torch.zeros(1, 5), what + " mean")
                v32 = (torch.tensor(4.0 ** k, dtype=torch.float32) + torch.tensor(eps, dtype=torch.float32)).double()     # the kernel's own fp32 add
                r64 = (1.0 / torch.sqrt(v32)).expand(5)
                fails.note("norm_fwd exact rstd", fails.abs(rstd, r64, HW * r64, what + " rstd (rsqrtf: 1 ulp)"))


def suite_norm_bwd(fails, K, dims=NORM_DIMS, rows_list=NORM_ROWS):
    for dim in dims:
        g = rng(200 + dim)
        for rows in rows_list:
            # exact regime: the statistics are handed in
            x, dy, w, mean, rstd = norm_bwd_exact_inputs(g, rows, dim)
            dw0, db0 = ints(g, (dim,), -5, 5, nonzero=True, dtype=torch.float32), ints(g, (dim,), -5, 5, nonzero=True, dtype=torch.float32)
            dx0 = ints(g, (rows, dim), -4, 4, nonzero=True)
            for rms in (True, False):
                what = f"norm_bwd exact {'rms' if rms else 'ln'} {rows}x{dim}"
                for acc in (None, dx0):
                    ref = norm_bwd_ref(x, dy, w, None if rms else mean, rstd, rms, dx0=acc, dw0=dw0, db0=db0, exact=True)
                    dx, dw, db = K.norm_bwd(x, dy, w, None if rms else mean, rstd, rms, acc, dw0, db0)
                    fails.exact(dw.view(1, -1), ref["dw"].float().view(1, -1), what + " dw onto nonzero")
                    fails.exact(db.view(1, -1), ref["db"].float().view(1, -1), what + " db onto nonzero")
                    fails.note("norm_bwd dx", fails.ulps(dx, ref["dx64"], 1, what + f" dx accum {acc is not None}", ref["dx_floor"]))
            # real statistics from the forward, random data
            x, dy, w = randn_bf(g, (rows, dim), 2.0, 0.5), randn_bf(g, (rows, dim)), mant15(g, (dim,))
            dw0, db0 = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
            for rms in (True, False):
                _, mean, rstd = K.norm_fwd(x, w, None, 1e-5 if rms else 1e-6, rms, True)
                ref = norm_bwd_ref(x, dy, w, mean, rstd, rms, dw0=dw0, db0=db0)
                dx, dw, db = K.norm_bwd(x, dy, w, mean, rstd, rms, None, dw0, db0)
                what = f"norm_bwd real {'rms' if rms else 'ln'} {rows}x{dim}"
                fails.note("norm_bwd dx", fails.ulps(dx, ref["dx64"], 1, what + " dx", ref["dx_floor"]))
                fails.note("norm_bwd dw", fails.abs(dw, ref["dw"], ref["dw_bound"], what + " dw"))
                fails.note("norm_bwd db", fails.abs(db, ref["db"], ref["db_bound"], what + " db"))


def suite_rope(fails, K, wrap=(1040, 64, 128, 347), table_S=2048):
    for hd in (8, 64, 72, 128):
        g = rng(300 + hd)
        S, nh = 7, 3
        cos, sin = K.rope_table(S, hd, 10000.0)
        for rows in (3 * S, 2 * S + 5):
            ld = nh * hd + 16
            qk = randn_bf(g, (rows, ld))
            qk[:, nh * hd:] = float("nan")
            for inv in (False, True):
                same_bits(fails, K.rope(qk, cos, sin, S, nh, hd, inv), rope_ref(qk, cos, sin, S, nh, hd, inv), f"rope hd {hd} rows {rows} S {S} inverse {inv}")
    rows, nh, hd, S = wrap                 # more than one trip of the grid-stride loop
    g = rng(399)
    cos, sin = K.rope_table(S, hd, 10000.0)
    qk = randn_bf(g, (rows, nh * hd))
    same_bits(fails, K.rope(qk, cos, sin, S, nh, hd, False), rope_ref(qk, cos, sin, S, nh, hd, False), f"rope wrap {rows}x{nh}x{hd}")
    for hd in (128, 72):
        cos, sin = K.rope_table(table_S, hd, 10000.0)
        c64, s64, floor = rope_table_ref(table_S, hd, 10000.0)
        fails.note("rope table", fails.ulps(cos, c64, 1, f"rope cos table S {table_S} hd {hd}", floor))
        fails.note("rope table", fails.ulps(sin, s64, 1, f"rope sin table S {table_S} hd {hd}", floor))


def _domain(fails, label, out, ref64, n, floor, z, what):
    """One activation output over the whole bf16 domain: finite wherever the float64 value is representable (+-inf or the largest bf16 where it
    is not), +-0 where float64 has underflowed to zero, within n ulps (+ floor) everywhere else."""
    o = out.detach().cpu().float().reshape(ref64.shape)
    over = ref64.abs() > BF_MAX
    fin = torch.isfinite(o)
    bad = ~fin & ~over
    fails.check(not bool(bad.any()), f"{what}: {int(bad.sum())} non-finite outputs; first at z = {z.flatten()[int(bad.flatten().nonzero()[0])].item() if bad.any() else 0:.6g}")
    fails.check(bool(((o.abs() >= BF_MAX) & (torch.sign(o) == torch.sign(ref64)))[over].all()), f"{what}: an overflowing product is not +-inf / the largest bf16")
    fails.check(bool((o[ref64 == 0] == 0).all()), f"{what}: nonzero output where the float64 value has underflowed to zero")
    keep = fin & ~over
    zero = torch.zeros_like(ref64)
    fails.note(label, fails.ulps(torch.where(keep, o.double(), zero).view(1, -1), torch.where(keep, ref64, zero).view(1, -1), n, what,
                                 None if floor is None else floor.view(1, -1)))


def suite_activations(fails, K):
    """act_bwd (acts 0 .. 4), swiglu_fwd and swiglu_bwd fed every finite bf16 bit pattern as z / g."""
    z = all_finite_bf16().view(8, -1)
    names = {0: "none", 1: "gelu", 2: "relu", 3: "silu", 4: "gelu_tanh"}
    for dhv in (1.0, -0.75):
        dh = torch.full(z.shape, dhv).to(BF)
        for act in range(5):
            ref, floor = act_bwd_ref(z, dh, act)
            _domain(fails, f"act_bwd {names[act]}", K.act_bwd(z, dh, act), ref, ULPS["dact1"], floor, z, f"act_bwd {names[act]} dh {dhv}")
        for uv in (1.0, -3.0):
            gu = torch.cat([z, torch.full(z.shape, uv).to(BF)], 1).contiguous()
            zz = torch.cat([z, z], 1)
            if dhv == 1.0:
                _domain(fails, "swiglu_fwd", K.swiglu_fwd(gu), swiglu_fwd_ref(gu), ULPS["swiglu"], None, z, f"swiglu_fwd u {uv}")
            _domain(fails, "swiglu_bwd", K.swiglu_bwd(gu, dh), swiglu_bwd_ref(gu, dh), ULPS["dact2"], None, zz, f"swiglu_bwd u {uv} dh {dhv}")


EDGE_CHUNKS = (1, 255, 256, 257)       # 8 elements; one chunk short of, exactly, and one chunk past one workgroup's 256 x 8


def suite_elementwise(fails, K):
    """add, colscale, copy_rows, vit_embed, gather_rows, the casts and transpose: bit-exact against torch fp32 arithmetic."""
    g = rng(400)
    for ch in EDGE_CHUNKS:
        a, b = randn_bf(g, (1, 8 * ch)), randn_bf(g, (1, 8 * ch))
        same_bits(fails, K.add(a, b), (a.float() + b.float()).to(BF), f"add {8 * ch}")
        same_bits(fails, K.add(a, None), a, f"add (copy) {8 * ch}")
        for dim in (8, 8 * ch):
            x, s = randn_bf(g, (8 * ch // dim, dim)), randn_bf(g, (dim,))
            same_bits(fails, K.colscale(x, s), (x.float() * s.float()[None]).to(BF), f"colscale {tuple(x.shape)}")
        f = torch.randn(8 * ch - 3, generator=g) * 10.0 ** torch.randint(-3, 4, (8 * ch - 3,), generator=g).float()
        for sc in (1.0, 0.37):
            same_bits(fails, K.cvt_f32_to_bf16(f, sc), (f * torch.tensor(sc, dtype=torch.float32)).to(BF), f"cvt f32 -> bf16 n {f.numel()} scale {sc}")
            same_bits(fails, K.cvt_bf16_to_f32(a[0, :8 * ch - 3], sc), a[0, :8 * ch - 3].float() * torch.tensor(sc, dtype=torch.float32), f"cvt bf16 -> f32 scale {sc}")
    for B, rows, dim in ((1, 1, 8), (2, 5, 264), (3, 51, 40)):
        Rs, Rd, sld, dld, sr0, dr0, dc0 = rows + 3, rows + 4, dim + 8, dim + 24, 2, 1, 8
        src = randn_bf(g, (B, Rs, sld))
        for accum in (False, True):
            dst = _sent((B, Rd, dld))
            if accum:
                dst[:, dr0:dr0 + rows, dc0:dc0 + dim] = randn_bf(g, (B, rows, dim))
            want = dst.clone()
            region = src[:, sr0:sr0 + rows, :dim].float()
            want[:, dr0:dr0 + rows, dc0:dc0 + dim] = ((region + dst[:, dr0:dr0 + rows, dc0:dc0 + dim].float()) if accum else region).to(BF)
            got = K.copy_rows(src, dst, B, rows, dim, src_batch_stride=Rs * sld, src_row0=sr0, src_ld=sld, dst_batch_stride=Rd * dld, dst_row0=dr0, dst_ld=dld, dst_col0=dc0, accumulate=accum)
            same_bits(fails, got, want, f"copy_rows B {B} rows {rows} dim {dim} accumulate {accum} (whole destination, guards included)")
    for dim in (8, 264):
        B, npatch, npre = 2, 5, 3
        patches, pos, prefix = randn_bf(g, (B * npatch, dim)), randn_bf(g, (npatch, dim)), randn_bf(g, (npre, dim))
        body = (patches.float().view(B, npatch, dim) + pos.float()[None]).to(BF)
        same_bits(fails, K.vit_embed(patches, pos, prefix, B, npatch, dim), torch.cat([prefix[None].expand(B, -1, -1), body], 1).reshape(-1, dim), f"vit_embed dim {dim}")
        same_bits(fails, K.vit_embed(patches, pos, None, B, npatch, dim), body.reshape(-1, dim), f"vit_embed dim {dim} no prefix")
        src = embed(randn_bf(g, (9, dim)), fill="nan")
        idx = torch.tensor([3, 8, 0, 7], dtype=torch.int32)
        dst = embed(BF, shape=(4, dim), fill="sentinel", device="cpu")
        want = dst.buf.clone()
        want[dst.r0:dst.r0 + 4, dst.c0:dst.c0 + dim] = src.view[idx.long()]
        same_bits(fails, K.gather_rows(src, idx, dim, dst, False), want, f"gather_rows dim {dim} (whole destination buffer)")
        upd = embed(randn_bf(g, (4, dim)), fill="nan")
        dst = embed(randn_bf(g, (9, dim)), fill="zero")
        dst.fill_guards("sentinel")
        want = dst.buf.clone()
        want[dst.r0 + idx.long(), dst.c0:dst.c0 + dim] = (dst.view[idx.long()].float() + upd.view.float()).to(BF)
        same_bits(fails, K.gather_rows(upd, idx, dim, dst, True), want, f"gather_rows scatter_add dim {dim} (whole destination buffer)")
    for rows in (1, 63, 64, 65, 130):
        for cols in (1, 63, 64, 65, 130):
            src = embed(randn_bf(g, (rows, cols)), align=4, fill="nan")
            dst = embed(BF, shape=(cols, rows), align=4, fill="sentinel", device="cpu")
            want = dst.buf.clone()
            want[dst.r0:dst.r0 + cols, dst.c0:dst.c0 + rows] = src.view.T
            same_bits(fails, K.transpose(src, dst), want, f"transpose {rows}x{cols} (whole destination buffer)")


NO_ROW_INDEX = (3, -1, 0, 7)


def suite_gather_no_row(fails, K):
    """gather_rows with an index < 0 ("no row": what ovla_assemble_multimodal leaves for an action slot the labels do not hold): the gather
    writes a ZERO row there, the scatter-add skips the entry.  `src` and `dst` are views inside larger allocations with three guard rows
    above them, so row -1 of either lies inside the same allocation whatever a kernel does with the index; the guards of the source hold
    NaN and those of the destination the sentinel, and whole destination buffers are compared bit for bit."""
    g = rng(410)
    idx = torch.tensor(NO_ROW_INDEX, dtype=torch.int32)
    keep = idx >= 0
    for dim in (8, 264):
        src = embed(randn_bf(g, (9, dim)), fill="nan")
        dst = embed(BF, shape=(4, dim), fill="sentinel", device="cpu")
        assert src.r0 >= 1 and dst.r0 >= 1
        rows = torch.zeros((4, dim), dtype=BF)
        rows[keep] = src.view[idx[keep].long()]
        want = dst.buf.clone()
        want[dst.r0:dst.r0 + 4, dst.c0:dst.c0 + dim] = rows
        same_bits(fails, K.gather_rows(src, idx, dim, dst, False), want, f"gather_rows index -1 dim {dim}: a zero row (whole destination buffer)")
        upd = embed(randn_bf(g, (4, dim)), fill="nan")
        dst = embed(randn_bf(g, (9, dim)), fill="zero")
        dst.fill_guards("sentinel")
        want = dst.buf.clone()
        want[dst.r0 + idx[keep].long(), dst.c0:dst.c0 + dim] = (dst.view[idx[keep].long()].float() + upd.view[keep].float()).to(BF)
        same_bits(fails, K.gather_rows(upd, idx, dim, dst, True), want, f"gather_rows scatter_add index -1 dim {dim}: entry skipped (whole destination buffer, guards included)")


WRAP_PARTS = ("add", "act_bwd", "colscale", "swiglu_fwd", "swiglu_bwd", "copy_rows", "vit_embed", "im2col", "cvt", "adamw_bf16", "adamw_f32")


def suite_wrap(fails, K, cap=GRID_CAP_ITEMS, adamw_cap=ADAMW_CAP_ITEMS, parts=WRAP_PARTS):
    """One case per kernel whose grid is capped (`parts`): work just over one trip of the grid-stride loop, with a tail that is no multiple of
    256.  Whole outputs are compared, on random data, so a shifted index shows."""
    g = rng(500)
    n = cap + 300
    assert n % 4 == 0 and set(parts) <= set(WRAP_PARTS)
    a, b = randn_bf(g, (1, 8 * n)), randn_bf(g, (1, 8 * n))
    B, rows = 4, n // 4
    if "add" in parts:
        same_bits(fails, K.add(a, b), (a.float() + b.float()).to(BF), f"add wrap {8 * n}")
    if "act_bwd" in parts:      # ReLU: exact, and a shifted index pairs a gradient with another element's sign
        same_bits(fails, K.act_bwd(a, b, 2), (b.float() * (a.float() > 0).float()).to(BF), f"act_bwd (relu) wrap {8 * n}")
    if "colscale" in parts:
        x, s = a.view(n // 4, 32), randn_bf(g, (32,))
        same_bits(fails, K.colscale(x, s), (x.float() * s.float()[None]).to(BF), f"colscale wrap {tuple(x.shape)}")
    if "swiglu_fwd" in parts or "swiglu_bwd" in parts:
        gu, dh = torch.cat([a.view(n // 4, 32), mant15(g, (n // 4, 32))], 1).contiguous(), mant15(g, (n // 4, 32))
        if "swiglu_fwd" in parts:
            fails.note("swiglu_fwd", fails.ulps(K.swiglu_fwd(gu), swiglu_fwd_ref(gu), ULPS["swiglu"], f"swiglu_fwd wrap {tuple(gu.shape)}"))
        if "swiglu_bwd" in parts:
            fails.note("swiglu_bwd", fails.ulps(K.swiglu_bwd(gu, dh), swiglu_bwd_ref(gu, dh), ULPS["dact2"], f"swiglu_bwd wrap {tuple(gu.shape)}"))
    if "copy_rows" in parts:
        src, dst = a.view(B, rows, 8), _sent((B, rows + 1, 16))
        want = dst.clone()
        want[:, 1:, 8:] = src
        same_bits(fails, K.copy_rows(src, dst, B, rows, 8, src_batch_stride=rows * 8, src_row0=0, src_ld=8, dst_batch_stride=(rows + 1) * 16, dst_row0=1, dst_ld=16, dst_col0=8, accumulate=False),
                  want, f"copy_rows wrap B {B} rows {rows}")
    if "vit_embed" in parts:
        npre, npatch = 3, rows - 3
        patches, pos, prefix = b.view(-1, 8)[:B * npatch], randn_bf(g, (npatch, 8)), randn_bf(g, (npre, 8))
        body = (patches.float().view(B, npatch, 8) + pos.float()[None]).to(BF)
        same_bits(fails, K.vit_embed(patches, pos, prefix, B, npatch, 8), torch.cat([prefix[None].expand(B, -1, -1), body], 1).reshape(-1, 8), f"vit_embed wrap B {B} tokens {rows}")
    if "im2col" in parts:
        px = randn_bf(g, (8, 6, 224, 224))
        cols = torch.nn.functional.unfold(px[:, 3:6].float(), kernel_size=14, stride=14).transpose(1, 2).reshape(8 * 256, 588).to(BF)
        same_bits(fails, K.im2col(px, 3, 14, 592), torch.cat([cols, torch.zeros(8 * 256, 4, dtype=BF)], 1), "im2col B 8 224x224 patch 14 ldo 592")
    if "cvt" in parts:
        f = torch.randn(cap + 77, generator=g)
        same_bits(fails, K.cvt_f32_to_bf16(f, 0.37), (f * torch.tensor(0.37, dtype=torch.float32)).to(BF), f"cvt f32 -> bf16 wrap {cap + 77}")
        same_bits(fails, K.cvt_bf16_to_f32(a[0, :cap + 77], 0.37), a[0, :cap + 77].float() * torch.tensor(0.37, dtype=torch.float32), f"cvt bf16 -> f32 wrap {cap + 77}")
    for dtype, part in ((BF, "adamw_bf16"), (torch.float32, "adamw_f32")):
        if part in parts:
            p, m, v, grad = adamw_inputs(g, adamw_cap + 77, dtype)
            hp = dict(step=3, lr=5e-4, weight_decay=0.01, grad_scale=0.37)
            for name, got, want in zip("pmv", K.adamw(p, m, v, grad, **hp), adamw_emulate(p, m, v, grad, **hp)):
                same_bits(fails, got, want, f"adamw wrap {dtype} n {adamw_cap + 77} {name}")


def suite_film_mean(fails, K):
    g = rng(600)
    for dim in (8, 264, 520):
        for rows in (1, 50):
            B = 3
            dy, xp = ints(g, (B * rows, dim), -4, 4, nonzero=True), ints(g, (B * rows, dim), -6, 6)
            gamma = choice(g, (B, dim), (-0.5, 0.0, 1.0, 3.0))
            dg0, db0 = ints(g, (B, dim), -5, 5, nonzero=True, dtype=torch.float32), ints(g, (B, dim), -5, 5, nonzero=True, dtype=torch.float32)
            want = film_bwd_ref(dy, xp, gamma, dg0, db0, B, rows)
            for name, got, ref in zip(("dy", "dgamma onto nonzero", "dbeta onto nonzero"), K.film_bwd(dy, xp, gamma, dg0, db0, B, rows), want):
                same_bits(fails, got, ref, f"film_bwd dim {dim} rows {rows} {name}")
        B, L = 3, 9
        x = ints(g, (B, L, dim), -8, 8)
        mask = torch.zeros((B, L), dtype=torch.uint8)
        mask[0, 4] = 1                       # count 1
        mask[1] = 1                          # count L; batch 2: all-zero mask -> zeros (pinned as it behaves now)
        same_bits(fails, K.masked_mean(x, mask, B, L, dim), masked_mean_ref(x, mask, B, L, dim), f"masked_mean dim {dim}")
        fails.check(bool((masked_mean_ref(x, mask, B, L, dim)[2] == 0).all()), "masked_mean reference: all-zero mask")


CE_VOCABS = (1, 8, 255, 256, 257, 1000)


def ce_rows(g, vocab):
    """Logit rows [R, ld] (ld = vocab rounded up to 8, + 8; padding columns hold +3e38 and NaN), targets, and the planted argmax of each row
    (-1: whatever the reference says)."""
    rows, want, inf_row = [], [], None

    def add(r, am=-1):
        rows.append(r)
        want.append(am)
    base = lambda: torch.randn(vocab, generator=g)  # noqa: E731
    add(base())
    r = base(); r[vocab // 2] = 16.0; add(r, vocab // 2)                                       # confident: loss ~ vocab e^-16
    r = base().clamp(max=8.0); r[0] = 9.0; add(r, 0)                                           # maximum at column 0
    r = base().clamp(max=8.0); r[vocab - 1] = 9.0; add(r, vocab - 1)                            # ... at vocab - 1
    add(torch.full((vocab,), 1.5), 0)                                                          # all equal
    if vocab >= 8:
        r = base(); r[1::2] = float("-inf"); add(r); inf_row = len(rows) - 1                   # -inf entries (its target: a finite column)
        r = base().clamp(max=8.0); r[5] = r[6] = 9.0; add(r, 5)                                # tie across lanes
    if vocab >= 255:
        r = base().clamp(max=8.0); r[67] = r[3] = 9.0; add(r, 3)                               # tie across waves (threads 3 and 67)
        r = base().clamp(max=8.0); r[130] = r[200] = r[253] = 9.0; add(r, 130)                 # ... waves 2 and 3
    if vocab > 256:
        r = base().clamp(max=8.0); r[256] = r[0] = 9.0; add(r, 0)                              # tie within one thread (j and j + 256)
        if vocab > 700:
            r = base().clamp(max=8.0); r[700] = r[444] = 9.0; add(r, 444)                      # thread 188: its first and second column
    R = len(rows)
    ld = -(-vocab // 8) * 8 + 8
    logits = torch.empty((R, ld), dtype=BF)
    logits[:, :vocab] = torch.stack(rows).to(BF)
    logits[:, vocab::2] = 3e38
    logits[:, vocab + 1::2] = float("nan")
    targets = torch.randint(0, vocab, (R,), generator=g)
    targets[0], targets[-1] = -1, vocab                                                        # clamped to 0 and vocab - 1
    if inf_row is not None:
        targets[inf_row] = 2 * (int(targets[inf_row]) // 2)
    if R > 2:
        targets[1] = vocab // 2                                                                # the confident row is right
    return logits, targets, torch.tensor(want, dtype=torch.int32)


def suite_token_ce(fails, K, big_vocab=32064):
    for vocab in CE_VOCABS + (big_vocab,):
        g = rng(700 + vocab)
        if vocab == big_vocab:
            r = torch.randn(vocab, generator=g)
            r[12345] = 16.0
            logits = torch.cat([r, torch.tensor([3e38, float("nan")] * 4)])[None].to(BF)
            targets, planted = torch.tensor([12345]), torch.tensor([12345], dtype=torch.int32)
        else:
            logits, targets, planted = ce_rows(g, vocab)
        gs = 2.0 ** -5
        ref = token_ce_ref(logits, targets, vocab, gs)
        what = f"token_ce vocab {vocab}"
        fails.check(bool(((planted < 0) | (planted == ref["argmax"])).all()), what + ": the reference does not find the planted argmax")
        loss, am, _ = K.token_ce(logits, targets, vocab, None, None)
        fails.note("token_ce loss", fails.abs(loss, ref["loss"], ref["loss_bound"], what + " loss"))
        fails.exact(am.view(1, -1), ref["argmax"].view(1, -1), what + " argmax (first maximum)")
        loss2, am2, d = K.token_ce(logits, targets, vocab, gs, _sent(logits.shape))
        same_bits(fails, loss2, loss, what + " loss with / without gradient")
        fails.note("token_ce grad", fails.ulps(d[:, :vocab].float(), ref["grad64"], 1, what + " gradient", ref["grad_floor"]))
        same_bits(fails, d[:, vocab:], _sent(logits.shape)[:, vocab:], what + " gradient padding untouched")
        loss3, am3, d_in = K.token_ce(logits, targets, vocab, gs, "inplace")
        same_bits(fails, d_in[:, :vocab], d[:, :vocab], what + " in-place gradient = out-of-place gradient")
        same_bits(fails, d_in[:, vocab:], logits[:, vocab:], what + " in-place: padding untouched")
        same_bits(fails, loss3, loss, what + " in-place loss")
        fails.exact(am3.view(1, -1), ref["argmax"].view(1, -1), what + " in-place argmax")
    # rows without a maximum: all -inf, only NaN -> column 0 (argmax_bins_kernel's rule)
    for vocab in (8, 257, 1000):
        logits = torch.zeros((3, vocab + 8), dtype=BF)
        logits[0, :vocab], logits[1, :vocab], logits[2, :vocab] = float("-inf"), float("nan"), 1.0
        logits[:, vocab:] = 3e38
        _, am, _ = K.token_ce(logits, torch.tensor([0, 1, 2]), vocab, None, None)
        fails.exact(am.view(1, -1), torch.zeros((1, 3), dtype=torch.int32), f"token_ce vocab {vocab}: argmax of all -inf / NaN / all-equal rows")


HEAD_DIMS, HEAD_ADIMS, HEAD_ROWS = (8, 264, 2048, 2056, 4096), (1, 7, 14, 16), (1, 5, 64)


def suite_head(fails, K, dims=HEAD_DIMS, adims=HEAD_ADIMS, rows_list=HEAD_ROWS):
    for dim in dims:
        for adim in adims:
            for rows in rows_list:
                g = rng(800 + dim + 17 * adim + rows)
                x, W, b, target = head_inputs(g, rows, dim, adim)
                scale = 2.0 ** -6
                dW0 = ints(g, (adim, dim), -5, 5, nonzero=True, dtype=torch.float32) * scale
                db0 = ints(g, (adim,), -5, 5, nonzero=True, dtype=torch.float32) * scale
                what = f"head dim {dim} adim {adim} rows {rows}"
                for mse in (False, True):
                    ref = head_ref(x, W, b, target, mse, scale=scale, loss0=17.0, dW0=dW0, db0=db0)
                    pred, loss = K.head_fwd(x, W, b, target, 17.0, mse)
                    fails.exact(pred, ref["pred"], what + f" pred mse {mse}")
                    same_bits(fails, loss, ref["loss_sum"], what + f" loss_sum onto 17 mse {mse}")
                    for name, got in zip(("dx", "dW", "db"), K.head_bwd(x, W, ref["pred"], target, scale, dW0, db0, mse, None)):
                        same_bits(fails, got, ref[name], what + f" fused backward mse {mse} {name}")
                fails.check(bool((head_ref(x, W, b, target, False, scale=scale)["dpred"] == 0).any()), what + ": no pred == target element")
                pred_nb, _ = K.head_fwd(x, W, None, None, None, False)
                fails.exact(pred_nb, head_ref(x, W, None, None, False)["pred"], what + " pred without bias / target")
                dpred = (ints(g, (rows, adim), -2, 2).float() * 0.125).to(BF)
                ref = head_ref(x, W, b, None, False, dW0=dW0, db0=db0, dpred=dpred)
                for name, got in zip(("dx", "dW", "db"), K.head_bwd(x, W, None, None, 0.0, dW0, db0, False, dpred)):
                    same_bits(fails, got, ref[name], what + f" explicit dpred {name}")


def suite_adamw(fails, K, n=2048 + 77, dtypes=(BF, torch.float32)):
    for dtype in dtypes:
        g = rng(900)
        p0, m0, v0, _ = adamw_inputs(g, n, dtype)
        grads = {step: adamw_inputs(g, n, dtype)[3] for step in ADAMW_STEPS}
        for lr, wd, gs, b2, eps in ADAMW_GRID:
            for step in ADAMW_STEPS:
                hp = dict(step=step, lr=lr, beta2=b2, eps=eps, weight_decay=wd, grad_scale=gs)
                want = adamw_emulate(p0, m0, v0, grads[step], **hp)
                for name, got, ref in zip("pmv", K.adamw(p0, m0, v0, grads[step], **hp), want):
                    same_bits(fails, got, ref, f"adamw {dtype} lr {lr} wd {wd} grad_scale {gs} beta2 {b2} eps {eps} step {step}: {name}")
        # the edge blocks do what they are there for
        p1, m1, v1 = adamw_emulate(p0, m0, v0, grads[1], step=1, lr=5e-4, weight_decay=0.0)
        q = n // 8
        fails.check(torch.equal(p1[:q], p0[:q]) and bool((v1[:q] == 0).all()), "adamw: zero gradient with zero state must leave the parameter (denominator = eps)")
        if dtype == BF:
            fails.check(bool((p1[q:2 * q] == p0[q:2 * q]).float().mean() > 0.9), "adamw: the large parameters' updates should be below half an ulp")


# ---- the real kernels behind the suites' interface ---------------------------------------------------------------------------------------------
class GpuKernels:
    """The suites' K for the real library: CPU tensors in, launches through `ops` on `dev`, CPU tensors out.  Every output a wrapper lets the
    caller place sits in a guarded buffer (Guarded / gemm_reference.embed) whose guards are checked after the launch."""

    def __init__(self, ops, dev, fails):
        self.ops, self.dev, self.fails = ops, dev, fails

    def _d(self, t):
        return None if t is None else t.to(self.dev)

    def _out(self, dtype, shape, launch, what):
        o = Guarded(dtype, tuple(shape), self.dev)
        launch(o.view)
        try:
            o.assert_guards(what)
        except AssertionError as e:
            self.fails.append(str(e))
        return o.view.cpu()

    def norm_fwd(self, x, w, b, eps, rms, save):
        st = {}

        def launch(out):
            _, st["mean"], st["rstd"] = self.ops.norm_fwd(self._d(x), self._d(w), self._d(b), eps=eps, rms=rms, out=out, save_stats=save)
        y = self._out(BF, x.shape, launch, f"norm_fwd {tuple(x.shape)}")
        return y, None if st["mean"] is None else st["mean"].cpu(), None if st["rstd"] is None else st["rstd"].cpu()

    def norm_bwd(self, x, dy, w, mean, rstd, rms, dx0, dw0, db0):
        dw, db = Guarded(torch.float32, dw0.shape, self.dev), Guarded(torch.float32, db0.shape, self.dev)
        dw.view.copy_(dw0), db.view.copy_(db0)

        def launch(out):
            if dx0 is not None:
                out.copy_(dx0)
            self.ops.norm_bwd(self._d(x), self._d(dy), self._d(w), self._d(mean), self._d(rstd), rms=rms, dx=out, dx_accum=dx0 is not None, dweight=dw.view, dbias=db.view)
        dx = self._out(BF, x.shape, launch, f"norm_bwd dx {tuple(x.shape)}")
        for o, name in ((dw, "dw"), (db, "db")):
            try:
                o.assert_guards(f"norm_bwd {name} {tuple(x.shape)}")
            except AssertionError as e:
                self.fails.append(str(e))
        return dx, dw.view.cpu(), db.view.cpu()

    def rope_table(self, S, hd, theta):
        cos, sin = self.ops.rope_table(S, hd, theta, self.dev)
        return cos.cpu(), sin.cpu()

    def rope(self, qk, cos, sin, S, nh, hd, inverse):
        e = embed(qk.to(self.dev), align=4, fill="zero")
        e.fill_guards("sentinel")
        self.ops.rope_(e.view, S, nh, hd, self._d(cos), self._d(sin), inverse=inverse)
        try:
            e.assert_guards(f"rope {tuple(qk.shape)} hd {hd}")
        except AssertionError as err:
            self.fails.append(str(err))
        return e.view.cpu()

    def act_bwd(self, z, dh, act):
        return self._out(BF, z.shape, lambda o: self.ops.act_bwd(self._d(z), self._d(dh), act, out=o), f"act_bwd {tuple(z.shape)}")

    def swiglu_fwd(self, gu):
        return self._out(BF, (gu.shape[0], gu.shape[1] // 2), lambda o: self.ops.swiglu_fwd(self._d(gu), out=o), f"swiglu_fwd {tuple(gu.shape)}")

    def swiglu_bwd(self, gu, dh):
        return self._out(BF, gu.shape, lambda o: self.ops.swiglu_bwd(self._d(gu), self._d(dh), out=o), f"swiglu_bwd {tuple(gu.shape)}")

    def add(self, a, b):
        return self._out(BF, a.shape, lambda o: self.ops.add(self._d(a), self._d(b), out=o), f"add {tuple(a.shape)}")

    def colscale(self, x, s):
        return self._out(BF, x.shape, lambda o: self.ops.colscale(self._d(x), self._d(s), out=o), f"colscale {tuple(x.shape)}")

    def cvt_f32_to_bf16(self, f, scale):
        return self._out(BF, f.shape, lambda o: self.ops.cvt_f32_to_bf16(self._d(f), dst=o, scale=scale), f"cvt_f32_to_bf16 {f.numel()}")

    def cvt_bf16_to_f32(self, x, scale):
        return self._out(torch.float32, x.shape, lambda o: self.ops.cvt_bf16_to_f32(self._d(x).contiguous(), dst=o, scale=scale), f"cvt_bf16_to_f32 {x.numel()}")

    def copy_rows(self, src, dst, B, rows, dim, **kw):
        d = dst.to(self.dev)
        self.ops.copy_rows(self._d(src), d, B, rows, dim, **kw)
        return d.cpu()

    def vit_embed(self, patches, pos, prefix, B, npatch, dim):
        ntok = npatch + (0 if prefix is None else prefix.shape[0])
        return self._out(BF, (B * ntok, dim), lambda o: self.ops.vit_embed(self._d(patches).contiguous(), self._d(pos), self._d(prefix), B, npatch, dim, out=o), f"vit_embed dim {dim}")

    def im2col(self, px, c0, patch, kp):
        return self.ops.im2col(self._d(px), c0, patch, kp).cpu()

    def gather_rows(self, src, idx, dim, dst, scatter_add):
        s, d = Embedded(src.buf.to(self.dev), src.r0, src.c0, src.rows, src.cols), Embedded(dst.buf.to(self.dev), dst.r0, dst.c0, dst.rows, dst.cols)
        self.ops.gather_rows(s.view, self._d(idx), dim, dst=d.view, scatter_add=scatter_add)
        return d.buf.cpu()

    def transpose(self, src, dst):
        s, d = Embedded(src.buf.to(self.dev), src.r0, src.c0, src.rows, src.cols), Embedded(dst.buf.to(self.dev), dst.r0, dst.c0, dst.rows, dst.cols)
        self.ops.transpose(s.view, d.view)
        return d.buf.cpu()

    def film_bwd(self, dy, xp, gamma, dg0, db0, B, rows):
        dg, db = Guarded(torch.float32, dg0.shape, self.dev), Guarded(torch.float32, db0.shape, self.dev)
        dg.view.copy_(dg0), db.view.copy_(db0)
        out = self._out(BF, dy.shape, lambda o: (o.copy_(dy), self.ops.film_bwd(o, self._d(xp), self._d(gamma), dg.view, db.view, B, rows)), f"film_bwd {tuple(dy.shape)}")
        for o in (dg, db):
            try:
                o.assert_guards(f"film_bwd dgamma / dbeta {tuple(dy.shape)}")
            except AssertionError as e:
                self.fails.append(str(e))
        return out, dg.view.cpu(), db.view.cpu()

    def masked_mean(self, x, mask, B, L, dim):
        return self.ops.masked_mean(self._d(x), self._d(mask), B, L, dim).cpu()

    def token_ce(self, logits, targets, vocab, grad_scale, dst):
        lg = logits.to(self.dev)
        d = dst.to(self.dev) if torch.is_tensor(dst) else None
        loss, am, out = self.ops.token_ce(lg, self._d(targets), vocab=vocab, grad_scale=grad_scale, inplace_grad=(isinstance(dst, str)), dlogits=d)
        if torch.is_tensor(dst):
            same_bits(self.fails, lg.cpu(), logits, f"token_ce vocab {vocab}: the out-of-place run changed its input")
        return loss.cpu(), am.cpu(), None if out is None else out.cpu()

    def head_fwd(self, x, W, b, target, loss0, mse):
        ls = None
        if loss0 is not None:
            ls = Guarded(torch.float32, (1,), self.dev)
            ls.view.fill_(loss0)
        pred = self._out(BF, (x.shape[0], W.shape[0]), lambda o: self.ops.head_out_fwd(self._d(x), self._d(W), self._d(b), self._d(target), None if ls is None else ls.view, mse=mse, out=o),
                         f"head_out_fwd {tuple(x.shape)} adim {W.shape[0]}")
        if ls is not None:
            try:
                ls.assert_guards("head_out_fwd loss_sum")
            except AssertionError as e:
                self.fails.append(str(e))
        return pred, None if ls is None else ls.view.cpu()

    def head_bwd(self, x, W, pred, target, scale, dW0, db0, mse, dpred):
        dW, db = Guarded(torch.float32, dW0.shape, self.dev), Guarded(torch.float32, db0.shape, self.dev)
        dW.view.copy_(dW0), db.view.copy_(db0)
        dx = self._out(BF, x.shape, lambda o: self.ops.head_out_bwd(self._d(x), self._d(W), self._d(pred), self._d(target), scale, dW.view, db.view, mse=mse, dpred=self._d(dpred), out=o),
                       f"head_out_bwd {tuple(x.shape)} adim {W.shape[0]}")
        for o in (dW, db):
            try:
                o.assert_guards(f"head_out_bwd dW / db {tuple(x.shape)}")
            except AssertionError as e:
                self.fails.append(str(e))
        return dx, dW.view.cpu(), db.view.cpu()

    def adamw(self, p, m, v, g, **hp):
        bufs = [Guarded(p.dtype, p.shape, self.dev) for _ in range(3)]
        for o, t in zip(bufs, (p, m, v)):
            o.view.copy_(t)
        self.ops.adamw(bufs[0].view, bufs[1].view, bufs[2].view, self._d(g), **hp)
        for o in bufs:
            try:
                o.assert_guards(f"adamw n {p.numel()}")
            except AssertionError as e:
                self.fails.append(str(e))
        return tuple(o.view.cpu() for o in bufs)
