"""The checks of tests/pointwise_reference.py discriminate (no GPU).

`Emulated` restates every kernel of csrc/elementwise.hip and csrc/head_optim.hip that the two GPU files test -- in fp32 on the CPU, with the
bf16 rounding points of the kernels' comments -- behind the interface the suites drive (`K`).  The GPU files hand the same suites the real
launches; here

* the correct emulation passes every suite, at every shape of the GPU files (the grid-stride cases at a cap of 1024 / 2048 work items instead
  of 1,048,576 / 2,097,152: the same suite, sampled);
* each planted bug (`MUTATIONS`) is rejected, by the check meant to catch it;
* for each bug the old `close()` of tests/test_kernels_gpu.py (max|err| <= 1.5e-2 max|ref| and mean|err| <= 2.5e-3 max|ref|, per tensor) is
  asked about the very same outputs, with the unmutated emulation as its reference; the verdicts are pinned in `OLD_CLOSE_ACCEPTS` and printed;
* an error of ten times any derived bound is rejected (`test_ten_times_a_bound_is_rejected`), and each bound's size is pinned where a term of it matters, so a bound multiplied by 20 fails this file.
"""
import pytest
import torch

from tests import pointwise_reference as P

BF = torch.bfloat16


def _r(x):
    return x.to(BF).float()


def _t(x):          # fp32 -> bf16 by truncation
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _exp(x):        # __expf: overflows to inf and underflows to 0 where fp32 does
    return torch.exp(x.double()).float()


def _f(v):
    return torch.tensor(v, dtype=torch.float32)


def fast_erf(x):
    ax = x.abs()
    t = 1.0 / (1.0 + _f(0.3275911) * ax)
    poly = t * (_f(0.254829592) + t * (_f(-0.284496736) + t * (_f(1.421413741) + t * (_f(-1.453152027) + t * _f(1.061405429)))))
    return torch.copysign(1.0 - poly * _exp(-ax * ax), x)


def act_grad32(z, act, tanh_clamp=True, tail=True):
    if act == 1:
        cdf = 0.5 * (1.0 + fast_erf(z * _f(0.70710678118654752440)))
        return cdf + z * (_f(0.39894228040143267794) * _exp(-0.5 * z * z))
    if act == 2:
        return (z > 0).float()
    if act == 3:
        s = P.sigmoid_f32(z, tail)
        return s * (1.0 + z * (1.0 - s))
    if act == 4:
        return P.gelu_tanh_grad_f32(z, tanh_clamp, tail)
    return torch.ones_like(z)


class Emulated:
    """fp32 restatements of the kernels, CPU tensors in and out.  `mut` plants one bug; `cap` / `adamw_cap` are the work items one trip of a
    grid-stride loop covers (the real kernels: 1,048,576 and 2,097,152)."""

    def __init__(self, mut=None, cap=1024, adamw_cap=2048):
        self.mut, self.cap, self.adamw_cap = mut, cap, adamw_cap

    def _store(self, v):
        return (_t(v) if self.mut == "truncate" else v).to(BF)

    def _trips(self, full, stale, item, cap=None):
        """What a grid-stride kernel leaves: everything, or (mutation) only the first `cap` work items of `item` elements each."""
        if self.mut != "one_trip":
            return full
        out = stale.clone().flatten()
        k = (cap or self.cap) * item
        out[:k] = full.flatten()[:k]
        return out.view(full.shape)

    # ---- norms ----
    def _live(self, dim):
        live = torch.ones(dim // 8, dtype=torch.bool)
        if self.mut == "drop_last_chunk":
            live[-1] = False
        if self.mut == "drop_slot3_lane0" and dim // 8 > 128 and P.norm_lanes(dim) == 64:
            live[128] = False                                    # lane 0 of the third register slot
        return live.repeat_interleave(8)

    def norm_fwd(self, x, w, b, eps, rms, save):
        xf, wf = x.float(), w.float()
        rows, dim = xf.shape
        live = self._live(dim)
        m = live.float()[None]
        mean = torch.zeros(rows) if rms else (xf * m).sum(-1) / dim
        d = xf if self.mut == "no_mean_in_var" else xf - mean[:, None]
        rstd = torch.rsqrt((d * d * m).sum(-1) / dim + _f(eps))
        if rms:
            y = wf[None] * _r(xf * rstd[:, None])
        else:
            bf = b.float()[None].expand(rows, dim) if b is not None else torch.zeros(rows, dim)
            y = P.fma32(((xf - mean[:, None]) * rstd[:, None]).contiguous(), wf[None].expand(rows, dim).contiguous(), bf.contiguous())
        y = self._store(y)
        if self.mut == "drop_last_chunk":
            y[:, ~live] = 0.0
        return y, (mean if save and not rms else None), (rstd if save else None)

    def norm_bwd(self, x, dy, w, mean, rstd, rms, dx0, dw0, db0):
        xf, g0, wf = x.float(), dy.float(), w.float()
        rows, dim = xf.shape
        mu = torch.zeros(rows) if rms else mean.float()
        xhat = (xf - mu[:, None]) * rstd[:, None]
        g = g0 * wf[None]
        m1 = torch.zeros(rows) if rms else g.sum(-1) / dim
        m2 = (g * xhat).sum(-1) / dim
        v = rstd[:, None] * (g - m1[:, None] - xhat * m2[:, None])
        dx = self._store(v if dx0 is None else dx0.float() + v)
        sw, sb = (g0 * xhat).sum(0), g0.sum(0)
        if self.mut == "assign":
            return dx, sw, sb
        return dx, dw0 + sw, db0 + sb

    # ---- RoPE ----
    def rope_table(self, S, hd, theta):
        half = hd // 2
        e = (torch.arange(half, dtype=torch.float32) * 2.0) / _f(float(hd))
        inv = 1.0 / torch.pow(_f(theta), e)
        ang = torch.arange(S, dtype=torch.float32)[:, None] * inv[None]
        return torch.cos(ang).to(BF), torch.sin(ang).to(BF)

    def rope(self, qk, cos, sin, S, nh, hd, inverse):
        rows, half = qk.shape[0], hd // 2
        pos = torch.arange(rows) % S
        if self.mut == "rope_pos_row":
            pos = torch.arange(rows)
            cos, sin = self.rope_table(rows, hd, 10000.0)        # the table the kernel would have run off
        c = cos.float()[pos][:, None, :]
        s = sin.float()[pos][:, None, :] * (-1.0 if inverse else 1.0)
        x = qk[:, :nh * hd].float().view(rows, nh, hd)
        a, b = x[..., :half], x[..., half:]
        if self.mut == "rope_partner4":
            b = torch.roll(b, -4, -1)
        lo, hi = _r(a * c) + _r(-b * s), _r(b * c) + _r(a * s)
        full = self._store(torch.cat([lo, hi], -1)).view(rows, nh * hd)
        out = qk.clone()
        if self.mut == "one_trip":                               # work item = (row, head, 4-column chunk of a half head)
            keep = (torch.arange(rows * nh * (hd // 8)) < self.cap).view(rows, nh, hd // 8).repeat_interleave(4, -1)
            full = torch.where(torch.cat([keep, keep], -1).view(rows, nh * hd), full, qk[:, :nh * hd])
        out[:, :nh * hd] = full
        return out

    # ---- activations ----
    def act_bwd(self, z, dh, act):
        full = self._store(dh.float() * act_grad32(z.float(), act, tanh_clamp=self.mut != "gelu_tanh_old", tail=self.mut != "sigmoid_no_tail"))
        return self._trips(full, torch.zeros_like(full), 8)

    def swiglu_fwd(self, gu):
        F = gu.shape[1] // 2
        g, u = gu[:, :F].float(), gu[:, F:].float()
        full = self._store(_r(P.silu_f32(g, self.mut != "sigmoid_no_tail")) * u)
        return self._trips(full, torch.zeros_like(full), 8)

    def swiglu_bwd(self, gu, dh):
        F = gu.shape[1] // 2
        g, u, d = gu[:, :F].float(), gu[:, F:].float(), dh.float()
        s = P.sigmoid_f32(g, self.mut != "sigmoid_no_tail")
        dg, du = d * u * (s * (1.0 + g * (1.0 - s))), d * _r(g * s)
        full = self._store(torch.cat([dg, du], 1))
        if self.mut != "one_trip":
            return full
        keep = (torch.arange(gu.shape[0] * (F // 8)) < self.cap).view(gu.shape[0], F // 8).repeat_interleave(8, 1)
        return torch.where(torch.cat([keep, keep], 1), full, torch.zeros_like(full))

    # ---- copies and casts ----
    def add(self, a, b):
        full = self._store(a.float() + b.float()) if b is not None else self._store(a.float())
        return self._trips(full, torch.zeros_like(full), 8)

    def colscale(self, x, s):
        full = self._store(x.float() * s.float()[None])
        return self._trips(full, torch.zeros_like(full), 8)

    def cvt_f32_to_bf16(self, f, scale):
        full = self._store(f * _f(scale))
        return self._trips(full, torch.zeros_like(full), 1)

    def cvt_bf16_to_f32(self, x, scale):
        full = x.float() * _f(scale)
        return self._trips(full, torch.zeros_like(full), 1)

    def copy_rows(self, src, dst, B, rows, dim, *, src_batch_stride, src_row0, src_ld, dst_batch_stride, dst_row0, dst_ld, dst_col0, accumulate):
        out = dst.clone()
        region = src[:, src_row0:src_row0 + rows, :dim].float()
        cur = out[:, dst_row0:dst_row0 + rows, dst_col0:dst_col0 + dim]
        full = self._store(region + cur.float() if accumulate else region)
        out[:, dst_row0:dst_row0 + rows, dst_col0:dst_col0 + dim] = self._trips(full, cur.contiguous(), 8)
        return out

    def vit_embed(self, patches, pos, prefix, B, npatch, dim):
        body = self._store(patches.float().view(B, npatch, dim) + pos.float()[None])
        full = (body if prefix is None else torch.cat([prefix[None].expand(B, -1, -1), body], 1)).reshape(-1, dim)
        return self._trips(full, torch.zeros_like(full), 8)

    def im2col(self, px, c0, patch, kp):
        B, _, H, W = px.shape
        cols = torch.nn.functional.unfold(px[:, c0:c0 + 3].float(), kernel_size=patch, stride=patch).transpose(1, 2).reshape(-1, 3 * patch * patch).to(BF)
        full = torch.cat([cols, torch.zeros(cols.shape[0], kp - cols.shape[1], dtype=BF)], 1)
        return self._trips(full, torch.full_like(full, 7.0), 1)

    def gather_rows(self, src, idx, dim, dst, scatter_add):
        out = dst.buf.clone()
        r0, c0 = dst.r0, dst.c0
        if self.mut == "gather_no_skip":       # the index taken as it comes: row -1 is the guard row above the view (inside the allocation)
            if scatter_add:
                rows = r0 + idx.long()
                out[rows, c0:c0 + dim] = self._store(dst.buf[rows, c0:c0 + dim].float() + src.view.float())
            else:
                out[r0:r0 + idx.numel(), c0:c0 + dim] = src.buf[src.r0 + idx.long(), src.c0:src.c0 + dim]
            return out
        keep = idx >= 0                        # an index < 0 is "no row": a zero row on gather, skipped on scatter-add
        ok = idx[keep].long()
        if scatter_add:
            out[r0 + ok, c0:c0 + dim] = self._store(dst.view[ok].float() + src.view[keep].float())
        else:
            rows = torch.zeros((idx.numel(), dim), dtype=BF)
            rows[keep] = src.view[ok]
            out[r0:r0 + idx.numel(), c0:c0 + dim] = rows
        return out

    def transpose(self, src, dst):
        out = dst.buf.clone()
        out[dst.r0:dst.r0 + dst.rows, dst.c0:dst.c0 + dst.cols] = src.view.T
        return out

    # ---- FiLM, masked mean ----
    def film_bwd(self, dy, xp, gamma, dg0, db0, B, rows):
        dim = dy.shape[1]
        d, x = dy.float().view(B, rows, dim), xp.float().view(B, rows, dim)
        one_plus = _r(1.0 + gamma.float())
        out = self._store(d * one_plus[:, None]).view(B * rows, dim)
        sg, sb = (d * x).sum(1), d.sum(1)
        return (out, sg, sb) if self.mut == "assign" else (out, dg0 + sg, db0 + sb)

    def masked_mean(self, x, mask, B, L, dim):
        return P.masked_mean_ref(x, mask, B, L, dim)

    # ---- token cross-entropy ----
    def token_ce(self, logits, targets, vocab, grad_scale, dst):
        x = logits[:, :vocab].float()
        R = x.shape[0]
        tgt = targets.clamp(0, vocab - 1)
        gt = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)           # `v > m` never holds for NaN
        m = gt.max(-1).values
        hit = (x == m[:, None]) & (m > float("-inf"))[:, None]
        first = torch.where(hit.any(-1), hit.float().argmax(-1), torch.full((R,), 0 if self.mut != "ce_no_clamp" else 0x7FFFFFFF))
        if self.mut == "last_max":
            first = torch.where(hit.any(-1), vocab - 1 - hit.flip(-1).float().argmax(-1), first)
        e = _exp(x - m[:, None])
        s = e.sum(-1)
        loss = (torch.log(s.double()).float() + m) - x.gather(1, tgt[:, None])[:, 0]
        d = None
        if grad_scale is not None:
            p = e * (1.0 / s)[:, None]
            if self.mut != "no_minus_one":
                p = p - torch.zeros_like(p).scatter_(1, tgt[:, None], 1.0)
            d = (logits if isinstance(dst, str) else dst).clone()
            d[:, :vocab] = self._store(p * _f(grad_scale))
        return loss, first.to(torch.int32), d

    # ---- head output ----
    def head_fwd(self, x, W, b, target, loss0, mse):
        v = _r(x.float() @ W.float().T + (b.float() if b is not None else 0.0))
        if loss0 is None:
            return self._store(v), None
        d = _r(target.float() - v)
        total = (_r(d * d) if mse else d.abs()).sum()
        return self._store(v), (total if self.mut == "assign" else _f(loss0) + total).view(1)

    def head_bwd(self, x, W, pred, target, scale, dW0, db0, mse, dpred):
        if dpred is None:
            d = _r(pred.float() - target.float())
            dp = _r(_r(2.0 * d * _f(scale))) if mse else _r(torch.sign(d) * _f(scale))
        else:
            dp = dpred.float()
        dx = self._store(dp @ W.float() + 0.0)          # the kernel's sum starts from +0
        gW, gb = dp.T @ x.float(), dp.sum(0)
        return (dx, gW, gb) if self.mut == "assign" else (dx, dW0 + gW, db0 + gb)

    # ---- AdamW ----
    def adamw(self, p, m, v, g, **hp):
        mut = {"adamw_fma": "fma", "adamw_no_grad_scale": "no_grad_scale"}.get(self.mut)
        new = P.adamw_emulate(p, m, v, g, mut=mut, **hp)
        return tuple(self._trips(n, o, 1, self.adamw_cap) for n, o in zip(new, (p, m, v)))


SUITES = {
    "norm_fwd": lambda f, K: P.suite_norm_fwd(f, K),
    "norm_bwd": lambda f, K: P.suite_norm_bwd(f, K),
    "rope": lambda f, K: P.suite_rope(f, K, wrap=(9, 16, 128, 4)),
    "activations": lambda f, K: P.suite_activations(f, K),
    "elementwise": lambda f, K: P.suite_elementwise(f, K),
    "wrap": lambda f, K: P.suite_wrap(f, K, cap=K.cap, adamw_cap=K.adamw_cap),
    "film_mean": lambda f, K: P.suite_film_mean(f, K),
    "token_ce": lambda f, K: P.suite_token_ce(f, K),
    "head": lambda f, K: P.suite_head(f, K),
    "adamw": lambda f, K: P.suite_adamw(f, K),
    "gather_no_row": lambda f, K: P.suite_gather_no_row(f, K),
}


@pytest.mark.parametrize("suite", list(SUITES))
def test_emulation_passes_every_check(suite):
    fails = P.Checks()
    P.Checks.worst = {}
    SUITES[suite](fails, Emulated())
    fails.done()
    print(f"{suite}: emulation, worst |err| / bound:", " ".join(f"[{k}] {v:.2f}" for k, v in sorted(P.Checks.worst.items())))
    assert all(v <= 1.0 for v in P.Checks.worst.values())


# mutation -> (what is planted, the reduced suite run that must reject it, a phrase of each check meant to catch it: all of them must have failed)
MUTATIONS = {
    "assign_norm": ("`=` for `+=` in norm_dwdb_kernel", "assign", lambda f, K: P.suite_norm_bwd(f, K, dims=(520,), rows_list=(3,)), "dw onto nonzero"),
    "assign_head": ("`=` for `+=` in head_out_bwd / atomicAdd(loss_sum)", "assign", lambda f, K: P.suite_head(f, K, dims=(264,), adims=(7,), rows_list=(5,)), "loss_sum onto 17"),
    "assign_film": ("`=` for atomicAdd(dgamma / dbeta)", "assign", lambda f, K: P.suite_film_mean(f, K), "dgamma onto nonzero"),
    "one_trip": ("a grid-stride loop that stops after one trip", "one_trip", SUITES["wrap"],
                 ("add wrap", "act_bwd (relu) wrap", "colscale wrap", "swiglu_fwd wrap", "swiglu_bwd wrap", "copy_rows wrap", "vit_embed wrap", "im2col B 8", "cvt f32 -> bf16 wrap",
                  "cvt bf16 -> f32 wrap", "adamw wrap torch.bfloat16", "adamw wrap torch.float32")),
    "one_trip_rope": ("... in rope_kernel", "one_trip", SUITES["rope"], "rope wrap"),
    "drop_last_chunk": ("the last 8-element chunk of a row dropped", "drop_last_chunk", lambda f, K: P.suite_norm_fwd(f, K, dims=(520,), rows_list=(3,)),
                        ("norm_fwd rms 3x520 bias False stats True rstd", "norm_fwd ln 3x520 bias True stats True mean", "norm_fwd ln 3x520 bias True stats False: ")),
    "drop_slot3_lane0": ("the chunk at lane 0 of the third register slot dropped (dim 1032)", "drop_slot3_lane0", lambda f, K: P.suite_norm_fwd(f, K, dims=(1032,), rows_list=(5,)), "5x1032 bias False stats True rstd"),
    "no_mean_in_var": ("mean not subtracted in the variance", "no_mean_in_var", lambda f, K: P.suite_norm_fwd(f, K, dims=(512,), rows_list=(4,)), "rstd"),
    "rope_partner4": ("RoPE partner column off by 4", "rope_partner4", SUITES["rope"], "rope hd"),
    "rope_pos_row": ("RoPE position taken as row instead of row % S", "rope_pos_row", SUITES["rope"], "rope hd"),
    "truncate": ("a truncating bf16 store", "truncate", SUITES["elementwise"], "add 8"),
    "last_max": ("argmax taking the last maximum instead of the first", "last_max", SUITES["token_ce"], "argmax (first maximum)"),
    "no_minus_one": ("CE gradient missing the - 1 at the target", "no_minus_one", SUITES["token_ce"], "gradient"),
    "ce_no_clamp": ("0x7fffffff left in argmax for a row without a maximum", "ce_no_clamp", SUITES["token_ce"], "all -inf / NaN"),
    "adamw_fma": ("AdamW with one fused multiply-add where the sequence has two roundings", "adamw_fma", lambda f, K: P.suite_adamw(f, K, n=512 + 77), "adamw torch.float32"),
    "adamw_no_grad_scale": ("AdamW ignoring grad_scale", "adamw_no_grad_scale", lambda f, K: P.suite_adamw(f, K, n=512 + 77), "grad_scale 0.37"),
    "sigmoid_no_tail": ("the sigmoid family without its tail: 0 from z = -88.7 on, where the value is still 1e-39 ... 4e-37", "sigmoid_no_tail", SUITES["activations"], "act_bwd silu dh 1.0: "),
    "gather_no_skip": ("gather_rows taking an index of -1 as a row: the row before the buffer", "gather_no_skip", SUITES["gather_no_row"],
                       ("gather_rows index -1", "gather_rows scatter_add index -1")),
    "gelu_tanh_old": ("gelu_tanh_grad with an unclamped polynomial factor: NaN at z = -1e19", "gelu_tanh_old", SUITES["activations"], "act_bwd gelu_tanh dh 1.0: "),
}
# What the old close() says when it is shown the same outputs.  It ACCEPTS a dropped register slot (rstd 0.4 % off: y stays inside 1.5e-2), a
# truncating store (at most one bf16 ulp, 7.8e-3 of the element), the fused multiply-add in AdamW (last-bit differences) and the sigmoid family
# returning 0 where the value is 1e-37 (nothing against max|ref| = 1).  It rejects what leaves stale elements behind, NaN, or an error of the size
# of the data -- where it is run at that shape, which for the wrap cases, most norm dims, RoPE's other head_dims, nonzero accumulators, rows
# without a maximum and inputs beyond +-6 it never was.  (An integer argmax was compared exactly by the old test too; it had one tie, across lanes.)
OLD_CLOSE_ACCEPTS = {"drop_slot3_lane0", "truncate", "adamw_fma", "sigmoid_no_tail"}
OLD_COMPARED = {"norm_fwd": (0,)}      # of a kernel's outputs, those the old tests compared with anything (default: all): mean / rstd never were


def old_close(out, ref, tol=1.5e-2, mean_tol=2.5e-3):
    out, ref = out.double(), ref.double()
    if not torch.isfinite(out[torch.isfinite(ref)]).all():
        return False
    ok = torch.isfinite(ref) & torch.isfinite(out)
    if not ok.any():
        return True
    scale = ref[ok].abs().max().item() + 1e-12
    err = (out - ref)[ok].abs()
    return err.max().item() / scale <= tol and err.mean().item() / scale <= mean_tol


class Both:
    """Runs the mutated and the clean emulation side by side; hands the suite the mutated outputs and keeps every (mutated, clean) pair of
    tensors for the old check."""

    def __init__(self, mut, **kw):
        self.bad, self.good, self.pairs = Emulated(mut, **kw), Emulated(None, **kw), []
        self.cap, self.adamw_cap = self.bad.cap, self.bad.adamw_cap

    def __getattr__(self, name):
        fb, fg = getattr(self.bad, name), getattr(self.good, name)

        def call(*a, **kw):
            ob, og = fb(*a, **kw), fg(*a, **kw)
            tb, tg = (ob if isinstance(ob, tuple) else (ob,)), (og if isinstance(og, tuple) else (og,))
            self.pairs += [(name, b, g) for i, (b, g) in enumerate(zip(tb, tg)) if i in OLD_COMPARED.get(name, range(9)) and torch.is_tensor(b) and not (b.shape == g.shape and torch.equal(P._bits(b), P._bits(g)))]
            return ob
        return call


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_planted_bug_is_rejected_and_what_the_old_check_says(name):
    what, mut, run, phrase = MUTATIONS[name]
    clean = P.Checks()
    run(clean, Emulated())
    clean.done()
    K, fails = Both(mut), P.Checks()
    run(fails, K)
    assert fails, f"{name} ({what}): not rejected"
    for ph in ((phrase,) if isinstance(phrase, str) else phrase):
        assert any(ph in m for m in fails), f"{name}: rejected, but not by the check meant to catch it ({ph!r}):\n" + "\n".join(fails[:5])
    assert K.pairs, "the mutation changed no output"
    verdicts = [old_close(b, g) for _, b, g in K.pairs]
    accepted = all(verdicts)
    print(f"{name}: {what}\n    new checks: rejected ({len(fails)} failures; first: {fails[0][:160]})\n    old close(): "
          f"{'ACCEPTS' if accepted else 'rejects'} ({sum(verdicts)} of {len(verdicts)} differing tensors pass it)")
    assert accepted == (name in OLD_CLOSE_ACCEPTS), f"{name}: the old close() {'accepts' if accepted else 'rejects'} it"


def test_the_fix_of_gelu_tanh_grad_changes_no_finite_result():
    """Over every finite bf16 input: the unclamped formula is NaN exactly at the predicted inputs, and wherever it is finite the clamped one has
    the same bits."""
    z = P.all_finite_bf16().float()
    old, new = P.gelu_tanh_grad_f32(z, False, False), P.gelu_tanh_grad_f32(z, True, True)
    assert torch.isfinite(new).all()
    nan = torch.isnan(old)
    assert nan.any() and float(z[nan & (z < 0)].max()) < -1e13 and float(z[nan & (z > 0)].min()) > 1e19
    for probe in (-2e13, -1e19, -3e38, 3e38):
        assert torch.isnan(P.gelu_tanh_grad_f32(torch.tensor([probe]).to(BF).float(), False, False)).all(), probe
    assert torch.equal(old[~nan].view(torch.int32), P.gelu_tanh_grad_f32(z, True, False)[~nan].view(torch.int32)), "the clamp alone changes no finite result"
    moved = old.view(torch.int32) != new.view(torch.int32)
    assert bool((old[moved & ~nan] == 0).all()) and float(z[moved & ~nan].max()) < -10.0, "the tail only ever replaces a 0, below the overflow of exp"
    assert bool(((new[nan] == 0) | (new[nan] == 1)).all())


# ---- ten times a bound is rejected ---------------------------------------------------------------------------------------------------------------
def _ulps_rejects_10x(ref64, n, floor, what):
    """An output that is exactly 0.9 / 10 times (n ulps + floor) off in one element passes / fails assert_ulps."""
    i = int(torch.randint(0, ref64.numel(), (1,), generator=P.rng(1)))
    step = n * P.ulp_bf16(ref64) + (floor if floor is not None else 0.0)
    for k, ok in ((0.9, True), (10.0, False)):
        out = ref64.clone()
        out.view(-1)[i] += k * step.reshape(-1)[i]
        if ok:
            P.assert_ulps(out, ref64, n, floor, what)
        else:
            with pytest.raises(AssertionError, match="beyond"):
                P.assert_ulps(out, ref64, n, floor, what)


def _abs_rejects_10x(ref64, bound, what):
    i = int(torch.randint(0, ref64.numel(), (1,), generator=P.rng(2)))
    for k, ok in ((0.9, True), (10.0, False)):
        out = ref64.clone()
        out.view(-1)[i] += k * bound.reshape(-1)[i]
        if ok:
            P.assert_abs(out, ref64, bound, what)
        else:
            with pytest.raises(AssertionError, match="beyond their bound"):
                P.assert_abs(out, ref64, bound, what)


def _pin(value, expected, what):
    """The bound's own size at this test's fixed data, within a factor of 2 of what its derivation gives: a bound scaled by 20 fails here."""
    assert expected / 2 <= float(value) <= expected * 2, f"{what}: the bound is {float(value):.3g}, its derivation gives about {expected:.3g}"


def test_ten_times_a_bound_is_rejected():
    """Every derived bound passes an error of 0.9 times itself and rejects 10 times itself, and its size at this data is pinned (`_pin`) to the
    figure its derivation gives; the constants are asserted at their derived values."""
    assert P.U32 == 2.0 ** -24 and P.HW == 2.0 ** -23 and P.ERF_GRAD_FLOOR == 1e-7 and P.ULPS["dact1"] == 1 and P.ULPS["swiglu"] == 2 and P.ULPS["dact2"] == 2
    g = P.rng(3)
    x, w, b = P.randn_bf(g, (5, 1032), 2.0, 0.5), P.mant15(g, (1032,)), P.randn_bf(g, (1032,))
    for rms in (True, False):
        r = P.norm_fwd_ref(x, w, None if rms else b, 1e-5, rms)
        _ulps_rejects_10x(r["y64"], r["ulps"], r["floor"], f"norm y rms {rms}")
        _abs_rejects_10x(r["rstd"], r["rstd_rel"] * r["rstd"], "rstd")
    _abs_rejects_10x(r["mean"], r["mean_bound"], "mean")
    # dim 1032 on one wave: T = 8 * 3 + 6 = 30 roundings; mean |x| ~ 1.65
    _pin(r["rstd_rel"].max(), 0.5 * 34 * 2.0 ** -24 + 2.0 ** -23, "rstd (relative)")
    _pin(r["mean_bound"].max(), 31 * 2.0 ** -24 * 1.65, "mean")
    _pin(r["floor"].median(), 3e-6, "LayerNorm y floor (median: |w| rstd d mean + |t| (d rstd + 2 u))")
    dy = P.randn_bf(g, (5, 1032))
    rb = P.norm_bwd_ref(x, dy, w, r["mean"].float(), r["rstd"].float(), False, dw0=torch.randn(1032, generator=g), db0=torch.randn(1032, generator=g))
    _ulps_rejects_10x(rb["dx64"], 1, rb["dx_floor"], "norm dx")
    _abs_rejects_10x(rb["dw"], rb["dw_bound"], "norm dw")
    _abs_rejects_10x(rb["db"], rb["db_bound"], "norm db")
    _pin(rb["dw_bound"].max(), 8 * 2.0 ** -24 * 12, "norm dw ((rows + 3) u sum |dy xhat|, the sum up to ~12)")
    _pin(rb["db_bound"].max(), 6 * 2.0 ** -24 * 10, "norm db ((rows + 1) u sum |dy|, the sum up to ~10)")
    _pin(rb["dx_floor"].max(), 3e-6, "norm dx floor")
    c64, s64, floor = P.rope_table_ref(2048, 72, 10000.0)
    _ulps_rejects_10x(c64, 1, floor, "rope table")
    _pin(floor.max(), 2047 * 2.0 ** -22, "rope table floor at position 2047")
    z = P.all_finite_bf16().view(8, -1)[:, 4000:4100].contiguous()          # ordinary magnitudes
    dh = torch.full(z.shape, -0.75).to(BF)
    for act in (1, 3, 4):
        ref, fl = P.act_bwd_ref(z, dh, act)
        _ulps_rejects_10x(ref, P.ULPS["dact1"], fl, f"act_bwd {act}")
    gu = torch.cat([z, torch.full(z.shape, -3.0).to(BF)], 1)
    _ulps_rejects_10x(P.swiglu_fwd_ref(gu), P.ULPS["swiglu"], None, "swiglu_fwd")
    _ulps_rejects_10x(P.swiglu_bwd_ref(gu, dh), P.ULPS["dact2"], None, "swiglu_bwd")
    logits, targets, _ = P.ce_rows(g, 1000)
    rc = P.token_ce_ref(logits, targets, 1000, 2.0 ** -5)
    _abs_rejects_10x(rc["loss"], rc["loss_bound"], "ce loss")
    _ulps_rejects_10x(rc["grad64"], 1, rc["grad_floor"], "ce gradient")
    _pin(rc["loss_bound"][0], 43 * 2.0 ** -24, "CE loss of a diffuse row (loss 8.9: ds / s ~ 15 u, 3 u |log s| ~ 12 u, u |log s + m| ~ 7 u, u |loss| ~ 9 u)")
    _pin(rc["loss_bound"][1], 30 * 2.0 ** -24, "CE loss of the confident row (T = 12, the maximum 16 -> |log s + m| u = 16 u, sum p (dist + 2) = 2)")
    _pin(rc["grad_floor"].max(), 2.0 ** -5 * 18 * 2.0 ** -24, "CE gradient floor (grad_scale 2^-5; p ~ 1: ds / s ~ 14 u, + 4 u)")
    assert float(rc["loss"][1]) < 5e-4 and float(rc["loss_bound"][1]) < 5e-6, "a confident row: the loss is ~1e-4 and the bound says what fp32 delivers there, not 2e-5"


# ---- the helpers themselves ------------------------------------------------------------------------------------------------------------------------
def _round_f32(exact):
    """The fp32 nearest to a Fraction (ties do not occur in the test's data)."""
    import fractions
    c = torch.tensor(float(exact), dtype=torch.float64).float()
    cands = [c, torch.nextafter(c, torch.tensor(float("inf"))), torch.nextafter(c, torch.tensor(float("-inf")))]
    return min(cands, key=lambda t: abs(fractions.Fraction(float(t)) - exact))


def test_fma32_is_a_correctly_rounded_fma():
    import fractions
    g = P.rng(4)
    a, b = torch.randn(200000, generator=g), torch.randn(200000, generator=g)
    c = -(a * b) * (1.0 + torch.randn(200000, generator=g) * 1e-6)           # heavy cancellation: the low half of the product decides
    got = P.fma32(a, b, c)
    for i in range(0, 200000, 397):
        exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
        assert float(got[i]) == float(_round_f32(exact)), i
    assert not torch.equal(got, a * b + c), "an unfused evaluation differs"
    big = torch.tensor([1.0, 3.0e38]), torch.tensor([1.0, 3.0]), torch.tensor([2.0 ** -60, 0.0])      # a sticky bit far below; overflow
    assert P.fma32(*big).tolist() == [1.0, float("inf")]


def test_sqrt32_is_correctly_rounded():
    import math
    x = torch.rand(100003, generator=P.rng(6)) * 1e-3 + 1e-12
    got = P.sqrt32(x)
    for i in range(0, 100003, 101):
        assert float(got[i]) == float(torch.tensor(math.sqrt(float(x[i])), dtype=torch.float64).float())
    print("torch.sqrt(fp32) differs from the IEEE result in", int((torch.sqrt(x) != got).sum()), "of", x.numel())


def test_generators_and_guards():
    g = P.rng(5)
    x = P.balanced_rows(g, 3, 520, 5)
    assert bool((x.double().sum(-1) == 0).all()) and bool(((x.double() ** 2).mean(-1) == 4.0 ** 5).all())
    m = P.mant15(g, (1000,)).double()
    mant, _ = torch.frexp(m.abs())
    assert set((mant * 2).unique().tolist()) == {1.0, 1.25, 1.5}
    assert P.all_finite_bf16().numel() == 65280 and P.all_finite_bf16().numel() % 8 == 0 and torch.isfinite(P.all_finite_bf16().float()).all()
    o = P.Guarded(BF, (5, 7))
    o.view.zero_()
    o.assert_guards("untouched")
    for i in (P.Guarded.PAD - 1, P.Guarded.PAD + 35):
        o = P.Guarded(torch.float32, (5, 7))
        o.buf[i] = 0.0
        with pytest.raises(AssertionError, match="guard elements overwritten"):
            o.assert_guards("touched")
    x, dy, w, mean, rstd = P.norm_bwd_exact_inputs(g, 9, 520)
    P.norm_bwd_ref(x, dy, w, mean, rstd, False, exact=True)
    with pytest.raises(AssertionError, match="exact regime"):
        P.norm_bwd_ref(x, dy, w, mean, rstd * 0.3, False, exact=True)
    assert P.red_terms(1032, 64) == 8 * 3 + 6 and P.red_terms(2056, 256) == 8 * 2 + 9 and P.red_terms(8, 64) == 8 + 6
