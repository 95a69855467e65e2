"""lora_dropout on the GPU: the three kernels of csrc/lora_dropout.hip bit for bit against the numpy mask contract
(tests/lora_dropout_reference.py), LoraLinear forward / backward against a float64 autograd restatement of peft's formula with the
numpy masks, and the engine-level behaviour (inert at p = 0, training-only, seeds, fresh masks per forward, adapter config, resume).

Exact regime (tests/gemm_reference.py): integer operands in [-3, 3], alpha = 0.5 and p in {0.5, 0.75}, so inv is 2 or 4, every product and
every partial sum is an exact fp32 number, and a correct kernel equals rbf(float64 reference) in ANY summation order.

Off the exact regime (p = 0.1, normal operands) the per-element bound is derived, not measured:
    |got - ref64| <= ulp_bf16(ref64) + n * 2^-24 * sum |terms|
one output rounding plus the standard bound of an n-term fp32 accumulation; ref64 uses the bf16-rounded dropout(x) that `apply` defines.
"""
import importlib
import itertools
import json

import numpy as np
import pytest
import torch

import gemm_reference as G
import lora_dropout_reference as R
from gemm_reference import Failures, rbf, ulp_bf16

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
SEED = 7 + (3 << 32)            # both key words in use
MODS = (11, 5, 0xFFFFFFF0, 2)   # arbitrary module ids, one per fused group
U32 = 2.0 ** -24                # fp32 unit roundoff


def key(p, call=3):
    return dict(p=p, seed=SEED, call=call)


def xd_ref(x_cpu, G_, p, call=3):
    """[dropout_g(x) for g < G_] as CPU bf16 tensors, by the numpy contract."""
    return [R.dropout(x_cpu, module=MODS[g], call=call, seed=SEED, p=p) for g in range(G_)]


def keep_ref(M, K, g, p, call=3):
    return torch.from_numpy(R.keep_mask(M, K, module=MODS[g], call=call, seed=SEED, p=p))


def padded(t, dev, align=8):
    """`t` as a strided device view with `align` sentinel columns to its right (ld = cols + align); returns the Embedded."""
    return G.embed(t.to(dev), align=align, top=0, bottom=0, left=0, right=1, fill="sentinel")


def bits_equal_nan_aware(got, ref):
    got, ref = got.cpu(), ref.cpu()
    nan = torch.isnan(ref.float())
    same = got.view(torch.int16) == ref.view(torch.int16)
    return bool((torch.where(nan, torch.isnan(got.float()), same)).all())


def bound_check(fails, got, ref64, n, abs_terms, what):
    """|got - ref64| <= ulp_bf16(ref64) + n 2^-24 sum|terms| per element; prints the worst ratio before asserting."""
    err = (got.detach().cpu().double() - ref64).abs()
    lim = ulp_bf16(ref64) + n * U32 * abs_terms
    worst = float((err / lim).max())
    print(f"{what}: worst |err| / bound = {worst:.3f}")
    fails.check(worst <= 1.0, f"{what}: {(err > lim).sum().item()} elements beyond the bound, worst ratio {worst:.3f}")


# ---- apply ---------------------------------------------------------------------------------------------------------------------------------------
def test_apply_bits(ops, dev):
    """M in {1, 70} x K in {8, 520} x G in {1, 3} x p in {0.5, 0.1}: bits equal numpy (float32 multiply, round to nearest even); x has
    ld = K + 8 with a sentinel pad that survives; the output's neighbours survive; NaN: dropped -> +0, kept -> NaN."""
    fails = Failures()
    for M, K, G_, p in itertools.product((1, 70), (8, 520), (1, 3), (0.5, 0.1)):
        what = f"apply M {M} K {K} G {G_} p {p}"
        x = torch.randn((M, K), generator=G.rng(M * K + G_)).to(BF)
        keep0 = keep_ref(M, K, 0, p)
        dropped, kept = (~keep0).nonzero(), keep0.nonzero()
        nan_d = tuple(dropped[0].tolist()) if len(dropped) else None      # (an 8-element mask can keep everything)
        nan_k = tuple(kept[-1].tolist()) if len(kept) else None
        for pos in (nan_d, nan_k):
            if pos is not None:
                x[pos] = float("nan")
        e = padded(x, dev)
        out = torch.full((G_ + 2, M, K), G.SENTINEL[2], dtype=torch.int16, device=dev).view(BF)   # the G buffers between two guard buffers
        got = ops.lora_dropout_apply(e.view, modules=MODS[:G_], out=out[1:1 + G_], **key(p))
        ref = xd_ref(x, G_, p)
        for g in range(G_):
            fails.check(bits_equal_nan_aware(got[g], ref[g]), f"{what}: group {g} differs from the numpy contract")
        g0 = got[0].cpu()
        fails.check(nan_d is None or g0.view(torch.int16)[nan_d].item() == 0, f"{what}: NaN in a dropped position must come out +0")
        fails.check(nan_k is None or bool(torch.isnan(g0.float()[nan_k])), f"{what}: NaN in a kept position must survive")
        fails.check(nan_d is not None or M * K < 64, f"{what}: no dropped position to test")
        try:
            e.assert_guards(what + " (x pad)")
        except AssertionError as err:
            fails.append(str(err))
        sent = G.SENTINEL[2]
        fails.check(bool((out[0].view(torch.int16) == sent).all() and (out[-1].view(torch.int16) == sent).all()), f"{what}: wrote outside its G buffers")
        again = ops.lora_dropout_apply(e.view, modules=MODS[:G_], **key(p))
        fails.check(torch.equal(again.view(torch.int16), got.view(torch.int16)), f"{what}: second call differs")
        other = ops.lora_dropout_apply(e.view, modules=MODS[:G_], **key(p, call=4))
        if M * K >= 64:
            fails.check(not torch.equal(other.view(torch.int16), got.view(torch.int16)), f"{what}: another call drew the same mask")
    fails.done()


def test_p_outside_range_is_refused(ops, dev):
    x = torch.zeros((8, 8), dtype=BF, device=dev)
    for p in (1.0, -0.1):
        with pytest.raises(ValueError):
            ops.lora_dropout_apply(x, modules=[0], p=p, seed=0, call=0)


# ---- proj ----------------------------------------------------------------------------------------------------------------------------------------
def test_proj_exact(ops, dev):
    """M in {1, 70, 161} x K in {8, 520, 2056} x G in {1, 2, 3}, r = 32, p in {0.5, 0.75}: equal to rbf(reference) and to the
    apply + ops.gemm composition, to the bit.  K = 8 and 520 are no multiples of 32; 520 / 32 and 2056 / 32 split unevenly over 4 waves."""
    fails, r = Failures(), 32
    for M, K, G_, p in itertools.product((1, 70, 161), (8, 520, 2056), (1, 2, 3), (0.5, 0.75)):
        what = f"proj M {M} K {K} G {G_} p {p}"
        g = G.rng(M + K + G_)
        x, A = G.operand(g, M, K), G.operand(g, G_ * r, K)
        ex, eA = padded(x, dev), padded(A, dev)
        et = G.embed(BF, shape=(M, G_ * r), align=4, top=1, bottom=1, left=0, right=1, fill="sentinel", device=dev)
        got = ops.lora_dropout_proj(ex.view, eA.view, alpha=0.5, modules=MODS[:G_], out=et.view, **key(p))
        xd = xd_ref(x, G_, p)
        acc = torch.cat([xd[i].double() @ A[i * r:(i + 1) * r].double().T for i in range(G_)], 1)
        assert torch.equal(acc, acc.round()) and float(acc.abs().max()) < 2 ** 23, "left the exact regime"
        fails.exact(got, rbf(0.5 * acc).to(BF), what)
        try:
            et.assert_guards(what + " (t pad)")
        except AssertionError as err:
            fails.append(str(err))
        xdev = ops.lora_dropout_apply(ex.view, modules=MODS[:G_], **key(p))
        comp = torch.cat([ops.gemm(xdev[i], eA.view[i * r:(i + 1) * r], alpha=0.5) for i in range(G_)], 1)
        fails.exact(got, comp, what + " vs apply + gemm")
        again = ops.lora_dropout_proj(ex.view, eA.view, alpha=0.5, modules=MODS[:G_], **key(p))
        fails.exact(again, got.contiguous(), what + " second call")
    fails.done()


def test_proj_bound(ops, dev):
    """p = 0.1, normal operands: one output rounding + the (K + 1)-term fp32 accumulation bound (K products, the alpha multiply)."""
    fails, r, p = Failures(), 32, 0.1
    for M, K, G_ in [(70, 520, 3), (161, 2056, 2)]:
        g = G.rng(K)
        x, A = torch.randn((M, K), generator=g).to(BF), (torch.randn((G_ * r, K), generator=g) / r).to(BF)
        got = ops.lora_dropout_proj(x.to(dev), A.to(dev), alpha=0.5, modules=MODS[:G_], **key(p))
        xd = xd_ref(x, G_, p)
        ref = torch.cat([0.5 * xd[i].double() @ A[i * r:(i + 1) * r].double().T for i in range(G_)], 1)
        mag = torch.cat([0.5 * xd[i].double().abs() @ A[i * r:(i + 1) * r].double().abs().T for i in range(G_)], 1)
        bound_check(fails, got, ref, K + 1, mag, f"proj bound M {M} K {K} G {G_}")
        again = ops.lora_dropout_proj(x.to(dev), A.to(dev), alpha=0.5, modules=MODS[:G_], **key(p))
        fails.check(torch.equal(again, got), "proj: second call differs")
    fails.done()


# ---- backproj ------------------------------------------------------------------------------------------------------------------------------------
def backproj_ref(dx, dt, AT, G_, r, p):
    """(ref64, sum |terms|): dx + sum_g keep_g ? inv * (dt_g . AT_g^T) : 0 in float64, inv the fp32 scale."""
    M, K = dx.shape
    inv = float(R.inv_scale(p))
    ref, mag = dx.double().clone(), dx.double().abs()
    for g in range(G_):
        keep = keep_ref(M, K, g, p).double()
        a, b = dt[:, g * r:(g + 1) * r].double(), AT[:, g * r:(g + 1) * r].double()
        ref += keep * inv * (a @ b.T)
        mag += keep * inv * (a.abs() @ b.abs().T)
    return ref, mag


def test_backproj_exact(ops, dev):
    """M in {1, 70, 161} x K in {8, 520} x G in {1, 3} x r in {8, 32, 64}, p in {0.5, 0.75}: in place on dx (ld = K + 8, the pad keeps its
    sentinel), equal to rbf(reference) to the bit."""
    fails = Failures()
    for M, K, G_, r, p in itertools.product((1, 70, 161), (8, 520), (1, 3), (8, 32, 64), (0.5, 0.75)):
        what = f"backproj M {M} K {K} G {G_} r {r} p {p}"
        g = G.rng(M + K + G_ + r)
        dx, dt, AT = G.ints(g, (M, K), -8, 8), G.operand(g, M, G_ * r), G.operand(g, K, G_ * r)
        ref, _ = backproj_ref(dx, dt, AT, G_, r, p)
        assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 23, "left the exact regime"
        edt, eat = padded(dt, dev), padded(AT, dev)
        outs = []
        for _ in range(2):
            e = padded(dx, dev)
            ops.lora_dropout_backproj(e.view, edt.view, eat.view, modules=MODS[:G_], **key(p))
            outs.append(e.view.contiguous())
            try:
                e.assert_guards(what + " (dx pad)")
            except AssertionError as err:
                fails.append(str(err))
        fails.exact(outs[0], rbf(ref).to(BF), what)
        fails.exact(outs[1], outs[0], what + " second call")
    fails.done()


def test_backproj_bound(ops, dev):
    """p = 0.1, normal operands: one output rounding + the fp32 accumulation bound with n = G (r + 2) + 1 terms (r products, the scale multiply
    and the add per group, the dx term)."""
    fails, p = Failures(), 0.1
    for M, K, G_, r in [(70, 520, 3, 32), (70, 520, 1, 8), (161, 264, 2, 128)]:
        g = G.rng(K + r)
        dx, dt, AT = (torch.randn(s, generator=g).to(BF) for s in ((M, K), (M, G_ * r), (K, G_ * r)))
        ref, mag = backproj_ref(dx, dt, AT, G_, r, p)
        got = ops.lora_dropout_backproj(dx.to(dev), dt.to(dev), AT.to(dev), modules=MODS[:G_], **key(p))
        bound_check(fails, got, ref, G_ * (r + 2) + 1, mag, f"backproj bound M {M} K {K} G {G_} r {r}")
    fails.done()


# ---- LoraLinear ----------------------------------------------------------------------------------------------------------------------------------
class _RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16: the rounding points of the backward (dt = bf16(s dy B), dx0 = bf16(dy W))."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return rbf(g)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("G_", [1, 3])
def test_lora_linear_matches_autograd(ops, dev, monkeypatch, G_, fused):
    """M = 72, in = 264, G groups of 256 outputs, r = 32, p = 0.5: y, dx, dA, dB against a float64 autograd restatement of
    y = W x + b + s B_g(A_g(dropout_g(x))) with the numpy masks.  The restatement takes the kernel's own t_s (checked against its own bound
    first) and rounds the two gradients the backward stores in bf16, so each comparison sees one kernel's arithmetic:
        y, dx   one output rounding + n 2^-24 sum|terms|; dx also one ulp of each bf16 intermediate it sums (dx0, dt through |A|)
        dA, dB  fp32 outputs: (M + 1) 2^-24 sum|terms|; dA also one ulp of dt through |dropout(x)|"""
    E = load("openvla-oft_amd.engine")
    monkeypatch.setattr(E, "_LORA_DROPOUT_FUSED", fused)
    M, K, gn, r, s, p = 72, 264, 256, 32, 0.5, 0.5
    N = G_ * gn
    g = G.rng(90 + G_)
    rn = lambda *shape, scale=1.0: (torch.randn(shape, generator=g) * scale).to(BF)  # noqa: E731
    x, W, bias, A, B, dy = rn(M, K), rn(N, K, scale=K ** -0.5), rn(N), rn(G_ * r, K, scale=1.0 / r), rn(N, r, scale=0.1), rn(M, N)
    store = E.ParamStore(dev)
    lin = E.LoraLinear(store, "lin", W.to(dev), bias.to(dev), A.to(dev), B.to(dev), G_, s, ref_names=[f"lin{i}" for i in range(G_)])
    store.finalize()
    lin.refresh_derived()
    lin.dropout, lin.module_ids = E.DropoutState(p, SEED), list(MODS[:G_])
    lin.dropout.begin_forward(True)
    call = lin.dropout.call
    assert call == 1
    y, saved = lin.fwd(x.to(dev))
    assert len(saved) == 3 and saved[2] == call
    lin.dropout.begin_forward(False)       # an evaluation forward in between must not disturb the saved backward
    dx = lin.bwd(dy.to(dev), saved)
    t_gpu = saved[1].cpu()

    fails = Failures()
    inv = float(R.inv_scale(p))
    x64 = x.double().requires_grad_(True)
    A64, B64 = A.double().requires_grad_(True), B.double().requires_grad_(True)
    xm = _RoundGrad.apply(x64)
    y64 = xm @ W.double().T + bias.double()
    ymag = x.double().abs() @ W.double().abs().T + bias.double().abs()
    cols, colmag, dts, xds, keeps = [], [], [], [], []
    for i in range(G_):
        keep = keep_ref(M, K, i, p, call).double()
        xd_bf = R.dropout(x, module=MODS[i], call=call, seed=SEED, p=p).double()
        xd = x64 * keep * inv
        xd = xd + (xd_bf - xd).detach()                                        # the value apply defines, the gradient of the formula
        u = _RoundGrad.apply(xd @ A64[i * r:(i + 1) * r].T)
        t = s * u
        bound_check(fails, t_gpu[:, i * r:(i + 1) * r], t.detach(), K + 1, s * (xd_bf.abs() @ A.double()[i * r:(i + 1) * r].abs().T), f"t_s group {i}")
        t = t + (t_gpu[:, i * r:(i + 1) * r].double() - t).detach()            # the kernel's own t_s from here on
        Bg = B64[i * gn:(i + 1) * gn]
        cols.append(t @ Bg.T)
        colmag.append(t.detach().abs() @ Bg.detach().abs().T)
        dts.append(rbf(s * dy.double()[:, i * gn:(i + 1) * gn] @ B.double()[i * gn:(i + 1) * gn]))
        xds.append(xd_bf)
        keeps.append(keep)
    y64 = y64 + torch.cat(cols, 1)
    y64.backward(dy.double())
    bound_check(fails, y, y64.detach(), K + r + 2, ymag + torch.cat(colmag, 1), "y")

    dyd = dy.double()
    # dB_g = dy_g^T t_g (fp32)
    dB_ref, dB_got = B64.grad, lin.B.grad.cpu().double()
    dB_mag = torch.cat([dyd[:, i * gn:(i + 1) * gn].abs().T @ t_gpu[:, i * r:(i + 1) * r].double().abs() for i in range(G_)], 0)
    w = float(((dB_got - dB_ref).abs() / ((M + 1) * U32 * dB_mag)).max())
    print(f"dB: worst |err| / bound = {w:.3f}")
    fails.check(w <= 1.0, f"dB beyond (M + 1) 2^-24 sum|terms|: ratio {w:.3f}")
    # dA_g = dt_g^T dropout_g(x) (fp32), dt within one bf16 ulp of its reference
    dA_ref, dA_got = A64.grad, lin.A.grad.cpu().double()
    dA_lim = torch.cat([(M + 1) * U32 * (dts[i].abs().T @ xds[i].abs()) + ulp_bf16(dts[i]).T @ xds[i].abs() for i in range(G_)], 0)
    w = float(((dA_got - dA_ref).abs() / dA_lim).max())
    print(f"dA: worst |err| / bound = {w:.3f}")
    fails.check(w <= 1.0, f"dA beyond its bound: ratio {w:.3f}")
    fails.check(float(dA_ref.abs().max()) > 0 and float(dB_ref.abs().max()) > 0, "degenerate gradients")
    # dx = bf16(bf16(dy W) + sum_g keep_g inv dt_g A_g)
    dx_ref = x64.grad
    dx0 = dyd @ W.double()
    lim = ulp_bf16(dx_ref) + ulp_bf16(dx0) + (N + 1) * U32 * (dyd.abs() @ W.double().abs())
    for i in range(G_):
        Ag = A.double()[i * r:(i + 1) * r].abs()
        lim = lim + keeps[i] * inv * (ulp_bf16(dts[i]) @ Ag + (r + 3) * U32 * (dts[i].abs() @ Ag))
    w = float(((dx.cpu().double() - dx_ref).abs() / lim).max())
    print(f"dx: worst |err| / bound = {w:.3f}")
    fails.check(w <= 1.0, f"dx beyond its bound: ratio {w:.3f}")
    # the LoRA part of dx is masked: where every group dropped the element, dx is exactly the base data gradient's bf16 value
    alldrop = torch.stack(keeps).sum(0) == 0
    base = ops.gemm(dy.to(dev), lin.WT).cpu()
    fails.check(bool(alldrop.any()) and torch.equal(dx.cpu()[alldrop], base[alldrop]), "dx changed where every group's mask dropped the element")
    fails.done()


# ---- engine --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(dev):
    from oracle import vla_oracle as vo

    E, Wm, synth, config_mod = (load("openvla-oft_amd." + m) for m in ("engine", "weights", "synthetic", "config"))
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    batch = synth.make_batch(2, seed=3, prompt_lens=[10, 8], image_size=56)

    def make(**kw):
        get, has = Wm.make_getter({k: v.clone() for k, v in sd.items()}, dev)
        return E.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="l1", has=has, **kw)

    def step(eng):
        """One training forward + backward from zeroed gradients -> (loss bits, {name: LoRA gradient})."""
        eng.zero_grad()
        loss_sum, count, _ = eng.train_step_fwd_bwd(batch)
        grads = {k: v.clone() for k, v in eng.export_trainable("grad").items() if ".lora_" in k}
        return loss_sum.clone(), grads

    def same(a, b):
        return torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])

    w = dict(E=E, cfg=cfg, sd=sd, batch=batch, make=make, step=step, same=same, synth=synth)
    w["plain"] = step(make())                                   # an engine built without the argument
    e = make(lora_dropout=0.25, dropout_seed=7)
    w["drop_engine"], w["drop"], w["drop2"] = e, step(e), step(e)   # two consecutive training forwards on one batch
    return w


def test_engine_arguments(world, monkeypatch):
    E, make = world["E"], world["make"]
    for p in (1.0, -0.01, 1.5):
        with pytest.raises(ValueError):
            E.DropoutState(p, 0)
    monkeypatch.setattr(E, "_FUSE", "act")
    with pytest.raises(ValueError, match="OVLA_FUSE_DACT"):
        E.DropoutState(0.1, 0)
    E.DropoutState(0.0, 0)            # p = 0 is compatible with everything
    monkeypatch.undo()
    ids = world["drop_engine"].dropout_module_ids()
    names = [rn for lin in world["drop_engine"].all_linears() if getattr(lin, "has_lora", False) for rn in lin.ref_names]
    assert list(ids) == names and list(ids.values()) == list(range(len(names))) and len(names) > 20
    assert any(n.endswith("q_proj") for n in ids) and any(n.endswith("k_proj") for n in ids), "fused groups carry one id per reference sub-linear"


def test_p_zero_is_inert(world):
    """(a) lora_dropout = 0.0: the same loss bits and gradient bits as an engine built without the argument."""
    assert world["same"](world["step"](world["make"](lora_dropout=0.0, dropout_seed=99)), world["plain"])


def test_dropout_changes_training(world):
    """(b) p = 0.25 changes the training loss and the LoRA gradients relative to p = 0."""
    loss, grads = world["drop"]
    loss0, grads0 = world["plain"]
    assert torch.isfinite(loss).all() and not torch.equal(loss, loss0)
    changed = [k for k in grads if not torch.equal(grads[k], grads0[k])]
    assert len(changed) > len(grads) // 2, f"only {len(changed)} of {len(grads)} LoRA gradients changed"
    assert all(torch.isfinite(v).all() for v in grads.values())


def test_seeds(world):
    """(c) the same seed twice gives identical bits, another seed different ones."""
    assert world["same"](world["step"](world["make"](lora_dropout=0.25, dropout_seed=7)), world["drop"])
    assert not world["same"](world["step"](world["make"](lora_dropout=0.25, dropout_seed=8)), world["drop"])


def test_fresh_masks_per_forward(world):
    """(e) two consecutive training forwards on one batch give different losses: `call` advanced."""
    assert world["drop_engine"].dropout.call == 2
    assert not torch.equal(world["drop"][0], world["drop2"][0])


def test_eval_never_drops(world, dev):
    """(d) eval_step and predict_action on the p = 0.25 engine equal the p = 0 engine bit for bit (and leave `call` alone)."""
    e0, e1 = world["make"](), world["drop_engine"]
    call = e1.dropout.call
    a, b = e0.eval_step(world["batch"]), e1.eval_step(world["batch"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and e1.dropout.call == call and not e1.dropout.active
    modeling = load("openvla-oft_amd.modeling")
    stats = {"k": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    g = torch.Generator().manual_seed(5)
    ids = torch.cat([torch.tensor([[1]]), torch.randint(3, 31000, (1, 11), generator=g)], 1)
    pv = torch.randn(1, 12, 56, 56, generator=g).to(BF).float()
    outs = []
    for kw in (dict(), dict(lora_dropout=0.25, dropout_seed=7)):
        vla = modeling.OpenVLAForActionPrediction(world["cfg"], world["sd"], device=dev, norm_stats=stats, **kw)
        outs.append(vla.predict_action(input_ids=ids, unnorm_key="k", pixel_values=pv, attention_mask=torch.ones_like(ids, dtype=torch.bool)))
    for u, v in zip(outs[0], outs[1]):
        assert torch.equal(u, v) if torch.is_tensor(u) else np.array_equal(np.asarray(u), np.asarray(v))


def test_no_drop_outside_a_training_forward(world, dev):
    """The drop decision lives only while a training forward runs.  After a training step at p = 0.25, the step-independent front that the
    graphs capture on its own (patches_dev, train=False: towers, projector, proprio token) and a directly called adapted linear equal the
    p = 0 engine bit for bit, and `call` does not move."""
    e0, e1, batch = world["make"](), world["drop_engine"], world["batch"]
    world["step"](e1)                                # the last forward of e1 is a training one
    assert not e1.dropout.active
    call = e1.dropout.call
    ids, lab = batch["input_ids"].to(dev), batch["labels"].to(dev)
    outs = [e.patches_dev(ids, lab, batch["pixel_values"], batch["proprio"], e.proprio, None, False)[0] for e in (e0, e1)]
    assert torch.equal(outs[0], outs[1]) and e1.dropout.call == call
    e1.dropout.active = True                         # even a flag left set by someone else is cleared by an inference entry
    assert torch.equal(e1.patches_dev(ids, lab, batch["pixel_values"], batch["proprio"], e1.proprio, None, False)[0], outs[0])
    x = torch.randn((8, e1.proj[0].in_f), generator=G.rng(5)).to(BF).to(dev)
    assert torch.equal(e0.proj[0].fwd(x)[0], e1.proj[0].fwd(x)[0]) and len(e1.proj[0].fwd(x)[1]) == 2
    # and a forward that raises does not leave the flag behind
    with pytest.raises(Exception):
        e1.forward_dev(ids[:, :0], lab, None, None, train=True)
    assert not e1.dropout.active


def test_finetune_records_dropout_and_resumes(world, tmp_path):
    """(f) finetune(cfg) with lora_dropout = 0.1 writes the value into adapter_config.json and its loss history differs from the 0.0 run;
    (g) resuming from the step-1 checkpoint reproduces step 2's loss bits (the checkpoint carries the mask stream's `call` counter)."""
    ft, synth = load("openvla-oft_amd.vla_scripts.finetune"), world["synth"]

    def run(p, root, **kw):
        cfg = ft.FinetuneConfig(run_root_dir=root, dataset_name="libero_spatial_no_noops", batch_size=2, num_images_in_input=2, use_proprio=True,
                                save_freq=1, wandb_log_freq=1, lora_dropout=p, **kw)
        first = 2 if kw.get("resume") else 0
        return ft.finetune(cfg, model_config=world["cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()}, log=lambda *_: None,
                           dataset=(synth.make_batch(2, seed=300 + s, prompt_lens=[9, 8], image_size=56) for s in range(first, 10)))

    h0 = run(0.0, tmp_path / "p0", max_steps=2)["loss_value"]
    h1 = run(0.1, tmp_path / "p1", max_steps=3)["loss_value"]
    assert len(h0) == 2 and len(h1) == 3 and all(np.isfinite(h1)) and h0 != h1[:2]
    ck = list((tmp_path / "p1").glob("*--1_chkpt"))
    assert len(ck) == 1
    assert json.loads((ck[0] / "lora_adapter" / "adapter_config.json").read_text())["lora_dropout"] == 0.1
    assert json.loads((list((tmp_path / "p0").glob("*--1_chkpt"))[0] / "lora_adapter" / "adapter_config.json").read_text())["lora_dropout"] == 0.0
    h2 = run(0.1, tmp_path / "p1r", max_steps=2, resume=True, resume_step=1, vla_path=str(ck[0]))["loss_value"]
    assert h2[0] == h1[2], f"resumed step: loss {h2[0]!r}, uninterrupted {h1[2]!r}"
    # the counter travels in the optimizer-state file; a checkpoint without one says so and leaves the engine's counter alone
    from safetensors.torch import load_file, save_file

    e = world["make"](lora_dropout=0.1, dropout_seed=ft.dropout_seed_for_rank(0))
    assert ft.load_training_checkpoint(ck[0], 1, e)["dropout_call"] and e.dropout.call == 2
    opt = ck[0] / "optimizer_state--1_checkpoint.safetensors"
    save_file({k: v for k, v in load_file(str(opt)).items() if k != "lora_dropout.call"}, str(opt))
    e.dropout.call = 0
    assert not ft.load_training_checkpoint(ck[0], 1, e)["dropout_call"] and e.dropout.call == 0
    h3 = run(0.1, tmp_path / "p1s", max_steps=2, resume=True, resume_step=1, vla_path=str(ck[0]))["loss_value"]
    assert np.isfinite(h3[0]) and h3[0] != h1[2], "without a stored counter the resumed run starts its mask stream at resume_step * grad_accumulation_steps"
