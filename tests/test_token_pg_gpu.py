"""ovla_token_pg: anchored bit for bit on ovla_token_ce where the two compute the same thing, against the float64 restatement
(tests/token_sample_reference.py) for a window and a temperature, the gate's truth table, agreement with ovla_sample_tokens, and the refusals."""
import importlib

import numpy as np
import pytest
import torch

from tests import token_sample_reference as R
from tests.gemm_reference import assert_ulps
from tests.pointwise_reference import assert_abs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = -1.7578125          # a bf16 value no gradient takes
SHAPES = ((1000, 1008), (32000, 32064))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def same(a, b, what):
    assert torch.equal(bits(a), bits(b)), f"{what}: bits differ"


def _rows(vocab, ld, rows=7, seed=0):
    g = torch.Generator().manual_seed(900 + vocab + seed)
    z = torch.randn(rows, ld, generator=g).to(BF)
    z[:, vocab:] = 3e38
    return z, torch.randint(0, vocab, (rows,), generator=g)


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("gs", (2.0 ** -5, 0.013))
def test_anchor_on_token_ce(ops, dev, vocab, ld, gs):
    """T = 1, the whole vocabulary, no old log-probabilities, advantage 1: ovla_token_ce's gradient and loss, bit for bit, in place too."""
    z, tgt = _rows(vocab, ld)
    one = torch.ones(7, device=dev)
    sent = torch.full((7, ld), SENT, dtype=BF, device=dev)
    loss, _, d_ce = ops.token_ce(z.to(dev), tgt.to(dev), vocab=vocab, grad_scale=gs, dlogits=sent.clone())
    lp, ent, ratio, clipped, d_pg = ops.token_pg(z.to(dev), tgt.to(dev).int(), one, vocab=vocab, grad_scale=gs, dlogits=sent.clone())
    same(d_pg, d_ce, "dlogits (the padding columns keep the sentinel in both)")
    same(lp, -loss, "logprob vs -loss_rows")
    assert bool((ratio == 1.0).all()) and int(clipped.sum()) == 0
    zi, zj = z.to(dev), z.to(dev)
    loss_i, _, _ = ops.token_ce(zi, tgt.to(dev), vocab=vocab, grad_scale=gs, inplace_grad=True)
    lp_i, *_ = ops.token_pg(zj, tgt.to(dev).int(), one, vocab=vocab, grad_scale=gs, inplace_grad=True)
    same(zj, zi, "in-place dlogits")
    same(zj[:, :vocab], d_ce[:, :vocab], "in-place = out-of-place")
    same(zj[:, vocab:], z[:, vocab:], "in-place: the padding columns are untouched")
    same(lp_i, lp, "in-place logprob")


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("wi", (0, 2))
@pytest.mark.parametrize("T", (0.5, 1.6))
def test_windowed_tempered_gradient(ops, dev, vocab, ld, wi, T):
    lo, hi = ((vocab - 256, vocab), (0, vocab), (3, 261))[wi]
    g = torch.Generator().manual_seed(31 + vocab + wi)
    z = R.eighths(g, (7, ld))
    outside = torch.ones(ld, dtype=torch.bool)
    outside[lo:hi] = False
    z[:, torch.nonzero(outside)[::2, 0]] = float("nan")            # NaN outside the window (and in the padding): a stored +0 all the same
    tokens = torch.randint(lo, hi, (7,), generator=g).int()
    adv = torch.tensor([1.0, -0.5, 2.25, -3.0, 0.125, 1.0, -1.0])
    gs = 1.0 / 56
    ref = R.pg_ref(z, vocab, lo, hi, T, tokens.numpy(), adv.numpy(), grad_scale=gs)
    sent = torch.full((7, ld), SENT, dtype=BF, device=dev)
    lp, ent, ratio, clipped, d = ops.token_pg(z.to(dev), tokens.to(dev), adv.to(dev), vocab=vocab, window=(lo, hi), temperature=T, grad_scale=gs, dlogits=sent)
    what = f"token_pg vocab {vocab} window [{lo}, {hi}) T={T}"
    assert_abs(lp, ref["logprob"], ref["logprob_bound"], what + " logprob")
    assert_abs(ent, ref["entropy"], ref["entropy_bound"], what + " entropy")
    d = d.cpu()
    assert_ulps(d[:, lo:hi].float(), ref["grad64"][:, lo:hi], 1, ref["grad_floor"][:, lo:hi], what + " gradient")
    for part in (d[:, :lo], d[:, hi:vocab]):
        assert bool((bits(part) == 0).all()), what + ": not +0 outside the window"
    assert bool((d[:, vocab:] == SENT).all()), what + ": the padding columns were written"
    # in place: the same bits
    zi = z.to(dev)
    ops.token_pg(zi, tokens.to(dev), adv.to(dev), vocab=vocab, window=(lo, hi), temperature=T, grad_scale=gs, inplace_grad=True)
    same(zi[:, :vocab], d[:, :vocab], what + " in place")
    # without a gradient the four row outputs keep their bits
    lp2, ent2, _, _, none = ops.token_pg(z.to(dev), tokens.to(dev), adv.to(dev), vocab=vocab, window=(lo, hi), temperature=T)
    assert none is None
    same(lp2, lp, what + " logprob without dlogits"), same(ent2, ent, what + " entropy without dlogits")


def test_gate_truth_table(ops, dev):
    vocab, ld, lo, hi, T, gs = 1000, 1008, 3, 261, 1.6, 0.25
    g = torch.Generator().manual_seed(77)
    z = R.eighths(g, (8, ld))
    tokens = torch.randint(lo, hi, (8,), generator=g).int()
    adv = torch.tensor([1.0, -1.0, 2.0, -0.5, 0.0, -2.0, 0.5, -1.0])
    zd, td, ad = z.to(dev), tokens.to(dev), adv.to(dev)
    kw = dict(vocab=vocab, window=(lo, hi), temperature=T, grad_scale=gs, inplace_grad=False)
    lp, ent, ratio, clipped, d = ops.token_pg(zd, td, ad, **kw)
    # on policy: ratio exactly 1, the run without old log-probabilities
    lp1, _, ratio1, clipped1, d1 = ops.token_pg(zd, td, ad, old_logprob=lp, **kw)
    assert bool((ratio1 == 1.0).all()) and int(clipped1.sum()) == 0
    same(d1[:, :vocab], d[:, :vocab], "on-policy gradient"), same(lp1, lp, "on-policy logprob")      # (columns >= vocab of a new tensor are never written)
    for shift, want_gated in ((-1.0, adv >= 0), (1.0, adv < 0)):       # ratio e^{+1} above 1.2: gated where adv >= 0;  e^{-1} below 0.8: where adv < 0
        old = (lp + shift).contiguous()
        ref = R.pg_ref(z, vocab, lo, hi, T, tokens.numpy(), adv.numpy(), old_logprob=old.cpu().numpy(), grad_scale=gs)
        assert np.array_equal(ref["clipped"].astype(bool), want_gated.numpy())
        _, _, ratio2, clipped2, d2 = ops.token_pg(zd, td, ad, old_logprob=old, **kw)
        assert np.array_equal(clipped2.cpu().numpy(), ref["clipped"]), f"old = logprob {shift:+}: clipped {clipped2.tolist()}"
        assert np.allclose(ratio2.cpu().numpy(), np.exp(-shift), rtol=1e-5)
        d2 = d2.cpu()
        gated = torch.as_tensor(ref["clipped"].astype(bool))
        assert bool((bits(d2[gated][:, :vocab]) == 0).all()), "a gated row is not all +0"
        # the ratio multiplies every element: expf (2 ulps) of a rounded difference of the kernel's own logprob (its bound), relative on c
        floor = ref["grad_floor"] + (ref["logprob_bound"] + 5 * 2.0 ** -24)[:, None] * ref["grad64"].abs()
        assert_ulps(d2[:, lo:hi].float(), ref["grad64"][:, lo:hi], 1, floor[:, lo:hi], f"old = logprob {shift:+}: the rows that are not gated scale by the ratio")
        kept = ~gated & torch.as_tensor(adv.numpy() != 0)
        assert bool((d2[kept][:, lo:hi].float().abs().sum(-1) > 0).all())


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_logprob_is_the_samplers(ops, dev, vocab, ld):
    """The shared row body: for the tokens ovla_sample_tokens drew, ovla_token_pg reports its log-probability and entropy bit for bit."""
    z = R.eighths(torch.Generator().manual_seed(55), (56, ld)).to(dev)
    one = torch.ones(56, device=dev)
    for window in ((vocab - 256, vocab), (0, vocab), (3, 261)):
        for T in R.GENERAL_T:
            tok, _, lp, ent = ops.sample_tokens(z, n_tokens=vocab, n_bins=255, vocab=vocab, window=window, temperature=T, seed=9, call=3)
            lp2, ent2, *_ = ops.token_pg(z, tok, one, vocab=vocab, window=window, temperature=T)
            same(lp2, lp, f"window {window} T={T} logprob"), same(ent2, ent, f"window {window} T={T} entropy")


def test_refusals_launch_nothing(ops, dev):
    _lib = importlib.import_module("openvla-oft_amd._lib")
    vocab = 1000
    z0 = R.eighths(torch.Generator().manual_seed(8), (7, vocab))
    tokens, adv = torch.full((7,), 5, dtype=torch.int32, device=dev), torch.ones(7, device=dev)
    cases = (
        (dict(window=(5, 5)), "window"), (dict(window=(0, vocab + 1)), "window"), (dict(window=(-2, 9)), "window"),
        (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
        (dict(clip=(1.2, 0.8)), "clip_lo"), (dict(clip=(float("nan"), 1.2)), "clip_lo"),
        (dict(vocab=vocab + 8, window=(0, 8), grad_scale=None), "ld="),
    )
    for kw, phrase in cases:
        z = z0.to(dev)
        out = dict(logprob=torch.full((7,), -77.0, device=dev), entropy=torch.full((7,), -77.0, device=dev), ratio=torch.full((7,), -77.0, device=dev),
                   clipped=torch.full((7,), -77, dtype=torch.int32, device=dev))
        args = dict(vocab=vocab, window=(3, 261), temperature=1.0, grad_scale=1.0, inplace_grad=True)
        args.update(kw)
        with pytest.raises(_lib.OvlaError, match=phrase):
            ops.token_pg(z, tokens, adv, **args, **out)
        torch.cuda.synchronize()
        for name, t in out.items():
            assert bool((t == -77).all()), f"{kw}: {name} was written"
        same(z, z0, f"{kw}: the logits were overwritten")
    g = _lib.STRUCTS["ovla_token_pg_args"]()
    z = z0.to(dev)
    g.logits, g.ld, g.tokens, g.advantage = z.data_ptr(), z.stride(0), tokens.data_ptr(), 0
    g.temperature, g.clip_lo, g.clip_hi, g.rows, g.vocab, g.lo, g.hi = 1.0, 0.8, 1.2, 7, vocab, 0, vocab
    with pytest.raises(_lib.OvlaError, match="null pointer"):
        _lib.call("ovla_token_pg", g, torch.cuda.current_stream().cuda_stream)
