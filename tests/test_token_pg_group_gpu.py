"""ovla_token_pg_group: anchored bit for bit on ovla_token_pg at G = 1, exact duplication and padding identities, the on-policy reference, the
general case against the float64 twin (tests/token_group_reference.py), the entropy term alone, and the refusals."""
import importlib

import numpy as np
import pytest
import torch

from tests import token_group_reference as GR
from tests import token_sample_reference as R
from tests.gemm_reference import assert_ulps
from tests.pointwise_reference import assert_abs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SENT = -1.7578125          # a bf16 value no gradient takes
SHAPES = ((1000, 1008), (32000, 32064))
ADV7 = (1.0, -0.5, 2.25, -3.0, 0.125, 1.0, -1.0)


def windows(vocab):
    return ((vocab - 256, vocab), (0, vocab), (3, 261))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: bits differ"


def _case(vocab, ld, lo, hi, G, seed=0, rows=7):
    g = torch.Generator().manual_seed(600 + vocab + 3 * lo + G + seed)
    z = R.eighths(g, (rows, ld))
    tokens = torch.randint(lo, hi, (rows, G), generator=g).int()
    return z, tokens


def _sent(rows, ld, dev):
    return torch.full((rows, ld), SENT, dtype=BF, device=dev)


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("wi", (0, 1, 2))
def test_anchor_on_token_pg(ops, dev, vocab, ld, wi):
    """G = 1, no reference, ent_scale = 0: ovla_token_pg's five outputs bit for bit, out of place and in place, without and with old log-probabilities
    that gate some rows (all +0 there); the padding columns keep the sentinel."""
    lo, hi = windows(vocab)[wi]
    T, gs = 1.6, 1.0 / 56
    z, tokens = _case(vocab, ld, lo, hi, 1)
    adv = torch.tensor(ADV7)
    zd, td, ad = z.to(dev), tokens.to(dev), adv.to(dev)
    kw = dict(vocab=vocab, window=(lo, hi), temperature=T, grad_scale=gs)
    lp0, *_ = ops.token_pg(zd, td[:, 0].contiguous(), ad, vocab=vocab, window=(lo, hi), temperature=T)
    olds = (None, (lp0 + torch.tensor([0.5, 0.5, -0.5, -0.5, 0.01, -1.0, 1.0], device=dev)).contiguous())
    for old in olds:
        lp, ent, ratio, clipped, d = ops.token_pg(zd, td[:, 0].contiguous(), ad, old_logprob=old, dlogits=_sent(7, ld, dev), **kw)
        o2 = None if old is None else old.view(7, 1)
        glp, gratio, gclipped, gkl, gent, gd = ops.token_pg_group(zd, td, ad.view(7, 1), old_logprob=o2, dlogits=_sent(7, ld, dev), **kw)
        what = f"vocab {vocab} window [{lo}, {hi}) old={'yes' if old is not None else 'no'}"
        assert gkl is None
        same(gd, d, what + " dlogits (sentinel in the padding of both)")
        same(glp[:, 0], lp, what + " logprob"), same(gent, ent, what + " entropy"), same(gratio[:, 0], ratio, what + " ratio")
        same(gclipped[:, 0], clipped, what + " clipped")
        if old is not None:
            gated = clipped.bool().cpu()
            assert 0 < int(gated.sum()) < 7, "the case must gate some rows and keep some"
            assert bool((bits(gd.cpu()[gated][:, :vocab]) == 0).all()), what + ": a gated row is not all +0"
        zi = z.to(dev)
        ilp, *_ = ops.token_pg_group(zi, td, ad.view(7, 1), old_logprob=o2, inplace_grad=True, **kw)
        same(zi[:, :vocab], d[:, :vocab], what + " in place"), same(zi[:, vocab:], z[:, vocab:], what + " in place: padding untouched")
        same(ilp, glp, what + " in-place logprob")


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_exact_duplication_and_padding(ops, dev, vocab, ld):
    """x + x and a halved power-of-two scale are exact: G = 2 identical samples at grad_scale / 2 give the G = 1 bits.  Skipped samples add nothing:
    G = 4 with three zero advantages at 4 grad_scale gives the G = 1 bits of the remaining sample, with a NaN in a skipped sample's old_logprob."""
    lo, hi = windows(vocab)[0]
    T, gs = 0.5, 2.0 ** -6
    z, tokens = _case(vocab, ld, lo, hi, 1, seed=1)
    adv = torch.tensor(ADV7).view(7, 1)
    zd = z.to(dev)
    kw = dict(vocab=vocab, window=(lo, hi), temperature=T, inplace_grad=False)
    lp1, r1, c1, _, e1, d1 = ops.token_pg_group(zd, tokens.to(dev), adv.to(dev), grad_scale=gs, **kw)
    old = (lp1 + torch.tensor([0.1, -0.1, 0.05, 0.5, -0.5, 0.0, 0.02], device=dev).view(7, 1)).contiguous()
    for o in (None, old):
        lp1, r1, c1, _, e1, d1 = ops.token_pg_group(zd, tokens.to(dev), adv.to(dev), old_logprob=o, grad_scale=gs, **kw)
        t2, a2 = tokens.repeat(1, 2).contiguous().to(dev), adv.repeat(1, 2).contiguous().to(dev)
        o2 = None if o is None else o.repeat(1, 2).contiguous()
        lp2, r2, c2, _, e2, d2 = ops.token_pg_group(zd, t2, a2, old_logprob=o2, grad_scale=gs / 2, **kw)
        same(d2[:, :vocab], d1[:, :vocab], "duplicated samples")
        same(lp2, lp1.repeat(1, 2), "duplicated logprob"), same(e2, e1, "entropy"), same(r2, r1.repeat(1, 2), "ratio"), same(c2, c1.repeat(1, 2), "clipped")
        for slot in (0, 2, 3):
            g = torch.Generator().manual_seed(slot)
            t4 = torch.randint(lo, hi, (7, 4), generator=g).int()
            a4 = torch.zeros((7, 4))
            t4[:, slot], a4[:, slot] = tokens[:, 0], adv[:, 0]
            o4 = None
            if o is not None:
                o4 = torch.full((7, 4), float("nan"))
                o4[:, slot] = o[:, 0].cpu()
                o4 = o4.to(dev)
            # the kernel's grad_scale is absolute (a caller that folds 1 / G into it passes 4 x the G = 1 loss scale: the same number here)
            lp4, r4, c4, _, e4, d4 = ops.token_pg_group(zd, t4.to(dev), a4.to(dev), old_logprob=o4, grad_scale=(4 * gs) / 4, **kw)
            same(d4[:, :vocab], d1[:, :vocab], f"three padded samples, the live one in slot {slot}")
            same(lp4[:, slot], lp1[:, 0], "padded logprob"), same(e4, e1, "padded entropy")


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_on_policy_reference(ops, dev, vocab, ld):
    """ref_logprob = the kernel's own logprob: d = 0, expm1f(0) = 0, kl = +0 and k = +0, so w = c + 0 and the gradient keeps its bits for any kl_coef."""
    lo, hi = windows(vocab)[2]
    z, tokens = _case(vocab, ld, lo, hi, 3, seed=2)
    adv = torch.tensor(ADV7 * 3).view(3, 7).t().contiguous() * torch.tensor([1.0, -1.0, 0.5])
    zd, td, ad = z.to(dev), tokens.to(dev), adv.contiguous().to(dev)
    kw = dict(vocab=vocab, window=(lo, hi), temperature=1.6, grad_scale=1.0 / 21, inplace_grad=False)
    lp, _, _, kl0, _, d0 = ops.token_pg_group(zd, td, ad, **kw)
    assert kl0 is None
    for kl_coef in (0.0, 0.04, 3.0):
        lp1, _, _, kl, _, d1 = ops.token_pg_group(zd, td, ad, ref_logprob=lp, kl_coef=kl_coef, **kw)
        assert bool((bits(kl) == 0).all()), f"kl_coef {kl_coef}: kl is not +0 on policy"
        same(d1[:, :vocab], d0[:, :vocab], f"kl_coef {kl_coef}: on-policy gradient"), same(lp1, lp, "logprob")


def _general_inputs(vocab, ld, lo, hi, G, T):
    z, tokens = _case(vocab, ld, lo, hi, G, seed=3)
    tokens[:, 1] = tokens[:, 0]                                  # two samples share a token
    g = torch.Generator().manual_seed(G)
    adv = (torch.randint(1, 9, (7, G), generator=g).float() / 4.0) * torch.where(torch.arange(7 * G).view(7, G) % 3 == 1, -1.0, 1.0)
    outside = torch.ones(ld, dtype=torch.bool)
    outside[lo:hi] = False
    z[:, torch.nonzero(outside)[::2, 0]] = float("nan")          # NaN outside the window and in the padding
    base = GR.group_ref(z, vocab, lo, hi, T, tokens.numpy(), adv.numpy())["logprob"].float()
    # old: ratios e^(+-0.5) (gated where the advantage's sign says so) and e^(+-0.05) (kept); ref = logprob +- 0.5
    shift_old = torch.where(torch.arange(7 * G).view(7, G) % 2 == 0, 0.5, -0.05) * torch.where(torch.arange(G)[None, :] % 3 == 0, -1.0, 1.0)
    old = (base + shift_old).contiguous()
    ref = (base + torch.where(torch.arange(G)[None, :] % 2 == 0, 0.5, -0.5)).contiguous()
    return z, tokens, adv, old, ref


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("wi", (0, 1, 2))
@pytest.mark.parametrize("G", (3, 8))
@pytest.mark.parametrize("T", (0.5, 1.6))
def test_general_case_against_the_twin(ops, dev, vocab, ld, wi, G, T):
    lo, hi = windows(vocab)[wi]
    z, tokens, adv, old, ref = _general_inputs(vocab, ld, lo, hi, G, T)
    kw = dict(kl_coef=0.04, ent_scale=0.01 / 7, clip=(0.8, 1.2), grad_scale=1.0 / (7 * G))
    twin = GR.group_ref(z, vocab, lo, hi, T, tokens.numpy(), adv.numpy(), old_logprob=old.numpy(), ref_logprob=ref.numpy(), **kw)
    assert 0 < int(twin["clipped"].sum()) < 7 * G, "the inputs must gate some samples and keep some"
    zd, td, ad, od, rd = z.to(dev), tokens.to(dev), adv.to(dev), old.to(dev), ref.to(dev)
    lp, ratio, clipped, kl, ent, d = ops.token_pg_group(zd, td, ad, old_logprob=od, ref_logprob=rd, vocab=vocab, window=(lo, hi), temperature=T,
                                                        dlogits=_sent(7, ld, dev), **kw)
    what = f"token_pg_group vocab {vocab} window [{lo}, {hi}) G={G} T={T}"
    print(what, "worst |err| / bound:", "logprob", assert_abs(lp, twin["logprob"], twin["logprob_bound"], what + " logprob"),
          "entropy", assert_abs(ent, twin["entropy"], twin["entropy_bound"], what + " entropy"),
          "kl", assert_abs(kl, twin["kl"], twin["kl_bound"], what + " kl"))
    assert np.array_equal(clipped.cpu().numpy(), twin["clipped"]), what + " clipped"
    assert np.allclose(ratio.cpu().numpy(), twin["ratio"], rtol=1e-5)
    d = d.cpu()
    print("gradient worst ulp:", assert_ulps(d[:, lo:hi].float(), twin["grad64"][:, lo:hi], 1, twin["grad_floor"][:, lo:hi], what + " gradient"))
    for part in (d[:, :lo], d[:, hi:vocab]):
        assert bool((bits(part) == 0).all()), what + ": not +0 outside the window"
    assert bool((d[:, vocab:] == SENT).all()), what + ": the padding columns were written"
    zi = z.to(dev)
    ops.token_pg_group(zi, td, ad, old_logprob=od, ref_logprob=rd, vocab=vocab, window=(lo, hi), temperature=T, inplace_grad=True, **kw)
    same(zi[:, :vocab], d[:, :vocab], what + " in place")
    same(zi[:, vocab:], z[:, vocab:], what + " in place: the padding columns are untouched")


@pytest.mark.parametrize("G", (1, 2, 64))
def test_group_sizes_at_the_ends(ops, dev, G):
    """G = 1, 2 and the cap against the twin, surrogate and KL, on the small shape."""
    vocab, ld = SHAPES[0]
    lo, hi = windows(vocab)[2]
    z, tokens = _case(vocab, ld, lo, hi, G, seed=4)
    g = torch.Generator().manual_seed(G)
    adv = (torch.randint(1, 9, (7, G), generator=g).float() / 4.0) * torch.where(torch.arange(7 * G).view(7, G) % 3 == 1, -1.0, 1.0)
    base = GR.group_ref(z, vocab, lo, hi, 1.6, tokens.numpy(), adv.numpy())["logprob"].float()
    ref = (base + torch.where(torch.arange(G)[None, :] % 2 == 0, 0.5, -0.5)).contiguous()
    kw = dict(kl_coef=0.04, grad_scale=1.0 / (7 * G))
    twin = GR.group_ref(z, vocab, lo, hi, 1.6, tokens.numpy(), adv.numpy(), ref_logprob=ref.numpy(), **kw)
    lp, _, _, kl, ent, d = ops.token_pg_group(z.to(dev), tokens.to(dev), adv.to(dev), ref_logprob=ref.to(dev), vocab=vocab, window=(lo, hi), temperature=1.6,
                                              inplace_grad=False, **kw)
    assert_abs(lp, twin["logprob"], twin["logprob_bound"], f"G={G} logprob"), assert_abs(kl, twin["kl"], twin["kl_bound"], f"G={G} kl")
    assert_ulps(d.cpu()[:, lo:hi].float(), twin["grad64"][:, lo:hi], 1, twin["grad_floor"][:, lo:hi], f"G={G} gradient")


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("T", (0.5, 1.6))
def test_entropy_alone(ops, dev, vocab, ld, T):
    """All advantages 0, no reference: every sample is skipped and the gradient is the entropy term; with ent_scale = 0 too the rows are +0."""
    lo, hi = windows(vocab)[0]
    z, tokens = _case(vocab, ld, lo, hi, 3, seed=5)
    z[:, lo + 5] = float("-inf")                                 # probability 0: the term is skipped, not 0 * inf
    tokens[tokens == lo + 5] = lo + 6
    adv = torch.zeros((7, 3))
    twin = GR.group_ref(z, vocab, lo, hi, T, tokens.numpy(), adv.numpy(), ent_scale=0.25)
    _, _, _, _, ent, d = ops.token_pg_group(z.to(dev), tokens.to(dev), adv.to(dev), vocab=vocab, window=(lo, hi), temperature=T, ent_scale=0.25, grad_scale=1.0,
                                            dlogits=_sent(7, ld, dev))
    d = d.cpu()
    assert_abs(ent, twin["entropy"], twin["entropy_bound"], "entropy")
    assert_ulps(d[:, lo:hi].float(), twin["grad64"][:, lo:hi], 1, twin["grad_floor"][:, lo:hi], f"entropy term vocab {vocab} T={T}")
    assert float(d[:, lo:hi].float().abs().max()) > 0 and int(bits(d[:, lo + 5]).abs().sum()) == 0
    assert bool((bits(d[:, :lo]) == 0).all()) and bool((d[:, vocab:] == SENT).all())
    _, _, _, _, _, d0 = ops.token_pg_group(z.to(dev), tokens.to(dev), adv.to(dev), vocab=vocab, window=(lo, hi), temperature=T, grad_scale=1.0, dlogits=_sent(7, ld, dev))
    assert bool((bits(d0.cpu()[:, :vocab]) == 0).all()) and bool((d0.cpu()[:, vocab:] == SENT).all()), "every sample skipped, ent_scale = 0: +0 on [0, vocab)"


def test_refusals_launch_nothing(ops, dev):
    _lib = importlib.import_module("openvla-oft_amd._lib")
    vocab, G = 1000, 2
    z0 = R.eighths(torch.Generator().manual_seed(8), (7, vocab))
    tokens, adv = torch.full((7, G), 5, dtype=torch.int32, device=dev), torch.ones((7, G), device=dev)
    ref = torch.zeros((7, G), device=dev)
    cases = (
        (dict(window=(5, 5)), "window"), (dict(window=(0, vocab + 1)), "window"), (dict(window=(-2, 9)), "window"),
        (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
        (dict(clip=(1.2, 0.8)), "clip_lo"), (dict(clip=(float("nan"), 1.2)), "clip_lo"),
        (dict(vocab=vocab + 8, window=(0, 8), grad_scale=None), "ld="),
        (dict(kl_coef=-0.5), "kl_coef"), (dict(kl_coef=float("nan")), "kl_coef"), (dict(ent_scale=float("nan")), "ent_scale"),
        (dict(tokens=torch.zeros((7, 65), dtype=torch.int32, device=dev), advantage=torch.ones((7, 65), device=dev)), "G = 65"),
    )
    for kw, phrase in cases:
        kw = dict(kw)
        z = z0.to(dev)
        t, a = kw.pop("tokens", tokens), kw.pop("advantage", adv)
        n = t.shape[1]
        out = dict(logprob=torch.full((7, n), -77.0, device=dev), entropy=torch.full((7,), -77.0, device=dev), ratio=torch.full((7, n), -77.0, device=dev),
                   clipped=torch.full((7, n), -77, dtype=torch.int32, device=dev))
        args = dict(vocab=vocab, window=(3, 261), temperature=1.0, grad_scale=1.0, inplace_grad=True)
        args.update(kw)
        with pytest.raises(_lib.OvlaError, match=phrase):
            ops.token_pg_group(z, t, a, **args, **out)
        torch.cuda.synchronize()
        for name, o in out.items():
            assert bool((o == -77).all()), f"{kw}: {name} was written"
        same(z, z0, f"{kw}: the logits were overwritten")
    # G = 0, ref_logprob without kl, kl without ref_logprob, a null pointer: through the struct (the wrapper pairs kl with ref_logprob itself)
    z = z0.to(dev)
    lp, ratio, ent, kl = (torch.full((7, G), -77.0, device=dev) for _ in range(4))
    clipped = torch.full((7, G), -77, dtype=torch.int32, device=dev)

    def struct(**over):
        g = _lib.STRUCTS["ovla_token_pg_group_args"]()
        g.logits, g.ld, g.tokens, g.advantage = z.data_ptr(), z.stride(0), tokens.data_ptr(), adv.data_ptr()
        g.logprob, g.ratio, g.clipped, g.entropy = lp.data_ptr(), ratio.data_ptr(), clipped.data_ptr(), ent.data_ptr()
        g.dlogits, g.ld_d = z.data_ptr(), z.stride(0)
        g.temperature, g.clip_lo, g.clip_hi, g.grad_scale, g.rows, g.G, g.vocab, g.lo, g.hi = 1.0, 0.8, 1.2, 1.0, 7, G, vocab, 0, vocab
        for k, v in over.items():
            setattr(g, k, v)
        return g

    for over, phrase in ((dict(G=0), "G = 0"), (dict(ref_logprob=ref.data_ptr()), "come together"), (dict(kl=kl.data_ptr()), "come together"),
                         (dict(advantage=0), "null pointer")):
        with pytest.raises(_lib.OvlaError, match=phrase):
            _lib.call("ovla_token_pg_group", struct(**over), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for name, o in (("logprob", lp), ("ratio", ratio), ("entropy", ent), ("kl", kl), ("clipped", clipped)):
            assert bool((o == -77).all()), f"{over}: {name} was written"
        same(z, z0, f"{over}: the logits were overwritten")
