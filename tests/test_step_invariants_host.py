"""The training-step invariants without a GPU: the comparison helpers of tests/step_invariants.py catch seeded defects and name the tensor;
the identities that tests/test_step_invariants_gpu.py asserts bit for bit hold for the REFERENCE arithmetic (the fp32 oracle under autograd,
to 1e-6 relative) -- they are properties of the model, not of this implementation; `padding_mask` marks exactly the alignment gaps."""
import importlib

import pytest
import torch

from oracle import vla_oracle as vo
from tests import step_invariants as SI

BF = torch.bfloat16


# ---- the helpers catch seeded defects ----------------------------------------------------------------------------------------------------------
def synthetic_grads(seed):
    g = torch.Generator().manual_seed(seed)
    return {f"layer.{i}.{leaf}": torch.randn(shape, generator=g) * 10.0 ** (i - 3)
            for i in range(4) for leaf, shape in (("lora_A.weight", (32, 24)), ("lora_B.weight", (40, 32)), ("bias", (17,)))}


def findings_of(check):
    F = SI.Findings()
    check(F)
    return list(F)


def test_clean_results_pass_every_helper():
    g1, g2 = synthetic_grads(1), synthetic_grads(2)
    F = SI.Findings()
    F.same_grads({n: g1[n] + g2[n] for n in g1}, {n: g1[n] + g2[n] for n in g1}, "sum")
    F.same_grads({n: 0.5 * g for n, g in g1.items()}, {n: g * 0.5 for n, g in g1.items()}, "scale")
    F.all_finite(g1, "finite")
    F.every_tensor_nonzero(g1, "nonzero")
    F.all_zero(torch.zeros(5), "zeros")
    F.done()


def test_seeded_defects_are_reported_with_the_right_tensor():
    g1, g2 = synthetic_grads(1), synthetic_grads(2)
    want = {n: g1[n] + g2[n] for n in g1}
    victim = "layer.2.lora_B.weight"
    # one tensor overwritten with G2 instead of G1 + G2
    got = dict(want, **{victim: g2[victim].clone()})
    out = findings_of(lambda F: F.same_grads(got, want, "accumulate"))
    assert len(out) == 1 and victim in out[0] and f"{g1[victim].numel()} of {g1[victim].numel()} elements differ" in out[0] and "first at (0, 0)" in out[0], out
    # one tensor scaled by the wrong factor
    got = {n: 0.5 * g for n, g in g1.items()}
    got["layer.0.bias"] = g1["layer.0.bias"] * 1.0
    out = findings_of(lambda F: F.same_grads(got, {n: 0.5 * g for n, g in g1.items()}, "scale 0.5"))
    assert len(out) == 1 and "scale 0.5: layer.0.bias" in out[0] and "got" in out[0] and "want" in out[0], out
    # one element differing in the last bit, deep inside a tensor: the first differing index and both values
    got = {n: g.clone() for n, g in g1.items()}
    got[victim].view(torch.int32)[7, 5] += 1
    out = findings_of(lambda F: F.same_grads(got, g1, "bits"))
    assert len(out) == 1 and victim in out[0] and "1 of 1280 elements differ; first at (7, 5)" in out[0], out
    # -0.0 against +0.0 are different bits
    assert findings_of(lambda F: F.same_bits(torch.tensor([-0.0]), torch.tensor([0.0]), "signed zero"))
    # one element of the padding nonzero
    pad = torch.zeros(192)
    pad[130] = 1e-30
    out = findings_of(lambda F: F.all_zero(pad, "store 0 flat_grad padding"))
    assert len(out) == 1 and "store 0 flat_grad padding: 1 of 192" in out[0] and "flat index 130" in out[0], out
    # one tensor all zero
    got = dict(g1, **{victim: torch.zeros_like(g1[victim])})
    out = findings_of(lambda F: F.every_tensor_nonzero(got, "vacuous"))
    assert len(out) == 1 and victim in out[0] and "are zero" in out[0], out
    # one NaN
    got = {n: g.clone() for n, g in g1.items()}
    got["layer.3.bias"][4] = float("nan")
    out = findings_of(lambda F: F.all_finite(got, "finite"))
    assert len(out) == 1 and "layer.3.bias" in out[0] and "flat index 4" in out[0], out
    # a missing tensor
    got = {n: g for n, g in g1.items() if n != victim}
    out = findings_of(lambda F: F.same_grads(got, g1, "names"))
    assert len(out) == 1 and victim in out[0], out
    with pytest.raises(AssertionError, match="1 findings"):
        F = SI.Findings()
        F.all_zero(pad, "x")
        F.done()


def test_loss_reference_knows_when_any_order_is_exact():
    """L1 terms of 0.25 .. 2 (last place 2^-9, sum below 2^9): every order is exact and the restated sum is THE loss; one term of 2^-20 beside
    300 terms near 1.5 is not (2^-27 granularity against a sum of 450): the helper then bounds instead of pinning bits."""
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(24, 7, generator=g).to(BF)
    off = (0.25 + torch.rand(24, 7, generator=g)) * torch.where(torch.rand(24, 7, generator=g) < 0.5, -1.0, 1.0)
    target = (pred.float() + off).to(BF)
    total, n, order_free = SI.loss_reference(pred, target, mse=False)
    assert n == 168 and order_free
    d = (target.float() - pred.float()).to(BF).float().abs()
    for perm in (torch.arange(168), torch.randperm(168, generator=g), torch.argsort(d.reshape(-1))):
        s = torch.zeros((), dtype=torch.float32)
        for v in d.reshape(-1)[perm]:
            s = s + v
        assert float(s) == total
    F = SI.Findings()
    F.same_loss(torch.tensor([total], dtype=torch.float32), torch.tensor([total], dtype=torch.float32), (total, n, order_free), "loss")
    F.done()
    out = findings_of(lambda F: F.same_loss(torch.tensor([total], dtype=torch.float32), torch.tensor([total * (1 + 2.0 ** -20)], dtype=torch.float32), (total, n, True), "loss"))
    assert len(out) == 1 and "second loss_sum" in out[0], out
    pred = torch.zeros(43, 7).to(BF)
    target = torch.full((43, 7), 1.5).to(BF)
    target[5, 3] = 2.0 ** -20
    total, n, order_free = SI.loss_reference(pred, target, mse=False)
    assert n == 301 and not order_free and total == 450.0 + 2.0 ** -20
    near = torch.tensor([450.0], dtype=torch.float32)
    SI.Findings().same_loss(near, near, (total, n, order_free), "loss")
    out = findings_of(lambda F: F.same_loss(near, near * 1.01, (total, n, order_free), "loss"))
    assert len(out) == 1 and "second loss_sum" in out[0] and "beyond" in out[0], out
    # MSE terms: bf16(d * d)
    total, n, _ = SI.loss_reference(torch.tensor([[1.0, 3.0]]).to(BF), torch.tensor([[1.5, 0.0]]).to(BF), mse=True)
    assert (total, n) == (9.25, 2)


# ---- padding_mask ----------------------------------------------------------------------------------------------------------------------------------
def test_padding_mask_marks_exactly_the_alignment_gaps():
    engine_mod = importlib.import_module("openvla-oft_amd.engine")
    st = engine_mod.ParamStore(torch.device("cpu"))
    sizes = [("a", (3, 5), BF), ("b", (64,), BF), ("c", (65,), torch.float32), ("d", (2, 64), BF), ("e", (1,), torch.float32), ("f", (7, 9), BF)]
    for name, shape, dt in sizes:
        st.add(name, torch.ones(shape, dtype=dt))
    st.finalize()
    # reverse registration order per dtype, every view rounded up to 64 elements
    assert [(p.name, p.offset) for p in reversed(st.params) if p.dtype == BF] == [("f", 0), ("d", 64), ("b", 192), ("a", 256)]
    assert [(p.name, p.offset) for p in reversed(st.params) if p.dtype == torch.float32] == [("e", 0), ("c", 64)]
    want = {BF: [(63, 64), (271, 320)], torch.float32: [(1, 64), (129, 192)]}
    for dt, gaps in want.items():
        mask = SI.padding_mask(st, dt)
        expect = torch.zeros(st.flat[dt].numel(), dtype=torch.bool)
        for lo, hi in gaps:
            expect[lo:hi] = True
        assert mask.dtype == torch.bool and torch.equal(mask, expect), dt
        assert bool((st.flat[dt][mask] == 0).all()) and bool((st.flat[dt][~mask] == 1).all()), "every owned element was initialised, no gap was"
        assert int(mask.sum()) == st.flat[dt].numel() - sum(p.numel for p in st.params if p.dtype == dt)


# ---- the premises hold for the reference arithmetic ----------------------------------------------------------------------------------------------------
REL = 1e-6


@pytest.fixture(scope="module")
def oracle_world():
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    # (the towers return the output of block depth - 2: the last block's adapters are never run, and the engine does not hold them)
    unused = tuple(f"{p}blocks.{vc.depth - 1}." for p, vc in (("vision_backbone.featurizer.", ocfg.dino), ("vision_backbone.fused_featurizer.", ocfg.siglip)))
    trainable = sorted(k for k in sd if (".lora_" in k or k.startswith(("action_head.", "proprio_projector."))) and not k.startswith(unused))
    return dict(ocfg=ocfg, sd=sd, trainable=trainable, batches=[SI.make_batch(s) for s in SI.BATCH_SEEDS])


def oracle_grads(w, objective, steps):
    """fp32 autograd of the oracle: `steps` = [(batch, loss_scale), ...] backpropagated one after the other into the same .grad (what the
    engine's flat gradient buffers do across micro-steps).  -> (losses, {name: grad})."""
    names = [n for n in w["trainable"] if objective == "l1" or not n.startswith("action_head.")]
    sdg = {k: (v.clone().requires_grad_(True) if k in names else v) for k, v in w["sd"].items()}
    o = vo.Oracle(w["ocfg"], sdg, mode="fp32")
    losses = []
    for batch, scale in steps:
        loss = o.train_forward(batch)[0] if objective == "l1" else o.train_forward_discrete(batch)[0]
        (loss * scale).backward()
        losses.append(loss.item())
    return losses, {n: sdg[n].grad.clone() for n in names}


def assert_close(got, want, what):
    bad = []
    for n in sorted(want):
        assert want[n].norm() > 0, f"{what}: {n} has a zero gradient in the oracle: the identity says nothing about it"
        e = ((got[n] - want[n]).norm() / want[n].norm()).item()
        if not e <= REL:
            bad.append(f"{n}: relative L2 {e:.3e}")
    assert not bad, f"{what}: {len(bad)} tensors beyond {REL}:\n" + "\n".join(bad[:8])


@pytest.mark.parametrize("objective", ["l1", "discrete"])
def test_the_identities_hold_for_the_fp32_oracle(oracle_world, objective):
    """Loss-scale linearity, additivity over two micro-batches and inertness of the ids under the padding, for the L1 and the discrete
    objective on the tiny config: fp32 autograd on the CPU, 1e-6 relative per tensor."""
    w = oracle_world
    b1, b2 = w["batches"]
    (l1,), g1 = oracle_grads(w, objective, [(b1, 1.0)])
    (_,), g2 = oracle_grads(w, objective, [(b2, 1.0)])
    # loss-scale linearity
    (ls,), gs = oracle_grads(w, objective, [(b1, 0.125)])
    assert ls == l1
    assert_close(gs, {n: 0.125 * g for n, g in g1.items()}, f"{objective}: loss_scale 0.125")
    # additivity over two micro-batches at 0.5 each
    _, gacc = oracle_grads(w, objective, [(b1, 0.5), (b2, 0.5)])
    assert_close(gacc, {n: 0.5 * g1[n] + 0.5 * g2[n] for n in g1}, f"{objective}: two micro-batches")
    assert all(((gacc[n] - 0.5 * g2[n]).norm() / gacc[n].norm()).item() > 1e-3 for n in g1), "the first micro-batch matters for every tensor"
    # the ids under the padding
    pad = ~b1["attention_mask"].bool()
    ids = b1["input_ids"].clone()
    ids[pad] = torch.randint(3, 31000, (int(pad.sum()),), generator=torch.Generator().manual_seed(77))
    assert int(pad.sum()) > 0 and bool((ids[pad] != b1["input_ids"][pad]).all()) and bool((b1["labels"][pad] == -100).all())
    (lp,), gp = oracle_grads(w, objective, [(dict(b1, input_ids=ids), 1.0)])
    assert abs(lp - l1) <= REL * abs(l1), (lp, l1)
    assert_close(gp, g1, f"{objective}: ids under the padding rewritten")
