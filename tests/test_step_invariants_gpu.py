"""Training-step invariants of `VLAEngine`, bit for bit (helpers and the reasoning: tests/step_invariants.py).

The oracle comparisons (test_engine_gpu.py, test_film_diffusion_gpu.py, test_fullsize_*) are statistical and run one backward into zeroed
gradients; the kernel files pin each launch on its own.  This file pins the layer in between -- how one step strings the launches together
across micro-steps, padded rows, flat buffers and the two vision-tower streams -- with identities that need no oracle: a gradient that is
overwritten instead of accumulated, a loss_scale that misses one path, a pad row that leaks into a weight gradient, a write into the
alignment padding of a flat buffer, a race between the tower streams each break one of them in at least one bit.

Five worlds (step_invariants.make_world): l1, film, diffusion, discrete, l1_dropout; B = 3 with ragged right padding.  The tests of one world
share their reference steps (step_invariants.fresh_step); the tests that move the parameters put them back.
"""
import contextlib
import math

import pytest
import torch

from tests import pointwise_reference as P
from tests import step_invariants as SI

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KINDS = SI.KINDS


@pytest.fixture(scope="module")
def worlds(dev):
    made = {}

    def get(kind):
        if kind not in made:
            made[kind] = SI.make_world(dev, kind)
        return made[kind]

    yield get
    made.clear()


def loss_ref(world, which, res):
    """The restated loss of step result `res` on batch `which` (None for `discrete`: a torch sum in a fixed order)."""
    tgt = SI.step_target(world, which)
    return None if tgt is None else SI.loss_reference(res.pred, tgt, mse=world["kind"] == "diffusion")


@contextlib.contextmanager
def restored(world):
    """The parameters, optimizer state, clipping state and dropout counter of the world as they were, whatever the body did to them."""
    eng = world["eng"]
    snap = [{dt: f.clone() for dt, f in st.flat.items()} for st in eng.stores]
    call = eng.dropout.call
    try:
        yield eng
    finally:
        for st, s in zip(eng.stores, snap):
            for dt, f in st.flat.items():
                f.copy_(s[dt])
            st.exp_avg, st.exp_avg_sq, st.step = {}, {}, 0
        eng._grad_clip = None
        eng.dropout.call = call
        eng.refresh_derived()
        eng.zero_grad()


# ---- the premise: gradients exist, and a step is a pure function of its inputs -----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_gradient_is_finite_and_nonzero(worlds, kind):
    """The invariants below are blind to a gradient that is consistently zero: every exported tensor is finite and has a nonzero element."""
    world = worlds(kind)
    res = SI.fresh_step(world, 0)
    F = SI.Findings()
    names = set(res.grads)
    F.check(names == set(world["eng"].export_trainable("data")) and len(names) > 50, f"{len(names)} gradient tensors")
    F.check(any(".lora_A.weight" in n for n in names) and any("self_attn.q_proj.lora_B" in n for n in names), "LoRA factors of towers and decoder")
    if kind == "film":
        F.check(any(".scale.weight" in n for n in names) and any(".shift.bias" in n for n in names), "film: scale / shift Linears are exported")
    if kind == "diffusion":
        F.check(any(n.startswith("noisy_action_projector.") for n in names), "diffusion: the noisy-action projector is exported")
    if kind == "discrete":
        F.check(not any(n.startswith("action_head.") for n in names), "discrete: no head")
    F.all_finite(res.grads, kind)
    F.every_tensor_nonzero(res.grads, kind)
    F.check(bool(torch.isfinite(res.loss_sum).all()) and float(res.loss_sum) > 0 and res.count > 0, f"loss_sum {res.loss_sum.tolist()} over {res.count}")
    F.done()


@pytest.mark.parametrize("kind", KINDS)
def test_two_identical_steps_give_identical_bits(worlds, kind):
    """From zeroed gradients, twice: the same prediction bits and the same gradient bits for every tensor (stricter than the 5e-6 relative of
    test_full_size_step_is_reproducible, which predates the fixed-order TN reduce); the loss as Findings.same_loss states."""
    world = worlds(kind)
    a = SI.fresh_step(world, 0)
    b = SI.fresh_step(world, 0, memo=False)
    F = SI.Findings()
    F.same_bits(b.pred, a.pred, f"{kind}: predictions")
    ref = loss_ref(world, 0, a)
    if ref is not None:
        print(f"{kind}: loss_sum {float(a.loss_sum)!r} / {float(b.loss_sum)!r}, exact sum of its {ref[1]} terms {ref[0]!r}, order-free in fp32: {ref[2]}")
    F.same_loss(b.loss_sum, a.loss_sum, ref, f"{kind}: loss_sum")
    F.same_grads(b.grads, a.grads, f"{kind}: second run")
    F.done()


# ---- loss_scale reaches every path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_loss_scale_scales_every_gradient_exactly(worlds, kind):
    """s = 0.5, 0.125: grads(s) == s * grads(1) under bit equality for every tensor (a power of two commutes with every bf16 and fp32
    rounding of the backward); predictions and loss do not see the scale."""
    world = worlds(kind)
    one = SI.fresh_step(world, 0)
    F = SI.Findings()
    for s in (0.5, 0.125):
        got = SI.fresh_step(world, 0, loss_scale=s)
        F.same_bits(got.pred, one.pred, f"{kind} scale {s}: predictions")
        F.same_loss(got.loss_sum, one.loss_sum, loss_ref(world, 0, one), f"{kind} scale {s}: loss_sum")
        F.same_grads(got.grads, {n: g * s for n, g in one.grads.items()}, f"{kind} scale {s}")
    F.done()


# ---- every backward ADDS, once per element ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_micro_steps_accumulate_with_one_add_per_element(worlds, kind):
    """zero; step(b1, 0.5); step(b2, 0.5) == G(b1, 0.5) + G(b2, 0.5), the fp32 add done by torch on the device: one rounded add per element,
    as the kernels' single `+=` (an overwrite leaves G(b2); a second add per element rounds twice).  And step(b1); step(b1) == 2 G(b1).
    l1_dropout: the dropout counter is pinned so that the accumulating run's two forwards draw the masks of the two separate runs."""
    world = worlds(kind)
    eng = world["eng"]
    g1, g2 = SI.fresh_step(world, 0, 0.5, call=0), SI.fresh_step(world, 1, 0.5, call=1)
    eng.zero_grad()
    first = SI.step(world, world["batches"][0], 0.5, call=0)
    acc = SI.step(world, world["batches"][1], 0.5)                  # the forward advanced the counter: this one draws with call 1 -> 2, as g2
    F = SI.Findings()
    F.check(kind != "l1_dropout" or eng.dropout.call == 2, f"dropout counter {eng.dropout.call} after two forwards from 0")
    F.same_grads(first.grads, g1.grads, f"{kind}: first micro-step")
    F.same_bits(acc.pred, g2.pred, f"{kind}: predictions of the second micro-step")
    F.same_grads(acc.grads, {n: g1.grads[n] + g2.grads[n] for n in g1.grads}, f"{kind}: G(b1) + G(b2)")
    moved = sum(not torch.equal(acc.grads[n], g2.grads[n]) for n in g2.grads)
    F.check(moved == len(g2.grads), f"{kind}: only {moved} of {len(g2.grads)} tensors differ from G(b2) alone: the comparison above is vacuous for the rest")
    one = SI.fresh_step(world, 0, 1.0, call=0)
    eng.zero_grad()
    SI.step(world, world["batches"][0], 1.0, call=0)
    twice = SI.step(world, world["batches"][0], 1.0, call=0)
    F.same_grads(twice.grads, {n: 2.0 * g for n, g in one.grads.items()}, f"{kind}: the same batch twice")
    F.done()


# ---- pad columns are inert ---------------------------------------------------------------------------------------------------------------------------
def rewrite_pads(batch, seed):
    """The ids under attention_mask == 0 replaced by random valid non-action ids (not the pad id); labels stay IGNORE there."""
    out = dict(batch)
    pad = ~batch["attention_mask"].bool()
    assert int(pad.sum()) > 0 and bool((batch["labels"][pad] == -100).all())
    ids = batch["input_ids"].clone()
    ids[pad] = torch.randint(3, 31000, (int(pad.sum()),), generator=torch.Generator().manual_seed(seed))
    assert bool((ids[pad] != batch["input_ids"][pad]).all())
    out["input_ids"] = ids
    return out


def shorten_longest(batch):
    """The longest row loses two PROMPT tokens (it keeps its action chunk and stop token, moved two places left); its mask and labels follow,
    and the two ids beyond its new end are kept as they were -- an action id and the stop id under mask 0 and label IGNORE.  Every row of the
    batch now ends in padding, the last two columns are padding in all of them."""
    out = dict(batch)
    ids, lab, am = batch["input_ids"].clone(), batch["labels"].clone(), batch["attention_mask"].clone()
    r = int(am.sum(1).argmax())
    n = int(am[r].sum())
    assert n == ids.shape[1] and bool((lab[r, :4] == -100).all())
    ids[r, :n - 2] = torch.cat([batch["input_ids"][r, :1], batch["input_ids"][r, 3:n]])
    lab[r, :n - 2] = torch.cat([batch["labels"][r, :1], batch["labels"][r, 3:n]])
    lab[r, n - 2:] = -100
    am[r, n - 2:] = False
    out.update(input_ids=ids, labels=lab, attention_mask=am)
    return out


@pytest.mark.parametrize("variant", ["ragged", "every_row_padded"])
@pytest.mark.parametrize("kind", KINDS)
def test_ids_under_the_padding_change_nothing(worlds, kind, variant):
    """Loss, predictions and every gradient of a batch are bit-identical to those of the same batch with other ids under its padding: a pad
    position is masked as a key, and its own rows carry an exactly zero gradient into the LoRA weight-gradient GEMMs, which contract over
    all B * S rows.  `every_row_padded`: the same on the batch whose longest row was shortened (shorten_longest).
    film: the reference's FiLM average includes the pad positions (VLAEngine.language_average), so the ids under the padding legitimately
    reach the loss through it; both runs are handed the average of the unmodified batch (train_step_fwd_bwd(film_avg=...))."""
    world = worlds(kind)
    eng, dev = world["eng"], world["eng"].device
    base = world["batches"][0] if variant == "ragged" else shorten_longest(world["batches"][0])
    other = rewrite_pads(base, seed=77)
    kw = dict(diffusion=world["diffusion"][0]) if kind == "diffusion" else {}
    if kind == "film":
        kw["film_avg"] = eng.language_average(base["input_ids"].to(dev), base["labels"].to(dev))
    runs = []
    for b in (base, other):
        eng.zero_grad()
        runs.append(SI.step(world, b, 1.0, call=0, **kw))
    F = SI.Findings()
    if variant == "ragged":       # (film: the explicit average is the one the step computes itself)
        F.same_grads(runs[0].grads, SI.fresh_step(world, 0).grads, f"{kind}: the unmodified batch against the shared reference step")
    F.every_tensor_nonzero(runs[0].grads, f"{kind} {variant}")
    F.same_bits(runs[1].pred, runs[0].pred, f"{kind} {variant}: predictions")
    F.same_loss(runs[1].loss_sum, runs[0].loss_sum, loss_ref(world, 0, runs[0]), f"{kind} {variant}: loss_sum")
    F.same_grads(runs[1].grads, runs[0].grads, f"{kind} {variant}: ids under the padding rewritten")
    F.done()


# ---- the two tower streams ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["l1", "film"])
def test_one_tower_stream_or_two_same_bits(worlds, kind, monkeypatch):
    """OVLA_VIT_STREAMS=1 (both towers on the main stream, read per call) against the default two streams, twice: the same loss, predictions
    and gradients.  A tower that ran ahead of its inputs, or shared a workspace with the other, would differ from the serial run."""
    world = worlds(kind)
    F = SI.Findings()
    for rnd in range(2):
        monkeypatch.delenv("OVLA_VIT_STREAMS", raising=False)
        two = SI.fresh_step(world, 0, memo=False)
        F.check(world["eng"]._side_stream() is not None, "the default run uses the side stream")
        monkeypatch.setenv("OVLA_VIT_STREAMS", "1")
        F.check(world["eng"]._side_stream() is None, "OVLA_VIT_STREAMS=1 is read per call")
        one = SI.fresh_step(world, 0, memo=False)
        F.same_bits(one.pred, two.pred, f"{kind} round {rnd}: predictions")
        F.same_loss(one.loss_sum, two.loss_sum, loss_ref(world, 0, two), f"{kind} round {rnd}: loss_sum")
        F.same_grads(one.grads, two.grads, f"{kind} round {rnd}: one stream against two")
    F.done()


# ---- the flat buffers ----------------------------------------------------------------------------------------------------------------------------------
def full_linears(eng):
    engine_mod = SI.load("openvla-oft_amd.engine")
    return [lin for lin in eng.all_linears() if isinstance(lin, engine_mod.FullLinear)]


@pytest.mark.parametrize("kind", KINDS)
def test_alignment_padding_and_padded_columns_stay_zero(worlds, kind):
    """After a backward the elements of every flat gradient buffer that no Param owns are exactly zero (ovla_grad_sumsq sums the whole
    buffer: a stray value would change the clip coefficient); after two optimizer steps (a plain and a clipped one) so are those of the
    parameters and both moments, and the zero-padded input columns of every FullLinear (the noisy-action projector: 1 padded to 8).
    With clipping enabled, the norm of grad_clip_stats() is the float64 norm of the exported, unpadded gradients -- each rounded to bf16
    where its parameter is bf16, as ovla_grad_sumsq sees it -- rounded to fp32: test_grad_clip_gpu.py pins that quantity bit for bit to a
    restatement in the kernel's order; from another order of the same double sum it is within half an fp32 ulp (2^-24 relative) plus the
    order's own error, below n 2^-53 < 1e-9 for these n < 4e6 elements."""
    world = worlds(kind)
    F = SI.Findings()
    with restored(world) as eng:
        gaps = 0
        for k in range(2):
            eng.zero_grad()
            SI.step(world, world["batches"][k], 1.0, call=k)
            for i, st in enumerate(eng.stores):
                for dt, g in st.flat_grad.items():
                    mask = SI.padding_mask(st, dt)
                    gaps += int(mask.sum())
                    F.all_zero(g[mask], f"{kind} step {k}: store {i} {dt} flat_grad, alignment padding")
            if k == 1:
                data, grads = eng.export_trainable("data"), eng.export_trainable("grad")
                total = sum(float(((g.to(BF) if data[n].dtype == BF else g).double() ** 2).sum()) for n, g in grads.items())
                want = math.sqrt(total)
                eng.enable_grad_clip(max_norm=0.25 * want)
            eng.adamw_step(lr=5e-4)
            eng.refresh_derived()
        stats = eng.grad_clip_stats()
        print(f"{kind}: gradient norm {stats['norm']!r}, float64 norm of the exported gradients {want!r}, coef {stats['coef']!r}")
        F.check(abs(stats["norm"] - want) <= want * (2.0 ** -24 + 1e-9), f"{kind}: grad_clip_stats norm {stats['norm']!r} against the exported gradients' {want!r}")
        F.check(0.2 < stats["coef"] < 0.3 and (stats["steps"], stats["clipped"], stats["skipped"]) == (1, 1, 0), f"{kind}: the second step was clipped: {stats}")
        # (discrete: no head; its stores hold LoRA factors and the proprio projector only, every size a multiple of 64 -- no gap exists there)
        F.check(gaps > 0 or kind == "discrete", f"{kind}: the flat buffers have no alignment padding at all: nothing was checked")
        for i, st in enumerate(eng.stores):
            for dt in st.flat:
                mask = SI.padding_mask(st, dt)
                for what, buf in (("flat", st.flat[dt]), ("exp_avg", st.exp_avg[dt]), ("exp_avg_sq", st.exp_avg_sq[dt])):
                    F.all_zero(buf[mask], f"{kind}: store {i} {dt} {what} after two optimizer steps, alignment padding")
                F.check(bool((st.exp_avg_sq[dt][~mask] != 0).any()), f"{kind}: store {i} {dt}: the optimizer moved nothing")
        padded = [lin for lin in full_linears(eng) if lin.in_pad != lin.in_f]
        F.check(kind != "diffusion" or any(lin.in_f == 1 and lin.in_pad == 8 for lin in padded), "diffusion: the noisy-action projector's fc1 is padded 1 -> 8")
        for lin in padded:
            F.all_zero(lin.W.grad[:, lin.in_f:], f"{kind}: {lin.name} W.grad[:, {lin.in_f}:]")
            F.all_zero(lin.W.data[:, lin.in_f:], f"{kind}: {lin.name} W.data[:, {lin.in_f}:]")
    F.done()


@pytest.mark.parametrize("kind", KINDS)
def test_derived_copies_follow_the_optimizer(worlds, kind):
    """After a step, adamw_step and refresh_derived(): A^T, the stacked B_g^T and W^T hold the torch transposes of what derived_pairs() names,
    and every fp32-master FullLinear's compute copies are the bf16 (RNE) casts of its parameters."""
    world = worlds(kind)
    engine_mod = SI.load("openvla-oft_amd.engine")
    F = SI.Findings()
    with restored(world) as eng:
        before = [{dt: f.clone() for dt, f in st.flat.items()} for st in eng.stores]
        eng.zero_grad()
        SI.step(world, world["batches"][0], 1.0, call=0)
        eng.adamw_step(lr=5e-4)
        eng.refresh_derived()
        for i, st in enumerate(eng.stores):
            for dt, f in st.flat.items():
                F.check(not torch.equal(f, before[i][dt]), f"{kind}: store {i} {dt}: the optimizer step changed no parameter")
        pairs = masters = 0
        for lin in eng.all_linears():
            if isinstance(lin, engine_mod.LoraLinear):
                if lin.WT is not None:
                    F.same_bits(lin.WT, lin.W.t().contiguous(), f"{kind}: {lin.name} WT")
                for j, (src, dst) in enumerate(lin.derived_pairs()):
                    pairs += 1
                    F.same_bits(dst, src.t().contiguous(), f"{kind}: {lin.name} derived pair {j} ({'AT' if j == 0 else 'BT'})")
            elif lin.master_fp32:
                masters += 1
                F.same_bits(lin.Wc, lin.W.data.to(BF), f"{kind}: {lin.name} Wc")
                if lin.b is not None:
                    F.same_bits(lin.bc, lin.b.data.to(BF), f"{kind}: {lin.name} bc")
        F.check(pairs > 40 and masters >= 2, f"{kind}: {pairs} derived pairs, {masters} fp32-master linears")
    F.done()


# ---- malformed action labels ---------------------------------------------------------------------------------------------------------------------------
def test_gather_rows_takes_a_negative_index_as_no_row(ops, dev):
    """Kernel level (the suite and its planted bug: tests/pointwise_reference.py::suite_gather_no_row, test_pointwise_reference.py): indices
    [3, -1, 0, 7]; the gather leaves a zero row at position 1, the scatter-add skips the entry; whole buffers, guards included."""
    fails = P.Checks()
    P.suite_gather_no_row(fails, P.GpuKernels(ops, dev, fails))
    fails.done()


def malformed(batch, how):
    out = dict(batch)
    lab = batch["labels"].clone()
    pos = (lab[1] > 31743).nonzero().reshape(-1)
    assert pos.numel() == 56
    if how == "one_short":
        lab[1, int(pos[-1])] = -100            # the last action label of row 1: a truncated sample
    else:
        assert int(lab[1, 2]) == -100
        lab[1, 2] = 31800                      # one more, on a prompt position
    out["labels"] = lab
    return out


@pytest.mark.parametrize("how,count", [("one_short", 55), ("one_more", 57)])
def test_malformed_action_labels_are_refused_before_anything_is_staged(worlds, how, count):
    """A row with 55 or 57 action labels raises ValueError naming the row and the count from forward, train_step_fwd_bwd and
    train_step_discrete, and the device allocation is what it was: nothing was uploaded or launched."""
    l1, disc = worlds("l1"), worlds("discrete")
    bad = malformed(l1["batches"][0], how)
    calls = [("forward", lambda: l1["eng"].forward(bad["input_ids"], bad["attention_mask"], bad["pixel_values"], bad["labels"], proprio=bad["proprio"], train=False)),
             ("train_step_fwd_bwd", lambda: l1["eng"].train_step_fwd_bwd(bad)),
             ("train_step_discrete", lambda: disc["eng"].train_step_discrete(bad))]
    for who, call in calls:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError, match=f"row 1 holds {count} action labels"):
            call()
        assert torch.cuda.memory_allocated() == before, f"{who}: {torch.cuda.memory_allocated() - before} bytes were staged before the refusal"
    good = l1["batches"][0]
    l1["eng"].check_action_labels(good["labels"], l1["cfg"].num_action_tokens)


def test_device_resident_short_labels_stay_inside_their_buffers(worlds):
    """Labels that live on the device cannot be checked without a synchronisation: the missing slot stays -1 in action_rows and
    ovla_gather_rows takes it as "no row", so the inference forward on the selected rows reads nothing outside its buffers and returns
    finite rows -- and the rows of the well-formed samples are those of the well-formed batch."""
    world = worlds("l1")
    eng, dev = world["eng"], world["eng"].device
    good, bad = world["batches"][0], malformed(world["batches"][0], "one_short")
    run = lambda b: eng.forward(b["input_ids"].to(dev), b["attention_mask"], b["pixel_values"], b["labels"].to(dev), proprio=b["proprio"], train=False, sel="actions")  # noqa: E731
    ref, out = run(good), run(bad)
    rows = out["action_rows"].cpu()
    assert int((rows < 0).sum()) == 1 and int(rows[1, 55]) == -1 and torch.equal(rows[:, :55], ref["action_rows"].cpu()[:, :55])
    ah, ah_ref = out["action_hidden"].view(3, 56, -1), ref["action_hidden"].view(3, 56, -1)
    assert bool(torch.isfinite(ah.float()).all())
    assert torch.equal(ah[0], ah_ref[0]) and torch.equal(ah[2], ah_ref[2]), "the other samples do not see row 1's labels"
