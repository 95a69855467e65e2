"""VLAEngine.sample_action_tokens / policy_logprobs / train_step_policy_gradient on the tiny discrete world of tests/step_invariants.py: the
gradient anchored bit for bit on the cross-entropy pieces, the on-policy ratio, learning in both directions, the two step invariants on the
new step, resume of the token stream, and the refusals."""
import pytest
import torch

from tests import step_invariants as si

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def world(dev):
    w = si.make_world(dev, "discrete")
    eng, batch = w["eng"], w["batches"][0]
    eng.token_sample.seed, eng.token_sample.call = 0xABCDEF0123456789, 5
    w["draw"] = eng.sample_action_tokens(batch, temperature=1.0)          # the fixed drawn chunk the tests below train on
    w["draw_call"] = 5
    return w


def _pg(world, loss_scale=1.0, **kw):
    eng, batch = world["eng"], world["batches"][0]
    eng.zero_grad()
    stats = eng.train_step_policy_gradient(batch, world["draw"]["tokens"], kw.pop("advantages", torch.ones(3)), loss_scale=loss_scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def test_draw_shapes_and_window(world):
    eng, d = world["eng"], world["draw"]
    B, A = 3, world["cfg"].num_action_tokens
    lo, hi = eng.token_window("actions")
    assert (lo, hi) == (31744, 32000)
    for k, dt in (("tokens", torch.int32), ("bins", torch.int32), ("logprob", F32), ("entropy", F32)):
        assert d[k].shape == (B, A) and d[k].dtype == dt and d[k].is_cuda
    assert bool(((d["tokens"] >= lo) & (d["tokens"] < hi)).all())
    assert torch.equal(d["bins"], (32000 - d["tokens"] - 1).clamp(0, 254))
    assert bool((d["logprob"] < 0).all()) and bool((d["entropy"] > 0).all())
    assert eng.token_sample.call == world["draw_call"] + 1
    assert len(set(d["tokens"].reshape(-1).tolist())) > 8                # 168 draws: not one token


def test_gradient_anchor_on_the_cross_entropy_pieces(world):
    """Advantage 1, no old log-probabilities, T = 1, the whole vocabulary: the accumulators of forward -> lm_loss_fwd -> lm_loss_bwd ->
    backward_from_rows on the same rows and targets, bit for bit."""
    eng, batch, f = world["eng"], world["batches"][0], si.Findings()
    ls = 0.5
    stats, got = _pg(world, loss_scale=ls, window="vocab")
    eng.zero_grad()
    out = eng.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"), train=True, sel="actions")
    _, idx = eng.action_hidden(out)
    targets = world["draw"]["tokens"].reshape(-1).to(torch.int64)
    loss_rows, _, dlogits = eng.lm_loss_fwd(out, idx, targets, grad_scale=ls / targets.numel())
    eng.backward_from_rows(eng.lm_loss_bwd(dlogits), idx, out)
    want = si.export_grads(eng)
    f.same_grads(got, want, "policy-gradient step vs the cross-entropy pieces")
    f.every_tensor_nonzero(got, "policy-gradient step")
    f.check(float(stats["ratio"]) == 1.0 and float(stats["clip_frac"]) == 0.0, "ratio / clip fraction without old log-probabilities")
    f.check(abs(float(stats["logprob"]) + float(loss_rows.mean())) < 1e-5 * abs(float(loss_rows.mean())) + 1e-6, "mean logprob vs -mean loss")
    f.done()


def test_on_policy_logprobs_are_the_draws(world):
    eng, batch, d = world["eng"], world["batches"][0], world["draw"]
    pl = eng.policy_logprobs(batch, d["tokens"], temperature=1.0)
    assert torch.equal(pl["logprob"].view(torch.int32), d["logprob"].view(torch.int32)), "policy_logprobs != the draw's logprob bits"
    assert torch.equal(pl["entropy"].view(torch.int32), d["entropy"].view(torch.int32))
    # host tokens, another temperature and window: a different number
    other = eng.policy_logprobs(batch, d["tokens"].cpu(), temperature=1.6, window="vocab")
    assert not torch.equal(other["logprob"], d["logprob"])


def test_reproducible_and_loss_scale_exact(world):
    f = si.Findings()
    s1, g1 = _pg(world, old_logprobs=world["draw"]["logprob"], advantages=torch.tensor([1.0, -0.5, 2.0]), temperature=1.6)
    s2, g2 = _pg(world, old_logprobs=world["draw"]["logprob"], advantages=torch.tensor([1.0, -0.5, 2.0]), temperature=1.6)
    f.same_grads(g1, g2, "two identical steps")
    for k in s1:
        f.same_bits(s1[k], s2[k], f"two identical steps: {k}")
    _, g4 = _pg(world, loss_scale=4.0, old_logprobs=world["draw"]["logprob"], advantages=torch.tensor([1.0, -0.5, 2.0]), temperature=1.6)
    f.same_grads(g4, {n: 4.0 * g for n, g in g1.items()}, "loss_scale = 4 vs 4 x (loss_scale = 1)")
    f.all_finite(g1, "policy-gradient step")
    f.done()


def test_per_token_advantages_and_gating(world):
    """[B, A] advantages; with old log-probabilities one nat above / below the current ones every row is gated on one side of the sign rule."""
    eng, d = world["eng"], world["draw"]
    A = world["cfg"].num_action_tokens
    adv = torch.ones(3, A)
    adv[:, ::2] = -1.0
    stats, g = _pg(world, advantages=adv, old_logprobs=d["logprob"] - 1.0)      # ratio e > 1.2: gated where adv >= 0
    assert abs(float(stats["clip_frac"]) - float((adv >= 0).float().mean())) < 1e-6
    stats, g = _pg(world, advantages=torch.ones(3), old_logprobs=d["logprob"] - 1.0)
    assert float(stats["clip_frac"]) == 1.0
    assert all(not bool((t != 0).any()) for t in g.values()), "every row gated: the gradient must be exactly zero"


@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_it_learns(world, sign):
    eng, batch, d = world["eng"], world["batches"][0], world["draw"]
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    try:
        for st in eng.stores:
            st.init_optimizer()
        before = float(eng.policy_logprobs(batch, d["tokens"])["logprob"].sum())
        for _ in range(6):
            eng.zero_grad()
            eng.train_step_policy_gradient(batch, d["tokens"], torch.full((3,), sign))
            eng.adamw_step(1e-3)
            eng.refresh_derived()
        after = float(eng.policy_logprobs(batch, d["tokens"])["logprob"].sum())
        assert (after - before) * sign > 0.0, f"advantage {sign:+}: summed logprob {before} -> {after}"
    finally:
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()


def test_resume_continues_the_token_stream(world):
    eng, batch = world["eng"], world["batches"][0]
    eng.token_sample.call = 40
    eng.sample_action_tokens(batch)
    sd = {k: v.clone() if torch.is_tensor(v) else v for k, v in eng.optimizer_state_dict().items()}
    assert int(sd["token_sample.call"]) == 41
    uninterrupted = eng.sample_action_tokens(batch)
    eng.token_sample.call = 7
    eng.load_optimizer_state_dict(sd)
    assert eng.token_sample.call == 41
    resumed = eng.sample_action_tokens(batch)
    assert torch.equal(resumed["tokens"], uninterrupted["tokens"]) and torch.equal(resumed["logprob"].view(torch.int32), uninterrupted["logprob"].view(torch.int32))
    assert not torch.equal(eng.sample_action_tokens(batch)["tokens"], resumed["tokens"])      # the next call: another draw
    del sd["token_sample.call"]                                                                # a file from before the stream existed
    eng.load_optimizer_state_dict(sd)
    assert eng.token_sample.call == 0
    # row keys: observation b drawn under key k is the same draw wherever it sits
    eng.token_sample.call = 9
    a = eng.sample_action_tokens(batch, row_keys=[10, 11, 12])
    eng.token_sample.call = 9
    b = eng.sample_action_tokens(batch, row_keys=[10, 99, 12])
    assert torch.equal(a["tokens"][0], b["tokens"][0]) and torch.equal(a["tokens"][2], b["tokens"][2]) and not torch.equal(a["tokens"][1], b["tokens"][1])


def test_refusals(world):
    eng, batch, d = world["eng"], world["batches"][0], world["draw"]
    with pytest.raises(ValueError, match="tokens"):
        eng.train_step_policy_gradient(batch, d["tokens"][:2], torch.ones(3))
    with pytest.raises(ValueError, match="advantages"):
        eng.train_step_policy_gradient(batch, d["tokens"], torch.ones(2))
    with pytest.raises(ValueError, match="window"):
        eng.sample_action_tokens(batch, window="bins")
    ops_err = si.load("openvla-oft_amd._lib").OvlaError
    with pytest.raises(ops_err, match="temperature"):
        eng.sample_action_tokens(batch, temperature=0.0)
    with pytest.raises(ops_err, match="clip_lo"):
        eng.train_step_policy_gradient(batch, d["tokens"], torch.ones(3), clip=(1.2, 0.8))
    if not eng.ema_enabled:            # (the last test of the module: the shadows stay with the world)
        eng.enable_ema()
    with eng.ema_weights():
        with pytest.raises(RuntimeError, match="train_step_policy_gradient inside ema_weights"):
            eng.train_step_policy_gradient(batch, d["tokens"], torch.ones(3))
