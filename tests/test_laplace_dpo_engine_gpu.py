"""Preference optimisation through the engine on the tiny L1 world of tests/step_invariants.py (B = 3, chunk 8, action_dim 7): the DPO step's
accumulators are the group step's on the pair with the advantages (+coef, -coef) bit for bit, a fresh scale head at b0 = 1 is the fixed scale 1.0,
the step issues the group step's launches with ovla_laplace_dpo in place of ovla_laplace_pg(_rows), the NLL term alone is the G = 1 group step on the
chosen chunk, one optimizer step widens the margin, and rl.preference_pairs / dpo_step_continuous / online_dpo_step_continuous with their refusals."""
import importlib

import numpy as np
import pytest
import torch

from tests import step_invariants as si

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
SCALE = [0.3, 1.0, 0.05, 0.5, 0.7, 0.25, 0.1]
PRE = "action_scale_head."
WEIGHTS = torch.tensor([1.0, 0.5, 2.0])
load = importlib.import_module


def split(grads):
    return {n: g for n, g in grads.items() if not n.startswith(PRE)}, {n: g for n, g in grads.items() if n.startswith(PRE)}


def set_head(eng, weight=None, bias=None):
    """The scale head's parameters: `weight` a float (uniform(-weight, weight), seeded) or None (zeros); `bias` a list of scales b0 or None (0)."""
    sh = eng.scale_head
    g = torch.Generator().manual_seed(17)
    w = torch.zeros(sh.w.shape) if weight is None else (torch.rand(sh.w.shape, generator=g) * 2 - 1) * weight
    b = torch.zeros(sh.b.shape) if bias is None else torch.tensor(bias).log()
    sh.w.data.copy_(w.to(eng.device, BF)), sh.b.data.copy_(b.to(eng.device, BF))


@pytest.fixture(scope="module")
def world(dev):
    w = si.make_world(dev, "l1")
    eng, batch = w["eng"], w["batches"][0]
    eng.token_sample.seed, eng.token_sample.call = 0xABCDEF0123456789, 6
    eng.attach_scale_head(1.0)
    mean = eng.action_logprobs(batch, torch.zeros(3, 1, 8, 7), 1.0)["mean"].float()
    g = torch.Generator().manual_seed(23)
    off = lambda lo: ((torch.randint(lo, 65, (3, 8, 7), generator=g).float() / 64.0) * torch.where(torch.rand((3, 8, 7), generator=g) < 0.5, -1.0, 1.0)).to(dev)   # noqa: E731
    w["pairs"] = dict(chosen=mean + 0.5 * off(8), rejected=mean + off(8), ref=(mean + 0.0625).to(BF), mean=mean)
    return w


def _launches(monkeypatch, fn):
    lib, names = load("openvla-oft_amd._lib"), []
    real = lib.check
    with monkeypatch.context() as m:
        m.setattr(lib, "check", lambda rc, what: (names.append(what), real(rc, what))[1])
        out = fn()
    return names, out


def _dpo(world, scale, chosen=None, rejected=None, **kw):
    eng, batch, p = world["eng"], world["batches"][0], world["pairs"]
    kw.setdefault("ref_means", p["ref"])
    eng.zero_grad()
    stats = eng.train_step_action_dpo(batch, p["chosen"] if chosen is None else chosen, p["rejected"] if rejected is None else rejected, scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def _group(world, actions, advantages, scale, **kw):
    eng, batch = world["eng"], world["batches"][0]
    eng.zero_grad()
    stats = eng.train_step_action_pg_group(batch, actions, advantages, scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


@pytest.mark.parametrize("learned", (False, True), ids=("fixed", "learned"))
def test_the_step_is_the_group_step_on_the_pair(world, learned):
    eng, p, f = world["eng"], world["pairs"], si.Findings()
    B, C = 3, 8
    set_head(eng, weight=0.02, bias=SCALE)
    scale = "learned" if learned else SCALE
    extra = {}
    if learned:
        ls = eng.action_logprobs(world["batches"][0], torch.zeros(3, 1, 8, 7), "learned")["log_scale"].float()
        f.check(float(ls.std()) > 0.05, "the head's widths vary")
        extra["ref_log_scales"] = (ls - 0.25).to(BF)
    pair = torch.stack([p["chosen"], p["rejected"]], dim=1)           # [B, 2, chunk, action_dim]
    try:
        for loss_type, nll_coef, loss_scale in (("sigmoid", 0.0, 1.0), ("sigmoid", 0.5, 4.0), ("ipo", 0.0, 1.0)):
            kw = dict(beta=0.05, weights=WEIGHTS, label_smoothing=0.1, loss_type=loss_type, nll_coef=nll_coef, loss_scale=loss_scale, **extra)
            stats, grads = _dpo(world, scale, **kw)
            coef = stats["coef"]
            f.check(coef.shape == (B,) and coef.dtype == F32 and bool((coef != 0).all()) and bool(torch.isfinite(coef).all()), f"coef {coef}")
            first = coef
            if nll_coef > 0:                                            # the launch's own rounding: (nll_coef w) nll_scale, then one add
                first = coef + (torch.tensor(nll_coef, dtype=F32, device=eng.device) * WEIGHTS.to(eng.device)) * torch.tensor(loss_scale / (B * C), dtype=F32, device=eng.device)
            adv = torch.stack([first, -coef], dim=1)
            _, want = _group(world, pair, adv, scale, loss_scale=float(B * C * 2))      # the group step's own grad_scale is then exactly 1
            tag = f"{loss_type}, nll_coef {nll_coef}, loss_scale {loss_scale}"
            f.same_grads(grads, want, f"train_step_action_dpo vs the group step on the pair ({tag})")
            f.all_finite(grads, tag), f.every_tensor_nonzero(grads if learned else split(grads)[0], tag)
            f.check(set(stats) == {"loss", "margin", "reward_chosen", "reward_rejected", "accuracy", "logprob_chosen", "logprob_rejected", "coef"}, f"statistics {sorted(stats)}")
            f.check(all(v.device == eng.device and bool(torch.isfinite(v).all()) for v in stats.values()), "finite statistics on the device")
            f.check(abs(float(stats["margin"]) * 0.05 - (float(stats["reward_chosen"]) - float(stats["reward_rejected"]))) < 1e-4 * max(1.0, abs(float(stats["margin"]))),
                    "beta margin = reward_chosen - reward_rejected")
            same, grads2 = _dpo(world, scale, **kw)
            f.same_grads(grads2, grads, f"two identical steps ({tag})"), f.same_bits(same["coef"], coef, "coef of two identical steps")
    finally:
        eng.zero_grad()
    f.done()


def test_fresh_scale_head_at_one_is_the_fixed_scale(world):
    eng, f = world["eng"], si.Findings()
    set_head(eng)
    try:
        kw = dict(beta=0.05, weights=WEIGHTS, label_smoothing=0.1, nll_coef=0.5)
        s_want, g_want = _dpo(world, 1.0, **kw)
        s_got, g_got = _dpo(world, "learned", ref_log_scales=torch.zeros(3, 8, 7), **kw)
        rest, own = split(g_got)
        f.same_grads(rest, split(g_want)[0], "every accumulator outside the scale head's store: learned (b0 = 1) vs scale = 1.0")
        for k in s_want:
            f.same_bits(s_got[k], s_want[k], f"statistics: {k}")
        f.every_tensor_nonzero(own, "the scale head's accumulators")
        f.check(all(not bool((g != 0).any()) for g in split(g_want)[1].values()), "the numeric-scale step leaves the scale head's accumulators at zero")
        pref_fixed = eng.action_preference(world["batches"][0], world["pairs"]["chosen"], world["pairs"]["rejected"], 1.0, beta=0.05, ref_means=world["pairs"]["ref"],
                                           weights=WEIGHTS, label_smoothing=0.1)
        for k in ("loss", "margin", "accuracy", "reward_chosen", "logprob_rejected"):
            # (the training and the inference forward agree in bits on this world -- no dropout, the same schedules)
            f.same_bits(pref_fixed[k], s_want[k], f"action_preference vs the step's statistics: {k}")
    finally:
        eng.zero_grad()
    f.done()


def test_launch_list(world, monkeypatch):
    eng, batch, p = world["eng"], world["batches"][0], world["pairs"]
    set_head(eng, weight=0.02, bias=SCALE)
    pair, adv = torch.stack([p["chosen"], p["rejected"]], dim=1), torch.tensor([[1.0, -1.0]] * 3)
    try:
        for scale, shipped, extra in ((SCALE, "ovla_laplace_pg", {}), ("learned", "ovla_laplace_pg_rows", dict(ref_log_scales=torch.zeros(3, 8, 7)))):
            eng.zero_grad()
            grp, _ = _launches(monkeypatch, lambda: eng.train_step_action_pg_group(batch, pair, adv, scale))
            eng.zero_grad()
            dpo, _ = _launches(monkeypatch, lambda: eng.train_step_action_dpo(batch, p["chosen"], p["rejected"], scale, beta=0.05, ref_means=p["ref"], weights=WEIGHTS, **extra))
            assert grp.count(shipped) == 1 and "ovla_laplace_dpo" not in grp, "the group step issues what it issued before"
            assert dpo.count("ovla_laplace_dpo") == 1 and "ovla_laplace_pg" not in dpo and "ovla_laplace_pg_rows" not in dpo
            assert dpo == ["ovla_laplace_dpo" if n == shipped else n for n in grp], "the step's launches are the group step's, in its order: one forward, one backward"
            eng.zero_grad()
            l1, _ = _launches(monkeypatch, lambda: eng.train_step_fwd_bwd(batch))
            assert "ovla_laplace_dpo" not in l1
            inf, _ = _launches(monkeypatch, lambda: eng.action_logprobs(batch, pair, scale))
            prf, _ = _launches(monkeypatch, lambda: eng.action_preference(batch, p["chosen"], p["rejected"], scale, beta=0.05, ref_means=p["ref"], **extra))
            assert prf == ["ovla_laplace_dpo" if n == shipped else n for n in inf], "action_preference is the inference forward and the one launch"
    finally:
        eng.zero_grad()


def test_nll_alone_is_the_group_step_on_the_chosen_chunk(world):
    eng, batch, f = world["eng"], world["batches"][0], si.Findings()
    demo = batch["actions"].to(BF).float().reshape(3, 8, 7)
    try:
        for loss_scale in (1.0, 0.5):
            stats, grads = _dpo(world, 1.0, chosen=demo, rejected=torch.zeros(3, 8, 7), beta=0.0, nll_coef=1.0, loss_scale=loss_scale)
            _, want = _group(world, demo[:, None], torch.ones(3, 1), 1.0, loss_scale=loss_scale)
            f.same_grads(grads, want, f"beta = 0, nll_coef = 1 vs the group step at G = 1, adv = 1 (loss_scale {loss_scale})")
            f.check(not bool((stats["coef"] != 0).any()), "beta = 0: coef is 0")
            f.every_tensor_nonzero(split(grads)[0], "the NLL term alone")
    finally:
        eng.zero_grad()
    f.done()


def test_first_order_effect(world):
    """One small AdamW step on the preference loss widens the margin of the same pairs.  The margin is piecewise linear in the prediction with
    kinks at the two chunks, and an AdamW step moves every parameter by about the learning rate whatever the gradient's size (see
    test_laplace_pg_engine_gpu.test_first_order_effect: lr = 1e-4 moves the prediction by a few hundredths): "first order" needs the kinks
    well beyond that, so the pair lies two units on either side of the prediction -- every element then has the slope 2 / b towards the chosen
    chunk and none can cross a kink.  (With the world's own pairs, 1/16 from the prediction, the same step carries it past them.)"""
    eng, batch, p = world["eng"], world["batches"][0], world["pairs"]
    set_head(eng)
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    kw = dict(beta=0.05, ref_means=p["ref"])
    side = torch.where(torch.rand((3, 8, 7), generator=torch.Generator().manual_seed(29)) < 0.5, -2.0, 2.0).to(eng.device)
    far = dict(chosen=p["mean"] + side, rejected=p["mean"] - side)
    try:
        for st in eng.stores:
            st.init_optimizer()
        before = eng.action_preference(batch, far["chosen"], far["rejected"], 1.0, **kw)
        eng.zero_grad()
        eng.train_step_action_dpo(batch, far["chosen"], far["rejected"], 1.0, **kw)
        eng.adamw_step(1e-4)
        eng.refresh_derived()
        after = eng.action_preference(batch, far["chosen"], far["rejected"], 1.0, **kw)
        assert float(after["margin"]) > float(before["margin"]), f"margin {float(before['margin'])} -> {float(after['margin'])}"
        assert float(after["loss"]) < float(before["loss"]), f"loss {float(before['loss'])} -> {float(after['loss'])}"
    finally:
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()


def test_preference_pairs(dev):
    rl = load("openvla-oft_amd.rl")
    g = torch.Generator().manual_seed(2)
    actions = torch.randn((4, 5, 8, 7), generator=g).to(dev)
    rewards = torch.tensor([[1.0, 3.0, 3.0, 0.0, 0.0], [2.0, 2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 5.0, -1.0, 5.0], [0.5, 0.25, 0.75, 0.25, 0.5]]).to(dev)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                          # a readback would raise
    try:
        chosen, rejected, weight = rl.preference_pairs(actions, rewards)
        _, _, gapped = rl.preference_pairs(actions, rewards, min_gap=3.0)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    hi, lo = rewards.cpu().numpy().argmax(1), rewards.cpu().numpy().argmin(1)      # (numpy: the first occurrence)
    assert list(hi) == [1, 0, 2, 2] and list(lo) == [3, 0, 1, 1]
    for b in range(4):
        assert torch.equal(chosen[b], actions[b, hi[b]]) and torch.equal(rejected[b], actions[b, lo[b]]), f"group {b}"
    assert chosen.shape == (4, 8, 7) and weight.dtype == F32 and weight.device == actions.device
    assert weight.tolist() == [1.0, 0.0, 1.0, 1.0], "a tied group gets weight 0"
    assert gapped.tolist() == [0.0, 0.0, 1.0, 0.0], "max - min <= min_gap gets weight 0"
    with pytest.raises(ValueError, match="rewards"):
        rl.preference_pairs(actions, rewards[:, :4])


def test_rl_steps_and_refusals(world, dev):
    eng, batch, cfg, p, f = world["eng"], world["batches"][0], world["cfg"], world["pairs"], si.Findings()
    rl = load("openvla-oft_amd.rl")
    set_head(eng, weight=0.02, bias=SCALE)
    seen = []

    def reward_fn(b, actions):
        seen.append(actions.detach().clone())
        target = b["actions"].to(actions.device, F32).reshape(3, 1, cfg.chunk, cfg.action_dim)
        return -(actions - target).abs().mean((2, 3))

    with pytest.raises(ValueError, match="reference"):
        rl.dpo_step_continuous(eng, batch, p["chosen"], p["rejected"], scale=1.0, beta=0.05)
    with pytest.raises(ValueError, match="reference"):
        rl.online_dpo_step_continuous(eng, batch, reward_fn, group_size=4, scale=1.0, beta=0.05)
    f.check(eng.token_sample.call == 6 and not seen, "a refused call draws nothing")
    eng.set_reference_policy()
    try:
        for scale in (1.0, "learned"):
            eng.zero_grad()
            stats = rl.dpo_step_continuous(eng, batch, p["chosen"], p["rejected"], scale=scale, beta=0.05, weights=WEIGHTS, nll_coef=0.1, inner_steps=2)
            grads = si.export_grads(eng)
            f.check(bool(torch.isfinite(stats["loss"])) and float(stats["reward_chosen"]) == 0.0 and float(stats["margin"]) == 0.0, f"on-policy reference: {stats}")
            f.all_finite(grads, f"dpo_step_continuous({scale})"), f.every_tensor_nonzero(grads if scale == "learned" else split(grads)[0], f"dpo_step_continuous({scale})")
            # given means take the place of the snapshot's
            eng.zero_grad()
            given = rl.dpo_step_continuous(eng, batch, p["chosen"], p["rejected"], scale=scale, beta=0.05, weights=WEIGHTS, nll_coef=0.1,
                                           ref_means=eng.reference_action_means(batch), ref_log_scales=eng.reference_action_policy(batch)["log_scale"] if scale == "learned" else None)
            f.same_bits(given["coef"], stats["coef"], "ref_means given vs fetched")
            # online: the reward function sees the clamped draws, the step works on the raw ones
            seen.clear()
            eng.token_sample.call = 50
            eng.zero_grad()
            online = rl.online_dpo_step_continuous(eng, batch, reward_fn, group_size=4, scale=scale, beta=0.05)
            g_online = si.export_grads(eng)
            f.check(eng.token_sample.call == 51 and len(seen) == 1 and tuple(seen[0].shape) == (3, 4, 8, 7), "one draw of G = 4, one reward call")
            eng.token_sample.call = 50
            draw = eng.sample_actions_laplace(batch, scale, num_samples=4)
            f.check(float(draw["actions"].abs().max()) > 1.0 and float(seen[0].abs().max()) <= 1.0, "reward_fn sees the clamped draws")
            f.same_bits(seen[0], draw["actions"].clamp(-1.0, 1.0), "the clamped draws")
            chosen, rejected, weight = rl.preference_pairs(draw["actions"], reward_fn(batch, seen[0]))
            eng.zero_grad()
            rl.dpo_step_continuous(eng, batch, chosen, rejected, scale=scale, beta=0.05, weights=weight)
            f.same_grads(si.export_grads(eng), g_online, f"online step ({scale}) vs the DPO step on the RAW best and worst draw")
            f.check({"reward", "weights", "loss", "margin", "accuracy", "coef"} <= set(online) and bool((online["weights"] == 1).all()), f"online statistics {sorted(online)}")
            f.all_finite(g_online, "online"), f.every_tensor_nonzero(g_online if scale == "learned" else split(g_online)[0], "online")
        # the engine's refusals
        kw = dict(beta=0.05, ref_means=p["ref"])
        with pytest.raises(ValueError, match="ref_log_scales"):
            eng.train_step_action_dpo(batch, p["chosen"], p["rejected"], 1.0, ref_log_scales=torch.zeros(3, 8, 7), **kw)
        with pytest.raises(ValueError, match="come together"):
            eng.train_step_action_dpo(batch, p["chosen"], p["rejected"], "learned", **kw)
        with pytest.raises(ValueError, match="ref_means"):
            eng.train_step_action_dpo(batch, p["chosen"], p["rejected"], 1.0, beta=0.05, ref_means=None)
        for bad in (dict(beta=-1.0), dict(beta=float("nan")), dict(label_smoothing=0.5), dict(nll_coef=-1.0), dict(loss_type="hinge"), dict(loss_type="ipo", beta=0.0)):
            with pytest.raises(ValueError):
                eng.train_step_action_dpo(batch, p["chosen"], p["rejected"], 1.0, **{**kw, **bad})
        with pytest.raises(ValueError, match="chosen"):
            eng.train_step_action_dpo(batch, p["chosen"][:2], p["rejected"], 1.0, **kw)
        with eng.reference_policy():
            with pytest.raises(RuntimeError, match="reference_policy"):
                eng.train_step_action_dpo(batch, p["chosen"], p["rejected"], 1.0, **kw)
    finally:
        eng.drop_reference_policy()
        eng.zero_grad()
    # inside ema_weights(), and an engine without the L1 head
    other = si.make_world(dev, "l1")["eng"]
    other.enable_ema()
    with other.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            other.train_step_action_dpo(batch, p["chosen"], p["rejected"], 1.0, beta=0.05, ref_means=p["ref"])
    disc = si.make_world(dev, "discrete")
    for name in ("train_step_action_dpo", "action_preference"):
        with pytest.raises(RuntimeError, match="head='l1'"):
            getattr(disc["eng"], name)(disc["batches"][0], p["chosen"], p["rejected"], 1.0, beta=0.05, ref_means=p["ref"])
    with pytest.raises(RuntimeError, match="head='l1'"):
        rl.dpo_step_continuous(disc["eng"], disc["batches"][0], p["chosen"], p["rejected"], scale=1.0, beta=0.05, ref_means=p["ref"])
    f.done()
