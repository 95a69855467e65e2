"""The Laplace policy through the engine on the tiny L1 world of tests/step_invariants.py (B = 3, chunk 8, action_dim 7):
train_step_action_pg_group anchored bit for bit on the existing L1 step, G draws from one forward and one launch, the frozen reference policy's
closed-form KL, the first-order effect of a step, rl.grpo_step_continuous, and predict_action / predict_action_batch with action_noise_scale."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import step_invariants as si

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
SCALE = [0.3, 1.0, 0.05, 0.5, 0.7, 0.25, 0.1]
ADV4 = torch.tensor([[1.0, -0.5, 2.0, -1.0], [0.25, 0.5, -2.0, 1.0], [-1.0, -1.0, 3.0, 0.5]])
load = importlib.import_module


def i32(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


@pytest.fixture(scope="module")
def world(dev):
    w = si.make_world(dev, "l1")
    eng, batch = w["eng"], w["batches"][0]
    eng.token_sample.seed, eng.token_sample.call = 0xABCDEF0123456789, 6
    w["keys4"] = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23], [7, 5, 3, -1]])
    w["draw4"] = eng.sample_actions_laplace(batch, SCALE, num_samples=4, row_keys=w["keys4"])
    return w


def _group(world, actions, advantages, scale=SCALE, loss_scale=1.0, **kw):
    eng, batch = world["eng"], world["batches"][0]
    eng.zero_grad()
    stats = eng.train_step_action_pg_group(batch, actions, advantages, scale, loss_scale=loss_scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def _launches(monkeypatch, fn):
    lib, names = load("openvla-oft_amd._lib"), []
    real = lib.check
    with monkeypatch.context() as m:
        m.setattr(lib, "check", lambda rc, what: (names.append(what), real(rc, what))[1])
        out = fn()
    return names, out


def test_anchor_on_the_l1_step(world):
    """The batch's bf16 target chunk as the single draw, adv = 1, scale = 1, loss_scale = 1: dpred = bf16(sign(pred - target) / 24), what
    train_step_fwd_bwd(loss_scale = action_dim) hands its head (7 / (24 * 7) and 1 / 24 are the same correctly rounded quotient) -- the same
    accumulators bit for bit, through a different kernel."""
    eng, batch, cfg, f = world["eng"], world["batches"][0], world["cfg"], si.Findings()
    want = si.fresh_step(world, 0, loss_scale=float(cfg.action_dim), memo=False)
    f.every_tensor_nonzero(want.grads, "the L1 step")
    target = batch["actions"].to(BF).float().reshape(3, 1, cfg.chunk, cfg.action_dim)
    s, got = _group(world, target, torch.ones(3, 1), scale=1.0)
    f.same_grads(got, want.grads, "train_step_action_pg_group on the target chunk vs train_step_fwd_bwd(loss_scale = action_dim)")
    f.check(float(s["ratio"]) == 1.0 and float(s["clip_frac"]) == 0.0 and float(s["kl"]) == 0.0 and float(s["loss"]) == -1.0, f"statistics {s}")
    # the log-probability at scale 1 is -(L1 distance + action_dim log 2) per chunk step
    l1 = (want.pred.float() - si.step_target(world, 0).to(want.pred.device).float()).abs().sum(1)
    lp = -(l1 + cfg.action_dim * float(np.log(2.0))).mean()
    f.check(abs(float(s["logprob"]) - float(lp)) <= 1e-5 * abs(float(lp)), f"logprob {float(s['logprob'])} vs {float(lp)}")
    f.done()


def test_reproducible_and_loss_scale_exact(world):
    d4, f = world["draw4"], si.Findings()
    kw = dict(old_logprobs=d4["logprob"] + 0.04, ref_means=d4["mean"].float() + 0.125, kl_coef=0.0625)
    s1, g1 = _group(world, d4["actions"], ADV4, **kw)
    s2, g2 = _group(world, d4["actions"], ADV4, **kw)
    f.same_grads(g1, g2, "two identical group steps")
    for k in s1:
        f.same_bits(s1[k], s2[k], f"two identical group steps: {k}")
    _, g4 = _group(world, d4["actions"], ADV4, loss_scale=4.0, **kw)
    f.same_grads(g4, {n: 4.0 * g for n, g in g1.items()}, "loss_scale = 4 vs 4 x (loss_scale = 1)")
    f.all_finite(g1, "group step"), f.every_tensor_nonzero(g1, "group step")
    f.check(float(s1["kl"]) > 0.0 and set(s1) == {"loss", "logprob", "ratio", "clip_frac", "kl"}, "statistics")
    # [B, G, chunk] advantages: the per-draw ones repeated
    _, g3 = _group(world, d4["actions"], ADV4[:, :, None].expand(3, 4, 8), **kw)
    f.same_grads(g3, g1, "advantages [B, G, chunk]")
    f.done()


def test_draws_one_forward_one_launch(world, monkeypatch):
    eng, batch, cfg = world["eng"], world["batches"][0], world["cfg"]
    d4, keys = world["draw4"], world["keys4"]
    C, Ad = cfg.chunk, cfg.action_dim
    assert d4["actions"].shape == (3, 4, C, Ad) and d4["actions"].dtype == F32 and d4["actions"].is_cuda
    assert d4["logprob"].shape == (3, 4, C) and d4["logprob"].dtype == F32 and d4["mean"].shape == (3, C, Ad) and d4["mean"].dtype == BF
    eng.token_sample.call = 6
    names, again = _launches(monkeypatch, lambda: eng.sample_actions_laplace(batch, SCALE, num_samples=4, row_keys=keys))
    assert eng.token_sample.call == 7, "the group draw advances the stream once"
    assert names.count("ovla_laplace_sample") == 1 and "ovla_laplace_pg" not in names
    assert torch.equal(i32(again["actions"]), i32(d4["actions"])) and torch.equal(i32(again["logprob"]), i32(d4["logprob"]))
    assert names.count("ovla_head_out_fwd") == 1, "one forward, one head"
    for g in range(4):                                           # draw (b, g) is the single draw of observation b under the key keys[b, g]
        eng.token_sample.call = 6
        one = eng.sample_actions_laplace(batch, SCALE, row_keys=keys[:, g:g + 1])
        assert torch.equal(i32(one["actions"][:, 0]), i32(d4["actions"][:, g])) and torch.equal(i32(one["logprob"][:, 0]), i32(d4["logprob"][:, g])), f"draw {g}"
    assert not torch.equal(d4["actions"][:, 0], d4["actions"][:, 1])
    eng.token_sample.call = 6
    dflt = eng.sample_actions_laplace(batch, SCALE, num_samples=2)
    eng.token_sample.call = 6
    one = eng.sample_actions_laplace(batch, SCALE, row_keys=[[1], [3], [5]])
    assert torch.equal(i32(dflt["actions"][:, 1]), i32(one["actions"][:, 0])), "default keys b * G + g"
    eng.token_sample.call = 6
    full = eng.sample_actions_laplace(batch, SCALE, num_samples=4, row_keys=keys[:, :, None] * C + torch.arange(C)[None, None, :])
    assert torch.equal(i32(full["actions"]), i32(d4["actions"])), "[B, G, chunk] keys"
    eng.token_sample.call = 7
    assert not torch.equal(eng.sample_actions_laplace(batch, SCALE, num_samples=4, row_keys=keys)["actions"], d4["actions"]), "the next call draws anew"
    # the draws scatter around the mean by the scale; their log-probabilities are what action_logprobs recomputes
    z = (d4["actions"] - d4["mean"].float()[:, None]) / torch.tensor(SCALE, device=eng.device)
    assert 0.5 < float(z.abs().mean()) < 1.5, f"E|e| = 1; {float(z.abs().mean())} over {z.numel()} draws"
    pl = eng.action_logprobs(batch, d4["actions"], SCALE)
    assert torch.equal(i32(pl["logprob"]), i32(d4["logprob"])) and torch.equal(i32(pl["mean"]), i32(d4["mean"]))
    call = eng.token_sample.call
    with pytest.raises(ValueError, match="num_samples"):
        eng.sample_actions_laplace(batch, SCALE, num_samples=65)
    with pytest.raises(ValueError, match="row_keys"):
        eng.sample_actions_laplace(batch, SCALE, num_samples=4, row_keys=[1, 2, 3])
    with pytest.raises(ValueError, match="scale"):
        eng.sample_actions_laplace(batch, [0.1, 0.2], num_samples=4)
    assert eng.token_sample.call == call, "a refused call does not advance the stream"


def test_launch_lists(world, monkeypatch):
    """One ovla_laplace_pg launch per group step, in place of nothing else: the step's other launches are the L1 step's, and the plain L1 step
    issues neither Laplace kernel."""
    eng, batch, d4 = world["eng"], world["batches"][0], world["draw4"]
    eng.zero_grad()
    l1, _ = _launches(monkeypatch, lambda: eng.train_step_fwd_bwd(batch))
    eng.zero_grad()
    pg, _ = _launches(monkeypatch, lambda: eng.train_step_action_pg_group(batch, d4["actions"], ADV4, SCALE, old_logprobs=d4["logprob"]))
    eng.zero_grad()
    assert "ovla_laplace_pg" not in l1 and "ovla_laplace_sample" not in l1
    assert pg.count("ovla_laplace_pg") == 1 and "ovla_laplace_sample" not in pg
    assert [n for n in pg if n != "ovla_laplace_pg"] == l1, "the group step's other launches are the L1 step's, in its order"
    assert pg[pg.index("ovla_laplace_pg") - 1] == "ovla_head_out_fwd" and pg[pg.index("ovla_laplace_pg") + 1] == "ovla_head_out_bwd"


def _train_two_steps(eng, batch, d4):
    for st in eng.stores:
        st.init_optimizer()
    adv = torch.tensor([[1.0, -1.0, 0.5, -0.5]] * 3)
    for _ in range(2):
        eng.zero_grad()
        eng.train_step_action_pg_group(batch, d4["actions"], adv, SCALE)
        eng.adamw_step(1e-3)
        eng.refresh_derived()


def test_reference_policy(world):
    eng, batch, d4, f = world["eng"], world["batches"][0], world["draw4"], si.Findings()
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    with pytest.raises(RuntimeError, match="set_reference_policy"):
        eng.reference_action_means(batch)
    try:
        eng.set_reference_policy()
        ref0 = eng.reference_action_means(batch)
        f.check(ref0.shape == d4["mean"].shape and ref0.dtype == BF, "reference_action_means' shape")
        f.same_bits(ref0, d4["mean"], "reference_action_means right after set_reference_policy")
        s0, g0 = _group(world, d4["actions"], ADV4, old_logprobs=d4["logprob"])
        s1, g1 = _group(world, d4["actions"], ADV4, old_logprobs=d4["logprob"], ref_means=ref0, kl_coef=0.5)
        f.check(float(s1["kl"]) == 0.0, f"on-policy reference: kl = {float(s1['kl'])}")
        f.same_grads(g1, g0, "on-policy reference: the kl_coef = 0 accumulators")
        _train_two_steps(eng, batch, d4)
        f.same_bits(eng.reference_action_means(batch), ref0, "reference_action_means after two optimizer steps")
        now = eng.action_logprobs(batch, d4["actions"], SCALE)
        f.check(not torch.equal(now["mean"], ref0), "the live prediction moved with the weights")
        s2, g2 = _group(world, d4["actions"], torch.zeros(3, 4), ref_means=ref0, kl_coef=0.5)
        f.check(float(s2["kl"]) > 0.0 and bool(torch.isfinite(s2["kl"])), f"kl after training = {float(s2['kl'])}")
        f.check(float(s2["loss"]) == 0.5 * float(s2["kl"]), "zero advantages: the loss is the KL penalty")
        f.all_finite(g2, "the KL term alone"), f.every_tensor_nonzero(g2, "the KL term alone")
        with eng.reference_policy():
            with pytest.raises(RuntimeError, match="inside reference_policy"):
                eng.train_step_action_pg_group(batch, d4["actions"], ADV4, SCALE)
        if not eng.ema_enabled:
            eng.enable_ema()
        with eng.ema_weights():
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                eng.train_step_action_pg_group(batch, d4["actions"], ADV4, SCALE)
    finally:
        eng.drop_reference_policy()
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()
    f.done()


def test_first_order_effect(world):
    """One group step, then AdamW at a small learning rate: the positive-advantage draws become likelier, the negative ones less likely.
    The log-probability is piecewise linear in the prediction with kinks at the draws, which lie about one scale away from it, and an AdamW step
    moves every parameter by about the learning rate whatever the gradient's size: "first order" needs a step that moves the prediction by a
    small fraction of the scale.  A wide scale (4 normalised units, uniform) and lr = 1e-4 keep it there; at the world's own scales (down to
    0.05) and lr = 3e-4 the step carries the prediction past every draw and all log-probabilities fall (-32 ... -49 measured)."""
    eng, batch = world["eng"], world["batches"][0]
    wide = 4.0
    eng.token_sample.call = 21
    d4 = eng.sample_actions_laplace(batch, wide, num_samples=4)
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    adv = torch.tensor([[1.0, -1.0, 1.0, -1.0], [-1.0, 1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]])
    pos = (adv > 0).to(eng.device)
    try:
        for st in eng.stores:
            st.init_optimizer()
        before = eng.action_logprobs(batch, d4["actions"], wide)["logprob"]
        eng.zero_grad()
        eng.train_step_action_pg_group(batch, d4["actions"], adv, wide)
        eng.adamw_step(1e-4)
        eng.refresh_derived()
        after = eng.action_logprobs(batch, d4["actions"], wide)["logprob"]
        delta = (after - before).mean(-1)                        # [B, G]
        assert float(delta[pos].mean()) > 0.0 and float(delta[~pos].mean()) < 0.0, f"positive draws {float(delta[pos].mean())}, negative {float(delta[~pos].mean())}"
    finally:
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()


def test_grpo_step_continuous(world):
    eng, batch, cfg, f = world["eng"], world["batches"][0], world["cfg"], si.Findings()
    rl = load("openvla-oft_amd.rl")
    seen = {}

    def reward_fn(b, actions):
        seen.update(shape=tuple(actions.shape), lo=float(actions.min()), hi=float(actions.max()), device=actions.device)
        target = b["actions"].to(actions.device, F32).reshape(3, 1, cfg.chunk, cfg.action_dim)
        return -(actions - target).abs().mean((2, 3))

    runs = []
    eng.set_reference_policy()
    try:
        for _ in range(2):
            eng.token_sample.call = 50
            eng.zero_grad()
            stats = rl.grpo_step_continuous(eng, batch, reward_fn, group_size=4, scale=1.0, kl_coef=0.04, clip=(0.8, 1.2), inner_steps=2)
            runs.append(({k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)))
            assert eng.token_sample.call == 51
        eng.token_sample.call = 50
        raw = eng.sample_actions_laplace(batch, 1.0, num_samples=4)["actions"]
    finally:
        eng.drop_reference_policy()
        eng.zero_grad()
    assert seen["shape"] == (3, 4, cfg.chunk, cfg.action_dim) and seen["device"] == eng.device
    assert float(raw.abs().max()) > 1.0, "at scale 1 some of 672 raw draws leave [-1, 1]"
    assert seen["lo"] == -1.0 and seen["hi"] == 1.0, f"reward_fn saw [{seen['lo']}, {seen['hi']}]: not the clamped draws"
    (s1, g1), (s2, g2) = runs
    f.same_grads(g1, g2, "two grpo_step_continuous runs from the same state")
    for k in s1:
        f.same_bits(s1[k], s2[k], f"two grpo_step_continuous runs: {k}")
    f.all_finite(g1, "grpo_step_continuous"), f.every_tensor_nonzero(g1, "grpo_step_continuous")
    adv = s1["advantages"]
    f.check(adv.shape == (3, 4) and adv.device == eng.device and bool((adv.mean(1).abs() <= 8 * 2.0 ** -23 * adv.abs().max(1).values.clamp_min(1.0)).all()),
            "the advantages have zero group mean")
    f.check(float(s1["kl"]) == 0.0 and float(s1["ratio"]) == 1.0, "on policy: kl == 0, ratio == 1")
    f.check(float(s1["reward"]) < 0.0 and set(s1) >= {"loss", "logprob", "clip_frac", "ratio", "kl", "reward"} and all(v.device == eng.device for v in s1.values()),
            "statistics")
    f.done()


def test_refusals(world, dev):
    eng, batch, d4 = world["eng"], world["batches"][0], world["draw4"]
    with pytest.raises(ValueError, match="actions"):
        eng.train_step_action_pg_group(batch, d4["actions"][:, 0], torch.ones(3, 1), SCALE)
    with pytest.raises(ValueError, match="advantages"):
        eng.train_step_action_pg_group(batch, d4["actions"], torch.ones(3), SCALE)
    with pytest.raises(ValueError, match="old_logprobs"):
        eng.train_step_action_pg_group(batch, d4["actions"], torch.ones(3, 4), SCALE, old_logprobs=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="ref_means"):
        eng.train_step_action_pg_group(batch, d4["actions"], torch.ones(3, 4), SCALE, ref_means=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="ref_means"):
        eng.train_step_action_pg_group(batch, d4["actions"], torch.ones(3, 4), SCALE, kl_coef=0.5)
    err = load("openvla-oft_amd._lib").OvlaError
    with pytest.raises(err, match="kl_coef"):
        eng.train_step_action_pg_group(batch, d4["actions"], torch.ones(3, 4), SCALE, kl_coef=-1.0)
    with pytest.raises(err, match="scale"):
        eng.train_step_action_pg_group(batch, d4["actions"], torch.ones(3, 4), 0.0)
    eng.zero_grad()
    other = si.make_world(dev, "discrete")["eng"]
    for call in (lambda: other.sample_actions_laplace(batch, SCALE), lambda: other.action_logprobs(batch, d4["actions"], SCALE),
                 lambda: other.train_step_action_pg_group(batch, d4["actions"], torch.ones(3, 4), SCALE)):
        with pytest.raises(RuntimeError, match="head='l1'"):
            call()


# ---- predict_action / predict_action_batch with action_noise_scale --------------------------------------------------------------------------------
UNNORM = "d"


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def vla_world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats={UNNORM: {"action": {"q01": [-2.0] * 7, "q99": [1.0] * 7}}})
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head."))
    g = torch.Generator().manual_seed(5)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in (7, 12, 9)]
    pv = torch.randn(3, 12, 56, 56, generator=g).to(BF).float()
    vla.engine.token_sample.seed = 0x0123456789ABCDEF
    return dict(vla=vla, head=head, cfg=cfg, prompts=prompts, pv=pv, modeling=modeling)


def _noisy(w, idx, call, keys=None, **kw):
    vla = w["vla"]
    vla.engine.token_sample.call = call
    a, h, st = vla.predict_action_batch([(w["prompts"][i], None) for i in idx], w["pv"][idx], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=SCALE,
                                        return_sample=True, sample_keys=keys, **kw)
    assert vla.engine.token_sample.call == call + 1, "one noisy call advances the stream by one"
    assert isinstance(st, w["modeling"].SampledActions)
    return a, st


def test_predict_action_batch_with_noise(vla_world, monkeypatch):
    w, vla, cfg = vla_world, vla_world["vla"], vla_world["cfg"]
    C, Ad = cfg.chunk, cfg.action_dim
    plain_call = lambda: vla.predict_action_batch([(p, None) for p in w["prompts"]], w["pv"], unnorm_key=UNNORM, action_head=w["head"])
    plain_call()                                                 # (a shape's first call also plans its GEMM schedules)
    plain_names, plain = _launches(monkeypatch, plain_call)
    assert "ovla_laplace_sample" not in plain_names, "without action_noise_scale no draw is launched"
    vla.engine.token_sample.call = 3
    names, (a, h, st) = _launches(monkeypatch, lambda: vla.predict_action_batch([(p, None) for p in w["prompts"]], w["pv"], unnorm_key=UNNORM, action_head=w["head"],
                                                                                action_noise_scale=SCALE, return_sample=True, sample_keys=[5, 8, 50]))
    assert names.count("ovla_laplace_sample") == 1 and [n for n in names if n != "ovla_laplace_sample"] == plain_names
    assert a.shape == (3, C, Ad) and st.actions.shape == (3, C, Ad) and st.actions.dtype == F32 and st.logprobs.shape == (3, C) and st.mean.dtype == BF and st.actions.is_cuda
    # the returned actions are the draw, un-normalised as always; the mean is what the plain call decodes
    want = np.stack([vla._unnormalize_actions(st.actions[b].cpu().numpy(), UNNORM) for b in range(3)])
    assert np.array_equal(a, want)
    assert np.array_equal(plain[0], np.stack([vla._unnormalize_actions(st.mean[b].float().cpu().numpy(), UNNORM) for b in range(3)]))
    assert not np.array_equal(a, plain[0]) and torch.equal(h, plain[1])
    # reproducible for a fixed call, different on the next
    a2, st2 = _noisy(w, [0, 1, 2], 3, keys=[5, 8, 50])
    assert np.array_equal(a2, a) and torch.equal(i32(st2.actions), i32(st.actions)) and torch.equal(i32(st2.logprobs), i32(st.logprobs))
    a3, _ = _noisy(w, [0, 1, 2], 4, keys=[5, 8, 50])
    assert not np.array_equal(a3, a)
    # independent of the observation's batch given its key; pad_to changes nothing; sample_seed replaces the seed
    a1, st1 = _noisy(w, [1], 3, keys=[8])
    assert np.array_equal(a1[0], a[1]) and torch.equal(i32(st1.logprobs[0]), i32(st.logprobs[1]))
    ar, _ = _noisy(w, [2, 0], 3, keys=[50, 5])
    assert np.array_equal(ar[0], a[2]) and np.array_equal(ar[1], a[0])
    ap, stp = _noisy(w, [0, 1, 2], 3, keys=[5, 8, 50], pad_to=4)
    assert np.array_equal(ap, a) and stp.actions.shape == (3, C, Ad) and torch.equal(i32(stp.actions), i32(st.actions))
    asd, _ = _noisy(w, [0, 1, 2], 3, keys=[5, 8, 50], sample_seed=77)
    assert not np.array_equal(asd, a)
    # the draw is what the engine's group step takes
    ids, mask = w["prompts"][0][None], torch.ones((1, len(w["prompts"][0])), dtype=torch.bool)
    vla.engine.token_sample.call = 3
    one = vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=SCALE,
                             return_sample=True, sample_keys=[5])
    assert vla.engine.token_sample.call == 4 and len(one) == 3 and one[0].shape == (C, Ad) and one[2].actions.shape == (1, C, Ad)
    assert np.array_equal(one[0], vla._unnormalize_actions(one[2].actions[0].cpu().numpy(), UNNORM))
    vla.engine.token_sample.call = 3
    again = vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=SCALE,
                               sample_keys=[5])
    assert len(again) == 2 and np.array_equal(again[0], one[0])
    vla.engine.token_sample.call = 4
    nxt = vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=SCALE, sample_keys=[5])
    assert not np.array_equal(nxt[0], one[0])
    plain_names1, _ = _launches(monkeypatch, lambda: vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"]))
    assert "ovla_laplace_sample" not in plain_names1


def test_predict_action_noise_refusals(vla_world):
    w, vla = vla_world, vla_world["vla"]
    prompts = [(p, None) for p in w["prompts"]]
    ids, mask = w["prompts"][0][None], torch.ones((1, len(w["prompts"][0])), dtype=torch.bool)
    call = vla.engine.token_sample.call = 9
    with pytest.raises(ValueError, match="action_head"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_noise_scale=0.1)
    with pytest.raises(ValueError, match="action_head"):
        vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_noise_scale=0.1)
    with pytest.raises(ValueError, match="policies"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_noise_scale=0.1, policy=["a", "b", "c"])
    with pytest.raises(ValueError, match="return_sample"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], return_sample=True)
    with pytest.raises(ValueError, match="sample_keys"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=0.1, sample_keys=[1, 2])
    with pytest.raises(ValueError, match="positive and finite"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=-0.1)
    diff = w["modeling"].DiffusionActionHead.__new__(w["modeling"].DiffusionActionHead)       # (only its class is looked at: refused before any use)
    diff.noise_scheduler = None
    with pytest.raises(ValueError, match="diffusion"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=diff, action_noise_scale=0.1)
    with pytest.raises(ValueError, match="do_sample=True draws action TOKENS"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], do_sample=True)
    vla.use_graph = True
    try:
        with pytest.raises(ValueError, match="graph replay"):
            vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=0.1)
        with pytest.raises(ValueError, match="graph replay"):
            vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=0.1)
    finally:
        vla.use_graph = False
    assert vla.engine.token_sample.call == call, "a refused call does not advance the stream"
