"""The learned Laplace scale through the engine on the tiny L1 world of tests/step_invariants.py (B = 3, chunk 8, action_dim 7): a fresh scale
head at b0 = 1 is the fixed-scale policy at 1.0 bit for bit, the scale's gradient stops at the head's hidden output (every accumulator outside
the scale head's store keeps its bits), the maximum-likelihood fit beside the L1 step and on a frozen policy, the first-order effect of a step,
the reference policy's mean and scale, rl.grpo_step_continuous and predict_action(_batch) with action_noise_scale="learned"."""
import importlib
import math

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import step_invariants as si

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
ADV4 = torch.tensor([[1.0, -0.5, 2.0, -1.0], [0.25, 0.5, -2.0, 1.0], [-1.0, -1.0, 3.0, 0.5]])
KEYS4 = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23], [7, 5, 3, -1]])
SCALE = [0.3, 1.0, 0.05, 0.5, 0.7, 0.25, 0.1]
PRE = "action_scale_head."
load = importlib.import_module


def i32(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def split(grads):
    """(the accumulators outside the scale head's store, those inside it)."""
    return {n: g for n, g in grads.items() if not n.startswith(PRE)}, {n: g for n, g in grads.items() if n.startswith(PRE)}


def set_head(eng, weight=None, bias=None):
    """Writes the scale head's parameters: `weight` a float (uniform(-weight, weight), seeded) or None (zeros); `bias` a list of scales b0 or None (0)."""
    sh = eng.scale_head
    g = torch.Generator().manual_seed(17)
    w = torch.zeros(sh.w.shape) if weight is None else (torch.rand(sh.w.shape, generator=g) * 2 - 1) * weight
    b = torch.zeros(sh.b.shape) if bias is None else torch.tensor(bias).log()
    sh.w.data.copy_(w.to(eng.device, BF)), sh.b.data.copy_(b.to(eng.device, BF))


@pytest.fixture(scope="module")
def world(dev):
    w = si.make_world(dev, "l1")
    eng = w["eng"]
    eng.token_sample.seed, eng.token_sample.call = 0xABCDEF0123456789, 6
    with pytest.raises(ValueError, match="attach_scale_head"):
        eng.sample_actions_laplace(w["batches"][0], "learned")
    assert eng.token_sample.call == 6, "a refused call does not advance the stream"
    assert eng.attach_scale_head(1.0) is eng.scale_head and eng.scale_bounds == (-6.0, 1.0)
    return w


def _launches(monkeypatch, fn):
    lib, names = load("openvla-oft_amd._lib"), []
    real = lib.check
    with monkeypatch.context() as m:
        m.setattr(lib, "check", lambda rc, what: (names.append(what), real(rc, what))[1])
        out = fn()
    return names, out


def _group(world, actions, advantages, scale, **kw):
    eng, batch = world["eng"], world["batches"][0]
    eng.zero_grad()
    stats = eng.train_step_action_pg_group(batch, actions, advantages, scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def _draw(world, scale, call=6, G=4, keys=KEYS4):
    eng = world["eng"]
    eng.token_sample.call = call
    return eng.sample_actions_laplace(world["batches"][0], scale, num_samples=G, row_keys=keys)


def test_attach_ordering_and_refusals(dev):
    w = si.make_world(dev, "l1")
    eng, batch = w["eng"], w["batches"][0]
    for name in ("action_logprobs", "train_step_action_pg_group"):
        with pytest.raises(ValueError, match="attach_scale_head"):
            getattr(eng, name)(batch, torch.zeros(3, 1, 8, 7), *((torch.ones(3, 1),) if name.startswith("train") else ()), "learned")
    with pytest.raises(ValueError, match="fit_scale|attach_scale_head"):
        eng.train_step_fwd_bwd(batch, fit_scale=True)
    with pytest.raises(ValueError, match="attach_scale_head"):
        eng.train_step_scale_nll(batch)
    with pytest.raises(ValueError, match="bounds"):
        eng.attach_scale_head(0.1, bounds=(1.0, -6.0))
    with pytest.raises(ValueError, match="init_scale|scale"):
        eng.attach_scale_head(-0.1)
    assert eng.scale_head is None and len(eng.stores) == 3
    # whatever enumerates the stores when it is enabled comes after the scale head
    eng.set_reference_policy()
    with pytest.raises(RuntimeError, match="set_reference_policy"):
        eng.attach_scale_head(0.1)
    eng.drop_reference_policy()
    for enable, name in ((eng.enable_grad_clip, "enable_grad_clip"), (eng.enable_tensor_stats, "enable_tensor_stats"),
                         (eng.enable_fp32_optimizer_state, "enable_fp32_optimizer_state"), (eng.enable_ema, "enable_ema")):
        enable()
        with pytest.raises(RuntimeError, match=name):
            eng.attach_scale_head(0.1)
    assert eng.scale_head is None
    other = si.make_world(dev, "discrete")["eng"]
    with pytest.raises(RuntimeError, match="head='l1'"):
        other.attach_scale_head(0.1)
    # a fresh engine: per-dimension initial scales land in the bias, and the store is one of `stores`
    w2 = si.make_world(dev, "l1")["eng"]
    n = len(w2.stores)
    w2.attach_scale_head(SCALE, bounds=(-5.0, 0.5))
    assert len(w2.stores) == n + 1 and w2.stores[-1] is w2.scale_head.store and w2.scale_bounds == (-5.0, 0.5)
    assert torch.equal(w2.scale_head.b.data.cpu(), torch.tensor(SCALE).log().to(BF)) and bool((w2.scale_head.w.data == 0).all())
    assert {PRE + "log_scale.weight", PRE + "log_scale.bias"} <= set(w2.export_trainable("data"))
    with pytest.raises(RuntimeError, match="already"):
        w2.attach_scale_head(0.1)
    w2.enable_grad_clip(), w2.enable_tensor_stats(), w2.enable_ema()          # ... and afterwards they count it in
    assert w2._grad_clip["slots"].numel() == sum(len(st.flat_grad) for st in w2.stores) and PRE + "log_scale.bias" in w2._tensor_stats["names"]
    assert w2.scale_head.store.ema_shadow is not None


def test_fresh_head_at_one_is_the_fixed_scale_policy(world):
    eng, batch, f = world["eng"], world["batches"][0], si.Findings()
    set_head(eng)
    want, got = _draw(world, 1.0), _draw(world, "learned")
    assert eng.token_sample.call == 7
    f.same_bits(got["actions"], want["actions"], "draws"), f.same_bits(got["logprob"], want["logprob"], "the draws' log-probabilities")
    f.same_bits(got["mean"], want["mean"], "mean")
    f.check(got["log_scale"].shape == (3, 8, 7) and got["log_scale"].dtype == BF and bool((got["log_scale"] == 0).all()), "log_scale of the fresh head")
    f.check(got["entropy"].shape == (3, 8) and bool(((got["entropy"] - 7 * (1 + math.log(2.0))).abs() < 1e-5).all()), "entropy = 7 (1 + ln 2)")
    lp_want, lp_got = eng.action_logprobs(batch, want["actions"], 1.0), eng.action_logprobs(batch, want["actions"], "learned")
    f.same_bits(lp_got["logprob"], lp_want["logprob"], "action_logprobs"), f.same_bits(lp_got["logprob"], want["logprob"], "action_logprobs vs the draw")
    f.same_bits(lp_got["entropy"], got["entropy"], "entropy of action_logprobs")
    kw = dict(old_logprobs=want["logprob"] + 0.04, ref_means=want["mean"].float() + 0.125, kl_coef=0.0625)
    s_want, g_want = _group(world, want["actions"], ADV4, 1.0, **kw)
    s_got, g_got = _group(world, want["actions"], ADV4, "learned", ref_log_scales=torch.zeros(3, 8, 7), **kw)
    rest, own = split(g_got)
    f.same_grads(rest, split(g_want)[0], "every accumulator outside the scale head's store: learned (b0 = 1) vs scale = 1.0")
    for k in s_want:
        f.same_bits(s_got[k], s_want[k], f"statistics: {k}")
    f.check(set(s_got) == set(s_want) | {"entropy", "scale"} and float(s_got["scale"]) == 1.0, f"statistics {sorted(s_got)}")
    f.every_tensor_nonzero(own, "the scale head's accumulators"), f.all_finite(own, "the scale head's accumulators")
    f.check(all(not bool((g != 0).any()) for g in split(g_want)[1].values()), "the numeric-scale step leaves the scale head's accumulators at zero")
    f.done()


def test_scale_gradient_stops_at_the_hidden_output_and_launch_list(world, monkeypatch):
    eng, batch, f = world["eng"], world["batches"][0], si.Findings()
    set_head(eng, weight=0.02, bias=SCALE)
    try:
        d4 = _draw(world, "learned")
        ls = d4["log_scale"].float()
        f.check(float(ls.std()) > 0.05 and bool(torch.isfinite(ls).all()), f"the head's widths vary: std of log_scale {float(ls.std())}")
        pol = dict(ref_means=d4["mean"].float() + 0.125, ref_log_scales=d4["log_scale"].float() - 0.25)
        kw = dict(old_logprobs=d4["logprob"] + 0.04, kl_coef=0.0625, entropy_coef=0.03, **pol)
        s1, g1 = _group(world, d4["actions"], ADV4, "learned", **kw)
        with monkeypatch.context() as m:
            m.setattr(eng.scale_head, "bwd", lambda h2, dls: None)             # the same call with dlog_scale discarded
            s2, g2 = _group(world, d4["actions"], ADV4, "learned", **kw)
        f.same_grads(split(g1)[0], split(g2)[0], "the accumulators outside the scale head's store, with and without the scale head's backward")
        f.every_tensor_nonzero(split(g1)[1], "the scale head's accumulators"), f.all_finite(g1, "the learned step")
        f.check(all(not bool((g != 0).any()) for g in split(g2)[1].values()), "dlog_scale discarded: the scale head's accumulators stay zero")
        f.check(float(s1["kl"]) > 0 and float(s1["entropy"]) != 0 and 0.05 < float(s1["scale"]) < 1.0, f"statistics {s1}")
        s3, g3 = _group(world, d4["actions"], ADV4, "learned", **kw)
        f.same_grads(g3, g1, "two identical learned steps")
        _, g4 = _group(world, d4["actions"], ADV4, "learned", loss_scale=4.0, **kw)
        f.same_grads(g4, {n: 4.0 * g for n, g in g1.items()}, "loss_scale = 4 vs 4 x (loss_scale = 1)")
        # the launch list: the numeric step's, ovla_laplace_pg_rows in place of ovla_laplace_pg, plus the scale head's forward and backward
        eng.zero_grad()
        num, _ = _launches(monkeypatch, lambda: eng.train_step_action_pg_group(batch, d4["actions"], ADV4, SCALE, old_logprobs=d4["logprob"]))
        eng.zero_grad()
        lrn, _ = _launches(monkeypatch, lambda: eng.train_step_action_pg_group(batch, d4["actions"], ADV4, "learned", old_logprobs=d4["logprob"]))
        eng.zero_grad()
        assert "ovla_laplace_pg_rows" not in num and num.count("ovla_laplace_pg") == 1, "a numeric scale takes the fixed-scale launches with a head attached"
        assert lrn.count("ovla_laplace_pg_rows") == 1 and "ovla_laplace_pg" not in lrn and "ovla_laplace_sample_rows" not in lrn
        i = lrn.index("ovla_laplace_pg_rows")
        assert lrn[i - 2: i] == ["ovla_head_out_fwd"] * 2 and lrn[i + 1: i + 3] == ["ovla_head_out_bwd"] * 2
        assert lrn[: i - 1] + ["ovla_laplace_pg"] + lrn[i + 2:] == num, "the learned step's other launches are the numeric step's, in its order"
        smp, _ = _launches(monkeypatch, lambda: _draw(world, "learned"))
        assert smp.count("ovla_laplace_sample_rows") == 1 and smp.count("ovla_head_out_fwd") == 2 and "ovla_laplace_sample" not in smp
        with pytest.raises(ValueError, match="learned"):
            eng.train_step_action_pg_group(batch, d4["actions"], ADV4, SCALE, entropy_coef=0.1)
        with pytest.raises(ValueError, match="come together"):
            eng.train_step_action_pg_group(batch, d4["actions"], ADV4, "learned", ref_means=pol["ref_means"], kl_coef=0.1)
    finally:
        eng.zero_grad()
    f.done()


def test_fit_scale_beside_the_l1_step_and_on_a_frozen_policy(world, monkeypatch):
    eng, batch, f = world["eng"], world["batches"][0], si.Findings()
    set_head(eng, weight=0.02, bias=SCALE)
    want = si.fresh_step(world, 0, memo=False)
    eng.zero_grad()
    l1, _ = _launches(monkeypatch, lambda: eng.train_step_fwd_bwd(batch))
    eng.zero_grad()
    fit, (loss_sum, count, pred) = _launches(monkeypatch, lambda: eng.train_step_fwd_bwd(batch, fit_scale=True))
    grads = si.export_grads(eng)
    side = {k: v.detach().clone() for k, v in eng.last_scale_fit.items()}
    rest, own = split(grads)
    f.same_bits(loss_sum, want.loss_sum, "loss"), f.same_bits(pred, want.pred, "predictions"), f.check(count == want.count, "count")
    f.same_grads(rest, split(want.grads)[0], "the accumulators outside the scale head's store: fit_scale vs the plain step")
    f.every_tensor_nonzero(own, "fit_scale: the scale head's accumulators"), f.all_finite(own, "fit_scale")
    f.check(all(not bool((g != 0).any()) for g in split(want.grads)[1].values()), "the plain step leaves the scale head's accumulators at zero")
    assert fit[: len(l1)] == l1 and fit[len(l1):] == ["ovla_head_out_fwd", "ovla_laplace_pg_rows", "ovla_head_out_bwd"], "the side step is three launches after the L1 step's"
    # the frozen-policy fit touches the scale head's store alone, with the side step's bits
    eng.zero_grad()
    nll_names, nll = _launches(monkeypatch, lambda: eng.train_step_scale_nll(batch))
    g_nll = si.export_grads(eng)
    for n, g in split(g_nll)[0].items():
        f.all_zero(g, f"train_step_scale_nll wrote {n}")
    assert nll_names[-3:] == ["ovla_head_out_fwd", "ovla_laplace_pg_rows", "ovla_head_out_bwd"] and not any("bwd" in n for n in nll_names[:-3]), "no backward but the scale head's"
    inf_pred = eng.action_logprobs(batch, torch.zeros(3, 1, 8, 7), "learned")["mean"].reshape(-1, 7)
    # (the training and the inference forward agree in bits on this world -- no dropout, the same schedules -- so both fits see the same h2)
    f.same_bits(inf_pred, want.pred, "the inference forward's prediction vs the training forward's")
    f.same_grads(split(g_nll)[1], own, "train_step_scale_nll vs the fit_scale side step")
    f.same_bits(nll["nll"], side["nll"], "nll"), f.same_bits(nll["scale"], side["scale"], "scale")
    lp = eng.action_logprobs(batch, batch["actions"].to(BF).float().reshape(3, 1, 8, 7), "learned")
    f.check(abs(float(nll["nll"]) + float(lp["logprob"].mean())) <= 1e-5 * abs(float(nll["nll"])), "nll is minus the mean log-probability of the target chunk")
    _, g_half = (eng.zero_grad(), eng.train_step_scale_nll(batch, loss_scale=0.5))
    f.same_grads(split(si.export_grads(eng))[1], {n: 0.5 * g for n, g in split(g_nll)[1].items()}, "loss_scale = 0.5")
    eng.zero_grad()
    f.done()


def test_first_order_effect(world):
    """One AdamW step on the scale head's store lowers the NLL of the same batch; and a positive advantage on a draw three widths from the mean
    raises that element's b: with one live chunk step the weight gradient is -|dlog_scale| h2, so the step adds lr (1 + sum_k |h2_k|) to its
    log-scale, whatever the head's weights."""
    eng, batch = world["eng"], world["batches"][0]
    set_head(eng, weight=0.02, bias=SCALE)
    sh = eng.scale_head
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    try:
        sh.store.init_optimizer()
        eng.zero_grad()
        before = eng.train_step_scale_nll(batch)["nll"].item()
        sh.store.adamw_step(1e-3)
        eng.zero_grad()
        after = eng.train_step_scale_nll(batch)["nll"].item()
        assert after < before, f"NLL {before} -> {after}"
        eng.load_trainable(snap), sh.store.init_optimizer(), eng.zero_grad()
        pol = eng.action_logprobs(batch, torch.zeros(3, 1, 8, 7), "learned")
        b = pol["log_scale"].float().clamp(*eng.scale_bounds).exp()
        far = (pol["mean"].float() + 3.0 * b)[:, None]                          # [B, 1, chunk, action_dim]: every element three widths out
        adv = torch.zeros(3, 1, 8)
        adv[0, 0, 0] = 1.0
        eng.train_step_action_pg_group(batch, far, adv, "learned")
        own = split(si.export_grads(eng))[1]
        assert bool((own[PRE + "log_scale.bias"] < 0).all()), "q = 3: d loss / d s = (1 - q) c < 0 in every dimension"
        sh.store.adamw_step(1e-3)
        eng.zero_grad()
        ls = eng.action_logprobs(batch, torch.zeros(3, 1, 8, 7), "learned")["log_scale"].float()
        assert bool((ls[0, 0] > pol["log_scale"].float()[0, 0]).all()), f"log-scale of the live chunk step: {pol['log_scale'][0, 0]} -> {ls[0, 0]}"
    finally:
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()


def test_reference_policy(world):
    eng, batch, f = world["eng"], world["batches"][0], si.Findings()
    set_head(eng, weight=0.02, bias=SCALE)
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    with pytest.raises(RuntimeError, match="set_reference_policy"):
        eng.reference_action_policy(batch)
    try:
        d4 = _draw(world, "learned")
        eng.set_reference_policy()
        pol = eng.reference_action_policy(batch)
        f.same_bits(pol["mean"], d4["mean"], "reference mean right after set_reference_policy")
        f.same_bits(pol["log_scale"], d4["log_scale"], "reference log-scale right after set_reference_policy")
        for n, t in eng.export_trainable("data").items():
            f.same_bits(t, snap[n], f"live bits after reference_action_policy: {n}")
        kw = dict(old_logprobs=d4["logprob"], ref_means=pol["mean"], ref_log_scales=pol["log_scale"], kl_coef=0.5)
        s0, g0 = _group(world, d4["actions"], ADV4, "learned", old_logprobs=d4["logprob"])
        s1, g1 = _group(world, d4["actions"], ADV4, "learned", **kw)
        f.check(float(s1["kl"]) == 0.0, f"on-policy reference: kl = {float(s1['kl'])}")
        f.same_grads(g1, g0, "on-policy reference: the kl_coef = 0 accumulators")
        for st in eng.stores:
            st.init_optimizer()
        for _ in range(2):
            eng.zero_grad()
            eng.train_step_action_pg_group(batch, d4["actions"], torch.tensor([[1.0, -1.0, 0.5, -0.5]] * 3), "learned")
            eng.adamw_step(1e-3)
            eng.refresh_derived()
        again = eng.reference_action_policy(batch)
        f.same_bits(again["mean"], pol["mean"], "reference mean after two optimizer steps")
        f.same_bits(again["log_scale"], pol["log_scale"], "reference log-scale after two optimizer steps")
        now = eng.action_logprobs(batch, d4["actions"], "learned")
        f.check(not torch.equal(now["log_scale"], pol["log_scale"]) and not torch.equal(now["mean"], pol["mean"]), "the live policy moved, mean and scale")
        s2, g2 = _group(world, d4["actions"], torch.zeros(3, 4), "learned", ref_means=pol["mean"], ref_log_scales=pol["log_scale"], kl_coef=0.5)
        f.check(float(s2["kl"]) > 0.0 and bool(torch.isfinite(s2["kl"])), f"kl after training = {float(s2['kl'])}")
        f.check(float(s2["loss"]) == 0.5 * float(s2["kl"]), "zero advantages: the loss is the KL penalty")
        f.every_tensor_nonzero(g2, "the KL term alone"), f.all_finite(g2, "the KL term alone")
    finally:
        eng.drop_reference_policy()
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()
    f.done()


def test_grpo_step_continuous_learned(world):
    eng, batch, cfg, f = world["eng"], world["batches"][0], world["cfg"], si.Findings()
    rl = load("openvla-oft_amd.rl")
    set_head(eng, weight=0.02, bias=SCALE)

    def reward_fn(b, actions):
        target = b["actions"].to(actions.device, F32).reshape(3, 1, cfg.chunk, cfg.action_dim)
        return -(actions - target).abs().mean((2, 3))

    eng.set_reference_policy()
    try:
        eng.token_sample.call = 50
        eng.zero_grad()
        stats = rl.grpo_step_continuous(eng, batch, reward_fn, group_size=4, scale="learned", kl_coef=0.04, entropy_coef=0.01, inner_steps=2)
        grads = si.export_grads(eng)
        assert eng.token_sample.call == 51
        with pytest.raises(ValueError, match="entropy_coef"):
            rl.grpo_step_continuous(eng, batch, reward_fn, group_size=4, scale=1.0, entropy_coef=0.01)
    finally:
        eng.drop_reference_policy()
        eng.zero_grad()
    f.check(set(stats) >= {"loss", "logprob", "clip_frac", "ratio", "kl", "entropy", "scale", "reward", "advantages"}, f"statistics {sorted(stats)}")
    f.check(all(bool(torch.isfinite(v).all()) and v.device == eng.device for v in stats.values()), "finite statistics on the device")
    f.check(float(stats["kl"]) == 0.0 and float(stats["ratio"]) == 1.0, "on policy: kl == 0, ratio == 1")
    f.all_finite(grads, "grpo_step_continuous(learned)"), f.every_tensor_nonzero(grads, "grpo_step_continuous(learned)")
    f.done()


# ---- predict_action / predict_action_batch with action_noise_scale="learned" ------------------------------------------------------------------------
UNNORM = "d"


@pytest.fixture(scope="module")
def vla_world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats={UNNORM: {"action": {"q01": [-2.0] * 7, "q99": [1.0] * 7}}})
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict={k[len("action_head."):]: v for k, v in sd.items() if k.startswith("action_head.")})
    g = torch.Generator().manual_seed(5)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in (7, 12, 9)]
    pv = torch.randn(3, 12, 56, 56, generator=g).to(BF).float()
    vla.engine.token_sample.seed = 0x0123456789ABCDEF
    return dict(vla=vla, head=head, cfg=cfg, prompts=prompts, pv=pv, modeling=modeling)


def test_predict_action_with_the_learned_scale(vla_world, monkeypatch, tmp_path):
    w, vla, cfg = vla_world, vla_world["vla"], vla_world["cfg"]
    ops = load("openvla-oft_amd.ops")
    C, Ad = cfg.chunk, cfg.action_dim
    prompts = [(p, None) for p in w["prompts"]]
    call = lambda scale, at=3, **kw: (setattr(vla.engine.token_sample, "call", at),  # noqa: E731
                                      vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale=scale, return_sample=True,
                                                               sample_keys=[5, 8, 50], **kw))[1]
    with pytest.raises(ValueError, match="attach_scale_head"):
        call("learned")
    assert vla.engine.token_sample.call == 3, "a refused call does not advance the stream"
    # a fresh head at b0 = 1 draws what action_noise_scale = 1.0 draws
    vla.attach_scale_head(1.0)
    a1, h1, s1 = call(1.0)
    a2, h2, s2 = call("learned")
    assert vla.engine.token_sample.call == 4
    assert np.array_equal(a1, a2) and torch.equal(i32(s1.actions), i32(s2.actions)) and torch.equal(i32(s1.logprobs), i32(s2.logprobs)) and torch.equal(i32(s1.mean), i32(s2.mean))
    assert s1.log_scale is None and s2.log_scale.shape == (3, C, Ad) and s2.log_scale.dtype == BF and bool((s2.log_scale == 0).all())
    # any weights, through a checkpoint file: the draw is sample_actions_laplace's launch on the head's mean and the scale head's output
    g = torch.Generator().manual_seed(3)
    sd = {"log_scale.weight": ((torch.rand(Ad, cfg.llm_dim, generator=g) * 2 - 1) * 0.02).to(BF), "log_scale.bias": torch.tensor(SCALE).log().to(BF)}
    torch.save(sd, tmp_path / "action_scale_head--5_checkpoint.pt")
    vla.load_scale_head(tmp_path / "action_scale_head--5_checkpoint.pt")
    names, (a3, h3, s3) = _launches(monkeypatch, lambda: call("learned"))
    assert names.count("ovla_laplace_sample_rows") == 1 and "ovla_laplace_sample" not in names and names.count("ovla_head_out_fwd") == 2
    assert float(s3.log_scale.float().std()) > 0.05 and torch.equal(i32(s3.mean), i32(s1.mean)) and torch.equal(h3, h1)
    keys = (torch.tensor([5, 8, 50])[:, None] * C + torch.arange(C)[None, :]).reshape(-1, 1).to(torch.int32).to(vla.device)
    words = vla.engine.token_sample.words(3)
    act, lp, _ = ops.laplace_sample_rows(s3.mean.reshape(-1, Ad).contiguous(), s3.log_scale.reshape(-1, Ad).contiguous(), vla.scale_bounds, 1,
                                         seed=words[0] | (words[1] << 32), call=words[2], row_key=keys)
    assert torch.equal(i32(act.view(3, C, Ad)), i32(s3.actions)) and torch.equal(i32(lp.view(3, C)), i32(s3.logprobs))
    assert np.array_equal(a3, np.stack([vla._unnormalize_actions(s3.actions[b].cpu().numpy(), UNNORM) for b in range(3)]))
    z = (s3.actions - s3.mean.float()) / s3.log_scale.float().exp()
    assert 0.5 < float(z.abs().mean()) < 1.5, f"E|e| = 1; {float(z.abs().mean())}"
    # an observation alone under its key, padded, and through predict_action
    vla.engine.token_sample.call = 3
    a_one, _, s_one = vla.predict_action_batch(prompts[1:2], w["pv"][1:2], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale="learned", return_sample=True, sample_keys=[8])
    assert np.array_equal(a_one[0], a3[1]) and torch.equal(i32(s_one.log_scale[0]), i32(s3.log_scale[1]))
    a_pad, _, s_pad = call("learned", pad_to=4)
    assert np.array_equal(a_pad, a3) and s_pad.log_scale.shape == (3, C, Ad)
    ids, mask = w["prompts"][0][None], torch.ones((1, len(w["prompts"][0])), dtype=torch.bool)
    vla.engine.token_sample.call = 3
    one = vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale="learned",
                             return_sample=True, sample_keys=[5])
    assert vla.engine.token_sample.call == 4 and len(one) == 3 and one[0].shape == (C, Ad) and one[2].log_scale.shape == (1, C, Ad)
    assert np.array_equal(one[0], vla._unnormalize_actions(one[2].actions[0].cpu().numpy(), UNNORM))
    act1, lp1, _ = ops.laplace_sample_rows(one[2].mean.reshape(-1, Ad).contiguous(), one[2].log_scale.reshape(-1, Ad).contiguous(), vla.scale_bounds, 1,
                                           seed=words[0] | (words[1] << 32), call=words[2], row_key=keys[:C].contiguous())
    assert torch.equal(i32(act1.view(1, C, Ad)), i32(one[2].actions)) and torch.equal(i32(lp1.view(1, C)), i32(one[2].logprobs))
    vla.engine.token_sample.call = 3
    again = vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale="learned",
                               sample_keys=[5])
    assert len(again) == 2 and np.array_equal(again[0], one[0])
    # the refusals of the numeric form
    at = vla.engine.token_sample.call
    with pytest.raises(ValueError, match="action_head"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_noise_scale="learned")
    with pytest.raises(ValueError, match="policies"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_noise_scale="learned", policy=["a", "b", "c"])
    with pytest.raises(ValueError, match="learned"):
        vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale="fitted")
    vla.use_graph = True
    try:
        with pytest.raises(ValueError, match="graph replay"):
            vla.predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale="learned")
        with pytest.raises(ValueError, match="graph replay"):
            vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=w["pv"][:1], unnorm_key=UNNORM, action_head=w["head"], action_noise_scale="learned")
    finally:
        vla.use_graph = False
    assert vla.engine.token_sample.call == at, "a refused call does not advance the stream"
