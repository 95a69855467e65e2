"""The value head and the PPO step through the engine on the tiny L1 world of tests/step_invariants.py (B = 3 and its first two observations,
chunk 8, action_dim 7): a fresh critic values everything at +0, an attached but unused critic moves nothing (with and without a scale head, in
both attach orders), the value loss's gradient stops at the head's hidden output and equals the direct kernel calls on the step's own hidden
output, the frozen-policy fit, checkpoints, the refusals, rl.gae + rl.ppo_step_continuous and predict_action's SampledActions.value."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import step_invariants as si

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
PRE, SPRE = "action_value_head.", "action_scale_head."
SCALE = [0.3, 1.0, 0.05, 0.5, 0.7, 0.25, 0.1]
KEYS = torch.tensor([[10], [20], [7]])
RETURNS = torch.tensor([1.25, -0.5, 2.0])
load = importlib.import_module


def i32(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def split(grads):
    """(the accumulators outside the value head's store, those inside it)."""
    return {n: g for n, g in grads.items() if not n.startswith(PRE)}, {n: g for n, g in grads.items() if n.startswith(PRE)}


def sub_batch(batch, B):
    return {k: (v[:B] if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def set_value_head(eng, weight=0.02, bias=0.375):
    vh = eng.value_head
    g = torch.Generator().manual_seed(23)
    vh.w.data.copy_(((torch.rand(vh.w.shape, generator=g) * 2 - 1) * weight).to(eng.device, BF))
    vh.b.data.copy_(torch.full(vh.b.shape, bias).to(eng.device, BF))


def set_scale_head(eng):
    sh = eng.scale_head
    g = torch.Generator().manual_seed(17)
    sh.w.data.copy_(((torch.rand(sh.w.shape, generator=g) * 2 - 1) * 0.02).to(eng.device, BF))
    sh.b.data.copy_(torch.tensor(SCALE).log().to(eng.device, BF))


def _launches(monkeypatch, fn):
    lib, names = load("openvla-oft_amd._lib"), []
    real = lib.check
    with monkeypatch.context() as m:
        m.setattr(lib, "check", lambda rc, what: (names.append(what), real(rc, what))[1])
        out = fn()
    return names, out


@pytest.fixture(scope="module")
def worlds(dev):
    """plain: no extra head.  v: a value head.  s: a scale head.  sv / vs: both, attached in either order.  Equal weights everywhere."""
    out = {}
    for name in ("plain", "v", "s", "sv", "vs"):
        w = si.make_world(dev, "l1")
        eng = w["eng"]
        for c in name if name != "plain" else "":
            if c == "v":
                assert eng.attach_value_head() is eng.value_head
            else:
                eng.attach_scale_head(1.0)
        if name == "v":
            vals = [eng.action_values(sub_batch(w["batches"][0], B)) for B in (2, 3)]       # the FRESH head, before any weight is written
            w["fresh_values"] = vals
        if eng.value_head is not None:
            set_value_head(eng)
        if eng.scale_head is not None:
            set_scale_head(eng)
        eng.token_sample.seed = 0xABCDEF0123456789
        out[name] = w
    return out


def _draw(w, scale, B=3, **kw):
    eng = w["eng"]
    eng.token_sample.call = 6
    return eng.sample_actions_laplace(sub_batch(w["batches"][0], B), scale, num_samples=1, row_keys=KEYS[:B], **kw)


def _pg(w, draw, scale, B=3, **kw):
    eng = w["eng"]
    eng.zero_grad()
    adv = torch.tensor([[1.0], [-0.5], [2.0]])[:B]
    stats = eng.train_step_action_pg_group(sub_batch(w["batches"][0], B), draw["actions"], adv, scale, old_logprobs=draw["logprob"] + 0.04, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def test_fresh_head_values_every_observation_at_zero(worlds):
    for v, B in zip(worlds["v"]["fresh_values"], (2, 3)):
        assert v.shape == (B,) and v.dtype == F32 and bool((i32(v) == 0).all()), f"a fresh critic: {v}"
    eng = worlds["v"]["eng"]
    assert len(eng.stores) == len(worlds["plain"]["eng"].stores) + 1 and eng.stores[-1] is eng.value_head.store
    assert worlds["sv"]["eng"].stores[-1] is worlds["sv"]["eng"].value_head.store and worlds["vs"]["eng"].stores[-1] is worlds["vs"]["eng"].value_head.store
    assert {PRE + "value.weight", PRE + "value.bias"} <= set(eng.export_trainable("data"))
    assert tuple(eng.value_head.w.shape) == (1, eng.cfg.llm_dim) and tuple(eng.value_head.b.shape) == (1,)


@pytest.mark.parametrize("with_head,without,scale", [("v", "plain", SCALE), ("sv", "s", "learned"), ("vs", "s", "learned"), ("sv", "s", SCALE)])
def test_an_unused_value_head_moves_nothing(worlds, monkeypatch, with_head, without, scale):
    f = si.Findings()
    a, b = worlds[with_head], worlds[without]
    d = _draw(b, scale)
    da = _draw(a, scale)
    f.same_bits(da["actions"], d["actions"], "draws"), f.same_bits(da["logprob"], d["logprob"], "log-probabilities")
    f.check("value" not in da, "no value without return_value")
    for B in (2, 3):
        dB = {k: v[:B] for k, v in d.items()}
        (sa, ga), (sb, gb) = _pg(a, dB, scale, B), _pg(b, dB, scale, B)
        rest, own = split(ga)
        f.same_grads(rest, gb, f"B = {B}: group step without returns, {with_head} vs {without}")
        f.check(set(sa) == set(sb), f"statistics {sorted(sa)}")
        for k in sb:
            f.same_bits(sa[k], sb[k], f"B = {B} statistics: {k}")
        for n, g in own.items():
            f.all_zero(g, f"the unused value head's accumulator {n}")
    ra, rb = si.fresh_step(a, 0, memo=False), si.fresh_step(b, 0, memo=False)
    f.same_grads(split(ra.grads)[0], rb.grads, "train_step_fwd_bwd"), f.same_bits(ra.loss_sum, rb.loss_sum, "L1 loss")
    for n, g in split(ra.grads)[1].items():
        f.all_zero(g, f"train_step_fwd_bwd wrote {n}")
    batch = a["batches"][0]
    a["eng"].zero_grad(), b["eng"].zero_grad()
    na, _ = _launches(monkeypatch, lambda: a["eng"].train_step_action_pg_group(batch, d["actions"], torch.ones(3, 1), scale, old_logprobs=d["logprob"]))
    nb, _ = _launches(monkeypatch, lambda: b["eng"].train_step_action_pg_group(batch, d["actions"], torch.ones(3, 1), scale, old_logprobs=d["logprob"]))
    a["eng"].zero_grad(), b["eng"].zero_grad()
    assert na == nb and "ovla_value_loss" not in na, "without returns the step issues the launches it issued before"
    f.done()


@pytest.mark.parametrize("name,scale", [("v", SCALE), ("sv", "learned"), ("vs", "learned")])
@pytest.mark.parametrize("B", [2, 3])
def test_value_loss_gradient_stops_at_the_hidden_output(worlds, monkeypatch, dev, name, scale, B):
    f, w, ops = si.Findings(), worlds[name], load("openvla-oft_amd.ops")
    eng, batch = w["eng"], sub_batch(worlds[name]["batches"][0], B)
    vh = eng.value_head
    d = _draw(w, scale, B)
    s0, g0 = _pg(w, d, scale, B)
    seen = []
    real_fwd = vh.fwd
    old = eng.action_values(batch) + torch.tensor([0.5, 0.5, 0.0], device=dev)[:B]   # -> unclipped, clipped, lc == l (unclipped)
    kw = dict(returns=RETURNS[:B], old_values=old, value_coef=0.25, value_clip=0.1, loss_scale=2.0)
    with monkeypatch.context() as m:
        m.setattr(vh, "fwd", lambda h2: (seen.append(h2.detach().clone()), real_fwd(h2))[1])
        s1, g1 = _pg(w, d, scale, B, **kw)
    s0s, g0s = _pg(w, d, scale, B, loss_scale=2.0)
    rest, own = split(g1)
    f.same_grads(rest, split(g0s)[0], "every accumulator outside the value store: with returns vs without")
    f.check(set(s1) == set(s0) | {"value_loss", "value_clip_frac", "explained_variance", "value"}, f"statistics {sorted(s1)}")
    f.every_tensor_nonzero(own, "the value head's accumulators"), f.all_finite(own, "the value head's accumulators")
    # the direct calls on the step's own h2
    assert len(seen) == 1 and seen[0].shape == (B * 8, eng.cfg.llm_dim)
    h2 = seen[0]
    u = ops.head_out_fwd(h2, vh.w.data, vh.b.data)
    value, du, st = ops.value_loss(u, 8, returns=RETURNS[:B].to(dev), old_value=old, value_clip=0.1, grad_scale=2.0 * 0.25 / B)
    dW, db = torch.zeros_like(vh.w.grad), torch.zeros_like(vh.b.grad)
    ops.head_out_bwd(h2, vh.w.data, None, None, 0.0, dW, db, dpred=du)
    f.same_bits(own[PRE + "value.weight"], dW.float(), "dW vs the direct ovla_head_out_bwd on the step's h2")
    f.same_bits(own[PRE + "value.bias"], db.float(), "db vs the direct call")
    f.same_bits(s1["value"], value, "value"), f.same_bits(s1["value"], eng.action_values(batch), "the step's value vs action_values")
    f.same_bits(s1["value_loss"], st[2] / st[0], "value_loss"), f.same_bits(s1["value_clip_frac"], st[1] / st[0], "value_clip_frac")
    f.check(float(st[0]) == B and 0 < float(st[1]) < B, f"clipped and unclipped observations in one step: {st.tolist()}")
    v64, r64 = value.double().cpu(), RETURNS[:B].double()
    ev = 1.0 - float(((r64 - v64) ** 2).sum() / ((r64 - r64.mean()) ** 2).sum())
    f.check(abs(float(s1["explained_variance"]) - ev) <= 1e-5 * max(1.0, abs(ev)), f"explained variance {float(s1['explained_variance'])} vs {ev}")
    for k in s0:
        f.same_bits(s1[k], s0s[k], f"the policy's statistic {k}")
    # three launches more, after the policy-gradient kernel (and the scale head's backward)
    eng.zero_grad()
    base, _ = _launches(monkeypatch, lambda: _pg(w, d, scale, B, loss_scale=2.0))
    full, _ = _launches(monkeypatch, lambda: _pg(w, d, scale, B, **kw))
    eng.zero_grad()
    i = full.index("ovla_value_loss")
    assert full.count("ovla_value_loss") == 1 and full[i - 1] == "ovla_head_out_fwd" and full[i + 1] == "ovla_head_out_bwd"
    assert full[: i - 1] + full[i + 2:] == base, "the step's other launches are those of the step without returns, in its order"
    with pytest.raises(ValueError, match="returns"):
        eng.train_step_action_pg_group(batch, d["actions"], torch.ones(B, 1), scale, value_clip=0.1)
    with pytest.raises(ValueError, match="old_values"):
        eng.train_step_action_pg_group(batch, d["actions"], torch.ones(B, 1), scale, returns=RETURNS[:B], value_clip=0.1)
    f.done()


@pytest.mark.parametrize("name,scale", [("v", SCALE), ("vs", "learned")])
def test_sample_with_value(worlds, name, scale):
    w = worlds[name]
    eng, batch = w["eng"], w["batches"][0]
    plain, withv = _draw(w, scale), _draw(w, scale, return_value=True)
    assert eng.token_sample.call == 7
    for k in plain:
        assert torch.equal(i32(plain[k]), i32(withv[k])), f"{k}: the draw keeps its bits"
    assert set(withv) == set(plain) | {"value"} and withv["value"].shape == (3,) and withv["value"].dtype == F32
    assert torch.equal(i32(withv["value"]), i32(eng.action_values(batch)))
    assert float(withv["value"].abs().min()) > 0 and float(withv["value"].std()) > 0
    with pytest.raises(ValueError, match="attach_value_head"):
        worlds["plain"]["eng"].sample_actions_laplace(batch, SCALE, return_value=True)
    with pytest.raises(ValueError, match="attach_value_head"):
        worlds["s"]["eng"].action_values(batch)


def test_train_step_value_fits_the_critic_alone(worlds, monkeypatch):
    f, w = si.Findings(), worlds["sv"]
    eng, batch = w["eng"], w["batches"][0]
    vh = eng.value_head
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    try:
        eng.zero_grad()
        names, stats = _launches(monkeypatch, lambda: eng.train_step_value(batch, RETURNS))
        rest, own = split(si.export_grads(eng))
        for n, g in rest.items():
            f.all_zero(g, f"train_step_value wrote {n}")
        f.every_tensor_nonzero(own, "train_step_value: the value head's accumulators")
        assert names[-3:] == ["ovla_head_out_fwd", "ovla_value_loss", "ovla_head_out_bwd"] and not any("bwd" in n for n in names[:-3]), "no backward but the value head's"
        f.same_bits(stats["value"], eng.action_values(batch), "value")
        _, own_half = (eng.zero_grad(), eng.train_step_value(batch, RETURNS, loss_scale=0.5), split(si.export_grads(eng)))[2]
        f.same_grads(own_half, {n: 0.5 * g for n, g in own.items()}, "loss_scale = 0.5")
        vh.store.init_optimizer()
        losses = []
        for _ in range(6):
            eng.zero_grad()
            losses.append(float(eng.train_step_value(batch, RETURNS)["value_loss"]))
            vh.store.adamw_step(1e-3)       # an Adam step moves a value by about lr (1 + sum_k |h2_k|), some 0.1 here: well inside the errors of ~1
        f.check(losses[-1] < losses[0] and all(np.isfinite(losses)), f"value_loss over six steps on one batch: {losses}")
        for n, t in eng.export_trainable("data").items():
            if not n.startswith(PRE):
                f.same_bits(t, snap[n], f"the frozen policy: {n}")
    finally:
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()
    f.done()


def test_checkpoint_round_trip(worlds, dev):
    w = worlds["v"]
    eng, batch = w["eng"], w["batches"][0]
    eng.zero_grad()
    eng.train_step_value(batch, RETURNS)
    for st in eng.stores:
        st.init_optimizer()
    eng.value_head.store.adamw_step(1e-2)
    try:
        sd, opt = {k: v.detach().clone() for k, v in eng.export_trainable("data").items()}, {k: v.detach().clone() for k, v in eng.optimizer_state_dict().items()}
        other = si.make_world(dev, "l1")["eng"]
        other.attach_value_head(state_dict=sd)
        other.load_trainable(sd)
        assert torch.equal(i32(other.action_values(batch)), i32(eng.action_values(batch)))
        stripped = si.make_world(dev, "l1")["eng"]
        stripped.attach_value_head(state_dict={k[len(PRE):]: v for k, v in sd.items() if k.startswith(PRE)})
        assert torch.equal(i32(stripped.action_values(batch)), i32(eng.action_values(batch)))
        other.load_optimizer_state_dict(opt)
        vs, vo_ = eng.value_head.store, other.value_head.store
        assert vo_.step == vs.step == 1
        for dt in vs.exp_avg:
            assert torch.equal(vo_.exp_avg[dt], vs.exp_avg[dt]) and torch.equal(vo_.exp_avg_sq[dt], vs.exp_avg_sq[dt])
            assert bool((vs.exp_avg[dt] != 0).any()), "the head's moments moved"
    finally:
        set_value_head(eng)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()


def test_attach_ordering_and_refusals(dev):
    w = si.make_world(dev, "l1")
    eng, batch = w["eng"], w["batches"][0]
    with pytest.raises(ValueError, match="attach_value_head"):
        eng.train_step_value(batch, RETURNS)
    with pytest.raises(ValueError, match="attach_value_head"):
        eng.train_step_action_pg_group(batch, torch.zeros(3, 1, 8, 7), torch.ones(3, 1), 1.0, returns=RETURNS)
    eng.set_reference_policy()
    with pytest.raises(RuntimeError, match="attach_value_head after set_reference_policy"):
        eng.attach_value_head()
    eng.drop_reference_policy()
    for enable, name in ((eng.enable_grad_clip, "enable_grad_clip"), (eng.enable_tensor_stats, "enable_tensor_stats"),
                         (eng.enable_fp32_optimizer_state, "enable_fp32_optimizer_state"), (eng.enable_ema, "enable_ema")):
        enable()
        with pytest.raises(RuntimeError, match=name):
            eng.attach_value_head()
    assert eng.value_head is None
    other = si.make_world(dev, "discrete")["eng"]
    with pytest.raises(RuntimeError, match="head='l1'"):
        other.attach_value_head()
    w2 = si.make_world(dev, "l1")["eng"]
    w2.attach_value_head()
    with pytest.raises(RuntimeError, match="already"):
        w2.attach_value_head()
    with pytest.raises(ValueError, match="shape"):
        si.make_world(dev, "l1")["eng"].attach_value_head(state_dict={"value.weight": torch.zeros(2, w2.cfg.llm_dim), "value.bias": torch.zeros(1)})
    w2.enable_grad_clip(), w2.enable_tensor_stats(), w2.enable_ema()          # ... and afterwards they count it in
    assert w2._grad_clip["slots"].numel() == sum(len(st.flat_grad) for st in w2.stores) and PRE + "value.bias" in w2._tensor_stats["names"]
    assert w2.value_head.store.ema_shadow is not None
    with w2.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            w2.train_step_value(batch, RETURNS)
        with pytest.raises(RuntimeError, match="ema_weights"):
            w2.train_step_action_pg_group(batch, torch.zeros(3, 1, 8, 7), torch.ones(3, 1), 1.0, returns=RETURNS)
        assert w2.action_values(batch).shape == (3,)                            # inference is allowed


def test_reference_policy_scope_refuses_the_value_step(dev):
    eng = si.make_world(dev, "l1")
    batch, eng = eng["batches"][0], eng["eng"]
    eng.attach_value_head()
    eng.set_reference_policy()
    with eng.reference_policy():
        with pytest.raises(RuntimeError, match="reference_policy"):
            eng.train_step_value(batch, RETURNS)
        with pytest.raises(RuntimeError, match="reference_policy"):
            eng.attach_value_head()


@pytest.mark.parametrize("name,scale", [("v", SCALE), ("sv", "learned")])
def test_gae_then_ppo_step_is_the_hand_assembled_group_step(worlds, dev, name, scale):
    f, w, rl = si.Findings(), worlds[name], load("openvla-oft_amd.rl")
    eng, batch = w["eng"], w["batches"][0]
    d = _draw(w, scale, return_value=True)
    # a rollout buffer of N = 3 trajectories of T = 4 steps; the minibatch is step t = 1 of each
    g = torch.Generator().manual_seed(9)
    rewards, values = torch.randn(3, 4, generator=g).to(dev), torch.randn(3, 4, generator=g).to(dev)
    values[:, 1] = d["value"]
    dones = torch.tensor([[0, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 0]], dtype=torch.bool, device=dev)
    adv, ret = rl.gae(rewards, values, torch.randn(3, generator=g).to(dev), dones, lengths=[4, 3, 2], gamma=0.97, lam=0.9)
    assert adv.shape == (3, 4) and adv.device == eng.device and float(adv[1, 3]) == 0.0 and float(ret[2, 2]) == 0.0
    valid = torch.tensor([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 0, 0]], dtype=torch.bool, device=dev)
    assert abs(float(adv[valid].mean())) < 1e-6 and abs(float(adv[valid].var(unbiased=False)) - 1.0) < 1e-5
    raw, _ = rl.gae(rewards, values, torch.zeros(3, device=dev), dones, lengths=torch.tensor([4, 3, 2], device=dev), gamma=0.97, lam=0.9, normalize=False)
    assert not torch.equal(raw, adv)
    with pytest.raises(load("openvla-oft_amd._lib").OvlaError, match="length"):
        rl.gae(rewards, values, torch.zeros(3, device=dev), dones, lengths=[4, 5, 2])
    kw = dict(value_coef=0.5, value_clip=0.2, loss_scale=1.5)
    eng.zero_grad()
    got = rl.ppo_step_continuous(eng, batch, d["actions"][:, 0], d["logprob"][:, 0] + 0.04, adv[:, 1], ret[:, 1], d["value"] + 0.3, scale=scale, **kw)
    g_got = si.export_grads(eng)
    extra = dict(entropy_coef=0.0) if scale == "learned" else {}
    eng.zero_grad()
    want = eng.train_step_action_pg_group(batch, d["actions"], adv[:, 1].reshape(3, 1), scale, old_logprobs=d["logprob"] + 0.04, kl_coef=0.0, clip=(0.8, 1.2),
                                          returns=ret[:, 1], old_values=d["value"] + 0.3, **kw, **extra)
    g_want = si.export_grads(eng)
    eng.zero_grad()
    f.check(set(got) == set(want), f"statistics {sorted(got)}")
    for k in want:
        f.same_bits(got[k], want[k], f"statistics: {k}")
    f.same_grads(g_got, g_want, "ppo_step_continuous vs the hand-assembled group step")
    f.every_tensor_nonzero(g_got, "the PPO step"), f.all_finite(g_got, "the PPO step")
    with pytest.raises(ValueError, match="actions"):
        rl.ppo_step_continuous(eng, batch, d["actions"], d["logprob"][:, 0], adv[:, 1], ret[:, 1], scale=scale)
    f.done()


# ---- predict_action: SampledActions.value -------------------------------------------------------------------------------------------------------
UNNORM = "d"


def test_predict_action_reports_the_value(dev, monkeypatch):
    modeling, config_mod, ops = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config"), load("openvla-oft_amd.ops")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats={UNNORM: {"action": {"q01": [-2.0] * 7, "q99": [1.0] * 7}}})
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict={k[len("action_head."):]: v for k, v in sd.items() if k.startswith("action_head.")})
    g = torch.Generator().manual_seed(5)
    prompts = [(torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]), None) for n in (7, 12, 9)]
    pv = torch.randn(3, 12, 56, 56, generator=g).to(BF).float()
    vla.engine.token_sample.seed = 0x0123456789ABCDEF
    C = cfg.chunk

    def call(scale, **kw):
        vla.engine.token_sample.call = 3
        return vla.predict_action_batch(prompts, pv, unnorm_key=UNNORM, action_head=head, action_noise_scale=scale, return_sample=True, sample_keys=[5, 8, 50], **kw)

    a0, h0, s0 = call(0.5)
    assert s0.value is None, "no value without load_value_head"
    names0, _ = _launches(monkeypatch, lambda: call(0.5))
    vsd = {"value.weight": ((torch.rand(1, cfg.llm_dim, generator=g) * 2 - 1) * 0.02).to(BF), "value.bias": torch.tensor([0.375]).to(BF)}
    assert vla.load_value_head(vsd) is vla.value_head
    names1, (a1, h1, s1) = _launches(monkeypatch, lambda: call(0.5))
    assert np.array_equal(a0, a1) and torch.equal(h0, h1) and all(torch.equal(i32(getattr(s0, k)), i32(getattr(s1, k))) for k in ("actions", "logprobs", "mean"))
    assert s1.value.shape == (3,) and s1.value.dtype == F32 and names1.count("ovla_value_loss") == 1 and "ovla_value_loss" not in names0
    # the engine's value of the same observations: the head's hidden output of the same action rows, the value head, the pooling launch
    comp = head.comp
    _, _, _, h2 = comp.fwd(h1.to(BF).contiguous().view(-1, cfg.llm_dim), return_hidden=True)
    want = ops.value_loss(ops.head_out_fwd(h2, vsd["value.weight"].to(dev), vsd["value.bias"].to(dev)), C)
    assert torch.equal(i32(s1.value), i32(want)) and float(s1.value.abs().min()) > 0
    # without return_sample nothing changes; an observation alone reports its own value; predict_action too
    vla.engine.token_sample.call = 3
    plain = vla.predict_action_batch(prompts, pv, unnorm_key=UNNORM, action_head=head, action_noise_scale=0.5, sample_keys=[5, 8, 50])
    assert len(plain) == 2 and np.array_equal(plain[0], a1)
    vla.engine.token_sample.call = 3
    _, _, s_one = vla.predict_action_batch(prompts[1:2], pv[1:2], unnorm_key=UNNORM, action_head=head, action_noise_scale=0.5, return_sample=True, sample_keys=[8])
    assert torch.equal(i32(s_one.value), i32(s1.value[1:2]))
    ids, mask = prompts[0][0][None], torch.ones((1, len(prompts[0][0])), dtype=torch.bool)
    vla.engine.token_sample.call = 3
    one = vla.predict_action(input_ids=ids, attention_mask=mask, pixel_values=pv[:1], unnorm_key=UNNORM, action_head=head, action_noise_scale=0.5, return_sample=True,
                             sample_keys=[5])
    assert one[2].value.shape == (1,) and bool(torch.isfinite(one[2].value).all())
    _, _, _, h2_one = comp.fwd(one[1].to(BF).contiguous().view(-1, cfg.llm_dim), return_hidden=True)
    assert torch.equal(i32(one[2].value), i32(ops.value_loss(vla.value_head.fwd(h2_one), C)))
    # with the learned scale as well
    vla.attach_scale_head(0.5)
    _, _, s2 = call("learned")
    assert torch.equal(i32(s2.value), i32(s1.value)) and s2.log_scale is not None
