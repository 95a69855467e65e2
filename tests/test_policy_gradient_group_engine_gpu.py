"""The group forms through the engine on the tiny discrete world of tests/step_invariants.py: train_step_policy_gradient_group anchored bit for bit
on train_step_policy_gradient, G draws from one forward, the frozen reference policy, the first-order effect of each term, rl.grpo_step, and
predict_action_batch(num_samples=G)."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import step_invariants as si

pytestmark = pytest.mark.gpu
F32, BF = torch.float32, torch.bfloat16
ADV3 = (1.0, -0.5, 2.0)


def i32(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def world(dev):
    w = si.make_world(dev, "discrete")
    eng, batch = w["eng"], w["batches"][0]
    eng.token_sample.seed, eng.token_sample.call = 0xABCDEF0123456789, 5
    w["draw"] = eng.sample_action_tokens(batch, temperature=1.0)                      # [B, A]: the single draw the anchors train on
    eng.token_sample.call = 6
    w["keys4"] = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23], [7, 5, 3, 1]])
    w["draw4"] = eng.sample_action_tokens(batch, temperature=1.0, num_samples=4, row_keys=w["keys4"])
    return w


def _single(world, loss_scale=1.0, **kw):
    eng, batch = world["eng"], world["batches"][0]
    eng.zero_grad()
    stats = eng.train_step_policy_gradient(batch, world["draw"]["tokens"], kw.pop("advantages", torch.tensor(ADV3)), loss_scale=loss_scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def _group(world, tokens, advantages, loss_scale=1.0, **kw):
    eng, batch = world["eng"], world["batches"][0]
    eng.zero_grad()
    stats = eng.train_step_policy_gradient_group(batch, tokens, advantages, loss_scale=loss_scale, **kw)
    return {k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)


def test_group_step_is_the_single_step(world):
    """G = 1: train_step_policy_gradient's accumulators bit for bit.  G = 2 duplicated draws: the same (x + x and the halved scale are exact).
    G = 4 with three zero-advantage draws at 4 x loss_scale: the same (skipped samples add nothing; 4 ls / (4 n) is ls / n)."""
    d, f = world["draw"], si.Findings()
    A = world["cfg"].num_action_tokens
    old = (d["logprob"] + 0.1 * torch.tensor(ADV3, device=d["logprob"].device)[:, None]).contiguous()     # ratios e^-0.1, e^0.05, e^-0.2: some gated
    for o, name in ((None, "no old log-probabilities"), (old, "old log-probabilities")):
        s1, want = _single(world, loss_scale=0.5, old_logprobs=o, temperature=1.6)
        f.every_tensor_nonzero(want, name)
        tok1 = d["tokens"][:, None, :]
        s, got = _group(world, tok1, torch.tensor(ADV3)[:, None], loss_scale=0.5, old_logprobs=None if o is None else o[:, None, :], temperature=1.6)
        f.same_grads(got, want, f"G = 1 ({name})")
        for k in s1:
            f.same_bits(s[k], s1[k], f"G = 1 ({name}): {k}")
        f.check(float(s["kl"]) == 0.0, "kl without a reference")
        _, got = _group(world, tok1.expand(3, 2, A), torch.tensor(ADV3)[:, None].expand(3, 2), loss_scale=0.5,
                        old_logprobs=None if o is None else o[:, None, :].expand(3, 2, A), temperature=1.6)
        f.same_grads(got, want, f"G = 2 duplicated ({name})")
        g = torch.Generator().manual_seed(3)
        tok4 = torch.randint(31744, 32000, (3, 4, A), generator=g).int()
        tok4[:, 2] = d["tokens"].cpu()
        adv4 = torch.zeros(3, 4)
        adv4[:, 2] = torch.tensor(ADV3)
        old4 = None
        if o is not None:
            old4 = torch.full((3, 4, A), float("nan"))
            old4[:, 2] = o.cpu()
        _, got = _group(world, tok4, adv4, loss_scale=2.0, old_logprobs=old4, temperature=1.6)
        f.same_grads(got, want, f"G = 4, three zero-advantage draws ({name})")
    f.done()


def test_reproducible_and_loss_scale_exact(world):
    d4, f = world["draw4"], si.Findings()
    adv = torch.tensor([[1.0, -0.5, 2.0, -1.0], [0.25, 0.5, -2.0, 1.0], [-1.0, -1.0, 3.0, 0.5]])
    kw = dict(old_logprobs=d4["logprob"], ref_logprobs=d4["logprob"] + 0.5, kl_coef=0.0625, entropy_coef=0.03125, temperature=1.6)
    s1, g1 = _group(world, d4["tokens"], adv, **kw)
    s2, g2 = _group(world, d4["tokens"], adv, **kw)
    f.same_grads(g1, g2, "two identical group steps")
    for k in s1:
        f.same_bits(s1[k], s2[k], f"two identical group steps: {k}")
    _, g4 = _group(world, d4["tokens"], adv, loss_scale=4.0, **kw)
    f.same_grads(g4, {n: 4.0 * g for n, g in g1.items()}, "loss_scale = 4 vs 4 x (loss_scale = 1)")
    f.all_finite(g1, "group step"), f.every_tensor_nonzero(g1, "group step")
    f.check(float(s1["kl"]) > 0.0 and float(s1["entropy"]) > 0.0, "kl and entropy are reported")
    f.done()


def test_num_samples_draws_from_one_forward(world, monkeypatch):
    eng, batch, cfg = world["eng"], world["batches"][0], world["cfg"]
    A, d4, keys = cfg.num_action_tokens, world["draw4"], world["keys4"]
    for k, dt in (("tokens", torch.int32), ("bins", torch.int32), ("logprob", F32)):
        assert d4[k].shape == (3, 4, A) and d4[k].dtype == dt and d4[k].is_cuda
    assert d4["entropy"].shape == (3, A)
    lib, names = importlib.import_module("openvla-oft_amd._lib"), []
    real = lib.check
    with monkeypatch.context() as m:
        m.setattr(lib, "check", lambda rc, what: (names.append(what), real(rc, what))[1])
        eng.token_sample.call = 6
        again = eng.sample_action_tokens(batch, temperature=1.0, num_samples=4, row_keys=keys)
    assert eng.token_sample.call == 7, "the group draw advances the stream once"
    assert names.count("ovla_sample_tokens_group") == 1 and "ovla_sample_tokens" not in names
    assert torch.equal(again["tokens"], d4["tokens"])
    for g in range(4):
        eng.token_sample.call = 6
        one = eng.sample_action_tokens(batch, temperature=1.0, row_keys=keys[:, g])
        assert torch.equal(one["tokens"], d4["tokens"][:, g]) and torch.equal(one["bins"], d4["bins"][:, g]), f"draw {g}: tokens"
        assert torch.equal(i32(one["logprob"]), i32(d4["logprob"][:, g])) and torch.equal(i32(one["entropy"]), i32(d4["entropy"])), f"draw {g}: logprob / entropy bits"
    assert not torch.equal(d4["tokens"][:, 0], d4["tokens"][:, 1])
    # default keys b * G + g: the batch of repeated observations under default keys
    eng.token_sample.call = 6
    dflt = eng.sample_action_tokens(batch, num_samples=2)
    eng.token_sample.call = 6
    one = eng.sample_action_tokens(batch, row_keys=[1, 3, 5])
    assert torch.equal(dflt["tokens"][:, 1], one["tokens"])
    # [B, G, A] keys
    eng.token_sample.call = 6
    full = eng.sample_action_tokens(batch, num_samples=4, row_keys=keys[:, :, None] * A + torch.arange(A)[None, None, :])
    assert torch.equal(full["tokens"], d4["tokens"])
    pl = eng.policy_logprobs(batch, d4["tokens"])
    assert pl["logprob"].shape == (3, 4, A) and torch.equal(i32(pl["logprob"]), i32(d4["logprob"])) and torch.equal(i32(pl["entropy"]), i32(d4["entropy"]))
    with pytest.raises(ValueError, match="num_samples"):
        eng.sample_action_tokens(batch, num_samples=65)
    with pytest.raises(ValueError, match="row_keys"):
        eng.sample_action_tokens(batch, num_samples=4, row_keys=[1, 2, 3])


def _train_two_steps(eng, batch, d4):
    for st in eng.stores:
        st.init_optimizer()
    adv = torch.tensor([[1.0, -1.0, 0.5, -0.5]] * 3)
    for _ in range(2):
        eng.zero_grad()
        eng.train_step_policy_gradient_group(batch, d4["tokens"], adv)
        eng.adamw_step(1e-3)
        eng.refresh_derived()


def test_reference_policy(world):
    eng, batch, d4, f = world["eng"], world["batches"][0], world["draw4"], si.Findings()
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    adv = torch.tensor([[1.0, -0.5, 2.0, -1.0], [0.25, 0.5, -2.0, 1.0], [-1.0, -1.0, 3.0, 0.5]])
    with pytest.raises(RuntimeError, match="set_reference_policy"):
        eng.reference_logprobs(batch, d4["tokens"])
    try:
        eng.set_reference_policy()
        assert eng.has_reference_policy and eng.reference_policy_bytes() == sum(t.numel() * t.element_size() for st in eng.stores for t in st.flat.values())
        ref0 = eng.reference_logprobs(batch, d4["tokens"])["logprob"]
        f.same_bits(ref0, eng.policy_logprobs(batch, d4["tokens"])["logprob"], "reference_logprobs right after set_reference_policy")
        f.same_grads({n: t.float() for n, t in eng.export_trainable("data").items()}, {n: t.float() for n, t in snap.items()}, "the scope restored the live bits")
        s0, g0 = _group(world, d4["tokens"], adv, old_logprobs=d4["logprob"])
        s1, g1 = _group(world, d4["tokens"], adv, old_logprobs=d4["logprob"], ref_logprobs=ref0, kl_coef=0.5)
        f.same_grads(g1, g0, "on-policy reference: the kl_coef = 0 accumulators")
        f.check(float(s1["kl"]) == 0.0, "on-policy reference: kl == 0")
        _train_two_steps(eng, batch, d4)
        live = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
        f.same_bits(eng.reference_logprobs(batch, d4["tokens"])["logprob"], ref0, "reference_logprobs after two optimizer steps")
        now = eng.policy_logprobs(batch, d4["tokens"])["logprob"]
        f.check(not torch.equal(now, ref0), "policy_logprobs moved with the weights")
        f.same_grads({n: t.float() for n, t in eng.export_trainable("data").items()}, {n: t.float() for n, t in live.items()}, "the scope restored the trained bits")
        s2, _ = _group(world, d4["tokens"], adv, ref_logprobs=ref0, kl_coef=0.5)
        f.check(float(s2["kl"]) > 0.0, f"kl after training = {float(s2['kl'])}")
        # training inside the scope, and nesting
        with eng.reference_policy():
            assert eng.in_reference_scope
            for call in (lambda: eng.train_step_policy_gradient_group(batch, d4["tokens"], adv), lambda: eng.train_step_policy_gradient(batch, world["draw"]["tokens"], torch.ones(3)),
                         lambda: eng.train_step_discrete(batch), lambda: eng.adamw_step(1e-3), lambda: eng.reference_logprobs(batch, d4["tokens"])):
                with pytest.raises(RuntimeError, match="inside reference_policy"):
                    call()
        assert not eng.in_reference_scope
        if not eng.ema_enabled:
            eng.enable_ema()
        with eng.reference_policy():
            with pytest.raises(RuntimeError, match="inside reference_policy"):
                with eng.ema_weights():
                    pass
        with eng.ema_weights():
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                with eng.reference_policy():
                    pass
            with pytest.raises(RuntimeError, match="inside ema_weights"):
                eng.train_step_policy_gradient_group(batch, d4["tokens"], adv)
        # export / load round trip, in export_trainable("data")'s key layout
        sd = eng.export_reference_policy()
        assert set(sd) == set(snap) and all(torch.equal(sd[n], snap[n]) for n in snap), "the exported reference is the snapshot taken at set_reference_policy"
        eng.set_reference_policy()                                           # the reference is now the trained weights ...
        f.check(not torch.equal(eng.reference_logprobs(batch, d4["tokens"])["logprob"], ref0), "a new snapshot is another reference")
        eng.load_reference_policy({n: t.cpu() for n, t in sd.items()})       # ... and the saved one again
        f.same_bits(eng.reference_logprobs(batch, d4["tokens"])["logprob"], ref0, "reference_logprobs after the export / load round trip")
        f.same_grads({n: t.float() for n, t in eng.export_trainable("data").items()}, {n: t.float() for n, t in live.items()}, "load_reference_policy left the live bits")
        f.same_bits(eng.policy_logprobs(batch, d4["tokens"])["logprob"], now, "load_reference_policy left the derived copies")
        with pytest.raises(KeyError):
            eng.load_reference_policy({})
    finally:
        eng.drop_reference_policy()
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()
    f.done()


def test_reference_scope_in_fp32_optimizer_state_mode(dev):
    """A world of its own (the mode cannot be switched off): the scope leaves the parameters AND the fp32 master bit for bit."""
    w = si.make_world(dev, "discrete")
    eng, batch = w["eng"], w["batches"][0]
    eng.enable_fp32_optimizer_state()
    assert eng.optimizer_state_precision == "fp32"
    eng.token_sample.call = 6
    d4 = eng.sample_action_tokens(batch, num_samples=4)
    eng.set_reference_policy()
    ref0 = eng.reference_logprobs(batch, d4["tokens"])["logprob"]
    _train_two_steps(eng, batch, d4)
    live = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    master = [{dt: m.clone() for dt, m in st.master.items()} for st in eng.stores]
    assert any(len(m) for m in master)
    ref1 = eng.reference_logprobs(batch, d4["tokens"])["logprob"]
    assert torch.equal(i32(ref1), i32(ref0)) and not torch.equal(eng.policy_logprobs(batch, d4["tokens"])["logprob"], ref0)
    after = eng.export_trainable("data")
    assert all(torch.equal(after[n], live[n]) for n in live), "the parameters changed across the scope"
    for st, ms in zip(eng.stores, master):
        for dt, m in ms.items():
            assert torch.equal(i32(st.master[dt]), i32(m)), "the fp32 master changed across the scope"
        assert st.master_matches_param()


def test_first_order_effect(world):
    """One group step, then AdamW at a small learning rate: the positive-advantage draws become likelier, the negative ones less likely; an entropy
    bonus alone raises the entropy."""
    eng, batch, d4 = world["eng"], world["batches"][0], world["draw4"]
    snap = {n: t.detach().clone() for n, t in eng.export_trainable("data").items()}
    adv = torch.tensor([[1.0, -1.0, 1.0, -1.0], [-1.0, 1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]])
    pos = (adv > 0).to(eng.device)
    try:
        for entropy_coef, a in ((0.0, adv), (1.0, torch.zeros(3, 4))):
            eng.load_trainable(snap)
            for st in eng.stores:
                st.init_optimizer()
            before = eng.policy_logprobs(batch, d4["tokens"])
            eng.zero_grad()
            eng.train_step_policy_gradient_group(batch, d4["tokens"], a, entropy_coef=entropy_coef)
            eng.adamw_step(3e-4)
            eng.refresh_derived()
            after = eng.policy_logprobs(batch, d4["tokens"])
            if entropy_coef == 0.0:
                delta = (after["logprob"] - before["logprob"]).mean(-1)          # [B, G]
                assert float(delta[pos].mean()) > 0.0 and float(delta[~pos].mean()) < 0.0, f"positive draws {float(delta[pos].mean())}, negative {float(delta[~pos].mean())}"
            else:
                assert float(after["entropy"].mean()) > float(before["entropy"].mean()), "the entropy bonus did not raise the entropy"
    finally:
        eng.load_trainable(snap)
        for st in eng.stores:
            st.init_optimizer()
        eng.zero_grad()


def test_grpo_step(world):
    eng, batch, cfg, f = world["eng"], world["batches"][0], world["cfg"], si.Findings()
    rl = importlib.import_module("openvla-oft_amd.rl")
    seen = {}

    def reward_fn(b, actions):
        seen["shape"] = tuple(actions.shape)
        target = b["actions"].to(actions.device, torch.float32).reshape(3, 1, cfg.chunk, cfg.action_dim)
        return -(actions - target).abs().mean((2, 3))

    runs = []
    eng.set_reference_policy()
    try:
        for _ in range(2):
            eng.token_sample.call = 50
            eng.zero_grad()
            stats = rl.grpo_step(eng, batch, reward_fn, group_size=4, kl_coef=0.04, entropy_coef=0.01, clip=(0.8, 1.2), temperature=1.0, inner_steps=2)
            runs.append(({k: v.detach().clone() for k, v in stats.items()}, si.export_grads(eng)))
            assert eng.token_sample.call == 51
    finally:
        eng.drop_reference_policy()
        eng.zero_grad()
    assert seen["shape"] == (3, 4, cfg.chunk, cfg.action_dim)
    (s1, g1), (s2, g2) = runs
    f.same_grads(g1, g2, "two grpo_step runs from the same state")
    for k in s1:
        f.same_bits(s1[k], s2[k], f"two grpo_step runs: {k}")
    f.every_tensor_nonzero(g1, "grpo_step")
    adv = s1["advantages"]
    f.check(adv.shape == (3, 4) and bool((adv.mean(1).abs() <= 8 * 2.0 ** -23 * adv.abs().max(1).values.clamp_min(1.0)).all()), "the advantages have zero group mean")
    f.check(float(s1["kl"]) == 0.0 and float(s1["ratio"]) == 1.0, "on policy: kl == 0, ratio == 1")
    f.check(float(s1["reward"]) < 0.0 and set(s1) >= {"loss", "logprob", "entropy", "clip_frac", "ratio", "kl", "reward"}, "statistics")
    f.done()


def test_refusals(world):
    eng, batch, d4 = world["eng"], world["batches"][0], world["draw4"]
    with pytest.raises(ValueError, match="tokens"):
        eng.train_step_policy_gradient_group(batch, world["draw"]["tokens"], torch.ones(3, 1))
    with pytest.raises(ValueError, match="advantages"):
        eng.train_step_policy_gradient_group(batch, d4["tokens"], torch.ones(3))
    with pytest.raises(ValueError, match="ref_logprobs"):
        eng.train_step_policy_gradient_group(batch, d4["tokens"], torch.ones(3, 4), ref_logprobs=torch.zeros(3, 4))
    err = importlib.import_module("openvla-oft_amd._lib").OvlaError
    with pytest.raises(err, match="kl_coef"):
        eng.train_step_policy_gradient_group(batch, d4["tokens"], torch.ones(3, 4), kl_coef=-1.0)
    eng.zero_grad()


# ---- predict_action_batch(num_samples=G) ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vla_world(dev):
    modeling, config_mod = importlib.import_module("openvla-oft_amd.modeling"), importlib.import_module("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats={"d": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}})
    g = torch.Generator().manual_seed(5)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in (7, 12, 9)]
    pv = torch.randn(3, 12, 56, 56, generator=g).to(BF).float()
    vla.engine.token_sample.seed = 0x0123456789ABCDEF
    return dict(vla=vla, cfg=cfg, prompts=[(p, None) for p in prompts], pv=pv, modeling=modeling)


def test_predict_action_batch_num_samples(vla_world):
    w, vla, cfg = vla_world, vla_world["vla"], vla_world["cfg"]
    A = cfg.num_action_tokens
    keys = np.array([[5, 6, 7], [8, 9, 10], [50, 40, 30]])
    kw = dict(unnorm_key="d", do_sample=True, return_tokens=True, temperature=1.6)
    vla.engine.token_sample.call = 3
    a, h, st = vla.predict_action_batch(w["prompts"], w["pv"], num_samples=3, sample_keys=keys, **kw)
    assert vla.engine.token_sample.call == 4
    assert a.shape == (3, 3, cfg.chunk, cfg.action_dim) and h.shape[:2] == (3, A)
    assert isinstance(st, w["modeling"].SampledTokens) and st.tokens.shape == (3, 3, A) and st.logprobs.shape == (3, 3, A) and st.entropy.shape == (3, A)
    for g in range(3):
        vla.engine.token_sample.call = 3
        a1, _, st1 = vla.predict_action_batch(w["prompts"], w["pv"], sample_keys=keys[:, g], **kw)
        assert np.array_equal(a1, a[:, g]) and torch.equal(st1.tokens, st.tokens[:, g]), f"draw {g}"
        assert torch.equal(i32(st1.logprobs), i32(st.logprobs[:, g])) and torch.equal(i32(st1.entropy), i32(st.entropy))
    assert not torch.equal(st.tokens[:, 0], st.tokens[:, 1])
    vla.engine.token_sample.call = 3
    ap, _, stp = vla.predict_action_batch(w["prompts"], w["pv"], num_samples=3, sample_keys=keys, pad_to=4, **kw)
    assert np.array_equal(ap, a) and torch.equal(stp.tokens, st.tokens), "pad_to changes nothing for the real observations"
    call = vla.engine.token_sample.call
    with pytest.raises(ValueError, match="num_samples"):
        vla.predict_action_batch(w["prompts"], w["pv"], unnorm_key="d", num_samples=3)
    with pytest.raises(ValueError, match="sample_keys"):
        vla.predict_action_batch(w["prompts"], w["pv"], num_samples=3, sample_keys=[1, 2, 3], **kw)
    vla.use_graph = True
    try:
        with pytest.raises(ValueError, match="graph replay"):
            vla.predict_action_batch(w["prompts"], w["pv"], num_samples=3, **kw)
    finally:
        vla.use_graph = False
    assert vla.engine.token_sample.call == call, "a refused call does not advance the stream"
