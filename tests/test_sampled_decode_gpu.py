"""do_sample=True through predict_action / predict_action_batch: the batched discrete chunk under hipGraph replay (ovla_sample_tokens inside the
graph, its state and row keys in static buffers) equals the eager run bit for bit, every call draws anew, an observation's draw depends on its
key and not on its batch, `pad_to` changes nothing -- and with do_sample=False a chunk issues the launches it always did."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
UNNORM = "d"


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats={UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}})
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head."))
    g = torch.Generator().manual_seed(5)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in (7, 12, 9)]
    pv = torch.randn(3, 12, 56, 56, generator=g).to(BF).float()
    vla.engine.token_sample.seed = 0x0123456789ABCDEF
    return dict(vla=vla, head=head, cfg=cfg, prompts=prompts, pv=pv, modeling=modeling)


def _run(w, idx, call, graph=False, **kw):
    """One sampled batch of the observations `idx` at stream position `call` -> (actions, tokens, logprobs, entropy) on the host."""
    vla = w["vla"]
    vla.engine.token_sample.call = call
    vla.use_graph = graph              # (enable_graph_replay(False) would drop the captured graphs: the tests below count them)
    try:
        a, h, st = vla.predict_action_batch([(w["prompts"][i], None) for i in idx], w["pv"][idx], unnorm_key=UNNORM, do_sample=True, return_tokens=True,
                                            temperature=kw.pop("temperature", 1.6), **kw)
    finally:
        vla.use_graph = False
    assert vla.engine.token_sample.call == call + 1, "one sampled call advances the stream by one"
    assert isinstance(st, w["modeling"].SampledTokens) and st.tokens.shape == (len(idx), w["cfg"].num_action_tokens)
    return a, st.tokens.cpu(), st.logprobs.cpu(), st.entropy.cpu()


def _same(x, y):
    return np.array_equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2].view(torch.int32), y[2].view(torch.int32)) \
        and torch.equal(x[3].view(torch.int32), y[3].view(torch.int32))


def test_actions_come_from_the_drawn_bins(world):
    vla = world["vla"]
    a, tok, lp, ent = _run(world, [0, 1, 2], 3)
    lo, hi = vla.engine.token_window("actions")
    assert bool(((tok >= lo) & (tok < hi)).all()) and bool((lp < 0).all()) and bool((ent > 0).all())
    bins = np.clip(vla.vocab_size - tok.numpy() - 1, 0, vla.bin_centers.shape[0] - 1)
    want = np.stack([vla._unnormalize_actions(vla.bin_centers[bins[b]].reshape(world["cfg"].chunk, world["cfg"].action_dim), UNNORM) for b in range(3)])
    assert np.array_equal(a, want)
    greedy = vla.predict_action_batch([(p, None) for p in world["prompts"]], world["pv"], unnorm_key=UNNORM)[0]
    assert not np.array_equal(a, greedy), "T = 1.6 on 168 rows: the draw is not the greedy decode"


def test_graph_replay_equals_eager_and_every_call_draws_anew(world):
    vla = world["vla"]
    eager = _run(world, [0, 1, 2], 11)
    captured = _run(world, [0, 1, 2], 11, graph=True)              # the capture and its first replay
    assert any(k[0] == "batch" and "sample" in k for k in vla._graphs), "the sampled batch took the graph path"
    replayed = _run(world, [0, 1, 2], 11, graph=True)              # a replay of the captured graph
    assert _same(eager, captured) and _same(eager, replayed), "graph replay on == off, bit for bit"
    n_graphs = len(vla._graphs)
    nxt = _run(world, [0, 1, 2], 12, graph=True)
    assert len(vla._graphs) == n_graphs, "another call is the same graph"
    assert not torch.equal(nxt[1], replayed[1]), "an advanced call draws other tokens"
    assert _same(nxt, _run(world, [0, 1, 2], 12))
    _run(world, [0, 1, 2], 12, graph=True, temperature=0.5)
    assert len(vla._graphs) == n_graphs + 1, "the temperature is part of the graph key"
    # sample_seed replaces the stream's seed for the call
    assert not torch.equal(_run(world, [0, 1, 2], 12, sample_seed=99)[1], nxt[1])
    assert _same(_run(world, [0, 1, 2], 12, sample_seed=99), _run(world, [0, 1, 2], 12, graph=True, sample_seed=99))


@pytest.mark.parametrize("graph", (False, True))
def test_an_observations_draw_depends_on_its_key_not_on_its_batch(world, graph):
    full = _run(world, [0, 1, 2], 20, graph=graph, sample_keys=[5, 6, 7])
    alone = _run(world, [1], 20, graph=graph, sample_keys=[6])
    assert np.array_equal(full[0][1], alone[0][0]) and torch.equal(full[1][1], alone[1][0]) and torch.equal(full[2][1].view(torch.int32), alone[2][0].view(torch.int32))
    swapped = _run(world, [2, 1, 0], 20, graph=graph, sample_keys=[7, 6, 5])
    assert torch.equal(swapped[1][[2, 1, 0]], full[1])
    other_key = _run(world, [1], 20, graph=graph, sample_keys=[8])
    assert not torch.equal(other_key[1], alone[1])
    padded = _run(world, [0, 1, 2], 20, graph=graph, sample_keys=[5, 6, 7], pad_to=4)
    assert _same(padded, full), "pad_to changes nothing for the real observations"
    assert _same(_run(world, [0, 1, 2], 20, graph=graph, pad_to=4), _run(world, [0, 1, 2], 20, graph=graph)), "default keys: the observations' indices"


def test_predict_action_samples_too(world):
    vla, p = world["vla"], world["prompts"][0]
    kw = dict(unnorm_key=UNNORM, pixel_values=world["pv"][:1], attention_mask=torch.ones(1, p.numel(), dtype=torch.bool))
    vla.engine.token_sample.call = 30
    a, h, st = vla.predict_action(p[None], do_sample=True, return_tokens=True, temperature=1.6, **kw)
    assert vla.engine.token_sample.call == 31 and st.tokens.shape == (1, world["cfg"].num_action_tokens)
    vla.engine.token_sample.call = 30
    a2, _, st2 = vla.predict_action(p[None], do_sample=True, return_tokens=True, temperature=1.6, **kw)
    assert np.array_equal(a, a2) and torch.equal(st.tokens, st2.tokens)
    a3, _, st3 = vla.predict_action(p[None], do_sample=True, return_tokens=True, temperature=1.6, **kw)      # call 31
    assert not torch.equal(st3.tokens, st.tokens)
    assert len(vla.predict_action(p[None], do_sample=False, **kw)) == 2


def test_refusals(world):
    vla, head = world["vla"], world["head"]
    vla.enable_graph_replay(False)     # drops the graphs the tests above captured
    batch = [(p, None) for p in world["prompts"]]
    call = vla.engine.token_sample.call
    with pytest.raises(ValueError, match="do_sample=True draws action TOKENS"):
        vla.predict_action_batch(batch, world["pv"], unnorm_key=UNNORM, action_head=head, do_sample=True)
    p = world["prompts"][0]
    with pytest.raises(ValueError, match="do_sample=True draws action TOKENS"):
        vla.predict_action(p[None], unnorm_key=UNNORM, action_head=head, do_sample=True, pixel_values=world["pv"][:1],
                           attention_mask=torch.ones(1, p.numel(), dtype=torch.bool))
    with pytest.raises(ValueError, match="return_tokens"):
        vla.predict_action_batch(batch, world["pv"], unnorm_key=UNNORM, return_tokens=True)
    with pytest.raises(ValueError, match="sample_keys"):
        vla.predict_action_batch(batch, world["pv"], unnorm_key=UNNORM, do_sample=True, sample_keys=[1, 2])
    assert vla.engine.token_sample.call == call, "a refused call does not advance the stream"


def _launches(monkeypatch, fn):
    """The names of the library calls `fn` issues, in order (every entry point reports through _lib.check)."""
    lib, names = load("openvla-oft_amd._lib"), []
    real = lib.check

    def check(rc, what):
        names.append(what)
        return real(rc, what)

    with monkeypatch.context() as m:
        m.setattr(lib, "check", check)
        fn()
    return names


@pytest.mark.parametrize("graph", (False, True))
def test_without_do_sample_a_chunk_issues_the_launches_it_always_did(world, monkeypatch, graph):
    """The greedy chunk never reaches the sampler, and the sampled chunk is the greedy one with its decode launch exchanged: eager, lm_head's logits
    go to ovla_sample_tokens instead of the fp32 copy torch's argmax reads; captured, ovla_sample_tokens stands where ovla_argmax_bins stood."""
    vla = world["vla"]
    batch = [(p, None) for p in world["prompts"][:2]]
    vla._graphs.clear()                # both captures happen inside the counted calls

    def run(**kw):
        vla.enable_graph_replay(graph)
        try:
            vla.predict_action_batch(batch, world["pv"][:2], unnorm_key=UNNORM, **kw)
        finally:
            vla.enable_graph_replay(False)

    greedy = _launches(monkeypatch, run)
    sampled = _launches(monkeypatch, lambda: run(do_sample=True, temperature=1.6))
    assert "ovla_sample_tokens" not in greedy and len(greedy) > 50
    old = "ovla_argmax_bins" if graph else "ovla_cvt_bf16_to_f32"
    assert greedy.count(old) >= 1
    assert [("ovla_sample_tokens" if n == old else n) for n in greedy] == sampled, "the sampled chunk differs from the greedy one in more than the decode launch"
