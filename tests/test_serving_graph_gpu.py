"""The batched serving path under hipGraph replay: FiLM (ragged language average inside the graph) and the discrete head (lm_head GEMM +
ovla_argmax_bins inside the graph) equal their eager runs bit for bit; `pad_to` changes nothing for the real observations; a coalescing
server answers every `/act` caller with the bits of `/act_batch([payload])`, and a malformed request costs nobody else an answer."""
import importlib
import threading

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
UNNORM = "libero_spatial_no_noops"
TOK_POS, TOK_NEG = 31800, 31900   # bins 199 and 99 of n_tokens = 32000


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def _inputs(lens, seed):
    g = torch.Generator().manual_seed(seed)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in lens]
    return prompts, torch.randn(len(lens), 12, 56, 56, generator=g).to(BF).float(), (torch.rand(len(lens), 8, generator=g) * 2 - 1).to(BF).float().numpy()


@pytest.fixture(scope="module")
def film(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=4, film=True).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats={"d": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}, use_film=True)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head."))
    prompts, pv, _ = _inputs((6, 14, 10), 6)
    return dict(vla=vla, head=head, prompts=prompts, pv=pv)


@pytest.fixture(scope="module")
def plain(dev):
    """The standard tiny model (tests/test_api_gpu.py's) with its L1 head and proprio projector."""
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    stats = {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 1], "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]},
                      "proprio": {"q01": [-2.0] * 8, "q99": [2.0] * 8, "min": [-3.0] * 8, "max": [3.0] * 8}}}
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats=stats)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head."))
    pp = modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict={"module." + k: v for k, v in _sub(sd, "proprio_projector.").items()})
    prompts, pv, proprio = _inputs((7, 12, 9), 5)
    return dict(vla=vla, head=head, pp=pp, cfg=cfg, prompts=prompts, pv=pv, proprio=proprio)


def _graph(vla, on, fn):
    vla.enable_graph_replay(on)
    try:
        return fn()
    finally:
        vla.enable_graph_replay(False)


def test_film_batch_under_graph_replay_equals_eager(film):
    vla, head, prompts, pv = film["vla"], film["head"], film["prompts"], film["pv"]
    run = lambda idx: vla.predict_action_batch([(prompts[i], None) for i in idx], pv[idx], unnorm_key="d", action_head=head, use_film=True)  # noqa: E731
    a_e, h_e = run([0, 1, 2])
    h_e = h_e.clone()

    def graphed():
        a, h = run([0, 1, 2])
        assert any(k[0] == "batch" and k[-2] is True for k in vla._graphs), "the FiLM batch took the graph path"
        a2, h2 = run([0, 1, 2])       # a replay of the captured graph, not its capture
        a1, h1 = run([1])
        return a, h.clone(), a2, h2.clone(), a1, h1.clone()

    a_g, h_g, a_g2, h_g2, a_1, h_1 = _graph(vla, True, graphed)
    assert np.array_equal(a_e, a_g) and torch.equal(h_e, h_g), "graph replay on == off, bit for bit"
    assert np.array_equal(a_e, a_g2) and torch.equal(h_e, h_g2)
    assert np.array_equal(a_g[1], a_1[0]) and torch.equal(h_g[1], h_1[0]), "row 1 == the same observation submitted alone"
    assert not np.array_equal(a_e[0], a_e[1])


def test_discrete_batch_under_graph_replay_equals_eager(plain):
    vla, prompts, pv = plain["vla"], plain["prompts"], plain["pv"]
    run = lambda: vla.predict_action_batch([(p, None) for p in prompts], pv, unnorm_key=UNNORM)  # noqa: E731
    # An lm_head under which every action row has ONE largest logit, whatever the hidden states are: token TOK_POS carries +e_d, TOK_NEG
    # carries -e_d, two decoys carry half of that and every other row is zero, so a row's logits are {+h_d, -h_d, +-h_d / 2, 0, ...}: the
    # maximum is |h_d| at exactly one column unless h_d == 0.  d = the hidden dimension whose sign is most evenly split over the B * A
    # rows (the hidden states do not depend on lm_head), so that both tokens occur and a row mix-up would show in the actions.
    _, h0 = run()
    B, A, D = h0.shape
    hf = h0.reshape(B * A, D).float()
    split = ((hf > 0).sum(0) - B * A / 2).abs() + (hf == 0).any(0) * (B * A)
    d = int(split.argmin())
    W = torch.zeros_like(vla.engine.lm_head)
    W[TOK_POS, d], W[TOK_NEG, d], W[TOK_POS + 1, d], W[TOK_NEG + 1, d] = 1.0, -1.0, 0.5, -0.5
    vla.engine.lm_head.copy_(W)
    a_e, h_e = run()
    h_e = h_e.clone()
    assert torch.equal(h_e, h0)
    logits = vla.logits_for(h_e.view(B * A, D))
    top2 = logits.topk(2, dim=1).values
    assert bool((top2[:, 0] > top2[:, 1]).all()), "precondition: every one of the B * A rows has a unique maximum"
    tok = logits.argmax(1).cpu().numpy()
    assert set(tok.tolist()) == {TOK_POS, TOK_NEG}, "both tokens occur"

    def graphed():
        a, h = run()
        assert any(k[0] == "batch" and k[-1] is True for k in vla._graphs), "the discrete batch took the discrete graph"
        a2, h2 = run()
        return a, h.clone(), a2, h2.clone()

    a_g, h_g, a_g2, h_g2 = _graph(vla, True, graphed)
    assert torch.equal(h_e, h_g) and torch.equal(h_e, h_g2)
    assert np.array_equal(a_e, a_g) and np.array_equal(a_e, a_g2), "token-derived actions: graphed == un-graphed, exactly"
    want = vla.bin_centers[np.clip(vla.vocab_size - tok - 1, 0, vla.bin_centers.shape[0] - 1)].reshape(B, 8, 7)
    assert np.array_equal(a_g, np.stack([vla._unnormalize_actions(w, UNNORM) for w in want]))


def test_pad_to_changes_nothing_for_the_real_observations(plain):
    vla = plain["vla"]
    run = lambda pad_to: vla.predict_action_batch([(p, None) for p in plain["prompts"]], plain["pv"], unnorm_key=UNNORM, proprio=plain["proprio"],  # noqa: E731
                                                  proprio_projector=plain["pp"], action_head=plain["head"], pad_to=pad_to)
    a, h = run(None)
    a4, h4 = run(4)
    assert a4.shape == a.shape == (3, 8, 7) and h4.shape == h.shape
    assert np.array_equal(a, a4) and torch.equal(h, h4)
    a3, h3 = run(2)                   # a pad_to that is not beyond B is ignored
    assert np.array_equal(a, a3) and torch.equal(h, h3)


def _glue():
    utils = load("openvla-oft_amd.experiments.robot.openvla_utils")

    class P56(utils.PrismaticProcessor):   # the tiny test towers take 56 x 56 inputs
        def __call__(self, text, image):
            out = super().__call__(text, image)
            out["pixel_values"] = out["pixel_values"][:, :, ::4, ::4].contiguous()
            return out

    tok = lambda text: [1] + [3 + (ord(c) % 200) for c in text][:20]  # noqa: E731
    rng = np.random.default_rng(4)
    obs = [{"full_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), "wrist_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
            "state": rng.uniform(-1, 1, 8), "instruction": t} for t in ("pick up the black bowl", "open the drawer", "put the cup on the plate", "x")]
    return P56(tok), obs


def test_coalescing_server_answers_like_act_batch_of_one(plain):
    dep = load("openvla-oft_amd.vla_scripts.deploy")
    proc, obs = _glue()
    vla, head, pp = plain["vla"], plain["head"], plain["pp"]
    kw = dict(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=UNNORM, num_open_loop_steps=8)
    payloads = [dep._encode(o) for o in obs]
    del payloads[3]["instruction"]        # malformed at the request level only: nothing unusual ever reaches a kernel
    try:
        base = dep.OpenVLAServer(dep.DeployConfig(**kw), vla=vla, processor=proc, action_head=head, proprio_projector=pp)
        assert base._coalescer is None
        want = [base.act_batch([p])[0] for p in payloads[:3]]
        assert base.act_batch([payloads[3]]) == "error"
        server = dep.OpenVLAServer(dep.DeployConfig(coalesce_ms=20.0, **kw), vla=vla, processor=proc, action_head=head, proprio_projector=pp)
        got, gate = {}, threading.Barrier(4)

        def client(i):
            gate.wait()
            got[i] = server.act(payloads[i])

        threads = [threading.Thread(target=client, args=(i,)) for i in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads)
        print(f"forwards for the three valid requests: {server._coalescer.calls}")
        assert server._coalescer.calls < 3, "at least two of the three valid requests shared a forward"
        assert any(k[0] == "batch" and k[1] >= 2 for k in vla._graphs), "a merged forward (B >= 2) ran under graph replay"
        grouped = server.act_batch(payloads[:3])      # /act_batch goes through the same worker, as one group
        server.close()
        assert not server._coalescer.alive
    finally:
        vla.enable_graph_replay(False)
    assert got[3] == "error", "the malformed request answers 'error'"
    for i in range(3):
        assert isinstance(want[i], list) and len(want[i]) == 8 and isinstance(got[i], list) and len(got[i]) == 8
        for a, b, c in zip(got[i], want[i], grouped[i]):
            assert np.array_equal(dep._decode(a), dep._decode(b)), f"client {i}: coalesced /act != /act_batch([payload])"
            assert np.array_equal(dep._decode(c), dep._decode(b))
    assert not np.array_equal(dep._decode(want[0][0]), dep._decode(want[1][0]))
