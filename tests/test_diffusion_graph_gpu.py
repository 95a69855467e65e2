"""The diffusion head's DDIM sampler under graph replay (engine.DiffusionGraph: a prefix capture and a step capture replayed n_steps times, the
scheduler step on the device) against the host loop that stays in place with graph replay off: the same bits, for `predict_action`,
`predict_action_batch` and the server.  5-step sampler, explicit start noise, the tiny model of the G19 reference fixture."""
import importlib

import numpy as np
import pytest
import torch

from tests import test_ref_fixtures_gpu as rf     # helpers only: fixture(), build(), relmax()

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
KEY = "libero"
N_STEPS = 5
LENS = (5, 14, 9)     # with the 56 action slots: text buckets of 64 and 72 tokens


def _world(dev, mode, film):
    g = rf.fixture("g19_ref_forward_predict.npz")
    modeling, engine = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.engine")
    action = {k[len("stats."):]: v.tolist() for k, v in g.items() if k.startswith("stats.")}
    stats = {KEY: {"action": action, "proprio": {"q01": [-2.0] * 8, "q99": [2.0] * 8, "min": [-3.0] * 8, "max": [3.0] * 8}}}
    vla, cfg, sd, sub, pp = rf.build(dev, g, mode, film, diffusion=True, stats=stats)
    assert int(g["diffusion.T"]) == N_STEPS
    head = modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=N_STEPS, device=dev, state_dict=sub("action_head."))
    nap = modeling.NoisyActionProjector(cfg.llm_dim, device=dev, state_dict=sub("noisy_action_projector."))
    gen = torch.Generator().manual_seed(21)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=gen)]) for n in LENS]
    return dict(g=g, vla=vla, cfg=cfg, pp=pp, head=head, nap=nap, film=film, stats=stats, engine=engine, prompts=prompts,
                pv=torch.randn(len(LENS), 12, 56, 56, generator=gen).to(BF).float(),
                proprio=(torch.rand(len(LENS), 8, generator=gen) * 2 - 1).to(BF).float().numpy(),
                noise=torch.randn(2, len(LENS), 8, 7, generator=gen))


_worlds = {}


@pytest.fixture
def world(dev, request):
    """One model per (mask mode, FiLM) for the module; graph replay is off (and every captured graph dropped) when a test ends."""
    key = getattr(request, "param", ("bidirectional", False))
    if key not in _worlds:
        _worlds[key] = _world(dev, *key)
    w = _worlds[key]
    yield w
    w["vla"].enable_graph_replay(False)


PLAIN, FILM = ("bidirectional", False), ("bidirectional", True)


def _one(w, noise):
    """predict_action on the fixture's observation 0 -> (actions, hidden states as a host copy)."""
    g, pid = w["g"], torch.from_numpy(w["g"]["prompt_ids"])
    a, h = w["vla"].predict_action(input_ids=pid, unnorm_key=KEY, proprio=g["proprio"][0], proprio_projector=w["pp"], action_head=w["head"],
                                   noisy_action_projector=w["nap"], use_film=w["film"], pixel_values=torch.from_numpy(g["pixel_values"][:1]).to(BF),
                                   attention_mask=torch.ones_like(pid, dtype=torch.bool), noise=noise)
    assert a.shape == (8, 7) and tuple(h.shape) == (1, 56, w["cfg"].llm_dim)
    return a, h.float().cpu().numpy()


def _batch(w, idx, noise, pad_to=None):
    a, h = w["vla"].predict_action_batch([(w["prompts"][i], None) for i in idx], w["pv"][idx], unnorm_key=KEY, proprio=w["proprio"][idx],
                                         proprio_projector=w["pp"], action_head=w["head"], noisy_action_projector=w["nap"], use_film=w["film"],
                                         noise=noise[idx], pad_to=pad_to)
    assert a.shape == (len(idx), 8, 7) and tuple(h.shape) == (len(idx), 56, w["cfg"].llm_dim)
    return a, h.float().cpu().numpy()


def _diffusion_graphs(w):
    return [g for g in w["vla"]._graphs.values() if isinstance(g, w["engine"].DiffusionGraph)]


@pytest.mark.parametrize("world", [PLAIN, FILM], indirect=True, ids=["plain", "film"])
def test_predict_action_graph_equals_host_loop(world):
    w, vla = world, world["vla"]
    n0, n1 = world["noise"][0, :1], world["noise"][1, :1]
    a_e, h_e = _one(w, n0)
    a_e1, h_e1 = _one(w, n1)
    assert not np.array_equal(a_e, a_e1)
    vla.enable_graph_replay(True)
    a_g, h_g = _one(w, n0)
    assert np.array_equal(a_e, a_g) and np.array_equal(h_e, h_g), "graph replay on == off, bit for bit"
    # a second chunk on the SAME captured graphs, from other noise: the sample and the step index start afresh
    a_g1, h_g1 = _one(w, n1)
    assert np.array_equal(a_e1, a_g1) and np.array_equal(h_e1, h_g1)
    a_g0, _ = _one(w, n0)
    assert np.array_equal(a_e, a_g0)
    graphs = _diffusion_graphs(w)
    assert len(graphs) == 1 and len(vla._graphs) == 1, "one capture served the three chunks"
    assert graphs[0].step_replays == 3 * N_STEPS


def test_graphed_call_replays_a_diffusion_graph(world):
    """Proof that the graph path ran: a DiffusionGraph sits in vla._graphs and its step graph was replayed n_steps times for the one chunk; with
    graph replay off nothing is captured."""
    w, vla = world, world["vla"]
    _one(w, w["noise"][0, :1])
    assert not vla._graphs
    vla.enable_graph_replay(True)
    _one(w, w["noise"][0, :1])
    graphs = _diffusion_graphs(w)
    assert len(graphs) == 1 and graphs[0].n_steps == N_STEPS and graphs[0].step_replays == N_STEPS
    assert int(graphs[0].step.item()) == N_STEPS, "the device step index walked the whole schedule"


@pytest.mark.parametrize("world", [PLAIN, FILM], indirect=True, ids=["plain", "film"])
def test_predict_action_batch_graph_equals_host_loop(world):
    w, vla, noise = world, world["vla"], world["noise"][0]
    idx = [0, 1, 2]
    a_e, h_e = _batch(w, idx, noise)
    vla.enable_graph_replay(True)
    a_g, h_g = _batch(w, idx, noise)
    assert np.array_equal(a_e, a_g) and np.array_equal(h_e, h_g), "B = 3, three prompt lengths: graph replay on == off"
    assert any(k[0] == "batch" and k[1] == 3 for k in vla._graphs) and len(_diffusion_graphs(w)) == 1
    for b in idx:
        a_1, h_1 = _batch(w, [b], noise)
        assert np.array_equal(a_g[b], a_1[0]) and np.array_equal(h_g[b], h_1[0]), f"row {b} == the same observation as a batch of one"
    a_4, h_4 = _batch(w, idx, noise, pad_to=4)
    assert np.array_equal(a_g, a_4) and np.array_equal(h_g, h_4), "pad_to = 4: the same bits for the three real rows"
    assert any(k[0] == "batch" and k[1] == 4 for k in vla._graphs)
    assert all(g.step_replays % N_STEPS == 0 and g.step_replays > 0 for g in _diffusion_graphs(w))
    assert not np.array_equal(a_g[0], a_g[1])


@pytest.mark.parametrize("world", [("causal", True), FILM], indirect=True, ids=["causal", "bidirectional"])
def test_graphed_sampler_meets_the_g19_reference_loop(world):
    """The bounds of test_g19_diffusion_predict_action_matches_reference_loop, for the sampler under graph replay."""
    w, g = world, world["g"]
    mode = w["cfg"].mask_mode
    w["vla"].enable_graph_replay(True)
    act, ah = _one(w, torch.from_numpy(g["diffusion.start_noise"]))
    assert len(_diffusion_graphs(w)) == 1
    action = w["stats"][KEY]["action"]
    scale = np.where(action["mask"], 0.5 * (np.array(action["q99"]) - np.array(action["q01"])), 1.0)
    e = np.abs((act - g[f"{mode}.film.predict.p.diffusion.actions"]) / scale).max()
    eh = rf.relmax(ah, g[f"{mode}.film.predict.p.diffusion.hidden"])
    print(f"G19 diffusion under graph replay, {mode}: actions L-inf {e:.3e}, last-step hidden rel-max {eh:.3e}")
    assert e < 0.1 and eh < 6e-2


def test_server_runs_the_diffusion_head_under_graph_replay(world):
    dep, utils = load("openvla-oft_amd.vla_scripts.deploy"), load("openvla-oft_amd.experiments.robot.openvla_utils")

    class P56(utils.PrismaticProcessor):   # the tiny test towers take 56 x 56 inputs
        def __call__(self, text, image):
            out = super().__call__(text, image)
            out["pixel_values"] = out["pixel_values"][:, :, ::4, ::4].contiguous()
            return out

    rng = np.random.default_rng(4)
    obs = [{"full_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), "wrist_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
            "state": rng.uniform(-1, 1, 8), "instruction": t} for t in ("pick up the black bowl", "open the drawer")]
    w, vla = world, world["vla"]
    dcfg = dep.DeployConfig(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=KEY, num_open_loop_steps=8, use_l1_regression=False,
                            use_diffusion=True, num_diffusion_steps=N_STEPS)
    assert not vla.use_graph
    server = dep.OpenVLAServer(dcfg, vla=vla, processor=P56(lambda text: [1] + [3 + (ord(c) % 200) for c in text][:20]), action_head=w["head"],
                               proprio_projector=w["pp"], noisy_action_projector=w["nap"])
    assert vla.use_graph, "OpenVLAServer(use_diffusion=True) turns graph replay on"
    chunks = server.act_batch([dep._encode(o) for o in obs])
    assert chunks != "error" and len(chunks) == 2
    for c in chunks:
        c = [dep._decode(a) for a in c]
        assert len(c) == 8 and all(a.shape == (7,) and np.isfinite(a).all() for a in c)
    graphs = _diffusion_graphs(w)
    assert len(graphs) == 1 and graphs[0].B == 2 and graphs[0].step_replays == N_STEPS, "the batch of two was sampled by a DiffusionGraph"
    single = server.act(dep._encode(obs[0]))
    assert single != "error" and len(single) == 8
    assert len(_diffusion_graphs(w)) == 2
