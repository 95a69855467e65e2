"""The `/act` server with per-request policies: requests of different policies are coalesced into one forward and each answer carries the
bits of `/act_batch([payload])` alone; a server without policies answers a payload without "policy" exactly as before."""
import importlib
import threading

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
UNNORM = "suite"
PROPRIO = {"q01": [-2.0] * 8, "q99": [2.0] * 8, "min": [-3.0] * 8, "max": [3.0] * 8}
STATS = {"x": {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}, "proprio": PROPRIO}},
         "y": {UNNORM: {"action": {"q01": [-2.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 3]}, "proprio": {**PROPRIO, "q99": [1.5] * 8}}}}


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


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
            "state": rng.uniform(-1, 1, 8), "instruction": t} for t in ("pick up the black bowl", "open the drawer")]
    return utils, P56(tok), obs


@pytest.fixture(scope="module")
def world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)
    cfg = config_mod.VLAConfig.from_any(ocfg)
    sds = {nm: {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=seed).items()} for nm, seed in (("base", 0), ("x", 1), ("y", 2))}
    base = {k: v for k, v in sds["base"].items() if ".lora_" not in k and not k.startswith(("action_head.", "proprio_projector."))}
    specs = {}
    for nm in ("x", "y"):
        sd = sds[nm]
        specs[nm] = dict(lora_state_dict={k: (v * 8.0 if ".lora_B." in k else v).to(BF).float() for k, v in sd.items() if ".lora_" in k},
                         action_head=modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head.")),
                         proprio_projector=modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=_sub(sd, "proprio_projector.")),
                         norm_stats=STATS[nm])
    return dict(modeling=modeling, cfg=cfg, base=base, specs=specs, sds=sds, dev=dev)


def test_coalesced_requests_of_two_policies_share_one_forward(world):
    dep = load("openvla-oft_amd.vla_scripts.deploy")
    _, proc, obs = _glue()
    w = world
    vla = w["modeling"].OpenVLAForActionPrediction(w["cfg"], w["base"], device=w["dev"], norm_stats=STATS["x"])
    kw = dict(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=UNNORM, num_open_loop_steps=8)
    payloads = [dep._encode({**o, "policy": nm}) for o, nm in zip(obs, ("x", "y"))]
    try:
        base = dep.OpenVLAServer(dep.DeployConfig(**kw), vla=vla, processor=proc, policies=w["specs"])
        assert base._coalescer is None and vla.policies == ("x", "y")
        want = [base.act_batch([p])[0] for p in payloads]
        assert all(isinstance(a, list) and len(a) == 8 for a in want)
        swapped = base.act_batch([dep._encode({**obs[0], "policy": "y"})])[0]
        assert not np.array_equal(dep._decode(swapped[0]), dep._decode(want[0][0])), "the policy name decides the answer"
        assert base.act(dep._encode({**obs[0], "policy": "nobody"})) == "error"
        assert base.act(dep._encode(obs[0])) == "error", "a server with policies needs the name"
        alone = base.act(payloads[1])
        server = dep.OpenVLAServer(dep.DeployConfig(coalesce_ms=2000.0, max_batch=2, **kw), vla=vla, processor=proc, policies=w["specs"])
        got, gate = {}, threading.Barrier(2)

        def client(i):
            gate.wait()
            got[i] = server.act(payloads[i])

        threads = [threading.Thread(target=client, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads)
        assert server._coalescer.calls == 1, "the two policies' requests were merged into one forward"
        assert server.act(dep._encode({**obs[0], "policy": "nobody"})) == "error"
        server.close()
    finally:
        vla.enable_graph_replay(False)
    for i in range(2):
        assert isinstance(got[i], list) and len(got[i]) == 8
        for a, b in zip(got[i], want[i]):
            assert np.array_equal(dep._decode(a), dep._decode(b)), f"client {i}: coalesced /act != /act_batch([payload])"
    for a, b in zip(alone, want[1]):
        assert np.array_equal(dep._decode(a), dep._decode(b)), "uncoalesced /act with a policy == /act_batch([payload])"


def test_server_without_policies_is_unchanged(world):
    dep = load("openvla-oft_amd.vla_scripts.deploy")
    utils, proc, obs = _glue()
    w, sd = world, world["sds"]["base"]
    vla = w["modeling"].OpenVLAForActionPrediction(w["cfg"], sd, device=w["dev"], norm_stats=STATS["x"])
    head = w["modeling"].L1RegressionActionHead(w["cfg"].llm_dim, w["cfg"].llm_dim, 7, device=w["dev"], state_dict=_sub(sd, "action_head."))
    pp = w["modeling"].ProprioProjector(w["cfg"].llm_dim, 8, device=w["dev"], state_dict=_sub(sd, "proprio_projector."))
    kw = dict(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=UNNORM, num_open_loop_steps=8)
    try:
        server = dep.OpenVLAServer(dep.DeployConfig(**kw), vla=vla, processor=proc, action_head=head, proprio_projector=pp)
        assert server.policies == () and vla.policies == ()
        got = server.act(dep._encode(obs[0]))
        want = utils.get_vla_action(server.cfg, vla, proc, dict(obs[0]), obs[0]["instruction"], action_head=head, proprio_projector=pp)
        assert isinstance(got, list) and len(got) == 8
        for a, b in zip(got, want):
            assert np.array_equal(dep._decode(a), b)
        assert server.act(dep._encode({**obs[0], "policy": "x"})) == "error", "no policies configured: a named policy is an error"
    finally:
        vla.enable_graph_replay(False)
