"""The policy pool: any number of registered policies on one base model, `resident` of them in the adapter slots at a time, swapped in by one
ovla_copy_table launch each (enable_policy_pool / add_policy / remove_policy / predict_action_batch(policy=[...])).  Six policies (seeds 1-6)
on the tiny configuration of test_multi_adapter_gpu.py; every comparison is bit for bit."""
import copy
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
LENS = [7, 12, 9, 15, 7]
B_SCALE = 8.0   # as in test_multi_adapter_gpu.py: two policies' actions differ far beyond rounding
NAMES = ("x", "y", "z", "u", "v", "w")
PROPRIO = {"q01": [-2.0] * 8, "q99": [2.0] * 8, "min": [-3.0] * 8, "max": [3.0] * 8}
IDENT = {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}, "proprio": PROPRIO}}
STATS_ODD = {UNNORM: {"action": {"q01": [-2.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 3]}, "proprio": {**PROPRIO, "q99": [1.5] * 8}}}
STATS = {nm: (STATS_ODD if k % 2 else IDENT) for k, nm in enumerate(NAMES)}
ROTATION = ("xyzu", "vwxy", "zuvw", "xyzu")


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)
    cfg = config_mod.VLAConfig.from_any(ocfg)
    base = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items() if ".lora_" not in k and not k.startswith(("action_head.", "proprio_projector."))}
    pol = {}
    for seed, nm in enumerate(NAMES, start=1):
        sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=seed).items()}
        pol[nm] = dict(lora={k: (v * B_SCALE if ".lora_B." in k else v).to(BF).float() for k, v in sd.items() if ".lora_" in k},
                       head=modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head.")),
                       pp=modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=_sub(sd, "proprio_projector.")))
    g = torch.Generator().manual_seed(3)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    pv = torch.randn(len(LENS), 12, 56, 56, generator=g).to(BF).float()
    proprio = (torch.rand(len(LENS), 8, generator=g) * 2 - 1).to(BF).float().numpy()
    w = dict(modeling=modeling, cfg=cfg, ocfg=ocfg, base=base, pol=pol, prompts=prompts, pv=pv, proprio=proprio, dev=dev, alone={})

    def fresh(names=(), resident=None):
        vla = modeling.OpenVLAForActionPrediction(cfg, base, device=dev, norm_stats=IDENT)
        if resident is not None:
            vla.enable_policy_pool(resident)
        for nm in names:
            vla.add_policy(nm, pol[nm]["lora"], action_head=pol[nm]["head"], proprio_projector=pol[nm]["pp"], norm_stats=STATS[nm])
        return vla

    w["fresh"] = fresh
    w["pool"] = fresh(NAMES, resident=4)
    return w


def _run(w, vla, idx, policy):
    """predict_action_batch on the samples idx (in that order) with policy[k] for idx[k] -> [(actions, hidden)] in that order."""
    idx = list(idx)
    a, h = vla.predict_action_batch([(w["prompts"][i], None) for i in idx], w["pv"][idx], unnorm_key=UNNORM, proprio=w["proprio"][idx], policy=list(policy))
    assert a.shape == (len(idx), 8, 7) and h.shape == (len(idx), 56, w["cfg"].llm_dim)
    return [(a[k], h[k].clone()) for k in range(len(idx))]


def _alone(w, nm, i):
    """Observation i under policy nm, run alone (B = 1) on the shared pool model; computed once."""
    if (nm, i) not in w["alone"]:
        w["alone"][(nm, i)] = _run(w, w["pool"], [i], [nm])[0]
    return w["alone"][(nm, i)]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and torch.equal(got[1], want[1])


def _assign(batch):
    """Five observations over the four policies of a batch: observation k takes policy k % 4."""
    return [batch[k % 4] for k in range(len(LENS))]


def test_pool_equals_direct_registration(world):
    w, vla, idx = world, world["pool"], list(range(len(LENS)))
    assert vla.policies == NAMES and vla.engine.n_slots == 4 and vla.policy_pool_bytes > 0
    for members in ("xyzu", "vwxy"):
        direct = w["fresh"](members)
        assert direct.engine.n_slots == 4 and direct.engine.pool is None
        for assign in (_assign(members), _assign(members[::-1])):
            want = _run(w, direct, idx, assign)
            got = _run(w, vla, idx, assign)
            check = [k for k in idx if members == "xyzu" or assign[k] in "vw"]
            assert check
            for k in check:
                assert _same(got[k], want[k]), f"sample {k} under {assign[k]}: pool != add_policy{tuple(members)}"
                assert _same(_alone(w, assign[k], k), want[k]), f"sample {k} under {assign[k]}: alone on the pool != add_policy{tuple(members)}"
        del direct
    # other neighbours, other slots: v and w beside z and u, after a batch that moved everything
    _run(w, vla, idx, _assign("wzvu"))
    got = _run(w, vla, idx, _assign("uvzw"))
    for k in idx:
        assert _same(got[k], _alone(w, _assign("uvzw")[k], k))
    # the un-normalisation is each policy's own: x and y differ in their statistics
    ax, ay = _alone(w, "x", 0), _alone(w, "y", 0)
    assert not np.array_equal(ax[0], ay[0]) and not torch.equal(ax[1], ay[1])


def _rotate(w, vla):
    """The four batches of ROTATION on all five observations -> results per batch, the load_slot calls per batch, and the planner's own count."""
    eng = vla.engine
    shadow, before = copy.deepcopy(eng.pool_state), dict(vla.policy_pool_stats)
    calls, real = [], eng.load_slot
    eng.load_slot = lambda s, nm: (calls.append((s, nm)), real(s, nm))[1]
    results, per_batch, expected = [], [], 0
    try:
        for batch in ROTATION:
            resident_before = list(eng.pool_state.names)
            needed = list(dict.fromkeys(_assign(batch)))
            plan = shadow.plan(needed)
            shadow.commit(plan, needed)
            expected += len(plan)
            n0 = len(calls)
            results.append(_run(w, vla, range(len(LENS)), _assign(batch)))
            per_batch.append(calls[n0:])
            assert calls[n0:] == plan, "the loads are the planner's"
            assert not any(nm in resident_before for _, nm in calls[n0:]), "a resident policy was reloaded"
            assert all(eng.pool_state.names[s] == resident_before[s] for s in range(4) if resident_before[s] in needed), "a needed resident moved"
    finally:
        del eng.load_slot   # the instance attribute that shadowed the method
    after = vla.policy_pool_stats
    assert after["loads"] - before["loads"] == expected == len(calls)
    assert after["passes"] - before["passes"] == len(ROTATION)
    assert after["hits"] - before["hits"] == 4 * len(ROTATION) - expected
    return results, per_batch


def test_rotation(world):
    w = world
    vla = w["fresh"](NAMES, resident=4)
    results, per_batch = _rotate(w, vla)
    assert [len(c) for c in per_batch] == [4, 2, 2, 2], "from empty slots: four loads, then the two newcomers of each batch"
    assert vla.policy_pool_stats == dict(loads=10, hits=6, passes=4)
    for batch, res in zip(ROTATION, results):
        for k, nm in enumerate(_assign(batch)):
            assert _same(res[k], _alone(w, nm, k)), f"batch {batch}: sample {k} under {nm} differs from its answer alone"


def test_graph_replay(world):
    w, vla = world, world["pool"]
    vla.enable_graph_replay(True)
    try:
        results, _ = _rotate(w, vla)
        graphs = [g for k, g in vla._graphs.items() if "policies" in k]
        assert len(graphs) == 1 and graphs[0].captures == 1, "one captured graph for the (B, L) used"
        again, _ = _rotate(w, vla)
        assert [g for k, g in vla._graphs.items() if "policies" in k] == graphs and graphs[0].captures == 1, "swaps never recapture"
    finally:
        vla.enable_graph_replay(False)
    for batch, res, res2 in zip(ROTATION, results, again):
        for k, nm in enumerate(_assign(batch)):
            assert _same(res[k], _alone(w, nm, k)) and _same(res2[k], _alone(w, nm, k)), f"batch {batch}: replay of sample {k} under {nm} != eager"


def test_splitting(world):
    w, vla = world, world["pool"]
    idx, policy = [0, 1, 2, 3, 4, 0, 1], ["x", "y", "z", "u", "v", "w", "x"]
    before = vla.policy_pool_stats
    got = _run(w, vla, idx, policy)
    assert vla.policy_pool_stats["passes"] - before["passes"] == 2, "six distinct policies at four slots: two passes"
    for k, (i, nm) in enumerate(zip(idx, policy)):
        assert _same(got[k], _alone(w, nm, i)), f"row {k} (sample {i} under {nm}) differs from its answer alone"
    # pad_to repeats observation 0 with its policy: no further policy, the same bits
    padded = vla.predict_action_batch([(w["prompts"][i], None) for i in idx[:3]], w["pv"][idx[:3]], unnorm_key=UNNORM, proprio=w["proprio"][idx[:3]],
                                      policy=policy[:3], pad_to=4)
    for k in range(3):
        assert _same((padded[0][k], padded[1][k]), got[k])


def test_removal_and_replacement(world):
    w = world
    vla = w["fresh"](("x", "y"), resident=4)   # four slots, as the shared pool model: outputs are reproducible per (policy, resident)
    idx = [0, 1, 2]
    x0 = _run(w, vla, idx, ["x"] * 3)
    y0 = _run(w, vla, idx, ["y"] * 3)
    assert all(_same(x0[k], _alone(w, "x", i)) for k, i in enumerate(idx)) and not _same(x0[0], y0[0])
    assert "x" in vla.engine.pool_state.names
    vla.remove_policy("x")
    assert vla.policies == ("y",) and "x" not in vla.engine.pool_state.names
    with pytest.raises(ValueError, match="unknown policy"):
        _run(w, vla, idx, ["x"] * 3)
    with pytest.raises(ValueError, match="unknown policy"):
        vla.remove_policy("x")
    p = w["pol"]["y"]
    loads = vla.policy_pool_stats["loads"]
    vla.add_policy("x", p["lora"], action_head=p["head"], proprio_projector=p["pp"], norm_stats=STATS["y"])   # the name x, y's tensors
    x1 = _run(w, vla, idx, ["x", "y", "x"])
    assert vla.policy_pool_stats["loads"] == loads + 1, "the re-registered name is loaded afresh, never served from its stale slot"
    for k in range(3):
        assert _same(x1[k], y0[k]), "rows routed to the re-registered x carry y's bits"
    with pytest.raises(ValueError, match="policy pool"):
        w["fresh"](("x",)).remove_policy("x")


def test_refusals(world):
    w = world
    modeling, cfg, dev, pol = w["modeling"], w["cfg"], w["dev"], w["pol"]
    add = lambda vla, nm, **kw: vla.add_policy(nm, pol[nm]["lora"], **{**dict(action_head=pol[nm]["head"], proprio_projector=pol[nm]["pp"]), **kw})  # noqa: E731
    vla = w["fresh"](("x",))
    with pytest.raises(ValueError, match="before the first add_policy"):
        vla.enable_policy_pool(4)
    for nm in ("y", "z", "u"):
        add(vla, nm)
    with pytest.raises(ValueError, match="at most"):
        add(vla, "v")
    assert vla.policies == ("x", "y", "z", "u") and vla.policy_pool_bytes == 0
    pooled = w["fresh"]()
    for bad in (0, 5, -1, 2.0, True):
        with pytest.raises(ValueError, match="resident"):
            pooled.enable_policy_pool(bad)
    assert pooled.enable_policy_pool(2) is pooled and pooled.policy_pool_stats == dict(loads=0, hits=0, passes=0)
    with pytest.raises(ValueError, match="already"):
        pooled.enable_policy_pool(2)
    add(pooled, "x")
    with pytest.raises(ValueError, match="before the first add_policy"):
        pooled.enable_policy_pool(2)
    with pytest.raises(ValueError, match="other shapes"):
        add(pooled, "y", action_head=modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 6, device=dev))
    sdd = {k: v.to(BF).float() for k, v in vo.random_state_dict(w["ocfg"], seed=1, diffusion=True).items()}
    dhead = modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=4, device=dev, state_dict=_sub(sdd, "action_head."))
    with pytest.raises(ValueError, match="diffusion"):
        add(pooled, "y", action_head=dhead)
    with pytest.raises(ValueError, match="either every policy"):
        add(pooled, "y", action_head=None)
    half = {k: (v[:16] if ".lora_A." in k else v[:, :16]).contiguous() for k, v in pol["y"]["lora"].items()}
    with pytest.raises(ValueError, match="rank"):
        pooled.add_policy("y", half, action_head=pol["y"]["head"], proprio_projector=pol["y"]["pp"])
    with pytest.raises(ValueError, match="lora_alpha"):
        add(pooled, "y", lora_alpha=32)
    fewer = {k: v for k, v in pol["y"]["lora"].items() if "projector.fc3" not in k}
    with pytest.raises(ValueError, match="different sets"):
        pooled.add_policy("y", fewer, action_head=pol["y"]["head"], proprio_projector=pol["y"]["pp"])
    assert pooled.policies == ("x",) and list(pooled.engine.pool) == ["x"], "a refused policy changes nothing"
    for nm in ("y", "z", "u", "v", "w"):   # and no limit on the number
        add(pooled, nm)
    assert pooled.policies == NAMES and pooled.engine.n_slots == 2


def test_server_with_a_pool_of_two(world):
    dep = load("openvla-oft_amd.vla_scripts.deploy")
    utils = load("openvla-oft_amd.experiments.robot.openvla_utils")
    w = world

    class P56(utils.PrismaticProcessor):   # the tiny test towers take 56 x 56 inputs
        def __call__(self, text, image):
            out = super().__call__(text, image)
            out["pixel_values"] = out["pixel_values"][:, :, ::4, ::4].contiguous()
            return out

    proc = P56(lambda text: [1] + [3 + (ord(c) % 200) for c in text][:20])
    rng = np.random.default_rng(4)
    obs = [{"full_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), "wrist_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
            "state": rng.uniform(-1, 1, 8), "instruction": t} for t in ("pick up the black bowl", "open the drawer")]
    specs = {nm: dict(lora_state_dict=w["pol"][nm]["lora"], action_head=w["pol"][nm]["head"], proprio_projector=w["pol"][nm]["pp"], norm_stats=STATS[nm])
             for nm in NAMES}
    vla = w["fresh"]()
    kw = dict(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=UNNORM, num_open_loop_steps=8)
    payloads = [dep._encode({**obs[k % 2], "policy": nm}) for k, nm in enumerate(NAMES + NAMES[::-1])]
    seen = []
    try:
        server = dep.OpenVLAServer(dep.DeployConfig(coalesce_ms=300.0, max_batch=4, batch_buckets=(4,), resident_policies=2, **kw), vla=vla, processor=proc,
                                   policies=specs)
        assert vla.policies == NAMES and vla.engine.n_slots == 2 and server._coalescer.max_keys == 2
        run_batch = server._run_batch

        def counting(items, pad_to):
            seen.append([o["policy"] for o, _ in items])
            return run_batch(items, pad_to)

        server._coalescer.batch_fn = counting
        got, gate = {}, threading.Barrier(len(payloads))

        def client(i):
            gate.wait()
            got[i] = server.act(payloads[i])

        threads = [threading.Thread(target=client, args=(i,)) for i in range(len(payloads))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads)
        n_coalesced = len(seen)
        want = [server.act_batch([p])[0] for p in payloads]
        group = server.act_batch(payloads[:6])     # six policies in one pre-formed group: split into passes by the model
        assert server.act(dep._encode({**obs[0], "policy": "nobody"})) == "error"
        server.close()
    finally:
        vla.enable_graph_replay(False)
    assert sorted(nm for b in seen[:n_coalesced] for nm in b) == sorted(NAMES + NAMES) and n_coalesced < len(payloads), "the requests were coalesced"
    assert all(len(set(b)) <= 2 for b in seen[:n_coalesced]), f"a coalesced forward saw more than two distinct policies: {seen[:n_coalesced]}"
    for i, p in enumerate(payloads):
        assert isinstance(got[i], list) and len(got[i]) == 8 and isinstance(want[i], list)
        for a, b in zip(got[i], want[i]):
            assert np.array_equal(dep._decode(a), dep._decode(b)), f"client {i}: coalesced /act != /act_batch([payload])"
    for i in range(6):
        for a, b in zip(group[i], want[i]):
            assert np.array_equal(dep._decode(a), dep._decode(b)), f"/act_batch of six policies: element {i} != /act_batch([payload])"
    assert not np.array_equal(dep._decode(want[0][0]), dep._decode(want[2][0])), "the policy name decides the answer"
