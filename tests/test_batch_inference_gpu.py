"""Batched action-chunk inference (OpenVLAForActionPrediction.predict_action_batch, get_vla_action_batch, /act_batch) and the fixed GEMM
schedules behind it (ovla_gemm_bf16_fixed): every observation's outputs are the same bits whatever else is in the batch."""
import importlib
import types

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
UNNORM = "libero_spatial_no_noops"
LENS = [7, 12, 9, 15, 7]


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)   # wide enough that the planner's schedules differ between batch 1 and 5
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    sdd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0, diffusion=True).items()}   # the diffusion head + noisy-action projector
    cfg = config_mod.VLAConfig.from_any(ocfg)
    stats = {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 1], "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]},
                      "proprio": {"q01": [-2.0] * 8, "q99": [2.0] * 8, "min": [-3.0] * 8, "max": [3.0] * 8}}}
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats=stats)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head."))
    dhead = modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=4, device=dev, state_dict=_sub(sdd, "action_head."))
    pp = modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict={"module." + k: v for k, v in _sub(sd, "proprio_projector.").items()})
    nap = modeling.NoisyActionProjector(cfg.llm_dim, device=dev, state_dict=_sub(sdd, "noisy_action_projector."))
    g = torch.Generator().manual_seed(3)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    B = len(LENS)
    pv = torch.randn(B, 12, 56, 56, generator=g).to(BF).float()
    proprio = (torch.rand(B, 8, generator=g) * 2 - 1).to(BF).float().numpy()
    noise = torch.randn(B, 8, 7, generator=g).to(BF).float()
    return dict(vla=vla, head=head, dhead=dhead, pp=pp, nap=nap, cfg=cfg, ocfg=ocfg, sd=sd, stats=stats, prompts=prompts, pv=pv, proprio=proprio,
                noise=noise, modeling=modeling)


def _batch(w, idx, kind):
    """predict_action_batch on the samples `idx` (in that order) -> per-sample (actions, hidden) keyed by sample index."""
    vla = w["vla"]
    prompts = [(w["prompts"][i], torch.ones(len(w["prompts"][i]), dtype=torch.bool)) for i in idx]
    pv = w["pv"][list(idx)]
    if kind == "l1":
        a, h = vla.predict_action_batch(prompts, pv, unnorm_key=UNNORM, proprio=w["proprio"][list(idx)], proprio_projector=w["pp"], action_head=w["head"])
    elif kind == "discrete":
        a, h = vla.predict_action_batch(prompts, pv, unnorm_key=UNNORM)
    else:
        a, h = vla.predict_action_batch(prompts, pv, unnorm_key=UNNORM, proprio=w["proprio"][list(idx)], proprio_projector=w["pp"],
                                        action_head=w["dhead"], noisy_action_projector=w["nap"], noise=w["noise"][list(idx)])
    assert a.shape == (len(idx), 8, 7) and h.shape == (len(idx), 56, w["cfg"].llm_dim)
    return {i: (a[k], h[k].clone()) for k, i in enumerate(idx)}


@pytest.mark.parametrize("kind", ["l1", "discrete", "diffusion"])
def test_batched_outputs_do_not_depend_on_the_batch(world, kind):
    B = len(LENS)
    full = _batch(world, list(range(B)), kind)
    rev = _batch(world, list(reversed(range(B))), kind)
    for i in range(B):
        alone = _batch(world, [i], kind)[i]
        for other in (rev[i], alone):
            assert np.array_equal(full[i][0], other[0]), f"sample {i}: actions differ across batch compositions"
            assert torch.equal(full[i][1], other[1]), f"sample {i}: action hidden states differ across batch compositions"
        if kind == "discrete":   # the token ids behind the bins, too
            tok = lambda h: world["vla"].logits_for(h).argmax(1)  # noqa: E731
            assert torch.equal(tok(full[i][1]), tok(alone[1]))


def test_the_planner_alone_would_not_be_invariant(world):
    """At these sizes the planner's own schedule differs between batch 1 and batch 5 for some decoder GEMM: invariance above is the fixed
    schedule's doing, and the fixed schedule is one per problem class (host-only query, no M in it)."""
    ops, cfg = load("openvla-oft_amd.ops"), world["cfg"]
    D, F = cfg.llm_dim, cfg.llm_ff
    P = 2 * cfg.dino.n_patches + 1
    bucket = lambda n: (n + 1 + 56 + 1 + 7) // 8 * 8  # noqa: E731
    M1, M5 = P + bucket(LENS[0]), len(LENS) * (P + bucket(max(LENS)))
    shapes = [(3 * D, D), (D, D), (2 * F, D), (D, F)]
    plan = lambda M, n, k: (lambda p: (p[0], p[2] > 0, p[3]))(ops.gemm_plan(M, n, k))  # noqa: E731  (tile, K-split remainder?, splits)
    differ = [(n, k) for n, k in shapes if plan(M1, n, k) != plan(M5, n, k)]
    assert differ
    for n, k in differ:   # one fixed schedule, so it differs from the planner's choice at batch 1 or at batch 5
        tile, splits = ops.gemm_fixed_schedule(n, k)
        assert (tile, splits > 1, splits) != plan(M1, n, k) or (tile, splits > 1, splits) != plan(M5, n, k)
    first = [ops.gemm_fixed_schedule(n, k) for n, k in shapes]
    ops._fixed_cache.clear()   # a fresh query (no cached value) gives the same schedules
    assert [ops.gemm_fixed_schedule(n, k) for n, k in shapes] == first


@pytest.fixture(scope="module")
def small(dev):
    """The standard tiny model (tests/test_api_gpu.py's): where test_predict_action_l1_and_discrete's absolute bounds against the oracle hold."""
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    sdd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=1, diffusion=True).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    stats = {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 1], "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    w = dict(cfg=cfg, ocfg=ocfg, sd=sd, sdd=sdd, stats=stats, vla=modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats=stats),
             vla_d=modeling.OpenVLAForActionPrediction(cfg, sdd, device=dev, norm_stats=stats),
             head=modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head.")),
             dhead=modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=5, device=dev, state_dict=_sub(sdd, "action_head.")),
             pp=modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict={"module." + k: v for k, v in _sub(sd, "proprio_projector.").items()}),
             pp_d=modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=_sub(sdd, "proprio_projector.")),
             nap=modeling.NoisyActionProjector(cfg.llm_dim, device=dev, state_dict=_sub(sdd, "noisy_action_projector.")))
    g = torch.Generator().manual_seed(5)
    w["prompts"] = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    w["pv"] = torch.randn(len(LENS), 12, 56, 56, generator=g).to(BF).float()
    w["proprio"] = (torch.rand(len(LENS), 8, generator=g) * 2 - 1).to(BF).float().numpy()
    w["noise"] = torch.randn(len(LENS), 8, 7, generator=g).to(BF).float()
    return w


def test_batched_matches_predict_action_and_oracle(small):
    """Every sample of a mixed-length batch, every head: within test_predict_action_l1_and_discrete's absolute 5e-2 of the bf16-emulating oracle
    (L1) and of predict_action on the same observation; discrete tokens as in that test; the DDIM trajectory within test_ddim_sampling_matches_oracle's
    8e-2 of predict_action with the same noise.  A masking, row-offset or timestep-embedding bug is an O(1) error."""
    w, B = small, len(LENS)
    prompts = [(p, None) for p in w["prompts"]]
    one = lambda vla, i, **kw: vla.predict_action(input_ids=w["prompts"][i][None], attention_mask=torch.ones(1, len(w["prompts"][i]), dtype=torch.bool),  # noqa: E731
                                                   pixel_values=w["pv"][i: i + 1], unnorm_key=UNNORM, **kw)
    o16 = vo.Oracle(w["ocfg"], w["sd"], mode="bf16")
    act, hid = w["vla"].predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, proprio=w["proprio"], proprio_projector=w["pp"], action_head=w["head"])
    act_d, hid_d = w["vla"].predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM)
    act_n, _ = w["vla_d"].predict_action_batch(prompts, w["pv"], unnorm_key=UNNORM, proprio=w["proprio"], proprio_projector=w["pp_d"], action_head=w["dhead"],
                                               noisy_action_projector=w["nap"], noise=w["noise"])
    for i in range(B):
        ids = w["prompts"][i][None]
        ref, _ = o16.predict_action(ids, torch.ones_like(ids, dtype=torch.bool), w["pv"][i: i + 1], proprio=w["proprio"][i],
                                    unnorm_stats=w["stats"][UNNORM]["action"])
        a1, _ = one(w["vla"], i, proprio=w["proprio"][i], proprio_projector=w["pp"], action_head=w["head"])
        print(f"sample {i}: L1 Linf vs oracle {np.abs(act[i] - ref).max():.3e}, vs predict_action {np.abs(act[i] - a1).max():.3e}")
        assert np.abs(act[i] - ref).max() < 5e-2 and np.abs(act[i] - a1).max() < 5e-2
        # discrete: argmax token ids of the action rows and the decoded bins, against predict_action's (token path)
        ad1, hd1 = one(w["vla"], i)
        tok, tok1 = w["vla"].logits_for(hid_d[i]).argmax(1), w["vla"].logits_for(hd1[0]).argmax(1)
        assert (tok == tok1).float().mean().item() >= 0.9
        agree = (tok == tok1).cpu().numpy().reshape(8, 7)
        assert np.array_equal(act_d[i][agree], ad1[agree]), "equal tokens decode to equal bins"
        an1, _ = one(w["vla_d"], i, proprio=w["proprio"][i], proprio_projector=w["pp_d"], action_head=w["dhead"], noisy_action_projector=w["nap"],
                     noise=w["noise"][i: i + 1])
        print(f"sample {i}: 5-step DDIM Linf vs predict_action {np.abs(act_n[i] - an1).max():.3e}")
        assert np.abs(act_n[i] - an1).max() < 8e-2


@pytest.fixture(scope="module")
def merged(world, dev):
    """world's model with its adapters merged: the RMSNorm-folded decoder (merge_and_unload folds the norms into the projections)."""
    w = dict(world)
    w["vla"] = world["modeling"].OpenVLAForActionPrediction(world["cfg"], world["sd"], device=dev, norm_stats=world["stats"]).merge_and_unload()
    return w


@pytest.mark.parametrize("kind", ["l1", "discrete"])
def test_merged_folded_decoder_is_invariant(merged, kind):
    """The folded path (rowscale / rowsq / RoPE / SwiGLU epilogues on fixed schedules, shared fold buffers across layers) is bit-invariant too,
    including a batch of 10 whose M = B * S is beyond 1024, where the planner's schedules would drop the fold."""
    llm = merged["vla"].engine.llm
    assert getattr(llm, "folded", False) and llm._fold_fixed_ok() and llm._swiglu_fixed
    B = len(LENS)
    full = _batch(merged, list(range(B)), kind)
    rev = _batch(merged, list(reversed(range(B))), kind)
    big = _batch_dup(merged, list(range(B)) * 2, kind)   # M = 10 * (33 patch / proprio rows + an 80-token bucket) = 1130 rows
    for i in range(B):
        alone = _batch(merged, [i], kind)[i]
        for other in (rev[i], alone, big[i], big[i + B]):
            assert np.array_equal(full[i][0], other[0]) and torch.equal(full[i][1], other[1]), f"sample {i}"


def _batch_dup(w, idx, kind):
    """Like _batch, for an index list with repeats: results keyed by position in `idx`."""
    vla, prompts = w["vla"], [(w["prompts"][i], None) for i in idx]
    if kind == "l1":
        a, h = vla.predict_action_batch(prompts, w["pv"][idx], unnorm_key=UNNORM, proprio=w["proprio"][idx], proprio_projector=w["pp"], action_head=w["head"])
    else:
        a, h = vla.predict_action_batch(prompts, w["pv"][idx], unnorm_key=UNNORM)
    return {k: (a[k], h[k].clone()) for k in range(len(idx))}


def test_batched_graph_replay_equals_eager(world):
    vla, w = world["vla"], world
    idx = [0, 1, 2, 3, 4]
    eager = _batch(w, idx, "l1")
    vla.enable_graph_replay(True)
    try:
        graph = _batch(w, idx, "l1")
        pv0 = w["pv"]
        w["pv"] = (pv0 + 0.25 * torch.randn(pv0.shape, generator=torch.Generator().manual_seed(1))).to(BF).float()
        graph2 = _batch(w, idx, "l1")
        vla.enable_graph_replay(False)
        eager2 = _batch(w, idx, "l1")
        w["pv"] = pv0
    finally:
        vla.enable_graph_replay(False)
    for i in idx:
        assert np.array_equal(eager[i][0], graph[i][0]) and torch.equal(eager[i][1], graph[i][1])
        assert np.array_equal(eager2[i][0], graph2[i][0]) and torch.equal(eager2[i][1], graph2[i][1])
        assert not np.array_equal(eager[i][0], eager2[i][0])


def _glue(world):
    utils = load("openvla-oft_amd.experiments.robot.openvla_utils")

    class P56(utils.PrismaticProcessor):   # the tiny test towers take 56 x 56 inputs
        def __call__(self, text, image):
            out = super().__call__(text, image)
            out["pixel_values"] = out["pixel_values"][:, :, ::4, ::4].contiguous()
            return out

    tok = lambda text: [1] + [3 + (ord(c) % 200) for c in text][:20]  # noqa: E731
    rng = np.random.default_rng(4)
    obs = [{"full_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), "wrist_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
            "state": rng.uniform(-1, 1, 8), "instruction": t} for t in ("pick up the black bowl", "open the drawer", "put the cup on the plate")]
    return utils, P56(tok), obs


def test_get_vla_action_batch_and_act_batch(world):
    from fastapi.testclient import TestClient

    dep = load("openvla-oft_amd.vla_scripts.deploy")
    utils, proc, obs = _glue(world)
    vla, head, pp = world["vla"], world["head"], world["pp"]
    cfg = types.SimpleNamespace(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=UNNORM, num_open_loop_steps=8)
    mine = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o.items()} for o in obs]
    got = utils.get_vla_action_batch(cfg, vla, proc, mine, [o["instruction"] for o in obs], action_head=head, proprio_projector=pp)
    assert len(got) == 3 and all(len(g) == 8 for g in got)
    norm = [utils.normalize_proprio(o["state"], vla.norm_stats[UNNORM]["proprio"]) for o in obs]
    for o, n in zip(mine, norm):
        assert np.array_equal(o["state"], n), "obs['state'] is normalised in place"
    # the batched eager call on the same inputs
    prompts, pvs = [], []
    for o in obs:
        p = f"In: What action should the robot take to {o['instruction'].lower()}?\nOut:"
        ims = utils.prepare_images_for_vla([o["full_image"], o["wrist_image"]], cfg)
        inp = proc(p, ims[0])
        prompts.append((inp["input_ids"], inp["attention_mask"]))
        pvs.append(torch.cat([inp["pixel_values"], proc(p, ims[1])["pixel_values"]], 1))
    ref, _ = vla.predict_action_batch(prompts, torch.cat(pvs), unnorm_key=UNNORM, proprio=np.stack(norm), proprio_projector=pp, action_head=head)
    for g, r in zip(got, ref):
        assert all(np.array_equal(a, b) for a, b in zip(g, r))
    dcfg = dep.DeployConfig(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=UNNORM, num_open_loop_steps=8)
    server = dep.OpenVLAServer(dcfg, vla=vla, processor=proc, action_head=head, proprio_projector=pp)   # (graph replay on)
    try:
        client = TestClient(server.build_app())
        r = client.post("/act_batch", json=[dep._encode(o) for o in obs])
        assert r.status_code == 200
        chunks = [dep._decode(c) for c in r.json()]
        assert len(chunks) == 3
        for c, g in zip(chunks, got):
            assert len(c) == 8 and all(np.array_equal(a, b) for a, b in zip(c, g)), "/act_batch == get_vla_action_batch (graph == eager)"
        assert client.post("/act_batch", json=[dep._encode(obs[0]), {"instruction": "no images"}]).json() == "error"
        assert client.post("/act_batch", json=[]).json() == "error"
    finally:
        vla.enable_graph_replay(False)


def test_film_batched_is_invariant(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=4, film=True).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    stats = {"d": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats=stats, use_film=True)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head."))
    g = torch.Generator().manual_seed(6)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in (6, 14, 10)]
    pv = torch.randn(3, 12, 56, 56, generator=g).to(BF).float()

    def run(idx):
        a, h = vla.predict_action_batch([(prompts[i], None) for i in idx], pv[idx], unnorm_key="d", action_head=head, use_film=True)
        return {i: (a[k], h[k].clone()) for k, i in enumerate(idx)}

    full, rev = run([0, 1, 2]), run([2, 1, 0])
    for i in range(3):
        alone = run([i])[i]
        for other in (rev[i], alone):
            assert np.array_equal(full[i][0], other[0]) and torch.equal(full[i][1], other[1])
        one, _ = vla.predict_action(input_ids=prompts[i][None], attention_mask=torch.ones(1, len(prompts[i]), dtype=torch.bool), pixel_values=pv[i: i + 1],
                                    unnorm_key="d", action_head=head, use_film=True)
        assert np.abs(one - full[i][0]).max() < 5e-2


# ---- kernel level: the fixed schedule at M = 608, 1216, 4864 -------------------------------------------------------------------------------
def _fp32_reference(a, W, kind, kw):
    """The epilogue in fp32 torch on the fp32 product (independent of the library): what the bf16 result must approximate."""
    F_ = torch.nn.functional
    acc = a.float() @ W.float().t()
    M, N = acc.shape
    if "rowscale" in kw:
        parts, eps, _ = kw["rowscale"]
        acc = acc * torch.rsqrt(parts.sum(1, keepdim=True) / a.shape[1] + eps)
    if kind in ("plain",):
        return acc, None
    if kind == "residual_rowsq":
        return acc + kw["residual"].float(), None
    if kind == "rope_fold":
        cos, sin, S, cols = kw["rope"]
        pos = torch.arange(M, device=a.device) % S
        c2, s2 = torch.cat([cos.float()[pos]] * 2, 1)[:, None], torch.cat([sin.float()[pos]] * 2, 1)[:, None]
        x = acc[:, :cols].reshape(M, cols // 128, 128)
        rot = torch.cat([-x[..., 64:], x[..., :64]], -1)
        return torch.cat([(x * c2 + rot * s2).reshape(M, cols), acc[:, cols:]], 1), None
    if kind == "swiglu_fold":
        return F_.silu(acc[:, : N // 2]) * acc[:, N // 2:], None
    z = acc + kw["bias"].float()
    if kind == "gelu_layerscale":
        return F_.gelu(z) * kw["colscale"].float(), None
    if kind == "relu_residual":
        return F_.relu(z) + kw["residual"].float(), None
    if kind == "relu_cpre":
        return F_.relu(z), z
    raise AssertionError(kind)


def _rows_case(dev, N, K, kind):
    ops = load("openvla-oft_amd.ops")
    g = torch.Generator(device=dev).manual_seed(N + K)
    Mmax = 4864
    A = (torch.randn(Mmax, K, device=dev, generator=g) * 0.5).to(BF)
    W = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(BF)
    bias, cs = torch.randn(N, device=dev, generator=g).to(BF), torch.rand(N, device=dev, generator=g).to(BF)
    outs = []
    for M in (608, 1216, 4864):
        a = A[:M]
        kw = {}
        if kind == "residual_rowsq":
            kw = dict(residual=(A[:M, :N] if K >= N else torch.ones((M, N), dtype=BF, device=dev)),
                      rowsq_out=torch.empty((M, N // 64), dtype=torch.float32, device=dev))
        elif kind == "rope_fold":
            cos, sin = ops.rope_table(608, 128, 10000.0, dev)
            kw = dict(rope=(cos, sin, 608, 2 * (N // 3)), rowscale=(ops.row_sumsq(a), 1e-6, torch.empty(M, dtype=torch.float32, device=dev)))
        elif kind == "swiglu_fold":
            kw = dict(act=ops.ACT_SWIGLU, rowscale=(ops.row_sumsq(a), 1e-6, torch.empty(M, dtype=torch.float32, device=dev)))
        elif kind == "gelu_layerscale":
            kw = dict(bias=bias, act=ops.ACT_GELU, colscale=cs)
        elif kind == "relu_residual":
            kw = dict(bias=bias, act=ops.ACT_RELU, residual=torch.ones((M, N), dtype=BF, device=dev))
        elif kind == "relu_cpre":   # the action head's fc1 (ReLU, the pre-activation kept)
            kw = dict(bias=bias, act=ops.ACT_RELU, c_pre=torch.empty((M, N), dtype=BF, device=dev))
        with ops.batch_invariant():
            c = ops.gemm(a, W, **kw)
        extra = kw.get("rowsq_out", kw.get("c_pre"))
        outs.append((c[:608].clone(), None if extra is None else extra[:608].clone()))
        ref, ref_pre = _fp32_reference(a, W, kind, kw)
        tol = 2e-2 * ref.abs().max().item() + 2e-2
        err = (c.float() - ref).abs().max().item()
        assert err <= tol, (N, K, kind, M, err, tol)
        if ref_pre is not None:
            assert (kw["c_pre"].float() - ref_pre).abs().max().item() <= 2e-2 * ref_pre.abs().max().item() + 2e-2
        if kind == "residual_rowsq":   # the producer-side sums of squares are those of the bf16 output row, per 64-column group
            sq = (c.float() ** 2).view(M, N // 64, 64).sum(-1)
            assert torch.allclose(kw["rowsq_out"], sq, rtol=1e-4, atol=1e-4)
    for c, e in outs[1:]:
        assert torch.equal(c, outs[0][0]), (N, K, kind)
        if e is not None:
            assert torch.equal(e, outs[0][1]), (N, K, kind)


@pytest.mark.parametrize("N,K,kind", [
    (12288, 4096, "rope_fold"), (4096, 4096, "residual_rowsq"), (22016, 4096, "swiglu_fold"), (4096, 11008, "residual_rowsq"),
    (4096, 4096, "plain"), (32064, 4096, "plain"), (4352, 1024, "gelu_layerscale"), (1152, 4608, "gelu_layerscale"), (4096, 4096, "relu_residual"),
    (4096, 28672, "relu_cpre"), (768, 256, "plain"), (512, 256, "relu_residual")])
def test_fixed_schedule_rows_do_not_depend_on_m(dev, N, K, kind):
    _rows_case(dev, N, K, kind)


def test_device_pixel_values_batch_layout(dev):
    """The device image path of get_vla_action_batch: all B * I frames in one pass, row b == device_pixel_values of observation b alone."""
    utils = load("openvla-oft_amd.experiments.robot.openvla_utils")
    rng = np.random.default_rng(8)
    per_obs = [[rng.integers(0, 256, (224, 224, 3), dtype=np.uint8) for _ in range(2)] for _ in range(3)]
    cfg = types.SimpleNamespace(center_crop=True)
    got = utils.device_pixel_values_batch(per_obs, cfg)
    assert got.shape == (3, 12, 224, 224)
    for b, images in enumerate(per_obs):
        assert torch.equal(got[b], utils.device_pixel_values(images, cfg)[0])
