"""Multi-adapter serving: several fine-tuned policies (LoRA adapters + L1 head + proprio projector + statistics) on one base model, mixed in
one batched forward by predict_action_batch(policy=[...]).  Routing is device data: a row's bits depend on its own adapter and on the slot
count only, one captured graph serves every assignment.  The CPU tests (no `gpu` mark) cover the slot layout and the fixed-schedule query."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo

BF = torch.bfloat16
load = importlib.import_module
UNNORM = "suite"
LENS = [7, 12, 9, 15, 7]
B_SCALE = 8.0   # lora_B of the random policies is scaled up so that two policies' actions differ far beyond the comparison tolerance
IDENT = {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
STATS_Y = {UNNORM: {"action": {"q01": [-2.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 3], "mask": [True] * 6 + [False]}}}


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


# ======================================================================================================================
# CPU
# ======================================================================================================================
def test_slot_layout_against_numpy():
    """A_slots / B_slots (engine.fill_slot, the layout LoraLinear.set_slot writes) against  y = x W^T + sum_s [slot = s] t_s B_s^T  in float64, for fused groups."""
    engine = load("openvla-oft_amd.engine")
    rng = np.random.default_rng(0)
    M, K, r, scale, rows_per_obs = 12, 24, 8, 0.5, 3
    for G, n in ((1, 1), (1, 2), (3, 2), (2, 4)):
        gn = 16
        W, x = rng.standard_normal((G * gn, K)), rng.standard_normal((M, K))
        As, Bs = [rng.standard_normal((G * r, K)) for _ in range(n)], [rng.standard_normal((G * gn, r)) for _ in range(n)]
        slots = rng.integers(0, n, M // rows_per_obs)
        A_slots, B_slots = torch.zeros(G * n * r, K, dtype=torch.float64), torch.zeros(G * gn, n * r, dtype=torch.float64)
        for s in range(n):                                                     # what LoraLinear.set_slot runs
            engine.fill_slot(A_slots, B_slots, s, torch.from_numpy(As[s]), torch.from_numpy(Bs[s]), G)
        A_slots, B_slots = A_slots.numpy(), B_slots.numpy()
        assert A_slots.shape == (G * n * r, K) and B_slots.shape == (G * gn, n * r)
        t = scale * x @ A_slots.T                                              # the projection GEMM
        for m in range(M):                                                     # ovla_lora_route
            for g in range(G):
                for s in range(n):
                    if s != slots[m // rows_per_obs]:
                        t[m, engine.slot_a_rows(g, s, n, r)] = 0.0
        got = np.concatenate([x @ W[g * gn:(g + 1) * gn].T + t[:, g * n * r:(g + 1) * n * r] @ B_slots[g * gn:(g + 1) * gn].T for g in range(G)], 1)   # K-extension, k2_group_n = gn
        want = np.empty_like(got)
        for m in range(M):
            s = slots[m // rows_per_obs]
            for g in range(G):
                ts = scale * x[m] @ As[s][g * r:(g + 1) * r].T
                want[m, g * gn:(g + 1) * gn] = x[m] @ W[g * gn:(g + 1) * gn].T + ts @ Bs[s][g * gn:(g + 1) * gn].T
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12)


def test_fixed_schedule_exists_for_every_slotted_class():
    """Host-only query: every decoder, tower and projector problem class of the tiny and the 7B configuration has a fixed schedule at the
    K-extension widths of 1 .. 4 slots (K2 = 32 n), with and without k2_group_n, on a tile configuration that accepts any K2 (not 18 / 22)."""
    import __graft_entry__ as g

    g._pkg()
    ops, config = load("openvla-oft_amd.ops"), load("openvla-oft_amd.config")
    for cfg in (config.VLAConfig.from_any(vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)), config.OPENVLA_7B):
        D, F, vis = cfg.llm_dim, cfg.llm_ff, cfg.vision_dim
        classes = [(3 * D, D, D, ops.EPI_ROPE), (D, D, 0, 0), (2 * F, D, F, 0), (D, F, 0, 0), (4 * vis, vis, 0, ops.EPI_GENERAL), (D, 4 * vis, 0, ops.EPI_GENERAL), (D, D, 0, 0)]
        for vc in (cfg.dino, cfg.siglip):
            d, m = vc.dim, vc.mlp_hidden
            classes += [(3 * d, d, 0, 0), (d, d, 0, ops.EPI_GENERAL), (d, d, 0, 0), (m, d, 0, ops.EPI_GENERAL), (d, m, 0, ops.EPI_GENERAL), (d, m, 0, 0)]
        for N, K, gn, epi in classes:
            for K2 in (32, 64, 96, 128):
                for kg in {gn, 0}:
                    tile, splits = ops.gemm_fixed_schedule(N, K, K2, kg, epi)
                    assert tile in (1, 2, 5, 17) or (tile == 18 and K2 <= 96), (N, K, K2, kg, epi, tile)
                    assert 1 <= splits <= 8
                assert ops.gemm_fixed_schedule(K2 * (3 if gn == D else 2 if gn else 1), K)[0] > 0      # the projection t = x A_slots^T


# ======================================================================================================================
# GPU
# ======================================================================================================================
def _policy_tensors(ocfg, seed):
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=seed).items()}
    lora = {k: (v * B_SCALE if ".lora_B." in k else v).to(BF).float() for k, v in sd.items() if ".lora_" in k}
    return dict(lora=lora, head_sd={k: v for k, v in sd.items() if k.startswith("action_head.")}, pp_sd={k: v for k, v in sd.items() if k.startswith("proprio_projector.")})


@pytest.fixture(scope="module")
def world(dev):
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)
    cfg = config_mod.VLAConfig.from_any(ocfg)
    base = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items() if ".lora_" not in k and not k.startswith(("action_head.", "proprio_projector."))}
    pol = {name: _policy_tensors(ocfg, seed) for name, seed in (("x", 1), ("y", 2), ("z", 3))}
    for p in pol.values():
        p["head"] = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(p["head_sd"], "action_head."))
        p["pp"] = modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=_sub(p["pp_sd"], "proprio_projector."))
    g = torch.Generator().manual_seed(3)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    pv = torch.randn(len(LENS), 12, 56, 56, generator=g).to(BF).float()
    proprio = (torch.rand(len(LENS), 8, generator=g) * 2 - 1).to(BF).float().numpy()
    w = dict(modeling=modeling, cfg=cfg, ocfg=ocfg, base=base, pol=pol, prompts=prompts, pv=pv, proprio=proprio, dev=dev, models={})

    def model(names, heads=True, stats=None):
        """A base model with the named policies in that slot order (cached)."""
        key = (tuple(names), heads)
        if key not in w["models"]:
            vla = modeling.OpenVLAForActionPrediction(cfg, base, device=dev, norm_stats=IDENT)
            for nm in names:
                p = pol[nm]
                vla.add_policy(nm, p["lora"], action_head=p["head"] if heads else None, proprio_projector=p["pp"] if heads else None,
                               norm_stats=(stats or {}).get(nm))
            w["models"][key] = vla
        return w["models"][key]

    w["model"] = model
    # the existing single-adapter path: X's adapters in the state dict
    w["single_x"] = modeling.OpenVLAForActionPrediction(cfg, {**base, **pol["x"]["lora"]}, device=dev, norm_stats=IDENT)
    return w


def _run(w, vla, idx, policy, heads=True):
    """predict_action_batch on the samples idx (in that order) with policy[k] for idx[k] -> {sample: (actions, hidden)}."""
    prompts = [(w["prompts"][i], None) for i in idx]
    kw = dict(proprio=w["proprio"][list(idx)]) if heads else {}
    a, h = vla.predict_action_batch(prompts, w["pv"][list(idx)], unnorm_key=UNNORM, policy=policy, **kw)
    assert a.shape == (len(idx), 8, 7) and h.shape == (len(idx), 56, w["cfg"].llm_dim)
    return {i: (a[k], h[k].clone()) for k, i in enumerate(idx)}


def _single(w, idx, name="x"):
    p = w["pol"][name]
    a, h = w["single_x"].predict_action_batch([(w["prompts"][i], None) for i in idx], w["pv"][list(idx)], unnorm_key=UNNORM, proprio=w["proprio"][list(idx)],
                                              proprio_projector=p["pp"], action_head=p["head"])
    return {i: (a[k], h[k].clone()) for k, i in enumerate(idx)}


@pytest.mark.gpu
def test_one_slot_is_the_existing_path(world):
    """n = 1: the slotted base model computes, bit for bit, what a model built with X's adapters in its state dict computes."""
    w, idx = world, list(range(len(LENS)))
    vla = w["model"](["x"])
    assert vla.policies == ("x",) and vla.engine.n_slots == 1
    got, want = _run(w, vla, idx, ["x"] * len(idx)), _single(w, idx)
    for i in idx:
        assert np.array_equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]), f"sample {i}"
    base_only = vla.predict_action_batch([(w["prompts"][0], None)], w["pv"][:1], unnorm_key=UNNORM)[1]     # without policy=: the base model, no adapter
    assert not torch.equal(base_only[0], got[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["l1", "discrete"])
def test_routing_invariance(world, kind):
    """An observation routed to X: the same bits alone, among Y's, in reversed order, and on a model whose slots are (Z, X)."""
    w, heads = world, kind == "l1"
    xy, zx = w["model"](["x", "y"], heads), w["model"](["z", "x"], heads)
    B = len(LENS)
    for i in (0, 3):
        alone = _run(w, xy, [i], ["x"], heads)[i]
        idx = list(range(B))
        among = _run(w, xy, idx, ["x" if k == i else "y" for k in idx], heads)
        rev = _run(w, xy, idx[::-1], ["x" if k == i else "y" for k in idx[::-1]], heads)
        other = _run(w, zx, idx, ["x" if k == i else "z" for k in idx], heads)
        for name, res in (("among Y", among[i]), ("reversed", rev[i]), ("slots (Z, X)", other[i])):
            assert np.array_equal(alone[0], res[0]) and torch.equal(alone[1], res[1]), f"sample {i} {name}"
        j = (i + 1) % B                     # and its Y neighbour is not X's result for that observation
        assert not torch.equal(among[j][1], _run(w, xy, [j], ["x"], heads)[j][1])


@pytest.mark.gpu
def test_one_captured_graph_serves_two_assignments(world):
    w, idx = world, list(range(len(LENS)))
    vla = w["model"](["x", "y"])
    a1, a2 = ["x", "y", "x", "y", "x"], ["y", "y", "x", "x", "y"]
    e1, e2 = _run(w, vla, idx, a1), _run(w, vla, idx, a2)
    vla.enable_graph_replay(True)
    try:
        g1 = _run(w, vla, idx, a1)
        graphs = [g for k, g in vla._graphs.items() if "policies" in k]
        assert len(graphs) == 1 and graphs[0].captures == 1
        g2 = _run(w, vla, idx, a2)
        g1b = _run(w, vla, idx, a1)
        assert [g for k, g in vla._graphs.items() if "policies" in k] == graphs and graphs[0].captures == 1, "no new capture for another assignment"
    finally:
        vla.enable_graph_replay(False)
    for i in idx:
        for got, want in ((g1, e1), (g2, e2), (g1b, e1)):
            assert np.array_equal(got[i][0], want[i][0]) and torch.equal(got[i][1], want[i][1]), f"sample {i}: graph replay != eager"
    assert not np.array_equal(e1[1][0], e2[2][0])


@pytest.mark.gpu
def test_right_answers_at_two_slots(world):
    """Rows routed to X at n = 2 against the single-adapter X model, with the tolerance taken from that path's own distance to the oracle's
    fp32 forward of base + X:  err_multi <= 1.5 * err_single  (K2 = 64 may resolve to another fixed schedule: only summation orders differ).
    Both errors and the oracle's distance between the policies are printed; DESIGN.md section 5 is where a run's figures are recorded."""
    w, idx = world, list(range(len(LENS)))
    ops = load("openvla-oft_amd.ops")
    px, py = w["pol"]["x"], w["pol"]["y"]
    stats = {"x": IDENT, "y": STATS_Y}
    key = (("x", "y"), "stats")
    if key not in w["models"]:
        vla = w["modeling"].OpenVLAForActionPrediction(w["cfg"], w["base"], device=w["dev"], norm_stats=IDENT)
        for nm in ("x", "y"):
            vla.add_policy(nm, w["pol"][nm]["lora"], action_head=w["pol"][nm]["head"], proprio_projector=w["pol"][nm]["pp"], norm_stats=stats[nm])
        w["models"][key] = vla
    vla = w["models"][key]
    assign = ["x", "y", "x", "y", "x"]
    multi, single = _run(w, vla, idx, assign), _single(w, idx)
    ox = vo.Oracle(w["ocfg"], {**w["base"], **px["lora"], **px["head_sd"], **px["pp_sd"]}, mode="fp32")
    oy = vo.Oracle(w["ocfg"], {**w["base"], **py["lora"], **py["head_sd"], **py["pp_sd"]}, mode="fp32")
    oyx = vo.Oracle(w["ocfg"], {**w["base"], **py["lora"], **px["head_sd"], **px["pp_sd"]}, mode="fp32")   # X's head on Y's adapters: a routing mistake
    err_single = err_multi = 0.0
    gap = gap_lora = np.inf
    for i in (0, 2, 4):
        ids = w["prompts"][i][None]
        ref = lambda o: o.predict_action(ids, torch.ones_like(ids, dtype=torch.bool), w["pv"][i: i + 1], proprio=w["proprio"][i])[0]  # noqa: E731
        rx = ref(ox)
        err_single = max(err_single, float(np.abs(single[i][0] - rx).max()))
        err_multi = max(err_multi, float(np.abs(multi[i][0] - rx).max()))
        gap, gap_lora = min(gap, float(np.abs(rx - ref(oy)).max())), min(gap_lora, float(np.abs(rx - ref(oyx)).max()))
    tol = 1.5 * err_single
    print(f"err_single {err_single:.4e}  err_multi {err_multi:.4e}  oracle |X - Y| {gap:.4e}  oracle |X - (Y adapters, X head)| {gap_lora:.4e}")
    assert gap >= 10 * tol and gap_lora >= 10 * tol, "precondition: the policies differ by 10x the tolerance, so a routing mistake cannot pass"
    assert err_multi <= tol
    # per-policy un-normalisation: each observation's actions are its own policy's head on its hidden states under its own q01 / q99
    for i, nm in zip(idx, assign):
        with ops.batch_invariant(True):
            normalized = w["pol"][nm]["head"].predict_action(multi[i][1][None]).reshape(8, 7).float().cpu().numpy()
        assert np.array_equal(multi[i][0], vla._unnormalize_actions(normalized, UNNORM, stats[nm]))
        assert not np.array_equal(multi[i][0], vla._unnormalize_actions(normalized, UNNORM, stats["y" if nm == "x" else "x"]))


@pytest.mark.gpu
def test_refusals(world):
    w = world
    modeling, cfg, dev, pol = w["modeling"], w["cfg"], w["dev"], w["pol"]
    engine = load("openvla-oft_amd.engine")
    x = pol["x"]
    fresh = lambda: modeling.OpenVLAForActionPrediction(cfg, w["base"], device=dev, norm_stats=IDENT)  # noqa: E731
    vla = fresh()
    vla.add_policy("x", x["lora"], action_head=x["head"], proprio_projector=x["pp"])
    half = {k: (v[:16] if ".lora_A." in k else v[:, :16]).contiguous() for k, v in pol["y"]["lora"].items()}
    with pytest.raises(ValueError, match="rank"):
        vla.add_policy("y", half, action_head=pol["y"]["head"], proprio_projector=pol["y"]["pp"])
    with pytest.raises(ValueError, match="lora_alpha"):
        vla.add_policy("y", pol["y"]["lora"], action_head=pol["y"]["head"], proprio_projector=pol["y"]["pp"], lora_alpha=32)
    fewer = {k: v for k, v in pol["y"]["lora"].items() if "projector.fc3" not in k}
    with pytest.raises(ValueError, match="different sets"):
        vla.add_policy("y", fewer, action_head=pol["y"]["head"], proprio_projector=pol["y"]["pp"])
    assert vla.policies == ("x",) and vla.engine.n_slots == 1, "a refused policy changes nothing"
    for nm in ("a", "b", "c"):
        vla.add_policy(nm, pol["y"]["lora"], action_head=pol["y"]["head"], proprio_projector=pol["y"]["pp"])
    with pytest.raises(ValueError, match="at most"):
        vla.add_policy("fifth", pol["z"]["lora"], action_head=pol["z"]["head"], proprio_projector=pol["z"]["pp"])
    one = [(w["prompts"][0], None)]
    with pytest.raises(ValueError, match="unknown policy"):
        vla.predict_action_batch(one, w["pv"][:1], unnorm_key=UNNORM, proprio=w["proprio"][:1], policy=["nobody"])
    sdd = {k: v.to(BF).float() for k, v in vo.random_state_dict(w["ocfg"], seed=1, diffusion=True).items()}
    dhead = modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=4, device=dev, state_dict=_sub(sdd, "action_head."))
    nap = modeling.NoisyActionProjector(cfg.llm_dim, device=dev, state_dict=_sub(sdd, "noisy_action_projector."))
    with pytest.raises(ValueError, match="diffusion"):
        vla.predict_action_batch(one, w["pv"][:1], unnorm_key=UNNORM, proprio=w["proprio"][:1], action_head=dhead, noisy_action_projector=nap, policy=["x"])
    film_sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(vo.tiny_config(), seed=4, film=True, lora=False).items()}
    fcfg = load("openvla-oft_amd.config").VLAConfig.from_any(vo.tiny_config())
    fvla = modeling.OpenVLAForActionPrediction(fcfg, film_sd, device=dev, norm_stats=IDENT, use_film=True)
    with pytest.raises(ValueError, match="FiLM"):
        fvla.predict_action_batch(one, w["pv"][:1], unnorm_key=UNNORM, use_film=True, policy=["x"])
    with pytest.raises(ValueError, match="merged or trainable"):
        w["single_x"].add_policy("y", pol["y"]["lora"])
    merged = modeling.OpenVLAForActionPrediction(cfg, {**w["base"], **x["lora"]}, device=dev, norm_stats=IDENT).merge_and_unload()
    with pytest.raises(ValueError, match="merged or trainable"):
        merged.add_policy("y", pol["y"]["lora"])
    lin = next(l for l in vla.engine.llm.linears() if getattr(l, "n_slots", 0))
    assert isinstance(lin, engine.LoraLinear) and lin.n_slots == 4
    with pytest.raises(RuntimeError, match="inference-only"):
        lin.bwd(torch.zeros(8, lin.out_f, dtype=BF, device=dev), None)
