"""output_attentions through the layers above the kernel: engine.AttnCapture inside LlamaStack.fwd (a read-only launch per layer: every
other result keeps its bits), OpenVLAForActionPrediction.forward(output_attentions=True), and the ActionAttention of predict_action /
predict_action_batch.  The kernel itself: tests/test_attn_probs_gpu.py."""
import importlib

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import attn_probs_reference as pr
from tests import attn_reference as ar
from tests import step_invariants as si

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
UNNORM = "libero_spatial_no_noops"
LENS = [7, 12, 9]


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ"


@pytest.fixture(scope="module")
def tw(dev):
    """The reduced LoRA model of the engine tests with its ragged B = 3 batches (unfolded decoder, trainable)."""
    return si.make_world(dev, "l1")


@pytest.fixture(scope="module")
def fw(dev):
    """An adapter-free decoder wide enough for the RMSNorm fold (llm_dim % 512 == 0, head_dim 128): the folded inference path."""
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0, lora=False).items()}
    vla = modeling.OpenVLAForActionPrediction(config_mod.VLAConfig.from_any(ocfg), sd, device=dev)
    assert getattr(vla.engine.llm, "folded", False)
    return dict(eng=vla.engine, batch=si.make_batch(2))


@pytest.fixture(scope="module")
def small(dev):
    """The standard tiny model with an L1 head, a diffusion head and three prompts of different lengths (tests/test_batch_inference_gpu.py's)."""
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    sdd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=1, diffusion=True).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    stats = {UNNORM: {"action": {"q01": [-1.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 1], "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    w = dict(cfg=cfg, modeling=modeling, vla=modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats=stats),
             vla_d=modeling.OpenVLAForActionPrediction(cfg, sdd, device=dev, norm_stats=stats),
             head=modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head.")),
             dhead=modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=3, device=dev, state_dict=_sub(sdd, "action_head.")),
             pp=modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict={"module." + k: v for k, v in _sub(sd, "proprio_projector.").items()}),
             pp_d=modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=_sub(sdd, "proprio_projector.")),
             nap=modeling.NoisyActionProjector(cfg.llm_dim, device=dev, state_dict=_sub(sdd, "noisy_action_projector.")))
    g = torch.Generator().manual_seed(5)
    w["prompts"] = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    w["pv"] = torch.randn(len(LENS), 12, 56, 56, generator=g).to(BF).float()
    w["proprio"] = (torch.rand(len(LENS), 8, generator=g) * 2 - 1).to(BF).float().numpy()
    return w


def _fwd(eng, batch, **kw):
    return eng.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"), **kw)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["unfolded", "folded", "folded-invariant"])
@pytest.mark.parametrize("sel", [None, "actions"], ids=["all-rows", "sel"])
def test_capture_keeps_the_forward_bits(tw, fw, which, sel):
    """hidden / action_hidden with and without attn_capture are the same bits: fold on and off, `sel` on and off."""
    engine, ops = load("openvla-oft_amd.engine"), load("openvla-oft_amd.ops")
    eng, batch = (tw["eng"], tw["batches"][0]) if which == "unfolded" else (fw["eng"], fw["batch"])
    with ops.batch_invariant(True) if which == "folded-invariant" else ops.batch_invariant(False):
        if which == "folded-invariant":
            assert eng.llm._fold_fixed_ok(), "the fixed-schedule fold is not available at these shapes: the test would not cover it"
        plain = _fwd(eng, batch, train=False, sel=sel)
        cap = engine.AttnCapture(rows="actions", per_head=True)
        got = _fwd(eng, batch, train=False, sel=sel, attn_capture=cap)
    assert "attention" not in plain and got["attention"]["mean"] is cap.result()["mean"]
    key = "hidden" if sel is None else "action_hidden"
    same_bits(got[key], plain[key], f"{which} {key}")
    B, S = batch["input_ids"].shape[0], got["S"]
    A, H, L = eng.cfg.num_action_tokens, eng.cfg.llm_heads, len(eng.llm.layers)
    att = got["attention"]
    assert att["mean"].shape == (L, B * A, S) and att["per_head"].shape == (L, B * A, H, S) and att["layers"] == list(range(L))
    same_bits(att["rows"], got["action_rows"].reshape(-1), "rows")
    assert torch.isfinite(att["mean"]).all() and bool((att["mean"].sum(-1) - 1).abs().max() < 1e-3)


def test_capture_keeps_the_training_step_bits(tw):
    """train=True: predictions, loss and every gradient buffer with and without attn_capture."""
    engine = load("openvla-oft_amd.engine")
    eng, batch = tw["eng"], tw["batches"][0]
    F = si.Findings()
    eng.zero_grad()
    plain = si.step(tw, batch)
    eng.zero_grad()
    cap = engine.AttnCapture(rows="actions")
    loss_sum, count, pred = eng.train_step_fwd_bwd(batch, attn_capture=cap)
    grads = si.export_grads(eng)
    F.same_bits(pred, plain.pred, "predictions")
    F.same_loss(loss_sum, plain.loss_sum, si.loss_reference(pred, si.step_target(tw, 0), mse=False), "loss_sum")
    F.same_grads(grads, plain.grads, "gradients")
    F.every_tensor_nonzero(grads, "gradients")
    F.done()
    assert cap.result()["mean"].shape[0] == len(eng.llm.layers) and torch.isfinite(cap.result()["mean"]).all()


def test_each_layer_is_captured_from_its_own_qkv_and_lse(tw):
    """train=True keeps every layer's qkv, o and lse: the capture of layer i is bit-equal to ops.attn_probs on layer i's saved tensors at
    the action rows (the right layer, rows and views); P @ V reproduces the saved o inside the forward's own bound (c = 3); padding keys
    are exactly 0 and the rows sum to 1 inside the bound.  `layers` selects and orders the captured layers."""
    engine, ops = load("openvla-oft_amd.engine"), load("openvla-oft_amd.ops")
    eng, batch = tw["eng"], tw["batches"][0]
    cfg = eng.cfg
    D, H, hd, A = cfg.llm_dim, cfg.llm_heads, cfg.llm_dim // cfg.llm_heads, cfg.num_action_tokens
    cap = engine.AttnCapture(rows="actions", per_head=True)
    out = _fwd(eng, batch, train=True, attn_capture=cap)
    B, S = batch["input_ids"].shape[0], out["S"]
    saved_layers, kv_len = out["saved"].lsaved[0], out["kv_len"]
    rows_dev = out["action_rows"].reshape(-1)
    rows = rows_dev.cpu().tolist()
    att = out["attention"]
    assert len(saved_layers) == len(eng.llm.layers) == att["mean"].shape[0]
    causal = cfg.mask_mode == "causal"
    kvl = kv_len.cpu().tolist()
    assert min(kvl) < S, "the batch has no padding keys: the test would not cover them"
    heads = lambda t: t.detach().cpu().double().reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()  # noqa: E731
    valid = torch.ones(len(rows), dtype=torch.bool)
    for li, sv in enumerate(saved_layers):
        qkv, o, lse = sv[3], sv[4], sv[5]
        P, Pm = ops.attn_probs(qkv[:, :D], qkv[:, D:2 * D], lse, B, S, H, hd, rows=rows_dev, kv_len=kv_len, causal=causal, per_head=True)
        same_bits(att["per_head"][li], P, f"layer {li} per-head capture")
        same_bits(att["mean"][li], Pm, f"layer {li} mean capture")
        if li > 0:
            assert not torch.equal(att["mean"][li], att["mean"][li - 1])
        q, k, v = heads(qkv[:, :D]), heads(qkv[:, D:2 * D]), heads(qkv[:, 2 * D:])
        P_ref, lse_ref, E = pr.reference(q, k, v, kvl, causal, hd ** -0.5)
        Pc = P.cpu()
        pr.check_probs(Pc, pr.gather(P_ref, rows), pr.gather(E, rows), 2, what=f"layer {li} P")
        pr.check_row_sums(Pc, pr.gather(E, rows), valid, 2, what=f"layer {li} row sums")
        # the head mean's rows: the mean of H sums inside 2 E each, plus the fp32 roundings of the H adds and the scaling (2^-23 per element sum)
        mean_err = (att["mean"][li].cpu().double().sum(-1) - 1.0).abs()
        assert bool((mean_err <= 2 * pr.gather(E, rows).amax(-1) + (H + 1) * 2.0 ** -23).all()), f"layer {li}: head-mean row sums off by {float(mean_err.max()):.3e}"
        for i, r in enumerate(rows):
            assert not (Pc[i, :, kvl[r // S]:] != 0).any(), f"layer {li}: a padding key of list entry {i} is not exactly 0"
        PV = torch.stack([torch.einsum("hs,hsd->hd", Pc[i].double(), v[r // S]) for i, r in enumerate(rows)])
        O = o.detach().cpu().double().reshape(B * S, H, hd)[rows]
        ar.check_elementwise(O, PV, pr.gather(P_ref @ v.abs(), rows), c=3, what=f"layer {li}: saved o vs P @ V")
    last = engine.AttnCapture(rows=rows_dev[:8].clone(), layers=[-1, 0])
    out2 = _fwd(eng, batch, train=False, attn_capture=last)
    assert out2["attention"]["layers"] == [len(saved_layers) - 1, 0] and out2["attention"]["per_head"] is None
    same_bits(out2["attention"]["mean"][0], att["mean"][-1][:8], "layers=[-1, 0]: first slot is the last layer")
    same_bits(out2["attention"]["mean"][1], att["mean"][0][:8], "layers=[-1, 0]: second slot is layer 0")


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _one(w, i, vla=None, **kw):
    vla = w["vla"] if vla is None else vla
    return vla.predict_action(input_ids=w["prompts"][i][None], attention_mask=torch.ones(1, len(w["prompts"][i]), dtype=torch.bool),
                              pixel_values=w["pv"][i: i + 1], unnorm_key=UNNORM, **kw)


def test_forward_output_attentions(small):
    """forward(output_attentions=True).attentions: n_layers tensors [B, H, S, S], equal to an engine capture of all rows; None otherwise."""
    w = small
    vla, cfg, engine = w["vla"], w["cfg"], load("openvla-oft_amd.engine")
    batch = si.make_batch(2)
    args = dict(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], pixel_values=batch["pixel_values"], labels=batch["labels"])
    with torch.no_grad():
        plain = vla.forward(**args)
        assert plain.attentions is None and vla.forward(**args, output_attentions=False).attentions is None
        out = vla.forward(**args, output_attentions=True)
    same_bits(out.hidden_states[-1], plain.hidden_states[-1], "hidden_states[-1]")
    B, S = out.hidden_states[-1].shape[:2]
    H = cfg.llm_heads
    assert isinstance(out.attentions, tuple) and len(out.attentions) == cfg.llm_layers
    cap = engine.AttnCapture(rows="all", per_head=True)
    ref = _fwd(vla.engine, batch | {"proprio": None}, train=False, attn_capture=cap)["attention"]
    assert ref["rows"] is None
    for li, a in enumerate(out.attentions):
        assert a.shape == (B, H, S, S) and a.dtype == torch.float32 and not a.requires_grad
        same_bits(a.contiguous(), ref["per_head"][li].view(B, S, H, S).permute(0, 2, 1, 3).contiguous(), f"attentions[{li}]")
        same_bits(pr.head_mean(ref["per_head"][li]), ref["mean"][li], f"mean of layer {li}")
    assert out["attentions"] is out.attentions


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph-replay"])
def test_predict_action_output_attentions(small, graph):
    """Actions and hidden states are the bits of the call without the flag, with graph replay on and off; no graph is built or dropped."""
    w = small
    vla = w["vla"]
    kw = dict(proprio=w["proprio"][1], proprio_projector=w["pp"], action_head=w["head"])
    vla.enable_graph_replay(graph)
    try:
        a0, h0 = _one(w, 1, **kw)
        n_graphs = len(vla._graphs)
        assert n_graphs == (1 if graph else 0)
        a1, h1, att = _one(w, 1, output_attentions=True, **kw)
        assert len(vla._graphs) == n_graphs
        a2, h2 = _one(w, 1, **kw)
    finally:
        vla.enable_graph_replay(False)
    assert np.array_equal(a0, a1) and np.array_equal(a0, a2)
    same_bits(h1, h0, "hidden with the flag")
    same_bits(h2, h0, "hidden after the flagged call")
    cfg = w["cfg"]
    A, n_p = cfg.num_action_tokens, cfg.dino.n_patches
    S = att.mean.shape[-1]
    assert isinstance(att, w["modeling"].ActionAttention) and att.mean.shape == (cfg.llm_layers, 1, A, S) and att.mean.dtype == torch.float32
    lay = att.layout[0]
    n_text = LENS[1] + 1                       # the prompt and the 29871 predict_action appends
    assert list(lay) == ["bos", "image0", "image1", "proprio", "text", "actions", "stop", "padding"]
    assert lay["bos"] == (0, 1) and lay["image0"] == (1, 1 + n_p) and lay["image1"] == (1 + n_p, 1 + 2 * n_p) and lay["proprio"] == (1 + 2 * n_p, 2 + 2 * n_p)
    assert lay["text"] == (2 + 2 * n_p, 1 + 2 * n_p + n_text) and lay["actions"] == (lay["text"][1], lay["text"][1] + A)
    assert lay["stop"] == (lay["actions"][1], lay["actions"][1] + 1) and lay["padding"] == (lay["stop"][1], S)
    stops = [0] + [r[1] for r in lay.values()]
    assert all(r[0] == s for r, s in zip(lay.values(), stops)) and stops[-1] == S, "the ranges tile [0, S)"
    mass = att.token_mass()
    assert mass.shape == (cfg.llm_layers, 1, A, len(lay))
    # the row-sum bound of the kernel test with its largest E over these rows: 2 units of LSE_U * (1 + |lse| + scale * max |q|.|k|) < 2^-17 * 64
    assert float((mass.sum(-1) - 1).abs().max()) <= 2 * ar.LSE_U * 64
    g = int(round(n_p ** 0.5))
    for i in range(2):
        pm = att.patch_maps(image=i)
        assert pm.shape == (cfg.llm_layers, 1, A, g, g)
        k0, k1 = lay[f"image{i}"]
        same_bits(pm.reshape(cfg.llm_layers, 1, A, g * g), att.mean[..., k0:k1], f"patch_maps(image={i})")
        same_bits(mass[..., list(lay).index(f"image{i}")], att.mean[..., k0:k1].sum(-1), f"token_mass image{i}")


def test_predict_action_batch_maps_do_not_depend_on_the_batch(small):
    """An observation's maps are the same bits alone and inside a batch of three with mixed prompt lengths, in either order: equal up to
    its own key length, exactly 0 behind it."""
    w = small
    vla = w["vla"]

    def run(idx):
        prompts = [(w["prompts"][i], None) for i in idx]
        a, h, att = vla.predict_action_batch(prompts, w["pv"][idx], unnorm_key=UNNORM, proprio=w["proprio"][idx], proprio_projector=w["pp"],
                                             action_head=w["head"], output_attentions=True)
        a0, h0 = vla.predict_action_batch(prompts, w["pv"][idx], unnorm_key=UNNORM, proprio=w["proprio"][idx], proprio_projector=w["pp"], action_head=w["head"])
        assert np.array_equal(a, a0)
        same_bits(h, h0, "hidden with and without the flag")
        return {i: (att.mean[:, k], att.layout[k]) for k, i in enumerate(idx)}

    full, rev = run([0, 1, 2]), run([2, 1, 0])
    assert len(vla._graphs) == 0
    for i in range(3):
        alone = run([i])[i]
        n = alone[1]["padding"][0]                                   # this observation's key length
        for name, (m, lay) in (("batch of three", full[i]), ("reversed batch", rev[i])):
            assert lay["padding"][0] == n and {k: v for k, v in lay.items() if k != "padding"} == {k: v for k, v in alone[1].items() if k != "padding"}
            same_bits(m[..., :n].contiguous(), alone[0][..., :n].contiguous(), f"observation {i}, {name}")
            assert not (m[..., n:] != 0).any() and not (alone[0][..., n:] != 0).any(), f"observation {i}: padding keys are not exactly 0"
    assert full[1][1]["padding"][0] > full[0][1]["padding"][0], "the prompts have different lengths"


def test_diffusion_head_refuses_output_attentions(small):
    w = small
    kw = dict(proprio=w["proprio"][0], proprio_projector=w["pp_d"], action_head=w["dhead"], noisy_action_projector=w["nap"])
    with pytest.raises(ValueError, match="diffusion"):
        _one(w, 0, vla=w["vla_d"], output_attentions=True, **kw)
    with pytest.raises(ValueError, match="diffusion"):
        w["vla_d"].predict_action_batch([(w["prompts"][0], None)], w["pv"][:1], unnorm_key=UNNORM, proprio=w["proprio"][:1], proprio_projector=w["pp_d"],
                                        action_head=w["dhead"], noisy_action_projector=w["nap"], output_attentions=True)
    a, h = _one(w, 0, vla=w["vla_d"], **kw)                           # and still samples without the flag
    assert a.shape == (8, 7)
