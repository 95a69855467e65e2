"""Per-tensor statistics in the engine and the fine-tune driver, on the reduced-size model of test_grad_clip_gpu.py: the names, every tensor's
record against the numpy restatement (tests/tensor_stats_reference.py) in both optimizer-state modes, agreement with the global clip norm,
read-only collection, the localisation of one NaN, and the driver's history, log file and switches."""
import importlib
import json
import math

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import tensor_stats_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
FIELDS = {"grad_norm", "param_norm", "grad_absmax", "n_nonfinite", "n_bad_steps"}


def bits_of(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == BF:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int64).numpy().view(np.uint64) if t.dtype == torch.float64 else t.view(torch.int32).numpy().view(np.uint32)


@pytest.fixture(scope="module")
def world(dev):
    config_mod, synth, ft, K = (load("openvla-oft_amd." + m) for m in ("config", "synthetic", "vla_scripts.finetune", "prismatic.vla.constants"))
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    base = config_mod.VLAConfig.from_any(ocfg)
    fcfg = ft.FinetuneConfig()
    cfg = config_mod.VLAConfig(**{**base.__dict__, "num_images": 2, "lora_rank": fcfg.lora_rank, "lora_alpha": min(fcfg.lora_rank, 16),
                                  "action_dim": K.ACTION_DIM, "chunk": K.NUM_ACTIONS_CHUNK, "proprio_dim": K.PROPRIO_DIM,
                                  "norm_type": K.ACTION_PROPRIO_NORMALIZATION_TYPE.value})
    stats = {"libero_spatial_no_noops": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    return dict(cfg=cfg, base_cfg=base, sd=sd, synth=synth, ft=ft, stats=stats)


def fresh(world, dev):
    engine_mod, weights_mod = load("openvla-oft_amd.engine"), load("openvla-oft_amd.weights")
    get, has = weights_mod.make_getter({k: v.clone() for k, v in world["sd"].items()}, dev)
    return engine_mod.VLAEngine(world["cfg"], get, dev, lora=True, use_proprio=True, head="l1", has=has)


def batch_of(world, i):
    return world["synth"].make_batch(2, seed=100 + i, prompt_lens=[9, 8], image_size=56)


def trained_state(e):
    return {(w, i, str(dt)): bits_of(t) for w in ("flat", "exp_avg", "exp_avg_sq", "master") for i, st in enumerate(e.stores) for dt, t in getattr(st, w).items()}


def same_state(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def backward(e, world, i):
    e.zero_grad()
    loss_sum, _, _ = e.train_step_fwd_bwd(batch_of(world, i))
    return bits_of(loss_sum)


def all_params(e):
    return {name: (st, p) for st in e.stores for name, p in st.named().items()}


def test_api_needs_enable_and_names_are_the_stores_names(world, dev):
    e = fresh(world, dev)
    assert not e.tensor_stats_enabled
    for call in (e.tensor_stats, e.first_nonfinite, e.collect_tensor_stats):
        with pytest.raises(RuntimeError, match="enable_tensor_stats"):
            call()
    e.enable_tensor_stats()
    held = e._tensor_stats
    e.enable_tensor_stats()
    assert e.tensor_stats_enabled and e._tensor_stats is held, "idempotent"
    table = e.tensor_stats()
    union = set().union(*(st.named().keys() for st in e.stores))
    assert set(table) == union and len(table) == sum(len(st.params) for st in e.stores) > 20
    assert all(set(s) == FIELDS for s in table.values())
    assert all(s == dict(grad_norm=0.0, param_norm=0.0, grad_absmax=0.0, n_nonfinite=0, n_bad_steps=0) for s in table.values()), "zeroed before a collection"
    assert e.first_nonfinite() is None
    # table order: the stores in order, bf16 before fp32, ascending offset
    order = [p.name for st in e.stores for dt in st.flat for p in sorted((q for q in st.params if q.dtype == dt), key=lambda q: q.offset)]
    assert list(table) == order
    e.enable_ema()
    with e.ema_weights():                                           # the flat buffers hold the averaged weights: refused like the other enable_* calls
        for call in (e.enable_tensor_stats, e.collect_tensor_stats):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()


@pytest.mark.parametrize("mode", ("param", "fp32"))
def test_every_tensor_equals_the_restatement_and_the_global_norm_agrees(world, dev, mode):
    e = fresh(world, dev)
    if mode == "fp32":
        e.enable_fp32_optimizer_state()
    e.enable_tensor_stats()
    e.enable_grad_clip(math.inf)
    backward(e, world, 0)
    e.adamw_step(5e-4)                                              # a first step: in fp32 mode the master then differs from the bf16 parameter
    e.refresh_derived()
    backward(e, world, 1)
    scale = 0.5
    e.collect_tensor_stats(grad_scale=scale)
    table = e.tensor_stats()
    for name, (st, p) in all_params(e).items():
        rounds = p.dtype == BF and not st.fp32_state
        if p.dtype == BF and st.fp32_state:
            data = st.master[BF][p.offset:p.offset + p.numel].cpu().numpy()
        else:
            data = p.data.detach().float().cpu().numpy().reshape(-1)   # bf16 -> fp32 is exact
        want = R.segment_stats(p.grad.detach().cpu().numpy().reshape(-1), data, grad_scale=scale, grad_round_bf16=rounds)
        got = table[name]
        assert np.float64(got["grad_norm"]).tobytes() == np.sqrt(want["grad_sumsq"]).tobytes(), (name, got, want)
        assert np.float64(got["param_norm"]).tobytes() == np.sqrt(want["param_sumsq"]).tobytes(), (name, got, want)
        assert np.float32(got["grad_absmax"]).tobytes() == want["grad_absmax"].tobytes() and (got["n_nonfinite"], got["n_bad_steps"]) == (0, 0), (name, got, want)
    assert sum(s["grad_norm"] > 0 for s in table.values()) > len(table) // 2 and all(s["param_norm"] >= 0 for s in table.values())
    # sqrt of the summed per-tensor sums against the clip state's norm, (float)sqrt of the per-buffer double sums: the same squares, added
    # in another order in double (relative 1e-16 each), then one fp32 rounding -- within 2 fp32 ulps
    e.adamw_step(5e-4, grad_scale=scale)
    norm = np.float32(e.grad_clip_stats()["norm"])
    sums = load("openvla-oft_amd.ops").read_tensor_stats(e._tensor_stats["out"])["grad_sumsq"]   # the device's double sums themselves
    mine = np.float32(math.sqrt(float(sums.sum())))
    ulps = abs(int(norm.view(np.int32)) - int(mine.view(np.int32)))
    print(f"{mode}: clip norm {norm!r}, per-tensor {mine!r}, {ulps} ulps")
    assert ulps <= 2


def test_collection_is_read_only(world, dev):
    e, plain = fresh(world, dev), fresh(world, dev)
    e.enable_tensor_stats()
    for i in range(3):
        la, lb = backward(e, world, i), backward(plain, world, i)
        e.collect_tensor_stats()
        e.adamw_step(5e-4), plain.adamw_step(5e-4)
        e.refresh_derived(), plain.refresh_derived()
        assert np.array_equal(la, lb), f"loss of step {i}"
        assert same_state(trained_state(e), trained_state(plain)), f"parameters or moments after step {i}"
    assert e.first_nonfinite() is None and all(s["n_bad_steps"] == 0 for s in e.tensor_stats().values())


def test_one_nan_is_localised_and_latched(world, dev):
    e = fresh(world, dev)
    e.enable_tensor_stats()
    e.enable_grad_clip(math.inf)
    lora = sorted(n for n in e.store.named() if n.endswith(".lora_B"))
    name = lora[len(lora) // 2]
    backward(e, world, 0)                                           # a clean first step: the skipped one starts from allocated, non-zero moments
    e.collect_tensor_stats()
    e.adamw_step(5e-4)
    e.refresh_derived()
    assert e.first_nonfinite() is None
    backward(e, world, 1)
    e.store.named()[name].grad.view(-1)[3] = float("nan")           # one element of one LoRA factor's gradient, after the backward
    before = trained_state(e)
    e.collect_tensor_stats()
    e.adamw_step(5e-4)
    e.refresh_derived()
    assert e.first_nonfinite() == name
    table = e.tensor_stats()
    assert table[name]["n_nonfinite"] == 1 and math.isnan(table[name]["grad_norm"]) and table[name]["n_bad_steps"] == 1
    assert all(s["n_nonfinite"] == 0 and s["n_bad_steps"] == 0 and math.isfinite(s["grad_norm"]) for n, s in table.items() if n != name)
    assert e.grad_clip_stats()["skipped"] == 1 and same_state(trained_state(e), before), "the guard skipped the step"
    backward(e, world, 2)
    e.collect_tensor_stats()
    e.adamw_step(5e-4)
    e.refresh_derived()
    table = e.tensor_stats()
    assert e.first_nonfinite() is None and e.grad_clip_stats()["skipped"] == 1
    assert {n for n, s in table.items() if s["n_bad_steps"] > 0} == {name} and table[name]["n_bad_steps"] == 1 and table[name]["n_nonfinite"] == 0


# ----------------------------------------------------------------------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------------------------------------------------------------------
def drive(world, root, *, lines=None, poison=None, **kw):
    """Three optimizer steps of the driver.  `poison` = (collection index, tensor name): one NaN is written into that tensor's gradient right
    before that collection, as a backward that produced it would have left it."""
    ft = world["ft"]
    engines, orig = [], ft.VLAEngine

    def build(*a, **k):
        eng = orig(*a, **k)
        engines.append(eng)
        if poison is not None:
            collect, calls = eng.collect_tensor_stats, [0]

            def poisoned_collect(**kw):
                if calls[0] == poison[0]:
                    eng.store.named()[poison[1]].grad.view(-1)[0] = float("nan")
                calls[0] += 1
                collect(**kw)

            eng.collect_tensor_stats = poisoned_collect
        return eng

    cfg = ft.FinetuneConfig(run_root_dir=root, dataset_name="libero_spatial_no_noops", batch_size=2, num_images_in_input=2, use_proprio=True,
                            wandb_log_freq=1, max_steps=3, save_freq=100)
    ft.VLAEngine = build
    try:
        hist = ft.finetune(cfg, model_config=world["base_cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()},
                           dataset=(batch_of(world, i) for i in range(12)), dataset_statistics=world["stats"],
                           log=(lines.append if lines is not None else (lambda *_: None)), **kw)
    finally:
        ft.VLAEngine = orig
    return hist, (engines[0] if engines else None)


def test_driver_history_file_and_switches(world, dev, tmp_path):
    ft = world["ft"]
    today = {"loss_value", "learning_rate", "val", "grad_norm", "grad_clip_coef", "skipped_steps"}
    hist_off, engine_off = drive(world, tmp_path / "off")
    assert set(hist_off) == today and not engine_off.tensor_stats_enabled
    assert not list((tmp_path / "off").rglob("tensor_stats.jsonl")), "tensor_stats_freq=None writes no file"
    hist, engine = drive(world, tmp_path / "on", tensor_stats_freq=1)
    assert set(hist) == today | {"tensor_stats", "nonfinite_tensors"} and engine.tensor_stats_enabled
    assert hist["loss_value"] == hist_off["loss_value"] and hist["grad_norm"] == hist_off["grad_norm"], "read-only"
    assert [s for s, _ in hist["tensor_stats"]] == [0, 1, 2] and hist["nonfinite_tensors"] == [[], [], []]
    names = set().union(*(st.named().keys() for st in engine.stores))
    groups = {ft.tensor_stats_group(n) for n in names}
    assert {"vision_backbone.featurizer", "vision_backbone.fused_featurizer", "projector", "proprio_projector", "action_head",
            "language_model.model.layers.0"} <= groups
    for step, (_, g) in enumerate(hist["tensor_stats"]):
        assert set(g) == groups and all(set(v) == FIELDS - {"n_bad_steps"} for v in g.values())
        # the groups partition the tensors: their squares sum to the global norm the clip state logged for that step
        total = math.sqrt(sum(v["grad_norm"] ** 2 for v in g.values()))
        assert total == pytest.approx(hist["grad_norm"][step], rel=1e-6)
    log_file, = (tmp_path / "on").rglob("tensor_stats.jsonl")
    rows = [json.loads(l) for l in log_file.read_text().splitlines()]
    assert [r["step"] for r in rows] == [0, 1, 2] and all(set(r["tensors"]) == names and all(set(s) == FIELDS for s in r["tensors"].values()) for r in rows)
    # every second step: collected on steps 0 and 2, read back at the logging step that follows each
    hist2, _ = drive(world, tmp_path / "every2", tensor_stats_freq=2)
    assert [s for s, _ in hist2["tensor_stats"]] == [0, 2] and len(hist2["loss_value"]) == 3
    assert hist2["tensor_stats"][1][1] == hist["tensor_stats"][2][1]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="tensor_stats_freq"):
            drive(world, tmp_path / "bad", tensor_stats_freq=bad)


def test_driver_names_the_tensor_behind_a_skipped_step(world, dev, tmp_path):
    probe = fresh(world, dev)
    name = sorted(n for n in probe.store.named() if n.endswith(".lora_A"))[0]
    del probe
    lines = []
    hist, engine = drive(world, tmp_path / "nan", lines=lines, poison=(1, name), tensor_stats_freq=1)
    assert hist["skipped_steps"] == [0, 1, 1] and hist["nonfinite_tensors"] == [[], [name], [name]]
    group = world["ft"].tensor_stats_group(name)
    assert [g[group]["n_nonfinite"] for _, g in hist["tensor_stats"]] == [0, 1, 0] and math.isnan(hist["tensor_stats"][1][1][group]["grad_norm"])
    steps = [str(l) for l in lines if str(l).startswith("step ")]
    assert len(steps) == 3 and f"skipped 1 non-finite gradient in {name}" in steps[1], steps
    assert "non-finite" not in steps[0] and "non-finite" not in steps[2], "named once, on the logging step where the count rose"
    assert engine.tensor_stats()[name]["n_bad_steps"] == 1
