"""finetune(action_scale="fit") on the tiny configuration of the driver tests (tests/test_grad_clip_gpu.py), four optimizer steps: the L1 run
keeps its bits, the checkpoint holds the scale head and its moments, a resumed run lands on the uninterrupted one, and without the option the
files and history keys are the ones the driver always wrote."""
import importlib
import math

import pytest
import torch

from oracle import vla_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
SCALE_PREFIX = "action_scale_head."


@pytest.fixture(scope="module")
def world(dev):
    config_mod, synth, ft = (load("openvla-oft_amd." + m) for m in ("config", "synthetic", "vla_scripts.finetune"))
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    stats = {"libero_spatial_no_noops": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    return dict(base_cfg=config_mod.VLAConfig.from_any(ocfg), sd=sd, synth=synth, ft=ft, stats=stats)


def batch_of(world, i):
    return world["synth"].make_batch(2, seed=100 + i, prompt_lens=[9, 8], image_size=56)


def drive(world, root, *, first=0, **kw):
    ft = world["ft"]
    engines, orig = [], ft.VLAEngine

    def build(*a, **k):
        engines.append(orig(*a, **k))
        return engines[-1]

    opts = {k: kw.pop(k) for k in ("action_scale", "init_action_scale", "action_scale_bounds") if k in kw}
    cfg = ft.FinetuneConfig(**{**dict(run_root_dir=root, dataset_name="libero_spatial_no_noops", batch_size=2, num_images_in_input=2, use_proprio=True,
                                      wandb_log_freq=1, max_steps=4, save_freq=2), **kw})
    ft.VLAEngine = build
    try:
        hist = ft.finetune(cfg, model_config=world["base_cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()},
                           dataset=(batch_of(world, i) for i in range(first, 12)), dataset_statistics=world["stats"], log=lambda *_: None, **opts)
    finally:
        ft.VLAEngine = orig
    engine, = engines
    return hist, engine


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


@pytest.fixture(scope="module")
def runs(world, dev, tmp_path_factory):
    root = tmp_path_factory.mktemp("scale_head")
    hist, engine = drive(world, root / "fit", action_scale="fit", init_action_scale=0.5)
    hist_off, engine_off = drive(world, root / "off")
    ck, = (root / "fit").glob("*--2_chkpt")
    ck_off, = (root / "off").glob("*--2_chkpt")
    return dict(hist=hist, engine=engine, hist_off=hist_off, engine_off=engine_off, ck=ck, ck_off=ck_off)


def test_the_l1_run_keeps_its_bits(runs):
    hist, hist_off = runs["hist"], runs["hist_off"]
    assert len(hist["loss_value"]) == 4 and hist["loss_value"] == hist_off["loss_value"], "the L1 loss history"
    live, off = runs["engine"].export_trainable("data"), runs["engine_off"].export_trainable("data")
    assert {k for k in live if not k.startswith(SCALE_PREFIX)} == set(off) and len(off) > 10
    for k, v in off.items():
        assert torch.equal(bits(live[k]), bits(v)), f"{k}: the fitted run's bits differ from the plain run's"
    assert len(hist["scale_nll"]) == len(hist["action_scale"]) == 4
    assert all(math.isfinite(x) for x in hist["scale_nll"]) and all(0.0 < b < 2.72 for b in hist["action_scale"])
    assert abs(hist["action_scale"][0] - 0.5) < 0.01, "the first step sees the fresh head: b = init_action_scale up to the bias's bf16 rounding"
    w, b = live[SCALE_PREFIX + "log_scale.weight"], live[SCALE_PREFIX + "log_scale.bias"]
    assert bool((w != 0).any()) and bool((b.float() != math.log(0.5)).any()), "four AdamW steps moved the scale head"
    assert runs["engine_off"].scale_head is None and len(runs["engine_off"].stores) + 1 == len(runs["engine"].stores)


def test_checkpoint_holds_the_scale_head_and_its_moments(runs):
    from safetensors.torch import load_file

    listing = lambda d: sorted(str(f.relative_to(d)) for f in d.rglob("*"))  # noqa: E731
    fit, off = listing(runs["ck"]), listing(runs["ck_off"])
    assert set(fit) - set(off) == {"action_scale_head--2_checkpoint.pt"} and set(off) <= set(fit)
    assert not any("scale" in f for f in off), "without action_scale the checkpoint's file list is what it was"
    part = torch.load(str(runs["ck"] / "action_scale_head--2_checkpoint.pt"), weights_only=True, map_location="cpu")
    assert set(part) == {"log_scale.weight", "log_scale.bias"} and part["log_scale.weight"].dtype == BF and tuple(part["log_scale.bias"].shape) == (7,)
    osd, osd_off = load_file(str(runs["ck"] / "optimizer_state--2_checkpoint.safetensors")), load_file(str(runs["ck_off"] / "optimizer_state--2_checkpoint.safetensors"))
    i = len(runs["engine"].stores) - 1
    assert set(osd) - set(osd_off) == {f"store{i}.step", f"store{i}.bf16.exp_avg", f"store{i}.bf16.exp_avg_sq"} and set(osd_off) <= set(osd)
    assert int(osd[f"store{i}.step"].item()) == 3 and bool((osd[f"store{i}.bf16.exp_avg"].float() != 0).any())
    for k in osd_off:
        assert torch.equal(osd[k], osd_off[k]), f"optimizer state {k}"
    # without the option: the history keys the driver always had (the non-finite guard is on by default)
    assert set(runs["hist_off"]) == {"loss_value", "learning_rate", "val", "grad_norm", "grad_clip_coef", "skipped_steps"}
    assert set(runs["hist"]) == set(runs["hist_off"]) | {"scale_nll", "action_scale"}


def test_resume_lands_on_the_uninterrupted_run(runs, world, tmp_path):
    """The checkpoint of log step 2 holds three optimizer steps; resumed for one more it ends where the four-step run ended."""
    hist, resumed = drive(world, tmp_path / "resumed", first=3, resume=True, resume_step=2, vla_path=str(runs["ck"]), max_steps=3, action_scale="fit",
                          init_action_scale=0.25)   # (another initial scale: the loaded head replaces it)
    want, got = runs["engine"].export_trainable("data"), resumed.export_trainable("data")
    assert set(want) == set(got)
    for k, v in want.items():
        assert torch.equal(bits(got[k]), bits(v)), f"{k}: resumed vs uninterrupted"
    assert hist["loss_value"] == runs["hist"]["loss_value"][3:] and hist["scale_nll"] == runs["hist"]["scale_nll"][3:]
    st, st_r = runs["engine"].scale_head.store, resumed.scale_head.store
    assert st.step == st_r.step == 4 and torch.equal(bits(st.exp_avg[BF]), bits(st_r.exp_avg[BF]))


def test_refusals(world, tmp_path):
    ft = world["ft"]
    with pytest.raises(ValueError, match="action_scale"):
        ft.finetune(ft.FinetuneConfig(), action_scale="learned")
    with pytest.raises(ValueError, match="use_l1_regression"):
        ft.finetune(ft.FinetuneConfig(use_l1_regression=False, use_diffusion=True), action_scale="fit")
    with pytest.raises(ValueError, match="use_l1_regression"):
        ft.finetune(ft.FinetuneConfig(use_l1_regression=False, use_diffusion=False), action_scale="fit")
