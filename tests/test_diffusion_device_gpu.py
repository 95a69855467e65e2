"""The diffusion objective on the device (VLAEngine.draw_diffusion / sample_actions, `diffusion_noise.call` in the checkpoint,
finetune(diffusion_noise="device")) on a reduced-size model built like test_api_gpu.py::world: diffusion head, FiLM off, 2 images, proprio."""
import importlib
import shutil

import numpy as np
import pytest
import torch

import diffusion_noise_reference as R
from lora_dropout_reference import bf16_bits_to_f32, to_bits
from oracle import vla_oracle as vo

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module
SEED = 0xD1FF + (2 << 32)
NP = "action_head.noise_predictor.mlp_resnet."


@pytest.fixture(scope="module")
def world(dev):
    config_mod, synth = load("openvla-oft_amd.config"), load("openvla-oft_amd.synthetic")
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0, diffusion=True).items()}
    # the same model with the MLPResNet as an L1 head: the L1 objective's resume distance is measured on it
    sd_l1 = {("action_head.model." + k[len(NP):] if k.startswith(NP) else k): v for k, v in sd.items() if not k.startswith("noisy_action_projector.")}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    stats = {"libero_spatial_no_noops": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    return dict(cfg=cfg, ocfg=ocfg, sd=sd, sd_l1=sd_l1, synth=synth, stats=stats)


def fresh(world, dev, head="diffusion", T=50, seed=SEED):
    engine_mod, weights_mod = load("openvla-oft_amd.engine"), load("openvla-oft_amd.weights")
    src = world["sd"] if head == "diffusion" else world["sd_l1"]
    get, has = weights_mod.make_getter({k: v.clone() for k, v in src.items()}, dev)
    kw = dict(num_diffusion_steps=T, diffusion_seed=seed) if head == "diffusion" else {}
    return engine_mod.VLAEngine(world["cfg"], get, dev, lora=True, use_proprio=True, head=head, has=has, **kw)


def batch_of(world, i, B=2):
    return world["synth"].make_batch(B, seed=100 + i, prompt_lens=[9, 8, 11][:B], image_size=56)


def test_draw_is_the_kernels_contract_for_the_engines_seed_and_call(world, dev):
    eng = fresh(world, dev)
    D, T = world["cfg"].llm_dim, 50
    diffusion = load("openvla-oft_amd.diffusion")
    ab = diffusion.DDIMScheduler(T).add_noise_coefficients().numpy()
    enc = diffusion.SinusoidalPositionalEncoding(D)
    eng.diffusion.call = 41
    for k in range(2):
        b = batch_of(world, k, B=3)
        d = eng.draw_diffusion(b["actions"])
        call = 41 + k
        assert eng.diffusion.call == call + 1, "one draw advances the counter by one"
        assert all(d[name].is_cuda for name in ("noise", "noisy_actions", "timestep_emb", "timesteps"))
        assert d["noise"].shape == (3, 8, 7) and d["noisy_actions"].shape == (3, 8, 7) and d["timestep_emb"].shape == (3, D) and d["timesteps"].dtype == torch.int32
        t_ref = R.timesteps(3, T, call=call, seed=SEED)
        assert np.array_equal(d["timesteps"].cpu().numpy(), t_ref)
        z = R.normals(3, 56, call=call, seed=SEED)
        lo, hi = R.bf16_bracket(z)
        noise_bits = to_bits(d["noise"].reshape(3, 56))
        got = bf16_bits_to_f32(noise_bits).astype(np.float64)
        assert ((got == lo) | (got == hi)).all() and (np.abs(got - z) <= 0.5 * R.bf16_ulp(z) + 1e-5).all()
        acts = to_bits(b["actions"].to(BF).reshape(3, 56))
        assert np.array_equal(to_bits(d["noisy_actions"].reshape(3, 56)), R.add_noise_bits(acts, noise_bits, ab, t_ref))
        want = torch.cat([enc(torch.tensor([float(t)])).to(BF) for t in t_ref])
        assert torch.equal(d["timestep_emb"].cpu(), want)
    with pytest.raises(RuntimeError, match="num_diffusion_steps"):
        fresh(world, dev, head="l1").draw_diffusion(b["actions"])


def test_step_with_device_noise_never_reads_the_device_back(world, dev, monkeypatch):
    """Host-side assertion, no timing: while draw_diffusion + train_step_fwd_bwd run, every readback of a device tensor raises."""
    eng = fresh(world, dev)
    b = batch_of(world, 0)
    eng.zero_grad()
    eng.train_step_fwd_bwd(b, diffusion=eng.draw_diffusion(b["actions"]))   # warm-up: lazily built tables and workspaces
    eng.zero_grad()
    torch.cuda.synchronize()
    calls = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def guarded(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda:
                calls.append(_name)
                raise AssertionError(f"Tensor.{_name}() on a device tensor: a host synchronisation inside the step")
            return _orig(self, *a, **kw)

        monkeypatch.setattr(torch.Tensor, name, guarded)
    d = eng.draw_diffusion(b["actions"])
    loss_sum, count, _ = eng.train_step_fwd_bwd(b, diffusion=d)
    monkeypatch.undo()
    assert not calls and loss_sum.is_cuda
    assert np.isfinite(loss_sum.item() / count)


def test_resume_continues_the_noise_stream_and_the_trajectory(world, dev, tmp_path):
    """Three updates with device noise, checkpoint, a fourth.  A fresh engine resumed from the checkpoint draws the fourth draw's very bits and
    lands where the uninterrupted run does -- as closely as the L1 objective (whose step has no noise at all) does on the same model; with
    `diffusion_noise.call` stripped from the file it replays the noise of step 0 and does not."""
    from safetensors.torch import load_file, save_file

    ft = load("openvla-oft_amd.vla_scripts.finetune")
    fcfg = ft.FinetuneConfig(learning_rate=5e-4)

    def update(e, i, diffusion):
        b = batch_of(world, i)
        e.zero_grad()
        d = e.draw_diffusion(b["actions"]) if diffusion else None
        e.train_step_fwd_bwd(b, diffusion=d)
        e.adamw_step(ft.learning_rate_at(fcfg, i))
        e.refresh_derived()
        return d

    def params(e):
        return {k: v.float().cpu().clone() for k, v in e.export_trainable("data").items()}

    def dist(e, straight):
        cur = params(e)
        num = sum(((cur[k] - straight[k]) ** 2).sum().item() for k in straight)
        return (num / sum((straight[k] ** 2).sum().item() for k in straight)) ** 0.5

    def run(head, tag):
        diffusion = head == "diffusion"
        e0 = fresh(world, dev, head=head)
        for i in range(3):
            update(e0, i, diffusion)
        ck = ft.save_training_checkpoint(tmp_path / tag, 3, e0, world["stats"], rank=0)
        d0 = update(e0, 3, diffusion)
        straight = params(e0)
        e1 = fresh(world, dev, head=head)
        info = ft.load_training_checkpoint(ck, 3, e1)
        assert info["optimizer"] and not info["missing"] and info["diffusion_call"] == diffusion
        d1 = update(e1, 3, diffusion)
        return ck, d0, d1, dist(e1, straight), straight

    _, _, _, dist_l1, _ = run("l1", "l1")
    ck, d0, d1, dist_with, straight = run("diffusion", "diff")
    assert "diffusion_noise.call" in load_file(str(ck / "optimizer_state--3_checkpoint.safetensors"))
    assert torch.equal(d1["timesteps"], d0["timesteps"]) and torch.equal(d1["noise"].view(torch.int16), d0["noise"].view(torch.int16))
    assert torch.equal(d1["noisy_actions"].view(torch.int16), d0["noisy_actions"].view(torch.int16))
    # the same checkpoint without the counter
    ck2 = tmp_path / "stripped"
    shutil.copytree(ck, ck2)
    osd = load_file(str(ck2 / "optimizer_state--3_checkpoint.safetensors"))
    assert int(osd.pop("diffusion_noise.call").item()) == 3
    save_file(osd, str(ck2 / "optimizer_state--3_checkpoint.safetensors"))
    e2 = fresh(world, dev)
    info = ft.load_training_checkpoint(ck2, 3, e2)
    assert info["optimizer"] and not info["diffusion_call"] and e2.diffusion.call == 0
    d2 = update(e2, 3, True)
    assert not torch.equal(d2["noise"].view(torch.int16), d0["noise"].view(torch.int16))
    dist_without = dist(e2, straight)
    print(f"resumed vs uninterrupted, rel-L2 over all trainable tensors: diffusion with the counter {dist_with:.3e}, without {dist_without:.3e}; "
          f"L1 objective on the same model {dist_l1:.3e}")
    assert dist_without > 5 * dist_with
    assert dist_with <= 2 * dist_l1        # 2x: the extra noisy-action projector path adds its own fp32-atomic weight gradients


def test_sampler_equals_the_host_loop_bit_for_bit(world, dev, monkeypatch):
    T = 5
    eng = fresh(world, dev, T=T)
    diffusion = load("openvla-oft_amd.diffusion")
    b = batch_of(world, 7, B=3)
    D, B = world["cfg"].llm_dim, 3
    X = torch.randn(B, 8, 7, generator=torch.Generator().manual_seed(9))
    got = eng.sample_actions(b, start_noise=X)
    assert got.is_cuda and got.dtype == BF and got.shape == (B, 8, 7)
    # OpenVLAForActionPrediction._infer's host loop on the same engine
    sched, enc = diffusion.DDIMScheduler(num_train_timesteps=T), diffusion.SinusoidalPositionalEncoding(D)
    sched.set_timesteps(T)
    cur = X.to(BF).float()
    cached = None
    for t in sched.timesteps:
        temb = enc(torch.tensor([float(t)])).to(BF).reshape(1, D).expand(B, D)
        out = eng.forward(b["input_ids"], b["attention_mask"], b["pixel_values"], b["labels"], proprio=b["proprio"], train=False, noisy_actions=cur.to(BF),
                          timestep_emb=temb, cached_patches=cached, sel="actions")
        cached = out["patches"]
        ah, _ = eng.action_hidden(out)
        eps = eng.head.fwd(ah)[0].reshape(cur.shape).float().cpu()
        cur = sched.step(eps, int(t), cur).prev_sample.to(BF).float()
    assert torch.isfinite(cur).all() and not torch.equal(cur, X.to(BF).float())
    assert torch.equal(got.float().cpu(), cur)
    # without start noise: stream 2 at the current call, the same bits twice, and the counter stays
    call = eng.diffusion.call
    a1, a2 = eng.sample_actions(b), eng.sample_actions(b)
    assert eng.diffusion.call == call and torch.equal(a1, a2) and not torch.equal(a1, got)
    ops, st = load("openvla-oft_amd.ops"), eng.diffusion
    start = ops.diffusion_noise(torch.zeros(B, 56, dtype=BF, device=dev), st.ab, st.temb_table, seed=SEED, call=call, stream=R.STREAM_SAMPLER)[0]
    lo, hi = R.bf16_bracket(R.normals(B, 56, call=call, seed=SEED, stream=R.STREAM_SAMPLER))
    got_start = bf16_bits_to_f32(to_bits(start)).astype(np.float64)
    assert ((got_start == lo) | (got_start == hi)).all()
    assert torch.equal(eng.sample_actions(b, start_noise=start.view(B, 8, 7)), a1)
    # one action label removed from one row: refused by check_action_labels before any launch
    bad, launches, lib = dict(b, labels=b["labels"].clone()), [], load("openvla-oft_amd._lib")
    bad["labels"][1, int((bad["labels"][1] > 31743).nonzero()[0])] = -100
    monkeypatch.setattr(lib, "call", lambda name, *a: launches.append(name))
    with pytest.raises(ValueError, match="row 1 holds 55 action labels"):
        eng.sample_actions(bad)
    assert not launches


def _driver_cfg(ft, tmp_path, **kw):
    base = dict(run_root_dir=tmp_path, dataset_name="libero_spatial_no_noops", batch_size=2, num_images_in_input=2, use_proprio=True, use_l1_regression=False,
                use_diffusion=True, num_diffusion_steps=5, max_steps=3, wandb_log_freq=1, save_freq=100, diffusion_sample_freq=2)
    return ft.FinetuneConfig(**{**base, **kw})


def test_driver_with_device_noise_logs_sampled_l1(world, dev, tmp_path):
    ft = load("openvla-oft_amd.vla_scripts.finetune")
    data = [batch_of(world, i) for i in range(3)]
    hist = ft.finetune(_driver_cfg(ft, tmp_path, use_val_set=True, val_freq=2), model_config=world["cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()},
                       log=lambda *_: None, dataset=iter(data), val_dataset=lambda: [batch_of(world, 20), batch_of(world, 21)], diffusion_noise="device")
    assert len(hist["loss_value"]) == 3 and all(np.isfinite(hist["loss_value"]))
    for k in ("curr_action_l1_loss", "next_actions_l1_loss"):            # batches 0 and 2 of 0, 1, 2
        assert len(hist[k]) == 2 and all(np.isfinite(hist[k])) and all(v > 0 for v in hist[k]), (k, hist[k])
    (step, val), = hist["val"]                                           # run_validation samples on every validation batch (finetune.py:735)
    assert step == 2 and val["val/num_batches"] == 2
    assert all(np.isfinite(val[k]) and val[k] > 0 for k in ("val/loss_value", "val/curr_action_l1_loss", "val/next_actions_l1_loss"))
    with pytest.raises(ValueError, match="use_diffusion"):
        ft.finetune(ft.FinetuneConfig(run_root_dir=tmp_path, use_l1_regression=True), model_config=world["cfg"], diffusion_noise="device")
    with pytest.raises(ValueError, match="diffusion_noise"):
        ft.finetune(_driver_cfg(ft, tmp_path), model_config=world["cfg"], diffusion_noise="gpu")


def test_driver_resume_continues_or_starts_the_stream(world, dev, tmp_path, monkeypatch):
    """finetune(resume=True, diffusion_noise="device"): the first draw after the resume is at the saved counter; a checkpoint without one (written
    with host noise) starts the stream at resume_step * grad_accumulation_steps, the lora_dropout rule."""
    from safetensors.torch import load_file, save_file

    ft, engine_mod = load("openvla-oft_amd.vla_scripts.finetune"), load("openvla-oft_amd.engine")
    seen = []
    orig = engine_mod.VLAEngine.draw_diffusion

    def recording(self, actions):
        seen.append(self.diffusion.call)
        return orig(self, actions)

    monkeypatch.setattr(engine_mod.VLAEngine, "draw_diffusion", recording)
    sd = lambda: {k: v.clone() for k, v in world["sd"].items()}  # noqa: E731
    data = lambda: iter([batch_of(world, i) for i in range(4)])  # noqa: E731
    ft.finetune(_driver_cfg(ft, tmp_path, save_freq=2, diffusion_sample_freq=100), model_config=world["cfg"], state_dict=sd(), log=lambda *_: None, dataset=data(),
                diffusion_noise="device")
    assert seen == [0, 1, 2]
    ck, = tmp_path.glob("*--2_chkpt")
    f = ck / "optimizer_state--2_checkpoint.safetensors"
    assert int(load_file(str(f))["diffusion_noise.call"].item()) == 3        # saved after the third draw
    resume = lambda: _driver_cfg(ft, tmp_path, resume=True, resume_step=2, vla_path=str(ck), max_steps=4, diffusion_sample_freq=100)  # noqa: E731
    seen.clear()
    ft.finetune(resume(), model_config=world["cfg"], state_dict=sd(), log=lambda *_: None, dataset=data(), diffusion_noise="device")
    assert seen[0] == 3
    osd = load_file(str(f))
    del osd["diffusion_noise.call"]
    save_file(osd, str(f))
    seen.clear()
    ft.finetune(resume(), model_config=world["cfg"], state_dict=sd(), log=lambda *_: None, dataset=data(), diffusion_noise="device")
    assert seen[0] == 2 * 1


def test_driver_with_host_noise_is_unchanged(world, dev, tmp_path):
    """diffusion_noise="host" (the default): no sampled-L1 histories, and the losses of the loop as it was -- make_diffusion's arithmetic restated
    here on an engine of the driver's configuration, step by step."""
    ft, config_mod, C, diffusion = (load("openvla-oft_amd." + m) for m in ("vla_scripts.finetune", "config", "prismatic.vla.constants", "diffusion"))
    engine_mod, weights_mod = load("openvla-oft_amd.engine"), load("openvla-oft_amd.weights")
    fcfg = _driver_cfg(ft, tmp_path)
    data = [batch_of(world, i) for i in range(3)]
    hist = ft.finetune(fcfg, model_config=world["cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()}, log=lambda *_: None, dataset=iter(data))
    assert "curr_action_l1_loss" not in hist and "next_actions_l1_loss" not in hist and len(hist["loss_value"]) == 3
    mc = config_mod.VLAConfig(**{**world["cfg"].__dict__, "num_images": 2, "lora_rank": fcfg.lora_rank, "lora_alpha": min(fcfg.lora_rank, 16),
                                 "action_dim": C.ACTION_DIM, "chunk": C.NUM_ACTIONS_CHUNK, "proprio_dim": C.PROPRIO_DIM,
                                 "norm_type": C.ACTION_PROPRIO_NORMALIZATION_TYPE.value})
    get, has = weights_mod.make_getter({k: v.clone() for k, v in world["sd"].items()}, dev)
    eng = engine_mod.VLAEngine(mc, get, dev, lora=True, use_proprio=True, head="diffusion", use_film=False, has=has)
    assert eng.diffusion is None
    sched, enc, gen = diffusion.DDIMScheduler(5), diffusion.SinusoidalPositionalEncoding(mc.llm_dim), torch.Generator().manual_seed(7)
    want = []
    eng.zero_grad()
    for i, b in enumerate(data):
        gt = b["actions"].to("cpu", torch.float32)
        noise = torch.randn(gt.shape, generator=gen).to(BF).float()
        ts = torch.randint(0, 5, (gt.shape[0],), generator=gen)
        d = dict(noise=noise, noisy_actions=sched.add_noise(gt, noise, ts).to(BF), timestep_emb=enc(ts.float()).to(BF))
        loss_sum, count, _ = eng.train_step_fwd_bwd(b, diffusion=d)
        eng.adamw_step(ft.learning_rate_at(fcfg, i))
        eng.refresh_derived()
        eng.zero_grad()
        want.append(loss_sum.item() / count)
    print(f"host-noise driver losses {hist['loss_value']} vs the restated loop {want}")
    # the loss sum and the weight gradients behind the later losses are accumulated with fp32 atomics: equal to rounding (the bound of the resume
    # tests, 2e-3 relative), not bit for bit
    assert np.allclose(hist["loss_value"], want, rtol=2e-3, atol=0)
