"""LoRA fine-tune driver (mirror of vla-scripts/finetune.py: FinetuneConfig :79-131, run_forward_pass :280-451,
save_training_checkpoint :584-675, finetune :763-1154) on the HIP engine.

  torchrun --standalone --nnodes 1 --nproc-per-node N -m ...   (one process per GPU, RCCL through torch.distributed)

What differs from the reference, deliberately:
  * the optimisation step runs the engine's fused path: explicit forward/backward kernels, gradients accumulated in flat
    fp32 buffers, one fused AdamW launch per dtype (same arithmetic as torch.optim.AdamW on bf16 / fp32 parameters), one
    large RCCL all-reduce per bucket instead of four DDP wrappers;
  * the frozen lm_head + cross-entropy the reference computes and discards in L1 mode is not executed;
  * the data source is pluggable: `dataset` is any iterable of collated batches (prismatic/util/data_utils.py:102-156
    layout).  The TF/RLDS pipeline is out of scope; without one, seeded synthetic
    LIBERO-shaped batches are used (`synthetic.make_batch`).
`run_forward_pass` keeps the reference signature and works through torch autograd for glue that wants it.
"""
from __future__ import annotations

import contextlib
import json
import math
import os
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Iterable, Optional, Tuple

import torch

from .. import synthetic
from ..config import OPENVLA_7B, VLAConfig
from ..dp import GradReducer
from ..engine import VLAEngine
from ..prismatic.training.train_utils import get_current_action_mask, get_next_actions_mask
from ..prismatic.vla import constants as C
from ..weights import load_lora_adapter, make_getter, random_state_dict, save_lora_adapter, vision_backbone_keys_from_reference


@dataclass
class FinetuneConfig:
    # fmt: off
    vla_path: str = "openvla/openvla-7b"
    data_root_dir: Path = Path("datasets/rlds")
    dataset_name: str = "aloha_scoop_x_into_bowl"
    run_root_dir: Path = Path("runs")
    shuffle_buffer_size: int = 100_000
    use_l1_regression: bool = True
    use_diffusion: bool = False
    num_diffusion_steps: int = 50
    use_film: bool = False
    num_images_in_input: int = 1
    use_proprio: bool = False
    batch_size: int = 8
    learning_rate: float = 5e-4
    lr_warmup_steps: int = 0
    num_steps_before_decay: int = 100_000
    grad_accumulation_steps: int = 1
    max_steps: int = 200_000
    use_val_set: bool = False
    val_freq: int = 10_000
    val_time_limit: int = 180
    save_freq: int = 10_000
    save_latest_checkpoint_only: bool = False
    resume: bool = False
    resume_step: Optional[int] = None
    image_aug: bool = True
    diffusion_sample_freq: int = 50
    use_lora: bool = True
    lora_rank: int = 32
    lora_dropout: float = 0.0
    merge_lora_during_training: bool = True
    wandb_entity: str = "your-wandb-entity"
    wandb_project: str = "your-wandb-project"
    run_id_note: Optional[str] = None
    run_id_override: Optional[str] = None
    wandb_log_freq: int = 10
    # fmt: on


def remove_ddp_in_checkpoint(state_dict) -> dict:
    """finetune.py:134-156"""
    return {(k[7:] if k.startswith("module.") else k): v for k, v in state_dict.items()}


def get_run_id(cfg) -> str:
    """finetune.py:159-190"""
    if cfg.run_id_override is not None:
        return cfg.run_id_override
    if cfg.resume:
        run_id = cfg.vla_path.split("/")[-1]
        if "chkpt" in run_id.split("--")[-1]:
            run_id = "--".join(run_id.split("--")[:-1])
        return run_id
    run_id = f"{cfg.vla_path.split('/')[-1]}+{cfg.dataset_name}+b{cfg.batch_size * cfg.grad_accumulation_steps}+lr-{cfg.learning_rate}"
    if cfg.use_lora:
        run_id += f"+lora-r{cfg.lora_rank}+dropout-{cfg.lora_dropout}"
    if cfg.image_aug:
        run_id += "--image_aug"
    if cfg.run_id_note is not None:
        run_id += f"--{cfg.run_id_note}"
    return run_id


def dropout_seed_for_rank(rank: int) -> int:
    """The 64-bit Philox key of the lora_dropout masks: the rank in the high word, so every data-parallel rank draws different masks
    (each rank's nn.Dropout has its own generator state in the reference, too)."""
    return 7 + (int(rank) << 32)


def diffusion_seed_for_rank(rank: int) -> int:
    """The 64-bit Philox key of the device diffusion noise (finetune(diffusion_noise="device")): the rank in the high word like
    dropout_seed_for_rank, another low word, so the noise shares no generator output with the lora_dropout masks."""
    return 0xD1FF + (int(rank) << 32)


def learning_rate_at(cfg, gradient_step_idx: int) -> float:
    """MultiStepLR(milestones=[num_steps_before_decay], gamma=0.1) + optional linear warm-up 10% -> 100%
    (finetune.py:958-962, 1094-1098).  The step index is the number of optimizer steps already taken."""
    lr = cfg.learning_rate * (0.1 if gradient_step_idx >= cfg.num_steps_before_decay else 1.0)
    if cfg.lr_warmup_steps > 0:
        progress = min((gradient_step_idx + 1) / cfg.lr_warmup_steps, 1.0)
        lr = cfg.learning_rate * (0.1 + 0.9 * progress)
    return lr


def ema_decay_at(k: int, *, max_decay: float, power: Optional[float] = 0.75, inv_gamma: float = 1.0, update_after: int = 0) -> float:
    """The decay of the k-th EMA update (k counts from 1), in double precision: the warm-up of diffusers' EMAModel.get_decay, which Diffusion
    Policy trains with -- 0 while step = k - update_after - 1 <= 0 (the shadow goes all the way to the parameters), then
    min(max_decay, 1 - (1 + step / inv_gamma) ** -power); `power=None` is the constant decay max_decay.  diffusers is not installed here:
    restated from its published formula, PARITY UNPINNED against the library.  The reference (vla-scripts/finetune.py) has no EMA."""
    step = k - update_after - 1
    if step <= 0:
        return 0.0
    if power is None:
        return float(max_decay)
    return min(float(max_decay), 1.0 - (1.0 + step / inv_gamma) ** (-power))


def run_diffusion_sampling(vla, action_head, noisy_action_projector, proprio_projector, batch, batch_size, num_patches, actions_shape, device_id,
                           current_action_mask, next_actions_mask, use_proprio, use_film) -> torch.Tensor:
    """finetune.py:454-540: reverse diffusion for the whole batch -- start from N(0, 1) noise, and for every DDIM timestep predict the
    noise from the action rows of the VLM's last hidden state and step x_t -> x_{t-1}.  The reference re-runs the vision backbone in every
    step; its output does not depend on t, so here the projected patches of the first step are reused (same numbers, one tower pass).
    METRICS-ONLY deviation from the reference's arithmetic (this function feeds the logged diffusion L1 numbers, never a gradient): the start
    noise is drawn on the host and `scheduler.step` runs there in fp32 on the bf16-rounded sample, rounding to bf16 once per step, where the
    reference keeps `curr_noisy_actions` / `noise_pred` in bf16 on the device throughout (finetune.py:490-540); `predict_action`'s diffusion
    branch (modeling.py) is the deployment path and rounds where the reference does.  The per-step `.cpu()` is one host sync per DDIM step."""
    head, eng = action_head.module, vla.module.engine
    cfg = eng.cfg
    A = cfg.num_action_tokens
    cur = torch.randn((batch_size, C.NUM_ACTIONS_CHUNK, C.ACTION_DIM)).to(torch.bfloat16)
    head.noise_scheduler.set_timesteps(head.num_diffusion_steps)
    cached = None
    for t in head.noise_scheduler.timesteps:
        temb = head.time_encoder(torch.full((batch_size,), float(t))).to(torch.bfloat16).unsqueeze(1)          # (B, 1, llm_dim)
        out = eng.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"],
                          proprio=batch["proprio"] if use_proprio else None, train=False, noisy_actions=cur, timestep_emb=temb,
                          proprio_projector=proprio_projector.module.comp if use_proprio else None,
                          noisy_action_projector=noisy_action_projector.module.comp, cached_patches=cached, sel="actions")
        cached = out["patches"]
        ah, _ = eng.action_hidden(out)
        noise_pred = head.predict_noise(ah.view(batch_size, A, cfg.llm_dim)).reshape(cur.shape).float().cpu()
        cur = head.noise_scheduler.step(noise_pred, t, cur.float()).prev_sample.to(torch.bfloat16)
    return cur.reshape(actions_shape).to(device_id)


def run_forward_pass(vla, action_head, noisy_action_projector, proprio_projector, batch, action_tokenizer, device_id, use_l1_regression,
                     use_diffusion, use_proprio, use_film, num_patches, compute_diffusion_l1=False, num_diffusion_steps=None
                     ) -> Tuple[torch.Tensor, Dict[str, float]]:
    """finetune.py:280-451 with the reference's signature and all three objectives, through the autograd bridge of modeling.py
    (`loss.backward()` then drives the engine's explicit backward):
      discrete (neither head flag)   loss = output.loss (next-token cross entropy), token accuracies and decoded L1 of the current /
                                     next actions from output.logits[:, num_patches:-1].argmax(2)                       (:357-378)
      use_l1_regression              L1Loss(gt, head.predict_action(action rows))                                       (:396-400)
      use_diffusion                  MSE(noise_pred, noise); with compute_diffusion_l1 additionally a full DDIM sampling
                                     (run_diffusion_sampling) for the current / next L1 metrics                         (:402-430)"""
    metrics: Dict[str, float] = {}
    gt = batch["actions"].to(device_id).to(torch.bfloat16)
    noisy = None
    if use_diffusion:                                                                   # :327-333
        noisy = action_head.module.sample_noisy_actions(gt)
    output = vla(input_ids=batch["input_ids"], attention_mask=batch["attention_mask"], pixel_values=batch["pixel_values"], labels=batch["labels"],
                 output_hidden_states=True, proprio=batch["proprio"] if use_proprio else None,
                 proprio_projector=proprio_projector if use_proprio else None, use_film=use_film,
                 noisy_actions=noisy["noisy_actions"] if use_diffusion else None,
                 noisy_action_projector=noisy_action_projector if use_diffusion else None,
                 diffusion_timestep_embeddings=noisy["diffusion_timestep_embeddings"] if use_diffusion else None)
    ids = batch["labels"][:, 1:].to(device_id)
    cur, nxt = get_current_action_mask(ids), get_next_actions_mask(ids)
    if not (use_l1_regression or use_diffusion):                                        # :357-378
        from ..prismatic.training.train_utils import compute_actions_l1_loss, compute_token_accuracy

        loss = output.loss
        predicted = output.logits[:, num_patches:-1].argmax(dim=2)
        metrics["loss_value"] = loss.item()
        for name, m in (("curr_action", cur), ("next_actions", nxt)):
            metrics[f"{name}_accuracy"] = compute_token_accuracy(predicted, ids, mask=m).item()
            metrics[f"{name}_l1_loss"] = compute_actions_l1_loss(action_tokenizer, predicted, ids, mask=m).item()
        return loss, metrics
    last = output.hidden_states[-1]
    text_hidden = last[:, num_patches:-1]
    B = batch["input_ids"].shape[0]
    ah = text_hidden[cur | nxt].reshape(B, C.NUM_ACTIONS_CHUNK * C.ACTION_DIM, -1).to(torch.bfloat16)
    pred = None
    if use_l1_regression:
        pred = action_head.module.predict_action(ah)
        loss = torch.nn.L1Loss()(gt, pred)
    if use_diffusion:                                                                   # :402-430
        noise_pred = action_head.module.predict_noise(ah).reshape(noisy["noise"].shape)
        loss = torch.nn.functional.mse_loss(noise_pred, noisy["noise"].to(noise_pred.device), reduction="mean")
        if compute_diffusion_l1:
            with torch.no_grad():
                pred = run_diffusion_sampling(vla, action_head, noisy_action_projector, proprio_projector, batch, B, num_patches, gt.shape, device_id,
                                              cur, nxt, use_proprio, use_film)
    metrics["loss_value"] = loss.item()
    if pred is not None:                                                                # :437-448 (should_log_l1_loss)
        metrics["curr_action_l1_loss"] = torch.nn.L1Loss()(gt[:, 0], pred[:, 0]).item()
        metrics["next_actions_l1_loss"] = torch.nn.L1Loss()(gt[:, 1:], pred[:, 1:]).item()
    return loss, metrics


_COMPONENT_PREFIXES = {"proprio_projector": "proprio_projector.", "noisy_action_projector": "noisy_action_projector.", "action_head": "action_head.",
                       "action_scale_head": "action_scale_head.",   # the learned Laplace scale (finetune(action_scale="fit")); absent without it
                       "vision_backbone": "vision_backbone."}   # FiLM scale/shift Linears (finetune.py:640-645 saves the wrapped backbone)


def save_training_checkpoint(run_dir: Path, log_step: int, engine: VLAEngine, dataset_statistics: Optional[dict], rank: int,
                             latest_only: bool = False, save_optimizer: bool = True, into: Optional[Path] = None) -> Path:
    """finetune.py:584-675: `{component}--{step}_checkpoint.pt` (+ `lora_adapter/` in peft's format, `dataset_statistics.json`).
    The LoRA merge of the reference (:663-675) is the separate merge_lora_weights_and_save step.  Beyond the reference:
    `optimizer_state--{step}_checkpoint.safetensors` (AdamW moments + step counters), so a resumed run continues the same
    trajectory instead of restarting the moments from zero.
    With weight EMA enabled (VLAEngine.enable_ema) that file also carries the shadows and the EMA step, and rank 0 writes a second complete
    fine-tune output directory `ckpt / "ema"` with the averaged weights (inside engine.ema_weights(), no optimizer state; `into` names it): every
    loader takes it as it takes `ckpt`, and as a sub-directory it leaves find_checkpoint_file's one-match rule for the live files alone.  Called
    inside an ema_weights() scope, this writes the averaged weights as `ckpt` and no sub-directory."""
    ckpt = run_dir if latest_only else Path(str(run_dir) + f"--{log_step}_chkpt")
    if into is not None:
        ckpt = Path(into)
    suffix = "latest_checkpoint" if latest_only else f"{log_step}_checkpoint"
    if rank == 0:
        (ckpt / "lora_adapter").mkdir(parents=True, exist_ok=True)
        if dataset_statistics is not None:
            (ckpt / "dataset_statistics.json").write_text(json.dumps(dataset_statistics))
        exp = {k: v.detach().to("cpu") for k, v in engine.export_trainable("data").items()}
        save_lora_adapter(ckpt / "lora_adapter", exp, r=engine.cfg.lora_rank, lora_alpha=engine.cfg.lora_alpha,
                          lora_dropout=engine.dropout.p)   # peft on-disk format
        for comp, prefix in _COMPONENT_PREFIXES.items():
            if comp == "vision_backbone":
                continue
            sd = {k[len(prefix):]: v.contiguous() for k, v in exp.items() if k.startswith(prefix) and ".lora_" not in k}
            if sd:
                torch.save(sd, ckpt / f"{comp}--{suffix}.pt")
        if engine.use_film:
            # finetune.py:640-655: the whole FiLM-wrapped backbone (frozen towers + their adapters + scale / shift), in the reference's key layout,
            # so that get_vla(cfg.use_film) -- here or in the reference -- finds what _apply_film_to_vla loads (openvla_utils.py:311-349)
            torch.save({k: v.detach().to("cpu").contiguous() for k, v in engine.vision_backbone_state_dict().items()}, ckpt / f"vision_backbone--{suffix}.pt")
        if save_optimizer:
            from safetensors.torch import save_file

            save_file({k: v.detach().to("cpu").contiguous() for k, v in engine.optimizer_state_dict().items()},
                      str(ckpt / f"optimizer_state--{suffix}.safetensors"))
        if engine.ema_enabled and not engine.in_ema_scope:
            with engine.ema_weights():
                save_training_checkpoint(run_dir, log_step, engine, dataset_statistics, rank, latest_only, save_optimizer=False, into=ckpt / "ema")
    return ckpt


def load_training_checkpoint(ckpt: Path, log_step: Optional[int], engine: VLAEngine, load_optimizer: bool = True, log=None) -> dict:
    """Resume (finetune.py:134-156 `load_checkpoint(module_name, path, step)` per component + the lora adapter the reference
    re-attaches through its merged checkpoint): reads `{component}--{step}_checkpoint.pt` (`latest` when step is None), the
    peft adapter directory and, if present, the optimizer state, which also carries the lora_dropout mask stream's `call` counter
    (`dropout_call` in the result: False when the checkpoint has none) and, for an engine with device diffusion noise, that stream's
    (`diffusion_call`).  Only `weights_only=True` / safetensors loaders are used."""
    ckpt = Path(ckpt)
    suffix = "latest_checkpoint" if log_step is None else f"{log_step}_checkpoint"
    sd: Dict[str, torch.Tensor] = {}
    adapter_dir = ckpt / "lora_adapter"
    if adapter_dir.is_dir():
        adapter, _ = load_lora_adapter(adapter_dir)
        sd.update(adapter)
    for comp, prefix in _COMPONENT_PREFIXES.items():
        f = ckpt / f"{comp}--{suffix}.pt"
        if f.is_file():
            part = remove_ddp_in_checkpoint(torch.load(str(f), weights_only=True, map_location="cpu"))
            if comp == "vision_backbone":    # reference key layout (or the FiLM-only files of earlier rounds); only the trainable tensors are taken
                part = vision_backbone_keys_from_reference(part)
                sd.update({k: v for k, v in part.items() if ".lora_" in k or ".scale." in k or ".shift." in k})
            else:
                sd.update({prefix + k: v for k, v in part.items()})
    missing = engine.load_trainable(sd, strict=False)
    opt = ckpt / f"optimizer_state--{suffix}.safetensors"
    loaded_opt = has_call = has_noise_call = False
    if load_optimizer and opt.is_file():
        from safetensors.torch import load_file

        osd = load_file(str(opt))
        engine.load_optimizer_state_dict(osd, log=log)   # raises for an fp32-state file and an engine in the default mode (and says how to load it)
        loaded_opt, has_call, has_noise_call = True, "lora_dropout.call" in osd, "diffusion_noise.call" in osd
    return {"missing": missing, "optimizer": loaded_opt, "tensors": len(sd), "dropout_call": has_call, "diffusion_call": has_noise_call}


def load_ema_state(ckpt: Path, log_step: Optional[int], engine: VLAEngine) -> bool:
    """Reads the weight-EMA shadows and step of a checkpoint's optimizer-state file into an engine that has EMA enabled (the resume load runs
    before enable_ema, so it cannot).  False -- and nothing is changed -- when the file is absent or holds no `ema.` entry."""
    suffix = "latest_checkpoint" if log_step is None else f"{log_step}_checkpoint"
    opt = Path(ckpt) / f"optimizer_state--{suffix}.safetensors"
    if not opt.is_file():
        return False
    from safetensors import safe_open

    with safe_open(str(opt), framework="pt", device="cpu") as f:
        ema = {k: f.get_tensor(k) for k in f.keys() if k.startswith("ema.")}
    return engine.load_ema_state_dict(ema)


def load_grad_clip_state(ckpt: Path, log_step: Optional[int], engine: VLAEngine) -> bool:
    """Reads the `grad_clip.` counters of a checkpoint's optimizer-state file into an engine that has gradient clipping enabled (the resume
    load runs before enable_grad_clip).  False -- and nothing is changed -- when the file is absent or holds none."""
    suffix = "latest_checkpoint" if log_step is None else f"{log_step}_checkpoint"
    opt = Path(ckpt) / f"optimizer_state--{suffix}.safetensors"
    if not opt.is_file():
        return False
    from safetensors import safe_open

    with safe_open(str(opt), framework="pt", device="cpu") as f:
        sd = {k: f.get_tensor(k) for k in f.keys() if k.startswith("grad_clip.")}
    return engine.load_grad_clip_state_dict(sd)


def sampled_l1_metrics(engine: VLAEngine, batch: dict) -> Dict[str, float]:
    """finetune.py:410-448 for the diffusion objective: a chunk sampled by the whole reverse diffusion (VLAEngine.sample_actions, no host round
    trip between its steps) against the ground truth -- L1 of chunk step 0 and of the rest.  The two `.item()` are the only synchronisation."""
    pred = engine.sample_actions(batch).float()
    gt = batch["actions"].to(pred.device, torch.bfloat16).float().reshape(pred.shape)
    return {"curr_action_l1_loss": torch.nn.L1Loss()(gt[:, 0], pred[:, 0]).item(), "next_actions_l1_loss": torch.nn.L1Loss()(gt[:, 1:], pred[:, 1:]).item()}


def tensor_stats_group(name: str) -> str:
    """The owning module of a trainable tensor, the key of history["tensor_stats"]: each decoder layer, each vision tower, the projector
    and each head-side store (proprio_projector, action_head, noisy_action_projector) by the first component of its name."""
    m = re.match(r"language_model\.model\.layers\.\d+", name)
    if m:
        return m.group(0)
    for tower in ("vision_backbone.fused_featurizer", "vision_backbone.featurizer"):
        if name.startswith(tower + "."):
            return tower
    return name.split(".", 1)[0]


def group_tensor_stats(table: Dict[str, Dict[str, float]]) -> Dict[str, Dict[str, float]]:
    """VLAEngine.tensor_stats() summed per tensor_stats_group: the group norms are the square roots of the summed squares (NaN and inf
    propagate), grad_absmax the maximum, n_nonfinite the sum."""
    groups: Dict[str, Dict[str, float]] = {}
    for name, s in table.items():
        g = groups.setdefault(tensor_stats_group(name), {"grad_norm": 0.0, "param_norm": 0.0, "grad_absmax": 0.0, "n_nonfinite": 0})
        g["grad_norm"] += s["grad_norm"] * s["grad_norm"]
        g["param_norm"] += s["param_norm"] * s["param_norm"]
        g["grad_absmax"] = max(g["grad_absmax"], s["grad_absmax"])
        g["n_nonfinite"] += s["n_nonfinite"]
    for g in groups.values():
        g["grad_norm"], g["param_norm"] = math.sqrt(g["grad_norm"]), math.sqrt(g["param_norm"])
    return groups


def run_validation(engine: VLAEngine, cfg: FinetuneConfig, val_batches: Iterable[dict], log_step: int, log, *, discrete: bool, make_diffusion=None,
                   metric_fn=None, sample_l1: bool = False) -> Dict[str, float]:
    """finetune.py:678-760: the training loss (and, for the discrete objective, the token metrics; with `sample_l1`, the diffusion objective's
    sampled L1 of every batch, :735) on the validation loader without gradients, cut short after `cfg.val_time_limit` seconds, averaged over
    the batches seen, logged with a `val/` prefix."""
    import time

    start, rows = time.time(), []
    for batch in val_batches:
        if not cfg.use_proprio:
            batch = {**batch, "proprio": None}
        loss_sum, count, pred = engine.eval_step(batch, diffusion=make_diffusion(batch) if make_diffusion else None, discrete=discrete)
        m = {"loss_value": loss_sum.item() / count}
        if metric_fn is not None:
            m.update(metric_fn(batch, pred))
        if sample_l1:
            m.update(sampled_l1_metrics(engine, batch))
        m["loss"] = m["loss_value"]
        rows.append(m)
        if time.time() - start > cfg.val_time_limit:
            break
    if not rows:
        return {}
    avg = {f"val/{k}": sum(r[k] for r in rows) / len(rows) for k in rows[0]}
    avg["val/num_batches"] = len(rows)
    log(f"step {log_step}: " + " ".join(f"{k} {v:.5f}" for k, v in avg.items()))
    return avg


def finetune(cfg: FinetuneConfig, *, model_config: VLAConfig = OPENVLA_7B, state_dict: Optional[Dict[str, torch.Tensor]] = None,
             dataset: Optional[Iterable[dict]] = None, dataset_statistics: Optional[dict] = None, log=print, tokenizer=None,
             val_dataset=None, diffusion_noise: str = "host", ema_decay: Optional[float] = None, ema_power: Optional[float] = 0.75,
             ema_inv_gamma: float = 1.0, ema_update_after: int = 0, max_grad_norm: Optional[float] = None,
             skip_nonfinite_steps: bool = True, optimizer_state: str = "param", tensor_stats_freq: Optional[int] = None,
             action_scale: Optional[str] = None, init_action_scale=0.1, action_scale_bounds=(-6.0, 1.0)) -> Dict[str, list]:
    """finetune.py:763-1154.  Returns the logged metric history.  Data source, in this order: `dataset` (any iterable of collated
    batches); an episode store at `cfg.data_root_dir / cfg.dataset_name` (prismatic/vla/datasets/rlds_free.py: the reference's
    RLDSDataset + RLDSBatchTransform + collator, finetune.py:981-1016, with the frames augmented and normalised on the device --
    needs `tokenizer(text) -> ids` or tokenizer files under `cfg.vla_path`); otherwise seeded synthetic batches of the recipe's shape.
    `diffusion_noise` (diffusion objective only): "host" draws noise and timesteps from a CPU torch.Generator, which waits for the device on
    every step and whose state no checkpoint holds; "device" draws them in one launch (VLAEngine.draw_diffusion) from a counter saved with the
    optimizer state, so a resumed run continues the uninterrupted one's noise, and every `cfg.diffusion_sample_freq` batches (and on every
    validation batch) samples a chunk (VLAEngine.sample_actions) for `curr_action_l1_loss` / `next_actions_l1_loss` (finetune.py:1053, :410-448).
    `ema_decay` in [0, 1) switches on the weight EMA the reference lacks (diffusers' EMAModel; Diffusion Policy evaluates on it): fp32 shadows of
    the trainable buffers, updated on the device after every optimizer step (not per micro-batch) with the decay ema_decay_at(k, max_decay=ema_decay,
    power=ema_power, inv_gamma=ema_inv_gamma, update_after=ema_update_after).  Validation -- its sampled L1 included, under the same `val/` keys
    -- runs on the averaged weights, the training-time sampling stays on the live ones; every checkpoint holds the shadows (optimizer-state
    file, so a resumed run continues shadow and schedule) and an `ema/` sub-directory that serves and merges like any fine-tune output.  The
    shadows are rank-local: the parameters are identical on every rank after the all-reduced step, so the shadows are too, and nothing is
    communicated.  With `ema_decay=None` nothing of this runs.
    `max_grad_norm` clips the global norm of the gradients (every trainable tensor, after the all-reduce and the 1 / world scaling, in the
    parameter's precision) as torch.nn.utils.clip_grad_norm_ does, and `skip_nonfinite_steps` makes a step whose norm is NaN or Inf a no-op for
    parameters and AdamW moments -- both on the device, in front of the fused AdamW (VLAEngine.enable_grad_clip), with no readback: the
    host does not learn of a skip, so a skipped step still consumes its step number in the bias correction and the LR schedule, and the EMA
    update after it averages the unchanged parameters.  `max_grad_norm=None` with the guard on means the guard alone (max_norm = inf); with the
    guard off as well nothing of this runs.  When it runs, the logging steps read the statistics back (the host waits there anyway) and the
    history gains `grad_norm`, `grad_clip_coef` (both of that step) and `skipped_steps` (the running count); the optimizer-state file gains
    the counters `grad_clip.steps / clipped / skipped`, which a resumed run continues.
    `optimizer_state`: "param" keeps the AdamW state of the bf16 trainables (LoRA factors, action head) in bf16 exactly as torch.optim.AdamW does;
    "fp32" gives them an fp32 master copy and fp32 moments (VLAEngine.enable_fp32_optimizer_state, +8 bytes per element), switched on before the
    resume load, the EMA and the clipping: the second moment then decays, updates below half a bf16 ulp accumulate, the EMA follows the master
    and the norm is taken over the unrounded gradient.  The model checkpoints keep their format (they hold bf16_rne(master)); the
    optimizer-state file holds fp32 moments and `store{i}.bf16.master`, and loads only into an "fp32" run, while an "fp32" run resumes from a
    "param" checkpoint by widening.  The master is rank-local and identical on every rank; with the default OVLA_DP_COMM_DTYPE=param the reduced
    gradient of the bf16 buffers has passed through a bf16 wire, OVLA_DP_COMM_DTYPE=fp32 keeps it in full precision.
    `tensor_stats_freq=k` (k >= 1; None: nothing of this runs) collects, on the optimizer steps with log_step % k == 0, the per-tensor
    statistics of VLAEngine.collect_tensor_stats -- gradient norm as AdamW sees it, parameter norm, largest finite |gradient|, non-finite count
    of every trainable tensor -- on the device, between the reducer and the optimizer step, one launch pair per flat buffer and no readback.
    A logging step after a collection reads the records back once: history gains `tensor_stats`, a list of (collected step, {group: {grad_norm,
    param_norm, grad_absmax, n_nonfinite}}) per owning module (tensor_stats_group), and `nonfinite_tensors`, the sorted names whose gradient
    has been non-finite on a collected step so far; rank 0 appends one JSON line {"step", "tensors": {name: {...}}} with the full table to
    `run_dir/tensor_stats.jsonl`.  With the step guard on, a log line whose skipped count rose names up to three tensors whose n_bad_steps
    rose with it.  The statistics are rank-local and identical on every rank (they are taken of the reduced gradient), so only rank 0 writes.
    The n_bad_steps counters are NOT checkpointed: they restart at 0 on resume.
    `action_scale="fit"` (L1 objective only; None: nothing of this runs) attaches the learned Laplace scale head (VLAEngine.attach_scale_head with
    `init_action_scale`, a scalar or one value per action dimension, and `action_scale_bounds`, the clamp of its log-scale) before the resume
    load and before fp32 state, EMA, clipping and tensor statistics are enabled, and fits it by maximum likelihood on the demonstrations beside
    the L1 step (train_step_fwd_bwd(fit_scale=True): three small launches after each backward).  Its gradient stops at the head's hidden
    output: loss, LoRA factors and action head keep the bits of a run without it, as long as `max_grad_norm` does not clip -- the global norm
    counts the scale head's gradient too.  The history gains `scale_nll` (mean negative log-likelihood per chunk step) and `action_scale` (mean
    b) at the logging steps; checkpoints gain `action_scale_head--{step}_checkpoint.pt` (what vla.load_scale_head reads) and the
    optimizer-state file its moments, and a resumed run continues both."""
    if action_scale not in (None, "fit"):
        raise ValueError(f'action_scale = {action_scale!r} (None or "fit")')
    if action_scale is not None and not cfg.use_l1_regression:
        raise ValueError('action_scale="fit" fits the Laplace scale of the L1 head: it needs cfg.use_l1_regression (not the diffusion or the discrete objective)')
    fit_scale = action_scale == "fit"
    if tensor_stats_freq is not None and (isinstance(tensor_stats_freq, bool) or not isinstance(tensor_stats_freq, int) or tensor_stats_freq < 1):
        raise ValueError(f"tensor_stats_freq = {tensor_stats_freq!r} (an integer >= 1, or None)")
    if optimizer_state not in ("param", "fp32"):
        raise ValueError(f'optimizer_state = {optimizer_state!r} ("param" or "fp32")')
    if max_grad_norm is not None and not float(max_grad_norm) > 0.0:   # NaN fails the comparison too
        raise ValueError(f"max_grad_norm = {max_grad_norm} (a positive number, or None)")
    grad_clip = max_grad_norm is not None or bool(skip_nonfinite_steps)
    if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
        raise ValueError(f"ema_decay = {ema_decay} is outside [0, 1)")
    if diffusion_noise not in ("host", "device"):
        raise ValueError(f'diffusion_noise = {diffusion_noise!r} ("host" or "device")')
    device_noise = diffusion_noise == "device"
    if device_noise and not cfg.use_diffusion:
        raise ValueError('diffusion_noise="device" needs cfg.use_diffusion: the other objectives draw no noise')
    assert cfg.use_lora, "Only LoRA fine-tuning is supported. Please set --use_lora=True!"
    assert not (cfg.use_l1_regression and cfg.use_diffusion), "Cannot do both L1 regression and diffusion. Please pick one of them!"
    discrete = not (cfg.use_l1_regression or cfg.use_diffusion)    # next-token cross entropy on the action tokens (finetune.py:357-378)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist

    if world > 1 and not dist.is_initialized():
        dist.init_process_group("nccl", device_id=dev)
    run_dir = cfg.run_root_dir / get_run_id(cfg)
    if rank == 0:
        os.makedirs(run_dir, exist_ok=True)
    model_config = VLAConfig(**{**model_config.__dict__, "num_images": cfg.num_images_in_input, "lora_rank": cfg.lora_rank,
                                "lora_alpha": min(cfg.lora_rank, 16), "action_dim": C.ACTION_DIM, "chunk": C.NUM_ACTIONS_CHUNK,
                                "proprio_dim": C.PROPRIO_DIM, "norm_type": C.ACTION_PROPRIO_NORMALIZATION_TYPE.value})
    if state_dict is None:
        log(f"[finetune] no checkpoint at `{cfg.vla_path}` is loadable offline: using seeded random weights of the architecture")
        state_dict = random_state_dict(model_config, dev, seed=0, lm_head=discrete, film=cfg.use_film, diffusion=cfg.use_diffusion)
    get, has = make_getter(state_dict, dev)
    engine = VLAEngine(model_config, get, dev, lora=True, use_proprio=cfg.use_proprio, head="none" if discrete else ("diffusion" if cfg.use_diffusion else "l1"),
                       use_film=cfg.use_film, has=has, lora_dropout=cfg.lora_dropout, dropout_seed=dropout_seed_for_rank(rank),
                       **(dict(num_diffusion_steps=cfg.num_diffusion_steps, diffusion_seed=diffusion_seed_for_rank(rank)) if device_noise else {}))
    if cfg.use_diffusion:   # DiffusionActionHead.sample_noisy_actions (action_heads.py:167-197), host side
        from ..diffusion import DDIMScheduler, SinusoidalPositionalEncoding

        sched, time_enc = DDIMScheduler(cfg.num_diffusion_steps), SinusoidalPositionalEncoding(model_config.llm_dim)
        noise_gen = torch.Generator().manual_seed(7 + rank)
    if fit_scale:   # its store joins engine.stores: before everything below that enumerates them
        engine.attach_scale_head(init_action_scale, bounds=action_scale_bounds)
    log(f"# total trainable params: {engine.num_trainable()}")
    if optimizer_state == "fp32":   # before the resume load (which then fills master and fp32 moments), the EMA shadows and the clip state
        engine.enable_fp32_optimizer_state()
        log(f"[finetune] optimizer_state=fp32: fp32 master weights and AdamW moments for the bf16 trainables, +{engine.fp32_optimizer_state_bytes()} bytes")
    else:
        log("[finetune] optimizer_state=param: AdamW state in each parameter's dtype")
    if cfg.resume:   # finetune.py:193-209: the trainable components come from the checkpoint directory `vla_path` at `resume_step`
        assert cfg.resume_step is not None, "resume=True needs resume_step"
        info = load_training_checkpoint(Path(cfg.vla_path), cfg.resume_step, engine, log=log)
        if not info["dropout_call"]:   # a checkpoint from before the counter was saved was trained with dropout ignored: there is no mask stream to
            # continue, only one to start; start it at a position that depends on the step, so two resumes at different steps do not share masks
            engine.dropout.call = (cfg.resume_step * cfg.grad_accumulation_steps) & 0xFFFFFFFF
        if device_noise and not info["diffusion_call"]:   # the same rule for the noise stream of a checkpoint written with host noise
            engine.diffusion.call = (cfg.resume_step * cfg.grad_accumulation_steps) & 0xFFFFFFFF
        log(f"[finetune] resumed step {cfg.resume_step} from {cfg.vla_path}: {info['tensors']} tensors, optimizer state: {info['optimizer']}, "
            f"{len(info['missing'])} trainable tensors kept at their initial values")
    if ema_decay is not None:
        engine.enable_ema()
        if cfg.resume:   # the shadows are allocated after the load: read the optimizer-state file's ema.* entries now, if it has them
            resumed_ema = load_ema_state(Path(cfg.vla_path), cfg.resume_step, engine)
            log(f"[finetune] weight EMA continues at update {engine.ema_step}" if resumed_ema else
                "[finetune] the checkpoint holds no EMA state (trained without ema_decay): the shadow starts at the loaded parameters, ema_step = 0")
    if grad_clip:
        engine.enable_grad_clip(math.inf if max_grad_norm is None else float(max_grad_norm), skip_nonfinite=bool(skip_nonfinite_steps))
        if cfg.resume:   # allocated after the load, like the EMA shadows: read the optimizer-state file's grad_clip.* counters now
            resumed_clip = load_grad_clip_state(Path(cfg.vla_path), cfg.resume_step, engine)
            log(f"[finetune] gradient clipping continues its counters: {engine.grad_clip_stats()}" if resumed_clip else
                "[finetune] the checkpoint holds no grad_clip counters: they start at 0")
    if tensor_stats_freq is not None:
        engine.enable_tensor_stats()
    reducer = GradReducer(engine.stores, world) if world > 1 else None
    engine.attach_reducer(reducer, overlap=cfg.grad_accumulation_steps == 1 and os.environ.get("OVLA_DP_OVERLAP", "1") != "0")   # overlap only when every backward ends a step
    if dataset is None and (Path(cfg.data_root_dir) / cfg.dataset_name).is_dir():
        from ..prismatic.vla import datasets as D
        from ..prismatic.vla.action_tokenizer import ActionTokenizer

        if tokenizer is None:
            from transformers import AutoTokenizer   # tokenizer files inside the checkpoint directory

            tok = AutoTokenizer.from_pretrained(cfg.vla_path)
            tokenizer = lambda text: tok(text, add_special_tokens=True).input_ids  # noqa: E731
        vocab = type("Vocab", (), {"vocab_size": model_config.vocab - model_config.pad_to_multiple_of})()   # 32000 (constants.py / modeling_prismatic.py:732)
        side = model_config.dino.image_size
        train_dataset = D.EpisodeDataset(cfg.data_root_dir, cfg.dataset_name,
                                         D.RLDSBatchTransform(ActionTokenizer(vocab), tokenizer, use_wrist_image=cfg.num_images_in_input > 1,
                                                              use_proprio=cfg.use_proprio),
                                         resize_resolution=(side, side), shuffle_buffer_size=cfg.shuffle_buffer_size, image_aug=cfg.image_aug,
                                         seed=7, rank=rank, world_size=world)
        if dataset_statistics is None:
            dataset_statistics = train_dataset.dataset_statistics    # saved next to every checkpoint (finetune.py:1003-1005)
        collator = D.DeviceCollator(2048, model_config.pad_token_id, device=dev, image_aug=cfg.image_aug, seed=1000 + rank, image_size=side)
        dataset = D.batches(train_dataset, collator, cfg.batch_size)
        if cfg.use_val_set and val_dataset is None:    # finetune.py:990-1000, 1017-1026: the store's val/ split, augmented like the training frames
            val_ds = D.EpisodeDataset(cfg.data_root_dir, cfg.dataset_name, train_dataset.batch_transform, resize_resolution=(side, side),
                                      shuffle_buffer_size=cfg.shuffle_buffer_size // 10, image_aug=cfg.image_aug, train=False, seed=11, rank=rank,
                                      world_size=world)
            val_collator = D.DeviceCollator(2048, model_config.pad_token_id, device=dev, image_aug=cfg.image_aug, seed=2000 + rank, image_size=side)
            val_dataset = lambda: D.batches(val_ds, val_collator, cfg.batch_size)  # noqa: E731
        log(f"[finetune] episode store {cfg.data_root_dir / cfg.dataset_name}: {len(train_dataset)} frames, image_aug={cfg.image_aug}")
    if dataset is None:
        def synthetic_stream():
            step = 0
            while True:
                yield synthetic.make_batch(cfg.batch_size, seed=1000 * (step + 1) + rank, num_images=cfg.num_images_in_input,
                                           chunk=C.NUM_ACTIONS_CHUNK, action_dim=C.ACTION_DIM, proprio_dim=C.PROPRIO_DIM,
                                           image_size=model_config.dino.image_size)
                step += 1
        dataset = synthetic_stream()
    if cfg.use_val_set and val_dataset is None:
        raise ValueError("use_val_set=True needs a validation source: an episode store with a val/ split, or `val_dataset` (a callable returning an iterable of batches)")
    history = {"loss_value": [], "learning_rate": [], "val": []}
    if discrete:
        from ..prismatic.training.train_utils import compute_actions_l1_loss, compute_token_accuracy
        from ..prismatic.vla.action_tokenizer import ActionTokenizer

        metric_tok = ActionTokenizer(type("Vocab", (), {"vocab_size": model_config.vocab - model_config.pad_to_multiple_of})())
        history.update({k: [] for k in ("curr_action_accuracy", "curr_action_l1_loss", "next_actions_accuracy", "next_actions_l1_loss")})
    if device_noise:
        history.update({"curr_action_l1_loss": [], "next_actions_l1_loss": []})
    if ema_decay is not None:
        history["ema_decay"] = []
    if grad_clip:
        history.update({"grad_norm": [], "grad_clip_coef": [], "skipped_steps": []})
    if tensor_stats_freq is not None:
        history.update({"tensor_stats": [], "nonfinite_tensors": []})
    if fit_scale:
        history.update({"scale_nll": [], "action_scale": []})
    step_kw = dict(fit_scale=True) if fit_scale else {}
    stats_step = None                   # the step of a collection not yet read back
    stats_table, bad_seen = {}, {}       # the last table read back; each tensor's n_bad_steps at the last logging step
    skipped_seen = engine.grad_clip_stats()["skipped"] if grad_clip and tensor_stats_freq is not None else 0

    def make_diffusion(batch):   # DiffusionActionHead.sample_noisy_actions (action_heads.py:167-197)
        if device_noise:
            return engine.draw_diffusion(batch["actions"])
        gt = batch["actions"].to("cpu", torch.float32)
        noise = torch.randn(gt.shape, generator=noise_gen).to(torch.bfloat16).float()
        tsteps = torch.randint(0, cfg.num_diffusion_steps, (gt.shape[0],), generator=noise_gen)
        return dict(noise=noise, noisy_actions=sched.add_noise(gt, noise, tsteps).to(torch.bfloat16), timestep_emb=time_enc(tsteps.float()).to(torch.bfloat16))

    def token_metrics(batch, pred_ids):   # finetune.py:358-377
        gt_ids = batch["labels"][:, 1:].to("cpu")
        out = {}
        for name, m in (("curr_action", get_current_action_mask(gt_ids)), ("next_actions", get_next_actions_mask(gt_ids))):
            out[f"{name}_accuracy"] = compute_token_accuracy(pred_ids, gt_ids, m).item()
            out[f"{name}_l1_loss"] = compute_actions_l1_loss(metric_tok, pred_ids, gt_ids, m).item()
        return out

    engine.zero_grad()
    for batch_idx, batch in enumerate(dataset):
        if not cfg.use_proprio:
            batch = {**batch, "proprio": None}
        diffusion = make_diffusion(batch) if cfg.use_diffusion else None
        if device_noise and batch_idx % cfg.diffusion_sample_freq == 0:   # finetune.py:1053: before the step, with the parameters the loss sees
            for k, v in sampled_l1_metrics(engine, batch).items():
                history[k].append(v)
        if discrete:
            loss_sum, count, pred_ids = engine.train_step_discrete(batch, loss_scale=1.0 / cfg.grad_accumulation_steps)
        else:
            loss_sum, count, _ = engine.train_step_fwd_bwd(batch, loss_scale=1.0 / cfg.grad_accumulation_steps, diffusion=diffusion, **step_kw)
        gradient_step_idx = batch_idx // cfg.grad_accumulation_steps
        log_step = gradient_step_idx if not cfg.resume else cfg.resume_step + gradient_step_idx
        if (batch_idx + 1) % cfg.grad_accumulation_steps == 0:
            if reducer is not None:
                reducer.all_reduce()
            lr = learning_rate_at(cfg, gradient_step_idx)
            if tensor_stats_freq is not None and log_step % tensor_stats_freq == 0:   # of the gradient adamw_step is about to see
                engine.collect_tensor_stats(grad_scale=1.0 / world)
                stats_step = log_step
            engine.adamw_step(lr, grad_scale=1.0 / world)
            if ema_decay is not None:
                decay = ema_decay_at(engine.ema_step + 1, max_decay=ema_decay, power=ema_power, inv_gamma=ema_inv_gamma, update_after=ema_update_after)
                engine.ema_update(decay)
            engine.refresh_derived()
            engine.zero_grad()
            if log_step % cfg.wandb_log_freq == 0:
                history["loss_value"].append(loss_sum.item() / count)
                history["learning_rate"].append(lr)
                if ema_decay is not None:
                    history["ema_decay"].append(decay)
                if fit_scale:   # of this step's last micro-batch, read where the loss was just read
                    history["scale_nll"].append(engine.last_scale_fit["nll"].item())
                    history["action_scale"].append(engine.last_scale_fit["scale"].item())
                if discrete:
                    for k, v in token_metrics(batch, pred_ids).items():
                        history[k].append(v)
                clip_note = ""
                if grad_clip:   # the feature's only readback, where the loss was just read
                    stats = engine.grad_clip_stats()
                    history["grad_norm"].append(stats["norm"])
                    history["grad_clip_coef"].append(stats["coef"])
                    history["skipped_steps"].append(stats["skipped"])
                    clip_note = f" grad_norm {stats['norm']:.4g} clip_coef {stats['coef']:.4g} skipped {stats['skipped']}"
                if stats_step is not None:   # the statistics' only readback, once per collection that a logging step follows
                    stats_table = engine.tensor_stats()
                    history["tensor_stats"].append((stats_step, group_tensor_stats(stats_table)))
                    history["nonfinite_tensors"].append(sorted(n for n, s in stats_table.items() if s["n_bad_steps"] > 0))
                    if rank == 0:
                        with open(run_dir / "tensor_stats.jsonl", "a") as f:
                            f.write(json.dumps({"step": stats_step, "tensors": stats_table}) + "\n")
                    stats_step = None
                if tensor_stats_freq is not None:
                    rose = [n for n, s in stats_table.items() if s["n_bad_steps"] > bad_seen.get(n, 0)]
                    if grad_clip and stats["skipped"] > skipped_seen and rose:
                        clip_note += f" non-finite gradient in {', '.join(rose[:3])}" + (f" (+{len(rose) - 3} more)" if len(rose) > 3 else "")
                    bad_seen = {n: s["n_bad_steps"] for n, s in stats_table.items()}
                    skipped_seen = stats["skipped"] if grad_clip else 0
                if rank == 0:
                    log(f"step {log_step}: loss {history['loss_value'][-1]:.5f} lr {lr:.2e}{clip_note}")
            if cfg.use_val_set and log_step > 0 and log_step % cfg.val_freq == 0:   # finetune.py:1128-1144
                with engine.ema_weights() if ema_decay is not None else contextlib.nullcontext():   # validation sees the averaged weights
                    history["val"].append((log_step, run_validation(engine, cfg, val_dataset(), log_step, log if rank == 0 else (lambda *_: None), discrete=discrete,
                                                                    make_diffusion=make_diffusion if cfg.use_diffusion else None,
                                                                    metric_fn=token_metrics if discrete else None, sample_l1=device_noise)))
            if gradient_step_idx > 0 and log_step % cfg.save_freq == 0:
                save_training_checkpoint(run_dir, log_step, engine, dataset_statistics, rank, cfg.save_latest_checkpoint_only)
                if world > 1:
                    dist.barrier()
            if log_step + 1 >= cfg.max_steps:
                break
    return history
