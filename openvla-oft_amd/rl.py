"""Group-relative policy optimisation (GRPO): the pieces between the engine's group entry points and a caller's training loop.  The optimizer
step, the learning-rate schedule, checkpointing and the environments stay the caller's.

grpo_step works on the discrete action-token path (VLAEngine.sample_action_tokens(num_samples=G), reference_logprobs,
train_step_policy_gradient_group).  grpo_step_continuous works on the continuous L1 head, the flagship configuration: L1 regression is maximum
likelihood for a Laplace distribution of fixed scale around the head's prediction, so that distribution is the policy the head already is
(VLAEngine.sample_actions_laplace, reference_action_means, train_step_action_pg_group).  Its `scale` is in normalised action units: a scalar or
one value per action dimension, which is not trained, or "learned" -- the scale head's (VLAEngine.attach_scale_head: one linear map beside the
head's output layer predicts log b per chunk step and dimension).  That head is fitted by maximum likelihood on demonstrations
(finetune(action_scale="fit"), VLAEngine.train_step_scale_nll), and with scale="learned" the policy gradient moves mean and scale together,
the KL is to the reference's mean and scale (reference_action_policy) and `entropy_coef` keeps the scale from collapsing.  Either way the KL
to the reference policy is closed-form, no estimator is needed.
"""
from __future__ import annotations

from typing import Callable, Dict

import numpy as np
import torch


def group_advantages(rewards: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """GRPO's advantage of rewards [B, G]: (r - mean_g) / (std_g + eps) with the group's population standard deviation, fp32, computed where
    `rewards` lives.  A constant group (G = 1 included) gives exactly 0."""
    r = torch.as_tensor(rewards).to(torch.float32)
    if r.dim() != 2:
        raise ValueError(f"rewards: {tuple(r.shape)} (one row of G rewards per observation)")
    centred = r - r.mean(dim=1, keepdim=True)
    std = centred.square().mean(dim=1, keepdim=True).sqrt()
    return centred / (std + eps)


def bin_centres(cfg, device) -> torch.Tensor:
    """The action tokenizer's bin centres (modeling.OpenVLAForActionPrediction.bin_centers), fp32 [n_action_bins - 1] on the device."""
    edges = np.linspace(-1, 1, cfg.n_action_bins)
    return torch.from_numpy((edges[:-1] + edges[1:]) / 2.0).to(device, torch.float32)


def grpo_step(engine, batch: dict, reward_fn: Callable, *, group_size: int, kl_coef: float = 0.0, entropy_coef: float = 0.0, clip=(0.8, 1.2),
              temperature: float = 1.0, inner_steps: int = 1, loss_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """One GRPO iteration on one batch: draw `group_size` chunks per observation from one forward, decode their bins to normalised actions,
    reward_fn(batch, actions [B, G, chunk, action_dim]) -> rewards [B, G], group advantages, the reference policy's log-probabilities when one
    is set and kl_coef > 0, then `inner_steps` group micro-steps with the draw's log-probabilities as old_logprobs.  Gradients accumulate in the
    engine's flat buffers.  -> the last micro-step's statistics plus `reward` (the mean) and `advantages` [B, G], all on the device."""
    cfg = engine.cfg
    draw = engine.sample_action_tokens(batch, temperature=temperature, num_samples=group_size)
    B, G = draw["bins"].shape[:2]
    actions = bin_centres(cfg, engine.device)[draw["bins"].long()].view(B, G, cfg.chunk, cfg.action_dim)
    rewards = torch.as_tensor(reward_fn(batch, actions)).to(engine.device, torch.float32)
    if tuple(rewards.shape) != (B, G):
        raise ValueError(f"reward_fn returned {tuple(rewards.shape)}, expected {(B, G)}")
    adv = group_advantages(rewards)
    ref = None
    if kl_coef > 0.0 and engine.has_reference_policy:
        ref = engine.reference_logprobs(batch, draw["tokens"], temperature=temperature)["logprob"]
    stats = None
    for _ in range(int(inner_steps)):
        stats = engine.train_step_policy_gradient_group(batch, draw["tokens"], adv, old_logprobs=draw["logprob"], ref_logprobs=ref, kl_coef=kl_coef if ref is not None else 0.0,
                                                        entropy_coef=entropy_coef, clip=clip, temperature=temperature, loss_scale=loss_scale)
    stats = dict(stats)
    stats.update(reward=rewards.mean(), advantages=adv)
    return stats


def grpo_step_continuous(engine, batch: dict, reward_fn: Callable, *, group_size: int, scale, kl_coef: float = 0.0, clip=(0.8, 1.2), inner_steps: int = 1,
                         loss_scale: float = 1.0, clamp=(-1.0, 1.0), entropy_coef: float = 0.0) -> Dict[str, torch.Tensor]:
    """One GRPO iteration on one batch of an L1-head engine: draw `group_size` chunks per observation from the Laplace policy of scale `scale`
    around the head's prediction (one forward), reward_fn(batch, actions [B, G, chunk, action_dim]) -> rewards [B, G] on the draws CLAMPED to
    `clamp` (what a robot would execute; None: the raw draws), group advantages, the reference policy's means when one is set and kl_coef > 0,
    then `inner_steps` group micro-steps with the draw's log-probabilities as old_logprobs.  Log-probabilities and gradients use the RAW
    draws.  Gradients accumulate in the engine's flat buffers.  -> the last micro-step's statistics plus `reward` (the mean) and `advantages`
    [B, G], all on the device.
    scale="learned" (engine.attach_scale_head): the widths are the scale head's; the reference is its mean AND log-scale
    (engine.reference_action_policy), the policy gradient moves both, and `entropy_coef` weighs the entropy bonus that keeps the scale from
    collapsing.  The statistics gain `entropy` and `scale`."""
    learned = isinstance(scale, str)
    if entropy_coef != 0.0 and not learned:
        raise ValueError('entropy_coef belongs to scale="learned": a fixed scale has a constant entropy')
    draw = engine.sample_actions_laplace(batch, scale, num_samples=group_size)
    B, G = draw["actions"].shape[:2]
    executed = draw["actions"] if clamp is None else draw["actions"].clamp(float(clamp[0]), float(clamp[1]))
    rewards = torch.as_tensor(reward_fn(batch, executed)).to(engine.device, torch.float32)
    if tuple(rewards.shape) != (B, G):
        raise ValueError(f"reward_fn returned {tuple(rewards.shape)}, expected {(B, G)}")
    adv = group_advantages(rewards)
    ref, extra = None, {}
    if kl_coef > 0.0 and engine.has_reference_policy:
        if learned:
            pol = engine.reference_action_policy(batch)
            ref, extra["ref_log_scales"] = pol["mean"], pol["log_scale"]
        else:
            ref = engine.reference_action_means(batch)
    if learned:
        extra["entropy_coef"] = entropy_coef
    stats = None
    for _ in range(int(inner_steps)):
        stats = engine.train_step_action_pg_group(batch, draw["actions"], adv, scale, old_logprobs=draw["logprob"], ref_means=ref,
                                                  kl_coef=kl_coef if ref is not None else 0.0, clip=clip, loss_scale=loss_scale, **extra)
    stats = dict(stats)
    stats.update(reward=rewards.mean(), advantages=adv)
    return stats
