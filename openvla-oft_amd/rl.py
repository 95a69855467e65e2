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

Those are bandit methods: G chunks of ONE observation are scored against each other, and nothing knows that a chunk is one step of an episode.
gae and ppo_step_continuous are the episodic side (PPO): a value head beside the L1 head (VLAEngine.attach_value_head; action_values,
sample_actions_laplace(return_value=True) record the critic's value with each rollout step), generalised advantage estimation over a
caller-owned rollout buffer [N trajectories, T steps] on the device (ovla_gae, ovla_advantage_normalize: nothing is read back between the
buffer and the training step), and one minibatch of that buffer through train_step_action_pg_group at G = 1 with the clipped value loss
beside the clipped surrogate.  The critic's gradient stops at the head's hidden output: it fits the value on the policy's features and does
not shape them.  The rollout buffer, the environments, minibatching and the optimizer loop stay the caller's.

Everything above needs a scalar reward for every drawn chunk.  preference_pairs, dpo_step_continuous and online_dpo_step_continuous train on
COMPARISONS instead (direct preference optimisation on the same Laplace policy): per observation a chosen and a rejected chunk -- this rollout
succeeded and that one failed, an operator preferred A over B, the demonstration beats the policy's own draw -- and a reference policy.  The
loss is a function of the margin between the two chunks' summed log-ratios to the reference, and VLAEngine.train_step_action_dpo takes it
from ONE training forward and one backward (ovla_laplace_dpo).  dpo_step_continuous runs that step on given pairs, fetching the reference's
means (and log-scales under scale="learned") when the caller has not computed them once per dataset; online_dpo_step_continuous draws G
chunks per observation, scores them with a reward function and lets preference_pairs pick the best and the worst as the pair;
VLAEngine.action_preference reports margin and accuracy of held-out pairs.  `nll_coef` adds the chosen chunk's negative log-likelihood, the
usual regulariser that keeps the chosen chunk's probability from falling with the rejected one's.
"""
from __future__ import annotations

from typing import Callable, Dict

import numpy as np
import torch

from . import ops


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


def gae(rewards, values, bootstrap, dones, lengths=None, gamma: float = 0.99, lam: float = 0.95, normalize: bool = True, eps: float = 1e-8):
    """Generalised advantage estimation over a rollout buffer, on the device: rewards, values [N, T], bootstrap [N] (the critic's value of the
    observation after the last recorded step), dones [N, T] (true: the episode ended after this step), lengths [N] (steps recorded per
    trajectory, default T) -> (advantages, returns) fp32 [N, T], +0 beyond a trajectory's length.  One ovla_gae launch and, with `normalize`,
    one ovla_advantage_normalize launch on the advantages (mean 0, population std 1 over the recorded steps; the returns are not normalised);
    nothing is read back.  `lengths` given on the HOST (a list, an array, a CPU tensor) is checked against [0, T] before the launch; a device
    tensor is taken as it is and clamped by the kernels."""
    tensors = [t for t in (rewards, values, bootstrap, dones, lengths) if isinstance(t, torch.Tensor) and t.is_cuda]
    if not tensors:
        raise ValueError("gae works on the device: at least one of its inputs must be a device tensor")
    dev = tensors[0].device

    def on_dev(t, dtype):
        return torch.as_tensor(t).to(dev, dtype).contiguous()

    r = on_dev(rewards, torch.float32)
    if r.dim() != 2:
        raise ValueError(f"rewards: {tuple(r.shape)} ([N trajectories, T steps])")
    N, T = r.shape
    v, bs, d = on_dev(values, torch.float32), on_dev(bootstrap, torch.float32).reshape(-1), on_dev(torch.as_tensor(dones) != 0, torch.uint8)
    if tuple(v.shape) != (N, T) or tuple(d.shape) != (N, T) or bs.numel() != N:
        raise ValueError(f"values {tuple(v.shape)}, dones {tuple(d.shape)}, bootstrap {tuple(bs.shape)} for rewards {(N, T)}")
    ln = host = None
    if lengths is not None:
        if not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            host = [int(x) for x in torch.as_tensor(lengths).reshape(-1).tolist()]
        ln = on_dev(lengths, torch.int32).reshape(-1)
        if ln.numel() != N:
            raise ValueError(f"lengths: {ln.numel()} for {N} trajectories")
    adv, ret = ops.gae(r, v, bs, d, length=ln, host_lengths=host, gamma=gamma, lam=lam)
    if normalize:
        ops.advantage_normalize(adv, length=ln, host_lengths=host, eps=eps)
    return adv, ret


def ppo_step_continuous(engine, batch: dict, actions, old_logprobs, advantages, returns, old_values=None, *, scale, clip=(0.8, 1.2), value_coef: float = 0.5,
                        value_clip: float = 0.0, kl_coef: float = 0.0, entropy_coef: float = 0.0, inner_steps: int = 1,
                        loss_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """One PPO iteration on one minibatch of a rollout buffer of an L1-head engine with a value head: `batch` the B observations, `actions`
    [B, chunk, action_dim] the RAW chunks drawn at rollout time (sample_actions_laplace), `old_logprobs` [B, chunk] their log-probabilities then,
    `advantages` [B] and `returns` [B] from gae, `old_values` [B] the critic's values then (needed with value_clip > 0).  The reference
    policy's means (and log-scales under scale="learned") when one is set and kl_coef > 0, then `inner_steps` micro-steps of
    train_step_action_pg_group at G = 1 with the value loss.  Gradients accumulate in the engine's flat buffers; nothing is read back.
    -> the last micro-step's statistics (loss, logprob, ratio, clip_frac, kl, value_loss, value_clip_frac, explained_variance, value; entropy
    and scale under scale="learned")."""
    learned = isinstance(scale, str)
    if entropy_coef != 0.0 and not learned:
        raise ValueError('entropy_coef belongs to scale="learned": a fixed scale has a constant entropy')
    cfg, B = engine.cfg, batch["input_ids"].shape[0]
    act = torch.as_tensor(actions)
    if tuple(act.shape) != (B, cfg.chunk, cfg.action_dim):
        raise ValueError(f"actions: {tuple(act.shape)}, expected {(B, cfg.chunk, cfg.action_dim)}")
    old_lp = torch.as_tensor(old_logprobs)
    if tuple(old_lp.shape) != (B, cfg.chunk):
        raise ValueError(f"old_logprobs: {tuple(old_lp.shape)}, expected {(B, cfg.chunk)}")
    adv = torch.as_tensor(advantages)
    if adv.numel() != B:
        raise ValueError(f"advantages: {tuple(adv.shape)} for {B} observations")
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
        stats = engine.train_step_action_pg_group(batch, act.reshape(B, 1, cfg.chunk, cfg.action_dim), adv.reshape(B, 1), scale,
                                                  old_logprobs=old_lp.reshape(B, 1, cfg.chunk), ref_means=ref, kl_coef=kl_coef if ref is not None else 0.0,
                                                  clip=clip, loss_scale=loss_scale, returns=returns, old_values=old_values, value_coef=value_coef,
                                                  value_clip=value_clip, **extra)
    return dict(stats)


def preference_pairs(actions, rewards, min_gap: float = 0.0):
    """The pair of a group: actions [B, G, chunk, action_dim], rewards [B, G] -> (chosen, rejected [B, chunk, action_dim], weight fp32 [B]) where
    `actions` lives, nothing read back.  chosen is the draw of the highest reward, rejected that of the lowest, the lowest index winning a tie;
    weight is 0 where max - min <= min_gap (a group that does not tell its draws apart: train_step_action_dpo skips it), else 1."""
    act = torch.as_tensor(actions)
    r = torch.as_tensor(rewards).to(act.device, torch.float32)
    if act.dim() != 4 or tuple(r.shape) != tuple(act.shape[:2]):
        raise ValueError(f"actions {tuple(act.shape)} ([B, G, chunk, action_dim]) with rewards {tuple(r.shape)} ([B, G])")
    B, G = r.shape
    order = torch.arange(G, device=r.device).expand(B, G)
    hi, lo = r.max(dim=1, keepdim=True).values, r.min(dim=1, keepdim=True).values
    first = lambda hit: torch.where(hit, order, G).min(dim=1).values   # noqa: E731  (the lowest index among the hits; every row has one)
    i_hi, i_lo = first(r == hi), first(r == lo)
    rows = torch.arange(B, device=r.device)
    weight = ((hi - lo).reshape(B) > float(min_gap)).to(torch.float32)
    return act[rows, i_hi], act[rows, i_lo], weight


def dpo_step_continuous(engine, batch: dict, chosen, rejected, *, scale, beta: float, ref_means=None, ref_log_scales=None, weights=None, label_smoothing: float = 0.0,
                        loss_type: str = "sigmoid", nll_coef: float = 0.0, inner_steps: int = 1, loss_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """One DPO iteration on one batch of an L1-head engine: `chosen`, `rejected` [B, chunk, action_dim] the RAW chunks of each observation's
    pair, `weights` [B] (0 skips a pair).  Without `ref_means` the reference policy's means (and log-scales under scale="learned") are fetched
    from the engine's reference snapshot (set_reference_policy: one inference forward); a caller that trains several epochs on a fixed dataset
    computes them once and passes them.  ValueError with neither: DPO has no meaning without a reference.  Then `inner_steps` micro-steps of
    train_step_action_dpo; gradients accumulate in the engine's flat buffers, nothing is read back.  -> the last micro-step's statistics."""
    learned = isinstance(scale, str)
    if ref_means is None:
        if not engine.has_reference_policy:
            raise ValueError("dpo_step_continuous needs a reference: engine.set_reference_policy() or ref_means")
        if learned:
            pol = engine.reference_action_policy(batch)
            ref_means, ref_log_scales = pol["mean"], pol["log_scale"]
        else:
            ref_means = engine.reference_action_means(batch)
    stats = None
    for _ in range(int(inner_steps)):
        stats = engine.train_step_action_dpo(batch, chosen, rejected, scale, beta=beta, ref_means=ref_means, ref_log_scales=ref_log_scales, weights=weights,
                                             label_smoothing=label_smoothing, loss_type=loss_type, nll_coef=nll_coef, loss_scale=loss_scale)
    return dict(stats)


def online_dpo_step_continuous(engine, batch: dict, reward_fn: Callable, *, group_size: int, scale, beta: float, clamp=(-1.0, 1.0), min_gap: float = 0.0,
                               ref_means=None, ref_log_scales=None, label_smoothing: float = 0.0, loss_type: str = "sigmoid", nll_coef: float = 0.0,
                               inner_steps: int = 1, loss_scale: float = 1.0) -> Dict[str, torch.Tensor]:
    """One online DPO iteration: draw `group_size` chunks per observation from the Laplace policy (sample_actions_laplace, one forward),
    reward_fn(batch, actions [B, G, chunk, action_dim]) -> rewards [B, G] on the draws CLAMPED to `clamp` (what a robot would execute; None: the
    raw draws), the best and the worst draw of each group as its pair (preference_pairs; a group whose rewards lie within `min_gap` is
    skipped), then dpo_step_continuous on the RAW draws.  -> its statistics plus `reward` (the mean) and `weights` [B], all on the device."""
    if int(group_size) < 2:
        raise ValueError(f"group_size = {group_size}: a pair needs two draws")
    if ref_means is None and not engine.has_reference_policy:
        raise ValueError("online_dpo_step_continuous needs a reference: engine.set_reference_policy() or ref_means")
    draw = engine.sample_actions_laplace(batch, scale, num_samples=group_size)
    B, G = draw["actions"].shape[:2]
    executed = draw["actions"] if clamp is None else draw["actions"].clamp(float(clamp[0]), float(clamp[1]))
    rewards = torch.as_tensor(reward_fn(batch, executed)).to(engine.device, torch.float32)
    if tuple(rewards.shape) != (B, G):
        raise ValueError(f"reward_fn returned {tuple(rewards.shape)}, expected {(B, G)}")
    chosen, rejected, weight = preference_pairs(draw["actions"], rewards, min_gap)
    stats = dpo_step_continuous(engine, batch, chosen, rejected, scale=scale, beta=beta, ref_means=ref_means, ref_log_scales=ref_log_scales, weights=weight,
                                label_smoothing=label_smoothing, loss_type=loss_type, nll_coef=nll_coef, inner_steps=inner_steps, loss_scale=loss_scale)
    stats.update(reward=rewards.mean(), weights=weight)
    return stats
