"""Reference-facing model classes over the HIP engine.

Mirrors the call signatures the LIBERO fine-tune / eval glue uses:
  OpenVLAForActionPrediction.forward / .predict_action      prismatic/extern/hf/modeling_prismatic.py:499-675, 946-1060
  L1RegressionActionHead.predict_action                     prismatic/models/action_heads.py:84-107
  ProprioProjector / NoisyActionProjector                   prismatic/models/projectors.py:6-49
`forward` returns hidden states that carry a torch autograd edge into the engine's explicit backward, so reference-style
glue (`loss = L1Loss(gt, head.predict_action(h)); loss.backward()`) works unchanged; the fused training step
(engine.train_step_fwd_bwd) is what `finetune()` and bench.py use.  All arithmetic runs in libovla_hip.so.
"""
from __future__ import annotations

import contextlib
import math
from typing import NamedTuple, Any, Dict, List, Optional, Tuple

import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .config import VLAConfig
from .diffusion import DDIMScheduler, SinusoidalPositionalEncoding
from .engine import MAX_SLOTS, AttnCapture, ChunkGraph, DiffusionGraph, ActionHead, ActionScaleHead, ActionValueHead, MlpProjector, ParamStore, SlotProjectors, VLAEngine, build_component
from .policy_pool import split_passes
from .weights import make_getter

BF16 = torch.bfloat16
IGNORE_INDEX = -100
ACTION_TOKEN_BEGIN_IDX = 31743
STOP_INDEX = 2


def _device(device=None) -> torch.device:
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("openvla-oft_amd runs on MI355X only: there is no CPU / eager fallback for the HIP path")
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


# ======================================================================================================================
# torch-facing parameter views (so `optimizer = AdamW(module.parameters())` style glue keeps working)
# ======================================================================================================================
class _StoreModule:
    """Gives a ParamStore the small part of the nn.Module protocol the reference glue touches."""

    store: ParamStore

    def _torch_params(self):
        st = self.store
        if not hasattr(st, "_tparams"):
            st._tparams = {}
            st._tgrad = {dt: torch.zeros_like(flat) for dt, flat in st.flat.items()}
            for p in st.params:
                tp = nn.Parameter(p.data, requires_grad=True)
                st._tparams[p.name] = tp
        return st._tparams

    def parameters(self):
        return list(self._torch_params().values())

    def named_parameters(self):
        return list(self._torch_params().items())

    def publish_grads(self):
        """fp32 accumulators -> `.grad` views in the parameter dtype (what autograd would have produced)."""
        st = self.store
        tps = self._torch_params()
        for dt, g32 in st.flat_grad.items():
            if dt == BF16:
                ops.cvt_f32_to_bf16(g32, st._tgrad[dt])
            else:
                st._tgrad[dt].copy_(g32)
        for p in st.params:
            tps[p.name].grad = st._tgrad[p.dtype][p.offset: p.offset + p.numel].view(p.shape)
        st._published = True

    def _reset_if_cleared(self):
        """optimizer.zero_grad() (set_to_none) cleared the published grads -> start a fresh accumulation."""
        st = self.store
        if getattr(st, "_published", False) and all(tp.grad is None for tp in self._torch_params().values()):
            st.zero_grad()
            st._published = False

    def train(self, mode: bool = True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    @property
    def module(self):  # DDP-style `.module` access used by the reference glue (finetune.py:398)
        return self


# ======================================================================================================================
# components
# ======================================================================================================================
def _linear_init(out_f, in_f, gen):
    """nn.Linear default init (kaiming uniform a=sqrt(5) -> U(-1/sqrt(in), 1/sqrt(in)) for weight and bias)."""
    b = 1.0 / math.sqrt(in_f)
    return (torch.rand(out_f, in_f, generator=gen) * 2 - 1) * b, (torch.rand(out_f, generator=gen) * 2 - 1) * b


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, head_mod, train):
        B = h.shape[0]
        comp = head_mod.comp
        pred, _, saved = comp.fwd(h.detach().to(BF16).contiguous().view(-1, h.shape[-1]), train=train)
        ctx.saved, ctx.mod, ctx.shape = saved, head_mod, h.shape
        return pred.view(B, comp.cfg.chunk, comp.cfg.action_dim)

    @staticmethod
    def backward(ctx, dpred):
        comp = ctx.mod.comp
        dah = comp.bwd(ctx.saved, dpred=dpred.to(BF16).contiguous().view(-1, comp.cfg.action_dim))
        ctx.mod.publish_grads()
        return dah.view(ctx.shape), None, None


class L1RegressionActionHead(_StoreModule):
    """prismatic/models/action_heads.py:84-107: MLPResNet(num_blocks=2, input_dim*ACTION_DIM -> hidden -> action_dim)."""

    prefix = "model."

    def __init__(self, input_dim: int = 4096, hidden_dim: int = 4096, action_dim: int = 7, *, num_actions_chunk: int = 8, device=None,
                 state_dict: Optional[Dict[str, torch.Tensor]] = None, seed: int = 0):
        if input_dim != hidden_dim:
            raise ValueError("the reference always builds the head with input_dim == hidden_dim == llm_dim")
        self.action_dim, self.llm_dim = action_dim, input_dim
        self.cfg = VLAConfig(llm_dim=input_dim, action_dim=action_dim, chunk=num_actions_chunk)
        self.device = _device(device)
        self.training = False
        sd = state_dict if state_dict is not None else self._default_init(seed)
        self._build(sd)

    def _default_init(self, seed):
        g = torch.Generator().manual_seed(seed)
        D, A, p = self.llm_dim, self.action_dim, self.prefix
        sd = {}
        for name, dim in (("layer_norm1", D * A), ("layer_norm2", D), ("mlp_resnet_blocks.0.ffn.0", D), ("mlp_resnet_blocks.1.ffn.0", D)):
            sd[p + name + ".weight"], sd[p + name + ".bias"] = torch.ones(dim), torch.zeros(dim)
        for name, o, i in (("fc1", D, D * A), ("mlp_resnet_blocks.0.ffn.1", D, D), ("mlp_resnet_blocks.1.ffn.1", D, D), ("fc2", A, D)):
            sd[p + name + ".weight"], sd[p + name + ".bias"] = _linear_init(o, i, g)
        return sd

    def _build(self, sd):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}   # DDP prefix tolerance (finetune.py:134-156)
        get, _ = make_getter(sd, self.device)
        self.comp = build_component(ActionHead, self.device, get, self.prefix, cfg=self.cfg)
        self.store = self.comp.store

    def predict_action(self, actions_hidden_states: torch.Tensor) -> torch.Tensor:
        """(B, chunk*action_dim, D) -> (B, chunk, action_dim) bf16."""
        self._reset_if_cleared()
        if torch.is_grad_enabled() and actions_hidden_states.requires_grad:
            return _HeadFn.apply(actions_hidden_states, self, True)
        with torch.no_grad():
            return _HeadFn.apply(actions_hidden_states, self, False)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {}
        for lin in self.comp.linears():
            out.update(lin.export("data"))
        for p in self.comp.plain_params():
            out[p.name] = p.data
        return {k: v.detach().clone() for k, v in out.items()}

    def load_state_dict(self, sd):
        self._build(sd)


class DiffusionActionHead(L1RegressionActionHead):
    """prismatic/models/action_heads.py:144-211: the same MLPResNet predicting the noise, plus the DDIM scheduler and the
    sinusoidal timestep encoder."""

    prefix = "noise_predictor.mlp_resnet."

    def __init__(self, input_dim: int = 4096, hidden_dim: int = 4096, action_dim: int = 7, num_diffusion_steps: int = 100, **kw):
        super().__init__(input_dim, hidden_dim, action_dim, **kw)
        self.noise_scheduler = DDIMScheduler(num_train_timesteps=num_diffusion_steps, beta_schedule="squaredcos_cap_v2")
        self.num_diffusion_steps = num_diffusion_steps
        self.time_encoder = SinusoidalPositionalEncoding(dim=hidden_dim)

    def sample_noisy_actions(self, ground_truth_actions: torch.Tensor, generator: Optional[torch.Generator] = None):
        """action_heads.py:167-197 (host-side: a chunk is a few hundred numbers)."""
        gt = ground_truth_actions.detach().to("cpu", torch.float32)
        B = gt.shape[0]
        noise = torch.randn(gt.shape, generator=generator).to(BF16).float()
        timesteps = torch.randint(0, self.noise_scheduler.config.num_train_timesteps, (B,), generator=generator)
        noisy = self.noise_scheduler.add_noise(gt, noise, timesteps).to(BF16)
        temb = self.time_encoder(timesteps.float()).to(BF16).unsqueeze(1)
        return dict(noise=noise.to(BF16), noisy_actions=noisy, diffusion_timestep_embeddings=temb, timesteps=timesteps)

    def predict_noise(self, actions_hidden_states: torch.Tensor) -> torch.Tensor:
        """action_heads.py:199-211"""
        return self.predict_action(actions_hidden_states)


class ProprioProjector(_StoreModule):
    """prismatic/models/projectors.py:6-24 (fp32 parameters, bf16 compute: finetune.py:895-901 never casts it)."""

    prefix = ""

    def __init__(self, llm_dim: int, proprio_dim: int, *, device=None, state_dict=None, seed: int = 0):
        self.llm_dim, self.in_dim = llm_dim, proprio_dim
        self.device = _device(device)
        self.training = False
        if state_dict is None:
            g = torch.Generator().manual_seed(seed)
            state_dict = {}
            state_dict["fc1.weight"], state_dict["fc1.bias"] = _linear_init(llm_dim, proprio_dim, g)
            state_dict["fc2.weight"], state_dict["fc2.bias"] = _linear_init(llm_dim, llm_dim, g)
        self.load_state_dict(state_dict)

    def load_state_dict(self, sd):
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        raw = lambda name: sd[name].detach().to(self.device, torch.float32)   # keep fp32 masters exact
        self.comp = build_component(MlpProjector, self.device, raw, self.prefix)
        self.store = self.comp.store

    def state_dict(self):
        out = {}
        for lin in self.comp.linears():
            out.update(lin.export("data"))
        return {k: v.detach().clone() for k, v in out.items()}


class NoisyActionProjector(ProprioProjector):
    """prismatic/models/projectors.py:27-49"""

    def __init__(self, llm_dim: int, *, device=None, state_dict=None, seed: int = 0):
        super().__init__(llm_dim, 1, device=device, state_dict=state_dict, seed=seed)


# ======================================================================================================================
# the VLA
# ======================================================================================================================
class _LMLossFn(torch.autograd.Function):
    """`output.loss` of the reference's forward (LlamaForCausalLM with `labels`: logits.float(), shift by one, cross entropy with
    ignore_index -100, mean over the counted labels; modeling_prismatic.py:632-643 + :486-496 for the multimodal labels), computed on
    the counted rows only, by the engine's pieces of train_step_discrete (counted_rows, lm_loss_fwd, lm_loss_bwd, backward_from_rows).  The mean's
    1 / n_tok rides in the token gradient and the incoming d loss in the backward GEMM's alpha.  `out`: the engine forward's result."""

    @staticmethod
    def forward(ctx, hidden, vla, labels, out):
        eng = vla.engine
        if eng.lm_head is None:
            raise RuntimeError("output.loss / output.logits need language_model.lm_head.weight, which this checkpoint was loaded without")
        bb, jj, rows_idx, targets = eng.counted_rows(labels.to("cpu", torch.int64), out["S"], out["P"])
        n_tok = rows_idx.numel()
        need_grad = ctx.needs_input_grad[0]
        loss_rows, amax, logits = eng.lm_loss_fwd(out, rows_idx, targets, grad_scale=(1.0 / n_tok) if need_grad else None)
        if need_grad:
            ctx.dlogits, ctx.rows_idx, ctx.out, ctx.eng = logits, rows_idx, out, eng
        vla._last_token_argmax = (bb, jj, amax)
        return loss_rows.sum() / n_tok

    @staticmethod
    def backward(ctx, dloss):
        dhidden = ctx.eng.backward_from_rows(ctx.eng.lm_loss_bwd(ctx.dlogits, alpha=float(dloss)), ctx.rows_idx, ctx.out, run=False)
        return dhidden.view(ctx.out["hidden"].shape), None, None, None


class PrismaticCausalLMOutputWithPast:
    """prismatic/extern/hf/modeling_prismatic.py:266-278 / :668-675.  `hidden_states[-1]` (post final norm) and `projector_features`
    are materialised by the forward; `loss` and `logits` -- which the reference always computes and the L1 / diffusion recipes throw
    away (finetune.py:396-407) -- are computed on first access: `loss` as an autograd node on the hidden state (`loss.backward()`
    works), `logits` as the fp32 [B, S, vocab] tensor of the frozen lm_head without a gradient edge (0.6 GB at B = 8).
    `attentions`: None, or with forward(output_attentions=True) a tuple of n_layers detached fp32 [B, H, S, S] tensors, the decoder's attention
    probabilities as the HF decoder returns them (engine.AttnCapture(rows="all", per_head=True): B*H*S*S*4 bytes per layer)."""

    past_key_values = None
    attentions = None

    def __init__(self, vla, hidden, labels, out):
        self._vla, self._labels, self._out = vla, labels, out           # `out`: the engine forward's result behind `hidden`
        self.hidden_states = (hidden,)
        self.projector_features = out["all_patches"]
        self._loss = self._logits = None
        att = out.get("attention")
        if att is not None:   # output_attentions=True: per layer [B, H, S, S], permuted views of the [B*S, H, S] capture
            B, S = hidden.shape[0], hidden.shape[1]
            self.attentions = tuple(p.detach().view(B, S, p.shape[1], S).permute(0, 2, 1, 3) for p in att["per_head"])

    @property
    def loss(self) -> torch.Tensor:
        if self._loss is None:
            self._loss = _LMLossFn.apply(self.hidden_states[-1], self._vla, self._labels, self._out)
        return self._loss

    @property
    def logits(self) -> torch.Tensor:
        if self._logits is None:
            h = self.hidden_states[-1].detach()
            B, S, D = h.shape
            self._logits = self._vla.logits_for(h.reshape(B * S, D)).view(B, S, -1)
        return self._logits

    def __getitem__(self, key):   # ModelOutput-style access: out["loss"], out["hidden_states"]
        return getattr(self, key)


class SampledTokens(NamedTuple):
    """What a sampled decode drew (predict_action / predict_action_batch with do_sample=True, return_tokens=True): device tensors [B, A] --
    the action-token ids (int32), their log-probabilities under softmax(logits[action window] / temperature) and the entropy of that
    distribution per action row (fp32).  `logprobs` is the `old_logprobs` of VLAEngine.train_step_policy_gradient."""
    tokens: torch.Tensor
    logprobs: torch.Tensor
    entropy: torch.Tensor


class SampledActions(NamedTuple):
    """What a noisy L1 decode drew (predict_action / predict_action_batch with action_noise_scale, return_sample=True): device tensors in
    NORMALISED action units -- the draw fp32 [B, chunk, action_dim], its log-probability per chunk step fp32 [B, chunk] under the Laplace
    policy around the head's prediction, and that prediction bf16 [B, chunk, action_dim].  `actions[:, None]` / `logprobs[:, None]` are the
    `actions` / `old_logprobs` of VLAEngine.train_step_action_pg_group.  With action_noise_scale="learned" also the scale head's raw log-scale
    bf16 [B, chunk, action_dim] (None with a numeric scale).  With a value head loaded (load_value_head) also the critic's value of each
    observation fp32 [B] from the same forward (None without one): the `old_values` of a PPO step."""
    actions: torch.Tensor
    logprobs: torch.Tensor
    mean: torch.Tensor
    log_scale: Optional[torch.Tensor] = None
    value: Optional[torch.Tensor] = None


class ActionAttention:
    """What the rows that predict the action slots look at: the third element of predict_action / predict_action_batch with
    `output_attentions=True`.

    mean    fp32 [n_layers, B, A, S] on the device: the head-averaged attention probabilities of each observation's A action rows over the S
            keys of the multimodal sequence (a padding key is exactly 0).
    layout  per observation, an ordered dict of named half-open key ranges (start, stop) that tile [0, S): bos, image0 ... image{I-1},
            proprio and timestep when present, text (the prompt), actions (the A slots), stop, padding."""

    def __init__(self, mean: torch.Tensor, layout: List[Dict[str, Tuple[int, int]]], patches_per_image: int):
        self.mean, self.layout, self.patches_per_image = mean, layout, patches_per_image

    @property
    def range_names(self) -> List[str]:
        return list(self.layout[0])

    def token_mass(self) -> torch.Tensor:
        """fp32 [n_layers, B, A, n_ranges]: the probability mass of each action row inside each named range (in `range_names` order)."""
        nl, B, A, _ = self.mean.shape
        out = torch.zeros((nl, B, A, len(self.range_names)), dtype=torch.float32, device=self.mean.device)
        for b, lay in enumerate(self.layout):
            for i, (k0, k1) in enumerate(lay.values()):
                if k1 > k0:
                    out[:, b, :, i] = self.mean[:, b, :, k0:k1].sum(-1)
        return out

    def patch_maps(self, image: int = 0) -> torch.Tensor:
        """fp32 [n_layers, B, A, g, g] with g * g = patches per image: the attention of each action row over image `image`'s patch grid."""
        g = int(round(self.patches_per_image ** 0.5))
        if g * g != self.patches_per_image:
            raise ValueError(f"patch_maps: {self.patches_per_image} patches per image are not a square grid")
        nl, B, A, _ = self.mean.shape
        k0, k1 = self.layout[0][f"image{image}"]           # the image ranges are the same for every observation of a batch
        return self.mean[:, :, :, k0:k1].reshape(nl, B, A, g, g)


def _attention_layout(n_images: int, patches_per_image: int, P: int, S: int, text_lens, A: int, proprio: bool, timestep: bool = False):
    """The named key ranges of each observation's multimodal sequence (ovla_assemble_multimodal: BOS, the P patch-side tokens, the text after
    BOS).  `text_lens`: tokens of each text row (BOS, prompt, A action slots, stop)."""
    layouts = []
    for n in text_lens:
        n = int(n)
        lay, k = {"bos": (0, 1)}, 1
        for i in range(n_images):
            lay[f"image{i}"] = (k, k + patches_per_image)
            k += patches_per_image
        for name, on in (("proprio", proprio), ("timestep", timestep)):
            if on:
                lay[name] = (k, k + 1)
                k += 1
        assert k == P + 1, f"layout: {k - 1} patch-side tokens accounted for, the forward assembled {P}"
        end = P + n
        lay["text"], lay["actions"], lay["stop"], lay["padding"] = (k, end - A - 1), (end - A - 1, end - 1), (end - 1, end), (end, S)
        layouts.append(lay)
    return layouts


class _VisionBackboneHandle:
    """vla.vision_backbone.{get_num_patches, get_num_images_in_input, set_num_images_in_input} (modeling_prismatic.py:159-184)"""

    def __init__(self, cfg: VLAConfig):
        self._cfg = cfg
        self.num_images_in_input = cfg.num_images

    def get_num_patches(self) -> int:
        return self._cfg.dino.n_patches

    def get_num_images_in_input(self) -> int:
        return self.num_images_in_input

    def set_num_images_in_input(self, n: int) -> None:
        self.num_images_in_input = n


class _VLMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, vla, kwargs, train):
        out = vla.engine.forward(train=train, **kwargs)
        ctx.vla, ctx.saved = vla, out["saved"]
        ctx.mark_non_differentiable(out["action_rows"])
        vla._last = out
        return out["hidden"], out["action_rows"]

    @staticmethod
    def backward(ctx, dhidden, _):
        eng = ctx.vla.engine
        B, S, D = dhidden.shape
        eng.backward_from_hidden(dhidden.to(BF16).contiguous().view(B * S, D), ctx.saved)
        ctx.vla.publish_grads()
        for comp in (ctx.saved.proprio_projector, ctx.saved.noisy_action_projector):
            if comp is not None and hasattr(comp, "owner"):
                comp.owner.publish_grads()
        return None, None, None, None


class OpenVLAForActionPrediction(_StoreModule):
    """prismatic/extern/hf/modeling_prismatic.py:720-1087 over the HIP engine."""

    def __init__(self, cfg: VLAConfig, state_dict: Dict[str, torch.Tensor], *, device=None, lora: Optional[bool] = None,
                 norm_stats: Optional[dict] = None, use_film=None, lora_dropout: float = 0.0, dropout_seed: int = 0):
        """`use_film`: None (True iff the state dict carries FiLM scale / shift Linears), False, True (the model's own FiLM Linears, trained and
        evaluated as the reference's FiLMedPrismaticVisionBackbone), or "per_policy": a BASE model for multi-policy serving whose towers carry
        FiLM slot storage and no FiLM Linears of their own -- every add_policy brings its `film` tensors, every observation of
        predict_action_batch(policy=[...]) is modulated by its own policy's.  Inference only."""
        self.cfg = cfg
        self.device = _device(device)
        get, has = make_getter(state_dict, self.device)
        if lora is None:   # per Linear: a merged checkpoint may still carry the towers' adapters (the reference's FiLM evaluation path)
            lora = "auto" if any(k.endswith(".lora_A.weight") for k in state_dict) else False
        if use_film is None:
            use_film = any(".scale.weight" in k for k in state_dict)
        self.engine = VLAEngine(cfg, get, self.device, lora=lora, use_proprio=False, head="none", has=has, use_film=use_film,
                                lora_dropout=lora_dropout, dropout_seed=dropout_seed)   # (training forwards only: predict_action* never drops)
        self.store = self.engine.store
        self.llm_dim = cfg.llm_dim
        self.norm_stats = norm_stats or {}
        self.bins = np.linspace(-1, 1, cfg.n_action_bins)                       # :725-729
        self.bin_centers = (self.bins[:-1] + self.bins[1:]) / 2.0
        self.vocab_size = cfg.vocab - cfg.pad_to_multiple_of                    # :732
        self.vision_backbone = _VisionBackboneHandle(cfg)
        self.config = type("Cfg", (), {"image_sizes": [cfg.dino.image_size, cfg.siglip.image_size], "pad_token_id": cfg.pad_token_id})()
        self.training = False
        self._anchor = torch.zeros((), device=self.device, requires_grad=True)
        # hipGraph replay of predict_action (L1 / discrete paths: ChunkGraph; diffusion head: DiffusionGraph).  Off by default: a captured graph
        # pins the parameter buffers it was captured with, so it is for deployment (weights frozen), not for evaluation inside a training loop.
        self.use_graph = os.environ.get("OVLA_INFER_GRAPH", "0") == "1"
        self._graphs: Dict[tuple, Any] = {}
        # predict_action_batch: captured graphs kept per (B, text bucket, ...), least recently used evicted first.  A coalescing server raises it to
        # 4 text-length buckets per batch bucket (deploy.OpenVLAServer), so that prompts of varied length do not thrash captures.
        self.max_batch_graphs = 8
        # multi-policy serving (add_policy): name -> dict(lora, head, pp, norm_stats), in adapter-slot order
        self._policies: Dict[str, dict] = {}
        self._policy_gen = 0
        # policy pool (enable_policy_pool): the slot count, and the slot-resident head / proprio projector objects the forward reads
        self._pool_resident = 0
        self._slot_heads: Optional[list] = None
        self._slot_pps: Optional[list] = None

    # -- several fine-tuned policies on one base model ------------------------------------------------------------------------------------
    @property
    def film_per_policy(self) -> bool:
        """True for a base model built with use_film="per_policy": every policy brings its own FiLM Linears."""
        return bool(getattr(self.engine, "film_per_policy", False))

    @property
    def policies(self) -> Tuple[str, ...]:
        """Names of the registered policies, in adapter-slot order."""
        return tuple(self._policies)

    def add_policy(self, name: str, lora_state_dict: Dict[str, torch.Tensor], *, action_head=None, proprio_projector=None,
                   norm_stats: Optional[dict] = None, lora_alpha: Optional[float] = None, film: Optional[Dict[str, torch.Tensor]] = None):
        """Registers one fine-tune's outputs (finetune.py:584-675: `lora_adapter/`, `action_head--*.pt`, `proprio_projector--*.pt`,
        `dataset_statistics.json`) as a policy of this BASE model: its adapters go into the next adapter slot of every adapted linear
        (engine.set_adapter_slots; tensor names as lora_state_dict() emits and weights.load_lora_adapter returns), its L1 head, proprio projector
        and un-normalisation statistics are kept for predict_action_batch(policy=[...]).  At most engine.MAX_SLOTS policies; all with the
        model configuration's rank and lora_alpha (`lora_alpha`: the adapter_config.json value, checked when given), the same adapted linears,
        and alike in having a head / a proprio projector or not.  The model must carry no merged or trainable adapters.  Adding a policy changes
        the slot count n and with it the K-extension width: outputs of earlier policies are reproducible per (policy, n), not across n.
        Every policy's adapter tensors stay referenced on the host and each call refills all slots of all linears (the slot count changed): with
        at most 4 policies that is a handful of copies per linear, done once at registration.
        After enable_policy_pool: no limit on the number of policies, the slot count stays the pool's `resident`, nothing is reallocated and no
        captured graph is dropped; the policy's tensors go to device memory (engine.pool_add) and reach a slot when a batch needs them.
        `film`: the policy's FiLM scale / shift Linears (the scale / shift tensors of its `vision_backbone--*_checkpoint.pt`) under the engine's
        names `vision_backbone.{featurizer,fused_featurizer}.blocks.{i}.{scale,shift}.{weight,bias}`, for exactly the towers' used blocks.
        Required for every policy of a model built with use_film="per_policy", refused on any other model.  A refused policy changes nothing."""
        if not isinstance(name, str) or not name:
            raise ValueError("add_policy: the policy name must be a non-empty string")
        if name in self._policies:
            raise ValueError(f"add_policy: a policy named {name!r} is already registered")
        if action_head is not None and hasattr(action_head, "noise_scheduler"):
            raise ValueError("add_policy: per-policy diffusion heads are not supported (L1 head, or none for the discrete token path)")
        if film is not None and not self.film_per_policy:
            raise ValueError("add_policy: `film` was given, but the model was not built with use_film=\"per_policy\" (a model without FiLM has no "
                             "place for FiLM tensors; a model with its own FiLM Linears serves one policy)")
        if film is None and self.film_per_policy:
            raise ValueError("add_policy: a model built with use_film=\"per_policy\" needs every policy's FiLM tensors (`film`)")
        pol = dict(lora=dict(lora_state_dict), head=action_head, pp=proprio_projector, norm_stats=norm_stats, lora_alpha=lora_alpha,
                   film=None if film is None else dict(film))
        pols = list(self._policies.values()) + [pol]
        for what in ("head", "pp"):
            if len({p[what] is None for p in pols}) > 1:
                raise ValueError(f"add_policy: either every policy brings its own {'action head' if what == 'head' else 'proprio projector'} or none does")
        if self._pool_resident:
            return self._pool_add_policy(name, pol)
        self.engine.set_adapter_slots([p["lora"] for p in pols], lora_alpha=[p["lora_alpha"] for p in pols],
                                      film=[p["film"] for p in pols] if self.film_per_policy else None)   # validates before it changes anything
        self._policies[name] = pol
        self._policy_gen += 1
        for k in [k for k in self._graphs if "policies" in k]:   # captured against the previous slot storage
            del self._graphs[k]
        return self

    # -- the policy pool: any number of registered policies, `resident` of them in the adapter slots at a time ---------------------------------
    def enable_policy_pool(self, resident: int = 4):
        """Before the first add_policy: from then on add_policy registers into a pool without a limit on the number of policies (their tensors
        stay in device memory), remove_policy takes one out again, and predict_action_batch(policy=[...]) copies the up-to-`resident` policies
        a forward needs into fixed slot storage just before it (one ovla_copy_table launch per policy that is not there yet; least recently
        used slot first: policy_pool.plan_loads).  The slot count is `resident` (1 .. engine.MAX_SLOTS) from the first add_policy on and never
        changes: K-extension width, fixed schedules and captured graphs stay valid for the life of the model, and a policy's outputs are
        reproducible per (policy, resident) whatever else is registered or resident.  A forward costs what n = `resident` slots cost, however
        few policies are registered.  All policies must be alike in having a head / a proprio projector, with identical shapes."""
        if self._policies:
            raise ValueError("enable_policy_pool: call it before the first add_policy (the slot count is fixed from then on)")
        if self._pool_resident:
            raise ValueError("enable_policy_pool: the pool is enabled already")
        if isinstance(resident, bool) or not isinstance(resident, int) or not 1 <= resident <= MAX_SLOTS:
            raise ValueError(f"enable_policy_pool: resident = {resident!r} (1 .. {MAX_SLOTS}: at most {MAX_SLOTS} adapter slots ride in one launch)")
        self._pool_resident = resident
        return self

    @property
    def policy_pool_resident(self) -> int:
        """The pool's slot count; 0 without a pool."""
        return self._pool_resident

    @staticmethod
    def _store_layout(mod):
        return None if mod is None else [(p.name, p.shape, p.dtype, p.offset) for p in mod.store.params]

    @staticmethod
    def _param_pairs(src, dst):
        """(source, destination) of everything a head's / projector's forward reads: the flat parameter buffers, and the bf16 compute copies of
        fp32-master linears."""
        pairs = [(flat, dst.store.flat[dt]) for dt, flat in src.store.flat.items()]
        for ls, ld in zip(src.comp.linears(), dst.comp.linears()):
            if ls.master_fp32:
                pairs.append((ls.Wc, ld.Wc))
                if ls.bc is not None:
                    pairs.append((ls.bc, ld.bc))
        return pairs

    def _pool_add_policy(self, name, pol):
        eng, head, pp = self.engine, pol["head"], pol["pp"]
        first = eng.pool is None
        if not first:   # same head / projector shapes as the slot-resident objects
            for what, mod, slots in (("action head", head, self._slot_heads), ("proprio projector", pp, self._slot_pps)):
                if mod is not None and self._store_layout(mod) != self._store_layout(slots[0]):
                    raise ValueError(f"add_policy: the {what} of {name!r} has other shapes than the pool's (one head / projector shape per pool)")
        else:
            eng.init_policy_pool(self._pool_resident, pol["lora"], lora_alpha=pol["lora_alpha"], film=pol["film"])   # validates before it allocates
            R = self._pool_resident
            if head is not None:
                sd, c = head.state_dict(), head.cfg
                self._slot_heads = [L1RegressionActionHead(c.llm_dim, c.llm_dim, c.action_dim, num_actions_chunk=c.chunk, device=self.device, state_dict=sd)
                                    for _ in range(R)]
            if pp is not None:
                sd = pp.state_dict()
                self._slot_pps = [ProprioProjector(pp.llm_dim, pp.in_dim, device=self.device, state_dict=sd) for _ in range(R)]
            self._policy_gen += 1

        def slot_pairs(s):
            return (self._param_pairs(head, self._slot_heads[s]) if head is not None else []) + \
                   (self._param_pairs(pp, self._slot_pps[s]) if pp is not None else [])

        eng.pool_add(name, pol["lora"], lora_alpha=pol["lora_alpha"], slot_pairs=slot_pairs, film=pol["film"])
        self._policies[name] = dict(pol, lora=None, film=None)   # the pool holds the adapters (and FiLM tensors) on the device: no host reference is kept
        return self

    def remove_policy(self, name: str):
        """Pool mode: takes `name` out of the pool.  Its slot is stale from here on: a later add_policy under the same name is loaded afresh."""
        if not self._pool_resident:
            raise ValueError("remove_policy needs the policy pool (enable_policy_pool): without it the slot layout is the registration order")
        if name not in self._policies:
            raise ValueError(f"remove_policy: unknown policy {name!r} (registered: {list(self._policies)})")
        self.engine.pool_remove(name)
        del self._policies[name]
        return self

    @property
    def policy_pool_stats(self) -> Dict[str, int]:
        """loads (slot swaps performed), hits (needed policies found resident), passes (forwards) since enable_policy_pool."""
        st = getattr(self.engine, "pool_state", None)
        return dict(st.stats) if st is not None else dict(loads=0, hits=0, passes=0)

    @property
    def policy_pool_bytes(self) -> int:
        """Device memory the registered policies hold beside the slot storage: adapters (bf16), head and proprio projector parameters with
        their compute copies.  Gradient and optimizer buffers of heads / projectors that were trained in this process are not counted."""
        if not self._pool_resident or self.engine.pool is None:
            return 0
        total = self.engine.pool_bytes()
        for p in self._policies.values():
            for mod, slots in ((p["head"], self._slot_heads), (p["pp"], self._slot_pps)):
                if mod is not None:
                    total += sum(a.numel() * a.element_size() for a, _ in self._param_pairs(mod, slots[0]))
        return total

    def policy_norm_stats(self, name: Optional[str] = None) -> dict:
        """The statistics a policy un-normalises with: its own `norm_stats` when add_policy was given some, otherwise the model's (also for None)."""
        own = self._policies[name]["norm_stats"] if name is not None else None
        return own if own is not None else self.norm_stats

    def merge_and_unload(self):
        """peft `merge_and_unload()` of merge_lora_weights_and_save.py:60-67 on device: W += (alpha/r) B A for every adapted
        Linear; the model becomes inference-only.  Returns self, like peft."""
        self.engine.merge_lora()
        self._graphs.clear()
        return self

    def enable_graph_replay(self, on: bool = True):
        self.use_graph = on
        if not on:
            self._graphs.clear()
        return self

    # -- forward (:499-675) -------------------------------------------------------------------------------------------
    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def forward(self, input_ids=None, attention_mask=None, pixel_values=None, labels=None, inputs_embeds=None, past_key_values=None,
                use_cache=None, output_attentions=None, output_hidden_states=None, output_projector_features=None, return_dict=None,
                proprio=None, proprio_projector=None, noisy_actions=None, noisy_action_projector=None,
                diffusion_timestep_embeddings=None, use_film: bool = False):
        if input_ids is None or pixel_values is None or labels is None:
            raise ValueError("Invalid PrismaticForConditionalGeneration `forward()` call: the HIP path implements the multimodal "
                             "action-prediction branch (input_ids, pixel_values and labels are required)")
        if input_ids.shape[0] != pixel_values.shape[0]:
            raise ValueError("Non-homogenous batch of (text, image) input -- forward() does not support mixed batches!")
        if past_key_values is not None or inputs_embeds is not None:
            raise ValueError("cached generation / inputs_embeds are not part of the parallel-decoding action path")
        if use_film != self.engine.use_film:
            raise ValueError(f"use_film={use_film} but the model was built with use_film={self.engine.use_film} (FiLM adds parameters to the "
                             "vision backbone: finetune.py:874-888, openvla_utils.py:311-349)")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids, dtype=torch.bool)
        self._reset_if_cleared()
        for m in (proprio_projector, noisy_action_projector):
            if m is not None:
                m._reset_if_cleared()
                m.comp.owner = m
        kwargs = dict(input_ids=input_ids, attention_mask=attention_mask, pixel_values=pixel_values, labels=labels, proprio=proprio,
                      noisy_actions=noisy_actions, timestep_emb=diffusion_timestep_embeddings,
                      proprio_projector=None if proprio_projector is None else proprio_projector.comp,
                      noisy_action_projector=None if noisy_action_projector is None else noisy_action_projector.comp)
        if output_attentions:
            kwargs["attn_capture"] = AttnCapture(rows="all", per_head=True)
        if torch.is_grad_enabled():
            hidden, _ = _VLMFn.apply(self._anchor, self, kwargs, True)
        else:
            with torch.no_grad():
                hidden, _ = _VLMFn.apply(self._anchor, self, kwargs, False)
        # the reference also returns the CE loss / fp32 logits of the frozen lm_head; in L1 / diffusion mode they are discarded
        # (finetune.py:400,407), so the output object computes them on first access only
        return PrismaticCausalLMOutputWithPast(self, hidden, labels, self._last)

    def logits_for(self, hidden_rows: torch.Tensor) -> torch.Tensor:
        """lm_head on selected hidden rows [n, D] -> fp32 logits [n, vocab] (discrete action-token path, :929-942)."""
        if self.engine.lm_head is None:
            raise RuntimeError("this checkpoint was loaded without language_model.lm_head.weight")
        return ops.cvt_bf16_to_f32(self.engine.lm_head_rows(hidden_rows))[: hidden_rows.shape[0]]

    # -- the one inference path behind predict_action and predict_action_batch, with graph replay on or off -------------------------------
    @staticmethod
    def _ddim_tables(action_head):
        """(coef fp32 [n_steps, 4], timestep embeddings bf16 [n_steps, D]) of the head's scheduler after set_timesteps: what the host loop
        computes step by step (sched.step's scalars, time_encoder(float(t)).to(bf16)), as DiffusionGraph's two device tables."""
        sched = action_head.noise_scheduler
        temb = torch.cat([action_head.time_encoder(torch.tensor([float(t)])).to(BF16).reshape(1, -1) for t in sched.timesteps])
        return sched.step_coefficients(), temb

    def _graph_key(self, batch, B, L, pixel_shape, *, use_proprio, head_comp, pp_comp, film, discrete, ddim, n_policies, sample=None):
        """The key of a captured graph in self._graphs.  predict_action: one graph per (text length, head, projector), led by "ddim" for the
        sampler.  The batch API: ("batch", B, text bucket, ...), what _evict_batch_graph counts.  `ddim`: (id of the noisy-action projector,
        sampling steps, training steps)."""
        shape = tuple(pixel_shape)
        if n_policies:   # the key holds the policy set's identity and n, never the assignment: one capture serves every assignment
            return ("batch", B, L, shape, use_proprio, ops.BATCH_INVARIANT_DEFAULT, "policies", self._policy_gen, n_policies, "discrete" if discrete else "l1")
        if not batch:
            return ("ddim", L, shape, id(head_comp), id(pp_comp)) + ddim if ddim else (L, shape, id(head_comp), id(pp_comp))
        key = ("batch", B, L, shape, id(head_comp), id(pp_comp), ops.BATCH_INVARIANT_DEFAULT, film)
        if sample is not None:   # the sampled decode is captured: temperature and window are part of the graph
            return key + (discrete, "sample") + sample
        return key + ("ddim",) + ddim if ddim else key + (discrete,)

    def _graph_for(self, key, build):
        """The graph under `key` in self._graphs; on first use `build()` -> (the graph, the components whose parameters its kernels read)."""
        g = self._graphs.pop(key, None)
        if g is None:
            if key[0] == "batch":
                self._evict_batch_graph()
            g, keep = build()
            g._keep = keep   # the captured kernels read these parameter buffers: keep them alive
        self._graphs[key] = g   # (re)inserted last: dict order is least recently used first
        return g

    def _evict_batch_graph(self):
        batched = [k for k in self._graphs if k[0] == "batch"]
        if len(batched) >= self.max_batch_graphs:   # B and the bucket come from callers (/act_batch): keep the most recent few
            del self._graphs[batched[0]]

    def _sample_spec(self, do_sample, temperature, sample_seed, sample_keys, B, discrete: bool, return_tokens: bool, num_samples=None):
        """The `sample` argument of _infer for a do_sample=True call (None otherwise): temperature, the action-token window, the generator's
        three words (the engine's token stream, advanced by one; `sample_seed` replaces its seed for this draw), and the int32 key of every
        action row -- observation key k_b (sample_keys[b], default b) gives k_b * A + a.  `num_samples=G`: G draws per observation from the one
        forward; sample_keys [B, G] (default b * G + g), the keys int32 [B * A, G] (ovla_sample_tokens_group's layout) and "G" in the dict."""
        if not do_sample:
            if return_tokens:
                raise ValueError("return_tokens=True goes with do_sample=True (the greedy decode reports no log-probabilities)")
            if num_samples is not None:
                raise ValueError("num_samples goes with do_sample=True (the greedy decode has one result)")
            return None
        if not discrete:
            raise ValueError("do_sample=True draws action TOKENS: it is the discrete path's (no action head, no per-policy heads); L1 and diffusion "
                             "heads are deterministic regressors / have their own noise")
        st, A = self.engine.token_sample, self.cfg.num_action_tokens
        group = {}
        if num_samples is not None:
            G = int(num_samples)
            if not 1 <= G <= ops.PG_GROUP_MAX:
                raise ValueError(f"num_samples = {G} (1 .. {ops.PG_GROUP_MAX})")
            keys = torch.arange(B * G, dtype=torch.int64).view(B, G) if sample_keys is None else torch.as_tensor(np.asarray(sample_keys)).to(torch.int64)
            if tuple(keys.shape) != (B, G):
                raise ValueError(f"sample_keys: {tuple(keys.shape)} for {B} observations of {G} draws")
            rows = (keys[:, None, :] * A + torch.arange(A, dtype=torch.int64)[None, :, None]).reshape(B * A, G) & 0xFFFFFFFF
            group = dict(G=G)
        else:
            keys = torch.arange(B, dtype=torch.int64) if sample_keys is None else torch.as_tensor(np.asarray(sample_keys)).to(torch.int64).reshape(-1)
            if keys.numel() != B:
                raise ValueError(f"sample_keys: {keys.numel()} keys for {B} observations")
            rows = (keys[:, None] * A + torch.arange(A, dtype=torch.int64)[None, :]).reshape(-1) & 0xFFFFFFFF
        rows = torch.where(rows >= 2 ** 31, rows - 2 ** 32, rows).to(torch.int32)
        words = st.words(st.advance())
        if sample_seed is not None:
            words[0], words[1] = int(sample_seed) & 0xFFFFFFFF, (int(sample_seed) >> 32) & 0xFFFFFFFF
        return dict(temperature=float(temperature), window=self.engine.token_window("actions"), words=words, keys=rows, out={}, **group)

    def _laplace_spec(self, action_noise_scale, sample_keys, B, *, action_head, noisy_action_projector=None, return_sample: bool = False):
        """The `laplace` argument of _infer for a call with action_noise_scale (None otherwise): the per-dimension scale and the int32 key of
        every chunk step -- observation key k_b (sample_keys[b], default b) gives k_b * chunk + c.  Everything is validated here and nothing
        advances: _laplace_advance takes the generator's words once the call can no longer be refused."""
        if action_noise_scale is None:
            if return_sample:
                raise ValueError("return_sample=True goes with action_noise_scale (the plain L1 decode draws nothing)")
            return None
        if action_head is None:
            raise ValueError("action_noise_scale draws around an L1 head's prediction: pass action_head (the token path draws with do_sample=True)")
        if noisy_action_projector is not None or hasattr(action_head, "noise_scheduler"):
            raise ValueError("action_noise_scale is the L1 head's Laplace policy: a diffusion head has its own noise")
        if self.use_graph:
            raise ValueError("action_noise_scale is not supported under graph replay (the captured chunk holds no draw): enable_graph_replay(False)")
        C = self.cfg.chunk
        learned = isinstance(action_noise_scale, str)
        if learned:
            if action_noise_scale != "learned":
                raise ValueError(f'action_noise_scale = {action_noise_scale!r} (a number, one per action dimension, or "learned")')
            if self.scale_head is None:
                raise ValueError('action_noise_scale="learned" needs attach_scale_head() / load_scale_head()')
            b = None
        else:
            b, _ = ops.laplace_scales(action_noise_scale, self.cfg.action_dim)
            if not bool(np.all((b > 0) & np.isfinite(b))):
                raise ValueError(f"action_noise_scale = {action_noise_scale!r} (positive and finite)")
        keys = torch.arange(B, dtype=torch.int64) if sample_keys is None else torch.as_tensor(np.asarray(sample_keys)).to(torch.int64).reshape(-1)
        if keys.numel() != B:
            raise ValueError(f"sample_keys: {keys.numel()} keys for {B} observations")
        rows = (keys[:, None] * C + torch.arange(C, dtype=torch.int64)[None, :]).reshape(-1, 1) & 0xFFFFFFFF
        rows = torch.where(rows >= 2 ** 31, rows - 2 ** 32, rows).to(torch.int32)
        return dict(scale=b, learned=learned, value=return_sample and self.value_head is not None, keys=rows, out={})

    def _laplace_advance(self, laplace, sample_seed):
        """The generator's three words of this draw (the engine's token stream, advanced by one; `sample_seed` replaces its seed)."""
        if laplace is not None:
            st = self.engine.token_sample
            words = st.words(st.advance())
            if sample_seed is not None:
                words[0], words[1] = int(sample_seed) & 0xFFFFFFFF, (int(sample_seed) >> 32) & 0xFFFFFFFF
            laplace["words"] = words
        return laplace

    def _laplace_draw(self, pred, laplace):
        """One ovla_laplace_sample launch around the head's prediction [B, chunk, action_dim] -> the draw, fp32 of the same shape."""
        B, C, Ad = pred.shape
        w = laplace["words"]
        mean = pred.reshape(B * C, Ad).contiguous()
        act, lp = ops.laplace_sample(mean, laplace["scale"], 1, seed=w[0] | (w[1] << 32), call=w[2], row_key=laplace["keys"].to(self.device))
        laplace["out"].update(actions=act.view(B, C, Ad), logprobs=lp.view(B, C), mean=mean.view(B, C, Ad))
        return laplace["out"]["actions"]

    def _laplace_draw_learned(self, hidden, action_head, laplace):
        """The draw that needs the head's hidden output, from the action hidden states [B, chunk * action_dim, D]: the L1 head with its hidden
        output, then -- learned scale -- the scale head and one ovla_laplace_sample_rows launch, or -- numeric scale with a value wanted -- the
        ovla_laplace_sample launch of _laplace_draw; with a value head and return_sample the value head and ovla_value_loss' pooling after it
        -> the draw fp32 [B, chunk, action_dim] (what VLAEngine.sample_actions_laplace issues after its forward)."""
        comp, C, Ad = action_head.comp, self.cfg.chunk, self.cfg.action_dim
        B, w = hidden.shape[0], laplace["words"]
        with torch.no_grad():
            mean, _, _, h2 = comp.fwd(hidden.detach().to(BF16).contiguous().view(-1, hidden.shape[-1]), return_hidden=True)
            if laplace["learned"]:
                ls = self.scale_head.fwd(h2)
                act, lp, _ = ops.laplace_sample_rows(mean, ls, self.scale_bounds, 1, seed=w[0] | (w[1] << 32), call=w[2], row_key=laplace["keys"].to(self.device))
                laplace["out"].update(actions=act.view(B, C, Ad), logprobs=lp.view(B, C), mean=mean.view(B, C, Ad), log_scale=ls.view(B, C, Ad))
            else:
                self._laplace_draw(mean.view(B, C, Ad), laplace)
            if laplace["value"]:
                laplace["out"]["value"] = ops.value_loss(self.value_head.fwd(h2), C)
        return laplace["out"]["actions"]

    # -- the learned Laplace scale (engine.ActionScaleHead): a component of the model beside whichever L1 head a call passes ---------------------
    scale_head = None
    scale_bounds = ops.LAPLACE_SCALE_BOUNDS

    def attach_scale_head(self, init_scale=0.1, bounds=ops.LAPLACE_SCALE_BOUNDS, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        """Gives the model a scale head (weight 0 and bias log(init_scale), or `state_dict`'s `log_scale.weight` / `log_scale.bias`, with or
        without the `action_scale_head.` prefix): what action_noise_scale="learned" draws with.  Replaces an earlier one."""
        lo, hi = float(bounds[0]), float(bounds[1])
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"bounds = {bounds}: two finite log-scales, lo <= hi")
        prefix = "action_scale_head."
        sd = ActionScaleHead.init_tensors(self.cfg, init_scale, self.device, prefix)
        if state_dict is not None:
            given = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
            for k, v in sd.items():
                src = given[k] if k in given else given[k[len(prefix):]]
                if tuple(src.shape) != tuple(v.shape):
                    raise ValueError(f"{k}: shape {tuple(src.shape)} != {tuple(v.shape)}")
                sd[k] = src.to(self.device, BF16)
        self.scale_head = build_component(ActionScaleHead, self.device, sd.__getitem__, prefix, cfg=self.cfg)
        self.scale_bounds = (lo, hi)
        return self.scale_head

    def load_scale_head(self, path, bounds=ops.LAPLACE_SCALE_BOUNDS):
        """attach_scale_head from a fine-tuning run's `action_scale_head--{step}_checkpoint.pt`."""
        return self.attach_scale_head(bounds=bounds, state_dict=torch.load(path, map_location="cpu", weights_only=True))

    # -- the critic of PPO (engine.ActionValueHead): a component of the model, as the scale head is ------------------------------------------------
    value_head = None

    def load_value_head(self, state_dict):
        """Gives the model a value head from `value.weight` [1, llm_dim] / `value.bias` [1] (with or without the `action_value_head.` prefix; a
        state dict, or the path of a saved one).  With it a noisy L1 decode with return_sample=True also reports the critic's value of each
        observation (SampledActions.value); nothing else changes.  Replaces an earlier one."""
        if not isinstance(state_dict, dict):
            state_dict = torch.load(state_dict, map_location="cpu", weights_only=True)
        prefix = "action_value_head."
        given = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state_dict.items()}
        sd = ActionValueHead.init_tensors(self.cfg, self.device, prefix)
        for k, v in sd.items():
            src = given[k] if k in given else given[k[len(prefix):]]
            if tuple(src.shape) != tuple(v.shape):
                raise ValueError(f"{k}: shape {tuple(src.shape)} != {tuple(v.shape)}")
            sd[k] = src.to(self.device, BF16)
        self.value_head = build_component(ActionValueHead, self.device, sd.__getitem__, prefix, cfg=self.cfg)
        return self.value_head

    @staticmethod
    def _sampled_actions(laplace, return_sample: bool) -> tuple:
        if not return_sample:
            return ()
        o = laplace["out"]
        return (SampledActions(o["actions"], o["logprobs"], o["mean"], o.get("log_scale"), o.get("value")),)

    def _decode(self, pred, bins, hidden, sample=None):
        """Normalised actions [B, chunk, action_dim] from whichever the forward produced: the head's prediction (:923-927); the bin indices, when
        the lm_head GEMM + ovla_argmax_bins ran inside a graph; otherwise the greedy token decode of the action hidden states (:929-942)."""
        cfg = self.cfg
        if pred is not None:
            normalized = pred.float().cpu().numpy()
        else:
            if bins is None and sample is not None and "G" in sample:   # G draws per action row from the one forward: [B * A, G] -> [B, G, A]
                (B, A), G, w = hidden.shape[:2], sample["G"], sample["words"]
                tok, b, lp, ent = ops.sample_tokens_group(self.engine.lm_head_rows(hidden.view(-1, cfg.llm_dim))[:B * A], G, n_tokens=self.vocab_size,
                                                          n_bins=self.bin_centers.shape[0], window=sample["window"], temperature=sample["temperature"],
                                                          seed=w[0] | (w[1] << 32), call=w[2], row_key=sample["keys"].contiguous().to(self.device))
                per_draw = lambda t: t.view(B, A, G).permute(0, 2, 1).contiguous()
                sample["out"].update(tokens=per_draw(tok), logprobs=per_draw(lp), entropy=ent)
                return self.bin_centers[per_draw(b).cpu().numpy().astype(np.int64)].reshape(B, G, cfg.chunk, cfg.action_dim)
            if bins is None and sample is not None:   # the draw of ChunkGraph(sample=...), as eager launches
                n = hidden.shape[0] * hidden.shape[1]
                w = sample["words"]
                tok, b, lp, ent = ops.sample_tokens(self.engine.lm_head_rows(hidden.view(-1, cfg.llm_dim))[:n], n_tokens=self.vocab_size,
                                                    n_bins=self.bin_centers.shape[0], window=sample["window"], temperature=sample["temperature"],
                                                    seed=w[0] | (w[1] << 32), call=w[2], row_key=sample["keys"].to(self.device))
                sample["out"].update(tokens=tok, logprobs=lp, entropy=ent)
                bins = b.cpu().numpy().astype(np.int64)
            if bins is None:
                tok = self.logits_for(hidden.view(-1, cfg.llm_dim)).argmax(dim=1).cpu().numpy()
                bins = np.clip(self.vocab_size - tok - 1, a_min=0, a_max=self.bin_centers.shape[0] - 1)
            normalized = self.bin_centers[bins]
        return normalized.reshape(hidden.shape[0], cfg.chunk, cfg.action_dim)

    def _infer(self, ids, mask, labels, pixel_values, prop, *, batch: bool, action_head=None, proprio_projector=None, noisy_action_projector=None,
               noise=None, policy=None, attention: Optional[dict] = None, sample: Optional[dict] = None, laplace: Optional[dict] = None):
        """The forward on prepared ids / mask / labels [B, L], the action rows, the head (L1, or the DDIM sampler from `noise`) or the token
        decode -> (normalised actions ndarray [B, chunk, action_dim], action hidden states [B, A, D] in a tensor of their own).
        `batch` is the mode.  False (predict_action): the planner's GEMM schedules, FiLM's average over all L positions, a graph per key.
        True (predict_action_batch): every GEMM under ops.batch_invariant(ops.BATCH_INVARIANT_DEFAULT), FiLM's average over each row's own
        tokens, "batch" graph keys under the LRU rule, and the token decode inside the graph.
        `policy`: (adapter slot per observation, the policies' head components or None, their proprio projector components or None).
        `attention` (a dict to fill; output_attentions=True): the eager forward (routed with `policy`) with an AttnCapture of the action rows;
        self._graphs is neither used nor touched.  It receives the capture's `mean` [n_layers, B*A, S] and the sequence's P and S.
        `sample` (what _sample_spec returns; do_sample=True): the token decode draws instead of taking the maximum -- inside the batched
        discrete graph, otherwise as the same launch after the forward -- and sample["out"] receives tokens / logprobs / entropy [B*A].
        `laplace` (what _laplace_spec returns; action_noise_scale, the eager L1 path only): the actions are one Laplace draw around the head's
        prediction (one ovla_laplace_sample launch after the head) and laplace["out"] receives actions / logprobs / mean."""
        cfg, eng = self.cfg, self.engine
        (B, L), A, D = ids.shape, cfg.num_action_tokens, cfg.llm_dim
        slots, heads, pps = policy if policy is not None else (None, None, None)
        use_proprio = prop is not None
        head_comp, nap_comp = getattr(action_head, "comp", None), getattr(noisy_action_projector, "comp", None)
        pp_comp = proprio_projector.comp if use_proprio and proprio_projector is not None else None
        use_diffusion = noisy_action_projector is not None and hasattr(action_head, "noise_scheduler")
        if attention is not None and use_diffusion:
            raise ValueError("output_attentions=True with a diffusion head: every DDIM step has its own maps (fifty sets per chunk), which is not supported")
        use_graph = self.use_graph and attention is None
        capture = AttnCapture(rows="actions") if attention is not None else None
        discrete = action_head is None and heads is None
        film, film_avg = batch and eng.use_film, None
        if film and not use_graph:
            # FiLM's language average over each prompt's OWN tokens (padding would enter the mean: film_vit_wrapper.py:243): one ragged launch
            # for the batch, bit for bit ovla_language_average on each unpadded row.  (Under graph replay the launch is part of the graph.)
            film_avg = torch.zeros(((B + 7) // 8 * 8, D), dtype=BF16, device=self.device)
            ops.language_average_ragged(ids.to(self.device), labels.to(self.device), mask.sum(1).to(torch.int32).to(self.device), eng.embed, film_avg)
        pred = bins = ddim = None
        with ops.batch_invariant(ops.BATCH_INVARIANT_DEFAULT) if batch else contextlib.nullcontext():
            if use_diffusion:                                                                 # :793-877, per sample
                sched = action_head.noise_scheduler
                sched.set_timesteps(action_head.num_diffusion_steps)
                if noise is None:
                    noise = torch.randn((B, cfg.chunk, cfg.action_dim))
                cur = torch.as_tensor(noise).to("cpu", torch.float32).reshape(B, cfg.chunk, cfg.action_dim).to(BF16).float()
                ddim = (id(nap_comp), len(sched.timesteps), sched.config.num_train_timesteps)
            # the batched discrete graph holds its decode: a sampled one is a graph of its own, keyed by temperature and window
            graph_sample = (sample["temperature"], sample["window"]) if sample is not None and batch and discrete and policy is None else None
            if use_graph:
                def build():
                    invariant = ops.BATCH_INVARIANT_DEFAULT if batch else False
                    if use_diffusion:
                        coef, temb = self._ddim_tables(action_head)
                        g = DiffusionGraph(eng, B, L, pixel_values.shape, head=head_comp, noisy_action_projector=nap_comp, coef=coef, temb_table=temb,
                                           use_proprio=use_proprio, proprio_projector=pp_comp, invariant=invariant, film=film)
                        return g, (head_comp, pp_comp, nap_comp)
                    per_slot, keep = None, (head_comp, pp_comp)
                    if policy is not None:
                        per_slot = [(None if heads is None else heads[s], None if pps is None else pps[s]) for s in range(eng.n_slots)]
                        keep = (heads, pps)
                    g = ChunkGraph(eng, B, L, pixel_values.shape, head=head_comp, use_proprio=use_proprio, proprio_projector=pp_comp, invariant=invariant,
                                   film=film, discrete=batch and discrete, n_tokens=self.vocab_size, n_bins=self.bin_centers.shape[0], policies=per_slot,
                                   sample=graph_sample)
                    return g, keep

                key = self._graph_key(batch, B, L, pixel_values.shape, use_proprio=use_proprio, head_comp=head_comp, pp_comp=pp_comp, film=film,
                                      discrete=discrete, ddim=ddim, n_policies=eng.n_slots if policy is not None else 0, sample=graph_sample)
                g = self._graph_for(key, build)
                if use_diffusion:
                    # the whole loop from two captured graphs, no host work between the steps (engine.DiffusionGraph): same bits as the loop below
                    sample, ah = g(ids, mask, pixel_values, labels, prop, cur)
                    cur = sample.reshape(B, cfg.chunk, cfg.action_dim)
                else:
                    # one hipGraph per key: ~1.3 k launches -> one graph launch (engine.ChunkGraph)
                    if graph_sample is not None:
                        res = g(ids, mask, pixel_values, labels, prop, slots=slots, sample_state=sample["words"], row_key=sample["keys"])
                        sample["out"].update(tokens=res[2].clone(), logprobs=res[4].clone(), entropy=res[5].clone())   # out of the static buffers
                    else:
                        res = g(ids, mask, pixel_values, labels, prop, slots=slots)
                    pred, ah = res[0], res[1]
                    if len(res) > 2:        # lm_head GEMM + the token decode ran inside the graph: only the bin indices come back
                        bins = res[3].cpu().numpy().astype(np.int64)
                hidden = ah.view(B, A, D).clone()   # out of the graph's static buffer
            elif use_diffusion:
                cached = None
                for t in sched.timesteps:
                    temb = action_head.time_encoder(torch.tensor([float(t)])).to(BF16).reshape(1, D).expand(B, D)
                    out = self.engine.forward(ids, mask, pixel_values, labels, proprio=prop, train=False, noisy_actions=cur.to(BF16), timestep_emb=temb,
                                              proprio_projector=pp_comp, noisy_action_projector=nap_comp, cached_patches=cached, sel="actions",
                                              film_avg=film_avg)
                    cached = out["patches"]                                                   # vision features reused across steps (:810)
                    ah, _ = eng.action_hidden(out)
                    eps = action_head.predict_noise(ah.view(B, A, D)).reshape(cur.shape).float().cpu()
                    cur = sched.step(eps, int(t), cur).prev_sample.to(BF16).float()
                hidden = ah.view(B, A, D).clone()
            else:
                route = contextlib.nullcontext()
                if slots is not None:
                    route = eng.routing(torch.tensor(slots, dtype=torch.int32).to(self.device), host_slots=slots)
                with route:
                    out = self.engine.forward(ids, mask, pixel_values, labels, proprio=prop, train=False,
                                              proprio_projector=SlotProjectors(pps, eng.route) if pps is not None else pp_comp, sel="actions",
                                              film_avg=film_avg, attn_capture=capture)
                    if attention is not None:
                        attention.update(mean=out["attention"]["mean"], P=out["P"], S=out["S"])
                    ah, _ = eng.action_hidden(out)                                            # rows P+NPT .. P+NPT+A-1 (:915-920)
                    hidden = ah.view(B, A, D).clone()
                    if heads is not None:
                        pred = eng.policy_heads_fwd(ah, heads)
                    elif action_head is not None and laplace is not None and (laplace["learned"] or laplace["value"]):
                        pred = self._laplace_draw_learned(hidden, action_head, laplace)
                    elif action_head is not None:
                        pred = action_head.predict_action(hidden)
                        if laplace is not None:
                            pred = self._laplace_draw(pred, laplace)
            normalized = cur.numpy() if use_diffusion else self._decode(pred, bins, hidden, sample)
        return normalized, hidden

    def _infer_pooled(self, ids, mask, labels, pixel_values, prop, policy, use_proprio, attention: Optional[dict] = None):
        """_infer(batch=True) of a pooled model: per pass of at most `resident` distinct policies (in order of first appearance) plan the
        residency, load what is missing (engine.load_slot: one launch per policy, on the stream of the forward), route each observation to its
        policy's slot.  The fixed schedules make an observation's bits independent of its batch, so the split does not show in the results."""
        eng, st = self.engine, self.engine.pool_state
        heads = [h.comp for h in self._slot_heads] if self._slot_heads is not None else None
        pps = [p.comp for p in self._slot_pps] if use_proprio else None
        passes = split_passes(policy, self._pool_resident)
        normalized = hidden = None
        for needed in passes:
            rows = [b for b, p in enumerate(policy) if p in needed]
            loads = st.plan(needed)
            for s, nm in loads:
                eng.load_slot(s, nm)
            slot_of = st.commit(loads, needed)
            whole = len(passes) == 1
            sub = (lambda t: t) if whole else (lambda t: None if t is None else t[rows])
            att_p = None if attention is None else {}
            n_p, h_p = self._infer(sub(ids), sub(mask), sub(labels), sub(pixel_values), sub(prop), batch=True,
                                   policy=([slot_of[policy[b]] for b in rows], heads, pps), attention=att_p)
            if whole:
                if attention is not None:
                    attention.update(att_p)
                return n_p, h_p
            if attention is not None:   # the passes' maps, stitched by observation the way `hidden` is
                m = att_p["mean"]
                A = m.shape[1] // len(rows)
                if "mean" not in attention:
                    attention.update(mean=torch.empty((m.shape[0], len(policy) * A, m.shape[2]), dtype=m.dtype, device=m.device), P=att_p["P"], S=att_p["S"])
                attention["mean"].view(m.shape[0], len(policy), A, m.shape[2])[:, rows] = m.view(m.shape[0], len(rows), A, m.shape[2])
            if normalized is None:
                normalized = np.empty((len(policy),) + n_p.shape[1:], dtype=n_p.dtype)
                hidden = torch.empty((len(policy),) + tuple(h_p.shape[1:]), dtype=h_p.dtype, device=h_p.device)
            normalized[rows], hidden[rows] = n_p, h_p
        return normalized, hidden

    # -- predict_action (:946-1060) -------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict_action(self, input_ids=None, unnorm_key=None, proprio=None, proprio_projector=None, action_head=None,
                       noisy_action_projector=None, use_film: bool = False, output_attentions: bool = False, do_sample: bool = False,
                       temperature: float = 1.0, sample_seed: Optional[int] = None, sample_keys=None, return_tokens: bool = False,
                       action_noise_scale=None, return_sample: bool = False, **kwargs):
        """`do_sample=True` (the discrete token path only; ValueError with a head): the action tokens are DRAWN from softmax(logits[action ids] /
        temperature) on the device (ovla_sample_tokens) and the actions come from the drawn bins; `return_tokens=True` appends a SampledTokens.
        Every sampled call advances the engine's token stream by one; `sample_seed` replaces its seed for this call; `sample_keys` names the
        observation's key in the generator (default 0).  With do_sample=False every launch is the one issued before.
        `action_noise_scale` (an L1 `action_head`, the eager path only; ValueError under graph replay, with a diffusion head or with no head,
        before anything advances): the returned actions are ONE draw from the Laplace policy of that scale (a scalar or one value per action
        dimension, normalised units) around the head's prediction (ovla_laplace_sample), un-normalised as always; `return_sample=True` appends a
        SampledActions holding the normalised draw.  The call advances the engine's token stream by one; `sample_seed` / `sample_keys` as above.
        With action_noise_scale=None every launch is the one issued before.  action_noise_scale="learned" (attach_scale_head / load_scale_head):
        the widths are the scale head's, per chunk step and dimension (ovla_laplace_sample_rows); same refusals, and the SampledActions also
        holds the log-scale.  With a value head (load_value_head) and return_sample=True the SampledActions also holds the critic's value of the
        observation from the same forward (two launches after the draw); without one the field is None and nothing else changes."""
        cfg = self.cfg
        if use_film != self.engine.use_film:
            raise ValueError(f"use_film={use_film} but the model was built with use_film={self.engine.use_film}")
        A = cfg.num_action_tokens
        assert input_ids.shape[0] == 1, "Generation is only currently supported for batch size of 1!"
        pixel_values, attention_mask = kwargs["pixel_values"], kwargs["attention_mask"]
        input_ids = input_ids.to("cpu", torch.int64)
        attention_mask = attention_mask.to("cpu")
        if not torch.all(input_ids[:, -1] == 29871):                                      # :974-977
            input_ids = torch.cat((input_ids, torch.tensor([[29871]], dtype=torch.int64)), dim=1)
            attention_mask = torch.cat((attention_mask, torch.ones((1, 1), dtype=attention_mask.dtype)), dim=1)
        ids = torch.cat([input_ids, torch.ones((1, A), dtype=torch.int64), torch.full((1, 1), STOP_INDEX, dtype=torch.int64)], dim=-1)
        mask = torch.cat([attention_mask, torch.ones((1, A + 1), dtype=attention_mask.dtype)], dim=-1)
        labels = torch.full_like(ids, IGNORE_INDEX)                                      # :983-993
        labels[:, input_ids.shape[-1]:] = ACTION_TOKEN_BEGIN_IDX + 1
        labels[:, -1] = STOP_INDEX
        use_proprio = proprio_projector is not None and proprio is not None
        prop = torch.as_tensor(np.asarray(proprio), dtype=torch.float32) if use_proprio else None
        attention = {} if output_attentions else None   # -> a third result, an ActionAttention (the eager forward; no graph is used or built)
        laplace = self._laplace_spec(action_noise_scale, sample_keys, 1, action_head=action_head, noisy_action_projector=noisy_action_projector,
                                     return_sample=return_sample)
        sample = self._sample_spec(do_sample, temperature, sample_seed, sample_keys, 1, action_head is None, return_tokens)
        normalized, hidden = self._infer(ids, mask, labels, pixel_values, prop, batch=False, action_head=action_head, proprio_projector=proprio_projector,
                                         noisy_action_projector=noisy_action_projector, noise=kwargs.get("noise"), attention=attention, sample=sample,
                                         laplace=self._laplace_advance(laplace, sample_seed))
        res = (self._unnormalize_actions(normalized[0], unnorm_key), hidden)
        if attention is not None:
            res += (self._action_attention(attention, mask, pixel_values, use_proprio),)
        return res + self._sampled_tokens(sample, 1, return_tokens) + self._sampled_actions(laplace, return_sample)

    def _sampled_tokens(self, sample, B: int, return_tokens: bool) -> tuple:
        if not return_tokens:
            return ()
        o, A = sample["out"], self.cfg.num_action_tokens
        if "G" in sample:
            return (SampledTokens(o["tokens"], o["logprobs"], o["entropy"].view(B, A)),)
        return (SampledTokens(o["tokens"].view(B, A), o["logprobs"].view(B, A), o["entropy"].view(B, A)),)

    def _action_attention(self, attention: dict, mask, pixel_values, use_proprio: bool) -> ActionAttention:
        """The ActionAttention of an _infer(attention=...) call on text rows `mask` [B, L] (right-padded)."""
        mean, P, S = attention["mean"], attention["P"], attention["S"]
        B, A = mask.shape[0], self.cfg.num_action_tokens
        n_images = pixel_values.shape[1] // 6
        n_vis = P - (1 if use_proprio else 0)
        layout = _attention_layout(n_images, n_vis // n_images, P, S, mask.to("cpu").sum(1).tolist(), A, use_proprio)
        return ActionAttention(mean.view(mean.shape[0], B, A, S), layout, n_vis // n_images)

    # -- batched inference (not in the reference: its predict_action asserts batch size 1) -----------------------------------------------
    @torch.no_grad()
    def predict_action_batch(self, prompts, pixel_values, unnorm_key=None, proprio=None, proprio_projector=None, action_head=None,
                             noisy_action_projector=None, use_film: bool = False, noise=None, pad_to: Optional[int] = None, policy=None,
                             output_attentions: bool = False, do_sample: bool = False, temperature: float = 1.0, sample_seed: Optional[int] = None,
                             sample_keys=None, return_tokens: bool = False, num_samples: Optional[int] = None, action_noise_scale=None,
                             return_sample: bool = False):
        """predict_action for B observations in one forward.  prompts: list of B (input_ids, attention_mask) pairs ([1, L_b] or [L_b], lengths may
        differ; masks right-padded), pixel_values [B, 6 I, H, W], proprio [B, proprio_dim], noise [B, chunk, action_dim] (diffusion: each sample's
        DDIM trajectory starts from its own noise).  Returns (actions [B, chunk, action_dim] unnormalised with `unnorm_key`, action hidden states
        [B, A, D]).  Every GEMM runs under its fixed schedule (ops.batch_invariant), so each observation's outputs are the same bits whatever else
        is in the batch and in whatever order (OVLA_BATCH_INVARIANT=0: the planner's schedules, for A/B measurement only).
        `pad_to` > B: the batch is filled to `pad_to` observations by repeating observation 0 (valid data, never zeros) and the extra outputs are
        dropped -- the same bits for the B real ones, and a caller with arbitrary arrival counts (the coalescing server) captures one graph per
        bucket instead of one per count.
        `policy` (a model with add_policy): one registered policy name per observation.  Each observation runs under its own policy's LoRA
        adapters (all of them in the same launches: engine.LoraLinear adapter slots), L1 head, proprio projector and un-normalisation statistics
        (`unnorm_key` is looked up in the policy's own norm_stats when it has them); without per-policy heads the discrete token path with the
        shared lm_head.  `pad_to` repeats observation 0's policy.  On a model built with use_film="per_policy" (pass use_film=True) each observation's
        towers are modulated by its own policy's FiLM Linears (one ovla_film_vectors launch per forward), and `policy` is required.  A model with
        its own FiLM Linears and diffusion heads are not supported with `policy`.
        `output_attentions=True` returns a third element, an ActionAttention: the head-averaged attention of every observation's action rows, from the
        eager forward (routed with `policy`; no graph is used or built).  An observation's maps are the same bits alone and in any batch, up to its own
        key length; its padding keys are 0.  Not with a diffusion head (ValueError).
        `do_sample=True` (the discrete token path without `policy`; ValueError otherwise): every observation's action tokens are drawn from
        softmax(logits[action ids] / temperature) on the device, inside the captured graph under graph replay (ovla_sample_tokens in place of
        ovla_argmax_bins; each replay draws under the `call` its load() wrote).  `sample_keys` [B]: each observation's key in the generator (default
        its index) -- an observation draws the same tokens alone and in any batch under the same key and call.  `return_tokens=True` appends a
        SampledTokens.  Every sampled call advances the engine's token stream by one; `sample_seed` replaces its seed for this call.
        `num_samples=G` (with do_sample=True, the eager path only): G draws per observation from the ONE forward (one ovla_sample_tokens_group
        launch): actions [B, G, chunk, action_dim], SampledTokens with tokens / logprobs [B, G, A] and entropy [B, A]; `sample_keys` [B, G]
        (default b * G + g) -- draw (b, g) is the num_samples=None draw of observation b under the key sample_keys[b, g].  Under graph replay it
        raises: the captured decode holds one draw per observation.
        `action_noise_scale` (an L1 `action_head` without `policy`, the eager path only; ValueError otherwise, before anything advances): every
        observation's actions are ONE draw from the Laplace policy of that scale around the head's prediction (one ovla_laplace_sample launch for
        the batch); `sample_keys` [B] as above -- an observation draws the same chunk alone and in any batch under the same key and call.
        `return_sample=True` appends a SampledActions.  The call advances the engine's token stream by one.  action_noise_scale="learned": the
        model's scale head (attach_scale_head / load_scale_head) sets the widths, as in predict_action."""
        cfg = self.cfg
        if do_sample and policy is not None:
            raise ValueError("predict_action_batch(do_sample=True) is not supported with per-request policies")
        if action_noise_scale is not None and policy is not None:
            raise ValueError("predict_action_batch(action_noise_scale=...) is not supported with per-request policies")
        if num_samples is not None and self.use_graph:
            raise ValueError("predict_action_batch(num_samples=...) is not supported under graph replay (the captured decode draws once per "
                             "observation): enable_graph_replay(False), or call it once per draw with sample_keys")
        per_policy_film = bool(getattr(self.engine, "film_per_policy", False))
        if use_film != self.engine.use_film:
            raise ValueError(f"use_film={use_film} but the model was built with use_film={self.engine.use_film}")
        B, A = len(prompts), cfg.num_action_tokens
        if B == 0:
            raise ValueError("predict_action_batch: no observations")
        if pixel_values.shape[0] != B:
            raise ValueError(f"predict_action_batch: {B} prompts but pixel_values holds {pixel_values.shape[0]} observations")
        if policy is None and per_policy_film:
            raise ValueError("predict_action_batch: a model built with use_film=\"per_policy\" has no FiLM Linears of its own: name each "
                             "observation's policy (policy=[...])")
        if policy is not None:
            policy = list(policy)
            if self.engine.use_film and not per_policy_film:
                raise ValueError("predict_action_batch(policy=...): a model with its own FiLM Linears serves one policy; per-request policies with FiLM "
                                 "need a base model built with use_film=\"per_policy\" (add_policy(..., film=...))")
            if noisy_action_projector is not None or hasattr(action_head, "noise_scheduler"):
                raise ValueError("predict_action_batch(policy=...): diffusion heads are not supported with per-request policies")
            if action_head is not None or proprio_projector is not None:
                raise ValueError("predict_action_batch(policy=...): the action head and the proprio projector come from each observation's policy")
            if len(policy) != B:
                raise ValueError(f"predict_action_batch: {len(policy)} policy names for {B} observations")
            unknown = sorted({str(p) for p in policy if p not in self._policies})
            if unknown:
                raise ValueError(f"predict_action_batch: unknown policy {unknown} (registered: {list(self._policies)})")
        if pad_to is not None and pad_to > B:
            fill = [0] * (pad_to - B)

            def rep(t):   # [B, ...] -> [pad_to, ...]: observation 0 repeated behind the real ones
                if t is None:
                    return None
                t = t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))
                if t.shape[0] != B:
                    raise ValueError(f"predict_action_batch: a per-observation input holds {t.shape[0]} rows for {B} observations")
                return torch.cat([t, t[fill]])

            prop_p = rep(proprio)
            res = self.predict_action_batch(list(prompts) + [prompts[0]] * len(fill), rep(pixel_values), unnorm_key=unnorm_key,
                                            proprio=None if prop_p is None else prop_p.cpu().numpy(), proprio_projector=proprio_projector,
                                            action_head=action_head, noisy_action_projector=noisy_action_projector, use_film=use_film,
                                            noise=rep(noise), policy=None if policy is None else policy + [policy[0]] * len(fill),
                                            output_attentions=output_attentions, do_sample=do_sample, temperature=temperature, sample_seed=sample_seed,
                                            sample_keys=None if sample_keys is None else list(sample_keys) + [list(sample_keys)[0]] * len(fill),
                                            return_tokens=return_tokens, num_samples=num_samples, action_noise_scale=action_noise_scale,
                                            return_sample=return_sample)
            tail = ()
            if return_sample:
                tail, res = (SampledActions(*(None if t is None else t[:B] for t in res[-1])),), res[:-1]
            if return_tokens:
                tail = (SampledTokens(*(t[:B] for t in res[-1])),) + tail
            if output_attentions:
                att = res[2]
                return (res[0][:B], res[1][:B], ActionAttention(att.mean[:, :B], att.layout[:B], att.patches_per_image)) + tail
            return (res[0][:B], res[1][:B]) + tail
        use_proprio = proprio_projector is not None and proprio is not None
        if policy is not None:
            use_proprio = proprio is not None and next(iter(self._policies.values()))["pp"] is not None
        prop = None
        if use_proprio:
            prop = torch.as_tensor(np.asarray(proprio), dtype=torch.float32)
            if prop.ndim != 2 or prop.shape[0] != B:
                raise ValueError(f"predict_action_batch: proprio must be [{B}, proprio_dim], got {tuple(prop.shape)}")
        use_diffusion = noisy_action_projector is not None and hasattr(action_head, "noise_scheduler")
        rows = []   # per sample: prompt (+ 29871) + A action slots + stop, as predict_action builds it (:974-993)
        for ids, mask in prompts:
            ids = torch.as_tensor(ids).to("cpu", torch.int64).reshape(-1)
            mask = torch.ones_like(ids, dtype=torch.bool) if mask is None else torch.as_tensor(mask).to("cpu").reshape(-1).bool()
            if mask.shape != ids.shape:
                raise ValueError("predict_action_batch: input_ids and attention_mask lengths differ")
            n = int(self.engine.check_right_padding(mask[None])[0])
            ids = ids[:n]
            if n == 0 or int(ids[-1]) != 29871:
                ids = torch.cat([ids, torch.tensor([29871], dtype=torch.int64)])
            rows.append(torch.cat([ids, torch.ones(A, dtype=torch.int64), torch.tensor([STOP_INDEX], dtype=torch.int64)]))
        # right-pad to a bucket (a multiple of 8; at least 65 - P so that every composition takes the same attention variant, S > 64)
        P = self.engine.num_patches_total(pixel_values.shape[1] // 6, use_proprio, use_diffusion)
        Lb = max(max(len(r) for r in rows), 65 - P)
        Lb = (Lb + 7) // 8 * 8
        ids = torch.full((B, Lb), cfg.pad_token_id, dtype=torch.int64)
        mask = torch.zeros((B, Lb), dtype=torch.bool)
        labels = torch.full((B, Lb), IGNORE_INDEX, dtype=torch.int64)
        for b, r in enumerate(rows):
            ids[b, : len(r)], mask[b, : len(r)] = r, True
            labels[b, len(r) - A - 1: len(r)] = ACTION_TOKEN_BEGIN_IDX + 1
            labels[b, len(r) - 1] = STOP_INDEX
        attention = {} if output_attentions else None
        extra = (lambda: (self._action_attention(attention, mask, pixel_values, use_proprio),)) if output_attentions else (lambda: ())
        laplace = self._laplace_spec(action_noise_scale, sample_keys, B, action_head=action_head, noisy_action_projector=noisy_action_projector,
                                     return_sample=return_sample)
        sample = self._sample_spec(do_sample, temperature, sample_seed, sample_keys, B, action_head is None and policy is None, return_tokens, num_samples)
        laplace = self._laplace_advance(laplace, sample_seed)
        if policy is not None and self._pool_resident:
            normalized, hidden = self._infer_pooled(ids, mask, labels, pixel_values, prop, policy, use_proprio, attention=attention)
            stats = [self.policy_norm_stats(p) for p in policy]
            return (np.stack([self._unnormalize_actions(normalized[b], unnorm_key, stats[b]) for b in range(B)]), hidden) + extra()
        if policy is not None:   # each observation under its own policy's adapter slot, head, proprio projector and statistics
            names = list(self._policies)
            pols = list(self._policies.values())
            heads = [p["head"].comp for p in pols] if pols[0]["head"] is not None else None
            pps = [p["pp"].comp for p in pols] if use_proprio else None
            normalized, hidden = self._infer(ids, mask, labels, pixel_values, prop, batch=True, policy=([names.index(p) for p in policy], heads, pps),
                                             attention=attention)
            stats = [self.policy_norm_stats(p) for p in policy]
            return (np.stack([self._unnormalize_actions(normalized[b], unnorm_key, stats[b]) for b in range(B)]), hidden) + extra()
        normalized, hidden = self._infer(ids, mask, labels, pixel_values, prop, batch=True, action_head=action_head, proprio_projector=proprio_projector,
                                         noisy_action_projector=noisy_action_projector, noise=noise, attention=attention, sample=sample, laplace=laplace)
        return ((np.stack([self._unnormalize_actions(normalized[b], unnorm_key) for b in range(B)]), hidden) + extra() + self._sampled_tokens(sample, B, return_tokens)
                + self._sampled_actions(laplace, return_sample))

    # -- statistics (:772-791, :1062-1087) -------------------------------------------------------------------------------
    @staticmethod
    def _check_unnorm_key(norm_stats, unnorm_key):
        if unnorm_key is None:
            assert len(norm_stats) == 1, (
                f"Your model was trained on more than one dataset, please pass a `unnorm_key` from the following options to choose the "
                f"statistics used for un-normalizing actions: {norm_stats.keys()}")
            unnorm_key = next(iter(norm_stats.keys()))
        assert unnorm_key in norm_stats, (
            f"The `unnorm_key` you chose is not in the set of available dataset statistics, please choose from: {norm_stats.keys()}")
        return unnorm_key

    def get_action_dim(self, unnorm_key=None) -> int:
        return len(self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]["min"])

    def get_action_stats(self, unnorm_key=None, norm_stats=None):
        norm_stats = self.norm_stats if norm_stats is None else norm_stats   # a policy's own statistics (add_policy)
        return norm_stats[self._check_unnorm_key(norm_stats, unnorm_key)]["action"]

    def _unnormalize_actions(self, normalized_actions, unnorm_key=None, norm_stats=None):
        stats = self.get_action_stats(unnorm_key, norm_stats)
        if self.cfg.norm_type == "bounds":
            mask = stats.get("mask", np.ones_like(stats["min"], dtype=bool))
            high, low = np.array(stats["max"]), np.array(stats["min"])
        elif self.cfg.norm_type == "bounds_q99":
            mask = stats.get("mask", np.ones_like(stats["q01"], dtype=bool))
            high, low = np.array(stats["q99"]), np.array(stats["q01"])
        else:
            raise ValueError("Unsupported action/proprio normalization type detected!")
        return np.where(mask, 0.5 * (normalized_actions + 1) * (high - low + 1e-8) + low, normalized_actions)

    # -- checkpoint surface --------------------------------------------------------------------------------------------
    def lora_state_dict(self) -> Dict[str, torch.Tensor]:
        """LoRA adapters under `<linear>.lora_A.weight` / `.lora_B.weight` (peft adds `base_model.model.` + `.default`)."""
        out = {}
        for lin in self.engine.vlm_linears():
            out.update(lin.export("data"))
        return {k: v.detach().clone() for k, v in out.items()}
