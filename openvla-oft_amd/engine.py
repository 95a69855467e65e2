"""Execution engine of the OpenVLA-OFT action-chunk path on MI355X.

Host-side orchestration only: every tensor op below is a hand-written gfx950 kernel reached through the C-ABI
(`ops.py` -> libovla_hip.so).  PyTorch supplies device memory and the HIP stream.  Forward and backward are written
out explicitly per block (no autograd tape, no tracing compiler): each `fwd` returns the activations its `bwd` needs.

HBM layout (sized for 288 GB):
  * frozen base weights are resident twice, as W [out, in] and W^T [in, out], so forward AND data-gradient GEMMs are
    the same K-contiguous "NT" kernel (no transposed-operand kernel variants, no per-step transposes);
  * Llama q|k|v and gate|up are fused along N; their LoRA pairs are stacked the same way and ride in the GEMM's
    K-extension (one launch per fused linear);
  * all trainable tensors (LoRA A/B, action head, projectors) are views into two flat buffers (bf16 / fp32) with matching
    flat fp32 gradient buffers: one fused AdamW launch and one RCCL all-reduce per dtype bucket;
  * activations for the backward stay resident in bf16 (no recompute at 288 GB).
"""
from __future__ import annotations

import contextlib
import logging
import math
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import os

import numpy as np
import torch

from . import _lib, ops
from .config import VLAConfig, VitConfig
from .policy_pool import Residency

BF16 = torch.bfloat16
F32 = torch.float32
# Which activation derivatives ride in the data-gradient GEMM's epilogue (ovla.h "backward epilogues"): none | act | swiglu | all.
# Bit-identical to the separate act_bwd / swiglu_bwd kernels and it saves the dh round trip, but measured on MI355X it is NOT faster
# (B = 8: none 177.1-177.6 ms/step, act 177.5-178.0, swiglu 178.0, all 178.1-178.4): a 256x256 tile owns its CU, so the extra epilogue
# traffic is exposed, while the separate elementwise kernels already run at the HBM roofline.  Round 2 moved SwiGLU' into the UNROLLED epilogue
# (gemm_nt.hip fast_swiglu_bwd): still no gain (170.0 / 170.4 with vs 170.5 / 170.3 without).  Default: separate kernels.
_FUSE = os.environ.get("OVLA_FUSE_DACT", "none")
# The forward RoPE rides in the q|k|v projection's epilogue (bit-identical to the separate rope pass).  Round 1 had it only in the 4x2-wave
# layout's ROLLED epilogue, where it cost more than the 33 us pass it replaced (177.8-178.0 vs 176.7-177.0 ms/step) and was left off; round 2
# put it into the default 2x4 layout's unrolled read-back (a wave takes its columns together with their rotation partners: no extra LDS
# traffic beyond one more slab read, no barrier) -- see DESIGN.md section 6 for the A/B.  OVLA_FUSE_ROPE_FWD=0 restores the separate pass.
# The INVERSE RoPE of the backward, which needs no loads beyond the tables and no LDS (attention-backward epilogue), is on: -0.6 ms.
_FUSE_ROPE_FWD = os.environ.get("OVLA_FUSE_ROPE_FWD", "1") == "1"
_GROUP_TN = os.environ.get("OVLA_GROUP_TN", "1") == "1"   # ViT blocks: two neighbouring linears' LoRA weight-gradient problems in one launch (A/B switch)
_FUSE_ACT, _FUSE_SWIGLU = _FUSE in ("act", "all"), _FUSE in ("swiglu", "all")
# OVLA_ASYNC_UPLOAD=0: upload ids / labels / lengths with synchronous pageable copies as before (A/B switch of VLAEngine.forward's pinned upload)
_ASYNC_UPLOAD = os.environ.get("OVLA_ASYNC_UPLOAD", "1") != "0"
# OVLA_FOLD_RMSNORM=0: keep the decoder's RMSNorms as their own launches on the merged inference path (A/B switch of LlamaStack.fold_norms).
_FOLD_RMSNORM = os.environ.get("OVLA_FOLD_RMSNORM", "1") != "0"
# OVLA_INFER_W4=0: the folded inference path's projections take the planner's tile instead of the 4-wave 128x256 configuration (A/B switch of LlamaStack._infer_tile)
_INFER_W4 = os.environ.get("OVLA_INFER_W4", "1") != "0"
# OVLA_LORA_DROPOUT_FUSED=0: with lora_dropout > 0 the training forward materialises dropout_g(x) per fused group (ovla_lora_dropout_apply) and
# projects each with an ordinary GEMM, instead of masking the fragments in registers (ovla_lora_dropout_proj).  Same masks; A/B switch.
_LORA_DROPOUT_FUSED = os.environ.get("OVLA_LORA_DROPOUT_FUSED", "1") != "0"


# ======================================================================================================================
# trainable-parameter store
# ======================================================================================================================
class Param:
    """Handle to one trainable tensor living in a flat buffer (`data`), with its fp32 gradient view (`grad`)."""

    def __init__(self, name, init: torch.Tensor):
        self.name, self.shape, self.dtype = name, tuple(init.shape), init.dtype
        self._init = init
        self.data: Optional[torch.Tensor] = None
        self.grad: Optional[torch.Tensor] = None
        self.offset = 0

    @property
    def numel(self):
        return math.prod(self.shape)


class ParamStore:
    ALIGN = 64  # elements; keeps every view 128-byte aligned

    def __init__(self, device):
        self.device = device
        self.params: List[Param] = []
        self.flat: Dict[torch.dtype, torch.Tensor] = {}
        self.flat_grad: Dict[torch.dtype, torch.Tensor] = {}
        self.exp_avg: Dict[torch.dtype, torch.Tensor] = {}
        self.exp_avg_sq: Dict[torch.dtype, torch.Tensor] = {}
        self.step = 0
        self.finalized = False
        self.ema_shadow: Optional[Dict[torch.dtype, torch.Tensor]] = None   # weight EMA (enable_ema): one fp32 shadow per flat buffer
        self.ema_step = 0
        self.fp32_state = False   # enable_fp32_state: the bf16 buffer's AdamW runs on an fp32 master copy and fp32 moments
        self.master: Dict[torch.dtype, torch.Tensor] = {}   # {BF16: fp32 master of flat[BF16]} in fp32 mode; flat[BF16] == bf16_rne(master)

    def add(self, name: str, init: torch.Tensor) -> Param:
        assert not self.finalized and init.dtype in (BF16, F32)
        p = Param(name, init.to(self.device))
        self.params.append(p)
        return p

    def finalize(self):
        """Lays the tensors out in REVERSE registration order (= the order the backward produces their gradients), so
        gradient buckets complete front to back."""
        for dtype in (BF16, F32):
            group = [p for p in reversed(self.params) if p.dtype == dtype]
            total = 0
            for p in group:
                p.offset = total
                total += (p.numel + self.ALIGN - 1) // self.ALIGN * self.ALIGN
            if total == 0:
                continue
            flat = torch.zeros(total, dtype=dtype, device=self.device)
            grad = torch.zeros(total, dtype=F32, device=self.device)
            for p in group:
                p.data = flat[p.offset: p.offset + p.numel].view(p.shape)
                p.data.copy_(p._init)
                p.grad = grad[p.offset: p.offset + p.numel].view(p.shape)
                p._init = None
            self.flat[dtype], self.flat_grad[dtype] = flat, grad
        self.finalized = True

    def init_optimizer(self):
        for dtype, flat in self.flat.items():
            state_dtype = F32 if self.fp32_state else dtype
            self.exp_avg[dtype] = torch.zeros_like(flat, dtype=state_dtype)
            self.exp_avg_sq[dtype] = torch.zeros_like(flat, dtype=state_dtype)
        self.step = 0

    # -- fp32 optimizer state for the bf16 buffer (ovla.h "AdamW on fp32 master weights"): opt-in, the default is torch's bf16 state ---------------
    def enable_fp32_state(self):
        """From now on the bf16 flat buffer's AdamW step is ovla_adamw_master: an fp32 master copy (the current parameters widened exactly) and
        fp32 moments (existing bf16 moments widened exactly, a fresh optimizer's zeros) take the update, and the bf16 buffer is bf16_rne(master)
        after every step.  The fp32 flat buffer keeps ovla_adamw.  Idempotent."""
        if self.fp32_state:
            return
        self.fp32_state = True
        if BF16 not in self.flat:
            return
        self.rewiden_master()
        if self.exp_avg:
            self.exp_avg[BF16], self.exp_avg_sq[BF16] = self.exp_avg[BF16].float(), self.exp_avg_sq[BF16].float()

    def rewiden_master(self):
        """master <- the bf16 parameters widened exactly: after anything but the optimizer has written the flat buffer (a checkpoint load)."""
        if not self.fp32_state or BF16 not in self.flat:
            return
        if BF16 not in self.master:
            self.master[BF16] = torch.empty(self.flat[BF16].numel(), dtype=F32, device=self.device)
        ops.cvt_bf16_to_f32(self.flat[BF16], self.master[BF16])

    def master_matches_param(self) -> bool:
        """bf16_rne(master) == param, bit for bit, checked on the device (one boolean is read back)."""
        if BF16 not in self.master:
            return True
        rounded = ops.cvt_f32_to_bf16(self.master[BF16])
        return bool(torch.equal(rounded.view(torch.int16), self.flat[BF16].view(torch.int16)))

    def zero_grad(self):
        for g in self.flat_grad.values():
            g.zero_()

    def adamw_step(self, lr: float, *, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, clip_state=None):
        """torch.optim.AdamW(trainable_params, lr) of vla-scripts/finetune.py:952 as one fused launch per dtype.  With `clip_state` (the device
        state VLAEngine.adamw_step filled, ovla.h "Gradient-norm clipping") the launches are ovla_adamw_clipped: the gradient is scaled by the
        state's coefficient, and a step the state marks as skipped writes nothing.  `step` advances either way -- the host never learns of a
        skip -- so a skipped step consumes its step number in the bias correction (and, in the driver, in the LR schedule).  In fp32 mode
        (enable_fp32_state) the bf16 buffer's launch is ovla_adamw_master, with or without the state."""
        if not self.exp_avg:
            self.init_optimizer()
        self.step += 1
        for dtype, flat in self.flat.items():
            if dtype in self.master:   # fp32 state: the update runs on the master, the bf16 buffer receives its rounding
                ops.adamw_master(self.master[dtype], self.exp_avg[dtype], self.exp_avg_sq[dtype], flat, self.flat_grad[dtype], step=self.step, lr=lr,
                                 beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale, clip_state=clip_state)
            elif clip_state is None:
                ops.adamw(flat, self.exp_avg[dtype], self.exp_avg_sq[dtype], self.flat_grad[dtype], step=self.step, lr=lr, beta1=beta1,
                          beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale)
            else:
                ops.adamw_clipped(flat, self.exp_avg[dtype], self.exp_avg_sq[dtype], self.flat_grad[dtype], clip_state, step=self.step, lr=lr,
                                  beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale)

    # -- weight EMA (ovla.h "Weight EMA"): the reference has none; diffusers' EMAModel, which Diffusion Policy evaluates on ------------------------
    def enable_ema(self):
        """One fp32 shadow per flat buffer, initialised exactly from the current parameters (bf16 widened, fp32 copied); ema_step = 0.  In fp32
        mode the bf16 buffer's shadow starts from, and ema_update follows, its fp32 master."""
        self.ema_shadow = {}
        for dtype, flat in self.flat.items():
            shadow = torch.empty(flat.numel(), dtype=F32, device=self.device)
            if dtype in self.master:
                shadow.copy_(self.master[dtype])
            elif dtype == BF16:
                ops.cvt_bf16_to_f32(flat, shadow)
            else:
                shadow.copy_(flat)
            self.ema_shadow[dtype] = shadow
        self.ema_step = 0

    def ema_update(self, decay: float):
        """shadow <- shadow - (1 - decay) (shadow - param), one launch per dtype; 1 - decay is formed in double and rounded to fp32 once."""
        if self.ema_shadow is None:
            raise RuntimeError("ema_update without enable_ema()")
        self.ema_step += 1
        for dtype, flat in self.flat.items():
            ops.ema_update(self.master.get(dtype, flat), self.ema_shadow[dtype], 1.0 - float(decay))

    def ema_swap_in(self) -> Dict[torch.dtype, torch.Tensor]:
        """Writes the averaged weights over the live ones -- bf16_rne(shadow) into the bf16 buffer, shadow into the fp32 one -- and returns
        copies of the live buffers for ema_restore."""
        stash = {dtype: flat.clone() for dtype, flat in self.flat.items()}
        for dtype, flat in self.flat.items():
            if dtype == BF16:
                ops.cvt_f32_to_bf16(self.ema_shadow[dtype], flat)
            else:
                flat.copy_(self.ema_shadow[dtype])
        return stash

    def ema_restore(self, stash: Dict[torch.dtype, torch.Tensor]):
        for dtype, flat in self.flat.items():
            flat.copy_(stash[dtype])

    def num_trainable(self):
        return sum(p.numel for p in self.params)

    def named(self) -> Dict[str, Param]:
        return {p.name: p for p in self.params}


# ======================================================================================================================
# linears
# ======================================================================================================================
MAX_SLOTS = 4   # adapters that ride in one launch (K2 = n * r <= 128 at r = 32)


def slot_a_rows(g: int, s: int, n: int, r: int) -> slice:
    """Rows of A_slots (= columns of t) that hold group g of adapter slot s: group-major, [(g n + s) r, (g n + s + 1) r)."""
    return slice((g * n + s) * r, (g * n + s + 1) * r)


def fill_slot(A_slots, B_slots, s: int, lora_A, lora_B, groups: int):
    """Writes adapter s into the slot storage of one (fused) linear: A_slots [G*n*r, in], B_slots [out, n*r]; lora_A is [G*r, in] (the groups'
    lora_A stacked), lora_B is [out, r].  THE layout (LoraLinear.set_slot goes through here): with t = s * x . A_slots^T and every column block
    of a foreign slot zeroed per row, the K-extended GEMM  y = x W^T + t_g . B_slots[group g rows]^T  gives each row  x W^T + t_own B_own^T."""
    r = lora_B.shape[1]
    n = B_slots.shape[1] // r
    for g in range(groups):
        A_slots[slot_a_rows(g, s, n, r)] = lora_A[g * r:(g + 1) * r].to(A_slots.device, A_slots.dtype)
    B_slots[:, s * r:(s + 1) * r] = lora_B.to(B_slots.device, B_slots.dtype)


class SlotRoute:
    """The engine-level routing context of multi-policy serving: which adapter slot each observation of the running forward takes, as a DEVICE
    int32 buffer (so a captured graph serves any assignment), and how many observations there are.  Every slotted LoraLinear holds the engine's
    one instance and derives rows_per_obs from its own row count (rows are ordered by observation everywhere: towers (b, img, token),
    projector (b, patch), decoder (b, s), selected action rows (b, a))."""

    def __init__(self):
        self.obs_slot: Optional[torch.Tensor] = None
        self.n_obs = 0
        self.host_slots: Optional[List[int]] = None   # the same values on the host where the caller has them: the library validates them


class DropoutState:
    """The engine-level state of peft's lora_dropout (finetune.py:119 -> LoraConfig): probability, 64-bit seed, the 32-bit `call` counter that
    advances once per training forward (every micro-batch of a gradient accumulation draws fresh masks) and whether the running forward drops.
    Every adapted LoraLinear holds the engine's one instance; the masks themselves are never stored (ovla.h "LoRA dropout")."""

    def __init__(self, p: float = 0.0, seed: int = 0):
        p = float(p)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"lora_dropout = {p} is outside [0, 1)")
        if p > 0.0 and _FUSE != "none":
            raise ValueError("lora_dropout > 0 cannot be combined with OVLA_FUSE_DACT: the activation derivative cannot ride in the epilogue of a "
                             "data-gradient GEMM whose sum is completed by a later kernel")
        self.p, self.seed, self.call, self.active = p, int(seed) & 0xFFFFFFFFFFFFFFFF, 0, False

    def begin_forward(self, train: bool):
        """Called once per forward: training forwards advance `call` and drop, everything else never drops."""
        self.active = bool(train) and self.p > 0.0
        if self.active:
            self.call = (self.call + 1) & 0xFFFFFFFF

    def end_forward(self):
        """`active` is true only WHILE a training forward runs: whatever calls a linear outside one (a graph's prefix capture through
        patches_dev, a component forward) does not drop.  The backward needs no flag: it takes `call` from what the forward saved."""
        self.active = False


class DiffusionNoiseState:
    """The engine-level state of the diffusion objective's device noise (ovla.h "Diffusion noise"): 64-bit seed, the 32-bit `call` counter that
    advances once per draw (VLAEngine.draw_diffusion) and is checkpointed with the optimizer state, and the device tables of the head's T
    training timesteps -- `ab` / `temb_table` for ovla_diffusion_noise, `coef` / `step_temb` (rows in the sampler's order) for the DDIM loop of
    VLAEngine.sample_actions.  The tables are the host scheduler's and time encoder's own numbers, built once."""

    def __init__(self, num_diffusion_steps: int, seed: int = 0):
        if int(num_diffusion_steps) < 1:
            raise ValueError(f"num_diffusion_steps = {num_diffusion_steps}")
        self.T, self.seed, self.call = int(num_diffusion_steps), int(seed) & 0xFFFFFFFFFFFFFFFF, 0
        self.ab = self.temb_table = self.coef = self.step_temb = None

    def tables(self, D: int, device):
        if self.ab is None:
            from .diffusion import DDIMScheduler, SinusoidalPositionalEncoding

            sched, enc = DDIMScheduler(num_train_timesteps=self.T), SinusoidalPositionalEncoding(D)
            sched.set_timesteps(self.T)
            rows = [enc(torch.tensor([float(t)])).to(BF16).reshape(1, D) for t in range(self.T)]   # row t: what the host path encodes for timestep t
            self.ab = sched.add_noise_coefficients().to(device)
            self.temb_table = torch.cat(rows).contiguous().to(device)
            self.coef = sched.step_coefficients().to(device)
            self.step_temb = torch.cat([rows[int(t)] for t in sched.timesteps]).contiguous().to(device)
        return self


class TokenSampleState:
    """The engine-level state of stochastic action-token decoding (ovla.h "Token sampling and the policy-gradient objective"): 64-bit seed and
    the 32-bit `call` counter that advances once per draw (VLAEngine.sample_action_tokens, a sampled predict_action) and is checkpointed
    with the optimizer state.  A draw is a pure function of (seed, call, row key, token id); nothing else is stored."""

    def __init__(self, seed: int = 0):
        self.seed, self.call = int(seed) & 0xFFFFFFFFFFFFFFFF, 0

    def advance(self) -> int:
        """-> the `call` of this draw; the next draw takes the next one."""
        call = self.call
        self.call = (self.call + 1) & 0xFFFFFFFF
        return call

    def words(self, call: Optional[int] = None) -> List[int]:
        """(seed_lo, seed_hi, call): the three 32-bit words of ovla_sample_tokens' device-side state."""
        return [self.seed & 0xFFFFFFFF, self.seed >> 32, (self.call if call is None else call) & 0xFFFFFFFF]


class SlotProjectors:
    """Every registered policy's proprio projector on all B observations, then each observation's own row (ovla_select_by_slot): n small
    forwards instead of data-dependent grouping, which a captured graph could not hold.  Quacks like MlpProjector.fwd for patches_dev."""

    def __init__(self, comps, route: SlotRoute):
        self.comps, self.route = list(comps), route

    def fwd(self, x, train: bool):
        assert not train, "multi-policy serving is inference-only"
        ys = torch.stack([c.fwd(x, False)[0] for c in self.comps])          # [n, rows padded to 8, D]
        out = torch.zeros_like(ys[0])
        B = self.route.n_obs
        ops.select_by_slot(ys, self.route.obs_slot, rows_per_obs=1, rows=B, out=out[:B], host_slots=self.route.host_slots)
        return out, None


def film_linear_names(towers) -> List[str]:
    """The FiLM Linears of both towers in table order: towers = [(prefix, used blocks, dim)], per block `scale` then `shift`
    (film_vit_wrapper.py:53-54).  The order of ovla_film_vectors' descriptor table and of FilmSlots.names."""
    return [f"{prefix}blocks.{i}.{kind}" for prefix, blocks, _ in towers for i in range(blocks) for kind in ("scale", "shift")]


def fill_film_slot(W_slots, b_slots, s: int, W, b):
    """Writes policy s's Linear (W [dim, D], b [dim]) into the slot storage of one FiLM Linear: W_slots [n, dim, D], b_slots [n, dim].  THE layout
    ovla_film_vectors reads: out[b] = b_slots[slot(b)] + W_slots[slot(b)] . avg[b]."""
    W_slots[s] = W.to(W_slots.device, W_slots.dtype)
    b_slots[s] = b.to(b_slots.device, b_slots.dtype)


def check_film_tensors(film, towers, D: int, device, who: str) -> Dict[str, torch.Tensor]:
    """A policy's FiLM tensors against towers = [(prefix, used blocks, dim)]: the exact key set `<film_linear_names>.{weight,bias}`, shapes
    (dim, D) / (dim,), finite.  -> the tensors in bf16 (RNE from what was given) on `device`.  Raises before anything is changed."""
    if not isinstance(film, dict):
        raise ValueError(f"{who}: `film` must be a dict of the policy's FiLM tensors (vision_backbone.featurizer.blocks.0.scale.weight, ...)")
    dims = {nm: dim for prefix, blocks, dim in towers for nm in film_linear_names([(prefix, blocks, dim)])}
    want = {f"{nm}.{leaf}" for nm in dims for leaf in ("weight", "bias")}
    missing, stray = sorted(want - set(film)), sorted(set(film) - want)
    if missing or stray:
        raise ValueError(f"{who}: the FiLM tensors must be exactly the scale / shift Linears of the towers' used blocks: "
                         f"{len(missing)} missing (e.g. {missing[:2]}), {len(stray)} unknown (e.g. {stray[:2]})")
    out = {}
    for nm, dim in dims.items():
        for leaf, shape in (("weight", (dim, D)), ("bias", (dim,))):
            t = film[f"{nm}.{leaf}"]
            if tuple(t.shape) != shape:
                raise ValueError(f"{who}: {nm}.{leaf} has shape {tuple(t.shape)}, the model's is {shape}")
            if not bool(torch.isfinite(t.float()).all()):
                raise ValueError(f"{who}: {nm}.{leaf} holds non-finite values")
            out[f"{nm}.{leaf}"] = t.detach().to(device, torch.float32).to(BF16).contiguous()
    return out


class FilmSlots:
    """Per-policy FiLM of both towers (multi-policy serving; inference only): per FiLM Linear the n policies' weights W_slots [n, dim, D] and
    biases b_slots [n, dim] in bf16 (the reference evaluates the backbone after `.to(torch.bfloat16)`: RNE from the fp32 checkpoint tensors), the
    gamma / beta output buffers [MAX_OBS, dim] that ONE ovla_film_vectors launch per forward fills for the observations of the batch, and
    the launch's device table, built once per slot allocation.  Empty slots hold zeros and no observation is routed to one."""

    MAX_OBS = ops.FILM_MAX_OBS

    def __init__(self, towers, n: int, D: int, device):
        if not 1 <= n <= MAX_SLOTS:
            raise ValueError(f"FilmSlots: {n} slots (1 .. {MAX_SLOTS} supported)")
        self.n, self.D = n, D
        self.names = film_linear_names(towers)
        dims = [dim for _, blocks, dim in towers for _ in range(2 * blocks)]
        self.W_slots = {nm: torch.zeros((n, dim, D), dtype=BF16, device=device) for nm, dim in zip(self.names, dims)}
        self.b_slots = {nm: torch.zeros((n, dim), dtype=BF16, device=device) for nm, dim in zip(self.names, dims)}
        self.out = {nm: torch.zeros((self.MAX_OBS, dim), dtype=BF16, device=device) for nm, dim in zip(self.names, dims)}
        self.table = ops.film_table([(self.W_slots[nm], self.b_slots[nm], self.out[nm]) for nm in self.names], device)

    def set_slot(self, s: int, film: Dict[str, torch.Tensor]):
        """Policy s from checked tensors (check_film_tensors)."""
        for nm in self.names:
            fill_film_slot(self.W_slots[nm], self.b_slots[nm], s, film[nm + ".weight"], film[nm + ".bias"])

    def slot_pairs(self, s: int, film: Dict[str, torch.Tensor]):
        """(source, destination) of loading checked tensors into slot s: what the policy pool's copy table moves."""
        return [pr for nm in self.names for pr in ((film[nm + ".weight"], self.W_slots[nm][s]), (film[nm + ".bias"], self.b_slots[nm][s]))]

    def launch(self, avg, route: "SlotRoute"):
        """gamma / beta of every block of both towers for the route's observations: ONE launch on the current stream."""
        if route.n_obs > self.MAX_OBS:
            raise ValueError(f"per-policy FiLM: {route.n_obs} observations in one forward (at most {self.MAX_OBS})")
        ops.film_vectors(self.table, avg, route.obs_slot, host_slots=route.host_slots)

    def vectors(self, prefix: str, i: int, n_obs: int):
        """(gamma, beta) [n_obs, dim] of block i of the tower `prefix`: views of the launch's outputs."""
        return self.out[f"{prefix}blocks.{i}.scale"][:n_obs], self.out[f"{prefix}blocks.{i}.shift"][:n_obs]


def launch_tn(probs):
    """The weight-gradient TN problems of one linear, or of a tn_queue, in launches of at most ops.TN_MAX_GROUP (more than one launch only
    with dropout's per-group dA problems on a fused linear: G dB + G dA instead of G + 1)."""
    for i in range(0, len(probs), ops.TN_MAX_GROUP):
        ops.gemm_tn_grouped(probs[i:i + ops.TN_MAX_GROUP])


class LoraLinear:
    """Frozen nn.Linear (+ optional bias) with peft-style LoRA adapters; `groups` fused sub-linears share the input.

    forward:  t_s = s * x A^T ;  y = x W^T (+ bias) + t_s B^T                     (one K-extended GEMM)
    backward: dt  = s * dy_g B_g   (per group);  dx = dy W + dt A                  (one K-extended GEMM on W^T / A^T)
              dB_g += dy_g^T t_s,g ;  dA += dt^T x                                 (TN GEMMs, fp32 accumulate)
    with lora_dropout active (training forwards of an engine built with lora_dropout > 0; masks from ovla.h "LoRA dropout"):
    forward:  t_s,g = s * dropout_g(x) A_g^T  (ovla_lora_dropout_proj: masks in registers), the K-extended GEMM as above
    backward: dx = dy W, then dx += sum_g mask_g * inv * (dt_g A_g) in place (ovla_lora_dropout_backproj);  dA_g += dt_g^T dropout_g(x)
    """

    def __init__(self, store: Optional[ParamStore], name: str, W: torch.Tensor, bias: Optional[torch.Tensor], lora_A: Optional[torch.Tensor],
                 lora_B: Optional[torch.Tensor], groups: int, scale: float, need_dgrad: bool = True, ref_names=None):
        self.name, self.W, self.bias, self.groups, self.scale = name, W.contiguous(), bias, groups, scale
        self.ref_names = ref_names or [name]   # the reference's nn.Linear module path of every fused group
        self.out_f, self.in_f = W.shape
        self.group_n = self.out_f // groups
        self.WT = ops.transpose(self.W) if need_dgrad else None
        self.has_lora = lora_A is not None
        if self.has_lora:
            self.r = lora_A.shape[0] // groups
            assert lora_A.shape == (groups * self.r, self.in_f) and lora_B.shape == (self.out_f, self.r)
            self.A = store.add(name + ".lora_A", lora_A.to(BF16))
            self.B = store.add(name + ".lora_B", lora_B.to(BF16))
            self.AT = None   # [in, G*r]   derived
            self.BT = None   # list of [r, group_n] derived
        self.dropout: Optional[DropoutState] = None   # the engine's DropoutState when lora_dropout > 0 (VLAEngine.__init__)
        self.module_ids: List[int] = []               # one mask stream per fused group (peft: one nn.Dropout per adapted nn.Linear)

    def derived_pairs(self):
        """(src, dst) transposes that re-derive A^T [in, G*r] and the stacked B_g^T [G*r, group_n] from the trainable factors."""
        if not self.has_lora:
            return []
        dev = self.W.device
        if self.AT is None:
            self.AT = torch.empty((self.in_f, self.groups * self.r), dtype=BF16, device=dev)
            self.BT = torch.empty((self.groups * self.r, self.group_n), dtype=BF16, device=dev)
        pairs = [(self.A.data, self.AT)]
        for g in range(self.groups):
            pairs.append((self.B.data[g * self.group_n:(g + 1) * self.group_n], self.BT[g * self.r:(g + 1) * self.r]))
        return pairs

    def refresh_derived(self):
        for src, dst in self.derived_pairs():
            ops.transpose(src, dst)

    def export(self, kind: str = "data") -> Dict[str, torch.Tensor]:
        """Trainable tensors (kind='data') or their fp32 gradients (kind='grad') under the reference/peft-style names."""
        out = {}
        if self.has_lora:
            A, Bm = getattr(self.A, kind), getattr(self.B, kind)
            for g, rn in enumerate(self.ref_names):
                out[rn + ".lora_A.weight"] = A[g * self.r:(g + 1) * self.r]
                out[rn + ".lora_B.weight"] = Bm[g * self.group_n:(g + 1) * self.group_n]
        return out

    def merge(self):
        """W += s * B A in place (peft `merge_and_unload`, vla-scripts/merge_lora_weights_and_save.py:60-67): per fused group
        one rank-r GEMM whose epilogue adds the frozen weight (delta and sum each rounded to bf16, as peft's
        `weight.data += delta` on bf16 tensors).  The adapters stay allocated but are no longer applied: inference only."""
        if not self.has_lora or getattr(self, "merged", False):
            return
        if self.AT is None:
            self.refresh_derived()
        gn, r = self.group_n, self.r
        for g in range(self.groups):
            Wg = self.W[g * gn:(g + 1) * gn]
            ops.gemm(self.B.data[g * gn:(g + 1) * gn], self.AT[:, g * r:(g + 1) * r], out=Wg, residual=Wg, alpha=self.scale)
        if self.WT is not None:
            ops.transpose(self.W, self.WT)
        self.merged = True

    # -- adapter slots (multi-policy serving; inference only) -------------------------------------------------------------------------------
    def init_slots(self, n: int, r: int, route: "SlotRoute"):
        """Frozen storage for n adapters of rank r in the layout of fill_slot (zero until set_slot fills it): A_slots [G*n*r, in] makes the
        ordinary projection GEMM produce t [M, G*n*r] directly, B_slots [out, n*r] is the K-extension's B2.  Only on a linear without adapters of
        its own; `route` is the engine's SlotRoute, whose device obs_slot buffer says which slot each observation takes."""
        if self.has_lora:
            raise ValueError(f"{self.name}: adapter slots need a linear without merged or trainable adapters")
        if not 1 <= n <= MAX_SLOTS:
            raise ValueError(f"{self.name}: {n} adapter slots (1 .. {MAX_SLOTS} supported)")
        if r % 8:
            raise ValueError(f"{self.name}: slot rank {r} must be a multiple of 8")
        dev = self.W.device
        self.n_slots, self.slot_r, self.route = n, r, route
        self.A_slots = torch.zeros((self.groups * n * r, self.in_f), dtype=BF16, device=dev)
        self.B_slots = torch.zeros((self.out_f, n * r), dtype=BF16, device=dev)

    def clear_slots(self):
        self.n_slots, self.A_slots, self.B_slots = 0, None, None

    def set_slot(self, s: int, lora_A: torch.Tensor, lora_B: torch.Tensor):
        """Adapter s: lora_A [G*r, in] (the fused groups' A stacked as in __init__), lora_B [out, r]."""
        n, r, G = self.n_slots, self.slot_r, self.groups
        if not 0 <= s < n:
            raise ValueError(f"{self.name}: slot {s} of {n}")
        if tuple(lora_A.shape) != (G * r, self.in_f) or tuple(lora_B.shape) != (self.out_f, r):
            raise ValueError(f"{self.name}: adapter shapes {tuple(lora_A.shape)} / {tuple(lora_B.shape)} do not fit rank {r} "
                             f"(want {(G * r, self.in_f)} / {(self.out_f, r)})")
        fill_slot(self.A_slots, self.B_slots, s, lora_A, lora_B, G)

    def slots_active(self) -> bool:
        return bool(getattr(self, "n_slots", 0)) and self.route.obs_slot is not None

    def fwd(self, x, *, act=0, residual=None, colscale=None, c_pre=None, film=None, out=None, rope=None):
        """x [M, in] -> (y [M, out], saved).  `rope` = (cos, sin, S, cols): RoPE on the first `cols` output columns in the GEMM epilogue."""
        t_s = None
        if self.slots_active():
            # n adapters in one launch: project against all of them, zero every foreign slot's columns per row (ovla_lora_route: the assignment is
            # device data), then the usual K-extended GEMM with K2 = n * r.  Zeros add nothing to the fp32 accumulator: a row sees its own adapter.
            rt, n, r, M = self.route, self.n_slots, self.slot_r, x.shape[0]
            if M % rt.n_obs:
                raise RuntimeError(f"{self.name}: {M} rows do not divide over {rt.n_obs} observations")
            t_s = ops.gemm(x, self.A_slots, alpha=self.scale)
            ops.lora_route(t_s, rt.obs_slot, G=self.groups, n=n, r=r, rows_per_obs=M // rt.n_obs, host_slots=rt.host_slots)
            y = ops.gemm(x, self.W, out=out, bias=self.bias, act=act, residual=residual, colscale=colscale, c_pre=c_pre, film=film,
                         a2=t_s, b2=self.B_slots, k2_group_n=self.group_n if self.groups > 1 else 0, rope=rope)
            return y, None
        if self.has_lora and not getattr(self, "merged", False):
            do = self.dropout
            if do is not None and do.active:
                # t_s = s * dropout_g(x) . A_g^T with the masks evaluated in registers; the K-extended main GEMM below is the usual one
                key = dict(modules=self.module_ids, p=do.p, seed=do.seed, call=do.call)
                if _LORA_DROPOUT_FUSED and self.r == 32:
                    t_s = ops.lora_dropout_proj(x, self.A.data, alpha=self.scale, **key)
                else:
                    r = self.r
                    xd = ops.lora_dropout_apply(x, **key)
                    t_s = torch.empty((x.shape[0], self.groups * r), dtype=BF16, device=x.device)
                    for g in range(self.groups):
                        ops.gemm(xd[g], self.A.data[g * r:(g + 1) * r], alpha=self.scale, out=t_s[:, g * r:(g + 1) * r])
                y = ops.gemm(x, self.W, out=out, bias=self.bias, act=act, residual=residual, colscale=colscale, c_pre=c_pre, film=film,
                             a2=t_s, b2=self.B.data, k2_group_n=self.group_n if self.groups > 1 else 0, rope=rope)
                return y, (x, t_s, do.call)
            t_s = ops.gemm(x, self.A.data, alpha=self.scale)
            y = ops.gemm(x, self.W, out=out, bias=self.bias, act=act, residual=residual, colscale=colscale, c_pre=c_pre, film=film,
                         a2=t_s, b2=self.B.data, k2_group_n=self.group_n if self.groups > 1 else 0, rope=rope)
        else:
            y = ops.gemm(x, self.W, out=out, bias=self.bias, act=act, residual=residual, colscale=colscale, c_pre=c_pre, film=film, rope=rope)
        return y, (x, t_s)

    def bwd(self, dy, saved, need_dx=True, dact=None, tn_queue=None):
        """dy [M, out] (gradient w.r.t. the pre-activation linear output) -> dx [M, in]; accumulates LoRA grads.
        `dact` = ("act", z, act_id) / ("swiglu", gu): the data-gradient GEMM's epilogue also applies the derivative of the
        activation that PRODUCED this linear's input (returns dz / d(gate|up) instead of dx: ovla.h backward epilogues).
        `tn_queue`: a list that collects this linear's weight-gradient TN problems instead of launching them; the caller launches the
        list (ops.gemm_tn_grouped) BEFORE anything overwrites `dy` -- two neighbouring linears' four small problems share one launch."""
        if getattr(self, "n_slots", 0):
            raise RuntimeError(f"{self.name}: this linear carries adapter slots (multi-policy serving); that path is inference-only")
        x, t_s = saved[:2]
        drop_call = saved[2] if len(saved) > 2 else None   # the forward dropped: its masks are regenerated from (seed, call, module)
        dx = None
        if getattr(self, "merged", False):
            raise RuntimeError(f"{self.name}: LoRA adapters were merged into the base weight; this engine is inference-only")
        if self.has_lora:
            r, G, gn = self.r, self.groups, self.group_n
            # dt[:, g] = s * dy_g . B_g for every fused group in ONE block-diagonal skinny GEMM
            dt = ops.gemm(dy, self.BT, alpha=self.scale, a_group_n=r if G > 1 else 0)
            # dB_g += dy_g^T t_g ; dA += dt^T x : one grouped launch
            probs = [(dy[:, g * gn:(g + 1) * gn], t_s[:, g * r:(g + 1) * r], self.B.grad[g * gn:(g + 1) * gn]) for g in range(G)]
            probs.append((dt, x, self.A.grad))
            if drop_call is not None:
                # dA_g += dt_g^T dropout_g(x): the dropped input is regenerated into a buffer of its own (not a fixed workspace: tn_queue may launch
                # the problem later, and the two towers run on two streams)
                assert dact is None, "lora_dropout: a fused activation derivative needs the complete dx"
                do = self.dropout
                key = dict(modules=self.module_ids, p=do.p, seed=do.seed, call=drop_call)
                xd = ops.lora_dropout_apply(x, **key)
                probs.pop()
                probs.extend((dt[:, g * r:(g + 1) * r], xd[g], self.A.grad[g * r:(g + 1) * r]) for g in range(G))
            if tn_queue is not None:
                tn_queue.extend(probs)
            else:
                launch_tn(probs)
            if need_dx and drop_call is not None:
                dx = ops.gemm(dy, self.WT)
                ops.lora_dropout_backproj(dx, dt, self.AT, **key)
            elif need_dx:
                dx = ops.gemm(dy, self.WT, a2=dt, b2=self.AT, dact=dact)
        elif need_dx:
            dx = ops.gemm(dy, self.WT, dact=dact)
        return dx


class FullLinear:
    """Fully trainable nn.Linear (action head, proprio / noisy-action projector, FiLM).  `master_fp32`: parameters live
    in fp32 (the reference never casts these modules, finetune.py:895-901) and a bf16 compute copy is refreshed after
    each optimizer step -- what autocast does on every call.  The input width is zero-padded to a multiple of 8 (the
    GEMM's K granularity; proprio_dim 8, noisy-action dim 1): the padded columns see zero inputs, get zero gradients
    and stay zero, and are sliced off on export."""

    def __init__(self, store: ParamStore, name: str, W: torch.Tensor, bias: Optional[torch.Tensor], master_fp32: bool = False):
        dt = F32 if master_fp32 else BF16
        self.name, self.master_fp32 = name, master_fp32
        self.out_f, self.in_f = W.shape
        self.in_pad = (self.in_f + 7) // 8 * 8
        Wp = torch.zeros((self.out_f, self.in_pad), dtype=dt, device=W.device)
        Wp[:, : self.in_f] = W.to(dt)
        self.W = store.add(name + ".weight", Wp)
        self.b = store.add(name + ".bias", bias.to(dt)) if bias is not None else None
        self.Wc = self.bc = None

    def derived_pairs(self):
        return []   # nothing to transpose; the bf16 compute copy is refreshed by refresh_derived()

    def refresh_derived(self):
        if self.master_fp32:
            self.Wc = ops.cvt_f32_to_bf16(self.W.data, self.Wc)
            if self.b is not None:
                self.bc = ops.cvt_f32_to_bf16(self.b.data, self.bc)
        else:
            self.Wc, self.bc = self.W.data, (None if self.b is None else self.b.data)

    def export(self, kind: str = "data") -> Dict[str, torch.Tensor]:
        out = {self.name + ".weight": getattr(self.W, kind)[:, : self.in_f]}
        if self.b is not None:
            out[self.name + ".bias"] = getattr(self.b, kind)
        return out

    def fwd(self, x, *, act=0, residual=None, c_pre=None, split_k=1):
        y = ops.gemm(x, self.Wc, bias=self.bc, act=act, residual=residual, c_pre=c_pre, split_k=split_k)
        return y, (x,)

    def bwd(self, dy, saved, need_dx=True):
        (x,) = saved
        M = dy.shape[0]
        ops.gemm_tn(dy, x, out=self.W.grad)
        if self.b is not None:
            ops.colsum(dy, self.b.grad)
        if not need_dx:
            return None
        if M % 8 != 0:
            raise RuntimeError(f"{self.name}: row count {M} must be a multiple of 8 for the data gradient")
        dyT = ops.transpose(dy)                                               # [out, M]
        return ops.gemm_tn(dyT, self.Wc, accumulate=False, out_dtype=BF16)   # [M, in] = dy . W  (contract over `out`)


# ======================================================================================================================
# ViT (timm VisionTransformer blocks; reference call site modeling_prismatic.py:127-139,186-227)
# ======================================================================================================================
ACT_ID = {"gelu": ops.ACT_GELU, "gelu_tanh": ops.ACT_GELU_TANH}


def lora_predicate(lora, has):
    """`lora` True / False: every adapted Linear / none.  "auto": exactly the Linears whose adapter tensors are in the state dict -- a merged
    checkpoint whose vision backbone still carries its adapters (the reference's FiLM evaluation path re-attaches LoRA to the towers only:
    experiments/robot/openvla_utils.py:311-349) loads with adapters on the towers and none on the decoder."""
    if lora == "auto":
        if has is None:
            raise ValueError('lora="auto" needs the state dict\'s `has`')

        def pred(names):
            flags = [has(n + ".lora_A.weight") for n in names]
            if any(flags) != all(flags):
                raise ValueError(f"LoRA adapters present for only some of the fused linears {names}")
            return flags[0]

        return pred
    return lambda names: bool(lora)


class VitTower:
    def __init__(self, store, prefix: str, vc: VitConfig, get, cfg: VLAConfig, lora, film: bool = False):
        self.vc, self.prefix = vc, prefix
        lora = lora if callable(lora) else lora_predicate(lora, None)
        w = get(prefix + "patch_embed.proj.weight").reshape(vc.dim, -1)                 # [dim, 3*p*p]
        self.patch_w = torch.zeros((vc.dim, vc.patch_k), dtype=BF16, device=w.device)
        self.patch_w[:, : w.shape[1]] = w
        self.patch_b = get(prefix + "patch_embed.proj.bias")
        self.pos = get(prefix + "pos_embed").reshape(vc.n_patches, vc.dim).contiguous()
        pre = []
        if vc.n_prefix > 0:
            pre.append(get(prefix + "cls_token").reshape(1, vc.dim))
            if vc.n_prefix > 1:
                pre.append(get(prefix + "reg_token").reshape(vc.n_prefix - 1, vc.dim))
        self.prefix_tokens = torch.cat(pre, 0).contiguous() if pre else None
        self.act = ACT_ID[vc.act]
        self.blocks = []
        s = cfg.lora_scale

        def L(name, groups=1):
            A = get(name + ".lora_A.weight") if lora([name]) else None
            Bm = get(name + ".lora_B.weight") if lora([name]) else None
            return LoraLinear(store, name, get(name + ".weight"), get(name + ".bias"), A, Bm, groups, s)

        # only blocks 0 .. depth-2 are ever used: the forward returns the output of block depth-2
        # (get_intermediate_layers(n={depth-2})); the last block's output is discarded (film_vit_wrapper.py:124-137)
        self.film = film
        self.film_slots: Optional[FilmSlots] = None   # film == "per_policy": the engine's FilmSlots once slots are allocated (VLAEngine._alloc_film_slots)
        for i in range(vc.depth - 1):
            p = f"{prefix}blocks.{i}."
            fl = None
            if film and film != "per_policy":   # film_vit_wrapper.py:53-54: fp32 nn.Linear(llm_dim, vision_dim) pairs, trained in full
                fl = (FullLinear(store, p + "scale", get(p + "scale.weight").float(), get(p + "scale.bias").float(), master_fp32=True),
                      FullLinear(store, p + "shift", get(p + "shift.weight").float(), get(p + "shift.bias").float(), master_fp32=True))
            blk = dict(film=fl, ln1_w=get(p + "norm1.weight"), ln1_b=get(p + "norm1.bias"), ln2_w=get(p + "norm2.weight"), ln2_b=get(p + "norm2.bias"),
                       qkv=L(p + "attn.qkv"), proj=L(p + "attn.proj"), fc1=L(p + "mlp.fc1"), fc2=L(p + "mlp.fc2"),
                       ls1=get(p + "ls1.scale_factor") if vc.layerscale else None, ls2=get(p + "ls2.scale_factor") if vc.layerscale else None)
            self.blocks.append(blk)

    def linears(self):
        for b in self.blocks:
            yield from (b["qkv"], b["proj"], b["fc1"], b["fc2"])
            if b["film"] is not None:
                yield from b["film"]

    def export_frozen(self) -> Dict[str, torch.Tensor]:
        """The tower's frozen tensors under their checkpoint names (views, no copies): what `vision_backbone--{step}_checkpoint.pt` carries
        beside the adapters and the FiLM Linears (finetune.py:640-655 saves the whole wrapped backbone)."""
        vc, p = self.vc, self.prefix
        out = {p + "patch_embed.proj.weight": self.patch_w[:, : 3 * vc.patch * vc.patch].reshape(vc.dim, 3, vc.patch, vc.patch),
               p + "patch_embed.proj.bias": self.patch_b, p + "pos_embed": self.pos.reshape(1, vc.n_patches, vc.dim)}
        if self.prefix_tokens is not None:
            out[p + "cls_token"] = self.prefix_tokens[:1].reshape(1, 1, vc.dim)
            if vc.n_prefix > 1:
                out[p + "reg_token"] = self.prefix_tokens[1:].reshape(1, vc.n_prefix - 1, vc.dim)
        for i, b in enumerate(self.blocks):
            q = f"{p}blocks.{i}."
            out.update({q + "norm1.weight": b["ln1_w"], q + "norm1.bias": b["ln1_b"], q + "norm2.weight": b["ln2_w"], q + "norm2.bias": b["ln2_b"]})
            for nm, key in (("attn.qkv", "qkv"), ("attn.proj", "proj"), ("mlp.fc1", "fc1"), ("mlp.fc2", "fc2")):
                if getattr(b[key], "merged", False):
                    raise RuntimeError("the adapters were merged into the base weights: there is no training-time backbone state to export")
                out[q + nm + ".weight"], out[q + nm + ".bias"] = b[key].W, b[key].bias
            if b["ls1"] is not None:
                out[q + "ls1.scale_factor"], out[q + "ls2.scale_factor"] = b["ls1"], b["ls2"]
        return out

    def fwd(self, pixels, c0: int, n_img: int, train: bool, film_avg=None):
        """pixels bf16 [B, 6*n_img, H, W]; image i uses channels [c0 + 6 i, +3).  All images go through the tower as one
        batch of B*n_img (ordered (b, img)).  Returns (tokens [B*n_img*T, dim] after block depth-2, saved)."""
        vc = self.vc
        B = pixels.shape[0] * n_img
        cols = ops.im2col(pixels, c0, vc.patch, vc.patch_k, n_img=n_img, img_cstride=6)
        patches = ops.gemm(cols, self.patch_w, bias=self.patch_b)
        x = ops.vit_embed(patches, self.pos, self.prefix_tokens, B, vc.n_patches, vc.dim)
        T = vc.n_patches + vc.n_prefix
        H, hd = vc.heads, vc.head_dim
        saved = []
        for i, blk in enumerate(self.blocks):
            h1, mean1, rstd1 = ops.norm_fwd(x, blk["ln1_w"], blk["ln1_b"], eps=vc.eps, rms=False, save_stats=train)
            qkv, s_qkv = blk["qkv"].fwd(h1)
            o, lse = ops.attn_fwd(qkv[:, : vc.dim], qkv[:, vc.dim: 2 * vc.dim], qkv[:, 2 * vc.dim:], B, T, H, hd)
            fsv = None
            if self.film == "per_policy":
                # the same modulation with each observation's OWN policy's gamma / beta: views of what the forward's one ovla_film_vectors
                # launch wrote (VLAEngine.vision_fwd) instead of two M = 8 GEMMs per block
                gamma, beta = self.film_slots.vectors(self.prefix, i, pixels.shape[0])
                x2, s_proj = blk["proj"].fwd(o, residual=x, colscale=blk["ls1"], film=(gamma, beta, n_img * T))
            elif blk["film"] is not None:
                # x = (x + ls1 * attn(...)) * (1 + gamma) + beta, gamma/beta = Linear(mean language embedding) per SAMPLE
                # (both images of a sample share them): fused into the proj GEMM's epilogue
                gamma, s_sc = blk["film"][0].fwd(film_avg)
                beta, s_sh = blk["film"][1].fwd(film_avg)
                xpre = torch.empty_like(x) if train else None
                x2, s_proj = blk["proj"].fwd(o, residual=x, colscale=blk["ls1"], film=(gamma, beta, n_img * T), c_pre=xpre)
                fsv = (gamma, s_sc, s_sh, xpre, n_img * T)
            else:
                x2, s_proj = blk["proj"].fwd(o, residual=x, colscale=blk["ls1"])
            h2, mean2, rstd2 = ops.norm_fwd(x2, blk["ln2_w"], blk["ln2_b"], eps=vc.eps, rms=False, save_stats=train)
            z = torch.empty((h2.shape[0], vc.mlp_hidden), dtype=BF16, device=h2.device) if train else None
            hmid, s_fc1 = blk["fc1"].fwd(h2, act=self.act, c_pre=z)
            x3, s_fc2 = blk["fc2"].fwd(hmid, residual=x2, colscale=blk["ls2"])
            if train:
                saved.append((x, mean1, rstd1, s_qkv, qkv, o, lse, s_proj, x2, mean2, rstd2, s_fc1, z, s_fc2, fsv))
            x = x3
        return x, (saved, B)

    def bwd(self, dx, saved_all):
        """dx [B*T, dim]: gradient w.r.t. the tower output (prefix rows already zero).  Pixels need no gradient."""
        vc = self.vc
        saved, B = saved_all
        T = vc.n_patches + vc.n_prefix
        H, hd = vc.heads, vc.head_dim
        for bi, (blk, sv) in enumerate(zip(reversed(self.blocks), reversed(saved))):
            first_block = bi == len(saved) - 1      # block 0: nothing upstream is trainable (patch / position embeddings are frozen)
            x, mean1, rstd1, s_qkv, qkv, o, lse, s_proj, x2, mean2, rstd2, s_fc1, z, s_fc2, fsv = sv
            # x3 = x2 + ls2 * fc2(act(fc1(ln2(x2))))
            d = ops.colscale(dx, blk["ls2"]) if blk["ls2"] is not None else dx
            tnq = [] if _GROUP_TN else None   # fc2's and fc1's LoRA weight gradients: four ~9 MB problems in ONE launch, before norm_bwd rewrites dx
            if _FUSE_ACT:
                dz = blk["fc2"].bwd(d, s_fc2, dact=("act", z, self.act), tn_queue=tnq)  # dh * act'(z) in the dgrad GEMM's epilogue
            else:
                dz = ops.act_bwd(z, blk["fc2"].bwd(d, s_fc2, tn_queue=tnq), self.act)
            dh2 = blk["fc1"].bwd(dz, s_fc1, tn_queue=tnq)
            if tnq:
                launch_tn(tnq)
            ops.norm_bwd(x2, dh2, blk["ln2_w"], mean2, rstd2, rms=False, dx=dx, dx_accum=True)       # dx now = d x2
            if fsv is not None:   # through the FiLM modulation: dgamma, dbeta, dx <- dx * (1 + gamma)
                gamma, s_sc, s_sh, xpre, frows = fsv
                nb = gamma.shape[0]
                dg = torch.zeros((nb, vc.dim), dtype=F32, device=dx.device)
                db = torch.zeros((nb, vc.dim), dtype=F32, device=dx.device)
                ops.film_bwd(dx, xpre, gamma, dg, db, dx.shape[0] // frows, frows)
                blk["film"][0].bwd(ops.cvt_f32_to_bf16(dg), s_sc, need_dx=False)
                blk["film"][1].bwd(ops.cvt_f32_to_bf16(db), s_sh, need_dx=False)
            # x2 = x + ls1 * proj(attn(qkv(ln1(x))))
            d = ops.colscale(dx, blk["ls1"]) if blk["ls1"] is not None else dx
            tnq = [] if _GROUP_TN else None   # likewise proj + qkv
            do = blk["proj"].bwd(d, s_proj, tn_queue=tnq)
            dqkv = torch.empty_like(qkv)
            D = vc.dim
            ops.attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, do, lse, B, T, H, hd, dq=dqkv[:, :D], dk=dqkv[:, D:2 * D],
                         dv=dqkv[:, 2 * D:])
            dh1 = blk["qkv"].bwd(dqkv, s_qkv, need_dx=not first_block, tn_queue=tnq)   # block 0 still needs its LoRA gradients, not d x
            if tnq:
                launch_tn(tnq)
            if not first_block:
                ops.norm_bwd(x, dh1, blk["ln1_w"], mean1, rstd1, rms=False, dx=dx, dx_accum=True)    # dx now = d x
        return None  # patch embedding / position embedding are frozen and the pixels need no gradient


# ======================================================================================================================
# Llama decoder stack (transformers LlamaModel; reference call site modeling_prismatic.py:632-643)
# ======================================================================================================================
class AttnCapture:
    """Asks a forward for the decoder's attention probabilities (`attn_capture=` of VLAEngine.forward / forward_dev, LlamaStack.fwd).

    rows      "actions": the B*A rows that predict the action slots (the assembly kernel's `action_rows`, already on the device: no host
              sync); "all": every one of the B*S rows; or an int32 device tensor of flattened rows b*S + s (any order, repeats allowed,
              an index outside [0, B*S) gives a zero row).
    per_head  also keep the per-head probabilities [n_layers, R, H, S] (the head mean [n_layers, R, S] is always kept).
    layers    the decoder layers to capture (indices, negative ones count from the end); None: all of them.

    The flash kernels never form P: right after each selected layer's ops.attn_fwd ONE ops.attn_probs launch recomputes it for the listed rows
    from the same qkv views and lse.  It reads only, so hidden states, losses and gradients keep their bits.  Both buffers are allocated once
    per forward.  Memory: the mean is R*S*4 bytes per layer (A = 56 of S = 608: 136 KB); rows="all" with per_head is B*H*S*S*4 bytes per
    layer -- 47 MB at the 7B decoder's H = 32, S = 608 and B = 1, 1.5 GB for its 32 layers, 12 GB at B = 8: choose `layers` accordingly.

    After the forward its result dict holds attention = dict(mean, per_head (or None), rows (the int32 tensor, None for "all"), layers)."""

    def __init__(self, rows="actions", per_head: bool = False, layers=None):
        if isinstance(rows, str):
            if rows not in ("actions", "all"):
                raise ValueError(f"AttnCapture: rows must be \"actions\", \"all\" or an int32 device tensor, got {rows!r}")
        elif not (torch.is_tensor(rows) and rows.dtype == torch.int32 and rows.dim() == 1 and rows.numel() > 0):
            raise ValueError("AttnCapture: a row list must be a non-empty 1-D int32 tensor of flattened rows b*S + s")
        self.rows, self.per_head = rows, bool(per_head)
        self.layers = None if layers is None else [int(i) for i in layers]
        self._slot = None

    def begin(self, n_layers: int, action_rows, B: int, S: int, H: int, device):
        """Resolves rows and layers for one forward and allocates its buffers."""
        if self.layers is None:
            sel = list(range(n_layers))
        else:
            sel = [i + n_layers if i < 0 else i for i in self.layers]
            if any(not 0 <= i < n_layers for i in sel) or len(set(sel)) != len(sel):
                raise ValueError(f"AttnCapture: layers {self.layers} are not distinct indices into {n_layers} decoder layers")
        if isinstance(self.rows, str):
            if self.rows == "actions" and action_rows is None:
                raise ValueError("AttnCapture(rows=\"actions\") needs the forward's action_rows (LlamaStack.fwd alone: pass the row tensor)")
            rows = action_rows.reshape(-1).contiguous() if self.rows == "actions" else None
        else:
            rows = self.rows.to(device).contiguous()
        R = B * S if rows is None else rows.numel()
        self._slot = {li: n for n, li in enumerate(sel)}
        self._rows, self._sel = rows, sel
        self._mean = torch.empty((len(sel), R, S), dtype=F32, device=device)
        self._per_head = torch.empty((len(sel), R, H, S), dtype=F32, device=device) if self.per_head else None

    def layer(self, li: int, q, k, lse, B, S, H, hd, kv_len, causal):
        n = self._slot.get(li)
        if n is not None:
            ops.attn_probs(q, k, lse, B, S, H, hd, rows=self._rows, kv_len=kv_len, causal=causal,
                           out=(None if self._per_head is None else self._per_head[n], self._mean[n]))

    def result(self) -> Dict[str, Any]:
        return dict(mean=self._mean, per_head=self._per_head, rows=self._rows, layers=list(self._sel))


class LlamaStack:
    def __init__(self, store, cfg: VLAConfig, get, lora):
        self.cfg = cfg
        lora = lora if callable(lora) else lora_predicate(lora, None)
        D, F, s = cfg.llm_dim, cfg.llm_ff, cfg.lora_scale
        self.layers = []
        for i in range(cfg.llm_layers):
            p = f"language_model.model.layers.{i}."

            def fused(names, sub):
                W = torch.cat([get(p + sub + n + ".weight") for n in names], 0)
                on = lora([p + sub + n for n in names])
                A = torch.cat([get(p + sub + n + ".lora_A.weight") for n in names], 0) if on else None
                Bm = torch.cat([get(p + sub + n + ".lora_B.weight") for n in names], 0) if on else None
                return LoraLinear(store, p + sub + "+".join(names), W, None, A, Bm, len(names), s, ref_names=[p + sub + n for n in names])

            self.layers.append(dict(
                qkv=fused(["q_proj", "k_proj", "v_proj"], "self_attn."), o=fused(["o_proj"], "self_attn."),
                gu=fused(["gate_proj", "up_proj"], "mlp."), down=fused(["down_proj"], "mlp."),
                n1=get(p + "input_layernorm.weight"), n2=get(p + "post_attention_layernorm.weight")))
        self.norm_w = get("language_model.model.norm.weight")
        self.hd = D // cfg.llm_heads
        self.cos = self.sin = None
        self.on_grads_ready = None

    def linears(self):
        for l in self.layers:
            yield from (l["qkv"], l["o"], l["gu"], l["down"])

    # -- RMSNorm folded around the projections (inference on adapter-free weights) ------------------------------------------------------
    def fold_norms(self):
        """`north_star`'s "fused RMSNorm + RoPE + QKV" on the inference path (HF LlamaDecoderLayer: input_layernorm -> q|k|v, post_attention_layernorm
        -> gate|up; call site modeling_prismatic.py:901-912).  y = (w * x * rstd) W^T = rstd * (x (W w)^T): the norm WEIGHT is folded into a second
        copy of the frozen projection weight (columns scaled, rounded to bf16 once, offline), the per-row sum of squares comes out of the PRODUCING
        GEMM's epilogue (o_proj / down_proj with the residual add: ovla_gemm_args.rowsq_out; the first layer's from ovla_row_sumsq) and rstd scales
        the accumulator in the consuming GEMM's epilogue, before the RoPE rotation (rowscale_part) -- no norm kernel, no normalised activations in
        HBM.  Needs weights without live adapters (merged or adapter-free) and costs a second copy of the q|k|v and gate|up weights (+9 GB at 7B).
        The rounding points move (the reference rounds x * rstd and w * (.) to bf16 before the GEMM): tests/test_fullsize_e2e_gpu.py bounds the delta."""
        for l in self.layers:
            for key, nk in (("qkv", "n1"), ("gu", "n2")):
                lin = l[key]
                if lin.has_lora and not getattr(lin, "merged", False):
                    raise RuntimeError("fold_norms: the decoder still carries live LoRA adapters (merge_lora() first)")
                l[key + "_n"] = ops.colscale(lin.W, l[nk])          # bf16(W[n, k] * w[k])
        self.folded = True
        self._fold_plan = {}

    def _infer_tile(self, M: int) -> int:
        """Tile configuration of the folded inference path's four projections.  A few hundred rows (the batch-1 chunk: M = 608 = 4.75 row tiles of 128): the
        4-wave 128x256 configuration with the hand-scheduled K loop (ovla.h tile 122: -9...-16 % per projection on cold weights, tools/cold_gemm_probe.py);
        otherwise 0 = the planner's choice.  OVLA_INFER_W4=0 switches it off."""
        D, F = self.cfg.llm_dim, self.cfg.llm_ff
        return 122 if _INFER_W4 and 256 < M <= 1024 and D % 256 == 0 and F % 128 == 0 and D <= 4096 and self.hd == 128 else 0

    def _fold_ok(self, M: int) -> bool:
        """The fold runs in the 128x128 and the 4-wave 128x256 GEMM configurations only (ovla.h): usable when all four projections of an M-row forward
        resolve to the former or take the latter."""
        ok = self._fold_plan.get(M)
        if ok is None:
            D, F = self.cfg.llm_dim, self.cfg.llm_ff
            ok = D % 512 == 0 and self.hd == 128 and (self._infer_tile(M) == 122 or all(ops.gemm_plan(M, n, k)[0] == 1 for n, k in ((3 * D, D), (D, D), (2 * F, D), (D, F))))
            self._fold_plan[M] = ok
        return ok

    def _fold_fixed_ok(self) -> bool:
        """Batch-invariant mode: the fold is usable when the fixed schedule of each folded projection's class exists -- a property of the
        shapes, never of M (so M = B * S beyond 1024 keeps the fold)."""
        ok = getattr(self, "_fold_fixed", None)
        if ok is None:
            D, F = self.cfg.llm_dim, self.cfg.llm_ff
            ok = D % 512 == 0 and self.hd == 128
            try:
                for n, k, epi in ((3 * D, D, ops.EPI_ROPE | ops.EPI_ROWSCALE), (D, D, ops.EPI_ROWSQ), (D, F, ops.EPI_ROWSQ)):
                    ok = ok and ops.gemm_fixed_schedule(n, k, epi=epi)[0] > 0
                self._swiglu_fixed = ok and ops.gemm_fixed_schedule(2 * F, D, epi=ops.EPI_ROWSCALE | ops.EPI_SWIGLU)[0] > 0
            except _lib.OvlaError:
                ok, self._swiglu_fixed = False, False
            self._fold_fixed = ok
        return ok

    def _tables(self, S, device):
        if self.cos is None or self.cos.shape[0] < S:
            n = max(S, self.cfg.max_positions)
            self.cos, self.sin = ops.rope_table(n, self.hd, self.cfg.rope_theta, device)
        return self.cos, self.sin

    def fwd(self, x, B: int, S: int, kv_len, train: bool, sel=None, attn_capture=None):
        """x bf16 [B*S, D] (inputs_embeds) -> (hidden_states[-1] [B*S, D] (post final norm), saved).
        `sel` (int32 [n], flattened (b, s) rows, n % 8 == 0): only these rows of hidden_states[-1] are wanted (the rows that predict
        the action tokens: everything else of the last layer's output is discarded by run_forward_pass / predict_action).  The last
        layer then runs its attention-output projection, MLP and the final norm on those n rows only (K / V still come from every
        row) and the result is [n, D] in `sel` order -- the same numbers, 9 % of the rows for three of its four GEMMs.
        `attn_capture` (an AttnCapture the caller has begun): one read-only ops.attn_probs launch behind each selected layer's attention;
        None issues exactly the launches and allocations of a forward without the argument."""
        cfg = self.cfg
        D, H, hd, F = cfg.llm_dim, cfg.llm_heads, self.hd, cfg.llm_ff
        cos, sin = self._tables(S, x.device)
        causal = cfg.mask_mode == "causal"
        saved = []
        if sel is not None and (sel.numel() % 8 != 0 or sel.numel() == 0):
            raise ValueError("LlamaStack.fwd: the number of selected rows must be a positive multiple of 8")
        M = x.shape[0]
        invariant = ops.batch_invariant_enabled()
        # (live adapter slots: the unfolded path, as for any adapter-carrying decoder -- the folded launches bypass LoraLinear.fwd)
        rt = getattr(self, "slot_route", None)   # set by VLAEngine.set_adapter_slots when a decoder linear carries slots
        slotted = rt is not None and rt.obs_slot is not None
        fold = (not train) and getattr(self, "folded", False) and _FOLD_RMSNORM and not slotted and (self._fold_fixed_ok() if invariant else self._fold_ok(M))
        part = rbuf = None
        itile = 0
        if fold:   # sums of squares of the first layer's input rows; every later layer's come out of the down projection's epilogue
            part = ops.row_sumsq(x)
            rbuf = torch.empty(M, dtype=F32, device=x.device)
            itile = self._infer_tile(M)
            if invariant:   # (ops.gemm ignores the tile in this mode; 122 only keeps the one-launch SwiGLU branch, chosen by shape alone)
                itile = 122 if self._swiglu_fixed else 0
        for li, l in enumerate(self.layers):
            last_sel = sel is not None and li == len(self.layers) - 1
            if fold:   # RMSNorm + RoPE + q|k|v in ONE launch: rstd from `part`, folded weight, rotation in the epilogue
                qkv = ops.gemm(x, l["qkv_n"], rope=(cos, sin, S, 2 * D), rowscale=(part, cfg.rms_eps, rbuf), tile=itile)
                s_qkv = r1 = None
            else:
                h1, _, r1 = ops.norm_fwd(x, l["n1"], eps=cfg.rms_eps, rms=True, save_stats=train)
                if _FUSE_ROPE_FWD and hd == 128:    # RoPE on the q | k heads in the projection's epilogue (ovla_gemm_args.rope_*)
                    qkv, s_qkv = l["qkv"].fwd(h1, rope=(cos, sin, S, 2 * D))
                else:
                    qkv, s_qkv = l["qkv"].fwd(h1)
                    ops.rope_(qkv, S, 2 * H, hd, cos, sin)
            o, lse = ops.attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], B, S, H, hd, kv_len=kv_len, causal=causal)
            if attn_capture is not None:
                attn_capture.layer(li, qkv[:, :D], qkv[:, D:2 * D], lse, B, S, H, hd, kv_len, causal)
            if fold and not last_sel:
                part2 = torch.empty((M, D // 64), dtype=F32, device=x.device)
                x2 = ops.gemm(o, l["o"].W, residual=x, rowsq_out=part2, tile=itile)
                if itile == 122:   # RMSNorm + gate|up + SwiGLU in ONE launch (ovla.h: OVLA_ACT_SWIGLU on the 128x256 configuration): the [M, 2F] intermediate never exists
                    hm = ops.gemm(x2, l["gu_n"], rowscale=(part2, cfg.rms_eps, rbuf), tile=22, act=ops.ACT_SWIGLU)
                else:
                    gu = ops.gemm(x2, l["gu_n"], rowscale=(part2, cfg.rms_eps, rbuf), tile=itile)
                    hm = ops.swiglu_fwd(gu)
                part = torch.empty((M, D // 64), dtype=F32, device=x.device)
                x = ops.gemm(hm, l["down"].W, residual=x2, rowsq_out=part, tile=itile)
                continue
            if last_sel:
                x2, s_o = l["o"].fwd(ops.gather_rows(o, sel, D), residual=ops.gather_rows(x, sel, D))
            else:
                x2, s_o = l["o"].fwd(o, residual=x)
            h2, _, r2 = ops.norm_fwd(x2, l["n2"], eps=cfg.rms_eps, rms=True, save_stats=train)
            gu, s_gu = l["gu"].fwd(h2)
            hm = ops.swiglu_fwd(gu)
            x3, s_d = l["down"].fwd(hm, residual=x2)
            if train:
                saved.append((x, r1, s_qkv, qkv, o, lse, s_o, x2, r2, s_gu, gu, s_d))
            x = x3
        out, _, rf = ops.norm_fwd(x, self.norm_w, eps=cfg.rms_eps, rms=True, save_stats=train)
        return out, (saved, x, rf, B, S, kv_len, sel)

    def bwd(self, dout, saved_all):
        """dout [B*S, D] gradient of hidden_states[-1] ([n, D] for the selected rows if the forward ran with `sel`) -> gradient of
        inputs_embeds (in a fresh buffer)."""
        cfg = self.cfg
        saved, x_last, rf, B, S, kv_len, sel = saved_all
        D, H, hd, F = cfg.llm_dim, cfg.llm_heads, self.hd, cfg.llm_ff
        causal = cfg.mask_mode == "causal"
        dx = ops.norm_bwd(x_last, dout, self.norm_w, None, rf, rms=True)
        for li, (l, sv) in enumerate(zip(reversed(self.layers), reversed(saved))):
            x, r1, s_qkv, qkv, o, lse, s_o, x2, r2, s_gu, gu, s_d = sv
            if _FUSE_SWIGLU:
                dgu = l["down"].bwd(dx, s_d, dact=("swiglu", gu))        # SwiGLU' in the dgrad GEMM's epilogue: dh never hits HBM
            else:
                dgu = ops.swiglu_bwd(gu, l["down"].bwd(dx, s_d))
            dh2 = l["gu"].bwd(dgu, s_gu)
            ops.norm_bwd(x2, dh2, l["n2"], None, r2, rms=True, dx=dx, dx_accum=True)                   # dx = d x2
            do = l["o"].bwd(dx, s_o)
            if sel is not None and li == 0:   # last layer on the selected rows: back to all rows (zero gradient everywhere else)
                do_full = torch.zeros((B * S, D), dtype=BF16, device=dx.device)
                dx_full = torch.zeros((B * S, D), dtype=BF16, device=dx.device)
                ops.gather_rows(do, sel, D, dst=do_full, scatter_add=True)
                ops.gather_rows(dx, sel, D, dst=dx_full, scatter_add=True)                             # the residual x -> x2 at those rows
                do, dx = do_full, dx_full
            dqkv = torch.empty_like(qkv)
            # dq / dk leave the attention backward already rotated back (inverse RoPE in its epilogues: no separate pass)
            ops.attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, do, lse, B, S, H, hd, kv_len=kv_len, causal=causal,
                         dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:], rope=(self.cos, self.sin))
            dh1 = l["qkv"].bwd(dqkv, s_qkv)
            ops.norm_bwd(x, dh1, l["n1"], None, r1, rms=True, dx=dx, dx_accum=True)                    # dx = d x
            if self.on_grads_ready is not None:   # this layer's LoRA gradients are final: the reducer may ship them
                self.on_grads_ready(l["qkv"].A)
        return dx


# ======================================================================================================================
# MLPResNet action head (prismatic/models/action_heads.py:38-107; L1 loss finetune.py:400, MSE :407)
# ======================================================================================================================
class ActionHead:
    def __init__(self, store, get, prefix: str, cfg: VLAConfig):
        D, A = cfg.llm_dim, cfg.action_dim
        self.cfg, self.prefix = cfg, prefix
        self.ln1_w = store.add(prefix + "layer_norm1.weight", get(prefix + "layer_norm1.weight"))
        self.ln1_b = store.add(prefix + "layer_norm1.bias", get(prefix + "layer_norm1.bias"))
        self.fc1 = FullLinear(store, prefix + "fc1", get(prefix + "fc1.weight"), get(prefix + "fc1.bias"))
        self.blocks = []
        for b in range(2):
            q = f"{prefix}mlp_resnet_blocks.{b}.ffn."
            self.blocks.append(dict(ln_w=store.add(q + "0.weight", get(q + "0.weight")), ln_b=store.add(q + "0.bias", get(q + "0.bias")),
                                    fc=FullLinear(store, q + "1", get(q + "1.weight"), get(q + "1.bias"))))
        self.ln2_w = store.add(prefix + "layer_norm2.weight", get(prefix + "layer_norm2.weight"))
        self.ln2_b = store.add(prefix + "layer_norm2.bias", get(prefix + "layer_norm2.bias"))
        self.out_w = store.add(prefix + "fc2.weight", get(prefix + "fc2.weight"))
        self.out_b = store.add(prefix + "fc2.bias", get(prefix + "fc2.bias"))

    def linears(self):
        yield self.fc1
        for b in self.blocks:
            yield b["fc"]

    def plain_params(self):
        yield from (self.ln1_w, self.ln1_b, self.ln2_w, self.ln2_b, self.out_w, self.out_b)
        for b in self.blocks:
            yield from (b["ln_w"], b["ln_b"])

    def fwd(self, actions_hidden, target=None, mse=False, train=False, return_hidden=False):
        """actions_hidden bf16 [B*A_tokens, D] (row-major (b, token)) == reshape(B, chunk, action_dim*D).
        Returns (pred [B*chunk, action_dim], loss_sum fp32[1] or None, saved); with `return_hidden` also the post-layer_norm2 activations
        bf16 [B*chunk, D] the output layer reads (what ActionScaleHead takes; in training mode a view of what `saved` holds anyway)."""
        cfg = self.cfg
        rows = actions_hidden.shape[0] // cfg.action_dim
        x0 = actions_hidden.view(rows, cfg.action_dim * cfg.llm_dim)
        rows_real = rows
        if rows % 8:   # e.g. ALOHA: batch 4 x chunk 25; the GEMM-shaped data gradients want M % 8 == 0: zero-pad the rows
            rows = (rows + 7) // 8 * 8
            xp = torch.zeros((rows, x0.shape[1]), dtype=BF16, device=x0.device)
            xp[:rows_real] = x0
            x0 = xp
        h0, m0, r0 = ops.norm_fwd(x0, self.ln1_w.data, self.ln1_b.data, eps=1e-5, rms=False, save_stats=train)
        z1 = torch.empty((rows, cfg.llm_dim), dtype=BF16, device=x0.device) if train else None
        split = 8 if rows <= 256 else 1      # small-M weight stream: split K over the chip
        x, s1 = self.fc1.fwd(h0, act=ops.ACT_RELU, c_pre=z1, split_k=split)
        blocks_saved = []
        for b in self.blocks:
            hb, mb, rb = ops.norm_fwd(x, b["ln_w"].data, b["ln_b"].data, eps=1e-5, rms=False, save_stats=train)
            # x_new = relu(fc(ln(x))) + x : epilogue applies the activation before the residual add
            zb = torch.empty_like(x) if train else None
            xn, sb = b["fc"].fwd(hb, act=ops.ACT_RELU, residual=x, c_pre=zb, split_k=2 if rows <= 256 else 1)
            blocks_saved.append((x, mb, rb, zb, sb))
            x = xn
        h2, m2, r2 = ops.norm_fwd(x, self.ln2_w.data, self.ln2_b.data, eps=1e-5, rms=False, save_stats=train)
        loss_sum = torch.zeros(1, dtype=F32, device=x0.device) if target is not None else None
        pred = ops.head_out_fwd(h2[:rows_real], self.out_w.data, self.out_b.data, target, loss_sum, mse=mse)
        saved = (x0, m0, r0, z1, s1, blocks_saved, x, m2, r2, h2, pred, target, mse, rows_real) if train else None
        if return_hidden:
            return pred, loss_sum, saved, h2[:rows_real]
        return pred, loss_sum, saved

    def check_fused_tail(self):   # bench.py still calls this after its timed steps; it goes when that call does
        pass

    def bwd(self, saved, dloss: float = 1.0, dpred=None):
        """Returns d(actions_hidden) [B*A_tokens, D]; accumulates the head's gradients.  With `dpred` (bf16
        [rows, action_dim]) the upstream gradient is taken as given (loss computed by the caller); otherwise the fused
        L1 / MSE gradient of mean-reduced loss * dloss is used."""
        cfg = self.cfg
        x0, m0, r0, z1, s1, blocks_saved, xl, m2, r2, h2, pred, target, mse, rows_real = saved
        rows = x0.shape[0]
        dh2 = ops.head_out_bwd(h2[:rows_real], self.out_w.data, pred, target, dloss / (rows_real * cfg.action_dim), self.out_w.grad, self.out_b.grad,
                               mse=mse, dpred=dpred)
        if rows != rows_real:
            dp = torch.zeros((rows, h2.shape[1]), dtype=BF16, device=h2.device)
            dp[:rows_real] = dh2
            dh2 = dp
        dx = ops.norm_bwd(xl, dh2, self.ln2_w.data, m2, r2, rms=False, dweight=self.ln2_w.grad, dbias=self.ln2_b.grad)
        for b, (xin, mb, rb, zb, sb) in zip(reversed(self.blocks), reversed(blocks_saved)):
            dz = ops.act_bwd(zb, dx, ops.ACT_RELU)
            dhb = b["fc"].bwd(dz, sb)
            ops.norm_bwd(xin, dhb, b["ln_w"].data, mb, rb, rms=False, dx=dx, dx_accum=True, dweight=b["ln_w"].grad, dbias=b["ln_b"].grad)
        dz1 = ops.act_bwd(z1, dx, ops.ACT_RELU)
        dh0 = self.fc1.bwd(dz1, s1)
        dx0 = ops.norm_bwd(x0, dh0, self.ln1_w.data, m0, r0, rms=False, dweight=self.ln1_w.grad, dbias=self.ln1_b.grad)
        return dx0[:rows_real].reshape(rows_real * cfg.action_dim, cfg.llm_dim)


class ActionScaleHead:
    """The learned Laplace scale of the L1 head (ovla.h "Laplace policy with a learned scale"): one linear map on the head's post-layer_norm2
    activations h2 [rows, llm_dim] -> the log-scale s bf16 [rows, action_dim], beside the head's own output layer.  Its gradient STOPS at h2:
    the backward forms dW and db and discards dx, so the mean's path keeps the bits it has without a scale head."""

    def __init__(self, store, get, prefix: str, cfg: VLAConfig):
        self.cfg, self.prefix = cfg, prefix
        self.w = store.add(prefix + "log_scale.weight", get(prefix + "log_scale.weight"))
        self.b = store.add(prefix + "log_scale.bias", get(prefix + "log_scale.bias"))

    def linears(self):
        return ()

    def plain_params(self):
        yield from (self.w, self.b)

    def fwd(self, h2):
        return ops.head_out_fwd(h2, self.w.data, self.b.data)

    def bwd(self, h2, dlog_scale):
        ops.head_out_bwd(h2, self.w.data, None, None, 0.0, self.w.grad, self.b.grad, dpred=dlog_scale)   # (dx is dropped: the gradient stops at h2)

    @staticmethod
    def init_tensors(cfg: VLAConfig, init_scale, device, prefix: str = "action_scale_head.") -> Dict[str, torch.Tensor]:
        """weight 0, bias log(b0) (b0 a scalar or one value per action dimension): exactly the fixed-scale policy of scale b0, up to the bias's
        bf16 rounding."""
        b0, _ = ops.laplace_scales(init_scale, cfg.action_dim)
        if not bool(np.all((b0 > 0) & np.isfinite(b0))):
            raise ValueError(f"init_scale = {init_scale}: positive and finite")
        return {prefix + "log_scale.weight": torch.zeros((cfg.action_dim, cfg.llm_dim), dtype=BF16, device=device),
                prefix + "log_scale.bias": torch.from_numpy(np.log(b0.astype(np.float64)).astype(np.float32)).to(device, BF16)}


class ActionValueHead:
    """The critic of PPO on the L1 head (ovla.h "Value head and generalised advantage estimation"): one linear map on the head's
    post-layer_norm2 activations h2 [rows, llm_dim] -> u bf16 [rows, 1], one number per chunk step, which ovla_value_loss pools into one value
    per observation.  Like the scale head's, its gradient STOPS at h2: the backward forms dW and db and discards dx, so every accumulator of
    the policy keeps the bits it has without a critic (a design choice; a critic that shapes the trunk is not built)."""

    def __init__(self, store, get, prefix: str, cfg: VLAConfig):
        self.cfg, self.prefix = cfg, prefix
        self.w = store.add(prefix + "value.weight", get(prefix + "value.weight"))
        self.b = store.add(prefix + "value.bias", get(prefix + "value.bias"))

    def linears(self):
        return ()

    def plain_params(self):
        yield from (self.w, self.b)

    def fwd(self, h2):
        return ops.head_out_fwd(h2, self.w.data, self.b.data)

    def bwd(self, h2, du):
        ops.head_out_bwd(h2, self.w.data, None, None, 0.0, self.w.grad, self.b.grad, dpred=du)   # (dx is dropped: the gradient stops at h2)

    @staticmethod
    def init_tensors(cfg: VLAConfig, device, prefix: str = "action_value_head.") -> Dict[str, torch.Tensor]:
        """weight 0 and bias 0: a fresh critic values every observation at exactly +0."""
        return {prefix + "value.weight": torch.zeros((1, cfg.llm_dim), dtype=BF16, device=device),
                prefix + "value.bias": torch.zeros(1, dtype=BF16, device=device)}


class MlpProjector:
    """fc1 -> GELU -> fc2 with fully trainable fp32 parameters (ProprioProjector / NoisyActionProjector,
    prismatic/models/projectors.py:6-49)."""

    def __init__(self, store, get, prefix: str):
        self.prefix = prefix
        self.fc1 = FullLinear(store, prefix + "fc1", get(prefix + "fc1.weight").float(), get(prefix + "fc1.bias").float(), master_fp32=True)
        self.fc2 = FullLinear(store, prefix + "fc2", get(prefix + "fc2.weight").float(), get(prefix + "fc2.bias").float(), master_fp32=True)

    def linears(self):
        return (self.fc1, self.fc2)

    def fwd(self, x, train: bool):
        """x bf16 [rows, in] (rows padded to a multiple of 8 by the caller)."""
        if x.shape[1] != self.fc1.in_pad:
            xp = torch.zeros((x.shape[0], self.fc1.in_pad), dtype=BF16, device=x.device)
            xp[:, : x.shape[1]] = x
            x = xp
        z = torch.empty((x.shape[0], self.fc1.out_f), dtype=BF16, device=x.device) if train else None
        h, s1 = self.fc1.fwd(x, act=ops.ACT_GELU, c_pre=z)
        y, s2 = self.fc2.fwd(h)
        return y, (s1, z, s2)

    def bwd(self, dy, saved):
        s1, z, s2 = saved
        dh = self.fc2.bwd(dy, s2)
        dz = ops.act_bwd(z, dh, ops.ACT_GELU)
        self.fc1.bwd(dz, s1, need_dx=False)


def build_component(cls, device, get, prefix, **kw):
    """Builds a stand-alone component (its own ParamStore) from reference-named tensors."""
    st = ParamStore(device)
    comp = cls(st, get=get, prefix=prefix, **kw)
    st.finalize()
    comp.store = st
    for lin in comp.linears():
        lin.refresh_derived()
    return comp


# ======================================================================================================================
# the whole path
# ======================================================================================================================
class ForwardSaved(NamedTuple):
    """What a training forward keeps for backward_from_hidden (`saved` of forward()'s result; None without `train`)."""
    vsaved: Any
    psaved: Any
    nsaved: Any
    lsaved: Any
    B: int
    S: int
    P: int
    n_vis: int
    proprio_projector: Any
    noisy_action_projector: Any
    action_rows: torch.Tensor


class VLAEngine:
    """Prismatic VLM stack + heads.  `get(name)` returns the bf16 device tensor of a reference-named parameter
    (see weights.py for the state-dict naming)."""

    def __init__(self, cfg: VLAConfig, get, device, *, lora: bool = True, use_proprio: bool = True, head: str = "l1", use_film: bool = False,
                 has=None, lora_dropout: float = 0.0, dropout_seed: int = 0, num_diffusion_steps: Optional[int] = None, diffusion_seed: int = 0,
                 sample_seed: int = 0):
        if head not in ("l1", "diffusion", "none"):
            raise ValueError(head)
        self.dropout = DropoutState(lora_dropout, dropout_seed)
        self.token_sample = TokenSampleState(sample_seed)   # stochastic action-token decoding (sample_action_tokens, a sampled predict_action)
        # device noise of the diffusion objective (draw_diffusion / sample_actions): only an engine told the head's T carries the state
        if num_diffusion_steps is not None and head != "diffusion":
            raise ValueError("num_diffusion_steps belongs to the diffusion head")
        self.diffusion = DiffusionNoiseState(num_diffusion_steps, diffusion_seed) if num_diffusion_steps is not None else None
        ops.check_device(device.index or 0)
        self.cfg, self.device, self.lora = cfg, device, lora
        self.route, self.n_slots = SlotRoute(), 0   # multi-policy serving (set_adapter_slots / routing)
        self.pool: Optional[Dict[str, dict]] = None   # the policy pool (init_policy_pool): name -> its tensors in device memory
        lora = lora_predicate(lora, has)
        st = self.store = ParamStore(device)
        # registration order = forward order (the store reverses it into backward order)
        if use_film not in (False, True, "per_policy"):
            raise ValueError(f'use_film = {use_film!r} (False, True or "per_policy")')
        # "per_policy": the towers carry FiLM SLOT storage (FilmSlots, allocated with the adapter slots) and no FiLM Linears of their own;
        # every observation is modulated by its own policy's scale / shift Linears.  Inference only.
        self.film_per_policy = use_film == "per_policy"
        self.film_slots: Optional[FilmSlots] = None
        self.use_film = bool(use_film)
        tower_film = "per_policy" if self.film_per_policy else bool(use_film)
        self.dino = VitTower(st, "vision_backbone.featurizer.", cfg.dino, get, cfg, lora, film=tower_film)
        self.siglip = VitTower(st, "vision_backbone.fused_featurizer.", cfg.siglip, get, cfg, lora, film=tower_film)
        s = cfg.lora_scale

        def L(name):
            return LoraLinear(st, name, get(name + ".weight"), get(name + ".bias"), get(name + ".lora_A.weight") if lora([name]) else None,
                              get(name + ".lora_B.weight") if lora([name]) else None, 1, s)

        self.proj = [L("projector.fc1"), L("projector.fc2"), L("projector.fc3")]
        self.embed = get("language_model.model.embed_tokens.weight")
        self.llm = LlamaStack(st, cfg, get, lora)
        self.lm_head = get("language_model.lm_head.weight") if (has is None or has("language_model.lm_head.weight")) else None
        self._lm_head_t = None      # its transpose, made by the first lm_loss_bwd
        st.finalize()
        # components are separate modules with their own parameter stores, like the reference's DDP-wrapped
        # ProprioProjector / action head / NoisyActionProjector (finetune.py:894-932); they can also be built standalone
        # (modeling.py) and passed in per call.
        self.proprio = self.noisy = self.head = None
        self.head_kind = head
        if use_proprio:
            self.proprio = build_component(MlpProjector, device, get, "proprio_projector.")
        if head == "diffusion":
            self.noisy = build_component(MlpProjector, device, get, "noisy_action_projector.")
        if head != "none":
            self.head = build_component(ActionHead, device, get, "action_head.noise_predictor.mlp_resnet." if head == "diffusion" else "action_head.model.",
                                        cfg=cfg)
        self.refresh_derived()
        ids = self.dropout_module_ids()
        for lin in self.all_linears():
            if isinstance(lin, LoraLinear) and lin.has_lora:
                lin.module_ids = [ids[rn] for rn in lin.ref_names]
                lin.dropout = self.dropout if self.dropout.p > 0.0 else None
        if _FOLD_RMSNORM and not any(l.has_lora for l in self.llm.linears()):
            self.llm.fold_norms()       # an adapter-free decoder (merged checkpoint): inference-only model, fold the RMSNorms (LlamaStack.fold_norms)

    @property
    def stores(self):
        return [self.store] + [m.store for m in (self.proprio, self.noisy, self.head, self.scale_head, self.value_head) if m is not None]

    # -- the learned Laplace scale of the L1 head (ActionScaleHead): opt-in, a store of its own -----------------------------------------------------
    scale_head: Optional["ActionScaleHead"] = None
    scale_bounds: Tuple[float, float] = ops.LAPLACE_SCALE_BOUNDS

    def attach_scale_head(self, init_scale=0.1, bounds=ops.LAPLACE_SCALE_BOUNDS, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        """Attaches the scale head: weight 0 and bias log(init_scale) (or `state_dict`'s `action_scale_head.log_scale.{weight, bias}`), its
        log-scale clamped to `bounds` by the kernels (the default, b in about [0.0025, 2.7] normalised units, is a design choice).  Its store joins
        `stores`: zero_grad, adamw_step, export_trainable / load_trainable, the optimizer-state dict see it like the head's.  The clip slots, the
        tensor-statistics tables, the EMA shadows, fp32 optimizer state, the reference snapshot and a reducer enumerate `stores` when they are
        enabled, so this comes BEFORE any of them (RuntimeError otherwise).  Needs head='l1'."""
        self._l1_head("attach_scale_head")
        self._not_in_ema_scope("attach_scale_head")
        if self.scale_head is not None:
            raise RuntimeError("attach_scale_head: a scale head is attached already")
        self._attach_before_enumerators("attach_scale_head", "scale head")
        lo, hi = float(bounds[0]), float(bounds[1])
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"bounds = {bounds}: two finite log-scales, lo <= hi")
        prefix = "action_scale_head."
        sd = ActionScaleHead.init_tensors(self.cfg, init_scale, self.device, prefix)
        if state_dict is not None:
            for k, v in sd.items():
                src = state_dict[k] if k in state_dict else state_dict[k[len(prefix):]]
                if tuple(src.shape) != tuple(v.shape):
                    raise ValueError(f"{k}: shape {tuple(src.shape)} != {tuple(v.shape)}")
                sd[k] = src.to(self.device, BF16)
        self.scale_head = build_component(ActionScaleHead, self.device, sd.__getitem__, prefix, cfg=self.cfg)
        self.scale_bounds = (lo, hi)
        return self.scale_head

    def _attach_before_enumerators(self, who: str, what_head: str):
        """A head with a store of its own joins `stores` before anything that enumerates them when it is enabled (RuntimeError otherwise)."""
        late = [what for what, on in (("enable_grad_clip", self._grad_clip is not None), ("enable_tensor_stats", self._tensor_stats is not None),
                                      ("enable_ema", self.ema_enabled), ("enable_fp32_optimizer_state", self.store.fp32_state),
                                      ("set_reference_policy", self._reference is not None), ("attach_reducer", getattr(self, "reducer", None) is not None)) if on]
        if late:
            raise RuntimeError(f"{who} after {', '.join(late)}: they enumerate the stores when they are enabled; attach the {what_head} first")

    # -- the critic of PPO on the L1 head (ActionValueHead): opt-in, a store of its own, beside the scale head in either order ----------------------
    value_head: Optional["ActionValueHead"] = None

    def attach_value_head(self, state_dict: Optional[Dict[str, torch.Tensor]] = None):
        """Attaches the value head: weight 0 and bias 0 (or `state_dict`'s `action_value_head.value.{weight, bias}`).  Its store joins `stores`
        as the scale head's does, with the same ordering rule: BEFORE the clip slots, the tensor-statistics tables, the EMA shadows, fp32 optimizer
        state, the reference snapshot and a reducer (RuntimeError otherwise).  Needs head='l1'."""
        self._l1_head("attach_value_head")
        self._not_in_ema_scope("attach_value_head")
        if self.value_head is not None:
            raise RuntimeError("attach_value_head: a value head is attached already")
        self._attach_before_enumerators("attach_value_head", "value head")
        prefix = "action_value_head."
        sd = ActionValueHead.init_tensors(self.cfg, self.device, prefix)
        if state_dict is not None:
            for k, v in sd.items():
                src = state_dict[k] if k in state_dict else state_dict[k[len(prefix):]]
                if tuple(src.shape) != tuple(v.shape):
                    raise ValueError(f"{k}: shape {tuple(src.shape)} != {tuple(v.shape)}")
                sd[k] = src.to(self.device, BF16)
        self.value_head = build_component(ActionValueHead, self.device, sd.__getitem__, prefix, cfg=self.cfg)
        return self.value_head

    def _critic(self, who: str) -> "ActionValueHead":
        if self.value_head is None:
            raise ValueError(f"{who} needs attach_value_head()")
        return self.value_head

    def _learned(self, scale, who: str) -> bool:
        """True for scale == "learned" (ValueError without a scale head); a numeric scale takes the fixed-scale code whether or not one is attached."""
        if not isinstance(scale, str):
            return False
        if scale != "learned":
            raise ValueError(f'{who}: scale = {scale!r} (a number, one per action dimension, or "learned")')
        if self.scale_head is None:
            raise ValueError(f'{who}: scale="learned" needs attach_scale_head()')
        return True

    def zero_grad(self):
        for st in self.stores:
            st.zero_grad()
        if getattr(self, "reducer", None) is not None:
            self.reducer.reset()

    def adamw_step(self, lr: float, **kw):
        self._not_in_ema_scope("adamw_step")
        clip = self._grad_clip
        if clip is None:
            for st in self.stores:
                st.adamw_step(lr, **kw)
            return
        # the global norm of the gradients as AdamW will see them (after the reducer, times grad_scale, in the parameter's precision): one
        # sum-of-squares per flat buffer, one coefficient launch, then the clipped AdamW launches.  Nothing is read back.
        grad_scale = kw.get("grad_scale", 1.0)
        slot = 0
        for st in self.stores:
            for dt, grad in st.flat_grad.items():
                # (fp32 optimizer state: ovla_adamw_master does not round the gradient to bf16, and the norm is of the gradient it sees)
                ops.grad_sumsq(grad, clip["slots"], slot, clip["workspace"], is_bf16=dt == BF16 and not st.fp32_state, grad_scale=grad_scale)
                slot += 1
        ops.grad_clip_coef(clip["slots"], clip["state"], clip["max_norm"], clip["skip_nonfinite"])
        for st in self.stores:
            st.adamw_step(lr, clip_state=clip["state"], **kw)

    # -- gradient-norm clipping and the non-finite step guard (ovla.h "Gradient-norm clipping") ---------------------------------------------------
    _grad_clip: Optional[dict] = None

    @property
    def grad_clip_enabled(self) -> bool:
        return self._grad_clip is not None

    def enable_grad_clip(self, max_norm: float = math.inf, skip_nonfinite: bool = True):
        """From now on adamw_step clips the global gradient norm (every store, both dtypes) to `max_norm` as torch's clip_grad_norm_ does, and,
        with `skip_nonfinite`, leaves parameters and moments untouched on a step whose norm is NaN or Inf.  max_norm = inf: guard only.
        Allocates one double slot per (store, dtype) flat buffer -- in `stores` order, bf16 before fp32 --, the device state and the partials
        workspace.  A skipped step still advances ParamStore.step: it consumes its step number in the bias correction and the LR schedule, and
        an EMA update after it averages the unchanged parameters.  The zero padding of the flat buffers contributes nothing to the norm.
        Data parallel: the norm is taken where adamw_step reads the gradients, after the reducer; every rank holds the same reduced bits and
        computes the same coefficient, nothing is communicated."""
        max_norm = float(max_norm)
        if not max_norm > 0.0:
            raise ValueError(f"max_norm = {max_norm} (a positive number, or inf for the non-finite guard alone)")
        bufs = [g for st in self.stores for g in st.flat_grad.values()]
        self._grad_clip = dict(max_norm=max_norm, skip_nonfinite=bool(skip_nonfinite),
                               slots=torch.zeros(len(bufs), dtype=torch.float64, device=self.device), state=ops.grad_clip_state(self.device),
                               workspace=torch.zeros(max(1, max(ops.grad_sumsq_workspace_elems(g.numel()) for g in bufs)), dtype=torch.float64,
                                                     device=self.device))

    def grad_clip_stats(self) -> Dict[str, float]:
        """The state of the last adamw_step and the counters, {norm, coef, skipped, clipped, steps}.  The feature's ONLY readback: it waits for
        the device, so call it where the host synchronises anyway (the driver does at its logging steps)."""
        if self._grad_clip is None:
            raise RuntimeError("grad_clip_stats without enable_grad_clip()")
        s = ops.read_grad_clip_state(self._grad_clip["state"])
        return {"norm": s["norm"], "coef": s["coef"], "skipped": s["skipped"], "clipped": s["clipped"], "steps": s["steps"]}

    def load_grad_clip_state_dict(self, sd: Dict[str, torch.Tensor]) -> bool:
        """Restores the three counters from the `grad_clip.` entries of an optimizer state dict into an engine with the feature enabled.
        False, and nothing changes, when `sd` has none (written by a run without it: the counters stay where they are, 0 in a fresh engine)."""
        if self._grad_clip is None or "grad_clip.steps" not in sd:
            return False
        counters = [int(sd[f"grad_clip.{k}"].item()) for k in ("steps", "clipped", "skipped")]
        self._grad_clip["state"][3:6].copy_(torch.tensor(counters, dtype=torch.int32))
        return True

    # -- per-tensor statistics (ovla.h "Per-tensor statistics"): opt-in, read-only -------------------------------------------------------------------
    _tensor_stats: Optional[dict] = None

    @property
    def tensor_stats_enabled(self) -> bool:
        return self._tensor_stats is not None

    def enable_tensor_stats(self):
        """Allocates what collect_tensor_stats needs: per (store, dtype) flat buffer -- in `stores` order, bf16 before fp32 -- the segment table
        of its tensors (Param.offset, Param.numel, ascending offset) and its plan, copied to the device once; one zeroed `out` record per
        tensor (the n_bad_steps latches start at 0 and are not checkpointed) and one partials workspace shared by the buffers.  Idempotent.
        Refused inside ema_weights(): the flat buffers hold the averaged weights."""
        self._not_in_ema_scope("enable_tensor_stats")
        if self._tensor_stats is not None:
            return
        tables, names = [], []
        for st in self.stores:
            for dt, flat in st.flat.items():
                params = sorted((p for p in st.params if p.dtype == dt), key=lambda p: p.offset)
                plan = ops.tensor_stats_plan([(p.offset, p.numel) for p in params], flat.numel(), device=self.device)
                tables.append(dict(store=st, dtype=dt, plan=plan, first=len(names)))
                names += [p.name for p in params]
        assert len(set(names)) == len(names), "two trainable tensors share a name"
        out, partials = ops.tensor_stats_buffers(len(names), max(t["plan"]["total_chunks"] for t in tables), self.device)
        self._tensor_stats = dict(tables=tables, names=names, out=out, partials=partials)

    def collect_tensor_stats(self, grad_scale: float = 1.0):
        """One launch pair per flat buffer: the statistics of every trainable tensor's gradient as adamw_step(grad_scale=...) will see it (the
        same `is_bf16 and not fp32_state` rounding rule as its norm) and of its parameter (in fp32-state mode the fp32 master), into the device
        records.  Call it after the reducer and before adamw_step.  Writes nothing but its own records; nothing is read back."""
        self._not_in_ema_scope("collect_tensor_stats")
        ts = self._tensor_stats
        if ts is None:
            raise RuntimeError("collect_tensor_stats without enable_tensor_stats()")
        for t in ts["tables"]:
            st, dt, n = t["store"], t["dtype"], t["plan"]["n_segs"]
            ops.tensor_stats(t["plan"], st.flat_grad[dt], st.master.get(dt, st.flat[dt]), ts["out"][t["first"]: t["first"] + n], ts["partials"],
                             grad_round_bf16=dt == BF16 and not st.fp32_state, grad_scale=grad_scale)

    def tensor_stats(self) -> Dict[str, Dict[str, float]]:
        """The records of the last collect_tensor_stats, {name: {grad_norm, param_norm, grad_absmax, n_nonfinite, n_bad_steps}} in table order,
        keyed by the stores' ParamStore.named() names; the norms are the square roots of the double sums (NaN or inf as computed).  The
        feature's ONLY readback: it waits for the device, so call it where the host synchronises anyway."""
        if self._tensor_stats is None:
            raise RuntimeError("tensor_stats without enable_tensor_stats()")
        rec = ops.read_tensor_stats(self._tensor_stats["out"])
        return {name: {"grad_norm": math.sqrt(r["grad_sumsq"]), "param_norm": math.sqrt(r["param_sumsq"]), "grad_absmax": float(r["grad_absmax"]),
                       "n_nonfinite": int(r["n_nonfinite"]), "n_bad_steps": int(r["n_bad_steps"])}
                for name, r in zip(self._tensor_stats["names"], rec)}

    def first_nonfinite(self) -> Optional[str]:
        """The first tensor, in table order, whose last collected gradient held a NaN or Inf; None when there is none (this reads back)."""
        return next((name for name, s in self.tensor_stats().items() if s["n_nonfinite"] > 0), None)

    # -- fp32 optimizer state (ovla.h "AdamW on fp32 master weights") -----------------------------------------------------------------------------
    @property
    def optimizer_state_precision(self) -> str:
        """"param": AdamW state in each buffer's own dtype, as torch.optim.AdamW keeps it (the default); "fp32": enable_fp32_optimizer_state."""
        return "fp32" if self.store.fp32_state else "param"

    def enable_fp32_optimizer_state(self):
        """Every store's bf16 buffer gets an fp32 master copy and fp32 AdamW moments (ParamStore.enable_fp32_state); the fp32 buffers are as
        before.  +8 bytes per bf16 trainable element.  Call it before enable_ema (the shadows then start from, and follow, the master); a later
        load_trainable re-widens the master from the loaded parameters.  Refused inside ema_weights(): the flat buffers hold the averaged weights."""
        self._not_in_ema_scope("enable_fp32_optimizer_state")
        for st in self.stores:
            st.enable_fp32_state()

    def fp32_optimizer_state_bytes(self) -> int:
        """Device bytes fp32 mode adds: 4 for the master and 2 for each widened moment, per element of a bf16 flat buffer."""
        return sum(8 * st.flat[BF16].numel() for st in self.stores if BF16 in st.flat)

    # -- weight EMA: fp32 shadows of every store's flat buffers, updated after the optimizer step, swapped in for evaluation and export -----------
    _ema_scope = False  # true while ema_weights() holds the averaged weights in the flat buffers

    @property
    def ema_enabled(self) -> bool:
        return self.store.ema_shadow is not None

    @property
    def ema_step(self) -> int:
        """The number of EMA updates taken (the same in every store)."""
        return self.store.ema_step

    @property
    def in_ema_scope(self) -> bool:
        return self._ema_scope

    def _not_in_ema_scope(self, who: str):
        if self._ema_scope:
            raise RuntimeError(f"{who} inside ema_weights(): the flat buffers hold the averaged weights, not the ones being trained")
        if self._ref_scope:
            raise RuntimeError(f"{who} inside reference_policy(): the flat buffers hold the reference snapshot, not the weights being trained")

    def enable_ema(self):
        self._not_in_ema_scope("enable_ema")
        for st in self.stores:
            st.enable_ema()

    def ema_update(self, decay: float):
        """One EMA update of every store with this decay (the schedule is the caller's: vla_scripts/finetune.py ema_decay_at).  Stream-ordered
        launches only, nothing is read back."""
        self._not_in_ema_scope("ema_update")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ema decay = {decay} is outside [0, 1]")
        for st in self.stores:
            st.ema_update(decay)

    @contextlib.contextmanager
    def ema_weights(self):
        """Scope in which the flat buffers hold the averaged weights: eval_step, sample_actions, export_trainable("data"),
        vision_backbone_state_dict() and save_training_checkpoint see them with no change of their own.  On exit the live bits come back
        exactly; the derived copies are re-derived on both sides.  Training entry points and ema_update raise inside, and so does nesting."""
        if not self.ema_enabled:
            raise RuntimeError("ema_weights() without enable_ema()")
        self._not_in_ema_scope("ema_weights")
        stash = [st.ema_swap_in() for st in self.stores]
        self._ema_scope = True
        try:
            self.refresh_derived()
            yield self
        finally:
            for st, live in zip(self.stores, stash):
                st.ema_restore(live)
            self._ema_scope = False
            self.refresh_derived()

    def num_trainable(self):
        return sum(st.num_trainable() for st in self.stores)

    # -- bookkeeping -----------------------------------------------------------------------------------------------------
    def all_linears(self):
        yield from self.dino.linears()
        yield from self.siglip.linears()
        yield from self.proj
        for m in (self.proprio, self.noisy, self.head):
            if m is not None:
                yield from m.linears()
        yield from self.llm.linears()

    def dropout_module_ids(self) -> Dict[str, int]:
        """The stable 32-bit `module` id of every adapted reference sub-linear (its word of the mask's Philox counter): the position in
        all_linears() x ref_names, so the fused q|k|v and gate|up linears carry one id -- one independent mask -- per fused group."""
        names = [rn for lin in self.all_linears() if isinstance(lin, LoraLinear) and lin.has_lora for rn in lin.ref_names]
        return {rn: i for i, rn in enumerate(names)}

    def merge_lora(self):
        """Folds every LoRA adapter of the VLM into its base weight (what the reference does before deployment:
        merge_lora_weights_and_save.py).  Afterwards forward() runs plain GEMMs; training entry points raise."""
        for lin in self.vlm_linears():
            if isinstance(lin, LoraLinear):
                lin.merge()
        self.lora_merged = True
        if _FOLD_RMSNORM:
            self.llm.fold_norms()       # adapter-free decoder: RMSNorm + RoPE + q|k|v (and RMSNorm + gate|up) become one launch each at inference

    # -- adapter slots: several fine-tuned policies on one base model (inference only) ---------------------------------------------------------
    def _check_adapters(self, adapters: List[Dict[str, torch.Tensor]], lora_alpha=None):
        """What set_adapter_slots and the policy pool check before they change anything: a base model without adapters of its own, every
        policy with the configuration's lora_alpha and rank, no stray tensors, whole fused groups, one adapted set.
        -> (the model's LoraLinears, the names of the adapted ones; an empty set for no adapters)."""
        if getattr(self, "lora_merged", False) or any(isinstance(l, LoraLinear) and l.has_lora for l in self.vlm_linears()):
            raise ValueError("adapter slots need a base model built without merged or trainable LoRA adapters")
        cfg = self.cfg
        for s, a in enumerate(lora_alpha or []):
            if a is not None and float(a) != float(cfg.lora_alpha):
                raise ValueError(f"policy {s}: lora_alpha {a} differs from the model configuration's {cfg.lora_alpha} (one alpha / r scales every slot)")
        linears = [l for l in self.vlm_linears() if isinstance(l, LoraLinear)]
        known = {rn + suffix for l in linears for rn in l.ref_names for suffix in (".lora_A.weight", ".lora_B.weight")}
        unused = tuple(f"{t.prefix}blocks.{t.vc.depth - 1}." for t in (self.dino, self.siglip))   # each tower's last block is never run (VitTower)
        plans = []
        for s, sd in enumerate(adapters):
            stray = [k for k in sd if k not in known and not k.startswith(unused)]
            if stray:
                raise ValueError(f"policy {s}: {len(stray)} tensors name no adapted linear of this model, e.g. {stray[:2]}")
            adapted = frozenset(l.name for l in linears if any(rn + ".lora_A.weight" in sd for rn in l.ref_names))
            plans.append(adapted)
            for l in linears:
                if l.name in adapted and not all(rn + sfx in sd for rn in l.ref_names for sfx in (".lora_A.weight", ".lora_B.weight")):
                    raise ValueError(f"policy {s}: adapters present for only some of the fused linears {l.ref_names}")
                for rn in l.ref_names:
                    if l.name in adapted and sd[rn + ".lora_A.weight"].shape[0] != cfg.lora_rank:
                        raise ValueError(f"policy {s}: {rn} has rank {sd[rn + '.lora_A.weight'].shape[0]}, the model configuration's is {cfg.lora_rank} "
                                         "(mixed ranks are not supported)")
        if any(p != plans[0] for p in plans):
            raise ValueError("the policies adapt different sets of linears")
        return linears, (plans[0] if plans else frozenset())

    def _film_towers(self):
        return [(t.prefix, len(t.blocks), t.vc.dim) for t in (self.dino, self.siglip)]

    def _alloc_film_slots(self, n: int):
        """FiLM slot storage for n policies on both towers (n = 0 removes it); the towers read their blocks' gamma / beta from it."""
        self.film_slots = FilmSlots(self._film_towers(), n, self.cfg.llm_dim, self.device) if n else None
        self.dino.film_slots = self.siglip.film_slots = self.film_slots

    def _check_film(self, film, n: int, who: str):
        """`film` (one dict per policy, or None) against the engine's mode, before anything changes -> the checked bf16 device tensors per policy."""
        if not self.film_per_policy:
            if film is not None and any(f is not None for f in film):
                raise ValueError(f"{who}: FiLM tensors were given, but the model was not built with use_film=\"per_policy\" "
                                 "(a model without FiLM has no place for them; a model with its own FiLM Linears serves one policy)")
            return None
        if n == 0 and not film:
            return []
        if film is None or len(film) != n or any(f is None for f in film):
            raise ValueError(f"{who}: a model built with use_film=\"per_policy\" needs every policy's FiLM tensors (`film`)")
        return [check_film_tensors(f, self._film_towers(), self.cfg.llm_dim, self.device, f"{who}: policy {s}") for s, f in enumerate(film)]

    def set_adapter_slots(self, adapters: List[Dict[str, torch.Tensor]], *, lora_alpha: Optional[List[Optional[float]]] = None, film=None):
        """adapters[s]: policy s's LoRA tensors under the names lora_state_dict() / weights.load_lora_adapter use (`<linear>.lora_A.weight`,
        `.lora_B.weight`, un-fused per q/k/v and gate/up).  Allocates n = len(adapters) slots on every adapted linear and fills them; an empty
        list removes the slots.  The model must carry no merged or trainable adapters of its own; all policies must adapt the same linears with
        one rank and one lora_alpha -- the model configuration's, whose alpha / r scales every slot's projection.
        `film` (an engine built with use_film="per_policy": required; any other engine: refused): film[s] is policy s's FiLM tensors under
        `vision_backbone.{featurizer,fused_featurizer}.blocks.{i}.{scale,shift}.{weight,bias}` for the towers' used blocks, exactly; they go to
        slot s of the FiLM slot storage (FilmSlots) in bf16."""
        n = len(adapters)
        if n > MAX_SLOTS:
            raise ValueError(f"{n} policies: at most {MAX_SLOTS} adapter slots ride in one launch")
        if self.pool is not None:
            raise ValueError("set_adapter_slots: this engine's slots belong to its policy pool (pool_add / load_slot)")
        linears, adapted = self._check_adapters(adapters, lora_alpha)
        film = self._check_film(film, n, "set_adapter_slots")   # every policy's FiLM tensors (a per-policy-FiLM engine), validated before anything changes
        if self.film_per_policy:
            self._alloc_film_slots(n)
            for s in range(n):
                self.film_slots.set_slot(s, film[s])
        cfg, plans = self.cfg, [adapted]
        for l in linears:
            l.clear_slots()
            if n and l.name in plans[0]:
                l.init_slots(n, cfg.lora_rank, self.route)
                for s, sd in enumerate(adapters):
                    l.set_slot(s, torch.cat([sd[rn + ".lora_A.weight"] for rn in l.ref_names], 0), torch.cat([sd[rn + ".lora_B.weight"] for rn in l.ref_names], 0))
        self.n_slots = n
        self.llm.slot_route = self.route if any(getattr(l, "n_slots", 0) for l in self.llm.linears()) else None

    # -- policy pool: any number of registered policies in device memory, `resident` of them in the slot storage -----------------------------
    def init_policy_pool(self, resident: int, template_adapter: Dict[str, torch.Tensor], *, lora_alpha: Optional[float] = None, film=None):
        """Allocates the slot storage for n = `resident` adapters on every linear that `template_adapter` adapts -- once: the slot count, and with
        it the K-extension width, the fixed schedules and every captured graph, stays what it is for the life of the model.  Empty slots hold
        zeros and no row is ever routed to one (policy_pool.Residency knows which are filled).  Registers nothing."""
        if self.pool is not None:
            raise ValueError("init_policy_pool: the pool exists already")
        if not 1 <= int(resident) <= MAX_SLOTS:
            raise ValueError(f"init_policy_pool: resident = {resident} (1 .. {MAX_SLOTS}: at most {MAX_SLOTS} adapter slots ride in one launch)")
        if self.n_slots:
            raise ValueError("init_policy_pool: this engine already carries adapter slots (set_adapter_slots)")
        linears, adapted = self._check_adapters([template_adapter], [lora_alpha])
        if not adapted:
            raise ValueError("init_policy_pool: the template adapter adapts no linear of this model")
        self._check_film([film], 1, "init_policy_pool")   # (the template's FiLM tensors are validated, nothing of them is stored)
        if self.film_per_policy:
            self._alloc_film_slots(int(resident))
        for l in linears:
            if l.name in adapted:
                l.init_slots(int(resident), self.cfg.lora_rank, self.route)
        self.n_slots = int(resident)
        self.llm.slot_route = self.route if any(getattr(l, "n_slots", 0) for l in self.llm.linears()) else None
        self.pool = {}
        self.pool_state = Residency(int(resident))
        self._pool_linears = [l for l in linears if l.name in adapted]
        self._pool_adapted = adapted
        self._pool_tables: Dict[Tuple[str, int], dict] = {}

    def pool_add(self, name: str, adapter: Dict[str, torch.Tensor], *, lora_alpha: Optional[float] = None, slot_pairs=None, film=None):
        """Registers `name`: validated exactly as set_adapter_slots validates (rank, alpha, the pool's adapted set, stray tensors, and on a
        per-policy-FiLM engine its `film` tensors), then every adapted linear's cat(lora_A) [G r, in] and cat(lora_B) [out, r] -- and the FiLM
        tensors -- are stored in bf16 on the device.  `slot_pairs(s)` -> [(src, dst)]: further
        tensors that belong to the policy and have to reach slot s with the adapters (the head's and the proprio projector's parameters)."""
        if self.pool is None:
            raise ValueError("pool_add: no policy pool (init_policy_pool)")
        if name in self.pool:
            raise ValueError(f"pool_add: a policy named {name!r} is already in the pool")
        _, adapted = self._check_adapters([adapter], [lora_alpha])
        if adapted != self._pool_adapted:
            raise ValueError("the policies adapt different sets of linears")
        film = self._check_film([film], 1, f"pool_add({name!r})")   # per-policy FiLM: checked, bf16, on the device
        dev, r = self.device, self.cfg.lora_rank
        tensors = {}
        for l in self._pool_linears:
            A = torch.cat([adapter[rn + ".lora_A.weight"] for rn in l.ref_names], 0).to(dev, BF16).contiguous()
            Bm = torch.cat([adapter[rn + ".lora_B.weight"] for rn in l.ref_names], 0).to(dev, BF16).contiguous()
            if tuple(A.shape) != (l.groups * r, l.in_f) or tuple(Bm.shape) != (l.out_f, r):
                raise ValueError(f"{l.name}: adapter shapes {tuple(A.shape)} / {tuple(Bm.shape)} do not fit rank {r} "
                                 f"(want {(l.groups * r, l.in_f)} / {(l.out_f, r)})")
            tensors[l.name] = (A, Bm)
        self.pool[name] = dict(tensors=tensors, slot_pairs=slot_pairs, film=None if film is None else film[0])

    def pool_remove(self, name: str):
        """Forgets `name`: its tensors and its cached copy tables are released, the slot it occupied (if any) is empty and stale."""
        if self.pool is None or name not in self.pool:
            raise ValueError(f"pool_remove: unknown policy {name!r}")
        del self.pool[name]
        for key in [k for k in self._pool_tables if k[0] == name]:
            del self._pool_tables[key]
        self.pool_state.invalidate(name)

    def pool_slot_pairs(self, s: int, name: str):
        """Every (source, destination) tensor pair of loading `name` into slot s: per adapted linear the G row groups of lora_A into
        A_slots[slot_a_rows(g, s, n, r)] and lora_B into B_slots[:, s r:(s + 1) r], then the policy's own slot_pairs(s)."""
        p, n, r = self.pool[name], self.n_slots, self.cfg.lora_rank
        pairs = []
        for l in self._pool_linears:
            A, Bm = p["tensors"][l.name]
            pairs += [(A[g * r:(g + 1) * r], l.A_slots[slot_a_rows(g, s, n, r)]) for g in range(l.groups)]
            pairs.append((Bm, l.B_slots[:, s * r:(s + 1) * r]))
        if p["film"] is not None:   # the policy's scale / shift Linears into slot s of every FiLM Linear: the same launch
            pairs += self.film_slots.slot_pairs(s, p["film"])
        if p["slot_pairs"] is not None:
            pairs += list(p["slot_pairs"](s))
        return pairs

    def load_slot(self, s: int, name: str):
        """Policy `name` into slot s: ONE ovla_copy_table launch on the current stream (the table of a (policy, slot) pair is built on first use
        and kept).  The forward that follows is ordered behind it on both tower streams: the side stream forks from the current stream at the
        head of vision_fwd (side.wait_stream(main)), and a captured graph replays on the current stream."""
        if self.pool is None or name not in self.pool:
            raise ValueError(f"load_slot: unknown policy {name!r}")
        if not 0 <= s < self.n_slots:
            raise ValueError(f"load_slot: slot {s} of {self.n_slots}")
        tab = self._pool_tables.get((name, s))
        if tab is None:
            pairs = self.pool_slot_pairs(s, name)
            tab = self._pool_tables[(name, s)] = ops.copy_table_build([ops.copy_entry(a, b) for a, b in pairs], self.device, keep=pairs)
        ops.copy_table(tab)
        self.pool_state.names[s] = name
        return tab

    def pool_bytes(self) -> int:
        """Device bytes of the registered policies' adapter and FiLM tensors (the slot storage itself belongs to the linears / FilmSlots)."""
        pols = list((self.pool or {}).values())
        return sum(t.numel() * t.element_size() for p in pols for ab in p["tensors"].values() for t in ab) + \
            sum(t.numel() * t.element_size() for p in pols for t in (p["film"] or {}).values())

    @contextlib.contextmanager
    def routing(self, obs_slot: torch.Tensor, host_slots=None):
        """Inside: every slotted linear of this engine routes by `obs_slot` (device int32 [B], one adapter slot per observation of the forward).
        `host_slots`: the same values on the host, when the caller has them and they will not change under the launches (an eager forward; not a
        graph capture, whose buffer is rewritten before every replay): every routed launch then validates them (OVLA_EINVAL)."""
        assert obs_slot.dtype == torch.int32 and obs_slot.is_cuda and obs_slot.dim() == 1
        rt = self.route
        prev = (rt.obs_slot, rt.n_obs, rt.host_slots)
        rt.obs_slot, rt.n_obs, rt.host_slots = obs_slot, obs_slot.numel(), None if host_slots is None else [int(v) for v in host_slots]
        try:
            yield rt
        finally:
            rt.obs_slot, rt.n_obs, rt.host_slots = prev

    def policy_heads_fwd(self, ah, heads):
        """Every policy's L1 head on all B observations' action rows, then each observation's own prediction (ovla_select_by_slot) -> [B*chunk, action_dim]."""
        preds = torch.stack([h.fwd(ah)[0] for h in heads])                   # [n, B * chunk, action_dim]
        return ops.select_by_slot(preds, self.route.obs_slot, rows_per_obs=self.cfg.chunk, host_slots=self.route.host_slots)

    def lm_head_rows(self, hidden_rows):
        """lm_head on hidden rows [n, D] -> bf16 logits [n rounded up to a multiple of 8 (the GEMM's M granularity), vocab]; the rows past n are
        those of zero inputs."""
        n = hidden_rows.shape[0]
        rows = torch.zeros(((n + 7) // 8 * 8, self.cfg.llm_dim), dtype=BF16, device=self.device)
        rows[:n] = hidden_rows
        return ops.gemm(rows, self.lm_head)

    def merged_state_dict(self) -> Dict[str, torch.Tensor]:
        """Base VLM weights under the reference's HF key layout (un-fused q/k/v, gate/up), after merge_lora(): what
        merge_lora_weights_and_save.py writes with `save_pretrained`."""
        out: Dict[str, torch.Tensor] = {}
        for lin in self.vlm_linears():
            if not isinstance(lin, LoraLinear):
                continue
            gn = lin.group_n
            for g, rn in enumerate(lin.ref_names):
                out[rn + ".weight"] = lin.W[g * gn:(g + 1) * gn]
                if lin.bias is not None:
                    out[rn + ".bias"] = lin.bias[g * gn:(g + 1) * gn]
        return out

    def vlm_linears(self):
        yield from self.dino.linears()
        yield from self.siglip.linears()
        yield from self.proj
        yield from self.llm.linears()

    def refresh_derived(self):
        """Re-derives A^T / B^T / bf16 compute copies from the trainable tensors (after every optimizer step): all LoRA
        transposes of the VLM go in ONE batched launch (their addresses never change, so the descriptor table is built once)."""
        if getattr(self, "_ttab", None) is None:
            pairs = [pr for lin in self.vlm_linears() for pr in lin.derived_pairs()]
            self._ttab = ops.transpose_table(pairs, self.device) if pairs else False
        if self._ttab:
            ops.transpose_batched(self._ttab)
        for lin in self.vlm_linears():
            if isinstance(lin, FullLinear):   # FiLM scale / shift: refresh the bf16 compute copies of the fp32 masters
                lin.refresh_derived()
        for m in (self.proprio, self.noisy, self.head):
            if m is not None:
                for lin in m.linears():
                    lin.refresh_derived()

    def vision_backbone_state_dict(self) -> Dict[str, torch.Tensor]:
        """State dict of the (FiLM-wrapped, LoRA-adapted) vision backbone in the reference's key layout (weights.vision_backbone_keys_to_reference):
        frozen tower tensors + the towers' adapters + the FiLM scale / shift Linears -- the content of `vision_backbone--{step}_checkpoint.pt`
        (vla-scripts/finetune.py:640-655), which `get_vla(cfg)` with `cfg.use_film` loads back (experiments/robot/openvla_utils.py:311-349).
        The discarded last block of each tower is not held by this engine and is absent."""
        from .weights import vision_backbone_keys_to_reference

        if self.film_per_policy:
            raise RuntimeError("vision_backbone_state_dict: a per-policy-FiLM engine holds no FiLM Linears of its own (each policy's live in slot "
                               "storage): there is no single wrapped backbone to export")
        sd = {**self.dino.export_frozen(), **self.siglip.export_frozen()}
        sd.update({k: v for k, v in self.export_trainable("data").items() if k.startswith("vision_backbone.")})
        return vision_backbone_keys_to_reference(sd)

    def export_trainable(self, kind: str = "data") -> Dict[str, torch.Tensor]:
        """Every trainable tensor (or its fp32 gradient) keyed by the reference's parameter names: LoRA adapters as
        `<linear>.lora_A.weight` / `.lora_B.weight` (un-fused per q/k/v, gate/up), components as in their state dicts
        (prismatic/models/action_heads.py, projectors.py; finetune.py:584-675)."""
        out: Dict[str, torch.Tensor] = {}
        for lin in self.all_linears():
            out.update(lin.export(kind))
        if self.head is not None:
            for p in self.head.plain_params():
                out[p.name] = getattr(p, kind)
        for extra_head in (self.scale_head, self.value_head):
            if extra_head is not None:
                for p in extra_head.plain_params():
                    out[p.name] = getattr(p, kind)
        return out

    def load_trainable(self, sd: Dict[str, torch.Tensor], strict: bool = True) -> List[str]:
        """Inverse of export_trainable("data"): copies reference-named tensors (lora adapters, action head, projectors, FiLM)
        into the flat parameter buffers and re-derives the transposes / bf16 compute copies.  Returns the names not found in
        `sd` (raises instead when strict).  finetune.py:134-156,193-209 (resume)."""
        missing = []
        for name, view in self.export_trainable("data").items():
            if name in sd:
                src = sd[name]
                if tuple(src.shape) != tuple(view.shape):
                    raise ValueError(f"{name}: checkpoint shape {tuple(src.shape)} != model shape {tuple(view.shape)}")
                view.copy_(src.to(view.device, view.dtype))
            else:
                missing.append(name)
        for st in self.stores:   # fp32 optimizer state: the master follows what was loaded (a no-op in the default mode)
            st.rewiden_master()
        if missing and strict:
            raise KeyError(f"{len(missing)} trainable tensors missing from the checkpoint, e.g. {missing[:3]}")
        self.refresh_derived()
        return missing

    def optimizer_state_dict(self) -> Dict[str, torch.Tensor]:
        """AdamW moments + step of every parameter store as flat tensors (the layout is a pure function of the config).  The
        reference does not save optimizer state (finetune.py:584-675): this is the SURVEY.md 8f(3) extension."""
        out: Dict[str, torch.Tensor] = {}
        for i, st in enumerate(self.stores):
            if not st.exp_avg:
                st.init_optimizer()
            out[f"store{i}.step"] = torch.tensor([st.step], dtype=torch.int64)
            for dt in st.flat:
                tag = "bf16" if dt == BF16 else "f32"
                out[f"store{i}.{tag}.exp_avg"] = st.exp_avg[dt]
                out[f"store{i}.{tag}.exp_avg_sq"] = st.exp_avg_sq[dt]
                if dt in st.master:   # fp32 mode: the moments above are fp32 as they are, and the master goes with them
                    out[f"store{i}.{tag}.master"] = st.master[dt]
        out["lora_dropout.call"] = torch.tensor([self.dropout.call], dtype=torch.int64)   # the mask stream's position: a resumed run draws the masks the uninterrupted one would
        if self.diffusion is not None:   # ... and the noise and timesteps the uninterrupted one would
            out["diffusion_noise.call"] = torch.tensor([self.diffusion.call], dtype=torch.int64)
        if self.token_sample.call:   # ... and the action tokens (a stream that never drew is not written: a file without the entry loads as call = 0)
            out["token_sample.call"] = torch.tensor([self.token_sample.call], dtype=torch.int64)
        if self.ema_enabled:   # the averaged weights and the position of their decay schedule
            out["ema.step"] = torch.tensor([self.ema_step], dtype=torch.int64)
            for i, st in enumerate(self.stores):
                for dt, shadow in st.ema_shadow.items():
                    out[f"ema.store{i}.{'bf16' if dt == BF16 else 'f32'}.shadow"] = shadow
        if self.grad_clip_enabled:   # the counters of the clip / skip statistics (read back here: a checkpoint waits for the device anyway)
            stats = self.grad_clip_stats()
            for k in ("steps", "clipped", "skipped"):
                out[f"grad_clip.{k}"] = torch.tensor([stats[k]], dtype=torch.int64)
        return out

    def load_optimizer_state_dict(self, sd: Dict[str, torch.Tensor], log=None):
        """Inverse of optimizer_state_dict.  The precision of the checkpoint's state (fp32: it holds a `store{i}.bf16.master`) against this engine's:
          param -> param   the moments are copied.
          param -> fp32    the bf16 moments are widened exactly; the master stays what load_trainable left, the widened loaded parameters.  One
                           line goes to `log` (default: this module's logger).
          fp32  -> fp32    master and moments are copied, then bf16_rne(master) == param is checked on the device: a mismatch means the model
                           files and the optimizer file come from different steps, and raises ValueError.
          fp32  -> param   ValueError before anything is changed: rounding the state back to bf16 is the defect fp32 mode removes."""
        ckpt_fp32 = any(k.endswith(".bf16.master") for k in sd)
        if ckpt_fp32 and not self.store.fp32_state:
            raise ValueError('the optimizer state was saved with fp32 master weights and moments: load it into an engine with '
                             'enable_fp32_optimizer_state() (finetune(..., optimizer_state="fp32")); it is not rounded back to bf16')
        if "lora_dropout.call" in sd:
            self.dropout.call = int(sd["lora_dropout.call"].item()) & 0xFFFFFFFF
        if "diffusion_noise.call" in sd and self.diffusion is not None:
            self.diffusion.call = int(sd["diffusion_noise.call"].item()) & 0xFFFFFFFF
        self.token_sample.call = int(sd["token_sample.call"].item()) & 0xFFFFFFFF if "token_sample.call" in sd else 0   # (a file from before the stream existed)
        for i, st in enumerate(self.stores):
            if not st.exp_avg:
                st.init_optimizer()
            st.step = int(sd[f"store{i}.step"].item())
            for dt in st.flat:
                tag = "bf16" if dt == BF16 else "f32"
                for kind, buf in (("exp_avg", st.exp_avg[dt]), ("exp_avg_sq", st.exp_avg_sq[dt])):
                    src = sd[f"store{i}.{tag}.{kind}"]
                    if src.numel() != buf.numel():
                        raise ValueError(f"optimizer state store{i}.{tag}.{kind}: {src.numel()} elements, model has {buf.numel()}")
                    buf.copy_(src.to(buf.device, buf.dtype))   # (fp32 mode, bf16 moments in the checkpoint: an exact widening)
                if dt in st.master and ckpt_fp32:
                    src = sd[f"store{i}.{tag}.master"]
                    if src.numel() != st.master[dt].numel() or src.dtype != F32:
                        raise ValueError(f"optimizer state store{i}.{tag}.master: {src.numel()} {src.dtype} elements, model has {st.master[dt].numel()} fp32")
                    st.master[dt].copy_(src.to(self.device))
                    if not st.master_matches_param():
                        raise ValueError(f"optimizer state store{i}.{tag}.master does not round to the loaded bf16 parameters: the model files and the "
                                         f"optimizer-state file come from different steps")
        if self.store.fp32_state and not ckpt_fp32:
            (log or logging.getLogger(__name__).info)("[optimizer state] the checkpoint holds bf16 AdamW moments: widened exactly to fp32; the fp32 master "
                                                      "starts at the loaded bf16 parameters")
        if self.ema_enabled:
            self.load_ema_state_dict(sd)
        if self.grad_clip_enabled:
            self.load_grad_clip_state_dict(sd)

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]) -> bool:
        """Restores the shadows and the EMA step from the `ema.` entries of an optimizer state dict into an engine with EMA enabled.
        False, and nothing changes, when `sd` has none (written by a run without EMA)."""
        if "ema.step" not in sd:
            return False
        self._not_in_ema_scope("load_ema_state_dict")
        for i, st in enumerate(self.stores):
            st.ema_step = int(sd["ema.step"].item())
            for dt, shadow in st.ema_shadow.items():
                src = sd[f"ema.store{i}.{'bf16' if dt == BF16 else 'f32'}.shadow"]
                if src.numel() != shadow.numel() or src.dtype != F32:
                    raise ValueError(f"EMA shadow of store{i}: {src.numel()} {src.dtype} elements, model has {shadow.numel()} fp32")
                shadow.copy_(src.to(shadow.device))
        return True

    def num_patches_total(self, num_images: int, use_proprio: bool, use_diffusion: bool = False) -> int:
        """NUM_PATCHES of finetune.py:935-941."""
        return self.cfg.dino.n_patches * num_images + int(use_proprio) + int(use_diffusion)

    # -- forward pieces ----------------------------------------------------------------------------------------------------
    def vision_fwd(self, pixel_values, train: bool, film_avg=None):
        """pixel_values bf16 [B, 6*I, H, W] -> projected patches bf16 [B, I*Np, D] rows, saved.
        modeling_prismatic.py:186-227 + :250-262."""
        cfg = self.cfg
        B, C = pixel_values.shape[0], pixel_values.shape[1]
        I = C // 6
        Np, vd = cfg.dino.n_patches, cfg.vision_dim
        feats = torch.empty((B, I * Np, vd), dtype=BF16, device=self.device)   # == [(B*I), Np, vd]: (b, img) is the tower batch
        tower_saved = [None, None]

        def run_tower(k, tower, c0, col0):
            vc = tower.vc
            T = vc.n_patches + vc.n_prefix
            tok, sv = tower.fwd(pixel_values, c0, I, train, film_avg)
            # drop prefix tokens, concat features on dim 2 and images on dim 1 (modeling_prismatic.py:221-227)
            ops.copy_rows(tok, feats, B * I, Np, vc.dim, src_batch_stride=T * vc.dim, src_row0=vc.n_prefix, src_ld=vc.dim,
                          dst_batch_stride=Np * vd, dst_row0=0, dst_ld=vd, dst_col0=col0)
            tower_saved[k] = sv

        # The towers are independent until the feature concat: SigLIP runs on a second HIP stream beside DINOv2, so the
        # tails of one tower's mid-sized GEMMs and its latency-bound small kernels overlap with the other's work.
        if self.film_per_policy:
            # every block's gamma / beta of both towers, each observation under its own policy's Linears: ONE launch on the current stream,
            # ahead of the fork, so both tower streams are ordered behind it
            if train:
                raise RuntimeError("a per-policy-FiLM engine is inference-only: the FiLM Linears live in frozen slot storage, there is nothing to train")
            if self.film_slots is None or self.route.obs_slot is None:
                raise RuntimeError("per-policy FiLM: the forward must run inside engine.routing(obs_slot) on an engine with policies "
                                   "(set_adapter_slots(..., film=[...]) or the policy pool): without an assignment no observation has FiLM Linears")
            if self.route.n_obs != B or film_avg is None:
                raise RuntimeError(f"per-policy FiLM: the route covers {self.route.n_obs} observations, the forward has {B}")
            self.film_slots.launch(film_avg, self.route)
        side = self._side_stream()
        if side is not None:
            main = torch.cuda.current_stream(self.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                run_tower(1, self.siglip, 3, cfg.dino.dim)
            run_tower(0, self.dino, 0, 0)
            main.wait_stream(side)
        else:
            run_tower(0, self.dino, 0, 0)
            run_tower(1, self.siglip, 3, cfg.dino.dim)
        f2 = feats.view(B * I * Np, vd)
        z1 = torch.empty((f2.shape[0], 4 * vd), dtype=BF16, device=self.device) if train else None
        h1, s1 = self.proj[0].fwd(f2, act=ops.ACT_GELU, c_pre=z1)
        z2 = torch.empty((f2.shape[0], cfg.llm_dim), dtype=BF16, device=self.device) if train else None
        h2, s2 = self.proj[1].fwd(h1, act=ops.ACT_GELU, c_pre=z2)
        out, s3 = self.proj[2].fwd(h2)
        return out.view(B, I * Np, cfg.llm_dim), (tower_saved, s1, z1, s2, z2, s3, B, I)

    def vision_bwd(self, dpatches, saved):
        """dpatches bf16 [B*I*Np, D] contiguous."""
        cfg = self.cfg
        tower_saved, s1, z1, s2, z2, s3, B, I = saved
        Np, vd = cfg.dino.n_patches, cfg.vision_dim
        if _FUSE_ACT:
            d = self.proj[2].bwd(dpatches, s3, dact=("act", z2, ops.ACT_GELU))    # d z2 = d h2 * gelu'(z2), in the dgrad epilogue
            d = self.proj[1].bwd(d, s2, dact=("act", z1, ops.ACT_GELU))           # d z1
        else:
            d = ops.act_bwd(z2, self.proj[2].bwd(dpatches, s3), ops.ACT_GELU)
            d = ops.act_bwd(z1, self.proj[1].bwd(d, s2), ops.ACT_GELU)
        dfeat = self.proj[0].bwd(d, s1)                                           # [B*I*Np, vd]
        def run_tower(k, tower, col0):
            vc = tower.vc
            T = vc.n_patches + vc.n_prefix
            dtok = torch.zeros((B * I * T, vc.dim), dtype=BF16, device=self.device)
            # inverse of the feature concat: rows [n_prefix, T) of tower batch (b, img) <- columns [col0, col0+dim)
            ops.copy_rows(dfeat[:, col0: col0 + vc.dim], dtok, B * I, Np, vc.dim, src_batch_stride=Np * vd, src_row0=0, src_ld=vd,
                          dst_batch_stride=T * vc.dim, dst_row0=vc.n_prefix, dst_ld=vc.dim)
            tower.bwd(dtok, tower_saved[k])

        side = self._side_stream()
        if side is not None:   # same two-stream split as the forward; the towers' gradients live in disjoint buffer ranges
            main = torch.cuda.current_stream(self.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                run_tower(1, self.siglip, cfg.dino.dim)
            run_tower(0, self.dino, 0)
            main.wait_stream(side)   # before dfeat is released and before the optimizer / gradient reducer read the buffers
        else:
            run_tower(1, self.siglip, cfg.dino.dim)
            run_tower(0, self.dino, 0)

    def _side_stream(self):
        """Second HIP stream for the SigLIP tower (OVLA_VIT_STREAMS=1 disables the split)."""
        if os.environ.get("OVLA_VIT_STREAMS", "2") == "1":
            return None
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    # -- the training step pieces -------------------------------------------------------------------------------------------
    def language_average(self, ids_dev, lab_dev):
        """FiLM conditioning vector: mean of the token embeddings at every NON-action position of the text (BOS, prompt,
        stop AND pad tokens: modeling_prismatic.py:581-583 averages `input_embeddings[~all_actions_mask]`;
        film_vit_wrapper.py:243).  One kernel on device tensors (ids / labels int64 [B, L]): no host round trip, so the FiLM forward
        can be captured in a hipGraph.  Returned padded to a multiple of 8 rows (GEMM M granularity of the FiLM Linears)."""
        B = ids_dev.shape[0]
        avg = torch.zeros(((B + 7) // 8 * 8, self.cfg.llm_dim), dtype=BF16, device=self.device)
        return ops.language_average(ids_dev, lab_dev, self.embed, avg)

    def forward(self, input_ids, attention_mask, pixel_values, labels, proprio=None, noisy_actions=None, timestep_emb=None, train=False,
                proprio_projector=None, noisy_action_projector=None, cached_patches=None, sel=None, film_avg=None, attn_capture=None):
        """Multimodal forward (modeling_prismatic.py:571-643 without the discarded lm_head/CE in L1/diffusion mode).
        Returns dict(hidden [B,S,D], P, action_rows [B,A], patches, saved).  `cached_patches` (the `patches` of a previous
        call) skips the vision towers / projector / proprio projector: the DDIM sampler reuses them across its steps
        (modeling_prismatic.py:810).  `sel="actions"` (or an int32 tensor of flattened rows): only those rows of the last hidden state
        are computed (LlamaStack.fwd) and returned as `action_hidden` [n, D]; `hidden` is then None.  `attn_capture` (an AttnCapture): the result
        gains `attention`, the decoder's attention probabilities of the rows it names; everything else keeps its bits."""
        self._refuse_per_policy_film_training(train)
        ids, lab, lens_dev = self.upload_text(input_ids, attention_mask, labels)
        return self.forward_dev(ids, lab, lens_dev, pixel_values, proprio=proprio, noisy_actions=noisy_actions, timestep_emb=timestep_emb, train=train, sel=sel,
                                proprio_projector=proprio_projector, noisy_action_projector=noisy_action_projector, cached_patches=cached_patches, film_avg=film_avg,
                                attn_capture=attn_capture)

    def _refuse_per_policy_film_training(self, train: bool):
        if train and self.film_per_policy:
            raise RuntimeError("a per-policy-FiLM engine is inference-only: the FiLM Linears live in frozen slot storage, there is nothing to train")

    def upload_text(self, input_ids, attention_mask, labels):
        """The text side of a batch (host or device tensors [B, L]), validated on the host before anything is uploaded ->
        (ids int64 [B, L], labels int64 [B, L], text lengths int32 [B]) on the device."""
        dev = self.device
        B, L = input_ids.shape
        lens = self.check_right_padding(attention_mask)
        if not labels.is_cuda:   # (device-resident labels cannot be read without a sync: ovla_gather_rows skips the -1 a short row leaves)
            self.check_action_labels(labels, self.cfg.num_action_tokens)
        if input_ids.is_cuda or labels.is_cuda or not _ASYNC_UPLOAD:
            ids = input_ids.to(dev, torch.int64).contiguous()
            lab = labels.to(dev, torch.int64).contiguous()
            lens_dev = lens.to(torch.int32).to(dev)
        else:
            # ONE asynchronous upload per step from pinned memory (ids | labels | lengths packed): a pageable `.to(device)` is a synchronous copy
            # queued behind the whole previous step, so the host re-joined the GPU at every step boundary and started the ~3500 launches of the next
            # step from zero lead -- during the towers' 10-25 us kernels the GPU then ran at the host's launch rate.  PyTorch's caching host
            # allocator keeps the pinned block alive until the copy has completed.
            packed = torch.cat([input_ids.reshape(-1).to(torch.int64), labels.reshape(-1).to(torch.int64), lens.reshape(-1).to(torch.int64)]).pin_memory()
            packed_dev = packed.to(dev, non_blocking=True)
            ids, lab = packed_dev[: B * L].view(B, L), packed_dev[B * L: 2 * B * L].view(B, L)
            lens_dev = packed_dev[2 * B * L:].to(torch.int32)
        return ids, lab, lens_dev

    @staticmethod
    def check_right_padding(attention_mask) -> torch.Tensor:
        """Host-side validation of the collator's mask; returns the per-row text lengths (int64, CPU)."""
        am = attention_mask.to("cpu").bool()
        L = am.shape[1]
        lens = am.sum(1)
        if not bool((am == (torch.arange(L)[None, :] < lens[:, None])).all()):
            raise ValueError("attention_mask must be right padding (a prefix of ones per row), as produced by the reference collator")
        return lens

    @staticmethod
    def check_action_labels(labels, num_action_tokens: int, action_token_begin: int = 31743):
        """Host-side validation of the action labels: every row holds exactly `num_action_tokens` labels above `action_token_begin` (the rule
        of ovla_assemble_multimodal's action mask; IGNORE_INDEX never counts).  A truncated sample would leave -1 in `action_rows`, one with
        more would drop slots silently; the reference fails on both with a reshape error.  Raises before anything is uploaded or launched."""
        counts = (labels.to("cpu") > action_token_begin).sum(1)
        bad = torch.nonzero(counts != num_action_tokens).reshape(-1)
        if bad.numel():
            b = int(bad[0])
            raise ValueError(f"labels: row {b} holds {int(counts[b])} action labels (ids above {action_token_begin}), the model takes exactly "
                             f"{num_action_tokens} per row ({bad.numel()} of {labels.shape[0]} rows are malformed)")

    def patches_dev(self, ids, lab, pixel_values, proprio, proprio_projector, film_avg, train):
        """The step-independent front of forward_dev: FiLM average (unless given), both towers, the projector and the proprio token ->
        (base bf16 [B, n_vis (+ 1), D], n_vis, vision saved, proprio saved).  (base, n_vis) is forward_dev's `cached_patches`: the DDIM
        sampler computes it once per chunk (DiffusionGraph's prefix capture)."""
        cfg, dev = self.cfg, self.device
        B = ids.shape[0]
        psaved = None
        if not train:
            self.dropout.end_forward()   # (entered on its own by a graph's prefix capture: never drops, whatever ran before)
        if self.use_film and film_avg is None:
            film_avg = self.language_average(ids, lab)
        patches, vsaved = self.vision_fwd(pixel_values.to(dev, BF16).contiguous(), train, film_avg)
        n_vis = patches.shape[1]
        base = patches
        if proprio is not None and proprio_projector is not None:
            pr = torch.zeros(((B + 7) // 8 * 8, cfg.proprio_dim), dtype=BF16, device=dev)
            pr[:B] = proprio.reshape(B, -1).to(dev, BF16)
            pf, psaved = proprio_projector.fwd(pr, train)
            base = torch.empty((B, n_vis + 1, cfg.llm_dim), dtype=BF16, device=dev)   # token concat (pure data movement)
            base[:, :n_vis] = patches
            base[:, n_vis] = pf[:B]
        return base, n_vis, vsaved, psaved

    def forward_dev(self, ids, lab, text_lens, pixel_values, proprio=None, noisy_actions=None, timestep_emb=None, train=False,
                    proprio_projector=None, noisy_action_projector=None, cached_patches=None, film_avg=None, sel=None, attn_capture=None):
        """Device-only part of forward(): ids / lab int64 [B, L] and text_lens int32 [B] already on the device; launches
        kernels and allocates, never synchronises or reads host memory -- the part a hipGraph can capture (ChunkGraph)."""
        self._refuse_per_policy_film_training(train)
        self.dropout.begin_forward(train)
        try:
            return self._forward_dev(ids, lab, text_lens, pixel_values, proprio, noisy_actions, timestep_emb, train, proprio_projector,
                                     noisy_action_projector, cached_patches, film_avg, sel, attn_capture)
        finally:
            self.dropout.end_forward()

    def _forward_dev(self, ids, lab, text_lens, pixel_values, proprio, noisy_actions, timestep_emb, train, proprio_projector,
                     noisy_action_projector, cached_patches, film_avg, sel, attn_capture=None):
        cfg = self.cfg
        dev = self.device
        B, L = ids.shape
        proprio_projector = proprio_projector if proprio_projector is not None else self.proprio
        noisy_action_projector = noisy_action_projector if noisy_action_projector is not None else self.noisy
        vsaved = psaved = nsaved = None
        if cached_patches is not None:
            base, n_vis = cached_patches
        else:
            base, n_vis, vsaved, psaved = self.patches_dev(ids, lab, pixel_values, proprio, proprio_projector, film_avg, train)
        allp = base
        if timestep_emb is not None:
            allp = torch.empty((B, base.shape[1] + 1, cfg.llm_dim), dtype=BF16, device=dev)
            allp[:, : base.shape[1]] = base
            allp[:, base.shape[1]] = timestep_emb.to(dev, BF16).reshape(B, cfg.llm_dim)
        P = allp.shape[1]
        A = cfg.num_action_tokens
        noisy_feats = None
        if noisy_actions is not None:
            rows = (B * A + 7) // 8 * 8
            na = torch.zeros((rows, 1), dtype=BF16, device=dev)
            na[: B * A] = noisy_actions.reshape(B * A, 1).to(dev, BF16)
            nf, nsaved = noisy_action_projector.fwd(na, train)
            noisy_feats = nf[: B * A].view(B, A, cfg.llm_dim)
        mm, action_rows = ops.assemble_multimodal(ids, lab, self.embed, allp.contiguous(), A=A, noisy=noisy_feats, action_dim=cfg.action_dim)
        S = P + L
        kv_len = (text_lens + P).to(torch.int32)
        sel_rows = None
        if sel is not None and os.environ.get("OVLA_LAST_LAYER_SEL", "1") != "0":    # A/B switch
            sel_rows = action_rows.reshape(-1) if isinstance(sel, str) else sel
            if sel_rows.numel() % 8 != 0:
                sel_rows = None          # (e.g. ALOHA discrete: 4 x 351 rows) -> the full last layer
        if attn_capture is not None:
            attn_capture.begin(len(self.llm.layers), action_rows, B, S, cfg.llm_heads, dev)
        hidden, lsaved = self.llm.fwd(mm.view(B * S, cfg.llm_dim), B, S, kv_len, train, sel=sel_rows, attn_capture=attn_capture)
        saved = ForwardSaved(vsaved, psaved, nsaved, lsaved, B, S, P, n_vis, proprio_projector, noisy_action_projector, action_rows) if train else None
        # `all_patches` [B, P, D]: what sits between BOS and the text in the multimodal sequence (projected patches + proprio + timestep
        # tokens) = the reference's `projector_features` (modeling_prismatic.py:586-599, 674)
        on_rows = sel_rows is not None                                       # then `hidden` holds those rows only
        out = dict(hidden=None if on_rows else hidden.view(B, S, cfg.llm_dim), action_hidden=hidden if on_rows else None, sel_rows=sel_rows, P=P, S=S,
                   action_rows=action_rows, patches=(base, n_vis), saved=saved, all_patches=allp)
        if attn_capture is not None:
            out["attention"] = attn_capture.result()
            out["kv_len"] = kv_len
        return out

    def action_hidden(self, out):
        """(hidden rows that predict the action slots [B*A, D], their flattened row indices) of a forward() result, whether the last
        layer ran on the selected rows only (`sel="actions"`) or on all of them."""
        if out.get("action_hidden") is not None:
            return out["action_hidden"], out["sel_rows"]
        return self.gather_action_hidden(out["hidden"], out["action_rows"])

    def gather_action_hidden(self, hidden, action_rows):
        """Rows of hidden that predict the action slots: the hidden state at token i-1 predicts token i
        (finetune.py:385-394: text_hidden = last_hidden[:, P:-1] indexed with masks built from labels[:, 1:];
        modeling_prismatic.py:915-920).  `action_rows` (flattened (b, s) row of slot - 1) comes from the assembly kernel."""
        B, S, D = hidden.shape
        idx = action_rows.reshape(-1)
        return ops.gather_rows(hidden.view(B * S, D), idx, D), idx

    def backward_from_hidden(self, dhidden, saved):
        """dhidden bf16 [B*S, D] (gradient of hidden_states[-1]; [n, D] for the selected rows when the forward ran with `sel`) ->
        accumulates every VLM / projector gradient."""
        B, S, n_vis, D = saved.B, saved.S, saved.n_vis, self.cfg.llm_dim
        dmm_flat = self.llm.bwd(dhidden, saved.lsaved)
        dmm = dmm_flat.view(B, S, D)
        if saved.nsaved is not None:
            # the projected noisy-action features sit AT the action slots: one row after the row that predicts them
            slot_rows = (saved.action_rows.reshape(-1) + 1).contiguous()
            n = slot_rows.numel()
            dn = torch.zeros(((n + 7) // 8 * 8, D), dtype=BF16, device=self.device)
            ops.gather_rows(dmm_flat, slot_rows, D, dst=dn)
            saved.noisy_action_projector.bwd(dn, saved.nsaved)
        if saved.psaved is not None:
            dpr = torch.zeros(((B + 7) // 8 * 8, D), dtype=BF16, device=self.device)
            dpr[:B] = dmm[:, 1 + n_vis]
            saved.proprio_projector.bwd(dpr, saved.psaved)
        dpatches = dmm[:, 1: 1 + n_vis].contiguous().view(B * n_vis, D)
        self.vision_bwd(dpatches, saved.vsaved)

    def backward_from_rows(self, drows, rows_idx, out, run: bool = True):
        """drows bf16 [n, D], the gradient of the hidden rows `rows_idx` of the forward result `out`, sent into the decoder: as it is when the last layer
        ran on exactly these rows, else scatter-added into a zero [B*S, D].  `run=False` returns that instead (the autograd bridge calls later)."""
        if out["sel_rows"] is None:
            dhidden = torch.zeros((out["action_rows"].shape[0] * out["S"], drows.shape[1]), dtype=BF16, device=self.device)
            drows = ops.gather_rows(drows, rows_idx, drows.shape[1], dst=dhidden, scatter_add=True)
        if not run:
            return drows
        self.backward_from_hidden(drows, out["saved"])

    def attach_reducer(self, reducer, overlap: bool = True):
        """Overlaps the data-parallel gradient all-reduce with the backward: the head's gradients go out as soon as its
        backward is done, each Llama layer's LoRA gradients as soon as that layer is done (the flat buffers are in
        completion order), the rest (projector, ViT towers, proprio projector) at the end of the step."""
        self.reducer = reducer
        self._overlap = overlap and reducer is not None
        if not self._overlap:
            self.llm.on_grads_ready = None
            return

        def llm_layer_done(first_param):   # first-registered param of the layer = LAST in the reversed layout
            reducer.notify(self.store, BF16, first_param.offset + (first_param.numel + ParamStore.ALIGN - 1) // ParamStore.ALIGN * ParamStore.ALIGN)

        self.llm.on_grads_ready = llm_layer_done

    def train_step_fwd_bwd(self, batch: dict, loss_scale: float = 1.0, action_head=None, proprio_projector=None, diffusion=None,
                           noisy_action_projector=None, film_avg=None, attn_capture=None, fit_scale: bool = False):
        """One run_forward_pass (finetune.py:280-451) + backward.  L1 branch by default; with
        `diffusion = dict(noise, noisy_actions, timestep_emb)` the noise-prediction MSE branch (:402-407).
        Gradients accumulate in the flat buffers.  `film_avg` (what language_average returns) replaces the FiLM conditioning vector the forward
        would compute from the batch's own ids.  `attn_capture` (an AttnCapture): filled by the step's forward (read its result() afterwards); loss and
        gradients keep their bits.  Returns (loss_sum fp32[1] device, element count, predictions).
        `fit_scale` (L1 only, attach_scale_head): after the L1 backward, the maximum-likelihood side step of the scale head on the step's own
        hidden output and predictions (_nll_of_target: three launches into the scale head's store alone; its dict(nll, scale) is left in
        `self.last_scale_fit`).  The L1 step's loss, predictions and every other gradient accumulator keep their bits."""
        self._not_in_ema_scope("train_step_fwd_bwd")
        if fit_scale:
            if diffusion is not None or self.head_kind != "l1":
                raise ValueError("fit_scale fits the Laplace scale of the L1 head: not with a diffusion objective")
            self._learned("learned", "train_step_fwd_bwd(fit_scale=True)")
        extra = {} if attn_capture is None else dict(attn_capture=attn_capture)
        if fit_scale:
            extra["fit_scale"] = True
        return self._head_step(batch, diffusion, action_head if action_head is not None else self.head, loss_scale,
                               proprio_projector=proprio_projector, noisy_action_projector=noisy_action_projector, film_avg=film_avg, **extra)

    def eval_step(self, batch: dict, diffusion=None, discrete: bool = False):
        """run_forward_pass under torch.no_grad() (run_validation, finetune.py:678-760): the same loss as the training step,
        no activations kept, no gradients touched.  Returns (loss_sum fp32[1] device, count, predictions)."""
        if discrete:
            return self.train_step_discrete(batch, backward=False)
        return self._head_step(batch, diffusion, self.head, None)

    last_scale_fit: Optional[Dict[str, torch.Tensor]] = None   # dict(nll, scale) of the last train_step_fwd_bwd(fit_scale=True), device scalars

    def _head_step(self, batch: dict, diffusion, head, loss_scale: Optional[float], noisy_action_projector=None, fit_scale: bool = False, **fwd_kw):
        """The L1 / noise-prediction MSE objective of one batch: the forward on the action rows, the head and its loss; with a `loss_scale`
        (the training step) also the backward of both, and with `fit_scale` the scale head's side step after them.
        -> (loss_sum fp32[1] device, element count, predictions)."""
        cfg, train = self.cfg, loss_scale is not None
        if diffusion is not None:
            fwd_kw.update(noisy_actions=diffusion["noisy_actions"], timestep_emb=diffusion["timestep_emb"], noisy_action_projector=noisy_action_projector)
        out = self.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"),
                           train=train, sel="actions", **fwd_kw)
        ah, idx = self.action_hidden(out)
        tgt_src = diffusion["noise"] if diffusion is not None else batch["actions"]
        target = tgt_src.to(self.device, BF16).reshape(batch["input_ids"].shape[0] * cfg.chunk, cfg.action_dim).contiguous()
        if fit_scale:
            pred, loss_sum, hsaved, h2 = head.fwd(ah, target=target, mse=False, train=train, return_hidden=True)
        else:
            pred, loss_sum, hsaved = head.fwd(ah, target=target, mse=diffusion is not None, train=train)
        if train:
            dah = head.bwd(hsaved, dloss=loss_scale)
            if getattr(self, "_overlap", False) and hasattr(head, "store"):
                for dt, g in head.store.flat_grad.items():
                    self.reducer.notify(head.store, dt, g.numel())
            self.backward_from_rows(dah, idx, out)
            if fit_scale:
                with torch.no_grad():
                    self.last_scale_fit = self._nll_of_target(pred, h2, target, loss_scale)
        return loss_sum, pred.numel(), pred

    # -- the diffusion objective on the device ------------------------------------------------------------------------------
    def _diffusion_state(self, who: str) -> DiffusionNoiseState:
        if self.diffusion is None or self.head is None or self.noisy is None:
            raise RuntimeError(f"{who} needs an engine built with head='diffusion' and num_diffusion_steps")
        return self.diffusion.tables(self.cfg.llm_dim, self.device)

    def _actions_dev(self, actions) -> torch.Tensor:
        """Ground-truth chunks bf16 [B, chunk * action_dim] on the device; a host tensor goes up from pinned memory without blocking."""
        B = actions.shape[0]
        if not actions.is_cuda:
            a = actions.to(BF16).reshape(B, -1).contiguous()
            return a.pin_memory().to(self.device, non_blocking=True) if _ASYNC_UPLOAD else a.to(self.device)
        return actions.to(self.device, BF16).reshape(B, -1)

    def draw_diffusion(self, actions) -> Dict[str, torch.Tensor]:
        """DiffusionActionHead.sample_noisy_actions (action_heads.py:167-197) in one launch on the device: the `diffusion` argument of
        train_step_fwd_bwd / eval_step -- dict(noise, noisy_actions bf16 [B, chunk, action_dim], timestep_emb bf16 [B, D], timesteps int32 [B]),
        all device tensors, a pure function of (seed, call) by ovla.h "Diffusion noise".  Advances `call` by one; reads nothing back."""
        st = self._diffusion_state("draw_diffusion")
        a = self._actions_dev(actions)
        shape = (a.shape[0], self.cfg.chunk, self.cfg.action_dim)
        noise, noisy, temb, ts = ops.diffusion_noise(a, st.ab, st.temb_table, seed=st.seed, call=st.call, stream=0)
        st.call = (st.call + 1) & 0xFFFFFFFF
        return dict(noise=noise.view(shape), noisy_actions=noisy.view(shape), timestep_emb=temb, timesteps=ts)

    def sample_actions(self, batch: dict, start_noise=None) -> torch.Tensor:
        """The reverse diffusion of a whole batch (finetune.py:454-540, the sampled-L1 metrics of the diffusion objective) as eager launches with
        no host round trip: per DDIM step ovla_ddim_prepare, the forward on the cached patches, the noise-predicting head, ovla_ddim_step; the
        step index and the sample live on the device (DiffusionGraph's step, uncaptured), the rounding points are those of the host loop of
        OpenVLAForActionPrediction._infer.  Inference mode (no dropout, adapters unmerged), no gradients.  Start noise: `start_noise`
        [B, chunk, action_dim], else stream 2 of the noise generator at the current `call` (not advanced: every draw_diffusion moves it on).
        -> bf16 [B, chunk, action_dim] on the device."""
        st = self._diffusion_state("sample_actions")
        cfg, dev = self.cfg, self.device
        B = batch["input_ids"].shape[0]
        n = B * cfg.chunk * cfg.action_dim
        with torch.no_grad():
            ids, lab, lens_dev = self.upload_text(batch["input_ids"], batch["attention_mask"], batch["labels"])   # (raises before any launch)
            if start_noise is None:
                zeros = torch.zeros((B, cfg.chunk * cfg.action_dim), dtype=BF16, device=dev)
                start = ops.diffusion_noise(zeros, st.ab, st.temb_table, seed=st.seed, call=st.call, stream=2)[0]
            else:
                start = torch.as_tensor(start_noise).to(BF16).to(dev)
            assert start.numel() == n, f"start noise of {start.numel()} elements for {n}"
            sample = start.reshape(-1).to(F32).contiguous()       # bf16-rounded values held in fp32, as the host loop holds them
            step = torch.zeros(1, dtype=torch.int32, device=dev)
            temb = torch.empty((B, cfg.llm_dim), dtype=BF16, device=dev)
            noisy = torch.empty(n, dtype=BF16, device=dev)
            cached = None
            for _ in range(st.T):
                ops.ddim_prepare(step, st.step_temb, temb, sample, noisy)
                out = self.forward_dev(ids, lab, lens_dev, batch["pixel_values"], proprio=batch.get("proprio"), noisy_actions=noisy, timestep_emb=temb,
                                       train=False, cached_patches=cached, sel="actions")
                cached = out["patches"]                           # vision features reused across the steps
                ah, _ = self.action_hidden(out)
                eps = self.head.fwd(ah)[0]
                ops.ddim_step(sample, eps, st.coef, step)
            return sample.to(BF16).view(B, cfg.chunk, cfg.action_dim)

    def train_step_discrete(self, batch: dict, loss_scale: float = 1.0, proprio_projector=None, backward: bool = True):
        """run_forward_pass's discrete branch (finetune.py:357-378) + backward: `loss = output.loss`, the LlamaForCausalLM
        next-token cross entropy over the multimodal labels (logits.float(), shift by one, ignore_index -100, mean), with the
        frozen lm_head applied ONLY to the rows whose shifted label counts (the action tokens and the stop token: A + 1 rows per
        sample instead of all S).  Returns (loss_sum fp32[1] device, token count, predicted ids int64 [B, L - 1] on the host
        layout of `output.logits[:, num_patches:-1].argmax(2)` with -1 where no row was evaluated)."""
        if backward:
            self._not_in_ema_scope("train_step_discrete")
        if self.lm_head is None:
            raise RuntimeError("the discrete objective needs language_model.lm_head.weight in the checkpoint")
        labels = batch["labels"].to("cpu", torch.int64)
        self.check_action_labels(labels, self.cfg.num_action_tokens)
        B, L = labels.shape
        use_pp = batch.get("proprio") is not None and (proprio_projector is not None or self.proprio is not None)
        P = self.num_patches_total(batch["pixel_values"].shape[1] // 6, use_pp)
        bb, jj, rows_idx, targets = self.counted_rows(labels, P + L, P)
        n_tok = rows_idx.numel()
        out = self.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"),
                           train=backward, proprio_projector=proprio_projector, sel=rows_idx)     # last layer on the counted rows only
        assert out["P"] == P and out["S"] == P + L
        loss_rows, amax, dlogits = self.lm_loss_fwd(out, rows_idx, targets, grad_scale=loss_scale / n_tok if backward else None)
        pred = torch.full((B, L - 1), -1, dtype=torch.int64)
        pred[bb, jj] = amax.to("cpu", torch.int64)
        if backward:
            self.backward_from_rows(self.lm_loss_bwd(dlogits), rows_idx, out)
        return loss_rows.sum().reshape(1), n_tok, pred

    # -- stochastic decoding and the policy-gradient objective on the action tokens (ovla.h "Token sampling and the policy-gradient objective") --
    def token_window(self, window) -> Tuple[int, int]:
        """"actions": the n_action_bins ids the action tokenizer writes, [n_tokens - n_action_bins, n_tokens); "vocab": every lm_head row; or (lo, hi)."""
        n_tokens = self.cfg.vocab - self.cfg.pad_to_multiple_of
        if window == "actions":
            return n_tokens - self.cfg.n_action_bins, n_tokens
        if window == "vocab":
            return 0, self.cfg.vocab
        if isinstance(window, (tuple, list)) and len(window) == 2:
            return int(window[0]), int(window[1])
        raise ValueError(f'window = {window!r} ("actions", "vocab" or (lo, hi))')

    def _action_logits(self, batch: dict, train: bool, who: str):
        """The forward on the action rows and lm_head on them -> (out, rows_idx, bf16 logits [B * A padded to 8, vocab], B * A).  The action slots'
        inputs are zeroed by ovla_assemble_multimodal: the logits do not depend on which tokens the labels hold there."""
        if self.lm_head is None:
            raise RuntimeError(f"{who} needs language_model.lm_head.weight in the checkpoint")
        out = self.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"),
                           train=train, sel="actions")
        ah, idx = self.action_hidden(out)
        return out, idx, self.lm_head_rows(ah), ah.shape[0]

    def _rows_dev(self, t, dtype, B: int, what: str):
        """A per-token [B, A] or (with `per_obs`) per-observation [B] host or device tensor -> contiguous [B * A] on the device."""
        A = self.cfg.num_action_tokens
        t = torch.as_tensor(t).to(self.device, dtype)
        if t.numel() == B and t.dim() <= 1 and what == "advantages":
            t = t.reshape(B, 1).expand(B, A)
        if t.numel() != B * A:
            raise ValueError(f"{what}: {tuple(t.shape)} for {B} observations of {A} action tokens")
        return t.reshape(B * A).contiguous()

    def _group_rows(self, t, dtype, B: int, G: int, what: str, per_draw: bool = False):
        """A per-token [B, G, A] (or, with `per_draw`, per-draw [B, G]) host or device tensor -> contiguous [B * A, G] on the device: the group
        kernels' layout, one row of G samples per action row."""
        A = self.cfg.num_action_tokens
        t = torch.as_tensor(t).to(self.device, dtype)
        if per_draw and tuple(t.shape) == (B, G):
            t = t.reshape(B, G, 1).expand(B, G, A)
        if tuple(t.shape) != (B, G, A):
            raise ValueError(f"{what}: {tuple(t.shape)} for {B} observations of {G} draws of {A} action tokens")
        return t.permute(0, 2, 1).reshape(B * A, G).contiguous()

    def _group_out(self, t, B: int, G: int):
        """[B * A, G] kernel output -> [B, G, A]."""
        return t.view(B, self.cfg.num_action_tokens, G).permute(0, 2, 1).contiguous()

    def _sample_action_tokens_group(self, batch: dict, G: int, temperature: float, window, row_keys):
        """sample_action_tokens(num_samples=G): one forward, ONE ovla_sample_tokens_group launch.  Observation b's draw g has the key
        row_keys[b, g] (default b * G + g), its token a the generator key `key * A + a` -- what the single-draw call gives an observation under
        that key, so draw (b, g) is that call's draw bit for bit."""
        cfg, B = self.cfg, batch["input_ids"].shape[0]
        A, G = cfg.num_action_tokens, int(G)
        if not 1 <= G <= ops.PG_GROUP_MAX:
            raise ValueError(f"num_samples = {G} (1 .. {ops.PG_GROUP_MAX})")
        lo, hi = self.token_window(window)
        keys = torch.arange(B * G, dtype=torch.int32, device=self.device).view(B, G) if row_keys is None else torch.as_tensor(row_keys).to(self.device, torch.int32)
        if tuple(keys.shape) == (B, G):
            keys = keys.reshape(B, G, 1) * A + torch.arange(A, dtype=torch.int32, device=self.device)[None, None, :]
        keys = self._group_rows(keys, torch.int32, B, G, "row_keys")
        with torch.no_grad():
            _, _, logits, n = self._action_logits(batch, False, "sample_action_tokens")
            st = self.token_sample
            tok, bins, lp, ent = ops.sample_tokens_group(logits[:n], G, n_tokens=cfg.vocab - cfg.pad_to_multiple_of, n_bins=cfg.n_action_bins - 1, window=(lo, hi),
                                                         temperature=temperature, seed=st.seed, call=st.advance(), row_key=keys)
        return dict(tokens=self._group_out(tok, B, G), bins=self._group_out(bins, B, G), logprob=self._group_out(lp, B, G), entropy=ent.view(B, A))

    def sample_action_tokens(self, batch: dict, temperature: float = 1.0, window="actions", row_keys=None, num_samples: Optional[int] = None):
        """Draws the chunk's action tokens from softmax(logits[window] / temperature): one forward (inference mode) on the action rows, lm_head
        on them, ONE ovla_sample_tokens launch; nothing is read back.  `row_keys` int32 [B, A] (or [B]: key * A + a per token) replaces the
        row index in the generator's counter, so k draws of one observation in a batch differ and a draw does not depend on its position.
        Advances the token stream's `call` by one.  -> dict(tokens, bins int32, logprob, entropy fp32), each [B, A] on the device.
        `num_samples=G`: G draws per observation from the ONE forward (one ovla_sample_tokens_group launch, `call` advanced once): tokens / bins /
        logprob [B, G, A], entropy [B, A]; `row_keys` [B, G] (key * A + a per token; default b * G + g) or [B, G, A]."""
        if num_samples is not None:
            return self._sample_action_tokens_group(batch, num_samples, temperature, window, row_keys)
        cfg, B = self.cfg, batch["input_ids"].shape[0]
        A = cfg.num_action_tokens
        lo, hi = self.token_window(window)
        keys = None
        if row_keys is not None:
            keys = torch.as_tensor(row_keys).to(self.device, torch.int32)
            if keys.numel() == B:
                keys = keys.reshape(B, 1) * A + torch.arange(A, dtype=torch.int32, device=self.device)[None, :]
            if keys.numel() != B * A:
                raise ValueError(f"row_keys: {tuple(keys.shape)} for {B} observations of {A} action tokens")
            keys = keys.reshape(B * A).contiguous()
        with torch.no_grad():
            _, _, logits, n = self._action_logits(batch, False, "sample_action_tokens")
            st = self.token_sample
            tok, bins, lp, ent = ops.sample_tokens(logits[:n], n_tokens=cfg.vocab - cfg.pad_to_multiple_of, n_bins=cfg.n_action_bins - 1, window=(lo, hi),
                                                   temperature=temperature, seed=st.seed, call=st.advance(), row_key=keys)
        return dict(tokens=tok.view(B, A), bins=bins.view(B, A), logprob=lp.view(B, A), entropy=ent.view(B, A))

    def policy_logprobs(self, batch: dict, tokens, temperature: float = 1.0, window="actions"):
        """Log-probability and entropy of given action tokens [B, A] under the current weights: the forward of sample_action_tokens, then
        ovla_token_pg without a gradient -- for the tokens a draw returned, the bits that draw reported.  -> dict(logprob, entropy) [B, A].
        Tokens [B, G, A] (a group draw): one forward, one ovla_token_pg_group launch -> logprob [B, G, A], entropy [B, A]."""
        B, A = batch["input_ids"].shape[0], self.cfg.num_action_tokens
        if torch.as_tensor(tokens).dim() == 3:
            G = torch.as_tensor(tokens).shape[1]
            tok = self._group_rows(tokens, torch.int32, B, G, "tokens")
            with torch.no_grad():
                _, _, logits, n = self._action_logits(batch, False, "policy_logprobs")
                lp, _, _, _, ent, _ = ops.token_pg_group(logits[:n], tok, torch.ones((n, G), dtype=F32, device=self.device), window=self.token_window(window),
                                                         temperature=temperature)
            return dict(logprob=self._group_out(lp, B, G), entropy=ent.view(B, A))
        tok = self._rows_dev(tokens, torch.int32, B, "tokens")
        with torch.no_grad():
            _, _, logits, n = self._action_logits(batch, False, "policy_logprobs")
            lp, ent, _, _, _ = ops.token_pg(logits[:n], tok, torch.ones(n, dtype=F32, device=self.device), window=self.token_window(window), temperature=temperature)
        return dict(logprob=lp.view(B, A), entropy=ent.view(B, A))

    def train_step_policy_gradient(self, batch: dict, tokens, advantages, old_logprobs=None, clip=(0.8, 1.2), temperature: float = 1.0, window="actions",
                                   loss_scale: float = 1.0):
        """One policy-gradient micro-step on drawn action tokens: the PPO / GRPO clipped surrogate
            loss = -(1 / (B A)) sum_{b, a} min(ratio A_b, clip(ratio, clip[0], clip[1]) A_b),   ratio = exp(logprob - old_logprob)  (1 without old_logprobs)
        and its backward through lm_head and the decoder, into the flat gradient buffers.  `tokens` int32 [B, A], `advantages` [B] or [B, A],
        `old_logprobs` [B, A] (what sample_action_tokens / policy_logprobs returned when the tokens were drawn), host or device tensors.
        The forward does not depend on `tokens` (the action slots' inputs are zero): they only select the targets.
        -> dict of device scalars: loss, logprob (mean), entropy (mean), clip_frac, ratio (mean)."""
        self._not_in_ema_scope("train_step_policy_gradient")
        self._refuse_per_policy_film_training(True)
        B = batch["input_ids"].shape[0]
        tok = self._rows_dev(tokens, torch.int32, B, "tokens")
        adv = self._rows_dev(advantages, F32, B, "advantages")
        old = None if old_logprobs is None else self._rows_dev(old_logprobs, F32, B, "old_logprobs")
        lo, hi = self.token_window(window)
        out, idx, logits, n = self._action_logits(batch, True, "train_step_policy_gradient")
        lp, ent, ratio, clipped, _ = ops.token_pg(logits[:n], tok, adv, window=(lo, hi), temperature=temperature, old_logprob=old, clip=clip,
                                                  grad_scale=loss_scale / n, inplace_grad=True)
        logits[n:].zero_()
        dah = self.lm_loss_bwd(logits)
        if getattr(self, "_overlap", False) and self.head is not None and hasattr(self.head, "store"):   # (no head trains here: its gradients are final)
            for dt, g in self.head.store.flat_grad.items():
                self.reducer.notify(self.head.store, dt, g.numel())
        self.backward_from_rows(dah, idx, out)
        # the surrogate's value from the row outputs (device arithmetic, nothing read back): min(r A, clip(r) A)
        surr = torch.minimum(ratio * adv, ratio.clamp(float(clip[0]), float(clip[1])) * adv)
        return dict(loss=-surr.mean(), logprob=lp.mean(), entropy=ent.mean(), clip_frac=clipped.to(F32).mean(), ratio=ratio.mean())

    def train_step_policy_gradient_group(self, batch: dict, tokens, advantages, old_logprobs=None, ref_logprobs=None, kl_coef: float = 0.0,
                                         entropy_coef: float = 0.0, clip=(0.8, 1.2), temperature: float = 1.0, window="actions", loss_scale: float = 1.0):
        """One GRPO / PPO micro-step on G drawn chunks per observation, from ONE forward and ONE backward:
            loss = (1 / (B A G)) sum_{b, g, a} [ -min(ratio A_bg, clip(ratio) A_bg) + kl_coef kl ]  -  entropy_coef (1 / (B A)) sum_{b, a} H
        with kl = expm1(d) - d, d = ref_logprob - logprob (Schulman's k3 estimator of KL(policy || reference)) and H the row entropy.  The forward
        does not depend on the tokens, so the G surrogates share the logits and their gradients are summed in dlogits (ovla_token_pg_group, in
        place) before lm_head's and the decoder's backward.  `tokens` int32 [B, G, A]; `advantages` [B, G] or [B, G, A]; `old_logprobs` /
        `ref_logprobs` [B, G, A] (sample_action_tokens(num_samples=G) / reference_logprobs), host or device tensors.
        -> dict of device scalars: loss, logprob, entropy, clip_frac, ratio, kl (means; kl is 0 without ref_logprobs)."""
        self._not_in_ema_scope("train_step_policy_gradient_group")
        self._refuse_per_policy_film_training(True)
        B = batch["input_ids"].shape[0]
        tokens = torch.as_tensor(tokens)
        if tokens.dim() != 3:
            raise ValueError(f"tokens: {tuple(tokens.shape)} ([B, G, A])")
        G = tokens.shape[1]
        tok = self._group_rows(tokens, torch.int32, B, G, "tokens")
        adv = self._group_rows(advantages, F32, B, G, "advantages", per_draw=True)
        old = None if old_logprobs is None else self._group_rows(old_logprobs, F32, B, G, "old_logprobs")
        ref = None if ref_logprobs is None else self._group_rows(ref_logprobs, F32, B, G, "ref_logprobs")
        lo, hi = self.token_window(window)
        out, idx, logits, n = self._action_logits(batch, True, "train_step_policy_gradient_group")
        lp, ratio, clipped, kl, ent, _ = ops.token_pg_group(logits[:n], tok, adv, window=(lo, hi), temperature=temperature, old_logprob=old, ref_logprob=ref,
                                                            kl_coef=kl_coef, ent_scale=entropy_coef * loss_scale / n, clip=clip, grad_scale=loss_scale / (n * G),
                                                            inplace_grad=True)
        logits[n:].zero_()
        dah = self.lm_loss_bwd(logits)
        if getattr(self, "_overlap", False) and self.head is not None and hasattr(self.head, "store"):   # (no head trains here: its gradients are final)
            for dt, g in self.head.store.flat_grad.items():
                self.reducer.notify(self.head.store, dt, g.numel())
        self.backward_from_rows(dah, idx, out)
        surr = torch.minimum(ratio * adv, ratio.clamp(float(clip[0]), float(clip[1])) * adv)
        kl_mean = kl.mean() if kl is not None else torch.zeros((), dtype=F32, device=self.device)
        ent_mean = ent.mean()
        return dict(loss=-surr.mean() + float(kl_coef) * kl_mean - float(entropy_coef) * ent_mean, logprob=lp.mean(), entropy=ent_mean,
                    clip_frac=clipped.to(F32).mean(), ratio=ratio.mean(), kl=kl_mean)

    # -- the frozen reference policy of the KL penalty: a snapshot of the trainables, swapped in for its log-probabilities ---------------------------
    _reference: Optional[list] = None     # per store: {dtype: a copy of the flat parameter buffer}
    _ref_scope = False

    @property
    def has_reference_policy(self) -> bool:
        return self._reference is not None

    @property
    def in_reference_scope(self) -> bool:
        return self._ref_scope

    def set_reference_policy(self):
        """Snapshots every store's flat parameter buffers, in their own dtype, as the reference policy ("the trainables as they are now").
        Replaces an earlier snapshot.  Checkpoints do not hold it: export_reference_policy / load_reference_policy save it like an adapter."""
        self._not_in_ema_scope("set_reference_policy")
        self._reference = [{dt: flat.clone() for dt, flat in st.flat.items()} for st in self.stores]

    def drop_reference_policy(self):
        self._not_in_ema_scope("drop_reference_policy")
        self._reference = None

    def reference_policy_bytes(self) -> int:
        return 0 if self._reference is None else sum(t.numel() * t.element_size() for snap in self._reference for t in snap.values())

    @contextlib.contextmanager
    def reference_policy(self):
        """Scope in which the flat buffers hold the reference snapshot (as ema_weights() holds the averaged weights): inference entry points see
        the reference policy with no change of their own.  On exit the live bits come back exactly; the derived copies are re-derived on both
        sides.  The fp32 master of fp32-optimizer-state mode is not touched.  Training entry points raise inside; it nests neither with itself
        nor with ema_weights()."""
        if self._reference is None:
            raise RuntimeError("reference_policy() without set_reference_policy() / load_reference_policy()")
        self._not_in_ema_scope("reference_policy")
        stash = [{dt: flat.clone() for dt, flat in st.flat.items()} for st in self.stores]
        for st, snap in zip(self.stores, self._reference):
            for dt, flat in st.flat.items():
                flat.copy_(snap[dt])
        self._ref_scope = True
        try:
            self.refresh_derived()
            yield self
        finally:
            for st, live in zip(self.stores, stash):
                for dt, flat in st.flat.items():
                    flat.copy_(live[dt])
            self._ref_scope = False
            self.refresh_derived()

    def reference_logprobs(self, batch: dict, tokens, temperature: float = 1.0, window="actions"):
        """policy_logprobs under the reference policy: the two swaps around one forward."""
        with self.reference_policy():
            return self.policy_logprobs(batch, tokens, temperature=temperature, window=window)

    def export_reference_policy(self) -> Dict[str, torch.Tensor]:
        """The reference snapshot in export_trainable("data")'s key layout, as copies (save it like an adapter)."""
        with self.reference_policy():
            return {k: v.detach().clone() for k, v in self.export_trainable("data").items()}

    def load_reference_policy(self, sd: Dict[str, torch.Tensor]):
        """Sets the reference policy from a state dict in export_trainable("data")'s key layout (every trainable tensor must be present).  The
        live parameters, their derived copies and the optimizer state keep their bits."""
        self._not_in_ema_scope("load_reference_policy")
        views = self.export_trainable("data")
        missing = [k for k in views if k not in sd]
        if missing:
            raise KeyError(f"{len(missing)} trainable tensors missing from the reference policy, e.g. {missing[:3]}")
        for name, view in views.items():
            if tuple(sd[name].shape) != tuple(view.shape):
                raise ValueError(f"{name}: reference shape {tuple(sd[name].shape)} != model shape {tuple(view.shape)}")
        stash = [{dt: flat.clone() for dt, flat in st.flat.items()} for st in self.stores]
        try:
            for name, view in views.items():
                view.copy_(sd[name].to(view.device, view.dtype))
            self._reference = [{dt: flat.clone() for dt, flat in st.flat.items()} for st in self.stores]
        finally:
            for st, live in zip(self.stores, stash):
                for dt, flat in st.flat.items():
                    flat.copy_(live[dt])

    # -- the Laplace policy on the L1 head (ovla.h "Laplace policy on the L1 head"): draws around the head's prediction, their log-probabilities,
    # -- and the group policy-gradient step on them ------------------------------------------------------------------------------------------
    def _l1_head(self, who: str, action_head=None):
        if self.head_kind != "l1" or (self.head is None and action_head is None):
            raise RuntimeError(f"{who} needs an engine built with head='l1' (the Laplace policy is the L1 head's; this one has head={self.head_kind!r})")
        return action_head if action_head is not None else self.head

    def _action_means(self, batch: dict, train: bool, head, proprio_projector=None, learned: bool = False, hidden: bool = False):
        """The forward on the action rows and the L1 head on them -> (out, rows_idx, pred bf16 [B * chunk, action_dim], the head's saved state);
        with `learned` also (h2, log_scale): the head's post-layer_norm2 activations and the scale head's output bf16 [B * chunk, action_dim];
        with `hidden` (and not `learned`) also h2 -- the same launches, one more view."""
        kw = {} if proprio_projector is None else dict(proprio_projector=proprio_projector)
        out = self.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"),
                           train=train, sel="actions", **kw)
        ah, idx = self.action_hidden(out)
        if not learned and not hidden:
            pred, _, hsaved = head.fwd(ah, train=train)
            return out, idx, pred, hsaved
        pred, _, hsaved, h2 = head.fwd(ah, train=train, return_hidden=True)
        if not learned:
            return out, idx, pred, hsaved, h2
        return out, idx, pred, hsaved, h2, self.scale_head.fwd(h2)

    def _chunk_rows(self, t, dtype, B: int, G: int, what: str, per_draw: bool = False, per_dim: bool = False):
        """A per-step [B, G, chunk] (with `per_draw` also per-draw [B, G]; with `per_dim` [B, G, chunk, action_dim]) host or device tensor ->
        contiguous [B * chunk, G (, action_dim)] on the device: the Laplace kernels' layout, one row of G samples per chunk step."""
        C, Ad = self.cfg.chunk, self.cfg.action_dim
        t = torch.as_tensor(t).to(self.device, dtype)
        if per_draw and tuple(t.shape) == (B, G):
            t = t.reshape(B, G, 1).expand(B, G, C)
        want = (B, G, C, Ad) if per_dim else (B, G, C)
        if tuple(t.shape) != want:
            raise ValueError(f"{what}: {tuple(t.shape)} for {B} observations of {G} draws of {C} steps" + (f" of {Ad} dimensions" if per_dim else ""))
        if per_dim:
            return t.permute(0, 2, 1, 3).reshape(B * C, G, Ad).contiguous()
        return t.permute(0, 2, 1).reshape(B * C, G).contiguous()

    def _chunk_out(self, t, B: int, G: int):
        """[B * chunk, G (, action_dim)] kernel output -> [B, G, chunk (, action_dim)]."""
        C = self.cfg.chunk
        if t.dim() == 3:
            return t.view(B, C, G, t.shape[2]).permute(0, 2, 1, 3).contiguous()
        return t.view(B, C, G).permute(0, 2, 1).contiguous()

    def sample_actions_laplace(self, batch: dict, scale, num_samples: int = 1, row_keys=None, return_value: bool = False):
        """Draws G = num_samples chunks per observation from the Laplace policy of scale `scale` (a scalar or one value per action dimension,
        in normalised action units) around the L1 head's prediction: one forward (inference mode) on the action rows, the head, ONE
        ovla_laplace_sample launch; nothing is read back.  Advances the token stream's `call` by one.  `row_keys` int32 [B, G] (observation draw
        key k gives its step c the generator key k * chunk + c; default b * G + g) or [B, G, chunk]: a draw does not depend on its position.
        -> dict(actions fp32 [B, G, chunk, action_dim], logprob fp32 [B, G, chunk], mean bf16 [B, chunk, action_dim]) on the device.
        scale="learned" (attach_scale_head): the widths are the scale head's, per chunk step and dimension -- the head with its hidden output,
        the scale head, ONE ovla_laplace_sample_rows launch; the dict gains log_scale bf16 [B, chunk, action_dim] (the raw, unclamped output) and
        entropy fp32 [B, chunk].
        return_value=True (attach_value_head): the dict gains value fp32 [B], the critic's value of each observation from the SAME forward
        (action_values' bits: two launches after the draw); the draws keep their bits.  Without it every launch is the one issued before."""
        head = self._l1_head("sample_actions_laplace")
        learned = self._learned(scale, "sample_actions_laplace")
        cfg, B, G = self.cfg, batch["input_ids"].shape[0], int(num_samples)
        C = cfg.chunk
        if not 1 <= G <= ops.PG_GROUP_MAX:
            raise ValueError(f"num_samples = {G} (1 .. {ops.PG_GROUP_MAX})")
        if not learned:
            ops.laplace_scales(scale, cfg.action_dim)            # (raises before anything advances)
        keys = torch.arange(B * G, dtype=torch.int32, device=self.device).view(B, G) if row_keys is None else torch.as_tensor(row_keys).to(self.device, torch.int32)
        if tuple(keys.shape) == (B, G):
            keys = keys.reshape(B, G, 1) * C + torch.arange(C, dtype=torch.int32, device=self.device)[None, None, :]
        keys = self._chunk_rows(keys, torch.int32, B, G, "row_keys")
        if return_value:
            self._critic("sample_actions_laplace(return_value=True)")
        with torch.no_grad():
            st = self.token_sample
            if learned:
                _, _, pred, _, h2, ls = self._action_means(batch, False, head, learned=True)
                act, lp, ent = ops.laplace_sample_rows(pred, ls, self.scale_bounds, G, seed=st.seed, call=st.advance(), row_key=keys)
                res = dict(actions=self._chunk_out(act, B, G), logprob=self._chunk_out(lp, B, G), mean=pred.view(B, C, cfg.action_dim),
                           log_scale=ls.view(B, C, cfg.action_dim), entropy=ent.view(B, C))
            else:
                h2 = None
                if return_value:
                    _, _, pred, _, h2 = self._action_means(batch, False, head, hidden=True)
                else:
                    _, _, pred, _ = self._action_means(batch, False, head)
                act, lp = ops.laplace_sample(pred, scale, G, seed=st.seed, call=st.advance(), row_key=keys)
                res = dict(actions=self._chunk_out(act, B, G), logprob=self._chunk_out(lp, B, G), mean=pred.view(B, C, cfg.action_dim))
            if return_value:
                res["value"] = self._values_of(h2)
        return res

    def _values_of(self, h2) -> torch.Tensor:
        """The value head on h2 [B * chunk, D] and the pooling launch (ovla_value_loss without returns) -> fp32 [B]."""
        return ops.value_loss(self.value_head.fwd(h2), self.cfg.chunk)

    def action_values(self, batch: dict) -> torch.Tensor:
        """The critic's value of every observation, fp32 [B] on the device: the inference forward on the action rows, the head with its hidden
        output, the value head, ovla_value_loss without returns (the mean of the chunk's per-step outputs).  Nothing is read back."""
        head = self._l1_head("action_values")
        self._critic("action_values")
        with torch.no_grad():
            _, _, _, _, h2 = self._action_means(batch, False, head, hidden=True)
            return self._values_of(h2)

    def _value_targets(self, B: int, returns, old_values, value_clip: float):
        """returns / old_values (host or device, B elements each) -> fp32 [B] device tensors (old: None without clipping); raises before any launch."""
        def per_obs(t, what):
            t = torch.as_tensor(t).to(self.device, F32)
            if t.numel() != B:
                raise ValueError(f"{what}: {tuple(t.shape)} for {B} observations")
            return t.reshape(B).contiguous()

        if not value_clip >= 0.0:
            raise ValueError(f"value_clip = {value_clip} (must not be negative or NaN; 0: no clipping)")
        if value_clip > 0.0 and old_values is None:
            raise ValueError("value_clip > 0 needs old_values (the values the rollout recorded)")
        return per_obs(returns, "returns"), (per_obs(old_values, "old_values") if value_clip > 0.0 else None)

    def _value_step(self, h2, targets, value_clip: float, grad_scale: float) -> Dict[str, torch.Tensor]:
        """The critic's side step on the step's own h2: the value head's forward, ONE ovla_value_loss launch, the value head's backward into its
        own store (three launches; nothing else is written, nothing is read back).  `targets`: _value_targets' pair.
        -> dict(value_loss, value_clip_frac, explained_variance device scalars, value fp32 [B])."""
        vh = self.value_head
        returns, old = targets
        value, du, s = ops.value_loss(vh.fwd(h2), self.cfg.chunk, returns=returns, old_value=old, value_clip=value_clip, grad_scale=grad_scale)
        vh.bwd(h2, du)
        if getattr(self, "_overlap", False):
            for dt, g in vh.store.flat_grad.items():
                self.reducer.notify(vh.store, dt, g.numel())
        return dict(value_loss=s[2] / s[0], value_clip_frac=s[1] / s[0], explained_variance=1.0 - s[5] / (s[6] - s[4] * s[4] / s[0]), value=value)

    def train_step_value(self, batch: dict, returns, old_values=None, value_clip: float = 0.0, loss_scale: float = 1.0):
        """The critic alone on a FROZEN policy (as train_step_scale_nll fits the scale): the inference-mode forward on the action rows, the head
        with its hidden output, then the three launches of the value step with grad_scale = loss_scale / B:
            loss = (1 / B) sum_b 0.5 max((v_b - R_b)^2, (clip(v_b; old_b +- value_clip) - R_b)^2)
        No decoder backward, no LoRA, head or scale-head gradient is touched, nothing is read back.  `returns` [B], `old_values` [B] (with
        value_clip > 0).  -> dict(value_loss, value_clip_frac, explained_variance, value)."""
        self._not_in_ema_scope("train_step_value")
        head = self._l1_head("train_step_value")
        self._critic("train_step_value")
        B = batch["input_ids"].shape[0]
        targets = self._value_targets(B, returns, old_values, float(value_clip))
        with torch.no_grad():
            _, _, _, _, h2 = self._action_means(batch, False, head, hidden=True)
            return self._value_step(h2, targets, float(value_clip), loss_scale / B)

    def action_logprobs(self, batch: dict, actions, scale):
        """Log-probability of given chunks [B, G, chunk, action_dim] under the Laplace policy around the current weights' prediction: the
        forward of sample_actions_laplace, then ovla_laplace_pg without a gradient -- for the chunks a draw returned, the bits that draw
        reported.  -> dict(logprob fp32 [B, G, chunk], mean bf16 [B, chunk, action_dim]).  scale="learned": ovla_laplace_pg_rows at the scale head's
        widths; the dict gains log_scale bf16 [B, chunk, action_dim] and entropy fp32 [B, chunk]."""
        head = self._l1_head("action_logprobs")
        learned = self._learned(scale, "action_logprobs")
        cfg, B = self.cfg, batch["input_ids"].shape[0]
        actions = torch.as_tensor(actions)
        if actions.dim() != 4:
            raise ValueError(f"actions: {tuple(actions.shape)} ([B, G, chunk, action_dim])")
        G = actions.shape[1]
        act = self._chunk_rows(actions, F32, B, G, "actions", per_dim=True)
        with torch.no_grad():
            if learned:
                _, _, pred, _, _, ls = self._action_means(batch, False, head, learned=True)
                lp, _, _, _, ent, _, _ = ops.laplace_pg_rows(pred, ls, self.scale_bounds, act, torch.ones((pred.shape[0], G), dtype=F32, device=self.device))
                return dict(logprob=self._chunk_out(lp, B, G), mean=pred.view(B, cfg.chunk, cfg.action_dim), log_scale=ls.view(B, cfg.chunk, cfg.action_dim),
                            entropy=ent.view(B, cfg.chunk))
            _, _, pred, _ = self._action_means(batch, False, head)
            lp, _, _, _, _ = ops.laplace_pg(pred, act, torch.ones((pred.shape[0], G), dtype=F32, device=self.device), scale)
        return dict(logprob=self._chunk_out(lp, B, G), mean=pred.view(B, cfg.chunk, cfg.action_dim))

    def reference_action_means(self, batch: dict) -> torch.Tensor:
        """The L1 head's prediction under the reference policy, bf16 [B, chunk, action_dim]: train_step_action_pg_group's `ref_means` (the two swaps
        around one forward)."""
        head = self._l1_head("reference_action_means")
        with self.reference_policy():
            with torch.no_grad():
                _, _, pred, _ = self._action_means(batch, False, head)
        return pred.view(batch["input_ids"].shape[0], self.cfg.chunk, self.cfg.action_dim)

    def reference_action_policy(self, batch: dict) -> Dict[str, torch.Tensor]:
        """Mean and log-scale under the reference policy (the scale head's store is snapshotted with the others), dict(mean, log_scale) bf16
        [B, chunk, action_dim]: train_step_action_pg_group(scale="learned")'s `ref_means` / `ref_log_scales`."""
        head = self._l1_head("reference_action_policy")
        self._learned("learned", "reference_action_policy")
        with self.reference_policy():
            with torch.no_grad():
                _, _, pred, _, _, ls = self._action_means(batch, False, head, learned=True)
        shape = (batch["input_ids"].shape[0], self.cfg.chunk, self.cfg.action_dim)
        return dict(mean=pred.view(shape), log_scale=ls.view(shape))

    def _scale_bwd(self, h2, dlog_scale):
        """The scale head's backward into its own store (and the reducer's notification, as for the head's)."""
        sh = self.scale_head
        sh.bwd(h2, dlog_scale)
        if getattr(self, "_overlap", False):
            for dt, g in sh.store.flat_grad.items():
                self.reducer.notify(sh.store, dt, g.numel())

    def _nll_of_target(self, pred, h2, target, loss_scale: float = 1.0):
        """The maximum-likelihood side step of the scale head on a target chunk bf16 [rows, action_dim]: the scale head on h2, ovla_laplace_pg_rows
        at G = 1 (adv = 1, no ratio, no reference, no entropy bonus, no dpred) with grad_scale = loss_scale / rows, the scale head's backward.  Three
        launches; nothing but the scale head's store is written.  -> dict(nll, scale) device scalars: the mean negative log-likelihood per chunk
        step and the mean b."""
        n = pred.shape[0]
        ls = self.scale_head.fwd(h2)
        lp, _, _, _, _, _, dls = ops.laplace_pg_rows(pred, ls, self.scale_bounds, target.float().view(n, 1, -1), torch.ones((n, 1), dtype=F32, device=self.device),
                                                     grad_scale=loss_scale / n, want_dpred=False)
        self._scale_bwd(h2, dls)
        return dict(nll=-lp.mean(), scale=ls.float().clamp(*self.scale_bounds).exp().mean())

    def train_step_scale_nll(self, batch: dict, loss_scale: float = 1.0):
        """The post-hoc maximum-likelihood fit of the scale head on a FROZEN policy: the inference-mode forward on the action rows, the head with
        its hidden output, then the three launches of the side step on the batch's bf16 target chunk.  No decoder backward, no LoRA or head
        gradient is touched, nothing is read back.  -> dict(nll, scale) device scalars."""
        self._not_in_ema_scope("train_step_scale_nll")
        head = self._l1_head("train_step_scale_nll")
        self._learned("learned", "train_step_scale_nll")
        cfg = self.cfg
        target = batch["actions"].to(self.device, BF16).reshape(batch["input_ids"].shape[0] * cfg.chunk, cfg.action_dim).contiguous()
        with torch.no_grad():
            out = self.forward(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], proprio=batch.get("proprio"),
                               train=False, sel="actions")
            ah, _ = self.action_hidden(out)
            pred, _, _, h2 = head.fwd(ah, return_hidden=True)
            return self._nll_of_target(pred, h2, target, loss_scale)

    def train_step_action_pg_group(self, batch: dict, actions, advantages, scale, old_logprobs=None, ref_means=None, kl_coef: float = 0.0, clip=(0.8, 1.2),
                                   loss_scale: float = 1.0, action_head=None, proprio_projector=None, entropy_coef: float = 0.0, ref_log_scales=None,
                                   returns=None, old_values=None, value_coef: float = 0.5, value_clip: float = 0.0):
        """One GRPO / PPO micro-step on G drawn chunks per observation under the Laplace policy of the L1 head, from ONE forward and ONE backward:
            loss = (1 / (B chunk G)) sum_{b, g, c} -min(ratio A_bg, clip(ratio) A_bg)  +  kl_coef (1 / (B chunk)) sum_{b, c} kl
        with ratio = exp(logprob - old_logprob) per chunk step (1 without old_logprobs) and kl the closed-form KL(policy || reference) of two
        Laplace distributions of the same scale, summed over the action dimensions.  The forward does not depend on the draws: the training
        forward on the action rows, the head, one ovla_laplace_pg launch that forms the gradient with respect to the head's prediction, then the
        head's and the decoder's backward into the flat gradient buffers.  `actions` fp32 [B, G, chunk, action_dim] (RAW draws, normalised units);
        `advantages` [B, G] or [B, G, chunk]; `old_logprobs` [B, G, chunk] (sample_actions_laplace / action_logprobs); `ref_means`
        [B, chunk, action_dim] (reference_action_means), required with kl_coef > 0; host or device tensors.
        -> dict of device scalars: loss, logprob, ratio, clip_frac, kl (means; kl is 0 without ref_means).
        scale="learned" (attach_scale_head): the scale head runs on the head's hidden output, ONE ovla_laplace_pg_rows launch takes the place of
        ovla_laplace_pg and also forms the gradient with respect to the log-scale, the scale head's backward follows it (two launches more), and
        the mean's path -- the head's backward, the reducer's notification, the decoder's backward -- is unchanged: the scale's gradient stops at
        the head's hidden output.  The KL is between Laplace distributions of different scale (`ref_log_scales` [B, chunk, action_dim] beside
        `ref_means`: reference_action_policy), and the loss gains - entropy_coef (1 / (B chunk)) sum_{b, c} entropy, the bonus that keeps the scale
        from collapsing.  The statistics gain entropy (mean per chunk step) and scale (mean b).  entropy_coef and ref_log_scales belong to the
        learned scale alone (ValueError with a numeric one).
        `returns` [B] (attach_value_head): the PPO step.  The loss gains value_coef (1 / B) sum_b 0.5 max((v_b - R_b)^2, (clip(v_b; old_b +-
        value_clip) - R_b)^2) with v_b the critic's value of observation b (`old_values` [B] with value_clip > 0): the value head's forward on
        the step's own hidden output, ONE ovla_value_loss launch with grad_scale = loss_scale value_coef / B, the value head's backward -- three
        launches into the value head's store alone, its gradient stops at the hidden output, so every other accumulator keeps the bits of the
        same step without `returns`.  The statistics gain value_loss, value_clip_frac, explained_variance (device scalars) and value fp32 [B];
        `loss` stays the policy's.  Without `returns` the step issues exactly the launches it issued before, with or without a value head."""
        self._not_in_ema_scope("train_step_action_pg_group")
        self._refuse_per_policy_film_training(True)
        head = self._l1_head("train_step_action_pg_group", action_head)
        learned = self._learned(scale, "train_step_action_pg_group")
        if not learned and (entropy_coef != 0.0 or ref_log_scales is not None):
            raise ValueError('entropy_coef and ref_log_scales belong to scale="learned"')
        if learned and (ref_means is None) != (ref_log_scales is None):
            raise ValueError('scale="learned": ref_means and ref_log_scales come together (reference_action_policy)')
        cfg, B = self.cfg, batch["input_ids"].shape[0]
        actions = torch.as_tensor(actions)
        if actions.dim() != 4:
            raise ValueError(f"actions: {tuple(actions.shape)} ([B, G, chunk, action_dim])")
        G = actions.shape[1]
        act = self._chunk_rows(actions, F32, B, G, "actions", per_dim=True)
        adv = self._chunk_rows(advantages, F32, B, G, "advantages", per_draw=True)
        old = None if old_logprobs is None else self._chunk_rows(old_logprobs, F32, B, G, "old_logprobs")
        ref = None
        if ref_means is not None:
            ref = torch.as_tensor(ref_means).to(self.device, BF16)
            if ref.numel() != B * cfg.chunk * cfg.action_dim:
                raise ValueError(f"ref_means: {tuple(ref.shape)} for {B} observations of {cfg.chunk} steps of {cfg.action_dim} dimensions")
            ref = ref.reshape(B * cfg.chunk, cfg.action_dim).contiguous()
        elif kl_coef > 0.0:
            raise ValueError("kl_coef > 0 needs ref_means (reference_action_means)")
        ref_ls = None
        if ref_log_scales is not None:
            ref_ls = torch.as_tensor(ref_log_scales).to(self.device, BF16)
            if ref_ls.numel() != B * cfg.chunk * cfg.action_dim:
                raise ValueError(f"ref_log_scales: {tuple(ref_ls.shape)} for {B} observations of {cfg.chunk} steps of {cfg.action_dim} dimensions")
            ref_ls = ref_ls.reshape(B * cfg.chunk, cfg.action_dim).contiguous()
        critic = returns is not None
        if critic:
            self._critic("train_step_action_pg_group(returns=...)")
            targets = self._value_targets(batch["input_ids"].shape[0], returns, old_values, float(value_clip))
        elif old_values is not None or value_clip != 0.0:
            raise ValueError("old_values and value_clip belong to the value loss: they need returns")
        extra = {}
        if learned:
            out, idx, pred, hsaved, h2, ls = self._action_means(batch, True, head, proprio_projector, learned=True)
            n = pred.shape[0]
            lp, ratio, clipped, kl, ent, dpred, dls = ops.laplace_pg_rows(pred, ls, self.scale_bounds, act, adv, old_logprob=old, ref_pred=ref, ref_log_scale=ref_ls,
                                                                          kl_coef=kl_coef, clip=clip, grad_scale=loss_scale / (n * G), kl_scale=loss_scale / n,
                                                                          entropy_coef=entropy_coef, ent_scale=loss_scale / n)
            self._scale_bwd(h2, dls)
            extra = dict(entropy=ent.mean(), scale=ls.float().clamp(*self.scale_bounds).exp().mean())
        else:
            ops.laplace_scales(scale, cfg.action_dim)
            if critic:
                out, idx, pred, hsaved, h2 = self._action_means(batch, True, head, proprio_projector, hidden=True)
            else:
                out, idx, pred, hsaved = self._action_means(batch, True, head, proprio_projector)
            n = pred.shape[0]
            lp, ratio, clipped, kl, dpred = ops.laplace_pg(pred, act, adv, scale, old_logprob=old, ref_pred=ref, kl_coef=kl_coef, clip=clip,
                                                           grad_scale=loss_scale / (n * G), kl_scale=loss_scale / n)
        if critic:
            with torch.no_grad():
                extra.update(self._value_step(h2, targets, float(value_clip), loss_scale * float(value_coef) / B))
        dah = head.bwd(hsaved, dpred=dpred)
        if getattr(self, "_overlap", False) and hasattr(head, "store"):
            for dt, g in head.store.flat_grad.items():
                self.reducer.notify(head.store, dt, g.numel())
        self.backward_from_rows(dah, idx, out)
        surr = torch.minimum(ratio * adv, ratio.clamp(float(clip[0]), float(clip[1])) * adv)
        kl_mean = kl.mean() if kl is not None else torch.zeros((), dtype=F32, device=self.device)
        loss = -surr.mean() + float(kl_coef) * kl_mean
        if learned:
            loss = loss - float(entropy_coef) * extra["entropy"]
        return dict(loss=loss, logprob=lp.mean(), ratio=ratio.mean(), clip_frac=clipped.to(F32).mean(), kl=kl_mean, **extra)

    # -- preference optimisation on the Laplace policy: a chosen and a rejected chunk per observation (ovla.h: ovla_laplace_dpo) -----------------
    def _preference_inputs(self, who: str, B: int, chosen, rejected, scale, beta, ref_means, ref_log_scales, weights, label_smoothing, loss_type, nll_coef):
        """Validates and lays out what both preference entry points hand the launch; raises before any launch.
        -> (learned, dict of ops.laplace_dpo's keyword arguments, weights fp32 [B] or None)."""
        learned = self._learned(scale, who)
        cfg = self.cfg
        C, Ad = cfg.chunk, cfg.action_dim
        if not learned and ref_log_scales is not None:
            raise ValueError('ref_log_scales belongs to scale="learned"')
        if ref_means is None:
            raise ValueError(f"{who} needs ref_means (reference_action_means): a preference is a log-ratio to a reference policy")
        if learned and ref_log_scales is None:
            raise ValueError('scale="learned": ref_means and ref_log_scales come together (reference_action_policy)')
        if C > ops.DPO_CHUNK_MAX:
            raise ValueError(f"{who}: chunk = {C} (at most {ops.DPO_CHUNK_MAX} steps per observation)")
        if loss_type not in ops.DPO_LOSS_TYPES:
            raise ValueError(f"loss_type = {loss_type!r} (one of {sorted(ops.DPO_LOSS_TYPES)})")
        if not (beta >= 0.0 and math.isfinite(beta)) or (loss_type == "ipo" and beta == 0.0):
            raise ValueError(f"beta = {beta} (finite and not negative; positive for the IPO loss)")
        if not 0.0 <= label_smoothing < 0.5:
            raise ValueError(f"label_smoothing = {label_smoothing} (in [0, 0.5))")
        if not nll_coef >= 0.0:
            raise ValueError(f"nll_coef = {nll_coef} (must not be negative or NaN)")

        def rows_of(t, dtype, what):
            t = torch.as_tensor(t).to(self.device, dtype)
            if tuple(t.shape) not in ((B, C, Ad), (B * C, Ad)):
                raise ValueError(f"{what}: {tuple(t.shape)} for {B} observations of {C} steps of {Ad} dimensions")
            return t.reshape(B * C, Ad).contiguous()

        kw = dict(ref_pred=rows_of(ref_means, BF16, "ref_means"), chosen=rows_of(chosen, F32, "chosen"), rejected=rows_of(rejected, F32, "rejected"))
        if learned:
            kw.update(ref_log_scale=rows_of(ref_log_scales, BF16, "ref_log_scales"), bounds=self.scale_bounds)
        else:
            ops.laplace_scales(scale, Ad)
            kw.update(scale=scale)
        w = None
        if weights is not None:
            w = torch.as_tensor(weights).to(self.device, F32)
            if w.numel() != B:
                raise ValueError(f"weights: {tuple(w.shape)} for {B} observations")
            w = w.reshape(B).contiguous()
        kw.update(weight=w, beta=float(beta), label_smoothing=float(label_smoothing), loss_type=loss_type, nll_coef=float(nll_coef))
        return learned, kw, w

    def _preference_stats(self, r: dict, w, beta: float, B: int) -> Dict[str, torch.Tensor]:
        """The launch's per-observation outputs -> device scalars, weighted means over the observations with w > 0 (a skipped observation's
        outputs are +0 and its weight is 0), and coef fp32 [B].  Nothing is read back."""
        C = self.cfg.chunk
        w = torch.ones(B, dtype=F32, device=self.device) if w is None else w
        mean = lambda t: (w * t).sum() / w.sum()   # noqa: E731
        lp = r["logprob"].view(B, C, 2).mean(1)
        return dict(loss=mean(r["loss"]), margin=mean(r["margin"]), reward_chosen=float(beta) * mean(r["h"][:, 0]), reward_rejected=float(beta) * mean(r["h"][:, 1]),
                    accuracy=mean((r["margin"] > 0).to(F32)), logprob_chosen=mean(lp[:, 0]), logprob_rejected=mean(lp[:, 1]), coef=r["coef"])

    def train_step_action_dpo(self, batch: dict, chosen, rejected, scale, *, beta: float, ref_means, ref_log_scales=None, weights=None, label_smoothing: float = 0.0,
                              loss_type: str = "sigmoid", nll_coef: float = 0.0, loss_scale: float = 1.0, action_head=None, proprio_projector=None):
        """One direct-preference-optimisation micro-step under the Laplace policy of the L1 head, from ONE forward and ONE backward:
            loss = (1 / B) sum_b w_b l(beta m_b)  +  nll_coef (1 / (B chunk)) sum_{b, c} w_b (-logprob of the chosen chunk's step c)
        with m_b the margin between the chosen and the rejected chunk's log-ratio to the reference policy, summed over the chunk's steps, and
        l(z) = (1 - eps) softplus(-z) + eps softplus(z) (loss_type "sigmoid", eps = label_smoothing) or (m - 1 / (2 beta))^2 ("ipo").  The body is
        train_step_action_pg_group's with one ovla_laplace_dpo launch in place of ovla_laplace_pg(_rows): the training forward on the action
        rows, the head (and the scale head under scale="learned"), that launch -- it reduces the margin, turns it into the pair's implied
        advantages and forms the gradient with respect to the prediction (and the log-scale) -- the scale head's backward when learned, the
        head's and the decoder's backward into the flat gradient buffers.  `chosen`, `rejected` [B, chunk, action_dim]: RAW chunks in normalised
        units; `ref_means` [B, chunk, action_dim] (reference_action_means; computed once per dataset if the caller likes), with `ref_log_scales`
        under scale="learned" (reference_action_policy); `weights` [B] >= 0, an observation of weight 0 is skipped and may hold anything; host
        or device tensors.
        -> dict of device scalars, weighted means over the observations with w > 0: loss (the preference term), margin, reward_chosen
        (beta times the chosen chunk's log-ratio), reward_rejected, accuracy (the share with m > 0), logprob_chosen, logprob_rejected (per chunk
        step); and coef fp32 [B], the implied advantage of each pair as the launch applied it.  Nothing is read back."""
        self._not_in_ema_scope("train_step_action_dpo")
        self._refuse_per_policy_film_training(True)
        head = self._l1_head("train_step_action_dpo", action_head)
        B, C = batch["input_ids"].shape[0], self.cfg.chunk
        learned, kw, w = self._preference_inputs("train_step_action_dpo", B, chosen, rejected, scale, beta, ref_means, ref_log_scales, weights, label_smoothing,
                                                 loss_type, nll_coef)
        kw.update(grad_scale=loss_scale / B, nll_scale=loss_scale / (B * C))
        if learned:
            out, idx, pred, hsaved, h2, ls = self._action_means(batch, True, head, proprio_projector, learned=True)
            r = ops.laplace_dpo(pred, chunk=C, log_scale=ls, **kw)
            self._scale_bwd(h2, r["dlog_scale"])
        else:
            out, idx, pred, hsaved = self._action_means(batch, True, head, proprio_projector)
            r = ops.laplace_dpo(pred, chunk=C, **kw)
        dah = head.bwd(hsaved, dpred=r["dpred"])
        if getattr(self, "_overlap", False) and hasattr(head, "store"):
            for dt, g in head.store.flat_grad.items():
                self.reducer.notify(head.store, dt, g.numel())
        self.backward_from_rows(dah, idx, out)
        return self._preference_stats(r, w, beta, B)

    def action_preference(self, batch: dict, chosen, rejected, scale, *, beta: float, ref_means, ref_log_scales=None, weights=None, label_smoothing: float = 0.0,
                          loss_type: str = "sigmoid", action_head=None):
        """train_step_action_dpo's launch without gradients, on the inference forward: margin and accuracy of held-out pairs under the current
        weights.  Same arguments, same statistics (and coef at grad_scale 1 / B); nothing is written but the outputs, nothing is read back."""
        head = self._l1_head("action_preference", action_head)
        B, C = batch["input_ids"].shape[0], self.cfg.chunk
        learned, kw, w = self._preference_inputs("action_preference", B, chosen, rejected, scale, beta, ref_means, ref_log_scales, weights, label_smoothing,
                                                 loss_type, 0.0)
        kw.update(grad_scale=1.0 / B, want_dpred=False, want_dlog_scale=False)
        with torch.no_grad():
            if learned:
                _, _, pred, _, _, ls = self._action_means(batch, False, head, learned=True)
                r = ops.laplace_dpo(pred, chunk=C, log_scale=ls, **kw)
            else:
                _, _, pred, _ = self._action_means(batch, False, head)
                r = ops.laplace_dpo(pred, chunk=C, **kw)
        return self._preference_stats(r, w, beta, B)

    # -- the next-token cross entropy on the counted rows: train_step_discrete above and modeling._LMLossFn (`output.loss`) ------------------
    def counted_rows(self, labels, S: int, P: int):
        """Host int64 labels [B, L] -> (bb, jj, rows_idx int32 [n_tok] device, targets int64 [n_tok] device).  Text position j + 1 with
        labels[b, j + 1] != -100 is predicted by the hidden state of text position j, which sits at multimodal row b * S + P + j (the BOS row
        is 0, the patches are rows 1..P; modeling_prismatic.py:474-496)."""
        bb, jj = torch.nonzero(labels[:, 1:] != -100, as_tuple=True)
        if bb.numel() == 0:
            raise ValueError("no label in the batch is different from IGNORE_INDEX")
        return bb, jj, (bb * S + P + jj).to(torch.int32).to(self.device), labels[bb, jj + 1].contiguous().to(self.device)

    def lm_loss_fwd(self, out, rows_idx, targets, grad_scale: Optional[float]):
        """Frozen lm_head (bf16, as under autocast) + ovla_token_ce on the rows `rows_idx` of the forward result `out` -> (loss per row fp32
        [n_tok], argmax [n_tok], logits bf16 [n_tok padded to 8, vocab]).  With a `grad_scale` the logits come back overwritten by
        grad_scale * d loss_rows / d logits, pad rows zero: lm_loss_bwd's argument."""
        n_tok, D = rows_idx.numel(), self.cfg.llm_dim
        if out["sel_rows"] is not None:
            x = out["action_hidden"]                       # n_tok % 8 == 0 and the last layer ran on these rows: already gathered
        else:
            x = torch.zeros(((n_tok + 7) // 8 * 8, D), dtype=BF16, device=self.device)
            ops.gather_rows(out["hidden"].detach().view(-1, D), rows_idx, D, dst=x)
        logits = ops.gemm(x, self.lm_head)
        loss_rows, amax, _ = ops.token_ce(logits[:n_tok], targets, grad_scale=grad_scale)
        if grad_scale is not None:
            logits[n_tok:].zero_()
        return loss_rows, amax, logits

    def lm_loss_bwd(self, dlogits, alpha: float = 1.0):
        """alpha * dlogits @ W_lm_head -> gradient of the hidden rows lm_loss_fwd read, bf16 [rows, D]."""
        if self._lm_head_t is None:
            self._lm_head_t = ops.transpose(self.lm_head)                    # frozen: one transposed copy for the data gradient
        return ops.gemm(dlogits, self._lm_head_t, alpha=alpha)


# ======================================================================================================================
# what the two inference graphs below share
# ======================================================================================================================
class _StaticInputs:
    """What ChunkGraph and DiffusionGraph share: the static device buffers that load() fills before a replay (ids / labels / text lengths /
    pixels / proprio), the ragged FiLM average at the head of a captured forward, and the rule for a capture (one eager warm-up, then the
    capture with a workspace cache of its own)."""

    def __init__(self, engine: "VLAEngine", B: int, L: int, pixel_shape, use_proprio: bool, invariant: bool, film: bool):
        if film and not engine.use_film:
            raise ValueError(f"{type(self).__name__}(film=True) needs an engine built with use_film=True")
        dev = engine.device
        self.engine, self.B, self.L = engine, B, L
        self.invariant = invariant   # capture every GEMM under its fixed schedule (ops.batch_invariant): the batched inference API
        self.film = film
        self.ids = torch.zeros((B, L), dtype=torch.int64, device=dev)
        self.lab = torch.full((B, L), -100, dtype=torch.int64, device=dev)
        self.lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        self.pixels = torch.zeros(tuple(pixel_shape), dtype=BF16, device=dev)
        self.proprio = torch.zeros((B, engine.cfg.proprio_dim), dtype=BF16, device=dev) if use_proprio else None

    def load(self, input_ids, attention_mask, pixel_values, labels, proprio=None):
        lens = VLAEngine.check_right_padding(attention_mask)
        assert tuple(input_ids.shape) == (self.B, self.L), f"{type(self).__name__} captured for ids {(self.B, self.L)}, got {tuple(input_ids.shape)}"
        self.ids.copy_(input_ids.to(torch.int64), non_blocking=True)
        self.lab.copy_(labels.to(torch.int64), non_blocking=True)
        self.lens.copy_(lens.to(torch.int32), non_blocking=True)
        self.pixels.copy_(pixel_values.reshape(self.pixels.shape), non_blocking=True)
        if self.proprio is not None:
            self.proprio.copy_(proprio.reshape(self.proprio.shape), non_blocking=True)

    def _film_average(self):
        """film=True: the conditioning vectors of the static ids / labels / lengths, one ragged launch; otherwise None (the engine's own rule)."""
        if not self.film:
            return None
        eng = self.engine
        film_avg = torch.zeros(((self.B + 7) // 8 * 8, eng.cfg.llm_dim), dtype=BF16, device=eng.device)
        return ops.language_average_ragged(self.ids, self.lab, self.lens, eng.embed, film_avg)

    @contextlib.contextmanager
    def _capturing(self, warm_up):
        """Call after load() of a representative input.  Runs `warm_up` eagerly once (lazy tables, kernel attributes); inside, the captures."""
        assert ops.PROFILE is None, "no per-launch event timing inside a graph capture"
        warm_up()
        torch.cuda.synchronize(self.engine.device)
        outer_ws, ops._ws_cache = ops._ws_cache, {}          # workspaces allocated while capturing belong to the graphs' pools
        try:
            yield
        finally:
            self._ws, ops._ws_cache = ops._ws_cache, outer_ws


# ======================================================================================================================
# hipGraph replay of the single-chunk inference forward (BASELINE.json configs[1])
# ======================================================================================================================
class ChunkGraph(_StaticInputs):
    """The batch-B inference forward (vision towers on their two streams -> projector -> assembly -> Llama stack -> action
    row gather -> optional L1 head) captured ONCE as a hipGraph and replayed per observation: ~1.3 k kernel launches become
    one graph launch, which is what bounds batch-1 latency.  Inputs are copied into static device buffers before each
    replay; outputs are static buffers too (clone them to keep a result across calls).

    Everything the capture allocates (activations, split-K workspaces) lives in the graph's private pool and stays valid as
    long as this object does.  Text length L is part of the captured shapes: callers pad the prompt to a bucket (right
    padding is masked exactly: padded keys contribute exact zeros) or keep one ChunkGraph per L.

    `film=True` (a FiLM engine, right-padded batch): the conditioning vectors come from ONE ragged launch over the static ids / labels / lengths
    (ovla_language_average_ragged: row b averages its own lens[b] tokens, pad tokens never enter), inside the graph.  Without it a FiLM engine
    averages over all L positions, which is the reference's rule for an unpadded prompt (predict_action).
    `discrete=True` (no action head, engine.lm_head present): the graph goes on to the lm_head GEMM on the action rows and the greedy decode
    (ovla_argmax_bins); replay() then returns (None, action hidden, token int32 [B*A], bin int32 [B*A]).
    `policies` (multi-policy serving, an engine with adapter slots): [(L1 head component or None, proprio projector component or None)] in slot
    order.  The graph then routes every slotted linear by the static `obs_slot` buffer that load(slots=...) writes, runs EVERY policy's head and
    proprio projector on all B observations and picks each observation's own with one ovla_select_by_slot each: the assignment is data, so one
    capture serves every assignment of the same policy set.  With `film=True` on a per-policy-FiLM engine the graph also holds the ragged
    language average and the ONE ovla_film_vectors launch that turns it into every block's gamma / beta under each observation's own policy;
    load(slots=...) rewrites only `obs_slot`."""

    def __init__(self, engine: "VLAEngine", B: int, L: int, pixel_shape, *, head=None, use_proprio: bool = True, proprio_projector=None,
                 invariant: bool = False, film: bool = False, discrete: bool = False, n_tokens: Optional[int] = None, n_bins: Optional[int] = None,
                 policies=None, sample=None):
        dev = engine.device
        self.policies = policies
        self.obs_slot = None
        if policies is not None:
            if len(policies) != engine.n_slots or not policies:
                raise ValueError(f"ChunkGraph: {len(policies)} policies for an engine with {engine.n_slots} adapter slots")
            if head is not None or proprio_projector is not None:
                raise ValueError("ChunkGraph(policies=...): heads and proprio projectors come per policy")
            if film != engine.film_per_policy:
                raise ValueError("ChunkGraph(policies=..., film=...): FiLM with per-request policies goes with an engine built with "
                                 "use_film=\"per_policy\", and such an engine with film=True (its own FiLM Linears serve one policy)")
            self.slot_heads = [h for h, _ in policies] if all(h is not None for h, _ in policies) else None
            self.obs_slot = torch.zeros(B, dtype=torch.int32, device=dev)
            if use_proprio:
                proprio_projector = SlotProjectors([p for _, p in policies], engine.route)
        super().__init__(engine, B, L, pixel_shape, use_proprio, invariant, film)
        self.head = head
        if discrete and (head is not None or engine.lm_head is None):
            raise ValueError("ChunkGraph(discrete=True) is the token path: no action head, and the checkpoint's lm_head must be loaded")
        self.discrete = discrete
        self.n_tokens = n_tokens if n_tokens is not None else engine.cfg.vocab - engine.cfg.pad_to_multiple_of   # modeling_prismatic.py:732
        self.n_bins = n_bins if n_bins is not None else engine.cfg.n_action_bins - 1                              # bin_centers.shape[0]
        # `sample` = (temperature, (lo, hi)): ovla_sample_tokens in place of ovla_argmax_bins.  The generator's (seed_lo, seed_hi, call) and the
        # row keys are static device buffers that load() writes, so every replay draws what the eager call with the same values draws.
        if sample is not None and not discrete:
            raise ValueError("ChunkGraph(sample=...) goes with discrete=True")
        self.sample = None if sample is None else (float(sample[0]), (int(sample[1][0]), int(sample[1][1])))
        if self.sample is not None:
            self.sample_state = torch.zeros(3, dtype=torch.int32, device=dev)
            self.row_key = torch.arange(B * engine.cfg.num_action_tokens, dtype=torch.int32, device=dev)
        self.proprio_projector = proprio_projector
        self.graph = None
        self.out = None
        self.captures = 0

    def _run(self):
        if self.policies is not None:
            with self.engine.routing(self.obs_slot):
                return self._run_routed()
        return self._run_routed()

    def _run_routed(self):
        eng = self.engine
        with ops.batch_invariant(self.invariant):
            out = eng.forward_dev(self.ids, self.lab, self.lens, self.pixels, proprio=self.proprio, train=False,
                                  proprio_projector=self.proprio_projector, sel="actions", film_avg=self._film_average())
            ah, _ = eng.action_hidden(out)
            pred = self.head.fwd(ah)[0] if self.head is not None else None
            if self.policies is not None and self.slot_heads is not None:
                pred = eng.policy_heads_fwd(ah, self.slot_heads)
            if self.discrete:   # modeling.logits_for's GEMM, then the decode on the bf16 logits
                if self.sample is not None:
                    tok, bins, lp, ent = ops.sample_tokens(eng.lm_head_rows(ah)[: ah.shape[0]], n_tokens=self.n_tokens, n_bins=self.n_bins, window=self.sample[1],
                                                           temperature=self.sample[0], state_dev=self.sample_state, row_key=self.row_key)
                    return pred, ah, tok, bins, lp, ent
                tok, bins = ops.argmax_bins(eng.lm_head_rows(ah)[: ah.shape[0]], n_tokens=self.n_tokens, n_bins=self.n_bins)
                return pred, ah, tok, bins
        return pred, ah

    def load(self, input_ids, attention_mask, pixel_values, labels, proprio=None, slots=None, sample_state=None, row_key=None):
        super().load(input_ids, attention_mask, pixel_values, labels, proprio)
        if (sample_state is None) != (self.sample is None):
            raise ValueError("ChunkGraph.load: `sample_state` goes with a graph built with sample=")
        if sample_state is not None:   # (seed_lo, seed_hi, call) as 32-bit words; row_key int32 [B * A], default the row indices
            words = torch.tensor([int(v) & 0xFFFFFFFF for v in sample_state], dtype=torch.int64)
            self.sample_state.copy_(torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32), non_blocking=True)
            if row_key is None:
                row_key = torch.arange(self.row_key.numel(), dtype=torch.int32)
            self.row_key.copy_(torch.as_tensor(row_key).to(torch.int32).reshape(-1), non_blocking=True)
        if (slots is None) != (self.obs_slot is None):
            raise ValueError("ChunkGraph.load: `slots` goes with a graph built with policies=")
        if slots is not None:   # the host sees the values here: an out-of-range slot never reaches a kernel
            slots = [int(v) for v in slots]
            if len(slots) != self.B or any(not 0 <= v < len(self.policies) for v in slots):
                raise ValueError(f"ChunkGraph.load: slots {slots} for {self.B} observations and {len(self.policies)} policies")
            self.obs_slot.copy_(torch.tensor(slots, dtype=torch.int32), non_blocking=True)

    def capture(self):
        """Call after load() of a representative input: one eager warm-up (lazy tables, kernel attributes), then the capture."""
        with self._capturing(self._run):
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.out = self._run()
            self.captures += 1
        return self

    def replay(self):
        self.graph.replay()
        return self.out

    def __call__(self, input_ids, attention_mask, pixel_values, labels, proprio=None, slots=None, sample_state=None, row_key=None):
        self.load(input_ids, attention_mask, pixel_values, labels, proprio, slots, sample_state, row_key)
        if self.graph is None:
            self.capture()
        return self.replay()


# ======================================================================================================================
# hipGraph replay of the DDIM sampler (BASELINE.json configs[5]: FiLM + diffusion head)
# ======================================================================================================================
class DiffusionGraph(_StaticInputs):
    """The diffusion head's sampling loop (modeling_prismatic.py:793-877) as TWO captures over static buffers, with no host work between the
    steps:

      prefix  once per chunk: the optional ragged FiLM average, both towers on their two streams, the projector and the proprio token
              (VLAEngine.patches_dev) -> the static `patches` every step reuses (the reference caches them too, :810);
      step    replayed n_steps times back to back: ovla_ddim_prepare (timestep token + bf16(sample) from the device step index) -> noisy-action
              projector, assembly, Llama stack on the cached patches (forward_dev) -> action rows -> noise-predicting head -> ovla_ddim_step
              (sample updated in place, step index advanced).

    The host loop it replaces (OpenVLAForActionPrediction.predict_action / predict_action_batch with graph replay off) enqueues ~1.3 k
    launches per step, then synchronises, steps the scheduler in CPU torch and uploads the sample again; both compute the same bits.
    `coef` / `temb_table`: DDIMScheduler.step_coefficients() and the bf16 time_encoder rows of the scheduler's timesteps, one row per step.
    `invariant` and `film` as in ChunkGraph.  `step_replays` counts the step graph's replays over the object's life."""

    def __init__(self, engine: "VLAEngine", B: int, L: int, pixel_shape, *, head, noisy_action_projector, coef, temb_table,
                 use_proprio: bool = True, proprio_projector=None, invariant: bool = False, film: bool = False):
        super().__init__(engine, B, L, pixel_shape, use_proprio, invariant, film)
        dev, cfg = engine.device, engine.cfg
        if head is None or noisy_action_projector is None:
            raise ValueError("DiffusionGraph needs the noise-predicting head and the noisy-action projector")
        self.head, self.noisy_action_projector, self.proprio_projector = head, noisy_action_projector, proprio_projector
        self.n_steps = int(coef.shape[0])
        if tuple(coef.shape) != (self.n_steps, 4) or tuple(temb_table.shape) != (self.n_steps, cfg.llm_dim):
            raise ValueError(f"DiffusionGraph: coef {tuple(coef.shape)} / temb_table {tuple(temb_table.shape)} for {self.n_steps} steps, D = {cfg.llm_dim}")
        self.coef = coef.to(dev, F32).contiguous()
        self.temb_table = temb_table.to(dev, BF16).contiguous()
        n = B * cfg.chunk * cfg.action_dim
        self.sample = torch.zeros(n, dtype=F32, device=dev)           # the trajectory, bf16-rounded values held in fp32 (as the host loop holds them)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)     # index into the scheduler's timesteps; n_steps = sampling finished
        self.temb = torch.zeros((B, cfg.llm_dim), dtype=BF16, device=dev)
        self.noisy = torch.zeros(n, dtype=BF16, device=dev)
        self.prefix_graph = self.step_graph = None
        self.patches = self.ah = None
        self.step_replays = 0

    def _run_prefix(self):
        eng = self.engine
        with ops.batch_invariant(self.invariant):
            pp = self.proprio_projector if self.proprio_projector is not None else eng.proprio
            base, n_vis, _, _ = eng.patches_dev(self.ids, self.lab, self.pixels, self.proprio, pp, self._film_average(), False)
        return base, n_vis

    def _run_step(self, patches):
        eng = self.engine
        with ops.batch_invariant(self.invariant):
            ops.ddim_prepare(self.step, self.temb_table, self.temb, self.sample, self.noisy)
            out = eng.forward_dev(self.ids, self.lab, self.lens, self.pixels, train=False, noisy_actions=self.noisy, timestep_emb=self.temb,
                                  noisy_action_projector=self.noisy_action_projector, cached_patches=patches, sel="actions")
            ah, _ = eng.action_hidden(out)
            eps = self.head.fwd(ah)[0]
            ops.ddim_step(self.sample, eps, self.coef, self.step)
        return ah

    def load(self, input_ids, attention_mask, pixel_values, labels, proprio, noise):
        """noise: the start of the trajectory, fp32 [B, chunk, action_dim] already rounded through bf16."""
        super().load(input_ids, attention_mask, pixel_values, labels, proprio)
        self.sample.copy_(noise.reshape(-1).to(F32), non_blocking=True)
        self.step.zero_()

    def capture(self):
        """Call after load() of a representative input: one eager prefix + step as warm-up (lazy tables, kernel attributes), the loaded sample
        and step index put back, then the two captures."""
        def warm_up():
            start = self.sample.clone()
            self._run_step(self._run_prefix())
            self.sample.copy_(start)
            self.step.zero_()

        with self._capturing(warm_up):
            self.prefix_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.prefix_graph):
                self.patches = self._run_prefix()
            self.step_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.step_graph):
                self.ah = self._run_step(self.patches)
        return self

    def replay(self):
        """-> (sample fp32 [B * chunk * action_dim] on the HOST, the last step's action hidden states bf16 [B * A, D] in a static device buffer).
        The copy of the sample is the loop's only synchronisation."""
        self.prefix_graph.replay()
        for _ in range(self.n_steps):
            self.step_graph.replay()
        self.step_replays += self.n_steps
        return self.sample.cpu(), self.ah

    def __call__(self, input_ids, attention_mask, pixel_values, labels, proprio=None, noise=None):
        self.load(input_ids, attention_mask, pixel_values, labels, proprio, noise)
        if self.step_graph is None:
            self.capture()
        return self.replay()
