"""Worlds, one training step and bit-level comparison helpers for the training-step invariants (tests/test_step_invariants_gpu.py on the
device, tests/test_step_invariants_host.py for the helpers themselves and for the premises on the fp32 oracle).  Helpers only: no fixtures.

The invariants are algebraic identities of one step of `VLAEngine` -- how it strings its launches together across micro-steps, padded rows
and flat buffers -- and need no oracle:

    every gradient element receives ONE fp32 add per backward     =>  G(zero; b1, b2) == G(zero; b1) + G(zero; b2), one rounded add
    split reductions run in a fixed order                          =>  two identical steps give identical bits
    a power of two commutes with every bf16 and fp32 rounding      =>  G(loss_scale = s) == s * G(loss_scale = 1)
    pad positions are masked as keys and carry a zero gradient     =>  the ids under attention_mask == 0 change nothing
    every Param owns [offset, offset + numel) of its flat buffer   =>  the alignment gaps stay exactly zero

The one quantity the code forms with an order that is not fixed is the head's `loss_sum`: ovla_head_out_fwd adds one term per (row, action
dimension) with a float atomicAdd, in the order the workgroups finish.  `loss_reference` restates the terms from the prediction bits; where
their sum is exact in fp32 in ANY order (`order_free`) the loss is compared bit for bit -- against that restatement too --, otherwise to the
worst case of the n fp32 adds (`Findings.same_loss`).
"""
import importlib
import math
from typing import Dict, NamedTuple, Optional

import torch

from oracle import vla_oracle as vo

BF = torch.bfloat16
KINDS = ("l1", "film", "diffusion", "discrete", "l1_dropout")
PROMPT_LENS = [10, 8, 12]
BATCH_SEEDS = (2, 5)
load = importlib.import_module


# ---- worlds ----------------------------------------------------------------------------------------------------------------------------------
def make_batch(seed: int):
    """B = 3, ragged right padding (rows of 66, 64 and 69 tokens), two 56 x 56 images, bf16-exact float inputs."""
    synth = load("openvla-oft_amd.synthetic")
    batch = synth.make_batch(3, seed=seed, prompt_lens=PROMPT_LENS, image_size=56)
    for k in ("pixel_values", "proprio", "actions"):
        batch[k] = batch[k].to(BF).float()
    return batch


def diffusion_inputs(cfg, batch, seed: int):
    """The explicit `diffusion` argument of train_step_fwd_bwd, built on the host as test_film_diffusion_gpu.py::test_diffusion_training_step
    builds it: nothing is drawn inside the step."""
    dmod = load("openvla-oft_amd.diffusion")
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(3, 8, 7, generator=g).to(BF).float()
    timesteps = torch.randint(0, 50, (3,), generator=g)
    sched, enc = dmod.DDIMScheduler(50), dmod.SinusoidalPositionalEncoding(cfg.llm_dim)
    return dict(noise=noise, noisy_actions=sched.add_noise(batch["actions"], noise, timesteps).to(BF), timestep_emb=enc(timesteps.float()).to(BF))


def make_world(dev, kind: str) -> dict:
    """The reduced model of the engine tests under one objective: `l1`, `film` (L1 + FiLM), `diffusion` (noise-prediction MSE), `discrete`
    (next-token cross entropy, no head) or `l1_dropout` (L1 with lora_dropout = 0.25).  Two batches of the same shapes."""
    assert kind in KINDS, kind
    engine_mod, weights_mod, config_mod = (load(f"openvla-oft_amd.{m}") for m in ("engine", "weights", "config"))
    film, diffusion = kind == "film", kind == "diffusion"
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0, film=film, diffusion=diffusion).items()}
    cfg = config_mod.VLAConfig.from_any(ocfg)
    get, has = weights_mod.make_getter(sd, dev)
    head = {"diffusion": "diffusion", "discrete": "none"}.get(kind, "l1")
    extra = dict(lora_dropout=0.25, dropout_seed=1234) if kind == "l1_dropout" else {}
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head=head, use_film=film, has=has, **extra)
    batches = [make_batch(s) for s in BATCH_SEEDS]
    diff = [diffusion_inputs(cfg, b, 40 + i) for i, b in enumerate(batches)] if diffusion else [None, None]
    return dict(kind=kind, eng=eng, cfg=cfg, ocfg=ocfg, sd=sd, batches=batches, diffusion=diff, memo={})


class StepResult(NamedTuple):
    loss_sum: torch.Tensor            # fp32 [1], a device clone
    count: int
    grads: Dict[str, torch.Tensor]    # name -> fp32 clone of export_trainable("grad")
    pred: torch.Tensor                # predictions (bf16 [rows, action_dim]; int64 ids for `discrete`), a clone


def export_grads(eng) -> Dict[str, torch.Tensor]:
    return {n: g.detach().float().clone() for n, g in eng.export_trainable("grad").items()}


def step(world, batch, loss_scale: float = 1.0, *, call: Optional[int] = None, diffusion=None, film_avg=None) -> StepResult:
    """One forward + backward of the world's objective INTO WHATEVER THE GRADIENT BUFFERS HOLD (the caller zeroes them).  `call`: the value
    `engine.dropout.call` is set to before the step -- the forward advances it by one and draws its masks from the result, so two steps
    given the same `call` share their masks (only `l1_dropout` drops).  `diffusion`: the explicit noise inputs that go with `batch` (a
    `diffusion` world; default: those of the world's first batch when `batch` is that batch)."""
    eng, kind = world["eng"], world["kind"]
    if call is not None:
        eng.dropout.call = int(call)
    if kind == "discrete":
        loss_sum, count, pred = eng.train_step_discrete(batch, loss_scale=loss_scale)
    else:
        kw = {}
        if kind == "diffusion":
            kw["diffusion"] = diffusion if diffusion is not None else world["diffusion"][[id(b) for b in world["batches"]].index(id(batch))]
        if film_avg is not None:
            kw["film_avg"] = film_avg
        loss_sum, count, pred = eng.train_step_fwd_bwd(batch, loss_scale=loss_scale, **kw)
    return StepResult(loss_sum.detach().clone(), int(count), export_grads(eng), pred.detach().clone())


def fresh_step(world, which: int, loss_scale: float = 1.0, call: int = 0, memo: bool = True) -> StepResult:
    """step() of the world's batch `which` from zeroed gradients; remembered per (batch, scale, call), so the tests share their references."""
    key = (which, float(loss_scale), int(call))
    if memo and key in world["memo"]:
        return world["memo"][key]
    world["eng"].zero_grad()
    res = step(world, world["batches"][which], loss_scale, call=call)
    if memo:
        world["memo"][key] = res
    return res


def step_target(world, which: int):
    """What the head's loss compares the prediction with (None for `discrete`, whose loss is a torch sum of per-row values)."""
    if world["kind"] == "discrete":
        return None
    src = world["diffusion"][which]["noise"] if world["kind"] == "diffusion" else world["batches"][which]["actions"]
    return src.to(BF).reshape(-1, world["cfg"].action_dim)


# ---- the flat buffers ------------------------------------------------------------------------------------------------------------------------
def padding_mask(store, dtype) -> torch.Tensor:
    """bool over the flat buffer of `dtype` (on its device): True on every element NO Param owns -- the gaps that align each view to
    ParamStore.ALIGN elements.  From p.offset and p.numel alone."""
    flat = store.flat[dtype]
    owned = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    for p in store.params:
        if p.dtype == dtype:
            assert 0 <= p.offset and p.offset + p.numel <= flat.numel(), p.name
            assert not bool(owned[p.offset:p.offset + p.numel].any()), f"{p.name} overlaps another parameter"
            owned[p.offset:p.offset + p.numel] = True
    return ~owned


# ---- the loss, restated from the prediction bits -----------------------------------------------------------------------------------------------
def loss_reference(pred, target, mse: bool):
    """ovla_head_out_fwd's loss terms from bf16 `pred` / `target` [rows, adim]: d = bf16(target - pred), term = bf16(d * d) (MSE) or |d| (L1).
    -> (their exact sum as a Python float (float64 holds it exactly), n, order_free).  order_free: every term is a multiple of q = the last
    bit of the smallest nonzero term, and sum / q < 2^24 -- then every partial sum of every order is representable in fp32 and the atomic
    adds are exact whatever order they arrive in."""
    p, t = pred.detach().cpu().to(BF).float(), target.detach().cpu().to(BF).float()
    d = (t - p).to(BF).float()
    terms = ((d * d).to(BF) if mse else d.abs().to(BF)).double().reshape(-1)
    total = float(terms.sum())
    nz = terms[terms > 0]
    if nz.numel() == 0:
        return total, terms.numel(), True
    q = 2.0 ** (math.frexp(float(nz.min()))[1] - 1 - 7)          # last place of a bf16 (8 significant bits) at the smallest term
    return total, terms.numel(), bool(total / q < 2.0 ** 24)


def ulp32(x: float) -> float:
    return 2.0 ** (math.frexp(abs(x))[1] - 24) if x != 0.0 else 2.0 ** -149


# ---- comparison helpers ------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


class Findings(list):
    """Collects every mismatch of a test that walks over the tensors of a step (the style of gemm_reference.Failures): each entry names the
    tensor, how many elements differ, the first differing index and both values there; `done()` asserts once."""

    def same_bits(self, a, b, what: str) -> bool:
        if a.shape != b.shape or a.dtype != b.dtype:
            self.append(f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}")
            return False
        b = b.to(a.device)
        if torch.equal(_bits(a), _bits(b)):
            return True
        bad = (_bits(a) != _bits(b)).reshape(-1)
        i = int(bad.nonzero()[0])
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), a.shape)) if a.dim() else ()
        self.append(f"{what}: {int(bad.sum())} of {a.numel()} elements differ; first at {idx}: got {a.reshape(-1)[i].item()!r} want {b.reshape(-1)[i].item()!r}")
        return False

    def same_grads(self, got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], what: str, exclude=()):
        """Every tensor of two gradient dicts, bit for bit; a name in only one of them is a finding too."""
        if set(got) != set(want):
            self.append(f"{what}: tensor names differ: {sorted(set(got) ^ set(want))[:4]}")
        for n in sorted(set(got) & set(want)):
            if n not in exclude:
                self.same_bits(got[n], want[n], f"{what}: {n}")

    def all_finite(self, grads: Dict[str, torch.Tensor], what: str):
        for n in sorted(grads):
            bad = ~torch.isfinite(grads[n]).reshape(-1)
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                self.append(f"{what}: {n}: {int(bad.sum())} of {bad.numel()} elements are not finite; first at flat index {i}: {grads[n].reshape(-1)[i].item()!r}")

    def every_tensor_nonzero(self, grads: Dict[str, torch.Tensor], what: str):
        for n in sorted(grads):
            if not bool((grads[n] != 0).any()):
                self.append(f"{what}: {n}: all {grads[n].numel()} elements are zero")

    def all_zero(self, t, what: str):
        nz = (t != 0).reshape(-1) | torch.isnan(t).reshape(-1)
        if bool(nz.any()):
            i = int(nz.nonzero()[0])
            self.append(f"{what}: {int(nz.sum())} of {nz.numel()} elements are not zero; first at flat index {i}: {t.reshape(-1)[i].item()!r}")

    def same_loss(self, a, b, ref, what: str):
        """Two loss sums of the same forward.  `ref` = loss_reference(...) or None (a loss formed in a fixed order: bits).  order_free: both
        equal the exact sum of the restated terms, bit for bit.  Otherwise each of the n adds rounds by at most half an ulp of a partial sum
        that never exceeds the total (the terms are non-negative), so both lie within n / 2 ulp(total) of the exact sum."""
        if ref is None:
            return self.same_bits(a, b, what)
        total, n, order_free = ref
        for tag, v in (("first", a), ("second", b)):
            v = float(v.reshape(-1)[0])
            if order_free:
                self.check(v == total, f"{what}: {tag} loss_sum {v!r} is not the exact sum {total!r} of its {n} terms (exact in fp32 in any order)")
            else:
                self.check(abs(v - total) <= 0.5 * n * ulp32(total * (1.0 + n * 2.0 ** -23)), f"{what}: {tag} loss_sum {v!r} is beyond {n} / 2 ulp of the exact sum {total!r}")

    def check(self, cond, what: str):
        if not cond:
            self.append(what)

    def done(self):
        assert not self, f"{len(self)} findings:\n" + "\n".join(self[:16])
