"""Gradient-norm clipping and the non-finite step guard on the GPU: ovla_grad_sumsq, ovla_grad_clip_coef and ovla_adamw_clipped bit for bit
against the numpy restatement (tests/grad_clip_reference.py), then the engine (off means off, the clipped step, the skipped step, the
optimizer-state counters), the fine-tune driver and a two-rank run, on the reduced-size model of test_ema_gpu.py or on raw buffers.  Every
comparison is exact."""
import importlib
import math
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import grad_clip_reference as R
from oracle import vla_oracle as vo
from tests.pointwise_reference import adamw_inputs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BF = torch.bfloat16
load = importlib.import_module
GUARD = 64
C = R.CHUNK
# every size at which the code takes another path: nothing, the scalar tail alone, a partial 16-byte group, one wave / one workgroup of groups,
# the last chunk short by one, exactly full, over by one, several chunks, 515 partials: every lane of the second launch adds two or three, and
# 1285 partials: every lane of the second launch takes one batch of four loads and one or two single ones after it
SIZES = (0, 1, 7, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5, 515 * C + 3, 1285 * C + 3)
SCALES = (1.0, 1.0 / 3.0)


def bits_of(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == BF:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.view(torch.int64).numpy().view(np.uint64) if t.dtype == torch.float64 else t.view(torch.int32).numpy().view(np.uint32)


def same_scalar(got, want):
    """Bit equality of two floats of one width, a NaN matching any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype
    return bool(np.isnan(want) and np.isnan(got)) or got.tobytes() == want.tobytes()


@pytest.fixture(scope="module")
def gradient_values():
    """One host array of mixed-sign values over six decades, shared (read-only) by every size."""
    g = np.random.default_rng(17)
    n = max(SIZES)
    v = (g.standard_normal(n) * 10.0 ** g.uniform(-3, 3, n)).astype(np.float32)
    v.setflags(write=False)
    return v


# ----------------------------------------------------------------------------------------------------------------------------------------
# the kernels on raw buffers
# ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES, ids=["scale1", "scale_third"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_sumsq_equals_the_restatement_bit_for_bit(ops, dev, gradient_values, dtype, scale):
    for n in SIZES:
        host = np.full(n + 2 * GUARD, np.nan, np.float32)            # NaN on both sides of the n elements: one read outside [0, n) poisons the sum
        host[GUARD:GUARD + n] = gradient_values[:n]
        buf = torch.from_numpy(host).to(dev)
        n_partials = ops.grad_sumsq_workspace_elems(n)
        assert n_partials == (n + C - 1) // C
        ws = torch.full((n_partials + 2,), math.nan, dtype=torch.float64, device=dev)   # stale NaNs inside, two guards behind
        slots = torch.full((3,), math.nan, dtype=torch.float64, device=dev)
        # (n is passed as the argument: the view of an empty tensor has no address.  The workspace is told to be exactly its partials' size.)
        ops.grad_sumsq(buf[GUARD:], slots, 1, ws[:max(1, n_partials)], is_bf16=dtype == "bf16", grad_scale=scale, n=n)
        got = slots.cpu().numpy()
        want = R.grad_sumsq(gradient_values[:n], scale, dtype == "bf16")
        assert np.isfinite(want) and got[1].tobytes() == want.tobytes(), f"{dtype} scale {scale} n {n}: {got[1]!r} != {want!r}"
        assert np.isnan(got[0]) and np.isnan(got[2]), f"n {n}: a neighbouring slot was written"
        assert bool(torch.isnan(ws[n_partials:]).all()), f"n {n}: the workspace was written past its {n_partials} partials"
        assert np.array_equal(bits_of(buf), host.view(np.uint32)), f"n {n}: the gradient was written"
    # the same call with n smaller than the buffer: the argument, not the tensor, bounds the reads
    n = 3 * C + 5
    buf = torch.from_numpy(np.concatenate([gradient_values[:n], np.full(C, np.nan, np.float32)])).to(dev)
    ops.grad_sumsq(buf, slots, 0, ws, is_bf16=dtype == "bf16", grad_scale=scale, n=n)
    assert slots[0].cpu().numpy().tobytes() == R.grad_sumsq(gradient_values[:n], scale, dtype == "bf16").tobytes()


def run_clip(ops, dev, grads, scale, max_norm, state, skip_nonfinite=True):
    """sumsq of a (bf16-parameter, fp32-parameter) pair of gradient buffers into two slots, then the coefficient launch."""
    slots = torch.full((2,), math.nan, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, max(ops.grad_sumsq_workspace_elems(g.size) for g in grads)), dtype=torch.float64, device=dev)
    for k, g in enumerate(grads):
        ops.grad_sumsq(torch.from_numpy(g).to(dev), slots, k, ws, is_bf16=k == 0, grad_scale=scale)
    ops.grad_clip_coef(slots, state, max_norm, skip_nonfinite)
    return ops.read_grad_clip_state(state)


def test_coefficient_cases_and_counters(ops, dev, gradient_values):
    a, b = gradient_values[:C + 9].copy(), gradient_values[C + 9:C + 9 + 777].copy()
    with_nan, with_inf = b.copy(), a.copy()
    with_nan[500], with_inf[C + 3] = np.nan, -np.inf
    norm = float(np.sqrt(R.grad_sumsq(a, 1.0, True) + R.grad_sumsq(b, 1.0, False)))
    cases = [("below the threshold", (a, b), 1.0, 2.0 * norm, dict(coef=1.0, skip=0)),
             ("above the threshold", (a, b), 1.0, 0.3 * norm, dict(skip=0)),
             ("above, scaled gradients", (a, b), 1.0 / 3.0, 0.2 * norm, dict(skip=0)),
             ("all-zero gradient", (np.zeros(300, np.float32), np.zeros(5, np.float32)), 1.0, 1.0, dict(coef=1.0, norm=0.0, skip=0)),
             ("guard only", (a, b), 1.0, math.inf, dict(coef=1.0, skip=0)),
             ("one NaN element", (a, with_nan), 1.0, 0.3 * norm, dict(coef=1.0, skip=1)),
             ("one Inf element", (with_inf, b), 1.0, 0.3 * norm, dict(coef=1.0, skip=1, norm=math.inf)),
             ("clean again", (a, b), 1.0, 0.3 * norm, dict(skip=0))]
    state, want = ops.grad_clip_state(dev), R.new_state()
    for what, grads, scale, max_norm, pins in cases:
        got = run_clip(ops, dev, grads, scale, max_norm, state)
        want = R.clip_coef([R.grad_sumsq(grads[0], scale, True), R.grad_sumsq(grads[1], scale, False)], np.float32(max_norm), want)
        assert same_scalar(np.float32(got["norm"]), want["norm"]) and same_scalar(np.float32(got["coef"]), want["coef"]), (what, got, want)
        assert (got["skip"], got["steps"], got["clipped"], got["skipped"]) == (want["skip"], want["steps"], want["clipped"], want["skipped"]), (what, got, want)
        for k, v in pins.items():
            assert got[k] == v, (what, k, got)
        if "above" in what or what == "clean again":
            assert 0.0 < got["coef"] < 1.0, (what, got)
    assert (got["steps"], got["clipped"], got["skipped"]) == (8, 3, 2)
    # the guard switched off: a NaN norm is recorded, nothing is skipped or counted, the coefficient is 1
    off = run_clip(ops, dev, (a, with_nan), 1.0, 0.3 * norm, ops.grad_clip_state(dev), skip_nonfinite=False)
    assert math.isnan(off["norm"]) and (off["coef"], off["skip"], off["steps"], off["clipped"], off["skipped"]) == (1.0, 0, 1, 0, 0)
    _lib = load("openvla-oft_amd._lib")
    for bad in (0.0, -2.0, math.nan):
        with pytest.raises(_lib.OvlaError, match="ovla_grad_clip_coef"):
            ops.grad_clip_coef(torch.zeros(2, dtype=torch.float64, device=dev), state, bad)
    assert ops.read_grad_clip_state(state)["steps"] == 8, "a refused call launches nothing"


def device_state(dev, coef, skip):
    """A state as ovla_grad_clip_coef would have left it, written from the host."""
    words = np.zeros(6, np.int32)
    words[0:2] = np.array([coef, 123.0], np.float32).view(np.int32)
    words[2] = skip
    return torch.from_numpy(words).to(dev)


def guarded(t, dev):
    """CPU tensor -> (device buffer with GUARD sentinel elements on both sides, the view of the middle)."""
    buf = torch.full((t.numel() + 2 * GUARD,), 7.25, dtype=t.dtype)
    buf[GUARD:GUARD + t.numel()] = t
    buf = buf.to(dev)
    return buf, buf[GUARD:GUARD + t.numel()]


@pytest.mark.parametrize("scale", SCALES, ids=["scale1", "scale_third"])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "f32"])
def test_adamw_clipped_identity_restatement_and_skip(ops, dev, dtype, scale):
    n = 2048 + 77                                                    # nine workgroups, the last one partial
    p, m, v, grad = adamw_inputs(torch.Generator().manual_seed(3), n, dtype)
    hp = dict(step=3, lr=5e-4, grad_scale=scale)
    g_dev = grad.to(dev)

    def run(coef, skip, clipped=True):
        bufs = [guarded(t, dev) for t in (p, m, v)]
        views = [b[1] for b in bufs]
        if clipped:
            ops.adamw_clipped(*views, g_dev, device_state(dev, coef, skip), **hp)
        else:
            ops.adamw(*views, g_dev, **hp)
        for (buf, _), name in zip(bufs, "pmv"):
            assert bool((buf[:GUARD] == 7.25).all()) and bool((buf[-GUARD:] == 7.25).all()), f"coef {coef} skip {skip}: a guard of {name} was written"
        return [bits_of(x) for x in views]

    plain = run(None, None, clipped=False)
    assert all(np.array_equal(a, b) for a, b in zip(run(1.0, 0), plain)), "coef == 1: bit-identical to ovla_adamw, tail included"
    coef = np.float32(0.37)
    want = R.adamw_clipped(p, m, v, grad, dict(skip=0, coef=coef), **hp)
    got = run(float(coef), 0)
    for a, w, name in zip(got, want, "pmv"):
        assert np.array_equal(a, bits_of(w)), f"{name}: {int((a != bits_of(w)).sum())} of {n} elements differ from the restatement"
    assert not np.array_equal(got[0], plain[0]), "the coefficient is applied"
    before = [bits_of(t) for t in (p, m, v)]
    assert all(np.array_equal(a, b) for a, b in zip(run(0.5, 1), before)), "skip: parameters and moments keep their bits"
    assert g_dev.cpu().equal(grad), "the gradient is never written"


# ----------------------------------------------------------------------------------------------------------------------------------------
# the engine
# ----------------------------------------------------------------------------------------------------------------------------------------
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


def tensors(e, which):
    """{(store index, dtype tag): device tensor} of the flat parameters ("flat"), moments ("exp_avg", "exp_avg_sq") or gradients ("flat_grad")."""
    return {(i, "bf16" if dt == BF else "f32"): t for i, st in enumerate(e.stores) for dt, t in getattr(st, which).items()}


def buffers(e, which):
    return {k: bits_of(t) for k, t in tensors(e, which).items()}


def trained_state(e):
    return {w: buffers(e, w) for w in ("flat", "exp_avg", "exp_avg_sq")}


def same_state(a, b):
    return all(a[w].keys() == b[w].keys() and all(np.array_equal(a[w][k], b[w][k]) for k in a[w]) for w in a)


def backward(e, world, i):
    e.zero_grad()
    loss_sum, _, _ = e.train_step_fwd_bwd(batch_of(world, i))
    return bits_of(loss_sum)


def step(e, world, i, lr=5e-4, **kw):
    loss = backward(e, world, i)
    e.adamw_step(lr, **kw)
    e.refresh_derived()
    return loss


def test_engine_huge_max_norm_is_the_plain_engine_bit_for_bit(world, dev):
    e_clip, e_plain = fresh(world, dev), fresh(world, dev)
    assert not e_plain.grad_clip_enabled
    with pytest.raises(RuntimeError, match="enable_grad_clip"):
        e_plain.grad_clip_stats()
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="max_norm"):
            e_clip.enable_grad_clip(bad)
    e_clip.enable_grad_clip(1e30)
    assert e_clip.grad_clip_enabled and e_clip._grad_clip["slots"].numel() == sum(len(st.flat) for st in e_clip.stores) >= 3
    for i in range(3):
        assert np.array_equal(step(e_clip, world, i), step(e_plain, world, i)), f"loss of step {i}"
        assert same_state(trained_state(e_clip), trained_state(e_plain)), f"parameters or moments after step {i}"
    s = e_clip.grad_clip_stats()
    assert set(s) == {"norm", "coef", "skipped", "clipped", "steps"}
    assert (s["coef"], s["skipped"], s["clipped"], s["steps"]) == (1.0, 0, 0, 3) and 0.0 < s["norm"] < math.inf


def test_engine_clipped_step_equals_the_restatement(world, dev):
    e = fresh(world, dev)
    step(e, world, 0)                                               # a plain first step: the clipped one starts from non-zero moments
    backward(e, world, 1)
    scale, lr = 0.5, 5e-4
    host = {w: {k: t.detach().cpu().clone() for k, t in tensors(e, w).items()} for w in ("flat", "exp_avg", "exp_avg_sq", "flat_grad")}
    keys = list(host["flat"])
    assert keys == sorted(keys) and len({i for i, _ in keys}) == 3 and {t for _, t in keys} == {"bf16", "f32"}, "stores in order, bf16 before fp32"
    slots = [R.grad_sumsq(host["flat_grad"][k].numpy(), scale, k[1] == "bf16") for k in keys]
    max_norm = float(np.float32(0.25 * math.sqrt(sum(slots))))
    e.enable_grad_clip(max_norm)
    e.adamw_step(lr, grad_scale=scale)
    want = R.clip_coef(slots, np.float32(max_norm), R.new_state())
    got = e.grad_clip_stats()
    assert same_scalar(np.float32(got["norm"]), want["norm"]) and same_scalar(np.float32(got["coef"]), want["coef"]), (got, want)
    assert 0.2 < got["coef"] < 0.3 and (got["steps"], got["clipped"], got["skipped"]) == (1, 1, 0)
    after = trained_state(e)
    for k in keys:
        p, m, v = R.adamw_clipped(host["flat"][k], host["exp_avg"][k], host["exp_avg_sq"][k], host["flat_grad"][k], want, step=2, lr=lr, grad_scale=scale)
        for w, t in (("flat", p), ("exp_avg", m), ("exp_avg_sq", v)):
            assert np.array_equal(after[w][k], bits_of(t)), f"{w} of store {k}: {int((after[w][k] != bits_of(t)).sum())} elements differ from the restatement"


def test_engine_skips_a_non_finite_step_and_trains_on(world, dev):
    e, plain = fresh(world, dev), fresh(world, dev)
    e.enable_grad_clip(math.inf)                                    # guard only: every finite step is the plain engine's
    e.enable_ema()
    step(e, world, 0), step(plain, world, 0)
    e.ema_update(0.5)
    backward(e, world, 1)
    e.stores[0].flat_grad[BF][5] = float("nan")                     # one element of one flat gradient buffer, from the host
    before, shadow_before = trained_state(e), {k: v.clone() for k, v in e.stores[0].ema_shadow.items()}
    e.adamw_step(5e-4)
    e.ema_update(0.5)                                               # runs as usual, on the unchanged parameters
    e.refresh_derived()
    s = e.grad_clip_stats()
    assert math.isnan(s["norm"]) and (s["coef"], s["skipped"], s["clipped"], s["steps"]) == (1.0, 1, 0, 2)
    assert same_state(trained_state(e), before), "a skipped step leaves every parameter and moment bit-unchanged"
    assert all(st.step == 2 for st in e.stores), "the host does not learn of the skip: the step number is consumed"
    assert any(not torch.equal(v, shadow_before[k]) for k, v in e.stores[0].ema_shadow.items()) and e.ema_step == 2
    # the following clean step equals the plain engine's, whose step counters are advanced by hand past the skipped number
    for st in plain.stores:
        st.step += 1
    assert np.array_equal(step(e, world, 2), step(plain, world, 2))
    assert same_state(trained_state(e), trained_state(plain)) and not same_state(trained_state(e), before)
    s = e.grad_clip_stats()
    assert math.isfinite(s["norm"]) and s["norm"] > 0 and (s["coef"], s["skipped"], s["clipped"], s["steps"]) == (1.0, 1, 0, 3)


def test_optimizer_state_carries_the_counters_only_when_enabled(world, dev):
    e, plain = fresh(world, dev), fresh(world, dev)
    backward(e, world, 0)
    norm = math.sqrt(sum(R.grad_sumsq(t.cpu().numpy(), 1.0, dt == BF) for st in e.stores for dt, t in st.flat_grad.items()))
    e.enable_grad_clip(0.5 * norm)
    e.adamw_step(5e-4)
    e.refresh_derived()
    step(plain, world, 0)
    osd, osd_plain = e.optimizer_state_dict(), plain.optimizer_state_dict()
    clip_keys = sorted(k for k in osd if k.startswith("grad_clip."))
    assert clip_keys == ["grad_clip.clipped", "grad_clip.skipped", "grad_clip.steps"] and not any(k.startswith("grad_clip.") for k in osd_plain)
    assert all(osd[k].dtype == torch.int64 and osd[k].shape == (1,) for k in clip_keys)
    assert [int(osd[k].item()) for k in clip_keys] == [1, 0, 1]
    assert {k for k in osd if not k.startswith("grad_clip.")} == set(osd_plain)
    host = {k: v.detach().cpu().clone() for k, v in osd.items()}
    e2 = fresh(world, dev)
    e2.load_optimizer_state_dict(host)                              # not enabled: the entries are neither required nor read
    assert not e2.grad_clip_enabled
    e2.enable_grad_clip(0.5 * norm)
    assert e2.grad_clip_stats()["steps"] == 0
    e2.load_optimizer_state_dict(host)
    s = e2.grad_clip_stats()
    assert (s["steps"], s["clipped"], s["skipped"]) == (1, 1, 0)
    e2.load_trainable({k: v.detach().cpu().clone() for k, v in e.export_trainable("data").items()})
    la, lb = step(e, world, 1), step(e2, world, 1)                  # the resumed engine continues counters and trajectory
    assert np.array_equal(la, lb) and same_state(trained_state(e), trained_state(e2))
    assert e2.grad_clip_stats() == e.grad_clip_stats() and e2.grad_clip_stats()["steps"] == 2
    e2.load_optimizer_state_dict({k: v for k, v in host.items() if not k.startswith("grad_clip.")})   # enabled, none present: kept
    assert e2.grad_clip_stats()["steps"] == 2


# ----------------------------------------------------------------------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------------------------------------------------------------------
def drive(world, root, *, first=0, lines=None, clip=None, **kw):
    ft = world["ft"]
    engines, orig = [], ft.VLAEngine

    def build(*a, **k):
        engines.append(orig(*a, **k))
        return engines[-1]

    cfg = ft.FinetuneConfig(**{**dict(run_root_dir=root, dataset_name="libero_spatial_no_noops", batch_size=2, num_images_in_input=2, use_proprio=True,
                                      wandb_log_freq=1, max_steps=3, save_freq=2), **kw})
    ft.VLAEngine = build
    try:
        hist = ft.finetune(cfg, model_config=world["base_cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()},
                           dataset=(batch_of(world, i) for i in range(first, 12)), dataset_statistics=world["stats"],
                           log=(lines.append if lines is not None else (lambda *_: None)), **(clip or {}))
    finally:
        ft.VLAEngine = orig
    engine, = engines
    return hist, engine


@pytest.fixture(scope="module")
def runs(world, dev, tmp_path_factory):
    """Three optimizer steps with max_grad_norm = 1e-3 and three with the feature switched off, each with a checkpoint after the third."""
    root, lines = tmp_path_factory.mktemp("grad_clip"), []
    hist, engine = drive(world, root / "clip", lines=lines, clip=dict(max_grad_norm=1e-3))
    hist_off, engine_off = drive(world, root / "off", clip=dict(skip_nonfinite_steps=False))
    ck, = (root / "clip").glob("*--2_chkpt")
    ck_off, = (root / "off").glob("*--2_chkpt")
    return dict(hist=hist, engine=engine, lines=lines, ck=ck, hist_off=hist_off, engine_off=engine_off, ck_off=ck_off)


def test_driver_logs_the_three_series_and_checkpoints_the_counters(runs):
    from safetensors.torch import load_file

    hist, engine, hist_off = runs["hist"], runs["engine"], runs["hist_off"]
    assert engine.grad_clip_enabled and engine._grad_clip["max_norm"] == 1e-3 and engine._grad_clip["skip_nonfinite"]
    assert len(hist["grad_norm"]) == len(hist["grad_clip_coef"]) == len(hist["skipped_steps"]) == len(hist["loss_value"]) == 3
    assert all(math.isfinite(x) and x > 1e-3 for x in hist["grad_norm"]) and all(0.0 < c < 1.0 for c in hist["grad_clip_coef"])
    assert hist["skipped_steps"] == [0, 0, 0]
    assert sum("grad_norm" in str(l) and "clip_coef" in str(l) and "skipped 0" in str(l) for l in runs["lines"]) == 3, runs["lines"]
    osd = load_file(str(runs["ck"] / "optimizer_state--2_checkpoint.safetensors"))
    assert [int(osd[f"grad_clip.{k}"].item()) for k in ("steps", "clipped", "skipped")] == [3, 3, 0]
    # without the feature: the old history keys, the old optimizer-state keys, the same files in the checkpoint directory
    assert not runs["engine_off"].grad_clip_enabled
    assert set(hist_off) == {"loss_value", "learning_rate", "val"} and set(hist) == set(hist_off) | {"grad_norm", "grad_clip_coef", "skipped_steps"}
    osd_off = load_file(str(runs["ck_off"] / "optimizer_state--2_checkpoint.safetensors"))
    assert set(osd_off) == {k for k in osd if not k.startswith("grad_clip.")}
    listing = lambda d: sorted(str(f.relative_to(d)) for f in d.rglob("*"))  # noqa: E731
    assert listing(runs["ck"]) == listing(runs["ck_off"]), "no new file in a checkpoint directory"


def test_driver_default_is_the_guard_alone(runs, world, dev, tmp_path):
    """max_grad_norm=None with the guard on: max_norm = inf, coefficient 1 on every step, the losses of the run without the feature bit for bit."""
    hist_guard, engine_guard = drive(world, tmp_path / "guard")
    assert engine_guard.grad_clip_enabled and engine_guard._grad_clip["max_norm"] == math.inf
    assert hist_guard["grad_clip_coef"] == [1.0, 1.0, 1.0] and hist_guard["skipped_steps"] == [0, 0, 0]
    assert hist_guard["loss_value"] == runs["hist_off"]["loss_value"] and hist_guard["grad_norm"][0] == runs["hist"]["grad_norm"][0]


def test_driver_resume_continues_the_counters(runs, world, dev, tmp_path):
    lines = []
    _, resumed = drive(world, tmp_path / "resumed", first=3, lines=lines, resume=True, resume_step=2, vla_path=str(runs["ck"]), max_steps=4,
                       clip=dict(max_grad_norm=1e-3))
    assert any("continues its counters" in str(l) for l in lines), lines
    s = resumed.grad_clip_stats()
    assert (s["steps"], s["clipped"], s["skipped"]) == (5, 5, 0), "three steps in the checkpoint, two after it"


# ----------------------------------------------------------------------------------------------------------------------------------------
# two ranks
# ----------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world_size, port, out):
    import torch.distributed as dist

    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    engine_mod, weights_mod, config_mod, synth, dp = (load("openvla-oft_amd." + m) for m in ("engine", "weights", "config", "synthetic", "dp"))
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(config_mod.VLAConfig.from_any(ocfg), get, dev, lora=True, use_proprio=True, head="l1", has=has)
    eng.enable_grad_clip(1e-3)
    red = dp.GradReducer(eng.stores, world_size, bucket_bytes=64 << 10, comm_dtype="fp32")
    eng.attach_reducer(red, overlap=True)
    batch = synth.make_batch(4, seed=31, prompt_lens=[10, 8, 12, 9], image_size=56)
    eng.zero_grad()
    eng.train_step_fwd_bwd({k: (v[2 * rank:2 * rank + 2] if torch.is_tensor(v) else v) for k, v in batch.items()})
    red.all_reduce()
    eng.adamw_step(lr=5e-4, grad_scale=1.0 / world_size)
    eng.refresh_derived()
    stats = eng.grad_clip_stats()
    torch.save({"stats": stats, "params": {k: v.detach().float().cpu().clone() for k, v in eng.export_trainable("data").items()}}, f"{out}/rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_compute_the_same_norm_and_land_on_the_same_parameters(dev, tmp_path):
    import torch.multiprocessing as mp

    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    assert np.float32(r0["stats"]["norm"]).tobytes() == np.float32(r1["stats"]["norm"]).tobytes() and r0["stats"] == r1["stats"]
    assert 0.0 < r0["stats"]["coef"] < 1.0 and (r0["stats"]["steps"], r0["stats"]["clipped"], r0["stats"]["skipped"]) == (1, 1, 0)
    for k in r0["params"]:
        assert torch.equal(r0["params"][k], r1["params"][k]), f"ranks disagree on the updated {k}"
