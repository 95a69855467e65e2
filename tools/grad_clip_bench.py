"""Gradient clipping beside ovla_adamw on flat buffers of the full-size trainable stores (OpenVLA-7B, LoRA r = 32, L1 head + proprio
projector: the sizes are read from an engine of that configuration), and the optimizer step / the fine-tune step with the feature on and off.

Per buffer, in one process: warm-up, then `--reps` rounds of (ovla_grad_sumsq -- both of its launches --, ovla_adamw, ovla_adamw_clipped),
ALTERNATED, each between its own pair of HIP events; the coefficient launch is timed the same way on the engine's slots.  The buffers are
allocated for the measurement, so the engine's state is not touched.  Bytes per element, from the kernels' loads and stores: sumsq 4 (the fp32
gradient, read once; the partials are 8 bytes per 8192 elements); AdamW, plain or clipped, 3 x 2 read + 4 read + 3 x 2 written = 16 (bf16)
or 3 x 4 + 4 + 3 x 4 = 28 (fp32).
Then VLAEngine.adamw_step alone (gradients left in place, HIP events) and the whole fine-tune step (fwd + bwd + AdamW + refresh, host clock
between two synchronisations), each alternated in blocks with the feature off and on.  Everything is reported, nothing is a pass / fail
condition: the step differs by +-3 % between machines.
Usage: python tools/grad_clip_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--no-step] > profiles/grad_clip_bench.jsonl"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module
BF = torch.bfloat16
ADAMW_BYTES = {BF: 16, torch.float32: 28}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_kernels(ops, dev, name, dtype, n, reps):
    g = torch.Generator(device=dev).manual_seed(n % 9973)
    param = (torch.randn(n, device=dev, generator=g) * 0.02).to(dtype)
    m, v = torch.zeros_like(param), torch.zeros_like(param)
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    slots = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.zeros(ops.grad_sumsq_workspace_elems(n), dtype=torch.float64, device=dev)
    state = ops.grad_clip_state(dev)
    ops.grad_sumsq(grad, slots, 0, ws, is_bf16=dtype == BF)
    ops.grad_clip_coef(slots, state, 1.0)          # a real coefficient below 1 for the clipped launches
    step = [0]

    def adamw(clipped):
        step[0] += 1
        if clipped:
            ops.adamw_clipped(param, m, v, grad, state, step=step[0], lr=5e-4)
        else:
            ops.adamw(param, m, v, grad, step=step[0], lr=5e-4)

    runs = {"sumsq": lambda: ops.grad_sumsq(grad, slots, 0, ws, is_bf16=dtype == BF), "adamw": lambda: adamw(False), "adamw_clipped": lambda: adamw(True)}
    for fn in runs.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    out = dict(buffer=name, dtype="bf16" if dtype == BF else "f32", elements=n, coef_during_measurement=ops.read_grad_clip_state(state)["coef"])
    for k in runs:
        out[f"{k}_us"] = 1e3 * med[k]
        out[f"{k}_us_min_max"] = [1e3 * min(ms[k]), 1e3 * max(ms[k])]
    out["sumsq_TBps"] = 4 * n / (med["sumsq"] * 1e-3) / 1e12
    out["adamw_TBps"] = ADAMW_BYTES[dtype] * n / (med["adamw"] * 1e-3) / 1e12
    out["adamw_clipped_TBps"] = ADAMW_BYTES[dtype] * n / (med["adamw_clipped"] * 1e-3) / 1e12
    out["sumsq_over_adamw"] = med["sumsq"] / med["adamw"]
    out["adamw_clipped_over_adamw"] = med["adamw_clipped"] / med["adamw"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    engine_mod, weights_mod, synth, config_mod, ops = (load(f"openvla-oft_amd.{m}") for m in ("engine", "weights", "synthetic", "config", "ops"))
    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="l1", has=has)
    del sd, get
    torch.cuda.empty_cache()
    names = ["vlm lora"] + [n for n, m in (("proprio projector", eng.proprio), ("noisy projector", eng.noisy), ("action head", eng.head)) if m is not None]
    for name, st in zip(names, eng.stores):
        for dt, flat in st.flat.items():
            r = time_kernels(ops, dev, name, dt, flat.numel(), args.reps)
            print(json.dumps(dict(metric="ovla_grad_sumsq (two launches) / ovla_adamw / ovla_adamw_clipped, alternated, HIP events (us, median)", **r)), flush=True)
    eng.enable_grad_clip(1.0)
    clip = eng._grad_clip
    coef_ms = [timed(lambda: ops.grad_clip_coef(clip["slots"], clip["state"], clip["max_norm"])) for _ in range(args.reps + 3)][3:]
    print(json.dumps(dict(metric="ovla_grad_clip_coef, one launch, HIP events (us, median)", n_slots=clip["slots"].numel(), coef_us=1e3 * float(np.median(coef_ms)),
                          coef_us_min_max=[1e3 * min(coef_ms), 1e3 * max(coef_ms)])), flush=True)

    def with_feature(on):
        eng._grad_clip = clip if on else None

    # the optimizer step alone: the gradients of one backward stay in place, the parameters move a little on every call
    for st in eng.stores:
        for g in st.flat_grad.values():
            g.normal_(0.0, 1e-3)
    step_ms = {False: [], True: []}
    for on in (False, True):
        with_feature(on)
        for _ in range(3):
            eng.adamw_step(5e-4)
    for _ in range(args.reps):
        for on in (False, True):
            with_feature(on)
            step_ms[on].append(timed(lambda: eng.adamw_step(5e-4)))
    off_med, on_med = float(np.median(step_ms[False])), float(np.median(step_ms[True]))
    print(json.dumps(dict(metric="VLAEngine.adamw_step, every store: feature off vs on, alternated, HIP events (us, median)", launches_off=len(clip["slots"]),
                          launches_on=3 * len(clip["slots"]) + 1, off_us=1e3 * off_med, on_us=1e3 * on_med, on_minus_off_us=1e3 * (on_med - off_med),
                          on_over_off=on_med / off_med, stats=eng.grad_clip_stats())), flush=True)
    if not args.no_step:
        try:
            batches = [synth.make_batch(args.batch, seed=1000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
                       for i in range(args.steps)]

            def block(on):
                with_feature(on)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in batches:
                    eng.train_step_fwd_bwd(b)
                    eng.adamw_step(5e-4)
                    eng.refresh_derived()
                    eng.zero_grad()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / len(batches)

            eng.zero_grad()
            block(False), block(True)
            off, on = [], []
            for _ in range(args.blocks):
                off.append(block(False))
                on.append(block(True))
            print(json.dumps(dict(metric="fine-tune step (fwd + bwd + AdamW + refresh), ms/step: clipping off vs on, alternated blocks (report only)", batch=args.batch,
                                  steps_per_block=args.steps, off_ms=off, on_ms=on, off_ms_median=float(np.median(off)), on_ms_median=float(np.median(on)),
                                  on_minus_off_ms=float(np.median(on) - np.median(off)), stats=eng.grad_clip_stats())), flush=True)
        except torch.cuda.OutOfMemoryError as e:
            print(json.dumps(dict(metric="fine-tune step with clipping on / off", skipped=f"does not fit: {e}"[:200])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
