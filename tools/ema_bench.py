"""ovla_ema_update against ovla_adamw on flat buffers of the full-size trainable stores (OpenVLA-7B, LoRA r = 32, L1 head + proprio projector:
the sizes are read from an engine of that configuration), and the fine-tune step with the EMA update on and off.

Per buffer, in one process: warm-up of both kernels, then `--reps` rounds of (one EMA launch, one AdamW launch), ALTERNATED, each launch
between its own pair of HIP events.  The buffers are allocated for the measurement (param, exp_avg, exp_avg_sq in the store's dtype, fp32
grad and shadow), so the engine's state is not touched.  Bytes per element, from the kernels' loads and stores: EMA 2 + 4 + 4 = 10 (bf16
parameter) or 4 + 4 + 4 = 12 (fp32); AdamW 3 x 2 read + 4 read + 3 x 2 written = 16 (bf16) or 3 x 4 + 4 + 3 x 4 = 28 (fp32).
THE CONDITION (exit status 1 if it fails): on each buffer the median EMA launch takes no longer than the median AdamW launch.
Report only (box-to-box spread of the step is +-3 %, no threshold): ms per step of fwd + bwd + AdamW + refresh with and without
ema_update, alternated in blocks of `--steps` steps; skipped with `--no-step` or when the step does not fit.
Usage: python tools/ema_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] > profiles/ema_bench.jsonl"""
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
BYTES = {("ema", BF): 10, ("ema", torch.float32): 12, ("adamw", BF): 16, ("adamw", torch.float32): 28}


def time_kernels(ops, dev, name, dtype, n, reps):
    g = torch.Generator(device=dev).manual_seed(n % 9973)
    param = (torch.randn(n, device=dev, generator=g) * 0.02).to(dtype)
    m, v = torch.zeros_like(param), torch.zeros_like(param)
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    shadow = param.float()
    step = [0]

    def adamw():
        step[0] += 1
        ops.adamw(param, m, v, grad, step=step[0], lr=5e-4)

    runs = {"ema": lambda: ops.ema_update(param, shadow, 1e-4), "adamw": adamw}
    for fn in runs.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    return dict(buffer=name, dtype="bf16" if dtype == BF else "f32", elements=n, ema_us=1e3 * med["ema"], adamw_us=1e3 * med["adamw"],
                ema_us_min_max=[1e3 * min(ms["ema"]), 1e3 * max(ms["ema"])], adamw_us_min_max=[1e3 * min(ms["adamw"]), 1e3 * max(ms["adamw"])],
                ema_TBps=BYTES["ema", dtype] * n / (med["ema"] * 1e-3) / 1e12, adamw_TBps=BYTES["adamw", dtype] * n / (med["adamw"] * 1e-3) / 1e12,
                ema_not_slower=med["ema"] <= med["adamw"])


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
    rows = [time_kernels(ops, dev, name, dt, flat.numel(), args.reps) for name, st in zip(names, eng.stores) for dt, flat in st.flat.items()]
    for r in rows:
        print(json.dumps(dict(metric="ovla_ema_update vs ovla_adamw, one launch each, alternated, HIP events (us, median)", **r)), flush=True)
    ok = all(r["ema_not_slower"] for r in rows)
    if not args.no_step:
        try:
            batches = [synth.make_batch(args.batch, seed=1000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
                       for i in range(args.steps)]
            eng.enable_ema()

            def block(ema):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in batches:
                    eng.train_step_fwd_bwd(b)
                    eng.adamw_step(5e-4)
                    if ema:
                        eng.ema_update(0.9999)
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
            print(json.dumps(dict(metric="fine-tune step (fwd + bwd + AdamW + refresh), ms/step: EMA off vs on, alternated blocks (report only)", batch=args.batch,
                                  steps_per_block=args.steps, off_ms=off, on_ms=on, off_ms_median=float(np.median(off)), on_ms_median=float(np.median(on)),
                                  on_minus_off_ms=float(np.median(on) - np.median(off)))), flush=True)
        except torch.cuda.OutOfMemoryError as e:
            print(json.dumps(dict(metric="fine-tune step with EMA on / off", skipped=f"does not fit: {e}"[:200])), flush=True)
    print(json.dumps(dict(metric="condition: on each buffer the EMA launch takes no longer than the AdamW launch", holds=ok)), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
