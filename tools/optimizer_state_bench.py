"""fp32 optimizer state beside the torch-faithful bf16 state: ovla_adamw_master against ovla_adamw on flat buffers of the full-size bf16
trainable stores (OpenVLA-7B, LoRA r = 32, L1 head: the sizes are read from an engine of that configuration), the fine-tune step of
BASELINE.json configs[2] in both modes, and the two CPU demonstrations of what bf16 state loses.

Per buffer, in one process: warm-up, then `--reps` rounds of (ovla_adamw on bf16 state, ovla_adamw_master, ovla_adamw_master behind a clip
state), ALTERNATED, each between its own pair of HIP events.  The buffers are allocated for the measurement.  Bytes per element, from the
kernels' loads and stores: ovla_adamw on bf16 3 x 2 read + 4 read + 3 x 2 written = 16; ovla_adamw_master 4 + 3 x 4 read, 3 x 4 + 2 written = 30.
The expectation from bytes is master / bf16 = 30 / 16 = 1.875; `within_bound` says whether it stayed under 1.1 x that.
Then the whole fine-tune step (fwd + bwd + AdamW + refresh, host clock between two synchronisations), alternated in blocks between the two
modes of one engine (the tool swaps the state dictionaries; a training run chooses once).
`--cpu-demo` alone needs no GPU: 1024 parameters, N(0, 1) gradients for 1000 steps, then N(0, 0.1^2) for 5000 (median sqrt(v) at both points
and the step-size ratio), and p = 1 with a constant gradient at lr = 1e-4 (the published parameter after 40 steps), each with bf16 and fp32 state.
Usage: python tools/optimizer_state_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--no-step] [--cpu-demo] > profiles/optimizer_state_bench.jsonl"""
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
F32 = torch.float32
BYTES_BF16, BYTES_MASTER = 16, 30


def cpu_demo(seed=0):
    """The two defects with torch.optim.AdamW on the CPU (ovla_adamw's bf16 path reproduces it bit for bit), seeded."""
    out = {}
    for name, dtype in (("bf16", BF), ("fp32", F32)):
        g = torch.Generator().manual_seed(seed)
        p = torch.nn.Parameter(torch.zeros(1024, dtype=dtype))
        opt = torch.optim.AdamW([p], lr=1e-4, weight_decay=0.0)
        med = {}
        for k in range(1, 6001):
            p.grad = (torch.randn(1024, generator=g) * (1.0 if k <= 1000 else 0.1)).to(dtype)
            opt.step()
            if k in (1000, 6000):
                med[k] = float(opt.state[p]["exp_avg_sq"].float().sqrt().median())
        out[name] = med
    decay = dict(metric="median sqrt(exp_avg_sq) of 1024 parameters: N(0,1) gradients for 1000 steps, then N(0, 0.1^2) for 5000 (torch.optim.AdamW, CPU)", seed=seed,
                 bf16_step1000=out["bf16"][1000], bf16_step6000=out["bf16"][6000], fp32_step1000=out["fp32"][1000], fp32_step6000=out["fp32"][6000],
                 bf16_step_smaller_by=out["bf16"][6000] / out["fp32"][6000])
    lost = {}
    for name, dtype in (("bf16", BF), ("fp32", F32)):
        p = torch.nn.Parameter(torch.ones(1, dtype=dtype))
        opt = torch.optim.AdamW([p], lr=1e-4, weight_decay=0.0)
        first = None
        for k in range(1, 41):
            p.grad = torch.ones(1, dtype=dtype)
            opt.step()
            if first is None and float(p.detach().to(BF)) != 1.0:
                first = k
        lost[name] = dict(after_40_steps=float(p.detach()), published_bf16_first_leaves_1_at_step=first)
    return [decay, dict(metric="p = 1, constant gradient 1, lr = 1e-4, wd = 0 (torch.optim.AdamW, CPU)", **{f"{k}_{kk}": vv for k, v in lost.items() for kk, vv in v.items()})]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_kernels(ops, dev, name, n, reps):
    g = torch.Generator(device=dev).manual_seed(n % 9973)
    master = torch.randn(n, device=dev, generator=g) * 0.02
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    p_bf, m_bf, v_bf = master.to(BF), torch.zeros(n, dtype=BF, device=dev), torch.zeros(n, dtype=BF, device=dev)
    param, m, v = master.to(BF), torch.zeros_like(master), torch.zeros_like(master)
    slots = torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.zeros(ops.grad_sumsq_workspace_elems(n), dtype=torch.float64, device=dev)
    state = ops.grad_clip_state(dev)
    ops.grad_sumsq(grad, slots, 0, ws, is_bf16=False)
    ops.grad_clip_coef(slots, state, 1.0)          # a real coefficient below 1 for the launches behind the state
    step = [0]

    def run(which):
        step[0] += 1
        if which == "adamw_bf16":
            ops.adamw(p_bf, m_bf, v_bf, grad, step=step[0], lr=5e-4)
        else:
            ops.adamw_master(master, m, v, param, grad, step=step[0], lr=5e-4, clip_state=state if which == "master_clipped" else None)

    kinds = ("adamw_bf16", "master", "master_clipped")
    for k in kinds:
        for _ in range(3):
            run(k)
    ms = {k: [] for k in kinds}
    for _ in range(reps):
        for k in kinds:
            ms[k].append(timed(lambda: run(k)))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    out = dict(buffer=name, elements=n, coef_during_measurement=ops.read_grad_clip_state(state)["coef"])
    for k in kinds:
        out[f"{k}_us"] = 1e3 * med[k]
        out[f"{k}_us_min_max"] = [1e3 * min(ms[k]), 1e3 * max(ms[k])]
        out[f"{k}_TBps"] = (BYTES_BF16 if k == "adamw_bf16" else BYTES_MASTER) * n / (med[k] * 1e-3) / 1e12
    out["master_over_bf16"] = med["master"] / med["adamw_bf16"]
    out["master_clipped_over_bf16"] = med["master_clipped"] / med["adamw_bf16"]
    out["expected_from_bytes"] = BYTES_MASTER / BYTES_BF16
    out["within_bound"] = bool(max(med["master"], med["master_clipped"]) <= 1.1 * (BYTES_MASTER / BYTES_BF16) * med["adamw_bf16"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--cpu-demo", action="store_true", help="only the two CPU demonstrations (no GPU needed)")
    args = ap.parse_args()
    for row in cpu_demo():
        print(json.dumps(row), flush=True)
    if args.cpu_demo:
        return 0
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
        if BF in st.flat:
            r = time_kernels(ops, dev, name, st.flat[BF].numel(), args.reps)
            print(json.dumps(dict(metric="ovla_adamw (bf16 state) / ovla_adamw_master / ovla_adamw_master behind a clip state, alternated, HIP events (us, median)", **r)), flush=True)
    if args.no_step:
        return 0
    try:
        # both modes in one engine: the bf16 moments of the default mode are kept aside while fp32 mode runs, and the other way round
        for st in eng.stores:
            st.init_optimizer()
        param_state = [(dict(st.exp_avg), dict(st.exp_avg_sq)) for st in eng.stores]
        eng.enable_fp32_optimizer_state()
        fp32_state = [(dict(st.exp_avg), dict(st.exp_avg_sq), dict(st.master)) for st in eng.stores]

        def mode(fp32):
            for st, ps, fs in zip(eng.stores, param_state, fp32_state):
                st.fp32_state = fp32
                st.exp_avg, st.exp_avg_sq, st.master = (dict(fs[0]), dict(fs[1]), dict(fs[2])) if fp32 else (dict(ps[0]), dict(ps[1]), {})

        batches = [synth.make_batch(args.batch, seed=1000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
                   for i in range(args.steps)]

        def block(fp32):
            mode(fp32)
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
        print(json.dumps(dict(metric="fine-tune step (fwd + bwd + AdamW + refresh), ms/step: optimizer_state param vs fp32, alternated blocks (report only)", batch=args.batch,
                              steps_per_block=args.steps, param_ms=off, fp32_ms=on, param_ms_median=float(np.median(off)), fp32_ms_median=float(np.median(on)),
                              fp32_minus_param_ms=float(np.median(on) - np.median(off)), extra_bytes=eng.fp32_optimizer_state_bytes())), flush=True)
    except torch.cuda.OutOfMemoryError as e:
        print(json.dumps(dict(metric="fine-tune step, optimizer_state param vs fp32", skipped=f"does not fit: {e}"[:200])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
