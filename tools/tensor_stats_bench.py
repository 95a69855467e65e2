"""Per-tensor statistics (ovla_tensor_stats) beside ovla_grad_sumsq on the flat trainable buffers of a full-size engine (OpenVLA-7B, LoRA
r = 32, L1 head + proprio projector), and the fine-tune step with a collection on every step against the step without the feature.

Per (store, dtype) buffer, in one process, on the engine's own buffers (both kernels only read them): warm-up, then `--reps` rounds of
    sumsq       ovla_grad_sumsq over the whole buffer (both of its launches)
    stats       ovla_tensor_stats over the buffer's segment table (both of its launches)
    per_tensor  one ovla_grad_sumsq pair per tensor of the table: the launch count the table-driven pair replaces
ALTERNATED, each between its own pair of HIP events.  Bytes per element, from the kernels' loads: sumsq 4 (the fp32 gradient); stats 4 + 2
(bf16 parameter) or 4 + 4 (fp32 parameter, or the fp32 master in fp32-state mode), so the bytes say 1.5x and 2x.  The partials are 8 (sumsq)
and 32 (stats) bytes per 8192 elements.  Then the whole fine-tune step (fwd + bwd + [collect] + AdamW + refresh, host clock between two
synchronisations) in alternated blocks without and with collect_tensor_stats on every step; "without" issues the launches the step issued
before the feature existed.  Everything is reported, nothing is a pass / fail condition.
Usage: python tools/tensor_stats_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--no-step] > profiles/tensor_stats_bench.jsonl"""
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_buffer(ops, eng, table, name, reps):
    st, dt, plan = table["store"], table["dtype"], table["plan"]
    ts = eng._tensor_stats
    grad, param = st.flat_grad[dt], st.master.get(dt, st.flat[dt])
    rounds = dt == BF and not st.fp32_state
    out = ts["out"][table["first"]: table["first"] + plan["n_segs"]]
    slots = torch.zeros(1, dtype=torch.float64, device=grad.device)
    ws = torch.zeros(ops.grad_sumsq_workspace_elems(grad.numel()), dtype=torch.float64, device=grad.device)
    views = [grad[o: o + n] for o, n in plan["segs_host"].tolist() if n > 0]

    def per_tensor():
        for v in views:
            ops.grad_sumsq(v, slots, 0, ws, is_bf16=rounds)

    runs = {"sumsq": lambda: ops.grad_sumsq(grad, slots, 0, ws, is_bf16=rounds),
            "stats": lambda: ops.tensor_stats(plan, grad, param, out, ts["partials"], grad_round_bf16=rounds),
            "per_tensor": per_tensor}
    for fn in runs.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    med = {k: float(np.median(x)) for k, x in ms.items()}
    elements = int(plan["segs_host"][:, 1].sum())
    param_bytes = 2 if param.dtype == BF else 4
    r = dict(buffer=name, param_dtype="bf16" if param.dtype == BF else "f32", buffer_elements=grad.numel(), segment_elements=elements,
             tensors=plan["n_segs"], chunks=plan["total_chunks"], sumsq_chunks=ops.grad_sumsq_workspace_elems(grad.numel()), bytes_ratio=(4 + param_bytes) / 4)
    for k in runs:
        r[f"{k}_us"] = 1e3 * med[k]
        r[f"{k}_us_min_max"] = [1e3 * min(ms[k]), 1e3 * max(ms[k])]
    r["sumsq_TBps"] = 4 * grad.numel() / (med["sumsq"] * 1e-3) / 1e12
    r["stats_TBps"] = (4 + param_bytes) * elements / (med["stats"] * 1e-3) / 1e12
    r["stats_over_sumsq"] = med["stats"] / med["sumsq"]
    r["per_tensor_over_stats"] = med["per_tensor"] / med["stats"]
    r["per_tensor_launches"] = 2 * len(views)
    return r


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
    eng.enable_tensor_stats()
    for st in eng.stores:
        for g in st.flat_grad.values():
            g.normal_(0.0, 1e-3)
    names = ["vlm lora"] + [n for n, m in (("proprio projector", eng.proprio), ("noisy projector", eng.noisy), ("action head", eng.head)) if m is not None]
    store_name = {id(st): n for n, st in zip(names, eng.stores)}
    for table in eng._tensor_stats["tables"]:
        r = time_buffer(ops, eng, table, store_name[id(table["store"])], args.reps)
        print(json.dumps(dict(metric="ovla_grad_sumsq / ovla_tensor_stats / one ovla_grad_sumsq per tensor, alternated, HIP events (us, median)", **r)), flush=True)
    collect_ms = [timed(eng.collect_tensor_stats) for _ in range(args.reps + 3)][3:]
    t0 = time.perf_counter()
    table = eng.tensor_stats()
    readback_ms = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(dict(metric="VLAEngine.collect_tensor_stats, every buffer, HIP events (us, median); tensor_stats() readback, host clock (ms, one call)",
                          launches=2 * len(eng._tensor_stats["tables"]), tensors=len(table), collect_us=1e3 * float(np.median(collect_ms)),
                          collect_us_min_max=[1e3 * min(collect_ms), 1e3 * max(collect_ms)], readback_ms=readback_ms)), flush=True)
    if not args.no_step:
        try:
            batches = [synth.make_batch(args.batch, seed=1000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
                       for i in range(args.steps)]

            def block(on):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in batches:
                    eng.train_step_fwd_bwd(b)
                    if on:
                        eng.collect_tensor_stats()
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
            print(json.dumps(dict(metric="fine-tune step (fwd + bwd + AdamW + refresh), ms/step: no collection vs collect_tensor_stats on every step, alternated blocks (report only)",
                                  batch=args.batch, steps_per_block=args.steps, off_ms=off, on_ms=on, off_ms_median=float(np.median(off)),
                                  on_ms_median=float(np.median(on)), on_minus_off_ms=float(np.median(on) - np.median(off)),
                                  first_nonfinite=eng.first_nonfinite())), flush=True)
        except torch.cuda.OutOfMemoryError as e:
            print(json.dumps(dict(metric="fine-tune step with and without the collection", skipped=f"does not fit: {e}"[:200])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
