"""Batched action-chunk inference at OpenVLA-7B shapes (merged decoder, RMSNorm folded, L1 head): chunks/s of the batch-1 graph path that
predict_action replays, against the batched forward that predict_action_batch runs -- B = 1, 2, 4, 8, 16, eager and hipGraph, with the fixed
GEMM schedules (OVLA_BATCH_INVARIANT=1, the default) and with the planner's own (0).  One process, one JSON line per configuration;
the last line summarises.  Engine level: ChunkGraph replays and engine.forward -- the device work of predict_action (batch 1, graph) and
predict_action_batch -- without the API's host-side prompt assembly and unnormalisation on either side.  Usage: python tools/batch_infer_bench.py [--batches 1,2,4,8,16] [--reps 10] > profiles/batch_infer_bench.jsonl"""
import argparse
import importlib
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    ops, engine_mod, weights_mod, synth, config_mod = (load(f"openvla-oft_amd.{m}") for m in ("ops", "engine", "weights", "synthetic", "config"))
    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=False)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=False, use_proprio=True, head="l1", has=has)
    del sd, get
    eng.llm.fold_norms()

    def batch(B):
        lens = [(11, 17, 9, 14)[i % 4] for i in range(B)]   # mixed prompt lengths, right-padded to the longest
        b = synth.make_batch(B, seed=77, prompt_lens=lens, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
        b["pixel_values"] = b["pixel_values"].to(dev, torch.bfloat16)
        b["proprio"] = b["proprio"].to(dev, torch.bfloat16).reshape(B, -1)
        return b

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        b = batch(B)
        inputs = (b["input_ids"], b["attention_mask"], b["pixel_values"], b["labels"], b["proprio"])
        for invariant in (True, False):
            g = engine_mod.ChunkGraph(eng, B, b["input_ids"].shape[1], b["pixel_values"].shape, head=eng.head, use_proprio=True, invariant=invariant)
            t_graph = timed(lambda: g(*inputs), args.reps)

            def eager():
                with ops.batch_invariant(invariant):
                    out = eng.forward(b["input_ids"], b["attention_mask"], b["pixel_values"], b["labels"], proprio=b["proprio"], train=False, sel="actions")
                    ah, _ = eng.action_hidden(out)
                    return eng.head.fwd(ah)[0]

            t_eager = timed(eager, max(3, args.reps // 2))
            row = dict(B=B, L=int(b["input_ids"].shape[1]), invariant=invariant, graph_ms=1e3 * t_graph, eager_ms=1e3 * t_eager,
                       graph_chunks_per_s=B / t_graph, eager_chunks_per_s=B / t_eager)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del g
            torch.cuda.empty_cache()
    base = next(r for r in rows if r["B"] == 1 and not r["invariant"])   # = predict_action's graph path (planner schedules, batch 1)
    best8 = [r for r in rows if r["B"] == 8 and r["invariant"]]
    summary = dict(metric="batched inference chunks/s, OpenVLA-7B merged + folded, L1 head", batch1_graph_chunks_per_s=base["graph_chunks_per_s"])
    if best8:
        summary.update(b8_invariant_graph_chunks_per_s=best8[0]["graph_chunks_per_s"], b8_over_batch1=best8[0]["graph_chunks_per_s"] / base["graph_chunks_per_s"])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
