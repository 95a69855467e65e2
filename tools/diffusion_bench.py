"""The diffusion head's sampler at full size (BASELINE.json configs[5]: OpenVLA-7B shapes, FiLM, 3 images, chunk 25 x 14, 50 DDIM steps;
synthetic weights, merged + RMSNorm-folded decoder): ms per chunk and chunks/s of predict_action_batch with the host loop (graph replay off:
per step ~1.3 k eager launches, a device sync, the scheduler step in CPU torch, an upload) and with engine.DiffusionGraph (graph replay on),
at B = 1 and B = 8.  The two are ALTERNATED in one process, `--reps` rounds each; one JSON line per batch size with every round's time, so
that the alternation's own run-to-run spread can be read beside the difference; the first graphed call (capture) is not timed.  Also checks
that both paths returned the same bits.  Usage: python tools/diffusion_bench.py [--batches 1,8] [--reps 3] [--steps 50] > profiles/diffusion_bench.jsonl"""
import argparse
import dataclasses
import importlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    weights_mod, config_mod, modeling = (load(f"openvla-oft_amd.{m}") for m in ("weights", "config", "modeling"))
    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(config_mod.OPENVLA_7B, num_images=3, chunk=25, action_dim=14, proprio_dim=14)   # ALOHA constants
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=False, film=True, diffusion=True)
    stats = {"aloha": {"action": {"q01": [-1.0] * 14, "q99": [1.0] * 14, "mask": [True] * 14}}}
    sub = lambda pre: {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}  # noqa: E731
    vla = modeling.OpenVLAForActionPrediction(cfg, {k: v for k, v in sd.items() if not k.startswith(("action_head.", "proprio_projector.", "noisy_action_projector."))},
                                              device=dev, norm_stats=stats, lora=False, use_film=True)
    head = modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, cfg.action_dim, num_diffusion_steps=args.steps, num_actions_chunk=cfg.chunk, device=dev,
                                        state_dict=sub("action_head."))
    pp = modeling.ProprioProjector(cfg.llm_dim, cfg.proprio_dim, device=dev, state_dict=sub("proprio_projector."))
    nap = modeling.NoisyActionProjector(cfg.llm_dim, device=dev, state_dict=sub("noisy_action_projector."))
    del sd
    vla.merge_and_unload()
    gen = torch.Generator().manual_seed(1)

    def run(B, inputs, graph):
        vla.use_graph = graph   # (not enable_graph_replay(False): that would drop the captured graphs between the alternated rounds)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, h = vla.predict_action_batch(inputs["prompts"], inputs["pv"], unnorm_key="aloha", proprio=inputs["proprio"], proprio_projector=pp, action_head=head,
                                        noisy_action_projector=nap, use_film=True, noise=inputs["noise"])
        torch.cuda.synchronize()
        return time.perf_counter() - t0, a, h.clone()

    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        lens = [(11, 17, 9, 14)[i % 4] for i in range(B)]
        inputs = dict(prompts=[(torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=gen)]), None) for n in lens],
                      pv=torch.randn(B, 6 * cfg.num_images, 224, 224, generator=gen).to(dev, torch.bfloat16),
                      proprio=(torch.rand(B, cfg.proprio_dim, generator=gen) * 2 - 1).numpy(), noise=torch.randn(B, cfg.chunk, cfg.action_dim, generator=gen))
        _, a_h, h_h = run(B, inputs, False)     # warm-ups: lazy tables, kernel attributes; the graphs' capture
        _, a_g, h_g = run(B, inputs, True)
        same = bool(np.array_equal(a_h, a_g) and torch.equal(h_h, h_g))
        host, graph = [], []
        for _ in range(args.reps):
            host.append(run(B, inputs, False)[0])
            graph.append(run(B, inputs, True)[0])
        med = lambda v: float(np.median(v))  # noqa: E731
        row = dict(B=B, steps=args.steps, chunk=cfg.chunk, action_dim=cfg.action_dim, num_images=cfg.num_images, film=True, same_bits=same,
                   host_ms=[1e3 * t for t in host], graph_ms=[1e3 * t for t in graph], host_ms_median=1e3 * med(host), graph_ms_median=1e3 * med(graph),
                   host_chunks_per_s=B / med(host), graph_chunks_per_s=B / med(graph), graph_speedup=med(host) / med(graph))
        rows.append(row)
        print(json.dumps(row), flush=True)
        vla.enable_graph_replay(False)          # drop this batch size's graphs before the next
        torch.cuda.empty_cache()
    print(json.dumps(dict(metric="DDIM sampling, ms per chunk batch: host loop vs graph replay (predict_action_batch, FiLM + diffusion, 3 images, 25 x 14)",
                          **{f"b{r['B']}_{k}": r[k] for r in rows for k in ("host_ms_median", "graph_ms_median", "graph_speedup", "same_bits")})), flush=True)


if __name__ == "__main__":
    main()
