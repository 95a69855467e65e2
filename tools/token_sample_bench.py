"""Stochastic action-token decoding and the policy-gradient step at full size (OpenVLA-7B, LoRA r = 32, discrete token path), each against what
it stands beside, ALTERNATED in one process.  Everything is reported, nothing is a pass / fail condition.

  kernels   ovla_argmax_bins / ovla_sample_tokens and ovla_token_ce / ovla_token_pg on bf16 logits [batch * 56, 32064], each between its own
            pair of HIP events (us, median).  A chunk's logits are batch * 56 * 32064 * 2 bytes (3.6 MB at batch 1).
  chunk     the batched discrete ChunkGraph (fixed GEMM schedules, lm_head + decode inside the graph) with the greedy decode and with
            sample=(temperature, action window): one replay each between HIP events, alternated.
  step      VLAEngine.train_step_discrete and VLAEngine.train_step_policy_gradient (fwd + bwd, gradients accumulate), host clock between two
            synchronisations, alternated blocks.
Usage: python tools/token_sample_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--no-step] > profiles/token_sample_bench.jsonl"""
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


def alternate(runs, reps, warm=3):
    for fn in runs.values():
        for _ in range(warm):
            fn()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    return {k: dict(us=1e3 * float(np.median(v)), us_min_max=[1e3 * min(v), 1e3 * max(v)]) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    engine_mod, weights_mod, synth, config_mod, ops, _lib = (load(f"openvla-oft_amd.{m}") for m in ("engine", "weights", "synthetic", "config", "ops", "_lib"))
    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    print(json.dumps(dict(metric="build", device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), torch=torch.__version__, batch=args.batch)), flush=True)
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=True)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="none", has=has)
    del sd, get
    torch.cuda.empty_cache()
    A, B = cfg.num_action_tokens, args.batch
    window = eng.token_window("actions")
    n_tokens, n_bins = cfg.vocab - cfg.pad_to_multiple_of, cfg.n_action_bins - 1

    # -- the kernels on a chunk's logits ---------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    for rows in sorted({A, B * A}):
        logits = torch.randn(rows, cfg.vocab, device=dev, generator=g).to(BF)
        tok = torch.randint(window[0], window[1], (rows,), device=dev, generator=g).to(torch.int32)
        tgt, adv, scratch = tok.to(torch.int64), torch.ones(rows, device=dev), torch.empty_like(logits)
        res = alternate({
            "argmax_bins": lambda: ops.argmax_bins(logits, n_tokens=n_tokens, n_bins=n_bins),
            "sample_tokens_actions": lambda: ops.sample_tokens(logits, n_tokens=n_tokens, n_bins=n_bins, window=window, temperature=args.temperature, seed=1, call=2),
            "sample_tokens_vocab": lambda: ops.sample_tokens(logits, n_tokens=n_tokens, n_bins=n_bins, temperature=args.temperature, seed=1, call=2),
            "token_ce": lambda: ops.token_ce(logits, tgt, grad_scale=1.0 / rows, dlogits=scratch),
            "token_pg_actions": lambda: ops.token_pg(logits, tok, adv, window=window, temperature=args.temperature, grad_scale=1.0 / rows, dlogits=scratch),
            "token_pg_vocab": lambda: ops.token_pg(logits, tok, adv, temperature=args.temperature, grad_scale=1.0 / rows, dlogits=scratch),
        }, args.reps)
        print(json.dumps(dict(metric="token kernels on bf16 logits [rows, vocab], alternated, HIP events (us, median)", rows=rows, vocab=cfg.vocab,
                              logits_MB=rows * cfg.vocab * 2 / 1e6, window=list(window), **res)), flush=True)
        del logits, scratch

    # -- the batched discrete chunk under graph replay: greedy against sampled -----------------------------------------------------------------
    batch = synth.make_batch(B, seed=1000, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
    L = batch["input_ids"].shape[1]
    graphs = {}
    with torch.no_grad():
        for name, sample in (("greedy", None), ("sampled", (args.temperature, window))):
            gr = engine_mod.ChunkGraph(eng, B, L, batch["pixel_values"].shape, discrete=True, invariant=ops.BATCH_INVARIANT_DEFAULT, sample=sample)
            kw = {} if sample is None else dict(sample_state=eng.token_sample.words(7))
            gr.load(batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["labels"], batch["proprio"], **kw)
            gr.capture()
            graphs[name] = gr
        res = alternate({k: gr.replay for k, gr in graphs.items()}, args.reps)
    print(json.dumps(dict(metric="batched discrete chunk, one graph replay: greedy decode vs sample=(T, action window), alternated, HIP events (us, median)", batch=B,
                          temperature=args.temperature, sampled_minus_greedy_us=res["sampled"]["us"] - res["greedy"]["us"],
                          sampled_over_greedy=res["sampled"]["us"] / res["greedy"]["us"], **res)), flush=True)
    del graphs
    torch.cuda.empty_cache()

    # -- the training step: next-token cross entropy against the clipped policy gradient ----------------------------------------------------------
    if not args.no_step:
        try:
            batches = [synth.make_batch(B, seed=2000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
                       for i in range(args.steps)]
            draws = [eng.sample_action_tokens(b, temperature=args.temperature) for b in batches]
            advs = [torch.randn(B, device=dev) for _ in batches]

            def block(pg):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b, d, a in zip(batches, draws, advs):
                    if pg:
                        eng.train_step_policy_gradient(b, d["tokens"], a, old_logprobs=d["logprob"], temperature=args.temperature)
                    else:
                        eng.train_step_discrete(b)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0) / len(batches)

            eng.zero_grad()
            block(False), block(True)
            ce, pg = [], []
            for _ in range(args.blocks):
                ce.append(block(False))
                pg.append(block(True))
            print(json.dumps(dict(metric="training step (fwd + bwd), ms/step: train_step_discrete vs train_step_policy_gradient, alternated blocks (report only)",
                                  batch=B, steps_per_block=args.steps, discrete_ms=ce, policy_gradient_ms=pg, discrete_ms_median=float(np.median(ce)),
                                  policy_gradient_ms_median=float(np.median(pg)), pg_minus_discrete_ms=float(np.median(pg) - np.median(ce)),
                                  rows_discrete=B * (A + 1), rows_policy_gradient=B * A)), flush=True)
        except torch.cuda.OutOfMemoryError as e:
            print(json.dumps(dict(metric="training step, discrete vs policy gradient", skipped=f"does not fit: {e}"[:200])), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
