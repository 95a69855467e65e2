"""What output_attentions costs at the full-size decoder shapes (S = 608, H = 32, head_dim 128; random OpenVLA-7B-shaped weights).

1. `ovla_attn_probs` per layer at B = 1 and B = 8: rows="actions" (56 rows per observation, head mean only) and rows="all" + per-head,
   each beside the time ITS OWN BYTES take at the copy rate measured in the same run.  Bytes, from the kernel's loads and stores: the listed
   Q rows (R H hd 2) + every K row of the batch (B S H hd 2) + lse (R H 4) + the row list (R 4) read, P (R H S 4) and / or P_mean (R S 4)
   written.  The copy rate is that of a device-to-device copy of the rows="all" variant's byte count (it reads n / 2 and writes n / 2);
   a copy of the rows="actions" variant's few MB is timed as well, because at that size a copy is a launch, not a stream.  All variants of
   one batch size are ALTERNATED in one process, every launch between its own pair of HIP events, after three untimed rounds.  The ratio
   kernel time / time of its bytes at the copy rate is reported; no threshold is set.
2. A batch-1 chunk (predict_action, merged LoRA, L1 head, eager) with and without output_attentions, alternated, host clock around calls
   that end in the device-to-host copy of the actions.
3. `--default-only`: part 2's flag-off leg alone, eager and under graph replay, using nothing this feature added -- the same file runs in a
   checkout of the parent commit, so the default path of both commits can be timed in alternating processes on one machine.

Usage: python tools/attn_probs_bench.py [--reps 30] [--chunks 20] [--no-chunk] [--default-only] >> profiles/attention_maps.jsonl"""
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
S, H, HD, A = 608, 32, 128, 56


def alternated(fns, reps):
    """{name: [ms per launch]}: three untimed rounds, then `reps` rounds of every variant in turn, each between its own event pair."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def kernel_part(ops, dev, B, reps):
    D = H * HD
    g = torch.Generator(device=dev).manual_seed(B)
    qkv = torch.randn(B * S, 3 * D, device=dev, generator=g).to(BF)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    _, lse = ops.attn_fwd(q, k, v, B, S, H, HD)
    rows = torch.cat([torch.arange(b * S + S - A - 2, b * S + S - 2, dtype=torch.int32) for b in range(B)]).to(dev)   # the rows in front of the slots
    R_act, R_all = rows.numel(), B * S
    mean_act = torch.empty(R_act, S, device=dev)
    P_all, mean_all = torch.empty(R_all, H, S, device=dev), torch.empty(R_all, S, device=dev)
    common = B * S * D * 2
    bytes_act = R_act * D * 2 + common + R_act * H * 4 + R_act * 4 + R_act * S * 4
    bytes_all = R_all * D * 2 + common + R_all * H * 4 + R_all * H * S * 4 + R_all * S * 4
    src = {n: torch.empty(nb // 2, dtype=torch.uint8, device=dev) for n, nb in (("act", bytes_act), ("all", bytes_all))}
    dst = {n: torch.empty_like(t) for n, t in src.items()}
    fns = {"actions_mean": lambda: ops.attn_probs(q, k, lse, B, S, H, HD, rows=rows, out=(None, mean_act)),
           "all_per_head": lambda: ops.attn_probs(q, k, lse, B, S, H, HD, out=(P_all, mean_all)),
           "copy_actions_bytes": lambda: dst["act"].copy_(src["act"]),
           "copy_all_bytes": lambda: dst["all"].copy_(src["all"])}
    ms = alternated(fns, reps)
    med = {n: float(np.median(x)) for n, x in ms.items()}
    rate = bytes_all / (med["copy_all_bytes"] * 1e-3)                                   # bytes / s of a streaming copy
    row = dict(metric="ovla_attn_probs per layer beside its bytes at the copy rate (us, median of alternated launches)", B=B, S=S, H=H, head_dim=HD,
               reps=reps, copy_rate_TBps=rate / 1e12)
    for name, nb, copy in (("actions_mean", bytes_act, "copy_actions_bytes"), ("all_per_head", bytes_all, "copy_all_bytes")):
        at_rate = nb / rate * 1e6
        row[name] = dict(rows=R_act if name == "actions_mean" else R_all, bytes=nb, us=1e3 * med[name], us_min_max=[1e3 * min(ms[name]), 1e3 * max(ms[name])],
                         bytes_at_copy_rate_us=at_rate, ratio_to_bytes_at_copy_rate=1e3 * med[name] / at_rate,
                         same_size_copy_us=1e3 * med[copy], ratio_to_same_size_copy=med[name] / med[copy])
    return row


def build_model(dev):
    weights_mod, config_mod, modeling = load("openvla-oft_amd.weights"), load("openvla-oft_amd.config"), load("openvla-oft_amd.modeling")
    cfg = config_mod.OPENVLA_7B
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=True)
    stats = {"libero": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    sub = lambda pre: {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}  # noqa: E731
    vla = modeling.OpenVLAForActionPrediction(cfg, {k: v for k, v in sd.items() if not k.startswith(("action_head.", "proprio_projector."))}, device=dev,
                                              norm_stats=stats)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=sub("action_head."))
    pp = modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=sub("proprio_projector."))
    del sd
    vla.merge_and_unload()
    g = torch.Generator().manual_seed(0)
    ids = torch.cat([torch.tensor([1]), torch.randint(3, 31000, (36,), generator=g), torch.tensor([29871])])[None]      # 38 prompt tokens: S = 608
    call = dict(input_ids=ids, attention_mask=torch.ones_like(ids, dtype=torch.bool), pixel_values=torch.randn(1, 12, 224, 224, generator=g).to(BF),
                unnorm_key="libero", proprio=np.zeros(8, np.float32), proprio_projector=pp, action_head=head)
    return vla, call


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--chunks", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--no-chunk", action="store_true")
    ap.add_argument("--default-only", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ops = load("openvla-oft_amd.ops")
    ops.check_device(0)
    if not args.default_only:
        for B in (1, 8):
            print(json.dumps(kernel_part(ops, dev, B, args.reps)), flush=True)
        if args.no_chunk:
            return 0
    vla, call = build_model(dev)
    plain = lambda: vla.predict_action(**call)  # noqa: E731
    if args.default_only:
        out = dict(metric="batch-1 chunk, default path (no output_attentions), ms per predict_action: blocks of calls in one process", tag=args.tag,
                   calls_per_block=args.chunks)
        for mode in ("eager", "graph"):
            vla.enable_graph_replay(mode == "graph")
            for _ in range(3):
                plain()
            out[mode + "_ms"] = [timed(plain, args.chunks) for _ in range(args.blocks)]
        vla.enable_graph_replay(False)
        print(json.dumps(out), flush=True)
        return 0
    flagged = lambda: vla.predict_action(**call, output_attentions=True)  # noqa: E731
    for _ in range(3):
        plain(), flagged()
    off, on = [], []
    for _ in range(args.blocks):
        off.append(timed(plain, args.chunks))
        on.append(timed(flagged, args.chunks))
    att = flagged()[2]
    print(json.dumps(dict(metric="batch-1 chunk, eager, ms per predict_action: output_attentions off vs on, alternated blocks", calls_per_block=args.chunks,
                          off_ms=off, on_ms=on, off_ms_median=float(np.median(off)), on_ms_median=float(np.median(on)),
                          on_minus_off_ms=float(np.median(on) - np.median(off)), layers=att.mean.shape[0], mean_shape=list(att.mean.shape),
                          mean_bytes=att.mean.numel() * 4)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
