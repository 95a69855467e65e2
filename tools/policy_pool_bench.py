"""The policy pool at OpenVLA-7B shapes, on synthetic adapters, L1 heads and proprio projectors: what one slot swap costs and what it does to
serving throughput.  One process; the variants of every comparison alternate inside it (A B A B ...), one JSON line per measurement.

  (a) swap     one policy into one slot: the ovla_copy_table launch (engine.load_slot) against the method it replaces -- engine.fill_slot per
               adapted linear plus one copy_ per head / projector buffer into the same storage, fed from DEVICE tensors (the loop at its
               best: add_policy's own loop starts from host tensors).  Host time = enqueue only (perf_counter around the calls, device idle
               before); device time = hip events around the calls; end to end = enqueue + synchronize.
  (b) rate     bytes/s of the launch against ONE contiguous torch device-to-device copy of the same byte count, for the whole policy and per
               entry kind: lora_A row groups, lora_B 64-byte segments at a 256-byte stride, flat head / projector buffers.
  (c) serving  closed loop, predict_action_batch at B = 8 under graph replay: batches that alternate between two sets of 4 policies at
               resident = 4 (every forward swaps all four slots) against batches of one set (no swaps), chunks/s.

Usage: python tools/policy_pool_bench.py [--reps 10] [--iters 10] [--tiny] > profiles/policy_pool.jsonl"""
import argparse
import importlib
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module
BF = torch.bfloat16
UNNORM = "synthetic"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--policies", type=int, default=8)
    ap.add_argument("--tiny", action="store_true", help="the tests' tiny configuration (a functional check of this tool, not a measurement)")
    args = ap.parse_args()
    ops, engine_mod, weights_mod, synth, config_mod, modeling = (load(f"openvla-oft_amd.{m}") for m in ("ops", "engine", "weights", "synthetic", "config", "modeling"))
    dev = torch.device("cuda:0")
    if args.tiny:
        from oracle import vla_oracle as vo

        cfg, image = config_mod.VLAConfig.from_any(vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)), 56
    else:
        cfg, image = config_mod.OPENVLA_7B, 224
    stats = {UNNORM: {"action": {"q01": [-1.0] * cfg.action_dim, "q99": [1.0] * cfg.action_dim}}}
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=False)
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, lora=False, norm_stats=stats)
    del sd
    eng = vla.engine
    vla.enable_policy_pool(4)
    linears = [l for l in eng.vlm_linears() if isinstance(l, engine_mod.LoraLinear)]
    r, D = cfg.lora_rank, cfg.llm_dim
    names = [f"p{k}" for k in range(args.policies)]
    g = torch.Generator(device=dev)
    for k, nm in enumerate(names):
        g.manual_seed(100 + k)
        lora = {}
        for l in linears:
            for rn in l.ref_names:
                lora[rn + ".lora_A.weight"] = (torch.randn(r, l.in_f, generator=g, device=dev) * 0.02).to(BF)
                lora[rn + ".lora_B.weight"] = (torch.randn(l.group_n, r, generator=g, device=dev) * 0.02).to(BF)
        vla.add_policy(nm, lora, action_head=modeling.L1RegressionActionHead(D, D, cfg.action_dim, num_actions_chunk=cfg.chunk, device=dev, seed=k),
                       proprio_projector=modeling.ProprioProjector(D, cfg.proprio_dim, device=dev, seed=k))
        del lora
    torch.cuda.synchronize()
    print(json.dumps(dict(what="pool", config="tiny" if args.tiny else "7b", policies=len(names), resident=4, policy_pool_bytes=vla.policy_pool_bytes,
                          bytes_per_policy=vla.policy_pool_bytes // len(names), adapted_linears=len(linears))), flush=True)

    def measure(fn):
        """-> (host enqueue ms, device ms between hip events, end-to-end ms) of one call on an idle device."""
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return 1e3 * (t1 - t0), e0.elapsed_time(e1), 1e3 * (t2 - t0)

    def alternate(variants, reps):
        """{name: fn} run A B A B ... (after one untimed round) -> {name: medians of (host, device, end to end)}."""
        for fn in variants.values():
            fn()
        samples = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                samples[k].append(measure(fn))
        return {k: [statistics.median(c) for c in zip(*v)] for k, v in samples.items()}

    # ---- (a) one policy swap ---------------------------------------------------------------------------------------------------------------
    slot, name = 1, names[-1]
    pairs = eng.pool_slot_pairs(slot, name)
    extra = eng.pool[name]["slot_pairs"](slot)
    tab = eng.load_slot(slot, name)

    def loop():
        for l in eng._pool_linears:
            A, Bm = eng.pool[name]["tensors"][l.name]
            engine_mod.fill_slot(l.A_slots, l.B_slots, slot, A, Bm, l.groups)
        for src, dst in extra:
            dst.copy_(src)

    res = alternate({"table": lambda: eng.load_slot(slot, name), "loop": loop}, args.reps)
    n_copies = sum(l.groups + 1 for l in eng._pool_linears) + len(extra)
    for k, (host, devt, e2e) in res.items():
        print(json.dumps(dict(what="swap", variant=k, bytes=tab["nbytes"], launches=1 if k == "table" else n_copies, entries=tab["n"], tiles=tab["total"],
                              host_ms=host, device_ms=devt, end_to_end_ms=e2e, device_GBps=tab["nbytes"] / devt / 1e6)), flush=True)

    # ---- (b) copy rate by entry kind -------------------------------------------------------------------------------------------------------
    n_adapter = len(pairs) - len(extra)
    kinds = {"all": pairs, "lora_A rows": [p for p in pairs[:n_adapter] if p[1].is_contiguous()], "lora_B 64-byte segments": [p for p in pairs[:n_adapter] if not p[1].is_contiguous()],
             "flat buffers": extra}
    for kind, sel in kinds.items():
        if not sel:
            continue
        t = ops.copy_table_build([ops.copy_entry(a, b) for a, b in sel], dev, keep=sel)
        src = torch.empty(t["nbytes"], dtype=torch.uint8, device=dev).random_(0, 256)
        dst = torch.empty_like(src)
        res = alternate({"table": lambda t=t: ops.copy_table(t), "torch": lambda: dst.copy_(src)}, args.reps)
        print(json.dumps(dict(what="rate", kind=kind, entries=t["n"], tiles=t["total"], bytes=t["nbytes"], table_device_ms=res["table"][1], torch_device_ms=res["torch"][1],
                              table_GBps=t["nbytes"] / res["table"][1] / 1e6, torch_GBps=t["nbytes"] / res["torch"][1] / 1e6,
                              table_over_torch=res["torch"][1] / res["table"][1])), flush=True)
        del src, dst, t

    # ---- (c) serving throughput ------------------------------------------------------------------------------------------------------------
    B = 8
    b = synth.make_batch(B, seed=77, prompt_lens=[(11, 17, 9, 14)[i % 4] for i in range(B)], num_images=cfg.num_images, chunk=cfg.chunk,
                         action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim, image_size=image)
    A = cfg.num_action_tokens
    prompts = [(b["input_ids"][i][: int(b["attention_mask"][i].sum()) - A - 1], None) for i in range(B)]
    pv, proprio = b["pixel_values"].to(dev, BF), b["proprio"].reshape(B, -1).numpy()
    sets = [[names[(4 * s + j % 4) % len(names)] for j in range(B)] for s in range(2)]
    vla.enable_graph_replay(True)

    def serve(policy_lists, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(iters):
            vla.predict_action_batch(prompts, pv, unnorm_key=UNNORM, proprio=proprio, policy=policy_lists[i % len(policy_lists)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    serve(sets, 2)   # captures the (B, L) graph, fills the tables of both sets
    rounds = {"4 policies, no swaps": [], "8 policies, 4 swaps per forward": []}
    for _ in range(3):
        serve([sets[0]], 1)
        before = vla.policy_pool_stats["loads"]
        rounds["4 policies, no swaps"].append(serve([sets[0]], args.iters))
        assert vla.policy_pool_stats["loads"] == before
        rounds["8 policies, 4 swaps per forward"].append(serve(sets, args.iters))
        assert vla.policy_pool_stats["loads"] - before >= 4 * (args.iters - 1)
    for k, v in rounds.items():
        ms = 1e3 * statistics.median(v)
        print(json.dumps(dict(what="serving", variant=k, B=B, ms_per_forward=ms, chunks_per_s=B / ms * 1e3, rounds_ms=[1e3 * x for x in v])), flush=True)
    print(json.dumps(dict(what="stats", **vla.policy_pool_stats)), flush=True)


if __name__ == "__main__":
    main()
