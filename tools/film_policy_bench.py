"""Per-policy FiLM at OpenVLA-7B shapes, on synthetic weights: what the one routed launch costs against the launches it stands in for, what it
does to serving throughput, and what a FiLM policy adds to a slot swap.  One process; the variants of every comparison alternate inside it
(A B A B ..., one untimed round first), one JSON line per measurement.  Device time is the distance of two hip events around `inner`
consecutive calls, divided by `inner`; the weights of one slot (0.88 GB) exceed every cache, so consecutive calls stream from HBM.

  (a) launch   ovla_film_vectors for 8 observations (all 98 FiLM Linears of both towers) with 1, 2 and 4 distinct slots in use.
  (b) linears  the 98 FullLinear.fwd launches (M = 8 GEMMs under the batch path's fixed schedules) that a use_film=True engine issues for the
               same 8 observations: the single-policy path, the comparator.
  (c) serving  closed loop, predict_action_batch at B = 8 under graph replay: four FiLM policies mixed (pool, resident = 4, no swaps) against
               a single model with its own FiLM Linears, and against four policies without FiLM (what the routed launch adds to multi-policy
               serving).
  (d) swap     one policy into one slot (engine.load_slot: one ovla_copy_table launch) with and without FiLM tensors.

Usage: python tools/film_policy_bench.py [--reps 10] [--inner 10] [--iters 10] [--tiny] > profiles/film_policies.jsonl"""
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
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tiny", action="store_true", help="the tests' tiny configuration (a functional check of this tool, not a measurement)")
    args = ap.parse_args()
    ops, engine_mod, weights_mod, synth, config_mod, modeling = (load(f"openvla-oft_amd.{m}") for m in ("ops", "engine", "weights", "synthetic", "config", "modeling"))
    dev = torch.device("cuda:0")
    if args.tiny:
        from oracle import vla_oracle as vo

        cfg, image = config_mod.VLAConfig.from_any(vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)), 56
    else:
        cfg, image = config_mod.OPENVLA_7B, 224
    D, r, B = cfg.llm_dim, cfg.lora_rank, 8
    stats = {UNNORM: {"action": {"q01": [-1.0] * cfg.action_dim, "q99": [1.0] * cfg.action_dim}}}
    towers = [("vision_backbone.featurizer.", cfg.dino.depth - 1, cfg.dino.dim), ("vision_backbone.fused_featurizer.", cfg.siglip.depth - 1, cfg.siglip.dim)]
    film_names = engine_mod.film_linear_names(towers)
    dims = {nm: dim for prefix, blocks, dim in towers for nm in engine_mod.film_linear_names([(prefix, blocks, dim)])}
    g = torch.Generator(device=dev)

    def film_tensors(seed):
        g.manual_seed(seed)
        out = {}
        for nm in film_names:
            out[nm + ".weight"] = (torch.randn(dims[nm], D, generator=g, device=dev) * 0.03).to(BF)
            out[nm + ".bias"] = (torch.randn(dims[nm], generator=g, device=dev) * 0.02).to(BF)
        return out

    def alternate(variants, reps, inner):
        """{name: fn} run A B A B ... (after one untimed round) -> {name: median device ms of one call}."""
        for fn in variants.values():
            fn()
        samples = {k: [] for k in variants}
        for _ in range(reps):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                samples[k].append(e0.elapsed_time(e1) / inner)
        return {k: statistics.median(v) for k, v in samples.items()}

    # ---- (a) + (b): the routed launch against the 98 Linear launches -------------------------------------------------------------------------
    slots = engine_mod.FilmSlots(towers, 4, D, dev)
    for s in range(4):
        slots.set_slot(s, film_tensors(10 + s))
    store = engine_mod.ParamStore(dev)
    own = film_tensors(10)
    linears = [engine_mod.FullLinear(store, nm, own[nm + ".weight"].float(), own[nm + ".bias"].float(), master_fp32=True) for nm in film_names]
    store.finalize()
    for lin in linears:
        lin.refresh_derived()
    del own
    avg = (torch.randn(B, D, generator=g, device=dev) * 0.1).to(BF)
    assigns = {1: [0] * B, 2: [b % 2 for b in range(B)], 4: [b % 4 for b in range(B)]}
    obs = {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in assigns.items()}
    slot_bytes = sum(2 * (dims[nm] * D + dims[nm]) for nm in film_names)

    def linears_fwd():
        with ops.batch_invariant(ops.BATCH_INVARIANT_DEFAULT):
            for lin in linears:
                lin.fwd(avg)

    variants = {f"launch_{k}_slots": (lambda k=k: ops.film_vectors(slots.table, avg, obs[k], host_slots=assigns[k])) for k in assigns}
    variants["linears_98"] = linears_fwd
    res = alternate(variants, args.reps, args.inner)
    # same inputs, slot 0: the launch against the Linears (summation orders differ: compared under the kernel test's bound, printed only)
    ops.film_vectors(slots.table, avg, obs[1], host_slots=assigns[1])
    worst = max(float((slots.out[nm][:B].float() - lin.fwd(avg)[0].float()).abs().max()) for nm, lin in zip(film_names, linears))
    torch.cuda.synchronize()
    for k in assigns:
        ms = res[f"launch_{k}_slots"]
        print(json.dumps(dict(what="launch", slots_used=k, B=B, linears=len(film_names), launches=1, device_ms=ms, bytes_streamed=k * slot_bytes,
                              GBps=k * slot_bytes / ms / 1e6, ms_per_used_slot=ms / k)), flush=True)
    print(json.dumps(dict(what="linears", B=B, launches=len(linears), device_ms=res["linears_98"], bytes_streamed=slot_bytes,
                          GBps=slot_bytes / res["linears_98"] / 1e6, max_abs_diff_to_launch=worst)), flush=True)
    del slots, linears, store
    torch.cuda.empty_cache()

    # ---- (c) + (d): serving and the slot swap -----------------------------------------------------------------------------------------------
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=False)
    n_pol = 5

    def pooled(film: bool):
        vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, lora=False, norm_stats=stats, use_film="per_policy" if film else False)
        vla.enable_policy_pool(4)
        lins = [l for l in vla.engine.vlm_linears() if isinstance(l, engine_mod.LoraLinear)]
        for k in range(n_pol):
            g.manual_seed(100 + k)
            lora = {}
            for l in lins:
                for rn in l.ref_names:
                    lora[rn + ".lora_A.weight"] = (torch.randn(r, l.in_f, generator=g, device=dev) * 0.02).to(BF)
                    lora[rn + ".lora_B.weight"] = (torch.randn(l.group_n, r, generator=g, device=dev) * 0.02).to(BF)
            vla.add_policy(f"p{k}", lora, action_head=modeling.L1RegressionActionHead(D, D, cfg.action_dim, num_actions_chunk=cfg.chunk, device=dev, seed=k),
                           proprio_projector=modeling.ProprioProjector(D, cfg.proprio_dim, device=dev, seed=k), film=film_tensors(200 + k) if film else None)
            del lora
        return vla

    multi_film, multi_plain = pooled(True), pooled(False)
    single = modeling.OpenVLAForActionPrediction(cfg, {**sd, **film_tensors(200)}, device=dev, lora=False, norm_stats=stats, use_film=True)
    head, pp = modeling.L1RegressionActionHead(D, D, cfg.action_dim, num_actions_chunk=cfg.chunk, device=dev, seed=0), modeling.ProprioProjector(D, cfg.proprio_dim, device=dev, seed=0)
    del sd
    b = synth.make_batch(B, seed=77, prompt_lens=[(11, 17, 9, 14)[i % 4] for i in range(B)], num_images=cfg.num_images, chunk=cfg.chunk,
                         action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim, image_size=image)
    A = cfg.num_action_tokens
    prompts = [(b["input_ids"][i][: int(b["attention_mask"][i].sum()) - A - 1], None) for i in range(B)]
    pv, proprio = b["pixel_values"].to(dev, BF), b["proprio"].reshape(B, -1).numpy()
    mixed = [f"p{j % 4}" for j in range(B)]
    calls = {
        "4 FiLM policies mixed (per-policy FiLM, pool of 4)": lambda: multi_film.predict_action_batch(prompts, pv, unnorm_key=UNNORM, proprio=proprio, use_film=True, policy=mixed),
        "4 policies mixed, no FiLM (pool of 4)": lambda: multi_plain.predict_action_batch(prompts, pv, unnorm_key=UNNORM, proprio=proprio, policy=mixed),
        "one model with its own FiLM Linears": lambda: single.predict_action_batch(prompts, pv, unnorm_key=UNNORM, proprio=proprio, proprio_projector=pp, action_head=head,
                                                                                   use_film=True),
    }
    for m in (multi_film, multi_plain, single):
        m.enable_graph_replay(True)

    def serve(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters

    for fn in calls.values():
        serve(fn, 2)   # captures the graph, loads the slots
    rounds = {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            rounds[k].append(serve(fn, args.iters))
    for k, v in rounds.items():
        ms = 1e3 * statistics.median(v)
        print(json.dumps(dict(what="serving", variant=k, B=B, ms_per_forward=ms, chunks_per_s=B / ms * 1e3, rounds_ms=[1e3 * x for x in v])), flush=True)

    swaps = {}
    for label, vla in (("with FiLM", multi_film), ("without FiLM", multi_plain)):
        tab = vla.engine.load_slot(1, f"p{n_pol - 1}")
        swaps[label] = (vla, tab)
    res = alternate({label: (lambda vla=vla: vla.engine.load_slot(1, f"p{n_pol - 1}")) for label, (vla, _) in swaps.items()}, args.reps, 1)
    for label, (vla, tab) in swaps.items():
        print(json.dumps(dict(what="swap", variant=label, bytes=tab["nbytes"], entries=tab["n"], tiles=tab["total"], device_ms=res[label],
                              device_GBps=tab["nbytes"] / res[label] / 1e6, pool_bytes_per_policy=vla.policy_pool_bytes // n_pol)), flush=True)


if __name__ == "__main__":
    main()
