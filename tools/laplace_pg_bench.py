"""The continuous-action group policy-gradient step at full size (BASELINE.json configs[2] shapes: OpenVLA-7B, LoRA r = 32, L1 head, batch 8, two
224 x 224 images + proprio), each variant against what it stands beside, ALTERNATED in one process.  The expectation under test: the group step
costs what the L1 step costs, because one tiny ovla_laplace_pg launch replaces the fused L1 gradient and everything else is the same forward and
backward.  Everything is reported, nothing is a pass / fail condition.

  step     VLAEngine.train_step_fwd_bwd (the L1 step) and train_step_action_pg_group at G = 8 and G = 16, and at G = 8 with ref_means + kl_coef
           (fwd + bwd, gradients accumulate), host clock between two synchronisations, alternated blocks.
  means    a plain inference forward with the head (action_logprobs' forward: _action_means) and reference_action_means (the same between the two
           swaps of the flat buffers and the re-derivation of the transposed copies), the same clock, alternated.
  kernels  ovla_laplace_sample and ovla_laplace_pg (with the gradient; G = 8 also with old log-probabilities and a reference) at G = 1, 8, 16 on
           bf16 predictions [batch * chunk, action_dim], each between its own pair of HIP events.
Writes <out-dir>/laplace_pg.md and <out-dir>/laplace_pg_bench.jsonl (the raw lines, also printed).
Usage: python tools/laplace_pg_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--out-dir profiles]"""
import argparse
import importlib
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
load = importlib.import_module
BF = torch.bfloat16
GROUPS = (1, 8, 16)
STEP_GROUPS = (8, 16)
SCALE = 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out-dir", default=str(Path(__file__).resolve().parent.parent / "profiles"))
    args = ap.parse_args()
    engine_mod, weights_mod, synth, config_mod, ops, _lib = (load(f"openvla-oft_amd.{m}") for m in ("engine", "weights", "synthetic", "config", "ops", "_lib"))
    pgb = load("pg_group_bench")                                 # the clocks: alternate (HIP events), host_blocks (host clock between synchronisations)
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        (out_dir / "laplace_pg_bench.jsonl").write_text("".join(json.dumps(r) + "\n" for r in lines))

    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    build = dict(metric="build", device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), torch=torch.__version__, batch=args.batch,
                 reps=args.reps, steps=args.steps, blocks=args.blocks, scale=SCALE)
    emit(**build)
    B, C, Ad = args.batch, cfg.chunk, cfg.action_dim
    rows = B * C

    # -- the kernels on a batch's predictions ------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    pred = (torch.rand(rows, Ad, device=dev, generator=g) * 2 - 1).to(BF)
    ref = (pred.float() + 0.05 * torch.randn(rows, Ad, device=dev, generator=g)).to(BF)
    draws = {G: ops.laplace_sample(pred, SCALE, G, seed=1, call=2) for G in GROUPS}
    adv = {G: torch.randn(rows, G, device=dev, generator=g) for G in GROUPS}
    dpred = torch.empty_like(pred)
    runs = {}
    for G in GROUPS:
        runs[f"laplace_sample_G{G}"] = lambda G=G: ops.laplace_sample(pred, SCALE, G, seed=1, call=2, action=draws[G][0], logprob=draws[G][1])
        runs[f"laplace_pg_G{G}"] = lambda G=G: ops.laplace_pg(pred, draws[G][0], adv[G], SCALE, grad_scale=1.0 / (rows * G), dpred=dpred)
    old8 = draws[8][1].clone()
    runs["laplace_pg_G8_old_ref"] = lambda: ops.laplace_pg(pred, draws[8][0], adv[8], SCALE, old_logprob=old8, ref_pred=ref, kl_coef=0.04, grad_scale=1.0 / (rows * 8),
                                                           kl_scale=1.0 / rows, dpred=dpred)
    kernels = pgb.alternate(runs, args.reps)
    emit(metric="Laplace kernels on bf16 predictions [rows, action_dim], alternated, HIP events (us, median)", rows=rows, action_dim=Ad, **kernels)

    # -- the training step ---------------------------------------------------------------------------------------------------------------------
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="l1", has=has)
    del sd, get
    torch.cuda.empty_cache()
    batches = [synth.make_batch(B, seed=2000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
               for i in range(args.steps)]
    for b in batches:                                            # inputs resident in HBM before the timed region, as in bench.py
        for k in ("pixel_values", "actions", "proprio"):
            b[k] = b[k].to(dev, BF)
    drawsG = {G: [eng.sample_actions_laplace(b, SCALE, num_samples=G) for b in batches] for G in STEP_GROUPS}
    advsG = {G: [torch.randn(B, G, device=dev) for _ in batches] for G in STEP_GROUPS}
    refs8 = [(d["mean"].float() + 0.05).to(BF) for d in drawsG[8]]            # a reference half a scale away: the KL term is not identically zero
    eng.set_reference_policy()

    def l1():
        for b in batches:
            eng.train_step_fwd_bwd(b)
        return len(batches)

    def group(G, **kw):
        def run():
            for i, (b, d, a) in enumerate(zip(batches, drawsG[G], advsG[G])):
                extra = dict(ref_means=refs8[i]) if kw else {}
                eng.train_step_action_pg_group(b, d["actions"], a, SCALE, old_logprobs=d["logprob"], **extra, **kw)
            return len(batches)
        return run

    eng.zero_grad()
    runs = {"l1_step": l1}
    for G in STEP_GROUPS:
        runs[f"group_G{G}"] = group(G)
    runs["group_G8_ref"] = group(8, kl_coef=0.04)
    steps = pgb.host_blocks(runs, args.blocks)
    emit(metric="training step (fwd + bwd), ms/step: train_step_fwd_bwd (L1) vs train_step_action_pg_group, alternated blocks (report only)", batch=B,
         steps_per_block=args.steps, rows=rows, g8_over_l1=steps["group_G8"]["ms_median"] / steps["l1_step"]["ms_median"], **steps)
    eng.zero_grad()

    def means(ref_scope):
        def run():
            with torch.no_grad():
                for b in batches:
                    if ref_scope:
                        eng.reference_action_means(b)
                    else:
                        eng._action_means(b, False, eng.head)
            return len(batches)
        return run

    mns = pgb.host_blocks({"inference_forward": means(False), "reference_action_means": means(True)}, args.blocks)
    emit(metric="the head's prediction, ms/call: a plain inference forward vs reference_action_means (two swaps + two refresh_derived), alternated blocks",
         batch=B, reference_bytes=eng.reference_policy_bytes(), swap_ms=mns["reference_action_means"]["ms_median"] - mns["inference_forward"]["ms_median"], **mns)

    # -- the document ------------------------------------------------------------------------------------------------------------------------------
    ms, us = pgb.ms, pgb.us
    s1 = steps["l1_step"]["ms_median"]
    md = [
        "# Continuous-action group policy gradient on the L1 head (`tools/laplace_pg_bench.py`)", "",
        f"One MI355X (gfx950; the runtime reports the device name \"{build['device']}\"), one process, synthetic weights, torch {build['torch']}, library source",
        f"hash `{build['source_hash']}`.  Raw lines: `profiles/laplace_pg_bench.jsonl` (`python tools/laplace_pg_bench.py --reps {args.reps} --batch {B} --steps",
        f"{args.steps} --blocks {args.blocks}`).  Full size, the shapes of BASELINE.json configs[2]: OpenVLA-7B, LoRA r = 32, L1 head, chunk {C} x {Ad} action",
        f"dimensions, batch {B}: {rows} prediction rows.  Nothing here was a target: the figures are what one run showed.  Each comparison is alternated inside",
        "one call; medians, [min, max] beside them.", "",
        "## The training step", "",
        f"Forward + backward into the gradient buffers, no optimizer step, host clock between two synchronisations, {args.steps} steps per block, one untimed",
        f"block each, then {args.blocks} blocks of each alternated.  The yardstick is `train_step_fwd_bwd`, the L1 regression step, in the same call.", "",
        "| step | ms / step, median [min, max] | over the L1 step |", "|---|---|---|",
        f"| `train_step_fwd_bwd` (L1 regression) | {ms(steps['l1_step'])} | 1.000 |",
    ]
    for G in STEP_GROUPS:
        r = steps[f"group_G{G}"]
        md.append(f"| `train_step_action_pg_group`, G = {G}, old log-probabilities | {ms(r)} | {r['ms_median'] / s1:.3f} |")
    r = steps["group_G8_ref"]
    md += [f"| the same, G = 8, `ref_means`, kl_coef 0.04 | {ms(r)} | {r['ms_median'] / s1:.3f} |", "",
           "## Reference means", "",
           f"A plain inference forward with the head and `reference_action_means`, ms per call, the same clock and alternation.  The reference snapshot holds",
           f"{eng.reference_policy_bytes() / 1e6:.1f} MB; the difference is two copies of it in, two out (stash and restore) and two `refresh_derived()`.", "",
           "| call | ms / call, median [min, max] |", "|---|---|",
           f"| inference forward + head | {ms(mns['inference_forward'])} |", f"| `reference_action_means` | {ms(mns['reference_action_means'])} |", "",
           "## The kernels", "",
           f"bf16 predictions `[{rows}, {Ad}]`, scale {SCALE}, each call between its own HIP events, 3 untimed calls, {args.reps} rounds alternated (µs).  These are",
           "launches of a few hundred lanes: the figures are launch latency, not throughput.", "",
           "| kernel | " + " | ".join(f"G = {G}" for G in GROUPS) + " |", "|---|" + "---|" * len(GROUPS),
           "| `laplace_sample` | " + " | ".join(us(kernels[f"laplace_sample_G{G}"]) for G in GROUPS) + " |",
           "| `laplace_pg` + gradient | " + " | ".join(us(kernels[f"laplace_pg_G{G}"]) for G in GROUPS) + " |", "",
           f"`laplace_pg` at G = 8 with old log-probabilities and a reference prediction (the KL term): {us(kernels['laplace_pg_G8_old_ref'])}.", ""]
    (out_dir / "laplace_pg.md").write_text("\n".join(md))
    return 0


if __name__ == "__main__":
    sys.exit(main())
