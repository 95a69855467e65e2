"""The learned Laplace scale at full size (BASELINE.json configs[2] shapes: OpenVLA-7B, LoRA r = 32, L1 head, batch 8, two 224 x 224 images +
proprio), each variant against what it stands beside, ALTERNATED in one process.  The expectation under test: the scale head costs launch latency
-- a handful of launches of a few hundred lanes beside a step of well over a hundred milliseconds.  Everything is reported, nothing is a pass /
fail condition; the difference of two medians is to be read beside the block-to-block spread printed with it.

  group    train_step_action_pg_group at G = 8 with a numeric scale and with scale="learned" (with and without reference + entropy bonus), fwd + bwd,
           host clock between two synchronisations, alternated blocks.
  fit      train_step_fwd_bwd (the L1 step) without and with fit_scale=True, the same clock, alternated.
  nll      a plain inference forward with the head (_action_means) and train_step_scale_nll, the same clock, alternated.
  kernels  ovla_laplace_sample_rows / ovla_laplace_pg_rows (G = 8, both gradients; also with old log-probabilities, a reference and the entropy
           bonus; and G = 1 without dpred: the NLL form) beside the fixed-scale pair, and the scale head's two launches (ovla_head_out_fwd /
           ovla_head_out_bwd on [rows, llm_dim]), on `rows` = batch * chunk prediction rows, each between its own pair of HIP events.
Writes <out-dir>/laplace_scale.md and <out-dir>/laplace_scale_bench.jsonl (the raw lines, also printed).
Usage: python tools/laplace_scale_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--out-dir profiles]"""
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
G = 8
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
        (out_dir / "laplace_scale_bench.jsonl").write_text("".join(json.dumps(r) + "\n" for r in lines))

    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    build = dict(metric="build", device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), torch=torch.__version__, batch=args.batch,
                 reps=args.reps, steps=args.steps, blocks=args.blocks, scale=SCALE, G=G)
    emit(**build)
    B, C, Ad, D = args.batch, cfg.chunk, cfg.action_dim, cfg.llm_dim
    rows = B * C
    bounds = ops.LAPLACE_SCALE_BOUNDS

    # -- the kernels on a batch's predictions ------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    pred = (torch.rand(rows, Ad, device=dev, generator=g) * 2 - 1).to(BF)
    ref = (pred.float() + 0.05 * torch.randn(rows, Ad, device=dev, generator=g)).to(BF)
    ls = (torch.randn(rows, Ad, device=dev, generator=g) * 0.3 - 2.3).to(BF)          # b around 0.1
    ref_ls = (ls.float() + 0.1 * torch.randn(rows, Ad, device=dev, generator=g)).to(BF)
    h2 = torch.randn(rows, D, device=dev, generator=g).to(BF)
    W, bias = (torch.randn(Ad, D, device=dev, generator=g) * 0.01).to(BF), torch.zeros(Ad, device=dev, dtype=BF)
    dW, db = torch.zeros(Ad, D, device=dev), torch.zeros(Ad, device=dev)
    act, lp = ops.laplace_sample(pred, SCALE, G, seed=1, call=2)
    act_r, lp_r, ent_r = ops.laplace_sample_rows(pred, ls, bounds, G, seed=1, call=2)
    adv = torch.randn(rows, G, device=dev, generator=g)
    target, ones = ref.float().view(rows, 1, Ad).contiguous(), torch.ones(rows, 1, device=dev)
    dpred, dls, ls_out, dx = torch.empty_like(pred), torch.empty_like(pred), torch.empty_like(pred), torch.empty_like(h2)
    old, old_r = lp.clone(), lp_r.clone()
    gs = 1.0 / (rows * G)
    runs = {
        "laplace_sample": lambda: ops.laplace_sample(pred, SCALE, G, seed=1, call=2, action=act, logprob=lp),
        "laplace_sample_rows": lambda: ops.laplace_sample_rows(pred, ls, bounds, G, seed=1, call=2, action=act_r, logprob=lp_r, entropy=ent_r),
        "laplace_pg": lambda: ops.laplace_pg(pred, act, adv, SCALE, grad_scale=gs, dpred=dpred),
        "laplace_pg_rows": lambda: ops.laplace_pg_rows(pred, ls, bounds, act_r, adv, grad_scale=gs, dpred=dpred, dlog_scale=dls),
        "laplace_pg_old_ref": lambda: ops.laplace_pg(pred, act, adv, SCALE, old_logprob=old, ref_pred=ref, kl_coef=0.04, grad_scale=gs, kl_scale=1.0 / rows, dpred=dpred),
        "laplace_pg_rows_old_ref_ent": lambda: ops.laplace_pg_rows(pred, ls, bounds, act_r, adv, old_logprob=old_r, ref_pred=ref, ref_log_scale=ref_ls, kl_coef=0.04,
                                                                   grad_scale=gs, kl_scale=1.0 / rows, entropy_coef=0.01, ent_scale=1.0 / rows, dpred=dpred, dlog_scale=dls),
        "laplace_pg_rows_nll": lambda: ops.laplace_pg_rows(pred, ls, bounds, target, ones, grad_scale=1.0 / rows, want_dpred=False, dlog_scale=dls),
        "scale_head_fwd": lambda: ops.head_out_fwd(h2, W, bias, out=ls_out),
        "scale_head_bwd": lambda: ops.head_out_bwd(h2, W, None, None, 0.0, dW, db, dpred=dls, out=dx),
    }
    kernels = pgb.alternate(runs, args.reps)
    emit(metric="kernels on bf16 predictions [rows, action_dim] / hidden [rows, llm_dim], G = 8, alternated, HIP events (us, median)", rows=rows, action_dim=Ad,
         llm_dim=D, **kernels)

    # -- the steps -----------------------------------------------------------------------------------------------------------------------------
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="l1", has=has)
    del sd, get
    torch.cuda.empty_cache()
    eng.attach_scale_head(SCALE)
    eng.scale_head.w.data.copy_((torch.randn(Ad, D, device=dev, generator=g) * 0.005).to(BF))     # widths that vary over the rows
    batches = [synth.make_batch(B, seed=2000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
               for i in range(args.steps)]
    for b in batches:                                            # inputs resident in HBM before the timed region, as in bench.py
        for k in ("pixel_values", "actions", "proprio"):
            b[k] = b[k].to(dev, BF)
    draws_n = [eng.sample_actions_laplace(b, SCALE, num_samples=G) for b in batches]
    draws_l = [eng.sample_actions_laplace(b, "learned", num_samples=G) for b in batches]
    advs = [torch.randn(B, G, device=dev) for _ in batches]
    refs = [dict(ref_means=(d["mean"].float() + 0.05).to(BF), ref_log_scales=(d["log_scale"].float() - 0.1).to(BF)) for d in draws_l]

    def group(scale, draws, **kw):
        def run():
            for i, (b, d, a) in enumerate(zip(batches, draws, advs)):
                extra = dict(refs[i], **kw) if kw else {}
                eng.train_step_action_pg_group(b, d["actions"], a, scale, old_logprobs=d["logprob"], **extra)
            return len(batches)
        return run

    eng.zero_grad()
    steps = pgb.host_blocks({"group_numeric": group(SCALE, draws_n), "group_learned": group("learned", draws_l),
                             "group_learned_ref_ent": group("learned", draws_l, kl_coef=0.04, entropy_coef=0.01)}, args.blocks)
    emit(metric="train_step_action_pg_group at G = 8 (fwd + bwd), ms/step: numeric scale vs scale='learned', alternated blocks (report only)", batch=B,
         steps_per_block=args.steps, rows=rows, learned_minus_numeric_ms=steps["group_learned"]["ms_median"] - steps["group_numeric"]["ms_median"], **steps)
    eng.zero_grad()

    def l1(**kw):
        def run():
            for b in batches:
                eng.train_step_fwd_bwd(b, **kw)
            return len(batches)
        return run

    fit = pgb.host_blocks({"l1_step": l1(), "l1_step_fit_scale": l1(fit_scale=True)}, args.blocks)
    emit(metric="train_step_fwd_bwd (fwd + bwd), ms/step: plain vs fit_scale=True, alternated blocks (report only)", batch=B, steps_per_block=args.steps,
         fit_minus_plain_ms=fit["l1_step_fit_scale"]["ms_median"] - fit["l1_step"]["ms_median"], **fit)
    eng.zero_grad()

    def fwd(nll):
        def run():
            with torch.no_grad():
                for b in batches:
                    if nll:
                        eng.train_step_scale_nll(b)
                    else:
                        eng._action_means(b, False, eng.head)
            return len(batches)
        return run

    nll = pgb.host_blocks({"inference_forward": fwd(False), "train_step_scale_nll": fwd(True)}, args.blocks)
    emit(metric="ms/call: a plain inference forward with the head vs train_step_scale_nll, alternated blocks (report only)", batch=B,
         nll_minus_forward_ms=nll["train_step_scale_nll"]["ms_median"] - nll["inference_forward"]["ms_median"], **nll)
    eng.zero_grad()

    # -- the document ------------------------------------------------------------------------------------------------------------------------------
    ms, us = pgb.ms, pgb.us

    def spread(r):
        return r["ms_min_max"][1] - r["ms_min_max"][0]

    def pair(title, table, base, rows_):
        out = [title, "", "| call | ms, median [min, max] | minus the yardstick (ms) | the yardstick's own spread, max - min (ms) |", "|---|---|---|---|"]
        for name, key in rows_:
            r = table[key]
            out.append(f"| {name} | {ms(r)} | {r['ms_median'] - table[base]['ms_median']:+.3f} | {spread(table[base]):.3f} |")
        return out + [""]

    md = [
        "# The learned Laplace scale on the L1 head (`tools/laplace_scale_bench.py`)", "",
        f"One MI355X (gfx950; the runtime reports the device name \"{build['device']}\"), one process, synthetic weights, torch {build['torch']}, library source",
        f"hash `{build['source_hash']}`.  Raw lines: `profiles/laplace_scale_bench.jsonl` (`python tools/laplace_scale_bench.py --reps {args.reps} --batch {B} --steps",
        f"{args.steps} --blocks {args.blocks}`).  Full size, the shapes of BASELINE.json configs[2]: OpenVLA-7B, LoRA r = 32, L1 head, chunk {C} x {Ad} action",
        f"dimensions, batch {B}: {rows} prediction rows, G = {G}.  Nothing here was a target: the figures are what one run showed.  Each comparison is alternated",
        f"inside one call ({args.steps} steps per block, one untimed block each, then {args.blocks} blocks of each); the yardstick of every table is its first row,",
        "measured in the same call, and a difference is to be read beside that row's own block-to-block spread, not against a threshold.", "",
    ]
    md += pair("## The group step", steps, "group_numeric", (("`train_step_action_pg_group`, numeric scale, old log-probabilities", "group_numeric"),
                                                             ("the same, `scale=\"learned\"`", "group_learned"),
                                                             ("`scale=\"learned\"`, reference mean + log-scale, kl_coef 0.04, entropy_coef 0.01", "group_learned_ref_ent")))
    md += pair("## The maximum-likelihood fit beside the L1 step", fit, "l1_step", (("`train_step_fwd_bwd` (L1 regression)", "l1_step"),
                                                                                     ("`train_step_fwd_bwd(fit_scale=True)`", "l1_step_fit_scale")))
    md += pair("## The fit on a frozen policy", nll, "inference_forward", (("inference forward + head", "inference_forward"), ("`train_step_scale_nll`", "train_step_scale_nll")))
    md += ["## The kernels", "",
           f"bf16 predictions `[{rows}, {Ad}]`, hidden `[{rows}, {D}]`, each call between its own HIP events, 3 untimed calls, {args.reps} rounds alternated (µs).",
           "These are launches of a few hundred lanes: the figures are launch latency, not throughput.", "",
           "| launch | µs, median [min, max] |", "|---|---|"]
    for name, key in (("`laplace_sample` (fixed scale)", "laplace_sample"), ("`laplace_sample_rows`", "laplace_sample_rows"), ("`laplace_pg` + dpred (fixed scale)", "laplace_pg"),
                      ("`laplace_pg_rows` + dpred + dlog_scale", "laplace_pg_rows"), ("`laplace_pg`, old log-probabilities + reference", "laplace_pg_old_ref"),
                      ("`laplace_pg_rows`, old log-probabilities + reference + entropy bonus", "laplace_pg_rows_old_ref_ent"),
                      ("`laplace_pg_rows`, G = 1, dlog_scale only (the NLL form)", "laplace_pg_rows_nll"), ("scale head forward (`head_out_fwd`)", "scale_head_fwd"),
                      ("scale head backward (`head_out_bwd`, dx discarded)", "scale_head_bwd")):
        md.append(f"| {name} | {us(kernels[key])} |")
    md.append("")
    (out_dir / "laplace_scale.md").write_text("\n".join(md))
    return 0


if __name__ == "__main__":
    sys.exit(main())
