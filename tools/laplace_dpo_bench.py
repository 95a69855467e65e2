"""The preference step on the L1 head at full size (BASELINE.json configs[2] shapes: OpenVLA-7B, LoRA r = 32, L1 head, batch 8, two 224 x 224 images +
proprio), against its yardstick and against the composition the existing entry points allow, ALTERNATED in one process.  The expectation from the
launch count: train_step_action_dpo is the L1 step's forward and backward with one launch of launch-latency size in place of the loss, and the
composition costs one inference forward more.  Everything is reported, nothing is a pass / fail condition; the difference of two medians is to be
read beside the yardstick's block-to-block spread printed with it.

  steps    train_step_fwd_bwd (the yardstick), train_step_action_dpo with given reference means, and the composition: action_logprobs under the
           live weights, the margin and the pair's advantages in torch, train_step_action_pg_group at G = 2.  Host clock between two
           synchronisations, alternated blocks.
  kernels  ovla_laplace_dpo at 64 rows with a by-value and with a per-element scale, beside ovla_laplace_pg / ovla_laplace_pg_rows at G = 2 on the
           same rows, each between its own HIP events.
Writes <out-dir>/laplace_dpo.md and <out-dir>/laplace_dpo_bench.jsonl (the raw lines, also printed).
Usage: python tools/laplace_dpo_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--out-dir profiles]"""
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
SCALE, BETA = 0.1, 0.1


def document(build, steps, kernels) -> str:
    """profiles/laplace_dpo.md from the emitted records (so the text can be rebuilt from laplace_dpo_bench.jsonl)."""
    pgb = load("pg_group_bench")
    ms, us = pgb.ms, pgb.us
    B, C, Ad = build["batch"], build["chunk"], build["action_dim"]
    rows = B * C
    base = steps["l1_step"]
    sp = base["ms_min_max"][1] - base["ms_min_max"][0]
    md = [
        "# Preference optimisation on the L1 head (`tools/laplace_dpo_bench.py`)", "",
        f"One MI355X (gfx950; the runtime reports the device name \"{build['device']}\"), one process, synthetic weights, torch {build['torch']}, library source",
        f"hash `{build['source_hash']}`.  Raw lines: `profiles/laplace_dpo_bench.jsonl` (`python tools/laplace_dpo_bench.py --reps {build['reps']} --batch {B} --steps",
        f"{build['steps']} --blocks {build['blocks']}`).  Full size, the shapes of BASELINE.json configs[2]: OpenVLA-7B, LoRA r = 32, L1 head, chunk {C} x {Ad} action",
        f"dimensions, batch {B}: {rows} rows.  Nothing here was a target: the figures are what one run showed.  The three step variants are alternated inside",
        f"one call ({build['steps']} steps per block, one untimed block each, then {build['blocks']} blocks of each); the yardstick is the first row, and a difference is to be",
        "read beside that row's own block-to-block spread, not against a threshold.", "",
        "## The step", "",
        "| call | ms, median [min, max] | minus the yardstick (ms) | the yardstick's own spread, max - min (ms) |", "|---|---|---|---|",
    ]
    for name, key in (("`train_step_fwd_bwd` (the L1 step: the yardstick)", "l1_step"),
                      ("`train_step_action_dpo`, numeric scale, reference means given", "dpo_step"),
                      ("the composition: `action_logprobs` + margin and advantages in torch + `train_step_action_pg_group` at G = 2", "composition")):
        r = steps[key]
        md.append(f"| {name} | {ms(r)} | {r['ms_median'] - base['ms_median']:+.3f} | {sp:.3f} |")
    md += ["", "## The launch", "",
           f"`[{rows}, {Ad}]` predictions, one pair per observation; each call between its own HIP events, 3 untimed calls, {build['reps']} rounds alternated (µs).  These",
           f"are launches of {B} workgroups of 64 lanes: the figures are launch latency.", "",
           "| launch | µs, median [min, max] |", "|---|---|"]
    for name, key in (("`ovla_laplace_dpo`, by-value scale", "dpo_fixed"), ("`ovla_laplace_dpo`, per-element scale", "dpo_rows"),
                      ("`ovla_laplace_pg`, G = 2 (the launch it replaces)", "pg_fixed"), ("`ovla_laplace_pg_rows`, G = 2", "pg_rows")):
        md.append(f"| {name} | {us(kernels[key])} |")
    d = steps["dpo_step"]["ms_median"] - base["ms_median"]
    dc = steps["composition"]["ms_median"] - steps["dpo_step"]["ms_median"]
    md += ["", "## Reading", "",
           f"The preference step's difference to the L1 step, {d:+.3f} ms, {'EXCEEDS' if abs(d) > sp else 'lies inside'} the yardstick's block-to-block spread of {sp:.3f} ms.",
           f"The composition from the existing entry points costs {dc:+.3f} ms more than the preference step: the inference forward of `action_logprobs`, which the",
           "one-launch form does not make.  Where the step's own difference goes: the L1 step's loss is formed inside the head's backward launch, the",
           "preference step puts `ovla_laplace_dpo` before it and places `chosen`, `rejected` and the reference means (three small copies when they are already on",
           "the device) and forms its seven statistics with a handful of small torch launches at the end; nothing is read back.", ""]
    return "\n".join(md)


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
        (out_dir / "laplace_dpo_bench.jsonl").write_text("".join(json.dumps(r) + "\n" for r in lines))

    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    build = dict(metric="build", device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), torch=torch.__version__, batch=args.batch,
                 reps=args.reps, steps=args.steps, blocks=args.blocks, scale=SCALE, beta=BETA, chunk=cfg.chunk, action_dim=cfg.action_dim, llm_dim=cfg.llm_dim)
    emit(**build)
    B, C, Ad = args.batch, cfg.chunk, cfg.action_dim
    rows = B * C

    # -- the launch ----------------------------------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    pred = (torch.randn(rows, Ad, device=dev, generator=g) * 0.3).to(BF)
    ref = (pred.float() + 0.02 * torch.randn(rows, Ad, device=dev, generator=g)).to(BF)
    ls = (torch.randn(rows, Ad, device=dev, generator=g) * 0.3 - 2.0).to(BF)
    ref_ls = (ls.float() + 0.1).to(BF)
    chosen = pred.float() + SCALE * torch.randn(rows, Ad, device=dev, generator=g)
    rejected = pred.float() + 2 * SCALE * torch.randn(rows, Ad, device=dev, generator=g)
    pair2 = torch.stack([chosen, rejected], dim=1).contiguous()
    adv2 = torch.tensor([[1.0, -1.0]], device=dev).repeat(rows, 1).contiguous()
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
    o = dict(logprob=f32(rows, 2), ref_logprob=f32(rows, 2), h=f32(B, 2), margin=f32(B), loss=f32(B), coef=f32(B), dpred=torch.empty(rows, Ad, dtype=BF, device=dev))
    dls = torch.empty(rows, Ad, dtype=BF, device=dev)
    pg = dict(logprob=f32(rows, 2), ratio=f32(rows, 2), clipped=torch.empty(rows, 2, dtype=torch.int32, device=dev), dpred=torch.empty(rows, Ad, dtype=BF, device=dev))
    ent, dls2 = f32(rows), torch.empty(rows, Ad, dtype=BF, device=dev)
    kw = dict(beta=BETA, grad_scale=1.0 / B, nll_coef=0.1, nll_scale=1.0 / rows)
    runs = {
        "dpo_fixed": lambda: ops.laplace_dpo(pred, ref, chosen, rejected, C, SCALE, **kw, **o),
        "dpo_rows": lambda: ops.laplace_dpo(pred, ref, chosen, rejected, C, log_scale=ls, ref_log_scale=ref_ls, dlog_scale=dls, **kw, **o),
        "pg_fixed": lambda: ops.laplace_pg(pred, pair2, adv2, SCALE, grad_scale=1.0, **pg),
        "pg_rows": lambda: ops.laplace_pg_rows(pred, ls, ops.LAPLACE_SCALE_BOUNDS, pair2, adv2, grad_scale=1.0, entropy=ent, dlog_scale=dls2, **pg),
    }
    kernels = pgb.alternate(runs, args.reps)
    emit(metric="launches, alternated, HIP events (us, median)", rows=rows, action_dim=Ad, **kernels)

    # -- the steps -----------------------------------------------------------------------------------------------------------------------------
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
    draws = [eng.sample_actions_laplace(b, SCALE, num_samples=2) for b in batches]
    pairs = [d["actions"] for d in draws]                        # [B, 2, chunk, action_dim]: draw 0 the chosen chunk, draw 1 the rejected one
    refs = [(d["mean"].float() + 0.01).to(BF) for d in draws]    # reference means, computed once per dataset
    ref_lps = []
    for p, r in zip(pairs, refs):
        a = p.permute(0, 2, 1, 3).reshape(rows, 2, Ad).contiguous()
        lp = ops.laplace_pg(r.reshape(rows, Ad).contiguous(), a, torch.ones(rows, 2, device=dev), SCALE)[0]
        ref_lps.append(lp.view(B, C, 2).permute(0, 2, 1).contiguous())

    def l1():
        for b in batches:
            eng.train_step_fwd_bwd(b)
        return len(batches)

    def dpo():
        for b, p, r in zip(batches, pairs, refs):
            eng.train_step_action_dpo(b, p[:, 0], p[:, 1], SCALE, beta=BETA, ref_means=r)
        return len(batches)

    def composition():
        for b, p, rlp in zip(batches, pairs, ref_lps):
            lp = eng.action_logprobs(b, p, SCALE)["logprob"]     # [B, 2, chunk]: the forward the one-launch form does not make
            h = (lp - rlp).sum(2)
            k = BETA * torch.sigmoid(-BETA * (h[:, 0] - h[:, 1]))
            eng.train_step_action_pg_group(b, p, torch.stack([k, -k], dim=1), SCALE, loss_scale=2.0 * C)
        return len(batches)

    eng.zero_grad()
    steps = pgb.host_blocks({"l1_step": l1, "dpo_step": dpo, "composition": composition}, args.blocks)
    emit(metric="fwd + bwd, ms/step: the L1 step vs train_step_action_dpo vs the three-call composition, alternated blocks (report only)", batch=B,
         steps_per_block=args.steps, rows=rows, dpo_minus_l1_ms=steps["dpo_step"]["ms_median"] - steps["l1_step"]["ms_median"],
         composition_minus_dpo_ms=steps["composition"]["ms_median"] - steps["dpo_step"]["ms_median"], **steps)
    eng.zero_grad()

    (out_dir / "laplace_dpo.md").write_text(document(build, steps, kernels))
    return 0


if __name__ == "__main__":
    sys.exit(main())
