"""The group policy-gradient step at full size (OpenVLA-7B, LoRA r = 32, discrete token path, batch 8), each variant against what it stands beside,
ALTERNATED in one process.  The claim under test: a G = 8 group step costs about one single-draw step, not eight, because the decoder forward does
not depend on the drawn tokens and the G surrogates are summed in dlogits before lm_head's backward.  Everything is reported, nothing is a pass /
fail condition.

  step      VLAEngine.train_step_policy_gradient (the single-draw step) and train_step_policy_gradient_group at G = 1, 4, 8, 16, and at G = 8 with
            ref_logprobs + kl_coef + entropy_coef (fwd + bwd, gradients accumulate), host clock between two synchronisations, alternated blocks.
  logprobs  policy_logprobs and reference_logprobs on [B, 8, A] tokens (the difference is the two swaps of the flat buffers and the re-derivation of
            the transposed copies), the same clock, alternated.
  kernels   ovla_token_pg / ovla_token_pg_group (G = 1, 4, 8, 16) with the gradient, and ovla_sample_tokens_group against G launches of
            ovla_sample_tokens, on bf16 logits [batch * 56, 32064], action window and whole vocabulary, each between its own pair of HIP events.
Writes <out-dir>/pg_group.md and <out-dir>/pg_group_bench.jsonl (the raw lines, also printed).
Usage: python tools/pg_group_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--out-dir profiles]"""
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
GROUPS = (1, 4, 8, 16)


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


def host_blocks(runs, blocks):
    """runs: name -> fn() doing `n` steps and returning n.  One untimed block each, then `blocks` rounds of all of them alternated -> ms per step."""
    def block(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    for fn in runs.values():
        block(fn)
    ms = {k: [] for k in runs}
    for _ in range(blocks):
        for k, fn in runs.items():
            ms[k].append(block(fn))
    return {k: dict(ms=v, ms_median=float(np.median(v)), ms_min_max=[min(v), max(v)]) for k, v in ms.items()}


def us(r):
    return f"{r['us']:.1f} [{r['us_min_max'][0]:.1f}, {r['us_min_max'][1]:.1f}]"


def ms(r):
    return f"{r['ms_median']:.2f} [{r['ms_min_max'][0]:.2f}, {r['ms_min_max'][1]:.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--out-dir", default=str(Path(__file__).resolve().parent.parent / "profiles"))
    args = ap.parse_args()
    engine_mod, weights_mod, synth, config_mod, ops, _lib = (load(f"openvla-oft_amd.{m}") for m in ("engine", "weights", "synthetic", "config", "ops", "_lib"))
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    lines = []

    def emit(**rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        (out_dir / "pg_group_bench.jsonl").write_text("".join(json.dumps(r) + "\n" for r in lines))

    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    build = dict(metric="build", device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), torch=torch.__version__, batch=args.batch,
                 reps=args.reps, steps=args.steps, blocks=args.blocks)
    emit(**build)
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=True)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="none", has=has)
    del sd, get
    torch.cuda.empty_cache()
    A, B, T = cfg.num_action_tokens, args.batch, args.temperature
    window = eng.token_window("actions")
    n_tokens, n_bins = cfg.vocab - cfg.pad_to_multiple_of, cfg.n_action_bins - 1
    rows = B * A

    # -- the kernels on the batch's logits ---------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    logits = torch.randn(rows, cfg.vocab, device=dev, generator=g).to(BF)
    scratch = torch.empty_like(logits)
    tok = {G: torch.randint(window[0], window[1], (rows, G), device=dev, generator=g).to(torch.int32) for G in GROUPS}
    adv = {G: torch.randn(rows, G, device=dev, generator=g) for G in GROUPS}
    kernels = {}
    for wname, w in (("actions", window), ("vocab", None)):
        runs = {"token_pg": lambda w=w: ops.token_pg(logits, tok[1][:, 0].contiguous(), adv[1][:, 0].contiguous(), window=w, temperature=T, grad_scale=1.0 / rows,
                                                     dlogits=scratch)}
        for G in GROUPS:
            runs[f"token_pg_group_G{G}"] = lambda w=w, G=G: ops.token_pg_group(logits, tok[G], adv[G], window=w, temperature=T, grad_scale=1.0 / (rows * G),
                                                                               dlogits=scratch)
        lp8 = ops.token_pg_group(logits, tok[8], adv[8], window=w, temperature=T)[0]
        runs["token_pg_group_G8_ref_entropy"] = lambda w=w: ops.token_pg_group(logits, tok[8], adv[8], window=w, temperature=T, old_logprob=lp8, ref_logprob=lp8,
                                                                               kl_coef=0.04, ent_scale=0.01 / rows, grad_scale=1.0 / (rows * 8), dlogits=scratch)
        for G in GROUPS:
            runs[f"sample_tokens_group_G{G}"] = lambda w=w, G=G: ops.sample_tokens_group(logits, G, n_tokens=n_tokens, n_bins=n_bins, window=w, temperature=T, seed=1, call=2)

            def launches(w=w, G=G):
                for _ in range(G):
                    ops.sample_tokens(logits, n_tokens=n_tokens, n_bins=n_bins, window=w, temperature=T, seed=1, call=2)

            runs[f"sample_tokens_x{G}"] = launches
        kernels[wname] = alternate(runs, args.reps)
        emit(metric="group kernels on bf16 logits [rows, vocab], alternated, HIP events (us, median)", rows=rows, vocab=cfg.vocab, window=wname,
             logits_MB=rows * cfg.vocab * 2 / 1e6, **kernels[wname])
    del logits, scratch
    torch.cuda.empty_cache()

    # -- the training step ---------------------------------------------------------------------------------------------------------------------
    batches = [synth.make_batch(B, seed=2000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
               for i in range(args.steps)]
    draws1 = [eng.sample_action_tokens(b, temperature=T) for b in batches]
    advs1 = [torch.randn(B, device=dev) for _ in batches]
    drawsG = {G: [eng.sample_action_tokens(b, temperature=T, num_samples=G) for b in batches] for G in GROUPS}
    advsG = {G: [torch.randn(B, G, device=dev) for _ in batches] for G in GROUPS}
    refs8 = [(d["logprob"] + 0.1).contiguous() for d in drawsG[8]]          # a reference a tenth of a nat away: the KL term is not identically zero
    eng.set_reference_policy()

    def single():
        for b, d, a in zip(batches, draws1, advs1):
            eng.train_step_policy_gradient(b, d["tokens"], a, old_logprobs=d["logprob"], temperature=T)
        return len(batches)

    def group(G, **kw):
        def run():
            for i, (b, d, a) in enumerate(zip(batches, drawsG[G], advsG[G])):
                extra = dict(ref_logprobs=refs8[i]) if kw else {}
                eng.train_step_policy_gradient_group(b, d["tokens"], a, old_logprobs=d["logprob"], temperature=T, **extra, **kw)
            return len(batches)
        return run

    eng.zero_grad()
    runs = {"single_draw": single}
    for G in GROUPS:
        runs[f"group_G{G}"] = group(G)
    runs["group_G8_ref_entropy"] = group(8, kl_coef=0.04, entropy_coef=0.01)
    steps = host_blocks(runs, args.blocks)
    emit(metric="training step (fwd + bwd), ms/step: train_step_policy_gradient vs train_step_policy_gradient_group, alternated blocks (report only)", batch=B,
         steps_per_block=args.steps, rows=rows, g8_over_single=steps["group_G8"]["ms_median"] / steps["single_draw"]["ms_median"], **steps)
    eng.zero_grad()

    def logprobs(ref):
        def run():
            with torch.no_grad():
                for b, d in zip(batches, drawsG[8]):
                    (eng.reference_logprobs if ref else eng.policy_logprobs)(b, d["tokens"], temperature=T)
            return len(batches)
        return run

    lps = host_blocks({"policy_logprobs": logprobs(False), "reference_logprobs": logprobs(True)}, args.blocks)
    emit(metric="log-probabilities of [B, 8, A] tokens, ms/call: policy_logprobs vs reference_logprobs (two swaps + two refresh_derived), alternated blocks",
         batch=B, reference_bytes=eng.reference_policy_bytes(), swap_ms=lps["reference_logprobs"]["ms_median"] - lps["policy_logprobs"]["ms_median"], **lps)

    # -- the document ------------------------------------------------------------------------------------------------------------------------------
    s1 = steps["single_draw"]["ms_median"]
    md = [
        "# Group policy gradient: G draws per forward (`tools/pg_group_bench.py`)", "",
        f"One MI355X (gfx950; the runtime reports the device name \"{build['device']}\"), one process, synthetic weights, torch {build['torch']}, library source",
        f"hash `{build['source_hash']}`.  Raw lines: `profiles/pg_group_bench.jsonl` (`python tools/pg_group_bench.py --reps {args.reps} --batch {B} --steps",
        f"{args.steps} --blocks {args.blocks}`).  Full size: OpenVLA-7B, LoRA r = 32, discrete token path, {A} action tokens per chunk, lm_head {cfg.vocab} rows,",
        f"batch {B}: {rows} action rows.  Nothing here was a target: the figures are what one run showed.  Each comparison is alternated inside one call;",
        "medians, [min, max] beside them.", "",
        "## The training step", "",
        f"Forward + backward into the gradient buffers, no optimizer step, host clock between two synchronisations, {args.steps} steps per block, one untimed",
        f"block each, then {args.blocks} blocks of each alternated.  The yardstick is `train_step_policy_gradient`, the single-draw step, in the same call.", "",
        "| step | ms / step, median [min, max] | over the single-draw step |", "|---|---|---|",
        f"| `train_step_policy_gradient` (one draw per observation) | {ms(steps['single_draw'])} | 1.000 |",
    ]
    for G in GROUPS:
        r = steps[f"group_G{G}"]
        md.append(f"| `train_step_policy_gradient_group`, G = {G} | {ms(r)} | {r['ms_median'] / s1:.3f} |")
    r = steps["group_G8_ref_entropy"]
    md += [f"| the same, G = 8, `ref_logprobs`, kl_coef 0.04, entropy_coef 0.01 | {ms(r)} | {r['ms_median'] / s1:.3f} |", "",
           f"G = 8 group step over the single-draw step: {steps['group_G8']['ms_median'] / s1:.3f} (eight single-draw steps would be 8.000).", "",
           "## Reference log-probabilities", "",
           f"`policy_logprobs` and `reference_logprobs` on `[{B}, 8, {A}]` tokens, ms per call, the same clock and alternation.  The reference snapshot holds",
           f"{eng.reference_policy_bytes() / 1e6:.1f} MB; the difference is two copies of it in, two out (stash and restore) and two `refresh_derived()`.", "",
           "| call | ms / call, median [min, max] |", "|---|---|",
           f"| `policy_logprobs` | {ms(lps['policy_logprobs'])} |", f"| `reference_logprobs` | {ms(lps['reference_logprobs'])} |", "",
           "## The kernels", "",
           f"bf16 logits `[{rows}, {cfg.vocab}]`, random normal, each call between its own HIP events, 3 untimed calls, {args.reps} rounds alternated (µs).  `x G` is",
           "G launches of the single-draw kernel between one pair of events.", ""]
    for wname, title in (("actions", "the 256 action ids"), ("vocab", "the whole vocabulary")):
        k = kernels[wname]
        md += [f"Window: {title}.", "", "| kernel | " + " | ".join(f"G = {G}" for G in GROUPS) + " |", "|---|" + "---|" * len(GROUPS),
               "| `token_pg_group` + gradient | " + " | ".join(us(k[f"token_pg_group_G{G}"]) for G in GROUPS) + " |",
               "| `sample_tokens_group` | " + " | ".join(us(k[f"sample_tokens_group_G{G}"]) for G in GROUPS) + " |",
               "| `sample_tokens` x G | " + " | ".join(us(k[f"sample_tokens_x{G}"]) for G in GROUPS) + " |", "",
               f"`token_pg` + gradient (the single-sample kernel): {us(k['token_pg'])}.  `token_pg_group` at G = 8 with old and reference log-probabilities and the",
               f"entropy term: {us(k['token_pg_group_G8_ref_entropy'])}.", ""]
    (out_dir / "pg_group.md").write_text("\n".join(md))
    return 0


if __name__ == "__main__":
    sys.exit(main())
