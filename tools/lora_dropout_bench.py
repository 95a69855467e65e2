"""What lora_dropout > 0 costs (csrc/lora_dropout.hip) at the fine-tune shapes of BASELINE.json configs[2] (M = 4864, r = 32).
  kernels   per launch: the fused projection (proj), the masked dx update (backproj) and the materialising kernel (apply) for q|k|v, o, gate|up and
            down, next to the p = 0 projection GEMM and to each kernel's bytes at the achievable HBM rate DESIGN.md section 4 uses (6.3 TB/s).
            Rotating operand sets larger than the 256 MB Infinity Cache keep the reads cold, as inside the step.
  --step    the whole train step (bench.py's step) at p = 0, p = 0.05 fused and p = 0.05 unfused, alternated in ONE process on one engine.
Prints one line per measurement; nothing is asserted."""
import argparse
import importlib
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module
ops = load("openvla-oft_amd.ops")
dev = torch.device("cuda:0")
BF = torch.bfloat16
HBM = 6.3e12   # achievable bytes / s


def bench(fn, iters=36):
    for i in range(6):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us


def kernels(M, p):
    r, s = 32, 0.5
    key = dict(p=p, seed=7, call=1)
    print(f"# M = {M}, r = {r}, p = {p}; us per launch (floor = bytes at {HBM / 1e12} TB/s)")
    for name, G, K in [("qkv", 3, 4096), ("o", 1, 4096), ("gate_up", 2, 4096), ("down", 1, 11008)]:
        mods = list(range(G))
        NSET = -(-320_000_000 // (M * K * 2)) + 1     # the rotated x sets total more than the 256 MB Infinity Cache at every K
        xs = [torch.randn(M, K, device=dev).to(BF) for _ in range(NSET)]
        dxs = [torch.randn(M, K, device=dev).to(BF) for _ in range(NSET)]   # backproj works in place: buffers of its own
        dts = [torch.randn(M, G * r, device=dev).to(BF) for _ in range(NSET)]
        A = (torch.randn(G * r, K, device=dev) / r).to(BF)
        AT = A.T.contiguous()
        xd = torch.empty((G, M, K), dtype=BF, device=dev)
        t0 = bench(lambda i: ops.gemm(xs[i % NSET], A, alpha=s))
        t1 = bench(lambda i: ops.lora_dropout_proj(xs[i % NSET], A, alpha=s, modules=mods, **key))
        t2 = bench(lambda i: ops.lora_dropout_backproj(dxs[i % NSET], dts[i % NSET], AT, modules=mods, **key))
        t3 = bench(lambda i: ops.lora_dropout_apply(xs[i % NSET], modules=mods, out=xd, **key))
        xb = M * K * 2
        fl = lambda nbytes: nbytes / HBM * 1e6  # noqa: E731
        print(f"{name:8s} K {K:5d} G {G} | proj p=0 (gemm) {t0:6.1f} | proj {t1:6.1f} (floor {fl(xb):5.1f}) | backproj {t2:6.1f} (floor {fl(2 * xb):5.1f}) | "
              f"apply {t3:6.1f} (floor {fl((1 + G) * xb):5.1f})", flush=True)


def step(rounds, steps):
    E, Wm, synth, config_mod = (load("openvla-oft_amd." + m) for m in ("engine", "weights", "synthetic", "config"))
    cfg = config_mod.OPENVLA_7B
    sd = Wm.random_state_dict(cfg, dev, seed=0, lm_head=False)
    get, has = Wm.make_getter(sd, dev)
    eng = E.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="l1", has=has, lora_dropout=0.05, dropout_seed=7)
    del sd, get
    torch.cuda.empty_cache()
    batch = synth.make_batch(8, seed=1000, num_images=cfg.num_images, chunk=cfg.chunk, action_dim=cfg.action_dim, proprio_dim=cfg.proprio_dim)
    for k in ("pixel_values", "actions", "proprio"):
        batch[k] = batch[k].to(dev, BF)

    def one(_):
        eng.zero_grad()
        eng.train_step_fwd_bwd(batch)
        eng.adamw_step(lr=5e-4)
        eng.refresh_derived()

    modes = [("p=0", 0.0, True), ("p=0.05 fused", 0.05, True), ("p=0.05 unfused", 0.05, False)]
    for rnd in range(rounds):
        for name, p, fused in modes:
            eng.dropout.p, E._LORA_DROPOUT_FUSED = p, fused
            print(f"round {rnd} {name:15s} {bench(one, iters=steps) / 1e3:7.2f} ms/step", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=4864)
    ap.add_argument("--p", type=float, default=0.05)
    ap.add_argument("--step", action="store_true", help="also time the whole train step (full-size model)")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=8)
    a = ap.parse_args()
    kernels(a.M, a.p)
    if a.step:
        step(a.rounds, a.steps)
