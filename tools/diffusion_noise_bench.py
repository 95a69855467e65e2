"""The diffusion fine-tune step with host noise against device noise at full size (BASELINE.json configs[5] shapes: OpenVLA-7B, FiLM, 3 images,
chunk 25 x 14, proprio 14, 50 training timesteps; synthetic weights and batches): ms per step (fwd + bwd + AdamW) of the loop of
`finetune()` with `make_diffusion`'s host arithmetic -- actions to the CPU, torch.randn / randint from a CPU generator, add_noise and the time
encoder on the host, three uploads -- and with VLAEngine.draw_diffusion (one ovla_diffusion_noise launch, nothing read back).  The two are
ALTERNATED in one process in blocks of `--steps` steps, `--reps` blocks each, every block timed by a host clock between two device
synchronisations; one JSON line with every block's time, so the alternation's own spread can be read beside the difference.
Usage: python tools/diffusion_noise_bench.py [--batch 4] [--steps 6] [--reps 3] > profiles/diffusion_noise_bench.jsonl"""
import argparse
import dataclasses
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    engine_mod, weights_mod, synth, config_mod, dmod = (load(f"openvla-oft_amd.{m}") for m in ("engine", "weights", "synthetic", "config", "diffusion"))
    dev = torch.device("cuda:0")
    T = 50
    cfg = dataclasses.replace(config_mod.OPENVLA_7B, num_images=3, chunk=25, action_dim=14, proprio_dim=14, norm_type="bounds")
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, film=True, diffusion=True)
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(cfg, get, dev, lora=True, use_proprio=True, head="diffusion", use_film=True, has=has, num_diffusion_steps=T, diffusion_seed=7)
    del sd
    batches = [synth.make_batch(args.batch, seed=1000 + i, num_images=3, chunk=25, action_dim=14, proprio_dim=14) for i in range(args.steps)]
    sched, enc, gen = dmod.DDIMScheduler(T), dmod.SinusoidalPositionalEncoding(cfg.llm_dim), torch.Generator().manual_seed(7)

    def host_noise(batch):   # make_diffusion of vla_scripts/finetune.py
        gt = batch["actions"].to("cpu", torch.float32)
        noise = torch.randn(gt.shape, generator=gen).to(BF).float()
        ts = torch.randint(0, T, (gt.shape[0],), generator=gen)
        return dict(noise=noise, noisy_actions=sched.add_noise(gt, noise, ts).to(BF), timestep_emb=enc(ts.float()).to(BF))

    def block(device_noise):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in batches:
            d = eng.draw_diffusion(batch["actions"]) if device_noise else host_noise(batch)
            loss_sum, count, _ = eng.train_step_fwd_bwd(batch, diffusion=d)
            eng.adamw_step(1e-5)
            eng.refresh_derived()
            eng.zero_grad()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(batches), loss_sum.item() / count

    eng.zero_grad()
    block(False), block(True)      # warm-up of both variants: lazy tables, workspaces, kernel attributes
    host, device, losses = [], [], []
    for _ in range(args.reps):
        ms, loss = block(False)
        host.append(ms)
        ms, loss_d = block(True)
        device.append(ms)
        losses.append((loss, loss_d))
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps(dict(metric="diffusion fine-tune step, ms/step: host noise vs device noise (7B, FiLM, 3 images, 25 x 14, T = 50)", batch=args.batch,
                          steps_per_block=args.steps, host_ms=host, device_ms=device, host_ms_median=med(host), device_ms_median=med(device),
                          device_minus_host_ms=med(device) - med(host), finite=bool(np.isfinite(losses).all()))), flush=True)


if __name__ == "__main__":
    main()
