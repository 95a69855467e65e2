"""ovla_ddim_step / ovla_ddim_prepare (csrc/ddim.hip): the DDIM sampler's per-step host work on the device, bit for bit the CPU torch expression
the host loop evaluates (`DDIMScheduler.step(eps, t, sample).prev_sample.to(bf16).float()`), driven by a device-side step index."""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
load = importlib.import_module

SCHEDULES = [(50, 50), (100, 5)]          # (training timesteps T, sampling steps)
SIZES = [56, 350, 3 * 350]                # 8 x 7 (less than a wave), 25 x 14 (no multiple of 4), three ALOHA chunks (more than one pass of the workgroup)


def _steps(n_steps):
    return [0, n_steps // 2, n_steps - 1]  # first (largest t), a middle one, last (prev_t < 0: final_alpha_cumprod, c3 = 0)


@pytest.fixture(scope="module")
def cases():
    """Every (T, n_steps, n, k) case once, on the CPU: inputs, the scheduler's own result, and which elements its clamp changed."""
    diffusion = load("openvla-oft_amd.diffusion")
    out, gen = [], torch.Generator().manual_seed(11)
    for T, n_steps in SCHEDULES:
        sched = diffusion.DDIMScheduler(num_train_timesteps=T)
        sched.set_timesteps(n_steps)
        coef = sched.step_coefficients()
        for n in SIZES:
            for k in _steps(n_steps):
                t = int(sched.timesteps[k])
                sample = torch.randn(n, generator=gen).to(BF).float()
                eps = torch.randn(n, generator=gen).to(BF)
                ref = sched.step(eps.float(), t, sample).prev_sample.to(BF).float()
                a_t = sched.alphas_cumprod[t]
                x0 = (sample - (1 - a_t) ** 0.5 * eps.float()) / a_t ** 0.5
                out.append(dict(T=T, n_steps=n_steps, n=n, k=k, coef=coef, sample=sample, eps=eps, ref=ref, clamped=(x0.abs() > 1.0)))
    return out


def test_reference_exercises_both_sides_of_the_clamp(cases):
    """For N(0, 1) inputs x0 leaves [-1, 1] for about a third of the elements at small t and for nearly all at the largest t: both branches of
    the kernel's clamp are compared below."""
    clamped = torch.cat([c["clamped"] for c in cases]).float().mean().item()
    last = torch.cat([c["clamped"] for c in cases if c["k"] == c["n_steps"] - 1]).float().mean().item()
    first = torch.cat([c["clamped"] for c in cases if c["k"] == 0]).float().mean().item()
    print(f"clamped: {clamped:.3f} of all elements, {last:.3f} at the last step, {first:.3f} at the first")
    assert clamped >= 0.10 and 1.0 - clamped >= 0.10
    assert 0.2 < last < 0.45 and first > 0.5   # P(|N(0, 1)| > 1) = 0.317 at t = 0; x0 is the inputs over a small a_t^1/2 at the largest t


def test_ddim_step_matches_cpu_scheduler_bit_for_bit(dev, ops, cases):
    clamped = torch.cat([c["clamped"] for c in cases]).float().mean().item()
    assert clamped >= 0.10 and 1.0 - clamped >= 0.10
    for c in cases:
        sample = c["sample"].to(dev)
        step = torch.tensor([c["k"]], dtype=torch.int32, device=dev)
        ops.ddim_step(sample, c["eps"].to(dev), c["coef"].to(dev), step)
        got = sample.cpu().numpy()
        tag = f"T={c['T']} steps={c['n_steps']} n={c['n']} k={c['k']}"
        assert np.array_equal(got, c["ref"].numpy()), f"{tag}: {np.sum(got != c['ref'].numpy())} of {c['n']} elements differ"
        assert int(step.item()) == c["k"] + 1, f"{tag}: the step index advances by one per call"


def test_step_index_walks_the_schedule_and_stops(dev, ops):
    """Five calls on one device index = the five-step host loop; a sixth call (k = n_steps) changes neither the sample nor the index."""
    diffusion = load("openvla-oft_amd.diffusion")
    sched = diffusion.DDIMScheduler(num_train_timesteps=100)
    sched.set_timesteps(5)
    gen = torch.Generator().manual_seed(12)
    cur = torch.randn(350, generator=gen).to(BF).float()
    eps = [torch.randn(350, generator=gen).to(BF) for _ in range(5)]
    sample, step, coef = cur.to(dev), torch.zeros(1, dtype=torch.int32, device=dev), sched.step_coefficients().to(dev)
    for k, t in enumerate(sched.timesteps):
        cur = sched.step(eps[k].float(), int(t), cur).prev_sample.to(BF).float()
        ops.ddim_step(sample, eps[k].to(dev), coef, step)
        assert int(step.item()) == k + 1
        assert np.array_equal(sample.cpu().numpy(), cur.numpy()), f"step {k}"
    ops.ddim_step(sample, eps[0].to(dev), coef, step)
    assert int(step.item()) == 5 and np.array_equal(sample.cpu().numpy(), cur.numpy())
    # ... and its other consumer, ovla_ddim_prepare, writes nothing at k = n_steps either
    table = torch.randn(5, 64, generator=gen).to(BF).to(dev)
    temb, noisy = torch.full((3, 64), 7.0, dtype=BF, device=dev), torch.full((350,), 7.0, dtype=BF, device=dev)
    ops.ddim_prepare(step, table, temb, sample, noisy)
    assert bool((temb == 7.0).all()) and bool((noisy == 7.0).all())


@pytest.mark.parametrize("B,n,D", [(1, 56, 64), (3, 3 * 350, 200)])
def test_ddim_prepare_writes_row_k_and_the_rounded_sample(dev, ops, B, n, D):
    gen = torch.Generator().manual_seed(13)
    table = torch.randn(5, D, generator=gen).to(BF)
    sample = torch.randn(n, generator=gen)                 # full fp32 values: the kernel's rounding to bf16 is torch's (nearest even)
    for k in (0, 3, 4):
        step = torch.tensor([k], dtype=torch.int32, device=dev)
        temb, noisy = torch.zeros((B, D), dtype=BF, device=dev), torch.zeros(n, dtype=BF, device=dev)
        ops.ddim_prepare(step, table.to(dev), temb, sample.to(dev), noisy)
        assert torch.equal(temb.cpu(), table[k][None].expand(B, D)), f"k={k}: every observation's timestep slot holds row k"
        assert torch.equal(noisy.cpu(), sample.to(BF)), f"k={k}: noisy actions = bf16(sample)"
        assert int(step.item()) == k, "prepare leaves the index alone"
