"""The diffusion-noise contract (include/ovla.h "Diffusion noise") on the CPU: the numpy restatement of tests/diffusion_noise_reference.py is
itself a sound N(0, 1) / uniform generator, a draw is a function of (seed, call, stream, sample, element) only, and the host tables the kernel
reads are the scheduler's and the time encoder's own numbers.  No GPU."""
import importlib

import numpy as np
import pytest
import torch

import diffusion_noise_reference as R
from lora_dropout_reference import KNOWN_ANSWERS, philox4x32_10

SEEDS = (7, 7 + 2 ** 32)
CALLS = (0, 1, 2)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("call", CALLS)
def test_normals_have_the_moments_of_a_standard_normal(seed, call):
    B, n = 64, 56
    z = R.normals(B, n, call=call, seed=seed)
    N = z.size
    assert N == 3584
    m, v, big = abs(z.mean()) * np.sqrt(N), z.var(), np.abs(z).max()
    print(f"seed {seed} call {call}: |mean| sqrt(N) {m:.3f}, variance {v:.4f}, max |z| {big:.3f}")
    assert m < 3
    assert 0.9 <= v <= 1.1
    assert big < 5.8 and R.Z_MAX < 5.8        # the construction's bound is 5.77


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("call", CALLS)
def test_timesteps_are_uniform(seed, call):
    B, T = 4096, 50
    t = R.timesteps(B, T, call=call, seed=seed)
    assert t.min() == 0 and t.max() == 49
    counts = np.bincount(t, minlength=T)
    chi2 = float(((counts - B / T) ** 2 / (B / T)).sum())
    print(f"seed {seed} call {call}: chi^2(49) = {chi2:.1f}")
    assert chi2 < 85


def test_generator_is_the_lora_dropout_one():
    for ctr, key, want in KNOWN_ANSWERS:
        assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == want
    o = R.words(np.array([3], np.uint64), np.array([5], np.uint64), 2, 9, 7 + (1 << 32))
    assert tuple(int(w[0]) for w in o) == tuple(int(w) for w in philox4x32_10(3, 5, 2, 9, 7, 1))


def test_a_draw_does_not_depend_on_the_batch():
    big = R.normals(8, 350, call=4, seed=11)
    for b in (0, 3, 7):
        assert np.array_equal(R.normals(1, 350, call=4, seed=11, b0=b)[0], big[b])
    assert np.array_equal(R.normals(3, 350, call=4, seed=11), big[:3])
    assert np.array_equal(R.normals(8, 5, call=4, seed=11), big[:, :5])           # nor on n: a tail discards, it does not re-deal
    tb = R.timesteps(8, 50, call=4, seed=11)
    assert np.array_equal(R.timesteps(3, 50, call=4, seed=11, b0=2), tb[2:5])


def test_call_seed_and_stream_each_change_every_word():
    j, b = np.arange(64, dtype=np.uint64)[None, :], np.arange(8, dtype=np.uint64)[:, None]
    base = R.words(j, b, 0, 5, 7)
    for other in (R.words(j, b, 0, 6, 7), R.words(j, b, 0, 5, 8), R.words(j, b, 0, 5, 7 + 2 ** 32), R.words(j, b, 2, 5, 7), R.words(j, b, 1, 5, 7)):
        for w0, w1 in zip(base, other):
            assert not (w0 == w1).any()


def test_exact_argument_reduction():
    u = np.arange(0, 2 ** 12, dtype=np.float64) * 2.0 ** -12
    c, s = R.cos_sin_2pi(u)
    assert np.abs(c - np.cos(2 * np.pi * u)).max() < 1e-15 and np.abs(s - np.sin(2 * np.pi * u)).max() < 1e-15
    quarter = 2 ** 10
    assert [c[0], s[0], c[quarter], s[quarter], c[2 * quarter], s[2 * quarter], c[3 * quarter], s[3 * quarter]] == [1, 0, 0, 1, -1, 0, 0, -1]


def test_bf16_bracket():
    z = np.array([0.0, 1.0, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -9, 1.0 - 2.0 ** -12, 3.3, -2.0 ** -20 * 1.3])
    lo, hi = R.bf16_bracket(z)
    assert np.all(lo <= z) and np.all(z <= hi)
    assert list(lo[:2]) == [0.0, 1.0] and list(hi[:2]) == [0.0, 1.0]
    assert (lo[2], hi[2]) == (1.0, 1.0 + 2.0 ** -7) and (lo[3], hi[3]) == (-1.0 - 2.0 ** -7, -1.0)
    assert (lo[4], hi[4]) == (1.0 - 2.0 ** -8, 1.0)                               # below a power of two the spacing halves
    assert np.all(hi[2:] - lo[2:] <= R.bf16_ulp(z[2:]))


def test_host_tables_are_the_schedulers_own_numbers():
    """ab row t = add_noise's two factors; with them, the three fp32 operations of the contract are add_noise bit for bit."""
    diffusion = importlib.import_module("openvla-oft_amd.diffusion")
    from lora_dropout_reference import from_bits, to_bits

    T = 50
    sched = diffusion.DDIMScheduler(T)
    ab = sched.add_noise_coefficients()
    assert ab.dtype == torch.float32 and tuple(ab.shape) == (T, 2) and ab.is_contiguous()
    assert torch.equal(ab[:, 0], sched.alphas_cumprod ** 0.5) and torch.equal(ab[:, 1], (1 - sched.alphas_cumprod) ** 0.5)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, 56, generator=g).to(torch.bfloat16)
    nz = torch.randn(T, 56, generator=g).to(torch.bfloat16)
    t = torch.arange(T)
    want = sched.add_noise(x.float(), nz.float(), t).to(torch.bfloat16)
    got = from_bits(R.add_noise_bits(to_bits(x), to_bits(nz), ab.numpy(), t.numpy()))
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
