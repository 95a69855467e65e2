"""The kernels of csrc/elementwise.hip against the float64 references of tests/pointwise_reference.py: bit equality wherever the result does not
depend on the order of fp32 sums (RoPE, copies, casts, every accumulator fed from the exact-regime generators), derived bf16-ulp bounds and
absolute floors per element everywhere else, every output a wrapper lets the caller place inside sentinel guards, activations over the whole
finite bf16 domain, and one launch per capped kernel that needs a second trip of its grid-stride loop.

The suites (shapes, data, checks) live in tests/pointwise_reference.py and are the ones tests/test_pointwise_reference.py runs on an fp32
emulation with planted bugs; here `GpuKernels` hands them the real launches.
"""
import pytest
import torch

from tests import pointwise_reference as P

pytestmark = pytest.mark.gpu


def run(suite, ops, dev, **kw):
    fails = P.Checks()
    suite(fails, P.GpuKernels(ops, dev, fails), **kw)
    fails.done()


def test_norm_forward_every_dispatch_edge(ops, dev):
    """dim 8 ... 4104 on both sides of <2> | <3> | workgroup, rows on both sides of the 4 rows per workgroup, RMS and LayerNorm, bias on / off,
    save_stats on / off: y per element, mean and rstd against float64, and per kernel variant rows of +-2^k whose mean is exactly 0."""
    run(P.suite_norm_fwd, ops, dev)


def test_norm_backward_exact_accumulators_and_real_statistics(ops, dev):
    """dw / db exact onto nonzero integers from handed-in statistics, dx and dx_accum within the derived bound; then real statistics."""
    run(P.suite_norm_bwd, ops, dev)


def test_rope_bit_exact_and_table(ops, dev):
    """head_dim 8 / 64 / 72 / 128, ld beyond the rotated columns with NaN there, rows = 3 S and rows % S != 0, forward and inverse, 1040 x 64 x
    128 (a second trip of the grid-stride loop); the S = 2048 tables against float64."""
    run(P.suite_rope, ops, dev)


def test_activations_over_every_finite_bf16(ops, dev):
    """act_bwd (acts 0 .. 4), swiglu_fwd and swiglu_bwd with every finite bf16 bit pattern as z / g: finite, +-0 where float64 has underflowed,
    1 ulp (2 for the SwiGLU pair) + fast_erf's floor everywhere (the extremes where gelu_tanh' would be 0 * inf, the 6 to 17 inputs per kernel
    between the overflow of exp at -88.7 and the underflow of the result at -104 included)."""
    run(P.suite_activations, ops, dev)


def test_copies_and_casts_bit_exact(ops, dev):
    run(P.suite_elementwise, ops, dev)


@pytest.mark.parametrize("part", [p for p in P.WRAP_PARTS if not p.startswith("adamw")])
def test_second_trip_of_the_grid_stride_loop(ops, dev, part):
    run(P.suite_wrap, ops, dev, parts=(part,))


def test_film_backward_and_masked_mean(ops, dev):
    run(P.suite_film_mean, ops, dev)


def test_zz_report_worst_ratios():
    print("\nworst observed |err| / bound:", " ".join(f"[{k}] {v:.2f}" for k, v in sorted(P.Checks.worst.items())))
    assert all(v <= 1.0 for v in P.Checks.worst.values())
