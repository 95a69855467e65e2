"""The kernels of csrc/head_optim.hip against tests/pointwise_reference.py: token cross-entropy with planted ties and derived bounds, the head
output layer in the exact regime (pred, loss_sum and every gradient bit for bit, onto nonzero accumulators), and AdamW bit for bit against
the op-by-op fp32 emulation of the kernels' documented sequence.  The suites are shared with tests/test_pointwise_reference.py (CPU emulation
with planted bugs); `GpuKernels` hands them the real launches.
"""
import pytest
import torch

from tests import pointwise_reference as P

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def run(suite, ops, dev, **kw):
    fails = P.Checks()
    suite(fails, P.GpuKernels(ops, dev, fails), **kw)
    fails.done()


def test_token_ce_ties_padding_bounds(ops, dev):
    """vocab 1 ... 1000 with ld = vocab rounded up to 8, + 8 (padding +3e38 / NaN) and one row of 32064: first maximum with ties inside a
    thread, across lanes and across waves, target clamps, loss and gradient per element, in place = out of place, rows without a maximum."""
    run(P.suite_token_ce, ops, dev)


@pytest.mark.parametrize("dim", P.HEAD_DIMS)
def test_head_output_exact(ops, dev, dim):
    run(P.suite_head, ops, dev, dims=(dim,))


def test_head_output_refuses_what_it_cannot_run(ops, dev):
    ovla_error = ops._lib.OvlaError
    x = lambda r, d: torch.ones((r, d), dtype=BF, device=dev)  # noqa: E731
    with pytest.raises(ovla_error):
        ops.head_out_fwd(x(4, 64), x(17, 64), None)                       # adim 17
    with pytest.raises(ovla_error):
        ops.head_out_fwd(x(4, 12), x(7, 12), None)                        # dim 12: no whole 16-byte chunks
    dW, db = torch.zeros((17, 64), device=dev), torch.zeros(17, device=dev)
    with pytest.raises(ovla_error):
        ops.head_out_bwd(x(4, 64), x(17, 64), x(4, 17), x(4, 17), 1.0, dW, db)
    rows = 48 * 1024 // (16 * 4) + 1                                      # rows * adim * 4 bytes just over the 48 KB slab
    dW, db = torch.zeros((16, 64), device=dev), torch.zeros(16, device=dev)
    with pytest.raises(ovla_error):
        ops.head_out_bwd(x(rows, 64), x(16, 64), x(rows, 16), x(rows, 16), 1.0, dW, db)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_adamw_bit_exact_over_the_hyperparameter_grid(ops, dev, dtype):
    run(P.suite_adamw, ops, dev, dtypes=(BF if dtype == "bf16" else torch.float32,))


@pytest.mark.parametrize("part", ["adamw_bf16", "adamw_f32"])
def test_adamw_second_trip_of_the_grid_stride_loop(ops, dev, part):
    run(P.suite_wrap, ops, dev, parts=(part,))


def test_zz_report_worst_ratios():
    print("\nworst observed |err| / bound:", " ".join(f"[{k}] {v:.2f}" for k, v in sorted(P.Checks.worst.items())))
    assert all(v <= 1.0 for v in P.Checks.worst.values())
