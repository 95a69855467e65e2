"""The other matmul kernels (gemm_tn, gemm_tn_grouped, colsum) with the exact operands of tests/gemm_reference.py: integer
products add exactly in fp32 whatever the M split, the chunk order or the order atomics land in, so every fp32 result is compared with
torch.equal against float64 and every bf16 one against its single rounding."""
import pytest
import torch

from tests import gemm_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _exact_f32(v64):
    R._exact32(v64, "reference")
    return v64.float()


def test_gemm_tn_every_out_mode(ops, dev):
    """M on both sides of the 64-row K step and of the 256-row M split (one and several partials), P and Q below, at and beyond a tile; X and Y
    are column blocks of wider matrices whose other columns are NaN; accumulate=True adds onto a nonzero integer C; alpha = 0.5."""
    fails = R.Failures()
    g = R.rng(20000)
    for M in (1, 63, 64, 65, 777):
        for P in (8, 32, 136, 264):
            for Q in (8, 32, 136, 264):
                x, y, c0 = R.operand(g, M, P), R.operand(g, M, Q), R.bias_like(g, P, Q).float()
                xe, ye = R.embed(x.to(dev), align=8, fill="nan"), R.embed(y.to(dev), align=8, fill="nan")
                ref = 0.5 * (x.double().T @ y.double())
                what = f"gemm_tn {M},{P},{Q}"
                acc = c0.to(dev)
                ops.gemm_tn(xe.view, ye.view, out=acc, alpha=0.5, accumulate=True)
                fails.exact(acc, _exact_f32(ref + c0.double()), what + " accumulate")
                fails.exact(ops.gemm_tn(xe.view, ye.view, alpha=0.5, accumulate=False, out_dtype=torch.float32), _exact_f32(ref), what + " fp32 store")
                fails.exact(ops.gemm_tn(xe.view, ye.view, alpha=0.5, accumulate=False, out_dtype=BF), R.rbf(ref).to(BF), what + " bf16 store")
    fails.done()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gemm_tn_grouped(ops, dev, n):
    fails = R.Failures()
    g = R.rng(21000 + n)
    sizes = [(777, 264, 32), (300, 32, 136), (65, 8, 264), (1, 136, 8)][:n]
    probs, refs = [], []
    for M, P, Q in sizes:
        x, y, c0 = R.operand(g, M, P), R.operand(g, M, Q), R.bias_like(g, P, Q).float()
        probs.append((R.embed(x.to(dev), align=8, fill="nan").view, R.embed(y.to(dev), align=8, fill="nan").view, c0.to(dev)))
        refs.append(_exact_f32(x.double().T @ y.double() + c0.double()))
    ops.gemm_tn_grouped(probs)
    for (M, P, Q), (_, _, out), ref in zip(sizes, probs, refs):
        fails.exact(out, ref, f"grouped problem {M},{P},{Q} of {n}")
    fails.done()


def test_colsum(ops, dev):
    fails = R.Failures()
    g = R.rng(23000)
    for M in (1, 255, 257, 1000):
        for N in (8, 264):
            x, o0 = R.operand(g, M, N), R.bias_like(g, N).float()
            xe = R.embed(x.to(dev), align=8, fill="nan")
            out = o0.to(dev)
            ops.colsum(xe.view, out)
            fails.exact(out[None], _exact_f32(x.double().sum(0) + o0.double())[None], f"colsum {M}x{N}")
    fails.done()
