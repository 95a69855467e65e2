"""The master-weight AdamW restatement (tests/adamw_master_reference.py) on the CPU: the suite passes on the restatement and catches each
planted bug, and the two facts that motivate fp32 optimizer state hold in torch's own bf16 arithmetic."""
import pytest
import torch

from tests import adamw_master_reference as M
from tests.gemm_reference import Failures
from tests.pointwise_reference import ADAMW_GRID

BF = torch.bfloat16
SMALL = dict(sizes=(3, 5, 256 + 77), grid=ADAMW_GRID[::5])     # the CPU run of the suite: the same cases on fewer sizes and hyperparameters


def run_suite(mut):
    fails = Failures()
    M.suite_master(fails, M.Restated(mut), **SMALL)
    return fails


def test_the_suite_passes_on_the_restatement():
    run_suite(None).done()


@pytest.mark.parametrize("mut,where", [("bf16_grad", "step 1: exp_avg"), ("stale_param", "step 1: param"), ("bf16_moments", "step 1: exp_avg_sq"),
                                       ("write_on_skip", "a skipped step must keep the bits of param")])
def test_the_suite_catches_each_planted_bug(mut, where):
    fails = run_suite(mut)
    assert fails and any(where in f for f in fails), f"{mut}: {fails[:3]}"
    if mut == "write_on_skip":
        assert all("skipped step" in f for f in fails), "only the skip case sees this bug"


def test_publication_is_the_cast_of_the_new_master_and_the_invariant_holds():
    master, m, v, param, grads = M.master_inputs(7, 300)
    for k, g in enumerate(grads):
        master, m, v, param = M.adamw_master(master, m, v, param, g, step=k + 1, lr=1e-2)
        assert torch.equal(param.view(torch.int16), master.to(BF).view(torch.int16))


def test_bf16_second_moment_never_decays():
    """exp_avg_sq.mul_(0.999) returns its input for every positive normal bf16 value: the decrement is below half an ulp."""
    bits = torch.arange(0x0080, 0x7F80, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF)
    assert v.numel() == 32512 and bool(torch.isfinite(v.float()).all()) and float(v.float().min()) == 2.0 ** -126
    assert torch.equal(v.mul(0.999).view(torch.int16), bits)
    assert bool((v.float().mul(0.999) < v.float()).all()), "in fp32 every one of them decays"


def test_bf16_parameter_loses_small_updates_and_the_master_keeps_them():
    """p = 1, g = 1, lr = 1e-4, wd = 0: the bf16 parameter is still exactly 1.0 after 40 steps; the rounded master first leaves 1.0 at step 20."""
    def torch_run(dtype):
        p = torch.nn.Parameter(torch.ones(1, dtype=dtype))
        opt = torch.optim.AdamW([p], lr=1e-4, weight_decay=0.0)
        out = []
        for _ in range(40):
            p.grad = torch.ones(1, dtype=dtype)
            opt.step()
            out.append(float(p.detach().to(BF)))
        return out, float(p.detach())

    bf, _ = torch_run(BF)
    assert bf == [1.0] * 40 and M.lost_update_run(40, BF) == bf
    pub, last = torch_run(torch.float32)
    assert pub[:19] == [1.0] * 19 and pub[19] == 0.99609375 and abs(last - 0.9960) < 1e-5, (pub[15:22], last)
    assert M.lost_update_run(40, torch.float32) == pub, "the restatement publishes what torch's fp32 AdamW rounds to"
