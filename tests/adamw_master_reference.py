"""The master-weight AdamW contract (include/ovla.h "AdamW on fp32 master weights") restated on CPU tensors, and the suite the GPU test and the
CPU test share.  The restatement composes three things that exist already and are not touched: the op-by-op fp32 AdamW emulation of
tests/pointwise_reference.py, the gradient and clip rule of tests/grad_clip_reference.py (is_bf16 = False: the optimizer-side dtype is fp32)
and torch's `.to(bfloat16)` (round to nearest even, NaN stays NaN, overflow gives +-inf).  Independent of the package; every comparison is
bit for bit.

    r = fp32(g * grad_scale) [ * coef ];  (master, m, v) <- adamw_f32(master, m, v, r);  param <- bf16(master);  a skipped step changes nothing
"""
import numpy as np
import torch

from tests import grad_clip_reference as R
from tests.pointwise_reference import ADAMW_GRID, adamw_emulate, adamw_inputs, rng, same_bits

BF = torch.bfloat16
MUTANTS = ("bf16_grad", "stale_param", "bf16_moments", "write_on_skip")
SIZES = (1, 3, 4, 5, 1021, 2048 + 77)      # the scalar tail alone, one group, a group and a tail, four workgroups short of full, nine with a tail


def adamw_master(master, m, v, param, g, *, state=None, grad_scale=1.0, mut=None, **hp):
    """ovla_adamw_master on CPU tensors (master, m, v, g fp32; param bf16): the new (master, m, v, param).  `state`: None, or a dict with `skip`
    and `coef` as grad_clip_reference.clip_coef returns it.  `mut` plants one bug:
      bf16_grad      the gradient rounded to bf16, as ovla_adamw forms it for a bf16 buffer
      stale_param    param cast from the OLD master
      bf16_moments   the moments rounded through bf16 on their way back
      write_on_skip  param still written (from the master) on a skipped step"""
    assert mut is None or mut in MUTANTS
    assert master.dtype == m.dtype == v.dtype == g.dtype == torch.float32 and param.dtype == BF
    if state is not None and state["skip"]:
        return master, m, v, (master.to(BF) if mut == "write_on_skip" else param)
    as_bf16 = mut == "bf16_grad"
    grad = R.seen_gradient(g.numpy(), grad_scale, as_bf16) if state is None else R.clipped_gradient(g.numpy(), grad_scale, state["coef"], as_bf16)
    new_master, new_m, new_v = adamw_emulate(master, m, v, torch.from_numpy(np.ascontiguousarray(grad)), grad_scale=1.0, **hp)   # (x * 1.0f is x)
    if mut == "bf16_moments":
        new_m, new_v = new_m.to(BF).float(), new_v.to(BF).float()
    return new_master, new_m, new_v, (master if mut == "stale_param" else new_master).to(BF)


def master_inputs(seed, n):
    """pointwise_reference.adamw_inputs in fp32 (a zero-state block, large parameters with tiny gradients, gradients from 1e-8 to 1e2), the bf16
    parameter that goes with the master, and three gradients for three consecutive steps."""
    g = rng(seed)
    master, m, v, _ = adamw_inputs(g, n, torch.float32)
    grads = [adamw_inputs(g, n, torch.float32)[3] for _ in range(3)]
    return master, m, v, master.to(BF), grads


def not_the_cast(master):
    """A bf16 tensor that differs from bf16(master) in every element: what a skipped step must leave alone."""
    return (master.to(BF).view(torch.int16) ^ 0x0155).view(BF)


def suite_master(fails, K, sizes=SIZES, grid=ADAMW_GRID):
    """K.adamw_master(master, m, v, param, g, state, **hp) -> the four new CPU tensors.  Three consecutive steps over the hyperparameter grid of
    suite_adamw at every size; then the clip state: coef == 1 is the call without a state, coef < 1 is the restatement, a skip leaves all four
    buffers -- a param that is NOT bf16(master) included -- as they were."""
    names = ("master", "exp_avg", "exp_avg_sq", "param")
    for n in sizes:
        master0, m0, v0, param0, grads = master_inputs(1000 + n, n)
        for lr, wd, gs, b2, eps in grid:
            got = want = (master0, m0, v0, param0)
            for k, g in enumerate(grads):
                hp = dict(step=k + 1, lr=lr, beta2=b2, eps=eps, weight_decay=wd, grad_scale=gs)
                want = adamw_master(*want, g, **hp)
                got = K.adamw_master(*got, g, None, **hp)
                for name, a, b in zip(names, got, want):
                    same_bits(fails, a, b, f"adamw_master n {n} lr {lr} wd {wd} grad_scale {gs} beta2 {b2} eps {eps} step {k + 1}: {name}")
                got = want          # the next step starts from the restatement's state: one wrong step is reported once
        hp = dict(step=3, lr=5e-4, grad_scale=1.0 / 3.0)
        start = (master0, m0, v0, param0)
        plain = K.adamw_master(*start, grads[0], None, **hp)
        for name, a, b in zip(names, K.adamw_master(*start, grads[0], dict(skip=0, coef=np.float32(1.0)), **hp), plain):
            same_bits(fails, a, b, f"adamw_master n {n}: coef == 1 against no clip state: {name}")
        state = dict(skip=0, coef=np.float32(0.37))
        clipped = K.adamw_master(*start, grads[0], state, **hp)
        for name, a, b in zip(names, clipped, adamw_master(*start, grads[0], state=state, **hp)):
            same_bits(fails, a, b, f"adamw_master n {n}: coef 0.37 against the restatement: {name}")
        fails.check(not torch.equal(clipped[0], plain[0]), f"adamw_master n {n}: the coefficient is applied")
        odd = (master0, m0, v0, not_the_cast(master0))
        for name, a, b in zip(names, K.adamw_master(*odd, grads[0], dict(skip=1, coef=np.float32(0.5)), **hp), odd):
            same_bits(fails, a, b, f"adamw_master n {n}: a skipped step must keep the bits of {name}")


class Restated:
    """The suite's K for the restatement itself, with or without a planted bug."""

    def __init__(self, mut=None):
        self.mut = mut

    def adamw_master(self, master, m, v, param, g, state, **hp):
        return adamw_master(master, m, v, param, g, state=state, mut=self.mut, **hp)


# ---- the two defects of bf16 optimizer state, as sequences the tests replay ---------------------------------------------------------------------
def lost_update_run(steps, dtype, lr=1e-4):
    """p = 1, constant gradient 1, weight_decay 0: the published parameter (a Python float) after each of `steps` steps, with the state in
    `dtype` (bf16: ovla_adamw's torch-faithful path; fp32: the master path, where the published value is bf16(master))."""
    one = torch.ones(1)
    if dtype == BF:
        p, m, v = one.to(BF), torch.zeros(1, dtype=BF), torch.zeros(1, dtype=BF)
    else:
        p, m, v, pub = one.clone(), torch.zeros(1), torch.zeros(1), one.to(BF)
    out = []
    for k in range(1, steps + 1):
        if dtype == BF:
            p, m, v = adamw_emulate(p, m, v, one, step=k, lr=lr, weight_decay=0.0)
            out.append(float(p))
        else:
            p, m, v, pub = adamw_master(p, m, v, pub, one, step=k, lr=lr, weight_decay=0.0)
            out.append(float(pub))
    return out
