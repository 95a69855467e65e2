"""ovla_adamw_master on the GPU, bit for bit: against the restatement (tests/adamw_master_reference.py), against the fp32 form of ovla_adamw /
ovla_adamw_clipped followed by a cast, at the edge values of the bf16 publication, behind the clip state, across a second trip of the
grid-stride loop, at its refusals, and on the two sequences that show what bf16 optimizer state loses.  Every output sits in a guarded buffer."""
import importlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import adamw_master_reference as M
from tests.gemm_reference import Failures
from tests.pointwise_reference import Guarded, adamw_inputs, rng, same_bits

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BF = torch.bfloat16
F32 = torch.float32
load = importlib.import_module
NAMES = ("master", "exp_avg", "exp_avg_sq", "param")


def device_state(dev, state):
    """None, or a device ovla_grad_clip_state as ovla_grad_clip_coef would have left it, written from the host."""
    if state is None:
        return None
    words = np.zeros(6, np.int32)
    words[0:2] = np.array([state["coef"], 123.0], np.float32).view(np.int32)
    words[2] = state["skip"]
    return torch.from_numpy(words).to(dev)


class GpuMaster:
    """The suite's K for the real kernel: CPU tensors in, one launch on guarded device buffers, CPU tensors out."""

    def __init__(self, ops, dev, fails):
        self.ops, self.dev, self.fails = ops, dev, fails

    def place(self, tensors):
        bufs = [Guarded(t.dtype, t.shape, self.dev) for t in tensors]
        for o, t in zip(bufs, tensors):
            o.view.copy_(t)
        return bufs

    def collect(self, bufs, what):
        for o, name in zip(bufs, NAMES):
            try:
                o.assert_guards(f"{what}: {name}")
            except AssertionError as e:
                self.fails.append(str(e))
        return tuple(o.view.cpu() for o in bufs)

    def adamw_master(self, master, m, v, param, g, state, **hp):
        bufs = self.place((master, m, v, param))
        g_dev = g.to(self.dev)
        self.ops.adamw_master(*(o.view for o in bufs), g_dev, clip_state=device_state(self.dev, state), **hp)
        self.fails.check(torch.equal(g_dev.cpu().view(torch.int32), g.view(torch.int32)), "adamw_master: the gradient was written")
        return self.collect(bufs, f"adamw_master n {master.numel()}")


def test_equals_the_restatement_over_the_grid_and_behind_the_clip_state(ops, dev):
    """Three consecutive steps over suite_adamw's hyperparameter grid at n in {1, 3, 4, 5, 1021, 2125}; coef == 1 is the call without a state,
    coef < 1 the restatement, and a skipped step keeps all four buffers, a param that is not bf16(master) included."""
    fails = Failures()
    M.suite_master(fails, GpuMaster(ops, dev, fails))
    fails.done()


@pytest.mark.parametrize("coef", [None, 0.37], ids=["plain", "clipped"])
def test_equals_the_fp32_adamw_kernels_followed_by_a_cast(ops, dev, coef):
    fails = Failures()
    K = GpuMaster(ops, dev, fails)
    n = 2048 + 77
    master, m, v, param, grads = M.master_inputs(5, n)
    state = None if coef is None else dict(skip=0, coef=np.float32(coef))
    old = [t.to(dev) for t in (master, m, v)]
    new = (master, m, v, param)
    for k, g in enumerate(grads):
        hp = dict(step=k + 1, lr=1e-2, grad_scale=0.37)
        if state is None:
            ops.adamw(*old, g.to(dev), **hp)
        else:
            ops.adamw_clipped(*old, g.to(dev), device_state(dev, state), **hp)
        new = K.adamw_master(*new, g, state, **hp)
        for name, a, b in zip(NAMES, new, [t.cpu() for t in old] + [old[0].cpu().to(BF)]):
            same_bits(fails, a, b, f"step {k + 1} against ovla_adamw{'_clipped' if state else ''}(is_bf16=0) and a cast: {name}")
    fails.done()


def f32_from_bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


EDGE_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,      # ties between two bf16 values: the even neighbour below, the even one above, both signs
             0x3F807FFF, 0x3F808001, 0x00000000, 0x80000000,      # either side of a tie; +0, -0
             0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80008000, 0x00007FFF,      # fp32 subnormals: least, greatest, ties of subnormal bf16, below half
             0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000,      # the largest fp32 that stays finite in bf16; the tie above it, FLT_MAX and -tie: +-inf
             0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC00000]      # +-inf; NaN: quiet, one whose payload sits in the low half only, negative


def test_publication_edge_values_equal_torchs_cast(ops, dev):
    """lr = 0, wd = 0 and zero gradients onto zero moments: the new master is the old one, and param is its cast -- ties both ways, zeros,
    subnormals, overflow to +-inf, infinities, and NaN as NaN (its payload is not part of the contract)."""
    fails = Failures()
    K = GpuMaster(ops, dev, fails)
    edge = f32_from_bits(EDGE_BITS)
    for shift in range(4):      # every value in each of a lane's four slots, and the last three of them in the scalar tail
        master = torch.cat([torch.ones(shift), edge])
        n = master.numel()
        zeros = torch.zeros(n)
        got = K.adamw_master(master, zeros, zeros, M.not_the_cast(master), zeros, None, step=1, lr=0.0, weight_decay=0.0)
        nan = torch.isnan(master)
        want = master.to(BF)
        assert int(nan.sum()) == 3 and bool(torch.isinf(want[~nan]).sum() == 5)
        fails.check(torch.equal(torch.isnan(got[3]), nan) and torch.equal(torch.isnan(got[0]), nan), f"shift {shift}: NaN stays NaN, in master and in param")
        same_bits(fails, got[3][~nan], want[~nan], f"shift {shift}: param against torch's .to(bfloat16)")
        same_bits(fails, got[0][~nan], master[~nan], f"shift {shift}: the master is unchanged by a zero step")
        same_bits(fails, got[1], zeros, f"shift {shift}: exp_avg")
        same_bits(fails, got[2], zeros, f"shift {shift}: exp_avg_sq")
    fails.done()


def test_second_trip_of_the_grid_stride_loop(ops, dev):
    cap = ops.ADAMW_MASTER_MAX_BLOCKS
    header = (ROOT / "include" / "ovla.h").read_text()
    assert int(re.search(r"#define\s+OVLA_ADAMW_MASTER_MAX_BLOCKS\s+(\d+)", header).group(1)) == cap
    n = cap * 256 * 4 + 1029      # one full trip, a second one of 257 groups (two workgroups, the second with one lane), and a tail of one
    g = rng(77)
    master, m, v, grad = adamw_inputs(g, n, F32)
    fails = Failures()
    hp = dict(step=2, lr=5e-4, grad_scale=0.37)
    got = GpuMaster(ops, dev, fails).adamw_master(master, m, v, M.not_the_cast(master), grad, None, **hp)
    for name, a, b in zip(NAMES, got, M.adamw_master(master, m, v, master.to(BF), grad, **hp)):
        same_bits(fails, a, b, f"n {n}: {name}")
    fails.done()


def test_refusals_launch_nothing(ops, dev):
    _lib = load("openvla-oft_amd._lib")
    fails = Failures()
    K = GpuMaster(ops, dev, fails)
    n = 300
    master, m, v, param, grads = M.master_inputs(9, n)
    start = (master, m, v, M.not_the_cast(master))
    bufs = K.place(start)
    g_dev = Guarded(F32, (n,), dev)
    g_dev.view.copy_(grads[0])
    ptr = dict(zip(NAMES + ("grad",), [o.view.data_ptr() for o in bufs] + [g_dev.view.data_ptr()]))

    def call(**over):
        a = _lib.STRUCTS["ovla_adamw_master_args"]()
        fields = dict(ptr, n=n, step=1, lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, grad_scale=1.0, clip_state=None)
        fields.update(over)
        for k, val in fields.items():
            setattr(a, k, val)
        _lib.call("ovla_adamw_master", a, torch.cuda.current_stream().cuda_stream)

    cases = [({k: None}, f"null {k}") for k in ptr]
    cases += [({k: ptr[k] + 8}, f"{k} 8 bytes off a 16-byte boundary") for k in ptr] + [(dict(param=ptr["param"] + 2), "param one element off")]
    cases += [(dict(n=0), "n = 0"), (dict(n=-4), "n < 0"), (dict(step=0), "step = 0"), (dict(step=-1), "step < 0")]
    for over, what in cases:
        with pytest.raises(_lib.OvlaError, match="ovla_adamw_master"):
            call(**over)
    torch.cuda.synchronize()
    for name, o, t in zip(NAMES, bufs, start):
        same_bits(fails, o.view.cpu(), t, f"after {len(cases)} refused calls: {name}")
    K.collect(bufs, "refused calls")
    call()      # the same arguments without the fault are accepted (a null clip_state is legal)
    fails.check(not torch.equal(bufs[0].view.cpu(), master), "the accepted call updates the master")
    fails.done()


def test_second_moment_decays_in_fp32_and_not_in_bf16(ops, dev):
    """One step with g = 1, then 200 steps with g = 0.  fp32 state: exp_avg_sq equals the restatement and strictly decreases every step.  The same
    sequence through ovla_adamw on bf16 state leaves v bit-equal to its value after the first step: the defect this kernel removes."""
    n, lr = 5, 1e-4
    one, zero = torch.ones(n), torch.zeros(n)
    want = (torch.full((n,), 0.5), zero, zero, torch.full((n,), 0.5).to(BF))
    dev_bufs = [t.clone().to(dev) for t in want]
    bf = [t.to(BF).to(dev) for t in want[:3]]
    g1, g0 = one.to(dev), zero.to(dev)
    trace, v_bf_first = [], None
    for k in range(1, 202):
        g_host, g_dev = (one, g1) if k == 1 else (zero, g0)
        want = M.adamw_master(*want, g_host, step=k, lr=lr, weight_decay=0.0)
        ops.adamw_master(*dev_bufs, g_dev, step=k, lr=lr, weight_decay=0.0)
        ops.adamw(*bf, g_dev, step=k, lr=lr, weight_decay=0.0)
        got = [t.cpu() for t in dev_bufs]
        for name, a, b in zip(NAMES, got, want):
            assert torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32)), f"step {k}: {name}"
        trace.append(float(got[2][0]))
        if k == 1:
            v_bf_first = bf[2].cpu().clone()
            assert float(v_bf_first[0]) > 0.0
        else:
            assert torch.equal(bf[2].cpu().view(torch.int16), v_bf_first.view(torch.int16)), f"step {k}: the bf16 second moment moved"
    # 200 multiplications by 0.999 = 0.8186...: the fp32 value must have fallen by that factor (0.83 leaves room for 200 roundings of 2^-24)
    assert all(b < a for a, b in zip(trace, trace[1:])) and trace[0] > 0.0 and trace[-1] < 0.83 * trace[0], (trace[0], trace[-1])


def test_small_updates_reach_the_parameter_through_the_master(ops, dev):
    """p = 1, g = 1, lr = 1e-4, wd = 0: param is 1.0 through step 19 and 0.99609375 at step 20; ovla_adamw's bf16 parameter is still 1.0 at step 40."""
    n = 7
    one = torch.ones(n, device=dev)
    master, m, v, param = one.clone(), torch.zeros_like(one), torch.zeros_like(one), one.to(BF)
    bf = [one.to(BF), torch.zeros(n, dtype=BF, device=dev), torch.zeros(n, dtype=BF, device=dev)]
    pub = []
    for k in range(1, 41):
        ops.adamw_master(master, m, v, param, one, step=k, lr=1e-4, weight_decay=0.0)
        ops.adamw(*bf, one, step=k, lr=1e-4, weight_decay=0.0)
        p = param.float().cpu()
        assert bool((p == p[0]).all())
        pub.append(float(p[0]))
    assert pub[:19] == [1.0] * 19 and pub[19] == 0.99609375, pub[15:22]
    assert pub == M.lost_update_run(40, F32)
    assert bool((bf[0].float().cpu() == 1.0).all()), "the bf16 path is still exactly 1.0 after 40 steps"
    assert abs(float(master[0]) - 0.9960) < 1e-5
