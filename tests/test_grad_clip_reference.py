"""Gradient clipping on the CPU: the numpy restatement (tests/grad_clip_reference.py) against closed forms on exact data, its coefficient and
clipped fp32 AdamW update against torch's clip_grad_norm_ + torch.optim.AdamW, the entry points' refusals (they refuse before any launch), and
the driver's argument check.  No GPU."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import grad_clip_reference as R

load = importlib.import_module
EPS32 = 2.0 ** -23


def exact_values(g, n):
    """k * 2^e with |k| <= 7 and e in [-3, 3]: exact in bf16; every square is k^2 4^e, an integer multiple of 2^-6 below 2^12, so any sum of
    up to 2^30 of them is exact in double -- every summation order gives the same bits."""
    k = g.integers(-7, 8, n)
    e = g.integers(-3, 4, n)
    units = int(np.sum(k.astype(np.int64) ** 2 * 4 ** (e.astype(np.int64) + 3)))   # the sum of squares in units of 2^-6, in integers (< 2^42)
    return (k * 2.0 ** e).astype(np.float32), units


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("n", [0, 1, 5, 255, 1027, R.CHUNK - 1, R.CHUNK, 3 * R.CHUNK + 5, 300 * R.CHUNK + 77])
def test_twin_on_exact_data_equals_the_closed_form_bit_for_bit(n, bf16):
    g = np.random.default_rng(n + 1)
    v, units = exact_values(g, n)
    for scale, shift in ((1.0, 0), (0.5, 2), (4.0, -4)):          # powers of two: the product is exact and the sum scales by scale^2 = 2^-shift
        want = math.ldexp(units, -6 - shift)                        # exact: units < 2^53
        got = R.grad_sumsq(v, scale, bf16)
        assert isinstance(got, np.float64) and got.tobytes() == np.float64(want).tobytes(), (n, bf16, scale, got, want)
    assert R.grad_sumsq(g.permutation(v), 1.0, bf16).tobytes() == np.float64(math.ldexp(units, -6)).tobytes(), "exact data: the order cannot matter"


def test_twin_order_is_the_documented_one():
    """Inexact data, where the order does matter: the vectorised restatement equals a literal element-by-element walk of the contract."""
    g = np.random.default_rng(5)
    n = R.CHUNK + 4 * R.LANES + 6
    v = (g.standard_normal(n) * 10.0 ** g.uniform(-3, 3, n)).astype(np.float32)
    q = v.astype(np.float64) ** 2

    def tree(s):
        waves = []
        for w in range(4):
            a = list(s[64 * w: 64 * w + 64])
            for h in (32, 16, 8, 4, 2, 1):
                for t in range(h):
                    a[t] = a[t] + a[t + h]
            waves.append(a[0])
        return (waves[0] + waves[1]) + (waves[2] + waves[3])

    partials = []
    for c0 in range(0, n, R.CHUNK):
        lanes = [np.float64(0.0)] * R.LANES
        for o in range(min(R.CHUNK, n - c0)):
            lanes[(o // 4) % R.LANES] = lanes[(o // 4) % R.LANES] + q[c0 + o]
        partials.append(tree(lanes))
    lanes = [np.float64(0.0)] * R.LANES
    for j, p in enumerate(partials):
        lanes[j % R.LANES] = lanes[j % R.LANES] + p
    assert R.grad_sumsq(v).tobytes() == np.float64(tree(lanes)).tobytes()


def test_twin_coefficient_cases_and_counters():
    st = R.new_state()
    st = R.clip_coef([9.0, 16.0], 10.0, st)                       # norm 5 below the threshold
    assert (st["norm"], st["coef"], st["skip"], st["steps"], st["clipped"], st["skipped"]) == (5.0, 1.0, 0, 1, 0, 0)
    st = R.clip_coef([9.0, 16.0], 2.5, st)                        # above: 2.5 / (5 + 1e-6) in fp32
    assert st["coef"] == np.float32(2.5) / np.float32(np.float32(5.0) + np.float32(1e-6)) and st["coef"] < 1 and st["clipped"] == 1
    st = R.clip_coef([0.0, 0.0], 1.0, st)                         # all-zero gradient: 1 / 1e-6 clamps to 1
    assert (st["norm"], st["coef"], st["skip"], st["clipped"]) == (0.0, 1.0, 0, 1)
    st = R.clip_coef([1e30, 1e30], math.inf, st)                  # guard only
    assert st["coef"] == 1.0 and st["skip"] == 0 and st["clipped"] == 1
    for bad in (math.nan, math.inf):
        before = st["skipped"]
        st = R.clip_coef([1.0, bad], 1.0, st)
        assert st["skip"] == 1 and st["coef"] == 1.0 and st["skipped"] == before + 1 and not np.isfinite(st["norm"])
    assert st["steps"] == 6 and st["clipped"] == 1 and st["skipped"] == 2
    off = R.clip_coef([math.nan], 1.0, R.new_state(), skip_nonfinite=False)
    assert off["skip"] == 0 and off["coef"] == 1.0 and off["skipped"] == 0


def test_twin_against_torch_clip_grad_norm_and_adamw():
    """One fp32 tensor of 3000 elements, one clipped AdamW step: the restatement against torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.

    The restatement's norm is the double sum rounded once (relative error <= eps / 2, eps = 2^-23).  torch sums the squares in fp32: with
    u = eps / 2 per operation, a chain of d additions of positive terms is off by at most d u relatively, and the square root halves it.  Its
    vectorised reduction keeps at least 8 lanes x 4 accumulators, so d <= 3000 / 32 + 8 (the combining tree) = 102 and the norm is within
    51 u = 25.5 eps, plus eps / 2 each for the squares' own rounding and the final root: the bound on the relative norm difference is 32 eps.
    The coefficient adds one fp32 add and one divide on either side (2 eps).  MEASURED here: norm 1.41e-7 (1.19 eps), coefficient 1.36e-7 (1.14 eps).

    The update: at step 1 AdamW moves a parameter by lr m^ / (sqrt(v^) + 1e-8) with |.| <= lr; a relative change delta of the gradient moves
    numerator and denominator by delta each, so the step by at most 2 delta lr; the ten-odd fp32 operations of either pipeline (torch's fp32 sqrt
    is a 1-ulp routine) add at most 16 eps lr, and the final parameter rounding eps |p| / 2 on each side.  MEASURED: 1.19e-7 (one ulp of a parameter near 1) against a bound of 4.40e-7.
    """
    n, lr, max_norm = 3000, 1e-3, 0.75
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen)
    grad = torch.randn(n, generator=gen) * torch.pow(10.0, torch.randint(-3, 1, (n,), generator=gen).float())
    p = torch.nn.Parameter(p0.clone())
    p.grad = grad.clone()
    torch_norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
    torch_coef_grad = p.grad.clone()
    torch.optim.AdamW([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01).step()

    st = R.clip_coef([R.grad_sumsq(grad.numpy())], max_norm, R.new_state())
    assert st["skip"] == 0 and st["coef"] < 1.0
    norm_diff = abs(float(st["norm"]) - torch_norm) / torch_norm
    k = int(torch.argmax(grad.abs()))
    torch_coef = float(torch_coef_grad[k]) / float(grad[k])         # torch's coefficient, from the largest element (one more rounding: eps / 2)
    coef_diff = abs(float(st["coef"]) - torch_coef) / torch_coef
    zeros = torch.zeros(n)
    got, _, _ = R.adamw_clipped(p0.clone(), zeros.clone(), zeros.clone(), grad, st, step=1, lr=lr)
    p_diff = float((got.double() - p.detach().double()).abs().max())
    p_bound = lr * (2 * 34.5 + 16) * EPS32 + EPS32 * float(p0.abs().max())
    print(f"norm {norm_diff:.3e} ({norm_diff / EPS32:.2f} eps), coefficient {coef_diff:.3e} ({coef_diff / EPS32:.2f} eps), parameters {p_diff:.3e} (bound {p_bound:.3e})")
    assert norm_diff <= 32 * EPS32
    assert coef_diff <= 34.5 * EPS32
    assert p_diff <= p_bound
    assert float((got.double() - p0.double()).abs().max()) > 100 * p_bound, "the step itself is far larger than the bound"


def test_entry_points_refuse_bad_arguments_before_any_launch():
    _lib = load("openvla-oft_amd._lib")
    lib = _lib.lib()
    ok = 0x10000   # an aligned non-null address: nothing is dereferenced before the refusal

    def sumsq(**kw):
        a = _lib.STRUCTS["ovla_grad_sumsq_args"]()
        a.grad, a.n, a.is_bf16, a.grad_scale, a.slots, a.slot, a.workspace, a.workspace_bytes = ok, R.CHUNK + 1, 0, 1.0, ok, 0, ok, 16
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ovla_grad_sumsq(ctypes.byref(a), None), lib.ovla_last_error().decode()

    for what, kw in {"null grad": dict(grad=None), "null slots": dict(slots=None), "null workspace": dict(workspace=None), "n -1": dict(n=-1),
                     "slot -1": dict(slot=-1), "misaligned grad": dict(grad=ok + 4), "misaligned slots": dict(slots=ok + 4),
                     "misaligned workspace": dict(workspace=ok + 4), "workspace too small": dict(workspace_bytes=8)}.items():
        rc, msg = sumsq(**kw)
        assert rc == -1 and "ovla_grad_sumsq" in msg, (what, rc, msg)

    def coef(**kw):
        a = _lib.STRUCTS["ovla_grad_clip_coef_args"]()
        a.slots, a.n_slots, a.max_norm, a.skip_nonfinite, a.state = ok, 2, 1.0, 1, ok
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ovla_grad_clip_coef(ctypes.byref(a), None), lib.ovla_last_error().decode()

    for what, kw in {"null slots": dict(slots=None), "null state": dict(state=None), "no slots": dict(n_slots=0), "max_norm 0": dict(max_norm=0.0),
                     "max_norm -1": dict(max_norm=-1.0), "max_norm NaN": dict(max_norm=math.nan)}.items():
        rc, msg = coef(**kw)
        assert rc == -1 and "ovla_grad_clip_coef" in msg, (what, rc, msg)

    a = _lib.STRUCTS["ovla_adamw_clipped_args"]()
    a.param, a.exp_avg, a.exp_avg_sq, a.grad, a.n, a.step, a.lr, a.clip_state = ok, ok, ok, ok, 8, 1, 1e-3, None
    assert lib.ovla_adamw_clipped(ctypes.byref(a), None) == -1 and "ovla_adamw_clipped" in lib.ovla_last_error().decode()
    # the clipped AdamW's arguments are ovla_adamw's, field for field, plus the state
    plain, clipped = _lib.STRUCT_FIELDS["ovla_adamw_args"], _lib.STRUCT_FIELDS["ovla_adamw_clipped_args"]
    assert clipped[:len(plain)] == plain and [f for f, _ in clipped[len(plain):]] == ["clip_state"]
    assert ctypes.sizeof(_lib.STRUCTS["ovla_grad_clip_state"]) == 24
    text = _lib.HEADER_PATH.read_text()
    assert f"#define OVLA_GRAD_SUMSQ_CHUNK {R.CHUNK}\n" in text and f"#define OVLA_GRAD_SUMSQ_LANES {R.LANES}\n" in text
    assert load("openvla-oft_amd.ops").GRAD_SUMSQ_CHUNK == R.CHUNK


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan])
def test_finetune_refuses_a_bad_max_grad_norm(bad, monkeypatch):
    ft = load("openvla-oft_amd.vla_scripts.finetune")

    def touched(*a, **kw):
        raise AssertionError("the device was touched before the argument check")

    monkeypatch.setattr(torch.cuda, "set_device", touched)
    with pytest.raises(ValueError, match="max_grad_norm"):
        ft.finetune(ft.FinetuneConfig(), max_grad_norm=bad)
