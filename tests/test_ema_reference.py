"""Weight EMA on the CPU: the driver's decay schedule against the restatement of tests/ema_reference.py and its known answers, the new
entry point's refusals (no device needed: it refuses before any launch), and the driver's argument check.  No GPU."""
import ctypes
import importlib
import itertools

import numpy as np
import pytest

import ema_reference as R

load = importlib.import_module


@pytest.fixture(scope="module")
def ft():
    return load("openvla-oft_amd.vla_scripts.finetune")


def test_schedule_equals_the_restatement_on_a_grid(ft):
    ks = (1, 2, 3, 4, 5, 10, 100, 1000, 10 ** 6)
    for k, max_decay, power, inv_gamma, after in itertools.product(ks, (0.0, 0.5, 0.99, 0.9999), (0.75, 2 / 3, 1.0, None), (1.0, 10.0), (0, 3, 100)):
        kw = dict(max_decay=max_decay, power=power, inv_gamma=inv_gamma, update_after=after)
        got, want = ft.ema_decay_at(k, **kw), R.ema_decay_at(k, **kw)
        assert isinstance(got, float) and got == want, (k, kw, got, want)
        assert 0.0 <= got <= max_decay
    assert ft.ema_decay_at(7, max_decay=0.9999) == R.ema_decay_at(7, max_decay=0.9999, power=0.75, inv_gamma=1.0, update_after=0)   # the defaults


def test_schedule_known_answers(ft):
    assert ft.ema_decay_at(1, max_decay=0.9999) == 0.0
    assert ft.ema_decay_at(2, max_decay=0.9999, power=0.75, inv_gamma=1.0) == 1 - 2 ** -0.75
    assert ft.ema_decay_at(10 ** 9, max_decay=0.9999) == 0.9999
    for after in (0, 3):
        for k in range(1, 12):
            want = 0.0 if k <= after + 1 else 0.97
            assert ft.ema_decay_at(k, max_decay=0.97, power=None, update_after=after) == want
    assert [ft.ema_decay_at(k, max_decay=0.9999, update_after=3) for k in (1, 2, 3, 4)] == [0.0] * 4
    assert ft.ema_decay_at(5, max_decay=0.9999, update_after=3) == 1 - 2 ** -0.75
    ds = [ft.ema_decay_at(k, max_decay=0.9999) for k in range(1, 200)]
    assert all(a <= b for a, b in zip(ds, ds[1:])), "the warm-up never decreases"


def test_restatement_is_three_separately_rounded_operations():
    """Known answers of the update itself, chosen so that a fused multiply-add or another association gives other bits."""
    s, p, w = np.float32(1.0), np.float32(1.0 - 2.0 ** -24), np.float32(2.0 ** -0.75)
    d = np.float32(s - p)
    assert R.ema_update([s], [p], w)[0] == np.float32(s - np.float32(w * d))
    assert R.ema_update([3.5], [-1.25], 1.0)[0] == np.float32(-1.25) and R.ema_update([3.5], [-1.25], 0.0)[0] == np.float32(3.5)
    # the product is rounded before the second subtraction: on random data a fused multiply-add (one rounding of s - w * d) gives other bits
    g = np.random.default_rng(0)
    s, p = g.standard_normal(4096).astype(np.float32), g.standard_normal(4096).astype(np.float32)
    d = (s - p).astype(np.float32)
    got = R.ema_update(s, p, w)
    assert np.array_equal(got, (s - (w * d).astype(np.float32)).astype(np.float32))
    fused = (s.astype(np.float64) - np.float64(w) * d.astype(np.float64)).astype(np.float32)
    assert 0 < int((got != fused).sum()) < 4096
    assert np.array_equal(R.widen_bf16([0x3F80, 0xC000, 0x0000, 0x8000]), np.array([1.0, -2.0, 0.0, -0.0], np.float32))
    assert list(R.bf16_rne_bits(np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -2.0], np.float32))) == [0x3F80, 0x3F80, 0x3F82, 0xC000]
    assert R.one_minus_decay(0.9999) == np.float32(1.0 - 0.9999) and R.one_minus_decay(0.0) == np.float32(1.0)


def test_entry_point_is_exported_and_refuses_before_any_launch():
    _lib = load("openvla-oft_amd._lib")
    lib = _lib.lib()
    assert "ovla_ema_update" in _lib.FUNCTIONS and [f for f, _ in _lib.STRUCT_FIELDS["ovla_ema_update_args"]] == ["param", "shadow", "n", "is_bf16", "one_minus_decay"]
    args = _lib.STRUCTS["ovla_ema_update_args"]()
    assert lib.ovla_ema_update(ctypes.byref(args), None) == -1
    assert b"ovla_ema_update" in lib.ovla_last_error()
    # every refusal comes before the pointers are used: host addresses stand in for device buffers
    buf = (ctypes.c_float * 16)()
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    for n, omd, off in ((-1, 0.5, 0), (4, 1.5, 0), (4, -0.1, 0), (4, float("nan"), 0), (4, 0.5, 4)):
        args.param, args.shadow, args.n, args.is_bf16, args.one_minus_decay = base + off, base, n, 0, omd
        assert lib.ovla_ema_update(ctypes.byref(args), None) == -1, (n, omd, off)
        assert b"ovla_ema_update" in lib.ovla_last_error()
    args.param, args.shadow, args.n, args.one_minus_decay = base, base, 0, 0.5
    assert lib.ovla_ema_update(ctypes.byref(args), None) == 0, "n == 0 is legal and launches nothing"


@pytest.mark.parametrize("bad", [1.0, -0.1])
def test_finetune_refuses_a_decay_outside_the_half_open_interval(ft, bad, monkeypatch):
    import torch

    def touched(*a, **kw):
        raise AssertionError("the device was touched before the argument check")

    monkeypatch.setattr(torch.cuda, "set_device", touched)
    with pytest.raises(ValueError, match="ema_decay"):
        ft.finetune(ft.FinetuneConfig(), ema_decay=bad)
