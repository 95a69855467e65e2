"""The weight-EMA contract (include/ovla.h "Weight EMA") restated in numpy, and the decay schedule of vla_scripts/finetune.py `ema_decay_at`
restated in Python floats.  Independent of the package: the tests compare the kernel and the driver against this file bit for bit.

    shadow[i] = s - omd * (s - float(param[i]))     three np.float32 operations, each rounded on its own; a bf16 parameter widened exactly
"""
import numpy as np


def widen_bf16(bits):
    """bf16 bit patterns (uint16) -> the fp32 numbers they are, exactly."""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_rne_bits(x):
    """fp32 -> bf16 bit patterns, round to nearest even (finite values and infinities; the tests give it no NaN)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def ema_update(shadow, param, omd):
    """One update.  `shadow` fp32, `param` fp32 (a bf16 parameter comes through widen_bf16), `omd` = one_minus_decay.  Returns the new shadow."""
    s, p, w = np.asarray(shadow, dtype=np.float32), np.asarray(param, dtype=np.float32), np.float32(omd)
    assert s.dtype == np.float32 and p.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        d = (s - p).astype(np.float32)
        u = (w * d).astype(np.float32)
        return (s - u).astype(np.float32)


def one_minus_decay(decay):
    """What ParamStore.ema_update hands the kernel: 1 - decay in double, rounded to fp32 once."""
    return np.float32(1.0 - float(decay))


def ema_decay_at(k, *, max_decay, power=0.75, inv_gamma=1.0, update_after=0):
    """The decay of the k-th update (k from 1): diffusers' EMAModel warm-up, in Python floats."""
    step = k - update_after - 1
    if step <= 0:
        return 0.0
    if power is None:
        return max_decay
    return min(max_decay, 1 - (1 + step / inv_gamma) ** -power)


def u32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def same_f32(got, want):
    """Bit equality of two fp32 arrays, a NaN matching any NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(np.isnan(got), nan)) and bool(np.array_equal(u32(got)[~nan], u32(want)[~nan]))
