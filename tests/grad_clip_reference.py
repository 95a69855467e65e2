"""The gradient-clipping contract (include/ovla.h "Gradient-norm clipping") restated in numpy: the fixed-order double sum of squares of
ovla_grad_sumsq, the state update of ovla_grad_clip_coef, and ovla_adamw_clipped as the clipped gradient handed to the AdamW emulation of
tests/pointwise_reference.py.  Independent of the package: the tests compare the kernels and the engine against this file bit for bit.

    r_i = fp32(g_i * grad_scale), rounded to bf16 for a bf16 parameter buffer;  q_i = double(r_i)^2 (exact)
    chunk c = elements [c C, (c + 1) C): element c C + o belongs to lane (o / 4) % L and is added in ascending o; the L lane sums go through
    THE TREE (per 64 lanes: h = 32 .. 1: s[t] += s[t + h]; then (w0 + w1) + (w2 + w3)); the partials are summed by lane j % L in ascending j
    and go through THE TREE again.

Padding with +0.0 restates "the element is not there": every running sum here is +0.0, positive or NaN, and x + 0.0 has the bits of x.
"""
import numpy as np

CHUNK, LANES = 8192, 256            # OVLA_GRAD_SUMSQ_CHUNK, OVLA_GRAD_SUMSQ_LANES
TRIPS = CHUNK // (4 * LANES)
EPS_TERM = np.float32(1e-6)         # clip_grad_norm_'s max_norm / (norm + 1e-6)


def widen_bf16(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even) as fp32; infinities stay, NaN stays NaN."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = widen_bf16(((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16))
    return np.where(np.isnan(x), np.float32(np.nan), r).astype(np.float32)


def seen_gradient(g, grad_scale, is_bf16):
    """The gradient as ovla_adamw forms it: one fp32 multiply, then the bf16 rounding of a bf16 buffer."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (np.asarray(g, dtype=np.float32) * np.float32(grad_scale)).astype(np.float32)
    return bf16_round(r) if is_bf16 else r


def tree(s):
    """THE TREE over the last axis (LANES doubles) -> one double per leading index."""
    w = np.asarray(s, dtype=np.float64).reshape(s.shape[:-1] + (LANES // 64, 64))
    for h in (32, 16, 8, 4, 2, 1):
        w = w[..., :h] + w[..., h:2 * h]
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def chunk_partials(q):
    """q float64 [n] -> the ceil(n / CHUNK) partials of the first launch."""
    n = q.shape[0]
    n_partials = (n + CHUNK - 1) // CHUNK
    padded = np.zeros(n_partials * CHUNK, np.float64)
    padded[:n] = q
    padded = padded.reshape(n_partials, TRIPS, LANES, 4)
    acc = np.zeros((n_partials, LANES), np.float64)
    for k in range(TRIPS):
        for j in range(4):
            acc = acc + padded[:, k, :, j]
    return tree(acc)


def final_sum(partials):
    """The second launch: lane t adds partials[t], partials[t + L], ... in ascending index, then THE TREE."""
    p = np.asarray(partials, dtype=np.float64)
    rounds = (p.shape[0] + LANES - 1) // LANES
    padded = np.zeros(rounds * LANES, np.float64)
    padded[:p.shape[0]] = p
    acc = np.zeros(LANES, np.float64)
    for row in padded.reshape(rounds, LANES):
        acc = acc + row
    return np.float64(tree(acc))


def grad_sumsq(g, grad_scale=1.0, is_bf16=False):
    """ovla_grad_sumsq: one double."""
    r = seen_gradient(g, grad_scale, is_bf16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return final_sum(chunk_partials(r * r))


def new_state():
    return dict(coef=np.float32(0.0), norm=np.float32(0.0), skip=0, steps=0, clipped=0, skipped=0)


def clip_coef(slots, max_norm, state, skip_nonfinite=True):
    """ovla_grad_clip_coef: returns the new state."""
    total = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in slots:
            total = total + np.float64(s)
        norm = np.float32(np.sqrt(total))
        st = dict(state, steps=state["steps"] + 1, norm=norm)
        if skip_nonfinite and not np.isfinite(total):
            st.update(skip=1, coef=np.float32(1.0), skipped=state["skipped"] + 1)
            return st
        coef = np.fmin(np.float32(1.0), np.float32(max_norm) / np.float32(norm + EPS_TERM)).astype(np.float32)
    st.update(skip=0, coef=coef, clipped=state["clipped"] + int(coef < np.float32(1.0)))
    return st


def clipped_gradient(g, grad_scale, coef, is_bf16):
    """The gradient entering ovla_adamw_clipped's element update: what grad.mul_(coef) leaves in a .grad of the parameter's dtype."""
    r = seen_gradient(g, grad_scale, is_bf16)
    with np.errstate(invalid="ignore", over="ignore"):
        c = (r * np.float32(coef)).astype(np.float32)
    return bf16_round(c) if is_bf16 else c


def adamw_clipped(p, m, v, g, state, *, grad_scale=1.0, **hp):
    """ovla_adamw_clipped on CPU torch tensors (p's dtype decides bf16 / fp32; g fp32): new (p, m, v).  A skipped step returns the inputs."""
    import torch

    from tests.pointwise_reference import adamw_emulate

    if state["skip"]:
        return p, m, v
    grad = clipped_gradient(g.numpy(), grad_scale, state["coef"], p.dtype == torch.bfloat16)
    return adamw_emulate(p, m, v, torch.from_numpy(grad), grad_scale=1.0, **hp)
