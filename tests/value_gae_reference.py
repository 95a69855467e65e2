"""numpy restatement of the value head's loss, generalised advantage estimation and advantage normalisation (include/ovla.h "Value head and
generalised advantage estimation") as the three kernels of `csrc/value_gae.hip` compute them.  Nothing here needs a GPU.  Every operator written in
the contract is one rounded numpy operation of the type named: np.float32 scalars and arrays for fp32, np.float64 for what the contract calls double.
numpy's + - * / and sqrt are IEEE in both types, fmin / fmax drop a NaN operand as fminf / fmaxf do, so the twins are bit for bit.

    value loss  acc = 0; acc = acc + float(u[b, c]) ascending c;  v = acc / float(chunk)
                e = v - R;  l = e e;  dl = e;   with value_clip > 0:  d = v - old;  vc = old + fmin(fmax(d, -clip), clip);  ec = vc - R;  lc = ec ec;
                lc > l: clipped, l = lc, dl = +0.   loss = 0.5 l.   dl == 0 or not valid: du rows +0; else w = dl grad_scale, du = bf16(w inv_chunk).
                stats over the valid observations, ascending b, in double: n, n clipped, sum loss, sum v, sum R, sum (R - v)^2, sum R^2, +0.
    gae         carry = 0; t = len - 1 .. 0:  nd = done ? 0 : 1;  vnext = t == len - 1 ? bootstrap : value[t + 1];
                delta = (reward + (gamma vnext) nd) - value;  carry = delta + (gamma_lambda nd) carry;  adv = carry;  ret = carry + value;  +0 beyond len.
    normalise   lane i of 256 sums its valid elements e = i, i + 256, ... in double from 0; the lane sums fold by s[i] += s[i + h], h = 128 .. 1.
                count, mean = sum / count, var = sum (x - mean)^2 / count, std = sqrt(var), all double;  adv = (adv - float(mean)) / (float(std) + eps).

`gae_definition64` is NOT a twin: it is the textbook definition A_t = sum_l (gamma lambda)^l delta_{t+l}, cut at `done`, in float64, written
independently of the recursion.  `gae_ref(..., mutant=...)` plants the four classic mistakes for the tests to kill.
"""
import numpy as np

from tests.lora_dropout_reference import f32_to_bf16_bits

F32, F64 = np.float32, np.float64
NORM_LANES = 256
MUTANTS = ("done_keeps_carry", "done_keeps_bootstrap", "vnext_is_value_t", "bootstrap_at_T_minus_1")


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    """fp32 -> the bf16 value (round to nearest even) as fp32."""
    return bf16_bits_to_f32(f32_to_bf16_bits(np.asarray(x, dtype=np.float32)))


def gamma_lambda32(gamma, lam):
    return F32(F64(gamma) * F64(lam))


def value_terms(v, R, old, clip):
    """One observation -> (loss, dl, clipped), fp32 scalars."""
    v, R, clip = F32(v), F32(R), F32(clip)
    with np.errstate(all="ignore"):
        e = F32(v - R)
        l = F32(e * e)
        dl, clipped = e, False
        if clip > 0:
            old = F32(old)
            d = F32(v - old)
            vc = F32(old + np.fmin(np.fmax(d, F32(-clip)), clip))
            ec = F32(vc - R)
            lc = F32(ec * ec)
            if lc > l:
                l, dl, clipped = lc, F32(0.0), True
        return F32(F32(0.5) * l), dl, clipped


def value_loss_ref(u, chunk, returns=None, old_value=None, valid=None, value_clip=0.0, grad_scale=0.0):
    """u: bf16-exact fp32 values (or uint16 bits) of B * chunk elements -> dict(value fp32 [B]) and, with returns, du_bits uint16 [B * chunk],
    stats fp32 [8], loss / dl fp32 [B] and clipped bool [B] (NaN / False where not valid)."""
    u = np.asarray(u)
    u = bf16_bits_to_f32(u) if u.dtype == np.uint16 else u.astype(np.float32)
    u = u.reshape(-1, chunk)
    B = u.shape[0]
    with np.errstate(all="ignore"):
        acc = np.zeros(B, dtype=np.float32)
        for c in range(chunk):
            acc = (acc + u[:, c]).astype(np.float32)
        value = (acc / F32(chunk)).astype(np.float32)
    out = dict(value=value)
    if returns is None:
        return out
    returns = np.asarray(returns, dtype=np.float32)
    inv_chunk = F32(F32(1.0) / F32(chunk))
    gs = F32(grad_scale)
    du = np.zeros((B, chunk), dtype=np.uint16)
    loss, dl, clipped = np.full(B, np.nan, dtype=np.float32), np.full(B, np.nan, dtype=np.float32), np.zeros(B, dtype=bool)
    s = np.zeros(7, dtype=np.float64)
    with np.errstate(all="ignore"):
        for b in range(B):
            if valid is not None and int(valid[b]) == 0:
                continue
            R = returns[b]
            loss[b], dl[b], clipped[b] = value_terms(value[b], R, old_value[b] if value_clip > 0 else 0.0, value_clip)
            if dl[b] != 0:                                   # (true for a NaN: multiplied through)
                w = F32(dl[b] * gs)
                du[b, :] = f32_to_bf16_bits(np.asarray([F32(w * inv_chunk)], dtype=np.float32))[0]
            v64, R64 = F64(value[b]), F64(R)
            r = R64 - v64
            s[0] = s[0] + 1.0
            if clipped[b]:
                s[1] = s[1] + 1.0
            s[2] = s[2] + F64(loss[b])
            s[3] = s[3] + v64
            s[4] = s[4] + R64
            s[5] = s[5] + r * r
            s[6] = s[6] + R64 * R64
        stats = np.zeros(8, dtype=np.float32)
        stats[:7] = s.astype(np.float32)
    out.update(du_bits=du.reshape(-1), stats=stats, loss=loss, dl=dl, clipped=clipped)
    return out


def value_loss64(v, R, old=None, clip=0.0):
    """The loss as a float64 function of the pooled value (for central differences): 0.5 max((v - R)^2, (clip(v) - R)^2)."""
    v, R = F64(v), F64(R)
    l = (v - R) ** 2
    if clip > 0:
        vc = F64(old) + min(max(v - F64(old), -F64(clip)), F64(clip))
        l = max(l, (vc - R) ** 2)
    return 0.5 * l


def gae_ref(reward, value, bootstrap, done, length=None, gamma=0.99, lam=0.95, dtype=np.float32, mutant=None, gamma_lambda=None):
    """The recursion of the contract in `dtype` (fp32: the kernel's twin; float64: the same recursion without fp32 rounding) -> (adv, ret) [N, T].
    `mutant`: one of MUTANTS, a planted mistake."""
    assert mutant is None or mutant in MUTANTS
    D = dtype
    reward, value, bootstrap = np.asarray(reward, dtype=D), np.asarray(value, dtype=D), np.asarray(bootstrap, dtype=D)
    done = np.asarray(done)
    N, T = reward.shape
    g = D(gamma)
    gl = D(gamma_lambda) if gamma_lambda is not None else (D(gamma_lambda32(gamma, lam)) if D is np.float32 else D(gamma) * D(lam))
    adv, ret = np.zeros((N, T), dtype=D), np.zeros((N, T), dtype=D)
    with np.errstate(all="ignore"):
        for n in range(N):
            ln = T if length is None else int(length[n])
            carry = D(0.0)
            for t in range(ln - 1, -1, -1):
                nd = D(0.0) if done[n, t] else D(1.0)
                last = (t == T - 1) if mutant == "bootstrap_at_T_minus_1" else (t == ln - 1)
                if mutant == "vnext_is_value_t":
                    vnext = bootstrap[n] if last else value[n, t]
                else:
                    vnext = bootstrap[n] if last else (value[n, t + 1] if t + 1 < T else D(0.0))
                nd_v = D(1.0) if mutant == "done_keeps_bootstrap" else nd
                nd_c = D(1.0) if mutant == "done_keeps_carry" else nd
                delta = D(D(reward[n, t] + D(D(g * vnext) * nd_v)) - value[n, t])
                carry = D(delta + D(D(gl * nd_c) * carry))
                adv[n, t] = carry
                ret[n, t] = D(carry + value[n, t])
    return adv, ret


def gae_definition64(reward, value, bootstrap, done, length=None, gamma=0.99, lam=0.95, gamma_lambda=None):
    """A_t = sum_{l >= 0} (gamma lambda)^l delta_{t + l} over the steps of t's own episode (the sum stops after the first done at or after t,
    and at the trajectory's length), delta_s = r_s + gamma V_{s+1} [not done_s] - V_s with V_len = bootstrap; ret = A + V.  float64, no recursion."""
    reward, value, bootstrap = np.asarray(reward, dtype=F64), np.asarray(value, dtype=F64), np.asarray(bootstrap, dtype=F64)
    done = np.asarray(done)
    N, T = reward.shape
    g = F64(gamma)
    gl = F64(gamma_lambda) if gamma_lambda is not None else F64(gamma) * F64(lam)
    adv, ret = np.zeros((N, T)), np.zeros((N, T))
    for n in range(N):
        ln = T if length is None else int(length[n])
        delta = np.zeros(ln)
        for s in range(ln):
            vnext = bootstrap[n] if s == ln - 1 else value[n, s + 1]
            delta[s] = reward[n, s] + (0.0 if done[n, s] else g * vnext) - value[n, s]
        for t in range(ln):
            a, w = 0.0, 1.0
            for s in range(t, ln):
                a += w * delta[s]
                if done[n, s]:
                    break
                w *= gl
            adv[n, t] = a
            ret[n, t] = a + value[n, t]
    return adv, ret


def gae_bound(reward, value, bootstrap, done, length=None, gamma=0.99, lam=0.95):
    """Elementwise bound on |fp32 recursion - float64 definition| for adv (ret: add 2^-24 |ret| + the same), derived from the operation count.
    With u = 2^-24 per rounded fp32 operation:  delta takes 4 operations on terms of magnitude at most m_t = |r| + gamma |vnext| + |v|, so
    |delta_hat - delta| <= 4 u m_t (1 + 4 u);  a step of the carry takes 3 more (gl nd is exact: nd is 0 or 1), so with M_t the same recursion on
    magnitudes, M_t = m_t + gl nd M_{t+1} >= |carry_t|, the error obeys  E_t <= 4 u m_t + gl nd E_{t+1} + 3 u M_t  up to second order; 1.01 covers
    the second-order terms for T <= 2^10, and the rounding of gamma and gamma_lambda to fp32 (relative u each, acting on every term of M) adds
    (len - t + 1) u M_t."""
    u = 2.0 ** -24
    reward, value, bootstrap = np.abs(np.asarray(reward, dtype=F64)), np.abs(np.asarray(value, dtype=F64)), np.abs(np.asarray(bootstrap, dtype=F64))
    N, T = reward.shape
    g, gl = F64(gamma), F64(gamma) * F64(lam)
    E = np.zeros((N, T))
    for n in range(N):
        ln = T if length is None else int(length[n])
        e, M = 0.0, 0.0
        for t in range(ln - 1, -1, -1):
            nd = 0.0 if done[n, t] else 1.0
            vnext = bootstrap[n] if t == ln - 1 else value[n, t + 1]
            m = reward[n, t] + g * vnext + value[n, t]
            M = m + gl * nd * M
            e = 4 * u * m + gl * nd * e + 3 * u * M
            E[n, t] = 1.01 * (e + (ln - t + 1) * u * M)
    return E


def _valid_mask(N, T, length):
    if length is None:
        return np.ones((N, T), dtype=bool)
    return np.arange(T)[None, :] < np.asarray(length).reshape(N, 1)


def _fixed_order_sum(x64, mask):
    """The contract's summation order over the valid elements of a flat float64 array."""
    n = x64.size
    pad = (-n) % NORM_LANES
    x = np.concatenate([np.where(mask, x64, 0.0), np.zeros(pad)]).reshape(-1, NORM_LANES)     # row j holds elements j * 256 + lane
    m = np.concatenate([mask, np.zeros(pad, dtype=bool)]).reshape(-1, NORM_LANES)
    s = np.zeros(NORM_LANES, dtype=np.float64)
    for j in range(x.shape[0]):
        s = np.where(m[j], s + x[j], s)          # an element that is not valid is not added (adding +0 would turn a -0 sum into +0)
    h = NORM_LANES // 2
    while h > 0:
        s[:h] = s[:h] + s[h:2 * h]
        h //= 2
    return F64(s[0])


def normalize_ref(adv, length=None, eps=1e-8):
    """-> the normalised copy of adv fp32 [N, T]; elements that are not valid keep their bits."""
    adv = np.asarray(adv, dtype=np.float32)
    N, T = adv.shape
    mask = _valid_mask(N, T, length).reshape(-1)
    flat = adv.reshape(-1)
    out = flat.copy()
    with np.errstate(all="ignore"):
        x64 = flat.astype(np.float64)
        count = _fixed_order_sum(np.ones_like(x64), mask)
        if count == 0:
            return out.reshape(N, T)
        mean = _fixed_order_sum(x64, mask) / count
        d = x64 - mean
        var = _fixed_order_sum(d * d, mask) / count
        denom = F32(F32(np.sqrt(var)) + F32(eps))
        out[mask] = ((flat[mask] - F32(mean)).astype(np.float32) / denom).astype(np.float32)
    return out.reshape(N, T)
