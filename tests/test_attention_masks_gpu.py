"""Attention kernels: the exact key set of every row, isolation from padding / bucket length / neighbouring heads / the
memory around the views, and per-element error bounds against a float64 reference (`tests/attn_reference.py`, whose checks
are shown to have teeth on the CPU by `tests/test_attention_reference.py`).

Everything goes through `ops.attn_fwd` / `ops.attn_bwd`; the backward consumes the kernel's own O and lse.  Bit-equality
between two runs is compared on the raw 16-bit patterns' values (`torch.equal`).
"""
import pytest
import torch

from tests import attn_reference as ar

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CASES = ar.CASES
KV_CASES = [c for c in CASES if c[4] is not None]
SENTINEL = 0x5A5A      # a finite bf16 pattern that no kernel writes by accident into every guard element
POISON = 9984.0        # 39 * 2^8: bf16-exact, finite, and large enough that exp2 of a poisoned score overflows fp32


def rnd(*shape, dev, scale=1.0, dtype=BF):   # the generator of tests/test_kernels_gpu.py
    return (torch.randn(*shape, device=dev, dtype=torch.float32) * scale).to(dtype)


def rows(t, dev):
    """[B, H, S, hd] (CPU) -> bf16 [B*S, H*hd] on the device."""
    B, H, S, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * hd).to(BF).to(dev).contiguous()


def heads(t, B, S, H, hd):
    """[B*S, H*hd] (device) -> float64 [B, H, S, hd] on the CPU."""
    return t.detach().cpu().double().reshape(B, S, H, hd).permute(0, 2, 1, 3).contiguous()


def kv_tensor(kvl, dev):
    return None if kvl is None else torch.tensor(kvl, dtype=torch.int32, device=dev)


def run(ops, q, k, v, do, B, S, H, hd, kv_len, causal, **outs):
    o, lse = ops.attn_fwd(q, k, v, B, S, H, hd, kv_len=kv_len, causal=causal, out=outs.get("out"))
    dq, dk, dv = ops.attn_bwd(q, k, v, o, do, lse, B, S, H, hd, kv_len=kv_len, causal=causal,
                              dq=outs.get("dq"), dk=outs.get("dk"), dv=outs.get("dv"))
    return o, lse, dq, dk, dv


_BASE = {}


def base(ops, dev, case):
    """Random inputs in the fused [B*S, 3*H*hd] layout and the kernels' outputs for them, computed once per case and
    shared (read-only) by the tests that compare another run against it."""
    key = ar.case_id(case)
    if key not in _BASE:
        B, H, S, hd, kvl, causal = case
        torch.manual_seed(B * 100 + S + hd)
        qkv = rnd(B * S, 3 * H * hd, dev=dev)
        q, k, v = qkv[:, : H * hd], qkv[:, H * hd: 2 * H * hd], qkv[:, 2 * H * hd:]
        do = rnd(B * S, H * hd, dev=dev)
        kv_len = kv_tensor(kvl, dev)
        _BASE[key] = dict(q=q, k=k, v=v, do=do, kv_len=kv_len, outs=run(ops, q, k, v, do, B, S, H, hd, kv_len, causal))
    return _BASE[key]


def assert_same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    if not torch.equal(a, b):
        diff = (a != b).nonzero()
        raise AssertionError(f"{what}: {len(diff)} of {a.numel()} elements differ, first at {tuple(diff[0].tolist())}: "
                             f"{a[tuple(diff[0])].item()} vs {b[tuple(diff[0])].item()}")


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_counting(ops, dev, case):
    """Uniform P over the visible keys and one-hot V / dO: lse, O and dV count the keys each row sees, exactly."""
    B, H, S, hd, kvl, causal = case
    q, k, v, do = (rows(t, dev) for t in ar.counting_inputs(B, H, S, hd))
    o, lse, dq, dk, dv = run(ops, q, k, v, do, B, S, H, hd, kv_tensor(kvl, dev), causal)
    ar.check_counting(heads(o, B, S, H, hd), lse.cpu(), heads(dk, B, S, H, hd), heads(dv, B, S, H, hd), kvl, causal)


def elementwise(ops, dev, q, k, v, do, B, S, H, hd, kvl, causal, label):
    scale = hd ** -0.5
    o, lse, dq, dk, dv = run(ops, q, k, v, do, B, S, H, hd, kv_tensor(kvl, dev), causal)
    hq, hk, hv, hdo = (heads(t, B, S, H, hd) for t in (q, k, v, do))
    rO, rlse, rdQ, rdK, rdV, P = ar.reference(hq, hk, hv, hdo, kvl, causal, scale)
    bO, bdQ, bdK, bdV = ar.bounds(hq, hk, hv, hdo, rO, P, scale)
    worst, failures = {}, []
    for name, check in (("lse", lambda: ar.check_lse(lse.cpu(), rlse, hq, hk, kvl, causal, scale)),
                        ("O", lambda: ar.check_elementwise(heads(o, B, S, H, hd), rO, bO, what="O")),
                        ("dQ", lambda: ar.check_elementwise(heads(dq, B, S, H, hd), rdQ, bdQ, what="dQ")),
                        ("dK", lambda: ar.check_elementwise(heads(dk, B, S, H, hd), rdK, bdK, what="dK")),
                        ("dV", lambda: ar.check_elementwise(heads(dv, B, S, H, hd), rdV, bdV, what="dV"))):
        try:
            worst[name] = f"{check():.2f}"
        except AssertionError as e:   # collect, so that the printed line names every tensor before the test fails
            worst[name] = "FAIL"
            failures.append(str(e))
    print(f"\n{label}: worst |err| / (2^-8 bound): " + " ".join(f"{n} {x}" for n, x in worst.items() if n != "lse")
          + f"; lse / its bound: {worst['lse']}")
    assert not failures, "; ".join(failures)


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_elementwise_bounds(ops, dev, case):
    """|out - ref| <= 3 * 2^-8 * bound per element (exactly 0 where the bound is 0), lse to fp32 accuracy."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case)
    elementwise(ops, dev, b["q"], b["k"], b["v"], b["do"], B, S, H, hd, kvl, causal, ar.case_id(case))


def test_elementwise_bounds_spiked_scores(ops, dev):
    """The same bounds across large running-max jumps between key tiles (the keys of test_attention_spiked_scores)."""
    torch.manual_seed(0)
    B, H, S, hd = 1, 1, 257, 128
    q, k, v, do = (rnd(S, hd, dev=dev) for _ in range(4))
    k[200] = q[5] * 4.0
    k[70] = q[9] * 3.0
    elementwise(ops, dev, q, k, v, do, B, S, H, hd, None, False, "spiked S257")


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KV_CASES, ids=ar.case_id)
def test_padding_is_isolated(ops, dev, case):
    """What the K / V rows >= kv_len[b] hold (zeros or +-9984) changes no bit anywhere, and their gradients are exactly 0."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case)
    pad = (torch.arange(S, device=dev)[None, :] >= b["kv_len"][:, None]).reshape(B * S, 1)
    sign = 1.0 - 2.0 * ((torch.arange(B * S, device=dev)[:, None] + torch.arange(H * hd, device=dev)[None, :]) % 2)
    poison = (sign * POISON).to(BF)
    assert torch.isfinite(poison).all() and torch.equal(poison.float().abs(), torch.full_like(sign, POISON))
    results = []
    for fill in (torch.zeros_like(poison), poison):
        k = torch.where(pad, fill, b["k"])
        v = torch.where(pad, fill, b["v"])
        results.append(run(ops, b["q"], k, v, b["do"], B, S, H, hd, b["kv_len"], causal))
    (o0, lse0, dq0, dk0, dv0), (o1, lse1, dq1, dk1, dv1) = results
    assert_same_bits(o0, o1, "O")
    assert_same_bits(lse0, lse1, "lse")
    assert_same_bits(dq0, dq1, "dQ")
    assert_same_bits(dk0, dk1, "dK")     # rows < kv_len: equal; rows >= kv_len: equal and, below, zero
    assert_same_bits(dv0, dv1, "dV")
    if bool(pad.any()):
        for name, t in (("dK", dk0), ("dK", dk1), ("dV", dv0), ("dV", dv1)):
            padded = t[pad[:, 0]]
            assert torch.isfinite(padded).all() and not (padded != 0).any(), f"{name} of padded keys is not exactly 0"
    for t in (o1, lse1, dq1, dk1, dv1):
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("case", [c for c in CASES if c[2] != 64], ids=ar.case_id)
def test_bucket_length_does_not_change_a_row(ops, dev, case):
    """The same rows and kv_len laid out in a longer bucket S' give the same bits (forward)."""
    B, H, S, hd, kvl, causal = case
    S2 = 64 if S < 64 else S + 37
    assert (S <= 64) == (S2 <= 64)
    b = base(ops, dev, case)
    kv_len = torch.tensor(kvl if kvl is not None else [S] * B, dtype=torch.int32, device=dev)
    torch.manual_seed(S2)
    qkv2 = rnd(B, S2, 3 * H * hd, dev=dev)            # the new rows: finite random values
    qkv2[:, :S] = torch.cat([b["q"], b["k"], b["v"]], dim=1).reshape(B, S, 3 * H * hd)
    qkv2 = qkv2.reshape(B * S2, 3 * H * hd)
    o2, lse2 = ops.attn_fwd(qkv2[:, : H * hd], qkv2[:, H * hd: 2 * H * hd], qkv2[:, 2 * H * hd:], B, S2, H, hd, kv_len=kv_len, causal=causal)
    o, lse = b["outs"][0], b["outs"][1]
    assert_same_bits(o2.reshape(B, S2, H * hd)[:, :S].reshape(B * S, H * hd), o, "O[:, :S]")
    assert_same_bits(lse2[:, :, :S].contiguous(), lse, "lse[:, :, :S]")
    assert torch.isfinite(o2).all() and torch.isfinite(lse2).all()


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_head_is_independent_of_its_neighbours(ops, dev, case):
    """One (b, h) computed alone (B = H = 1) equals its slice of the batched call: once on strided views of the same memory
    (grid decomposition, XCD remap), once copied into buffers whose other columns hold other values (for head_dim 72 the
    columns 72..95 of a row belong to the next head)."""
    B, H, S, hd, kvl, causal = case
    bb, h = B - 1, (H - 1) // 2      # a head with a right-hand neighbour wherever H > 1
    b = base(ops, dev, case)
    o, lse, dq, dk, dv = b["outs"]
    kv1 = None if kvl is None else b["kv_len"][bb: bb + 1].clone()
    r0, r1, c0, c1 = bb * S, (bb + 1) * S, h * hd, (h + 1) * hd
    want = dict(O=o[r0:r1, c0:c1], lse=lse[bb, h], dQ=dq[r0:r1, c0:c1], dK=dk[r0:r1, c0:c1], dV=dv[r0:r1, c0:c1])

    def alone(t):
        buf = rnd(S, hd + 24, dev=dev)
        buf[:, :hd] = t[r0:r1, c0:c1]
        return buf[:, :hd]

    torch.manual_seed(1)
    for label, view in (("view", lambda t: t[r0:r1, c0:c1]), ("copy", alone)):
        got = run(ops, view(b["q"]), view(b["k"]), view(b["v"]), view(b["do"]), 1, S, 1, hd, kv1, causal)
        for (name, w), g in zip(want.items(), got):
            assert_same_bits(g.reshape(w.shape), w.contiguous(), f"{name} ({label}, b={bb}, h={h})")


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_strides_and_guard_bands(ops, dev, case):
    """Q, K, V (and dO) in separate buffers with distinct row strides, O / dQ / dK / dV written into views of larger
    buffers: same bits as the contiguous run, and not one element written outside the views."""
    B, H, S, hd, kvl, causal = case
    D, R = H * hd, B * S
    b = base(ops, dev, case)

    def strided(t, extra):
        buf = rnd(R, D + extra, dev=dev)
        buf[:, :D] = t
        return buf[:, :D]

    def guarded():
        big = torch.full((R + 16, D + 16), SENTINEL, dtype=torch.int16, device=dev)
        return big, big.view(BF)[8: 8 + R, :D]

    torch.manual_seed(2)
    q, k, v, do = strided(b["q"], 8), strided(b["k"], 16), strided(b["v"], 24), strided(b["do"], 8)
    assert len({q.stride(0), k.stride(0), v.stride(0)}) == 3
    bufs = {name: guarded() for name in ("out", "dq", "dk", "dv")}
    o, lse, dq, dk, dv = run(ops, q, k, v, do, B, S, H, hd, b["kv_len"], causal, **{n: view for n, (_, view) in bufs.items()})
    bo, blse, bdq, bdk, bdv = b["outs"]
    for name, got, want in (("O", o, bo), ("dQ", dq, bdq), ("dK", dk, bdk), ("dV", dv, bdv)):
        assert got.data_ptr() == bufs[{"O": "out", "dQ": "dq", "dK": "dk", "dV": "dv"}[name]][1].data_ptr()
        assert_same_bits(got.contiguous(), want, name)
    assert_same_bits(lse, blse, "lse")
    for name, (big, _) in bufs.items():
        inside = torch.zeros_like(big, dtype=torch.bool)
        inside[8: 8 + R, :D] = True
        touched = (big != SENTINEL) & ~inside
        assert not touched.any(), f"{name}: {int(touched.sum())} guard elements overwritten, first at {tuple(touched.nonzero()[0].tolist())}"
