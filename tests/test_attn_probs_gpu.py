"""`ops.attn_probs` (csrc/attn_probs.hip): the attention probabilities of a list of query rows, recomputed from the q | k the forward
consumed and the lse it wrote.  Per-element bounds against the float64 reference, exact zeros, exact head mean, row gathering, operand
isolation and consistency with the forward's own O.  The reference and the bound: tests/attn_probs_reference.py (shown to have teeth
on the CPU by tests/test_attn_probs_reference.py)."""
import ctypes
import importlib

import pytest
import torch

from tests import attn_probs_reference as pr
from tests import attn_reference as ar

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CASES = pr.GPU_CASES
SENTINEL = 12345.0


def to_rows(t, dev):
    """[B, H, S, hd] (CPU) -> bf16 [B*S, H*hd] on the device."""
    B, H, S, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * hd).to(BF).to(dev)


def flat(T):
    """[B, H, S, ...] -> [B*S, H, ...]: the all-rows order."""
    return T.transpose(1, 2).reshape((T.shape[0] * T.shape[2], T.shape[1]) + tuple(T.shape[3:]))


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    if not torch.equal(a, b):
        diff = (a != b).nonzero()
        raise AssertionError(f"{what}: {len(diff)} of {a.numel()} elements differ, first at {tuple(diff[0].tolist())}: "
                             f"{a[tuple(diff[0])].item()} vs {b[tuple(diff[0])].item()}")


_BASE = {}


def base(ops, dev, case, gain=1.0, counting=False):
    """Inputs in the fused [B*S, 3*H*hd] layout, the device forward, the float64 reference and the all-rows probabilities for both lse
    sources, computed once per (case, inputs) and shared read-only."""
    key = (ar.case_id(case), gain, counting)
    if key not in _BASE:
        B, H, S, hd, kvl, causal = case
        scale = hd ** -0.5
        if counting:
            q, k, v, _ = ar.counting_inputs(B, H, S, hd)
        else:
            q, k, v = pr.inputs(case, gain)
        P_ref, lse_ref, E = pr.reference(q, k, v, kvl, causal, scale)
        qkv = torch.cat([to_rows(t, dev) for t in (q, k, v)], dim=1).contiguous()
        D = H * hd
        dq, dk, dv = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        kv_len = torch.tensor(kvl, dtype=torch.int32, device=dev)
        o, lse_dev = ops.attn_fwd(dq, dk, dv, B, S, H, hd, kv_len=kv_len, causal=causal)
        ar.check_lse(lse_dev.cpu(), lse_ref, q, k, kvl, causal, scale)
        lse_in = {"ref": lse_ref.float().to(dev).contiguous(), "dev": lse_dev}
        full = {n: ops.attn_probs(dq, dk, l, B, S, H, hd, kv_len=kv_len, causal=causal, per_head=True, mean=True) for n, l in lse_in.items()}
        rows = pr.row_list(B, S)
        _BASE[key] = dict(q=q, k=k, v=v, P_ref=P_ref, lse_ref=lse_ref, E=E, qkv=qkv, dq=dq, dk=dk, dv=dv, kv_len=kv_len, o=o, lse=lse_in,
                          full=full, rows=rows, rows_dev=torch.tensor(rows, dtype=torch.int32, device=dev), scale=scale)
    return _BASE[key]


def gathered(ops, b, case, src, **kw):
    B, H, S, hd, kvl, causal = case
    return ops.attn_probs(b["dq"], b["dk"], b["lse"][src], B, S, H, hd, rows=b["rows_dev"], kv_len=b["kv_len"], causal=causal, **kw)


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [1.0, 3.0])
@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_elementwise_bound_zeros_and_row_sums(ops, dev, case, gain):
    """|P - P_ref| <= c * P_ref * E + 2^-126 per element, exactly 0 on masked keys, |sum_k P - 1| <= c * E: all rows and the gathered
    list, with lse_ref (c = 1) and with the device forward's lse (c = 2).  Gain 1 is the deciding case (a bf16 P fails it)."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case, gain)
    rows = b["rows"]
    valid = torch.tensor([0 <= r < B * S for r in rows])
    for src, c in (("ref", 1), ("dev", 2)):
        P_all = b["full"][src][0].cpu()
        w_all = pr.check_probs(P_all, flat(b["P_ref"]), flat(b["E"]), c, what=f"P all rows ({src})")
        s_all = pr.check_row_sums(P_all, flat(b["E"]), torch.ones(B * S, dtype=torch.bool), c, what=f"row sums all rows ({src})")
        P_g = gathered(ops, b, case, src, per_head=True, mean=False)[0].cpu()
        w_g = pr.check_probs(P_g, pr.gather(b["P_ref"], rows), pr.gather(b["E"], rows), c, what=f"P gathered ({src})")
        s_g = pr.check_row_sums(P_g, pr.gather(b["E"], rows), valid, c, what=f"row sums gathered ({src})")
        print(f"\n{ar.case_id(case)} gain {gain} lse {src} (c = {c}): worst element {w_all:.3f} / {w_g:.3f} units, row sum {s_all:.3f} / {s_g:.3f} units")


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_counting_inputs_give_one_over_n(ops, dev, case):
    """Q = 0: every visible key of row s holds 1 / n(s); one key too many or too few is far outside the bound."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case, counting=True)
    exact = pr.counting_expected(B, S, kvl, causal).expand(B, H, S, S)
    for src, c in (("ref", 1), ("dev", 2)):
        pr.check_probs(b["full"][src][0].cpu(), flat(exact), flat(b["E"]), c, what=f"counting ({src})")
        pr.check_probs(gathered(ops, b, case, src, per_head=True)[0].cpu(), pr.gather(exact, b["rows"]), pr.gather(b["E"], b["rows"]), c,
                       what=f"counting gathered ({src})")


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_head_mean_is_the_fixed_order_mean(ops, dev, case):
    """P_mean is bit-equal to the sequential fp32 mean over h = 0 .. H-1 of the returned P, whether or not P is written too."""
    b = base(ops, dev, case)
    P, Pm = b["full"]["dev"]
    same_bits(Pm, pr.head_mean(P), "P_mean vs head_mean(P), all rows")
    Pg, Pmg = gathered(ops, b, case, "dev", per_head=True, mean=True)
    same_bits(Pmg, pr.head_mean(Pg), "P_mean vs head_mean(P), gathered")
    none, only = gathered(ops, b, case, "dev", per_head=False, mean=True)
    assert none is None
    same_bits(only, Pmg, "P_mean alone vs P_mean beside P")


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_gathered_rows_equal_the_all_rows_call(ops, dev, case):
    """A listed row holds the bits of that row in the all-rows call, wherever it stands in the list (permuted, repeated); a -1 and an
    index >= B*S give zero rows."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case)
    P, Pm = b["full"]["dev"]
    Pg, Pmg = gathered(ops, b, case, "dev", per_head=True, mean=True)
    rows = b["rows"]
    n_bad = 0
    for i, r in enumerate(rows):
        if 0 <= r < B * S:
            same_bits(Pg[i], P[r], f"P list entry {i} (row {r})")
            same_bits(Pmg[i], Pm[r], f"P_mean list entry {i} (row {r})")
        else:
            n_bad += 1
            assert not (Pg[i] != 0).any() and not (Pmg[i] != 0).any(), f"list entry {i} (index {r}) is not a zero row"
    assert n_bad == 2
    # another list length and order: the same bits again (nothing depends on R or on the position)
    rev = [r for r in reversed(rows) if 0 <= r < B * S][:7]
    P7, Pm7 = ops.attn_probs(b["dq"], b["dk"], b["lse"]["dev"], B, S, H, hd, rows=torch.tensor(rev, dtype=torch.int32, device=dev),
                             kv_len=b["kv_len"], causal=causal, per_head=True)
    for i, r in enumerate(rev):
        same_bits(P7[i], P[r], f"P short list entry {i} (row {r})")
        same_bits(Pm7[i], Pm[r], f"P_mean short list entry {i} (row {r})")


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_operand_isolation(ops, dev, case):
    """NaN in another batch entry's Q and K, in the K rows >= kv_len and in the Q rows that are not listed leaves the listed rows of
    one batch entry bit-unchanged and finite."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case)
    D = H * hd
    bb = B - 1                                               # the entry with the shortest kv_len: its own padding rows are poisoned too
    mine = [r for r in b["rows"] if bb * S <= r < (bb + 1) * S]
    assert mine and int(b["kv_len"][bb]) < S
    rows_dev = torch.tensor(mine + [-1], dtype=torch.int32, device=dev)
    want = ops.attn_probs(b["dq"], b["dk"], b["lse"]["dev"], B, S, H, hd, rows=rows_dev, kv_len=b["kv_len"], causal=causal, per_head=True)
    qkv = b["qkv"].clone()
    r_idx = torch.arange(B * S, device=dev)
    other = (r_idx // S) != bb
    pad = (r_idx % S) >= b["kv_len"][r_idx // S]
    unlisted = torch.ones(B * S, dtype=torch.bool, device=dev)
    unlisted[torch.tensor(mine, device=dev)] = False
    nan = torch.tensor(float("nan"), dtype=BF, device=dev)
    qkv[:, :D] = torch.where((other | unlisted)[:, None], nan, qkv[:, :D])
    qkv[:, D:2 * D] = torch.where((other | pad)[:, None], nan, qkv[:, D:2 * D])
    lse = b["lse"]["dev"].clone()
    lse[:bb] = float("nan")                                  # the other entries' statistics are not read either
    got = ops.attn_probs(qkv[:, :D], qkv[:, D:2 * D], lse, B, S, H, hd, rows=rows_dev, kv_len=b["kv_len"], causal=causal, per_head=True)
    for name, g, w in (("P", got[0], want[0]), ("P_mean", got[1], want[1])):
        assert torch.isfinite(g).all(), f"{name}: a NaN outside the row's operands reached the output"
        same_bits(g, w, name)


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_probabilities_reproduce_the_forward_output(ops, dev, case):
    """P_dev @ V against the device forward's O at the listed rows, inside the forward's own bound (check_elementwise, c = 3)."""
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case)
    rows = [r for r in b["rows"] if 0 <= r < B * S]
    P = ops.attn_probs(b["dq"], b["dk"], b["lse"]["dev"], B, S, H, hd, rows=torch.tensor(rows, dtype=torch.int32, device=dev),
                       kv_len=b["kv_len"], causal=causal, per_head=True, mean=False)[0].cpu().double()
    v = b["v"].double()
    PV = torch.stack([torch.einsum("hs,hsd->hd", P[i], v[r // S]) for i, r in enumerate(rows)])
    O = b["o"].cpu().double().reshape(B * S, H, hd)[rows]
    bO = pr.gather(b["P_ref"] @ v.abs(), rows)
    ar.check_elementwise(O, PV, bO, c=3, what="device O vs P_dev @ V")


def _args(lib, **f):
    g = lib.STRUCTS["ovla_attn_probs_args"]()
    for k, val in f.items():
        setattr(g, k, val)
    return g


def test_invalid_arguments_are_refused(ops, dev):
    """head_dim 72, null pointers, R = 0, neither output, rows == NULL with R != B*S and a stride that breaks the 16-byte loads:
    OVLA_EINVAL with a message, and the output buffers keep their bits."""
    lib = importlib.import_module("openvla-oft_amd._lib")
    B, H, S, hd = 1, 2, 64, 128
    qkv = torch.randn(B * S, 2 * H * hd + 8, device=dev).to(BF)
    lse = torch.zeros(B, H, S, device=dev)
    P = torch.full((B * S, H, S), SENTINEL, device=dev)
    Pm = torch.full((B * S, S), SENTINEL, device=dev)
    rows = torch.arange(B * S, dtype=torch.int32, device=dev)
    good = dict(Q=qkv.data_ptr(), K=qkv[:, H * hd:].data_ptr(), q_stride=qkv.stride(0), k_stride=qkv.stride(0), lse=lse.data_ptr(), kv_len=None,
                rows=rows.data_ptr(), P=P.data_ptr(), P_mean=Pm.data_ptr(), B=B, H=H, S=S, R=B * S, head_dim=hd, causal=0, scale=hd ** -0.5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = {"head_dim 72": dict(head_dim=72), "null Q": dict(Q=None), "null K": dict(K=None), "null lse": dict(lse=None),
           "no output": dict(P=None, P_mean=None), "R = 0": dict(R=0), "R < 0": dict(R=-3), "rows NULL, R != B*S": dict(rows=None, R=5),
           "q_stride % 8": dict(q_stride=qkv.stride(0) + 4), "k_stride % 8": dict(k_stride=qkv.stride(0) + 2),
           "Q misaligned": dict(Q=qkv.data_ptr() + 2), "empty": dict(S=0)}
    for name, change in bad.items():
        rc = lib.lib().ovla_attn_probs(ctypes.byref(_args(lib, **{**good, **change})), stream)
        msg = lib.lib().ovla_last_error().decode()
        assert rc != 0 and "ovla_attn_probs" in msg, f"{name}: rc {rc}, message {msg!r}"
    with pytest.raises(lib.OvlaError, match="head_dim 72"):
        ops.attn_probs(qkv[:, :H * 72], qkv[:, H * hd:H * hd + H * 72], lse, B, S, H, 72, out=(P, Pm))
    torch.cuda.synchronize()
    assert bool((P == SENTINEL).all()) and bool((Pm == SENTINEL).all()), "a refused call wrote to its outputs"
    rc = lib.lib().ovla_attn_probs(ctypes.byref(_args(lib, **good)), stream)                   # the unchanged arguments are accepted
    assert rc == 0, lib.lib().ovla_last_error().decode()
    torch.cuda.synchronize()
    assert not bool((P == SENTINEL).any()) and not bool((Pm == SENTINEL).any())


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_two_runs_give_the_same_bits(ops, dev, case):
    B, H, S, hd, kvl, causal = case
    b = base(ops, dev, case)
    again = ops.attn_probs(b["dq"], b["dk"], b["lse"]["dev"], B, S, H, hd, kv_len=b["kv_len"], causal=causal, per_head=True, mean=True)
    same_bits(again[0], b["full"]["dev"][0], "P")
    same_bits(again[1], b["full"]["dev"][1], "P_mean")
    g0, g1 = (gathered(ops, b, case, "dev", per_head=True, mean=True) for _ in range(2))
    same_bits(g0[0], g1[0], "P gathered")
    same_bits(g0[1], g1[1], "P_mean gathered")
