"""The checks of `tests/attn_probs_reference.py` pass what is right and reject what is off by one, on the CPU; and the C-ABI entry and
its wrapper exist (no GPU needed: the struct table is derived from include/ovla.h)."""
import importlib

import pytest
import torch

from tests import attn_probs_reference as pr
from tests import attn_reference as ar
from tests.conftest import load_pkg

CASES = pr.CPU_CASES


def _setup(case, gain):
    B, H, S, hd, kvl, causal = case
    scale = hd ** -0.5
    q, k, v = pr.inputs(case, gain)
    P_ref, lse_ref, E = pr.reference(q, k, v, kvl, causal, scale)
    return q, k, v, P_ref, lse_ref, E, scale


def _flat(T):
    """[B, H, S, ...] -> [B*S, H, ...] (the all-rows order of the kernel)."""
    return T.transpose(1, 2).reshape((T.shape[0] * T.shape[2], T.shape[1]) + tuple(T.shape[3:]))


@pytest.mark.parametrize("gain", [1.0, 3.0])
@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_fp32_restatement_passes(case, gain):
    """The formula evaluated in fp32 is far inside the bound, with lse_ref rounded to fp32 (c = 1) and with the lse of the fp32 forward
    restatement `attn_reference.emulate` (c = 2): below 0.02 units either way."""
    B, H, S, hd, kvl, causal = case
    q, k, v, P_ref, lse_ref, E, scale = _setup(case, gain)
    lse_emu = ar.emulate(q, k, v, torch.zeros_like(v), kvl, causal, scale)[1]
    ar.check_lse(lse_emu, lse_ref, q, k, kvl, causal, scale)
    valid = torch.ones(B * S, dtype=torch.bool)
    for lse, c in ((lse_ref.float(), 1), (lse_emu, 2)):
        P = pr.restate(q, k, lse, kvl, causal, scale)
        worst = pr.check_probs(_flat(P), _flat(P_ref), _flat(E), c)
        wsum = pr.check_row_sums(_flat(P), _flat(E), valid, c)
        print(f"\n{ar.case_id(case)} gain {gain} c={c}: worst element {worst:.4f} units, worst row sum {wsum:.4f} units")
        assert worst < 0.02 and wsum < 0.02


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_bf16_rounded_probabilities_are_rejected(case):
    """At gain 1 a P that went through bf16 (2^-9 relative) is outside the bound: the check separates an fp32 result from a bf16 one."""
    q, k, v, P_ref, lse_ref, E, scale = _setup(case, 1.0)
    P = ar._bf(pr.restate(q, k, lse_ref.float(), case[4], case[5], scale))
    with pytest.raises(AssertionError):
        pr.check_probs(_flat(P), _flat(P_ref), _flat(E), 2)


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_shifted_masks_are_rejected(case):
    """Every off-by-one variant of the mask (kv_len +- 1, causal diagonal +- 1) fails the elementwise check."""
    B, H, S, hd, kvl, causal = case
    q, k, v, P_ref, lse_ref, E, scale = _setup(case, 1.0)
    variants = ar.shifted_masks(B, S, kvl, causal)
    assert variants or (kvl is None and not causal)
    for name, vis in variants:
        P = pr.restate(q, k, lse_ref.float(), kvl, causal, scale, visible=vis)
        with pytest.raises(AssertionError):
            pr.check_probs(_flat(P), _flat(P_ref), _flat(E), 2, what=name)


@pytest.mark.parametrize("case", CASES, ids=ar.case_id)
def test_counting_inputs_give_uniform_rows(case):
    """Q = 0: P is 1 / n(s) on the visible keys; a shifted mask changes n and is rejected."""
    B, H, S, hd, kvl, causal = case
    scale = hd ** -0.5
    q, k, v, _ = ar.counting_inputs(B, H, S, hd)
    P_ref, lse_ref, E = pr.reference(q, k, v, kvl, causal, scale)
    exact = pr.counting_expected(B, S, kvl, causal).expand(B, H, S, S)
    assert float((P_ref - exact).abs().max()) < 1e-15
    P = pr.restate(q, k, lse_ref.float(), kvl, causal, scale)
    pr.check_probs(_flat(P), _flat(exact), _flat(E), 1, what="counting")
    for name, vis in ar.shifted_masks(B, S, kvl, causal):
        with pytest.raises(AssertionError):
            pr.check_probs(_flat(pr.restate(q, k, lse_ref.float(), kvl, causal, scale, visible=vis)), _flat(exact), _flat(E), 1, what=name)


def test_gather_and_row_list():
    B, S = 3, 130
    rows = pr.row_list(B, S)
    assert len(rows) == 21 and -1 in rows and B * S in rows and len(set(rows)) == 20
    T = torch.arange(B * 2 * S * 5, dtype=torch.float64).reshape(B, 2, S, 5)
    G = pr.gather(T, rows)
    for i, r in enumerate(rows):
        want = torch.zeros(2, 5, dtype=torch.float64) if not 0 <= r < B * S else T[r // S, :, r % S]
        assert torch.equal(G[i], want)


def test_head_mean_order():
    """head_mean is the sequential fp32 sum: it differs from a pairwise or float64 mean in the last bits on random data."""
    torch.manual_seed(0)
    P = torch.rand(7, 5, 33)
    m = pr.head_mean(P)
    acc = torch.zeros(7, 33)
    for h in range(5):
        acc += P[:, h]
    assert torch.equal(m, acc * torch.tensor(1.0 / 5.0, dtype=torch.float32))


def test_abi_entry_and_wrapper_exist():
    """include/ovla.h declares ovla_attn_probs with the documented fields and ops.attn_probs wraps it."""
    load_pkg()
    lib = importlib.import_module("openvla-oft_amd._lib")
    ops = importlib.import_module("openvla-oft_amd.ops")
    assert "ovla_attn_probs_args" in lib.STRUCTS
    names = [n for n, _ in lib.STRUCT_FIELDS["ovla_attn_probs_args"]]
    assert names == ["Q", "K", "q_stride", "k_stride", "lse", "kv_len", "rows", "P", "P_mean", "B", "H", "S", "R", "head_dim", "causal", "scale"]
    assert lib.FUNCTIONS["ovla_attn_probs"] == ("int", [("struct", "ovla_attn_probs_args"), ("plain", "void*")])
    assert callable(ops.attn_probs)
    engine = importlib.import_module("openvla-oft_amd.engine")
    cap = engine.AttnCapture(rows="actions", per_head=False, layers=None)
    assert cap.rows == "actions" and not cap.per_head
    with pytest.raises(ValueError):
        engine.AttnCapture(rows="everything")
