"""The attention checks of `attn_reference` have teeth, shown on the CPU before a GPU is involved.

`emulate` (the kernels restated in fp32 with their bf16 roundings) must pass every check with the right mask, and
`check_counting` must reject each off-by-one mask -- every one of its lse, O and dV sub-checks on its own, and the
per-element bound on dQ of the same run.  The last two tests show that the per-element bounds see errors that a bound normalised by the largest element of the tensor cannot.
"""
import pytest
import torch

from tests import attn_reference as ar


def randn_inputs(B, H, S, hd, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, S, hd, generator=g).to(torch.bfloat16).float() for _ in range(4))


def elementwise_ratios(outs, q, k, v, do, kvl, causal, scale):
    """check_elementwise on O, dQ, dK, dV and check_lse of `outs` against the float64 reference; the worst ratios."""
    O, lse, dQ, dK, dV = outs
    rO, rlse, rdQ, rdK, rdV, P = ar.reference(q, k, v, do, kvl, causal, scale)
    bO, bdQ, bdK, bdV = ar.bounds(q, k, v, do, rO, P, scale)
    r = {"lse": ar.check_lse(lse, rlse, q, k, kvl, causal, scale)}
    for name, out, ref, bound in (("O", O, rO, bO), ("dQ", dQ, rdQ, bdQ), ("dK", dK, rdK, bdK), ("dV", dV, rdV, bdV)):
        r[name] = ar.check_elementwise(out, ref, bound, what=name)
    return r


@pytest.mark.parametrize("case", ar.CASES, ids=ar.case_id)
def test_emulation_passes_and_shifted_masks_fail(case):
    B, H, S, hd, kvl, causal = case
    scale = hd ** -0.5
    # the correct emulation passes the counting check and, on counting and random inputs alike, the per-element bounds
    cq, ck, cv, cdo = ar.counting_inputs(B, H, S, hd)
    O, lse, dQ, dK, dV = ar.emulate(cq, ck, cv, cdo, kvl, causal, scale)
    ar.check_counting(O, lse, dK, dV, kvl, causal)
    elementwise_ratios((O, lse, dQ, dK, dV), cq, ck, cv, cdo, kvl, causal, scale)
    rO, _, rdQ, _, _, P = ar.reference(cq, ck, cv, cdo, kvl, causal, scale)
    bdQ = ar.bounds(cq, ck, cv, cdo, rO, P, scale)[1]
    q, k, v, do = randn_inputs(B, H, S, hd, seed=S + hd)
    r = elementwise_ratios(ar.emulate(q, k, v, do, kvl, causal, scale), q, k, v, do, kvl, causal, scale)
    print("emulation, worst |err| / (2^-8 bound):", " ".join(f"{n} {x:.2f}" for n, x in r.items()))

    # every applicable off-by-one mask is rejected, by each sub-check that depends on the key set
    shifted = ar.shifted_masks(B, S, kvl, causal)
    assert shifted, "no shifted mask applies to this case: it would pass without having shown anything"
    for name, vis in shifted:
        O, lse, dQ, dK, dV = ar.emulate(cq, ck, cv, cdo, kvl, causal, scale, visible=vis)
        for part in ("lse", "O", "dV"):
            with pytest.raises(AssertionError):
                ar.check_counting(O, lse, dK, dV, kvl, causal, parts=(part,))
            print(f"{name}: rejected by {part}")
        ar.check_counting(O, lse, dK, dV, kvl, causal, parts=("dK",))   # Q = 0: dK is 0 whatever the mask
        # dQ has no closed form (K is random) but its dS is a count too: a row that gains or loses a key k with k % hd == s % hd
        # moves by about 1 / (2 #{visible k : k % hd == s % hd}) of its bound
        with pytest.raises(AssertionError):
            ar.check_elementwise(dQ, rdQ, bdQ, what="dQ")
        print(f"{name}: rejected by dQ")


def test_shifted_masks_obey_their_rules():
    # kv_len moves only where it stays inside [1, S]; a causal shift that blinds row 0 is dropped
    names = [n for n, _ in ar.shifted_masks(2, 64, [64, 1], False)]
    assert names == ["kv_len+1", "kv_len-1"]
    up = dict(ar.shifted_masks(2, 64, [64, 1], False))["kv_len+1"]
    assert up[0].sum(-1).unique().tolist() == [64] and up[1].sum(-1).unique().tolist() == [2]
    assert [n for n, _ in ar.shifted_masks(1, 50, None, True)] == ["kv_len-1", "causal+1"]
    assert ar.shifted_masks(1, 50, None, False)[0][0] == "kv_len-1"


# A long causal context: row 0 returns v[0] (magnitude up to ~4) while a late row averages a thousand values, the situation
# in which a bound that follows the largest element of the tensor sees nothing.
LONG = (1, 1, 1159, 128, None, True)


@pytest.fixture(scope="module")
def long_case():
    B, H, S, hd, kvl, causal = LONG
    scale = hd ** -0.5
    q, k, v, do = randn_inputs(B, H, S, hd, seed=7)
    O, lse, dQ, dK, dV = ar.emulate(q, k, v, do, kvl, causal, scale)
    rO, rlse, rdQ, rdK, rdV, P = ar.reference(q, k, v, do, kvl, causal, scale)
    bO, bdQ, bdK, bdV = ar.bounds(q, k, v, do, rO, P, scale)
    return dict(q=q, k=k, scale=scale, lse=(lse, rlse), O=(O, rO, bO, 1100, 2e-2), dV=(dV, rdV, bdV, 500, 3e-2))


@pytest.mark.parametrize("which", ["O", "dV"])
def test_elementwise_bound_sees_one_row_that_is_a_quarter_off(long_case, which):
    """A late row (O) or a late key's row (dV) that is 25 % too small: under `tol * max|ref|` with the tolerance the existing
    test uses, far outside 3 * 2^-8 * bound.  (dQ and dK are left out: their bounds carry |dO| |V|^T + |delta| where the
    result has dP - delta and sums with signs, so on random data a whole late row is only 3 to 7 units of 2^-8 * bound; what
    pins their key sets is the counting run.)"""
    out, ref, bound, row, old_tol = long_case[which]
    out = out.clone()
    ar.check_elementwise(out, ref, bound, what=which)
    out[0, 0, row] *= 0.75
    assert float((out - ref).abs().max()) < old_tol * float(ref.abs().max()), "a max-normalised bound would see this too"
    with pytest.raises(AssertionError):
        ar.check_elementwise(out, ref, bound, what=which)


def test_lse_bound_sees_a_small_error(long_case):
    """1e-3 in one LSE: an error in the fourth significant digit, and seventy times below 1e-2 of the largest LSE."""
    B, H, S, hd, kvl, causal = LONG
    lse, ref = long_case["lse"]
    lse = lse.clone()
    ar.check_lse(lse, ref, long_case["q"], long_case["k"], kvl, causal, long_case["scale"])
    lse[0, 0, 300] += 1e-3
    assert 1e-3 < 1e-2 * float(ref.abs().max()) / 50
    with pytest.raises(AssertionError):
        ar.check_lse(lse, ref, long_case["q"], long_case["k"], kvl, causal, long_case["scale"])
