"""ovla_language_average_ragged: FiLM's conditioning vectors of a right-padded batch in one launch, bit for bit ovla_language_average on
every unpadded row."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
IGNORE, STOP, ACTION = -100, 2, 31744 + 5   # labels: not counted as a label / the stop token / an action token (> 31743)
B, L, D, VOCAB, PAD = 3, 24, 64, 512, 511


@pytest.fixture(scope="module")
def case(dev):
    g = torch.Generator().manual_seed(11)
    table = torch.randn(VOCAB, D, generator=g).to(BF)
    table[PAD] = 1e3                                         # a pad token that leaks into a mean is visible at once
    ids = torch.randint(1, 500, (B, L), generator=g)
    labels = torch.full((B, L), IGNORE, dtype=torch.int64)
    labels[0, 16:23], labels[0, 23] = ACTION, STOP           # 24 tokens: prompt, 7 action tokens, stop
    labels[1, 10:17] = ACTION                                # 17 tokens: the LAST counted position is an action token
    labels[2, 5:8], labels[2, 8] = ACTION, STOP              # 9 tokens
    return dict(table=table, ids=ids, labels=labels, dtable=table.to(dev))


def _check(ops, dev, case, lens):
    ids, labels = case["ids"].clone(), case["labels"].clone()
    for b, n in enumerate(lens):
        ids[b, n:], labels[b, n:] = PAD, IGNORE              # what a collator leaves behind a row: pad ids under ignored labels
    out = torch.zeros((8, D), dtype=BF, device=dev)
    ops.language_average_ragged(ids.to(dev), labels.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev), case["dtable"], out)
    assert torch.equal(out[B:], torch.zeros_like(out[B:])), "rows beyond B are not written"
    for b, n in enumerate(lens):
        alone = torch.zeros((1, D), dtype=BF, device=dev)
        ops.language_average(ids[b: b + 1, :n].contiguous().to(dev), labels[b: b + 1, :n].contiguous().to(dev), case["dtable"], alone)
        assert torch.equal(out[b].view(torch.int16), alone[0].view(torch.int16)), f"row {b} (length {n}) differs from the unpadded row's average"
        # and both are the masked mean: fp32 sum in position order, one rounding (half a bf16 ulp = 2^-9 relative)
        keep = labels[b, :n] <= 31743
        s = torch.zeros(D)
        for i in torch.nonzero(keep).flatten().tolist():
            s = s + case["table"][ids[b, i]].float()
        ref = s / float(keep.sum())
        assert torch.allclose(out[b].float().cpu(), ref, rtol=2.0 ** -8, atol=1e-6), f"row {b}"
        assert out[b].float().abs().max().item() < 10.0, "no pad row (1e3) entered the mean"


def test_ragged_rows_equal_the_unpadded_average(ops, dev, case):
    _check(ops, dev, case, (24, 17, 9))


def test_length_one_rows(ops, dev, case):
    _check(ops, dev, case, (1, 1, 1))
