"""ovla_argmax_bins: lowest index of the row maximum over [0, vocab) of bf16 logits, and the action-bin index
clip(n_tokens - token - 1, 0, n_bins - 1) (modeling_prismatic.py:929-942), against numpy on the fp32 copy."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ROWS, N_BINS = 5, 255
NEG = float("-inf")


def _base(vocab, seed):
    ld = (vocab + 7) // 8 * 8 + 8
    x = torch.randn(ROWS, ld, generator=torch.Generator().manual_seed(seed)).to(BF)
    x[:, vocab:] = 1000.0          # strictly larger than anything inside [0, vocab): must never be read into the result
    return x


def _n_tokens(vocab):
    return vocab - 64 if vocab - 64 > 0 else vocab


def _run(ops, dev, x, vocab):
    n_tokens = _n_tokens(vocab)
    tok, bins = ops.argmax_bins(x.to(dev), vocab=vocab, n_tokens=n_tokens, n_bins=N_BINS)
    torch.cuda.synchronize()
    assert tok.dtype == torch.int32 and bins.dtype == torch.int32
    want_tok = np.argmax(x[:, :vocab].float().numpy(), axis=1)       # numpy: the first occurrence of the maximum
    want_bin = np.clip(n_tokens - want_tok - 1, 0, N_BINS - 1)
    assert np.array_equal(tok.cpu().numpy(), want_tok), (tok.cpu().numpy(), want_tok)
    assert np.array_equal(bins.cpu().numpy(), want_bin), (bins.cpu().numpy(), want_bin)
    return want_tok, want_bin


@pytest.mark.parametrize("vocab", [7, 64, 1000, 32064])
def test_positions_and_ties(ops, dev, vocab):
    x = _base(vocab, vocab)
    far = 517 if vocab > 517 else vocab - 1
    group_last = (vocab // 16) * 8 + 7 if vocab >= 8 else vocab - 1   # last column of a 16-byte group in the middle of the row
    x[0, 0] = 100.0
    x[1, vocab - 1] = 100.0
    x[2, group_last] = 100.0
    x[3, 3] = x[3, far] = 100.0                                       # two equal maxima far apart: the lower index
    x[4, :vocab] = 0.5                                                # all equal: column 0
    tok, bins = _run(ops, dev, x, vocab)
    assert tok.tolist() == [0, vocab - 1, group_last, 3, 0]
    if vocab >= 1000:   # column 0 clips at the top bin, the last column (beyond n_tokens) at bin 0
        assert bins[0] == N_BINS - 1 and _n_tokens(vocab) - 1 > N_BINS - 1 and bins[1] == 0 and _n_tokens(vocab) - vocab < 0


@pytest.mark.parametrize("vocab", [7, 64, 1000, 32064])
def test_minus_infinity_and_unclipped_bins(ops, dev, vocab):
    x = _base(vocab, vocab + 1)
    n_tokens = _n_tokens(vocab)
    mid = max(n_tokens - 101, 0)                                      # decodes to bin 100 where the vocabulary is large enough
    x[0, :vocab] = NEG
    x[0, vocab // 2] = -3.0                                           # one finite column in a row of -inf
    x[1, :vocab: 3] = NEG                                             # -inf scattered through a random row
    x[2, :vocab] = NEG                                                # nothing but -inf: column 0
    x[3, mid] = 100.0
    x[4, :vocab] = NEG
    x[4, vocab - 1] = x[4, vocab - 2] = -1.0                          # a tie in the vocab % 8 tail (or the last group)
    tok, bins = _run(ops, dev, x, vocab)
    assert tok[0] == vocab // 2 and tok[2] == 0 and tok[3] == mid and tok[4] == vocab - 2
    if vocab >= 1000:
        assert bins[3] == 100


def test_rows_that_do_not_start_on_16_bytes(ops, dev):
    """A view whose rows start off a 16-byte boundary takes the column-by-column path: same answers."""
    vocab = 1000
    x = _base(vocab, 5)
    x[0, 0] = x[1, vocab - 1] = 100.0
    x[2, 3] = x[2, 517] = 100.0
    wide = torch.zeros(ROWS, x.shape[1] + 1, dtype=BF)
    wide[:, 1:] = x
    view = wide.to(dev)[:, 1:]
    assert view.data_ptr() % 16 != 0
    tok, bins = ops.argmax_bins(view, vocab=vocab, n_tokens=_n_tokens(vocab), n_bins=N_BINS)
    want = np.argmax(x[:, :vocab].float().numpy(), axis=1)
    assert np.array_equal(tok.cpu().numpy(), want) and tok[:3].tolist() == [0, vocab - 1, 3]
    assert np.array_equal(bins.cpu().numpy(), np.clip(_n_tokens(vocab) - want - 1, 0, N_BINS - 1))
