"""ovla_sample_tokens against the numpy restatement of THE SAMPLING CONTRACT (tests/token_sample_reference.py): forced and flat rows exactly,
general rows wherever the float64 keys decide, log-probability and entropy within their derived bounds, isolation from everything outside
the window, purity in (seed, call, row key), the device-side state, and the refusals."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import token_sample_reference as R
from tests.pointwise_reference import assert_abs

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_BINS = 255
SEED, CALL = 0x1234_5678_9ABC_DEF0, 17
ROWS = (1, 7, 56)
SHAPES = ((1000, 1000), (32000, 32064))


def windows(vocab):
    return ((vocab - 256, vocab), (0, vocab), (3, 261))


def _draw(ops, dev, z, vocab, window, T, *, seed=SEED, call=CALL, keys=None, **kw):
    zd = z if z.is_cuda else z.to(dev)
    kd = None if keys is None else torch.as_tensor(np.asarray(keys), dtype=torch.int32).to(dev)
    tok, bins, lp, ent = ops.sample_tokens(zd, n_tokens=vocab, n_bins=N_BINS, vocab=vocab, window=window, temperature=T, seed=seed, call=call, row_key=kd, **kw)
    torch.cuda.synchronize()
    tok, bins = tok.cpu().numpy(), bins.cpu().numpy()
    assert np.array_equal(bins, np.clip(vocab - tok - 1, 0, N_BINS - 1)), "bin != clip(n_tokens - token - 1, 0, n_bins - 1)"
    return tok, bins, lp.cpu(), (None if ent is None else ent.cpu())


def _check_stats(z, window, T, tok, lp, ent, what):
    st = R.row_stats_ref(z, *window, T, tok)
    assert_abs(lp, st["logprob"], st["logprob_bound"], what + " logprob")
    assert_abs(ent, st["entropy"], st["entropy_bound"], what + " entropy")


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_forced_rows(ops, dev, rows, vocab, ld):
    """One window column more than 19.5 T above every other: the Gumbel range [-2.812, 16.636] cannot bridge it, whatever the seed and call."""
    for wi, (lo, hi) in enumerate(windows(vocab)):
        g = torch.Generator().manual_seed(100 + rows + wi)
        z = R.eighths(g, (rows, ld))
        spots = [lo, hi - 1, lo + 5, ((lo + 8) // 8) * 8, ((hi - 1) // 8) * 8 - 1, (lo + hi) // 2, lo + 1]
        forced = np.array([spots[r % len(spots)] for r in range(rows)])
        z[torch.arange(rows), torch.as_tensor(forced)] = 40.0            # the others are <= 8 and 32 > 19.5 * 1.6
        zd = z.to(dev)
        for T in R.GENERAL_T:
            for seed, call in ((SEED, CALL), (1, 0), (0xFFFF_FFFF_FFFF_FFFF, 0xFFFF_FFFF)):
                tok, _, lp, ent = _draw(ops, dev, zd, vocab, (lo, hi), T, seed=seed, call=call)
                assert np.array_equal(tok, forced), f"window [{lo}, {hi}) T={T}: a forced row drew another token"
            _check_stats(z, (lo, hi), T, tok, lp, ent, f"forced rows={rows} window [{lo}, {hi}) T={T}")   # (the float64 logprob is -7e-6 .. 0)


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_flat_rows(ops, dev, rows, vocab, ld):
    """Equal logits: the lowest index holding the largest 23-bit integer -- an integer reference, no logarithm in it."""
    for wi, (lo, hi) in enumerate(windows(vocab)):
        g = torch.Generator().manual_seed(200 + rows + wi)
        z = R.eighths(g, (rows, ld))
        z[:, lo:hi] = 0.5
        for call in (CALL, CALL + 1):
            want, _ = R.flat_token_ref(np.arange(rows), lo, hi, seed=SEED, call=call)
            tok, _, lp, ent = _draw(ops, dev, z, vocab, (lo, hi), 1.6, call=call)
            assert np.array_equal(tok, want), f"flat rows={rows} window [{lo}, {hi}) call={call}"
        _check_stats(z, (lo, hi), 1.6, tok, lp, ent, f"flat rows={rows} window [{lo}, {hi})")


@pytest.mark.parametrize("vocab,ld", SHAPES)
@pytest.mark.parametrize("wi", (0, 1, 2))
def test_general_rows(ops, dev, vocab, ld, wi):
    """4096 (logits row, row key) pairs per temperature: the token is the restatement's wherever the float64 top-two gap exceeds max(4 e, 1e-3)."""
    lo, hi = windows(vocab)[wi]
    z, keys = R.general_rows(vocab, ld, lo, hi)
    zd = z.to(dev)
    for T in R.GENERAL_T:
        ref = R.general_ref(z, keys, lo, hi, T, seed=SEED, call=CALL)
        got = np.empty((R.GENERAL_ROWS, R.GENERAL_KEYS), dtype=np.int32)
        for k, key in enumerate(keys.tolist()):
            tok, _, lp, ent = _draw(ops, dev, zd, vocab, (lo, hi), T, keys=np.full(R.GENERAL_ROWS, key))
            got[:, k] = tok
            if k == 0:
                _check_stats(z, (lo, hi), T, tok, lp, ent, f"general vocab {vocab} window [{lo}, {hi}) T={T}")
        got = got.reshape(-1)
        decided = ref["decided"]
        assert 1.0 - decided.mean() <= 0.01, f"{100 * (1.0 - decided.mean()):.2f} % of the rows inside the near-tie margin"
        bad = np.nonzero(decided & (got != ref["token"]))[0]
        assert bad.size == 0, (f"vocab {vocab} window [{lo}, {hi}) T={T}: {bad.size} decided rows differ; first flat index {bad[0]}: got {got[bad[0]]} want "
                               f"{ref['token'][bad[0]]} gap {ref['gap'][bad[0]]:.3g} e {ref['e'][bad[0]]:.3g}")
        assert (got >= lo).all() and (got < hi).all()


def test_rows_off_16_bytes_take_the_scalar_path_to_the_same_bits(ops, dev):
    vocab, lo, hi = 1000, 3, 261
    z = R.eighths(torch.Generator().manual_seed(3), (7, vocab))
    wide = torch.zeros(7, vocab + 1, dtype=BF)
    wide[:, 1:] = z
    view = wide.to(dev)[:, 1:]
    assert view.data_ptr() % 16 != 0
    a = _draw(ops, dev, z, vocab, (lo, hi), 1.6)
    b = _draw(ops, dev, view, vocab, (lo, hi), 1.6)
    assert np.array_equal(a[0], b[0]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))


@pytest.mark.parametrize("window", ((744, 1000), (3, 261)))
def test_isolation(ops, dev, window):
    vocab, ld = 1000, 1008
    lo, hi = window
    z = R.eighths(torch.Generator().manual_seed(4), (56, ld))
    base = _draw(ops, dev, z, vocab, window, 1.0)
    p = z.clone()
    outside = torch.ones(ld, dtype=torch.bool)
    outside[lo:hi] = False
    idx = torch.nonzero(outside)[:, 0]
    p[:, idx[0::3]] = float("nan")
    p[:, idx[1::3]] = float("inf")
    p[:, idx[2::3]] = 3e38
    got = _draw(ops, dev, p, vocab, window, 1.0)
    assert np.array_equal(base[0], got[0]) and np.array_equal(base[1], got[1])
    assert torch.equal(base[2].view(torch.int32), got[2].view(torch.int32)) and torch.equal(base[3].view(torch.int32), got[3].view(torch.int32))
    # -inf inside the window has probability 0: never drawn, and the statistics are those of the remaining columns
    q = z.clone()
    q[:, lo:hi:2] = float("-inf")
    for call in range(4):
        tok, _, lp, ent = _draw(ops, dev, q, vocab, window, 1.6, call=call)
        assert ((tok - lo) % 2 == 1).all(), "a -inf column was drawn"
    _check_stats(q, window, 1.6, tok, lp, ent, "window with -inf columns")
    # nothing finite in the window: lo / NaN
    q[:, lo:hi] = float("-inf")
    tok, _, lp, ent = _draw(ops, dev, q, vocab, window, 1.0)
    assert (tok == lo).all() and torch.isnan(lp).all() and torch.isnan(ent).all()


def test_purity(ops, dev):
    """A row's draw is a function of (seed, call, row key, its logits): alone, at another position, among 55 other rows."""
    vocab, window = 32000, (31744, 32000)
    g = torch.Generator().manual_seed(6)
    z = R.eighths(g, (56, 32064))
    keys = np.arange(56) * 13 + 5
    full = _draw(ops, dev, z, vocab, window, 1.0, keys=keys)
    for r in (0, 31, 55):
        alone = _draw(ops, dev, z[r:r + 1], vocab, window, 1.0, keys=keys[r:r + 1])
        moved_z = R.eighths(g, (7, 32064))
        moved_z[4] = z[r]
        moved = _draw(ops, dev, moved_z, vocab, window, 1.0, keys=np.array([1, 2, 3, 4, keys[r], 6, 7]))
        for other, i in ((alone, 0), (moved, 4)):
            assert other[0][i] == full[0][r]
            assert other[2].view(torch.int32)[i] == full[2].view(torch.int32)[r] and other[3].view(torch.int32)[i] == full[3].view(torch.int32)[r]
    # null row keys are the row indices
    a, b = _draw(ops, dev, z, vocab, window, 1.0), _draw(ops, dev, z, vocab, window, 1.0, keys=np.arange(56))
    assert np.array_equal(a[0], b[0])
    # another call, another key, another seed: another draw
    assert not np.array_equal(full[0], _draw(ops, dev, z, vocab, window, 1.0, keys=keys, call=CALL + 1)[0])
    assert not np.array_equal(full[0], _draw(ops, dev, z, vocab, window, 1.0, keys=keys + 1)[0])
    assert not np.array_equal(full[0], _draw(ops, dev, z, vocab, window, 1.0, keys=keys, seed=SEED + 1)[0])
    # without the entropy output the other three keep their bits
    c = _draw(ops, dev, z, vocab, window, 1.0, keys=keys, entropy=False)
    assert c[3] is None and np.array_equal(c[0], full[0]) and torch.equal(c[2].view(torch.int32), full[2].view(torch.int32))


def test_device_state_gives_the_bits_of_the_host_values(ops, dev):
    vocab, window = 1000, (3, 261)
    z = R.eighths(torch.Generator().manual_seed(7), (7, vocab))
    seed, call = 0xFEDC_BA98_7654_3210, 0x8000_0001
    host = _draw(ops, dev, z, vocab, window, 1.6, seed=seed, call=call)
    state = torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32, call], dtype=np.uint32).view(np.int32)).to(dev)
    devs = _draw(ops, dev, z, vocab, window, 1.6, seed=1, call=2, state_dev=state)      # the host values are overridden
    assert np.array_equal(host[0], devs[0]) and torch.equal(host[2].view(torch.int32), devs[2].view(torch.int32))
    assert not np.array_equal(host[0], _draw(ops, dev, z, vocab, window, 1.6, seed=1, call=2)[0])


def test_refusals_launch_nothing(ops, dev):
    _lib = importlib.import_module("openvla-oft_amd._lib")
    vocab = 1000
    z = R.eighths(torch.Generator().manual_seed(8), (7, vocab)).to(dev)

    def outputs():
        return dict(token=torch.full((7,), -77, dtype=torch.int32, device=dev), bins=torch.full((7,), -77, dtype=torch.int32, device=dev),
                    logprob=torch.full((7,), -77.0, device=dev), entropy_out=torch.full((7,), -77.0, device=dev))

    cases = (
        (dict(window=(5, 5)), "window"), (dict(window=(9, 5)), "window"), (dict(window=(-1, 5)), "window"), (dict(window=(0, vocab + 1)), "window"),
        (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(temperature=float("nan")), "temperature"),
        (dict(vocab=vocab + 8, window=(0, 8)), "ld="),
    )
    for kw, phrase in cases:
        out = outputs()
        args = dict(n_tokens=vocab, n_bins=N_BINS, vocab=vocab, window=(3, 261), temperature=1.0, seed=SEED, call=CALL)
        args.update(kw)
        with pytest.raises(_lib.OvlaError, match=phrase):
            ops.sample_tokens(z, **args, **out)
        torch.cuda.synchronize()
        for name, t in out.items():
            assert bool((t == -77).all()), f"{kw}: {name} was written"
    # a null pointer
    out = outputs()
    g = _lib.STRUCTS["ovla_sample_tokens_args"]()
    g.logits, g.ld, g.token, g.bin, g.logprob = z.data_ptr(), z.stride(0), out["token"].data_ptr(), out["bins"].data_ptr(), 0
    g.temperature, g.rows, g.vocab, g.lo, g.hi, g.n_tokens, g.n_bins = 1.0, 7, vocab, 0, vocab, vocab, N_BINS
    with pytest.raises(_lib.OvlaError, match="null pointer"):
        _lib.call("ovla_sample_tokens", g, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out["token"] == -77).all()) and bool((out["bins"] == -77).all())
