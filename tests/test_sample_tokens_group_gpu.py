"""ovla_sample_tokens_group: draw (r, g) is ovla_sample_tokens' draw of row r under row key row_key[r, g], bit for bit, whatever the row count, the
key source, the load path or the source of the generator's state; ovla_token_pg_group reports the same log-probabilities."""
import pytest
import torch

from tests import token_sample_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SHAPES = ((1000, 1008), (32000, 32064))
ROWS = 8


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: bits differ"


def windows(vocab):
    return ((vocab - 256, vocab), (0, vocab), (3, 261))


def _single(ops, z, keys, **kw):
    """G launches of ovla_sample_tokens on the same rows, launch g under keys[:, g] -> token, bin, logprob [rows, G], entropy [rows]."""
    cols = [ops.sample_tokens(z, row_key=keys[:, g].contiguous(), **kw) for g in range(keys.shape[1])]
    return tuple(torch.stack([c[i] for c in cols], 1) for i in range(3)) + (cols[0][3],)


@pytest.mark.parametrize("vocab,ld,G", [(v, l, G) for v, l in SHAPES for G in (1, 2, 3, 8)] + [(1000, 1008, 64)])     # (the cap on the small shape)
def test_group_draws_are_the_single_draws(ops, dev, vocab, ld, G):
    z = R.eighths(torch.Generator().manual_seed(70 + G), (ROWS, ld)).to(dev)
    zu = torch.empty(ROWS * ld + 1, dtype=BF, device=dev)[1:].view(ROWS, ld)      # 2 bytes off a 16-byte boundary: the column-by-column path
    zu.copy_(z)
    explicit = (torch.arange(ROWS * G, dtype=torch.int32).view(ROWS, G) * 7919 + 11).to(dev)
    default = torch.arange(ROWS * G, dtype=torch.int32, device=dev).view(ROWS, G)
    for wi, window in enumerate(windows(vocab)):
        T = R.GENERAL_T[wi]
        kw = dict(n_tokens=vocab, n_bins=255, vocab=vocab, window=window, temperature=T, seed=9 + (5 << 32), call=3)
        for logits, path in ((z, "aligned"), (zu, "unaligned")):
            want = _single(ops, logits, explicit, **kw)
            got = ops.sample_tokens_group(logits, G, row_key=explicit, **kw)
            for name, a, b in zip(("token", "bin", "logprob", "entropy"), got, want):
                same(a, b, f"vocab {vocab} G={G} window {window} {path} explicit keys: {name}")
            got = ops.sample_tokens_group(logits, G, **kw)
            want = _single(ops, logits, default, **kw)
            for name, a, b in zip(("token", "bin", "logprob", "entropy"), got, want):
                same(a, b, f"vocab {vocab} G={G} window {window} {path} default keys r * G + g: {name}")
        if G > 1:
            tok = got[0]
            assert int((tok[:, 1:] != tok[:, :1]).sum()) > 0, "every draw of every row is the same token: the keys do not reach the generator"
        tok, _, lp, none = ops.sample_tokens_group(z, G, row_key=explicit, entropy=False, **kw)
        assert none is None
        same(tok, ops.sample_tokens_group(z, G, row_key=explicit, **kw)[0], "without the entropy output: token")


def test_a_rows_draws_do_not_depend_on_the_row_count(ops, dev):
    vocab, ld, G = 1000, 1008, 3
    z = R.eighths(torch.Generator().manual_seed(71), (ROWS, ld)).to(dev)
    keys = (torch.arange(ROWS * G, dtype=torch.int32).view(ROWS, G) * 31 + 5).to(dev)
    kw = dict(n_tokens=vocab, n_bins=255, vocab=vocab, window=(3, 261), temperature=1.6, seed=4, call=8)
    full = ops.sample_tokens_group(z, G, row_key=keys, **kw)
    for r0, r1 in ((0, 1), (5, 8), (2, 5)):
        part = ops.sample_tokens_group(z[r0:r1], G, row_key=keys[r0:r1].contiguous(), **kw)
        for name, a, b in zip(("token", "bin", "logprob", "entropy"), part, full):
            same(a, b[r0:r1], f"rows [{r0}, {r1}) alone: {name}")


def test_state_dev_override(ops, dev):
    vocab, ld, G = 1000, 1008, 4
    z = R.eighths(torch.Generator().manual_seed(72), (ROWS, ld)).to(dev)
    kw = dict(n_tokens=vocab, n_bins=255, vocab=vocab, window=(vocab - 256, vocab), temperature=1.0)
    seed, call = 0x1234567 + (0x89 << 32), 41
    want = ops.sample_tokens_group(z, G, seed=seed, call=call, **kw)
    state = torch.tensor([seed & 0xFFFFFFFF, seed >> 32, call], dtype=torch.int32, device=dev)
    got = ops.sample_tokens_group(z, G, seed=1, call=2, state_dev=state, **kw)
    for name, a, b in zip(("token", "bin", "logprob", "entropy"), got, want):
        same(a, b, f"state_dev: {name}")
    other = ops.sample_tokens_group(z, G, seed=1, call=2, **kw)
    assert not torch.equal(other[0], want[0]), "the host seed / call drew the same tokens: the override is not what decided"


@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_token_pg_group_reports_the_samplers_logprob(ops, dev, vocab, ld):
    G = 8
    z = R.eighths(torch.Generator().manual_seed(73), (ROWS, ld)).to(dev)
    one = torch.ones((ROWS, G), device=dev)
    for wi, window in enumerate(windows(vocab)):
        T = R.GENERAL_T[wi]
        tok, _, lp, ent = ops.sample_tokens_group(z, G, n_tokens=vocab, n_bins=255, vocab=vocab, window=window, temperature=T, seed=2, call=1)
        lp2, _, _, _, ent2, none = ops.token_pg_group(z, tok, one, vocab=vocab, window=window, temperature=T)
        assert none is None
        same(lp2, lp, f"window {window} T={T} logprob"), same(ent2, ent, f"window {window} T={T} entropy")


def test_refusals(ops, dev):
    import importlib

    _lib = importlib.import_module("openvla-oft_amd._lib")
    vocab = 1000
    z = R.eighths(torch.Generator().manual_seed(74), (ROWS, vocab)).to(dev)
    for G, kw, phrase in ((0, {}, "G = 0"), (65, {}, "G = 65"), (2, dict(window=(5, 5)), "window"), (2, dict(temperature=0.0), "temperature")):
        n = max(G, 1)
        out = dict(token=torch.full((ROWS, n), -77, dtype=torch.int32, device=dev), bins=torch.full((ROWS, n), -77, dtype=torch.int32, device=dev),
                   logprob=torch.full((ROWS, n), -77.0, device=dev), entropy_out=torch.full((ROWS,), -77.0, device=dev))
        args = dict(n_tokens=vocab, n_bins=255, vocab=vocab, window=(3, 261))
        args.update(kw)
        if G == 0:          # the wrapper's own shape check would stop G = 0: through the struct
            g = _lib.STRUCTS["ovla_sample_tokens_group_args"]()
            g.logits, g.ld, g.token, g.bin, g.logprob = z.data_ptr(), z.stride(0), out["token"].data_ptr(), out["bins"].data_ptr(), out["logprob"].data_ptr()
            g.temperature, g.rows, g.vocab, g.lo, g.hi, g.n_tokens, g.n_bins, g.G = 1.0, ROWS, vocab, 0, vocab, vocab, 255, 0
            with pytest.raises(_lib.OvlaError, match=phrase):
                _lib.call("ovla_sample_tokens_group", g, torch.cuda.current_stream().cuda_stream)
        else:
            with pytest.raises(_lib.OvlaError, match=phrase):
                ops.sample_tokens_group(z, G, **args, **out)
        torch.cuda.synchronize()
        for name, t in out.items():
            assert bool((t == -77).all()), f"G={G} {kw}: {name} was written"
