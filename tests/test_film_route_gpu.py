"""ovla_film_vectors (csrc/film_route.hip) through ops.film_vectors: every FiLM Linear of a table, for every observation under its own slot's
weights, in one launch.  Exact integer data against int64, random data against float64 under a derived bound, bit-invariance of a row under
everything but its own inputs, isolation from NaN elsewhere, untouched guard regions, device-side clamping.

One launch holds Linears of every out_f of the grid (8, 24, 128, 144) and one of 5 columns (no multiple of the 4 columns a wave computes)."""
import importlib

import numpy as np
import pytest
import torch

load = importlib.import_module
BF = torch.bfloat16
OUT_FS = (8, 24, 128, 144, 5)
GUARD = 64                      # bf16 elements on either side of every buffer (128 bytes: the 16-byte alignment of W and avg survives)
SENTINEL, NAN = 0x4321, 0x7FC0  # bf16 bit patterns
DS = (256, 264, 1024)           # 264 / 8 = 33 vectors: no multiple of the 64 lanes; 1024: two full rounds of them
NS = (1, 2, 4)
N_OBS = (1, 5, 8, 19)           # 19 with most of them on one slot: more than one group of 8 observations


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class Guarded:
    """A bf16 device tensor of `shape` inside a sentinel-filled buffer; `intact()` says whether the guards still hold the sentinel."""

    def __init__(self, values: torch.Tensor, dev):
        flat = values.to(BF).contiguous().view(torch.int16).reshape(-1)
        buf = torch.full((flat.numel() + 2 * GUARD,), SENTINEL, dtype=torch.int16)
        buf[GUARD:GUARD + flat.numel()] = flat
        self.buf = buf.to(dev)
        self.t = self.buf[GUARD:GUARD + flat.numel()].view(BF).view(values.shape)

    def intact(self):
        b = self.buf.cpu().numpy().view(np.uint16)
        return bool((b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all())


class Problem:
    """W[j] [n, out_f, D], bias[j] [n, out_f] and avg [n_obs + 2, D] as float64 arrays of bf16-representable values; run(slots) launches once and
    returns the per-linear outputs [n_obs, out_f] as bf16 bit patterns after checking everything that must not have been written."""

    def __init__(self, ops, dev, D, n, n_obs, W, bias, avg, out_fs=OUT_FS):
        self.ops, self.dev, self.D, self.n, self.n_obs, self.out_fs = ops, dev, D, n, n_obs, out_fs
        self.W, self.bias, self.avg = W, bias, avg
        self.gW = [Guarded(torch.from_numpy(w), dev) for w in W]
        self.gb = [Guarded(torch.from_numpy(b), dev) for b in bias]
        self.gavg = Guarded(torch.from_numpy(avg), dev)
        self.rows = n_obs + 3
        self.gout = [Guarded(torch.zeros(self.rows, f), dev) for f in out_fs]
        self.tab = ops.film_table([(w.t, b.t, o.t) for w, b, o in zip(self.gW, self.gb, self.gout)], dev)

    def run(self, slots, host=True, device_slots=None):
        for o in self.gout:
            o.t.view(torch.int16).fill_(SENTINEL)
        w_before = [_bits(w.t) for w in self.gW]
        a_before = _bits(self.gavg.t)
        obs_slot = torch.tensor(slots if device_slots is None else device_slots, dtype=torch.int32, device=self.dev)
        self.ops.film_vectors(self.tab, self.gavg.t, obs_slot, host_slots=slots if host else None)
        torch.cuda.synchronize()
        outs = []
        for o, w, wb in zip(self.gout, self.gW, w_before):
            got = _bits(o.t)
            assert o.intact() and w.intact(), "guard region written"
            assert (got[self.n_obs:] == SENTINEL).all(), "rows >= n_obs written"
            assert np.array_equal(_bits(w.t), wb), "weights written"
            outs.append(got[:self.n_obs])
        assert self.gavg.intact() and np.array_equal(_bits(self.gavg.t), a_before), "avg written"
        assert all(b.intact() for b in self.gb)
        return outs

    def want64(self, slots):
        """float64 [n_obs, out_f] per linear, and the magnitude sum  sum_k |w x| + |bias|  of every output"""
        vals, mags = [], []
        for W, b in zip(self.W, self.bias):
            v = np.stack([b[s] + W[s] @ self.avg[i] for i, s in enumerate(slots)])
            m = np.stack([np.abs(b[s]) + np.abs(W[s]) @ np.abs(self.avg[i]) for i, s in enumerate(slots)])
            vals.append(v); mags.append(m)
        return vals, mags


def _bf16_values(a):
    """float64 array rounded to bf16-representable values (RNE, as the device tensors will hold them)"""
    return torch.from_numpy(a).to(torch.float32).to(BF).to(torch.float64).numpy()


def _integer_problem(ops, dev, D, n, n_obs, seed):
    rng = np.random.default_rng(seed)
    W = [rng.integers(-4, 5, (n, f, D)).astype(np.float64) for f in OUT_FS]
    bias = [rng.integers(-4, 5, (n, f)).astype(np.float64) for f in OUT_FS]
    avg = rng.integers(-4, 5, (n_obs + 2, D)).astype(np.float64)
    return Problem(ops, dev, D, n, n_obs, W, bias, avg)


def _random_problem(ops, dev, D, n, n_obs, seed, out_fs=OUT_FS):
    rng = np.random.default_rng(seed)
    W = [_bf16_values(rng.standard_normal((n, f, D)) / np.sqrt(D)) for f in out_fs]
    bias = [_bf16_values(rng.standard_normal((n, f))) for f in out_fs]
    avg = _bf16_values(rng.standard_normal((n_obs + 2, D)))
    return Problem(ops, dev, D, n, n_obs, W, bias, avg, out_fs)


def _assignments(n, n_obs, seed):
    rng = np.random.default_rng(seed)
    crowded = [n - 1] * n_obs          # every observation on the last slot: ceil(n_obs / 8) groups of one slot, the other slots unused
    if n_obs > 2:
        crowded[1] = 0
    return [[int(v) for v in rng.integers(0, n, n_obs)], crowded, [b % n for b in range(n_obs)]]


def _rne_bits(v64):
    return torch.from_numpy(np.ascontiguousarray(v64)).to(torch.float32).to(BF).view(torch.int16).numpy().view(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", N_OBS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_exact_integer_data(dev, ops, D, n, n_obs):
    """|w|, |x|, |bias| <= 4 and D <= 1024: every partial sum is an integer below 2^24, exact in fp32 in any order, so the output must EQUAL
    bf16_rne(the int64 result)."""
    p = _integer_problem(ops, dev, D, n, n_obs, seed=D + 10 * n + n_obs)
    for slots in _assignments(n, n_obs, seed=n_obs):
        got = p.run(slots)
        want, _ = p.want64(slots)
        for j, (g, w) in enumerate(zip(got, want)):
            assert np.abs(w).max() < 2 ** 24
            assert np.array_equal(g, _rne_bits(w)), f"linear {j} (out_f {OUT_FS[j]}), slots {slots}"


@pytest.mark.gpu
def test_exact_at_the_largest_batch(dev, ops):
    """n_obs = 64, the most one launch takes: every slot needs more than one group of observations."""
    p = _integer_problem(ops, dev, 264, 4, 64, seed=64)
    for slots in _assignments(4, 64, seed=64):
        got = p.run(slots)
        want, _ = p.want64(slots)
        for j, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, _rne_bits(w)), f"linear {j} (out_f {OUT_FS[j]})"


@pytest.mark.gpu
@pytest.mark.parametrize("n_obs", N_OBS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("D", DS)
def test_random_data_within_the_derived_bound(dev, ops, D, n, n_obs):
    """|got - want| <= 2^-8 |want| + D 2^-23 (sum_k |w_k x_k| + |bias|): one bf16 rounding (2^-9) and fp32 accumulation in any order
    (gamma_D ~ D 2^-24), each with a factor 2 of headroom."""
    p = _random_problem(ops, dev, D, n, n_obs, seed=7 * D + n + n_obs)
    slots = _assignments(n, n_obs, seed=n_obs + 1)[0]
    got = p.run(slots)
    want, mag = p.want64(slots)
    for j, (g, w, m) in enumerate(zip(got, want, mag)):
        g64 = torch.from_numpy(g.view(np.int16).copy()).view(BF).to(torch.float64).numpy()
        err, bound = np.abs(g64 - w), 2.0 ** -8 * np.abs(w) + D * 2.0 ** -23 * m
        assert (err <= bound).all(), f"linear {j}: worst error / bound {float((err / bound).max()):.3f}"


@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_rows_depend_on_their_own_inputs_only(dev, ops, D):
    """One observation (its avg row, its policy's weights) alone, among others, in reversed order, first and last of 19, with its weights in
    another slot, at n = 2 and n = 4: the same bits every time."""
    rng = np.random.default_rng(D)
    Wx = [_bf16_values(rng.standard_normal((f, D)) / np.sqrt(D)) for f in OUT_FS]
    bx = [_bf16_values(rng.standard_normal(f)) for f in OUT_FS]
    ax = _bf16_values(rng.standard_normal(D))

    def run(n, slot_x, n_obs, pos, seed):
        r = np.random.default_rng(seed)
        W = [_bf16_values(r.standard_normal((n, f, D)) / np.sqrt(D)) for f in OUT_FS]
        bias = [_bf16_values(r.standard_normal((n, f))) for f in OUT_FS]
        avg = _bf16_values(r.standard_normal((n_obs + 2, D)))
        for j in range(len(OUT_FS)):
            W[j][slot_x], bias[j][slot_x] = Wx[j], bx[j]
        avg[pos] = ax
        slots = [int(v) for v in r.integers(0, n, n_obs)]
        slots[pos] = slot_x
        p = Problem(ops, dev, D, n, n_obs, W, bias, avg)
        fwd = [o[pos] for o in p.run(slots)]
        # the same batch in reversed order
        p.gavg.t[:n_obs] = p.gavg.t[:n_obs].flip(0)
        rev = [o[n_obs - 1 - pos] for o in p.run(slots[::-1])]
        return fwd, rev

    base, _ = run(2, 0, 1, 0, seed=1)                                  # alone
    cases = {"among others": run(2, 0, 8, 3, seed=2), "first of 19": run(2, 0, 19, 0, seed=3), "last of 19": run(2, 0, 19, 18, seed=4),
             "other slot": run(2, 1, 8, 3, seed=5), "n = 4": run(4, 3, 8, 5, seed=6), "n = 4, 19": run(4, 2, 19, 11, seed=7)}
    for name, (fwd, rev) in cases.items():
        for j in range(len(OUT_FS)):
            assert np.array_equal(fwd[j], base[j]), f"{name}: linear {j} differs from the observation alone"
            assert np.array_equal(rev[j], base[j]), f"{name}, reversed: linear {j} differs from the observation alone"


@pytest.mark.gpu
@pytest.mark.parametrize("D", DS)
def test_nan_elsewhere_changes_nothing(dev, ops, D):
    """NaN in every unused slot's weights and biases, in another observation's avg row, in another used slot's weights, and in avg columns
    past D: the rows that do not own them keep their bits."""
    n, n_obs = 4, 11
    slots = [0, 2, 0, 0, 2, 0, 0, 0, 0, 2, 0]          # slots 1 and 3 unused; slot 0 needs two groups
    clean = _random_problem(ops, dev, D, n, n_obs, seed=D + 1)
    want = clean.run(slots)
    nan = float("nan")

    def poisoned(what):
        W, bias, avg = [w.copy() for w in clean.W], [b.copy() for b in clean.bias], clean.avg.copy()
        if what == "unused slots":
            for j in range(len(OUT_FS)):
                W[j][1], W[j][3], bias[j][1], bias[j][3] = nan, nan, nan, nan
        elif what == "another observation":
            avg[4] = nan
            avg[n_obs:] = nan                               # rows the launch does not cover
        elif what == "another used slot":
            for j in range(len(OUT_FS)):
                W[j][2], bias[j][2] = nan, nan
        return Problem(ops, dev, D, n, n_obs, W, bias, avg)

    got = poisoned("unused slots").run(slots)
    for j in range(len(OUT_FS)):
        assert np.array_equal(got[j], want[j]), "an unused slot's weights were read"
    got = poisoned("another observation").run(slots)
    for j in range(len(OUT_FS)):
        keep = [b for b in range(n_obs) if b != 4]
        assert np.array_equal(got[j][keep], want[j][keep]) and (got[j][4] & 0x7FFF > 0x7F80).all()
    got = poisoned("another used slot").run(slots)
    for j in range(len(OUT_FS)):
        own = [b for b in range(n_obs) if slots[b] == 0]
        assert np.array_equal(got[j][own], want[j][own])
    # avg with a row stride above D: the pad columns hold NaN and are never read
    wide = torch.full((n_obs + 2, D + 8), nan, dtype=BF, device=dev)
    wide[:, :D] = clean.gavg.t
    for o in clean.gout:
        o.t.view(torch.int16).fill_(SENTINEL)
    ops.film_vectors(clean.tab, wide[:, :D], torch.tensor(slots, dtype=torch.int32, device=dev), host_slots=slots)
    torch.cuda.synchronize()
    for j, o in enumerate(clean.gout):
        assert np.array_equal(_bits(o.t)[:n_obs], want[j]) and (_bits(o.t)[n_obs:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_device_slots_are_clamped(dev, ops, n):
    """obs_slot on the device holding -3 or n + 5 (no host copy): the result of slot 0 / slot n - 1; with the host copy: refused, nothing launched."""
    _lib = load("openvla-oft_amd._lib")
    D, n_obs = 264, 5
    p = _random_problem(ops, dev, D, n, n_obs, seed=n)
    bad = [-3, n + 5, 0, n - 1, -1]
    clamped = [min(max(v, 0), n - 1) for v in bad]
    want = p.run(clamped)
    got = p.run(clamped, host=False, device_slots=bad)
    for j in range(len(OUT_FS)):
        assert np.array_equal(got[j], want[j])
    for o in p.gout:
        o.t.view(torch.int16).fill_(SENTINEL)
    with pytest.raises(_lib.OvlaError, match="obs_slot"):
        ops.film_vectors(p.tab, p.gavg.t, torch.tensor(bad, dtype=torch.int32, device=dev), host_slots=bad)
    torch.cuda.synchronize()
    assert all((_bits(o.t) == SENTINEL).all() for o in p.gout), "nothing was launched"
