"""The sampling contract's numpy restatement (tests/token_sample_reference.py) checked on the host: it draws the distribution it claims, each
planted mutant is rejected by the check meant to catch it, and the general input set of tests/test_token_sample_gpu.py leaves at most 1 % of
its rows inside the near-tie margin.  No GPU."""
import math

import numpy as np
import pytest
import torch

from tests import token_sample_reference as R

BF = torch.bfloat16
SEED, CALL = 0x1234_5678_9ABC_DEF0, 17
N_DRAWS = 20000
WINDOW = (3, 11)            # 8 window tokens, off a multiple of 4: absolute and window-relative ids take different generator words
LOGITS8 = (-1.0, 0.5, 2.0, -0.25, 1.125, 0.0, -3.0, 1.75)
SHAPES = ((1000, 1000), (32000, 32064))


def windows(vocab):
    return ((vocab - 256, vocab), (0, vocab), (3, 261))


def _row8():
    z = torch.full((1, 16), 50.0, dtype=BF)      # everything outside the window is far larger: it must not matter
    z[0, WINDOW[0]:WINDOW[1]] = torch.tensor(LOGITS8, dtype=BF)
    return z


# ---- the checks (each takes the restatement's mutation switches) ------------------------------------------------------------------------------
def check_distribution(T, **mut):
    """20 000 row keys on one row of 8 window tokens: every count within 6 binomial standard deviations of N p_j."""
    z = _row8().expand(N_DRAWS, -1)
    r = R.sample_ref(z, *WINDOW, T, seed=SEED, call=CALL, row_keys=np.arange(N_DRAWS), **mut)
    s = R.scaled(z[:1, WINDOW[0]:WINDOW[1]], T).astype(np.float64)[0]
    p = np.exp(s - s.max())
    p /= p.sum()
    counts = np.bincount(r["token"] - WINDOW[0], minlength=8)
    assert counts.sum() == N_DRAWS and r["token"].min() >= WINDOW[0] and r["token"].max() < WINDOW[1]
    for j in range(8):
        sd = math.sqrt(N_DRAWS * p[j] * (1.0 - p[j]))
        assert abs(counts[j] - N_DRAWS * p[j]) <= 6.0 * sd, f"T={T} token {j}: {counts[j]} draws, expected {N_DRAWS * p[j]:.1f} +- {sd:.1f}"


def check_window_independence(**mut):
    """A token id's variate belongs to the id, not to its place in the window: widening the window by columns of probability 0 changes no draw."""
    z = torch.full((200, 16), float("-inf"), dtype=BF)
    z[:, WINDOW[0]:WINDOW[1]] = torch.tensor(LOGITS8, dtype=BF)
    narrow = R.sample_ref(z, *WINDOW, 1.0, seed=SEED, call=CALL, **mut)
    wide = R.sample_ref(z, 0, 16, 1.0, seed=SEED, call=CALL, **mut)
    assert np.array_equal(narrow["token"], wide["token"]), "the draw depends on where the window starts"


def check_uniform_range(shift=9):
    """u = (2 k + 1) 2^-24 lies strictly inside (0, 1), so both logarithms are finite and g stays in the contract's range."""
    w = R.words(np.arange(64), 0, 1024, seed=SEED, call=CALL)
    k = R.uniform_int(w, shift)
    assert int(k.max()) < 2 ** 23, "the uniform's integer has more than 23 bits: u reaches past 1"
    with np.errstate(invalid="ignore", divide="ignore"):
        g = R.gumbel64(w, shift)
    assert np.isfinite(g).all() and g.min() >= R.GUMBEL_MIN and g.max() <= R.GUMBEL_MAX
    # the extreme words give the extreme variates the contract states
    ends = R.gumbel64(np.array([0, 0xFFFFFFFF], dtype=np.uint64))
    assert abs(ends[0] - R.GUMBEL_MIN) < 1e-3 and abs(ends[1] - R.GUMBEL_MAX) < 1e-3


def check_first_maximum(**mut):
    """Equal keys: the lowest index.  A window of -inf has only equal keys."""
    z = torch.full((4, 16), float("-inf"), dtype=BF)
    r = R.sample_ref(z, *WINDOW, 1.0, seed=SEED, call=CALL, **mut)
    assert (r["token"] == WINDOW[0]).all(), "equal keys: not the lowest index"


def _pg_inputs():
    g = torch.Generator().manual_seed(5)
    z = R.eighths(g, (6, 40))
    tokens = np.array([3, 5, 10, 7, 4, 9], dtype=np.int32)
    return z, tokens


def check_gradient_sums_to_zero(**mut):
    """sum_j (p_j - onehot_j) = 0: the gradient of a log-probability has no component along the constant vector, and the drawn token's own
    element is negative for a positive advantage."""
    z, tokens = _pg_inputs()
    r = R.pg_ref(z, 40, *WINDOW, 1.6, tokens, np.ones(6), grad_scale=0.5, **mut)
    g = r["grad64"]
    assert float(g.sum(-1).abs().max()) < 1e-12, "the gradient rows do not sum to zero"
    assert (g[torch.arange(6), torch.as_tensor(tokens, dtype=torch.long)] < 0).all()
    assert float(g[:, :WINDOW[0]].abs().max()) == 0.0 and float(g[:, WINDOW[1]:].abs().max()) == 0.0


def check_gate_truth_table(**mut):
    """PPO's clipped surrogate min(r A, clip(r) A) is flat in r only where r has ALREADY moved the way the advantage pushes it."""
    adv = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0, 0.0])
    ratio = np.array([0.5, 1.0, 1.5, 0.5, 1.0, 1.5, 1.5])
    gate, gated = R.gate_ref(adv, ratio, 0.8, 1.2, **mut)
    assert gated.tolist() == [False, False, True, True, False, False, True], gated.tolist()
    assert gate.tolist() == [0.5, 1.0, 0.0, 0.0, 1.0, 1.5, 0.0]


# ---- the restatement passes its checks -------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    from tests.lora_dropout_reference import KNOWN_ANSWERS, philox4x32_10
    for ctr, key, want in KNOWN_ANSWERS:
        assert tuple(int(v) for v in philox4x32_10(*ctr, *key)) == want


@pytest.mark.parametrize("T", R.GENERAL_T)
def test_contract_draws_the_softmax(T):
    check_distribution(T)


def test_contract_properties():
    check_window_independence()
    check_uniform_range()
    check_first_maximum()
    check_gradient_sums_to_zero()
    check_gate_truth_table()


def test_flat_rows_are_an_integer_argmax():
    """On equal logits the float64 keys and the integer reference agree (wherever the two largest integers differ)."""
    z = torch.zeros((56, 300), dtype=BF)
    tok, k = R.flat_token_ref(np.arange(56), 3, 261, seed=SEED, call=CALL)
    r = R.sample_ref(z, 3, 261, 1.0, seed=SEED, call=CALL)
    assert np.array_equal(tok, r["token"])
    assert len(set(tok.tolist())) > 40          # the rows do not share a draw


def test_stats_reference_against_direct_formulas():
    z, tokens = _pg_inputs()
    for T in R.GENERAL_T:
        st = R.row_stats_ref(z, *WINDOW, T, tokens)
        s = torch.from_numpy(R.scaled(z[:, WINDOW[0]:WINDOW[1]], T)).double()
        logp = torch.log_softmax(s, -1)
        want = logp[torch.arange(6), torch.as_tensor(tokens, dtype=torch.long) - WINDOW[0]]
        assert float((st["logprob"] - want).abs().max()) < 1e-12
        assert float((st["entropy"] - (-(logp.exp() * logp).sum(-1))).abs().max()) < 1e-12
        assert float(st["logprob_bound"].max()) < 1e-5 and float(st["entropy_bound"].max()) < 1e-4


# ---- planted mutants ------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "window-relative token id": (check_window_independence, dict(relative=True), "depends on where the window starts"),
    "w >> 8": (check_uniform_range, dict(shift=8), "more than 23 bits"),
    "last maximum": (check_first_maximum, dict(last_max=True), "not the lowest index"),
    "gradient without the - 1": (check_gradient_sums_to_zero, dict(minus_one=False), "do not sum to zero"),
    "gate ignores the advantage's sign": (check_gate_truth_table, dict(ignore_sign=True), "True"),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_planted_mutant_is_rejected(name):
    check, mut, phrase = MUTANTS[name]
    with pytest.raises(AssertionError) as exc:
        check(**mut)
    assert phrase in str(exc.value), f"{name}: rejected, but not by the check meant to catch it: {exc.value}"


def test_relative_mutant_also_fails_nothing_else():
    """The window-relative mutant still draws a valid distribution (it only moves the variates): the independence check is the one that sees it."""
    check_distribution(1.0, relative=True)


# ---- the near-tie condition on the general input set --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab,ld", SHAPES)
def test_general_inputs_leave_at_most_one_percent_undecided(vocab, ld):
    for lo, hi in windows(vocab):
        z, keys = R.general_rows(vocab, ld, lo, hi)
        for T in R.GENERAL_T:
            r = R.general_ref(z, keys, lo, hi, T, seed=SEED, call=CALL)
            assert r["token"].shape == (R.GENERAL_ROWS * R.GENERAL_KEYS,)
            assert float(np.abs(r["key1"]).max()) < 32.0 and float(r["e"].max()) < 2e-5
            undecided = 1.0 - r["decided"].mean()
            assert undecided <= 0.01, f"vocab {vocab} window [{lo}, {hi}) T={T}: {100 * undecided:.2f} % of the rows inside the near-tie margin"
