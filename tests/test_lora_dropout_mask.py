"""The LoRA-dropout mask contract (include/ovla.h "LoRA dropout") on the CPU: the numpy Philox4x32-10 of tests/lora_dropout_reference.py
against the generator's known answers, the statistics of the masks it defines, and the per-rank seeds of finetune()."""
import importlib
import itertools
import math

import numpy as np
import pytest

import lora_dropout_reference as R

SEED, M, K = 7, 256, 512
PS = (0.05, 0.25, 0.5)
STREAMS = [(module, call) for module in range(3) for call in range(2)]   # six masks per p


def test_philox_known_answers():
    for ctr, key, want in R.KNOWN_ANSWERS:
        got = tuple(int(w) for w in R.philox4x32_10(*ctr, *key))
        assert got == want, f"counter {ctr} key {key}: got {[hex(w) for w in got]} want {[hex(w) for w in want]}"
    # vectorised evaluation = element-wise evaluation
    ctrs = np.array([c for c, _, _ in R.KNOWN_ANSWERS[:1]] * 3, dtype=np.uint64).T
    out = R.philox4x32_10(*ctrs, 0, 0)
    assert all(int(out[w][i]) == R.KNOWN_ANSWERS[0][2][w] for w in range(4) for i in range(3))


def test_threshold_and_scale():
    assert R.threshold(0.5) == 32768 and R.threshold(0.75) == 49152 and R.threshold(0.0) == 0
    assert R.threshold(0.05) == 3276 and R.threshold(0.1) == 6553
    assert float(R.inv_scale(0.5)) == 2.0 and float(R.inv_scale(0.75)) == 4.0 and float(R.inv_scale(0.0)) == 1.0
    assert R.keep_mask(4, 16, module=3, call=9, seed=SEED, p=0.0).all(), "p = 0 keeps everything"


@pytest.fixture(scope="module")
def drops():
    """{p: [bool [M, K] drop masks of the six (module, call) streams]}"""
    return {p: [~R.keep_mask(M, K, module=mod, call=call, seed=SEED, p=p) for mod, call in STREAMS] for p in PS}


@pytest.mark.parametrize("p", PS)
def test_mask_statistics(drops, p):
    """Binomial bounds: the drop probability is exactly q = thr / 65536.  Total count within 3 sigma, every row and every column within
    5 sigma (768 counts per mask: the chance of one beyond 5 sigma is 4e-4), the joint-drop count of any two of the six masks within
    4 sigma of independence (probability q^2)."""
    q = R.threshold(p) / 65536.0
    worst = dict(total=0.0, row=0.0, col=0.0, joint=0.0)
    for d in drops[p]:
        sd = math.sqrt(M * K * q * (1 - q))
        worst["total"] = max(worst["total"], abs(d.sum() - q * M * K) / sd)
        worst["row"] = max(worst["row"], float(np.abs(d.sum(1) - q * K).max()) / math.sqrt(K * q * (1 - q)))
        worst["col"] = max(worst["col"], float(np.abs(d.sum(0) - q * M).max()) / math.sqrt(M * q * (1 - q)))
    for a, b in itertools.combinations(range(len(STREAMS)), 2):
        assert not np.array_equal(drops[p][a], drops[p][b]), f"streams {STREAMS[a]} and {STREAMS[b]} share a mask"
        q2 = q * q
        worst["joint"] = max(worst["joint"], abs((drops[p][a] & drops[p][b]).sum() - q2 * M * K) / math.sqrt(M * K * q2 * (1 - q2)))
    print(f"p = {p}: worst deviations in sigma: {worst}")
    assert worst["total"] <= 3.0 and worst["row"] <= 5.0 and worst["col"] <= 5.0 and worst["joint"] <= 4.0, worst


def test_mask_is_independent_of_everything_but_its_key():
    """Rows are indexed by q = m * (K / 8) + (k >> 3): the first rows of a taller matrix are the same mask; another seed word, module or call
    is another mask."""
    base = R.keep_mask(8, 64, module=1, call=2, seed=SEED, p=0.25)
    assert np.array_equal(R.keep_mask(16, 64, module=1, call=2, seed=SEED, p=0.25)[:8], base)
    for other in (dict(module=2, call=2, seed=SEED), dict(module=1, call=3, seed=SEED), dict(module=1, call=2, seed=SEED + 1),
                  dict(module=1, call=2, seed=SEED + (1 << 32))):
        assert not np.array_equal(R.keep_mask(8, 64, p=0.25, **other), base), other


def test_dropout_bits_round_to_nearest_even():
    x = np.array([0x3F80, 0x3F81, 0xBF83, 0x0000, 0x7F7F], dtype=np.uint16)           # 1, 1 + 2^-7, -(1 + 3 * 2^-7), 0, max
    keep = np.array([True, True, True, True, False])
    got = R.dropout_bits(x, keep, 0.5)
    assert got.tolist() == [0x4000, 0x4001, 0xC003, 0x0000, 0x0000]
    inv = float(R.inv_scale(0.1))
    y = R.bf16_bits_to_f32(R.dropout_bits(np.array([0x3F80], dtype=np.uint16), np.array([True]), 0.1))
    assert abs(float(y[0]) - inv) <= 2.0 ** -8 * inv


def test_finetune_seeds_differ_per_rank():
    ft = importlib.import_module("openvla-oft_amd.vla_scripts.finetune")
    s0, s1 = ft.dropout_seed_for_rank(0), ft.dropout_seed_for_rank(1)
    assert s0 == 7 and s1 == 7 + (1 << 32)
    assert R.seed_words(s0) != R.seed_words(s1)
    a = R.keep_mask(8, 64, module=0, call=1, seed=s0, p=0.25)
    assert not np.array_equal(a, R.keep_mask(8, 64, module=0, call=1, seed=s1, p=0.25))


def test_abi_declares_the_three_entry_points():
    import ctypes

    lib = importlib.import_module("openvla-oft_amd._lib")
    for name in ("apply", "proj", "backproj"):
        assert lib.FUNCTIONS[f"ovla_lora_dropout_{name}"] == ("int", [("struct", f"ovla_lora_dropout_{name}_args"), ("plain", "void*")])
        fields = dict(lib.STRUCT_FIELDS[f"ovla_lora_dropout_{name}_args"])
        assert fields["module"] is ctypes.c_uint32 * 4 and fields["seed_lo"] is ctypes.c_uint32 and fields["p"] is ctypes.c_float


def test_adapter_config_records_lora_dropout(tmp_path):
    import json

    import torch

    w = importlib.import_module("openvla-oft_amd.weights")
    t = {"m.q_proj.lora_A.weight": torch.zeros(4, 8), "m.q_proj.lora_B.weight": torch.zeros(8, 4)}
    d = w.save_lora_adapter(tmp_path / "a", t, r=4, lora_alpha=2, lora_dropout=0.05)
    assert json.loads((d / "adapter_config.json").read_text())["lora_dropout"] == 0.05
    assert json.loads((w.save_lora_adapter(tmp_path / "b", t, r=4, lora_alpha=2) / "adapter_config.json").read_text())["lora_dropout"] == 0.0
    tensors, cfg = w.load_lora_adapter(d)        # the reader takes any value: it only matters to a run that trains on
    assert cfg["lora_dropout"] == 0.05 and set(tensors) == set(t)
