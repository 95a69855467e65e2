"""Host side of batched inference (no GPU): the fixed GEMM schedule query (ovla_gemm_fixed_schedule), its documentation, and the argument
checks of predict_action_batch / get_vla_action_batch."""
import importlib
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
load = importlib.import_module


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g

    g._pkg()
    return load("openvla-oft_amd.ops")


# OpenVLA-7B decoder, tower, projector and head classes (N, K, K2, k2_group_n, epilogue flags)
CLASSES = [(12288, 4096, 0, 0, 1 | 2), (4096, 4096, 0, 0, 16), (22016, 4096, 0, 0, 2 | 4), (4096, 11008, 0, 0, 16), (4096, 4096, 0, 0, 0),
           (32064, 4096, 0, 0, 0), (4352, 1024, 0, 0, 8), (1152, 4608, 0, 0, 8), (4096, 28672, 0, 0, 8), (4096, 4096, 0, 0, 8), (32, 4096, 0, 0, 0),
           (12288, 4096, 32, 4096, 1), (768, 256, 0, 0, 0)]


def test_fixed_schedule_is_a_function_of_the_problem_class_only(ops):
    lib = load("openvla-oft_amd._lib").lib()
    for c in CLASSES:
        tile, splits = ops.gemm_fixed_schedule(*c)
        assert tile in (1, 2, 5, 17, 18, 22) and 1 <= splits <= 8, c
        ops._fixed_cache.clear()
        assert ops.gemm_fixed_schedule(*c) == (tile, splits)
        # one schedule for every M: the workspace it needs grows with the tiles, nothing else changes
        ws = [ops.gemm_fixed_workspace_bytes(M, c[0], (tile, splits)) for M in (8, 608, 1216, 4864)]
        assert ws == sorted(ws) and (splits == 1) == (ws[-1] == 0)
    s = load("openvla-oft_amd._lib").STRUCTS["ovla_gemm_schedule"]()
    assert lib.ovla_gemm_fixed_schedule(4096, 4096, 0, 0, 4, None) != 0      # null output
    import ctypes

    assert lib.ovla_gemm_fixed_schedule(4096 + 8, 100 * 8, 0, 0, 4, ctypes.byref(s)) != 0   # SwiGLU needs N = 2F, F % 128 == 0: no configuration


def test_fold_and_swiglu_classes_take_configurations_that_run_them(ops):
    assert ops.gemm_fixed_schedule(22016, 4096, epi=ops.EPI_ROWSCALE | ops.EPI_SWIGLU)[0] == 22
    assert ops.gemm_fixed_schedule(12288, 4096, epi=ops.EPI_ROPE | ops.EPI_ROWSCALE)[0] in (1, 22)
    assert ops.gemm_fixed_schedule(4096, 11008, epi=ops.EPI_ROWSQ)[0] in (1, 22)
    assert ops.gemm_fixed_schedule(4352, 1024, epi=ops.EPI_GENERAL)[0] in (1, 2, 5, 17)


def test_schedule_struct_and_entry_points_are_documented():
    _lib = load("openvla-oft_amd._lib")
    assert [f for f, _ in _lib.STRUCT_FIELDS["ovla_gemm_schedule"]] == ["tile", "splits"]
    for fn in ("ovla_gemm_fixed_schedule", "ovla_gemm_fixed_workspace_bytes", "ovla_gemm_bf16_fixed"):
        assert fn in _lib.FUNCTIONS
    doc = (ROOT / "INTEGRATION.md").read_text()
    m = re.search(r"ovla_gemm_schedule\s*\{([^}]*)\}", doc)
    assert m and [f.strip() for f in re.findall(r"int32_t\s+(\w+)", m.group(1))] == ["tile", "splits"]
    for fn in ("ovla_gemm_fixed_schedule", "ovla_gemm_bf16_fixed", "OVLA_BATCH_INVARIANT"):
        assert fn in doc or fn in (ROOT / "README.md").read_text()


def _fake_vla(use_film=False):
    config = load("openvla-oft_amd.config")
    return types.SimpleNamespace(cfg=config.VLAConfig(), engine=types.SimpleNamespace(use_film=use_film))


def test_predict_action_batch_validates_its_arguments():
    modeling = load("openvla-oft_amd.modeling")
    f = modeling.OpenVLAForActionPrediction.predict_action_batch
    ids = torch.tensor([1, 5, 6])
    with pytest.raises(ValueError, match="pixel_values"):
        f(_fake_vla(), [(ids, None), (ids, None)], torch.zeros(3, 12, 8, 8))
    with pytest.raises(ValueError, match="no observations"):
        f(_fake_vla(), [], torch.zeros(0, 12, 8, 8))
    with pytest.raises(ValueError, match="use_film"):
        f(_fake_vla(use_film=True), [(ids, None)], torch.zeros(1, 12, 8, 8))
    with pytest.raises(ValueError, match="proprio"):
        f(_fake_vla(), [(ids, None), (ids, None)], torch.zeros(2, 12, 8, 8), proprio=np.zeros((3, 8)), proprio_projector=object())


def test_get_vla_action_batch_validates_its_arguments():
    utils = load("openvla-oft_amd.experiments.robot.openvla_utils")
    cfg = types.SimpleNamespace(num_images_in_input=1, use_proprio=False, center_crop=True, unnorm_key="x", num_open_loop_steps=8)
    with pytest.raises(ValueError, match="task labels"):
        utils.get_vla_action_batch(cfg, None, None, [{}, {}], ["a"])
    with pytest.raises(ValueError, match="no observations"):
        utils.get_vla_action_batch(cfg, None, None, [], [])
