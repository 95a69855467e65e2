"""Batched inference at OpenVLA-7B size on the deployed path: LoRA merged, RMSNorm folded into the decoder's projections, L1 head.  B = 8
observations with mixed prompt lengths give every observation the same bits as a batch of 3 of them, and the actions stay within the absolute bounds
tests/test_fullsize_e2e_gpu.py holds the B = 8 path to (on the same trained-like conditioning)."""
import gc
import importlib

import numpy as np
import pytest
import torch

from tests import stage_harness as sh

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
LENS = [11, 17, 9, 14, 20, 8, 13, 16]
# tests/test_fullsize_e2e_gpu.py ABS: actions within 0.10 of fp32 (the conditioned head keeps fp32 inside [-1, 1]) and within 0.17 of another
# bf16 evaluation of the path
PRED_LINF_FP32, PRED_LINF_EAGER = 0.10, 0.17


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


@pytest.fixture(scope="module")
def full(dev):
    load = importlib.import_module
    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    cfg = config_mod.OPENVLA_7B
    sd = sh.conditioned_state_dict(cfg, dev, seed=1, branch_gain=0.25, head_gain=0.125)
    stats = {"d": {"action": {"q01": [-1.0] * cfg.action_dim, "q99": [1.0] * cfg.action_dim}}}
    vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev, norm_stats=stats).merge_and_unload()
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, cfg.action_dim, device=dev, state_dict=_sub(sd, "action_head."))
    pp = modeling.ProprioProjector(cfg.llm_dim, cfg.proprio_dim, device=dev, state_dict=_sub(sd, "proprio_projector."))
    del sd
    g = torch.Generator().manual_seed(21)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    pv = torch.randn(len(LENS), 6 * cfg.num_images, 224, 224, generator=g).to(BF)
    proprio = (torch.rand(len(LENS), cfg.proprio_dim, generator=g) * 2 - 1).to(BF).float().numpy()
    yield dict(cfg=cfg, vla=vla, head=head, pp=pp, prompts=prompts, pv=pv, proprio=proprio)
    del vla, head, pp
    gc.collect()
    torch.cuda.empty_cache()


def test_full_size_batch_of_8_equals_batch_of_3(full):
    vla, head, pp = full["vla"], full["head"], full["pp"]
    llm = vla.engine.llm
    assert getattr(llm, "folded", False) and llm._fold_fixed_ok(), "the merged decoder runs folded"

    def run(idx):
        a, h = vla.predict_action_batch([(full["prompts"][i], None) for i in idx], full["pv"][idx], unnorm_key="d", proprio=full["proprio"][idx],
                                        proprio_projector=pp, action_head=head)
        return a, h

    a8, h8 = run(list(range(len(LENS))))
    sub = [5, 0, 3]
    a3, h3 = run(sub)
    for k, i in enumerate(sub):
        assert np.array_equal(a8[i], a3[k]) and torch.equal(h8[i], h3[k]), f"sample {i}: batch of 8 vs batch of 3"
    worst = 0.0
    for i in range(len(LENS)):
        one, _ = vla.predict_action(input_ids=full["prompts"][i][None], attention_mask=torch.ones(1, LENS[i], dtype=torch.bool),
                                    pixel_values=full["pv"][i: i + 1], unnorm_key="d", proprio=full["proprio"][i], proprio_projector=pp, action_head=head)
        worst = max(worst, float(np.abs(a8[i] - one).max()))
    print(f"B = 8 batched actions: max |a| {np.abs(a8).max():.3f}; Linf vs predict_action (batch 1, planner schedules) {worst:.3e}")
    assert np.isfinite(a8).all() and np.abs(a8).max() <= 1.0 + PRED_LINF_FP32
    assert worst <= PRED_LINF_EAGER
