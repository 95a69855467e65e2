"""sha256 digests of what the inference API returns, for comparing two commits bit for bit: predict_action, predict_action_batch (also with
pad_to and for a single observation) and predict_action_batch(policy=...) on the tiny oracle configuration (56 x 56 images, seeded weights),
with the L1 head + proprio, the discrete token path, the diffusion head (4 DDIM steps from given noise) and FiLM + L1 -- with graph replay off,
then on; with replay on every case runs twice, so that the capturing call and a pure replay are both hashed.  Only the public API is used, so
the same file runs against any commit that has it.  Prints one JSON object {case: sha256 over the raw bytes of the actions and of the action
hidden states}; two commits compute the same if every digest is equal.  Usage: python tools/infer_digest.py > digests.json"""
import hashlib
import importlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module
BF = torch.bfloat16
LENS = (7, 12, 9)
KEY = "d"
STATS = {KEY: {"action": {"q01": [-1.0] * 7, "q99": [1.0, 0.5, 2, 1, 1, 1, 1], "mask": [True] * 6 + [False]}}}


def _sub(sd, pre):
    return {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}


def digest(actions, hidden) -> str:
    a, h = np.ascontiguousarray(actions), hidden.detach().contiguous().view(torch.int16).cpu().numpy()   # bf16 bits as they are
    m = hashlib.sha256()
    for x in (a, h):
        m.update(f"{x.dtype}{x.shape}".encode())
        m.update(x.tobytes())
    return m.hexdigest()


def cases(dev):
    """-> [(name, model, zero-argument call returning (actions, hidden))]"""
    from oracle import vla_oracle as vo

    modeling, config_mod = load("openvla-oft_amd.modeling"), load("openvla-oft_amd.config")
    g = torch.Generator().manual_seed(5)
    prompts = [torch.cat([torch.tensor([1]), torch.randint(3, 31000, (n - 1,), generator=g)]) for n in LENS]
    pv = torch.randn(len(LENS), 12, 56, 56, generator=g).to(BF).float()
    proprio = (torch.rand(len(LENS), 8, generator=g) * 2 - 1).to(BF).float().numpy()
    noise = torch.randn(len(LENS), 8, 7, generator=g)
    pairs = [(p, None) for p in prompts]

    def weights(ocfg, seed, film=False):
        return {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=seed, film=film).items()}

    def model(ocfg, sd, film=False):
        return modeling.OpenVLAForActionPrediction(config_mod.VLAConfig.from_any(ocfg), sd, device=dev, norm_stats=STATS, use_film=film)

    def head_pp(cfg, sd):
        return (modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=_sub(sd, "action_head.")),
                modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=_sub(sd, "proprio_projector.")))

    out = []
    sd, fsd = weights(vo.tiny_config(), 0), weights(vo.tiny_config(), 4, film=True)
    vla, fvla = model(vo.tiny_config(), sd), model(vo.tiny_config(), fsd, film=True)
    cfg = vla.cfg
    (head, pp), (fhead, _) = head_pp(cfg, sd), head_pp(cfg, fsd)
    dhead = modeling.DiffusionActionHead(cfg.llm_dim, cfg.llm_dim, 7, num_diffusion_steps=4, device=dev, seed=11)
    nap = modeling.NoisyActionProjector(cfg.llm_dim, device=dev, seed=12)
    l1 = dict(proprio_projector=pp, action_head=head)
    ddim = dict(proprio_projector=pp, action_head=dhead, noisy_action_projector=nap)

    def one(m, i, **kw):
        ids = prompts[i][None]
        if "proprio_projector" in kw:
            kw["proprio"] = proprio[i]
        if "noisy_action_projector" in kw:
            kw["noise"] = noise[i: i + 1]
        return lambda: m.predict_action(input_ids=ids, unnorm_key=KEY, pixel_values=pv[i: i + 1].to(BF), attention_mask=torch.ones_like(ids, dtype=torch.bool), **kw)

    def batch(m, idx, pad_to=None, with_proprio=False, **kw):
        if with_proprio or "proprio_projector" in kw:
            kw["proprio"] = proprio[idx]
        if "noisy_action_projector" in kw:
            kw["noise"] = noise[idx]
        return lambda: m.predict_action_batch([pairs[i] for i in idx], pv[idx], unnorm_key=KEY, pad_to=pad_to, **kw)

    out += [("one/l1_proprio", vla, one(vla, 0, **l1)), ("one/discrete", vla, one(vla, 1)), ("one/diffusion", vla, one(vla, 2, **ddim)),
            ("one/film_l1", fvla, one(fvla, 0, action_head=fhead, use_film=True))]
    for tag, idx, pad_to in (("batch", [0, 1, 2], None), ("batch_pad4", [0, 1, 2], 4), ("batch_single", [1], None)):
        out += [(f"{tag}/l1_proprio", vla, batch(vla, idx, pad_to, **l1)), (f"{tag}/discrete", vla, batch(vla, idx, pad_to)),
                (f"{tag}/diffusion", vla, batch(vla, idx, pad_to, **ddim)),
                (f"{tag}/film_l1", fvla, batch(fvla, idx, pad_to, action_head=fhead, use_film=True))]
    # two policies on one base model (the slotted GEMM classes have fixed schedules from llm_dim 1024 up)
    ocfg = vo.tiny_config(llm_dim=1024, llm_ff=2048, llm_heads=8)
    names = ("x", "y")
    for heads in (True, False):
        pvla = model(ocfg, {k: v for k, v in weights(ocfg, 0).items() if ".lora_" not in k and not k.startswith(("action_head.", "proprio_projector."))})
        for seed, nm in enumerate(names, start=1):
            sd = weights(ocfg, seed)
            h, p = head_pp(pvla.cfg, sd)
            lora = {k: (v * 8.0 if ".lora_B." in k else v).to(BF).float() for k, v in sd.items() if ".lora_" in k}
            pvla.add_policy(nm, lora, action_head=h if heads else None, proprio_projector=p if heads else None)
        for assign in ([0, 1, 1], [1, 0, 0]):
            out.append((f"policies/{'l1' if heads else 'discrete'}/{''.join(map(str, assign))}", pvla,
                        batch(pvla, [0, 1, 2], policy=[names[s] for s in assign], with_proprio=heads)))
    return out


def main():
    dev = torch.device("cuda:0")
    todo, result = cases(dev), {}
    for name, m, call in todo:
        m.enable_graph_replay(False)
        result[f"{name}/eager"] = digest(*call())
    for name, m, call in todo:
        m.enable_graph_replay(True)
        for nth in ("graph_first", "graph_second"):
            result[f"{name}/{nth}"] = digest(*call())
    for _, m, _ in todo:
        m.enable_graph_replay(False)
    print(json.dumps(result, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
