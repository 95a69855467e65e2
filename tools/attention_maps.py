"""Which camera, which patches and which prompt tokens the action rows look at: one observation -> an .npz of ActionAttention.token_mass() and
patch_maps(), and (with Pillow) one PNG heat map per image, averaged over the action rows and a range of decoder layers.

The observation is synthetic (random frames and state) or frame `--step` of episode `--episode` of an episode store (`--episodes ROOT`, the
layout of prismatic/vla/datasets/rlds_free.py; tools/make_synthetic_episodes.py writes one).  The model is a local checkpoint directory
(`--checkpoint`, with its L1 head and proprio projector when `--l1` / `--proprio`; it needs the tokenizer files) or, without one,
random weights of `--size` (tiny | 7b) -- maps of random weights mean nothing, they exercise the path.

  python tools/attention_maps.py --size tiny --out maps.npz
  python tools/attention_maps.py --checkpoint runs/ckpt --l1 --proprio --episodes datasets/rlds --episode 3 --step 20 --layers 24:32 --out maps.npz"""
import argparse
import importlib
import sys
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module
DATASET = "libero_spatial_no_noops"


def observation(args, side: int):
    if args.episodes:
        rlds_free = load("openvla-oft_amd.prismatic.vla.datasets.rlds_free")
        ep = rlds_free.list_episodes(Path(args.episodes), args.dataset)[args.episode]
        t = min(args.step, len(ep) - 1)
        return ({"full_image": np.asarray(ep["image"][t]), "wrist_image": np.asarray(ep["wrist_image"][t]), "state": np.asarray(ep["state"][t], np.float64)},
                ep.language_instruction or "do the task")
    rng = np.random.default_rng(args.seed)
    return ({"full_image": rng.integers(0, 256, (side, side, 3), dtype=np.uint8), "wrist_image": rng.integers(0, 256, (side, side, 3), dtype=np.uint8),
             "state": rng.uniform(-1, 1, 8)}, "pick up the black bowl and place it on the plate")


def random_model(size: str, dev):
    weights_mod, config_mod, modeling = load("openvla-oft_amd.weights"), load("openvla-oft_amd.config"), load("openvla-oft_amd.modeling")
    if size == "7b":
        cfg = config_mod.OPENVLA_7B
        sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=True)
    else:
        from oracle import vla_oracle as vo
        ocfg = vo.tiny_config()
        cfg = config_mod.VLAConfig.from_any(ocfg)
        sd = {k: v.to(torch.bfloat16).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    sub = lambda pre: {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}  # noqa: E731
    stats = {DATASET: {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "mask": [True] * 6 + [False]}, "proprio": {"q01": [-1.0] * 8, "q99": [1.0] * 8}}}
    vla = modeling.OpenVLAForActionPrediction(cfg, {k: v for k, v in sd.items() if not k.startswith(("action_head.", "proprio_projector."))}, device=dev,
                                              norm_stats=stats)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=sub("action_head."))
    pp_sd = sub("proprio_projector.")
    pp = modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=pp_sd if size == "7b" else {"module." + k: v for k, v in pp_sd.items()})
    rng = np.random.default_rng(1)
    vocab = {}
    tok = lambda text: [1] + [vocab.setdefault(w, int(rng.integers(3, 31000))) for w in text.split()] + [29871]  # noqa: E731  (no tokenizer files: a word -> id stub)
    return vla, head, pp, tok


def heat_png(path: Path, frame: np.ndarray, grid: np.ndarray):
    from PIL import Image

    g = grid / max(float(grid.max()), 1e-30)
    heat = np.asarray(Image.fromarray((255 * g).astype(np.uint8)).resize(frame.shape[1::-1], Image.BILINEAR), np.float32) / 255.0
    out = 0.45 * frame.astype(np.float32) + 0.55 * 255.0 * np.stack([heat, 0.25 * heat, 1.0 - heat], axis=-1) * heat[..., None] ** 0.5
    Image.fromarray(np.clip(out, 0, 255).astype(np.uint8)).save(path)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--checkpoint")
    ap.add_argument("--l1", action="store_true")
    ap.add_argument("--proprio", action="store_true")
    ap.add_argument("--size", choices=["tiny", "7b"], default="tiny")
    ap.add_argument("--episodes")
    ap.add_argument("--dataset", default=DATASET)
    ap.add_argument("--episode", type=int, default=0)
    ap.add_argument("--step", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--layers", default=":", help="decoder layers averaged in the PNGs, as a Python slice (default: all)")
    ap.add_argument("--out", default="attention_maps.npz")
    args = ap.parse_args()
    utils = load("openvla-oft_amd.experiments.robot.openvla_utils")
    dev = torch.device("cuda:0")
    c = types.SimpleNamespace(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key=args.dataset, num_open_loop_steps=8,
                              pretrained_checkpoint=args.checkpoint, use_l1_regression=args.l1, use_diffusion=False, use_film=False)
    if args.checkpoint:
        vla = utils.get_vla(c)
        c.use_proprio = args.proprio
        head = utils.get_action_head(c, vla.llm_dim) if args.l1 else None
        pp = utils.get_proprio_projector(c, vla.llm_dim, vla.cfg.proprio_dim) if args.proprio else None
        proc = utils.get_processor(c)
    else:
        vla, head, pp, tok = random_model(args.size, dev)
        proc = utils.PrismaticProcessor(tok)
    side = vla.config.image_sizes[0]
    obs, task = observation(args, side)
    frames = [obs["full_image"], obs["wrist_image"]]
    if side == 224:
        actions, att = utils.get_vla_action(c, vla, proc, obs, task, action_head=head, proprio_projector=pp, return_attention=True)
    else:   # the reduced model: its towers take side x side frames, which the 224-pixel image path does not produce
        chans = [torch.from_numpy(np.asarray(f, np.float32).transpose(2, 0, 1) / 127.5 - 1.0) for f in frames for _ in range(2)]
        prompt = f"In: What action should the robot take to {task.lower()}?\nOut:"
        actions, _, att = vla.predict_action(**proc.tokenize(prompt), pixel_values=torch.cat(chans)[None], unnorm_key=c.unnorm_key, proprio=obs["state"],
                                             proprio_projector=pp, action_head=head, output_attentions=True)
    names = att.range_names
    mass = att.token_mass().cpu().numpy()                                                    # [layers, 1, A, ranges]
    maps = {f"patch_maps_image{i}": att.patch_maps(image=i).cpu().numpy() for i in range(c.num_images_in_input)}
    np.savez(args.out, token_mass=mass, range_names=np.array(names), ranges=np.array([att.layout[0][n] for n in names]), actions=np.stack(actions), **maps)
    lo, _, hi = args.layers.partition(":")
    sl = slice(int(lo) if lo else None, int(hi) if hi else None)
    share = mass[sl].mean(axis=(0, 1, 2))
    print(f"{task!r}: layers [{args.layers}] mean attention mass of the {mass.shape[2]} action rows: " + ", ".join(f"{n} {s:.3f}" for n, s in zip(names, share)))
    try:
        for i, frame in enumerate(frames):
            png = Path(args.out).with_name(Path(args.out).stem + f"_image{i}.png")
            heat_png(png, np.asarray(frame), maps[f"patch_maps_image{i}"][sl].mean(axis=(0, 1, 2)))
            print(f"wrote {png}")
    except ImportError:
        print("Pillow is not installed: no PNG heat maps")
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
