"""fp32 optimizer state (VLAEngine.enable_fp32_optimizer_state, finetune(optimizer_state="fp32")) on the GPU, on the reduced-size model of
test_grad_clip_gpu.py: the invariant param == bf16_rne(master) and the restatement of every step, the default mode untouched, clipping, EMA on
the master, resume with the four checkpoint / engine combinations, the driver and a two-rank run.  Every comparison is exact."""
import importlib
import math
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import vla_oracle as vo
from tests import adamw_master_reference as M
from tests import ema_reference as E
from tests import grad_clip_reference as R
from tests.pointwise_reference import adamw_emulate

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BF = torch.bfloat16
F32 = torch.float32
load = importlib.import_module
LR = 5e-4
WHICH = ("flat", "exp_avg", "exp_avg_sq", "flat_grad", "master")


def bits_of(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == BF else t.view(torch.int32).numpy().view(np.uint32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits_of(a), bits_of(b))


@pytest.fixture(scope="module")
def world(dev):
    config_mod, synth, ft, K = (load("openvla-oft_amd." + m) for m in ("config", "synthetic", "vla_scripts.finetune", "prismatic.vla.constants"))
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    base = config_mod.VLAConfig.from_any(ocfg)
    fcfg = ft.FinetuneConfig()
    cfg = config_mod.VLAConfig(**{**base.__dict__, "num_images": 2, "lora_rank": fcfg.lora_rank, "lora_alpha": min(fcfg.lora_rank, 16),
                                  "action_dim": K.ACTION_DIM, "chunk": K.NUM_ACTIONS_CHUNK, "proprio_dim": K.PROPRIO_DIM,
                                  "norm_type": K.ACTION_PROPRIO_NORMALIZATION_TYPE.value})
    stats = {"libero_spatial_no_noops": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "min": [-1.0] * 7, "max": [1.0] * 7, "mask": [True] * 6 + [False]}}}
    return dict(cfg=cfg, base_cfg=base, sd=sd, synth=synth, ft=ft, stats=stats)


def fresh(world, dev, fp32=False):
    engine_mod, weights_mod = load("openvla-oft_amd.engine"), load("openvla-oft_amd.weights")
    get, has = weights_mod.make_getter({k: v.clone() for k, v in world["sd"].items()}, dev)
    e = engine_mod.VLAEngine(world["cfg"], get, dev, lora=True, use_proprio=True, head="l1", has=has)
    if fp32:
        e.enable_fp32_optimizer_state()
    return e


def batch_of(world, i):
    return world["synth"].make_batch(2, seed=100 + i, prompt_lens=[9, 8], image_size=56)


def snap(e):
    """{(store index, dtype tag): {flat, exp_avg, exp_avg_sq, flat_grad[, master]: CPU copy}} of every flat buffer of the engine."""
    out = {}
    for i, st in enumerate(e.stores):
        for dt in st.flat:
            out[(i, "bf16" if dt == BF else "f32")] = {w: getattr(st, w)[dt].detach().cpu().clone() for w in WHICH if dt in getattr(st, w)}
    return out


def same_snap(a, b, which=("flat", "exp_avg", "exp_avg_sq", "master")):
    return a.keys() == b.keys() and all(a[k].keys() == b[k].keys() and all(same(a[k][w], b[k][w]) for w in which if w in a[k]) for k in a)


def backward(e, world, i):
    e.zero_grad()
    loss_sum, _, _ = e.train_step_fwd_bwd(batch_of(world, i))
    return bits_of(loss_sum)


def step(e, world, i, **kw):
    loss = backward(e, world, i)
    e.adamw_step(LR, **kw)
    e.refresh_derived()
    return loss


def invariant_holds(e):
    return all(same(s["master"].to(BF), s["flat"]) for k, s in snap(e).items() if "master" in s) and all(st.master_matches_param() for st in e.stores)


def restated_step(before, k, *, state=None, grad_scale=1.0):
    """One optimizer step of every buffer of a snapshot (taken after the backward), by the restatements: the master form for a buffer that
    has a master, ovla_adamw's own (pointwise_reference / grad_clip_reference) for the others."""
    out = {}
    for key, s in before.items():
        hp = dict(step=k, lr=LR, grad_scale=grad_scale)
        if "master" in s:
            ma, m, v, p = M.adamw_master(s["master"], s["exp_avg"], s["exp_avg_sq"], s["flat"], s["flat_grad"], state=state, **hp)
            out[key] = dict(master=ma, exp_avg=m, exp_avg_sq=v, flat=p)
        else:
            p, m, v = adamw_emulate(s["flat"], s["exp_avg"], s["exp_avg_sq"], s["flat_grad"], **hp) if state is None else \
                R.adamw_clipped(s["flat"], s["exp_avg"], s["exp_avg_sq"], s["flat_grad"], state, **hp)
            out[key] = dict(exp_avg=m, exp_avg_sq=v, flat=p)
    return out


def assert_snap(got, want, what):
    for key, s in want.items():
        for w, t in s.items():
            assert same(got[key][w], t), f"{what}: {w} of store {key}: {int((bits_of(got[key][w]) != bits_of(t)).sum())} of {t.numel()} elements differ"


# ----------------------------------------------------------------------------------------------------------------------------------------
# the engine
# ----------------------------------------------------------------------------------------------------------------------------------------
def test_fp32_mode_keeps_the_invariant_and_equals_the_restatement(world, dev):
    e = fresh(world, dev)
    assert e.optimizer_state_precision == "param" and all(not st.master for st in e.stores)
    e.enable_fp32_optimizer_state()
    assert e.optimizer_state_precision == "fp32"
    start = snap(e)
    keys = sorted(start)
    assert len({i for i, _ in keys}) == 3 and {t for _, t in keys} == {"bf16", "f32"}
    for key, s in start.items():
        assert ("master" in s) == (key[1] == "bf16"), "a master for every bf16 buffer and for no fp32 one"
        if "master" in s:
            assert s["master"].dtype == F32 and same(s["master"], s["flat"].float()), "the master starts as the parameters widened exactly"
    assert e.fp32_optimizer_state_bytes() == 8 * sum(s["flat"].numel() for k, s in start.items() if k[1] == "bf16")
    for i in range(3):
        backward(e, world, i)
        before = snap(e) if i else {k: dict(s, exp_avg=torch.zeros_like(s["flat"], dtype=F32), exp_avg_sq=torch.zeros_like(s["flat"], dtype=F32)) for k, s in snap(e).items()}
        e.adamw_step(LR)
        e.refresh_derived()
        after = snap(e)
        assert all(s["exp_avg"].dtype == F32 and s["exp_avg_sq"].dtype == F32 for s in after.values()), "fp32 moments for every buffer"
        assert_snap(after, restated_step(before, i + 1), f"step {i + 1}")
        assert invariant_holds(e), f"step {i + 1}: param == bf16_rne(master)"
    moved = [k for k, s in after.items() if "master" in s and not same(s["master"], s["flat"].float())]
    assert moved == [k for k in keys if k[1] == "bf16"], "after three steps every master holds more than its bf16 rounding"
    e.enable_fp32_optimizer_state()      # idempotent
    assert same_snap(snap(e), after)


def test_default_mode_is_untouched(world, dev):
    e = fresh(world, dev)
    for i in range(3):
        backward(e, world, i)
        before = snap(e) if i else {k: dict(s, exp_avg=torch.zeros_like(s["flat"]), exp_avg_sq=torch.zeros_like(s["flat"])) for k, s in snap(e).items()}
        e.adamw_step(LR)
        e.refresh_derived()
        assert_snap(snap(e), restated_step(before, i + 1), f"default mode, step {i + 1}")       # torch's AdamW in the parameter's dtype
    after = snap(e)
    assert all("master" not in s and s["exp_avg"].dtype == s["flat"].dtype == s["exp_avg_sq"].dtype for s in after.values())
    osd = e.optimizer_state_dict()
    want_keys = {"lora_dropout.call"} | {f"store{i}.step" for i in range(3)} | {f"store{i}.{t}.{w}" for i, t in after for w in ("exp_avg", "exp_avg_sq")}
    assert set(osd) == want_keys
    for (i, t), s in after.items():
        for w in ("exp_avg", "exp_avg_sq"):
            assert same(osd[f"store{i}.{t}.{w}"], s[w])
    assert all(int(osd[f"store{i}.step"].item()) == 3 for i in range(3))
    fp32 = fresh(world, dev, fp32=True)
    for i in range(3):
        step(fp32, world, i)
    assert not same(snap(fp32)[(0, "bf16")]["flat"], after[(0, "bf16")]["flat"]), "the switch changes the trajectory, the default does not take it"


def test_clipping_in_fp32_mode(world, dev):
    # a huge max_norm is the plain fp32 mode bit for bit
    e_clip, e_plain = fresh(world, dev, fp32=True), fresh(world, dev, fp32=True)
    e_clip.enable_grad_clip(1e30)
    for i in range(2):
        assert np.array_equal(step(e_clip, world, i), step(e_plain, world, i))
        assert same_snap(snap(e_clip), snap(e_plain)), f"step {i + 1}"
    # a clipped step equals the restatement; the norm is over the gradient as this optimizer sees it: not rounded to bf16
    e = e_plain
    backward(e, world, 2)
    scale = 0.5
    before = snap(e)
    keys = sorted(before)
    slots = [R.grad_sumsq(before[k]["flat_grad"].numpy(), scale, False) for k in keys]
    assert slots[0] != R.grad_sumsq(before[keys[0]]["flat_grad"].numpy(), scale, True), "the two norms differ on this gradient"
    max_norm = float(np.float32(0.25 * math.sqrt(sum(slots))))
    e.enable_grad_clip(max_norm)
    e.adamw_step(LR, grad_scale=scale)
    e.refresh_derived()
    want = R.clip_coef(slots, np.float32(max_norm), R.new_state())
    got = e.grad_clip_stats()
    assert np.float32(got["norm"]).tobytes() == want["norm"].tobytes() and np.float32(got["coef"]).tobytes() == want["coef"].tobytes(), (got, want)
    assert 0.2 < got["coef"] < 0.3 and (got["steps"], got["clipped"], got["skipped"]) == (1, 1, 0)
    assert_snap(snap(e), restated_step(before, 3, state=want, grad_scale=scale), "clipped step")
    assert invariant_holds(e)
    # a planted Inf skips the step: master, moments and parameters keep their bits
    backward(e, world, 3)
    e.stores[0].flat_grad[BF][5] = float("inf")
    before = snap(e)
    e.adamw_step(LR)
    e.refresh_derived()
    s = e.grad_clip_stats()
    assert math.isinf(s["norm"]) and (s["skipped"], s["steps"]) == (1, 2)
    assert same_snap(snap(e), before) and invariant_holds(e)


def test_ema_follows_the_master(world, dev):
    e = fresh(world, dev, fp32=True)
    step(e, world, 0)
    e.enable_ema()
    s0 = snap(e)
    shadows0 = {(i, "bf16" if dt == BF else "f32"): sh.detach().cpu().clone() for i, st in enumerate(e.stores) for dt, sh in st.ema_shadow.items()}
    for key, s in s0.items():
        assert same(shadows0[key], s["master"] if "master" in s else s["flat"]), "the shadow starts from the master"
    step(e, world, 1)
    e.ema_update(0.5)
    s1 = snap(e)
    omd = E.one_minus_decay(0.5)
    differ = 0
    for i, st in enumerate(e.stores):
        for dt, sh in st.ema_shadow.items():
            key = (i, "bf16" if dt == BF else "f32")
            src = s1[key].get("master", s1[key]["flat"])
            assert E.same_f32(sh.cpu().numpy(), E.ema_update(shadows0[key].numpy(), src.numpy(), omd)), f"shadow of {key}: the reference applied to the master"
            if dt == BF:
                from_param = E.ema_update(shadows0[key].numpy(), E.widen_bf16(bits_of(s1[key]["flat"])), omd)
                differ += int((E.u32(sh.cpu().numpy()) != E.u32(from_param)).sum())
    assert differ > 0, "the shadow is not the reference applied to the bf16 parameters"
    with e.ema_weights():
        assert not same(snap(e)[(0, "bf16")]["flat"], s1[(0, "bf16")]["flat"])
        with pytest.raises(RuntimeError, match="ema_weights"):
            e.enable_fp32_optimizer_state()
    assert same_snap(snap(e), s1) and invariant_holds(e), "the scope restores the parameters' bits: the invariant holds on exit"
    plain = fresh(world, dev)
    plain.enable_ema()
    with plain.ema_weights():
        with pytest.raises(RuntimeError, match="ema_weights"):
            plain.enable_fp32_optimizer_state()
    assert plain.optimizer_state_precision == "param"


def saved(e):
    return ({k: v.detach().cpu().clone() for k, v in e.optimizer_state_dict().items()},
            {k: v.detach().cpu().clone() for k, v in e.export_trainable("data").items()})


def test_resume_and_the_four_checkpoint_engine_combinations(world, dev):
    a, p = fresh(world, dev, fp32=True), fresh(world, dev)
    for i in range(2):
        step(a, world, i), step(p, world, i)
    osd_a, params_a = saved(a)
    osd_p, params_p = saved(p)
    assert osd_a["store0.bf16.master"].dtype == F32 and osd_a["store0.bf16.exp_avg"].dtype == F32 and osd_a["store0.bf16.exp_avg_sq"].dtype == F32
    assert set(osd_a) - set(osd_p) == {f"store{i}.bf16.master" for i, st in enumerate(a.stores) if BF in st.flat}
    loss_a, loss_p = step(a, world, 2), step(p, world, 2)
    # fp32 -> fp32: the continued run lands on the uninterrupted one's master, moments and parameters
    b = fresh(world, dev, fp32=True)
    b.load_trainable(params_a)
    b.load_optimizer_state_dict(osd_a)
    assert invariant_holds(b)
    assert np.array_equal(step(b, world, 2), loss_a) and same_snap(snap(b), snap(a))
    # fp32 -> fp32 with parameters of another step: refused
    c = fresh(world, dev, fp32=True)
    with pytest.raises(ValueError, match="different steps"):
        c.load_optimizer_state_dict(osd_a)
    # fp32 -> param: refused, and the message names the switch
    d = fresh(world, dev)
    d.load_trainable(params_a)
    before = snap(d)
    with pytest.raises(ValueError, match='optimizer_state="fp32"'):
        d.load_optimizer_state_dict(osd_a)
    assert same_snap(snap(d), before) and all(st.step == 0 for st in d.stores), "refused before anything was changed"
    # param -> param: unchanged
    d.load_trainable(params_p)
    d.load_optimizer_state_dict(osd_p)
    assert np.array_equal(step(d, world, 2), loss_p) and same_snap(snap(d), snap(p))
    # param -> fp32: moments widened exactly, the master is the widened loaded parameters, one line says so
    lines = []
    f = fresh(world, dev, fp32=True)
    f.load_trainable(params_p)
    f.load_optimizer_state_dict(osd_p, log=lines.append)
    assert len(lines) == 1 and "widened" in lines[0]
    for (i, t), s in snap(f).items():
        for w in ("exp_avg", "exp_avg_sq"):
            assert same(s[w], osd_p[f"store{i}.{t}.{w}"].float()), f"{w} of store {(i, t)}"
        if "master" in s:
            assert same(s["master"], s["flat"].float())
    assert all(st.step == 2 for st in f.stores) and invariant_holds(f)
    step(f, world, 2)
    assert invariant_holds(f)
    b.load_optimizer_state_dict(saved(b)[0], log=lines.append)
    assert len(lines) == 1, "nothing is widened, nothing is logged, for an fp32 checkpoint"


# ----------------------------------------------------------------------------------------------------------------------------------------
# the driver
# ----------------------------------------------------------------------------------------------------------------------------------------
def drive(world, root, *, first=0, lines=None, extra=None, **kw):
    ft = world["ft"]
    engines, orig = [], ft.VLAEngine

    def build(*a, **k):
        engines.append(orig(*a, **k))
        return engines[-1]

    cfg = ft.FinetuneConfig(**{**dict(run_root_dir=root, dataset_name="libero_spatial_no_noops", batch_size=2, num_images_in_input=2, use_proprio=True,
                                      wandb_log_freq=1, max_steps=3, save_freq=2), **kw})
    ft.VLAEngine = build
    try:
        hist = ft.finetune(cfg, model_config=world["base_cfg"], state_dict={k: v.clone() for k, v in world["sd"].items()},
                           dataset=(batch_of(world, i) for i in range(first, 12)), dataset_statistics=world["stats"],
                           log=(lines.append if lines is not None else (lambda *_: None)), **(extra or {}))
    finally:
        ft.VLAEngine = orig
    engine, = engines
    return hist, engine


def test_driver_runs_logs_checkpoints_and_resumes(world, dev, tmp_path):
    from safetensors.torch import load_file

    with pytest.raises(ValueError, match="optimizer_state"):
        drive(world, tmp_path / "bad", extra=dict(optimizer_state="bf32"))
    lines = []
    hist, engine = drive(world, tmp_path / "fp32", lines=lines, extra=dict(optimizer_state="fp32", ema_decay=0.5, max_grad_norm=1e-3))
    assert engine.optimizer_state_precision == "fp32" and len(hist["loss_value"]) == 3 and invariant_holds(engine)
    mode = [l for l in map(str, lines) if "optimizer_state=fp32" in l]
    assert len(mode) == 1 and f"+{engine.fp32_optimizer_state_bytes()} bytes" in mode[0], lines
    ck, = (tmp_path / "fp32").glob("*--2_chkpt")
    osd = load_file(str(ck / "optimizer_state--2_checkpoint.safetensors"))
    assert osd["store0.bf16.master"].dtype == F32 and osd["store0.bf16.exp_avg"].dtype == F32 and osd["store0.bf16.exp_avg_sq"].dtype == F32
    assert not any(k.endswith(".f32.master") for k in osd) and any(".f32.exp_avg" in k for k in osd), "the fp32 buffers are as before"
    assert osd["ema.store0.bf16.shadow"].dtype == F32
    # the default run: says so, and writes the same files with the old optimizer-state keys
    lines_p = []
    _, engine_p = drive(world, tmp_path / "param", lines=lines_p, extra=dict(ema_decay=0.5, max_grad_norm=1e-3))
    assert engine_p.optimizer_state_precision == "param" and sum("optimizer_state=param" in str(l) for l in lines_p) == 1
    ck_p, = (tmp_path / "param").glob("*--2_chkpt")
    osd_p = load_file(str(ck_p / "optimizer_state--2_checkpoint.safetensors"))
    assert set(osd) - set(osd_p) == {k for k in osd if k.endswith(".bf16.master")} and osd_p["store0.bf16.exp_avg"].dtype == BF
    listing = lambda d: sorted(str(f.relative_to(d)) for f in d.rglob("*"))  # noqa: E731
    assert listing(ck) == listing(ck_p), "no new file in a checkpoint directory: the model checkpoints keep their format"
    # resume: an fp32 run continues from its own checkpoint, and from the default run's by widening; the default mode refuses the fp32 file
    lines_r = []
    _, resumed = drive(world, tmp_path / "resumed", first=3, lines=lines_r, resume=True, resume_step=2, vla_path=str(ck), max_steps=4,
                       extra=dict(optimizer_state="fp32", ema_decay=0.5, max_grad_norm=1e-3))
    assert invariant_holds(resumed) and all(st.step == 5 for st in resumed.stores) and not any("widened" in str(l) for l in lines_r)
    lines_w = []
    _, widened = drive(world, tmp_path / "widened", first=3, lines=lines_w, resume=True, resume_step=2, vla_path=str(ck_p), max_steps=4,
                       extra=dict(optimizer_state="fp32"))
    assert invariant_holds(widened) and sum("widened" in str(l) for l in lines_w) == 1
    with pytest.raises(ValueError, match='optimizer_state="fp32"'):
        drive(world, tmp_path / "refused", first=3, resume=True, resume_step=2, vla_path=str(ck), max_steps=4)


# ----------------------------------------------------------------------------------------------------------------------------------------
# two ranks
# ----------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world_size, port, out):
    import torch.distributed as dist

    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    engine_mod, weights_mod, config_mod, synth, dp = (load("openvla-oft_amd." + m) for m in ("engine", "weights", "config", "synthetic", "dp"))
    ocfg = vo.tiny_config()
    sd = {k: v.to(BF).float() for k, v in vo.random_state_dict(ocfg, seed=0).items()}
    get, has = weights_mod.make_getter(sd, dev)
    eng = engine_mod.VLAEngine(config_mod.VLAConfig.from_any(ocfg), get, dev, lora=True, use_proprio=True, head="l1", has=has)
    eng.enable_fp32_optimizer_state()
    red = dp.GradReducer(eng.stores, world_size, bucket_bytes=64 << 10, comm_dtype="fp32")
    eng.attach_reducer(red, overlap=True)
    batch = synth.make_batch(4, seed=31, prompt_lens=[10, 8, 12, 9], image_size=56)
    for _ in range(2):
        eng.zero_grad()
        eng.train_step_fwd_bwd({k: (v[2 * rank:2 * rank + 2] if torch.is_tensor(v) else v) for k, v in batch.items()})
        red.all_reduce()
        eng.adamw_step(lr=5e-4, grad_scale=1.0 / world_size)
        eng.refresh_derived()
    torch.save({"master": [st.master[BF].cpu() for st in eng.stores if BF in st.master], "param": [st.flat[BF].cpu() for st in eng.stores if BF in st.master],
                "invariant": all(st.master_matches_param() for st in eng.stores)}, f"{out}/rank{rank}.pt")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_end_on_identical_master_bits(dev, tmp_path):
    import torch.multiprocessing as mp

    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in (0, 1))
    assert r0["invariant"] and r1["invariant"] and len(r0["master"]) >= 2
    for a, b, p in zip(r0["master"], r1["master"], r0["param"]):
        assert same(a, b), "ranks disagree on the master"
        assert same(a.to(BF), p) and not same(a, p.float()), "param is the rounded master, and the master holds more than it"
