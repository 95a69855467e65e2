"""sha256 digests of what one training / evaluation step computes, for comparing two commits bit for bit: train_step_fwd_bwd (one step, a second
micro-step accumulated on top, loss_scale = 0.5) and eval_step for the L1, FiLM, diffusion and lora_dropout objectives, the L1 step with
OVLA_LAST_LAYER_SEL=0 (the full last layer and the scatter branch), train_step_discrete / eval_step(discrete=True) with the labels as generated
(171 counted rows: pad, gather and scatter) and with the stop-token labels ignored (168 rows: the selected-rows branch), the autograd bridge
(`output.loss.backward()` and finetune.run_forward_pass's L1 path) and sample_actions -- on the worlds of tests/step_invariants.py (the reduced
model, B = 3, rows of 64 to 69 tokens, 56 x 56 images).  Only public names are used, so the same file runs against any commit that has them.

Every case starts from zero_grad() and runs twice in the process; its digest covers the prediction bits and every tensor of
export_trainable("grad") (the bridge: every published `.grad`).  The head's loss_sum is a sum of float atomics in completion order
(tests/step_invariants.py): it stays out of the digest and is recorded beside it with its restatement from the prediction bits; the discrete
loss, a torch sum, is hashed.

    python tools/step_digest.py --side parent --commit C --tree T --out parent.json      (in a checkout of the parent; needs the GPU)
    python tools/step_digest.py --side branch --commit C --tree T --out branch.json      (in this tree; needs the GPU)
    python tools/step_digest.py --merge parent.json branch.json                          (no GPU) -> profiles/step_refactor_digests.json
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
load = importlib.import_module
HEAD_KINDS = ("l1", "film", "diffusion", "l1_dropout")
SAMPLER_STEPS = 5


def digest(tensors) -> str:
    """tensors: [(name, tensor)] -> sha256 over each name, dtype, shape and the raw bytes."""
    m = hashlib.sha256()
    for name, t in tensors:
        t = t.detach().contiguous().cpu()
        m.update(f"{name}{t.dtype}{tuple(t.shape)}".encode())
        m.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return m.hexdigest()


def of_step(res, with_loss: bool):
    return [("pred", res.pred)] + ([("loss_sum", res.loss_sum)] if with_loss else []) + sorted(res.grads.items())


def published(mods):
    """The `.grad` views publish_grads() hands to a torch optimizer, module by module."""
    return [(f"{i}:{n}", p.grad) for i, m in enumerate(mods) for n, p in sorted(m.named_parameters(), key=lambda kv: kv[0])]


def build_cases(dev):
    """-> [(name, zero-argument call returning (tensors to hash, head loss record or None))]"""
    si = load("step_invariants")
    engine_mod, weights_mod, modeling = load("openvla-oft_amd.engine"), load("openvla-oft_amd.weights"), load("openvla-oft_amd.modeling")
    ft = load("openvla-oft_amd.vla_scripts.finetune")
    worlds = {k: si.make_world(dev, k) for k in si.KINDS}
    cases = []

    def head_loss(world, which, res, scale=1.0):
        total, n, order_free = si.loss_reference(res.pred, si.step_target(world, which), world["kind"] == "diffusion")
        return dict(loss_sum=float(res.loss_sum.reshape(-1)[0]), count=res.count, loss_scale=scale, exact_sum=total, terms=n, order_free=order_free)

    def head_cases(kind, tag="", env=None):
        world = worlds[kind]

        def run(fn):
            def call():
                old = {k: os.environ.get(k) for k in (env or {})}
                os.environ.update(env or {})
                try:
                    world["eng"].zero_grad()
                    return fn()
                finally:
                    for k, v in old.items():
                        if v is None:
                            del os.environ[k]
                        else:
                            os.environ[k] = v
            return call

        def one(scale):
            res = si.step(world, world["batches"][0], scale, call=0)
            return of_step(res, False), head_loss(world, 0, res, scale)

        def accumulate():
            si.step(world, world["batches"][0], call=0)
            res = si.step(world, world["batches"][1], call=1)
            return of_step(res, False), head_loss(world, 1, res)

        def evaluate():
            loss_sum, count, pred = world["eng"].eval_step(world["batches"][0], diffusion=world["diffusion"][0])
            res = si.StepResult(loss_sum.detach().clone(), int(count), si.export_grads(world["eng"]), pred.detach().clone())
            return of_step(res, False), head_loss(world, 0, res)

        cases.append((f"{kind}{tag}/step", run(lambda: one(1.0))))
        if not tag:
            cases.extend([(f"{kind}/accumulate", run(accumulate)), (f"{kind}/loss_scale_0.5", run(lambda: one(0.5))), (f"{kind}/eval", run(evaluate))])

    for kind in HEAD_KINDS:
        head_cases(kind)
    head_cases("l1", tag="_full_last_layer", env={"OVLA_LAST_LAYER_SEL": "0"})

    # ---- discrete: labels as generated (3 x 57 counted rows), and with the stop-token labels ignored (3 x 56) ----
    disc = worlds["discrete"]
    as_made = disc["batches"][0]
    lab = as_made["labels"].clone()
    lab[(lab != -100) & (lab <= 31743)] = -100
    variants = (("discrete", as_made, 171), ("discrete_no_stop", dict(as_made, labels=lab), 168))

    def discrete_case(batch, rows, fn):
        def call():
            disc["eng"].zero_grad()
            loss_sum, count, pred = fn(batch)
            assert count == rows, f"{count} counted rows, the case is written for {rows}"
            return of_step(si.StepResult(loss_sum.detach().clone(), int(count), si.export_grads(disc["eng"]), pred.detach().clone()), True), None
        return call

    for name, batch, rows in variants:
        cases.append((f"{name}/step", discrete_case(batch, rows, lambda b: disc["eng"].train_step_discrete(b))))
        cases.append((f"{name}/loss_scale_0.5", discrete_case(batch, rows, lambda b: disc["eng"].train_step_discrete(b, loss_scale=0.5))))
        cases.append((f"{name}/eval", discrete_case(batch, rows, lambda b: disc["eng"].eval_step(b, discrete=True))))

    # ---- the autograd bridge ----
    def sub(sd, pre, add=""):
        return {add + k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}

    def api(world):
        cfg, sd = world["cfg"], world["sd"]
        vla = modeling.OpenVLAForActionPrediction(cfg, sd, device=dev)
        head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, cfg.action_dim, device=dev, state_dict=sub(sd, "action_head."))
        pp = modeling.ProprioProjector(cfg.llm_dim, cfg.proprio_dim, device=dev, state_dict=sub(sd, "proprio_projector.", "module."))
        return vla, head, pp

    dvla, _, dpp = api(disc)
    lvla, lhead, lpp = api(worlds["l1"])

    def bridge_discrete():
        for m in (dvla, dpp):
            m.store.zero_grad()
        out = dvla(input_ids=as_made["input_ids"], attention_mask=as_made["attention_mask"], pixel_values=as_made["pixel_values"], labels=as_made["labels"],
                   output_hidden_states=True, proprio=as_made["proprio"], proprio_projector=dpp)
        out.loss.backward()
        return [("loss", out.loss)] + published((dvla, dpp)), None

    def bridge_l1():
        batch = worlds["l1"]["batches"][0]
        for m in (lvla, lhead, lpp):
            m.store.zero_grad()
        loss, _ = ft.run_forward_pass(lvla, lhead, None, lpp, batch, None, dev, True, False, True, False, lvla.engine.num_patches_total(2, True))
        loss.backward()
        return [("loss", loss)] + published((lvla, lhead, lpp)), None

    cases += [("bridge/discrete_loss_backward", bridge_discrete), ("bridge/run_forward_pass_l1", bridge_l1)]

    # ---- the sampler, and one step on device-drawn noise: the diffusion world's weights and batch on an engine with the device noise state ----
    dworld = worlds["diffusion"]
    get, has = weights_mod.make_getter({k: v.clone() for k, v in dworld["sd"].items()}, dev)
    seng = engine_mod.VLAEngine(dworld["cfg"], get, dev, lora=True, use_proprio=True, head="diffusion", has=has, num_diffusion_steps=SAMPLER_STEPS, diffusion_seed=77)
    sbatch = dworld["batches"][0]
    noise = torch.randn(3, 8, 7, generator=torch.Generator().manual_seed(9))

    def device_noise_step():
        seng.zero_grad()
        seng.diffusion.call = 3
        d = seng.draw_diffusion(sbatch["actions"])
        loss_sum, count, pred = seng.train_step_fwd_bwd(sbatch, diffusion=d)
        total, n, order_free = si.loss_reference(pred, d["noise"].reshape(-1, 7), True)
        rec = dict(loss_sum=float(loss_sum.reshape(-1)[0]), count=int(count), loss_scale=1.0, exact_sum=total, terms=n, order_free=order_free)
        return [("pred", pred)] + sorted((k, v) for k, v in d.items()) + sorted(si.export_grads(seng).items()), rec

    def sample(start):
        def call():
            seng.zero_grad()
            seng.diffusion.call = 3
            return [("actions", seng.sample_actions(sbatch, start_noise=start))] + sorted(si.export_grads(seng).items()), None
        return call

    cases += [("diffusion/device_noise_step", device_noise_step), ("sample_actions/start_noise", sample(noise)), ("sample_actions/own_noise", sample(None))]
    return cases


def run(args):
    dev = torch.device("cuda:0")
    cases = build_cases(dev)
    passes = []
    for _ in range(2):
        got = {}
        for name, call in cases:
            tensors, loss = call()
            got[name] = (digest(tensors), loss)
        passes.append(got)
    result = dict(side=args.side, commit=args.commit, tree_openvla_oft_amd=args.tree, library_source_hash=load("openvla-oft_amd._lib").source_hash(),
                  digests={}, second_run={}, head_losses={}, not_repeatable=[])
    for name, _ in cases:
        (d1, l1), (d2, l2) = passes[0][name], passes[1][name]
        result["digests"][name], result["second_run"][name] = d1, d2
        if l1 is not None:
            result["head_losses"][name] = [l1, l2]
        if d1 != d2:
            result["not_repeatable"].append(name)
        print(f"{d1}  {name}" + ("" if d1 == d2 else f"   SECOND RUN DIFFERS: {d2}"))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(f"{len(cases)} cases, {len(result['not_repeatable'])} not repeatable within the process -> {args.out}")


def merge(parent_file, branch_file, out):
    si = load("step_invariants")
    parent, branch = (json.loads(Path(f).read_text()) for f in (parent_file, branch_file))
    names = sorted(set(parent["digests"]) | set(branch["digests"]))
    differing = [n for n in names if parent["digests"].get(n) != branch["digests"].get(n)]
    findings = si.Findings()
    for n in sorted(set(parent["head_losses"]) & set(branch["head_losses"])):
        for p, b in zip(parent["head_losses"][n], branch["head_losses"][n]):
            ref = (p["exact_sum"], p["terms"], p["order_free"])
            findings.check((b["exact_sum"], b["terms"], b["order_free"], b["count"]) == ref + (p["count"],), f"{n}: the restated loss terms differ")
            findings.same_loss(torch.tensor([p["loss_sum"]]), torch.tensor([b["loss_sum"]]), ref, f"{n} (first = parent, second = branch)")
    result = dict(cases=len(names), all_digests_equal=not differing, differing=differing, loss_findings=list(findings),
                  not_repeatable=dict(parent=parent["not_repeatable"], branch=branch["not_repeatable"]), parent=parent, branch=branch)
    Path(out).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(f"{len(names)} cases: {len(names) - len(differing)} digests equal, {len(differing)} differ {differing}; loss findings: {list(findings)}; "
          f"not repeatable: {result['not_repeatable']} -> {out}")
    return 1 if differing or findings or parent["not_repeatable"] or branch["not_repeatable"] else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--side", default="this tree")
    ap.add_argument("--commit", default="")
    ap.add_argument("--tree", default="", help="git tree hash of openvla-oft_amd/ (git rev-parse COMMIT:openvla-oft_amd)")
    ap.add_argument("--out", default="step_digests.json")
    ap.add_argument("--merge", nargs=2, metavar=("PARENT_JSON", "BRANCH_JSON"))
    a = ap.parse_args()
    sys.exit(merge(*a.merge, ROOT / "profiles" / "step_refactor_digests.json") if a.merge else run(a))
