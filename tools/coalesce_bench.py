"""Serving throughput with request coalescing, in process and without HTTP: N closed-loop clients (threads) call `OpenVLAServer.act` on
one full-size synthetic model (random OpenVLA-7B-shaped weights, merged LoRA, L1 head, proprio, two 224 x 224 frames per request, hipGraph
replay -- the model of tools/batch_infer_bench.py behind the whole request path: payload decode, device image prep, prompt assembly,
forward, un-normalisation, encode).  `coalesce_ms = 0` is the uncoalesced server (one request at a time behind its lock); the positive
settings merge whatever is waiting.  The settings are alternated inside one process, `--reps` times per client count; one JSON line per
(clients, coalesce_ms) with chunks/s and the p50 / p95 request latency over all repetitions, then a summary line.
Usage: python tools/coalesce_bench.py [--clients 1,2,4,8] [--coalesce-ms 0,2,5] [--requests 40] [--reps 2] > profiles/coalesce_bench.jsonl"""
import argparse
import importlib
import json
import sys
import threading
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
load = importlib.import_module


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", default="1,2,4,8")
    ap.add_argument("--coalesce-ms", default="0,2,5")
    ap.add_argument("--requests", type=int, default=40, help="timed requests per client and repetition")
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    weights_mod, config_mod, modeling, utils, dep = (load(f"openvla-oft_amd.{m}") for m in (
        "weights", "config", "modeling", "experiments.robot.openvla_utils", "vla_scripts.deploy"))
    dev = torch.device("cuda:0")
    cfg = config_mod.OPENVLA_7B
    sd = weights_mod.random_state_dict(cfg, dev, seed=0, lm_head=False, lora=True)
    stats = {"libero": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7, "mask": [True] * 6 + [False]}, "proprio": {"q01": [-1.0] * 8, "q99": [1.0] * 8}}}
    sub = lambda pre: {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}  # noqa: E731
    vla = modeling.OpenVLAForActionPrediction(cfg, {k: v for k, v in sd.items() if not k.startswith(("action_head.", "proprio_projector."))},
                                              device=dev, norm_stats=stats)
    head = modeling.L1RegressionActionHead(cfg.llm_dim, cfg.llm_dim, 7, device=dev, state_dict=sub("action_head."))
    pp = modeling.ProprioProjector(cfg.llm_dim, 8, device=dev, state_dict=sub("proprio_projector."))
    del sd
    vla.merge_and_unload()
    # no tokenizer files offline: a stub of 38 tokens whose ids depend on the text (one text-length bucket, so one graph per batch bucket)
    tok = lambda text: [1] + [3 + (ord(c) * 131 + i) % 30000 for i, c in enumerate(text)][:36] + [29871]  # noqa: E731
    proc = utils.PrismaticProcessor(tok)
    settings = [float(x) for x in args.coalesce_ms.split(",")]
    kw = dict(num_images_in_input=2, use_proprio=True, center_crop=True, unnorm_key="libero", num_open_loop_steps=8)
    servers = {ms: dep.OpenVLAServer(dep.DeployConfig(coalesce_ms=ms, **kw), vla=vla, processor=proc, action_head=head, proprio_projector=pp)
               for ms in settings}
    rng = np.random.default_rng(0)
    tasks = ["pick up the black bowl and place it on the plate", "open the top drawer of the cabinet and put the bowl in",
             "turn on the stove and put the moka pot on it", "put the wine bottle on top of the cabinet now"]

    def payload(i):
        return dep._encode({"full_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8), "wrist_image": rng.integers(0, 256, (224, 224, 3), dtype=np.uint8),
                            "state": rng.uniform(-1, 1, 8), "instruction": tasks[i % len(tasks)][: 32 + i % 5]})

    pool = [[payload(c * 7 + j) for j in range(4)] for c in range(max(int(x) for x in args.clients.split(",")))]

    def leg(server, n_clients, n_requests):
        """n_clients closed-loop threads, n_requests each -> (wall seconds, per-request latencies in seconds)."""
        lat, gate, bad = [[] for _ in range(n_clients)], threading.Barrier(n_clients + 1), []

        def client(c):
            gate.wait()
            for j in range(n_requests):
                t0 = time.perf_counter()
                r = server.act(pool[c][j % 4])
                lat[c].append(time.perf_counter() - t0)
                if r == "error":
                    bad.append((c, j))

        threads = [threading.Thread(target=client, args=(c,)) for c in range(n_clients)]
        for t in threads:
            t.start()
        gate.wait()
        t0 = time.perf_counter()
        for t in threads:
            t.join()
        wall = time.perf_counter() - t0
        if bad:
            raise RuntimeError(f"{len(bad)} requests answered 'error'")
        return wall, [x for per in lat for x in per]

    rows = []
    try:
        for n in [int(x) for x in args.clients.split(",")]:
            acc = {ms: dict(wall=0.0, lat=[], calls=0) for ms in settings}
            for ms in settings:                       # un-timed: graph captures of every bucket this client count reaches
                leg(servers[ms], n, 6)
            for _ in range(args.reps):
                for ms in settings:                   # alternated: drift hits every setting alike
                    co = servers[ms]._coalescer
                    c0 = co.calls if co is not None else 0
                    wall, lat = leg(servers[ms], n, args.requests)
                    acc[ms]["wall"] += wall
                    acc[ms]["lat"] += lat
                    acc[ms]["calls"] += (co.calls - c0) if co is not None else len(lat)
            for ms in settings:
                a = acc[ms]
                lat = np.asarray(a["lat"]) * 1e3
                row = dict(clients=n, coalesce_ms=ms, requests=len(lat), chunks_per_s=len(lat) / a["wall"], p50_ms=float(np.percentile(lat, 50)),
                           p95_ms=float(np.percentile(lat, 95)), mean_batch=len(lat) / max(a["calls"], 1))
                rows.append(row)
                print(json.dumps(row), flush=True)
    finally:
        for s in servers.values():
            s.close()
    summary = dict(metric="OpenVLAServer.act chunks/s, closed-loop clients, OpenVLA-7B shapes (synthetic weights), L1 head, graph replay")
    for n in sorted({r["clients"] for r in rows}):
        base = next((r for r in rows if r["clients"] == n and r["coalesce_ms"] == 0), None)
        for r in rows:
            if base is not None and r["clients"] == n and r["coalesce_ms"] > 0:
                summary[f"n{n}_ms{r['coalesce_ms']:g}_over_uncoalesced"] = r["chunks_per_s"] / base["chunks_per_s"]
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
