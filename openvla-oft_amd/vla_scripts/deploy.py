"""vla-scripts/deploy.py of the reference on the HIP engine: a FastAPI server whose `/act` endpoint maps
{observation images, state, "instruction"} to an action chunk (deploy.py:47-107).

Differences, all deliberate:
  * the reference guards nothing: `get_server_action` runs in FastAPI's thread pool with no lock around the model (deploy.py:78-107).
    One GPU engine with static hipGraph input buffers is not re-entrant, so requests are serialised by a lock here;
  * `json_numpy` (the reference's wire codec, absent from this image: PARITY UNPINNED) is restated in `encode_ndarray` /
    `decode_payload`: an ndarray travels as {"__numpy__": base64(raw bytes), "dtype": numpy descr string, "shape": [...]};
    the "encoded" double-encoding of deploy.py:80-95 (whole payload as ONE json string under the key "encoded") is kept;
  * components can be handed in already built (tests; no checkpoint exists offline), otherwise they are loaded exactly like the
    reference does (get_vla / get_action_head / get_proprio_projector / get_processor);
  * merged LoRA weights + hipGraph replay are switched on (`vla.enable_graph_replay()`): the deployment configuration of DESIGN.md §6,
    for the diffusion head too (its DDIM loop replays from engine.DiffusionGraph);
  * the reference's server never hands the noisy-action projector to `get_vla_action`, so its diffusion configuration cannot sample; here
    the projector is a component like the action head (handed in, or loaded with get_noisy_action_projector) and is passed on;
  * `coalesce_ms > 0` (not in the reference): independent `/act` callers that arrive within that window share ONE batched forward
    (`RequestCoalescer` -> `get_vla_action_batch`, padded to a bucket of `batch_buckets`).  Batch invariance is what makes that safe: a
    coalesced `/act` answer is bit-identical to `/act_batch([payload])` -- the fixed-schedule batch path at B = 1 -- whatever it was merged
    with.  It is NOT promised identical to the uncoalesced `/act`, which runs `predict_action` on the planner's schedules and is
    unchanged.  At `coalesce_ms == 0` (the default) no coalescer exists and both endpoints behave exactly as before.
  * `policies={name: fine-tune output directory | dict of add_policy arguments}` (not in the reference): one BASE model serves several
    fine-tuned policies.  A payload then names its policy under the key "policy"; requests of different policies share one batched forward
    (every policy's adapters ride in the same launches: OpenVLAForActionPrediction.add_policy / predict_action_batch(policy=...)), coalesced
    or not.  The coalescer knows nothing of it: the name travels inside the item.  An unknown or missing name answers "error" like any
    malformed payload.  With no policies configured a payload without "policy" is served exactly as before.
  * `resident_policies > 0` (not in the reference): the policies go into the model's policy pool (enable_policy_pool) -- any number of them
    registered, `resident_policies` (1 .. 4) in the adapter slots at a time, swapped in by one copy launch each just before a forward that
    needs them.  The coalescer then forms batches of at most that many distinct policies (key_fn / max_keys), so a coalesced forward never
    splits; an `/act_batch` group that names more is split into passes by predict_action_batch.  At 0 (the default) nothing changes: at most
    4 policies, registered once.
  * `policies` with `use_film` (not in the reference): the base model is built with use_film="per_policy" (get_vla(cfg, film_per_policy=True)) -- or
    handed in built that way -- and every policy brings its own FiLM scale / shift Linears (get_policy reads them from the fine-tune's
    vision-backbone checkpoint; a dict spec passes `film=`).  Payloads name their policy as above; one routed launch per forward gives each
    observation its own policy's FiLM.
"""
from __future__ import annotations

import base64
import json
import logging
import threading
import traceback
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Union

import numpy as np

from ..experiments.robot import openvla_utils as U
from ..prismatic.vla import constants as C
from .coalescer import RequestCoalescer


def encode_ndarray(a: np.ndarray) -> Dict[str, Any]:
    a = np.ascontiguousarray(a)
    return {"__numpy__": base64.b64encode(a.tobytes()).decode("ascii"), "dtype": np.lib.format.dtype_to_descr(a.dtype), "shape": list(a.shape)}


def _decode(obj):
    if isinstance(obj, dict):
        if "__numpy__" in obj:
            dt = np.lib.format.descr_to_dtype(obj["dtype"])
            return np.frombuffer(base64.b64decode(obj["__numpy__"]), dtype=dt).reshape(obj["shape"]).copy()
        return {k: _decode(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_decode(v) for v in obj]
    return obj


def _encode(obj):
    if isinstance(obj, np.ndarray):
        return encode_ndarray(obj)
    if isinstance(obj, (np.floating, np.integer)):
        return obj.item()
    if isinstance(obj, dict):
        return {k: _encode(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_encode(v) for v in obj]
    return obj


def decode_payload(payload: Dict[str, Any]):
    """-> (observation dict with ndarrays, double_encoded flag).  deploy.py:80-86."""
    double = "encoded" in payload
    if double:
        assert len(payload.keys()) == 1, "Only uses encoded payload!"
        payload = json.loads(payload["encoded"])
    return _decode(payload), double


@dataclass
class DeployConfig:
    # fmt: off
    host: str = "0.0.0.0"
    port: int = 8777
    model_family: str = "openvla"
    pretrained_checkpoint: Union[str, Path] = ""
    use_l1_regression: bool = True
    use_diffusion: bool = False
    num_diffusion_steps: int = 50
    use_film: bool = False
    num_images_in_input: int = 3
    use_proprio: bool = True
    center_crop: bool = True
    num_open_loop_steps: int = 25
    unnorm_key: Union[str, Path] = ""
    use_relative_actions: bool = False
    load_in_8bit: bool = False
    load_in_4bit: bool = False
    seed: int = 7
    graph_replay: bool = True           # hipGraph replay of predict_action (not in the reference)
    coalesce_ms: float = 0.0            # > 0: merge /act requests that arrive within this window into one batched forward (not in the reference)
    max_batch: int = 8                  # most requests merged into one forward
    batch_buckets: tuple = (1, 2, 4, 8)  # a merged batch runs at the smallest of these that holds it: bounds the number of captured graphs
    resident_policies: int = 0          # > 0: `policies` go into a policy pool with this many adapter slots (any number of policies; not in the reference)
    # fmt: on


class OpenVLAServer:
    def __init__(self, cfg, *, vla=None, processor=None, action_head=None, proprio_projector=None, noisy_action_projector=None, policies=None):
        self.cfg = cfg
        self.policies = tuple(policies) if policies else ()
        film_policies = bool(self.policies) and bool(getattr(cfg, "use_film", False))   # every policy brings its own FiLM Linears
        self.vla = vla if vla is not None else U.get_vla(cfg, film_per_policy=film_policies)
        if film_policies and not getattr(self.vla, "film_per_policy", False):
            raise ValueError("OpenVLAServer(policies=...) with cfg.use_film needs a base model built with use_film=\"per_policy\" "
                             "(a model with its own FiLM Linears serves one policy)")
        resident = int(getattr(cfg, "resident_policies", 0) or 0)
        if resident > 0 and not getattr(self.vla, "policy_pool_resident", 0):
            self.vla.enable_policy_pool(resident)   # before the first add_policy: the slot count is fixed from there on
        resident = getattr(self.vla, "policy_pool_resident", 0) if resident > 0 else 0   # a model handed in with its pool keeps its own slot count
        for name, spec in (policies or {}).items():   # head, proprio projector and statistics come with each policy
            if name in self.vla.policies:
                continue
            if isinstance(spec, dict):
                self.vla.add_policy(name, **spec)
            else:
                U.get_policy(cfg, self.vla, name, spec)
        self.proprio_projector = proprio_projector
        if self.proprio_projector is None and cfg.use_proprio and not self.policies:
            self.proprio_projector = U.get_proprio_projector(cfg, self.vla.llm_dim, C.PROPRIO_DIM)
        self.action_head = action_head
        if self.action_head is None and (cfg.use_l1_regression or cfg.use_diffusion) and not self.policies:
            self.action_head = U.get_action_head(cfg, self.vla.llm_dim)
        self.noisy_action_projector = noisy_action_projector
        if self.noisy_action_projector is None and cfg.use_diffusion and not self.policies:
            self.noisy_action_projector = U.get_noisy_action_projector(cfg, self.vla.llm_dim)
        if self.policies:
            if action_head is not None or proprio_projector is not None or noisy_action_projector is not None:
                raise ValueError("OpenVLAServer(policies=...): heads and projectors come with each policy")
            for name in self.policies:
                assert cfg.unnorm_key in self._norm_stats(name), f"Action un-norm key {cfg.unnorm_key} not found in the `norm_stats` of policy {name}!"
        else:
            assert cfg.unnorm_key in self.vla.norm_stats, f"Action un-norm key {cfg.unnorm_key} not found in VLA `norm_stats`!"
        self.processor = processor if processor is not None else U.get_processor(cfg)
        if getattr(cfg, "graph_replay", True):   # every head, the diffusion sampler included (engine.DiffusionGraph)
            self.vla.enable_graph_replay(True)
        self._lock = threading.Lock()
        self._coalescer = None
        if getattr(cfg, "coalesce_ms", 0.0) > 0:
            buckets = tuple(getattr(cfg, "batch_buckets", (1, 2, 4, 8)))
            # one captured graph per (batch bucket, 8-token text-length bucket): room for 4 text buckets per batch bucket before the least
            # recently used graph is evicted and recaptured (task prompts of varied length would otherwise thrash captures)
            self.vla.max_batch_graphs = max(getattr(self.vla, "max_batch_graphs", 8), 4 * len(buckets))
            keyed = dict(key_fn=lambda item: item[0].get("policy"), max_keys=resident) if resident > 0 and self.policies else {}
            self._coalescer = RequestCoalescer(self._run_batch, coalesce_ms=cfg.coalesce_ms, max_batch=getattr(cfg, "max_batch", 8), buckets=buckets, **keyed)

    # -- coalescing mode: the worker thread of self._coalescer is the only thread that touches the engine ---------------------------------
    def _norm_stats(self, policy: Optional[str]) -> dict:
        return self.vla.policy_norm_stats(policy) if policy is not None else self.vla.norm_stats

    def _policy_of(self, observation) -> Optional[str]:
        """The payload's policy name, checked against the configured set (None on a server without policies)."""
        name = observation.get("policy") if isinstance(observation, dict) else None
        if not self.policies:
            if name is not None:
                raise ValueError(f"the payload names policy {name!r} but this server has no policies configured")
            return None
        if not isinstance(name, str) or name not in self.policies:
            raise ValueError(f"the payload needs a 'policy' out of {list(self.policies)}, got {name!r}")
        return name

    def _proprio_dim(self, policy: Optional[str] = None) -> Optional[int]:
        """Length of the state vector the un-normalisation statistics are for (None: the checkpoint carries none, nothing to compare with)."""
        stats = self._norm_stats(policy).get(self.cfg.unnorm_key, {}).get("proprio")
        for k in ("q01", "min", "q99", "max"):
            if stats and k in stats:
                return len(stats[k])
        return None

    def _decode_valid(self, payload):
        """Decodes and validates one payload on the request thread, so that a malformed request never enters a batch.  The request contract
        in coalescing mode (`/act` and every element of `/act_batch`): an 'instruction' string, a 'full_image' H x W x 3 array, and with
        use_proprio a numeric 1-D 'state' of the length of the checkpoint's proprio statistics."""
        observation, double = decode_payload(payload)
        if not isinstance(observation, dict) or not isinstance(observation.get("instruction"), str):
            raise ValueError("the payload needs an 'instruction' string")
        policy = self._policy_of(observation)
        image = observation.get("full_image")
        if not isinstance(image, np.ndarray) or image.ndim != 3 or image.shape[-1] != 3:
            raise ValueError("the payload needs a 'full_image' array of shape [H, W, 3]")
        if self.cfg.use_proprio:
            if "state" not in observation:
                raise ValueError("the payload needs a 'state' array (use_proprio)")
            state = np.asarray(observation["state"])
            want = self._proprio_dim(policy)
            if state.ndim != 1 or state.dtype.kind not in "fiu" or (want is not None and state.shape[0] != want):
                raise ValueError(f"'state' must be a numeric vector of length {want}, got dtype {state.dtype} shape {state.shape}")
        return observation, double

    def _run_batch(self, items, pad_to):
        """RequestCoalescer's batch_fn: decoded (observation, double_encoded) pairs -> their encoded answers, from one forward at `pad_to`.
        Idempotent: get_vla_action_batch normalises obs["state"] IN PLACE before the forward can fail, and the coalescer re-runs the members of
        a failed batch one by one -- so it gets shallow copies, and a retried member starts from the state its caller sent."""
        observations = [dict(o) for o, _ in items]
        actions = U.get_vla_action_batch(self.cfg, self.vla, self.processor, observations, [o["instruction"] for o in observations],
                                         action_head=self.action_head, proprio_projector=self.proprio_projector,
                                         noisy_action_projector=self.noisy_action_projector, use_film=self.cfg.use_film, pad_to=pad_to,
                                         policies=[o["policy"] for o in observations] if self.policies else None)
        return [json.dumps(_encode(a)) if double else _encode(a) for a, (_, double) in zip(actions, items)]

    def close(self) -> None:
        """Drains and stops the coalescer's worker (a no-op at coalesce_ms == 0)."""
        if self._coalescer is not None:
            self._coalescer.close()

    def act(self, payload: Dict[str, Any]):
        """The body of `/act` without the HTTP layer: returns a list of actions (ndarrays), or the json_numpy-encoded string
        for a double-encoded request, or "error" (deploy.py:78-107)."""
        try:
            if self._coalescer is not None:
                return self._coalescer.submit(self._decode_valid(payload))
            observation, double = decode_payload(payload)
            instruction = observation["instruction"]
            if self._policy_of(observation) is not None:   # a policy request always takes the batch path (at B = 1): that is where the slots are routed
                with self._lock:
                    return self._run_batch([(observation, double)], None)[0]
            with self._lock:      # one engine, static graph buffers: serialise (the reference does not lock)
                action = U.get_vla_action(self.cfg, self.vla, self.processor, observation, instruction, action_head=self.action_head,
                                          proprio_projector=self.proprio_projector, noisy_action_projector=self.noisy_action_projector,
                                          use_film=self.cfg.use_film)
            return json.dumps(_encode(action)) if double else _encode(action)
        except Exception:  # noqa: BLE001 -- the reference answers "error" to any malformed request
            logging.error(traceback.format_exc())
            logging.warning("Your request threw an error; make sure your request complies with the expected format:\\n"
                            "{'observation': dict, 'instruction': str}\\n")
            return "error"

    def act_batch(self, payloads):
        """The body of `/act_batch`: a list of `/act` payloads -> the list of their action chunks, each encoded like `/act` answers it, from ONE
        batched forward (OpenVLAForActionPrediction.predict_action_batch); "error" if the request or any element of it is malformed."""
        try:
            if not isinstance(payloads, list) or not payloads:
                raise ValueError("/act_batch takes a non-empty list of observation payloads")
            if self._coalescer is not None:   # through the same worker, as one pre-formed group
                return self._coalescer.submit_group([self._decode_valid(p) for p in payloads])
            decoded = [decode_payload(p) for p in payloads]
            if any(self._policy_of(o) is not None for o, _ in decoded):
                with self._lock:
                    return self._run_batch(decoded, None)
            observations = [o for o, _ in decoded]
            instructions = [o["instruction"] for o in observations]
            with self._lock:
                actions = U.get_vla_action_batch(self.cfg, self.vla, self.processor, observations, instructions, action_head=self.action_head,
                                                 proprio_projector=self.proprio_projector, noisy_action_projector=self.noisy_action_projector,
                                                 use_film=self.cfg.use_film)
            return [json.dumps(_encode(a)) if double else _encode(a) for a, (_, double) in zip(actions, decoded)]
        except Exception:  # noqa: BLE001 -- like /act
            logging.error(traceback.format_exc())
            logging.warning("Your request threw an error; make sure your request is a list of {'observation': dict, 'instruction': str}\n")
            return "error"

    def build_app(self):
        from fastapi import FastAPI
        from fastapi.responses import JSONResponse

        app = FastAPI()

        @app.post("/act")
        def get_server_action(payload: Dict[str, Any]):
            return JSONResponse(self.act(payload))

        @app.post("/act_batch")
        def get_server_action_batch(payloads: List[Dict[str, Any]]):
            return JSONResponse(self.act_batch(payloads))

        self.app = app
        return app

    def run(self, host: str = "0.0.0.0", port: int = 8777) -> None:
        import uvicorn

        try:
            uvicorn.run(self.build_app(), host=host, port=port)
        finally:
            self.close()   # coalescing mode: requests still queued at shutdown are answered, then the worker is joined


def deploy(cfg: DeployConfig) -> None:
    OpenVLAServer(cfg).run(cfg.host, port=cfg.port)
