"""RequestCoalescer (vla_scripts/coalescer.py) on a fake batch function: grouping, the window, max_batch, bucket padding, failure isolation,
close(); and that a server at coalesce_ms = 0 has no coalescer.  No GPU, no library, no HTTP."""
import importlib
import threading
import time
import types

import pytest

load = importlib.import_module
WINDOW_MS = 150.0   # wide enough that eight threads started back to back land inside it on a loaded machine


@pytest.fixture(scope="module")
def co(pkg):
    return load("openvla-oft_amd.vla_scripts.coalescer")


class Recorder:
    """batch_fn: result = ("r", item); remembers every call as (items, pad_to)."""

    def __init__(self, poison=None, delay=0.0):
        self.calls, self.poison, self.delay = [], poison, delay

    def __call__(self, items, pad_to):
        self.calls.append((list(items), pad_to))
        if self.delay:
            time.sleep(self.delay)
        if self.poison is not None and self.poison in items:
            raise ValueError(f"poisoned item {self.poison}")
        return [("r", i) for i in items]


def _submit_all(c, items):
    """Submits every item from its own thread (all released together); returns {item: result or the exception}."""
    out, gate = {}, threading.Barrier(len(items))

    def one(i):
        gate.wait()
        try:
            out[i] = c.submit(i)
        except Exception as exc:  # noqa: BLE001
            out[i] = exc

    threads = [threading.Thread(target=one, args=(i,)) for i in items]
    for t in threads:
        t.start()
    for t in threads:
        t.join(10)
    assert not any(t.is_alive() for t in threads)
    return out


def test_eight_requests_inside_the_window_make_one_call(co):
    fn = Recorder()
    c = co.RequestCoalescer(fn, coalesce_ms=WINDOW_MS, max_batch=8)
    try:
        out = _submit_all(c, list(range(8)))
    finally:
        c.close()
    assert len(fn.calls) == 1 and sorted(fn.calls[0][0]) == list(range(8)) and fn.calls[0][1] == 8
    assert out == {i: ("r", i) for i in range(8)}, "each caller gets its own result"


def test_a_lone_request_leaves_after_the_window(co):
    fn = Recorder()
    c = co.RequestCoalescer(fn, coalesce_ms=40.0, max_batch=8)
    try:
        t0 = time.monotonic()
        assert c.submit("a") == ("r", "a")
        dt = time.monotonic() - t0
    finally:
        c.close()
    assert fn.calls == [(["a"], 1)]
    assert 0.035 <= dt < 2.0, f"held for {dt * 1e3:.1f} ms: the window is 40 ms, and it must not wait for max_batch"


def test_nine_requests_with_max_batch_eight_make_two_calls(co):
    fn = Recorder()
    c = co.RequestCoalescer(fn, coalesce_ms=WINDOW_MS, max_batch=8)
    try:
        out = _submit_all(c, list(range(9)))
    finally:
        c.close()
    assert sorted(len(items) for items, _ in fn.calls) == [1, 8]
    assert sorted(i for items, _ in fn.calls for i in items) == list(range(9))
    assert out == {i: ("r", i) for i in range(9)}


def test_three_items_run_as_a_bucket_of_four(co):
    fn = Recorder()
    c = co.RequestCoalescer(fn, coalesce_ms=WINDOW_MS, max_batch=8, buckets=(1, 2, 4, 8))
    try:
        out = _submit_all(c, ["a", "b", "c"])
        assert c.submit_group(["x", "y", "z", "u", "v"]) == [("r", i) for i in "xyzuv"]   # a pre-formed group: one call, bucket 8
    finally:
        c.close()
    assert len(fn.calls) == 2
    assert sorted(fn.calls[0][0]) == ["a", "b", "c"] and fn.calls[0][1] == 4, "three real items, presented at the bucket of 4"
    assert out == {i: ("r", i) for i in "abc"}, "three results"
    assert fn.calls[1] == (list("xyzuv"), 8)
    assert [c.bucket(n) for n in (1, 2, 3, 4, 5, 8, 9)] == [1, 2, 4, 4, 8, 8, None]


def test_a_poisoned_item_fails_its_own_caller_only(co):
    fn = Recorder(poison=2)
    c = co.RequestCoalescer(fn, coalesce_ms=WINDOW_MS, max_batch=8)
    try:
        out = _submit_all(c, [0, 1, 2, 3])
    finally:
        c.close()
    assert isinstance(out[2], ValueError)
    assert {i: out[i] for i in (0, 1, 3)} == {i: ("r", i) for i in (0, 1, 3)}
    assert len(fn.calls) == 5 and [len(items) for items, _ in fn.calls[1:]] == [1, 1, 1, 1], "one merged call, then the members one by one"


def test_a_worker_level_exception_fails_the_pending_futures(co):
    class Fatal(BaseException):
        pass

    def fn(items, pad_to):
        raise Fatal("not an ordinary error")

    c = co.RequestCoalescer(fn, coalesce_ms=20.0, max_batch=2)
    out = _submit_all(c, [0, 1, 2])       # nobody hangs (the helper joins with a timeout and asserts)
    assert all(isinstance(v, RuntimeError) for v in out.values())
    c.close(5)
    assert not c.alive
    with pytest.raises(RuntimeError):
        c.submit(3)


def test_close_with_pending_work_drains_and_joins(co):
    fn = Recorder(delay=0.05)
    c = co.RequestCoalescer(fn, coalesce_ms=10.0, max_batch=2)
    out = {}
    threads = [threading.Thread(target=lambda i=i: out.__setitem__(i, c.submit(i))) for i in range(6)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + 5
    while sum(len(items) for items, _ in fn.calls) + len(c._queue) < 6 and time.monotonic() < deadline:
        time.sleep(0.001)               # until all six are queued or running
    c.close(10)
    for t in threads:
        t.join(10)
    assert not c.alive and not any(t.is_alive() for t in threads)
    assert out == {i: ("r", i) for i in range(6)}, "queued work is finished, not dropped"
    assert not [t for t in threading.enumerate() if t.name == "ovla-coalescer"]
    with pytest.raises(RuntimeError):
        c.submit(7)


def test_server_without_coalescing_builds_no_coalescer(pkg, monkeypatch):
    dep = load("openvla-oft_amd.vla_scripts.deploy")
    built = []
    monkeypatch.setattr(dep, "RequestCoalescer", lambda *a, **k: built.append((a, k)) or types.SimpleNamespace(close=lambda: None))
    vla = types.SimpleNamespace(norm_stats={"k": {}}, llm_dim=8, enable_graph_replay=lambda on=True: None)
    mk = lambda **kw: dep.OpenVLAServer(dep.DeployConfig(unnorm_key="k", use_proprio=False, **kw), vla=vla, processor=object(),  # noqa: E731
                                        action_head=object())
    cfg = dep.DeployConfig()
    assert cfg.coalesce_ms == 0.0 and cfg.max_batch == 8 and tuple(cfg.batch_buckets) == (1, 2, 4, 8)
    server = mk()
    assert server._coalescer is None and not built
    server.close()                       # a no-op
    assert mk(coalesce_ms=5.0, max_batch=4)._coalescer is not None and len(built) == 1
    assert built[0][1]["coalesce_ms"] == 5.0 and built[0][1]["max_batch"] == 4 and tuple(built[0][1]["buckets"]) == (1, 2, 4, 8)


# ---- server level, on the CPU: the real get_vla_action_batch (which normalises obs["state"] in place) over a fake model -------------------------
POISON = 666


class FakeVLA:
    """Records the proprio every forward receives; the forward fails when a prompt carries the POISON token.  actions[b] = proprio[b, 0]."""

    def __init__(self):
        bounds = {"q01": [0.0] * 8, "q99": [4.0] * 8, "min": [0.0] * 8, "max": [4.0] * 8}
        self.norm_stats = {"k": {"proprio": bounds}}
        self.llm_dim, self.max_batch_graphs, self.seen = 8, 8, []
        self.config = types.SimpleNamespace(image_sizes=[224, 224])

    def enable_graph_replay(self, on=True):
        return self

    def predict_action_batch(self, batch, pixel_values, unnorm_key=None, proprio=None, pad_to=None, **kw):
        import numpy as np

        self.seen.append((len(batch), np.array(proprio, dtype=np.float64), pad_to))
        if any(POISON in ids.tolist() for ids, _ in batch):
            raise RuntimeError("the forward failed")
        return np.stack([np.full((8, 7), p[0]) for p in proprio]), None


def _fake_processor(text, image):
    import torch

    ids = torch.tensor([1, POISON if "poison" in text else 5])
    return {"input_ids": ids, "attention_mask": torch.ones_like(ids), "pixel_values": torch.zeros(1, 6, 2, 2)}


def test_a_retried_member_is_not_normalised_twice(pkg):
    """get_vla_action_batch rewrites obs["state"] with its normalised value before the forward can fail.  When a coalesced forward fails
    and its members are re-run one by one, the good member's forward must see its state normalised ONCE (1.0 -> -0.5 under bounds [0, 4]; a
    second pass would give -1.0), and its answer must be /act_batch([payload])'s of an uncoalesced server."""
    import numpy as np

    dep = load("openvla-oft_amd.vla_scripts.deploy")
    image = np.zeros((224, 224, 3), dtype=np.uint8)
    mk = lambda text, state: dep._encode({"full_image": image, "state": state, "instruction": text})  # noqa: E731
    good, bad = mk("open the drawer", np.full(8, 1.0)), mk("poison", np.full(8, 2.0))
    kw = dict(unnorm_key="k", use_proprio=True, center_crop=False, num_images_in_input=1, num_open_loop_steps=8)
    serve = lambda vla, **c: dep.OpenVLAServer(dep.DeployConfig(**kw, **c), vla=vla, processor=_fake_processor, action_head=object(),  # noqa: E731
                                               proprio_projector=object())
    want = serve(FakeVLA()).act_batch([good])[0]
    assert np.allclose(dep._decode(want)[0], -0.5, rtol=0, atol=1e-6)   # (the reference's 1e-8 in the denominator: not exactly -0.5)
    vla = FakeVLA()
    server = serve(vla, coalesce_ms=WINDOW_MS)
    assert vla.max_batch_graphs == 16, "room for four text-length buckets per batch bucket"
    got, gate = {}, threading.Barrier(2)

    def client(name, payload):
        gate.wait()
        got[name] = server.act(payload)

    threads = [threading.Thread(target=client, args=a) for a in (("good", good), ("bad", bad))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(10)
    assert not any(t.is_alive() for t in threads)
    # a state of the wrong length is refused on the request thread and never reaches a forward
    n_forwards = len(vla.seen)
    assert server.act(mk("open the drawer", np.full(7, 1.0))) == "error"
    assert server.act_batch([good, mk("open the drawer", np.ones((2, 4)))]) == "error"
    assert len(vla.seen) == n_forwards
    server.close()
    assert got["bad"] == "error"
    assert [n for n, _, _ in vla.seen] == [2, 1, 1] and vla.seen[0][2] == 2, "one merged forward that failed, then the members one by one"
    for n, proprio, _ in vla.seen:
        assert np.all(np.minimum(np.abs(proprio + 0.5), np.abs(proprio)) < 1e-6), f"a state went through the normalisation twice: {proprio}"
    assert isinstance(got["good"], list) and all(np.array_equal(dep._decode(a), dep._decode(b)) for a, b in zip(got["good"], want))
