"""The policy pool's host logic, without a GPU: the residency planner (policy_pool.plan_loads / Residency / split_passes) and the coalescer's
batches of at most `max_keys` distinct keys (RequestCoalescer(key_fn=, max_keys=)) on a fake batch function."""
import importlib
import threading

import pytest

load = importlib.import_module


@pytest.fixture(scope="module")
def pp(pkg):
    return load("openvla-oft_amd.policy_pool")


@pytest.fixture(scope="module")
def co(pkg):
    return load("openvla-oft_amd.vla_scripts.coalescer")


# ======================================================================================================================
# planner
# ======================================================================================================================
def _run(st, needed):
    loads = st.plan(needed)
    return loads, st.commit(loads, needed)


def test_residents_needed_by_the_batch_never_move(pp):
    st = pp.Residency(4)
    loads, slot_of = _run(st, ["x", "y", "z", "u"])
    assert loads == [(0, "x"), (1, "y"), (2, "z"), (3, "u")] and slot_of == {"x": 0, "y": 1, "z": 2, "u": 3}
    # v and w replace the two residents the batch does not need; x and y stay where they are, whatever their order in the batch
    loads, slot_of = _run(st, ["v", "y", "w", "x"])
    assert sorted(s for s, _ in loads) == [2, 3] and [n for _, n in loads] == ["v", "w"]
    assert slot_of["x"] == 0 and slot_of["y"] == 1 and st.names[:2] == ["x", "y"]
    assert pp.plan_loads(["a", "b"], [5, 9], ["b", "a"]) == []


def test_lru_eviction_and_the_lowest_slot_tie_rule(pp):
    # empty slots are older than any used one; among them the lowest goes first
    assert pp.plan_loads([None, None, None, None], [-1] * 4, ["p"]) == [(0, "p")]
    assert pp.plan_loads([None, "a", None, "b"], [-1, 3, -1, 1], ["p", "q", "r"]) == [(0, "p"), (2, "q"), (3, "r")]
    # least recently used first; equal ticks (slots last needed by the same batch): the lowest slot
    assert pp.plan_loads(["a", "b", "c", "d"], [4, 2, 3, 2], ["p"]) == [(1, "p")]
    assert pp.plan_loads(["a", "b", "c", "d"], [4, 2, 3, 2], ["p", "q", "r"]) == [(1, "p"), (3, "q"), (2, "r")]
    # a needed resident is no candidate however old it is
    assert pp.plan_loads(["a", "b", "c", "d"], [1, 2, 3, 4], ["a", "p"]) == [(1, "p")]
    st = pp.Residency(2)
    _run(st, ["a", "b"])
    _run(st, ["a"])                          # b is now the older one
    assert st.plan(["c"]) == [(1, "c")]
    # deterministic: the same inputs, the same plan
    args = (["a", None, "c", "d"], [7, -1, 7, 2], ["x", "y", "c"])
    assert pp.plan_loads(*args) == pp.plan_loads(*args) == [(1, "x"), (3, "y")]


def test_repeated_identical_batches_load_nothing(pp):
    st = pp.Residency(4)
    assert len(_run(st, ["x", "y", "z"])[0]) == 3
    for _ in range(3):
        assert _run(st, ["x", "y", "z"])[0] == [] and _run(st, ["z", "x"])[0] == []
    assert st.stats == dict(loads=3, hits=3 * 3 + 3 * 2, passes=7)


def test_the_rotation_of_the_gpu_test(pp):
    """{x,y,z,u}, {v,w,x,y}, {z,u,v,w}, {x,y,z,u} at four slots: 4 + 2 + 2 + 2 loads, residents never reloaded."""
    st = pp.Residency(4)
    counts = [len(_run(st, list(b))[0]) for b in ("xyzu", "vwxy", "zuvw", "xyzu")]
    assert counts == [4, 2, 2, 2] and st.stats == dict(loads=10, hits=6, passes=4)


def test_more_than_resident_distinct_policies_raises(pp):
    st = pp.Residency(2)
    with pytest.raises(ValueError, match="3 distinct policies for 2 resident slots"):
        st.plan(["a", "b", "c"])
    with pytest.raises(ValueError, match="not distinct"):
        st.plan(["a", "a"])
    with pytest.raises(ValueError):
        pp.Residency(0)
    assert pp.split_passes(list("abacbdae"), 2) == [["a", "b"], ["c", "d"], ["e"]]
    assert pp.split_passes(["a", "a"], 4) == [["a"]]


def test_a_removed_names_slot_is_never_a_hit(pp):
    st = pp.Residency(2)
    _run(st, ["x", "y"])
    assert st.invalidate("x") == 0 and st.names == [None, "y"] and st.invalidate("nobody") is None
    # the same name registered again (with other tensors): it has to be loaded, and the emptied slot is the first to be refilled
    hits = st.stats["hits"]
    loads, slot_of = _run(st, ["x"])
    assert loads == [(0, "x")] and slot_of == {"x": 0} and st.stats["hits"] == hits
    st.invalidate("y")
    assert st.plan(["z"]) == [(1, "z")], "the emptied slot goes before the least recently used one"


# ======================================================================================================================
# coalescer
# ======================================================================================================================
class Recorder:
    """batch_fn: result = ("r", item).  The first call (the plug) blocks until `release` is set, so that the test can queue its arrivals in a
    known order behind it: the worker then finds them all queued and no timing enters the batches."""

    def __init__(self):
        self.calls, self.entered, self.release = [], threading.Event(), threading.Event()

    def __call__(self, items, pad_to):
        self.calls.append((list(items), pad_to))
        if len(self.calls) == 1:
            self.entered.set()
            assert self.release.wait(10)
        return [("r", i) for i in items]


def _batches(co, arrivals, **kw):
    """The batches the coalescer forms for `arrivals` (queued in that order while the worker is busy), and each arrival's result in order."""
    fn = Recorder()
    c = co.RequestCoalescer(fn, coalesce_ms=1.0, max_batch=4, **kw)
    try:
        plug = c._enqueue([("plug", -1)], False)
        assert fn.entered.wait(10)
        futures = [c._enqueue([a], False) for a in arrivals]
        fn.release.set()
        results = [f.result(10)[0] for f in futures]
        assert plug.result(10) == [("r", ("plug", -1))]
    finally:
        c.close(10)
    return [items for items, _ in fn.calls[1:]], results


ARRIVALS = [(k, i) for i, k in enumerate("aabcacbbbdda")]


def test_no_batch_has_more_than_two_keys_and_order_is_kept(co):
    batches, results = _batches(co, ARRIVALS, key_fn=lambda item: item[0], max_keys=2)
    assert results == [("r", a) for a in ARRIVALS], "every caller gets its own result"
    assert [a for b in batches for a in b] == ARRIVALS, "arrival order is kept across the batches"
    assert all(len({k for k, _ in b}) <= 2 and len(b) <= 4 for b in batches)
    # a a b | c a c b -> stops at c (third key); c a c | b: b would be the third key; b b b d (max_batch); d a
    assert [[k for k, _ in b] for b in batches] == [list("aab"), list("cac"), list("bbbd"), list("da")]
    # the request that did not fit leads the next batch
    assert [b[0] for b in batches[1:]] == [ARRIVALS[3], ARRIVALS[6], ARRIVALS[10]]


def test_defaults_form_the_batches_they_always_formed(co):
    batches, results = _batches(co, ARRIVALS)
    assert batches == [ARRIVALS[i:i + 4] for i in range(0, len(ARRIVALS), 4)], "without key_fn / max_keys: max_batch alone cuts the queue"
    assert results == [("r", a) for a in ARRIVALS]
    keyed_wide, _ = _batches(co, ARRIVALS, key_fn=lambda item: item[0], max_keys=4)
    assert keyed_wide == batches, "a limit that max_batch already implies changes nothing"
    with pytest.raises(ValueError, match="go together"):
        co.RequestCoalescer(lambda items, pad_to: items, coalesce_ms=1.0, key_fn=lambda i: i)
    with pytest.raises(ValueError, match="go together"):
        co.RequestCoalescer(lambda items, pad_to: items, coalesce_ms=1.0, max_keys=2)


def test_server_config_defaults(pkg):
    dep = load("openvla-oft_amd.vla_scripts.deploy")
    assert dep.DeployConfig().resident_policies == 0
