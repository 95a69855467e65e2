"""Request coalescing for the `/act` server: independent callers that arrive within a short window share one batched forward.

`RequestCoalescer` knows nothing about the model (standard library only): it is built on an injected
`batch_fn(items, pad_to) -> results`, which must return one result per item, in order.  `pad_to` is the bucket (the smallest of
`buckets` that holds the group) the batch function should run its forward at; the padding itself is the batch function's business
(`predict_action_batch(pad_to=...)` repeats observation 0 on the device side) -- repeating an ITEM here instead would push a request's
host-side preparation through twice, and `get_vla_action_batch` normalises `obs["state"]` in place.

One worker thread owns every call of `batch_fn`, so a non-re-entrant engine needs no lock:
  * `submit(item)` enqueues and blocks the caller on its own future;
  * the worker takes the oldest request and collects more until `max_batch` are there or `coalesce_ms` have passed since that oldest
    request was ENQUEUED (time spent queueing behind the previous forward counts: under load the next group leaves at once);
  * if `batch_fn` raises for a coalesced group, its members are re-run one by one, so only the offenders get the exception and a member
    that succeeds alone gets its normal result;
  * `submit_group(items)` (a pre-formed batch, `/act_batch`) goes through the same worker as one call of its own and is never merged,
    split or retried: it succeeds or fails as a whole;
  * an exception that escapes the worker loop itself fails every pending future instead of leaving its caller blocked;
  * `close()` lets the worker drain what is queued, then joins it;
  * `key_fn` and `max_keys` (both or neither): a coalesced batch holds at most `max_keys` distinct `key_fn(item)` values.  Collection stops
    at the first queued request whose key would be one too many; that request stays at the head of the queue and leads the next batch, so
    the order of arrival is kept.  (The server's key is the payload's policy and the limit its number of resident adapter slots: a batch then
    never needs a second forward pass.)  Pre-formed groups are not examined.
"""
from __future__ import annotations

import collections
import threading
import time
from concurrent.futures import Future
from typing import Any, Callable, List, Optional, Sequence


class _Entry:
    __slots__ = ("items", "group", "future", "t")

    def __init__(self, items, group):
        self.items, self.group, self.future, self.t = items, group, Future(), time.monotonic()


class RequestCoalescer:
    def __init__(self, batch_fn: Callable[[List[Any], Optional[int]], Sequence[Any]], *, coalesce_ms: float, max_batch: int = 8,
                 buckets: Sequence[int] = (1, 2, 4, 8), key_fn: Optional[Callable[[Any], Any]] = None, max_keys: Optional[int] = None):
        if (key_fn is None) != (max_keys is None):
            raise ValueError("RequestCoalescer: key_fn and max_keys go together")
        if max_keys is not None and max_keys < 1:
            raise ValueError("max_keys must be at least 1")
        if coalesce_ms <= 0:
            raise ValueError("RequestCoalescer needs coalesce_ms > 0 (at 0 the server does not coalesce at all)")
        if max_batch < 1:
            raise ValueError("max_batch must be at least 1")
        self.batch_fn = batch_fn
        self.window = coalesce_ms / 1000.0
        self.max_batch = int(max_batch)
        self.key_fn, self.max_keys = key_fn, max_keys
        self.buckets = tuple(sorted(int(b) for b in buckets))
        self.calls = 0                     # batch_fn invocations (statistics for tools / tests)
        self._queue = collections.deque()
        self._cv = threading.Condition()
        self._closing = False
        self._dead: Optional[BaseException] = None
        self._thread = threading.Thread(target=self._worker, name="ovla-coalescer", daemon=True)
        self._thread.start()

    # -- callers ---------------------------------------------------------------------------------------------------------------------
    def bucket(self, n: int) -> Optional[int]:
        """Smallest configured bucket that holds n items; None (run at n itself) when n is beyond the largest."""
        return next((b for b in self.buckets if b >= n), None)

    def _enqueue(self, items, group: bool) -> Future:
        e = _Entry(items, group)
        with self._cv:
            if self._dead is not None:
                raise RuntimeError("the coalescer's worker has died") from self._dead
            if self._closing:
                raise RuntimeError("the coalescer is closed")
            self._queue.append(e)
            self._cv.notify_all()
        return e.future

    def submit(self, item):
        """One request: blocks until the worker has run a batch that contains it; returns its result or raises its exception."""
        return self._enqueue([item], False).result()[0]

    def submit_group(self, items):
        """A pre-formed batch: one call of batch_fn of its own; returns the list of results or raises."""
        items = list(items)
        if not items:
            raise ValueError("submit_group: no items")
        return list(self._enqueue(items, True).result())

    def close(self, timeout: Optional[float] = None) -> None:
        with self._cv:
            self._closing = True
            self._cv.notify_all()
        self._thread.join(timeout)

    @property
    def alive(self) -> bool:
        return self._thread.is_alive()

    # -- the worker ------------------------------------------------------------------------------------------------------------------
    def _take(self) -> Optional[List[_Entry]]:
        """Blocks for the next unit of work: one pre-formed group, or up to max_batch single requests.  None: closed and drained."""
        with self._cv:
            while not self._queue and not self._closing:
                self._cv.wait()
            if not self._queue:
                return None
            taken = [self._queue.popleft()]
            if taken[0].group:
                return taken
            deadline = taken[0].t + self.window
            keys = {self.key_fn(taken[0].items[0])} if self.key_fn is not None else None
            while len(taken) < self.max_batch:
                if self._queue:
                    if self._queue[0].group:      # order of arrival is kept: the group runs next, on its own
                        break
                    if keys is not None:
                        k = self.key_fn(self._queue[0].items[0])
                        if k not in keys and len(keys) >= self.max_keys:   # one key too many: it leads the next batch
                            break
                        keys.add(k)
                    taken.append(self._queue.popleft())
                    continue
                left = deadline - time.monotonic()
                if left <= 0 or self._closing:
                    break
                self._cv.wait(left)
            return taken

    def _call(self, items):
        self.calls += 1
        results = self.batch_fn(items, self.bucket(len(items)))
        if results is None or len(results) < len(items):
            raise RuntimeError(f"batch_fn returned {0 if results is None else len(results)} results for {len(items)} items")
        return results

    def _run(self, taken: List[_Entry]) -> None:
        if taken[0].group:
            e = taken[0]
            try:
                e.future.set_result(self._call(e.items))
            except Exception as exc:  # noqa: BLE001 -- handed to the caller
                e.future.set_exception(exc)
            return
        try:
            results = self._call([e.items[0] for e in taken])
        except Exception as exc:  # noqa: BLE001
            if len(taken) == 1:
                taken[0].future.set_exception(exc)
                return
            for e in taken:           # find the offenders: everyone else still gets an answer
                try:
                    e.future.set_result([self._call(e.items)[0]])
                except Exception as exc1:  # noqa: BLE001
                    e.future.set_exception(exc1)
            return
        for e, r in zip(taken, results):
            e.future.set_result([r])

    def _worker(self) -> None:
        taken: List[_Entry] = []
        try:
            while True:
                taken = self._take() or []
                if not taken:
                    return
                self._run(taken)
                taken = []
        except BaseException as exc:  # noqa: BLE001 -- nobody may be left waiting on a future that will never complete
            with self._cv:
                self._dead = exc
                pending = taken + list(self._queue)
                self._queue.clear()
            for e in pending:
                if not e.future.done():
                    e.future.set_exception(RuntimeError(f"the coalescer's worker died: {exc!r}"))
