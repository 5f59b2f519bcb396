"""The query coalescer with filtered requests (service/optimized_vector_store.py _QueryCoalescer
``query(q, k, filt)``): a batch holds one k class and one kind -- only unfiltered requests, run as
``run(Q, k)`` exactly as before, or only filtered ones, run as ``run(Q, k, filters)`` with each
request's filter in order.  Host logic only (a fake batched search); no test sleeps for a result:
the fake search blocks on an event the test sets."""
import threading

import numpy as np
import pytest

from service.optimized_vector_store import _QueryCoalescer


class _Gate:
    """A fake batched search whose first call blocks until released: the requests that arrive
    meanwhile queue up, so the batches after it are formed from a known pending list."""

    def __init__(self, fail_filtered=False):
        self.calls = []          # (args count, first column of Q, k, filters or None)
        self.entered = threading.Event()
        self.release = threading.Event()
        self.fail_filtered = fail_filtered

    def __call__(self, *args):
        Q, k = args[0], args[1]
        filters = args[2] if len(args) > 2 else None
        first = not self.calls
        self.calls.append((len(args), [int(q[0]) for q in Q], k, filters))
        if first:
            self.entered.set()
            assert self.release.wait(30)
        if filters is not None and self.fail_filtered:
            raise ValueError("device said no")
        out = []
        for j, q in enumerate(Q):
            tag = 0 if filters is None else filters[j]["t"]
            ix = [int(q[0]) * 1000 + tag * 100 + e for e in range(k)]
            out.append((ix, [float(-e) for e in range(k)], [{"id": i} for i in ix]))
        return out


def _queue(co, gate, reqs):
    """Block the coalescer's only slot with one opening request, queue ``reqs`` behind it in order
    (each (key, k, filt)), release.  Returns {key: result or exception}."""
    res = {}

    def worker(key, k, filt):
        try:
            q = np.array([key, 0.0], np.float32)
            res[key] = co.query(q, k) if filt is None else co.query(q, k, filt)
        except BaseException as e:  # noqa: BLE001
            res[key] = e

    opener = threading.Thread(target=worker, args=(999, 1, None), daemon=True)
    opener.start()
    threads = []
    try:
        assert gate.entered.wait(30)
        for key, k, filt in reqs:
            th = threading.Thread(target=worker, args=(key, k, filt), daemon=True)
            th.start()
            threads.append(th)
            # FIFO: each request is pending before the next one is sent.  A request that ends
            # instead of queueing (a coalescer that does not take a filter raises at once) is a
            # failure, never a wait.
            while True:
                with co._cv:
                    if len(co._pending) == len(threads):
                        break
                if not th.is_alive():
                    th.join()
                    raise AssertionError(f"request {key} ended without queueing: {res.get(key)!r}")
    finally:
        gate.release.set()  # whatever happened, nothing stays blocked in the fake search
    for th in [opener] + threads:
        th.join(timeout=30)
        assert not th.is_alive()
    return res


def test_kinds_never_share_a_batch_and_fifo_holds():
    gate = _Gate()
    co = _QueryCoalescer(gate, max_inflight=1)
    reqs = [(1, 3, None), (2, 3, {"t": 1}), (3, 2, None), (4, 5, {"t": 2}), (5, 4, {"t": 1}), (6, 1, None)]
    res = _queue(co, gate, reqs)
    # the opener alone, then the oldest pending request's kind: unfiltered 1, 3, 6, then filtered 2, 4, 5
    assert gate.calls[0] == (2, [999], 1, None)
    assert gate.calls[1] == (2, [1, 3, 6], 3, None)                       # two arguments, as before
    assert gate.calls[2] == (3, [2, 4, 5], 5, [{"t": 1}, {"t": 2}, {"t": 1}])  # each request's filter, in order
    assert len(gate.calls) == 3
    for key, k, filt in reqs:
        tag = 0 if filt is None else filt["t"]
        ix, sc, md = res[key]
        assert ix == [key * 1000 + tag * 100 + e for e in range(k)] and len(sc) == k and len(md) == k
    assert co.batches == 3 and co.queries == 7 and co._pending == [] and co._running == 0


def test_filtered_first_when_it_is_the_oldest():
    gate = _Gate()
    co = _QueryCoalescer(gate, max_inflight=1)
    _queue(co, gate, [(1, 2, {"t": 3}), (2, 2, None), (3, 2, {"t": 4})])
    assert [c[1] for c in gate.calls] == [[999], [1, 3], [2]]
    assert gate.calls[1][0] == 3 and gate.calls[1][3] == [{"t": 3}, {"t": 4}]
    assert gate.calls[2][0] == 2


def test_k_classes_still_split_within_a_kind():
    gate = _Gate()
    co = _QueryCoalescer(gate, max_inflight=1)
    _queue(co, gate, [(1, 3, {"t": 1}), (2, 40, {"t": 1}), (3, 16, {"t": 2}), (4, 250, {"t": 1}), (5, 200, {"t": 2})])
    assert [(c[1], c[2]) for c in gate.calls[1:]] == [([1, 3], 16), ([2, 5], 200), ([4], 250)]
    assert all(c[0] == 3 for c in gate.calls[1:])


def test_max_batch_counts_within_a_kind():
    gate = _Gate()
    co = _QueryCoalescer(gate, max_batch=2, max_inflight=1)
    _queue(co, gate, [(1, 1, {"t": 1}), (2, 1, None), (3, 1, {"t": 1}), (4, 1, {"t": 1})])
    assert [c[1] for c in gate.calls[1:]] == [[1, 3], [2], [4]]


def test_an_exception_reaches_every_caller_of_its_batch_only():
    gate = _Gate(fail_filtered=True)
    co = _QueryCoalescer(gate, max_inflight=1)
    res = _queue(co, gate, [(1, 2, {"t": 1}), (2, 2, None), (3, 2, {"t": 2})])
    assert isinstance(res[1], ValueError) and isinstance(res[3], ValueError) and str(res[1]) == "device said no"
    assert res[2][0] == [2000, 2001] and res[999][0] == [999000]
    # usable afterwards
    gate.fail_filtered = False
    assert co.query(np.array([7, 0], np.float32), 1, {"t": 5})[0] == [7500]


@pytest.mark.parametrize("filt", [None, {"t": 1}])
def test_a_lone_request_runs_at_once(filt):
    gate = _Gate()
    gate.release.set()
    co = _QueryCoalescer(gate)
    q = np.array([4, 0], np.float32)
    ix = (co.query(q, 2) if filt is None else co.query(q, 2, filt))[0]
    assert ix == ([4000, 4001] if filt is None else [4100, 4101])
    assert gate.calls == [(2 if filt is None else 3, [4], 2, None if filt is None else [filt])]
