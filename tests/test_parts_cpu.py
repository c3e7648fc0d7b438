"""``scan.objects.run_parts`` and ``PartChain``, the part driver and the host chain of the part-wise index builds, driven
directly with plain Python jobs: which worker runs which part, the sums a part sees, and what a failing part does to
the parts that wait for it.  No device, no fake of one."""
import threading

import pytest

from dataplug_amd.scan import objects as scan_objects
from dataplug_amd.scan.objects import PartChain, run_parts

GUARD = 20.0                  # seconds a test waits for a thread before it calls the run hung: a guard, not a timing


def guarded(fn):
    """``fn()`` on a thread of its own: {"value": ...} or {"error": ...}; fails the test where the call hangs."""
    result = {}

    def call():
        try:
            result["value"] = fn()
        except BaseException as e:
            result["error"] = e

    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(GUARD)
    assert not th.is_alive(), "run_parts hangs"
    return result


def chained(devs, values, gates=None, fail=None):
    """A chained run of len(values) parts in which every part publishes its value and then asks for the sum before
    it: (chain, {k: before(k)}, result).  ``gates[k]``: the parts that must have published before part k does (a wait
    in front of its publish, so the chain's invariant holds); ``fail``: (k, exception) raised in place of k's publish."""
    chain = PartChain(len(values), "test index")
    got, lock = {}, threading.Lock()

    def job(k, _):
        for j in (gates or {}).get(k, ()):
            assert chain.published[j].wait(GUARD), f"part {j} never published"
        if fail and fail[0] == k:
            raise fail[1]
        chain.publish(k, values[k])
        b = chain.before(k)
        with lock:
            got[k] = b

    return chain, got, guarded(lambda: run_parts(devs, len(values), job, chain))


@pytest.mark.parametrize("devs, want", [([0, 0, 0], [3, 2, 2, 3, 2, 2, 3]), ([0], [7] * 7)])
def test_parts_go_round_robin_in_order_on_one_thread_per_entry(devs, want):
    seen, lock = [], threading.Lock()

    def job(k, entry_parts):
        with lock:
            seen.append((k, entry_parts, threading.get_ident()))

    run_parts(devs, 7, job)
    assert sorted(k for k, _, _ in seen) == list(range(7))
    assert [n for _, n, _ in sorted(seen)] == want
    threads = {}
    for k, _, t in seen:                                 # in the order the parts ran
        threads.setdefault(k % len(devs), []).append((t, k))
    for entry, runs in threads.items():
        assert len({t for t, _ in runs}) == 1, "the parts of one entry share a thread"
        assert [k for _, k in runs] == list(range(entry, 7, len(devs))), "and run in increasing k"
    idents = {runs[0][0] for runs in threads.values()}
    assert len(idents) == len(devs)
    # several entries run on their persistent workers, a single one on the calling thread
    assert (threading.get_ident() in idents) == (len(devs) == 1)


def test_before_is_the_prefix_sum_whatever_the_order_of_publishing():
    values = [5, 0, 7, 1, 1 << 40, 3, 9, 2, 4]
    # parts 0, 1, 2 start side by side on three workers: part 2 publishes first, then part 0, then part 1
    chain, got, result = chained([0, 0, 0], values, gates={0: [2], 1: [0]})
    assert result == {"value": None}
    sums = [sum(values[:k]) for k in range(len(values))]
    assert got == dict(enumerate(sums))
    # a fresh thread's cursor, forwards and backwards
    assert [chain.before(k) for k in range(len(values))] == sums
    assert [chain.before(k) for k in reversed(range(len(values)))] == sums[::-1]


def test_parts_that_publish_before_they_wait_always_finish():
    """The chain's invariant.  Two entries, four parts: part 2 runs behind part 0 on one worker and part 1 waits for
    part 0 on the other.  Every part publishes first, so whatever a part waits for is published by a worker that is
    not itself waiting behind it; a part that waited first would hold its worker's next part back."""
    chain, got, result = chained([0, 0], [1, 2, 3, 4])
    assert result == {"value": None}
    assert got == {0: 0, 1: 1, 2: 3, 3: 6}
    assert all(e.is_set() for e in chain.published) and not chain.failed.is_set() and not chain.errors


def test_a_part_that_raises_releases_the_waiters_and_is_what_the_caller_sees():
    cause = OSError("cause")
    # part 1 fails before it publishes, once parts 2 and 3 have published: they wait for it (part 3 behind part 0)
    chain, got, result = chained([0, 0, 0], [1] * 6, gates={1: [2, 3]}, fail=(1, cause))
    assert "value" not in result and result["error"] is cause, "the caller must see the cause, not a waiter"
    assert set(got) <= {0}, "no part past 0 may get a sum"
    assert chain.errors[0] is cause and chain.failed.is_set()
    assert all(isinstance(e, RuntimeError) and str(e) == "test index: another part failed" for e in chain.errors[1:])
    assert not chain.published[1].is_set() and chain.published[2].is_set() and chain.published[3].is_set()
    assert "value" in guarded(scan_objects.release_workers)          # the workers are idle again: this returns
    chain, got, result = chained([0, 0, 0], [1] * 6)                 # and the same workers run a healthy build
    assert result == {"value": None} and got == {k: k for k in range(6)}


def test_a_fresh_chain_on_the_same_workers_knows_nothing_of_a_failed_one():
    old, _, result = chained([0, 0], [4, 4, 4, 4], fail=(0, ValueError("first")))
    assert isinstance(result["error"], ValueError) and old.failed.is_set()
    new, got, result = chained([0, 0], [2, 3, 5, 7])
    assert result == {"value": None} and got == {0: 0, 1: 2, 2: 5, 3: 10}
    assert not new.failed.is_set() and not new.errors and old.failed.is_set()


def test_without_a_chain_a_failure_is_raised_as_it_is():
    boom = KeyError("part 3")

    def job(k, _):
        if k == 3:
            raise boom

    assert guarded(lambda: run_parts([0, 0], 5, job))["error"] is boom
    assert guarded(lambda: run_parts([0], 5, job))["error"] is boom
