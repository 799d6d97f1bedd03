"""Host threads side by side (helper of tests/test_gpu_threads.py and tests/thread_first_calls.py; not a test).

The threading contract of include/spfe.h ("Threads"): one handle (or twin pair) is one thread's at a time, distinct handles may be
driven from distinct threads at the same moment.  run_side_by_side() is the harness that drives them so: one daemon thread per
worker, all released by one barrier, then free-running — no barrier between rounds, so that the calls of the threads interleave
as the scheduler has it (ctypes releases the GIL for the length of every library call).

The device buffers the record forms work on are graph_forms.Buffers with a torch.cuda.Stream per thread: its copies, fills and
waits stay on that stream, so no thread waits for another's work."""
import threading
import time
import traceback


class WorkerFailed(AssertionError):
    pass


def _exit_session(message):
    import pytest
    pytest.exit(message, returncode=1)


def run_side_by_side(workers, rounds, join_timeout, names=None, on_hang=_exit_session):
    """workers: callables worker(round), one thread each (up to 4: the count is the caller's, never the machine's); every thread
    waits at one barrier and then calls its worker for round 0 .. rounds - 1 without waiting for the others again.
    A worker's exception ends that thread's rounds; it is kept with its traceback and, after every thread has been joined,
    raised in the calling thread as WorkerFailed (all of them in the message, the first as __cause__).
    A thread that has not ended join_timeout seconds after the start counts as hung: on_hang("worker ..., round ...") is called
    — pytest.exit(..., returncode=1) by default, so that nothing further is started on the GPU in this session.  Nothing is
    tried again."""
    assert 1 <= len(workers) <= 4, len(workers)     # (one: a fresh thread beside the calling one)
    names = list(names) if names is not None else ["worker %d" % i for i in range(len(workers))]
    barrier = threading.Barrier(len(workers))
    at = [-1] * len(workers)                    # the round each thread is in (rounds: done)
    failed = [None] * len(workers)

    def body(i):
        try:
            barrier.wait(join_timeout)
            for r in range(rounds):
                at[i] = r
                workers[i](r)
            at[i] = rounds
        except BaseException as e:              # noqa: B902 — kept for the calling thread, whatever it is
            failed[i] = (e, traceback.format_exc())
            barrier.abort()                     # (a failure before the start must not leave the others waiting)

    threads = [threading.Thread(target=body, args=(i,), name=names[i], daemon=True) for i in range(len(workers))]
    t0 = time.monotonic()
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, t0 + join_timeout - time.monotonic()))
    hung = ["%s in round %d of %d" % (names[i], at[i], rounds) for i, t in enumerate(threads) if t.is_alive()]
    if hung:
        on_hang("threads still running %.0f s after the start, counted as hung: %s" % (join_timeout, "; ".join(hung)))
        raise WorkerFailed("hung: %s" % "; ".join(hung))
    bad = [(names[i], at[i], f) for i, f in enumerate(failed) if f is not None]
    if bad:
        text = "\n".join("--- %s, round %d ---\n%s" % (n, r, tb) for n, r, (_, tb) in bad)
        raise WorkerFailed("%d of %d threads failed\n%s" % (len(bad), len(workers), text)) from bad[0][2][0]
    return time.monotonic() - t0
