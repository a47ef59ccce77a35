"""CPU: the streamed scoring loop (models/stream_loop.py) against a stand-in pipeline -- the host-side contract the GPU tests
reach only through a model that owns a device context: results in feed order around a feed that takes the per-batch path,
back-pressure, padding of titles and answers to the graph's n_batch rows, slicing, and what is left behind when a loop ends
early.  No device and no libdae_hip.so."""
import os
import subprocess
import sys

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models import stream_loop
from spotify_recsys_challenge_2018_amd.models.stream_loop import SEEDS_FROM_INPUT
from spotify_recsys_challenge_2018_amd.utils import metrics as met

NB, K = 4, 3


class FakePipe:
    """What the loop may use of a `_lib.Pipeline`.  Feeds become launches of `feeds_per_launch` (a full group, or `flush`);
    the pipeline holds `launches` of them and answers "busy" to a submit beyond that.  A feed's lists carry its tag
    (x_positions[0, 1]) in every column but the first, which counts the rows."""

    def __init__(self, feeds_per_launch=2, launches=2, title_len=None, max_nnz=16, max_answers=None, ready_at_once=True,
                 guard_per_launch=0):
        self.per_launch, self.capacity = feeds_per_launch, launches * feeds_per_launch
        self.group_rows, self.max_nnz, self.title_len = feeds_per_launch * NB, max_nnz, title_len
        if max_answers is not None:                     # (as the real one: only a pipeline in evaluation mode has it)
            self.max_answers = max_answers
        self.ready_at_once = ready_at_once              # False: a non-waiting poll never finds a result
        self.guard_per_launch, self.guard_fallbacks = guard_per_launch, 0
        self.pending, self.users, self.h = 0, 0, object()
        self.queue, self.log, self.fed, self.handed = [], [], [], {}
        self.fail = None                                # raised by the next submit

    def _launch(self):
        if any(not launched for _tag, launched in self.queue):
            self.guard_fallbacks += self.guard_per_launch
        self.queue = [[tag, True] for tag, _launched in self.queue]

    def _take(self, positions, values, n_rows, answers, titles, titles_use):
        assert self.h is not None, "submit on a closed pipeline"
        if self.fail is not None:
            raise self.fail
        tag = int(np.asarray(positions)[0, 1])
        if self.pending == self.capacity:
            self.log.append(("submit", tag, False))
            return False
        self.fed.append(dict(tag=tag, n_rows=n_rows, answers=answers, titles=titles, use=titles_use))
        self.queue.append([tag, False])
        self.pending += 1
        if sum(not launched for _tag, launched in self.queue) == self.per_launch:
            self._launch()
        self.log.append(("submit", tag, True))
        return True

    def submit(self, positions, values, n_rows, titles=None, titles_use=None):
        return self._take(positions, values, n_rows, None, titles, titles_use)

    def submit_eval(self, positions, values, n_rows, answers, titles=None, titles_use=None):
        assert answers is not None
        return self._take(positions, values, n_rows, answers, titles, titles_use)

    def flush(self):
        self._launch()
        self.log.append(("flush",))

    def _next(self, wait):
        if self.pending == 0:
            return None
        tag, launched = self.queue[0]
        assert launched or not wait, "poll(wait=True) for a feed no launch holds: the library would block"
        if not launched or not (wait or self.ready_at_once):
            self.log.append(("poll", wait, None))
            return None
        self.queue.pop(0)
        self.pending -= 1
        self.log.append(("poll", wait, tag))
        return tag

    def poll(self, wait=True):
        tag = self._next(wait)
        if tag is None:
            return None
        self.handed[tag] = lists(tag, NB)
        return self.handed[tag]

    def poll_eval(self, wait=True):
        tag = self._next(wait)
        if tag is None:
            return None
        self.handed[tag] = records(tag, NB)
        return self.handed[tag]

    def stats(self):
        return {"launches": 0, "feeds": len(self.fed), "guard_fallbacks": self.guard_fallbacks}

    def close(self):
        self.h = None
        self.log.append(("close",))


def lists(tag, n):
    idx = np.full((n, K), tag, np.int32)
    idx[:, 0] = np.arange(n)
    return idx, idx.astype(np.float32) + 0.5


def records(tag, n):
    rec = np.zeros(n, met.RECORD_DTYPE)
    rec["m"], rec["first"] = tag, np.arange(n)
    return rec


def feed(tag, n_rows=NB, seeds=SEEDS_FROM_INPUT, nnz=2, extra=()):
    pos = np.array([[i % max(n_rows or NB, 1), tag] for i in range(nnz)], np.int64)
    return (pos, np.ones(nnz, np.float32), seeds, n_rows) + tuple(extra)


def tag_of(f):
    return int(f[0][0, 1])


def drive(pipe, feeds, fallback, **kw):
    return stream_loop.stream(pipe, feeds, fallback, NB, **kw)


def no_fallback(f):
    raise AssertionError("feed %d took the per-batch path" % tag_of(f))


def test_importing_the_loop_loads_neither_the_library_nor_torch():
    code = ("import sys\n"
            "from spotify_recsys_challenge_2018_amd.models import stream_loop, DAEs\n"
            "from spotify_recsys_challenge_2018_amd import _lib\n"
            "assert _lib._lib is None and 'torch' not in sys.modules\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


def test_results_come_in_feed_order_around_a_per_batch_feed():
    """Seven feeds, the fourth with explicit seed lists: one result per feed, in order, and the pipeline was flushed and
    drained before the per-batch path ran."""
    pipe = FakePipe()
    seen = []

    def fallback(f):
        assert pipe.pending == 0 and pipe.log[-1][0] == "poll" and ("flush",) in pipe.log
        seen.append((tag_of(f), len(pipe.log)))
        return lists(100 + tag_of(f), f[3])
    feeds = [feed(t, seeds=[[1]] * NB if t == 3 else SEEDS_FROM_INPUT) for t in range(7)]
    got = list(drive(pipe, feeds, fallback))
    assert [int(g[0][0, 1]) for g in got] == [0, 1, 2, 103, 4, 5, 6]
    assert [t for t, _at in seen] == [3] and [d["tag"] for d in pipe.fed] == [0, 1, 2, 4, 5, 6]
    before = pipe.log[:seen[0][1]]
    assert [e[2] for e in before if e[0] == "poll" and e[2] is not None] == [0, 1, 2]      # drained, in order, before it
    assert before.index(("flush",)) > before.index(("submit", 2, True))
    for g in got:
        assert g[1] is not None and np.array_equal(g[1], g[0].astype(np.float32) + 0.5)
    # without the scores: None in their place, on both paths
    got = list(drive(FakePipe(), feeds, lambda f: lists(100 + tag_of(f), f[3]), want_scores=False))
    assert [int(g[0][0, 1]) for g in got] == [0, 1, 2, 103, 4, 5, 6] and all(g[1] is None for g in got)


def test_one_non_waiting_poll_round_per_launch():
    """Results arrive a launch at a time: the loop asks without waiting once per `group_rows // n_batch` feeds, not per feed."""
    pipe = FakePipe(feeds_per_launch=3, launches=2)
    got = list(drive(pipe, [feed(t) for t in range(6)], no_fallback))
    assert len(got) == 6
    submits = [i for i, e in enumerate(pipe.log) if e[0] == "submit"]
    for n, (a, b) in enumerate(zip(submits, submits[1:] + [len(pipe.log)])):
        polled = [e for e in pipe.log[a + 1:b] if e[0] == "poll"]
        assert bool(polled) == ((n + 1) % 3 == 0), (n, polled)


def test_busy_submit_is_retried_after_a_waiting_poll():
    """Every lane full (`submit` answers False): the oldest result is waited for and handed out, then the same feed is
    submitted again -- nothing lost, nothing reordered."""
    pipe = FakePipe(feeds_per_launch=2, launches=2, ready_at_once=False)
    got = list(drive(pipe, [feed(t) for t in range(11)], no_fallback))
    assert [int(g[0][0, 1]) for g in got] == list(range(11))
    assert [d["tag"] for d in pipe.fed] == list(range(11))
    busy = [i for i, e in enumerate(pipe.log) if e[0] == "submit" and e[2] is False]
    assert busy
    for i in busy:
        tag = pipe.log[i][1]
        assert pipe.log[i + 1][:2] == ("poll", True) and pipe.log[i + 1][2] is not None
        assert pipe.log[i + 2][:2] == ("submit", tag)


def test_short_feeds_are_sliced_and_full_feeds_handed_out_as_they_are():
    pipe = FakePipe()
    rows = [NB, 1, NB, 3, None]
    got = list(drive(pipe, [feed(t, n_rows=n) for t, n in enumerate(rows)], no_fallback))
    assert all(d["n_rows"] == NB for d in pipe.fed)                 # every feed is fed as the graph's n_batch rows
    for t, (n, (gi, gs)) in enumerate(zip(rows, got)):
        hi, hs = pipe.handed[t]
        if n in (NB, None):
            assert gi is hi and gs is hs
        else:
            assert gi.shape == (n, K) and gs.shape == (n, K) and gi.base is hi and gs.base is hs
            assert np.array_equal(gi, hi[:n]) and np.array_equal(gs, hs[:n])


def test_a_feed_larger_than_a_launch_slot_takes_the_per_batch_path():
    pipe = FakePipe(max_nnz=5)
    taken = []

    def fallback(f):
        taken.append(tag_of(f))
        return lists(tag_of(f), f[3])
    feeds = [feed(0, nnz=5), feed(1, nnz=6), feed(2, n_rows=NB + 1), feed(3, seeds="other"), feed(4)]
    got = list(drive(pipe, feeds, fallback))
    assert taken == [1, 2, 3] and [d["tag"] for d in pipe.fed] == [0, 4]
    assert [g[0].shape[0] for g in got] == [NB, NB, NB + 1, NB, NB]


def test_early_stop_or_error_closes_the_pipeline_and_a_clean_run_keeps_it():
    key = (0, K, True, NB)
    feeds = [feed(t, seeds=[[1]] * NB if t == 2 else SEEDS_FROM_INPUT) for t in range(6)]
    # a clean run: cached, open, no loop on it
    pipe = FakePipe()
    cache = {key: (0, pipe)}
    assert len(list(drive(pipe, feeds, lambda f: lists(tag_of(f), f[3]), cache=cache, key=key))) == 6
    assert cache == {key: (0, pipe)} and pipe.h is not None and pipe.users == 0 and pipe.pending == 0
    # a consumer that stops after the first result
    pipe = FakePipe()
    cache = {key: (0, pipe)}
    it = drive(pipe, feeds, lambda f: lists(tag_of(f), f[3]), cache=cache, key=key)
    first = next(it)
    assert int(first[0][0, 1]) == 0 and pipe.users == 1
    it.close()
    assert cache == {} and pipe.h is None and pipe.users == 0
    # a per-batch path that raises
    pipe = FakePipe()
    cache = {key: (0, pipe)}

    def broken(f):
        raise RuntimeError("recommend failed")
    with pytest.raises(RuntimeError, match="recommend failed"):
        list(drive(pipe, feeds, broken, cache=cache, key=key))
    assert cache == {} and pipe.h is None and pipe.users == 0
    # feeds that raise while they are read
    pipe = FakePipe()
    cache = {key: (0, pipe)}

    def reader():
        yield feed(0)
        raise OSError("reader failed")
    with pytest.raises(OSError):
        list(drive(pipe, reader(), no_fallback, cache=cache, key=key))
    assert cache == {} and pipe.h is None
    # another key's pipeline was cached while this loop ran: one stays
    pipe, other = FakePipe(), FakePipe()
    cache = {key: (0, pipe)}
    it = drive(pipe, feeds[:2], no_fallback, cache=cache, key=key)
    next(it)
    cache["other"] = (0, other)
    assert len(list(it)) == 1
    assert cache == {"other": (0, other)} and pipe.h is None and other.h is not None


def test_evaluation_mode_pads_the_answers_and_checks_their_count():
    pipe = FakePipe(max_answers=6)
    answers = {0: [[5, 6], [], [7], [-1, 7, 7]], 1: [[1], [2, 3]], 2: [[1, 2], [3, 4], [5, 6], [7]], 3: [[9]] * NB}
    taken = []

    def fallback(f):
        taken.append(tag_of(f))
        return lists(tag_of(f), f[3])
    feeds = [(feed(t, n_rows=len(a)), a) for t, a in answers.items()]
    got = list(drive(pipe, feeds, fallback, want_scores=False, eval_mode=True))
    assert taken == [2] and [d["tag"] for d in pipe.fed] == [0, 1, 3]           # 7 answers > max_answers: per batch
    rp, col = pipe.fed[0]["answers"]
    assert rp.dtype == np.int32 and col.dtype == np.int32
    assert rp.tolist() == [0, 2, 2, 3, 6] and col.tolist() == [5, 6, 7, -1, 7, 7]
    rp, col = pipe.fed[1]["answers"]                                            # two rows of four: the rest are empty
    assert rp.tolist() == [0, 1, 3, 3, 3] and col.tolist() == [1, 2, 3] and len(rp) == NB + 1
    assert [g.dtype for g in got] == [met.RECORD_DTYPE] * 4 and [len(g) for g in got] == [4, 2, 4, 4]
    assert got[0] is pipe.handed[0] and got[1].base is pipe.handed[1] and got[1]["m"].tolist() == [1, 1]
    want = met.rank_records(lists(2, NB)[0], answers[2])
    assert got[2].tobytes() == want.tobytes()
    # a wrong number of answer lists
    pipe = FakePipe(max_answers=6)
    with pytest.raises(ValueError, match="answer lists"):
        list(drive(pipe, [(feed(0, n_rows=3), [[1], [2]])], fallback, want_scores=False, eval_mode=True))
    assert pipe.h is None
    with pytest.raises(ValueError, match="answer lists"):
        stream_loop.answers_csr([[1]], 2, NB)
    assert stream_loop.answers_csr([[1]] * (NB + 1), NB + 1, NB) is None


def test_titles_are_padded_to_the_launch_and_dropped_when_unused():
    L = 5
    pipe = FakePipe(title_len=L)
    t_full = [[1, 2, 3, -1, -1], None, [4] * L, [5] * L]
    feeds = [feed(0, extra=(t_full, np.ones(NB, np.float32))),
             feed(1, extra=(t_full, np.zeros(NB, np.float32))),                   # titles_use all zero: the plain DAE
             feed(2, n_rows=2, extra=(t_full[:2], [1.0, 1.0, 1.0])),              # fewer titles than rows: no title, no use
             feed(3, extra=(np.arange(NB * L).reshape(NB, L), [0.0, 1.0])),       # an array; a short titles_use
             feed(4, extra=(None, None)), feed(5)]
    got = list(drive(pipe, feeds, no_fallback, mixes_titles=True))
    assert [int(g[0][0, 1]) for g in got] == list(range(6))
    fed = {d["tag"]: d for d in pipe.fed}
    t, u = fed[0]["titles"], fed[0]["use"]
    assert t.dtype == np.int32 and t.shape == (NB, L) and u.dtype == np.float32 and u.tolist() == [1.0] * NB
    assert t.tolist() == [[1, 2, 3, -1, -1], [-1] * L, [4] * L, [5] * L]
    assert fed[1]["titles"] is None and fed[1]["use"] is None
    assert fed[2]["titles"].tolist() == [[1, 2, 3, -1, -1], [-1] * L, [-1] * L, [-1] * L]
    assert fed[2]["use"].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert fed[3]["titles"].tolist() == np.arange(NB * L).reshape(NB, L).tolist() and fed[3]["use"].tolist() == [0, 1, 0, 0]
    assert fed[4]["titles"] is None and fed[5]["titles"] is None
    assert stream_loop.title_block(t_full, np.zeros(NB), NB, L) == (None, None)
    # a pipeline without a title scorer: a DAE_title's titled feeds go per batch, a plain DAE's are fed without their titles
    taken = []

    def fallback(f):
        taken.append(tag_of(f))
        return lists(tag_of(f), f[3])
    pipe = FakePipe()
    list(drive(pipe, feeds, fallback, mixes_titles=True))
    assert taken == [0, 1, 2, 3, 4] and [d["tag"] for d in pipe.fed] == [5]
    pipe = FakePipe()
    list(drive(pipe, feeds, no_fallback, mixes_titles=False))
    assert [d["tag"] for d in pipe.fed] == list(range(6)) and all(d["titles"] is None for d in pipe.fed)


def test_an_out_of_range_feed_surfaces_as_value_error():
    key = (0, K, True, NB)
    for text, exc, match in (("dae_pipeline error -3: feed 1 holds a row index out of range", ValueError, "index out of range"),
                             ("dae_pipeline error -3: a title character outside the table", ValueError, "outside the table"),
                             ("dae_pipeline error -5: hipErrorLaunchFailure", _lib.DaeError, "hipErrorLaunchFailure")):
        pipe = FakePipe()
        cache = {key: (0, pipe)}
        it = drive(pipe, [feed(0), feed(1), feed(2)], no_fallback, cache=cache, key=key)
        pipe.fail = _lib.DaeError(text)
        with pytest.raises(exc, match=match) as info:
            list(it)
        assert type(info.value) is exc and cache == {} and pipe.h is None


def test_guard_fallbacks_of_this_loop_only_are_reported():
    """on_guard gets the launches the pipeline re-scored during THIS loop (the counters of earlier loops are not charged to it),
    also when the consumer stops early; a loop without any is silent."""
    told = []
    pipe = FakePipe(guard_per_launch=1)
    pipe.guard_fallbacks = 5
    assert len(list(drive(pipe, [feed(t) for t in range(5)], no_fallback, on_guard=told.append))) == 5
    assert told == [3] and pipe.guard_fallbacks == 8
    it = drive(pipe, [feed(t) for t in range(5)], no_fallback, on_guard=told.append)
    next(it)
    it.close()
    assert told == [3, 1]
    pipe = FakePipe()
    list(drive(pipe, [feed(0)], no_fallback, on_guard=told.append))
    assert told == [3, 1]
