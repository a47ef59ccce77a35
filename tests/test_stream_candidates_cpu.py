"""CPU: the streamed candidate calls without a device.  (1) The candidate staging of the pipeline's candidates mode
(csrc/pipeline_stage.h: the launch closing on candidate capacity or rows, the per-feed offsets, the rollback of a refused feed, a
feed without candidates, the result blocks' counts) as a stand-alone C++ program, tests/host/pipeline_cand_stage_main.cpp, built
plainly and with -fsanitize=address,undefined (a host executable with its own main; nothing is preloaded).  (2) The four new
entry points are declared, exported names and bound with matching argument counts.  (3) `score_candidates_iter` /
`rank_candidates_iter` refuse what they document before a pipeline exists, and hand a 2-D candidate array to the staging call
without a pass over its rows (asserted on the arrays a stubbed pipeline receives)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models import stream_loop
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_title
from spotify_recsys_challenge_2018_amd.models.stream_loop import SEEDS_FROM_INPUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]
ENTRY_POINTS = {"dae_pipeline_enable_candidates": 4, "dae_pipeline_submit_candidates": 11, "dae_pipeline_poll_candidates": 7,
                "dae_candidates_unique": 7}
NB, V = 4, 50


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "sanitized"])
def test_candidate_staging_as_a_standalone_program(tmp_path, flags):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    if flags:
        one = tmp_path / "one.cpp"
        one.write_text("int main() { return 0; }\n")
        probe = subprocess.run([cxx, *flags, str(one), "-o", str(tmp_path / "one")], capture_output=True, text=True)
        if probe.returncode != 0 or subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
            pytest.skip("%s cannot link the sanitizer runtime: %s" % (cxx, probe.stderr.strip()[-200:]))
    exe = str(tmp_path / "pipeline_cand_stage")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "pipeline_cand_stage_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def test_entry_points_declared_and_bound_with_matching_argument_counts():
    text = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    head = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {name: len([a for a in args.split(",") if a.strip()])
              for name, args in re.findall(r"\bint\s+(dae_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", head)}
    lib = _lib.load()
    for name, n_args in ENTRY_POINTS.items():
        assert counts.get(name) == n_args, (name, counts.get(name))
        assert name in _lib.EXPORTS, name
        assert len(getattr(lib, name).argtypes) == n_args, name
    assert int(re.search(r"#define\s+DAE_PIPE_BAD_ID\s+(\d+)", text).group(1)) == _lib.DAE_PIPE_BAD_ID
    assert int(re.search(r"#define\s+DAE_CAND_UNIQUE_MAX_V\s+(\d+)", text).group(1)) == _lib.DAE_CAND_UNIQUE_MAX_V


# ---- the Python side against a stand-in pipeline -------------------------------------------------------------------------------

class FakeCandPipe:
    """What `stream_loop.stream_candidates` may use of a `_lib.Pipeline` in candidates mode.  It keeps the very arrays
    `submit_candidates` was handed, and answers every feed with values that tell its ids back (score mode) or with lists that
    carry the feed's number (rank mode)."""

    def __init__(self, rank=False, k=3, max_candidates=64, max_nnz=16, group_rows=2 * NB):
        self.cand_rank, self.k, self.max_candidates, self.max_nnz, self.group_rows = rank, k, max_candidates, max_nnz, group_rows
        self.title_len, self.pending, self.users, self.h = None, 0, 0, object()
        self.fed, self.queue, self.flushed = [], [], 0

    def submit_candidates(self, positions, values, n_rows, candidates, titles=None, titles_use=None):
        self.fed.append(dict(n_rows=n_rows, rp=candidates[0], col=candidates[1], titles=titles))
        self.queue.append(len(self.fed) - 1)
        self.pending += 1
        return True

    def flush(self):
        self.flushed += 1

    def _next(self):
        if not self.queue:
            return None
        self.pending -= 1
        return self.queue.pop(0)

    def poll_candidates(self, wait=True, copy=False):
        i = self._next()
        return None if i is None else (self.fed[i]["col"].astype(np.float32) + 0.5, False)

    def poll(self, wait=True):
        i = self._next()
        if i is None:
            return None
        idx = np.full((NB, self.k), i, np.int32)
        return idx, idx.astype(np.float32)

    def close(self):
        self.h = None


def _model(cls=DAE):
    class C:
        save = "/tmp/_cand_unused"; n_input = V; hidden = 8; lr = 0.01; reg_lambda = 0.0; n_tracks = 40; initval = "NULL"; batch = NB
    return cls(C())


def _stubbed(monkeypatch, pipe):
    """A model that was never fit() -- no context, no device -- whose candidate loops get `pipe`."""
    m = _model()
    m.sync_params = lambda: None
    asked = []

    def pipeline_for(model, scorer, dtype, k, want_scores, eval_mode=False, catalogue=None, candidates=None):
        asked.append(dict(k=k, want_scores=want_scores, candidates=candidates, scorer=scorer))
        return ("key", pipe)
    monkeypatch.setattr(stream_loop, "pipeline_for", pipeline_for)
    return m, asked


def feed(tag, n_rows=NB, seeds=SEEDS_FROM_INPUT, nnz=2):
    pos = np.array([[i % max(n_rows or NB, 1), tag] for i in range(nnz)], np.int64)
    return pos, np.ones(nnz, np.float32), seeds, n_rows


def test_refusals_come_before_any_pipeline(monkeypatch):
    def no_pipeline(*a, **kw):
        raise AssertionError("a pipeline was asked for")
    monkeypatch.setattr(stream_loop, "pipeline_for", no_pipeline)
    m = _model()
    feeds = [(feed(0), [[1, 2]])]
    with pytest.raises(ValueError, match="catalogue"):
        m.score_candidates_iter(feeds, catalogue=object())
    with pytest.raises(ValueError, match="catalogue"):
        m.rank_candidates_iter(feeds, k=3, catalogue=object())
    with pytest.raises(ValueError, match="1024.*pipeline's limit"):
        m.rank_candidates_iter(feeds, k=1025)
    with pytest.raises(ValueError, match="kind"):
        m.score_candidates_iter(feeds, kind="softmax")
    # a titled stream has no logit (the check comes first: the object below has nothing else)
    with pytest.raises(ValueError, match="sigmoid"):
        DAE_title.score_candidates_iter(DAE_title.__new__(DAE_title), feeds, kind="logit")
    m.shard_scoring(0, 2)
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.score_candidates_iter(feeds)
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.rank_candidates_iter(feeds, k=3)


@pytest.mark.parametrize("bad", [V, -2, 2 ** 31])
def test_a_bad_id_raises_at_its_feed_after_the_feeds_before_it(monkeypatch, bad):
    pipe = FakeCandPipe()
    m, _asked = _stubbed(monkeypatch, pipe)
    feeds = [(feed(0), [[1, 2], [3]]), (feed(1), np.array([[4, 5], [6, -1]], np.int64)), (feed(2), [[7], [8, bad]]), (feed(3), [[9]])]
    it = m.score_candidates_iter(feeds)
    got = []
    with pytest.raises(ValueError, match="out of range"):
        for r in it:
            got.append(r)
    assert len(got) == 2 and len(pipe.fed) == 2                         # nothing of the bad feed reached the pipeline
    assert [a.tolist() for a in got[0]] == [[1.5, 2.5], [3.5], [], []]
    assert got[1].shape == (NB, 2) and got[1][:2].tolist() == [[4.5, 5.5], [6.5, -0.5]] and np.isneginf(got[1][2:]).all()
    assert pipe.h is None                                               # (a loop that ended in an error does not keep its pipeline)


def test_the_two_dimensional_form_reaches_the_staging_call_without_a_pass_over_its_rows(monkeypatch):
    pipe = FakeCandPipe(max_candidates=1 << 20)
    m, asked = _stubbed(monkeypatch, pipe)
    C = 1000
    a32 = np.arange(NB * C, dtype=np.int32).reshape(NB, C) % V
    a32[1, 5:] = -1
    a64 = a32[:3].astype(np.int64)
    got = list(m.score_candidates_iter([(feed(0), a32), (feed(1, n_rows=3), a64), (feed(2), [[1, 1], [], [2]])], kind="logit"))
    assert asked == [dict(k=1, want_scores=False, candidates=(False, _lib.DAE_OUT_LOGIT, m.cand_launch_ids), scorer=None)]
    f0, f1, f2 = pipe.fed
    # an int32 C-contiguous array is staged from its own memory: no copy, no per-row list
    assert f0["col"].dtype == np.int32 and np.shares_memory(f0["col"], a32) and f0["col"].shape == (NB * C,)
    assert f0["rp"].dtype == np.int32 and f0["rp"].tolist() == [0, C, 2 * C, 3 * C, 4 * C]
    # another integer type is converted in one piece; rows behind the array (and behind n_rows) are empty
    assert f1["col"].dtype == np.int32 and f1["col"].tolist() == a64.reshape(-1).tolist()
    assert f1["rp"].tolist() == [0, C, 2 * C, 3 * C, 3 * C] and f1["n_rows"] == NB
    assert f2["rp"].tolist() == [0, 2, 2, 3, 3] and f2["col"].tolist() == [1, 1, 2]
    # and the results come back in the callers' forms
    assert got[0].shape == (NB, C) and np.array_equal(got[0], a32.astype(np.float32) + 0.5)
    assert got[1].shape == (3, C) and np.array_equal(got[1], a64.astype(np.float32) + 0.5)
    assert [g.tolist() for g in got[2]] == [[1.5, 1.5], [], [2.5], []]
    assert pipe.h is not None and pipe.users == 0 and pipe.pending == 0


def test_feeds_the_pipeline_does_not_take_go_per_batch_in_order(monkeypatch):
    pipe = FakeCandPipe(rank=True, max_candidates=5, max_nnz=4)
    m, asked = _stubbed(monkeypatch, pipe)
    calls = []

    def rank_candidates(x_positions, x_ones, candidates, seeds, k=500, n_rows=None):
        assert pipe.pending == 0 and pipe.flushed >= 1                  # drained, in order, before the per-batch call
        calls.append(int(x_positions[0, 1]))
        idx = np.full((n_rows or NB, k), 100 + calls[-1], np.int32)
        return idx, idx.astype(np.float32)
    m.rank_candidates = rank_candidates
    feeds = [(feed(0), [[1, 2]]), (feed(1), [[1, 2, 3], [4, 5, 6]]),            # 6 ids > max_candidates
             (feed(2, seeds=[[1]] * NB), [[1]]),                                # explicit seed lists
             (feed(3, nnz=5), [[1]]),                                           # more entries than a launch slot
             (feed(4, n_rows=2), [[2], [3]])]
    got = list(m.rank_candidates_iter(feeds, k=3, want_scores=False))
    assert asked[0]["k"] == 3 and asked[0]["candidates"] == (True, _lib.DAE_OUT_SCORE, m.cand_launch_ids)
    assert calls == [1, 2, 3] and len(pipe.fed) == 2
    assert [int(g[0][0, 0]) for g in got] == [0, 101, 102, 103, 1] and all(g[1] is None for g in got)
    assert got[4][0].shape == (2, 3)
    # device_csr = False: every feed goes per batch, no pipeline
    m2, asked2 = _stubbed(monkeypatch, FakeCandPipe())
    m2.device_csr = False
    m2.score_candidates = lambda x_positions, x_ones, candidates, n_rows=None, kind="sigmoid": ("per batch", kind)
    assert list(m2.score_candidates_iter(feeds[:2], kind="logit")) == [("per batch", "logit")] * 2 and asked2 == []


def test_candidates_csr():
    rp, col = stream_loop.candidates_csr([[5, 3, 5, -1], [], [0]], 3, NB, 10)
    assert rp.dtype == np.int32 and col.dtype == np.int32 and rp.tolist() == [0, 4, 4, 5, 5] and col.tolist() == [5, 3, 5, -1, 0]
    rp, col = stream_loop.candidates_csr([], 2, NB, 10)
    assert rp.tolist() == [0] * (NB + 1) and col.size == 0
    with pytest.raises(ValueError, match="rows for a feed"):
        stream_loop.candidates_csr([[1], [2], [3]], 2, NB, 10)
    with pytest.raises(ValueError, match="integer array"):
        stream_loop.candidates_csr(np.zeros((2, 2), np.float32), 2, NB, 10)
    with pytest.raises(ValueError, match="out of range"):
        stream_loop.candidates_csr(np.array([[1, 10]]), 1, NB, 10)
