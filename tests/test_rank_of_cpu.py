"""CPU: what rank_of needs no device for -- the plan header as a stand-alone C++ program (plain and sanitized; nothing is
preloaded), the rank metrics of utils/metrics.py against brute force, the [BASE] eval_ranks key, and the agreement of
include/dae_hip.h with the ctypes bindings on the new entry points."""
import configparser
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd.utils import metrics as met

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]


def _cxx():
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    return cxx


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "sanitized"])
def test_plan_header_as_a_standalone_program(tmp_path, flags):
    cxx = _cxx()
    if flags:
        one = tmp_path / "one.cpp"
        one.write_text("int main() { return 0; }\n")
        probe = subprocess.run([cxx, *flags, str(one), "-o", str(tmp_path / "one")], capture_output=True, text=True)
        if probe.returncode != 0 or subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
            pytest.skip("%s cannot link the sanitizer runtime: %s" % (cxx, probe.stderr.strip()[-200:]))
    exe = str(tmp_path / "rank_of_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", *flags, "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "rank_of_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def test_plan_binding_agrees_with_the_header_constants():
    """dae_rank_of_plan (host only: no device is touched) returns the header's geometry."""
    from spotify_recsys_challenge_2018_amd import _lib
    a = _lib.rank_of_plan(256, 256, 2560)
    assert a == {"rows": 128, "capacity": 20, "row_groups": 2, "blocks_per_group": 128}
    b = _lib.rank_of_plan(256, 256, 25600)
    assert b["rows"] == 64 and b["capacity"] >= 100 and b["row_groups"] == 4
    # 160 KiB: hidden tile + 12 bytes per (row, answer) + 8 per row, 1 KiB left free
    for p, hp in ((a, 256), (b, 256), (_lib.rank_of_plan(40, 64, 400), 64)):
        assert p["rows"] * hp * 4 + p["rows"] * p["capacity"] * 12 + p["rows"] * 8 + 1024 <= 160 * 1024
    with pytest.raises(ValueError):
        _lib.rank_of_plan(5000, 256, 10)


# ---- utils/metrics.py over rank arrays ---------------------------------------------------------------------------------------------
def _random_ranks(rng, n, top):
    r = rng.integers(0, top, n)
    r[rng.random(n) < 0.2] = -1
    return r


@pytest.mark.parametrize("seed", range(5))
def test_rank_metrics_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    ranks = _random_ranks(rng, int(rng.integers(1, 400)), 20000).reshape(-1)
    lst = ranks.tolist()
    rr = [1.0 / (r + 1) if r >= 0 else 0.0 for r in lst]
    assert np.allclose(met.reciprocal_rank(ranks), rr, rtol=0, atol=0)
    assert met.mean_reciprocal_rank(ranks) == pytest.approx(sum(rr) / len(rr), rel=1e-15)
    ranked = sorted(r for r in lst if r >= 0)
    if ranked:
        assert met.mean_rank(ranks) == pytest.approx(sum(ranked) / len(ranked), rel=1e-15)
        mid = len(ranked) // 2
        want = ranked[mid] if len(ranked) % 2 else (ranked[mid - 1] + ranked[mid]) / 2
        assert met.median_rank(ranks) == want
    ks = [1, 10, 500, 1000, 5000, 10000, 10 ** 6]
    want = [sum(1 for r in lst if 0 <= r < k) / len(lst) for k in ks]
    assert np.array_equal(met.recall_at(ranks, ks), np.asarray(want))
    # the 2-D form of rank_of's results is taken as it is
    two_d = np.concatenate([ranks, np.full((-ranks.size) % 4, -1)]).reshape(-1, 4)
    assert met.reciprocal_rank(two_d).shape == two_d.shape
    assert met.recall_at(two_d, [500])[0] == sum(1 for r in lst if 0 <= r < 500) / two_d.size


def test_rank_metrics_edge_cases():
    assert met.mean_reciprocal_rank([]) == 0.0 and np.array_equal(met.recall_at([], [5, 10]), [0.0, 0.0])
    assert np.isnan(met.mean_rank([-1, -1])) and np.isnan(met.median_rank([]))
    assert met.mean_reciprocal_rank([-1, 0]) == 0.5 and np.array_equal(met.recall_at([-1, 0, 4, 5], [5]), [0.5])
    with pytest.raises(ValueError):
        met.recall_at([-2], [1])


@pytest.mark.parametrize("seed", range(4))
def test_auc_row_against_brute_force(seed):
    """A random ordering of n columns, P of them answers: the formula of the docstring against counted pairs."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 300))
    P = int(rng.integers(1, min(n, 12) + 1))
    order = rng.permutation(n)                                    # order[p] = the column at place p
    answers = rng.permutation(n)[:P]
    place = np.empty(n, np.int64); place[order] = np.arange(n)
    ranks = place[answers]
    is_answer = np.zeros(n, bool); is_answer[answers] = True
    before = [sum(1 for p in range(place[a]) if not is_answer[order[p]]) for a in answers]     # non-answers ahead of each answer
    want = 1.0 - (sum(before) / P) / (n - 1)
    got = met.auc_row(np.concatenate([ranks, [-1, ranks[0]]]), n)        # a miss and a repeat change nothing
    assert got == pytest.approx(want, rel=1e-12, abs=1e-15)
    pairwise = 1.0 - sum(before) / (P * (n - P)) if n > P else None
    if pairwise is not None:
        assert got == pytest.approx(1.0 - (1.0 - pairwise) * (n - P) / (n - 1), rel=1e-12, abs=1e-15)
    assert met.auc_row([0], n) == 1.0 and met.auc_row([n - 1], n) == 0.0
    assert np.isnan(met.auc_row([-1], n)) and np.isnan(met.auc_row([0], 1))
    with pytest.raises(ValueError):
        met.auc_row([n], n)


# ---- [BASE] eval_ranks ---------------------------------------------------------------------------------------------------------------
def _conf(extra):
    from spotify_recsys_challenge_2018_amd.main import Conf
    ini = configparser.ConfigParser()
    ini.read_string("[BASE]\nverbose = False\ndata_dir = d\nresult_dir = r\ntestsize = 10\n" + extra)
    return Conf("somewhere", ini)


def test_eval_ranks_key():
    assert _conf("").eval_ranks == "off"
    assert _conf("eval_ranks = off\n").eval_ranks == "off"
    assert _conf("eval_ranks = On\n").eval_ranks == "on"
    with pytest.raises(ValueError, match="eval_ranks"):
        _conf("eval_ranks = deep\n")


def test_eval_ranks_is_refused_under_title_before_anything_is_read():
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    conf = _conf("eval_ranks = on\n")
    conf.mode = "title"                                           # what set_title_conf leaves; nothing else is set: nothing else is read
    with pytest.raises(ValueError, match="eval_ranks"):
        main_train.run(conf, True)
    conf.eval_ranks = "off"
    with pytest.raises(AttributeError):                           # ... and without the key the run goes on to its readers
        main_train.run(conf, True)


def test_rank_line_of_the_driver(monkeypatch):
    """eval_ranks() of the driver on a stub model: feed by feed, -1 answers in the denominators, the line's numbers."""
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    from spotify_recsys_challenge_2018_amd.models.stream_loop import SEEDS_FROM_INPUT

    class Reader:
        test_idx = 0
        batches = [([[0, 1]], [[1], [2]], [[5, -1], [7]]), ([[0, 3]], [[3]], [[9, 9, 11]])]

        def next_batch_test(self):
            pos, seeds, answers = self.batches[self.test_idx]
            self.test_idx = (self.test_idx + 1) % len(self.batches)
            return np.asarray(pos), seeds, answers, [None] * len(seeds), np.ones(len(pos), np.float32)

    class Model:
        calls = 0

        def rank_of(self, x_positions, x_ones, columns, seeds, n_rows=None):
            Model.calls += 1
            assert seeds == SEEDS_FROM_INPUT
            assert n_rows == len(columns)
            return [np.asarray([{5: 0, 7: 600, 9: 4999, 11: 20000}.get(c, -1) for c in row], np.int32) for row in columns]

    mrr, med, rec = main_train.eval_ranks(Reader(), None, Model())
    assert Model.calls == 2
    ranks = [0, -1, 600, 4999, 4999, 20000]
    assert mrr == pytest.approx(sum(1.0 / (r + 1) for r in ranks if r >= 0) / 6)
    assert med == 4999.0 and np.allclose(rec, [1 / 6, 2 / 6, 4 / 6, 4 / 6])
    lines = []
    monkeypatch.setattr(main_train, "log_write", lambda conf, log: lines.append(log))
    conf = type("C", (), {"eval_ranks": "on"})()
    main_train._log_ranks(conf, {"test-1": Reader()}, Model())
    assert len(lines) == 1 and lines[0].startswith("seed num: test-1 ranks: mrr ") and "recall@10000 0.666667" in lines[0]
    conf.eval_ranks = "off"
    main_train._log_ranks(conf, {"test-1": Reader()}, Model())
    assert len(lines) == 1                                        # absent / off: no line, the logs stay as they were


# ---- header and bindings ---------------------------------------------------------------------------------------------------------------
def _header_args(name):
    text = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["dae_rank_of_plan", "dae_decode_rank_of", "dae_score_rank_of"])
def test_header_and_bindings_agree(name):
    """Argument by argument: a pointer in the header is a void pointer (or a typed one) in _lib.py, an int an int."""
    import ctypes
    from spotify_recsys_challenge_2018_amd import _lib
    assert name in _lib.EXPORTS
    fn = getattr(_lib.load(), name)
    args = _header_args(name)
    assert len(fn.argtypes) == len(args), (name, args)
    for a, t in zip(args, fn.argtypes):
        if "*" in a or "[" in a:
            assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
        else:
            assert a.startswith("int ") and t is ctypes.c_int, (name, a, t)
    assert _lib.load().dae_version() >= 1001


def test_the_two_entry_points_take_the_same_tail():
    """dae_score_rank_of = the batch CSR and the encoder in front, then dae_decode_rank_of's arguments from W_dec on."""
    d, s = _header_args("dae_decode_rank_of"), _header_args("dae_score_rank_of")
    names = lambda xs: [re.sub(r".*[\s*]", "", a) for a in xs]
    tail = names(d)[names(d).index("n_tracks"):]
    assert names(s)[-len(tail):] == tail and names(s)[:6] == ["ctx", "row_ptr", "col", "val", "W_enc", "b_enc"]
