"""CPU: what of the ranks under the ensemble needs no device (DESIGN.md 4e "Ranks under the ensemble").
1. utils/ensemble_fit.py search_simplex: against brute force (M = 2), as a pair-move local search (M = 3), its tie rules, its memo.
2. The drivers' keys [BASE] eval_ensemble_ranks / ensemble_fit: parsed, defaulted, refused by name in each wrong place.
3. DAE_ensemble.rank_of / fit_alphas argument refusals, with stub members in the models' place.
4. The scratch carve-up of dae_ensemble_rank_of as a stand-alone C++ program (tests/host/ensemble_rank_of_plan_main.cpp).
5. main_train.eval_ensemble_ranks on a stub model and reader: feed by feed, -1 answers in the denominators, the line's format."""
import itertools
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import main as cli
from spotify_recsys_challenge_2018_amd.main_runner import main_challenge, main_train
from spotify_recsys_challenge_2018_amd.models.ensemble import DAE_ensemble, SEEDS_FROM_INPUT, split_feeds
from spotify_recsys_challenge_2018_amd.utils.ensemble_fit import grid_alphas, parse_metric, search_simplex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---- 1. the search ----------------------------------------------------------------------------------------------------------------
def _counted(f):
    calls = []

    def g(a):
        assert a.dtype == np.float32 and abs(float(a.sum()) - 1.0) < 1e-6 and (a >= 0).all()
        calls.append(tuple(a.tolist()))
        return f(a)
    return g, calls


@pytest.mark.parametrize("steps", [1, 2, 3, 7, 10, 16])
def test_two_members_evaluate_the_whole_grid_and_match_brute_force(steps):
    rng = np.random.default_rng(steps)
    table = rng.integers(0, 4, steps + 1).astype(float)                       # few distinct values: ties are common
    f, calls = _counted(lambda a: table[int(round(float(a[0]) * steps))])
    alphas, value, trace = search_simplex(f, 2, steps=steps, rounds=4)
    assert len(calls) == steps + 1 == len(trace) and len(set(calls)) == steps + 1
    assert [int(round(c[0] * steps)) for c in calls] == list(range(steps + 1))          # alpha_0 ascending
    best = int(np.argmax(table))                                              # (argmax: the first of the ties)
    assert value == table[best] and np.array_equal(alphas, grid_alphas((best, steps - best), steps))
    assert all(np.array_equal(t[0], np.asarray(c, np.float32)) and t[1] == f(t[0]) for t, c in zip(trace, calls[:steps + 1]))


def test_one_member_is_one():
    alphas, value, trace = search_simplex(lambda a: 3.5, 1, steps=10)
    assert np.array_equal(alphas, np.ones(1, np.float32)) and value == 3.5 and len(trace) == 1


def _neighbours(pt):
    for i, j in itertools.permutations(range(len(pt)), 2):
        if pt[j] > 0:
            q = list(pt)
            q[i] += 1
            q[j] -= 1
            yield tuple(q)


def test_three_members_on_a_concave_separable_function():
    steps, target = 10, np.asarray([0.62, 0.29, 0.09])

    def concave(a):
        return -float(((np.asarray(a, np.float64) - target) ** 2).sum())
    f, calls = _counted(concave)
    alphas, value, trace = search_simplex(f, 3, steps=steps, rounds=50)
    pt = tuple(int(round(float(x) * steps)) for x in alphas)
    assert sum(pt) == steps and np.array_equal(alphas, grid_alphas(pt, steps))
    # a pair-move local optimum, no worse than every start; on a concave function over this grid that is the global optimum
    assert all(concave(grid_alphas(q, steps)) <= value for q in _neighbours(pt))
    starts = [(10, 0, 0), (0, 10, 0), (0, 0, 10), (4, 3, 3)]
    assert [tuple(int(round(x * steps)) for x in c) for c in calls[:4]] == starts          # the corners, then the centre
    assert all(value >= concave(grid_alphas(s, steps)) for s in starts)
    grid = [(i, j, steps - i - j) for i in range(steps + 1) for j in range(steps + 1 - i)]
    assert value == max(concave(grid_alphas(q, steps)) for q in grid) and pt == (6, 3, 1)
    # memoised: every evaluated point once, in the trace in order
    assert len(calls) == len(set(calls)) == len(trace) < len(grid)
    assert all(np.array_equal(t[0], np.asarray(c, np.float32)) for t, c in zip(trace, calls))
    # deterministic
    again = search_simplex(concave, 3, steps=steps, rounds=50)
    assert np.array_equal(again[0], alphas) and again[1] == value and len(again[2]) == len(trace)
    # rounds bounds the sweeps: none leaves the best start
    a0, v0, t0 = search_simplex(concave, 3, steps=steps, rounds=0)
    assert len(t0) == 4 and v0 == max(concave(grid_alphas(s, steps)) for s in starts)


def test_ties_go_to_the_earlier_candidate_and_moves_need_a_strict_improvement():
    f, calls = _counted(lambda a: 1.0)                                        # flat: nothing improves
    alphas, value, trace = search_simplex(f, 3, steps=4, rounds=4)
    assert np.array_equal(alphas, np.asarray([1, 0, 0], np.float32))          # the first corner, and it stays
    assert len(calls) == 4 + 2                                                # starts + the two moves off that corner, one sweep
    # the centre gives the remainder to the first members
    seen = []
    search_simplex(lambda a: seen.append(tuple(a.tolist())) or 0.0, 4, steps=6, rounds=0)
    assert seen[4] == tuple(grid_alphas((2, 2, 1, 1), 6).tolist())
    # equal corners: the earlier one; a later strictly better candidate wins
    assert np.array_equal(search_simplex(lambda a: float(a[1] == 1 or a[2] == 1), 3, steps=2, rounds=0)[0], [0, 1, 0])
    for bad in (dict(M=0), dict(M=2, steps=0), dict(M=2, rounds=-1)):
        with pytest.raises(ValueError, match="search_simplex"):
            search_simplex(lambda a: 0.0, bad.get("M", 2), steps=bad.get("steps", 4), rounds=bad.get("rounds", 1))


def test_metrics_by_name():
    ranks = np.asarray([0, 1, -1, 9, 499, 500])
    assert parse_metric("mrr")(ranks) == pytest.approx((1 + 0.5 + 0 + 0.1 + 1 / 500 + 1 / 501) / 6)
    assert parse_metric("recall@500")(ranks) == pytest.approx(4 / 6) and parse_metric("recall@1")(ranks) == pytest.approx(1 / 6)
    for bad in ("ndcg", "recall@", "recall@0", "recall@x", None):
        with pytest.raises(ValueError, match="metric"):
            parse_metric(bad)


# ---- 2. the keys ------------------------------------------------------------------------------------------------------------------
def _run_dir(tmp, base_keys=""):
    run = os.path.join(str(tmp), "run")
    os.makedirs(run, exist_ok=True)
    ini = open(os.path.join(G, "config.ini")).read()
    ini = ini.replace("[BASE]", "[BASE]\n" + base_keys) if base_keys else ini
    open(os.path.join(run, "config.ini"), "w").write(ini)
    return run


def test_keys_defaults_and_values(tmp_path):
    conf = cli.load_conf(_run_dir(tmp_path))
    assert conf.eval_ensemble_ranks == "off" and conf.ensemble_fit is None
    conf = cli.load_conf(_run_dir(tmp_path, "ensemble = w_pretrain\neval_ensemble_ranks = On\nensemble_fit = 5"))
    assert conf.eval_ensemble_ranks == "on" and conf.ensemble_fit == ("test-5", "mrr")
    conf = cli.load_conf(_run_dir(tmp_path, "ensemble = w_pretrain\nensemble_fit = 25r , Recall@500"))
    assert conf.ensemble_fit == ("test-25r", "recall@500")
    assert cli.load_conf(_run_dir(tmp_path, "ensemble = w_pretrain\nensemble_fit =")).ensemble_fit is None


@pytest.mark.parametrize("keys, match", [
    ("eval_ensemble_ranks = maybe", "eval_ensemble_ranks must be one of off | on"),
    ("ensemble_fit = 5", "ensemble_fit is set without"),
    ("ensemble = w_pretrain\nensemble_alpha = 0.5, 0.5\nensemble_fit = 5", "ensemble_fit and .BASE. ensemble_alpha are both set"),
    ("ensemble = w_pretrain\nensemble_fit = 5, ndcg", "metric must be mrr or recall@N"),
    ("ensemble = w_pretrain\nensemble_fit = 5, mrr, 3", "<seed>"),
])
def test_malformed_keys_are_refused_by_name(tmp_path, keys, match):
    with pytest.raises(ValueError, match=match):
        cli.load_conf(_run_dir(tmp_path, keys))


def _no_driver(monkeypatch):
    monkeypatch.setattr(main_train, "run", lambda *a, **kw: pytest.fail("the driver ran"))
    monkeypatch.setattr(main_challenge, "run", lambda *a, **kw: pytest.fail("the driver ran"))


@pytest.mark.parametrize("keys, flags, match", [
    ("eval_ensemble_ranks = on", ["--dae", "--testmode"], "eval_ensemble_ranks = on is set without"),
    ("eval_ensemble_ranks = on", ["--dae"], "eval_ensemble_ranks = on is set without"),
    ("eval_ensemble_ranks = on", ["--challenge"], "eval_ensemble_ranks = on is set without"),
    ("ensemble = w\neval_ensemble_ranks = on", ["--challenge"], "eval_ensemble_ranks = on is honoured by"),
    ("ensemble = w\neval_ensemble_ranks = on", ["--pretrain", "--testmode"], r"\[BASE\] ensemble"),
    ("ensemble = w\nensemble_fit = 77", ["--dae", "--testmode"], "ensemble_fit = test-77: the split's file .* is missing"),
    ("ensemble = w\nensemble_fit = 77", ["--challenge"], "ensemble_fit = test-77: the split's file .* is missing"),
])
def test_keys_in_the_wrong_place_are_refused_before_anything_is_read(tmp_path, monkeypatch, keys, flags, match):
    _run_dir(tmp_path, keys)
    monkeypatch.chdir(tmp_path)
    _no_driver(monkeypatch)
    with pytest.raises(ValueError, match=match):
        cli.main(["--dir", "run"] + flags)


@pytest.mark.parametrize("flags", [["--dae", "--testmode"], ["--title", "--testmode"]])
def test_keys_in_the_right_place_reach_their_driver(tmp_path, flags, monkeypatch):
    _run_dir(tmp_path, "ensemble = w_pretrain\neval_ensemble_ranks = on\nensemble_fit = 5")
    shutil.copytree(os.path.join(G, "data"), str(tmp_path / "data"))                  # test-5 exists
    monkeypatch.chdir(tmp_path)
    seen = []
    monkeypatch.setattr(main_train, "run", lambda conf, tm: seen.append((conf.eval_ensemble_ranks, conf.ensemble_fit, tm)))
    assert cli.main(["--dir", "run"] + flags) == 0
    assert seen == [("on", ("test-5", "mrr"), True)]


def test_main_train_refuses_the_keys_itself(tmp_path):
    """... for a caller that goes past main.py; the older rank keys beside an ensemble stay refused as they were."""
    conf = types.SimpleNamespace(ensemble=[], mode="dae", eval_ranks="off", eval_mixed_ranks="off", eval_ensemble_ranks="on")
    with pytest.raises(ValueError, match="eval_ensemble_ranks = on is set without"):
        main_train.run(conf, True)
    conf = types.SimpleNamespace(ensemble=["w"], mode="dae", eval_ranks="off", eval_mixed_ranks="off", ensemble_fit=("test-77", "mrr"),
                                 data_dir=str(tmp_path))
    with pytest.raises(ValueError, match="test-77: the split's file"):
        main_train.run(conf, True)
    conf = types.SimpleNamespace(ensemble=["w"], mode="dae", eval_ranks="on", eval_mixed_ranks="off", eval_ensemble_ranks="on")
    with pytest.raises(ValueError, match="eval_ranks = on: an ensemble has no rank_of"):
        main_train.run(conf, True)


# ---- 3. DAE_ensemble's arguments ----------------------------------------------------------------------------------------------------
def _stub(n_input=1000, n_tracks=800, hidden=64, batch=16, **kw):
    return types.SimpleNamespace(n_input=n_input, n_tracks=n_tracks, n_hidden=hidden, n_batch=batch, weights={}, biases={},
                                 ctx=object(), device_index=0, _score_shard=None, **kw)


def test_rank_of_and_fit_alphas_refuse_by_name_before_anything_is_launched():
    a, b = _stub(), _stub()
    ens = DAE_ensemble([a, b])
    feed = (np.zeros((0, 2), np.int64), np.zeros(0, np.float32), [[1, 2]] * 16, [[] for _ in range(16)])
    with pytest.raises(ValueError, match="rank_of: ranks inside a catalogue are not built"):
        ens.rank_of(*feed, catalogue=object())
    with pytest.raises(ValueError, match="metric 'ndcg'"):
        ens.fit_alphas([feed + (16,)], metric="ndcg")
    b._score_shard = {"rank": 0}
    with pytest.raises(ValueError, match="member 1 has a scoring shard"):
        ens.rank_of(*feed)
    with pytest.raises(ValueError, match="member 1 has a scoring shard"):
        ens.fit_alphas([feed + (16,)])
    assert np.array_equal(ens.alphas, np.full(2, np.float32(0.5)))            # a failed fit leaves the alphas as they were
    per_row = DAE_ensemble([_stub(), _stub()], alphas=np.full((2, 16), 0.5))
    with pytest.raises(ValueError, match=r"fit_alphas: per-row alphas \(an array \[M, n_rows\]\)"):
        per_row.fit_alphas([feed + (16,)])
    assert not hasattr(ens, "evaluate_iter")


def test_fit_alphas_searches_over_rank_of_and_keeps_the_best(monkeypatch):
    """With rank_of replaced by a function of the alphas: the metric is taken over the concatenated ranks of all feeds, -1 counting
    in the denominator, and the ensemble ends with the best grid point."""
    ens = DAE_ensemble([_stub(), _stub()])
    seen = []

    def rank_of(x_positions, x_ones, columns, seeds, n_rows=None, **kw):
        seen.append((tuple(ens.alphas.tolist()), n_rows, tuple(sorted(kw))))
        r = int(round(abs(float(ens.alphas[0]) - 0.3) * 10))                  # best at alpha_0 = 0.3
        return [np.asarray([r, -1], np.int32) for _ in range(n_rows)]
    monkeypatch.setattr(ens, "rank_of", rank_of)
    feeds = [("p", "o", "ans", SEEDS_FROM_INPUT, 3), ("p", "o", "ans", SEEDS_FROM_INPUT, 2, "titles", "use")]
    alphas, value, trace = ens.fit_alphas(feeds, steps=10)
    assert np.array_equal(alphas, np.asarray([0.3, 0.7], np.float32)) and np.array_equal(ens.alphas, alphas)
    assert value == 0.5 and len(trace) == 11 and len(seen) == 22              # (1 / 1 + 0) / 2; both feeds at every point
    assert seen[0][1:] == (3, ()) and seen[1][1:] == (2, ("titles", "titles_use"))


# ---- 4. the scratch carve-up ----------------------------------------------------------------------------------------------------------
def test_scratch_carve_up_as_a_standalone_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "ensemble_rank_of_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "ensemble_rank_of_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


# ---- 5. the evaluation line -----------------------------------------------------------------------------------------------------------
class _Reader:
    """Two batches of a test split in the reader's protocol."""

    def __init__(self):
        self.test_idx, self.n = 0, 0
        self.batches = [([[0, 1]], [[1], [2]], [[5, 6, -1], [7]], [[3, 4], None], [1.0]),
                        ([[0, 2]], [[3]], [[8, 9]], [None], [1.0])]

    def next_batch_test(self):
        b = self.batches[self.n]
        self.n = (self.n + 1) % len(self.batches)
        self.test_idx = self.n
        return b


class _Model:
    def __init__(self):
        self.calls = []

    def rank_of(self, x_positions, x_ones, columns, seeds, n_rows=None, **kw):
        self.calls.append((columns, seeds, n_rows, kw))
        return [np.asarray([-1 if c < 0 else (c - 5) * 300 for c in row], np.int32) for row in columns]


def test_eval_ensemble_ranks_feed_by_feed_and_the_line(tmp_path):
    m = _Model()
    conf = types.SimpleNamespace(mode="dae", dir=str(tmp_path), verbose=False, eval_ensemble_ranks="on")
    mrr, med, rec = main_train.eval_ensemble_ranks(_Reader(), conf, m)
    # ranks 0, 300, -1, 600 | 900, 1200: six answers, the -1 a miss in every denominator
    assert mrr == pytest.approx((1 + 1 / 301 + 0 + 1 / 601 + 1 / 901 + 1 / 1201) / 6) and med == 600.0
    assert np.allclose(rec, [2 / 6, 4 / 6, 5 / 6, 5 / 6])
    assert [(c[0], c[1], c[2], c[3]) for c in m.calls] == [([[5, 6, -1], [7]], SEEDS_FROM_INPUT, 2, {}), ([[8, 9]], SEEDS_FROM_INPUT, 1, {})]
    main_train._log_ensemble_ranks(conf, {"test-5": _Reader()}, m)
    line = open(tmp_path / "log.txt").read().splitlines()
    assert line == ["seed num: test-5 ensemble ranks: mrr %f median 600.0 recall@500 %f recall@1000 %f recall@5000 %f recall@10000 %f"
                    % (mrr, 2 / 6, 4 / 6, 5 / 6, 5 / 6)]
    # off: no line, no call; under --title the feeds carry the titles (a row without one: all padding, titles_use = 0)
    n = len(m.calls)
    conf.eval_ensemble_ranks = "off"
    main_train._log_ensemble_ranks(conf, {"test-5": _Reader()}, m)
    assert len(m.calls) == n and len(open(tmp_path / "log.txt").read().splitlines()) == 1
    f = next(split_feeds(_Reader(), True, 3))
    assert f[5] == [[3, 4], [-1, -1, -1]] and f[6].tolist() == [1.0, 0.0] and f[4] == 2 and f[3] == SEEDS_FROM_INPUT
    conf.mode, conf.strmaxlen = "title", 3
    main_train.eval_ensemble_ranks(_Reader(), conf, m)
    assert m.calls[-2][3]["titles"] == [[3, 4], [-1, -1, -1]] and m.calls[-1][3]["titles_use"].tolist() == [0.0]
