"""CPU: what the titled rank_of (dae_mix_rank_of, DAE_title.mixed_rank_of, [BASE] eval_mixed_ranks) needs no device for -- the
new symbol in the header and the bindings, the plan at the title feature width, the config key, and the driver's line on a stub
model against brute force."""
import configparser
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc")


# ---- the symbol ------------------------------------------------------------------------------------------------------------------
def _header_args(name):
    text = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
    assert m, "%s is not declared in include/dae_hip.h" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_call_and_the_bindings_list_it():
    from spotify_recsys_challenge_2018_amd import _lib
    args = _header_args("dae_mix_rank_of")
    assert "dae_mix_rank_of" in _lib.EXPORTS
    fn = getattr(_lib.load(), "dae_mix_rank_of")
    assert len(fn.argtypes) == len(args) == 24, args
    for a, t in zip(args, fn.argtypes):
        if "*" in a:
            assert t is ctypes.c_void_p, (a, t)
        elif a.startswith("int64_t "):
            assert t is ctypes.c_int64, (a, t)
        else:
            assert a.startswith("int ") and t is ctypes.c_int, (a, t)
    assert callable(getattr(_lib.Context, "mix_rank_of"))
    assert _lib.load().dae_version() >= 1002


def test_the_call_is_mix_candidates_then_decode_rank_of():
    """dae_mix_candidates' arguments up to V, then dae_decode_rank_of's from n_tracks on (out_logit is out_score here)."""
    names = lambda xs: [re.sub(r".*[\s*]", "", a) for a in xs]
    m, c, d = (names(_header_args(n)) for n in ("dae_mix_rank_of", "dae_mix_candidates", "dae_decode_rank_of"))
    head = c[:c.index("V") + 1]
    tail = d[d.index("n_tracks"):]
    assert m[:len(head)] == head
    assert m[len(head):] == [("out_score" if a == "out_logit" else a) for a in tail]


def test_not_built_lists_no_longer_name_the_titled_score():
    """The header's and DESIGN section 4d's NOT BUILT lists."""
    for path in (os.path.join(ROOT, "include", "dae_hip.h"), os.path.join(ROOT, "DESIGN.md")):
        assert "the titled (mixed) score" not in open(path).read(), path


# ---- the plan at the title feature width ---------------------------------------------------------------------------------------------
def _header_constant(name):
    m = re.search(r"constexpr int %s = ([^;]+);" % name, open(os.path.join(CSRC, "rank_of_plan.h")).read())
    assert m, name
    return int(eval(m.group(1)))          # (an integer expression such as 160 * 1024)


def _capacity(rows, hp):
    """dae_rank_of_capacity, from the header's constants."""
    lds, reserve, slot, per_row, max_c = (_header_constant(n) for n in ("DAE_RO_LDS_BYTES", "DAE_RO_LDS_RESERVE", "DAE_RO_SLOT_BYTES",
                                                                         "DAE_RO_ROW_BYTES", "DAE_RO_MAX_C"))
    left = lds - reserve - rows * hp * 4 - rows * per_row
    return 0 if left <= 0 else min(left // (slot * rows), max_c)


def test_plan_at_the_shipped_title_feature_width():
    from spotify_recsys_challenge_2018_amd import _lib
    assert _capacity(64, 448) == 62 and _capacity(32, 448) == 274 and _capacity(128, 448) == 0
    a = _lib.rank_of_plan(64, 448, 64)
    assert a["rows"] == 64 and a["capacity"] == 62 == _capacity(64, 448) and a["row_groups"] == 1
    b = _lib.rank_of_plan(64, 448, 64 * 100)
    assert b["rows"] == 32 and b["capacity"] == 274 == _capacity(32, 448) and b["row_groups"] == 2
    # a width that is no multiple of 32 is padded to one: 80 -> 96
    c = _lib.rank_of_plan(40, 80, 40)
    assert c["rows"] == 64 and c["capacity"] == _capacity(64, 96)


# ---- [BASE] eval_mixed_ranks -------------------------------------------------------------------------------------------------------
def _conf(extra):
    from spotify_recsys_challenge_2018_amd.main import Conf
    ini = configparser.ConfigParser()
    ini.read_string("[BASE]\nverbose = False\ndata_dir = d\nresult_dir = r\ntestsize = 10\n" + extra)
    return Conf("somewhere", ini)


def test_eval_mixed_ranks_key():
    assert _conf("").eval_mixed_ranks == "off"
    assert _conf("eval_mixed_ranks = off\n").eval_mixed_ranks == "off"
    assert _conf("eval_mixed_ranks = On\n").eval_mixed_ranks == "on"
    assert _conf("eval_mixed_ranks = on\n").eval_ranks == "off"           # the two keys are independent
    with pytest.raises(ValueError, match="eval_mixed_ranks"):
        _conf("eval_mixed_ranks = deep\n")


@pytest.mark.parametrize("mode", ["dae", "pretrain"])
def test_eval_mixed_ranks_is_refused_outside_title_before_anything_is_read(mode):
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    conf = _conf("eval_mixed_ranks = on\n")
    conf.mode = mode                                              # nothing else is set: nothing else is read
    with pytest.raises(ValueError, match="eval_mixed_ranks"):
        main_train.run(conf, True)
    conf.mode = "title"
    with pytest.raises(AttributeError):                           # ... under --title the run goes on to its readers
        main_train.run(conf, True)
    conf.eval_ranks = "on"
    with pytest.raises(ValueError, match="eval_ranks"):           # the plain key stays refused there
        main_train.run(conf, True)


def test_challenge_refuses_the_key_by_name(tmp_path):
    from spotify_recsys_challenge_2018_amd import main as cli
    golden = os.path.join(ROOT, "tests", "golden", "config.ini")
    (tmp_path / "run").mkdir()
    open(tmp_path / "run" / "config.ini", "w").write(open(golden).read().replace("[BASE]", "[BASE]\neval_mixed_ranks = on"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with pytest.raises(ValueError, match="eval_mixed_ranks"):
            cli.main(["--dir", "run", "--challenge"])
    finally:
        os.chdir(cwd)


def test_mixed_rank_line_of_the_driver(monkeypatch):
    """eval_mixed_ranks() of the driver on a stub model: feed by feed, the split's titles and titles_use as the title evaluation
    feeds them, -1 answers in the denominators, the line's numbers against brute force."""
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    from spotify_recsys_challenge_2018_amd.models.stream_loop import SEEDS_FROM_INPUT
    L = 4
    table = {5: 0, 7: 600, 9: 4999, 11: 20000, 13: 499}

    class Reader:
        test_idx = 0
        batches = [([[0, 1]], [[1], [2]], [[5, -1], [7]], [[3, 1, -1, -1], None]),
                   ([[0, 3]], [[3]], [[9, 9, 11, 13]], [[2, 2, 2, 2]])]

        def next_batch_test(self):
            pos, seeds, answers, titles = self.batches[self.test_idx]
            self.test_idx = (self.test_idx + 1) % len(self.batches)
            return np.asarray(pos), seeds, answers, titles, np.ones(len(pos), np.float32)

    class Model:
        calls = []

        def mixed_rank_of(self, x_positions, x_ones, columns, seeds, titles, titles_use, n_rows=None, want_scores=False):
            Model.calls.append((titles, np.asarray(titles_use).tolist()))
            assert seeds == SEEDS_FROM_INPUT and n_rows == len(columns) == len(titles) and not want_scores
            return [np.asarray([table.get(c, -1) for c in row], np.int32) for row in columns]

    conf = type("C", (), {})()
    conf.strmaxlen, conf.eval_mixed_ranks, conf.mode = L, "on", "title"
    mrr, med, rec = main_train.eval_mixed_ranks(Reader(), conf, Model())
    assert Model.calls == [([[3, 1, -1, -1], [-1] * L], [1.0, 0.0]), ([[2, 2, 2, 2]], [1.0])]
    ranks = [0, -1, 600, 4999, 4999, 20000, 499]
    assert mrr == pytest.approx(sum(1.0 / (r + 1) for r in ranks if r >= 0) / len(ranks))
    ranked = sorted(r for r in ranks if r >= 0)
    assert med == (ranked[2] + ranked[3]) / 2
    want = [sum(1 for r in ranks if 0 <= r < k) / len(ranks) for k in main_train.RANK_CUTS]
    assert np.allclose(rec, want, rtol=0, atol=1e-15) and want == [2 / 7, 3 / 7, 5 / 7, 5 / 7]

    lines = []
    monkeypatch.setattr(main_train, "log_write", lambda conf, log: lines.append(log))
    main_train._log_mixed_ranks(conf, {"test-1": Reader()}, Model())
    assert len(lines) == 1 and lines[0].startswith("seed num: test-1 mixed ranks: mrr ")
    w = lines[0].split()
    assert float(w[w.index("mrr") + 1]) == pytest.approx(mrr, abs=1e-6) and float(w[w.index("median") + 1]) == med
    assert [float(w[w.index("recall@%d" % k) + 1]) for k in main_train.RANK_CUTS] == [round(v, 6) for v in want]
    for key, mode in (("off", "title"), ("on", "dae")):           # off, or outside --title: no line
        conf.eval_mixed_ranks, conf.mode = key, mode
        main_train._log_mixed_ranks(conf, {"test-1": Reader()}, Model())
    assert len(lines) == 1
    del conf.eval_mixed_ranks                                     # absent: no line either
    main_train._log_mixed_ranks(conf, {"test-1": Reader()}, Model())
    assert len(lines) == 1
