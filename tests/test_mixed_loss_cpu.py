"""CPU: what the held-out loss under the title mix needs no device for -- the [BASE] eval_mixed_loss key and where the drivers
refuse it by name, the driver's feeds and its line on a stub reader and model, DAE_title.mixed_loss' refusals on a model that was
never fitted, the panel walk and scratch carve-up of dae_mix_loss_rows as a stand-alone C++ program
(tests/host/mix_loss_plan_main.cpp), and the agreement of include/dae_hip.h with the ctypes binding of the new entry point."""
import configparser
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(extra):
    from spotify_recsys_challenge_2018_amd.main import Conf
    ini = configparser.ConfigParser()
    ini.read_string("[BASE]\nverbose = False\ndata_dir = d\nresult_dir = r\ntestsize = 10\n" + extra)
    return Conf("somewhere", ini)


# ---- 1. the key -----------------------------------------------------------------------------------------------------------------------
def test_eval_mixed_loss_key():
    assert _conf("").eval_mixed_loss == "off"
    assert _conf("eval_mixed_loss = off\n").eval_mixed_loss == "off"
    assert _conf("eval_mixed_loss = On\n").eval_mixed_loss == "on"
    assert _conf("eval_mixed_loss = on\n").eval_loss == "off"                  # a key of its own
    with pytest.raises(ValueError, match="eval_mixed_loss"):
        _conf("eval_mixed_loss = rows\n")
    from spotify_recsys_challenge_2018_amd import main
    assert "eval_mixed_loss = off | on" in main.__doc__


def test_eval_mixed_loss_is_refused_by_name_where_it_does_not_apply(monkeypatch):
    from spotify_recsys_challenge_2018_amd.main_runner import main_train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    conf = _conf("eval_mixed_loss = on\n")
    for mode in ("dae", "pretrain"):                              # outside --title: before anything is read
        conf.mode = mode
        with pytest.raises(ValueError, match="eval_mixed_loss.*--title only"):
            main_train.run(conf, True)
    conf.mode = "title"
    conf.ensemble = ["w_other"]                                   # beside an ensemble key
    with pytest.raises(ValueError, match="eval_mixed_loss.*ensemble"):
        main_train.run(conf, True)
    conf.ensemble = []
    monkeypatch.setenv("WORLD_SIZE", "2")                         # a training run over ranks: the title scorer is vocabulary-sharded
    with pytest.raises(ValueError, match="eval_mixed_loss.*sharded"):
        main_train.run(conf, False)
    monkeypatch.delenv("WORLD_SIZE")
    for testmode in (True, False):                                # accepted under --title: the run goes on to its readers
        with pytest.raises(AttributeError):
            main_train.run(conf, testmode)
    # eval_loss keeps refusing --title, and now names the key that does apply
    conf = _conf("eval_loss = on\n")
    conf.mode = "title"
    with pytest.raises(ValueError, match="eval_loss.*--title.*eval_mixed_loss = on"):
        main_train.run(conf, True)


def test_challenge_refuses_the_key_by_name(tmp_path):
    from spotify_recsys_challenge_2018_amd import main as cli
    run = tmp_path / "run"
    run.mkdir()
    (run / "config.ini").write_text(open(os.path.join(ROOT, "tests", "golden", "config.ini")).read()
                                    .replace("[BASE]", "[BASE]\neval_mixed_loss = on"))
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        with pytest.raises(ValueError, match="eval_mixed_loss.*--title only"):
            cli.main(["--dir", "run", "--challenge"])
    finally:
        os.chdir(cwd)


# ---- 2. the driver's line -------------------------------------------------------------------------------------------------------------
def test_mixed_loss_line_of_the_driver(monkeypatch):
    """eval_mixed_loss() on a stub reader and model: feed by feed from per-row values, so a short last feed is averaged correctly;
    the split's titles and titles_use as fed (no title: titles_use = 0 and an all-padding row); targets with weight 1."""
    from spotify_recsys_challenge_2018_amd.main_runner import main_train

    class Reader:
        test_idx = 0
        batches = [([[0, 1], [1, 2]], [[1], [2]], [[5, -1], [7]], [[3, 4, -1], None]), ([[0, 3]], [[3]], [[9, 9, 11]], [[8, -1, -1]])]

        def next_batch_test(self):
            pos, seeds, answers, titles = self.batches[self.test_idx]
            self.test_idx = (self.test_idx + 1) % len(self.batches)
            return np.asarray(pos), seeds, answers, titles, np.ones(len(pos), np.float32)

    class Model:
        n_input = 10
        calls = []

        def mixed_loss(self, x_positions, x_ones, y_positions, y_ones, titles, titles_use, n_rows=None, per_row=False):
            assert per_row and len(y_ones) == len(y_positions) and (np.asarray(y_ones) == 1).all()
            assert len(titles) == n_rows and len(titles_use) == n_rows
            Model.calls.append((np.asarray(y_positions).tolist(), [list(t) for t in titles], np.asarray(titles_use).tolist()))
            return 99.0, np.arange(1, n_rows + 1, dtype=np.float32) * (10.0 if n_rows == 1 else 1.0)

    conf = type("C", (), {"eval_mixed_loss": "on", "mode": "title", "strmaxlen": 3})()
    assert main_train.eval_mixed_loss(Reader(), conf, Model()) == pytest.approx((1.0 + 2.0 + 10.0) / 3)
    assert Model.calls == [([[0, 1], [0, 5], [1, 2], [1, 7]], [[3, 4, -1], [-1, -1, -1]], [1.0, 0.0]),
                           ([[0, 3], [0, 9]], [[8, -1, -1]], [1.0])]
    del Model.calls[:]
    lines = []
    monkeypatch.setattr(main_train, "log_write", lambda conf, log: lines.append(log))
    main_train._log_mixed_loss(conf, {"test-1": Reader()}, Model())
    assert lines == ["seed num: test-1 mixed heldout loss: %f" % (13.0 / 3)]
    conf.eval_mixed_loss = "off"
    main_train._log_mixed_loss(conf, {"test-1": Reader()}, Model())
    old = type("C", (), {"mode": "title", "strmaxlen": 3})()      # a conf from before the key
    main_train._log_mixed_loss(old, {"test-1": Reader()}, Model())
    assert len(lines) == 1                                        # absent / off: no line, the logs stay as they were


# ---- 3. the model's refusals ----------------------------------------------------------------------------------------------------------
def test_the_model_refuses_by_name_before_any_upload():
    from spotify_recsys_challenge_2018_amd import _lib
    from spotify_recsys_challenge_2018_amd.models.DAEs import DAE_title

    class C:
        save, initval, DAEval, batch, n_input, hidden, lr, reg_lambda = "s", "NULL", "NULL", 4, 40, 32, 0.01, 0.0
    args = ([[0, 1]], [1.0], [[0, 1]], [1.0])
    t = DAE_title(C(), None)                                      # no fit(), no title scorer: nothing of a device exists
    with pytest.raises(_lib.DaeError, match="mixed_loss.*no fitted title scorer"):
        t.mixed_loss(*args, [[1, 2]], [1.0])
    t.title_model = type("T", (), {"ctx": None})()                # a title model that was never fitted
    with pytest.raises(_lib.DaeError, match="mixed_loss.*no fitted title scorer"):
        t.mixed_loss(*args, [[1, 2]], [1.0])
    t.title_model.ctx = object()                                  # from here on the refusals come before the scorer is touched
    with pytest.raises(ValueError, match="mixed_loss.*titles are required"):
        t.mixed_loss(*args, None, [1.0])
    t._score_shard = {"rank": 0}
    with pytest.raises(_lib.DaeError, match="mixed_loss.*scoring shard"):
        t.mixed_loss(*args, [[1, 2]], [1.0])
    t._score_shard, t._title_sharded = None, object()
    with pytest.raises(_lib.DaeError, match="mixed_loss.*shard_title_training"):
        t.mixed_loss(*args, [[1, 2]], [1.0])
    t._title_sharded = None
    with pytest.raises(ValueError, match="mixed_loss.*n_rows = 5"):
        t.mixed_loss(*args, [[1, 2]], [1.0], n_rows=5)
    for kw in ({"keep_prob": 0.8}, {"input_keep_prob": 0.75}, {"title_keep_prob": 0.9}):
        with pytest.raises(ValueError, match="mixed_loss.*explicit seed"):
            t.mixed_loss(*args, [[1, 2]], [1.0], **kw)
    with pytest.raises(_lib.DaeError, match="DAE_title.loss.*titles in use"):       # `loss` stays what it was
        t.loss(*args, titles=[[1, 2]], titles_use=[1.0, 0.0, 0.0, 0.0])


# ---- 4. the plan ----------------------------------------------------------------------------------------------------------------------
def test_panel_walk_and_carve_up_as_a_standalone_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "mix_loss_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "mix_loss_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
    text = open(os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc", "mix_loss_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).replace("dae_hip.h", "").lower()      # a header with no HIP in it


# ---- 5. the ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    from spotify_recsys_challenge_2018_amd import _lib
    text = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    m = re.search(r"\bint\s+dae_mix_loss_rows\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 21 and "dae_mix_loss_rows" in _lib.EXPORTS
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "title_ctx", "dae", "h", "ld_h", "H", "W_dec", "b_dec", "feat", "ld_feat", "OutW_T", "Out_b", "w_title", "w_playlist", "B", "V",
        "n_batch", "y_row_ptr", "y_col", "y_val", "row_loss", "cost_out"]
    types = _lib.load().dae_mix_loss_rows.argtypes
    assert len(types) == 21
    for a, t in zip(args, types):
        want = ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[a.split()[0]]
        assert t is want, (a, t)
    assert hasattr(_lib.Context, "mix_loss_rows")
