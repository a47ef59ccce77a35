"""CPU: what of the ensembles needs no device.
1. The plans of the ranking call of an ensemble -- the mixed score on a DAE's own hidden-256 context -- as a stand-alone C++
   program (tests/host/ensemble_plan_main.cpp over csrc/score_plan.h), shaped like tests/test_score_plan_cpu.py.
2. The drivers' keys: [BASE] ensemble / ensemble_alpha parsed by main.py, honoured or refused by name.
3. DAE_ensemble's argument checking, with stub members in the models' place."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import main as cli
from spotify_recsys_challenge_2018_amd.main_runner import main_challenge, main_train
from spotify_recsys_challenge_2018_amd.models.ensemble import DAE_ensemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


# ---- 1. the plans ---------------------------------------------------------------------------------------------------------------
def test_mixed_plans_on_a_dae_context_as_a_standalone_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "ensemble_plan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "ensemble_plan_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


# ---- 2. the keys ------------------------------------------------------------------------------------------------------------------
def _run_dir(tmp, base_keys="", challenge_keys=""):
    run = os.path.join(str(tmp), "run")
    os.makedirs(run, exist_ok=True)
    ini = open(os.path.join(G, "config.ini")).read()
    ini = ini.replace("[BASE]", "[BASE]\n" + base_keys) if base_keys else ini
    ini = ini.replace("[CHALLENGE]", "[CHALLENGE]\n" + challenge_keys) if challenge_keys else ini
    open(os.path.join(run, "config.ini"), "w").write(ini)
    return run


def test_keys_are_optional_and_parsed_like_the_other_optional_keys(tmp_path):
    conf = cli.load_conf(_run_dir(tmp_path))
    assert conf.ensemble == [] and conf.ensemble_alpha is None                 # absent: every run is what it is today
    run = _run_dir(tmp_path, "ensemble = w_pretrain ,  other/w_dae_h96")
    conf = cli.load_conf(run)
    assert conf.ensemble == [os.path.join(run, "w_pretrain"), os.path.join(run, "other/w_dae_h96")]        # as DAEval resolves
    assert conf.ensemble_alpha is None
    conf = cli.load_conf(_run_dir(tmp_path, "ensemble = w_pretrain\nensemble_alpha = 0.25, 0.75"))
    assert conf.ensemble_alpha == [0.25, 0.75]
    conf.set_dae_conf()
    conf.set_title_conf()
    assert conf.DAEval == os.path.join(run, "w_dae") and len(conf.ensemble) == 1
    assert cli.load_conf(_run_dir(tmp_path, "ensemble =")).ensemble == []


@pytest.mark.parametrize("keys, match", [
    ("ensemble = w_pretrain\nensemble_alpha = 0.5", "lists 1 weights for 2 members"),
    ("ensemble = a, b\nensemble_alpha = 0.5, 0.2", "lists 2 weights for 3 members"),
    ("ensemble_alpha = 0.5, 0.5", "ensemble_alpha is set without"),
    ("ensemble = w_pretrain\nensemble_alpha = half, half", "list of numbers"),
    ("ensemble = w_pretrain,, w_dae", "empty entry"),
])
def test_malformed_keys_are_refused_by_name(tmp_path, keys, match):
    with pytest.raises(ValueError, match=match):
        cli.load_conf(_run_dir(tmp_path, keys))


@pytest.mark.parametrize("flags", [["--pretrain"], ["--dae"], ["--title"], ["--pretrain", "--testmode"]])
def test_runs_that_do_not_honour_the_key_refuse_it_before_anything_is_read(tmp_path, flags, monkeypatch):
    """A training run (and --pretrain --testmode) refuses [BASE] ensemble by name; no reader and no model is built."""
    _run_dir(tmp_path, "ensemble = w_pretrain")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(main_train, "run", lambda *a, **kw: pytest.fail("the driver ran"))
    with pytest.raises(ValueError, match=r"\[BASE\] ensemble"):
        cli.main(["--dir", "run"] + flags)


@pytest.mark.parametrize("flags", [["--dae", "--testmode"], ["--title", "--testmode"], ["--challenge"]])
def test_runs_that_honour_the_key_reach_their_driver(tmp_path, flags, monkeypatch):
    _run_dir(tmp_path, "ensemble = w_pretrain\nensemble_alpha = 0.5, 0.5")
    monkeypatch.chdir(tmp_path)
    seen = []
    monkeypatch.setattr(main_train, "run", lambda conf, tm: seen.append(("train", conf.ensemble, conf.ensemble_alpha, tm)))
    monkeypatch.setattr(main_challenge, "run", lambda conf: seen.append(("challenge", conf.ensemble, conf.ensemble_alpha, None)))
    assert cli.main(["--dir", "run"] + flags) == 0
    assert len(seen) == 1 and seen[0][1] == [os.path.join(".", "run", "w_pretrain")] and seen[0][2] == [0.5, 0.5]


def test_main_train_refuses_the_key_itself():
    """... for a caller that goes past main.py: in a training run, in --pretrain --testmode, and beside the rank lines."""
    conf = types.SimpleNamespace(ensemble=["w"], mode="dae", eval_ranks="off", eval_mixed_ranks="off")
    with pytest.raises(ValueError, match="training run"):
        main_train.run(conf, False)
    conf.mode = "pretrain"
    with pytest.raises(ValueError, match="--pretrain --testmode"):
        main_train.run(conf, True)
    conf.mode, conf.eval_ranks = "dae", "on"
    with pytest.raises(ValueError, match="eval_ranks"):
        main_train.run(conf, True)


def test_challenge_refuses_the_key_where_the_plain_dae_would_shard_and_with_a_catalogue(tmp_path, monkeypatch):
    """Like `catalogue`: under torch.distributed.run the plain DAE runs vocabulary-sharded, which an ensemble is not -- refused
    on every rank before the process group; a titled run (batches dealt to the ranks) is not refused here."""
    monkeypatch.setattr(main_challenge, "_init_distributed", lambda conf: pytest.fail("the process group was reached"))
    conf = types.SimpleNamespace(ensemble=["w"], char_model="Char_CNN", title_save=str(tmp_path / "none"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="vocabulary-sharded over 2 ranks"):
        main_challenge.run(conf)
    conf.catalogue = "cat.txt"
    with pytest.raises(ValueError, match="catalogue"):
        main_challenge.run(conf)
    # titled (the title pickle exists): past the refusals
    open(str(tmp_path / "t.pkl"), "wb").close()
    conf = types.SimpleNamespace(ensemble=["w"], char_model="Char_CNN", title_save=str(tmp_path / "t"))

    class Reached(Exception):
        pass

    def reached(conf):
        raise Reached()
    monkeypatch.setattr(main_challenge, "_init_distributed", reached)
    with pytest.raises(Reached):
        main_challenge.run(conf)


# ---- 3. DAE_ensemble's arguments -----------------------------------------------------------------------------------------------------
def _stub(n_input=1000, n_tracks=800, hidden=64, batch=16, ctx=True, **kw):
    return types.SimpleNamespace(n_input=n_input, n_tracks=n_tracks, n_hidden=hidden, n_batch=batch, weights={}, biases={},
                                 ctx=object() if ctx else None, device_index=0, _score_shard=None, **kw)


def test_members_must_be_fitted_models_over_one_vocabulary():
    a, b = _stub(), _stub(hidden=256)
    ens = DAE_ensemble([a, b])
    assert ens.n_input == 1000 and ens.n_tracks == 800 and ens.n_batch == 16
    assert ens.alphas.dtype == np.float32 and np.array_equal(ens.alphas, np.full(2, np.float32(0.5)))
    assert np.array_equal(DAE_ensemble([a, b, _stub()]).alphas, np.full(3, np.float32(1) / np.float32(3)))      # float32(1 / M)
    with pytest.raises(ValueError, match="at least one member"):
        DAE_ensemble([])
    with pytest.raises(ValueError, match="member 1 has n_input = 999, member 0 has 1000"):
        DAE_ensemble([a, _stub(n_input=999)])
    with pytest.raises(ValueError, match="member 2 has n_tracks = 700, member 0 has 800"):
        DAE_ensemble([a, b, _stub(n_tracks=700)])
    with pytest.raises(ValueError, match="member 1 is not fitted"):
        DAE_ensemble([a, _stub(ctx=False)])
    with pytest.raises(ValueError, match="member 1 is listed twice"):
        DAE_ensemble([a, a])
    with pytest.raises(ValueError, match="member 0 is no DAE"):
        DAE_ensemble([object()])
    with pytest.raises(ValueError, match="title model is not fitted"):
        DAE_ensemble([a], title_model=types.SimpleNamespace(ctx=None, output_dim=1000))
    with pytest.raises(ValueError, match="title model scores 900 columns"):
        DAE_ensemble([a], title_model=types.SimpleNamespace(ctx=object(), output_dim=900))


def test_alphas_are_m_floats_or_an_array_of_rows():
    a, b = _stub(), _stub()
    assert np.array_equal(DAE_ensemble([a, b], alphas=[0.25, 0.75]).alphas, np.array([0.25, 0.75], np.float32))
    per_row = np.arange(32, dtype=np.float64).reshape(2, 16) / 32
    ens = DAE_ensemble([a, b], alphas=per_row)
    assert ens.alphas.shape == (2, 16) and ens.alphas.dtype == np.float32
    for bad in ([0.5], [0.2, 0.3, 0.5], np.zeros((3, 16)), 0.5, np.zeros((2, 4, 4))):
        with pytest.raises(ValueError, match="alphas must be 2 floats or an array"):
            DAE_ensemble([a, b], alphas=bad)


def test_limits_are_refused_by_name_before_anything_is_launched():
    """k > 1024, a catalogue, a member with a scoring shard: ValueError naming the limit (the stubs have no device to launch on)."""
    a, b = _stub(), _stub()
    ens = DAE_ensemble([a, b])
    feed = (np.zeros((0, 2), np.int64), np.zeros(0, np.float32), [[] for _ in range(16)])
    with pytest.raises(ValueError, match=r"1 <= k <= 1024 tracks per row \(got 1025\)"):
        ens.recommend(*feed, k=1025)
    with pytest.raises(ValueError, match="1 <= k <= 1024"):
        next(ens.recommend_iter([feed + (16,)], k=2000))
    with pytest.raises(ValueError, match="does not rank inside a catalogue"):
        ens.recommend(*feed, catalogue=object())
    b._score_shard = {"rank": 0}
    for call in (lambda: ens.recommend(*feed), lambda: ens.ensemble_scores(*feed[:2]),
                 lambda: ens.score_candidates(feed[0], feed[1], [[1]] * 16)):
        with pytest.raises(ValueError, match="member 1 has a scoring shard"):
            call()
    assert not hasattr(ens, "evaluate_iter")         # the drivers' evaluation takes its recommend_iter branch for an ensemble
