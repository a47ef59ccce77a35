"""GPU (-m gpu): the exact title mix (dae_mix_topk_exact, csrc/mixexact.hip and mix_*.hip) at DAE hidden sizes and title feature row
lengths other than the shipped 256 / 448 -- `[DAE] hidden`, `[TITLE] filter_num` and `filter_size` are free keys of the
reference's schema (main.py:46, :73-75).  The supported set is dae_mix_exact_shape_ok's: hidden 128 .. 512, rows of 64 .. 512,
both in steps of 64; those shapes run the two-GEMM bf16 launches (mix_bf16_steps_kernel: the step counts at run time, row
groups of 96 playlists up to hidden + row length 832, of 64 beyond) and return the fp32 title path's lists, indices AND
score bits, through `recommend`, `recommend_iter` and the C entry point.  Every other shape stays on the fp32 kernels and
says so once.

The vocabulary is the small one of tests/test_gpu_title_exact.py (2 000 tracks: 63 ranked tiles, the last one partial); with
that file's four filter sizes, filter_num 16 / 32 / 100 / 128 gives rows of 64 / 128 / 448 / 512.  At that size every wave of
a launch decodes one tile at most, so one case per row-group height runs 750 rows over a vocabulary with several tiles per
wave.  The row-group height is read from the library (dae_last_plan), not restated here."""
import pathlib
import tempfile
import warnings

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE_title, SEEDS_FROM_INPUT
from test_gpu_title_exact import _conf, _feed, _model, _same, _titles

pytestmark = pytest.mark.gpu
FALLBACK_LINE = "titled launches run on the fp32 kernels"

# (hidden, filter_num, feature row length, playlists per row group)
SHAPES = [
    (128, 16, 64, 96),        # the smallest of both: 12 steps, a title image of 4 (half a chunk)
    (192, 100, 448, 96),      # hidden not a multiple of 128: the DAE image ends on half a chunk
    (256, 25, 128, 96),       # the shipped hidden with another width; 100 features, 28 zero columns
    (384, 100, 448, 96),      # the largest shape on 96-row groups (52 steps: 156 KiB of hidden rows)
    (448, 100, 448, 64),      # the first shape on 64-row groups
    (512, 128, 512, 64),      # the largest supported shape
]


def _shape_model(tmp_path, hidden, filter_num, batch, n_tracks=2000, n_input=2300, **kw):
    conf = _conf(n_tracks=n_tracks, n_input=n_input, batch=batch)
    conf.hidden = hidden
    d = tmp_path / ("h%d_f%d_b%d" % (hidden, filter_num, batch))
    d.mkdir()
    return conf, _model(d, conf, filter_num=filter_num, **kw)


def _case(conf, trial, dead_row=5):
    """A feed of conf.batch rows: every third row without a title, two title-only playlists, and one row with neither input
    nor title (both mixing weights 0)."""
    B = conf.batch
    only = (2, min(11, B - 1))
    pos, ones, seeds = _feed(conf, 5 + trial, empty_rows=only + (dead_row,))
    titles = _titles(B, seed=6 + trial)
    use = (np.arange(B) % 3 != trial % 3).astype(np.float32)
    use[list(only)] = 1.0
    use[dead_row] = 0.0
    return pos, ones, seeds, titles, use


@pytest.mark.parametrize("hidden,filter_num,ld,rows_per_group", SHAPES)
def test_exact_title_mix_shapes_return_the_fp32_lists(tmp_path, capfd, hidden, filter_num, ld, rows_per_group):
    capfd.readouterr()
    for batch in (24, 200):                               # one partial row group; several, the last one partial
        conf, m = _shape_model(tmp_path, hidden, filter_num, batch)
        tm = m.title_model
        assert tm.ld == ld and m.n_hidden == hidden
        for trial, k in enumerate((37, 100, 500)):
            pos, ones, seeds, titles, use = _case(conf, trial)
            want = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="f32")
            with warnings.catch_warnings():
                warnings.simplefilter("error")            # a guard fallback would hide a broken bound
                got = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="exact_bf16")
            _same(got, want)
            assert tm.ctx.exact_stats_read()["rows"] == batch         # the two-GEMM launches ran
            assert tm.ctx.exact_guard_read()[0] == 0
            plan = tm.ctx.last_plan()                                 # the geometry the library chose for the launch
            assert plan["R_TILE"] == rows_per_group and plan["n_rg"] == -(-batch // rows_per_group), plan
        assert not getattr(m, "_guard_fallbacks", 0)
    assert FALLBACK_LINE not in capfd.readouterr().err


@pytest.mark.parametrize("hidden,filter_num", [(256, 100), (128, 16)])
def test_exact_title_mix_unfused_selection_above_k_512(tmp_path, hidden, filter_num):
    """k above 512: the refine launch cannot order the row itself (mix_plan.h `fuse`), so it leaves its compact lists and the
    selection kernel behind it ends the call.  The shipped shape and hidden 128 / rows of 64, one partial row group."""
    conf, m = _shape_model(tmp_path, hidden, filter_num, 24)
    tm = m.title_model
    for trial, k in enumerate((513, 777)):
        pos, ones, seeds, titles, use = _case(conf, trial)
        want = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="f32")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="exact_bf16")
        _same(got, want)
        assert tm.ctx.exact_stats_read()["rows"] == 24                # the two-GEMM launches ran
        assert tm.ctx.exact_guard_read()[0] == 0
    assert not getattr(m, "_guard_fallbacks", 0)


# (hidden, filter_num, feature row length, playlists per row group, tracks, columns)
MANY_TILES = [
    (128, 16, 64, 96, 140000, 170000),        # the full vocabulary at the smallest shape: 4 375 tiles on 32 x 8 waves per row group
    (512, 128, 512, 64, 40000, 45000),        # row groups of 64 at the largest: 1 250 tiles on 16 x 8 waves per row group
]


@pytest.mark.parametrize("hidden,filter_num,ld,rows_per_group,n_tracks,n_input", MANY_TILES)
def test_exact_title_mix_shapes_many_tiles_per_wave(tmp_path, capfd, hidden, filter_num, ld, rows_per_group, n_tracks, n_input):
    """The steady state of the kernel's tile loop, on each row-group height: a launch of 750 rows (the drivers' loop's 5 feeds
    of 150) over a vocabulary with several tiles for EVERY wave of the sample and of the filter launch -- the W ring running
    from a tile's last title chunk into the next tile's first DAE chunk, the bias fragments fetched a tile ahead, tiles
    claimed from the counter in LDS, several tiles of a workgroup appending to one row's candidate segment.  Lists and score
    bits of the fp32 path, through `recommend` and through the streamed loop (whose sample launch runs on the narrow grid
    of the overlap hint: about 8 tiles per wave)."""
    conf, m = _shape_model(tmp_path, hidden, filter_num, 750, n_tracks=n_tracks, n_input=n_input)
    tm = m.title_model
    assert tm.ld == ld
    capfd.readouterr()
    pos, ones, seeds = _feed(conf, 5, empty_rows=(3, 400))
    titles = _titles(conf.batch, seed=6)
    use = (np.arange(conf.batch) % 7 != 2).astype(np.float32)
    use[3] = use[400] = 1.0
    want = m.recommend(pos, ones, seeds, k=500, titles=titles, titles_use=use, dtype="f32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = m.recommend(pos, ones, seeds, k=500, titles=titles, titles_use=use, dtype="exact_bf16")
    _same(got, want)
    plan = tm.ctx.last_plan()
    waves = 8 * plan["nb_rg"]                                         # wave slots that share a row group's tiles
    assert plan["R_TILE"] == rows_per_group and plan["n_rg"] == -(-750 // rows_per_group), plan
    assert plan["n_filter_tiles"] == -(-n_tracks // 32) and plan["n_filter_tiles"] >= 4 * waves, plan
    assert plan["n_sample_tiles"] >= 2 * waves, plan
    st = tm.ctx.exact_stats_read()
    assert st["rows"] == 750 and st["candidates_per_row"] >= 500, st
    assert tm.ctx.exact_guard_read()[0] == 0 and not getattr(m, "_guard_fallbacks", 0)
    # the same rows through the library's titled pipeline: 5 feeds of 150 -> one launch, seeds = the playlists' own tracks
    conf2 = _conf(n_tracks=n_tracks, n_input=n_input, batch=150)
    conf2.hidden = hidden
    conf2.filter_num = filter_num
    conf2.DAEval = conf.DAEval
    m2 = DAE_title(conf2, tm)
    m2.fit()
    feeds = []
    for i in range(5):
        sel = (pos[:, 0] >= 150 * i) & (pos[:, 0] < 150 * (i + 1))
        p_i = pos[sel].copy(); p_i[:, 0] -= 150 * i
        o_i = ones[sel] if np.ndim(ones) and len(ones) == len(sel) else ones
        feeds.append((p_i, o_i, SEEDS_FROM_INPUT, 150, titles[150 * i:150 * (i + 1)], use[150 * i:150 * (i + 1)]))
    own = [sorted(set(int(c) for c in pos[pos[:, 0] == r, 1] if c < n_tracks)) for r in range(750)]
    want_own = m.recommend(pos, ones, own, k=500, titles=titles, titles_use=use, dtype="f32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got_it = list(m2.recommend_iter(feeds, k=500, dtype="exact_bf16"))
    assert np.array_equal(np.concatenate([g[0] for g in got_it]), want_own[0])
    assert np.array_equal(np.concatenate([g[1] for g in got_it]).view(np.uint32), want_own[1].view(np.uint32))
    (_gen, pipe), = m2._pipes.values()
    stp = pipe.stats()
    assert stp["feeds"] == 5 and 0 < stp["launches"] < 5 and stp["guard_fallbacks"] == 0, stp
    assert FALLBACK_LINE not in capfd.readouterr().err


def _c_call(m, conf, case, k):
    """dae_mix_topk_exact as DAE_title._submit calls it, without that method's choice of arithmetic -> (idx, score)."""
    import torch
    pos, ones, seeds, titles, use = case
    tm = m.title_model
    m._ensure_packed(_lib.DAE_DTYPE_BF16_EXACT)
    tm._ensure_packed(_lib.DAE_DTYPE_BF16_EXACT)
    m.ctx.bind_stream()
    tm.ctx.bind_stream()
    nb = conf.batch
    dev = m.weights["encoder_h"].device
    csr = m._upload_csr(pos, ones, n_rows=nb)
    h = torch.empty((nb, m.n_hidden), dtype=torch.float32, device=dev)
    m.ctx.encode(csr[0], csr[1], csr[2], m.weights["encoder_h"], m.biases["encoder_b"], h)
    w_t, w_p = m._mix_weights(csr, use, n_rows=nb)
    feat = tm.features(titles, nb)
    d_srp, d_sc = m._seed_csr_dev(seeds, csr, n_rows=nb)
    score = torch.empty((nb, k), dtype=torch.float32, device=dev)
    idx = torch.empty((nb, k), dtype=torch.int32, device=dev)
    tm.ctx.mix_topk_exact(m.ctx, feat, h, w_t, w_p, m.n_tracks, d_srp, d_sc, k, score, idx)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), score.cpu().numpy()


def test_exact_title_mix_c_entry_point_and_predicate(tmp_path):
    """The C entry point at hidden 128 / rows of 64 returns the fp32 path's lists; the predicate holds at the corners of the
    grid and just outside them."""
    conf, m = _shape_model(tmp_path, 128, 16, 24)
    case = _case(conf, 0)
    pos, ones, seeds, titles, use = case
    want = m.recommend(pos, ones, seeds, k=100, titles=titles, titles_use=use, dtype="f32")
    got = _c_call(m, conf, case, 100)
    assert np.array_equal(got[0], np.asarray(want[0]))
    assert np.array_equal(got[1].view(np.uint32), np.asarray(want[1]).view(np.uint32))
    assert m.title_model.ctx.exact_guard_read()[0] == 0
    for hidden in (128, 512):
        for ld in (64, 512):
            assert _lib.mix_exact_shape_ok(hidden, ld)
    assert _lib.mix_exact_shape_ok(256, 448) and _lib.mix_exact_shape_ok(320, 192)
    for hidden, ld in ((64, 448), (96, 448), (160, 448), (576, 448), (256, 0), (256, 32), (256, 96), (256, 576), (0, 0), (-64, 64)):
        assert not _lib.mix_exact_shape_ok(hidden, ld), (hidden, ld)


def test_exact_title_mix_other_shape_streamed(tmp_path, capfd):
    """The drivers' loop at hidden 128 / rows of 128: three feeds (a short one among them) with the playlists' own tracks as
    seeds through the library's titled pipeline (dae_title_score) -- the fp32 lists of the same rows."""
    conf, m = _shape_model(tmp_path, 128, 32, 24)
    assert m.title_model.ld == 128
    capfd.readouterr()
    B = conf.batch
    feeds, want = [], []
    for i in range(3):
        pos, ones, _s, titles, use = _case(conf, i)
        n = [B, 7, B][i]
        own = [sorted(set(int(c) for c in np.asarray(pos)[np.asarray(pos)[:, 0] == r, 1] if c < conf.n_tracks)) for r in range(B)]
        feeds.append((pos, ones, SEEDS_FROM_INPUT, n, [list(t) for t in titles], use))
        want.append(m.recommend(pos, ones, own, k=100, n_rows=n, titles=titles, titles_use=use, dtype="f32"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = list(m.recommend_iter(feeds, k=100, dtype="exact_bf16"))
    assert len(got) == 3
    for g, w in zip(got, want):
        _same(g, w)
    (_gen, pipe), = m._pipes.values()
    st = pipe.stats()
    assert st["feeds"] == 3 and st["guard_fallbacks"] == 0, st
    assert not getattr(m, "_guard_fallbacks", 0)
    assert FALLBACK_LINE not in capfd.readouterr().err


def test_title_mix_audit_is_silent_at_a_64_row_group_shape(tmp_path):
    """Hidden 448 / rows of 448 (row groups of 64), every launch audited on 8 random ranked tiles: nothing above a row's k-th
    score is missing from its list, and the counters say what was checked."""
    conf, m = _shape_model(tmp_path, 448, 100, 24)
    tc = m.title_model.ctx
    tc.set_exact_audit(1, 8)
    before = tc.exact_audit_read()
    for trial, k in enumerate((100, 37)):
        pos, ones, seeds, titles, use = _case(conf, trial)
        want = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="f32")
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="exact_bf16")
        _same(got, want)
        assert tc.exact_stats_read()["rows"] == conf.batch
    after = tc.exact_audit_read()
    assert after["audits"] - before["audits"] == 2
    assert after["checked"] - before["checked"] > 0 and after["violations"] == 0 and tc.exact_guard_read()[0] == 0


@pytest.mark.parametrize("hidden,filter_num,ld", [(96, 100, 448), (256, 144, 576)])
def test_exact_title_mix_shapes_still_outside(tmp_path, capfd, hidden, filter_num, ld):
    """Hidden 96 (a multiple of 32, not of 64) and rows of 576 (above 512): the fp32 lists from the fp32 kernels, one line on
    stderr, a refusal from the C entry point and from the predicate."""
    assert not _lib.mix_exact_shape_ok(hidden, ld)
    conf, m = _shape_model(tmp_path, hidden, filter_num, 24)
    assert m.title_model.ld == ld
    case = _case(conf, 0)
    pos, ones, seeds, titles, use = case
    capfd.readouterr()
    got = m.recommend(pos, ones, seeds, k=50, titles=titles, titles_use=use, dtype="exact_bf16")
    got2 = m.recommend(pos, ones, seeds, k=50, titles=titles, titles_use=use, dtype="exact_bf16")
    err = capfd.readouterr().err
    assert err.count(FALLBACK_LINE) == 1 and "hidden = %d" % hidden in err
    want = m.recommend(pos, ones, seeds, k=50, titles=titles, titles_use=use, dtype="f32")
    _same(got, want)
    _same(got2, want)
    assert m.title_model.ctx.exact_stats_read()["rows"] == 0          # no two-GEMM launch ran
    with pytest.raises(_lib.DaeError, match=r"hidden 128\.\.512"):
        _c_call(m, conf, case, 10)


@pytest.mark.parametrize("seed", [0, 1])
def test_exact_title_mix_shapes_fuzz(seed):
    """Random shapes of the supported grid, batches, vocabularies, models (bias, weight / feature / output scales), title
    usage and k, drawn as scripts/fuzz_title_exact.py draws them: the exact lists against the fp32 title path, bit for bit."""
    rng = np.random.default_rng(1000 + seed)
    tmp = pathlib.Path(tempfile.mkdtemp())
    lines, bad, ran = [], 0, 0
    for case in range(6):
        hidden = int(rng.choice(np.arange(128, 513, 64)))
        filter_num = int(rng.choice([16, 32, 48, 64, 80, 96, 112, 128]))          # x 4 filter sizes: rows of 64 .. 512
        nt = int(rng.choice([1500, 4000, 20000]))
        batch = int(rng.choice([7, 24, 96, 150, 200]))
        bias = str(rng.choice(["zipf", "zeros"]))
        w_scale = float(rng.choice([1.0, 1.0, 8.0, 40.0]))
        feat_scale = float(rng.choice([1.0, 1.0, 6.0, 25.0]))
        out_scale = float(rng.choice([1.0, 1.0, 10.0, 60.0]))
        (tmp / ("c%d" % case)).mkdir()
        conf, m = _shape_model(tmp / ("c%d" % case), hidden, filter_num, batch,
                               n_tracks=nt, n_input=nt + int(rng.integers(100, 3000)), bias=bias, w_scale=w_scale,
                               title_seed=int(rng.integers(1, 1000)), feat_scale=feat_scale, out_scale=out_scale)
        assert _lib.mix_exact_shape_ok(hidden, m.title_model.ld)
        k = int(rng.choice([1, 10, 100, 500, 777]))
        pos, ones, seeds = _feed(conf, int(rng.integers(0, 10000)), empty_rows=tuple(int(x) for x in rng.integers(0, batch, 2)))
        titles = _titles(batch, seed=int(rng.integers(0, 10000)))
        use = (rng.random(batch) < rng.choice([0.3, 0.8, 1.0])).astype(np.float32)
        if not use.any():
            use[0] = 1.0
        want = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="f32")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = m.recommend(pos, ones, seeds, k=k, titles=titles, titles_use=use, dtype="exact_bf16")
        same = np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        st = m.title_model.ctx.exact_stats_read()
        lines.append("case %d hidden %d rows %d tracks %d batch %d %s x%g feat x%g out x%g k %d: %s  rows %d cand %.0f fallbacks %d + %d rows%s"
                     % (case, hidden, m.title_model.ld, nt, batch, bias, w_scale, feat_scale, out_scale, k,
                        "same" if same else "DIFFERENT", st["rows"], st["candidates_per_row"],
                        getattr(m, "_guard_fallbacks", 0), getattr(m, "_guard_row_fallbacks", 0),
                        ("  (%s)" % str(w[0].message)[:100]) if w else ""))
        bad += 0 if same else 1
        # the case counts only if the two-GEMM launch produced the lists: it ran, and the launch was not re-scored with the fp32
        # kernels (single rows that overflow the refine launch's list under a flat bias may be: they are counted in the line)
        ran += 1 if st["rows"] == batch and not getattr(m, "_guard_fallbacks", 0) else 0
        del m
    assert bad == 0 and ran == 6, "\n".join(lines)
