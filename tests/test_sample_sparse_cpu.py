"""CPU: the decoded-tile table of the half-row-group sample (csrc/score_plan.h dae_sample_item_slot).

1. tests/host/sample_sparse_main.cpp as a stand-alone C++ program -- no device, no HIP: the one mapping the sample launch writes
   the table by and the threshold launch reads it by, over the plans whose sample may skip.
2. The poison of tests/test_gpu_sample_sparse.py bites: with the skipped slots of a popularity-model call still holding the
   logits of a weights x 40 call (the sample no longer stores skipped tiles), EVERY row has a stale value above its threshold
   among its skipped dense slots and among its unstored maxima -- a threshold launch that read them would move the threshold or
   emit a survivor that is none.  Modelled in numpy from the oracle's fp32 logits as tests/test_sample_skip_cpu.py models the
   bound (item = wave * nb_rg + workgroup, group = (workgroup, position in the tile))."""
import functools
import os
import shutil
import subprocess

import numpy as np

import oracle
from test_gpu_sample_skip import K, NT, _feed, _hidden, _model
from test_sample_skip_cpu import _cut16, _down, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 256
N_SAMP = 469


def test_sample_sparse_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "sample_sparse")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "sample_sparse_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


@functools.lru_cache(maxsize=None)
def sample_model(B, bias, scale=1.0):
    """The half-row-group sample of a B-row call on the (bias, scale) model at hidden 256, from the oracle's logits:
    tau [B] the rows' thresholds, zt [row, item, position] the dense sample, gmax [row, workgroup, position] the maxima,
    skipped [half group, item] the tiles the bound puts below the half group's safe threshold, nb_rg."""
    _, _, W_dec, b_dec = _model(bias, H, scale)
    h = _hidden(B, bias, H, scale)
    z = oracle.decode(h, W_dec, b_dec, 0, NT)
    n_seeds = np.diff(_feed(B)[3])
    W, b = W_dec[:NT].astype(np.float64), b_dec[:NT].astype(np.float64)
    s, n = W.sum(1), np.abs(W).sum(1)
    rho = (H + 2) * 2.0 ** -24 * (1.0 + 2.0 ** -10)
    tiny = (H + 2) * 2.0 ** -125
    a_c = _up(b + 0.5 * s + rho * (0.5 * n + np.abs(b)) + tiny + 2.0 ** -40 * (n + np.abs(b)))
    m_c = _up((1.0 + rho) * n * (1.0 + 2.0 ** -40))
    lo_c = _down(b + 0.5 * s - rho * (0.5 * n + np.abs(b)) - tiny - 2.0 ** -40 * (n + np.abs(b)))
    nt32 = (NT + 31) // 32
    pad = nt32 * 32 - NT

    def tiles(v, fill):
        return np.concatenate([v, np.full(pad, fill, v.dtype)]).reshape(nt32, 32)

    order = np.lexsort((np.arange(nt32), -tiles(b.astype(np.float32), -np.inf).max(1).astype(np.float64)))
    n_samp = (nt32 + 1) // 2
    assert n_samp == N_SAMP
    nb_rg = 256 // ((B + 127) // 128)
    assert n_samp <= 4 * nb_rg
    items = order[:n_samp]
    A_t, M_t = tiles(a_c, -np.inf).max(1)[items], tiles(m_c, 0).max(1)[items]
    lo_t = tiles(lo_c, -np.inf)[items]
    zt = np.concatenate([z, np.full((B, pad), -np.inf, np.float32)], 1).reshape(B, nt32, 32)[:, items, :]
    beta = np.full((nb_rg, 32), -np.inf, np.float32)
    gmax = np.full((B, nb_rg, 32), -np.inf, np.float32)
    for w in range(4):
        it = np.arange(w * nb_rg, min((w + 1) * nb_rg, n_samp))
        if it.size:
            beta[:it.size] = np.maximum(beta[:it.size], lo_t[it])
            gmax[:, :it.size] = np.maximum(gmax[:, :it.size], zt[:, it])
    beta_sorted = np.sort(beta.ravel())[::-1][:4096]
    need = K + n_seeds
    tau = _cut16(np.sort(gmax.reshape(B, -1), 1)[:, ::-1][np.arange(B), need - 1])
    n_hg = (B + 63) // 64
    skipped = np.zeros((n_hg, n_samp), bool)
    for hg in range(n_hg):
        rows = np.arange(hg * 64, min(hg * 64 + 64, B))
        d = float(_up(np.abs(h[rows].astype(np.float64) - 0.5).max()))
        pm = d * float(M_t.max())
        bk = float(beta_sorted[int(need[rows].max()) - 1])
        x = bk - pm - (abs(bk) + abs(pm)) * 2.0 ** -48
        tau_safe = float(_cut16(_down(x))[0])
        dd = d * (1.0 + 2.0 ** -40)
        U = A_t.astype(np.float64) + dd * M_t.astype(np.float64)
        U += (np.abs(A_t) + np.abs(dd * M_t)) * 2.0 ** -48
        skipped[hg] = U < tau_safe
    return dict(tau=tau, zt=zt, gmax=gmax, skipped=skipped, nb_rg=nb_rg, items=items)


def poison_bites(B):
    """Per row: does a skipped dense slot / an unstored maximum of the popularity-model call hold a weights x 40 logit above the
    row's threshold?  Returns ([B] bool, [B] bool, wave-tiles the model decodes)."""
    new, old = sample_model(B, "zipf"), sample_model(B, "zipf", 40.0)
    assert np.array_equal(new["items"], old["items"]) and new["nb_rg"] == old["nb_rg"]      # (the same biases: the same tile order)
    nb_rg = new["nb_rg"]
    dense, maxima = np.zeros(B, bool), np.zeros(B, bool)
    for r in range(B):
        sk = new["skipped"][r // 64]
        dense[r] = (old["zt"][r][sk] > new["tau"][r]).any()
        # a workgroup stores its 32 maxima unless every one of its (up to four) items is skipped
        wg_dead = np.ones(nb_rg, bool)
        for item in np.flatnonzero(~sk):
            wg_dead[item % nb_rg] = False
        maxima[r] = (old["gmax"][r][wg_dead] > new["tau"][r]).any()
    return dense, maxima, int((~new["skipped"]).sum())


def test_stale_slots_would_be_seen():
    dense, maxima, decoded = poison_bites(256)
    print("popularity model after weights x 40, 256 rows: %d of %d wave-tiles decoded; rows with a stale dense value above tau: %d, "
          "with a stale maximum above tau: %d" % (decoded, 4 * N_SAMP, int(dense.sum()), int(maxima.sum())))
    assert 0 < decoded <= N_SAMP                                       # (at most a quarter: tests/test_gpu_sample_skip.py)
    assert dense.all() and maxima.all()
