"""CPU: the threshold launch proves the filter launch's live list empty ("the empty list proved";
csrc/empty_proof.h).

1. tests/host/empty_proof_main.cpp as a stand-alone C++ program -- no device, no HIP: the index for D, the bound's monotonicity,
   the edges, and a fuzz of the implication.
2. The proof rebuilt in numpy from the formulas of csrc/prepack.hip (the tiles' {A_t, M_t}, the columns' lo_c, the tile order,
   the envelope G), csrc/decode_generic.hip (the half groups' D = dq and T = tau_safe) and csrc/decode_common.h (the tail's own
   test) on the ORACLE's hidden rows and fp32 logits at 30 000 + 6 000 columns, 130 rows: "proved" implies that the brute-force
   test on every item of the filter list, with the group's real d and real smallest threshold, keeps nothing.  The popularity
   model proves both groups, b_dec = 0 none; the same with hidden rows forced to {0, 1} (d = 0.5, the grid's last point).
3. A fuzz of random {A, M, d, tau} sets: negative A, M = 0, +-inf, NaN, d on grid points and one ulp to either side, T = -inf.
4. The headline's shape (170 000 columns, 140 000 tracks, 256 rows, three feeds): both groups prove; the margin G[j] - T is
   printed.  (No logits are needed for that: D, T and G come from the hidden rows and the image's bounds alone.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights
from test_sample_skip_cpu import B, H, K, NA, NT, _case, _cut16, _down, _up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 256                                       # d_j = j / 512, j = 0 .. 256


def test_empty_proof_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "empty_proof")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "empty_proof_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


# ---- the arithmetic of csrc/empty_proof.h, in numpy ---------------------------------------------------------------------------------
def proof_index(D):
    """The smallest j with j / 512 >= D; -1 for D > 0.5, D < 0 and a NaN."""
    D = np.float32(D)
    if not (D >= 0) or not (D <= 0.5):
        return -1
    j = int(np.float32(D * np.float32(512.0)))
    if np.float32(j) * np.float32(2.0 ** -9) < D:
        j += 1
    return j


def bound_U(A, M, d):
    """What dae_tile_is_live compares with tau_min (float pairs, d a double): the same operations in the same order."""
    with np.errstate(invalid="ignore", over="ignore"):
        A = np.asarray(A, np.float32).astype(np.float64)
        dd = np.float64(d) * (1.0 + 2.0 ** -40)
        dm = dd * np.asarray(M, np.float32).astype(np.float64)
        return A + dm + (np.abs(A) + np.abs(dm)) * 2.0 ** -48


def tail_keeps(A, M, d, tau_min):
    """The tail's own test per item: !(U < tau_min)."""
    with np.errstate(invalid="ignore"):
        return ~(bound_U(A, M, d) < np.float64(np.float32(tau_min)))


def envelope(A, M):
    """G[j], j = 0 .. 256: the NaN-keeping maximum over the items of U at d_j, rounded UP to float; all NaN if an item has a NaN
    pair or M < 0."""
    A, M = np.asarray(A, np.float32), np.asarray(M, np.float32)
    G = np.empty(GRID + 1, np.float32)
    bad = bool((~(M >= 0)).any() or np.isnan(A).any())
    for j in range(GRID + 1):
        U = bound_U(A, M, j / 512.0)
        G[j] = np.float32(np.nan) if bad or np.isnan(U).any() else _up(np.array([U.max()]))[0]
    return G


def proved(G, D, T):
    j = proof_index(D)
    with np.errstate(invalid="ignore"):
        return bool(j >= 0 and np.float64(G[j]) < np.float64(np.float32(T)))


# ---- the image's bounds and the launch geometry, as tests/test_sample_skip_cpu.py rebuilds them ----------------------------------
def image_tables(W, b, nt, hidden, k, nb_rg, waves=4):
    """W [nt, hidden], b [nt] in double (the ranked columns).  -> the filter list's {A_t, M_t}, the sample's mu_max and its group
    lower bounds sorted descending (the leading 4 096)."""
    s, n = W.sum(1), np.abs(W).sum(1)
    rho = (hidden + 2) * 2.0 ** -24 * (1.0 + 2.0 ** -10)
    tiny = (hidden + 2) * 2.0 ** -125
    a_c = _up(b + 0.5 * s + rho * (0.5 * n + np.abs(b)) + tiny + 2.0 ** -40 * (n + np.abs(b)))
    m_c = _up((1.0 + rho) * n * (1.0 + 2.0 ** -40))
    lo_c = _down(b + 0.5 * s - rho * (0.5 * n + np.abs(b)) - tiny - 2.0 ** -40 * (n + np.abs(b)))
    nt32 = (nt + 31) // 32
    pad = nt32 * 32 - nt

    def tiles(v, fill):
        return np.concatenate([v, np.full(pad, fill, v.dtype)]).reshape(nt32, 32)

    order = np.lexsort((np.arange(nt32), -tiles(b.astype(np.float32), -np.inf).max(1).astype(np.float64)))
    # score_plan.h dae_plan_topk: the sample stride for a launch of nb_rg workgroups per row group
    n_simd = nb_rg * 4
    rounds = max(int(nt32 / 8.0 / n_simd + 0.5), 1)
    S = (nt32 + rounds * n_simd - 1) // (rounds * n_simd)
    assert S >= 2
    n_samp = (nt32 + S - 1) // S
    assert n_samp <= nb_rg * waves
    A_all, M_all = tiles(a_c, -np.inf).max(1), tiles(m_c, 0).max(1)      # (the edge tile over its ranked columns only)
    samp, filt = order[:n_samp], order[n_samp:]
    lo_t = tiles(lo_c, -np.inf)[samp]
    beta = np.full((nb_rg, 32), -np.inf, np.float32)
    for w in range(waves):
        it = np.arange(w * nb_rg, min((w + 1) * nb_rg, n_samp))
        beta[:it.size] = np.maximum(beta[:it.size], lo_t[it])
    return {"A": A_all[filt], "M": M_all[filt], "mu_max": M_all[samp].max(), "beta": np.sort(beta.ravel())[::-1][:4096],
            "n_samp": n_samp, "samp": samp, "n_filter": filt.size}


def half_group_pairs(tab, h, n_seeds, k):
    """{dq, tau_safe} of every half group of 64 rows with a real row (decode_generic.hip, HALF)."""
    pairs = []
    for hg in range((h.shape[0] + 63) // 64):
        rows = slice(hg * 64, min(hg * 64 + 64, h.shape[0]))
        with np.errstate(invalid="ignore"):
            dmax = np.abs(h[rows].astype(np.float64) - 0.5).max()
        dq = np.float32(np.nan) if np.isnan(dmax) else _up(np.array([dmax]))[0]
        idx = k - 1 + int(n_seeds[rows].max())
        beta_k = float(tab["beta"][idx]) if idx < tab["beta"].size else -np.inf
        pm = float(dq) * float(tab["mu_max"])
        x = beta_k - pm
        x -= (abs(beta_k) + abs(pm)) * 2.0 ** -48
        tau_safe = np.float32(np.nan) if np.isnan(x) else _cut16(_down(np.array([x])))[0]
        pairs.append((dq, tau_safe))
    return pairs


def group_DT(pairs, rg):
    p = pairs[2 * rg:2 * rg + 2]
    with np.errstate(invalid="ignore"):
        D = np.float32(np.nan) if any(np.isnan(q[0]) for q in p) else max(q[0] for q in p)
        T = np.float32(np.nan) if any(np.isnan(q[1]) for q in p) else min(q[1] for q in p)
    return D, T


def real_thresholds(z, samp, n_seeds, k, nb_rg, waves=4):
    """The thresholds tau_select_kernel returns: the (k + seeds)-th largest group maximum of the row, cut to 16 key bits."""
    nrows, nt = z.shape
    nt32 = (nt + 31) // 32
    zt = np.concatenate([z, np.full((nrows, nt32 * 32 - nt), -np.inf, np.float32)], 1).reshape(nrows, nt32, 32)[:, samp, :]
    gmax = np.full((nrows, nb_rg, 32), -np.inf, np.float32)
    for w in range(waves):
        it = np.arange(w * nb_rg, min((w + 1) * nb_rg, samp.size))
        gmax[:, :it.size] = np.maximum(gmax[:, :it.size], zt[:, it])
    gsorted = np.sort(gmax.reshape(nrows, -1), 1)[:, ::-1]
    return _cut16(gsorted[np.arange(nrows), k + n_seeds - 1])


@pytest.mark.parametrize("rows01", [False, True], ids=["encoded", "rows01"])
@pytest.mark.parametrize("bias", ["zipf", "zeros"])
def test_proved_implies_the_tail_keeps_nothing(bias, rows01):
    W, b, h, z, n_seeds = _case(bias)
    if rows01:                                                         # d = 0.5 exactly: the grid's last point
        h = (np.random.default_rng(3).random((256, H)) < 0.5).astype(np.float32)[:B]
        z = oracle.decode(h, W.astype(np.float32), b.astype(np.float32), 0, NT)
    tab = image_tables(W, b, NT, H, K, 128)
    assert tab["n_samp"] == 469 and tab["n_filter"] == 469
    G = envelope(tab["A"], tab["M"])
    assert not np.isnan(G).any() and (np.diff(G.astype(np.float64)) >= 0).all()
    pairs = half_group_pairs(tab, h, n_seeds, K)
    tau = real_thresholds(z, tab["samp"], n_seeds, K, 128)
    for rg in range((B + 127) // 128):
        rows = slice(rg * 128, min(rg * 128 + 128, B))
        D, T = group_DT(pairs, rg)
        d = np.abs(h[rows].astype(np.float64) - 0.5).max()
        tau_min = tau[rows].min()
        assert float(D) >= d and float(T) <= float(tau_min), (D, d, T, tau_min)
        keeps = tail_keeps(tab["A"], tab["M"], d, tau_min)
        ok = proved(G, D, T)
        j = proof_index(D)
        print("%s bias%s, group %d: D = %.6f (j = %d), T = %.4f, tau_min = %.4f, G[j] = %.4f, margin G[j] - T = %.4f, proved %s, the tail keeps %d of %d"
              % (bias, ", rows in {0, 1}" if rows01 else "", rg, D, j, T, tau_min, G[j], float(G[j]) - float(T), ok, int(keeps.sum()), keeps.size))
        if rows01:
            assert D == np.float32(0.5) and j == GRID
        if ok:
            assert not keeps.any()
        assert ok == (bias == "zipf"), (bias, rg, ok)
        if bias == "zeros":
            assert keeps.any()


def test_fuzz_proved_implies_the_tail_keeps_nothing():
    rng = np.random.default_rng(11)
    inf = np.float32(np.inf)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    n_proved = 0
    n_sets = 3000
    for rep in range(n_sets):
        cnt = int(rng.integers(1, 40))
        kind = rep % 8
        A = (-12.0 + 6.0 * rng.random(cnt)).astype(np.float32)
        M = (2.0 * rng.random(cnt)).astype(np.float32)
        if kind == 4:
            A += np.float32(7.0)                                       # around zero, both signs
        if kind == 5:
            M[rng.random(cnt) < 0.3] = 0.0
        if kind == 6:
            sel = rng.random(cnt) < 0.06
            A[sel] = rng.choice(specials, int(sel.sum()))
        if kind == 7:
            sel = rng.random(cnt) < 0.06
            M[sel] = rng.choice(np.concatenate([specials, np.array([-0.25], np.float32)]), int(sel.sum()))
        gp = np.float32(int(rng.integers(0, GRID + 1))) * np.float32(2.0 ** -9)
        dk = int(rng.integers(0, 6))
        d = float(gp) if dk == 0 else max(float(np.nextafter(gp, -inf)), 0.0) if dk == 1 else float(np.nextafter(gp, inf)) if dk == 2 else 0.5 * rng.random()
        if rep % 97 == 0:
            d = 0.5 + rng.random()
        if rep % 101 == 0:
            d = float("nan")
        D = np.float32(np.nan) if np.isnan(d) else _up(np.array([d]))[0]
        if rng.random() < 0.25 and not np.isnan(D):
            D = np.float32(D + np.float32(0.01 * rng.random()))
        tau_min = np.float32(-10.0 + 10.0 * rng.random())
        if rep % 53 == 0:
            tau_min = -inf
        if rep % 59 == 0:
            tau_min = np.float32(np.nan)
        T = tau_min
        if rng.random() < 0.5 and not np.isnan(T):
            T = np.float32(T - np.float32(rng.random()))
        if rep % 61 == 0:
            T = -inf
        assert np.isnan(D) or float(D) >= d or np.isnan(d)
        # the envelope entry for D only (the whole grid of a set costs 257 passes)
        j = proof_index(D)
        ok = False
        if j >= 0:
            bad = bool((~(M >= 0)).any() or np.isnan(A).any())
            U = bound_U(A, M, j / 512.0)
            Gj = np.float32(np.nan) if bad or np.isnan(U).any() else _up(np.array([U.max()]))[0]
            with np.errstate(invalid="ignore"):
                ok = bool(np.float64(Gj) < np.float64(T))
        if ok:
            n_proved += 1
            assert not np.isneginf(T) and not np.isnan(D)
            assert not tail_keeps(A, M, d, tau_min).any(), (rep, A, M, d, D, tau_min, T)
    print("fuzz: %d of %d sets proved" % (n_proved, n_sets))
    assert n_proved > n_sets // 10


def test_the_headline_shape_proves_both_groups():
    """bench.py's flagship: 140 000 tracks + 30 000 artists at hidden 256, 256 rows, k = 500 (two row groups, 128 workgroups per
    half row group, sample stride 9: 487 sample tiles, 3 888 filter tiles)."""
    V, nt, rows = 170000, 140000, 256
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, bias="zipf", n_tracks=nt)
    tab = image_tables(W_dec[:nt].astype(np.float64), b_dec[:nt].astype(np.float64), nt, H, K, 128)
    assert tab["n_samp"] == 487 and tab["n_filter"] == 3888
    G = envelope(tab["A"], tab["M"])
    assert not np.isnan(G).any()
    for seed in (1, 2, 3):
        pos, ones, seeds = make_playlists(rows, nt, V - nt, seed=seed)
        rp, col, val = coo_to_csr(pos, ones, rows, V)
        srp, _ = seeds_to_csr(seeds, rows, nt)
        h = oracle.encode(rp, col, val, W_enc, b_enc)
        pairs = half_group_pairs(tab, h, np.diff(srp), K)
        for rg in range(2):
            D, T = group_DT(pairs, rg)
            j = proof_index(D)
            print("headline shape, feed %d, group %d: D = %.6f (j = %d), T = tau_safe = %.4f, G[j] = %.4f, margin G[j] - T = %.4f"
                  % (seed, rg, D, j, T, G[j], float(G[j]) - float(T)))
            assert proved(G, D, T), (seed, rg, D, T, G[j])
