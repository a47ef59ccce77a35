"""CPU: the threshold sample's skip ("the sample's own skip").

1. tests/host/sample_skip_main.cpp as a stand-alone C++ program -- no device, no HIP: the safe threshold's rule against
   dae_tau_search (csrc/tau_search.h) on random sets of maxima, and the plan's sample_skip field over a grid of shapes.
2. The bound itself, rebuilt in numpy from the formulas of csrc/prepack.hip and csrc/decode_generic.hip on the ORACLE's fp32
   logits at 30 000 + 6 000 columns, 130 rows (the grouping of the half-row-group launch: item = wave * 128 + workgroup,
   group = (workgroup, position in the tile)): tau_safe <= every row's real threshold, and no skipped tile holds an element
   that reaches its row's threshold."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr, seeds_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT, NA, H, K, B = 30000, 6000, 256, 500, 130
NB_RG, WAVES = 128, 4                      # two 128-row groups: 128 workgroups per half row group, four waves each


def test_sample_skip_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "sample_skip")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "spotify_recsys_challenge_2018_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "sample_skip_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def _okey(x):
    u = np.atleast_1d(np.asarray(x, np.float32)).view(np.uint32).copy()
    u[(u << np.uint32(1)) == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _cut16(x):
    """dae_tau_value(okey(x) >> 16, 1): the float of the key's 16 leading bits; -inf below the first finite prefix."""
    p = _okey(x) >> np.uint32(16)
    k = (p << np.uint32(16)).astype(np.uint32)
    u = np.where((k & np.uint32(0x80000000)) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(p >= 0x80, u.view(np.float32), np.float32(-np.inf)).astype(np.float32)


def _up(x):
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _down(x):
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(bias):
    W_enc, b_enc, W_dec, b_dec = make_weights(NT + NA, H, seed=0, bias=bias, n_tracks=NT)
    pos, ones, seeds = make_playlists(B, NT, NA, seed=1)
    rp, col, val = coo_to_csr(pos, ones, B, NT + NA)
    srp, _ = seeds_to_csr(seeds, B, NT)
    h = oracle.encode(rp, col, val, W_enc, b_enc)
    z = oracle.decode(h, W_dec, b_dec, 0, NT)                          # [B, NT] the canonical fp32 logits
    return W_dec[:NT].astype(np.float64), b_dec[:NT].astype(np.float64), h, z, np.diff(srp)


@pytest.mark.parametrize("bias", ["zipf", "zeros"])
def test_the_bound_on_the_oracles_logits(bias):
    W, b, h, z, n_seeds = _case(bias)
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

    # the tile order: largest bias among the ranked columns first, the lower tile on ties; the sample is every second tile's worth
    order = np.lexsort((np.arange(nt32), -tiles(b.astype(np.float32), -np.inf).max(1).astype(np.float64)))
    n_samp = (nt32 + 1) // 2
    assert n_samp == 469 and n_samp <= NB_RG * WAVES
    items = order[:n_samp]
    A_t, M_t = tiles(a_c, -np.inf).max(1)[items], tiles(m_c, 0).max(1)[items]
    mu_max = M_t.max()
    # groups (workgroup, position): the tiles of items w * 128 + workgroup
    lo_t = tiles(lo_c, -np.inf)[items]                                  # [item, position]
    zt = np.concatenate([z, np.full((B, pad), -np.inf, np.float32)], 1).reshape(B, nt32, 32)[:, items, :]      # [row, item, position]
    beta = np.full((NB_RG, 32), -np.inf, np.float32)
    gmax = np.full((B, NB_RG, 32), -np.inf, np.float32)
    for w in range(WAVES):
        it = np.arange(w * NB_RG, min((w + 1) * NB_RG, n_samp))
        beta[:it.size] = np.maximum(beta[:it.size], lo_t[it])
        gmax[:, :it.size] = np.maximum(gmax[:, :it.size], zt[:, it])
    beta_sorted = np.sort(beta.ravel())[::-1][:4096]
    gsorted = np.sort(gmax.reshape(B, -1), 1)[:, ::-1]
    need = K + n_seeds
    tau = _cut16(gsorted[np.arange(B), need - 1])                      # every row holds 4 096 finite maxima here
    assert np.isfinite(tau).all()
    for hg in range((B + 63) // 64):
        rows = np.arange(hg * 64, min(hg * 64 + 64, B))
        d = float(_up(np.abs(h[rows].astype(np.float64) - 0.5).max()))
        k_max = int(need[rows].max())
        pm = d * float(mu_max)
        x = float(beta_sorted[k_max - 1]) - pm
        x -= (abs(float(beta_sorted[k_max - 1])) + abs(pm)) * 2.0 ** -48
        tau_safe = float(_cut16(_down(x))[0])
        assert tau_safe <= tau[rows].min(), (bias, hg, tau_safe, tau[rows].min())
        dd = d * (1.0 + 2.0 ** -40)
        U = A_t.astype(np.float64) + dd * M_t.astype(np.float64)
        U += (np.abs(A_t) + np.abs(dd * M_t)) * 2.0 ** -48
        skipped = U < tau_safe
        reach = (zt[rows] >= tau[rows, None, None]).any(2).any(0)      # [item]: some row's element reaches its threshold
        assert not (skipped & reach).any(), (bias, hg, np.flatnonzero(skipped & reach)[:8])
        print("%s bias, half group %d (%d rows): d = %.4f, tau_safe = %.4f, min tau = %.4f, %d of %d tiles decoded, %d hold a survivor"
              % (bias, hg, rows.size, d, tau_safe, tau[rows].min(), int((~skipped).sum()), n_samp, int(reach.sum())))
        assert (~skipped).sum() >= reach.sum()
        if bias == "zipf":
            assert (~skipped).sum() <= n_samp // 4
        else:
            assert 0 < (~skipped).sum() < n_samp
