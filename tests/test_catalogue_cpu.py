"""CPU: the host side of the catalogue calls (`model.catalogue(columns)`, csrc/catalogue.hip) -- the validation of the column list
and its messages -- and the REFERENCE the GPU file (tests/test_gpu_catalogue.py) compares against: "the k best tracks among the
catalogue's columns" expressed with what the oracle already has, a full-width ranking whose seed lists are the row's seeds united
with the complement of the catalogue.  That construction is checked here against numpy's own lexsort over the catalogue's columns
alone, so the reference of the GPU file is itself checked."""
import numpy as np
import pytest

import oracle
from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, DAE_tied, catalogue_columns

U32 = np.uint32


# ---- the reference of the GPU file --------------------------------------------------------------------------------------------------
def union_seeds(srp, sc, cols, n_tracks):
    """Per row: the row's seeds, then every track column that is NOT in the catalogue -> (row_ptr int32, col int32).  (The oracle
    marks seeds in a bitmap: order and repeats do not matter to it.)"""
    B = len(srp) - 1
    comp = np.setdiff1d(np.arange(n_tracks, dtype=np.int32), np.asarray(cols, np.int32))
    rows = [np.concatenate([np.asarray(sc[srp[r]:srp[r + 1]], np.int32), comp]) for r in range(B)]
    rp = np.zeros(B + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    assert rp[-1] < 2 ** 31
    return rp.astype(np.int32), (np.concatenate(rows) if rows else np.zeros(0, np.int32)).astype(np.int32)


def reference(z, k, srp, sc, cols, n_tracks, out_kind=0):
    """The expected lists of a catalogue call: oracle.topk over the FULL width z [B, >= n_tracks] with seeds u complement.
    -> (score [B, k], idx [B, k]) as oracle.topk returns them."""
    srp2, sc2 = union_seeds(srp, sc, cols, n_tracks)
    return oracle.topk(np.ascontiguousarray(z), k, srp2, sc2, ncols=n_tracks, out_kind=out_kind)


def _okey(z):
    u = np.asarray(z, np.float32).view(U32)
    u = np.where((u << U32(1)) == 0, U32(0), u)                # the canonical key: -0 == +0
    return np.where(u >> 31, ~u, u | U32(0x80000000)).astype(np.int64)


def lexsort_rank(z_row, cols, seeds, k):
    """numpy's own ranking of one row over `cols` alone: key descending, column ascending, seeds and -inf dropped."""
    cols = np.asarray(cols, np.int64)
    zc = z_row[cols]
    keep = ~np.isin(cols, np.asarray(seeds, np.int64)) & (_okey(zc) > 0x007FFFFF)
    c, z = cols[keep], zc[keep]
    order = np.lexsort((c, -_okey(z)))[:k]
    idx = np.full(k, -1, np.int32); lg = np.full(k, -np.inf, np.float32)
    idx[:order.size] = c[order]; lg[:order.size] = z[order]
    return idx, lg


def random_catalogue(n_tracks, n, seed):
    return np.sort(np.random.default_rng(seed).permutation(n_tracks)[:n]).astype(np.int32)


def test_reference_is_the_lexsort_ranking_over_the_catalogue():
    rng = np.random.default_rng(7)
    B, V, nt, k = 6, 1300, 1100, 200
    z = np.round(rng.standard_normal((B, V)) * 4).astype(np.float32) / 4            # few distinct values: ties everywhere
    z[0, 5] = -np.inf; z[1, :40] = -0.0; z[1, 40:80] = 0.0
    from spotify_recsys_challenge_2018_amd.models.DAEs import seeds_to_csr
    for n in (1, 150, 199, 200, 700, nt):
        cols = catalogue_columns(random_catalogue(nt, n, seed=n), nt)
        seeds = [rng.permutation(nt)[:c].tolist() for c in (0, 5, 300, 40, 1, 1000)]
        seeds[3] = cols.tolist() + [3, 4]                                             # covers the whole catalogue
        srp, sc = seeds_to_csr(seeds, B, nt)
        assert n == nt or np.isin(sc, cols, invert=True).any()
        ws, wi = reference(z, k, srp, sc, cols, nt, out_kind=1)
        for r in range(B):
            idx, lg = lexsort_rank(z[r], cols, seeds[r], k)
            assert np.array_equal(wi[r], idx), (n, r)
            assert np.array_equal(ws[r].view(U32), lg.view(U32)), (n, r)
        assert (wi[3] == -1).all()
        if n < k:
            assert (wi[:, n:] == -1).all()
        assert np.isin(wi[wi >= 0], cols).all()


# ---- model.catalogue(columns): the host check --------------------------------------------------------------------------------------
class _Conf:
    save = "/tmp/_catalogue_unused"; n_input = 1200; lr = 0.01; reg_lambda = 0.0; initval = "NULL"
    batch = 4; hidden = 64; n_tracks = 1000


@pytest.mark.parametrize("cls", [DAE, DAE_tied])
def test_catalogue_refuses_bad_column_lists_on_the_host(cls):
    m = cls(_Conf())                                           # not fitted: nothing below may need the device
    for bad, msg in [([], "empty"),
                     ([3, 2, 5], r"columns\[1\] = 2 is below columns\[0\] = 3"),
                     ([1, 4, 4, 9], r"columns\[2\] = 4 is listed twice"),
                     ([-1, 4], r"columns\[0\] = -1 is negative"),
                     ([5, 1000], r"columns\[1\] = 1000 is no track column \(tracks are \[0, 1000\)"),
                     (np.array([1, 1100]), r"columns\[1\] = 1100 is no track column"),
                     ([0.5, 2.0], "integer column ids"),
                     ([[1, 2], [3, 4]], "flat sequence")]:
        with pytest.raises(ValueError, match=msg):
            m.catalogue(bad)
    # a well-formed list passes the host check; without fit() there is no device to put it on, and that is said
    with pytest.raises(_lib.DaeError, match=r"fit\(\)"):
        m.catalogue(range(0, 1000, 3))


def test_catalogue_columns_accepts_any_integer_sequence():
    want = np.arange(0, 50, 7, dtype=np.int32)
    for cols in (range(0, 50, 7), list(range(0, 50, 7)), tuple(range(0, 50, 7)), np.arange(0, 50, 7, dtype=np.int64),
                 np.arange(0, 50, 7, dtype=np.uint16)):
        got = catalogue_columns(cols, 1000)
        assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(catalogue_columns(np.arange(1000), 1000), np.arange(1000))     # the whole track range
    assert np.array_equal(catalogue_columns([999], 1000), [999])


def test_a_sharded_model_refuses_catalogue_like_the_candidate_calls():
    m = DAE(_Conf())
    m.shard_scoring(0, 2)
    with pytest.raises(_lib.DaeError, match="not vocabulary-sharded: this model has a scoring shard"):
        m.catalogue([1, 2, 3])
