"""CPU: the candidate-scoring entry points (include/dae_hip.h, csrc/candidates.hip) are declared in the header and bound in
_lib.py with matching argument counts; `candidates_to_csr`, the pure-numpy conversion of candidate lists to the CSR the
kernels take; the refusals that happen before any launch.  No device is needed."""
import os
import re

import numpy as np
import pytest

from spotify_recsys_challenge_2018_amd import _lib
from spotify_recsys_challenge_2018_amd.models.DAEs import DAE, candidates_to_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["dae_decode_candidates", "dae_score_candidates", "dae_mix_candidates", "dae_rank_candidates"]


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(dae_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text):
        out[name] = len([a for a in args.split(",") if a.strip()])
    return out


def test_entry_points_declared_and_bound_with_matching_argument_counts():
    counts = _header_arg_counts()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in counts, name
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)
        assert len(fn.argtypes) == counts[name], (name, len(fn.argtypes), counts[name])
    assert counts["dae_decode_candidates"] == 14 and counts["dae_mix_candidates"] == 20
    head = open(os.path.join(ROOT, "include", "dae_hip.h")).read()
    assert int(re.search(r"#define\s+DAE_CAND_CHUNK\s+(\d+)", head).group(1)) == _lib.DAE_CAND_CHUNK


def test_ragged_lists_with_empty_rows():
    cands = [[], [], [5, 3, 9, 3], [], [0], [7, 7], [], []]              # empty rows at the start, in the middle, at the end
    rp, col = candidates_to_csr(cands, 8, 10)
    assert rp.dtype == np.int32 and col.dtype == np.int32
    assert rp.tolist() == [0, 0, 0, 4, 4, 5, 7, 7, 7]
    assert col.tolist() == [5, 3, 9, 3, 0, 7, 7]                         # the caller's order, repeats kept
    for r, c in enumerate(cands):
        assert col[rp[r]:rp[r + 1]].tolist() == list(c)


def test_fewer_lists_than_rows_and_no_lists():
    rp, col = candidates_to_csr([[1, 2]], 3, 5)
    assert rp.tolist() == [0, 2, 2, 2] and col.tolist() == [1, 2]
    rp, col = candidates_to_csr([], 2, 5)
    assert rp.tolist() == [0, 0, 0] and col.size == 0
    rp, col = candidates_to_csr([np.array([4, 0], np.int64), (3,), range(2)], 3, 5)     # any sequence type per row
    assert rp.tolist() == [0, 2, 3, 5] and col.tolist() == [4, 0, 3, 0, 1]
    with pytest.raises(ValueError):
        candidates_to_csr([[1], [2], [3]], 2, 5)


def test_two_dimensional_form_keeps_padding_in_place():
    a = np.array([[3, 1, -1, -1], [-1, -1, -1, -1], [9, 9, 2, 0]], np.int32)
    rp, col = candidates_to_csr(a, 3, 10)
    assert rp.tolist() == [0, 4, 8, 12]
    assert col.tolist() == a.reshape(-1).tolist()
    rp, col = candidates_to_csr(a[:2].astype(np.int64), 4, 10)            # fewer rows than the feed: the rest are empty
    assert rp.tolist() == [0, 4, 8, 8, 8]
    with pytest.raises(ValueError):
        candidates_to_csr(a.astype(np.float32), 3, 10)


def test_duplicate_removal():
    cands = [[5, 3, 5, -1, 3, 9], [], [2, 2, 2], [-1, -1]]
    rp, col = candidates_to_csr(cands, 5, 10, unique=True)
    assert rp.tolist() == [0, 3, 3, 4, 4, 4]
    assert col.tolist() == [3, 5, 9, 2]                                   # once each, ascending, padding dropped
    a = np.array([[1, 1, -1], [0, 2, 0]], np.int64)
    rp, col = candidates_to_csr(a, 2, 3, unique=True)
    assert rp.tolist() == [0, 1, 3] and col.tolist() == [1, 0, 2]


@pytest.mark.parametrize("bad", [10, -2, 2 ** 31, -2 ** 40])
def test_out_of_range_ids_raise(bad):
    with pytest.raises(ValueError, match="out of range"):
        candidates_to_csr([[1, 2], [3, bad]], 2, 10)
    with pytest.raises(ValueError, match="out of range"):
        candidates_to_csr(np.array([[1, bad]], np.int64), 1, 10, unique=True)
    rp, col = candidates_to_csr([[9, -1, 0]], 1, 10)                      # the ends of the range and the padding id pass
    assert col.tolist() == [9, -1, 0]


def _plain_model(batch=4):
    class C:
        save = "/tmp/_cand_unused"; n_input = 50; hidden = 8; lr = 0.01; reg_lambda = 0.0; n_tracks = 40; initval = "NULL"
    C.batch = batch
    return DAE(C())


def test_bad_arguments_raise_before_anything_touches_the_device():
    """The model below was never fit(): it has no context, so reaching any launch would fail with an AttributeError."""
    m = _plain_model()
    pos, ones = np.array([[0, 1]], np.int64), np.ones(1, np.float32)
    with pytest.raises(ValueError, match="out of range"):
        m.score_candidates(pos, ones, [[1, 50]])
    with pytest.raises(ValueError, match="out of range"):
        m.rank_candidates(pos, ones, [[1, -7]], [[]], k=3)
    with pytest.raises(ValueError, match="kind"):
        m.score_candidates(pos, ones, [[1]], kind="softmax")


def test_a_model_with_a_scoring_shard_refuses():
    m = _plain_model()
    m.shard_scoring(0, 2)
    pos, ones = np.array([[0, 1]], np.int64), np.ones(1, np.float32)
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.score_candidates(pos, ones, [[1, 2]])
    with pytest.raises(_lib.DaeError, match="scoring shard"):
        m.rank_candidates(pos, ones, [[1, 2]], [[]], k=3)
