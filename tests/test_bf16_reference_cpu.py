"""CPU: the rounding-aware float64 reference of the bf16 training step (oracle/dae_numpy.py grads_bf16, bf16_bounds,
bf16_check) -- bf16_round against torch's conversion, grads_bf16 against grads where the two must agree, and the checker's
teeth: it accepts the reference (also with one-ulp flips of the ambiguous dz elements) and rejects each of five single
faults at V = 20 000, several of which a 2e-2-of-the-norm comparison lets through."""
import numpy as np
import pytest
import torch

import oracle
from oracle import dae_numpy as dn
from spotify_recsys_challenge_2018_amd.models.DAEs import coo_to_csr
from spotify_recsys_challenge_2018_amd.utils.synthetic import make_playlists, make_weights


def _torch_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_round_matches_torch_on_ties_subnormals_large_and_negative():
    bits = []
    for hi in (0x3F80, 0x3F81, 0x4000, 0x4001, 0x0000, 0x0001, 0x007F, 0x0080, 0x7F7E, 0x7F7F, 0x1234, 0x5A5B):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):       # below, at and above the midpoint
            bits += [(hi << 16) | lo, ((hi | 0x8000) << 16) | lo]
    rng = np.random.default_rng(0)
    bits += list(rng.integers(0, 0x7F7F0000, 4000, dtype=np.int64))
    bits += list(rng.integers(0, 0x7F7F0000, 4000, dtype=np.int64) | 0x80000000)
    a = np.array(bits, np.uint64).astype(np.uint32).view(np.float32)
    got = dn.bf16_round(a)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), _torch_bf16(a).view(np.uint32))
    # ties go to the even mantissa, both ways
    assert dn.bf16_round(np.float32(1.0 + 2 ** -8)) == np.float32(1.0)
    assert dn.bf16_round(np.float32(1.0 + 3 * 2 ** -8)) == np.float32(1.0 + 2 ** -6)
    # the float64 form rounds once: it agrees with the fp32 form wherever the value is an fp32, and does not double-round
    finite = a[np.isfinite(_torch_bf16(a))]
    assert np.array_equal(dn.bf16_round(finite.astype(np.float64)), dn.bf16_round(finite).astype(np.float64))
    x = 1.0 + 2 ** -8 + 2 ** -30                      # just above a midpoint; fp32 would round it onto the midpoint
    assert dn.bf16_round(np.float64(x)) == 1.0 + 2 ** -7
    assert dn.bf16_round(np.float32(x)) == np.float32(1.0)
    assert dn.bf16_ulp(1.5) == 2 ** -7 and dn.bf16_ulp(-3.0) == 2 ** -6 and dn.bf16_ulp(1e-45) == 2.0 ** -133


def _case(V, nt, H, B, seed=6, tied=False):
    W_enc, b_enc, W_dec, b_dec = make_weights(V, H, seed=4, bias="zipf", n_tracks=nt, tied=tied)
    b_enc = (np.random.default_rng(2).standard_normal(H) * 0.1).astype(np.float32)
    pos, ones, _ = make_playlists(B, nt, V - nt, seed=seed, seed_counts=(3, 9, 20))
    xr, xc, xv = coo_to_csr(pos[pos[:, 1] < nt], ones[pos[:, 1] < nt], B, V)
    y = dn.sparse_to_dense(pos, np.ones(len(pos), np.float32), B, V)
    x = dn.sparse_to_dense(pos[pos[:, 1] < nt], ones[pos[:, 1] < nt], B, V)
    h = oracle.encode(xr, xc, xv, W_enc, b_enc)
    return x, y, W_enc, b_enc, W_dec, b_dec, h


def test_grads_bf16_reduces_to_grads():
    V, nt, H, B = 700, 600, 128, 19
    x, y, W_enc, b_enc, W_dec, b_dec, _ = _case(V, nt, H, B)
    for tied, lam in ((False, 0.0), (True, 0.01)):
        Wd = W_enc if tied else W_dec                 # (grads() decodes with its W_dec argument: the tied model passes W_enc)
        ref = dn.grads(x, y, W_enc, b_enc, Wd, b_dec, n_batch=23, tied=tied, reg_lambda=lam)
        got = dn.grads_bf16(x, y, W_enc, b_enc, Wd, b_dec, n_batch=23, tied=tied, reg_lambda=lam,
                            round_dz=False, round_ops=False)
        for k in ("cost", "gW_enc", "gb_enc", "gb_dec") + (() if tied else ("gW_dec",)):
            assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-18), k
    # bf16-representable operands: h (sigmoid(b_enc) with W_enc = 0, b_enc the log-odds of bf16 values) and W_dec; the
    # default rounding of h and W then changes nothing, and only the dz store is left, here switched off
    q = dn.bf16_round(np.random.default_rng(3).uniform(0.1, 0.9, H).astype(np.float32)).astype(np.float64)
    b_enc16 = np.log(q / (1 - q))
    W_enc0 = np.zeros_like(W_enc)
    W_dec16 = dn.bf16_round(W_dec)
    ref = dn.grads(x, y, W_enc0, b_enc16, W_dec16, b_dec, n_batch=B, tied=False)
    got = dn.grads_bf16(x, y, W_enc0, b_enc16, W_dec16, b_dec, n_batch=B, tied=False, round_dz=False)
    assert np.array_equal(got["_aux"]["hb"], dn.bf16_round(got["_aux"]["h"]))
    assert np.allclose(got["_aux"]["hb"], got["_aux"]["h"], rtol=1e-15)
    for k in ("cost", "gW_enc", "gb_enc", "gW_dec", "gb_dec"):
        assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-18), k


def _old_global_check(got, ref, k):
    """tests/test_gpu_train.py::test_train_step_bf16_gemms' criterion: within 2e-2 of the gradient's Frobenius norm."""
    return np.linalg.norm(np.asarray(got[k], np.float64) - ref[k]) / np.linalg.norm(ref[k]) <= 2e-2


@pytest.fixture(scope="module")
def big():
    V, nt, H, B = 20000, 16000, 128, 64
    x, y, W_enc, b_enc, W_dec, b_dec, h = _case(V, nt, H, B, seed=8)
    # targets at column 0, at V - 1 and inside the last partial 64-column tile
    y[0, 0] = y[1, V - 1] = y[2, V - 5] = 1.0
    ref = dn.grads_bf16(x, y, W_enc, b_enc, W_dec, b_dec, n_batch=B, tied=False, h=h)
    bnd = dn.bf16_bounds(ref)
    return dict(V=V, H=H, B=B, x=x, y=y, W=(W_enc, b_enc, W_dec, b_dec), h=h, ref=ref, bnd=bnd)


KEYS = ("gW_enc", "gb_enc", "gW_dec", "gb_dec")


def test_checker_accepts_the_reference_and_its_midpoint_flips(big):
    ref, bnd = big["ref"], big["bnd"]
    assert max(dn.bf16_check(ref, ref, bnd).values()) == 0.0
    a = ref["_aux"]
    amb = bnd["amb"]
    assert amb.any(), "no ambiguous dz element: the flip case tests nothing"
    dz = ref["dzb"].copy()
    lo, hi = dn.bf16_round(a["dz"] - bnd["delta"]), dn.bf16_round(a["dz"] + bnd["delta"])
    dz[amb] = np.where(lo[amb] != dz[amb], lo[amb], hi[amb])       # the other neighbour of every ambiguous element
    assert (dz != ref["dzb"]).sum() == amb.sum()
    flipped = dn.bf16_backward(a, dz, rounded=True)
    r = dn.bf16_check(flipped, ref, bnd)
    assert max(r.values()) <= 1.0, r


def _faults(big):
    ref = big["ref"]
    a = ref["_aux"]
    V, B = big["V"], big["B"]
    out = {}
    g = {k: ref[k].copy() for k in KEYS}
    g["gW_dec"][4321] = 0.0
    out["one gW_dec row zeroed"] = g
    dz = a["dz"].copy()
    r = 5
    pos = big["y"][r] != 0
    dz[r, pos] = 0.55 * a["p"][r, pos] / (1 - a["p"][r, pos] + 1e-10) * (1 - a["p"][r, pos]) / B     # its value as a negative
    out["one playlist's positives left at their negative dz"] = dn.bf16_backward(a, dz)
    dz = a["dz"].copy()
    dz[:, V // 64 * 64:] = 0.0
    out["last partial tile of columns dropped"] = dn.bf16_backward(a, dz)
    dz = a["dz"].copy()
    dz[:, 12345] = -dz[:, 12345]
    out["sign error on one decoder column"] = dn.bf16_backward(a, dz)
    W_enc, b_enc, W_dec, b_dec = big["W"]
    out["every operand fp32"] = dn.grads_bf16(big["x"], big["y"], W_enc, b_enc, W_dec, b_dec, n_batch=B, tied=False,
                                              h=big["h"], round_dz=False, round_ops=False)
    return out


# whether the 2e-2-of-the-norm criterion lets the fault through on every gradient (measured; the new check must not)
OLD_MISSES = {"one gW_dec row zeroed": True, "one playlist's positives left at their negative dz": False,
              "last partial tile of columns dropped": False, "sign error on one decoder column": True,
              "every operand fp32": True}


@pytest.mark.parametrize("fault", list(OLD_MISSES))
def test_checker_rejects_each_single_fault(big, fault):
    ref, bnd = big["ref"], big["bnd"]
    got = _faults(big)[fault]
    r = dn.bf16_check(got, ref, bnd)
    assert max(r.values()) > 1.0, (fault, r)
    old_passes = all(_old_global_check(got, ref, k) for k in KEYS)
    if OLD_MISSES[fault] is not None:
        assert old_passes == OLD_MISSES[fault], (fault, r)
    print("%s: ratios %s, the 2e-2 global check %s" % (fault, r, "passes it" if old_passes else "catches it"))
