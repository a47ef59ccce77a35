"""CPU: the fp32 loss head of the training reference (oracle/dae_numpy.py fp32_head, grads_f32, the head="fp32" switch of
grads / grads_bf16, the intervals in bf16_bounds / f32_bounds / cost_interval; oracle/title_numpy.py likewise) checked
against the specification it restates -- a numpy float32 evaluation of DAEs.py:98-100 over the whole logit range -- against
the float64 head it replaces (different where fp32 saturates, identical bit for bit on every case the suite had), and the
input conditions of the saturated GPU cases (tests/test_gpu_train_saturated.py imports the case lists from here)."""
import numpy as np
import pytest

from oracle import dae_numpy as dn
from oracle import title_numpy as tn
from test_gpu_train_bf16_ref import CASES as BF16_CASES
from test_gpu_train_bf16_ref import make_case, reference

F = np.float32
U = 2.0 ** -24

# ---- the cases of tests/test_gpu_train_saturated.py ------------------------------------------------------------------
LOGITS = (4, 6, 8, 9.2, 10.5, 12, 13, 13.7, 13.9, 14.5, 15.5, 16.2, 16.6, 16.7, 17, 17.4, 20, 40, 87, 89, 104,
          -20, -25, -40, -87, -89, -104)
SATURATED = tuple(z for z in LOGITS if z >= 13.9)            # q = 1 - p < 1e-6: the fused kernel's exact branch


SHARD_EDGES = (672, 1024, 1344)


def plant_layout(V):
    """(column, logit, kind) for a vocabulary of V columns (tiles of 32).  V >= 600: column 0 and V - 1 saturated (V - 1
    in the last, partial tile when V % 32 != 0, next to columns past V), tile 2 (64..95) saturated in every column (with
    B % 32 == 0 rows in a wave: every lane on the exact branch), column 140 the only planted one of tile 4 (with one live
    row in a wave: one lane alone), then every logit of LOGITS as a negative, a target of 1 and a target of 0.5 / 2.0 in
    adjacent columns from 192 on, and eight saturated columns across each of SHARD_EDGES.  Smaller V (one or two tiles): every logit as a negative from column 1 on, a saturated
    target in column 0, a saturated negative in column V - 1."""
    if V < 600:
        out = [(0, 17.0, "pos"), (V - 1, 14.5, "neg")]
        out += [(1 + i, float(z), "neg") for i, z in enumerate(LOGITS) if 1 + i < V - 1]
        return out
    out = [(0, 17.0, "neg"), (V - 1, 14.5, "neg"), (V - 2, 20.0, "pos"), (140, 15.5, "neg")]
    out += [(64 + i, float(SATURATED[i % len(SATURATED)]), "neg") for i in range(32)]
    for b in SHARD_EDGES:                                   # a saturated run across each boundary of 2 and 3 shards of 2003
        if b + 4 <= V - 3:
            out += [(b - 4 + i, float(SATURATED[(3 * i) % len(SATURATED)]), "neg") for i in range(8)]
    for i, z in enumerate(LOGITS):
        out += [(192 + 3 * i + k, float(z), kind) for k, kind in enumerate(("neg", "pos", "mix"))]
    return out


PLANTED = [
    # V, nt, H, B, options                             the loss-head kernels train_plan selects (bf16 step | fp32 step)
    (2003, 1600, 256, 65, dict()),                     # decode_loss_dh_bf16 + loss_fixup<1,1,1> | decode_loss_shared_f32; partial
    #                                                    last tile; row 64 alone in its wave: one lane on the exact branch
    (2003, 1600, 256, 250, dict(tied=True, n_batch=256)),   # the same kernels, tied, n_batch > B, 26 live rows in the last wave
    (20000, 16000, 256, 65, dict()),                   # the same kernels, more tiles than workgroups
    (2003, 1600, 256, 65, dict(n_batch=365)),          # the same kernels; n_batch puts the exact dz of the logits 13 and 13.7 just
    #                                                    below a bf16 midpoint and 0.55 p / n_batch (the fused launch's short form
    #                                                    of a negative's dz) above it: test_short_form_flips_a_bf16_rounding
    (1500, 1200, 256, 64, dict()),                     # B <= 64: packed K5 (decode_f32_kernel EPI_LOSS, dz16) + loss_fixup<1,1> |
    #                                                    decode_f32_kernel EPI_LOSS fp32 + loss_fixup<0>
    (1101, 900, 128, 37, dict()),                      # hidden 128: decode_f32_kernel EPI_LOSS, dz16 + loss_fixup<1,1> | fp32
    (999, 800, 96, 70, dict(n_batch=80)),              # hidden 96: bf16 forward, fp32 dz: EPI_LOSS + loss_fixup<1> | fp32
    (1000, 800, 64, 33, dict(tied=True)),              # hidden 64, tied: as hidden 96
    (32, 20, 256, 250, dict()),                        # one tile (fused launch | shared fp32)
    (40, 30, 256, 65, dict()),                         # two tiles, the second partial with the saturated column V - 1
]

SPREAD = [
    # V, nt, H, B, options
    (3000, 2400, 256, 70, dict(spread=(12.0, 12), seed=9)),   # logits to 15.4: the band below the exact branch's threshold
    (3000, 2400, 256, 70, dict(spread=(16.0, 12))),    # logits to 22.3: > 100 elements on the exact branch, q = 0 admissible
    (3001, 2400, 128, 70, dict(spread=(14.0, 12), enc_scale=100.0)),   # hidden pre-activations past +-17 both ways
]
CAP_M0 = 0.002          # at most this share of a spread case's elements may have m = 0 admissible
CAP_COST = 0.02         # and its cost interval may be at most this wide, relative to the cost
MIN_Z105 = 0.0005       # at least this share of its logits above 10.5


def planted_case(V, nt, H, B, opt):
    return make_case(V, nt, H, B, planted=plant_layout(V), **opt)


# ---- the head against the specification ------------------------------------------------------------------------------
def _spec_fp32(z, y, n_batch):
    """DAEs.py:98-100 per element in numpy float32 (every operation rounds to fp32): (L, dz)."""
    z = z.astype(F)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        p = (F(1) / (F(1) + np.exp(-z, dtype=F))).astype(F)
        q = (F(1) - p).astype(F)
        a1 = (p + F(1e-10)).astype(F)
        a0 = (q + F(1e-10)).astype(F)
        L = -(F(y) * np.log(a1, dtype=F) + F(0.55) * F(1 - y) * np.log(a0, dtype=F))
        dz = -(F(y) / a1 - F(0.55) * F(1 - y) / a0) * p * q / F(n_batch)
    return L.astype(np.float64), dz.astype(np.float64)


def _z_grid():
    z = np.arange(-1100, 1101) / 10.0
    near = [c + d for c in (9.2, 13.8, 16.64, 88.0, -88.0) for d in np.arange(-40, 41) * 0.004]
    return np.concatenate([z, np.array(near)]).astype(F).astype(np.float64)          # logits the kernels can hold: fp32


@pytest.mark.parametrize("y", [0.0, 0.5, 1.0, 2.0])
def test_float32_evaluation_of_the_specification_lies_inside_the_interval(y):
    z = _z_grid()
    nb = 7
    hd = dn.fp32_head(z, y, nb)
    aL, adz = dn.head_allowance(hd, np.full(z.shape, y), nb)
    L, dz = _spec_fp32(z, y, nb)
    assert np.isfinite(L).all() and np.isfinite(dz).all()
    assert (hd["L_lo"] <= hd["L"]).all() and (hd["L"] <= hd["L_hi"]).all()
    assert (hd["dz_lo"] <= hd["dz"]).all() and (hd["dz"] <= hd["dz_hi"]).all()
    bad_L = (L < hd["L_lo"] - aL) | (L > hd["L_hi"] + aL)
    bad_d = (dz < hd["dz_lo"] - adz) | (dz > hd["dz_hi"] + adz)
    assert not bad_L.any(), (z[bad_L][:5], L[bad_L][:5], hd["L_lo"][bad_L][:5], hd["L_hi"][bad_L][:5])
    assert not bad_d.any(), (z[bad_d][:5], dz[bad_d][:5], hd["dz_lo"][bad_d][:5], hd["dz_hi"][bad_d][:5])
    # where q = 0 is admissible the fp32 result is one of the discrete values, within the hardware allowance
    for i in np.flatnonzero(hd["zero"])[::7]:
        cand = dn.head_candidates(z[i], y, nb)
        assert cand[0][0] == 0
        assert any(abs(dz[i] - d) <= 2.0 ** -18 * abs(d) + adz[i] - 2.0 ** -18 * max(abs(hd["dz_lo"][i]), abs(hd["dz_hi"][i]))
                   for _, _, d in cand), (z[i], dz[i], cand)


def test_the_saturated_values_of_the_specification():
    """The numbers the issue of record quotes: at q = 0 a negative's gradient is 0 and its loss term 12.66; at q = 2^-24
    they are 0.5491 / n_batch and 9.15."""
    (m0, L0, d0), (m1, L1, d1) = dn.head_candidates(17.0, 0.0, 1)[:2]
    assert (m0, m1) == (0, 1)
    assert d0 == 0.0 and abs(L0 - 12.66) < 0.005
    assert abs(d1 - 0.5491) < 1e-4 and abs(L1 - 9.15) < 0.005
    hd = dn.fp32_head(np.array([17.0, 40.0, 104.0, -104.0]), 0.0, 1)
    assert hd["zero"].tolist() == [True, True, True, False]
    assert (hd["dz_lo"][:3] == 0.0).all() and hd["dz_lo"][3] == 0.0 and hd["dz_hi"][3] < 1e-30


def test_the_window_covers_an_emulation_of_the_kernels_sigmoid():
    """arg = fl(-1.44269504f z), e = exp2(arg), s = fl(1 + e), p = rcp(s) in numpy float32, exp2 and rcp each the correctly
    rounded value moved by -1 / 0 / +1 ulp: inside head_window everywhere, and not by a wide margin above 0."""
    z = np.arange(-100, 110, 0.003).astype(F)
    z64 = z.astype(np.float64)
    p64 = 1.0 / (1.0 + np.exp(-z64))
    W, r = dn.head_window(z64)
    arg = (F(-1.44269504) * z).astype(F)
    with np.errstate(over="ignore"):
        e0 = np.exp2(arg.astype(np.float64)).astype(F)
    pos = z >= 0
    neg = ~pos & (p64 > 2.0 ** -120)                       # (below that p may be flushed to 0, which the head allows)
    worst_abs = worst_rel = 0.0
    for de in (-np.inf, 0, np.inf):
        e = np.maximum(e0 if de == 0 else np.nextafter(e0, F(de)), F(0))
        s = (F(1) + e).astype(F)
        p0 = (1.0 / s.astype(np.float64)).astype(F)
        for dr in (-np.inf, 0, np.inf):
            p = (p0 if dr == 0 else np.nextafter(p0, F(dr))).astype(np.float64)
            worst_abs = max(worst_abs, (np.abs(p - p64)[pos] / U).max())
            worst_rel = max(worst_rel, (np.abs(p - p64)[neg] / p64[neg] / U / r[neg]).max())
    print("worst deviation: %.4f units of 2^-24 at p >= 0.5 (window %d), %.3f of the relative window below"
          % (worst_abs, dn.HEAD_W, worst_rel))
    assert worst_abs <= dn.HEAD_W and worst_rel <= 1.0
    assert worst_abs > dn.HEAD_W - 1 and worst_rel > 0.5   # the window is not padded


def test_float64_head_differs_wherever_fp32_saturates():
    """Every negative with z >= 16.7: the float64 dz is outside rtol 2e-4 of the fp32 head's, and its loss term too."""
    z = np.arange(167, 1101) / 10.0
    hd = dn.fp32_head(z, 0.0, 1)
    p = 1.0 / (1.0 + np.exp(-z))
    dz64 = 0.55 / (1 - p + 1e-10) * p * (1 - p)
    L64 = -0.55 * np.log(1 - p + 1e-10)
    assert hd["zero"].all()
    assert (np.abs(dz64 - hd["dz"]) > 2e-7 + 2e-4 * np.abs(hd["dz"])).all()
    assert (np.abs(L64 - hd["L"]) > 2e-4 * np.abs(hd["L"])).all()
    # and below the saturated band the two are the same numbers
    z = np.arange(-1100, 150) / 10.0
    hd = dn.fp32_head(z, 0.0, 1)
    p = 1.0 / (1.0 + np.exp(-z))
    assert not hd["zero"].any()
    assert np.array_equal(hd["dz"], -(0.0 / (p + 1e-10) - 0.55 * (1 - 0.0) / (1 - p + 1e-10)) * p * (1 - p) / 1)


# ---- identical on every case the suite already had -------------------------------------------------------------------
def _same(a, b, keys=("cost", "gW_enc", "gb_enc", "gW_dec", "gb_dec")):
    for k in keys:
        if a[k] is None:
            assert b[k] is None
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


SMALL_BF16 = [c for c in BF16_CASES if c[0] <= 3001]
TRAIN_F32 = [(3000, 2400, 128, 37, False, 0.0), (1500, 1200, 64, 64, True, 0.0), (900, 700, 32, 10, False, 0.01),
             (2100, 2000, 256, 250, True, 0.02), (3000, 2500, 256, 37, False, 0.0), (33, 20, 256, 256, False, 0.0),
             (31, 20, 256, 3, False, 0.0)]                 # tests/test_gpu_train.py test_train_step_gradients, V <= 3001


@pytest.mark.parametrize("V,nt,H,B,opt", SMALL_BF16)
def test_fp32_head_equals_the_float64_head_on_the_bf16_cases(V, nt, H, B, opt):
    c = make_case(V, nt, H, B, **{k: v for k, v in opt.items() if k not in ("ikp", "kp")})
    c["h"] = None                                          # (float64 activations: nothing here touches a device)
    old, new = reference(c), reference(c, head="fp32")
    _same(old, new)
    assert np.array_equal(old["_aux"]["dz"], new["_aux"]["dz"])
    bo, bn = dn.bf16_bounds(old), dn.bf16_bounds(new)
    assert not bn["wide"].any() and not bn["zero"].any()
    for k in ("gW_enc", "gb_enc", "gW_dec", "gb_dec", "dh", "delta", "amb"):
        assert (bo[k] is None and bn[k] is None) or np.array_equal(bo[k], bn[k]), k
    lo, hi = dn.cost_interval(new, bn)
    assert lo <= old["cost"] <= hi


@pytest.mark.parametrize("V,nt,H,B,tied,lam", TRAIN_F32)
def test_fp32_head_equals_the_float64_head_on_the_fp32_cases(V, nt, H, B, tied, lam):
    c = make_case(V, nt, H, B, tied=tied, lam=lam)
    W_enc, b_enc, W_dec, b_dec = c["W"]
    Wd = W_enc if tied else W_dec
    old = dn.grads(c["x"], c["y"], W_enc, b_enc, Wd, b_dec, n_batch=B, tied=tied, reg_lambda=lam)
    new = dn.grads(c["x"], c["y"], W_enc, b_enc, Wd, b_dec, n_batch=B, tied=tied, reg_lambda=lam, head="fp32")
    _same(old, new)
    assert not new["_head"]["zero"].any()
    f32 = dn.grads_f32(c["x"], c["y"], W_enc, b_enc, Wd, b_dec, n_batch=B, tied=tied, reg_lambda=lam)
    for k in ("gW_enc", "gb_enc", "gW_dec", "gb_dec"):     # (the same arithmetic in grads_bf16's order of operations)
        assert old[k] is None or np.allclose(f32[k], old[k], rtol=1e-9, atol=1e-13), k
    assert not dn.f32_bounds(f32)["wide"].any()


# ---- the input conditions of the GPU cases, on the reference alone ---------------------------------------------------
def _stats(c, ref, b):
    z = ref["_aux"]["z"]
    lo, hi = dn.cost_interval(ref, b, summation=False)        # the head's part: what saturation makes uncertain
    return dict(zmin=float(z.min()), zmax=float(z.max()), z_gt_9p2=float((z > 9.2).mean()), z_gt_10p5=float((z > 10.5).mean()),
                n_q_lt_1e_6=int((b["q64"] < 1e-6).sum()), m0=float(b["zero"].mean()), wide=float(b["wide"].mean()),
                cost=float(ref["cost"]), cost_width=float((hi - lo) / abs(ref["cost"])))


@pytest.mark.parametrize("i", range(len(SPREAD)))
def test_spread_cases_meet_their_input_conditions(i):
    V, nt, H, B, opt = SPREAD[i]
    c = make_case(V, nt, H, B, **opt)
    for name, ref in (("bf16", reference(c, head="fp32")),
                      ("fp32", dn.grads_f32(c["x"], c["y"], *c["W"], n_batch=c["n_batch"], tied=False, h=c["h"]))):
        b = dn.bf16_bounds(ref)
        s = _stats(c, ref, b)
        print(name, s)
        assert s["m0"] <= CAP_M0 and s["cost_width"] <= CAP_COST, s
        assert s["z_gt_10p5"] >= MIN_Z105, s
        if opt["spread"][0] > 12.0:
            assert s["n_q_lt_1e_6"] >= 100, s
        if "enc_scale" in opt:
            pre = ref["_aux"]["xh"] @ ref["_aux"]["We"] + ref["_aux"]["be"]
            assert pre.max() > 17.0 and pre.min() < -17.0, (pre.min(), pre.max())


@pytest.mark.parametrize("i", range(len(PLANTED)))
def test_planted_cases_plant_what_they_say(i):
    V, nt, H, B, opt = PLANTED[i]
    c = planted_case(V, nt, H, B, opt)
    ref = reference(c, head="fp32")
    b = dn.bf16_bounds(ref)
    z = ref["_aux"]["z"]
    lay = plant_layout(V)
    assert len({col for col, _, _ in lay}) == len(lay)
    for col, logit, kind in lay:
        assert (z[:, col] == np.float64(F(logit))).all()                 # z is the planted logit, exactly, in every row
        ycol = c["y"][:, col]
        assert {"neg": (ycol == 0).all(), "pos": (ycol == 1).any() and (ycol == 0).any(),
                "mix": (ycol == 0.5).any() and (ycol == 2.0).any()}[kind]
        if kind == "neg":
            # q = 0 is admissible from m64 <= 3 on (z >= 15.54): 16.2 and above of the list, not 15.5
            assert b["zero"][:, col].all() == (logit >= 16.0) and b["zero"][:, col].any() == (logit >= 16.0)
    assert {z_ for _, z_, _ in lay} >= set(map(float, LOGITS)) or V < 64
    assert np.isfinite(ref["cost"]) and all(np.isfinite(ref[k]).all() for k in ("gW_enc", "gb_enc", "gb_dec"))
    if V >= 600:
        assert all(64 <= col < 96 and logit >= 13.9 for col, logit, _ in lay if 64 <= col < 96)
        assert sum(1 for col, _, _ in lay if 128 <= col < 160) == 1


def test_short_form_flips_a_bf16_rounding():
    """PLANTED's n_batch = 365 case is in a position to see the fused launch's 0.55 p / n_batch: at the planted logits 13 and
    13.7 the exact dz rounds to one bf16 value whichever way the hardware allowance (doubled) moves it, and 0.55 p / n_batch
    (off by 1e-10 / q = 4.4e-5 and 8.9e-5) rounds to the next one, so gb_dec of those columns moves by B bf16 steps."""
    nb = [o for *_, o in PLANTED if o.get("n_batch") == 365][0]["n_batch"]
    for z in (13.0, 13.7):
        z = np.float64(F(z))
        q = np.exp(-z) / (1 + np.exp(-z))
        exact, short = 0.55 * (1 - q) * q / (q + 1e-10) / nb, 0.55 * (1 - q) / nb
        r = dn.bf16_round(np.float64(exact))
        assert dn.bf16_round(np.float64(exact * (1 - 2.0 ** -17))) == r == dn.bf16_round(np.float64(exact * (1 + 2.0 ** -17)))
        assert dn.bf16_round(np.float64(short * (1 - 2.0 ** -17))) != r
        hd = dn.fp32_head(np.array([z]), 0.0, nb)
        aL, adz = dn.head_allowance(hd, np.zeros(1), nb)
        assert dn.bf16_round(hd["dz_lo"] - adz)[0] == r == dn.bf16_round(hd["dz_hi"] + adz)[0]


# ---- the title loss --------------------------------------------------------------------------------------------------
TITLE_W = ((0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.25, 0.75), (0.75, 0.125), (0.2, 0.6))


def _sigmoid32(z):
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-np.asarray(z, F), dtype=F))).astype(F)


def title_case(B=36, V=64):
    """Inputs of dae_title_loss_backward that plant the saturation points in the MIXED score: column v has the title logit
    LOGITS[v % 27] in every row, row r the mixing weights TITLE_W[r % 6] and DAE scores sigmoid(LOGITS[(v + r // 6) % 27]),
    so that with weights (0.5, 0.5) and equal logits, or (1, 0) / (0, 1), logit(yp) runs over LOGITS; targets alternate."""
    r, v = np.arange(B)[:, None], np.arange(V)[None, :]
    z = np.asarray(LOGITS, F)[(v % len(LOGITS)) + 0 * r]
    dae = _sigmoid32(np.asarray(LOGITS, F)[(v + r // len(TITLE_W)) % len(LOGITS)])
    w = np.asarray(TITLE_W, F)[np.arange(B) % len(TITLE_W)]
    y = ((r + v) % 2).astype(F)
    return z.astype(F), dae, y, w[:, 0].copy(), w[:, 1].copy()


def _title_spec_fp32(z, dae, y, wt, wp, n_batch):
    """title_loss_kernel's lines in numpy float32."""
    st = _sigmoid32(z)
    a = wt.astype(F)[:, None]
    yp = ((st * a).astype(F) + (dae * wp.astype(F)[:, None]).astype(F)).astype(F)
    a1 = (yp + F(1e-10)).astype(F)
    a0 = ((F(1) - yp).astype(F) + F(1e-10)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = -(y * np.log(a1, dtype=F) + F(0.55) * (F(1) - y) * np.log(a0, dtype=F))
        dz = -(y / a1 - F(0.55) * (F(1) - y) / a0) * F(1.0 / n_batch) * a * st * (F(1) - st)
    return L.astype(np.float64), dz.astype(np.float64)


def test_title_head_contains_a_float32_evaluation_and_saturates_where_float64_does_not():
    z, dae, y, wt, wp = title_case()
    nb = 40
    hd = tn.fp32_loss_head(z, dae, y, wt, wp, nb)
    L, dz = _title_spec_fp32(z, dae, y, wt, wp, nb)
    assert np.isfinite(L).all() and np.isfinite(dz).all()
    assert ((hd["L_lo"] <= L) & (L <= hd["L_hi"])).all()
    assert ((hd["dz_lo"] <= dz) & (dz <= hd["dz_hi"])).all()
    assert 50 <= hd["zero"].sum() <= 0.25 * z.size                   # the case reaches q = 0, in a minority of elements
    # float64's dz is outside the interval on most of those (it never sees q = 0)
    st = 1 / (1 + np.exp(-z.astype(np.float64)))
    yp = st * wt[:, None] + dae.astype(np.float64) * wp[:, None]
    dz64 = -(y / (yp + 1e-10) - 0.55 * (1 - y) / (1 - yp + 1e-10)) / nb * wt[:, None] * st * (1 - st)
    neg0 = hd["zero"] & (y == 0) & (st * (1 - st) * wt[:, None] > 1e-12)
    assert neg0.any()
    # an unsaturated grid: the interval is tight around float64 (relative width under 1e-3 of dz)
    zz = np.linspace(-6, 6, 64).astype(F)[None, :].repeat(36, 0)
    hd2 = tn.fp32_loss_head(zz, dae * F(0.5), y, wt, wp, nb)
    big = np.abs(hd2["dz_hi"]) > 1e-8
    assert ((hd2["dz_hi"] - hd2["dz_lo"])[big] <= 1e-3 * np.abs(hd2["dz_hi"])[big]).all()
