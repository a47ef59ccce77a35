"""CPU: the title scorer's reference helpers (oracle/title_numpy.py) that the GPU title tests lean on.

fma32 is checked against exact rational arithmetic, grads() against torch.autograd in float64, features_f32_chain
against the float64 features within feature_bounds, and title_grad_bounds two ways: a float32 evaluation of the same
graph (another summation order, other transcendentals) lies inside it, and five single faults of the kind a
backward kernel could have lie outside it."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import title_numpy as tn

N_CHAR = 41


def _round_f32(fr):
    """The float32 nearest to the rational fr, ties to even."""
    x = np.float32(float(fr))
    cands = [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.array(c).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_is_the_exact_fused_multiply_add():
    rng = np.random.default_rng(0)
    n = 3000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    c = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32)
    # edges where rounding a * b + c to float64 first lands on a float32 midpoint and ties-to-even then goes the wrong
    # way: a b = 2^-18 (1 - m^2 2^-46) just below half an ulp of c = 64 + 2^-17 (odd last bit), scaled and signed
    m = rng.integers(1, 300, 400).astype(np.float64)
    k = rng.integers(-30, 30, 400).astype(np.float64)
    sg = rng.choice([-1.0, 1.0], 400)
    ea = (1 + m * 2.0 ** -23).astype(np.float32)
    eb = (sg * np.exp2(k - 18) * (1 - m * 2.0 ** -23)).astype(np.float32)
    ec = (sg * np.exp2(k) * (64 + 2.0 ** -17)).astype(np.float32)
    a, b, c = np.concatenate([a, ea]), np.concatenate([b, eb]), np.concatenate([c, ec])
    got = tn.fma32(a, b, c)
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)],
                    np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    naive = (a.astype(np.float64) * b + c).astype(np.float32)                  # double rounding
    assert not np.array_equal(naive[-400:], want[-400:])                        # the edges are edges


def _case(E, fs, F, L, V=300, B=9, seed=0, kp=1.0):
    rng = np.random.default_rng(seed)
    p = tn.make_params(N_CHAR, E, fs, F, V, seed=seed)
    t = rng.integers(0, N_CHAR, (B, L))
    for r in range(B):
        t[r, int(rng.integers(1, L + 1)):] = -1
    t[0, :] = -1                                                              # an all-padding title
    t[1, 0], t[1, 1] = N_CHAR, 1000                                            # ids >= charsize
    t[2, 0], t[2, 1] = -7, -(2 ** 31)                                          # negative ids other than -1
    dae = 1.0 / (1.0 + np.exp(-rng.standard_normal((B, V))))
    y = (rng.random((B, V)) < 0.05).astype(np.float64)
    wt, wp = tn.mix_weights(rng.integers(0, 30, B), 1.0, (np.arange(B) % 4 != 3).astype(np.float32))
    km = np.floor(np.float32(kp) + rng.random((B, len(fs) * F)).astype(np.float32)) if kp < 1.0 else None
    return dict(titles=t, params=p, fs=fs, dae=dae, y=y, wt=wt, wp=wp, km=km, kp=kp)


def _torch_grads(c, dtype, argmax=None):
    """The title graph (Char_CNN.py:23-72, DAEs.py:176-195) under torch.autograd: returns cost, grads by TF name, argmax."""
    p, fs = c["params"], c["fs"]
    T = lambda a, g=True: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=g)
    v = {k: T(a) for k, a in p.items()}
    ids = torch.from_numpy(np.asarray(c["titles"], np.int64))
    ok = (ids >= 0) & (ids < N_CHAR)
    x = v["char_embedding"][torch.where(ok, ids, 0)] * ok[..., None].to(dtype)
    feats, args = [], []
    for i, f in enumerate(fs):
        win = x.unfold(1, f, 1).permute(0, 1, 3, 2).reshape(x.shape[0], x.shape[1] - f + 1, -1)       # [B, P, fs * E]
        conv = torch.relu(win @ v["Conv_W%d" % i].reshape(-1, v["Conv_W%d" % i].shape[-1]) + v["Conv_b%d" % i])
        F_ = conv.shape[2]
        if argmax is None:
            mx, ix = conv.max(dim=1)
        else:
            ix = torch.from_numpy(argmax[:, i * F_:(i + 1) * F_])
            mx = torch.gather(conv, 1, ix[:, None, :])[:, 0, :]
        feats.append(mx)
        args.append(ix)
    f = torch.cat(feats, 1) / c["kp"]
    if c["km"] is not None:
        f = f * torch.from_numpy(c["km"]).to(dtype)
    st = torch.sigmoid(f @ v["Output_W"] + v["Output_b"])
    wt, wp = T(c["wt"], False), T(c["wp"], False)
    yp = st * wt + T(c["dae"], False) * wp
    y = T(c["y"], False)
    B = y.shape[0]
    cost = -(y * torch.log(yp + 1e-10) + 0.55 * (1 - y) * torch.log(1 - yp + 1e-10)).sum() / B
    cost.backward()
    return float(cost.detach()), {k: t.grad.numpy().astype(np.float64) for k, t in v.items()}, torch.cat(args, 1).numpy()


def _ref(c, **kw):
    return tn.grads(c["titles"], c["params"], c["fs"], c["dae"], c["y"], c["wt"], c["wp"], c["y"].shape[0],
                    keep_mask=c["km"], keep_prob=c["kp"], **kw)


SHAPES = {                                    # (E, filter sizes, F, L)
    "odd_E": (7, [3, 5], 5, 12),
    "fs_1_and_L": (6, [1, 12], 4, 12),
    "eight_sizes": (4, [1, 2, 3, 4, 5, 6, 7, 8], 3, 12),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("kp", [1.0, 0.75])
def test_grads_equal_float64_autograd(name, kp):
    E, fs, F, L = SHAPES[name]
    c = _case(E, fs, F, L, kp=kp, seed=len(name))
    cost_t, g_t, arg_t = _torch_grads(c, torch.float64)
    cost, g, info = _ref(c, argmax=arg_t)        # (torch's max picks its own index on ties: the all-padding row)
    assert abs(cost - cost_t) <= 1e-12 * abs(cost_t)
    assert sorted(g) == sorted(g_t)
    for k in g:
        scale = max(1e-300, float(np.abs(g_t[k]).max()))
        assert np.max(np.abs(g[k] - g_t[k])) <= 1e-12 * scale, k
    # ids outside [0, charsize) embed to zero and receive nothing: the all-padding row gives only bias gradients
    assert not np.any(info["_aux"]["x"][0]) and not np.any(info["_aux"]["x"][2, :2])
    # without the override: the float64 forward's own first maximum, the same off the all-padding row
    _, _, info_d = _ref(c)
    assert np.array_equal(info_d["argmax"][1:], arg_t[1:])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_chain_features_within_their_bound(name):
    E, fs, F, L = SHAPES[name]
    c = _case(E, fs, F, L, seed=3)
    chain, arg = tn.features_f32_chain(c["titles"], c["params"], fs)
    f64 = tn.features(c["titles"], c["params"], fs)
    bound = tn.feature_bounds(c["titles"], c["params"], fs)
    assert chain.dtype == np.float32 and np.all(np.abs(chain - f64) <= bound)
    assert np.all(arg < L - np.repeat(fs, F) + 1)
    assert np.all(bound > 0) and np.any(chain != f64.astype(np.float32))      # rounding happened, and is covered


def _fault_case():
    # 2 sizes x 40 filters: the last MFMA block (32 filters) is partial; dropout on; padding everywhere
    return _case(9, [3, 4], 40, 14, V=400, B=16, seed=5, kp=0.8)


def test_float32_autograd_is_inside_the_bound():
    """Another fp32 evaluation of the same graph (torch's order of sums, its own exp / log) lies inside the bound: the
    bound does not reject honest rounding.  The reference routes through the float32 run's argmax, as the GPU tests route
    through the chain kernels'."""
    c = _fault_case()
    c32 = dict(c, params={k: a.astype(np.float32) for k, a in c["params"].items()},
               dae=c["dae"].astype(np.float32), y=c["y"].astype(np.float32))
    _, g32, arg32 = _torch_grads(c32, torch.float32)
    chain, arg_c = tn.features_f32_chain(c["titles"], c["params"], c["fs"])
    cost, g, info = _ref(c, argmax=arg32, gate=chain > 0)
    bounds = tn.title_grad_bounds(info)
    ratios = tn.grad_check(g32, g, bounds)
    print("float32 autograd error / bound:", {k: "%.3g" % v for k, v in sorted(ratios.items())})
    assert max(ratios.values()) <= 1.0, ratios
    assert max(ratios.values()) > 1e-4           # (the check compares something)


def test_bound_rejects_single_faults():
    """Each fault is one a kernel could plausibly have; every one must leave the bound.  The old check (np.allclose with
    rtol 2e-4, atol 2e-7) is evaluated on the same faults and its misses are printed."""
    c = _fault_case()
    chain, arg = tn.features_f32_chain(c["titles"], c["params"], c["fs"])
    gate = chain > 0
    cost, g, info = _ref(c, argmax=arg, gate=gate)
    bounds = tn.title_grad_bounds(info)
    a = info["_aux"]
    fs, F = c["fs"], 40
    P = np.concatenate([np.full(F, 14 - f + 1) for f in fs])
    assert (~gate).any() and (arg < P - 1).any()

    def rebuild(dg=None, arg_=None, titles=None):
        gW, gb, gE = tn.conv_backward(a["x"], a["titles"] if titles is None else titles, a["Ws"],
                                      a["dg"] if dg is None else dg, a["arg"] if arg_ is None else arg_, fs, N_CHAR)
        out = dict(g)
        for i in range(len(fs)):
            out["Conv_W%d" % i] = gW[i][:, :, None, :]
            out["Conv_b%d" % i] = gb[i]
        out["char_embedding"] = gE
        return out

    # gradient to the window after the argmax (clamped to the last window)
    f_arg = rebuild(arg_=np.minimum(arg + 1, P - 1))
    # the -1 padding id indexing the last embedding row (numpy's / an unchecked load's wrap-around)
    t_wrap = np.where(a["titles"] == -1, N_CHAR - 1, a["titles"])
    _, _, gE_wrap = tn.conv_backward(a["x"], t_wrap, a["Ws"], a["dg"], a["arg"], fs, N_CHAR)
    f_wrap = dict(g, char_embedding=gE_wrap)
    # the gate's dropout scaled by x kp instead of / kp
    f_kp = rebuild(dg=a["dg"] * c["kp"] * c["kp"])
    # the last filter of the partial last block dropped
    dg = a["dg"].copy()
    dg[:, len(fs) * F - 1] = 0.0
    f_drop = rebuild(dg=dg)
    # a feature whose ReLU is closed passing gradient: title_gate_kernel not gating (the forward unchanged)
    f_relu = rebuild(dg=a["dfeat"] * a["km"] / c["kp"])
    assert (~gate & (a["dfeat"] * a["km"] != 0)).any()
    faults = {"argmax+1": f_arg, "pad_wraps_to_last_row": f_wrap, "dropout_times_kp": f_kp,
              "partial_block_filter_dropped": f_drop, "closed_relu_passes": f_relu}
    missed_old = []
    for name, got in faults.items():
        r = tn.grad_check(got, g, bounds)
        assert max(r.values()) > 1.0, (name, r)
        if all(np.allclose(got[k], g[k], rtol=2e-4, atol=2e-7) for k in g):
            missed_old.append(name)
    assert tn.grad_check(g, g, bounds) == {k: 0.0 for k in g}

    # As the GPU tests check a step: on the kernels' own title logits (z=) and their own dfeat, so that only the loss
    # kernel's, the backward GEMMs' and the conv backward's rounding is bounded.  Two faults that stay inside rtol 2e-4:
    zf = a["z"].astype(np.float32)
    _, gz, iz = _ref(c, argmax=arg, gate=gate, z=zf)
    bz = tn.title_grad_bounds(iz, dae_zerr=None)
    rc, bc = tn.conv_grads_from_dfeat(iz, iz["_aux"]["dfeat"])
    assert all(np.allclose(rc[k], gz[k], rtol=1e-12, atol=0) for k in rc)      # the same gradients, given dfeat
    # title_loss_kernel on a low-precision exp (relative error 2^-16, a fast approximation instead of v_exp_f32)
    _, g_exp, _ = _ref(c, argmax=arg, gate=gate, z=zf.astype(np.float64) - 2.0 ** -16)
    # title_gate_kernel's grid-stride loop one playlist short: row 5 of dg never written (left 0)
    d5 = iz["_aux"]["dfeat"].copy()
    d5[5] = 0.0
    r5, _ = tn.conv_grads_from_dfeat(iz, d5)
    for name, got, ref_, bd in (("exp_2^-16", g_exp, gz, bz), ("gate_row_dropped", r5, rc, bc)):
        r = tn.grad_check({k: got[k] for k in ref_}, ref_, bd)
        assert max(r.values()) > 1.0, (name, r)
        if all(np.allclose(got[k], ref_[k], rtol=2e-4, atol=2e-7) for k in ref_):
            missed_old.append(name)
        for k in ref_:                                   # and no bound is vacuous: half of any gradient leaves it
            assert tn.grad_check({k: 0.5 * ref_[k]}, {k: ref_[k]}, bd)[k] > 1.0, (name, k)
    print("faults the old rtol check lets through:", missed_old or "none")
    assert "exp_2^-16" in missed_old
