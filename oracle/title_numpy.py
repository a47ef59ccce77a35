"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the reference's title scorer and of the DAE_title
mix (citations relative to /root/reference):

  models/title_models/Char_CNN.py:6-75   character embedding -> parallel "wide" convolutions over the
                                         title (one per filter size, VALID) -> ReLU -> max over time ->
                                         concat -> dropout -> sigmoid(features . Output_W + Output_b)
  models/DAEs.py:153-181 (App. B.6)      y = title_score * w_title + dae_score * w_playlist with
                                         x_count = row_sum * input_keep_prob,
                                         w_title = u / (u + x_count + 1e-10), w_playlist = x_count / (same)

PARITY UNPINNED like the rest of the TensorFlow boundary (oracle/dae_oracle.c header).  One documented
assumption: title indices are padded with -1 (spotify_reader.py:36) and tf.nn.embedding_lookup on the
GPU returns a ZERO vector for an out-of-range id (the CPU kernel raises); padding therefore embeds to 0.
Float64 internally so that it is a trustworthy yardstick for the fp32 kernels (gradients included).
"""
import numpy as np


def xavier_normal(rng, shape, fan_in, fan_out):
    """tf.contrib.layers.xavier_initializer(uniform=False): N(0, 2 / (fan_in + fan_out)), truncated at 2 sd
    in TF; the restatement draws a plain normal (only used to make test weights)."""
    return (rng.standard_normal(shape) * np.sqrt(2.0 / (fan_in + fan_out))).astype(np.float32)


def make_params(n_char, emb, filter_sizes, filter_num, n_output, seed=0):
    """The variables Char_CNN.py creates, under their TF names."""
    rng = np.random.default_rng(seed)
    p = {"char_embedding": xavier_normal(rng, (n_char, emb), n_char, emb)}
    for i, fs in enumerate(filter_sizes):
        p["Conv_W%d" % i] = xavier_normal(rng, (fs, emb, 1, filter_num), fs * emb, fs * emb * filter_num)
        p["Conv_b%d" % i] = xavier_normal(rng, (filter_num,), filter_num, 1)
    d = filter_num * len(filter_sizes)
    p["Output_W"] = xavier_normal(rng, (d, n_output), d, n_output)
    p["Output_b"] = xavier_normal(rng, (n_output,), n_output, 1)
    return p


def embed(titles, E):
    titles = np.asarray(titles, dtype=np.int64)
    ok = (titles >= 0) & (titles < E.shape[0])
    out = E.astype(np.float64)[np.where(ok, titles, 0)]
    out[~ok] = 0.0                                                   # padding (-1) embeds to zero
    return out                                                       # [B, L, emb]


def features(titles, params, filter_sizes, return_argmax=False):
    """Char_CNN.py:31-62 -> [B, n_sizes * filter_num] (before dropout)."""
    x = embed(titles, params["char_embedding"])
    B, L, _ = x.shape
    feats, args = [], []
    for i, fs in enumerate(filter_sizes):
        W = params["Conv_W%d" % i].astype(np.float64)[:, :, 0, :]   # [fs, emb, F]
        b = params["Conv_b%d" % i].astype(np.float64)
        P = L - fs + 1
        conv = np.stack([np.einsum("bdc,dcf->bf", x[:, p:p + fs, :], W) for p in range(P)], axis=1) + b
        conv = np.maximum(conv, 0.0)                                 # :49-50
        feats.append(conv.max(axis=1))                               # :56 one-max pooling
        args.append(conv.argmax(axis=1))
    f = np.concatenate(feats, axis=1)
    return (f, np.concatenate(args, axis=1)) if return_argmax else f


def forward(titles, params, filter_sizes, keep_mask=None, keep_prob=1.0):
    """-> (features after dropout, logits, title_score) ; Char_CNN.py:64-72."""
    f = features(titles, params, filter_sizes) / keep_prob
    if keep_mask is not None:
        f = f * keep_mask
    z = f @ params["Output_W"].astype(np.float64) + params["Output_b"].astype(np.float64)
    return f, z, 1.0 / (1.0 + np.exp(-z))


def mix_weights(row_sum, input_keep_prob, titles_use):
    """DAEs.py:159-162.  Returns (w_title, w_playlist) as float32 columns, computed in fp32 like the graph."""
    F = np.float32
    x_count = np.asarray(row_sum, F).reshape(-1, 1) * F(input_keep_prob)
    u = np.asarray(titles_use, F).reshape(-1, 1)
    deno = u + x_count + F(1e-10)
    return (u / deno).astype(F), (x_count / deno).astype(F)


def mix(title_score, dae_score, w_title, w_playlist):
    """DAEs.py:180."""
    return title_score * w_title + dae_score * w_playlist




# ---- the fp32 kernels' arithmetic, and what the training step's gradients may differ by ---------------------------------

U32 = 2.0 ** -24                       # unit roundoff of fp32


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays (broadcast), exactly: the product is exact in float64 (24 + 24 bits); the sum is
    rounded to ODD in float64 (TwoSum gives its error), so the final rounding to float32 is the single rounding of the
    exact a * b + c (Boldo & Melquiond: 53 >= 2 * 24 + 2)."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p, c = np.broadcast_arrays(p, c)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                    # p + c == s + err exactly
    bits = np.ascontiguousarray(s).view(np.int64)
    inexact = err != 0.0
    # the exact sum lies between s and its neighbour in the direction of err: of the two, take the one with an odd last
    # bit.  s is even here -> step one ulp towards err (same sign as s: magnitude up, else magnitude down).
    step = np.where((err > 0) == (s > 0), 1, -1).astype(np.int64)
    adj = np.where(inexact & ((bits & 1) == 0) & (s != 0.0), bits + step, bits)
    return adj.view(np.float64).astype(np.float32)


def _windows(x, fs):
    """[B, L, E] -> [B, P, fs * E]: the window at position p flattened as q = dp * E + c."""
    B, L, E = x.shape
    return np.stack([x[:, p:p + fs, :].reshape(B, fs * E) for p in range(L - fs + 1)], axis=1)


def features_f32_chain(titles, params, filter_sizes):
    """The features as the chain kernels of csrc/title.hip compute them (title_features_kernel, _wave_kernel, _mfma_kernel;
    DESIGN.md section 2): per (position, filter) acc = bias, then acc = fmaf(x[q], W[q][f], acc) for q = dp * E + c
    ascending; ReLU; the FIRST maximum over the positions.  -> (features float32 [B, n_sizes * F], argmax int64 [same])."""
    x = embed(titles, params["char_embedding"]).astype(np.float32)        # float32 values: exact
    B, L, E = x.shape
    feats, args = [], []
    for i, fs in enumerate(filter_sizes):
        W = np.asarray(params["Conv_W%d" % i], np.float32)[:, :, 0, :].reshape(fs * E, -1)
        b = np.asarray(params["Conv_b%d" % i], np.float32)
        win = _windows(x, fs)
        acc = np.broadcast_to(b, (B, win.shape[1], W.shape[1])).astype(np.float32)
        for q in range(fs * E):
            acc = fma32(win[:, :, q:q + 1], W[q][None, None, :], acc)
        conv = np.maximum(acc, np.float32(0.0))
        feats.append(conv.max(axis=1))
        args.append(conv.argmax(axis=1))                                    # first maximum
    return np.concatenate(feats, axis=1), np.concatenate(args, axis=1).astype(np.int64)


def _convs64(x, params, filter_sizes):
    """float64 convolutions before the ReLU, one [B, P, F] array per size, and their magnitudes |b| + sum |x W|."""
    out, mag = [], []
    for i, fs in enumerate(filter_sizes):
        W = params["Conv_W%d" % i].astype(np.float64)[:, :, 0, :]
        W = W.reshape(fs * W.shape[1], -1)
        b = params["Conv_b%d" % i].astype(np.float64)
        win = _windows(x, fs)
        out.append(win @ W + b)
        mag.append(np.abs(win) @ np.abs(W) + np.abs(b))
    return out, mag


def feature_bounds(titles, params, filter_sizes, extra_terms=0):
    """Element-wise bound on |fp32 feature - exact feature| for an fp32 evaluation of each convolution that rounds at most
    n = fs * E + 1 + extra_terms times: (n + 1) u max_pos (|b| + sum |x W|).  The chain kernels round fs * E times (one fmaf
    per term); the table path (title_features_table_kernel) rounds E times per table entry, then fs additions of the
    entries and the bias -- pass extra_terms = E + fs - fs * E for it (n = E + fs + 1).  Any order of a sum of n terms is
    within n u / (1 - n u) sum |terms| of it (Higham, Accuracy and Stability, 3.1); the + 1 covers the 1 / (1 - n u).
    ReLU and the max over positions move no value by more than the largest error of their inputs."""
    x = embed(titles, params["char_embedding"])
    E = x.shape[2]
    _, mag = _convs64(x, params, filter_sizes)
    return np.concatenate([(fs * E + 2 + extra_terms) * U32 * m.max(axis=1) for fs, m in zip(filter_sizes, mag)], axis=1)


def conv_backward(x, titles, Ws, dg, arg, filter_sizes, n_char):
    """Back through max over time -> convolution -> embedding, from the gated feature gradient dg [B, n_sizes * F]
    (float64): the gradient of a feature reaches the window at its argmax only.  x: the embedded titles [B, L, E]; Ws:
    [fs, E, F] per size.  -> (gW list, gb list, gE [n_char, E]).  Ids outside [0, n_char) receive nothing."""
    B, L, E = x.shape
    F = Ws[0].shape[2]
    titles = np.asarray(titles, np.int64)
    arg = np.asarray(arg, np.int64)
    gE = np.zeros((n_char, E))
    gWs, gbs = [], []
    bi = np.arange(B)[:, None]
    fidx = np.broadcast_to(np.arange(F), (B, F))
    for i, fs in enumerate(filter_sizes):
        d = dg[:, i * F:(i + 1) * F]
        a = arg[:, i * F:(i + 1) * F]
        gW = np.empty((fs, E, F))
        for dp in range(fs):
            pos = a + dp
            gW[dp] = np.einsum("bf,bfe->ef", d, x[bi, pos])
            t = titles[bi, pos]
            ok = (t >= 0) & (t < n_char) & (d != 0)
            np.add.at(gE, t[ok], d[ok][:, None] * Ws[i][dp].T[fidx[ok]])
        gWs.append(gW)
        gbs.append(d.sum(axis=0))
    return gWs, gbs, gE


def grads(titles, params, filter_sizes, dae_score, y, w_title, w_playlist, n_batch, keep_mask=None, keep_prob=1.0,
          argmax=None, gate=None, z=None):
    """Gradients of DAEs.py:193-195 (weighted BCE of the MIXED score, mean over n_batch) w.r.t. the title
    variables only (the DAE constants are frozen, DAEs.py:165-171).  float64.

    argmax / gate [B, n_sizes * F]: the window each feature's gradient goes to and whether its ReLU is open.  Default: the
    float64 forward's own decisions.  The kernels take theirs from the fp32 chain (features_f32_chain, checked bit for
    bit), which may differ on a near-tie between windows or a feature within rounding of 0; passing the chain's decisions
    routes the reference the same way.  The feature is then the float64 convolution at that window (0 where closed).
    z [B, V]: the title logits the loss reads (the kernels' fp32 forward, checked on its own); default f Wo + b in float64.
    With it the backward is checked on the forward values the kernels actually differentiate."""
    x = embed(titles, params["char_embedding"])
    B, L, Ec = x.shape
    n_char = params["char_embedding"].shape[0]
    convs, mag = _convs64(x, params, filter_sizes)
    if argmax is None:
        argmax = np.concatenate([np.maximum(c, 0.0).argmax(axis=1) for c in convs], axis=1)
    arg = np.asarray(argmax, np.int64)
    F = params["Conv_b0"].shape[0]
    pick = np.concatenate([np.take_along_axis(c, arg[:, i * F:(i + 1) * F][:, None, :], axis=1)[:, 0, :]
                           for i, c in enumerate(convs)], axis=1)
    S = np.concatenate([np.take_along_axis(m, arg[:, i * F:(i + 1) * F][:, None, :], axis=1)[:, 0, :]
                        for i, m in enumerate(mag)], axis=1)
    gate = pick > 0.0 if gate is None else np.asarray(gate, bool)
    f0 = np.where(gate, pick, 0.0)
    km = np.ones_like(f0) if keep_mask is None else keep_mask.astype(np.float64)
    f = f0 / keep_prob * km
    Wo = params["Output_W"].astype(np.float64)
    bo = params["Output_b"].astype(np.float64)
    z_given = z is not None
    z = np.asarray(z, np.float64) if z_given else f @ Wo + bo
    st = 1.0 / (1.0 + np.exp(-z))
    wt = np.asarray(w_title, np.float64).reshape(-1, 1); wp = np.asarray(w_playlist, np.float64).reshape(-1, 1)
    dae = np.asarray(dae_score, np.float64)
    yp = st * wt + dae * wp
    eps = 1e-10
    yv = np.asarray(y, np.float64)
    cost = -np.sum(yv * np.log(yp + eps) + 0.55 * (1 - yv) * np.log(1 - yp + eps)) / n_batch
    dyp = -(yv / (yp + eps) - 0.55 * (1 - yv) / (1 - yp + eps)) / n_batch
    dz = dyp * wt * st * (1 - st)
    g = {"Output_W": f.T @ dz, "Output_b": dz.sum(axis=0)}
    dfeat = dz @ Wo.T
    dg = dfeat * km / keep_prob * gate
    Ws = [params["Conv_W%d" % i].astype(np.float64)[:, :, 0, :] for i in range(len(filter_sizes))]
    gWs, gbs, gE = conv_backward(x, titles, Ws, dg, arg, filter_sizes, n_char)
    for i in range(len(filter_sizes)):
        g["Conv_W%d" % i] = gWs[i][:, :, None, :]
        g["Conv_b%d" % i] = gbs[i]
    g["char_embedding"] = gE
    aux = dict(x=x, titles=np.asarray(titles, np.int64), Ws=Ws, Wo=Wo, bo=bo, S=S, f0=f0, f=f, km=km, kp=keep_prob,
               arg=arg, gate=gate, z=z, z_given=z_given, st=st, dfeat=dfeat, yp=yp, y=yv, wt=wt, wp=wp, dae=dae, dz=dz, dg=dg, n_batch=n_batch,
               filter_sizes=list(filter_sizes), n_char=n_char)
    return cost, g, dict(features=f0, argmax=arg, z=z, title_score=st, y_pred=yp, _aux=aux)


def fp32_loss_head(z, dae, y, w_title, w_playlist, n_batch):
    """title_loss_kernel's loss head as fp32 evaluates it, per element, as INTERVALS (the DAE head's treatment,
    oracle/dae_numpy.py fp32_head, same window): where the mixed score yp = st w_t + dae w_p reaches 1 in fp32, 1 - yp is a
    small integer multiple of 2^-24 (0 included), and st (1 - st) cancels the same way; grads()' float64 sees neither, and
    title_grad_bounds' relative terms dyp / a0 grow past 1 there.
        st  in dae_numpy's admissible fp32 sigmoid of z (p and 1 - p as intervals);
        yp  = fl(fl(st w_t) + fl(dae w_p)), within 2 u of the exact mix of an admissible st (three roundings of
              non-negative terms); for yp >= 0.5 it lies on the grid of spacing 2^-24, so q = fl(1 - yp) = m 2^-24 for the
              integers m from floor((1 - yp_hi) / 2^-24) to ceil((1 - yp_lo) / 2^-24), m >= 0 (w_t + w_p <= 1 and both
              scores <= 1 keep yp <= 1); below 0.5, q is within 2^-25 of 1 - yp;
        L   = -[ y ln(yp + 1e-10) + 0.55 (1 - y) ln(q + 1e-10) ]
        dz  = -( y / (yp + 1e-10) - 0.55 (1 - y) / (q + 1e-10) ) w_t st (1 - st) / n_batch
    each factor monotone in its argument, so the ends of the arguments' intervals bound it; the hardware's log / division and
    the remaining fp32 products get 2^-18 relative (as the DAE head) and L 2^-22 (|y| + 0.55 |1 - y|) absolute.  dae, w_t,
    w_p: the fp32 values the kernel reads (no error of their own).  y in [0, 1].
    Returns dict(L_lo, L_hi, dz_lo, dz_hi, zero): allowances included; zero = the mask of elements where q = 0 is admissible."""
    from . import dae_numpy as dn
    u, eps = U32, 1e-10
    z = np.asarray(z, np.float64)
    dae = np.asarray(dae, np.float64)
    y = np.asarray(y, np.float64)
    wt = np.asarray(w_title, np.float64).reshape(-1, 1)
    wp = np.asarray(w_playlist, np.float64).reshape(-1, 1)
    assert ((y >= 0) & (y <= 1)).all() and (wt + wp <= 1.0).all() and (dae <= 1.0).all()
    s_lo, s_hi, c_lo, c_hi, _, _, _ = dn._head_pq(z)                       # st and 1 - st
    yp_lo = (s_lo * wt + dae * wp) * (1 - 2 * u)
    yp_hi = np.minimum((s_hi * wt + dae * wp) * (1 + 2 * u), 1.0)
    grid = yp_lo >= 0.5
    q_lo = np.where(grid, np.maximum(0.0, np.floor((1 - yp_hi) / u)) * u, np.maximum(1 - yp_hi - u / 2, 0.0))
    q_hi = np.where(grid, np.ceil((1 - yp_lo) / u) * u, 1 - yp_lo + u / 2)
    wy = np.abs(y) + 0.55 * np.abs(1 - y)
    L_lo = -(y * np.log(yp_hi + eps) + 0.55 * (1 - y) * np.log(q_hi + eps))
    L_hi = -(y * np.log(yp_lo + eps) + 0.55 * (1 - y) * np.log(q_lo + eps))
    aL = 2.0 ** -18 * np.maximum(np.abs(L_lo), np.abs(L_hi)) + 2.0 ** -22 * wy
    g1_lo, g1_hi = y / (yp_hi + eps), y / (yp_lo + eps)
    g0_lo, g0_hi = 0.55 * (1 - y) / (q_hi + eps), 0.55 * (1 - y) / (q_lo + eps)
    d_lo, d_hi = g1_lo - g0_hi, g1_hi - g0_lo                            # dL/dyp = -(d), d in [d_lo, d_hi]
    S_lo, S_hi = s_lo * c_lo * wt / n_batch, s_hi * c_hi * wt / n_batch       # >= 0
    cands = np.stack([d_lo * S_lo, d_lo * S_hi, d_hi * S_lo, d_hi * S_hi])
    dz_lo, dz_hi = -cands.max(axis=0), -cands.min(axis=0)
    adz = 2.0 ** -18 * np.maximum(np.abs(dz_lo), np.abs(dz_hi)) + 2.0 ** -126   # (below fp32's normal range: denormal or 0)
    return dict(L_lo=L_lo - aL, L_hi=L_hi + aL, dz_lo=dz_lo - adz, dz_hi=dz_hi + adz, zero=grid & (q_lo == 0), yp_lo=yp_lo, yp_hi=yp_hi)


def dae_logit_bounds(h, W_dec, b_dec):
    """Bound on |fp32 DAE logit - exact| for fp32 hidden activations h [B, H] known exactly (the encode kernel equals
    oracle.encode bit for bit): an fp32 sum of H products and the bias, (H + 2) u (sum_k |h W| + |b|)."""
    h = np.abs(np.asarray(h, np.float64))
    H = h.shape[1]
    return (H + 2) * U32 * (h @ np.abs(np.asarray(W_dec, np.float64)).T + np.abs(np.asarray(b_dec, np.float64)))


def grad_h_split(V, H, B, n_cu=256):
    """(chunk, n_chunk) of dae_launch_grad_h (csrc/train.hip) for dfeat = dz Wo^T with H = the feature row length: the V
    vocabulary rows are cut into n_chunk chunks of `chunk` rows, each summed in an accumulator of its own, and
    sum_chunks_kernel adds the n_chunk partials.  n_cu: DAE_NUM_CU (csrc/dae_internal.h)."""
    na = 4 if H % 128 == 0 else (2 if H % 64 == 0 else 1)
    bpad = (B + 63) // 64 * 64
    tiles = (H // (32 * na)) * (bpad // 64)
    want = max(1, (n_cu * 4) // tiles)
    chunk = max(16, (-(-V // want) + 15) // 16 * 16)
    return chunk, -(-V // chunk)


def _feature_logit_errors(a):
    """(ef, ez) of title_grad_bounds: the fp32 features after dropout and the fp32 title logits against grads()' float64."""
    u = U32
    F = a["Ws"][0].shape[2]
    E = a["x"].shape[2]
    ncols = np.concatenate([np.full(F, fs * E) for fs in a["filter_sizes"]])
    ef = (ncols + 2) * u * a["S"] * a["gate"] * a["km"] / a["kp"] + u * np.abs(a["f"])
    Woa = np.abs(a["Wo"])
    ez = (a["f"].shape[1] + 2) * u * (np.abs(a["f"]) @ Woa + np.abs(a["bo"])) + ef @ Woa
    return ef, ez


def title_logit_bounds(info):
    """Bound on |fp32 title logit of a training step - grads()' float64 z| (info from grads() without z=, with the chain's
    argmax and gate): ez of title_grad_bounds."""
    return _feature_logit_errors(info["_aux"])[1]


def title_grad_bounds(info, dae_zerr=0.0, w_rel=0.0, dfeat_split=None):
    """Element-wise bounds |kernel - grads()| for every title gradient, from info = grads(...)[2] computed with the chain's
    argmax and gate.  Keys as grads()' g.

    Derivation (u = 2^-24; a sum of n fp32 terms, any order, any tree, products exact or once rounded, is within
    (n + 2) u sum |terms| of its exact value: Higham 3.1, the + 2 for the product's rounding and 1 / (1 - n u)).
      features   ef0 = (fs E + 2) u S, S = |b| + sum |x W| at the chain's window (feature_bounds); the dropout's
                 (f / kp) * mask adds u |f|:  ef = ef0 mask / kp + u |f|.
      title logit   ez = (D + 2) u (|f| |Wo| + |bo|) + ef |Wo|  (the decoder GEMM over D = n_sizes F features);
                 0 when grads() was given the kernels' own logits (z=).
      DAE score  the caller's logit bound dae_zerr (dae_logit_bounds) moves sigmoid by dae (1 - dae) dae_zerr; the fp32
                 sigmoid adds the same terms as st below.  dae_zerr=None: grads() was given the DAE scores the loss reads
                 (the kernels' own), which carry no error.
      dz         title_loss_kernel:  st = 1 / (1 + __expf(-z)).  __expf is v_exp_f32 (1 ulp) of the fp32 product
                 -z log2(e): relative error 2 u (|z| + 1) of e^-z, twice that for margin; the logit error ez multiplies e^-z
                 by e^ez, relative 1.01 ez for ez < 0.01.  A relative error d of e^-z moves st by st (1 - st) d; the add and
                 the reciprocal add 3 u st:  dst = st (1 - st) (4 u (|z| + 1) + 1.01 ez) + 3 u st.
                 yp = st wt + dae wp:  dyp = wt dst + wp ddae + w_rel (st wt + dae wp) + 3 u yp  (w_rel: the caller's
                 relative bound on the fp32 mixing weights).
                 y = 1: 1 / (yp + 1e-10) is off by dyp / a1 + 2 u (relative); y = 0: 0.55 / (1 - yp + 1e-10) by
                 (dyp + 2 u) / a0 + 3 u (two roundings of 1 - yp + 1e-10, 0.55f, the division).
                 st (1 - st): dst / st + (dst + u) / (1 - st); inv_nb and the four products: 6 u; the weight: w_rel.
                 R = the sum of these relative errors; delta = |dz| R (1 + R) (a product of factors 1 + r_i is within
                 R (1 + R) of 1 for R < 1).
      backward   gOutput_W = f^T dz (B terms):   (B + 2) u fa^T |dz| + fa^T delta + ef^T |dz|,  fa = |f| + ef
                 gOutput_b = sum_b dz:          (B + 2) u sum |dz| + sum delta
                 dfeat = dz Wo^T:               edf = (n + 3) u |dz| |Wo|^T + delta |Wo|^T
                   with dfeat_split = (chunk, n_chunk) (grad_h_split: the kernel's two-level sum, chunks of rows in
                   accumulators of their own, then the partials) n = chunk + n_chunk: each chunk is within (chunk + 1) u
                   of its sum |terms|, the sum of the partials within (n_chunk + 1) u of sum |partials| <= sum |terms|.
                   Without it n = V (any order).
                 dg = dfeat * mask / kp, gated:  edg = gate (edf mask / kp + 2 u |dg|)
                 gconv_b, gconv_W (B terms, fmaf chains): (B + 3) u sum |terms| + the terms of edg.
                 gembedding (title_egrad_kernel): per (row, position) an LDS sum, in any order, of the n1 open features
                 whose window covers the position, each product rounded once; then one global atomicAdd of each nonzero
                 partial into its character's row, n2 of them per character in any order:
                 (max n1 + n2 + 3) u sum |terms| + the terms of edg.
                 The sums of terms are conv_backward() run on |x|, |W| and |dg| + edg (resp. edg).
      cost       a loss term's log is off by its argument's relative error (dyp / a1 + u, resp. (dyp + 2 u) / a0), plus
                 6 u |term| (v_log_f32, the ln 2 product, the two products with y); title_loss_kernel adds each term
                 through at most 14 roundings (4 per thread, a 6-level lane tree, 2 wave levels, inv_nb and its own
                 rounding) and title_cost_kernel sums the block partials in double and rounds once: the terms are >= 0,
                 so sum |terms| / n_batch is the cost itself: 21 u cost.
    Returns {key: bound array}, keys of grads()' g, plus "dfeat" (the bound of dz Wo^T, info["_aux"]["dfeat"]) and
    "cost" (a float)."""
    a = info["_aux"]
    u = U32
    fs_list, E = a["filter_sizes"], a["x"].shape[2]
    F = a["Ws"][0].shape[2]
    B, D = a["f"].shape
    V = a["dz"].shape[1]
    ef, ez_ = _feature_logit_errors(a)
    Woa = np.abs(a["Wo"])
    ez = 0.0 if a["z_given"] else ez_
    st, z, dae, wt, wp, yp, y = a["st"], a["z"], a["dae"], a["wt"], a["wp"], a["yp"], a["y"]
    with np.errstate(divide="ignore"):
        zd = np.log(np.maximum(dae, 1e-300)) - np.log(np.maximum(1.0 - dae, 1e-300))
    ddae = 0.0 if dae_zerr is None else dae * (1 - dae) * (1.01 * np.asarray(dae_zerr) + 4 * u * (np.abs(zd) + 1)) + 3 * u * dae
    dst = st * (1 - st) * (4 * u * (np.abs(z) + 1) + 1.01 * ez) + 3 * u * st
    dyp = wt * dst + wp * ddae + w_rel * (st * wt + dae * wp) + 3 * u * yp
    a1, a0 = yp + 1e-10, 1.0 - yp + 1e-10
    r_term = np.where(y != 0, dyp / a1 + 2 * u, (dyp + 2 * u) / a0 + 3 * u)
    R = r_term + dst / st + (dst + u) / (1 - st) + 6 * u + w_rel
    dza = np.abs(a["dz"])
    delta = dza * R * (1 + R)
    fa = np.abs(a["f"]) + ef
    out = {"Output_W": (B + 2) * u * (fa.T @ dza) + fa.T @ delta + ef.T @ dza,
           "Output_b": (B + 2) * u * dza.sum(axis=0) + delta.sum(axis=0)}
    n_df = V if dfeat_split is None else sum(dfeat_split)
    edf = (n_df + 3) * u * (dza @ Woa.T) + delta @ Woa.T
    dga = np.abs(a["dg"])
    edg = a["gate"] * (edf * a["km"] / a["kp"] + 2 * u * dga)
    out["dfeat"] = edf
    out["cost"] = (np.sum(np.where(y != 0, dyp / a1 + u, 0.55 * (dyp + 2 * u) / a0)) / a["n_batch"]
                   + 21 * u * info_cost(a))
    out.update(_conv_bounds(a, dga, edg))
    return out


def info_cost(a):
    """The cost of grads() from its _aux: sum of the loss terms / n_batch."""
    return float(np.sum(_loss_terms(a)) / a["n_batch"])


def _loss_terms(a):
    y, yp = a["y"], a["yp"]
    return -(y * np.log(yp + 1e-10) + 0.55 * (1 - y) * np.log(1 - yp + 1e-10))


def _conv_bounds(a, dga, edg):
    """Bounds of the conv / embedding gradients from |dg| and the error edg of dg (title_grad_bounds' derivation)."""
    u = U32
    fs_list = a["filter_sizes"]
    F = a["Ws"][0].shape[2]
    B = a["x"].shape[0]
    out = {}
    xa = np.abs(a["x"])
    Wa = [np.abs(W) for W in a["Ws"]]
    gW_t, gb_t, gE_t = conv_backward(xa, a["titles"], Wa, dga + edg, a["arg"], fs_list, a["n_char"])
    gW_e, gb_e, gE_e = conv_backward(xa, a["titles"], Wa, edg, a["arg"], fs_list, a["n_char"])
    # title_egrad_kernel's two levels: n1 terms per (row, position), n2 partials per character
    Bn, L = a["titles"].shape
    n1 = np.zeros((Bn, L))
    bi = np.broadcast_to(np.arange(Bn)[:, None], (Bn, F))
    for i, fs in enumerate(fs_list):
        gi = a["gate"][:, i * F:(i + 1) * F].astype(np.float64)
        for dp in range(fs):
            np.add.at(n1, (bi, a["arg"][:, i * F:(i + 1) * F] + dp), gi)
    ok = (a["titles"] >= 0) & (a["titles"] < a["n_char"]) & (n1 > 0)
    n2 = np.bincount(a["titles"][ok], minlength=a["n_char"]).astype(np.float64)
    n1max = np.zeros(a["n_char"])
    np.maximum.at(n1max, a["titles"][ok], n1[ok])
    for i in range(len(fs_list)):
        out["Conv_W%d" % i] = ((B + 3) * u * gW_t[i] + gW_e[i])[:, :, None, :]
        out["Conv_b%d" % i] = (B + 3) * u * gb_t[i] + gb_e[i]
    out["char_embedding"] = (n1max + n2 + 3)[:, None] * u * gE_t + gE_e
    return out


def conv_grads_from_dfeat(info, dfeat):
    """The conv and embedding gradients from a GIVEN dfeat [B, >= n_feat] (the one the kernels' conv backward reads,
    dae_title_loss_backward's output) and their bounds: then only title_gate/wgrad/egrad_kernel's own rounding is
    bounded -- the gate's (d / kp) * mask (one rounding), the wgrad fmaf chains over the batch, the egrad LDS and global
    atomics (title_grad_bounds' derivation, with edf = 0).  -> (reference {key: float64}, bounds {key: array})."""
    a = info["_aux"]
    nf = a["f"].shape[1]
    d = np.asarray(dfeat, np.float64)[:, :nf]
    dg = d * a["km"] / a["kp"] * a["gate"]
    gWs, gbs, gE = conv_backward(a["x"], a["titles"], a["Ws"], dg, a["arg"], a["filter_sizes"], a["n_char"])
    ref = {"char_embedding": gE}
    for i in range(len(a["filter_sizes"])):
        ref["Conv_W%d" % i] = gWs[i][:, :, None, :]
        ref["Conv_b%d" % i] = gbs[i]
    dga = np.abs(dg)
    return ref, _conv_bounds(a, dga, 2 * U32 * dga)


def grad_check(got, ref, bounds):
    """{key: max |got - ref| / bound} (inf where a non-finite value or a nonzero error meets a zero bound).  Passes when
    every ratio <= 1."""
    out = {}
    for k, r in ref.items():
        g = np.asarray(got[k], np.float64).reshape(np.shape(r))
        err = np.abs(g - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bounds[k])
        q = np.where(np.isfinite(g), q, np.inf)
        out[k] = float(q.max()) if q.size else 0.0
    return out
