"""TEST INFRASTRUCTURE ONLY -- literal dense numpy restatement of models/DAEs.py (reference).

PARITY UNPINNED at the TensorFlow boundary (see oracle/dae_oracle.c header): TensorFlow 1.x is not
available, the reference has no tests/vectors for this path.  This module follows the reference
statement by statement in the reference's own DENSE formulation, and is the yardstick the canonical
C oracle (dae_oracle.c) is checked against within fp32 re-association tolerance.

Citations are relative to /root/reference.
"""
import numpy as np

F = np.float32
U32 = 2.0 ** -24                       # unit roundoff of fp32


def sparse_to_dense(positions, values, n_batch, n_input):
    """DAEs.py:33-35 -- tf.sparse_tensor_to_dense(validate_indices=False): ASSIGNMENT, entries
    applied in order so the LAST duplicate wins (assumption documented there)."""
    x = np.zeros((n_batch, n_input), dtype=F)
    positions = np.asarray(positions, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(values, dtype=F).reshape(-1)
    if values.size == 1 and positions.shape[0] != 1:
        values = np.full(positions.shape[0], values[0], dtype=F)
    for (r, c), v in zip(positions, values):        # in order: last wins
        x[r, c] = v
    return x


def sigmoid(z):
    z = np.asarray(z, dtype=F)
    return (F(1.0) / (F(1.0) + np.exp(-z, dtype=F))).astype(F)


def forward(x, W_enc, b_enc, W_dec, b_dec, input_keep_mask=None, ikp=1.0,
            hidden_keep_mask=None, kp=1.0):
    """DAEs.py:40-42, 64-70, 73-77/141-145.  Masks are 0/1 arrays (None = keep all) standing in
    for floor(keep_prob + uniform)."""
    x = np.asarray(x, dtype=F)
    xd = x / F(ikp)
    if input_keep_mask is not None:
        xd = xd * input_keep_mask.astype(F)
    s = xd.sum(axis=1, keepdims=True, dtype=F)                      # :41
    xh = xd / (s + F(1e-10))                                        # :42
    h = sigmoid(xh @ W_enc + b_enc)                                 # :66-67
    h = h / F(kp)
    if hidden_keep_mask is not None:
        h = h * hidden_keep_mask.astype(F)                          # :68
    logits = h @ W_dec.T + b_dec                                    # :75 / :143
    return xh, h, logits.astype(F)


def loss_from_pred(y, y_pred, n_batch):
    """DAEs.py:98-100 (reg term added by the caller)."""
    y = np.asarray(y, dtype=F)
    L = -np.sum(y * np.log(y_pred + F(1e-10)) +
                F(0.55) * (F(1.0) - y) * np.log(F(1.0) - y_pred + F(1e-10)), axis=1, dtype=F)
    return F(L.sum(dtype=F) / F(n_batch))


def l2_loss(*tensors):
    """DAEs.py:79-82 / :147-150 -- tf.nn.l2_loss(t) = sum(t**2)/2."""
    return F(sum(float(np.sum(np.square(t.astype(np.float64)))) / 2.0 for t in tensors))


# ---- the fp32 loss head (DAEs.py:98-100 as TensorFlow evaluates it, in fp32), rounding-aware -----------------------------
# Specification, per element, z the logit, every operation rounded to fp32:
#     p  = sigmoid(z)                  q  = fl(1 - p)          (exact for p >= 0.5)
#     a1 = fl(p + 1e-10f)              a0 = fl(q + 1e-10f)
#     L  = -[ y ln a1 + 0.55 (1 - y) ln a0 ]
#     dz = -( y / a1 - 0.55 (1 - y) / a0 ) p q / n_batch
# For p >= 0.5 the grid of p has spacing 2^-24, so q = m 2^-24 for an integer m >= 0, and L and dz jump between neighbouring
# m: at m = 0 the negative's gradient is 0 and its loss term -0.55 ln 1e-10 = 12.66, at m = 1 they are 0.5491 / n_batch and
# 9.15.  float64 does not see this (at z = 17 it gives 0.549 / n_batch and 9.35), so the head below returns, per element,
# the INTERVAL of L and of dz over every fp32 value of p that a faithful evaluation of sigmoid may return.
HEAD_W = 3
HEAD_EPS = 1e-10


def head_window(z):
    """How far a faithful fp32 sigmoid may lie from the exact one, in units of 2^-24: absolute for z >= 0 (p >= 0.5, where
    2^-24 is the spacing of p), relative to p for z < 0.

    Derivation, for the sequence the kernels run (arg = fl(-1.44269504f z); e = v_exp_f32(arg); s = fl(1 + e);
    p = v_rcp_f32(s)); AMD documents v_exp_f32 and v_rcp_f32 as accurate to 1 ulp, read here the cautious way: the correctly
    rounded result moved by up to one ulp, 1.5 ulp from the true value, and an ulp is at most 2^-23 relative, so 3 units.
      * the product rounds to fp32: |arg| 2^-24 absolute in the exponent, and the constant 1.44269504f is 0.224 2^-24 below
        log2(e) relatively; together ln2 |arg| 1.224 2^-24 = 1.224 |z| 2^-24 relative in e;
      * v_exp_f32: 3 units relative in e;
      * s = fl(1 + e): half a spacing of s, at most 2^-24 relative (1 unit); for z >= 0, s is in [1, 2] and that is 2^-24
        absolute;
      * v_rcp_f32: 1.5 ulp of p: 3 units relative, or 1.5 units absolute where p is in [0.5, 1).
    z < 0:  e > 1 and ds / s <= de / e, so dp / p <= (1.224 |z| + 3) + 1 + 3 = 1.224 |z| + 7 units.
    z >= 0: dp = ds / s^2 + rcp's, ds = e (1.224 z + 3) 2^-24 + 2^-24, e = exp(-z):
            dp <= [ e (1.224 z + 3) + 1 ] / (1 + e)^2 + 1.5 units, whose maximum over z >= 0 is 2.90 (at z = 1.4), and 2.5 as
            z -> inf.  One corner lies above that: where s rounds to exactly 1 (e < 2^-24, z > 16.64; under 1 unit) a
            reciprocal moved UP one ulp is 1 + 2^-23, 2 units off, under 3 in all.  m is an integer, so HEAD_W = 3 is the
            window: |m - m64| <= 3 (p above 1 would give q < 0; the window keeps m >= 0, and v_rcp_f32(1.0) is 1.0).
    An emulation in numpy float32 of the four operations, v_exp and v_rcp each the correctly rounded value moved by -1 / 0 /
    +1 ulp, z from -100 to 110, stays inside both: 2.9985 units at z = 16.637, 0.93 of the relative window below 0
    (tests/test_train_saturated_reference_cpu.py runs it).
    Returns (W_abs for z >= 0, r_rel for z < 0), arrays shaped as z."""
    z = np.asarray(z, np.float64)
    return np.full(z.shape, float(HEAD_W)), 1.224 * np.abs(z) + 7.0


def _head_pq(z, z_err=0.0, W=None):
    """The admissible fp32 (p, q = 1 - p) of a float64 logit z, as intervals: (p_lo, p_hi, q_lo, q_hi, m_lo, m_hi, m64).
    z >= 0: q = m 2^-24 for the integers m with m >= 0 and |m - m64| <= W + m64 p z_err (z_err: the bound on the kernel's
    own logit error, which moves q by p q z_err); m_lo / m_hi / m64 are nan for z < 0.
    z < 0:  p within p64 (1 +- (r 2^-24 + q z_err)); below fp32's smallest normal number p may also be flushed to 0 (and
    v_exp_f32 overflows to inf from arg = 128 on, z < -88.7, which gives p = 0 too)."""
    z = np.asarray(z, np.float64)
    Wa, r = head_window(z)
    if W is not None:
        Wa = np.full(z.shape, float(W))
    with np.errstate(over="ignore"):
        ez = np.exp(-np.abs(z))
    small = ez / (1.0 + ez)                                   # sigmoid(-|z|): q64 for z >= 0, p64 for z < 0
    pos = z >= 0
    m64 = small / U32
    win = Wa + m64 * (1.0 - small) * z_err               # dq = p q dz
    m_lo = np.maximum(0.0, np.ceil(m64 - win))
    m_hi = np.floor(m64 + win)
    rel = r * U32 + (1.0 - small) * z_err                # dp = p q dz
    s_lo = small * (1.0 - rel)
    s_lo = np.where(s_lo < 2.0 ** -126, 0.0, np.maximum(s_lo, 0.0))
    s_hi = small * (1.0 + rel)
    q_lo = np.where(pos, m_lo * U32, 1.0 - s_hi)
    q_hi = np.where(pos, m_hi * U32, 1.0 - s_lo)
    p_lo = np.where(pos, 1.0 - m_hi * U32, s_lo)
    p_hi = np.where(pos, 1.0 - m_lo * U32, s_hi)
    nan = np.full(z.shape, np.nan)
    return p_lo, p_hi, q_lo, q_hi, np.where(pos, m_lo, nan), np.where(pos, m_hi, nan), np.where(pos, m64, nan)


def _head_terms(p_lo, p_hi, q_lo, q_hi, y, n_batch):
    """Intervals of the loss term and of dz over p in [p_lo, p_hi], q in [q_lo, q_hi], in float64.  Every factor is monotone
    (ln(q + eps), ln(p + eps), p, q, q / (q + eps), p / (p + eps)) and non-negative where it multiplies, so the ends of each
    factor's interval bound the product; the y and the 1 - y part are bounded separately and added."""
    eps = HEAD_EPS
    c1, c0 = y, 0.55 * (1.0 - y)
    a, b = -c1 * np.log(p_lo + eps), -c1 * np.log(p_hi + eps)
    c, d = -c0 * np.log(q_lo + eps), -c0 * np.log(q_hi + eps)
    L_lo = np.minimum(a, b) + np.minimum(c, d)
    L_hi = np.maximum(a, b) + np.maximum(c, d)
    a, b = -c1 * (p_lo / (p_lo + eps)) * q_lo / n_batch, -c1 * (p_hi / (p_hi + eps)) * q_hi / n_batch
    c, d = c0 * p_lo * (q_lo / (q_lo + eps)) / n_batch, c0 * p_hi * (q_hi / (q_hi + eps)) / n_batch
    d_lo = np.minimum(a, b) + np.minimum(c, d)
    d_hi = np.maximum(a, b) + np.maximum(c, d)
    return L_lo, L_hi, d_lo, d_hi


def fp32_head(z, y, n_batch, z_err=0.0, W=None):
    """The loss head per element as fp32 evaluates it (see the specification above), from the float64 logit z and target y.
    Returns a dict of arrays shaped as z:
      L_lo, L_hi, dz_lo, dz_hi   the interval of the loss term and of dz over the admissible p (head_window), before the
                                 hardware log / rcp allowance (head_allowance adds it);
      L, dz                      the central value: the float64 one (grads()' own expression, bit for bit) wherever m = 0 is
                                 not admissible; where it is (q may be exactly 0: the fp32 gradient may vanish, which float64
                                 never shows) the middle of the interval;
      zero                       the mask of those elements; m_lo, m_hi, m64 (nan for z < 0); q64 = 1 - p in float64.
    A scalar W overrides the derived window (the tests use it to show what a narrower one would miss)."""
    z = np.asarray(z, np.float64)
    y = np.broadcast_to(np.asarray(y, np.float64), z.shape)
    eps = HEAD_EPS
    p_lo, p_hi, q_lo, q_hi, m_lo, m_hi, m64 = _head_pq(z, z_err, W)
    L_lo, L_hi, d_lo, d_hi = _head_terms(p_lo, p_hi, q_lo, q_hi, y, n_batch)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
        q64 = np.where(z >= 0, np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))), 1.0 - p)
    L = -(y * np.log(p + eps) + 0.55 * (1 - y) * np.log(1 - p + eps))
    dz = -(y / (p + eps) - 0.55 * (1 - y) / (1 - p + eps)) * p * (1 - p) / n_batch
    zero = m_lo == 0
    L = np.where(zero, 0.5 * (L_lo + L_hi), L)
    dz = np.where(zero, 0.5 * (d_lo + d_hi), dz)
    return dict(L=L, dz=dz, L_lo=L_lo, L_hi=L_hi, dz_lo=d_lo, dz_hi=d_hi, zero=zero, m_lo=m_lo, m_hi=m_hi, m64=m64, q64=q64)


def head_candidates(z, y, n_batch, z_err=0.0, W=None):
    """For one element with z >= 0: the list of (m, L, dz) at every admissible integer m (q = m 2^-24 exactly): the discrete
    values a faithful fp32 evaluation can return, which a result has to be ONE of where m = 0 is among them."""
    _, _, _, _, m_lo, m_hi, _ = _head_pq(np.float64(z), z_err, W)
    out = []
    for m in range(int(m_lo), int(m_hi) + 1):
        q = np.float64(m) * U32
        L_lo, _, d_lo, _ = _head_terms(1.0 - q, 1.0 - q, q, q, np.float64(y), n_batch)
        out.append((m, float(L_lo), float(d_lo)))
    return out


def head_allowance(hd, y, n_batch):
    """What the hardware log / rcp and the fp32 roundings after p add to fp32_head's intervals: (aL, adz), per element.
    dz: 2^-18 |dz| (bf16_bounds' figure: v_rcp_f32, four or five fp32 products) plus bf16_bounds' absolute 2^-21 wy / n_batch
    for a target, plus 2^-126 (a result below fp32's normal range is rounded on the denormal grid or flushed to 0).
    L: 2^-18 |L| (v_log_f32 is 1 ulp of log2's value; a1, a0 round once) plus 2^-22 wy absolute (q = fl(1 - p)
    rounds by 2^-25 where p < 0.5, and log2 near 1 keeps no relative precision); wy = |y| + 0.55 |1 - y|."""
    y = np.asarray(y, np.float64)
    wy = np.abs(y) + 0.55 * np.abs(1 - y)
    aL = 2.0 ** -18 * np.maximum(np.abs(hd["L_lo"]), np.abs(hd["L_hi"])) + 2.0 ** -22 * wy
    adz = 2.0 ** -18 * np.maximum(np.abs(hd["dz_lo"]), np.abs(hd["dz_hi"])) + 2.0 ** -21 * wy * (y != 0) / n_batch + 2.0 ** -126
    return aL, adz


def grads(x, y, W_enc, b_enc, W_dec, b_dec, n_batch, tied, reg_lambda=0.0,
          input_keep_mask=None, ikp=1.0, hidden_keep_mask=None, kp=1.0, head="f64"):
    """Hand-derived gradient of DAEs.py:98-100 cost w.r.t. d_params (float64 internally so it is
    a trustworthy reference for the fp32 GPU kernels).  head="fp32": the loss term and dz of each element come from
    fp32_head (its central values: the same numbers bit for bit unless some logit is so large that fp32's 1 - p may be
    exactly 0); the result then carries "_head", fp32_head's dict.  grads_f32 is the form with bounds."""
    D = np.float64
    x = np.asarray(x, D); y = np.asarray(y, D)
    We = W_enc.astype(D); be = b_enc.astype(D); Wd = W_dec.astype(D); bd = b_dec.astype(D)
    xd = x / ikp
    if input_keep_mask is not None:
        xd = xd * input_keep_mask
    s = xd.sum(axis=1, keepdims=True)
    xh = xd / (s + 1e-10)
    pre = xh @ We + be
    sg = 1.0 / (1.0 + np.exp(-pre))
    hm = np.ones_like(sg) if hidden_keep_mask is None else hidden_keep_mask.astype(D)
    h = sg / kp * hm
    z = h @ Wd.T + bd
    p = 1.0 / (1.0 + np.exp(-z))
    eps = 1e-10
    L = -np.sum(y * np.log(p + eps) + 0.55 * (1 - y) * np.log(1 - p + eps), axis=1)
    dLdp = -(y / (p + eps) - 0.55 * (1 - y) / (1 - p + eps))
    dz = dLdp * p * (1 - p) / n_batch
    hd = None
    if head == "fp32":
        hd = fp32_head(z, y, n_batch)
        if hd["zero"].any():
            L = -np.sum(np.where(hd["zero"], -hd["L"], y * np.log(p + eps) + 0.55 * (1 - y) * np.log(1 - p + eps)), axis=1)
            dz = np.where(hd["zero"], hd["dz"], dz)
    else:
        assert head == "f64", head
    cost = L.sum() / n_batch
    gWd = dz.T @ h
    gbd = dz.sum(axis=0)
    dh = dz @ Wd
    dpre = dh * hm / kp * sg * (1 - sg)
    gWe = xh.T @ dpre
    gbe = dpre.sum(axis=0)
    if tied:
        gWe = gWe + gWd
        gWd = None
        cost += reg_lambda * 0.5 * ((We ** 2).sum() + (bd ** 2).sum() + (be ** 2).sum())
        gWe = gWe + reg_lambda * We
    else:
        cost += reg_lambda * 0.5 * ((We ** 2).sum() + (bd ** 2).sum() + (be ** 2).sum()
                                    + (Wd ** 2).sum())
        gWe = gWe + reg_lambda * We
        gWd = gWd + reg_lambda * Wd
    gbd = gbd + reg_lambda * bd
    gbe = gbe + reg_lambda * be
    out = dict(cost=cost, gW_enc=gWe, gb_enc=gbe, gW_dec=gWd, gb_dec=gbd, y_pred=p, h=h)
    if hd is not None:
        out["_head"] = hd
    return out


def adam_tf(p, m, v, g, lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer (DAEs.py:102) as TF1's ApplyAdam functor computes it, all in fp32
    (epsilon OUTSIDE the bias correction, dense update):
        alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)      (beta powers = fp32 running products)
        m += (g - m) * (1 - beta1);  v += (g*g - v) * (1 - beta2);  p -= (m * alpha) / (sqrt(v) + eps)
    Returns new (p, m, v)."""
    p = p.astype(F); m = m.astype(F); v = v.astype(F); g = g.astype(F)
    b1, b2 = F(beta1), F(beta2)
    b1p, b2p = F(1.0), F(1.0)
    for _ in range(int(t)):
        b1p = F(b1p * b1); b2p = F(b2p * b2)
    alpha = F(F(lr) * np.sqrt(F(1.0) - b2p, dtype=F) / (F(1.0) - b1p))
    m = (m + (g - m) * (F(1.0) - b1)).astype(F)
    v = (v + (g * g - v) * (F(1.0) - b2)).astype(F)
    p = (p - (m * alpha) / (np.sqrt(v, dtype=F) + F(eps))).astype(F)
    return p, m, v


def cand_generate(scores, seed, k=500):
    """main_challenge.py:28-36 / metrics.py:59-68, literally (slow: list.remove)."""
    cand = np.argsort(-1 * scores)
    cand = cand.tolist()
    for i in seed:
        try:
            cand.remove(i)
        except ValueError:
            pass
    return cand[:k]


def topk_valid_under_reference_rule(scores_row, seed, picked, k=500):
    """Set-parity check (SURVEY finding 5): `picked` is a valid reference answer iff it contains no
    seed, has min(k, available) entries, and every picked score >= every non-picked non-seed
    score.  Returns (ok, boundary_tie) where boundary_tie says the k-th and (k+1)-th scores tie
    (then several sets are equally valid under numpy's unspecified tie order)."""
    n = scores_row.shape[0]
    seedset = set(int(s) for s in seed if 0 <= int(s) < n)
    picked = [int(p) for p in picked if p >= 0]
    avail = n - len(seedset)
    if len(picked) != min(k, avail) or len(set(picked)) != len(picked):
        return False, False
    if seedset & set(picked):
        return False, False
    mask = np.ones(n, dtype=bool)
    mask[list(seedset)] = False
    mask[picked] = False
    lo_picked = scores_row[picked].min() if picked else np.inf
    hi_rest = scores_row[mask].max() if mask.any() else -np.inf
    return bool(lo_picked >= hi_rest), bool(lo_picked == hi_rest)


class NumpyTrainStages:
    """TEST INFRASTRUCTURE: float64 restatement of the three stages of the vocabulary-sharded
    training step (include/dae_hip.h dae_train_shard_*), dense formulation, keep
    probabilities 1.0 only.  Stands in for the device kernels in the gloo tests of
    sharding.ShardedTrainer and is the yardstick of the GPU stage tests.  Tensors are torch CPU
    tensors (written in place), matching HipTrainStages' call signature."""

    def __init__(self, V):
        self.V = V

    def _xhat(self, x, B):
        rp, col, val = (np.asarray(t) for t in x)
        xd = np.zeros((B, self.V), np.float64)
        for r in range(B):
            xd[r, col[rp[r]:rp[r + 1]]] = val[rp[r]:rp[r + 1]]
        return xd / (xd.sum(axis=1, keepdims=True) + 1e-10)                   # DAEs.py:41-42

    def encode(self, x, W_enc, lo, hi, ikp, seed, pre):
        assert ikp == 1.0
        xh = self._xhat(x, pre.shape[0])
        pre.copy_(_t(xh[:, lo:hi] @ W_enc.numpy().astype(np.float64)))        # DAEs.py:66

    def decode(self, pre, b_enc, y, W_enc, W_dec, b_dec, lo, hi, n_batch, tied, kp, seed, lam,
               gW_out, gb_dec, dh, cost):
        assert kp == 1.0
        D = np.float64
        B = pre.shape[0]
        Wd = (W_enc if tied else W_dec).numpy().astype(D)
        sg = 1.0 / (1.0 + np.exp(-(pre.numpy().astype(D) + b_enc.numpy().astype(D))))   # :67
        rp, col, val = (np.asarray(t) for t in y)
        yd = np.zeros((B, self.V), D)
        for r in range(B):
            yd[r, col[rp[r]:rp[r + 1]]] = val[rp[r]:rp[r + 1]]
        yd = yd[:, lo:hi]
        p = 1.0 / (1.0 + np.exp(-(sg @ Wd.T + b_dec.numpy().astype(D))))               # :75 / :143
        L = -np.sum(yd * np.log(p + 1e-10) + 0.55 * (1 - yd) * np.log(1 - p + 1e-10))   # :98-99
        dz = -(yd / (p + 1e-10) - 0.55 * (1 - yd) / (1 - p + 1e-10)) * p * (1 - p) / n_batch
        l2 = 0.5 * ((W_enc.numpy().astype(D) ** 2).sum() + (b_dec.numpy().astype(D) ** 2).sum())
        if lo == 0:
            l2 += 0.5 * (b_enc.numpy().astype(D) ** 2).sum()
        if not tied:
            l2 += 0.5 * (Wd ** 2).sum()
        cost.copy_(_t(np.array([L / n_batch + lam * l2])))
        gW_out.copy_(_t(dz.T @ sg))
        gb_dec.copy_(_t(dz.sum(axis=0)))
        dh.copy_(_t(dz @ Wd))
        self._sg = sg

    def finish(self, dh, x, W_enc, b_enc, W_dec, b_dec, lo, hi, tied, ikp, kp, seed, lam,
               gW_enc, gb_enc, gW_dec, gb_dec):
        D = np.float64
        sg = self._sg
        dpre = dh.numpy().astype(D) * sg * (1 - sg)
        gb_enc.copy_(_t(dpre.sum(axis=0) + lam * b_enc.numpy().astype(D)))
        ge = self._xhat(x, dh.shape[0])[:, lo:hi].T @ dpre
        if tied:
            ge = ge + gW_enc.numpy().astype(D)
        gW_enc.copy_(_t(ge + lam * W_enc.numpy().astype(D)))
        if not tied:
            gW_dec.copy_(_t(gW_dec.numpy().astype(D) + lam * W_dec.numpy().astype(D)))
        gb_dec.copy_(_t(gb_dec.numpy().astype(D) + lam * b_dec.numpy().astype(D)))

    def adam(self, p, m, v, g, lr, t):
        p2, m2, v2 = adam_tf(p.numpy(), m.numpy(), v.numpy(), g.numpy(), lr, t)
        p.copy_(_t(p2)); m.copy_(_t(m2)); v.copy_(_t(v2))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


# ---- bf16 training step (dae_set_train_dtype(BF16)): float64 arithmetic, bf16 rounding where the kernels round ----------

def bf16_round(a):
    """Nearest bf16 value, ties to even.  float32 input: the bit form of train.hip bf16_value / pk_bf16 (v_cvt_pk_bf16_f32),
    returned as float32.  float64 (any other) input: rounded once, directly from the float64 value (no double rounding
    through fp32), returned as float64; subnormals on bf16's grid (spacing 2^-133)."""
    a = np.asarray(a)
    if a.dtype == np.float32:
        u = a.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32)
    x = a.astype(np.float64)
    e = np.maximum(np.frexp(x)[1], -125) - 8                       # bf16 keeps 8 significant bits
    return np.ldexp(np.round(np.ldexp(x, -e)), e)                   # (np.round: half to even)


def bf16_ulp(x):
    """Spacing of the bf16 grid at |x| (float64): the gap between the two bf16 neighbours of x."""
    return np.ldexp(1.0, np.maximum(np.frexp(np.abs(np.asarray(x, np.float64)))[1], -125) - 8)


def grads_bf16(x, y, W_enc, b_enc, W_dec, b_dec, n_batch, tied, reg_lambda=0.0,
               input_keep_mask=None, ikp=1.0, hidden_keep_mask=None, kp=1.0,
               h=None, round_dz=None, round_ops=True, head="f64"):
    """Gradient of the training step under dae_set_train_dtype(BF16), as the kernels round it: float64 everywhere except
    where the kernels round an operand to bf16 (spotify_recsys_challenge_2018_amd/csrc):

      forward logits   z = bf16(h) . bf16(W_dec)^T + b_dec, for the negatives (K5: prepack.hip's prepack / pack_h kernels
                       for decode_generic.hip's EPI_LOSS; decode_f32.hip decode_loss_dh_bf16_kernel's K5D_FRAG and
                       K5D_STAGE round both operands with dae_bf16_rne / v_cvt_pk_bf16_f32, RNE) and for the positives
                       alike (train.hip loss_fixup_kernel<BF16>: dae_bf16_value on h and on W, an fmaf chain from +0,
                       then + bias).
      H % 128 == 0     dz is stored as bf16 (loss_fixup_kernel<.., DZ16>: pk_bf16(dzv, 0); the K5 epilogues: p.dz16 in
                       decode_generic.hip's EPI_LOSS, the packed pairs pk[] of decode_loss_dh_bf16_kernel), and
                       gW_dec = dz^T h (grad_wdec_t_kernel: pk_bf16x8 of h, the bf16 dz^T read as is), dh = dz W_dec
                       (grad_hidden_kernel<4, true, true>, or the fused K5 + K7 plus the fix-up's correction sum
                       (bf16(dz) - bf16(dz as a negative)) bf16(W), loss_fixup_kernel<.., CORR>) run on bf16(dz), bf16(h),
                       bf16(W_dec).  gb_dec sums the bf16 dz: grad_wdec_t_kernel forms it as an MFMA of the bf16 dz^T
                       with a ones operand.
      H % 128 != 0     only the forward GEMM is bf16: the backward GEMMs (grad_wdec_kernel<2|1>, grad_hidden_kernel<2|1>)
                       are fp32 on the unrounded dz, h and W_dec, and so is gb_dec.
      everything else  loss, dpre, the encoder gradient and l2 are fp32 in the kernels, float64 here.

    h: the fp32 hidden activations after dropout, [B, H].  Pass oracle.encode(..., ikp, kp, seed): the training step's K1
    is dae_launch_encode, which tests/test_gpu_parity.py::test_encode_dropout_bit_exact pins bit for bit to orc_encode
    (same fmaf chain per hidden unit in entry order, same sigmoid, the dropout as (x / kp) * floor(kp + u)), so bf16(h) has
    no ambiguity.  None: h = the float64 activation (then nothing is bit-exact, for CPU-only use).
    round_dz: store dz as bf16 (default: H % 128 == 0); round_ops=False leaves h and W_dec unrounded in every GEMM --
    with round_dz=False that is grads() itself.  The masks and keep probabilities are grads()'.
    head="fp32": the loss term and dz of each element from fp32_head, as in grads(); bf16_bounds then folds the head's
    intervals into its delta and cost_interval gives the interval of the cost.
    Returns grads()' keys plus "_aux" (the intermediates bf16_bounds / bf16_backward need)."""
    D = np.float64
    x = np.asarray(x, D); y = np.asarray(y, D)
    We = W_enc.astype(D); be = b_enc.astype(D); bd = b_dec.astype(D)
    Wd32 = np.asarray(W_enc if tied else W_dec, np.float32)
    H = We.shape[1]
    xd = x / ikp
    if input_keep_mask is not None:
        xd = xd * input_keep_mask
    xh = xd / (xd.sum(axis=1, keepdims=True) + 1e-10)
    sg = 1.0 / (1.0 + np.exp(-(xh @ We + be)))
    m = (np.ones_like(sg) if hidden_keep_mask is None else hidden_keep_mask.astype(D)) / kp
    h64 = sg * m if h is None else np.asarray(h, np.float32).astype(D)
    Wd = Wd32.astype(D)
    if round_ops:
        hb = bf16_round(h64) if h is None else bf16_round(np.asarray(h, np.float32)).astype(D)
        Wb = bf16_round(Wd32).astype(D)
    else:
        hb, Wb = h64, Wd
    if round_dz is None:
        round_dz = (H % 128) == 0
    z = hb @ Wb.T + bd
    p = 1.0 / (1.0 + np.exp(-z))
    eps = 1e-10
    L = -np.sum(y * np.log(p + eps) + 0.55 * (1 - y) * np.log(1 - p + eps), axis=1)
    dz = -(y / (p + eps) - 0.55 * (1 - y) / (1 - p + eps)) * p * (1 - p) / n_batch
    assert head in ("f64", "fp32"), head
    if head == "fp32":
        hd = fp32_head(z, y, n_batch)
        if hd["zero"].any():
            L = -np.sum(np.where(hd["zero"], -hd["L"], y * np.log(p + eps) + 0.55 * (1 - y) * np.log(1 - p + eps)), axis=1)
            dz = np.where(hd["zero"], hd["dz"], dz)
    cost = L.sum() / n_batch
    aux = dict(head=head, x=x, y=y, xh=xh, sg=sg, m=m, h=h64, hb=hb, W=Wd, Wb=Wb, bd=bd, We=We, be=be, Wd_own=W_dec.astype(D),
               z=z, p=p, dz=dz, dz16=bool(round_dz), bwd16=bool(round_dz) and round_ops, n_batch=n_batch, tied=tied,
               lam=reg_lambda)
    r = bf16_backward(aux, dz)
    l2 = (We ** 2).sum() + (bd ** 2).sum() + (be ** 2).sum() + (0.0 if tied else (W_dec.astype(D) ** 2).sum())
    r.update(cost=cost + reg_lambda * 0.5 * l2, y_pred=p, h=h64, _aux=aux)
    return r


def grads_f32(x, y, W_enc, b_enc, W_dec, b_dec, n_batch, tied, h=None, **kw):
    """The fp32 training step with the fp32 head, in the form f32_bounds takes: grads_bf16 with nothing rounded to bf16
    (that is grads(head="fp32"), plus "_aux").  h: as in grads_bf16 (the fp32 step's K1 is the same bit-exact launch)."""
    return grads_bf16(x, y, W_enc, b_enc, W_dec, b_dec, n_batch, tied, h=h, round_dz=False, round_ops=False, head="fp32", **kw)


def f32_bounds(ref, c=2.0, h_rel=0.0):
    """bf16_bounds for ref = grads_f32(): no operand is rounded to bf16, so what remains is the fp32 logit error, the head's
    intervals and the fp32 summations."""
    assert not ref["_aux"]["dz16"] and ref["_aux"]["head"] == "fp32"
    return bf16_bounds(ref, c=c, h_rel=h_rel)


def cost_interval(ref, bounds, summation=True):
    """[lo, hi] for the cost of ref = grads_bf16(head="fp32") / grads_f32(): the sums of the head's per-element intervals
    (bounds["L_lo"], bounds["L_hi"]: with the logit error and the hardware allowance in them) over n_batch, widened by the
    fp32 summation term (n + 2) u sum|terms| (n = B V terms, any order), plus the l2 term (float64 partials in the kernels:
    2^-20 relative is generous).  summation=False: the head's part alone (what the saturated elements make uncertain)."""
    a = ref["_aux"]
    nb, lam = a["n_batch"], a["lam"]
    n = bounds["L_lo"].size
    tot = np.maximum(np.abs(bounds["L_lo"]), np.abs(bounds["L_hi"])).sum()
    l2 = (a["We"] ** 2).sum() + (a["bd"] ** 2).sum() + (a["be"] ** 2).sum() + (0.0 if a["tied"] else (a["Wd_own"] ** 2).sum())
    reg = lam * 0.5 * l2
    w = ((n + 2) * U32 * tot / nb + 2.0 ** -20 * reg) if summation else 0.0
    return bounds["L_lo"].sum() / nb + reg - w, bounds["L_hi"].sum() / nb + reg + w


def bf16_backward(aux, dz, rounded=False):
    """The backward half of grads_bf16 from a given dz [B, V] (float64): bf16(dz) when the step stores it so (rounded=True:
    dz is already on the bf16 grid), then gW_dec, gb_dec, dh, dpre, the encoder gradient and the lambda terms."""
    a = aux
    if a["dz16"]:
        dzb = dz if rounded else bf16_round(dz)
        hB, WB = (a["hb"], a["Wb"]) if a["bwd16"] else (a["h"], a["W"])
    else:
        dzb, hB, WB = dz, a["h"], a["W"]
    lam = a["lam"]
    gWd = dzb.T @ hB
    gbd = dzb.sum(axis=0) + lam * a["bd"]
    dh = dzb @ WB
    dpre = dh * a["m"] * a["sg"] * (1 - a["sg"])
    gWe = a["xh"].T @ dpre + lam * a["We"]
    gbe = dpre.sum(axis=0) + lam * a["be"]
    if a["tied"]:
        gWe = gWe + gWd
        gWd = None
    else:
        gWd = gWd + lam * a["Wd_own"]
    return dict(gW_enc=gWe, gb_enc=gbe, gW_dec=gWd, gb_dec=gbd, dh=dh, dzb=dzb)


def bf16_bounds(ref, c=2.0, h_rel=0.0):
    """Element-wise bounds |kernel - grads_bf16| <= bound for gW_dec, gb_dec, gW_enc, gb_enc (and dh), from ref = grads_bf16().

    Derivation.  A sum of n fp32 terms (any order, any tree, products exact or once rounded) is off its exact value by at
    most (n + 2) u sum|terms|, u = 2^-24; c (2) leaves room for the fused launch, whose dh is the negatives' sum plus the
    fix-up's correction (sum|terms| up to twice the exact one).  Products of two bf16 values are exact in fp32.
    The rest is dz.  The kernel's fp32 dz differs from the float64 dz by at most
        delta = p(1-p)(|y| + 0.55|1-y|)/n_batch * dz_err   (d dz / d z times the logit error)
              + 2^-18 |dz|                                  (hardware exp2 / log / rcp, a few ulp each, with margin)
              + 2^-21 (|y| + 0.55|1-y|)/n_batch  [y != 0]   (absolute: 1 - p of a positive with p -> 1 keeps no
                                                             relative precision in fp32)
        dz_err = (H + 2) u (sum_k |bf16(h_k) bf16(w_k)| + |b|)  (the fp32 logit: H exact products, H adds, the bias)
    With ref = grads_bf16(head="fp32") the head's interval joins in: fp32_head is evaluated with z_err = dz_err, and an
    element whose interval reaches further from the central dz than the delta above (dev = max(hi - dz, dz - lo) > delta)
    takes dev plus the hardware allowance on the interval's ends (head_allowance) as its delta instead.  Nothing changes for an
    element whose interval is narrower, so at the logits of an untrained model the bounds are the same numbers as before.
    With dz stored as bf16 (H % 128 == 0) the two agree after rounding except where the float64 dz lies within delta of a
    rounding midpoint: those "ambiguous" elements may land one bf16 ulp apart, so each contributes ulp_bf16(dz) times
    |the other operand| to its sums.  Without the bf16 store every element contributes delta times |the other operand|.
        gW_dec[v,k] <= c (B+2) u sum_r |dz h| + sum_r A[r,v] |h[r,k]|      gb_dec[v] <= c (B+2) u sum_r |dz| + sum_r A[r,v]
        dh[r,k]     <= c (V+2) u sum_v |dz W| + sum_v A[r,v] |W[v,k]|
    dpre = dh m s(1-s) inherits dh's bound times |m s(1-s)|, plus 4u |dh m| (fp32 sigmoid's 1 - s is absolute) and 8u |dpre|;
    gW_enc and gb_enc sum it over the batch: sum_r |xhat| bound(dpre) + c (B+2) u sum|terms| (tied: plus gW_dec's bound).
    Lambda terms: 4u (|g| + lam |param|).  h_rel > 0 (the sharded stages, whose h comes from an all-reduced pre and is not
    bit-exact): h elements within h_rel |h| of a bf16 midpoint may round either way, adding ulp_bf16(h) |W| to the logit
    error and ulp_bf16(h) |dz| to gW_dec.
    Returns dict of bound arrays (keys as grads(), plus "dh") and "amb", the ambiguous-dz mask; with the fp32 head also the
    per-element intervals L_lo / L_hi / dz_lo / dz_hi (allowances included), "zero" (m = 0 admissible) and "wide"."""
    a = ref["_aux"]
    u = U32
    D = np.float64
    B, H = a["h"].shape
    V = a["W"].shape[0]
    nb = a["n_batch"]
    y, p, dz = a["y"], a["p"], a["dz"]
    hB = a["hb"] if a["bwd16"] else a["h"]
    WB = a["Wb"] if a["bwd16"] else a["W"]
    habs = np.abs(a["hb"])
    zerr = (H + 2) * u * (habs @ np.abs(a["Wb"]).T + np.abs(a["bd"]))
    hA = np.zeros_like(habs)
    if h_rel > 0:
        hh = a["h"]
        hamb = bf16_round(hh * (1 - h_rel)) != bf16_round(hh * (1 + h_rel))
        hA = hamb * bf16_ulp(hh)
        zerr = zerr + hA @ np.abs(a["Wb"]).T
    wy = np.abs(y) + 0.55 * np.abs(1 - y)
    delta = p * (1 - p) * wy / nb * zerr + 2.0 ** -18 * np.abs(dz) + 2.0 ** -21 * wy * (y != 0) / nb
    extra = {}
    wide = np.zeros(dz.shape, bool)
    if a.get("head") == "fp32":
        hd = fp32_head(a["z"], y, nb, z_err=zerr)
        aL, adz = head_allowance(hd, y, nb)
        dev = np.maximum(hd["dz_hi"] - dz, dz - hd["dz_lo"])
        wide = dev > delta
        delta = np.where(wide, dev + adz, delta)
        extra = dict(L_lo=hd["L_lo"] - aL, L_hi=hd["L_hi"] + aL, dz_lo=hd["dz_lo"] - adz, dz_hi=hd["dz_hi"] + adz,
                     zero=hd["zero"], wide=wide, q64=hd["q64"], z_err=zerr)
    if a["dz16"]:
        amb = bf16_round(dz - delta) != bf16_round(dz + delta)
        A = amb * bf16_ulp(dz)
        far = wide | (delta > 0.5 * bf16_ulp(dz))      # delta is not small against the bf16 step (a wide interval, or a dz
        if far.any():                                  # near 0 under an absolute term): it may land several steps away
            dzr = bf16_round(dz)
            A = np.where(far, np.maximum(bf16_round(dz + delta) - dzr, dzr - bf16_round(dz - delta)), A)
    else:
        amb = np.zeros(dz.shape, bool)
        A = delta
    dzb = np.abs(ref["dzb"] if "dzb" in ref else dz)
    hBa, WBa = np.abs(hB), np.abs(WB)
    lam = a["lam"]
    b_gWd = c * (B + 2) * u * (dzb.T @ hBa) + A.T @ hBa + (dzb.T @ hA if h_rel > 0 else 0.0)
    b_gbd = c * (B + 2) * u * dzb.sum(axis=0) + A.sum(axis=0) + 4 * u * (np.abs(ref["gb_dec"]) + lam * np.abs(a["bd"]))
    b_dh = c * (V + 2) * u * (dzb @ WBa) + A @ WBa
    ms = np.abs(a["m"]) * a["sg"] * (1 - a["sg"])
    dpre = ref["dh"] * a["m"] * a["sg"] * (1 - a["sg"])
    b_dpre = b_dh * ms + 4 * u * np.abs(ref["dh"] * a["m"]) + 8 * u * np.abs(dpre)
    xa = np.abs(a["xh"])
    b_gWe = xa.T @ b_dpre + c * (B + 2) * u * (xa.T @ np.abs(dpre)) + 4 * u * (np.abs(ref["gW_enc"]) + lam * np.abs(a["We"]))
    b_gbe = b_dpre.sum(axis=0) + c * (B + 2) * u * np.abs(dpre).sum(axis=0) + 4 * u * (np.abs(ref["gb_enc"]) + lam * np.abs(a["be"]))
    out = dict(gW_enc=b_gWe, gb_enc=b_gbe, gb_dec=b_gbd, dh=b_dh, amb=amb, delta=delta, **extra)
    if a["tied"]:
        out["gW_enc"] = b_gWe + b_gWd
        out["gW_dec"] = None
    else:
        out["gW_dec"] = b_gWd + 4 * u * (np.abs(ref["gW_dec"]) + lam * np.abs(a["Wd_own"]))
    return out


def bf16_check(got, ref, bounds, keys=("gW_enc", "gb_enc", "gW_dec", "gb_dec")):
    """{key: max |got - ref| / bound} over the elements (inf where a non-finite value or a nonzero error meets a zero
    bound).  got: arrays by grads() key; keys whose ref is None (tied gW_dec) are skipped.  Passes when every ratio <= 1."""
    out = {}
    for k in keys:
        if ref.get(k) is None or k not in got:
            continue
        g = np.asarray(got[k], np.float64)
        err = np.abs(g - ref[k])
        bd = bounds[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, err / bd)
        q = np.where(np.isfinite(g), q, np.inf)
        out[k] = float(q.max()) if q.size else 0.0
    return out
