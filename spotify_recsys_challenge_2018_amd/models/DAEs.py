"""Host-side mirror of the reference's models/DAEs.py object protocol on top of the
C ABI of libdae_hip.so.  PyTorch-ROCm is used for device memory and streams only; every hot
operation is a hand-written HIP kernel behind include/dae_hip.h.

Reference protocol (models/DAEs.py, all citations relative to /root/reference):
    model = DAE_tied(conf) | DAE(conf)          # :13 / :114   reads conf.save/batch/n_input/...
    model.fit()                                  # :84          builds the graph
    sess.run(model.init_op)                      # variables -> device
    sess.run(model.y_pred, feed_dict={model.x_positions:..., model.x_ones:...,
             model.keep_prob: 1.0, model.input_keep_prob: 1.0})          # main_train.py:66-68
    sess.run([model.optimizer, model.cost], feed_dict={... y_positions, y_ones, keep_prob,
             input_keep_prob})                                           # main_train.py:204-207
    model.save_model(sess)                       # :107-111  pickle [enc_W, dec_W, enc_b, dec_b]

The same calls work here through `Session` below.  Direct methods (`predict`, `recommend`,
`train_step`) are what the drivers of this repo use; `recommend` is the fused
encode -> decode -> top-k path that never materialises the [batch, n_input] matrix.
"""
import ctypes
import pickle

import numpy as np

from .. import _lib
from . import stream_loop
from .stream_loop import SEEDS_FROM_INPUT      # recommend(seeds=SEEDS_FROM_INPUT): the seeds are the input's track columns


# [BASE] decode_dtype values -> the C ABI's decode arithmetic (include/dae_hip.h)
_DECODE_DTYPES = {"f32": _lib.DAE_DTYPE_F32, "bf16": _lib.DAE_DTYPE_BF16, "exact_bf16": _lib.DAE_DTYPE_BF16_EXACT}


def _title_dtype(dtype, model):
    """Arithmetic of a title-mixed launch.  exact_bf16 has its own two-GEMM path (dae_mix_topk_exact, csrc/mixexact.hip and mix_*.hip)
    for the shapes the library says it takes (dae_mix_exact_shape_ok: DAE hidden 128 .. 512, title feature rows of 64 .. 512,
    both in steps of 64); any other model runs its titled launches on the fp32 kernels (the lists exact_bf16 promises are
    the fp32 lists either way)."""
    if dtype != _lib.DAE_DTYPE_BF16_EXACT:
        return dtype
    tm = model.title_model
    if tm is not None and not model.title_exact_off and _lib.mix_exact_shape_ok(model.n_hidden, tm.ld):
        return dtype
    if tm is not None and not model.title_exact_off and not model._title_fp32_said:
        # [DAE] hidden, [TITLE] filter_num / filter_size are free keys of the schema (main.py:46, :73-75): say ONCE that this
        # model's titled launches cost the fp32 kernels' time, instead of silently
        model._title_fp32_said = True
        import sys
        print("[dae] decode_dtype = exact_bf16: the exact title mix takes hidden = 128 .. 512 and title feature rows of 64 .. 512, "
              "both in steps of 64; this model has hidden = %d, %d-wide rows -- its titled launches run on the fp32 kernels "
              "(same lists, slower)" % (model.n_hidden, tm.ld), file=sys.stderr)
    return _lib.DAE_DTYPE_F32


def _deep_k_dtype(dtype, k, model):
    """Arithmetic of a plain ranking call at k > DAE_MAX_K.  The exact mode's kernels keep k <= 1024; its contract is
    the fp32 lists, so a deeper call runs the fp32 kernels and says so once, as `_title_dtype` does for its fallback."""
    if dtype != _lib.DAE_DTYPE_BF16_EXACT or k <= _lib.DAE_MAX_K:
        return dtype
    if not model._deep_k_said:
        model._deep_k_said = True
        import sys
        print("[dae] decode_dtype = exact_bf16: the exact mode ranks k <= %d; calls with a larger k (here %d) run on the fp32 "
              "kernels (same lists, slower)" % (_lib.DAE_MAX_K, k), file=sys.stderr)
    return _lib.DAE_DTYPE_F32


def _refuse_deep_k(k, what):
    if k > _lib.DAE_MAX_K:
        raise ValueError("%s takes k <= %d (got %d): deeper lists come from `recommend` / `rank_candidates` without titles, "
                         "k <= %d" % (what, _lib.DAE_MAX_K, k, _lib.DAE_MAX_K_DEEP))


class _Placeholder:
    """Stands in for a tf.placeholder: only used as a feed_dict key."""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<placeholder %s>" % self.name


class _Fetch:
    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<fetch %s>" % self.name


def coo_to_csr(positions, values, n_rows, n_cols=None):
    """DAEs.py:33-35 semantics for the kernels: the reference scatters COO (row, col) -> value
    into a dense matrix by ASSIGNMENT with validate_indices=False, so duplicates are the norm and
    the LAST occurrence wins.  Returns CSR with columns ascending per row:
    (row_ptr int32 [n_rows+1], col int32 [nnz], val float32 [nnz]).  Explicit zeros are kept out
    (a zero entry contributes nothing to the row sum or the gather)."""
    pos = np.asarray(positions, dtype=np.int64).reshape(-1, 2)
    n = pos.shape[0]
    vals = np.asarray(values, dtype=np.float32).reshape(-1)
    if vals.size == 1 and n != 1:
        vals = np.full(n, vals[0], dtype=np.float32)
    if vals.size != n:
        raise ValueError("positions (%d) and values (%d) differ in length" % (n, vals.size))
    if n == 0:
        return (np.zeros(n_rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                np.zeros(0, dtype=np.float32))
    rows, cols = pos[:, 0], pos[:, 1]
    if rows.min() < 0 or rows.max() >= n_rows:
        raise ValueError("row index out of range [0,%d)" % n_rows)
    if cols.min() < 0 or (n_cols is not None and cols.max() >= n_cols):
        raise ValueError("column index out of range")
    order = np.lexsort((np.arange(n), cols, rows))          # row, col, then feed order
    r, c, v = rows[order], cols[order], vals[order]
    last = np.ones(n, dtype=bool)
    last[:-1] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])        # last duplicate of each (row, col)
    keep = last & (v != 0.0)
    r, c, v = r[keep], c[keep], v[keep]
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    np.add.at(row_ptr, r + 1, 1)
    row_ptr = np.cumsum(row_ptr)
    return row_ptr.astype(np.int32), c.astype(np.int32), v.astype(np.float32)


def candidates_to_csr(candidates, n_rows, n_cols, unique=False):
    """Caller-given candidate columns -> the CSR the candidate kernels take (csrc/candidates.hip): (row_ptr int32
    [n_rows + 1], col int32 [n_cand]).  `candidates`: a list of per-row id sequences (ragged, possibly empty; fewer than
    n_rows lists leave the last rows empty), or a 2-D int array [n_rows, C].  Ids are GLOBAL columns, tracks and artists in any
    order; -1 is padding (it keeps its slot, so results stay aligned with the input).  unique: per row, padding dropped and
    every column listed once, ascending (what a ranking needs: a column listed twice would be ranked twice).  Any other id
    outside [0, n_cols) raises ValueError.  Pure numpy: needs no device."""
    import itertools
    if isinstance(candidates, np.ndarray) and candidates.ndim == 2:
        if candidates.dtype.kind not in "iu":
            raise ValueError("candidates: an integer array is required, got %s" % candidates.dtype)
        if candidates.shape[0] > n_rows:
            raise ValueError("candidates: %d rows for a feed of %d" % (candidates.shape[0], n_rows))
        lens = np.zeros(n_rows, dtype=np.int64)
        lens[:candidates.shape[0]] = candidates.shape[1]
        flat = candidates.astype(np.int64).reshape(-1)
    else:
        if len(candidates) > n_rows:
            raise ValueError("candidates: %d rows for a feed of %d" % (len(candidates), n_rows))
        lens = np.zeros(n_rows, dtype=np.int64)
        lens[:len(candidates)] = np.fromiter(map(len, candidates), dtype=np.int64, count=len(candidates))
        total = int(lens.sum())
        flat = np.fromiter(itertools.chain.from_iterable(candidates), dtype=np.int64, count=total)
    if flat.size and (flat.min() < -1 or flat.max() >= n_cols):
        bad = flat[(flat < -1) | (flat >= n_cols)][0]
        raise ValueError("candidate id %d out of range: -1 (padding) or [0, %d)" % (bad, n_cols))
    if flat.size >= 2 ** 31:
        raise ValueError("candidates: %d entries do not fit the int32 offsets of the CSR" % flat.size)
    if unique:
        rows = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
        ok = flat >= 0
        flat, rows = flat[ok], rows[ok]
        order = np.lexsort((flat, rows))
        flat, rows = flat[order], rows[order]
        first = np.ones(flat.size, dtype=bool)
        first[1:] = (rows[1:] != rows[:-1]) | (flat[1:] != flat[:-1])
        flat, rows = flat[first], rows[first]
        lens = np.bincount(rows, minlength=n_rows).astype(np.int64)
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(lens)
    return row_ptr.astype(np.int32), flat.astype(np.int32)


def seeds_to_csr(seeds, n_rows, n_tracks):
    """Per-row seed track lists (main_challenge.py:31-35 `cand.remove(i)`) -> CSR of sorted unique
    in-range track ids.  One lexsort over all rows (the per-row np.unique loop was the largest host cost
    of a scoring call)."""
    import itertools
    used = seeds[:n_rows] if len(seeds) > n_rows else seeds
    lens = np.zeros(n_rows, dtype=np.int64)
    lens[:len(used)] = np.fromiter(map(len, used), dtype=np.int64, count=len(used))
    total = int(lens.sum())
    if total == 0:
        return np.zeros(n_rows + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    flat = np.fromiter(itertools.chain.from_iterable(used), dtype=np.int64, count=total)
    rows = np.repeat(np.arange(n_rows, dtype=np.int64), lens)
    ok = (flat >= 0) & (flat < n_tracks)
    flat, rows = flat[ok], rows[ok]
    order = np.lexsort((flat, rows))
    flat, rows = flat[order], rows[order]
    first = np.ones(flat.size, dtype=bool)
    first[1:] = (rows[1:] != rows[:-1]) | (flat[1:] != flat[:-1])
    flat, rows = flat[first], rows[first]
    row_ptr = np.zeros(n_rows + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(rows, minlength=n_rows))
    return row_ptr.astype(np.int32), flat.astype(np.int32)


def catalogue_columns(columns, n_tracks):
    """The columns of a catalogue (`model.catalogue`) -> int32 array, or ValueError naming the first offender: the list holds
    track columns, each once, in ascending order (local order then equals global order: the canonical tie-break by column is the
    same inside the catalogue and outside).  Pure numpy: needs no device."""
    a = np.asarray(columns)
    if a.ndim != 1:
        raise ValueError("catalogue: a flat sequence of column ids is required, got shape %s" % (a.shape,))
    if a.size == 0:
        raise ValueError("catalogue: the list of columns is empty")
    if a.dtype.kind not in "iu":
        raise ValueError("catalogue: integer column ids are required, got %s" % a.dtype)
    a = a.astype(np.int64)
    bad = np.nonzero(a < 0)[0]
    if bad.size:
        raise ValueError("catalogue: columns[%d] = %d is negative" % (bad[0], a[bad[0]]))
    bad = np.nonzero(a >= n_tracks)[0]
    if bad.size:
        raise ValueError("catalogue: columns[%d] = %d is no track column (tracks are [0, %d); artist columns are never ranked)"
                         % (bad[0], a[bad[0]], n_tracks))
    bad = np.nonzero(np.diff(a) <= 0)[0]
    if bad.size:
        i = int(bad[0]) + 1
        if a[i] == a[i - 1]:
            raise ValueError("catalogue: columns[%d] = %d is listed twice (a duplicate of columns[%d])" % (i, a[i], i - 1))
        raise ValueError("catalogue: columns[%d] = %d is below columns[%d] = %d: the list must be sorted ascending"
                         % (i, a[i], i - 1, a[i - 1]))
    return a.astype(np.int32)


class CatalogueHandle:
    """What `model.catalogue(columns)` returns and `recommend(..., catalogue=handle)` takes: the column set on the device
    (_lib.Catalogue) and contexts of its OWN that hold the decoder rows of those columns as images -- one for the DAE's decoder
    and, on a DAE_title, one for the title scorer's output layer -- packed lazily per dtype.  The model's own full images are
    never re-tiled when full and catalogue calls alternate.  The images follow the model's weights: after a parameter change
    (`_mark_dirty` / the title model's `_params_gen`) the next call re-packs.  Memory per dtype in use: n x hidden x 4 (fp32) or
    2 (bf16) bytes plus bounds (exact_bf16: the fp32 rows as well), the same for the title rows; 4 (n + n_tracks) bytes for the
    column tables.  The streamed loops (`recommend_iter` / `evaluate_iter(..., catalogue=handle)`) run on pipelines in catalogue mode
    that hold images of their own; the handle remembers them.  `close()` closes those pipelines first, then frees everything."""

    def __init__(self, model, cols):
        import torch
        self.model, self.columns = model, cols
        self.ctx = _lib.Context(model.device_index)
        dev = torch.device("cuda", model.device_index)
        self.cat = _lib.Catalogue(self.ctx, torch.from_numpy(cols).to(dev), model.n_tracks)
        self.n = int(cols.size)
        self.title_ctx = _lib.Context(model.device_index) if model._title_scorer() is not None else None
        self._packed, self._title_packed = {}, {}        # image slot -> (weights generation, holds the exact mode's bounds)
        self._exact_title_said = False
        self._pipes = []                                 # the streamed loops' pipelines in catalogue mode (stream_loop.pipeline_for)

    def _title_dtype(self, dtype):
        """Arithmetic of a titled launch inside this catalogue: exact_bf16 has no catalogue mix and runs on the fp32 kernels (the
        lists it promises), said once per handle."""
        if dtype != _lib.DAE_DTYPE_BF16_EXACT:
            return dtype
        if not self._exact_title_said:
            self._exact_title_said = True
            import sys
            print("[dae] decode_dtype = exact_bf16: the exact title mix does not rank inside a catalogue; titled catalogue "
                  "calls run on the fp32 kernels (same lists, slower)", file=sys.stderr)
        return _lib.DAE_DTYPE_F32

    @staticmethod
    def _fresh(packed, slot, gen, dtype):
        have = packed.get(slot)
        return have is not None and have[0] == gen and (dtype != _lib.DAE_DTYPE_BF16_EXACT or have[1])

    def _ensure(self, dtype):
        """The DAE context's image of `dtype` holds the catalogue's rows of the model's CURRENT decoder."""
        m = self.model
        m.sync_params()
        slot = _lib.Context._slot(dtype)
        if not self._fresh(self._packed, slot, m._weights_gen, dtype):
            self.ctx.bind_stream()
            self.ctx.prepack_decoder_catalogue(self.cat, m.weights["decoder_h"], m.biases["decoder_b"], dtype)
            self._packed[slot] = (m._weights_gen, dtype == _lib.DAE_DTYPE_BF16_EXACT)

    def _ensure_title(self, dtype):
        """The same for the title scorer's Output_W^T / Output_b on the title context."""
        tm = self.model.title_model
        if dtype == _lib.DAE_DTYPE_F32:
            tm._check_f32_features()
        slot = _lib.Context._slot(dtype)
        if not self._fresh(self._title_packed, slot, tm._params_gen, dtype):
            self.title_ctx.bind_stream()
            self.title_ctx.prepack_decoder_catalogue(self.cat, tm.p["Output_WT"], tm.p["Output_b"], dtype)
            self._title_packed[slot] = (tm._params_gen, dtype == _lib.DAE_DTYPE_BF16_EXACT)

    def close(self):
        if getattr(self, "cat", None) is not None:
            # the pipelines read the column tables: gone first, and out of the model's cache.  One whose result arrays are still
            # alive in the caller's hands only stops taking feeds (`Pipeline.close`); it has nothing in flight once drained
            for pipe in self._pipes:
                if pipe.h is not None:
                    try:
                        pipe.flush()
                        while pipe.pending and (pipe.poll_eval(True) if pipe.eval else pipe.poll(True, copy=True)) is not None:
                            pass
                    except _lib.DaeError:
                        pass
                    pipe.close()
            for key in [key for key, (_gen, pipe) in self.model._pipes.items() if pipe in self._pipes]:
                self.model._pipes.pop(key, None)
            self._pipes = []
            self.cat.close()
            self.cat = None
            for c in (self.ctx, self.title_ctx):
                if c is not None:
                    c.close()
            self.ctx = self.title_ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DAE_tied:
    """Tied-weight denoising autoencoder (reference DAEs.py:13-111)."""

    tied = True

    def __init__(self, conf):
        self.save_dir = conf.save                       # DAEs.py:15
        self.n_batch = int(conf.batch)                  # :17
        self.n_input = int(conf.n_input)                # :18
        self.n_hidden = int(conf.hidden)                # :19
        self.learning_rate = float(conf.lr)             # :20
        self.reg_lambda = float(conf.reg_lambda)        # :21
        self.n_tracks = int(getattr(conf, "n_tracks", self.n_input))
        self.device_index = int(getattr(conf, "device_index", 0))
        self.init_seed = int(getattr(conf, "init_seed", 0))

        # feed_dict keys (DAEs.py:23-30)
        self.x_positions = _Placeholder("x_positions")
        self.x_ones = _Placeholder("x_ones")
        self.y_positions = _Placeholder("y_positions")
        self.y_ones = _Placeholder("y_ones")
        self.keep_prob = _Placeholder("keep_prob")
        self.input_keep_prob = _Placeholder("input_keep_prob")

        self.y_pred = None
        self.cost = None
        self.optimizer = None
        self.init_op = None
        self.weights = {}
        self.biases = {}
        self.d_params = []
        self.ctx = None
        self._adam = None
        self._step = 0
        self._packed_dirty = {_lib.DAE_DTYPE_F32: True, _lib.DAE_DTYPE_BF16: True, _lib.DAE_DTYPE_BF16_EXACT: True}
        self._packed_cols = {}
        # decode arithmetic of recommend(): "f32" (fp32 MFMA, bit-exact path), "bf16" (BASELINE configs[4]) or
        # "exact_bf16" (BASELINE north_star: bf16 MFMA filter + fp32 recomputation of the survivors -- the fp32
        # path's lists, bit for bit, at close to the bf16 rate)
        dd = str(getattr(conf, "decode_dtype", "f32"))
        if dd not in _DECODE_DTYPES:
            raise ValueError("decode_dtype %r: one of %s" % (dd, sorted(_DECODE_DTYPES)))
        self.decode_dtype = _DECODE_DTYPES[dd]
        # arithmetic of the training forward GEMM: "f32" (default) or "bf16" (BASELINE configs[3]: bf16 operands,
        # fp32 accumulate; loss, backward GEMMs, parameters and Adam stay fp32)
        self.train_dtype = _lib.DAE_DTYPE_BF16 if str(getattr(conf, "train_dtype", "f32")) == "bf16" \
            else _lib.DAE_DTYPE_F32
        # untied model, reg_lambda == 0: the encoder's gradient is row-sparse, and its dense Adam runs through
        # dae_adam_rows_* (bit-identical parameters, no HBM passes over the rows without gradient); "dense" keeps
        # dae_adam_step on the whole matrix
        self.encoder_adam = str(getattr(conf, "encoder_adam", "rows"))
        self.decoder_adam = str(getattr(conf, "decoder_adam", "fused"))        # "fused" (dae_arm_decoder_adam) | "dense"
        # ... and every `rows_adam_flush_every` steps all rows are brought up to date, which bounds how many missed
        # steps a rarely seen row has to replay when it is next named (a replay is sequential per element)
        self.rows_adam_flush_every = int(getattr(conf, "rows_adam_flush_every", 32))
        self.rows_adam_table = int(getattr(conf, "rows_adam_table", 1 << 16))      # alpha per step; doubles when full
        self._lazy = None
        self._rng = np.random.RandomState(int(getattr(conf, "dropout_seed", 1234)))
        self.device_csr = bool(getattr(conf, "device_csr", True))
        self._csr_status = None
        self._sharded = None          # sharding.ShardedTrainer when training is row-sharded over ranks
        self._train_feed = None       # attach_train_set(): the reader and its playlists on the device (_lib.TrainSet)
        self._params_stale = False
        self._score_shard = None      # shard_scoring(): this rank's vocabulary columns + the ShardedRanker
        self._copy_stream = None      # _to_dev(side_stream=True): the training loop's upload stream
        self._weights_gen = 0         # bumps with every change of the weights (a cached pipeline holds images of the old ones)
        self._pipes = {}              # the streamed loop's pipelines (stream_loop.py): key -> (generation, _lib.Pipeline)
        self.coalesce = self.n_lanes = None      # set from outside: feeds per launch, lanes (None: `_coalesce_count` / three)
        self.keep_pipelines, self._old_pipes = False, []      # ... and (diagnosis) retired pipelines kept alive, here
        self._deep_k_said = False     # `_deep_k_dtype` said that exact_bf16 calls with k > 1024 run on the fp32 kernels
        self._guard_fallbacks = 0     # batches / launches re-scored in fp32 because the exact mode's bound guard fired

    # -- parameters ---------------------------------------------------------------------------------
    def _xavier(self, rng, shape):
        """tf.contrib.layers.xavier_initializer() (uniform): U(+-sqrt(6/(fan_in+fan_out)))."""
        lim = np.sqrt(6.0 / (shape[0] + shape[1]))
        return rng.uniform(-lim, lim, size=shape).astype(np.float32)

    def _host_init(self):
        """DAEs.py:53-61: encoder_h Xavier, biases zero; decoder IS the encoder matrix."""
        rng = np.random.default_rng(self.init_seed)
        W = self._xavier(rng, (self.n_input, self.n_hidden))
        return [W, W, np.zeros(self.n_hidden, np.float32), np.zeros(self.n_input, np.float32)]

    def init_weight(self):
        import torch
        dev = torch.device("cuda", self.device_index)
        enc_W, dec_W, enc_b, dec_b = self._host_init()
        for a, shp in ((enc_W, (self.n_input, self.n_hidden)), (dec_W, (self.n_input, self.n_hidden)),
                       (enc_b, (self.n_hidden,)), (dec_b, (self.n_input,))):
            if tuple(a.shape) != shp:
                raise ValueError("initial value has shape %s, expected %s" % (a.shape, shp))
        self.weights["encoder_h"] = torch.from_numpy(np.ascontiguousarray(enc_W, np.float32)).to(dev)
        if self.tied:
            self.weights["decoder_h"] = self.weights["encoder_h"]
        else:
            self.weights["decoder_h"] = torch.from_numpy(np.ascontiguousarray(dec_W, np.float32)).to(dev)
        self.biases["encoder_b"] = torch.from_numpy(np.ascontiguousarray(enc_b, np.float32)).to(dev)
        self.biases["decoder_b"] = torch.from_numpy(np.ascontiguousarray(dec_b, np.float32)).to(dev)
        self.d_params = [self.weights["encoder_h"], self.weights["decoder_h"],
                         self.biases["encoder_b"], self.biases["decoder_b"]]
        self._mark_dirty()

    def fit(self):
        """DAEs.py:84-105.  Creates the device context, the parameters and the fetch handles."""
        self.ctx = _lib.Context(self.device_index)
        if self.train_dtype != _lib.DAE_DTYPE_F32:
            self.ctx.set_train_dtype(self.train_dtype)
        self.init_weight()
        self.y_pred = _Fetch("y_pred")
        self.cost = _Fetch("cost")
        self.optimizer = _Fetch("optimizer")
        self.init_op = _Fetch("init_op")
        self.hidden = _Fetch("hidden")

    # -- helpers ------------------------------------------------------------------------------------
    def _to_dev(self, a, dtype, side_stream=False):
        """Host array -> device tensor.  side_stream (the training loop): uploaded on a COPY stream.  A copy from pageable memory is stream-ordered
        and blocks the host until it has happened; on the compute stream that means "until everything queued before
        it has run", so the training loop could never get ahead of the GPU (0.25 ms per feed measured).  On its own
        stream the copy waits for earlier copies only; the compute stream waits for its event.  (The scoring loop
        stages its feeds inside the library: csrc/pipeline_stage.h.)"""
        import torch
        src = torch.from_numpy(np.ascontiguousarray(a))
        dev = torch.device("cuda", self.device_index)
        if not side_stream:                  # calls that fetch their result anyway (recommend, predict, ...)
            return src.to(dev, dtype=dtype, non_blocking=False)
        cs = self._copy_stream
        if cs is None:
            cs = self._copy_stream = torch.cuda.Stream(device=dev)
        cur = torch.cuda.current_stream(self.device_index)
        with torch.cuda.stream(cs):
            t = src.to(dev, dtype=dtype, non_blocking=False)
            ev = cs.record_event()
        cur.wait_event(ev)
        t.record_stream(cur)
        return t

    @staticmethod
    def _feed_arrays(positions, values):
        pos = np.ascontiguousarray(np.asarray(positions, dtype=np.int64).reshape(-1, 2))
        vals = np.ascontiguousarray(np.asarray(values, dtype=np.float32).reshape(-1))
        if vals.size != 1 and vals.size != pos.shape[0]:
            raise ValueError("positions (%d) and values (%d) differ in length" % (pos.shape[0], vals.size))
        return pos, vals

    def _upload_csr(self, positions, values, side_stream=False, n_rows=None):
        """The feed (COO in feed order, duplicates allowed) -> device CSR.  Default: upload the raw feed
        and build the CSR on the GPU (dae_coo_to_csr, csrc/csr.hip); `device_csr = False` keeps the numpy
        restatement `coo_to_csr` (same result entry for entry; it also range-checks eagerly)."""
        import torch
        if self.device_csr:
            pos, vals = self._feed_arrays(positions, values)
            d_pos = self._to_dev(pos if pos.shape[0] else np.zeros((1, 2), np.int64), torch.int64, side_stream)[:pos.shape[0]]
            d_val = self._to_dev(vals if vals.size else np.zeros(1, np.float32), torch.float32, side_stream)
            rp, c, v, status = self.ctx.coo_to_csr(d_pos, d_val, n_rows or self.n_batch, self.n_input)
            # checked lazily (no sync on the scoring path).  A flag is written on the stream that is current NOW -- the
            # main stream or the second scoring lane's -- so it travels with an event recorded behind its writer: whoever
            # reads it later, on whichever stream, waits for exactly that
            cur = torch.cuda.current_stream(self.device_index)
            pending = (self._csr_status or []) + [(status, cur.record_event())]
            if len(pending) > 64:                               # un-fetched training steps: fold on the device
                pending = [(self._fold_status(pending), cur.record_event())]
            self._csr_status = pending
            return rp, c, v
        rp, c, v = coo_to_csr(positions, values, n_rows or self.n_batch, self.n_input)
        if c.size == 0:          # keep valid device pointers for empty batches
            c = np.zeros(1, np.int32); v = np.zeros(1, np.float32)
        return self._to_dev(rp, torch.int32), self._to_dev(c, torch.int32), self._to_dev(v, torch.float32)

    def _fold_status(self, pending):
        """max over the pending range flags, on the current stream, ordered behind every flag's writer."""
        import torch
        cur = torch.cuda.current_stream(self.device_index)
        for st, ev in pending:
            cur.wait_event(ev)
            st.record_stream(cur)                               # allocated on its writer's stream, read (and freed) here
        return torch.cat([st for st, _ev in pending]).max().reshape(1)

    def _check_feed(self):
        """After the results of a call have been fetched: the device CSR builder skips entries whose row / column is
        out of range and raises the flag checked here."""
        if self._csr_status:
            bad = int(self._fold_status(self._csr_status).item())
            self._csr_status = None
            if bad:
                raise ValueError("feed holds a row or column index out of range (rows [0,%d) of each feed, columns [0,%d))"
                                 % (self.n_batch, self.n_input))

    check_feed = _check_feed

    def _mark_dirty(self):
        """The packed decoder images of the context(s) no longer hold the current weights."""
        self._packed_dirty = {_lib.DAE_DTYPE_F32: True, _lib.DAE_DTYPE_BF16: True, _lib.DAE_DTYPE_BF16_EXACT: True}
        self._packed_cols = {}
        self._weights_gen += 1

    # -- multi-GPU scoring (BASELINE.json configs[2]): vocabulary columns sharded over the ranks ----
    def shard_scoring(self, rank, world, group=None, exchange="allgather", tau_exchange=True):
        """`recommend` through sharding.ShardedRanker: this rank decodes and ranks only the vocabulary columns
        `sharding.scoring_shard(n_tracks, n_input, world, rank)` (W_enc is replicated, so every rank computes the same hidden
        activations with no collective), the per-shard top-k lists meet in ONE exchange (RCCL all-gather, or an
        all-to-all of the rows each rank owns) and are merged with the same key -- exact, since a shard's top-k
        holds its share of the global top-k.  Every rank feeds the same batches.

        exchange = "allgather": `recommend` returns all rows on every rank (main_challenge: rank 0 writes).
        exchange = "alltoall":  `recommend` returns the rows this rank owns (`owned_rows()`); n_batch is rounded
        up to a multiple of the world size (the extra rows are empty).
        tau_exchange: the shards' thresholds meet before the filter launches (one more collective of 4 bytes per row
        and rank; sharding.ShardedRanker "threshold exchange"): same lists, less selection work per shard."""
        from ..sharding import scoring_shard
        if exchange not in ("allgather", "alltoall"):
            raise ValueError("unknown exchange %r" % (exchange,))
        if exchange == "alltoall" and self.n_batch % world:
            if self.ctx is not None:
                raise _lib.DaeError("shard_scoring(alltoall) must round n_batch up before fit()")
            self.n_batch += world - self.n_batch % world
        shard = scoring_shard(self.n_tracks, self.n_input, world, rank)
        self._score_shard = {"rank": int(rank), "world": int(world), "group": group, "exchange": exchange,
                             "cols": shard, "rank_bound": shard[0][1], "rankers": {}, "tau_exchange": bool(tau_exchange)}
        self._mark_dirty()

    def owned_rows(self):
        """Rows of a batch whose final top-k `recommend` returns on this rank: all of them, except under
        shard_scoring(exchange="alltoall")."""
        sh = self._score_shard
        if sh is None or sh["exchange"] != "alltoall":
            return 0, self.n_batch
        from ..sharding import row_owner_bounds
        return row_owner_bounds(self.n_batch, sh["world"], sh["rank"])

    def _shard_ranker(self, dtype):
        sh = self._score_shard
        if dtype not in sh["rankers"]:
            from ..sharding import HipRankStages, ShardedRanker
            # the rank's image holds its track slice under the real ids, then its artist slice: rank only below the bound
            st = HipRankStages(self.ctx, self.weights["encoder_h"], self.biases["encoder_b"], sh["rank_bound"], dtype)
            two = dict(local_begin=st.local_begin, local_finish=st.local_finish) if sh.get("tau_exchange") else {}
            sh["rankers"][dtype] = ShardedRanker(st.local_topk, st.merge, group=sh["group"], exchange=sh["exchange"], **two)
        return sh["rankers"][dtype]

    # -- multi-GPU training: rows of W_enc / W_dec / b_dec sharded over the ranks ---------
    def shard_training(self, rank, world, group=None):
        """Train through sharding.ShardedTrainer: this rank updates only its vocabulary rows (two
        [batch, hidden] all-reduces per step over RCCL).  Inference keeps a full replica per rank
        (W_enc replicated); it is refreshed from the shards by `sync_params`, which the
        scoring / persistence entry points call when training has run since the last refresh."""
        from ..sharding import HipTrainStages, ShardedTrainer
        self._sharded = ShardedTrainer(self.get_params(), self.n_batch, self.learning_rate,
                                       self.reg_lambda, self.tied, HipTrainStages(self.ctx),
                                       device=self.weights["encoder_h"].device, rank=rank, world=world,
                                       group=group, seed=int(self._rng.randint(0, 2 ** 31 - 1)))

    def _flush_rows_adam(self):
        """Every encoder row current for the last training step (rows without gradient lag behind until someone
        needs the whole matrix: evaluation, saving, sharding)."""
        lz = self._lazy
        if lz is None or lz["flushed"] == self._step:
            return
        self.ctx.bind_stream()
        m, v = self._adam["encoder_h"]
        P = _lib._ptr
        self.ctx.check(self.ctx.lib.dae_adam_rows_flush(
            self.ctx.h, P(self.weights["encoder_h"]), P(m), P(v), P(lz["state"]), P(lz["tab"]), lz["tab"].numel(),
            self.n_input, self.n_hidden, 0.9, 0.999, 1e-8, self._step))
        lz["flushed"] = self._step

    def sync_params(self):
        """Parameters current on this rank: pending row updates of the encoder applied, and -- collective when
        sharded (every rank must call it at the same point) -- the replica refreshed from the shards."""
        self._flush_rows_adam()
        if self._sharded is None or not self._params_stale:
            return
        enc_W, dec_W, enc_b, dec_b = self._sharded.gather_params(as_numpy=False)     # stays on the device
        self.weights["encoder_h"].copy_(enc_W)
        if not self.tied:
            self.weights["decoder_h"].copy_(dec_W)
        self.biases["encoder_b"].copy_(enc_b)
        self.biases["decoder_b"].copy_(dec_b)
        self._params_stale = False
        self._mark_dirty()

    def _ensure_packed(self, dtype=_lib.DAE_DTYPE_F32, cols=None):
        """The context's packed decoder image of `dtype` holds columns `cols` (default: all) of the current
        weights.  (A context keeps one image per dtype: a sharded `recommend` and a dense `predict` on the same
        model re-tile when they alternate -- 0.13 ms.)"""
        self.sync_params()
        shard = cols is not None and isinstance(cols[0], (tuple, list))        # sharding.scoring_shard: (tracks, artists)
        cols = (0, self.n_input) if cols is None else (tuple(map(tuple, cols)) if shard else (int(cols[0]), int(cols[1])))
        if self._packed_dirty[dtype] or self._packed_cols.get(dtype) != cols:
            self.ctx.bind_stream()
            if shard:
                from ..sharding import prepack_scoring_shard
                _bound, self._shard_rows = prepack_scoring_shard(self.ctx, self.weights["decoder_h"],
                                                                 self.biases["decoder_b"], cols, dtype)
            else:
                self.ctx.prepack_decoder(self.weights["decoder_h"], self.biases["decoder_b"], cols[0], cols[1], dtype)
            self._packed_dirty[dtype] = False
            self._packed_cols[dtype] = cols
            # "bf16" and "exact_bf16" share the context's bf16 image: the exact prepack serves both, a plain bf16
            # prepack drops the bounds the exact mode needs
            if dtype == _lib.DAE_DTYPE_BF16_EXACT:
                self._packed_dirty[_lib.DAE_DTYPE_BF16] = False
                self._packed_cols[_lib.DAE_DTYPE_BF16] = cols
            elif dtype == _lib.DAE_DTYPE_BF16:
                self._packed_dirty[_lib.DAE_DTYPE_BF16_EXACT] = True

    def encode(self, x_positions, x_ones, keep_prob=1.0, input_keep_prob=1.0, seed=0):
        """DAEs.py:40-42 + :64-70 -> hidden [n_batch, n_hidden] (torch CUDA tensor)."""
        import torch
        self.sync_params()
        self.ctx.bind_stream()
        rp, c, v = self._upload_csr(x_positions, x_ones)
        h = torch.empty((self.n_batch, self.n_hidden), dtype=torch.float32,
                        device=self.weights["encoder_h"].device)
        self.ctx.encode(rp, c, v, self.weights["encoder_h"], self.biases["encoder_b"], h,
                        ikp=input_keep_prob, kp=keep_prob, seed=seed)
        return h

    def predict(self, x_positions, x_ones, keep_prob=1.0, input_keep_prob=1.0, seed=0):
        """sess.run(model.y_pred, ...) : dense scores [n_batch, n_input] float32 (host array)."""
        import torch
        self._ensure_packed()
        h = self.encode(x_positions, x_ones, keep_prob, input_keep_prob, seed)
        out = torch.empty((self.n_batch, self.n_input), dtype=torch.float32, device=h.device)
        self.ctx.decode_dense(h, out, apply_sigmoid=True)
        res = out.cpu().numpy()
        self._check_feed()
        return res

    def loss(self, x_positions, x_ones, y_positions, y_ones, keep_prob=1.0, input_keep_prob=1.0, seed=None, n_rows=None,
             per_row=False):
        """sess.run(model.cost, ...): the cost of a batch WITHOUT a step (dae_score_loss) -> float, or (cost, rows) with
        `per_row`: rows float32 [n_rows], the loss of each row over all columns; cost = sum(rows) / n_batch + reg_lambda * l2,
        in the arithmetic of the training step (`train_dtype`).  The same dropout masks as a step with the same `seed`; a
        keep probability below 1 needs an explicit seed (the model's own dropout stream is never drawn from, so a training
        run with calls of this in between trains the same model).  Nothing of the model changes."""
        import torch
        self._refuse_loss()
        if (float(keep_prob) < 1.0 or float(input_keep_prob) < 1.0) and seed is None:
            raise ValueError("loss: a keep probability below 1 needs an explicit seed")
        n = self.n_batch if n_rows is None else int(n_rows)
        self._ensure_packed(self.train_dtype)                 # (and the encoder's lazily updated rows: sync_params)
        self.ctx.bind_stream()
        x = self._upload_csr(x_positions, x_ones, n_rows=n)
        y = self._upload_csr(y_positions, y_ones, n_rows=n)
        dev = self.weights["encoder_h"].device
        cost = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty(n, dtype=torch.float32, device=dev) if per_row else None
        self.ctx.score_loss(x, y, self.weights["encoder_h"], self.biases["encoder_b"],
                            None if self.tied else self.weights["decoder_h"], self.biases["decoder_b"], self.n_batch, self.tied,
                            ikp=input_keep_prob, kp=keep_prob, seed=0 if seed is None else seed, reg_lambda=self.reg_lambda,
                            row_loss=rows, cost_out=cost)
        c = float(cost.item())
        res = (c, rows.cpu().numpy()) if per_row else c
        self._check_feed()
        return res

    def _refuse_loss(self):
        """`loss` is refused by name, before any launch, where its kernels do not apply."""
        if self._sharded is not None or self._score_shard is not None:
            raise _lib.DaeError("loss: not available on a vocabulary-sharded model (shard_training / shard_scoring): partial "
                                "costs across ranks are not built")

    def _dtype_of(self, dtype):
        if dtype is None:
            return self.decode_dtype
        if dtype in _DECODE_DTYPES:
            return _DECODE_DTYPES[dtype]
        if dtype in _DECODE_DTYPES.values():
            return int(dtype)
        raise ValueError("decode dtype %r: one of %s" % (dtype, sorted(_DECODE_DTYPES)))

    def _seed_csr_dev(self, seeds, csr, n_rows=None):
        """Seed lists -> device CSR.  `seeds` is a list of per-row track-id lists (main_challenge.py:31-35), or
        SEEDS_FROM_INPUT: the seeds are the playlist's own tracks -- what both reference drivers pass -- and are cut
        out of the input CSR on the device (dae_seeds_from_csr): no per-row list handling, no uploads."""
        import torch
        if isinstance(seeds, str):
            if seeds != SEEDS_FROM_INPUT:
                raise ValueError("seeds: a list of per-row id lists, or SEEDS_FROM_INPUT")
            return self.ctx.seeds_from_csr(csr[0], csr[1], self.n_tracks)
        srp, sc = seeds_to_csr(seeds, n_rows or self.n_batch, self.n_tracks)
        if sc.size == 0:
            sc = np.zeros(1, np.int32)
        return self._to_dev(srp, torch.int32), self._to_dev(sc, torch.int32)

    def _submit(self, x_positions, x_ones, seeds, k, dtype, n_rows=None):
        """Enqueue one batch of the fused scoring path on the current stream; nothing is fetched.
        -> (score, idx).  `n_rows`: rows of this launch when it is not the model's batch."""
        import torch
        nb = n_rows or self.n_batch
        dev = self.weights["encoder_h"].device
        csr = self._upload_csr(x_positions, x_ones, n_rows=nb)
        d_srp, d_sc = self._seed_csr_dev(seeds, csr, n_rows=nb)
        score = torch.empty((nb, k), dtype=torch.float32, device=dev)
        idx = torch.empty((nb, k), dtype=torch.int32, device=dev)
        self.ctx.score_topk(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"],
                            self.n_tracks, d_srp, d_sc, k, score, idx, dtype=dtype)
        return score, idx

    def _title_scorer(self):
        """The title scorer the launches of this model's pipeline mix in, or None.  (The pipeline computes what `_submit` does:
        nothing in this repository overrides `_submit` without being a DAE_title, so every model may stream.)"""
        return None

    def _guard_fell_back(self, what, n=1):
        """The bound guard fired and the caller (or the pipeline) re-scores in fp32: counted, and said once per event."""
        import warnings
        self._guard_fallbacks += n
        warnings.warn(what, stacklevel=2)

    # -- a catalogue: the same column subset for every row (csrc/catalogue.hip) -----------------------------------------------------
    def catalogue(self, columns):
        """A handle for `recommend(..., catalogue=handle)`: the k best tracks among THESE columns -- a market's catalogue, the
        tracks still licensed, another generator's pool -- at the cost of a ranking over len(columns) columns instead of n_tracks.
        columns: any integer sequence or array of track columns, ascending, each once; an unsorted, repeated, negative or
        non-track id or an empty list raises ValueError naming the offender, before anything touches the device.  The handle
        (CatalogueHandle) owns its contexts and images and follows this model's weights; `handle.close()` frees it.
        `recommend_iter`, `evaluate_iter` and `rank_candidates` take the handle as `catalogue=` too, and `main.py --challenge`
        reads one from `[CHALLENGE] catalogue`.  Not built: vocabulary shards (a model with a scoring shard is refused here), a
        catalogue key for `main_train.py eval`, deep k in the loops."""
        if self._score_shard is not None:
            raise _lib.DaeError("catalogue scoring is not vocabulary-sharded: this model has a scoring shard (shard_scoring); "
                                "rank a catalogue on a model that holds the whole decoder")
        cols = catalogue_columns(columns, self.n_tracks)
        if self.ctx is None:
            raise _lib.DaeError("catalogue(): call fit() first -- the handle lives on the model's device")
        return CatalogueHandle(self, cols)

    def _catalogue_begin(self, cat):
        if not isinstance(cat, CatalogueHandle) or cat.model is not self:
            raise ValueError("catalogue: a handle from this model's `catalogue(columns)` is required")
        if cat.cat is None:
            raise ValueError("catalogue: the handle has been closed")
        if self._score_shard is not None:
            raise _lib.DaeError("catalogue scoring is not vocabulary-sharded: this model has a scoring shard (shard_scoring); "
                                "rank a catalogue on a model that holds the whole decoder")

    def _recommend_catalogue(self, cat, x_positions, x_ones, seeds, k, n_rows, dtype):
        """`recommend` inside a catalogue: the feed's CSR and seed lists as always (global columns, built on this model's
        context), then dae_score_topk_catalogue on the handle's context -- its image holds the catalogue's rows only."""
        import torch
        dtype = _deep_k_dtype(self._dtype_of(dtype), k, self)
        cat._ensure(dtype)
        self.ctx.bind_stream()
        cat.ctx.bind_stream()
        n_rows = self.n_batch if n_rows is None else n_rows
        dev = self.weights["encoder_h"].device
        csr = self._upload_csr(x_positions, x_ones)
        d_srp, d_sc = self._seed_csr_dev(seeds, csr)
        score = torch.empty((self.n_batch, k), dtype=torch.float32, device=dev)
        idx = torch.empty((self.n_batch, k), dtype=torch.int32, device=dev)
        cat.ctx.score_topk_catalogue(cat.cat, csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"],
                                     d_srp, d_sc, k, score, idx, dtype=dtype)
        res = idx[:n_rows].cpu().numpy(), score[:n_rows].cpu().numpy()
        self._check_feed()
        if dtype == _lib.DAE_DTYPE_BF16_EXACT:
            # the exact mode's bound guard, on the handle's context: the same call again on the catalogue's fp32 image
            n_bad, col = cat.ctx.exact_guard_read()
            if n_bad:
                self._guard_fell_back("exact_bf16 (catalogue): the bound guard fired (%d survivors, e.g. catalogue position %d): "
                                      "this batch is re-scored with the fp32 kernels" % (n_bad, col))
                return self._recommend_catalogue(cat, x_positions, x_ones, seeds, k, n_rows, _lib.DAE_DTYPE_F32)
        return res

    def recommend(self, x_positions, x_ones, seeds, k=500, n_rows=None, dtype=None, catalogue=None):
        """Fused scoring path: encode -> decode -> top-k (track columns, seeds removed).
        Equivalent of main_challenge.py:80-90 / main_train.py:66-89 without the dense matrix.
        Returns (idx [n_rows,k] int32 with -1 padding, score [n_rows,k] float32).
        catalogue: a handle of `catalogue(columns)` -- the ranking is restricted to its columns (seeds and indices stay global
        columns; rows with fewer than k rankable columns are padded with -1): bit for bit the canonical ranking of the full
        image's scores over those columns, in every decode dtype, SEEDS_FROM_INPUT included."""
        import torch
        if catalogue is not None:
            self._catalogue_begin(catalogue)
            return self._recommend_catalogue(catalogue, x_positions, x_ones, seeds, k, n_rows, dtype)
        dtype = _deep_k_dtype(self._dtype_of(dtype), k, self)
        sh = self._score_shard
        self._ensure_packed(dtype, None if sh is None else sh["cols"])
        self.ctx.bind_stream()
        n_rows = self.n_batch if n_rows is None else n_rows
        if sh is not None:
            # vocabulary-sharded: local top-k over this rank's columns, one exchange, merge (sharding.ShardedRanker)
            csr = self._upload_csr(x_positions, x_ones)
            d_srp, d_sc = self._seed_csr_dev(seeds, csr)
            score, idx = self._shard_ranker(dtype).rank_batch((csr[0], csr[1], csr[2], d_srp, d_sc), k)
            if dtype == _lib.DAE_DTYPE_BF16_EXACT:
                # the exact mode's BOUND GUARD on a shard: a violation on ANY rank leaves the merged lists unproven (a column the
                # bf16 filter wrongly dropped may have been that rank's contribution) -> the ranks agree on the flag (one 4-byte
                # all-reduce per batch) and re-score the batch with the fp32 kernels together
                import torch.distributed as dist
                n_bad, col = self.ctx.exact_guard_read()
                flag = torch.tensor([1 if n_bad else 0], dtype=torch.int32)
                if dist.is_available() and dist.is_initialized() and dist.get_world_size(sh["group"]) > 1:
                    if dist.get_backend(sh["group"]) != "gloo":
                        flag = flag.to(idx.device)
                    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=sh["group"])
                if int(flag.item()):
                    self._guard_fell_back("exact_bf16 (vocabulary shard): the bound guard fired on %s: this batch is re-scored with "
                                          "the fp32 kernels on every rank"
                                          % ("this rank, e.g. column %d" % col if n_bad else "another rank"))
                    self._ensure_packed(_lib.DAE_DTYPE_F32, sh["cols"])
                    score, idx = self._shard_ranker(_lib.DAE_DTYPE_F32).rank_batch((csr[0], csr[1], csr[2], d_srp, d_sc), k)
            r0, r1 = self.owned_rows()
            n_own = max(0, min(r1, n_rows) - r0)
            res = idx[:n_own].cpu().numpy(), score[:n_own].cpu().numpy()
            self._check_feed()
            return res
        score, idx = self._submit(x_positions, x_ones, seeds, k, dtype)
        res = idx[:n_rows].cpu().numpy(), score[:n_rows].cpu().numpy()
        self._check_feed()
        if dtype == _lib.DAE_DTYPE_BF16_EXACT:
            # the exact mode's BOUND GUARD (include/dae_hip.h dae_exact_guard_read): a recomputed survivor outside the interval
            # the bf16 filter promised means the lists of this call are unproven -- the same call again on the fp32 kernels
            n_bad, col = self.ctx.exact_guard_read()
            if n_bad:
                self._guard_fell_back("exact_bf16: the bound guard fired (%d survivors, e.g. column %d): this batch is re-scored "
                                      "with the fp32 kernels" % (n_bad, col))
                return self.recommend(x_positions, x_ones, seeds, k=k, n_rows=n_rows, dtype=_lib.DAE_DTYPE_F32)
        return res

    # -- caller-given candidate columns (csrc/candidates.hip) ---------------------------------------------------------------------
    _CAND_KINDS = {"sigmoid": _lib.DAE_OUT_SCORE, "logit": _lib.DAE_OUT_LOGIT}

    def _cand_begin(self, candidates, n_rows, unique):
        """The prologue of the candidate calls.  On the host, before anything is launched: the refusal of a scoring shard and
        the range-checked CSR of the first n_rows rows' lists.  Then that CSR on the device over the launch's n_batch rows (the
        rows behind it are empty) and a zeroed status word.  -> (n_rows, host row_ptr, host col, (row_ptr, col) CUDA, status)."""
        import torch
        if self._score_shard is not None:
            raise _lib.DaeError("candidate scoring is not vocabulary-sharded: this model has a scoring shard (shard_scoring); "
                                "score candidates on a model that holds the whole decoder")
        n_rows = self.n_batch if n_rows is None else n_rows
        if n_rows > self.n_batch:
            raise ValueError("n_rows = %d exceeds the model's batch of %d" % (n_rows, self.n_batch))
        rp, col = candidates_to_csr(candidates, n_rows, self.n_input, unique=unique)
        self.sync_params()
        self.ctx.bind_stream()
        rp_b = np.full(self.n_batch + 1, rp[-1], np.int32)
        rp_b[:len(rp)] = rp
        d_rp = self._to_dev(rp_b, torch.int32)
        d_col = self._to_dev(col if col.size else np.zeros(1, np.int32), torch.int32)
        return n_rows, rp, col, (d_rp, d_col), torch.zeros(1, dtype=torch.int32, device=d_rp.device)

    def _cand_status(self, status):
        """The candidate kernels' range flag joins the feed's: checked lazily by `check_feed`, like the CSR builder's."""
        import torch
        cur = torch.cuda.current_stream(self.device_index)
        self._csr_status = (self._csr_status or []) + [(status, cur.record_event())]

    def _cand_scores(self, x_positions, x_ones, cand, n_cand, out_kind, status):
        """Enqueue encode + the candidates' chains on the current stream -> the values, a CUDA tensor in the order of the CSR."""
        import torch
        csr = self._upload_csr(x_positions, x_ones)
        out = torch.empty(max(n_cand, 1), dtype=torch.float32, device=csr[0].device)
        self.ctx.score_candidates(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"],
                                  self.weights["decoder_h"], self.biases["decoder_b"], cand, n_cand, out, out_kind=out_kind,
                                  status=status)
        self._cand_status(status)
        return out, csr

    @staticmethod
    def _cand_result(values, candidates, rp):
        """The fetched values in the caller's form: [n_rows, C] for the 2-D form, else one float32 array per row."""
        if isinstance(candidates, np.ndarray) and candidates.ndim == 2:
            out = np.full((len(rp) - 1, candidates.shape[1]), -np.inf, np.float32)
            out[:candidates.shape[0]] = values.reshape(candidates.shape)
            return out
        return [values[rp[r]:rp[r + 1]] for r in range(len(rp) - 1)]

    @staticmethod
    def _rank_result(values, columns, rp, n_rows, fill):
        """`rank_of`'s values in the caller's form: [n_rows, C] for the 2-D form (`fill` on the rows behind it), else one array
        per row."""
        if isinstance(columns, np.ndarray) and columns.ndim == 2:
            out = np.full((n_rows, columns.shape[1]), fill, values.dtype)
            out[:columns.shape[0]] = values.reshape(columns.shape)
            return out
        return [values[rp[r]:rp[r + 1]] for r in range(n_rows)]

    def score_candidates(self, x_positions, x_ones, candidates, n_rows=None, kind="sigmoid"):
        """What the model thinks of THESE columns for each playlist: `predict(...)[r][candidates[r]]` without the
        [n_batch, n_input] matrix -- per listed (row, column) the canonical fp32 chain of the dense decode, the same bits.
        candidates: a list of per-row id sequences (tracks and artists, any order, repeats allowed; ragged, possibly empty)
        -> a list of float32 arrays aligned with them; or a 2-D int array [n_rows, C] with -1 padding -> float32 [n_rows, C]
        (-inf beside a -1), so `score_candidates(feed, recommend(feed)[0])` equals `recommend(feed)[1]`.
        kind: "sigmoid" (the scores) or "logit".  An id outside -1 / [0, n_input) raises ValueError before any launch.
        Always fp32: the call is bound by the gathered decoder rows, not by the matrix units."""
        if kind not in self._CAND_KINDS:
            raise ValueError("kind %r: one of %s" % (kind, sorted(self._CAND_KINDS)))
        n_rows, rp, col, cand, status = self._cand_begin(candidates, n_rows, unique=False)
        out, _csr = self._cand_scores(x_positions, x_ones, cand, int(col.size), self._CAND_KINDS[kind], status)
        values = out.cpu().numpy()[:col.size]
        self._check_feed()
        return self._cand_result(values, candidates, rp)

    def _cand_in_catalogue(self, candidates, n_rows, catalogue):
        """The rows' candidate lists restricted to the catalogue's columns, on the host (the call de-duplicates there anyway):
        per row the sorted unique candidates that `handle.columns` holds.  Ids out of range are refused as without a catalogue."""
        if catalogue is None:
            return candidates
        self._catalogue_begin(catalogue)
        n = self.n_batch if n_rows is None else n_rows
        if n > self.n_batch:
            raise ValueError("n_rows = %d exceeds the model's batch of %d" % (n, self.n_batch))
        rp, col = candidates_to_csr(candidates, n, self.n_input, unique=True)
        keep = np.isin(col, catalogue.columns)
        return [col[rp[r]:rp[r + 1]][keep[rp[r]:rp[r + 1]]] for r in range(len(rp) - 1)]

    def rank_candidates(self, x_positions, x_ones, candidates, seeds, k=500, n_rows=None, catalogue=None):
        """`recommend` restricted to the caller's candidates: per row the k best of its candidate columns (each once, however
        often it is listed; seeds removed), logit descending then column ascending -> (idx [n_rows, k] int32 with -1 padding,
        score [n_rows, k] float32, -inf beside a -1).  seeds: as `recommend` takes them, SEEDS_FROM_INPUT included.  With
        candidates = range(n_tracks) this is `recommend`.  catalogue: a handle of `catalogue(columns)` -- only the row's
        candidates that lie in the catalogue are ranked (a row with none comes back all -1)."""
        candidates = self._cand_in_catalogue(candidates, n_rows, catalogue)
        n_rows, rp, col, cand, status = self._cand_begin(candidates, n_rows, unique=True)
        key, csr = self._cand_scores(x_positions, x_ones, cand, int(col.size), _lib.DAE_OUT_LOGIT, status)
        return self._cand_rank(cand, rp, key, seeds, csr, k, n_rows, _lib.DAE_OUT_SCORE)

    def _cand_rank(self, cand, rp, key, seeds, csr, k, n_rows, out_kind):
        import torch
        d_srp, d_sc = self._seed_csr_dev(seeds, csr)
        score = torch.empty((self.n_batch, k), dtype=torch.float32, device=key.device)
        idx = torch.empty((self.n_batch, k), dtype=torch.int32, device=key.device)
        self.ctx.rank_candidates(self.n_input, cand, key, int(np.diff(rp).max()) if len(rp) > 1 else 0, d_srp, d_sc, k, score, idx,
                                 out_kind=out_kind)
        res = idx[:n_rows].cpu().numpy(), score[:n_rows].cpu().numpy()
        self._check_feed()
        return res

    # -- exact ranks of given tracks over the whole vocabulary (csrc/rank_of.hip) --------------------------------------------------
    def rank_of(self, x_positions, x_ones, columns, seeds, n_rows=None, want_logits=False):
        """Where THESE tracks stand for each playlist among all its rankable tracks: per listed (row, column) the number of
        non-seed track columns that precede it in the canonical order (fp32 logit descending, column ascending), 0-based, so
        `rank_of(feed, recommend(feed, seeds)[0], seeds)` is `arange(k)` per row -- without the [n_batch, n_input] matrix, a sort
        and a search.  -1 for what cannot be ranked: a -1 (padding), an artist column, one of the row's seeds.
        columns: the two forms `score_candidates` takes -- a list of per-row id sequences (any order, repeats allowed; ragged,
        possibly empty) -> a list of int32 arrays aligned with them; or a 2-D int array [n_rows, C] with -1 padding -> int32
        [n_rows, C].  seeds: as `recommend` takes them, SEEDS_FROM_INPUT included.  want_logits: -> (ranks, logits), the
        canonical fp32 logits in the same form (-inf beside a rank of -1).  An id outside -1 / [0, n_input) raises ValueError
        before any launch; a model with a scoring shard refuses like the candidate calls.
        Always fp32, whatever the model's decode dtype: the ranks describe the canonical fp32 logits, the order an fp32 or
        exact_bf16 `recommend` lists by; a bf16 list may differ from them in its tail."""
        import torch
        n_rows, rp, col, ans, status = self._cand_begin(columns, n_rows, unique=False)
        self._ensure_packed(_lib.DAE_DTYPE_F32)
        self.ctx.bind_stream()
        csr = self._upload_csr(x_positions, x_ones)
        d_srp, d_sc = self._seed_csr_dev(seeds, csr)
        n = int(col.size)
        rank = torch.empty(max(n, 1), dtype=torch.int32, device=csr[0].device)
        logit = torch.empty(max(n, 1), dtype=torch.float32, device=csr[0].device) if want_logits else None
        self.ctx.score_rank_of(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"],
                               self.weights["decoder_h"], self.biases["decoder_b"], self.n_tracks, d_srp, d_sc, ans, n, rank,
                               out_logit=logit, status=status)
        self._cand_status(status)
        ranks = rank.cpu().numpy()[:n]
        logits = logit.cpu().numpy()[:n] if want_logits else None
        self._check_feed()

        def shaped(values, fill):
            return self._rank_result(values, columns, rp, n_rows, fill)

        if want_logits:
            return shaped(ranks, -1), shaped(logits, -np.inf)
        return shaped(ranks, -1)

    def recommend_iter(self, feeds, k=500, dtype=None, want_scores=True, catalogue=None):
        """`recommend` over a stream of batches (`_recommend_iter`).  k <= 1024: the pipeline behind the loop keeps that limit, and a
        larger k raises ValueError here, before a pipeline is created.
        catalogue: a handle of `catalogue(columns)` -- every feed gets what `recommend(feed, catalogue=handle)` returns for it
        alone, bit for bit, from a pipeline in catalogue mode (dae_pipeline_set_catalogue); feeds the pipeline
        does not take go through that call, in order."""
        _refuse_deep_k(k, "recommend_iter")
        if catalogue is not None:
            self._catalogue_begin(catalogue)
        return self._recommend_iter(feeds, k, dtype, want_scores, catalogue)

    def _recommend_iter(self, feeds, k, dtype, want_scores, catalogue=None):
        """`recommend` over a stream of batches with the host and the device overlapped (the loop of
        main_challenge.py:72-93 / main_train.py:62-96): `feeds` yields (x_positions, x_ones, seeds, n_rows) (DAE_title:
        + titles, titles_use); the generator yields (idx [n_rows,k], score [n_rows,k] or None) in order, one pair per feed.
        The loop itself is the library's (`dae_pipeline_*`, csrc/pipeline.hip + pipeline_issue.hip): consecutive feeds are scored in
        ONE launch of up to 1024 rows (2048 in the bf16 modes; `_coalesce_count`: the reference's batches of 150 / 250 rows
        pad to 256 alone), three library contexts take the launches in turn, the CSR of launch n + 1 is built while launch n
        scores, the lists leave through the copy engine.  Rows are scored independently: every feed gets the bits
        `recommend` returns for it alone (tests/test_gpu_stream_loop.py)."""
        if self._score_shard is not None:                             # (`_catalogue_begin` has refused a catalogue here)
            for f in feeds:                                           # the exchange is a collective: no run-ahead
                x_positions, x_ones, seeds, n_rows = f[:4]
                idx, score = self.recommend(x_positions, x_ones, seeds, k=k, n_rows=n_rows, dtype=dtype)
                yield idx, (score if want_scores else None)
            return
        # THE LOOP LIVES IN THE LIBRARY (include/dae_hip.h dae_pipeline_*): stream_loop.py copies feeds in and hands views of
        # pinned result blocks out; what the pipeline does not take goes through `recommend` feed by feed, in order.
        if self.device_csr:
            yield from self._stream(feeds, k, self._dtype_of(dtype), want_scores, catalogue=catalogue)
            return
        for f in feeds:                  # (device_csr = False: host-built CSRs -- the per-batch call)
            idx, score = self._recommend_feed(f, k, dtype, catalogue)
            yield idx, (score if want_scores else None)

    def evaluate_iter(self, feeds, k=500, dtype=None, catalogue=None):
        """The evaluation loop with the metrics computed on the device (`_evaluate_iter`).  k <= 1024 (the pipeline and the metrics
        kernel): a larger k raises ValueError here, before a pipeline is created.
        catalogue: a handle of `catalogue(columns)` -- the records are those of `recommend(feed, catalogue=handle)`'s lists.  The
        metrics see global columns (they run after the lists have been mapped back): an answer OUTSIDE the catalogue can never be
        hit and counts in the denominators, exactly as a -1 answer does.  A caller who wants recall within the catalogue filters
        the answers on the host before feeding them."""
        _refuse_deep_k(k, "evaluate_iter")
        if catalogue is not None:
            self._catalogue_begin(catalogue)
        return self._evaluate_iter(feeds, k, dtype, catalogue)

    def _evaluate_iter(self, feeds, k, dtype, catalogue=None):
        """The evaluation loop (main_train.py:48-100) with the metrics computed on the device: `feeds` yields
        (feed, answers) -- `feed` what `recommend_iter` takes, `answers` one id list per row of the feed (the reader's
        `test_answer`: ints, -1 and duplicates allowed) -- and the generator yields, per feed and in order, the rows' records
        (a numpy array of utils/metrics.py RECORD_DTYPE: hits_r, first, m, n_answer, dcg; `finish_*` there turn a record into
        r-precision, NDCG and clicks, bit for bit what get_r_precision / get_ndcg / get_rsc return for the row's list).
        Where `recommend_iter` runs on the library's pipeline, this does too, in its evaluation mode: the
        answers go up with the feed, dae_rank_metrics runs behind the scoring call and 24 bytes a row come back instead of
        the row's k indices.  Every other case (a vocabulary-sharded model, device_csr = False, explicit seed lists, a feed
        or its answers larger than a launch slot) goes feed by feed through `recommend` and `metrics.rank_records`."""
        if self._score_shard is None and self.device_csr:
            yield from self._stream(feeds, k, self._dtype_of(dtype), False, eval_mode=True, catalogue=catalogue)
            return
        from ..utils.metrics import rank_records
        for f, answers in feeds:
            yield rank_records(self._recommend_feed(f, k, dtype, catalogue)[0], answers)

    # -- the candidate calls over a stream of feeds (the pipeline's candidates mode: DESIGN.md 4b, 7) ---------------------------------
    cand_launch_ids = 1 << 21         # candidate ids one launch of the streamed candidate loops holds (a feed with more: per batch)

    def _cand_iter_begin(self, what, catalogue):
        """What the streamed candidate calls refuse before a pipeline is created."""
        if catalogue is not None:
            raise ValueError("%s: candidates inside a catalogue are not streamed (call it without catalogue=; "
                             "`rank_candidates(..., catalogue=)` takes one per batch)" % what)
        if self._score_shard is not None:
            raise _lib.DaeError("candidate scoring is not vocabulary-sharded: this model has a scoring shard (shard_scoring); "
                                "score candidates on a model that holds the whole decoder")

    def _title_kw(self, f):
        return {"titles": f[4], "titles_use": f[5] if len(f) > 5 else None} if len(f) > 4 and isinstance(self, DAE_title) else {}

    def score_candidates_iter(self, feeds, kind="sigmoid", catalogue=None):
        """`score_candidates` over a stream: `feeds` yields (feed, candidates) -- `feed` what `recommend_iter` takes (its seeds are
        not used), `candidates` what `score_candidates` takes -- and the generator yields, per feed and in order, what
        `score_candidates` returns for that feed alone: same containers, same bits (tests/test_gpu_candidates_loop.py).  The loop
        is the library's (the pipeline's candidates mode): the ids are staged and uploaded with the feed, consecutive
        feeds share a launch, nothing is synchronised per feed; a 2-D candidate array reaches the staging copy without a pass over
        its rows.  A feed the pipeline does not take (device_csr = False, more rows / entries / ids than a launch slot:
        `cand_launch_ids`) goes through `score_candidates`, in order.  An id outside -1 / [0, n_input) raises ValueError at its
        feed (those before it have been yielded).  catalogue= is refused: not built."""
        if kind not in self._CAND_KINDS:
            raise ValueError("kind %r: one of %s" % (kind, sorted(self._CAND_KINDS)))
        self._cand_iter_begin("score_candidates_iter", catalogue)

        def per_batch(f, cands):
            return self.score_candidates(f[0], f[1], cands, n_rows=f[3], kind=kind, **self._title_kw(f))
        return self._candidates_iter(feeds, False, self._CAND_KINDS[kind], 1, False, per_batch)

    def rank_candidates_iter(self, feeds, k=500, want_scores=True, catalogue=None):
        """`rank_candidates` over a stream (see `score_candidates_iter`): per feed, in order, (idx [n_rows, k], score [n_rows, k] or
        None) as `rank_candidates` returns them for that feed alone.  The rows' repeated candidates are dropped on the device
        (dae_candidates_unique), not by a pass over the lists here.  k <= 1024, the pipeline's limit: a larger k raises ValueError
        before a pipeline is created.  Feeds with explicit seed lists go through `rank_candidates`, in order."""
        if k > _lib.DAE_MAX_K:
            raise ValueError("rank_candidates_iter takes k <= %d, the pipeline's limit (got %d): deeper lists come from "
                             "`rank_candidates` per batch, k <= %d" % (_lib.DAE_MAX_K, k, _lib.DAE_MAX_K_DEEP))
        self._cand_iter_begin("rank_candidates_iter", catalogue)

        def per_batch(f, cands):
            idx, score = self.rank_candidates(f[0], f[1], cands, f[2], k=k, n_rows=f[3], **self._title_kw(f))
            return idx, (score if want_scores else None)
        return self._candidates_iter(feeds, True, _lib.DAE_OUT_SCORE, k, want_scores, per_batch)

    def _candidates_iter(self, feeds, rank, out_kind, k, want_scores, per_batch):
        if not self.device_csr:          # (host-built CSRs: the per-batch call)
            for f, cands in feeds:
                yield per_batch(f, cands)
            return
        self.sync_params()               # (the pipeline reads the weights, a titled one copies the title variables: current ones)
        cand = (bool(rank), int(out_kind), int(self.cand_launch_ids))
        key, pipe = stream_loop.pipeline_for(self, self._title_scorer(), _lib.DAE_DTYPE_F32, k, want_scores, candidates=cand)
        yield from stream_loop.stream_candidates(pipe, feeds, per_batch, self.n_batch, self.n_input, want_scores, self._pipes, key)

    def _recommend_feed(self, f, k, dtype, catalogue=None):
        """`recommend` of one feed of a loop.  Only a DAE_title takes the title items of a 5- or 6-item feed; a plain DAE scores
        the feed's first four items and ignores the rest."""
        kw = {"titles": f[4], "titles_use": f[5] if len(f) > 5 else None} if len(f) > 4 and isinstance(self, DAE_title) else {}
        if catalogue is not None:
            kw["catalogue"] = catalogue
        return self.recommend(f[0], f[1], f[2], k=k, n_rows=f[3], dtype=dtype, **kw)

    def _stream(self, feeds, k, dtype, want_scores, eval_mode=False, catalogue=None):
        """`stream_loop.stream` over this model's cached pipeline (catalogue: the one in that handle's catalogue mode)."""
        scorer = self._title_scorer()
        if scorer is not None:
            if catalogue is not None:            # (a titled exact_bf16 pipeline is refused inside a catalogue: fp32, said once)
                dtype = catalogue._title_dtype(dtype)
            dtype = _title_dtype(dtype, self)
        key, pipe = stream_loop.pipeline_for(self, scorer, dtype, k, want_scores, eval_mode, catalogue)

        def on_guard(n_fb):
            self._guard_fell_back("exact_bf16: the bound guard fired in %d launch(es) of the streamed loop: they were re-scored "
                                  "with the fp32 kernels" % n_fb, n_fb)
        return stream_loop.stream(pipe, feeds, lambda f: self._recommend_feed(f, k, dtype, catalogue), self.n_batch, want_scores, eval_mode,
                                  isinstance(self, DAE_title), on_guard if dtype == _lib.DAE_DTYPE_BF16_EXACT else None,
                                  self._pipes, key)

    def close_pipelines(self):
        """Close and forget the cached pipelines: the next streamed loop creates its own (e.g. after `n_lanes` changed)."""
        for _gen, pipe in self._pipes.values():
            pipe.close()
        self._pipes.clear()

    def _coalesce_count(self, dtype=None):
        """Feeds per launch of the streamed loop.  fp32 decode (the device is the limit): the count (<= 8, <= 1024 rows)
        that wastes the fewest padded rows of the 128-row groups the decode works in; more feeds on a tie.  150 -> 5
        (750 of 768 rows), 250 -> 4 (1000 of 1024), 256 -> 4, batches of >= 512 rows stay alone.  bf16 / exact_bf16
        (the host is the limit: ~0.3 ms of Python per launch against 0.2 ms of kernels for 1 024 rows): as many feeds
        as fit 2 048 rows, at most 8 (150 -> 8: 2.4 -> 3.3 M playlists/s).  `model.coalesce = n` overrides."""
        if self.coalesce:
            return max(1, int(self.coalesce))
        nb = self.n_batch
        if dtype is not None and dtype != _lib.DAE_DTYPE_F32:
            return max(1, min(8, 2048 // nb))
        best, best_eff = 1, 0.0
        for m in range(1, 9):
            if m > 1 and m * nb > 1024:
                break
            eff = m * nb / float(-(-m * nb // 128) * 128)
            if eff >= best_eff - 1e-9:
                best, best_eff = m, max(eff, best_eff)
        return best

    def train_step(self, x_positions, x_ones, y_positions, y_ones, keep_prob, input_keep_prob, fetch_cost=True):
        """sess.run([model.optimizer, model.cost], ...) (main_train.py:204-213) -> cost (float).
        `fetch_cost=False` returns the cost as a 0-dim DEVICE tensor and does not wait for the step: the host
        builds the next batch while this one runs (main_train accumulates the tensor and fetches it once per
        epoch); the feed's range flag is then checked by the next fetching call or `check_feed()`."""
        import torch
        self.ctx.bind_stream()
        if self._sharded is not None:
            x = self._upload_csr(x_positions, x_ones)
            y = self._upload_csr(y_positions, y_ones)
            self._params_stale = True
            cost = self._sharded.train_step(x, y, keep_prob, input_keep_prob, fetch_cost=fetch_cost)
            if fetch_cost:
                self._check_feed()
            return cost
        x = self._upload_csr(x_positions, x_ones, side_stream=True)
        y = self._upload_csr(y_positions, y_ones, side_stream=True)
        return self._train_step_csr(x, y, keep_prob, input_keep_prob, fetch_cost)

    def _train_step_csr(self, x, y, keep_prob, input_keep_prob, fetch_cost):
        """One Adam step on the device CSRs x, y = (row_ptr, col, val) of a batch, whichever feed built them (`train_step`:
        the host's COO through dae_coo_to_csr; `train_step_draw`: dae_train_batch).  -> the cost, as `train_step` returns it."""
        import torch
        dev = self.weights["encoder_h"].device
        if self._adam is None:
            self._grads = {}
            self._adam = {}
            names = ["encoder_h", "encoder_b", "decoder_b"] + ([] if self.tied else ["decoder_h"])
            for n in names:
                p = self.weights[n] if n in self.weights else self.biases[n]
                self._grads[n] = torch.zeros_like(p)
                self._adam[n] = (torch.zeros_like(p), torch.zeros_like(p))
            self._cost = torch.zeros(1, dtype=torch.float32, device=dev)
        (xr, xc, xv), (yr, yc, yv) = x, y
        seed = int(self._rng.randint(0, 2 ** 31 - 1))
        g = self._grads
        lib, ctx = self.ctx.lib, self.ctx
        P = _lib._ptr
        lz = None
        if not self.tied and self.reg_lambda == 0.0 and self.encoder_adam == "rows":
            if self._lazy is None:
                self._lazy = {"state": torch.zeros(2 * self.n_input, dtype=torch.int32, device=dev),
                              "tab": torch.zeros(max(8, int(self.rows_adam_table)), dtype=torch.float32, device=dev),
                              "flushed": self._step}
                ctx.check(lib.dae_set_enc_grad_prezeroed(ctx.h, 1))
            lz = self._lazy
            if self._step + 2 >= lz["tab"].numel():                       # alpha of every step so far
                lz["tab"] = torch.cat([lz["tab"], torch.zeros_like(lz["tab"])])
            # the rows this step's input names (the CSR's column array, length read on the device from row_ptr[B])
            # become current BEFORE the encode reads them
            rows_arg = (P(xc), ctypes.c_void_p(xr.data_ptr() + 4 * self.n_batch), int(xc.numel()))
            m_e, v_e = self._adam["encoder_h"]
            ctx.check(lib.dae_adam_rows_begin(ctx.h, P(self.weights["encoder_h"]), P(m_e), P(v_e), P(lz["state"]),
                                              P(lz["tab"]), lz["tab"].numel(), self.n_input, self.n_hidden,
                                              rows_arg[0], rows_arg[1], rows_arg[2], 0.9, 0.999, 1e-8, self._step + 1))
        # untied, reg_lambda == 0, hidden a multiple of 128: the dense Adam update of W_dec is applied inside the
        # decoder-gradient kernel (bit-identical parameters; the gradient never reaches memory)
        fuse_dec = (not self.tied and self.reg_lambda == 0.0 and self.n_hidden % 128 == 0
                    and self.decoder_adam == "fused")
        if fuse_dec:
            m_d, v_d = self._adam["decoder_h"]
            ctx.check(lib.dae_arm_decoder_adam(ctx.h, P(m_d), P(v_d), self.learning_rate, 0.9, 0.999, 1e-8,
                                               self._step + 1))
        ctx.check(lib.dae_train_forward_backward(
            ctx.h, P(xr), P(xc), P(xv), P(yr), P(yc), P(yv),
            P(self.weights["encoder_h"]), P(self.biases["encoder_b"]),
            P(self.weights["decoder_h"]), P(self.biases["decoder_b"]),
            self.n_input, self.n_hidden, self.n_batch, self.n_batch, 1 if self.tied else 0,
            float(input_keep_prob), float(keep_prob), seed, float(self.reg_lambda),
            P(g["encoder_h"]), P(g["encoder_b"]),
            P(g["decoder_h"]) if not self.tied else None, P(g["decoder_b"]), P(self._cost)))
        self._step += 1
        for n, grad in g.items():
            p = self.weights[n] if n in self.weights else self.biases[n]
            m, v = self._adam[n]
            if fuse_dec and n == "decoder_h":
                continue
            if lz is not None and n == "encoder_h":
                ctx.check(lib.dae_adam_rows_apply(ctx.h, P(p), P(m), P(v), P(grad), P(lz["state"]), P(lz["tab"]),
                                                  lz["tab"].numel(), self.n_input, self.n_hidden, rows_arg[0],
                                                  rows_arg[1], rows_arg[2], self.learning_rate, 0.9, 0.999, 1e-8,
                                                  self._step))
                if self.rows_adam_flush_every > 0 and self._step - lz["flushed"] >= self.rows_adam_flush_every:
                    self._flush_rows_adam()
                continue
            ctx.check(lib.dae_adam_step(ctx.h, P(p), P(m), P(v), P(grad), p.numel(),
                                        self.learning_rate, 0.9, 0.999, 1e-8, self._step))
        self._mark_dirty()
        if not fetch_cost:
            return self._cost[0].clone()
        cost = float(self._cost.item())
        self._check_feed()
        return cost

    # -- the device feed (csrc/train_feed.hip; DESIGN.md "The training feed") ---------------------------------------
    def attach_train_set(self, reader):
        """Keep `reader`'s training set on the device for `train_step_draw`: its flat id arrays and offsets are copied
        once (dae_train_set_create, which refuses ids outside their ranges).  Once per model, after fit().  A
        vocabulary-sharded model holds the set on every rank: the batch is replicated, only the vocabulary rows are
        sharded."""
        if self._train_feed is not None:
            raise _lib.DaeError("attach_train_set: this model already holds a training set")
        feed = {"reader": reader, "set": None,
                "trk_len": np.diff(reader._trk_off), "art_len": np.diff(reader._art_off)}
        if self._takes_device_feed():
            feed["set"] = _lib.TrainSet(self.ctx, reader._trk, reader._trk_off, reader._art, reader._art_off,
                                        reader.num_tracks, reader.num_items)
        self._train_feed = feed

    def _takes_device_feed(self):
        return True

    def _host_feed_step(self, draw, x_side, keep_prob, input_keep_prob, fetch_cost):
        """`train_step` on the host feed rebuilt from the draw: same batches, same results, nothing sped up."""
        from ..utils.data_reader import feed_from_draw
        x_pos, x_val, y_pos = feed_from_draw(self._train_feed["reader"], draw, x_side)
        return self.train_step(x_pos, x_val, y_pos, np.ones(len(y_pos), np.float32), keep_prob, input_keep_prob,
                               fetch_cost=fetch_cost)

    def train_step_draw(self, draw, x_side, keep_prob, input_keep_prob, fetch_cost=True):
        """`train_step` of the batch the reader's `next_batch_draw` names: draw int32 [3, n_batch] (playlist index, given
        tracks, given artists), x_side 0 / 1 / 2 = x is the tracks / the artists / both; y is the whole playlist.  Only the
        draw goes over the link (12 bytes a row, on the copy stream); both CSRs are built on the device from the attached
        set (dae_train_batch: two launches) and are, entry for entry, what `train_step` builds from `next_batch`'s COO -- so
        is everything after them.  A vocabulary-sharded model hands the same CSRs to its ShardedTrainer, as its `train_step`
        does (every rank draws the same batches); DAE_title has a `train_step_draw` of its own."""
        draw = self._checked_draw(draw)
        if self._train_feed["set"] is None:
            return self._host_feed_step(draw, x_side, keep_prob, input_keep_prob, fetch_cost)
        _d_draw, x, y = self._device_feed(draw, x_side)
        if self._sharded is not None:
            self._params_stale = True
            cost = self._sharded.train_step(x, y, keep_prob, input_keep_prob, fetch_cost=fetch_cost)
            if fetch_cost:
                self._check_feed()
            return cost
        return self._train_step_csr(x, y, keep_prob, input_keep_prob, fetch_cost)

    def _checked_draw(self, draw):
        if self._train_feed is None:
            raise _lib.DaeError("train_step_draw needs attach_train_set(reader) first")
        draw = np.ascontiguousarray(draw, dtype=np.int32)
        if draw.shape != (3, self.n_batch):
            raise ValueError("draw has shape %s, expected (3, %d)" % (draw.shape, self.n_batch))
        return draw

    def _device_feed(self, draw, x_side):
        """The draw uploaded and both CSRs of its batch built from the attached set (dae_train_batch) -> (d_draw, x, y); the
        feed's status word joins the pending range flags (`_check_feed`)."""
        import torch
        feed = self._train_feed
        if x_side not in (0, 1, 2):
            raise ValueError("x_side %r: 0 tracks, 1 artists, 2 both" % (x_side,))
        self.ctx.bind_stream()
        # room of the outputs: the playlists' lengths bound the kept entries of a side (an index out of range is the device's
        # to flag: its row is empty)
        idx = np.clip(draw[0], 0, len(feed["trk_len"]) - 1)
        n_trk, n_art = int(feed["trk_len"][idx].sum()), int(feed["art_len"][idx].sum())
        x_cap = (n_trk, n_art, n_trk + n_art)[x_side]
        d_draw = self._to_dev(draw, torch.int32, side_stream=True)
        x, y, status = self.ctx.train_batch(feed["set"], d_draw, x_side, x_cap, n_trk + n_art)
        cur = torch.cuda.current_stream(self.device_index)
        pending = (self._csr_status or []) + [(status, cur.record_event())]
        if len(pending) > 64:                                   # un-fetched training steps: fold on the device
            pending = [(self._fold_status(pending), cur.record_event())]
        self._csr_status = pending
        return d_draw, x, y

    # -- persistence ----------------------------------------------------------------------------------
    def get_params(self):
        """sess.run(model.d_params): [enc_W, dec_W (enc_W again when tied), enc_b, dec_b]."""
        self.sync_params()
        return [p.detach().cpu().numpy() for p in self.d_params]

    def save_model(self, sess=None):
        """DAEs.py:107-111: pickle of the four float32 arrays in d_params order."""
        with open(self.save_dir, "wb") as f:
            pickle.dump(self.get_params(), f)


class DAE(DAE_tied):
    """Untied DAE, optionally initialised from a pretrain pickle (reference DAEs.py:114-150)."""

    tied = False

    def __init__(self, conf):
        DAE_tied.__init__(self, conf)
        self.initval_dir = conf.initval               # DAEs.py:117

    def _host_init(self):
        if str(self.initval_dir).endswith("NULL"):    # DAEs.py:120 (Conf joins the dir in front)
            rng = np.random.default_rng(self.init_seed)
            return [self._xavier(rng, (self.n_input, self.n_hidden)),
                    self._xavier(rng, (self.n_input, self.n_hidden)),
                    np.zeros(self.n_hidden, np.float32), np.zeros(self.n_input, np.float32)]
        with open(self.initval_dir, "rb") as f:       # DAEs.py:130-135
            emb = pickle.load(f)
        return [np.array(emb[0], np.float32), np.array(emb[1], np.float32),
                np.array(emb[2], np.float32), np.array(emb[3], np.float32)]


class Session:
    """Minimal stand-in for tf.Session so that reference-style driver code runs unchanged:
    `sess.run(model.y_pred, feed_dict=...)`, `sess.run([model.optimizer, model.cost], ...)`, `sess.run(model.cost, ...)`,
    `sess.run(model.init_op)`, `sess.run(model.d_params)`."""

    def __init__(self, model=None):
        self.model = model
        self._loss_rng = np.random.RandomState(4321)      # seeds of `run(model.cost)`: not the model's dropout stream

    def run(self, fetches, feed_dict=None):
        m = self.model
        if m is None:
            raise ValueError("Session needs the model: Session(model)")
        feed = feed_dict or {}

        def g(ph, default=None):
            return feed.get(ph, default)

        if fetches is m.init_op:
            return None
        if fetches is m.d_params or (isinstance(fetches, list) and fetches and fetches == m.d_params):
            return m.get_params()
        if fetches is m.y_pred:
            return m.predict(g(m.x_positions), g(m.x_ones), g(m.keep_prob, 1.0),
                             g(m.input_keep_prob, 1.0))
        if fetches is m.cost or (isinstance(fetches, (list, tuple)) and len(fetches) == 1 and fetches[0] is m.cost):
            # the cost without a step (model.loss), dropout seeded from this session's own generator: fetching it never
            # changes a training run
            cost = m.loss(g(m.x_positions), g(m.x_ones), g(m.y_positions), g(m.y_ones), g(m.keep_prob, 1.0),
                          g(m.input_keep_prob, 1.0), seed=int(self._loss_rng.randint(0, 2 ** 31 - 1)))
            return cost if fetches is m.cost else [cost]
        if isinstance(fetches, (list, tuple)) and len(fetches) == 2 and fetches[0] is m.optimizer \
                and fetches[1] is m.cost:
            cost = m.train_step(g(m.x_positions), g(m.x_ones), g(m.y_positions), g(m.y_ones),
                                g(m.keep_prob, 1.0), g(m.input_keep_prob, 1.0))
            return None, cost
        raise ValueError("unsupported fetches %r" % (fetches,))


class DAE_title(DAE):
    """The challenge-time model (reference DAEs.py:153-201): a FROZEN DAE (its four arrays from `conf.DAEval`,
    :165-171) whose scores are mixed with the title scorer's,

        y = title_score * w_title + dae_score * w_playlist                                   (:180)
        x_count = row_sum(x) * input_keep_prob;  w_title = u / (u + x_count + 1e-10);  w_playlist = x_count / (same)

    with u = titles_use in {0, 1} per row (:156-162).  u = 0 gives w_playlist = 1.0f exactly, i.e. the plain
    DAE -- those batches take the fused scoring path.  With titles, `recommend` ranks the mixed score
    without either vocabulary-wide matrix (`_submit`; exact_bf16: both GEMMs in one launch per pass, csrc/mix_filter.hip) and
    the streamed loops run their titled launches on the library's pipeline; only the dense fetch of
    the protocol, `mixed_scores`, materialises the two matrices (`dae_mix_scores`)."""

    def __init__(self, conf, title_model):
        DAE.__init__(self, conf)
        self.initval_dir = conf.DAEval                    # DAEs.py:157: the frozen weights
        self.title_model = title_model
        self.title_exact_off = False      # set from outside: titled exact_bf16 launches on the fp32 kernels
        self._title_fp32_said = False     # `_title_dtype` said that this model's shapes have no exact title mix
        self._tcost = None                # train_step's cost word on the device
        self._ones_use = None             # train_step_draw's titles_use on the device
        self._title_sharded = None        # shard_title_training: the sharding.ShardedTitleTrainer the title steps go through
        self._title_stale = False         # ... and whether it has stepped since the title model's variables were refreshed
        # `_mix_guard_fired`: rows it re-scored alone; launches in a row whose rows overflowed the refine launch (two pause the
        # exact mix); titled launches left of that pause, which run on the fp32 kernels
        self._guard_row_fallbacks = self._mix_overflow_streak = self._mix_exact_pause = 0

    def _title_scorer(self):
        tm = self.title_model
        return tm if tm is not None and tm.ctx is not None else None

    def loss(self, x_positions, x_ones, y_positions, y_ones, keep_prob=1.0, input_keep_prob=1.0, seed=None, n_rows=None,
             per_row=False, titles=None, titles_use=None):
        """`DAE.loss` of the frozen DAE alone.  With titles in use it is refused by name: the loss head of the mixed score is
        another kernel (csrc/title.hip title_loss_kernel, inside the title training step only)."""
        if titles_use is not None and np.any(np.asarray(titles_use) != 0):
            raise _lib.DaeError("DAE_title.loss: not available with titles in use (titles_use != 0): the mixed-score loss head "
                                "is another kernel; without titles it is the DAE's own loss")
        if self._title_sharded is not None:
            raise _lib.DaeError("DAE_title.loss: not available on a vocabulary-sharded model (shard_title_training)")
        return DAE.loss(self, x_positions, x_ones, y_positions, y_ones, keep_prob, input_keep_prob, seed, n_rows, per_row)

    def mixed_loss(self, x_positions, x_ones, y_positions, y_ones, titles, titles_use, keep_prob=1.0, input_keep_prob=1.0,
                   title_keep_prob=1.0, seed=None, n_rows=None, per_row=False):
        """sess.run(model.cost, ...) of the title graph: the cost of a batch under the MIXED score WITHOUT a step
        (dae_mix_loss_rows) -> float, or (cost, rows) with `per_row`: rows float32 [n_rows], the loss of each row over all
        columns; cost = sum(rows) / n_batch (the title cost has no lambda term).  What `train_step` computes up to its loss:
        the frozen DAE's encode, the mixing weights and the title features with the three dropout masks a step with the same
        `seed` draws, then the mixed head on every column -- for rows, or whole batches, with titles_use = 0 as well (that is
        what the title step does: there is no dispatch to `DAE.loss`).  Always fp32, like `mixed_rank_of` (both fp32 images
        are packed for the call).  A keep probability below 1 needs an explicit seed; the model's own dropout stream is never
        drawn from, so a --title training run with calls of this in between trains the same title scorer.  Nothing of either
        model changes.  Refused by name before any upload: no fitted title scorer, no titles, a scoring shard,
        shard_title_training, n_rows > n_batch."""
        import torch
        tm = self._title_scorer()
        if tm is None:
            raise _lib.DaeError("mixed_loss: the model has no fitted title scorer (the loss of the DAE alone is `loss`)")
        if titles is None:
            raise ValueError("mixed_loss: titles are required (the loss of the DAE alone is `loss`)")
        if self._score_shard is not None:
            raise _lib.DaeError("mixed_loss: not available on a scoring shard (shard_scoring): partial costs across ranks are not "
                                "built")
        if self._title_sharded is not None:
            raise _lib.DaeError("mixed_loss: not available on a vocabulary-sharded title scorer (shard_title_training): partial "
                                "costs across ranks are not built")
        n = self.n_batch if n_rows is None else int(n_rows)
        if n < 1 or n > self.n_batch:
            raise ValueError("mixed_loss: n_rows = %d outside [1, n_batch = %d]" % (n, self.n_batch))
        if (float(keep_prob) < 1.0 or float(input_keep_prob) < 1.0 or float(title_keep_prob) < 1.0) and seed is None:
            raise ValueError("mixed_loss: a keep probability below 1 needs an explicit seed")
        seed = 0 if seed is None else int(seed)
        self._ensure_packed(_lib.DAE_DTYPE_F32)
        tm._ensure_packed(_lib.DAE_DTYPE_F32, features_table=float(title_keep_prob) == 1.0)
        self.ctx.bind_stream()
        tm.ctx.bind_stream()
        x = self._upload_csr(x_positions, x_ones, n_rows=n)
        y = self._upload_csr(y_positions, y_ones, n_rows=n)
        dev = self.weights["encoder_h"].device
        h = torch.empty((n, self.n_hidden), dtype=torch.float32, device=dev)
        self.ctx.encode(x[0], x[1], x[2], self.weights["encoder_h"], self.biases["encoder_b"], h,
                        ikp=input_keep_prob, kp=keep_prob, seed=seed)
        tu = np.ones(n, np.float32) if titles_use is None else np.asarray(titles_use, np.float32).reshape(-1)
        w_t, w_p = self._mix_weights(x, tu, input_keep_prob, seed, n_rows=n)
        feat = tm.features(titles, n, title_keep_prob, seed)
        cost = torch.empty(1, dtype=torch.float32, device=dev)
        rows = torch.empty(n, dtype=torch.float32, device=dev) if per_row else None
        tm.ctx.bind_stream()
        tm.ctx.mix_loss_rows(self.ctx, h, self.weights["decoder_h"], self.biases["decoder_b"], feat, tm.p["Output_WT"],
                             tm.p["Output_b"], w_t, w_p, self.n_batch, y, row_loss=rows, cost_out=cost)
        c = float(cost.item())
        res = (c, rows.cpu().numpy()) if per_row else c
        self._check_feed()
        return res

    # -- multi-GPU title training: the output layer's columns sharded over the ranks ----
    def shard_title_training(self, rank, world, group=None):
        """Train the title scorer through sharding.ShardedTitleTrainer: this rank owns the rows
        `sharding.shard_bounds(n_input, world, rank)` of Output_W^T and Output_b (with their Adam moments), decodes only
        those columns of the frozen DAE, and exchanges one [batch, features] all-reduce, the scalar cost and the embedding
        gradient per step; the small variables in front of the output layer are replicated.  `train_step` and
        `train_step_draw` then run that step; the title model's own variables are refreshed from the shards by
        `sync_params` (collective), which scoring and the end of an epoch call.  The trainer draws its dropout seeds from
        this model's own stream, so a sharded run draws what an unsharded one draws."""
        from ..sharding import HipTitleStages, ShardedTitleTrainer
        tm = self.title_model
        tm.check_trainable()
        self.sync_params()
        shape = dict(L=tm.input_len, n_char=tm.char_size, E=tm.embedding, filter_sizes=tm.filter_sizes, F=tm.filter_num, ld=tm.ld)
        stages = HipTitleStages(self.ctx, tm.ctx, self.weights["encoder_h"], self.biases["encoder_b"],
                                self._pack_frozen_dae, shape)
        self._title_sharded = ShardedTitleTrainer(tm.p, self.n_batch, tm.learning_rate, stages,
                                                  device=self.weights["encoder_h"].device, rank=rank, world=world,
                                                  group=group, seed=self._rng)
        self._title_stale = False

    def _pack_frozen_dae(self, lo, hi):
        """The DAE context's fp32 image holds the decoder columns [lo, hi): `_ensure_packed(cols=(lo, hi))` for the sharded
        title step, without the refresh of the title variables `sync_params` does on this class -- the DAE is frozen, and
        a step must not gather what the step before it left on the shards."""
        DAE.sync_params(self)
        dtype, cols = _lib.DAE_DTYPE_F32, (int(lo), int(hi))
        if self._packed_dirty[dtype] or self._packed_cols.get(dtype) != cols:
            self.ctx.bind_stream()
            self.ctx.prepack_decoder(self.weights["decoder_h"], self.biases["decoder_b"], cols[0], cols[1], dtype)
            self._packed_dirty[dtype] = False
            self._packed_cols[dtype] = cols

    def sync_params(self):
        """`DAE.sync_params`, and -- collective when the title training is sharded -- the title model's variables
        refreshed from the shards when a step has run since the last refresh."""
        DAE.sync_params(self)
        if self._title_sharded is not None and self._title_stale:
            self._title_stale = False
            self.title_model.ctx.bind_stream()
            self._title_sharded.sync_title_params(self.title_model)

    def _stream(self, feeds, k, dtype, want_scores, eval_mode=False, catalogue=None):
        self.sync_params()            # (the pipeline copies the title variables: current ones)
        return DAE._stream(self, feeds, k, dtype, want_scores, eval_mode, catalogue)

    def _row_sums(self, x_positions, x_ones):
        rp, _c, v = coo_to_csr(x_positions, x_ones, self.n_batch, self.n_input)
        rows = np.repeat(np.arange(self.n_batch), np.diff(rp))
        return np.bincount(rows, weights=v.astype(np.float64), minlength=self.n_batch).astype(np.float32)

    def _mix_weights(self, csr, titles_use, input_keep_prob=1.0, seed=0, n_rows=None):
        """DAEs.py:159-162 on the device: x_count = row_sum(x) * input_keep_prob; w_title = u / (u + x_count + 1e-10),
        w_playlist = x_count / (same) -- fp32 operations in the reference's order.  -> (w_title, w_playlist) [n_batch]."""
        import torch
        rp, c, v = csr
        dev = rp.device
        nb = n_rows or self.n_batch
        P = _lib._ptr
        u = np.zeros(nb, np.float32)
        tu = np.asarray(titles_use, np.float32).reshape(-1)
        u[:len(tu)] = tu[:nb]
        u = self._to_dev(u, torch.float32)
        w_t = torch.empty(nb, dtype=torch.float32, device=dev)
        w_p = torch.empty(nb, dtype=torch.float32, device=dev)
        # one launch (dae_mix_weights: the row sums of dae_row_sums and the four elementwise operations behind them)
        self.ctx.check(self.ctx.lib.dae_mix_weights(self.ctx.h, P(rp), P(c), P(v), nb, float(input_keep_prob), int(seed),
                                                    P(u), P(w_t), P(w_p)))
        return w_t, w_p

    def mixed_scores(self, x_positions, x_ones, titles, titles_use, input_keep_prob=1.0, title_keep_prob=1.0,
                     seed=0):
        """sess.run(model.y_pred, ...) of the title graph: dense mixed scores [n_batch, n_input] (CUDA tensor).  The
        dense fetch of the protocol; `recommend` never builds these matrices."""
        import torch
        self._ensure_packed()
        self.ctx.bind_stream()
        csr = self._upload_csr(x_positions, x_ones)
        h = torch.empty((self.n_batch, self.n_hidden), dtype=torch.float32, device=self.weights["encoder_h"].device)
        self.ctx.encode(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"], h,
                        ikp=input_keep_prob, kp=1.0, seed=seed)
        y = torch.empty((self.n_batch, self.n_input), dtype=torch.float32, device=h.device)
        self.ctx.decode_dense(h, y, apply_sigmoid=True)
        ts = self.title_model.score(titles, self.n_batch, title_keep_prob, seed)
        w_t, w_p = self._mix_weights(csr, titles_use, input_keep_prob, seed)
        self.ctx.bind_stream()
        P = _lib._ptr
        self.ctx.check(self.ctx.lib.dae_mix_scores(self.ctx.h, P(ts), int(ts.stride(0)), P(y), int(y.stride(0)),
                                                   P(w_t), P(w_p), self.n_batch, self.n_input))
        return y

    def train_step(self, x_positions, x_ones, y_positions, y_ones, keep_prob, input_keep_prob, titles=None,
                   titles_use=None, title_keep_prob=1.0, fetch_cost=True):
        """sess.run([model.optimizer, model.cost], ...) of the title graph (main_train.py:214-221): one Adam step
        on the title variables; the DAE arrays stay as loaded.  Returns the cost; `fetch_cost=False` as in
        `DAE_tied.train_step`: a 0-dim DEVICE tensor, no wait for the step."""
        import torch
        if titles is None:
            raise ValueError("DAE_title trains the title scorer: titles are required")
        tm = self.title_model
        tm.check_trainable(self.n_batch)
        self.ctx.bind_stream()
        dev = self.weights["encoder_h"].device
        x = self._upload_csr(x_positions, x_ones)
        y = self._upload_csr(y_positions, y_ones)

        # titles_use and the title rows go up where the step first reads them, as they always did: a pageable copy blocks
        # the host until the stream reaches it, and behind the DAE forward's launches that wait costs nothing -- in front
        # of them the device would sit idle meanwhile (measured: profiles/title_feed_notes.md)
        def use():
            u = torch.zeros(self.n_batch, dtype=torch.float32, device=dev)
            tu = np.ones(self.n_batch, np.float32) if titles_use is None else np.asarray(titles_use, np.float32).reshape(-1)
            u[:min(len(tu), self.n_batch)] = torch.from_numpy(tu[:self.n_batch]).to(dev)
            return u
        return self._title_step_csr(x, y, lambda: tm.titles_to_device(titles, self.n_batch), use, keep_prob, input_keep_prob,
                                    title_keep_prob, fetch_cost)

    def _title_step_csr(self, x, y, d_titles, d_use, keep_prob, input_keep_prob, title_keep_prob, fetch_cost):
        """One Adam step on the title variables from what already lies on the device, whichever feed put it there
        (`train_step`: the host's COO and title lists; `train_step_draw`: dae_train_batch and dae_train_titles):
        x, y = (row_ptr, col, val) CSRs of the batch, d_titles int32 [n_batch, strmaxlen], d_use float32 [n_batch]
        (titles_use) -- device tensors, or (the host feed) functions that upload them, called where the step first reads
        them.  -> the cost, as `train_step` returns it."""
        import torch
        tm = self.title_model                 # (its shape limits were checked by the caller, before its uploads)
        if self._title_sharded is not None:
            # the same step on this rank's columns (sharding.ShardedTitleTrainer); the title model's own variables go stale
            u = d_use() if callable(d_use) else d_use
            d_titles = d_titles() if callable(d_titles) else d_titles
            cost = self._title_sharded.train_step(x, y, d_titles, u, keep_prob, input_keep_prob, title_keep_prob,
                                                  fetch_cost=fetch_cost)
            self._title_stale = True
            if fetch_cost:
                self._check_feed()
            return cost
        seed = int(self._rng.randint(0, 2 ** 31 - 1))
        self._ensure_packed()
        self.ctx.bind_stream()
        tm.ctx.bind_stream()
        dev = self.weights["encoder_h"].device
        (xr, xc, xv), (yr, yc, yv) = x, y
        # frozen DAE forward with its dropouts (model.keep_prob = conf.kp, input_keep_prob; main_train.py:219-220)
        h = torch.empty((self.n_batch, self.n_hidden), dtype=torch.float32, device=dev)
        self.ctx.encode(xr, xc, xv, self.weights["encoder_h"], self.biases["encoder_b"], h,
                        ikp=input_keep_prob, kp=keep_prob, seed=seed)
        dae = torch.empty((self.n_batch, self.n_input), dtype=torch.float32, device=dev)
        self.ctx.decode_dense(h, dae, apply_sigmoid=True)
        # mixing weights (DAEs.py:159-162) from the dropped-out row sums
        s = torch.empty(self.n_batch, dtype=torch.float32, device=dev)
        P = _lib._ptr
        self.ctx.check(self.ctx.lib.dae_row_sums(self.ctx.h, P(xr), P(xc), P(xv), self.n_batch,
                                                 float(input_keep_prob), seed, P(s)))
        u = d_use() if callable(d_use) else d_use
        x_count = s * float(np.float32(input_keep_prob))
        deno = u + x_count + 1e-10
        w_t, w_p = (u / deno).contiguous(), (x_count / deno).contiguous()
        # title forward, keeping what the backward pass needs
        tm._ensure_packed(features_table=False)
        d_titles = d_titles() if callable(d_titles) else d_titles
        feat, d_titles, arg, raw = tm.features(d_titles, self.n_batch, title_keep_prob, seed, keep_for_backward=True)
        zt = torch.empty((self.n_batch, self.n_input), dtype=torch.float32, device=dev)
        tm.ctx.decode_dense(feat, zt, apply_sigmoid=False)
        if self._tcost is None:
            self._tcost = torch.zeros(1, dtype=torch.float32, device=dev)
        tm.backward_and_step(feat, d_titles, arg, raw, zt, dae, (yr, yc, yv), w_t, w_p, self.n_batch,
                             title_keep_prob, seed, self._tcost)
        if not fetch_cost:
            return self._tcost[0].clone()
        cost = float(self._tcost.item())
        self._check_feed()
        return cost

    def attach_train_set(self, reader):
        """`DAE_tied.attach_train_set`, and the reader's title rows join the set (dae_train_set_attach_titles: 4 x strmaxlen
        bytes a playlist): a title step is then named by its draw alone."""
        DAE.attach_train_set(self, reader)
        ts = self._train_feed["set"]
        try:
            n, L = ts.n_playlists, self.title_model.input_len
            ts.attach_titles(np.asarray(reader._titles, np.int32).reshape(n, L), self.title_model.char_size)
        except Exception:
            ts.close()
            self._train_feed = None
            raise
        self._ones_use = None         # the device feed's titles_use: all ones, made once

    def train_step_draw(self, draw, x_side, keep_prob, input_keep_prob, fetch_cost=True, title_keep_prob=1.0):
        """The title step of the batch a draw names (`DAE_tied.train_step_draw`): the draw is uploaded, both CSRs and the
        title rows come out of the attached set (dae_train_batch, dae_train_titles), titles_use is 1 for every row
        (main_train.py:221), and `_title_step_csr` does what `train_step` does behind its uploads -- for any draw the step
        `_host_feed_step` runs from the host's rebuild of the same batch."""
        import torch
        draw = self._checked_draw(draw)
        ts = self._train_feed["set"]
        if ts is None or not ts.has_titles:
            return self._host_feed_step(draw, x_side, keep_prob, input_keep_prob, fetch_cost, title_keep_prob)
        self.title_model.check_trainable(self.n_batch)
        d_draw, x, y = self._device_feed(draw, x_side)
        d_titles = self.ctx.train_titles(ts, d_draw)
        if self._ones_use is None:
            self._ones_use = torch.ones(self.n_batch, dtype=torch.float32, device=d_draw.device)
        return self._title_step_csr(x, y, d_titles, self._ones_use, keep_prob, input_keep_prob, title_keep_prob, fetch_cost)

    def _host_feed_step(self, draw, x_side, keep_prob, input_keep_prob, fetch_cost, title_keep_prob=1.0):
        """The title step of the batch a draw names, the feed AND the titles rebuilt on the host from the attached reader:
        what `train_step_draw` computes, through `train_step`'s uploads (the fallback for a set without titles)."""
        from ..utils.data_reader import feed_from_draw
        reader = self._train_feed["reader"]
        x_pos, x_val, y_pos = feed_from_draw(reader, draw, x_side)
        return self.train_step(x_pos, x_val, y_pos, np.ones(len(y_pos), np.float32), keep_prob, input_keep_prob,
                               titles=[reader._title(int(i)) for i in draw[0]],
                               titles_use=np.ones(self.n_batch, np.float32), title_keep_prob=title_keep_prob,
                               fetch_cost=fetch_cost)

    def _submit(self, x_positions, x_ones, seeds, k, dtype, titles=None, titles_use=None, n_rows=None):
        """One batch enqueued, nothing fetched (`n_rows`: rows of this launch when it is not the model's batch).  Without
        titles in use the mix reduces to the plain DAE (w_playlist is exactly 1.0f, App. B.6): the fused path of the base
        class.  With titles: the DAE term of the track columns goes to a transposed scratch (dae_decode_mix_term) and the
        title scorer's context runs the fused threshold path on sigmoid(z_title) * w_title + that term
        (dae_set_score_mix) -- no [batch, n_input] matrix of either."""
        if titles is None or titles_use is None or not np.any(np.asarray(titles_use)):
            return DAE._submit(self, x_positions, x_ones, seeds, k, dtype, n_rows=n_rows)
        import torch
        tm = self.title_model
        tm.ctx.bind_stream()
        dtype = _title_dtype(dtype, self)
        if dtype == _lib.DAE_DTYPE_BF16_EXACT and self._mix_exact_pause > 0:
            # rows of this model keep overflowing the refine launch's candidate buffers (a flat DAE bias: no prior for the
            # threshold sample): the exact launches are paused for a while instead of being run and re-scored every time
            self._mix_exact_pause -= 1
            self._ensure_packed(_lib.DAE_DTYPE_F32)
            tm._ensure_packed(_lib.DAE_DTYPE_F32)
            dtype = _lib.DAE_DTYPE_F32
        nb = n_rows or self.n_batch
        dev = self.weights["encoder_h"].device
        # (Measured and not kept: the launch's two independent preambles -- CSR build / encode / seeds / mixing weights, and the
        # title features -- on streams of their own, joined before dae_mix_topk_exact: 1.12 - 1.17 M playlists/s against
        # 1.22 M without.  The loop is bound by the host's ~0.6 ms per launch, and the fork adds events and stream switches.)
        csr = self._upload_csr(x_positions, x_ones, n_rows=nb)
        h = torch.empty((nb, self.n_hidden), dtype=torch.float32, device=dev)
        self.ctx.encode(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"], h)
        w_t, w_p = self._mix_weights(csr, titles_use, n_rows=nb)
        feat = tm.features(titles, nb)
        d_srp, d_sc = self._seed_csr_dev(seeds, csr, n_rows=nb)
        score = torch.empty((nb, k), dtype=torch.float32, device=dev)
        idx = torch.empty((nb, k), dtype=torch.int32, device=dev)
        if dtype == _lib.DAE_DTYPE_BF16_EXACT:
            # both GEMMs on bf16 operands in one launch per pass, the survivors recomputed in fp32 (csrc/mixexact.hip, mix_*.hip)
            gw = torch.empty(2, dtype=torch.int32, device=dev)
            tm.ctx.mix_topk_exact(self.ctx, feat, h, w_t, w_p, self.n_tracks, d_srp, d_sc, k, score, idx, guard_out=gw)
            # the guard words travel with the lists; what a re-scoring in fp32 needs, should they have moved
            idx._mix_guard = (gw, (x_positions, x_ones, seeds, titles, titles_use, n_rows))
            return score, idx
        nt32 = min((self.n_tracks + 31) // 32 * 32, self.n_input)
        y1T = torch.empty((nt32, nb), dtype=torch.float32, device=dev)
        self.ctx.decode_mix_term(h, w_p, self.n_tracks, y1T, dtype=dtype)
        tm.ctx.set_score_mix(y1T, w_t)
        try:
            tm.ctx.decode_topk(feat, self.n_tracks, d_srp, d_sc, k, score, idx, out_kind=_lib.DAE_OUT_LOGIT, dtype=dtype)
        finally:
            tm.ctx.set_score_mix()
        return score, idx

    def score_candidates_iter(self, feeds, kind="sigmoid", catalogue=None):
        """`DAE.score_candidates_iter` on a titled pipeline: feeds carry titles and titles_use, and every feed gets what this
        class's `score_candidates` returns for it -- the mixed score where titles are in use, the plain DAE's otherwise.
        kind "sigmoid" only: a stream may mix both kinds of feed, and the title mix has no logit."""
        if kind != "sigmoid":
            raise ValueError("kind %r: a titled stream scores kind = \"sigmoid\" only (the title-mixed score has no logit)" % (kind,))
        return DAE.score_candidates_iter(self, feeds, kind=kind, catalogue=catalogue)

    def _cand_mixed(self, x_positions, x_ones, titles, titles_use, cand, n_cand, status):
        """Enqueue the titled score of the listed pairs: encode, mixing weights, title features, then both chains per pair and
        `mixed_scores`' mix (dae_mix_candidates) -- no [n_batch, n_input] matrix of either scorer."""
        import torch
        tm = self.title_model
        tm.ctx.bind_stream()
        csr = self._upload_csr(x_positions, x_ones)
        h = torch.empty((self.n_batch, self.n_hidden), dtype=torch.float32, device=csr[0].device)
        self.ctx.encode(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"], h)
        w_t, w_p = self._mix_weights(csr, titles_use)
        feat = tm.features(titles, self.n_batch)
        out = torch.empty(max(n_cand, 1), dtype=torch.float32, device=h.device)
        tm.ctx.mix_candidates(self.ctx, h, self.weights["decoder_h"], self.biases["decoder_b"], feat, tm.p["Output_WT"],
                              tm.p["Output_b"], w_t, w_p, cand, n_cand, out, status=status)
        self._cand_status(status)
        return out, csr

    def score_candidates(self, x_positions, x_ones, candidates, n_rows=None, kind="sigmoid", titles=None, titles_use=None):
        """`DAE.score_candidates`; with titles in use the MIXED score of the listed pairs, `mixed_scores(...)[r][candidates[r]]`
        bit for bit (kind "sigmoid" only: the mix has no logit).  Without titles in use: the base class's call."""
        if titles is None or titles_use is None or not np.any(np.asarray(titles_use)):
            return DAE.score_candidates(self, x_positions, x_ones, candidates, n_rows=n_rows, kind=kind)
        if kind != "sigmoid":
            raise ValueError("kind %r: the title-mixed score has no logit; use kind = \"sigmoid\"" % (kind,))
        n_rows, rp, col, cand, status = self._cand_begin(candidates, n_rows, unique=False)
        out, _csr = self._cand_mixed(x_positions, x_ones, titles, titles_use, cand, int(col.size), status)
        values = out.cpu().numpy()[:col.size]
        self._check_feed()
        return self._cand_result(values, candidates, rp)

    def rank_of(self, x_positions, x_ones, columns, seeds, n_rows=None, want_logits=False, titles=None, titles_use=None):
        """`DAE.rank_of`: the ranks under the plain DAE logits.  With titles in use the call raises ValueError: the ranks under
        the title mix are `mixed_rank_of`'s."""
        if titles is not None and titles_use is not None and np.any(np.asarray(titles_use)):
            raise ValueError("rank_of: ranks under the title mix (titles / titles_use) are mixed_rank_of's; call rank_of without "
                             "titles for the ranks of the DAE's own logits")
        return DAE.rank_of(self, x_positions, x_ones, columns, seeds, n_rows=n_rows, want_logits=want_logits)

    def mixed_rank_of(self, x_positions, x_ones, columns, seeds, titles, titles_use, n_rows=None, want_scores=False,
                      catalogue=None):
        """`rank_of` under the score the titled `recommend` ranks: per listed (row, column) the number of non-seed track columns
        that precede it by y = title_score * w_title + dae_score * w_playlist (descending, ties by column ascending), so
        `mixed_rank_of(feed, recommend(feed, seeds, titles=, titles_use=)[0], seeds, titles, titles_use)` is `arange(k)` per
        row -- below position 1 024 too, where the titled lists end.  columns, seeds, n_rows, the -1 results: as `rank_of`.
        The dispatch is `recommend`'s: with no title in use this is `DAE.rank_of(...)`, and want_scores then returns the plain
        call's LOGITS; otherwise every row is ranked by y (rows with titles_use = 0 included) and want_scores returns y
        (-inf beside a rank of -1), `recommend`'s score column bit for bit.  Always fp32, whatever the model's decode dtype
        (both fp32 images are packed for the call).  A scoring shard is refused like the candidate calls, and so is
        catalogue= (`recommend`'s handle): ranks inside a catalogue are not built."""
        if catalogue is not None:
            raise ValueError("mixed_rank_of: ranks inside a catalogue are not built; the ranks are over all track columns "
                             "(call it without catalogue=)")
        if titles is None or titles_use is None or not np.any(np.asarray(titles_use)):
            return DAE.rank_of(self, x_positions, x_ones, columns, seeds, n_rows=n_rows, want_logits=want_scores)
        import torch
        n_rows, rp, col, ans, status = self._cand_begin(columns, n_rows, unique=False)
        tm = self.title_model
        self._ensure_packed(_lib.DAE_DTYPE_F32)
        tm._ensure_packed(_lib.DAE_DTYPE_F32)
        self.ctx.bind_stream()
        tm.ctx.bind_stream()
        csr = self._upload_csr(x_positions, x_ones)
        dev = csr[0].device
        h = torch.empty((self.n_batch, self.n_hidden), dtype=torch.float32, device=dev)
        self.ctx.encode(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"], h)
        w_t, w_p = self._mix_weights(csr, titles_use)
        feat = tm.features(titles, self.n_batch)
        d_srp, d_sc = self._seed_csr_dev(seeds, csr)
        n = int(col.size)
        rank = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        score = torch.empty(max(n, 1), dtype=torch.float32, device=dev) if want_scores else None
        tm.ctx.mix_rank_of(self.ctx, h, self.weights["decoder_h"], self.biases["decoder_b"], feat, tm.p["Output_WT"],
                           tm.p["Output_b"], w_t, w_p, self.n_tracks, d_srp, d_sc, ans, n, rank, out_score=score, status=status)
        self._cand_status(status)
        ranks = rank.cpu().numpy()[:n]
        scores = score.cpu().numpy()[:n] if want_scores else None
        self._check_feed()

        def shaped(values, fill):
            return self._rank_result(values, columns, rp, n_rows, fill)

        if want_scores:
            return shaped(ranks, -1), shaped(scores, -np.inf)
        return shaped(ranks, -1)

    def rank_candidates(self, x_positions, x_ones, candidates, seeds, k=500, n_rows=None, titles=None, titles_use=None,
                        catalogue=None):
        """`DAE.rank_candidates` (catalogue= included); with titles in use the candidates are ranked by the mixed score (score = y),
        as the titled `recommend` ranks the whole track range."""
        candidates = self._cand_in_catalogue(candidates, n_rows, catalogue)
        if titles is None or titles_use is None or not np.any(np.asarray(titles_use)):
            return DAE.rank_candidates(self, x_positions, x_ones, candidates, seeds, k=k, n_rows=n_rows)
        n_rows, rp, col, cand, status = self._cand_begin(candidates, n_rows, unique=True)
        key, csr = self._cand_mixed(x_positions, x_ones, titles, titles_use, cand, int(col.size), status)
        return self._cand_rank(cand, rp, key, seeds, csr, k, n_rows, _lib.DAE_OUT_LOGIT)     # (out_score holds y)

    def _mix_guard_fired(self, idx, k, score):
        """A launch of the exact title mix whose guard words moved is not trusted (a recomputed logit left the interval
        the bf16 launch promised for it, or a row overflowed its candidate list): -> (score, idx) of the same feed through
        the fp32 kernels, or None when the launch stands."""
        tag = getattr(idx, "_mix_guard", None)
        if tag is None:
            return None
        gw, (x_positions, x_ones, seeds, titles, titles_use, n_rows) = tag
        n_bad, col = (int(v) for v in gw.cpu())
        # (the shadow of the cumulative words lives on the context and is resynchronised by every dae_exact_guard_read on it:
        # ADVICE r4 -- a read elsewhere used to leave this comparison one reset behind)
        seen = getattr(self.title_model.ctx, "_guard_seen", 0)
        if not self.title_model.ctx.guard_moved(n_bad):
            self._mix_overflow_streak = 0
            return None
        import warnings
        import torch
        self._ensure_packed(_lib.DAE_DTYPE_F32)
        self.title_model._ensure_packed(_lib.DAE_DTYPE_F32)
        n_new = n_bad - seen
        nb = n_rows or self.n_batch
        if col == -3:
            # rows whose survivors overflow the refine launch's list return no recommendations (idx -1): when every event of
            # this launch is such a row (e.g. a title-only playlist under a flat title scorer: its scores cannot be told apart
            # by any bound), ONLY those rows are re-scored with the fp32 kernels and patched in
            rows = np.nonzero(idx[:nb, 0].cpu().numpy() < 0)[0]
            use = np.asarray(titles_use, np.float32).reshape(-1)
            if 0 < len(rows) == n_new and len(rows) <= nb // 2 and np.all(use[rows] > 0):
                P = np.asarray(x_positions, np.int64).reshape(-1, 2)
                sel = np.isin(P[:, 0], rows)
                newid = np.full(nb, -1, np.int64)
                newid[rows] = np.arange(len(rows))
                P2 = np.stack([newid[P[sel, 0]], P[sel, 1]], 1) if sel.any() else np.zeros((0, 2), np.int64)
                o = np.asarray(x_ones, np.float32).reshape(-1)
                O2 = o[sel] if o.size == len(P) else o
                seeds2 = seeds if isinstance(seeds, str) else [list(seeds[r]) if r < len(seeds) else [] for r in rows]
                T2 = np.asarray(titles, np.int64).reshape(-1, self.title_model.input_len)[rows]
                warnings.warn("exact_bf16 title mix: the bound guard fired (%d row(s) overflow the refine launch): those rows are "
                              "re-scored with the fp32 kernels" % len(rows))
                self._guard_row_fallbacks += len(rows)
                score2, idx2 = self._submit(P2, O2, seeds2, k, _lib.DAE_DTYPE_F32, T2, use[rows], n_rows=len(rows))
                rt = torch.from_numpy(rows).to(idx.device)
                idx_n, score_n = idx.clone(), score.clone()
                idx_n[rt] = idx2[:len(rows)]
                score_n[rt] = score2[:len(rows)]
                self._mix_overflow_streak = 0
                return score_n, idx_n
        if col in (-2, -3):                     # not a broken bound, but many rows the refine launch cannot hold: after two such
            self._mix_overflow_streak += 1                                                    # launches in a row the mode pauses
            if self._mix_overflow_streak >= 2:
                self._mix_exact_pause = 64      # launches on the fp32 kernels before it is tried again
                self._mix_overflow_streak = 0
        self._guard_fell_back("exact_bf16 title mix: the bound guard fired (%s): this launch is re-scored with the fp32 kernels"
                              % ("rows overflow the refine launch" if col in (-2, -3) else "column %d" % col))
        return self._submit(x_positions, x_ones, seeds, k, _lib.DAE_DTYPE_F32, titles, titles_use, n_rows=n_rows)

    def _recommend_catalogue_titled(self, cat, x_positions, x_ones, seeds, k, n_rows, dtype, titles, titles_use):
        """The titled `recommend` inside a catalogue: `_submit`'s fused mix with the two vocabulary-wide GEMMs on the handle's
        images -- the DAE term of the catalogue's n columns (dae_decode_mix_term on its DAE context), then the threshold path of
        its title context over sigmoid(z_title) * w_title + that term (dae_decode_topk_catalogue: seeds translated, ranked over
        n columns, indices mapped back).  Encode, mixing weights and title features are the model's own launches.  fp32 and
        plain bf16; exact_bf16 has no catalogue mix and runs on the fp32 kernels (the lists it promises), said once."""
        import torch
        dtype = cat._title_dtype(self._dtype_of(dtype))
        tm = self.title_model
        if cat.title_ctx is None:
            raise _lib.DaeError("catalogue: the handle was made before the title scorer was fitted; make a new one")
        cat._ensure(dtype)
        cat._ensure_title(dtype)
        for c in (self.ctx, tm.ctx, cat.ctx, cat.title_ctx):
            c.bind_stream()
        nb = self.n_batch
        n_rows = nb if n_rows is None else n_rows
        dev = self.weights["encoder_h"].device
        csr = self._upload_csr(x_positions, x_ones)
        h = torch.empty((nb, self.n_hidden), dtype=torch.float32, device=dev)
        self.ctx.encode(csr[0], csr[1], csr[2], self.weights["encoder_h"], self.biases["encoder_b"], h)
        w_t, w_p = self._mix_weights(csr, titles_use)
        feat = tm.features(titles, nb)
        d_srp, d_sc = self._seed_csr_dev(seeds, csr)
        score = torch.empty((nb, k), dtype=torch.float32, device=dev)
        idx = torch.empty((nb, k), dtype=torch.int32, device=dev)
        y1T = torch.empty((cat.n, nb), dtype=torch.float32, device=dev)
        cat.ctx.decode_mix_term(h, w_p, cat.n, y1T, dtype=dtype)
        cat.title_ctx.set_score_mix(y1T, w_t)
        try:
            cat.title_ctx.decode_topk_catalogue(cat.cat, feat, d_srp, d_sc, k, score, idx, out_kind=_lib.DAE_OUT_LOGIT, dtype=dtype)
        finally:
            cat.title_ctx.set_score_mix()
        res = idx[:n_rows].cpu().numpy(), score[:n_rows].cpu().numpy()
        self._check_feed()
        return res

    def recommend(self, x_positions, x_ones, seeds, k=500, n_rows=None, dtype=None, titles=None, titles_use=None, catalogue=None):
        """Top-k of the MIXED score (DAEs.py:176-181 + main_challenge.py:26-41) without either [batch, n_input] matrix
        (see `_submit`).  Same operations in the same order as `mixed_scores` + dae_topk_dense, hence the same bits
        (fp32).  dtype "bf16" (or [BASE] decode_dtype = bf16) runs BOTH vocabulary-wide GEMMs -- the DAE decoder and
        the title scorer's output layer -- on bf16 operands with fp32 accumulate; encode, title features, sigmoids,
        the mix, the threshold and the ranking stay fp32.
        catalogue: as `DAE.recommend` takes it -- the mixed score ranked over the handle's columns alone
        (`_recommend_catalogue_titled`)."""
        if titles is None or titles_use is None or not np.any(np.asarray(titles_use)):
            return DAE.recommend(self, x_positions, x_ones, seeds, k=k, n_rows=n_rows, dtype=dtype, catalogue=catalogue)
        _refuse_deep_k(k, "DAE_title.recommend with titles in use")       # (before any upload)
        if catalogue is not None:
            self._catalogue_begin(catalogue)
            return self._recommend_catalogue_titled(catalogue, x_positions, x_ones, seeds, k, n_rows, dtype, titles, titles_use)
        if self._score_shard is not None:
            raise _lib.DaeError("title-mixed batches are not vocabulary-sharded: run --challenge with titles on one "
                                "GPU per process group (playlist partitioning), or without the title variables")
        dtype = _title_dtype(self._dtype_of(dtype), self)
        self._ensure_packed(dtype)
        self.title_model._ensure_packed(dtype)
        self.ctx.bind_stream()
        score, idx = self._submit(x_positions, x_ones, seeds, k, dtype, titles, titles_use)
        n_rows = self.n_batch if n_rows is None else n_rows
        redo = self._mix_guard_fired(idx, k, score)
        if redo is not None:
            score, idx = redo
        res = idx[:n_rows].cpu().numpy(), score[:n_rows].cpu().numpy()
        self._check_feed()
        return res
