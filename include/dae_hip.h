/*
 * dae_hip.h -- C ABI of libdae_hip.so: the MI355X (gfx950) implementation of the
 * multi-hot denoising-autoencoder scoring path of hojinYang/spotify_recSys_challenge_2018.
 *
 * The reference has no FFI: its boundary is `sess.run(model.y_pred | [optimizer, cost], feed_dict)`
 * on the TF1 graph built in models/DAEs.py.  Each entry point below names the graph section
 * (reference file:line) it replaces.  A reference maintainer binds these with ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; dae_last_error(ctx) gives the message;
 *   - all data pointers are CALLER-OWNED DEVICE pointers (e.g. torch tensors); the library only
 *     allocates scratch inside the ctx (grown lazily, never inside a steady-state call once sized);
 *   - all work is enqueued on the ctx stream (dae_set_stream), no hidden synchronisation;
 *   - one ctx is not thread-safe; independent ctxs are;
 *   - indices are int32, values fp32; rows = playlists, columns = item ids (tracks then artists).
 *
 * Numerics contract (DESIGN.md "canonical order"): the fp32 path is bit-reproducible and equals
 * oracle/dae_oracle.c bit-for-bit: encode = fmaf chain over the de-duplicated non-zeros in
 * ascending column order; decode = fmaf chain over k = 0..H-1 (v_mfma_f32_32x32x2_f32 is exactly
 * that chain); ranking key = (fp32 logit desc, column index asc); scores = dae canonical sigmoid.
 */
#ifndef DAE_HIP_H
#define DAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dae_ctx dae_ctx;

/* error codes */
#define DAE_OK            0
#define DAE_ERR_ARG      -1   /* bad argument (shape, alignment, null pointer)           */
#define DAE_ERR_HIP      -2   /* a HIP runtime call failed                                */
#define DAE_ERR_NOMEM    -3   /* scratch allocation failed                                */
#define DAE_ERR_STATE    -4   /* call sequence error (e.g. weights not prepacked)         */

/* what dae_decode_topk / dae_topk_* write into out_score */
#define DAE_OUT_SCORE     0   /* canonical sigmoid(logit)  (what the reference ranks on)  */
#define DAE_OUT_LOGIT     1   /* raw fp32 logit (needed when shards are merged later)     */

/* decode arithmetic */
#define DAE_DTYPE_F32     0   /* v_mfma_f32_32x32x2_f32, exact fp32, bit-equal to oracle  */
#define DAE_DTYPE_BF16    1   /* v_mfma_f32_32x32x16_bf16, fp32 accumulate (cfg 5)        */
/* BASELINE.json north_star: the decode as a bf16 MFMA GEMM whose top-k lists are BIT-IDENTICAL to the fp32 path
 * (indices and scores; main_challenge.py:26-36 ranks the fp32 y_pred).  The bf16 GEMM only FILTERS: with a rigorous
 * per-column bound eps_c >= |z_fp32 - z_bf16| (bf16 rounding of both operands + both accumulations; computed by
 * dae_prepack_decoder, readable through dae_exact_bounds), the threshold is taken from lower bounds z_bf16 - eps_c,
 * every column with z_bf16 + eps_c >= threshold survives, and the survivors' logits are recomputed with the canonical
 * fp32 fmaf chain before they are ranked.  Accepted by dae_prepack_decoder (bf16 image + bounds + a row-major fp32
 * copy of the decoder rows), dae_score_topk and dae_decode_topk.  Precondition of the bound: hidden activations in
 * [0, 1] (sigmoid outputs, DAEs.py:66-67) -- always true in dae_score_topk; a row passed to dae_decode_topk that
 * violates it returns no recommendations (idx -1, score -inf).  Not available with dae_set_score_mix: the title mix
 * has its own exact entry point, dae_mix_topk_exact. */
#define DAE_DTYPE_BF16_EXACT 2

/* ---- lifecycle -------------------------------------------------------------------------- */

/* library ABI version (major*1000 + minor). */
int dae_version(void);

/* Create a context bound to HIP device `device`.  Replaces tf.Session() (main_challenge.py:66,
 * main_train.py:172). */
int dae_create(int device, dae_ctx** out);
int dae_destroy(dae_ctx* ctx);

/* Stream all later calls are enqueued on (a hipStream_t passed as void*; NULL = default stream). */
int dae_set_stream(dae_ctx* ctx, void* hip_stream);

/* Last error message of this ctx (never NULL). dae_last_error(NULL) = last creation error. */
const char* dae_last_error(const dae_ctx* ctx);

/* Bytes of device scratch currently held by the ctx. */
size_t dae_scratch_bytes(const dae_ctx* ctx);

/* Per-kernel timing for roofline reporting: when enabled, the dominant kernel of each
 * dae_decode_* call is bracketed by hipEvents on the ctx stream.  dae_profile_read
 * synchronises those events and returns total milliseconds and the launch count, then resets. */
int dae_profile_enable(dae_ctx* ctx, int on);
int dae_profile_read(dae_ctx* ctx, double* ms_total, int* launches);
/* Symbol (as rocprofv3's kernel trace prints it) of the kernel the last event pair bracketed; "" before the first. */
const char* dae_profile_kernel(const dae_ctx* ctx);

/* Engine clock actually sustained while other work runs (the chip clocks to its power budget: the fp32 matrix-core
 * roof moves with it).  Enqueues ONE wave on `hip_stream` (any stream; NULL = the ctx stream) that reads the shader
 * cycle counter (s_memtime) and the constant-rate wall clock (s_memrealtime) `window_us` apart and stores
 * {shader cycles, wall-clock ticks} in out2_dev (device, 2 x uint64).  wall_khz_out (host, may be NULL) receives the
 * wall clock's rate (hipDeviceAttributeWallClockRate).  GHz = cycles / ticks * wall_khz / 1e6. */
int dae_clock_probe(dae_ctx* ctx, void* hip_stream, int window_us, uint64_t* out2_dev, int* wall_khz_out);

/* Geometry of the last dae_decode_topk or dae_mix_topk_exact issued from the calling thread, for roofline accounting:
 * {R_TILE, n_row_groups, blocks_per_row_group, sample_stride S, n_sample_tiles (phase A),
 *  n_filter_tiles (phase B), fused(0/1), n_tiles}.  A tile is 32 vocabulary columns.  n_tiles counts the tiles the call
 * WALKS: those of the image that hold a ranked column, ceil((min(n_tracks, col_hi) - col_lo) / 32) -- not the image's
 * (0 when n_tracks <= col_lo: no launch).  (dae_mix_topk_exact: S = 1, fused = 0; its filter launch gives every workgroup of
 * blocks_per_row_group 8 waves that claim tiles.) */
int dae_last_plan(int32_t out[8]);

/* ---- input: COO -> CSR (DAEs.py:33-38 SparseTensor + sparse_tensor_to_dense) --------------- */

/* The reference feeds COO (row, col) pairs with duplicates and ASSIGNMENT semantics
 * (last occurrence wins).  The host shim (models/DAEs.py of this repo) de-duplicates and sorts
 * them into CSR (row_ptr[B+1], col ascending per row, val).  All encode/train entry points take
 * that CSR. */

/* ---- encode (DAEs.py:40-42 dropout+normalise, :64-70 encoder) ----------------------------- */

/* The feed of the reference graph on the device (models/DAEs.py:23-35; utils/data_reader.py builds
 * it row by row): COO entries (row, col) -> value in FEED ORDER, duplicates allowed;
 * tf.sparse_tensor_to_dense(validate_indices=False) scatters them by assignment, so the LAST
 * occurrence of a (row, col) wins.  Produces the CSR every other entry point takes: columns
 * ascending per row, one entry per (row, col), explicit zeros dropped.
 *   positions [nnz,2] int64 (row in batch, column), values [nnz] fp32 (or ONE value for all entries
 *   when values_broadcast != 0: the reference feeds np.ones / a scalar).
 *   row_ptr [n_rows+1], col / val with room for nnz entries (row_ptr[n_rows] of them are written).
 *   status: device int32, 0 = ok, bit 0 = an entry had row/col out of range (it is skipped; the host
 *   restatement raises ValueError for the same input). */
int dae_coo_to_csr(dae_ctx* ctx, const int64_t* positions, const float* values, int values_broadcast,
                   int64_t nnz, int n_rows, int n_cols, int32_t* row_ptr, int32_t* col, float* val,
                   int32_t* status);

/* The seed lists of a scoring call whose seeds are the playlist's OWN tracks -- what both reference drivers pass
 * (main_challenge.py:76-88 `seed` = the track ids x_positions feeds; main_train.py:64-89 `test_seed` likewise): the
 * columns < n_tracks of every row of the input CSR, as a CSR (seed_row_ptr [B+1], seed_col with room for
 * row_ptr[B] entries; sorted and unique per row because the input rows are).  Saves the host the list handling and
 * two uploads per batch.  Any B (slabs of 16384 rows inside). */
int dae_seeds_from_csr(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, int B, int n_tracks,
                       int32_t* seed_row_ptr, int32_t* seed_col);

/* ---- the training feed on the device (csrc/train_feed.hip; utils/data_reader.py) ------------ */

/* The training set as the reader holds it -- per side (tracks, artists) a flat id array and n_playlists + 1 offsets --
 * copied ONCE into device memory the set owns.  HOST arrays: trk / art int32, trk_off / art_off int64.  Refused here, on
 * the host and before any HIP call (DAE_ERR_ARG and a message): offsets that do not start at 0 or descend, a track id
 * outside [0, n_tracks), an artist id outside [n_tracks, n_items).  dae_train_batch relies on it and carries no per-entry
 * range flag.  The set belongs to ctx's device; destroy it before the process ends (it waits for the device first). */
typedef struct dae_train_set dae_train_set;
int dae_train_set_create(dae_ctx* ctx, const int32_t* trk, const int64_t* trk_off, const int32_t* art, const int64_t* art_off,
                         int n_playlists, int n_tracks, int n_items, dae_train_set** out);
int dae_train_set_destroy(dae_train_set* set);

/* Both CSRs of one training step from the reader's DRAWS, on ctx's stream, in two launches (no memset).
 *   draw   DEVICE int32 [3][B]: playlist index (the file's own), given tracks, given artists.  Entry i of a side (its
 *          position in the playlist) carries the value 1 if given < 0 || i < given, else 0; -1 feeds the whole side.
 *   x_side 0: x = the tracks, 1: the artists, 2: both (y's entries with x's values).  y = tracks u artists, value 1.
 * The result is what dae_coo_to_csr makes of that feed: among equal columns of a row the LAST position wins, zero values
 * are dropped, columns ascend; row_ptr[B] entries of col / val are written.  A playlist may be drawn into several rows.
 *   x_cap / y_cap: room of x_col, x_val / y_col, y_val in entries; nothing is written at or past it (row_ptr still holds
 *          the offsets of the whole result).
 *   status DEVICE int32, always written: bit 0 = a playlist index outside [0, n_playlists) (that row is empty), bit 1 =
 *          x_cap or y_cap was too small.
 * 1 <= B <= 4096.  Scratch: 8 bytes x B x the set's longest playlist (12 when a side of the set exceeds 512 entries:
 * such sides are ranked over global memory instead of LDS). */
int dae_train_batch(dae_ctx* ctx, const dae_train_set* set, const int32_t* draw, int B, int x_side,
                    int32_t* x_row_ptr, int32_t* x_col, float* x_val, int x_cap,
                    int32_t* y_row_ptr, int32_t* y_col, float* y_val, int y_cap, int32_t* status);

/* The playlists' TITLES join the set: what the reader appends per drawn playlist (data_reader.py:29 / :42, `titles`) and the
 * title step feeds as model_title.titles (main_train.py:218), so that a title step too is named by its draw alone.
 *   titles HOST int32 [n_playlists][L], copied once into an allocation the set owns (dae_train_set_destroy frees it):
 *          4 L bytes a playlist.  n_playlists must be the set's, 1 <= L <= 64 (the title kernels' longest title).
 * Refused on the host, before any HIP call (DAE_ERR_ARG): an entry that is neither -1 (no character) nor in [0, n_char).
 * A second attach: DAE_ERR_STATE.  The call has no context: its message is dae_last_error(NULL)'s. */
int dae_train_set_attach_titles(dae_train_set* set, const int32_t* titles, int n_playlists, int L, int n_char);

/* titles_out (DEVICE int32 [B][L]) row r = the title row of playlist draw[0][r]: one launch on ctx's stream, one wave per
 * row.  `draw` as dae_train_batch takes it (only its first B entries are read).  A playlist index outside
 * [0, n_playlists) gives a row of -1; dae_train_batch raises its status bit 0 for that same draw, so there is no second
 * status word here.  1 <= B <= 4096.  A set without titles: DAE_ERR_STATE. */
int dae_train_titles(dae_ctx* ctx, const dae_train_set* set, const int32_t* draw, int B, int32_t* titles_out);

/* h[r,:] = hidden_dropout( sigmoid( sum_c (x[r,c]/(s_r+1e-10)) * W_enc[c,:] + b_enc ) )
 *   x      = input_dropout(CSR row r), s_r = sum of surviving weights.
 *   ikp/kp = input / hidden keep probabilities (1.0 = identity, the inference setting);
 *   seed   = counter-based RNG seed for both dropouts (ignored when ikp == kp == 1).
 * W_enc [V,H] row-major fp32, b_enc [H], h_out [B,H] row-major fp32.  H % 4 == 0. */
int dae_encode(dae_ctx* ctx,
               const int32_t* row_ptr, const int32_t* col, const float* val,
               const float* W_enc, const float* b_enc,
               int V, int H, int B,
               float ikp, float kp, uint32_t seed,
               float* h_out);

/* ---- decoder weights ------------------------------------------------------------------------ */

/* Re-tile W_dec[col_lo:col_hi, :] (row-major [V,H] fp32, DAEs.py:123 / tied :54) and
 * b_dec[col_lo:col_hi] into the MFMA operand order the decode kernels stream (DESIGN.md "HBM
 * layout").  Call once per weight update (model load / after a training epoch); the packed copy
 * lives in the ctx.  dtype selects the fp32 or bf16 packed image (both may be resident). */
int dae_prepack_decoder(dae_ctx* ctx, const float* W_dec, const float* b_dec,
                        int V, int H, int col_lo, int col_hi, int dtype);

/* The same from a RANK-LOCAL copy of the rows (vocabulary shards: a rank holds only its own rows of W_dec):
 * W_rows [n_rows, H] / b_rows [n_rows] are the global columns col_lo .. col_lo + n_rows; the image covers exactly
 * those.  (dae_prepack_decoder indexes its arguments by global column; this entry point does the shift inside the
 * library, where the prepack kernels' access range is known.)  Replaces the same section as dae_prepack_decoder. */
int dae_prepack_decoder_rows(dae_ctx* ctx, const float* W_rows, const float* b_rows, int n_rows, int H, int col_lo,
                             int dtype);

/* Let `dst` use the decoder image `src` prepacked for `dtype` instead of holding a copy of its own (the contexts of
 * several batches in flight score with the same weights: one image stays resident in the 256 MB Infinity Cache where
 * two or three copies of 87 / 174 MB evict each other; it also saves their memory and re-tiling).  `dst` borrows the
 * buffers: `src` must outlive every use, must not be re-prepacked while `dst` has work in flight, and the caller orders
 * `src`'s prepack before `dst`'s first launch (streams!).  A later dae_prepack_decoder on `dst` gives it an image of its
 * own again.  Same device only. */
int dae_share_decoder(dae_ctx* dst, const dae_ctx* src, int dtype);

/* DAE_DTYPE_BF16_EXACT: copy the per-column bounds eps_c of the prepacked image (col_lo <= c < col_hi) to
 * eps_out (device, col_hi - col_lo floats).  |fp32 logit - bf16 logit| <= eps_c for every hidden row in [0, 1]^H;
 * DESIGN.md section 2b derives it, tests/test_gpu_exact.py checks it against measured differences. */
int dae_exact_bounds(dae_ctx* ctx, float* eps_out);

/* DAE_DTYPE_BF16_EXACT, the BOUND GUARD.  One term of eps_c -- the accumulation inside v_mfma_f32_32x32x16_bf16 -- rests
 * on an error model of that instruction, not on a specification.  So every survivor the refine launch recomputes in
 * fp32 is tested against what the filter launch promised for it (u - 2 eps_c <= z_fp32 <= u, u the stored upper bound;
 * both numbers are in registers: the test is free), and a violation is COUNTED in two device words of the context
 * instead of silently costing a true top-k column.  A caller that sees a count != 0 must treat the results of the calls
 * since the last read as unproven and re-run them with DAE_DTYPE_F32 (models/DAEs.py recommend / recommend_iter do).
 *   dae_exact_guard_read : synchronises the ctx stream; violations (count since the last read that returned != 0) and
 *                          one violating global column (-1 when none); resets the words when the count is non-zero.
 *   dae_exact_guard_words: the device address of {int32 violations, int32 column}, for a caller that fetches the words
 *                          with its results (no synchronisation here); valid for the life of the ctx.
 * The ranking values that reach main_challenge.py:26-36's argsort are fp32 either way: the guard protects the SET. */
int dae_exact_guard_read(dae_ctx* ctx, int32_t* violations, int32_t* column);
int dae_exact_guard_words(dae_ctx* ctx, const int32_t** words_dev);
/* The guard words {violations so far, a violating column} as they stand after everything enqueued on the context's stream so
 * far, copied to words_out_dev (DEVICE int32[2]) in stream order: a snapshot that travels with a launch's lists.  The words
 * are cumulative until a dae_exact_guard_read finds them non-zero (and resets them): a count that differs from the previous
 * launch's snapshot on the same context means THIS launch is unproven (models/DAEs.py: the interpreter loop). */
int dae_exact_guard_snapshot(dae_ctx* ctx, int32_t* words_out_dev);
/* How selective the filter was (the exact mode's rate depends on it, its results never): of the LAST exact scoring launch
 * of this context, out3 = {rows refined, candidates the bf16 filter launch left for them (sum over the rows), candidates
 * recomputed in fp32 after the narrowing step (sum)}.  Synchronises the ctx stream. */
int dae_exact_stats_read(dae_ctx* ctx, uint64_t out3[3]);

/* ---- skipped filter tiles (DAE_DTYPE_F32, hidden 225..256, batches that score in 128-row groups, no dae_set_score_mix) ----
 * dae_prepack_decoder(DAE_DTYPE_F32) keeps two floats per 32-column tile t of the image, A_t and M_t, with
 *   fp32 logit(r, c) <= A_t + d * M_t   for every column c of the tile and every hidden row r with |h[r][k] - 0.5| <= d, all k
 * (the rounding of the canonical chain is inside).  A ranking call knows each row's threshold tau before
 * its filter launch: per row group it takes d over the group's rows and tau_rg = the smallest of their thresholds, and the
 * filter launch walks only the tiles with !(A_t + d M_t < tau_rg).  A tile left out holds no logit the launch would have kept:
 * lists and scores are bit for bit those of the full walk.  The bounds belong to the image and travel with dae_share_decoder.
 *   dae_set_filter_skip : on (default) / off = the launch over every planned filter tile.
 *   dae_filter_skip_read: out3 = {filter launches that built live lists, planned filter tiles x row groups (sum), tiles they
 *                         walked (sum)} since the last read; resets the counters; synchronises the ctx stream.  dae_last_plan
 *                         keeps reporting the PLANNED tiles: the work really done is this.
 *   dae_filter_skip_last: the live tiles per row group of the context's last ranking call (live_out[0 .. min(cap, n_rg)), host);
 *                         *n_rg_out = 0 when that call's filter launch built no live lists.  Synchronises.
 *   dae_tile_bounds_read: the fp32 image's {A_t, M_t} pairs to ub_out (HOST, 2 floats per tile, at most cap_tiles tiles);
 *                         *ntiles_out = tiles of the image.  Synchronises. */
int dae_set_filter_skip(dae_ctx* ctx, int on);
int dae_filter_skip_read(dae_ctx* ctx, uint64_t out3[3]);
int dae_filter_skip_last(dae_ctx* ctx, int32_t* live_out, int cap, int* n_rg_out);
int dae_tile_bounds_read(dae_ctx* ctx, float* ub_out, int cap_tiles, int* ntiles_out);
/* The same switch covers the threshold SAMPLE of such a call where it runs in half row groups (65..256 rows, a sample of one
 * round of tiles): per column the image also keeps lo_c with fp32 logit(r, c) >= lo_c - d * m_c, so a lower bound tau_safe of
 * every row's threshold is known before the sample runs, and a wave whose tile has A_t + d M_t < tau_safe decodes nothing
 * (its logits could neither move tau nor survive it).  Thresholds, lists and scores stay bit for bit those of the full walk.
 *   dae_sample_skip_read: out3 = {sample launches that could skip, wave-tiles they planned (sum), wave-tiles they decoded
 *                         (sum)} since the last read; resets the counters; synchronises the ctx stream. */
int dae_sample_skip_read(dae_ctx* ctx, uint64_t out3[3]);
/* Where such a sample ran, the threshold launch that builds the live lists knows, per half row group, D >= the d of its rows and
 * tau_safe <= their thresholds, and the context keeps max over the filter launch's tiles of A_t + d M_t on a grid of d.  A row
 * group these prove to have NO live tile gets its empty list without the hand-off between the rows' workgroups; every other
 * group takes it as before.  Lists, counts and the counters of dae_filter_skip_read are the same either way.
 *   dae_live_proof_read: *groups_proved = row groups whose live list was proved empty since the last read; resets the counter;
 *                        synchronises the ctx stream. */
int dae_live_proof_read(dae_ctx* ctx, uint64_t* groups_proved);
/* The thresholds the context's last dae_score_topk / dae_decode_topk (its last slab of rows) computed and gave its own filter
 * launch: tau_out[0 .. B) on the HOST (what dae_score_topk_begin returns to its caller).  Synchronises the ctx stream. */
int dae_last_tau_read(dae_ctx* ctx, float* tau_out, int B);

/* Factor on every eps_c computed by the NEXT dae_prepack_decoder(DAE_DTYPE_BF16_EXACT) of this context (default 1).
 * > 1 widens the bounds: a safety margin for a caller who distrusts the error model (more survivors to recompute, same
 * results).  < 1 VOIDS the guarantee and exists so that the guard can be exercised: results may then differ from the
 * fp32 path, and dae_exact_guard_read reports it (tests/test_gpu_exact.py).  0 < scale <= 1024. */
int dae_set_exact_margin(dae_ctx* ctx, float scale);
/* The same hook for the columns [col_from, col_to) alone (global ids; applied by the NEXT exact prepack, the other columns
 * keep dae_set_exact_margin's factor): lets a test void the bound of a column that every row DROPS, which only the audit
 * below can see (tests/test_gpu_exact.py::test_audit_sees_a_violation_on_a_dropped_column).  col_from == col_to: none.
 * scale < 0 (>= -1024) FORGES the filter outright: the UPPER bound of those columns is put |scale| logits too low, so rows
 * drop columns that belong in their lists -- the failure the audits exist for (tests/test_gpu_title_exact.py). */
int dae_set_exact_margin_range(dae_ctx* ctx, int col_from, int col_to, float scale);

/* DAE_DTYPE_BF16_EXACT, the AUDIT of what the guard cannot see (csrc/audit.hip).  The guard tests the survivors the refine
 * launch recomputes; a column the bf16 filter launch DROPPED (upper bound u < the row's threshold) is never recomputed, so a
 * bound that fails there -- the only failure that can change a top-k list of main_challenge.py:28-36 -- would go unseen.
 * Every every_n-th exact scoring launch of the context (dae_decode_topk / dae_score_topk / dae_score_topk_finish; default 64,
 * 0 = never) therefore takes n_tiles (default 16, <= 64) pseudo-random 32-column tiles of the ranked columns -- different ones
 * each time; nearly all of their elements are dropped ones -- and for EVERY row of the launch recomputes both the filter
 * launch's upper bound u (the same bf16 MFMA sequence on the same operands: the same bits) and the canonical fp32 logit, and
 * counts every element outside [u - 2 eps_c, u] in the GUARD WORDS above: callers react exactly as to a survivor's violation.
 *   dae_exact_audit_read: out3 = {audits run, (row, column) elements checked, violations among them} since the context was
 *                         created; synchronises the ctx stream.
 * Proven: the bound, given the accumulation model of the bf16 MFMA.  Checked always: survivors.  Checked on a sample: dropped
 * columns (all rows x n_tiles x 32 columns per audit).  Assumed: nothing else.
 * Under the exact title mix (dae_mix_topk_exact / dae_title_score; set on the TITLE context, same defaults) the audit tests the
 * OUTCOME instead: the sampled tiles' mixed scores, recomputed with the canonical chains of both images and the fp32 path's mix
 * (DAEs.py:153-181), against the lists the launch just wrote -- an element above its row's k-th listed score that is neither
 * listed nor one of the row's seeds counts as a violation in the title context's guard words (csrc/audit.hip dae_launch_mix_audit). */
int dae_set_exact_audit(dae_ctx* ctx, int every_n, int n_tiles);
int dae_exact_audit_read(dae_ctx* ctx, uint64_t out3[3]);

/* ---- decode (DAEs.py:73-77 tied / :141-145 untied) ---------------------------------------- */

/* out[r, c-col_lo] = (apply_sigmoid ? sigmoid : id)( h[r,:] . W_dec[c,:] + b_dec[c] )
 * for c in the prepacked range.  out is [B, ld_out] fp32 with ld_out >= col_hi-col_lo.
 * This is the reference's y_pred (main_train.py:66, main_challenge.py:80). */
int dae_decode_dense(dae_ctx* ctx, const float* h, int B, int H, int dtype,
                     int apply_sigmoid, float* out, int64_t ld_out);

/* ---- rank (main_challenge.py:26-36, :87; metrics.py:59-68) ------------------------------- */

/* Fused decode + top-k over the prepacked column range restricted to track columns
 * (c < n_tracks, main_challenge.py:87), excluding each row's seed tracks
 * (seed_row_ptr[B+1], seed_col sorted ascending & unique per row; may be NULL = no seeds).
 * Order: logit descending, then column index ascending.  Writes k entries per row:
 * out_idx[r, i] = GLOBAL column id (or -1 when fewer than k candidates exist, as the reference's
 * cand[:500] of a short list), out_score per `out_kind`.
 * k: 1 <= k <= 4096 (DAE_MAX_K_DEEP) with DAE_DTYPE_F32 / DAE_DTYPE_BF16; 1 <= k <= 1024 (DAE_MAX_K) with
 * DAE_DTYPE_BF16_EXACT and on a context under dae_set_score_mix.  A larger k is refused before any launch, the message
 * naming the limit.  Lists of k > 1024 are prefix-extensions of the shorter ones: the same canonical order.
 * The ranked columns are a prefix of the image, and the call decodes the 32-column tiles that hold one and no other: the
 * columns behind them (the artist columns of the reference's vocabulary, which its graph computes before slicing them away,
 * main_challenge.py:87) can return nothing and are not read.  dae_decode_dense is the call that needs their logits.  An image
 * with no ranked column (n_tracks <= col_lo) launches no GEMM: every slot is (-1, -inf). */
int dae_decode_topk(dae_ctx* ctx, const float* h, int B, int H, int dtype,
                    int n_tracks,
                    const int32_t* seed_row_ptr, const int32_t* seed_col,
                    int k, int out_kind,
                    float* out_score, int32_t* out_idx);

/* The whole scoring path in one call: dae_encode (inference keep-probs) -> dae_decode_topk,
 * with the hidden activations kept inside the ctx in the decode kernels' operand order (no
 * [B,H] round trip, no re-pack pass).  Results are identical to calling the two separately.
 * This is what main_challenge.py:80-90 / main_train.py:66-89 do per batch.  As dae_decode_topk, it decodes the tiles with a
 * ranked column only.  k: as dae_decode_topk (4096; 1024 with DAE_DTYPE_BF16_EXACT or under dae_set_score_mix). */
int dae_score_topk(dae_ctx* ctx,
                   const int32_t* row_ptr, const int32_t* col, const float* val,
                   const float* W_enc, const float* b_enc, int V, int H, int B, int dtype,
                   int n_tracks,
                   const int32_t* seed_row_ptr, const int32_t* seed_col,
                   int k, int out_kind,
                   float* out_score, int32_t* out_idx);

/* dae_score_topk in two halves, for vocabulary-sharded scoring with a THRESHOLD EXCHANGE between them:
 *   begin:  encode + the threshold sample of this image's columns -> tau_out[B] (device): per row a valid lower bound
 *           of the k-th largest rankable non-seed logit among THIS image's columns (-inf when the ranked part of the image
 *           is small enough to be ranked densely, or empty).  The sample is drawn from the tiles with a ranked column, which
 *           are also all the filter launch of `finish` walks: the artist slice of a shard image is not read.  The k-th
 *           largest logit over ALL shards is at least every shard's bound, so the element-wise MAXIMUM of the shards'
 *           tau_out (one all-gather of 4 B per row and rank) is a valid -- and far tighter -- threshold for every shard.
 *   finish: the filter launch with `tau` (tau_out, or that maximum), the selection: out_score / out_idx hold the image's
 *           columns with logit >= tau in rank order, at most k, padded with (-inf, -1): merged over the shards
 *           (dae_topk_merge) they give exactly what the unsharded call returns.
 * One begin / finish pair at a time per context, same stream, 1 <= B <= 4096; seed_row_ptr of finish is the one
 * begin was given.  Replaces the same graph section as dae_score_topk (main_challenge.py:80-90, one batch).
 * k: 1 <= k <= 4096 with DAE_DTYPE_F32 / DAE_DTYPE_BF16, 1 <= k <= 1024 with DAE_DTYPE_BF16_EXACT (checked by begin). */
int dae_score_topk_begin(dae_ctx* ctx,
                         const int32_t* row_ptr, const int32_t* col, const float* val,
                         const float* W_enc, const float* b_enc,
                         int V, int H, int B, int dtype, int n_tracks,
                         const int32_t* seed_row_ptr, int k, float* tau_out);
int dae_score_topk_finish(dae_ctx* ctx, const float* tau,
                          const int32_t* seed_row_ptr, const int32_t* seed_col,
                          int out_kind, float* out_score, int32_t* out_idx);

/* Unfused ranking of caller-provided dense logits/scores [B, ld] whose column 0 is global
 * column `col_base`; ranks columns [0, ncols).  Same order/seed rules as dae_decode_topk.
 * (parity path: dae_decode_dense + dae_topk_dense must equal dae_decode_topk.)  1 <= k <= 4096: rows of k > 1024 are
 * ranked by an instantiation of the selection kernel with an 8192-key sort buffer, always one 1024-thread workgroup per row. */
int dae_topk_dense(dae_ctx* ctx, const float* logits, int64_t ld, int B, int ncols, int col_base,
                   const int32_t* seed_row_ptr, const int32_t* seed_col,
                   int k, int out_kind, float* out_score, int32_t* out_idx);

/* Merge G per-shard candidate lists (as produced with DAE_OUT_LOGIT, gathered by RCCL
 * all-gather into cand_logit/cand_idx [G, B, k]) into the global top-k.  idx == -1 entries are
 * ignored.  1 <= k <= 4096. */
int dae_topk_merge(dae_ctx* ctx, int G, int B, int k,
                   const float* cand_logit, const int32_t* cand_idx,
                   int out_kind, float* out_score, int32_t* out_idx);

/* Tell the context that `batches_in_flight` batches are being scored concurrently on different streams (their own
 * contexts).  With more than one, the latency-bound launches of the bf16 / exact paths take shapes that fit on a CU NEXT to
 * another batch's filter workgroup (fewer threads and registers): each is a little slower alone and the step is faster
 * (7.0 vs 6.5 M playlists/s with three batches in flight).  Results do not change.  Default: 1. */
int dae_set_overlap_hint(dae_ctx* ctx, int batches_in_flight);

/* Two batches in flight on two contexts / streams (bench.py): the dominant launch of the fused path (the threshold
 * filter over ~90 % of the vocabulary) occupies every CU, so two of them in flight only queue behind each other.  With a
 * gate, this context's launch waits for `wait_event` (a hipEvent_t the OTHER context records after its own launch) and
 * records `record_event` after itself: the two dominant launches alternate, everything else still overlaps.  Events are
 * caller-owned; NULL, NULL removes the gate.  Results are unaffected. */
int dae_set_decode_gate(dae_ctx* ctx, void* wait_event, void* record_event);

/* ---- the drivers' loop (main_challenge.py:72-93, main_train.py:62-96) ---------------------------------------------------
 *
 * The reference's loop per batch -- reader.next_batch() -> sess.run(y_pred, feed) -> cand_generate per row -- as a streaming
 * pipeline inside the library: HOST feeds in (the COO positions / values the reference's readers emit, utils/data_reader.py),
 * HOST top-k index lists out, nothing of the interpreter in between.  dae_pipeline_submit copies a feed into pinned staging
 * memory and returns; a library-owned thread issues the launches (upload, dae_coo_to_csr, dae_seeds_from_csr, dae_score_topk,
 * download) on `lanes` contexts / streams that take them in turn and share one packed decoder image; consecutive feeds share
 * a launch of up to `group_rows` rows (rows are scored independently: every feed gets the bits dae_score_topk gives it alone).
 * Seeds are the playlist's own tracks (the columns < n_tracks of its feed), what both reference drivers pass.
 * This group is the exception to "device pointers only": feeds and results are HOST memory.  One caller thread.
 *
 *   create : W_enc / b_enc / W_dec / b_dec are caller-owned DEVICE arrays ([V,H], [H], [V,H], [V]) that outlive the pipeline;
 *            dtype = DAE_DTYPE_*; a feed holds at most group_rows (<= 16384) rows and max_nnz entries; result_blocks pinned
 *            result blocks (>= lanes + 1) bound how many launches' lists the caller may hold at once.
 *   submit : positions [nnz,2] int64 (row in the FEED, column), values [nnz] fp32 (or one value: values_broadcast); n_rows
 *            rows.  Returns DAE_OK and the feed's ticket, or DAE_PIPE_BUSY (> 0): every lane holds lists that were not
 *            polled / released yet -- poll, then submit again.
 *   flush  : close the launch being filled (end of input; poll(wait) does it as well).
 *   poll   : the next feed IN SUBMISSION ORDER: *idx -> its [n_rows,k] global column ids (-1 = fewer candidates), *score
 *            (may be NULL) -> canonical sigmoid scores, both inside pinned result block *block, valid until
 *            dae_pipeline_release(block) (once per polled feed).  wait = 0: returns *n_rows = 0 when the feed is not ready.
 *            DAE_DTYPE_BF16_EXACT: a launch whose bound guard fired (dae_exact_guard_read) is re-scored with DAE_DTYPE_F32
 *            before its lists go out (dae_pipeline_stats counts it).
 *   stats  : {launches issued, feeds submitted, launches re-scored in fp32 after a bound-guard hit}. */
typedef struct dae_pipeline dae_pipeline;
#define DAE_PIPE_BUSY 1
/* k: 1 <= k <= 1024 for every dtype (a larger k is refused at creation). */
int dae_pipeline_create(int device, const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
                        int V, int H, int n_tracks, int dtype, int k, int group_rows, int64_t max_nnz, int lanes,
                        int want_scores, int result_blocks, dae_pipeline** out);
int dae_pipeline_destroy(dae_pipeline* p);
int dae_pipeline_submit(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                        int n_rows, uint64_t* ticket_out);
/* The TITLED loop -- what the reference's `--challenge` really runs (main_challenge.py:58-59, :72-93: every batch goes through
 * DAE_title with `titles` / `titles_use` in the feed; DAEs.py:153-181).  create_titled: the pipeline above plus the title
 * scorer's variables (caller-owned DEVICE arrays in the layout of dae_title_features / dae_title_score: emb [n_char][E], conv_w /
 * conv_b back to back, filter_sizes a HOST array of n_sizes entries, Output_WT [V][ld_feat] = Output_W^T zero padded,
 * Output_b [V]); titles are rows of L characters.  Every lane holds a second context for the title scorer on its stream.
 * submit_titled: a feed with its titles [n_rows][L] int32 (-1 = no character) and titles_use [n_rows] (HOST arrays) -> the
 * launch ranks y = sigmoid(z_title) * w_title + sigmoid(z_dae) * w_playlist (dae_title_score) with seeds = the playlist's own
 * tracks.  Feeds submitted WITHOUT titles (dae_pipeline_submit) on the same pipeline rank the plain DAE logits
 * (dae_score_topk), as `DAE_title.recommend` does for batches whose titles_use is all zero; the two kinds never share a launch.
 * At most 4096 rows per launch.  DAE_DTYPE_BF16_EXACT: a launch under which the title context's guard words moved (a bound
 * violated, or rows with more survivors than the refine launch lists) is re-scored with DAE_DTYPE_F32 before its lists go out;
 * after two launches in a row with overflowing rows the mode pauses for 64 launches (they run on the fp32 kernels). */
int dae_pipeline_create_titled(int device, const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
                               int V, int H, int n_tracks, const float* emb, int n_char, int E, const float* conv_w,
                               const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, const float* Output_WT,
                               const float* Output_b, int ld_feat, int L, int dtype, int k, int group_rows, int64_t max_nnz,
                               int lanes, int want_scores, int result_blocks, dae_pipeline** out);
int dae_pipeline_submit_titled(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                               int n_rows, const int32_t* titles, const float* titles_use, uint64_t* ticket_out);
int dae_pipeline_flush(dae_pipeline* p);
int dae_pipeline_poll(dae_pipeline* p, int wait, uint64_t* ticket, const int32_t** idx, const float** score, int* n_rows,
                      int* block);
int dae_pipeline_release(dae_pipeline* p, int block);
int dae_pipeline_stats(dae_pipeline* p, uint64_t out3[3]);
/* Where the host side of the loop spent its time since creation, nanoseconds: {the library thread issuing launches, the
 * library thread waiting for a staged launch, the caller inside dae_pipeline_submit, the caller waiting in dae_pipeline_poll}. */
int dae_pipeline_times(dae_pipeline* p, uint64_t out4[4]);
/* dae_set_exact_margin for the pipeline's own decoder image (re-tiled here; no feed may be in flight). */
int dae_pipeline_exact_margin(dae_pipeline* p, float scale);
const char* dae_pipeline_last_error(const dae_pipeline* p);

/* ---- ranking metrics on the device (the reference's utils/metrics.py: get_r_precision, get_ndcg, get_rsc) ------------------
 *
 * The RecSys Challenge 2018 is judged on R-precision, NDCG and recommended-songs clicks.  An evaluation needs three numbers
 * per playlist, not its k indices: dae_rank_metrics reads the top-k lists where the rankers wrote them and leaves one
 * 24-byte record per row.  The definitions, per row:
 *
 *   cand   = the entries >= 0 of the row's list idx[row * ld .. + k), in order (the rankers pad the tail with -1);
 *   answer = ans_col[ans_row_ptr[row] .. ans_row_ptr[row + 1]): int ids, unsorted, -1 (a track outside the vocabulary: it
 *            hits nothing and counts in n) and duplicates allowed, any length n;  hit(p) = cand[p] is one of them.
 *   hits_r   = number of p < min(n, len(cand)) with hit(p)                      -> r-precision = hits_r / n
 *   first    = the smallest p with hit(p), -1 when there is none                -> clicks = first / 10 (integer), 51 for -1
 *   m        = number of p >= 1 with hit(p)
 *   dcg      = (hit(0) ? 1.0 : 0.0), then += disc[p] for every hit p >= 1 in ASCENDING p, in float64
 *              -> NDCG = dcg / (1.0 + disc[1] + ... + disc[m]), the reference's ideal DCG: it grows with the number of hits,
 *                 not with n (metrics.py:29-42, kept as is)
 *   n_answer = n; 0 marks the record INVALID (an empty answer row: the reference divides by zero there, nothing is divided here)
 *
 * disc [k] float64 is the CALLER's table, disc[p] = 1 / log2(p + 1) as the caller's own logarithm gives it (disc[0] is never
 * read): with Python's 1 / math.log(p + 1, 2) the records reproduce utils/metrics.py bit for bit -- the kernel only adds, one
 * lane order, never reassociated, and the divisions are the host's.  An EMPTY cand (a list of -1 only), which get_ndcg cannot
 * answer (IndexError), is defined as dcg = 0, m = 0, first = -1: NDCG 0.0, clicks 51.
 * 1 <= k <= 1024, ld >= k; device pointers; asynchronous on the context's stream. */
typedef struct dae_metric_rec {
    int32_t hits_r, first, m, n_answer;
    double dcg;
} dae_metric_rec;
int dae_rank_metrics(dae_ctx* ctx, const int32_t* idx, int64_t ld, int B, int k, const int32_t* ans_row_ptr,
                     const int32_t* ans_col, const double* disc, dae_metric_rec* out);

/* The pipeline's EVALUATION mode (main_train.py:48-100 for every test split): the feeds come with their answers and what
 * leaves the device is each row's dae_metric_rec -- the lists never cross the link.
 *   enable_eval : once, before the first submit (DAE_ERR_STATE after it).  disc_host [k] float64 (HOST; see dae_rank_metrics);
 *                 max_answers = answer ids one launch may hold (a launch closes when the next feed's would not fit).
 *   submit_eval : dae_pipeline_submit / _submit_titled (titles, titles_use NULL: a plain feed) plus the feed's answers as a
 *                 HOST CSR: ans_row_ptr [n_rows + 1] (any base), ans_col int32.  Staged and uploaded with the feed.
 *   poll_eval   : dae_pipeline_poll with *rec -> the feed's [n_rows] records inside pinned result block *block.
 * dae_rank_metrics runs on the lane's stream behind the scoring call; coalescing, lanes, ordering, DAE_PIPE_BUSY and release
 * are the pipeline's as above, and so is the exact mode's guard: a launch that is re-scored in fp32 has its metrics
 * recomputed from the fp32 lists before they go out.  An eval pipeline takes only submit_eval / poll_eval, every other
 * pipeline only submit / submit_titled / poll: the wrong call returns DAE_ERR_STATE. */
int dae_pipeline_enable_eval(dae_pipeline* p, const double* disc_host, int64_t max_answers);
int dae_pipeline_submit_eval(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                             int n_rows, const int32_t* titles, const float* titles_use, const int32_t* ans_row_ptr,
                             const int32_t* ans_col, uint64_t* ticket_out);
int dae_pipeline_poll_eval(dae_pipeline* p, int wait, uint64_t* ticket, const dae_metric_rec** rec, int* n_rows, int* block);

/* ---- caller-given candidate columns (csrc/candidates.hip) -----------------------------------------------------------------
 *
 * What the reference answers with a slice of the dense matrix: main_train.py:66 / main_challenge.py:80 `sess.run(model.y_pred)`
 * followed by y_pred[r][cols] -- the scores of a FEW columns per playlist (a second-stage reranker's candidates, held-out
 * answers among sampled negatives, a market's catalogue) -- here without the [B, V] matrix: per listed (row, column) the
 * canonical fp32 chain of dae_decode_dense (fmaf over k = 0 .. H-1 from +0, then + b[c]) against the model's own row-major
 * tensors, bit for bit the dense value at [r, c].  No prepacked image is needed.
 *
 * The candidates are a CSR on the device: cand_row_ptr [B + 1] (starting at 0), cand_col [n_cand] int32 GLOBAL column ids,
 * tracks and artists in any order, duplicates allowed; n_cand = cand_row_ptr[B], passed by the caller (it sizes the launch:
 * nothing is read back; nothing at or past n_cand is touched).  An id of -1 is padding: its slot receives -inf.  Any other id
 * outside [0, V) receives a quiet NaN, is never dereferenced and ORs bit 0 into *status (DEVICE int32, nullable; the caller
 * zeroes it).  1 <= B <= 4096, H % 4 == 0, H <= 1024; the tensors 16-byte aligned.  Asynchronous on the context's stream;
 * only dae_score_candidates (hidden rows) and dae_rank_candidates (the pair lists) use the context's scratch.
 *
 * dae_decode_candidates: out[i] = (out_kind == DAE_OUT_SCORE ? sigmoid : id)(h[r,:] . W_dec[c,:] + b_dec[c]) for c = cand_col[i]
 *   of row r, in the order of cand_col (DAEs.py:73-77 tied -- pass the encoder matrix -- / :141-145 untied).
 * dae_score_candidates: the same behind dae_encode with the inference keep-probabilities on the batch CSR (DAEs.py:64-70); the
 *   hidden rows stay in the context's scratch, as dae_score_topk keeps them.
 * dae_mix_candidates (on the title scorer's context; `dae` the DAE's, same stream): the TITLED score of the same pairs,
 *   out[i] = sigmoid(feat[r,:] . OutW_T[c,:] + Out_b[c]) * w_title[r] + sigmoid(h[r,:] . W_dec[c,:] + b_dec[c]) * w_playlist[r]
 *   (DAEs.py:176-181) with dae_mix_scores' operations in its order: dae_decode_dense x 2 + dae_mix_scores at [r, c], bit for
 *   bit.  OutW_T [V][ld_feat] = Output_W^T zero padded, feat [B][ld_feat]; ld_feat % 4 == 0, ld_feat <= 1024.
 * dae_rank_candidates: the k best candidates of every row by `key` [n_cand] (the logits of dae_decode_candidates /
 *   dae_score_candidates with DAE_OUT_LOGIT, or the mixed scores of dae_mix_candidates), what main_challenge.py:26-36 does to
 *   a whole row: key descending, then column ascending; the row's seeds removed; out_idx / out_score [B, k], slots beyond the
 *   list (-1, -inf).  out_score follows out_kind for logits; for mixed keys pass DAE_OUT_LOGIT: it then holds y, as under
 *   dae_set_score_mix.  The existing selection kernel ranks the lists (no kernel of its own): they are written at a fixed row
 *   stride, so the call takes row_cap >= the longest row (entries of a row beyond row_cap are not ranked) and V (ids outside
 *   [0, V), -1 included, are absent; the seed bitmap covers [0, V)).  A column listed twice is ranked twice: de-duplicate
 *   before the call (models/DAEs.py does on the host, dae_candidates_unique on the device).  1 <= k <= 4096.  Scratch: 8 bytes x B x row_cap. */
#define DAE_CAND_CHUNK 256    /* candidates of one row a workgroup of the candidate kernels takes (a lane each) */
int dae_decode_candidates(dae_ctx* ctx, const float* h, int64_t ld_h, int B, int H, const float* W_dec, const float* b_dec, int V,
                          const int32_t* cand_row_ptr, const int32_t* cand_col, int n_cand, int out_kind, float* out,
                          int32_t* status);
int dae_score_candidates(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                         const float* b_enc, int V, int H, int B, const float* W_dec, const float* b_dec,
                         const int32_t* cand_row_ptr, const int32_t* cand_col, int n_cand, int out_kind, float* out,
                         int32_t* status);
int dae_mix_candidates(dae_ctx* title_ctx, dae_ctx* dae, const float* h, int64_t ld_h, int H, const float* W_dec,
                       const float* b_dec, const float* feat, int64_t ld_feat, const float* OutW_T, const float* Out_b,
                       const float* w_title, const float* w_playlist, int B, int V, const int32_t* cand_row_ptr,
                       const int32_t* cand_col, int n_cand, float* out, int32_t* status);
int dae_rank_candidates(dae_ctx* ctx, int B, int V, const int32_t* cand_row_ptr, const int32_t* cand_col, const float* key,
                        int row_cap, const int32_t* seed_row_ptr, const int32_t* seed_col, int k, int out_kind,
                        float* out_score, int32_t* out_idx);
/* dae_candidates_unique: the de-duplication dae_rank_candidates asks for, on the device.  cand_col_out[i] = cand_col_in[i], except
 *   that of all occurrences of a column within ONE row exactly one keeps its id and every other one becomes -1 (padding: absent
 *   for the ranking, -inf for the scoring calls).  Which occurrence survives is unspecified; it changes no output of
 *   dae_rank_candidates, because a column's key does not depend on its position.  -1 and ids outside [0, V) pass through
 *   untouched; nothing at or past n_cand is read or written; in == out is allowed (in place).  One workgroup per row with a
 *   bitmap over [0, V) in LDS, the row walked in chunks of DAE_CAND_CHUNK: V <= DAE_CAND_UNIQUE_MAX_V, a wider vocabulary is
 *   refused.  1 <= B <= 4096.  Asynchronous on the context's stream, no scratch. */
#define DAE_CAND_UNIQUE_MAX_V 1048576    /* a 128 KiB bitmap: the width at which the selection kernel gives up its own seed bitmap */
int dae_candidates_unique(dae_ctx* ctx, int B, int V, const int32_t* cand_row_ptr, const int32_t* cand_col_in, int32_t* cand_col_out,
                          int n_cand);

/* The pipeline's CANDIDATES mode: the three calls above over a stream of feeds -- a reranker's candidates, held-out answers among
 * sampled negatives, a market's columns, for very many playlists -- without a CSR build, an upload, a launch, a fetch and a
 * synchronisation per batch on the caller's side.  Every feed brings its candidate ids; what comes back is the value of every
 * listed pair (rank = 0) or each row's k best candidates (rank = 1).
 *   enable_candidates : once, before the first submit (DAE_ERR_STATE after it, on an evaluation pipeline and on a pipeline with a
 *                 catalogue; dae_pipeline_enable_eval and dae_pipeline_set_catalogue refuse a candidates pipeline in turn).
 *                 max_candidates = candidate ids one launch may hold (a launch closes when the next feed's would not fit, as with
 *                 max_answers).  rank = 0: the values of the listed pairs; rank = 1: per row the k best of its candidates, k as
 *                 the pipeline was created.  out_kind = DAE_OUT_SCORE or DAE_OUT_LOGIT (the values of rank = 0, the score column
 *                 of rank = 1); a titled pipeline takes DAE_OUT_SCORE only: the title mix has no logit.  group_rows <= 4096,
 *                 H % 4 == 0, H <= 1024 (the candidate kernels' limits).
 *   submit_candidates : dae_pipeline_submit / _submit_titled (titles, titles_use NULL: a plain feed) plus the feed's candidates as
 *                 a HOST CSR: cand_row_ptr [n_rows + 1] (any base), cand_col int32 GLOBAL column ids -- tracks and artists, -1
 *                 padding, duplicates allowed.  Staged and uploaded with the feed.  A feed with more ids than max_candidates is
 *                 refused (DAE_ERR_ARG: score it per batch); a refused feed leaves nothing staged, the pipeline takes the next.
 *   poll_candidates : rank = 0.  dae_pipeline_poll with *out -> the feed's *n_out floats inside pinned result block *block, in
 *                 the order of the feed's cand_col: -inf beside a -1, a quiet NaN beside another id outside [0, V).  The launch's
 *                 status word travels with the block: the call returns DAE_PIPE_BAD_ID (> 0, the results are valid and the
 *                 block is out) for every feed of a launch that held such an id -- a NaN then marks a bad id, not arithmetic.
 *                 rank = 1: the lists leave through dae_pipeline_poll ([n_rows, k], (-1, -inf) beyond a row's candidates,
 *                 scores when want_scores; an id outside [0, V) is absent).  The wrong poll for the mode: DAE_ERR_STATE.
 * What a lane issues per launch is nothing new: plain launches dae_score_candidates, titled ones the pipeline's title preamble
 * and dae_mix_candidates; rank = 1 runs dae_candidates_unique in front and dae_rank_candidates behind, over the logits (plain) or
 * the mixed values (titled, DAE_OUT_LOGIT: the score column holds y), seeds = the playlist's own tracks, row_cap = the launch's
 * longest row.  The chain is fp32 whatever dtype the pipeline was created with and reads no packed image.  Rows are independent:
 * every feed gets the bits those calls give it alone; coalescing, lanes, ordering, DAE_PIPE_BUSY, release and stats as above.
 * Memory: per launch slot 8 bytes per id (cand_col and the values, device; 4 pinned) and a row pointer; per result block
 * 4 * max_candidates pinned bytes instead of the lists (rank = 0); dae_rank_candidates' scratch in the lane's context. */
#define DAE_PIPE_BAD_ID 2
int dae_pipeline_enable_candidates(dae_pipeline* p, int64_t max_candidates, int rank, int out_kind);
int dae_pipeline_submit_candidates(dae_pipeline* p, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                                   int n_rows, const int32_t* titles, const float* titles_use, const int32_t* cand_row_ptr,
                                   const int32_t* cand_col, uint64_t* ticket_out);
int dae_pipeline_poll_candidates(dae_pipeline* p, int wait, uint64_t* ticket, const float** out, int64_t* n_out, int* n_rows,
                                 int* block);

/* ---- rank_of: the exact rank of given tracks among ALL rankable tracks of a row (csrc/rank_of.hip) --------------------------
 *
 * Where does this track stand for this playlist -- what MRR, mean / median rank, AUC, a recall curve at every cut-off and
 * hard-negative mining ask, and what no top-k list answers below position k -- without the [B, V] matrix, a sort and a search.
 *
 * The answers are a CSR on the device, as dae_rank_metrics and the candidate calls take theirs: ans_row_ptr [B + 1], ans_col
 * [n_ans] int32 GLOBAL column ids in any order, duplicates allowed; n_ans is passed by the caller (nothing is read back to size
 * a launch; nothing at or past n_ans is touched).  For answer i, column c of row r:
 *   UNRANKABLE: rank[i] = -1 when c == -1 (padding), c >= n_tracks (an artist column) or c is one of the row's seeds.
 *   OUT OF RANGE: any other id outside [0, V) also gives -1, is never dereferenced and ORs bit 0 into *status (DEVICE int32,
 *     nullable; the caller zeroes it), as in the candidate calls.
 *   OTHERWISE rank[i] = the number of columns c' in [0, n_tracks), c' != c, c' no seed of r, that PRECEDE c in the library's
 *     canonical order: fp32 logit descending under the composite key (orc_okey's order: -0 equal to +0, a NaN where that key
 *     puts it), ties broken by column ascending.  Ranks are 0-based, so rank_of(r, list[r][p]) == p for every position p of a
 *     list the fp32 (or exact-bf16) ranking calls return for the same seeds.  A duplicated answer gets the same rank twice.
 *   out_logit [n_ans] (nullable): the answer's canonical fp32 logit (the value of dae_decode_dense at [r, c], bit for bit);
 *     -inf beside rank -1 for padding, artists and seeds; NaN for an out-of-range id, like dae_decode_candidates.
 * Arithmetic: fp32 only -- a rank is a statement about the canonical fp32 logits, which DAE_DTYPE_F32 and DAE_DTYPE_BF16_EXACT
 * list by; a DAE_DTYPE_BF16 list may differ from them in its tail.
 *
 * The context must hold a plain DAE_DTYPE_F32 image over [0, V) of the same weights (dae_prepack_decoder): no fp32 image, a
 * catalogue image or a shard image (col_lo > 0 or col_hi < V) give DAE_ERR_STATE, the message saying which.  1 <= B <= 4096;
 * H % 4 == 0, H <= 1024; 1 <= n_tracks <= V; W_dec 16-byte aligned.  Any number of answers per row, 0 included: a row with more
 * than one pass of the counting launch holds (dae_rank_of_plan's C) takes more passes of the GEMM inside the same launch.
 * Asynchronous on the context's stream; all scratch (24 bytes per answer) sits in the context, and a steady state allocates
 * nothing; the counters are zeroed by the call itself.  Every refusal (a null pointer other than out_logit / status / both
 * seed arrays, n_ans < 0, a bad n_tracks, seeds given half, the image) comes before any launch.
 * dae_score_rank_of: the same behind dae_encode with the inference keep-probabilities, as dae_score_candidates.
 * dae_rank_of_plan: out = {rows per row group, answers of a row per pass C, row groups, workgroups per row group} of a call of
 *   these sizes (csrc/rank_of_plan.h); host only.
 *
 * dae_mix_rank_of (on the TITLE scorer's context; `dae` the DAE's, same stream): the same ranks under the TITLE MIX, the score
 *   `--challenge` ranks for every titled batch,
 *       y[r, c] = sigmoid(feat[r,:] . OutW_T[c,:] + Out_b[c]) * w_title[r] + sigmoid(h[r,:] . W_dec[c,:] + b_dec[c]) * w_playlist[r]
 *   with dae_mix_scores' operations in its order (the value of dae_mix_candidates at [r, c], bit for bit, and the value the titled
 *   ranking calls list by).  The contract is dae_decode_rank_of's with "fp32 logit" replaced by "mixed score y": the order is y
 *   descending under the same composite key, ties -- the common case, since sigmoids saturate -- by column ascending; out_score
 *   [n_ans] (nullable) holds y, -inf beside rank -1 for padding, artists and seeds, NaN for an out-of-range id (which ORs bit 0
 *   into *status).  Every row is ranked by y, rows with w_title == 0 included.  Arguments as dae_mix_candidates takes them (h [B][H]
 *   contiguous: ld_h == H; feat [B][ld_feat], OutW_T [V][ld_feat]; ld_feat % 4 == 0, ld_feat <= 1024; both tensors 16-byte aligned),
 *   then n_tracks, the seed CSR and the answers as above.  BOTH contexts must hold a plain DAE_DTYPE_F32 image over [0, V) (the
 *   title context's of OutW_T / Out_b, the DAE's of W_dec / b_dec) and be bound to one stream: no fp32 image, a catalogue image, a
 *   shard image, or dae_set_score_mix left set on either give DAE_ERR_STATE, the message naming the context; every refusal comes
 *   before any launch.  Launches (all on the shared stream, nothing read back): dae_mix_candidates over the answers,
 *   dae_decode_mix_term on the DAE's context, the memset, the sort, the counting launch with a mix epilogue over the title image,
 *   the finishing launch (the seeds leave by their mixed value).  Geometry: dae_rank_of_plan(B, ld_feat, n_ans).  Scratch, all in
 *   the title context (the DAE's keeps its packed hidden rows): 24 bytes per answer, plus 4 x B x nt32 bytes for the DAE's term
 *   (nt32 = n_tracks rounded up to 32, never past V); a steady state allocates nothing.
 * NOT BUILT: a bf16 count (the thresholds would have to come out of the bf16 MFMA chain), vocabulary shards, catalogue images,
 * the pipeline (plain and titled alike). */
int dae_rank_of_plan(int B, int H, int n_ans, int32_t out[4]);
int dae_decode_rank_of(dae_ctx* ctx, const float* h, int B, int H, const float* W_dec, const float* b_dec, int V, int n_tracks,
                       const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr, const int32_t* ans_col,
                       int n_ans, int32_t* out_rank, float* out_logit, int32_t* status);
int dae_score_rank_of(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                      const float* b_enc, int V, int H, int B, const float* W_dec, const float* b_dec, int n_tracks,
                      const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr, const int32_t* ans_col,
                      int n_ans, int32_t* out_rank, float* out_logit, int32_t* status);
int dae_mix_rank_of(dae_ctx* title_ctx, dae_ctx* dae, const float* h, int64_t ld_h, int H, const float* W_dec,
                    const float* b_dec, const float* feat, int64_t ld_feat, const float* OutW_T, const float* Out_b,
                    const float* w_title, const float* w_playlist, int B, int V, int n_tracks,
                    const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr,
                    const int32_t* ans_col, int n_ans, int32_t* out_rank, float* out_score, int32_t* status);

/* ---- a catalogue: rank a SHARED subset of the track columns (csrc/catalogue.hip) -------------------------------------------
 *
 * "The k best tracks among THESE columns, the same for every row" -- a market's catalogue, the non-explicit tracks, the tracks
 * still licensed, a second generator's pool: main_challenge.py:26-36's ranking with `cand` restricted to a column set.  The
 * candidate calls above answer it per row from the row-major tensors and lose to a dense decode from a few thousand columns per
 * row on; handing the complement to every row as seeds decodes the whole vocabulary to discard most of it.  A catalogue call
 * ranks an image made of the catalogue's decoder rows alone with the fused path of dae_score_topk: n columns of work, not V,
 * the same kernels and plans, the same bits.
 *
 * dae_catalogue_create: cols [n] (DEVICE int32) are GLOBAL track columns, STRICTLY ASCENDING (each once), inside [0, n_tracks),
 *   1 <= n <= n_tracks.  One launch validates the list and builds the inverse table local_of[n_tracks] (-1: not in the
 *   catalogue); the call copies the list, reads one status word back and so synchronises the context's stream (once per
 *   catalogue).  A violation: DAE_ERR_ARG, the message naming the first offending position and its value.  Memory: 4 (n + n_tracks)
 *   bytes.  Ascending order is the contract everything else rests on: local order equals global order, so the canonical
 *   tie-break (key descending, column ascending) is the same in both spaces.  The object belongs to ctx's device and is used
 *   read-only: any number of contexts of that device may rank with it.  dae_catalogue_destroy waits for the device first.
 * dae_prepack_decoder_catalogue: the context's image of `dtype` from rows cols[0 .. n) of the caller's row-major W_dec [V, H] and
 *   b_dec[cols] (V >= n_tracks; a title scorer's Output_W^T / Output_b likewise): LOCAL columns [0, n), col_lo = 0, no artist
 *   part, with everything dae_prepack_decoder leaves with an image -- the fp32 per-tile {A_t, M_t} bounds and the per-column
 *   lower bounds of the threshold sample, the exact mode's eps_c under dae_set_exact_margin (dae_set_exact_margin_range then
 *   names LOCAL columns) -- all computed from the gathered rows: a bound of a tile covers the 32 catalogue columns it holds.
 *   The rows are gathered into a temporary [n, H] that is freed before the call returns (it synchronises the stream); the image
 *   itself is n x H x 4 (fp32) or 2 (bf16) bytes plus bounds, and under DAE_DTYPE_BF16_EXACT the fp32 rows as well.  The image
 *   records which catalogue it was gathered from; any other prepack of the slot forgets it.
 * dae_score_topk_catalogue / dae_decode_topk_catalogue: dae_score_topk / dae_decode_topk with `cat` in the place of n_tracks.
 *   Seeds are GLOBAL columns, as everywhere else; out_idx holds GLOBAL columns, -1 padding.  n_seeds: the entries of seed_col,
 *   seed_row_ptr[B], passed by the caller as n_cand is to the candidate calls -- it sizes the translated lists in the context's
 *   scratch, nothing is read back and nothing at or past it is written (0 with NULL seeds).  Inside, per slab of 4096 rows:
 *   (a) two small launches translate the seed CSR into the image's columns -- per row the seeds that lie in the catalogue, in
 *   order, with fresh row pointers; seeds outside it cannot be ranked, and dropping them keeps the thresholds' k + n_seeds
 *   tight -- (b) the existing call runs on the image with n_tracks = n, (c) one launch maps out_idx through cols in place.
 *   The result is, bit for bit, the canonical ranking of the FULL image's logits restricted to the catalogue's columns: a logit
 *   depends on its own decoder row and the hidden row only, and every kernel runs the canonical chain per element.
 *   k: as the underlying call (4096; 1024 with DAE_DTYPE_BF16_EXACT).  An image that was not gathered from `cat` (a plain
 *   image, another catalogue's): DAE_ERR_STATE.  Every refusal comes before any launch.
 * dae_title_score_catalogue: dae_title_score plus `cat`, for DAE_DTYPE_F32 / DAE_DTYPE_BF16 (DAE_DTYPE_BF16_EXACT: DAE_ERR_ARG
 *   before any launch -- rank with DAE_DTYPE_F32, the same lists).  BOTH contexts hold catalogue images of `dtype` gathered from
 *   the same `cat`: the DAE's decoder and the title scorer's Output_W^T / Output_b.  The feed keeps its global columns (CSR,
 *   encode, mixing weights, seeds = the playlist's own tracks < n_tracks, which must be the catalogue's n_tracks); the seeds are
 *   translated behind that, the mix term and the ranking run over the n local columns, the indices are mapped back.
 *   n_rows <= 4096. */
typedef struct dae_catalogue dae_catalogue;
int dae_catalogue_create(dae_ctx* ctx, const int32_t* cols, int n, int n_tracks, dae_catalogue** out);
int dae_catalogue_destroy(dae_catalogue* cat);
int dae_prepack_decoder_catalogue(dae_ctx* ctx, const dae_catalogue* cat, const float* W_dec, const float* b_dec, int V, int H,
                                  int dtype);
int dae_score_topk_catalogue(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                             const float* b_enc, int V, int H, int B, int dtype, const dae_catalogue* cat,
                             const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seeds, int k, int out_kind,
                             float* out_score, int32_t* out_idx);
int dae_decode_topk_catalogue(dae_ctx* ctx, const float* h, int B, int H, int dtype, const dae_catalogue* cat,
                              const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seeds, int k, int out_kind,
                              float* out_score, int32_t* out_idx);
int dae_title_score_catalogue(dae_ctx* title_ctx, dae_ctx* dae, int dtype, const int64_t* positions, const float* values,
                              int values_broadcast, int64_t nnz, int n_rows, int V, const float* W_enc, const float* b_enc, int H,
                              const int32_t* titles, int L, const float* emb, int n_char, int E, const float* conv_w,
                              const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, int ld_feat,
                              const float* titles_use, int n_tracks, int k, float* out_score, int32_t* out_idx,
                              int32_t* guard_out, int32_t* csr_status, const dae_catalogue* cat);

/* The pipeline inside a catalogue: from this call on EVERY launch of `p` ranks cat's columns -- plain launches as
 * dae_score_topk_catalogue ranks them, titled ones as dae_title_score_catalogue, bit for bit; lists (and, in evaluation mode, the
 * candidates of dae_rank_metrics) are global columns.
 *   Once, before the first submit (like dae_pipeline_enable_eval; either order): DAE_ERR_STATE afterwards, or when a catalogue is
 *   set already.  DAE_ERR_ARG: a catalogue of another device; one created over another n_tracks than the pipeline's; a titled
 *   pipeline of DAE_DTYPE_BF16_EXACT (dae_title_score_catalogue has no such mode: create the pipeline with DAE_DTYPE_F32, the same
 *   lists).  A refused call leaves the pipeline as it was.
 *   The pipeline gathers images of its OWN from the W_dec / b_dec (and Output_W^T / Output_b) it was created with: lane 0 tiles
 *   them, the other lanes borrow them, and an fp32 image a lane needs later (the exact mode's guard re-run) is the catalogue's too.
 *   The seed translation runs on the pipeline's preparation stream, behind the launch's CSR, into buffers of the launch slot
 *   (4 (2 group_rows + max_nnz) bytes per slot); the lane's stream carries the ranking and the map-back.
 *   Evaluation mode: dae_rank_metrics runs AFTER the map-back, so an answer outside the catalogue can never be hit and counts in
 *   the record's denominators, exactly as a -1 answer does; a caller who wants recall within the catalogue filters the answers
 *   on the host before it feeds them.
 *   LIFETIME: the pipeline keeps the pointer, not a copy -- the caller keeps `cat` alive until dae_pipeline_destroy(p) has
 *   returned. */
int dae_pipeline_set_catalogue(dae_pipeline* p, const dae_catalogue* cat);

/* ---- training step (DAEs.py:98-102) ------------------------------------------------------ */

/* Arithmetic of the three GEMMs of the training step of this context (forward hidden x W_dec^T, gW_dec = dz^T h,
 * dh = dz W_dec): DAE_DTYPE_F32 (default; fp32 MFMA) or DAE_DTYPE_BF16 (BASELINE.json configs[3]: operands
 * rounded to bf16 in registers / by the prepack, fp32 accumulate; the loss, dL/dz, the encoder gradient, the
 * parameters and Adam stay fp32; the backward GEMMs switch only when H % 128 == 0).  Sticky; applies to
 * dae_train_forward_backward and dae_train_shard_decode.  Replaces nothing in the reference (TF1 is fp32). */
int dae_set_train_dtype(dae_ctx* ctx, int dtype);

/* Forward + loss + backward for one batch.  x_* = input CSR (after the host coin flip
 * tracks-only / artists-only, main_train.py:202-213), y_* = target CSR (values are the y_ones
 * of the feed).  n_batch = the fixed graph batch the mean divides by (DAEs.py:100).
 * tied != 0: W_dec aliases W_enc (DAE_tied); gW_dec is then ignored and gW_enc receives both
 * gradients.  Gradients are dense fp32 buffers the caller owns (overwritten).
 * cost_out: device scalar = mean_rows(L) + reg_lambda * l2 (DAEs.py:79-82/:147-150, :100).
 * A target row may hold any number of entries (one per column: the CSR contract), under every train dtype;
 * the same holds for dae_train_shard_decode.
 * 1 <= B <= 4096 rows, H % 32 == 0, H <= 1024.  A batch above 256 rows is walked in panels of 256 rows (and a shorter last
 * one) by the decode side of the step -- loss, dL/dz, the decoder gradient and dh; DESIGN.md "Batches above 256 rows" --
 * with the same meaning: cost = (1 / n_batch) sum over all B rows + lambda l2, every gradient the sum over all B rows, the
 * dropout masks keyed by the row's index in the batch.  A batch of at most 256 rows is one panel: the launches it always
 * made.  Scratch beyond [B, H]-sized buffers does not grow with B. */
int dae_train_forward_backward(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
        int V, int H, int B, int n_batch, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* gW_enc, float* gb_enc, float* gW_dec, float* gb_dec,
        float* cost_out);

/* ---- the loss without a step: the cost of a batch and the loss of each of its rows ----------------------------------
 * What sess.run(model.cost, feed) on a held-out batch is in the reference: the forward pass and the loss head of the step
 * (DAEs.py:98-100), no gradient, no Adam.  Nothing per element is kept in memory (no dz^T, no logits): the decode GEMM sums
 * every element's negative term per row, the rows' targets are redone from their own dot products as in the step.
 *
 * dae_decode_loss_rows: row_loss[r] (device, [B]) = sum over ALL V columns c of L(z[r][c], y[r][c]) for the hidden rows
 * h [B][H] (row-major, 16-byte aligned), y = the target CSR (0 where it has no entry; one entry per (row, column): the CSR
 * contract; a row may hold any number; a column outside [0, V) is the caller's error and is left out).  The GEMM runs over
 * the context's prepacked image of `dtype` (DAE_DTYPE_F32 or DAE_DTYPE_BF16; dae_prepack_decoder over [0, V), as for
 * dae_decode_dense), the targets' chains over the row-major W_dec [V][H] / b_dec [V] the image was packed from (as the
 * candidate calls take them).  DAE_ERR_STATE when the context holds no image of that dtype over [0, V); DAE_ERR_ARG for
 * B outside [1, 4096], H % 32 != 0, H > 1024.
 *
 * dae_score_loss: the step's encode (the same dropout masks as dae_train_forward_backward for the same seed and keep
 * probabilities), then the call above in the arithmetic of dae_set_train_dtype, then
 *   cost_out (device scalar, nullable) = (float)(sum_r (double)row_loss[r] / n_batch + reg_lambda * l2),
 * l2 over the tensors the step counts (W_enc, b_dec, b_enc, and W_dec unless tied).  row_loss: device [B], nullable.
 * tied != 0: W_dec is ignored (W_enc is the decoder, and the image must be of it).  DAE_ERR_ARG also when both outputs are
 * null.  There are no 256-row panels: B up to 4096 is one GEMM launch.
 *
 * Both write only their outputs and context scratch (reserved for the call's own shape), and the packed hidden image as
 * every decode call does: never the parameters, the Adam moments, the armed decoder Adam, dae_set_enc_grad_prezeroed or a
 * prepacked image.  Every sum runs in an order fixed by indices (no float atomics): the same inputs give the same bits. */
int dae_decode_loss_rows(dae_ctx* ctx, const float* h, int B, int H, int dtype,
                         const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                         const float* W_dec, const float* b_dec, int V, float* row_loss);
int dae_score_loss(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
        int V, int H, int B, int n_batch, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* row_loss, float* cost_out);

/* ---- the loss of the title scorer's MIXED score without a step --------------------------------------------------------
 * What the title step (main_train.py:214-221, DAEs.py:176-196) reports as its cost, with no gradient and no Adam: per row r and
 * column c of ALL V columns, in the title step's fp32 operations and order (no contraction),
 *   st = 1.0f / (1.0f + __expf(-z_title[r][c]));  pd = sigmoid(z_dae[r][c]) * w_playlist[r]  (the canonical sigmoid: the element
 *   dae_decode_mix_term writes);  yp = st * w_title[r] + pd;
 *   L(r, c) = -[y ln(yp + 1e-10f) + 0.55f (1 - y) ln(1 - yp + 1e-10f)],  y = the target CSR (0 where it has no entry; one entry
 *   per (row, column); a row may hold any number; a column outside [0, V) is the caller's error and is left out, never read),
 *   row_loss[r] (device [B], nullable) = sum_c L(r, c),
 *   cost_out (device scalar, nullable) = (float)(sum_r (double)row_loss[r] / n_batch)   (the title cost has no lambda term).
 * Nothing per element is kept: the title GEMM over the prepacked image sums every element's y = 0 term per row, the targets are
 * redone from their own two fmaf chains (over Output_W^T [V][ld_feat] / Out_b and W_dec [V][H] / b_dec, the tensors the images
 * were packed from), which in fp32 give the bits the GEMMs saw, and add L(y) - L(0).
 *
 * Called on the TITLE scorer's context with `dae` the DAE's, both bound to one stream (as dae_mix_candidates); h [B][H]
 * (ld_h == H), feat [B][ld_feat], w_title / w_playlist [B] (dae_mix_weights).  Both contexts need their plain fp32 image over
 * [0, V) (dae_prepack_decoder): DAE_ERR_STATE otherwise.  DAE_ERR_ARG: both outputs null, B outside [1, 4096], H % 32 != 0,
 * H > 1024, ld_feat % 4 != 0, ld_feat > 1024, ld_h != H, n_batch <= 0, h / W_dec / feat / Output_W^T not 16-byte aligned.
 *
 * The call walks panels of at most 256 rows: dae_decode_mix_term (n_cols = V) on the DAE's context, the title GEMM, the
 * finishing launch per panel; one cost launch over all rows at the end.  The transposed term buffer is one panel's
 * (4 * V32 * 256 bytes at most, V32 = V rounded up to 32), in the title context's scratch, which grows only
 * (csrc/mix_loss_plan.h).  It writes only its outputs, that scratch and the two packed hidden images: never a parameter, an Adam
 * moment, the title trainer's state or a prepacked image, and what dae_set_score_mix left in either context is neither read
 * nor changed.  Every sum runs in an order fixed by indices (no float atomics): the same inputs give the same bits. */
int dae_mix_loss_rows(dae_ctx* title_ctx, dae_ctx* dae, const float* h, int64_t ld_h, int H, const float* W_dec,
                      const float* b_dec, const float* feat, int64_t ld_feat, const float* OutW_T, const float* Out_b,
                      const float* w_title, const float* w_playlist, int B, int V, int n_batch,
                      const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                      float* row_loss, float* cost_out);

/* ---- the same step with the vocabulary ROW-SHARDED over ranks (training) ------
 * Rank g owns rows [col_lo, col_hi) of W_enc, W_dec and b_dec (pointers *_loc address the shard's
 * own [col_hi-col_lo, H] / [col_hi-col_lo] arrays); b_enc is replicated.  Every rank receives the
 * whole batch CSR with GLOBAL column ids.  One step = three stages around the two exchanges the
 * path really has (the caller issues them: RCCL all-reduce(sum) over [B,H] fp32):
 *
 *   dae_train_shard_encode   pre_partial[B,H] = sum over own columns of xhat * W_enc_loc rows
 *                            (xhat normalised by the row's global sum, DAEs.py:40-42, :66)
 *        -- all-reduce pre_partial --
 *   dae_train_shard_decode   h = dropout(sigmoid(pre + b_enc)) (:67-68); decode + loss + dz over own
 *                            columns (:75/:143, :98-100); gW_dec_loc, gb_dec_loc; dh_partial[B,H];
 *                            cost_partial (device scalar: own columns' loss / n_batch + lambda * l2
 *                            of the tensors this rank owns; b_enc counted by the col_lo == 0 rank)
 *        -- all-reduce dh_partial and cost_partial --
 *   dae_train_shard_finish   dpre, gb_enc (replicated, identical on all ranks), row-sparse gW_enc_loc
 *
 * tied != 0: W_dec_loc is ignored (W_enc_loc is the decoder), stage "decode" writes the decoder
 * gradient into gW_out = gW_enc_loc and stage "finish" accumulates the encoder part on top.
 * untied: gW_out = gW_dec_loc.  Adam is local: dae_adam_step on the owned rows.
 * The stages keep h / sigmoid in ctx scratch between calls: run them in order on one ctx.
 * With a single shard [0, V) the result equals dae_train_forward_backward up to fp32
 * re-association in the encoder sum.
 * 1 <= B <= 4096 for all three stages, as for dae_train_forward_backward: stage "decode" walks the same 256-row panels
 * (no exchange happens inside the stage), the other two run over all rows at once. */
int dae_train_shard_encode(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const float* W_enc_loc, int col_lo, int col_hi, int H, int B,
        float ikp, uint32_t seed, float* pre_partial);
int dae_train_shard_decode(dae_ctx* ctx, const float* pre, const float* b_enc,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc_loc, const float* W_dec_loc, const float* b_dec_loc,
        int col_lo, int col_hi, int H, int B, int n_batch, int tied,
        float kp, uint32_t seed, float reg_lambda,
        float* gW_out, float* gb_dec_loc, float* dh_partial, float* cost_partial);
int dae_train_shard_finish(dae_ctx* ctx, const float* dh,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const float* W_enc_loc, const float* b_enc, const float* W_dec_loc, const float* b_dec_loc,
        int col_lo, int col_hi, int H, int B, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* gW_enc_loc, float* gb_enc, float* gW_dec_loc, float* gb_dec_loc);

/* ---- title scorer of the challenge path (models/title_models/Char_CNN.py, models/DAEs.py:153-181) ---- */

/* Char_CNN.py:23-62: titles [B,L] int32 character ids (-1 = padding, embeds to zero) -> embedding [n_char,E]
 * -> for each of n_sizes filter sizes (host array filter_sizes) a VALID convolution with F filters
 * (conv_w = the TF variables Conv_W0.. [fs_i, E, 1, F] back to back, conv_b = Conv_b0.. [n_sizes, F]) -> ReLU
 * -> max over time -> concat -> dropout(keep_prob) -> feat [B, ld] (ld >= n_sizes*F, zero padded so that the
 * result can go straight into dae_decode_dense as a "hidden" matrix of size ld).  argmax / feat_raw (both
 * [B, n_sizes*F], nullable) keep the max positions and the pre-dropout features for the backward pass.
 * The vocabulary-wide output layer sigmoid(feat . Output_W + Output_b) (:64-72) is the decoder GEMM:
 * dae_prepack_decoder(Output_W^T [V, ld], Output_b) + dae_decode_dense(apply_sigmoid = 1). */
int dae_title_features(dae_ctx* ctx, const int32_t* titles, int B, int L, const float* emb, int n_char, int E,
                       const float* conv_w, const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F,
                       float keep_prob, uint32_t seed, float* feat, int64_t ld, int32_t* argmax, float* feat_raw);

/* A FROZEN title scorer's convolutions as a table (scoring: main_challenge.py:80-90 runs Char_CNN.py:23-62 with fixed
 * variables on every batch).  Titles are rows of character ids, so the inner sum of the convolution over the embedding has
 * only fs x (n_char + 1) distinct terms per filter: T[d][c][f] = sum_e emb[c][e] Conv_W[d][e][f].  After this call,
 * dae_title_features / dae_title_score on this context, called with THESE emb / conv_w arrays, keep_prob = 1 and no argmax /
 * feat_raw, sum fs table entries per (position, filter) instead of fs x E products -- the same real number in another
 * summation order (a different fp32 rounding; the title path is specified to a tolerance, as TF's conv2d has no documented
 * order).  The caller calls it again after the variables changed, or with emb = NULL to drop the table (training does:
 * calls with keep_prob < 1 or argmax never use it). */
int dae_title_prepack_features(dae_ctx* ctx, const float* emb, int n_char, int E, const float* conv_w,
                               const int32_t* filter_sizes, int n_sizes, int F);

/* DAEs.py:180: dae_score[r, c] = title_score[r, c] * w_title[r] + dae_score[r, c] * w_playlist[r] over the first
 * ncols columns; the weights are DAEs.py:159-162 (x_count = row_sum * input_keep_prob; u / (u + x_count + 1e-10),
 * x_count / (u + x_count + 1e-10)), computed by the caller from the feed. */
int dae_mix_scores(dae_ctx* ctx, const float* title_score, int64_t ld_title, float* dae_score, int64_t ld_dae,
                   const float* w_title, const float* w_playlist, int B, int ncols);

/* The same mix WITHOUT the two [B, V] score matrices (what `--challenge` runs for titled batches, main_challenge.py:80-90
 * with DAE_title.y_pred of DAEs.py:176-181):
 *
 * dae_decode_mix_term (on the DAE's context): outT[c * ldT + r] = w_playlist[r] * sigmoid(h[r,:] . W_dec[c,:] + b_dec[c])
 *   for the prepacked columns c < n_cols (pass n_tracks: only track columns are ranked) -- the second term of
 *   DAEs.py:180, stored TRANSPOSED ([column][row], ldT >= B) so that both sides touch whole cache lines.  Whole
 *   32-column tiles are written: outT needs room for n_cols rounded up to a multiple of 32 (but never past the image).
 * dae_set_score_mix (on the title scorer's context, whose prepacked "decoder" is Output_W^T / Output_b): until
 *   cleared with (NULL, 0, 0, NULL), dae_decode_topk on this context ranks
 *       y[r, c] = sigmoid(feat[r,:] . Output_W[:, c] + Output_b[c]) * w_title[r] + mixT[c * ld + r]
 *   instead of the logit -- same operations and order as dae_mix_scores, so the result is bit-identical to
 *   dae_mix_scores + dae_topk_dense(DAE_OUT_LOGIT) -- through the fused threshold path (sample tiles -> tau -> filter
 *   -> top-k); out_score holds y whatever out_kind says.  mixT ([n_cols][ld], columns past n_cols count as 0) and
 *   w_title are caller-owned device arrays. */
int dae_decode_mix_term(dae_ctx* ctx, const float* h, int B, int H, int dtype, const float* row_scale, int n_cols,
                        float* outT, int64_t ldT);
int dae_set_score_mix(dae_ctx* ctx, const float* mixT, int64_t ld, int n_cols, const float* w_title);

/* ---- ensembles: rank by a weighted sum of several DAEs' scores ----
 * THE CANONICAL VALUE.  M >= 1 members in the caller's order m = 0 .. M-1, each with its own encoder and decoder over the same
 * V columns / n_tracks tracks (hidden sizes may differ).  z_m[r,c]: member m's canonical fp32 logit of its own hidden row (the
 * chain of dae_decode_dense); a_m[r]: a per-row fp32 weight.  Every operation a single fp32 rounding, no contraction, in this
 * order:
 *     t_m[r,c] = dae_sigmoidf(z_m[r,c]) * a_m[r]
 *     acc      = t_0;   acc = acc + t_m   for m = 1 .. M-2        (untitled: the last member is not in acc)
 *     untitled:  y = t_{M-1} + acc                                (M = 1: y = t_0)
 *     titled:    acc also takes t_{M-1};  y = dae_sigmoidf(z_title) * w_title[r] + acc
 * -- the operations and order of dae_mix_scores and of the fused mix above: titled, M = 1, a_0 = w_playlist is the title mix
 * bit for bit; untitled, M = 2 is dae_decode_mix_term + dae_set_score_mix + dae_decode_topk.  Ranked in the library's canonical
 * order over the track columns: y descending, then column ascending, seeds removed, (-1, -inf) padding; out_score holds y.
 *
 * dae_decode_mix_term_add: accT[c * ldT + r] = accT[c * ldT + r] + sigmoid(h[r,:] . W_dec[c,:] + b_dec[c]) * row_scale[r] --
 *   a further member's term added to the buffer dae_decode_mix_term wrote: the same columns and whole 32-column tiles (never
 *   past the image), rows >= B untouched, DAE_DTYPE_F32 and DAE_DTYPE_BF16 images, any hidden size dae_decode_dense takes.  A
 *   read-modify-write: one call at a time per buffer.
 * dae_ensemble_topk: the ranking half in one call, on resident inputs.  members / h / H / row_scale: HOST arrays of M entries --
 *   member m's context (holding its decoder prepacked in `dtype` over all V columns), its hidden rows [B][H[m]] and its weights
 *   a_m [B] (device arrays).  title_ctx (nullable) with feat [B][ld_feat] / w_title [B]: the titled form; without it feat and
 *   w_title are NULL.  It launches dae_decode_mix_term for member 0, dae_decode_mix_term_add for the other members that go into
 *   acc, then dae_set_score_mix + dae_decode_topk on the RANKING context -- the title context, or member M-1's -- and clears the
 *   mix.  Scratch: the 4 * B * nt32 bytes of the term (nt32 = n_tracks rounded up to 32, never past V) in the ranking context,
 *   which also takes the error message.  Refused before any launch: null pointers or half a seed CSR (DAE_ERR_ARG);
 *   DAE_DTYPE_BF16_EXACT; k outside [1, 1024]; B > 4096; a context on another device, or bound to another stream (DAE_ERR_STATE);
 *   a context with no image of `dtype`, with a catalogue image or a shard image, or with dae_set_score_mix set (DAE_ERR_STATE);
 *   a context listed twice; images of different V or an H that is not its image's. */
int dae_decode_mix_term_add(dae_ctx* ctx, const float* h, int B, int H, int dtype, const float* row_scale, int n_cols,
                            float* accT, int64_t ldT);
int dae_ensemble_topk(dae_ctx* const* members, int M, const float* const* h, const int* H, const float* const* row_scale,
                      dae_ctx* title_ctx, const float* feat, int ld_feat, const float* w_title, int B, int dtype, int n_tracks,
                      const int32_t* seed_row_ptr, const int32_t* seed_col, int k, float* out_score, int32_t* out_idx);

/* ---- ranks under the ensemble (csrc/ensemble.hip, csrc/rank_of.hip; DESIGN.md section 4e "Ranks under the ensemble") ----
 * Both calls take the scorers as dae_ensemble_topk takes them -- members / h / H / row_scale: HOST arrays of M entries; title_ctx
 * (nullable) with feat [B][ld_feat] / w_title [B] -- plus what the candidate chains read: W_dec / b_dec, HOST arrays of the
 * members' row-major [V][H[m]] decoder tensors and [V] biases (device arrays, 16-byte aligned), and OutW_T [V][ld_feat] / Out_b
 * of the title scorer (all four title arguments NULL when untitled).  Both run on the RANKING context of dae_ensemble_topk --
 * the title context, or member M-1's -- which takes the scratch and the messages; every context on one device and one stream,
 * none listed twice, none with dae_set_score_mix set.  Always fp32.
 *
 * dae_ensemble_candidates: out[i] = the canonical value y (above) of column cand_col[i] for its row, for the candidate CSR of
 *   dae_decode_candidates (cand_row_ptr [B + 1], cand_col, the host-known n_cand; nothing at or past n_cand is touched, nothing
 *   is read back).  Per scorer dae_decode_candidates with DAE_OUT_SCORE -- the canonical chain over the row-major tensors, the
 *   title scorer's over feat / OutW_T / Out_b -- into scratch, then one combining launch per 8 members: t_m = s_m * a_m[row], acc
 *   over m ascending, y as above, every product and sum a single fp32 rounding.  Bit for bit the value dae_ensemble_topk lists
 *   by and DAE_ensemble.score_candidates computes.  Ids: -1 gives -inf; another id outside [0, V) gives a quiet NaN and ORs bit 0
 *   into *status (DEVICE int32, nullable).  1 <= B <= 4096; H[m] and ld_feat multiples of 4, at most 1024.  No image is needed.
 *   Scratch: 4 * (M (+ 1)) * n_cand bytes (csrc/ensemble_rank_of_plan.h).
 * dae_ensemble_rank_of: dae_mix_rank_of's contract under y -- per listed (row, column) the 0-based number of non-seed track
 *   columns that precede it, y descending under the composite key, then column ascending; -1 for padding, artists, seeds and ids
 *   out of range (which OR bit 0 into *status); out_score (nullable) holds y, -inf beside a -1 (NaN for an id out of range).
 *   n_seed: the length of seed_col, an upper bound of seed_row_ptr[B] (slots that belong to no row are never read); an
 *   out-of-range seed is ignored and raises no status.  EVERY context must hold a plain DAE_DTYPE_F32 image over [0, V) of its
 *   tensors.  Launches, all on the one stream: dae_ensemble_candidates' over the answers (the thresholds) and over the seed CSR
 *   (the seeds' values); the term buffer exactly as dae_ensemble_topk builds it ([nt32][B] in the ranking context;
 *   dae_decode_mix_term for member 0, dae_decode_mix_term_add for the others in acc, a -0.0f fill when there are none); the
 *   memset, the sort, the counting launch with the mix epilogue over the ranking scorer's image (weights: w_title, or a_{M-1}
 *   untitled), whose two operations are the combining launch's last two on the same operands -- an answer's own column meets its
 *   own value; the finishing launch, which takes each distinct seed out by its value from the seeds' pass.  Geometry:
 *   dae_rank_of_plan(B, H of the ranking scorer, n_ans).  Refused before any launch: everything dae_ensemble_topk refuses about
 *   its contexts; everything dae_decode_rank_of refuses about B, H, n_ans, alignment and half a seed CSR; n_seed < 0, or n_seed > 0
 *   without seeds; V that is not the images'.  n_ans == 0 returns DAE_OK and writes nothing.
 * NOT BUILT: a bf16 count, vocabulary shards, catalogues, the pipeline, one launch decoding all members per tile. */
int dae_ensemble_candidates(dae_ctx* const* members, int M, const float* const* h, const int* H, const float* const* row_scale,
                            const float* const* W_dec, const float* const* b_dec, dae_ctx* title_ctx, const float* feat,
                            int ld_feat, const float* OutW_T, const float* Out_b, const float* w_title, int B, int V,
                            const int32_t* cand_row_ptr, const int32_t* cand_col, int n_cand, float* out, int32_t* status);
int dae_ensemble_rank_of(dae_ctx* const* members, int M, const float* const* h, const int* H, const float* const* row_scale,
                         const float* const* W_dec, const float* const* b_dec, dae_ctx* title_ctx, const float* feat, int ld_feat,
                         const float* OutW_T, const float* Out_b, const float* w_title, int B, int V, int n_tracks,
                         const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seed, const int32_t* ans_row_ptr,
                         const int32_t* ans_col, int n_ans, int32_t* out_rank, float* out_score, int32_t* status);

/* DAE_DTYPE_BF16_EXACT for the title mix: the top-k of y = sigmoid(z_title) * w_title + sigmoid(z_dae) * w_playlist
 * (DAEs.py:176-181; what main_challenge.py:80-90 ranks for every titled batch) BIT-IDENTICAL to the fp32 path above
 * (dae_decode_mix_term + dae_set_score_mix + dae_decode_topk, or dae_mix_scores + dae_topk_dense), with both vocabulary-
 * wide GEMMs on v_mfma_f32_32x32x16_bf16: one launch decodes each 32-column tile against the hidden rows of BOTH scorers
 * on bounds of the two logits (sample: lower bounds -> threshold; filter: upper bounds -> candidates), and the candidates'
 * logits are recomputed with the canonical fp32 chains and mixed with dae_mix_scores' operations before they are ranked.
 * No [B, V] matrix and no transposed term.  Called on the TITLE scorer's context; `dae` is the DAE's.  Both must hold
 * their weights prepacked with DAE_DTYPE_BF16_EXACT over the same columns [0, V), and be bound to the same stream.
 * SHAPES: dae_mix_exact_shape_ok(hidden, ld_feat) -- DAE hidden 128 .. 512 and title rows (Output_W^T, the feature row
 * length) 64 .. 512, both in steps of 64.  Hidden 256 and rows of 448, the shipped shape, keep a kernel unrolled
 * for them; the other shapes share one kernel that takes the two step counts at run time (row groups of 96 playlists while
 * both scorers' rows fit the CU's LDS, of 64 beyond hidden + row length 832).  Any other shape: DAE_ERR_ARG -- rank it
 * with DAE_DTYPE_F32, which returns the same lists.  feat [B][ld_feat]: title features (dae_title_features; any finite
 * values -- the bound scales with the row's largest |feature|), h [B][ld_h]: the DAE's fp32 hidden rows (dae_encode),
 * w_title / w_playlist [B] in [0, 1] (DAEs.py:159-162).  Rows that violate a precondition return no recommendations
 * (idx -1).  The bound guard of the plain exact mode covers both GEMMs: dae_exact_guard_read / _words on the title
 * context; a row with more than 8192 columns left to recompute also counts there (column -3).  guard_out (nullable, DEVICE int32[2]):
 * receives the guard words {violations so far, a violating column} in stream order, for a fetch alongside the lists --
 * a count that grew since the previous launch's means THIS launch is not to be trusted (re-score it with
 * DAE_DTYPE_F32).  out_score holds y.  B <= 4096. */
/* One titled launch of the drivers' loop under DAE_DTYPE_BF16_EXACT in ONE call (main_challenge.py:72-93 with DAE_title:
 * `reader.next_batch()` -> `sess.run(model.y_pred)` -> `cand_generate`): the feed as the reader emits it (COO positions /
 * values ON THE DEVICE, as for dae_coo_to_csr), the titles [n_rows][L] int32 and titles_use [n_rows] on the device ->
 * dae_title_features, dae_coo_to_csr, dae_encode, dae_seeds_from_csr (seeds = the playlist's own tracks), dae_mix_weights,
 * dae_mix_topk_exact, with the intermediates in the title context's scratch.  Same results as the calls made one by one
 * (`DAE_title.recommend_iter` made them from Python: eight library calls and a dozen allocations, ~0.2 ms of a 0.6 ms
 * launch).  filter_sizes: HOST array.  csr_status: device int32, as dae_coo_to_csr's. */
/* dae_title_score: the same launch for any dtype -- DAE_DTYPE_BF16_EXACT as above; DAE_DTYPE_F32 / DAE_DTYPE_BF16 through the
 * fused mix (dae_decode_mix_term on the DAE's context, dae_set_score_mix + dae_decode_topk on the title context; both hold
 * their weights prepacked with that dtype), guard_out zeroed.  dae_title_score_exact = dae_title_score(DAE_DTYPE_BF16_EXACT).
 * k: 1 <= k <= 1024 for every dtype (as dae_mix_topk_exact), refused before any launch otherwise. */
int dae_title_score(dae_ctx* title_ctx, dae_ctx* dae, int dtype, const int64_t* positions, const float* values, int values_broadcast,
                    int64_t nnz, int n_rows, int V, const float* W_enc, const float* b_enc, int H,
                    const int32_t* titles, int L, const float* emb, int n_char, int E, const float* conv_w,
                    const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, int ld_feat,
                    const float* titles_use, int n_tracks, int k, float* out_score, int32_t* out_idx,
                    int32_t* guard_out, int32_t* csr_status);
int dae_title_score_exact(dae_ctx* title_ctx, dae_ctx* dae, const int64_t* positions, const float* values, int values_broadcast,
                          int64_t nnz, int n_rows, int V, const float* W_enc, const float* b_enc, int H,
                          const int32_t* titles, int L, const float* emb, int n_char, int E, const float* conv_w,
                          const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F, int ld_feat,
                          const float* titles_use, int n_tracks, int k, float* out_score, int32_t* out_idx,
                          int32_t* guard_out, int32_t* csr_status);
int dae_mix_topk_exact(dae_ctx* title_ctx, dae_ctx* dae, const float* feat, int64_t ld_feat, const float* h, int64_t ld_h,
                       int B, const float* w_title, const float* w_playlist, int n_tracks, const int32_t* seed_row_ptr,
                       const int32_t* seed_col, int k, float* out_score, int32_t* out_idx, int32_t* guard_out);
/* 1 when dae_mix_topk_exact (and dae_title_score under DAE_DTYPE_BF16_EXACT) takes a DAE of this hidden size with title
 * feature rows of this length, 0 otherwise.  Needs no context and no device. */
int dae_mix_exact_shape_ok(int hidden, int ld_feat);

/* Training of the title variables (main_train.py:214-221 feeds the playlist as x AND y, titles_use = 1; the DAE
 * arrays are constants, DAEs.py:165-171).  The caller runs the forward pieces -- dae_encode (dropout on) +
 * dae_decode_dense for the DAE scores, dae_title_features(argmax, feat_raw) + dae_decode_dense(apply_sigmoid = 0)
 * for the title logits, dae_row_sums for x_count -- and then:
 *
 * dae_row_sums: out[r] = reduce_sum of DAEs.py:41, the row sums of the dropped-out input with dae_encode's draws.
 *
 * dae_title_loss_backward: cost = mean_rows(weighted BCE of the MIXED score) (DAEs.py:193-195) and the gradients
 *   of the output layer: gOutput_WT [V, ld] (the transposed layout the library keeps Output_W in), gOutput_b [V],
 *   and dfeat [B, ld] = d cost / d features (after dropout).  ld % 32 == 0, B <= 256.
 *
 * dae_title_conv_backward: dfeat back through dropout, max over time, ReLU, the convolutions and the embedding:
 *   g_emb [n_char, E], g_conv_w / g_conv_b in the layout of dae_title_features (overwritten).
 * Then dae_adam_step on each variable. */
int dae_row_sums(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, int B,
                 float input_keep_prob, uint32_t seed, float* out);
/* The mixing weights of DAE_title (DAEs.py:159-162) in one launch: x_count = (the row sum of dae_row_sums) * input_keep_prob,
 * deno = titles_use + x_count + 1e-10, w_title = titles_use / deno, w_playlist = x_count / deno -- fp32 operations in the
 * reference's order.  titles_use, w_title, w_playlist: device arrays [B]. */
int dae_mix_weights(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, int B, float input_keep_prob,
                    uint32_t seed, const float* titles_use, float* w_title, float* w_playlist);
int dae_title_loss_backward(dae_ctx* ctx, const float* title_logits, int64_t ld_z, const float* dae_score, int64_t ld_d,
                            const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                            const float* w_title, const float* w_playlist, int B, int V, int n_batch,
                            const float* feat, int ld, const float* Output_WT, float* gOutput_WT, float* gOutput_b,
                            float* dfeat, float* cost_out);
/* dae_title_loss_backward restricted to the vocabulary columns [col_lo, col_hi) -- one rank's part of a vocabulary-sharded
 * title step.  title_logits / dae_score are [B, col_hi - col_lo]: column j is global column col_lo + j.  The y CSR is the
 * WHOLE batch's, with global column ids, ASCENDING AND UNIQUE within a row (what dae_coo_to_csr and dae_train_batch write):
 * the kernel binary-searches a row for its window; targets outside the window are ignored.  Output_WT_rows / gOutput_WT_rows
 * [col_hi - col_lo, ld] and gOutput_b_rows [col_hi - col_lo] are the rows col_lo .. col_hi of the full arrays.  dfeat_partial
 * [B, ld] and cost_partial are this window's ADDENDS of dfeat and of the cost (1 / n_batch applied, as in the dense call):
 * summed over a partition of the columns they give the dense call's values up to the order of the sum.  No [B, V] target
 * matrix is built.  On the same window the outputs equal, bit for bit, those of dae_title_loss_backward called with
 * V = col_hi - col_lo on the sliced inputs.
 * DAE_ERR_ARG before any launch: col_lo < 0, col_hi <= col_lo, B < 1, B > 256, ld % 32 != 0. */
int dae_title_loss_backward_cols(dae_ctx* ctx, const float* title_logits, int64_t ld_z, const float* dae_score, int64_t ld_d,
                                 const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                                 const float* w_title, const float* w_playlist, int B, int col_lo, int col_hi, int n_batch,
                                 const float* feat, int ld, const float* Output_WT_rows, float* gOutput_WT_rows,
                                 float* gOutput_b_rows, float* dfeat_partial, float* cost_partial);
int dae_title_conv_backward(dae_ctx* ctx, const int32_t* titles, int B, int L, const float* emb, int n_char, int E,
                            const float* conv_w, const int32_t* filter_sizes, int n_sizes, int F,
                            const int32_t* argmax, const float* feat_raw, const float* dfeat, int64_t ld,
                            float keep_prob, uint32_t seed, float* g_emb, float* g_conv_w, float* g_conv_b);

/* TF1 AdamOptimizer update (DAEs.py:102): lr_t = lr*sqrt(1-b2^t)/(1-b1^t);
 * m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g*g; p -= lr_t*m/(sqrt(v)+eps).  Dense over n elements.
 * t = 1-based step count. */
int dae_adam_step(dae_ctx* ctx, float* param, float* m, float* v, const float* grad,
                  int64_t n, float lr, float beta1, float beta2, float eps, int t);

/* The same dense Adam on a [n_rows, row_len] tensor whose gradient is ROW-SPARSE (the untied encoder: DAEs.py:66's
 * sparse_tensor_dense_matmul has a non-zero gradient only on the rows the batch's input names), without the seven
 * HBM passes over the rows that have none.  A row without gradient evolves by a recurrence nobody else reads, so its
 * (param, m, v) may stay at the step they were last current for and be brought up to date later by running the SAME
 * per-element update with g = 0 once per missed step, with the alpha of that step: the result is bit-identical to
 * calling dae_adam_step every step (tests/test_gpu_train.py).  Replaces nothing in the reference (TF1 applies the
 * dense update); it is how this build avoids 1.2 GB of traffic per step.
 *
 *   state   int32 [2 * n_rows], zero-initialised by the caller: the step each row is current for, and a claim mark
 *   lr_tab  float [tab_cap]: alpha of every step so far, written by dae_adam_rows_apply (entry t); t < tab_cap
 *   rows    int32 device list of the rows the coming / finished step touches (duplicates allowed, e.g. the column
 *           array of the input CSR); its length is read on the DEVICE from *n_listed_dev (e.g. &row_ptr[B]) when
 *           that pointer is not NULL, and is at most n_listed_max (which sizes the launch)
 *
 * Per step t = 1, 2, ...:
 *   dae_adam_rows_begin(rows of step t)   listed rows become current for step t - 1 -- BEFORE anything reads them
 *   ... forward / backward: the gradient rows land in the dense buffer `grad` (all other rows are zero) ...
 *   dae_adam_rows_apply(same rows)        listed rows take the update of step t; their gradient rows are zeroed
 *                                         again, so `grad` stays all-zero between steps (dae_set_enc_grad_prezeroed
 *                                         tells dae_train_forward_backward not to clear it)
 * and before anyone reads the WHOLE tensor (evaluation, saving, exchanging shards):
 *   dae_adam_rows_flush(t)                every row becomes current for step t */
int dae_adam_rows_begin(dae_ctx* ctx, float* param, float* m, float* v, int32_t* state, float* lr_tab, int tab_cap,
                        int n_rows, int row_len, const int32_t* rows, const int32_t* n_listed_dev, int n_listed_max,
                        float beta1, float beta2, float eps, int t);
int dae_adam_rows_apply(dae_ctx* ctx, float* param, float* m, float* v, float* grad, int32_t* state, float* lr_tab,
                        int tab_cap, int n_rows, int row_len, const int32_t* rows, const int32_t* n_listed_dev,
                        int n_listed_max, float lr, float beta1, float beta2, float eps, int t);
int dae_adam_rows_flush(dae_ctx* ctx, float* param, float* m, float* v, int32_t* state, const float* lr_tab,
                        int tab_cap, int n_rows, int row_len, float beta1, float beta2, float eps, int t);

/* Arms the NEXT dae_train_forward_backward of this context (untied model, reg_lambda = 0, H % 128 == 0) to apply the
 * dense Adam update of W_dec INSIDE the decoder-gradient kernel: each gradient tile is consumed in registers, W_dec
 * (which the call then writes through its const pointer), m and v are updated in place and gW_dec is not written
 * (it may be NULL).  The per-element operations are dae_adam_step's, so the parameters are bit-identical to writing
 * the gradient and calling dae_adam_step(W_dec, m, v, gW_dec, V*H, lr, ..., t); what disappears is one pass over the
 * gradient in each direction (1.2 GB -> 1.0 GB for Adam + the gradient at V = 170 000, H = 256).  m = NULL disarms.
 * A batch above 256 rows applies the update in its LAST panel: the earlier panels leave their sum in a [V, H] scratch of the
 * context, and the last one adds its tile to it in the order the unarmed step adds -- the bits stay those of "write gW_dec,
 * then dae_adam_step" at every B. */
int dae_arm_decoder_adam(dae_ctx* ctx, float* m, float* v, float lr, float beta1, float beta2, float eps, int t);

/* on != 0: the untied gW_enc buffer handed to dae_train_forward_backward is all-zero on entry (kept so by
 * dae_adam_rows_apply), so the step does not clear its 4*V*H bytes.  Sticky. */
int dae_set_enc_grad_prezeroed(dae_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif /* DAE_HIP_H */
