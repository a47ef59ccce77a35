// dae_internal.h -- shared between the translation units of libdae_hip.so (gfx950 only).
// Context object, error plumbing, canonical scalar device functions, kernel launcher prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/dae_hip.h"
#include "score_plan.h"            // dae_rowgeom, the host planners, DAE_KG / DAE_MAX_K / DAE_NUM_CU / DAE_NUM_XCD
#include "mix_plan.h"              // dae_mix_plan: the same for the exact title mix
#include "tau_search.h"            // DAE_KEY_NEG_INF, the threshold search (host and device)
#include "empty_proof.h"           // the envelope of a filter list and the proof that its live list is empty (host and device)

// ---------------------------------------------------------------------------------------------
// geometry constants of the decode path (see DESIGN.md "HBM layout")
// ---------------------------------------------------------------------------------------------
constexpr int DAE_TITLE_MAX_SIZES = 8;   // filter sizes a title scorer may have (title.hip's kernels, the table, dae_pipeline_create_titled)
constexpr int DAE_VT = 32;        // vocabulary columns per wave tile (MFMA M = 32)
constexpr int DAE_HPAD = 32;      // hidden size is zero-padded to a multiple of this
constexpr int DAE_REFINED_CAP = 4096;   // survivors per row the exact mode's compact lists hold (more: refined in place)
constexpr size_t DAE_GUARD_BYTES = 2 * sizeof(int);   // a context's guard words {violations, a violating column}

struct dae_buf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct dae_packed {            // one prepacked decoder image
    bool valid = false;
    bool borrowed = false;      // W / bias / bias16* / eps / W32 / tile_ub belong to ANOTHER context (dae_share_decoder): never freed here
    int V = 0, H = 0, Hp = 0;   // Hp = H padded to DAE_HPAD
    int col_lo = 0, col_hi = 0;
    int ntiles = 0;            // ceil((col_hi-col_lo)/32)
    dae_buf W;                 // fp32: [ntiles][Hp/8][64 lanes][4]   bf16: [ntiles][Hp/16][64 lanes] uint4 (prepack.hip)
    dae_buf bias;              // [ntiles*32] fp32, zero padded
    // fp32 image only (prepack.hip prepack_tile_kernel): per tile t two floats {A_t, M_t} with z32(r, c) <= A_t + d M_t for every
    // column c of the tile and every hidden row r whose entries lie within d of 0.5 -- what the filter launch of hidden 256
    // skips dead tiles by (score.hip topk_phase_b)
    // Layout: [ntiles][2] fp32 {A_t, M_t} (the two floats per tile the skip needs), then -- MORE than the per-tile pair -- the
    // columns' own {a_c, m_c}, [ntiles * 32][2]: the tile that holds a call's last ranked column is bounded over its ranked
    // columns alone (its other columns are the first artists, whose biases are the image's largest).  ub_valid: the bounds
    // belong to the current image (the training step's re-tiling leaves them out: such an image skips nothing).
    // Behind the columns' pairs their LOWER bounds, [ntiles * 32] fp32 lo_c with z32(r, c) >= lo_c - d m_c (-inf: no such column)
    // -- what the threshold sample's bound table is built from (prepack.hip sample_bound_kernel)
    dae_buf tile_ub; bool ub_valid = false;
    dae_buf bias16;            // bf16 image: [ntiles][64] uint4 bias fragments (prepack.hip)
    // tiles ordered by the largest bias among their rankable columns, descending (the threshold
    // sample of the fused path takes the head of this list); rebuilt when the image or the number
    // of rankable columns changes
    dae_buf order;             // [ceil(order_nrank / 32)] int32: the tiles with a rankable column only
    dae_buf ident;             // [ntiles] int32: 0, 1, 2, ... (the tile list of "all tiles")
    int order_nrank = -1;      // rankable columns the order was built for (-1: none)
    int order_nsamp = -1;
    long long order_gen = 0;   // process-wide stamp of the last rebuild of `order` (what a context's band list was cut from)
    // DAE_DTYPE_BF16_EXACT (bf16 image only; prepack.hip exact_bounds_kernel): per column c a rigorous bound
    // eps_c >= |z32(r, c) - z16(r, c)| for every hidden row with entries in [0, 1], the bias fragments of
    // b - eps (phase A: lower bounds of the fp32 logits) and b + eps (filter: upper bounds), and a row-major fp32
    // copy of the image's decoder rows for the exact re-scoring of the survivors (topk.hip ExactSrc)
    bool exact = false;
    dae_buf eps;               // [ntiles*32] fp32, zero padded; then one more float: the maximum (eps_max)
    dae_buf bias16_lo, bias16_hi;   // [ntiles][64] uint4, as bias16
    dae_buf W32;               // [col_hi - col_lo][H] fp32 row-major
    // the same image as the TITLE side of the exact title mix (mix_common.h): hidden rows with entries in [-F_r, F_r],
    // |z32 - z16| <= F_r alpha_c + beta_c; the bias fragments carry b -+ beta in k-slots 0..2 and -+alpha (bf16) in slot 3
    dae_buf mix_alpha, mix_beta;    // [ntiles*32] fp32 (alpha: the bf16 value the fragments hold)
    dae_buf mix16_lo, mix16_hi;     // [ntiles][64] uint4
    // the dae_catalogue the image was gathered from (catalogue.hip dae_prepack_decoder_catalogue; its columns are then the
    // catalogue's LOCAL ones), 0 = an image of the vocabulary's own columns.  Every prepack launcher resets it; it travels with
    // dae_share_decoder
    uint64_t cat_id = 0;
};

// the buffers of an image that dae_share_decoder lends to another context (`order` / `ident` stay each context's own)
template <class F>
inline void dae_packed_shared_bufs(dae_packed& pk, F&& f)
{
    for (dae_buf* b : {&pk.W, &pk.bias, &pk.tile_ub, &pk.bias16, &pk.bias16_lo, &pk.bias16_hi, &pk.eps, &pk.W32, &pk.mix_alpha,
                       &pk.mix_beta, &pk.mix16_lo, &pk.mix16_hi})
        f(*b);
}

struct dae_topk_state {     // what the second half of a fused scoring call needs from the first (score.hip topk_phase_a / _b)
    bool valid = false;
    const dae_packed* pk = nullptr;
    dae_rowgeom g{};
    int B = 0, k = 0;
    dae_score_plan plan{};  // score_plan.h
    const int* order = nullptr;
    int* sample_cnt = nullptr;
    const float* pend_h32 = nullptr;   // dae_score_topk_begin / _finish: the fp32 hidden rows of the pending call
    bool live_built = false;           // the threshold launch built the live lists in ctx->live (dae_score_plan::live_in_tau)
};

struct dae_ctx {
    int device = 0;
    // per-context (= per-device) one-time setup done so far, e.g. hipFuncSetAttribute of a kernel: a process-wide
    // `static bool` would skip it for the second device of a multi-device process
    std::unordered_set<const void*> first_use_done;
    hipStream_t stream = nullptr;
    std::string err;
    size_t scratch_total = 0;

    dae_packed pk_f32, pk_bf16;

    // scratch (grown lazily, never shrunk)
    dae_buf h_packed;          // [n_rg][Hp/8][RB][64][4] fp32 (or bf16 image)
    dae_buf h_packed16;        // bf16 image of the hidden tile [n_rg][Hp/16][RB][64][8 bf16]
    dae_buf h_scratch;         // [B,H] fp32 hidden activations when the caller does not keep them
    long long h_geom_key = -1; // (B, H, R_TILE) whose pad region of h_packed is known to be zero
    void* h_geom_ptr = nullptr;
    long long h16_geom_key = -1;   // the same for the bf16 image h_packed16 when the encode writes it directly
    void* h16_geom_ptr = nullptr;
    dae_buf sample;            // phase-A dense logits [Bpad][n_sample_cols]
    dae_buf gmax;              // phase-A group maxima [Bpad][4 * n_sample_tiles]
    dae_buf tau;               // [Bpad] fp32
    dae_buf sample_top;        // [Bpad][k] (logit, idx) pairs
    dae_buf cand;              // [nb_rg][Bpad][cap] pairs
    dae_buf cand_cnt;          // [nb_rg][Bpad] int
    dae_buf train_a, train_b, train_c, train_d;
    float* arm_m = nullptr; float* arm_v = nullptr; float arm_alpha = 0.f, arm_b1 = 0.f, arm_b2 = 0.f, arm_eps = 0.f;  // dae_arm_decoder_adam
    const float* mixT = nullptr; int64_t mix_ld = 0; const float* mix_w = nullptr; int mix_ncols = 0;   // dae_set_score_mix (caller-owned)
    hipEvent_t gate_wait = nullptr, gate_record = nullptr;   // dae_set_decode_gate (caller-owned events)
    int enc_grad_prezeroed = 0;        // untied gW_enc is all-zero on entry (dae_adam_rows_apply re-zeroes what it reads)
    int adam_t = 0; float adam_b1 = 0.f, adam_b2 = 0.f, adam_b1p = 1.f, adam_b2p = 1.f;   // running beta powers of dae_adam_alpha
    int train_dtype = DAE_DTYPE_F32;   // arithmetic of the training forward GEMM (dae_set_train_dtype)
    dae_buf csr_tmp;           // COO -> CSR scratch (csr.hip)
    dae_buf feed_tmp;          // dae_train_batch: the rows' kept counts and kept ids (train_feed.hip)
    dae_topk_state tk;
    int overlap_hint = 0;      // dae_set_overlap_hint: other batches are in flight on other streams -> kernel shapes that share CUs
    dae_buf row_bad;           // DAE_DTYPE_BF16_EXACT via dae_decode_topk: [Bpad] int32, 1 = the caller's hidden row leaves [0, 1]
    dae_buf refined;           // DAE_DTYPE_BF16_EXACT: [Bpad][DAE_REFINED_CAP] (fp32 logit, column) pairs + [Bpad] counts (refine.hip)
    dae_buf refstat; int refstat_rows = 0;   // DAE_DTYPE_BF16_EXACT: [rows][2] {candidates, recomputed} of the last refine launch
    dae_buf guard;             // DAE_DTYPE_BF16_EXACT: {violations of the bound seen by the refine launches, a violating column}
    float exact_margin = 1.0f; // dae_set_exact_margin: factor on every eps_c at the next exact prepack
    int margin_lo = 0, margin_hi = 0; float margin_scale = 1.0f;   // dae_set_exact_margin_range: columns [lo, hi) take this factor instead
    // the audit of dropped columns (audit.hip): every audit_every-th exact scoring launch checks audit_tiles random tiles
    int audit_every = 64, audit_tiles = 16;
    uint64_t audit_seq = 0, audits_run = 0;
    dae_buf title_y1;          // dae_title_rank (fp32 / bf16): the DAE term of the track columns, transposed
    dae_buf audit_stat;        // {elements checked, violations} | the sampled tile ids (allocated once)
    dae_buf audit;             // upper bounds of the sampled tiles [Bpad][tiles * 32]
    dae_buf mix_fhat;          // dae_mix_topk_exact: [Bpad] bf16 bits of the rows' feature bounds
    dae_buf title_scratch;     // dae_title_score_exact: CSR, seed lists, hidden rows, features, mixing weights of the launch
    // dae_title_prepack_features (title.hip): the convolutions of a FROZEN title scorer as a table over (filter size, offset,
    // character) -- which variables it was built from
    dae_buf title_tab; const float* ttab_emb = nullptr; const float* ttab_w = nullptr; int ttab_nchar = 0, ttab_E = 0, ttab_F = 0,
        ttab_nsizes = 0; int ttab_fs[DAE_TITLE_MAX_SIZES] = {0};
    // the bias-ordered tile list with its sample RE-DEALT for a launch geometry (dae_launch_tile_band): which order it was cut from
    dae_buf tile_band; long long band_gen = -1; int band_nsamp = 0, band_nbrg = 0, band_waves = 0;
    // the fp32 hidden-256 filter launch walks, per row group, only the tiles whose logit bound reaches the group's threshold
    // (built by the threshold launch itself -- tau_select.hip tau_select_kernel -- or, on foreign thresholds, by prepack.hip
    // live_tiles_kernel): [n_rg] counts (16 ints reserved at least) | [n_rg][n_filter] tile ids, in tsB's order
    int filter_skip = 1;       // dae_set_filter_skip
    dae_buf live; int live_n_rg = 0;       // live_n_rg: row groups of the last launch that built the lists (0: none yet)
    // the threshold launch's own words for that: 64 arrival counters (one per row group; zeroed when the buffer is (re)allocated,
    // left at zero by every launch) | [Bpad] doubles, the rows' max |h - 0.5|.  Nothing else re-zeroes the counters: a threshold
    // launch that never completes (a device fault) leaves them standing for the life of the context, like the rest of its state
    dae_buf live_sync; void* live_sync_zeroed = nullptr; size_t live_sync_zeroed_bytes = 0;   // (which allocation was zeroed)
    dae_buf cand_list;         // dae_rank_candidates: [B][row_cap] (key, column) pairs | [B] counts (candidates.hip)
    dae_buf mix_loss;          // the mixed loss without a step, on the title context: the DAE's term of one panel, transposed | partial table | row losses (mix_loss_plan.h)
    dae_buf loss_rows;         // the loss without a step: hidden rows [B][H] | partial table [grid][R_TILE] | row losses [B] | l2 partials (loss_rows.hip)
    dae_buf rank_of;           // dae_decode_rank_of: [n_ans] thresholds (u64) | logits | places | buckets, then [n_rg] longest rows (rank_of.hip)
    dae_buf cat_seeds;         // the catalogue calls: a slab's seed lists in the catalogue's columns, [4097] row pointers | [4096] counts | the columns (catalogue.hip)
    dae_buf skip_stat;         // 4 x uint64 {launches, planned tiles x row groups, live tiles} since the last dae_filter_skip_read |
                               // {row groups whose live list the threshold launch proved empty} since the last dae_live_proof_read
    // the threshold sample in half row groups skips the tiles a bound puts below tau (decode_generic.hip decode_f32_kernel's HALF):
    // row_d = [Bpad][4] floats, the rows' max |h - 0.5| by quarters, written by whoever wrote the packed fp32 hidden image
    // (the encode kernels, pack_h_d_kernel); row_d_fresh: ... for the image as it stands (set by that launch, taken by the next
    // threshold sample: an image with no published d skips nothing)
    dae_buf row_d; bool row_d_fresh = false;
    // the sample's bound table (prepack.hip sample_bound_kernel): 4 floats {mu_max, -, -, -} | [n_samp] {A_t, M_t} | [n_beta] beta
    // sorted descending | [DAE_PROOF_ENV] the envelope of the filter list (filter_envelope_kernel; empty_proof.h); built for one
    // tile order, sample geometry, filter list length and ranked-column count, like tile_band
    dae_buf samp_tab; long long tab_gen = -1; int tab_nsamp = 0, tab_nbrg = 0, tab_waves = 0, tab_nfilter = -1, tab_nrank = -1;
    dae_buf sskip_stat;        // DAE_SSKIP_SLOTS x uint64, one per workgroup of the sample launch: wave-tiles it decoded since the last dae_sample_skip_read
                               // | DAE_SSKIP_SLOTS x uint32: the decoded-tile table of the last sample launch that skipped (dae_sample_skip::tab)
                               // | DAE_SSKIP_PAIRS x float2: {dq, tau_safe} of its half groups (dae_sample_skip::pair)
    unsigned long long sskip_launches = 0, sskip_planned = 0;   // ... and the launches / planned wave-tiles (known on the host)

    // profiling of the dominant kernel
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;   // pairs (start, stop)
    size_t prof_used = 0;
    bool prof_armed = false;           // the next decode launch takes prof_ev[prof_used], [prof_used+1]
    std::string prof_kernel;           // symbol of the kernel the last armed pair bracketed (dae_profile_kernel)
};

extern thread_local std::string g_dae_create_err;

int dae_fail(dae_ctx* ctx, int code, const char* fmt, ...);
int dae_reserve(dae_ctx* ctx, dae_buf& b, size_t bytes);
int dae_ensure_guard(dae_ctx* ctx);       // ctx->guard: allocated and zeroed once (api.hip)

// What the context remembers about its packed fp32 hidden image (h_packed): for which (rows, row width, row-group height) and
// which allocation the pad rows / pad k are known to be zero (h_geom_key / h_geom_ptr: score.hip hidden_pads_zeroed), whether
// row_d belongs to it, and whether a pending dae_score_topk_begin still owns it.
inline long long dae_hidden_geom_key(int B, int H, int R_TILE)
{
    return ((long long)B << 32) | ((long long)H << 12) | (long long)R_TILE;
}
// A call outside the ranking path has just rewritten the WHOLE image, pads included, with dae_launch_pack_h (no row_d output)
// for B rows of width H in groups of R_TILE (loss_rows.hip, mix_loss.hip): the pads are zero for that geometry, row_d is not
// this image's, and a pending dae_score_topk_begin's hidden image is gone.
inline void dae_note_hidden_repacked(dae_ctx* ctx, int B, int H, int R_TILE)
{
    ctx->row_d_fresh = false;
    ctx->h_geom_key = dae_hidden_geom_key(B, H, R_TILE);
    ctx->h_geom_ptr = ctx->h_packed.p;
    ctx->tk.valid = false;
}

#define DAE_HIP_CHECK(ctx, expr)                                                              \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return dae_fail((ctx), DAE_ERR_HIP, "%s failed: %s (%s:%d)", #expr,               \
                            hipGetErrorString(_e), __FILE__, __LINE__);                       \
    } while (0)

#define DAE_CHECK_LAUNCH(ctx, name)                                                           \
    do {                                                                                      \
        hipError_t _e = hipGetLastError();                                                    \
        if (_e != hipSuccess)                                                                 \
            return dae_fail((ctx), DAE_ERR_HIP, "launch of %s failed: %s", name,              \
                            hipGetErrorString(_e));                                           \
    } while (0)

static inline int dae_round_up(int x, int m) { return (x + m - 1) / m * m; }
inline bool dae_known_dtype(int dtype) { return dtype == DAE_DTYPE_F32 || dtype == DAE_DTYPE_BF16 || dtype == DAE_DTYPE_BF16_EXACT; }

inline bool dae_first_use(dae_ctx* ctx, const void* key) { return ctx->first_use_done.insert(key).second; }
// before the first launch of `kernel` on this context: raise its dynamic-LDS limit (the kernel is its own first-use key)
template <class K>
inline hipError_t dae_lds_limit_once(dae_ctx* ctx, K* kernel, size_t bytes)
{
    const void* f = reinterpret_cast<const void*>(kernel);
    return dae_first_use(ctx, f) ? hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipSuccess;
}
// a launch that can be the profiled one: when a pair of profile events is armed (dae_profile_*: api.hip, score.hip) it takes the pair --
// e0 / e1 are left alone otherwise -- and notes the kernel's name
inline void dae_take_profile_events(dae_ctx* ctx, const char* kernel, hipEvent_t& e0, hipEvent_t& e1)
{
    if (!ctx->prof_armed) return;
    e0 = ctx->prof_ev[ctx->prof_used]; e1 = ctx->prof_ev[ctx->prof_used + 1];
    ctx->prof_armed = false;
    ctx->prof_used += 2;
    ctx->prof_kernel = kernel;
}

// The library reads no environment variable: an A/B of two kernel variants is two source trees, each built with build()
// (DESIGN.md section 8).

// ---------------------------------------------------------------------------------------------
// canonical scalar device functions -- the SPECIFICATION is DESIGN.md "canonical order"; the
// oracle (oracle/dae_oracle.c) restates the same arithmetic independently.  Built with
// -ffp-contract=off: every fused multiply-add below is explicit.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dae_sigmoidf(float x)
{
    float t = -x;
    t = fminf(fmaxf(t, -87.0f), 87.0f);
    float n = rintf(t * 1.44269504088896341f);
    float r = fmaf(n, -0.693145751953125f, t);
    r = fmaf(n, -1.42860682030941723e-6f, r);
    float p = 1.0f / 5040.0f;
    p = fmaf(p, r, 1.0f / 720.0f);
    p = fmaf(p, r, 1.0f / 120.0f);
    p = fmaf(p, r, 1.0f / 24.0f);
    p = fmaf(p, r, 1.0f / 6.0f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    float s = __uint_as_float((uint32_t)((int)n + 127) << 23);
    float e = p * s;
    return 1.0f / (1.0f + e);
}

// fp32 -> bf16, round to nearest even (oracle: bf16_round)
__device__ __forceinline__ unsigned dae_bf16_rne(float f)
{
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return u >> 16;
}

__device__ __forceinline__ uint32_t dae_mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352dU;
    x ^= x >> 15; x *= 0x846ca68bU;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float dae_uniform(uint32_t seed, uint32_t stream, uint32_t row,
                                             uint32_t col)
{
    uint32_t x = dae_mix32(seed + 0x9E3779B9U * (stream + 1U));
    x = dae_mix32(x ^ row);
    x = dae_mix32(x ^ col);
    return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// order-preserving fp32 -> u32 (bigger key = bigger float, -0 == +0)
__device__ __forceinline__ uint32_t dae_okey(float f)
{
    uint32_t u = __float_as_uint(f);
    if ((u << 1) == 0) u = 0;
    return (u & 0x80000000U) ? ~u : (u | 0x80000000U);
}
__device__ __forceinline__ float dae_okey_inv(uint32_t k)
{
    uint32_t u = (k & 0x80000000U) ? (k & 0x7FFFFFFFU) : ~k;
    return __uint_as_float(u);
}
// (DAE_KEY_NEG_INF = dae_okey(-inf), the "absent" marker: tau_search.h)

// inclusive scan over the 64 lanes of a wave (every lane active)
__device__ __forceinline__ unsigned dae_wave_scan_incl(unsigned v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}
__device__ __forceinline__ int dae_wave_scan_incl(int v, int lane) { return (int)dae_wave_scan_incl((unsigned)v, lane); }

// ---------------------------------------------------------------------------------------------
// launchers (each defined next to its kernels)
// ---------------------------------------------------------------------------------------------
// encode.hip
int dae_launch_encode(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val,
                      const float* W_enc, const float* b_enc, int V, int H, int B,
                      float ikp, float kp, uint32_t seed, float* h_out,
                      float* h_packed, int G, int RB, float* sg_out = nullptr,
                      float* xhat_out = nullptr, unsigned short* h_packed16 = nullptr, int NS = 0, float* d_out = nullptr);

// prepack.hip
// bounds: also the per-tile logit bounds (dae_packed::tile_ub) -- the scoring images; the training step's re-tiling passes false
int dae_launch_prepack_f32(dae_ctx* ctx, const float* W, const float* b, int V, int H,
                           int col_lo, int col_hi, bool bounds = true);
int dae_launch_prepack_bf16(dae_ctx* ctx, const float* W, const float* b, int V, int H,
                            int col_lo, int col_hi, int exact = 0);
// d_out (nullable): [g.Bpad][4], the rows' max |h - 0.5| by quarters of the hidden units (dae_ctx::row_d)
int dae_launch_pack_h(dae_ctx* ctx, const float* h, int B, int H, const dae_rowgeom& g, float* d_out = nullptr);
// row_bad (nullable): [g.Bpad] int32, 1 where a row of h has an entry outside [0, 1] (the exact mode's precondition)
int dae_launch_pack_h_bf16(dae_ctx* ctx, const float* h, int B, int H, const dae_rowgeom& g, int* row_bad = nullptr);
int dae_launch_tile_iota(dae_ctx* ctx, int* dst, int ntiles);      // dst[i] = i
// (re)build pk.order for `nrank` rankable columns; the first n_samp entries are the threshold sample
int dae_launch_tile_order(dae_ctx* ctx, dae_packed& pk, int nrank, int n_samp, int S);
bool dae_tile_order_sorted(int n_rank_tiles);    // the bias sort (true) or the strided list, by the number of ranked tiles
// band[0 .. n_samp): the sample of `order` dealt to the phase-A launch's slots so that the tiles ONE workgroup decodes in a round
// (item = round * nb_rg * waves + wave * nb_rg + bir) come from `waves` different popularity bands; band[n_samp ..) = order
int dae_launch_tile_band(dae_ctx* ctx, const int* order, int ntiles, int n_samp, int nb_rg, int waves, int* band);
// the live lists of an fp32 filter launch over `list[0 .. n_items)` (128-row groups, hidden tile packed in ctx->h_packed):
// live_cnt[rg] tiles of the list, in its order, at live_list[rg * n_items ..), can hold a logit >= min over the group's rows of tau
// the bound table of a threshold sample of n_items tiles of `list`, decoded by nb_rg workgroups of `waves` waves per half row
// group (item = wave * nb_rg + workgroup): head[0] = mu_max, ub_out[i] = {A_t, M_t} of item i, beta_out[0 .. n_beta) the largest
// group lower bounds, descending
int dae_launch_sample_bounds(dae_ctx* ctx, const dae_packed& pk, const int* list, int n_items, int nb_rg, int waves, int nrank,
                             float* head, float2* ub_out, float* beta_out, int n_beta, int n_filter, float* env_out);
int dae_launch_live_tiles(dae_ctx* ctx, const dae_packed& pk, const dae_rowgeom& g, int B, const int* list, int n_items,
                          const float* tau, int nrank, int* live_cnt, int* live_list, unsigned long long* stat);

// decode_f32.hip: the launchers that choose between a hidden-256 kernel and the generic one (by the predicates of score_plan.h)
struct dae_tileset {        // which wave tiles a decode launch walks
    int n_items;            // number of tiles in the set
    int stride;             // S
    int mode;               // informational: 0 = all tiles (identity list), 3 = ordered list
    const int* list;        // tile of item i; never null
};
constexpr int DAE_SSKIP_SLOTS = 2 * DAE_NUM_CU;      // workgroups of a half-row-group sample launch: 2 n_rg nb_rg <= 2 x 256
constexpr int DAE_SSKIP_PAIRS = DAE_SSKIP_SLOTS / DAE_NUM_XCD;   // ... and its half groups: nb_rg >= DAE_NUM_XCD
// what decode_f32_kernel's HALF skips sample tiles by (ub == nullptr: the full walk) -- DESIGN.md section 2
struct dae_sample_skip {
    const float2* ub;                 // [n_items] {A_t, M_t} of the sample's items, in list order
    const float* beta; int n_beta;    // the group lower bounds, sorted descending
    const float* mu;                  // -> mu_max
    const float* row_d;               // [Bpad][4] the rows' max |h - 0.5| by quarters
    const int32_t* seed_row_ptr; int k;   // need = k + seeds of the row, as tau_select_kernel's
    unsigned long long* stat;         // [grid of the launch] += wave-tiles decoded, per workgroup (DAE_SSKIP_SLOTS words)
    unsigned* tab;                    // nullable: [2 n_rg][nb_rg] the decoded-tile table (score_plan.h dae_sample_item_slot) -- the launch
                                      // stores the decoded tiles' slots only, and dae_launch_tau_select must be given the same table
    float2* pair;                     // nullable: [2 n_rg] {dq, tau_safe} of every half group, stored by its workgroup 0 (what the threshold
                                      // launch proves an empty live list from: dae_tau_live::pair)
};
// dense epilogue: out[row*ld + item*32 + vl] (item = position of the tile in the set)
// gmax (nullable): [B][ld_gmax] maxima of every lane's two 8-column groups, 4 per (row, item) -- the threshold
// sample's input to dae_launch_tau_select
int dae_launch_decode_dense_f32(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts,
                                int apply_sigmoid, int mask_from_col, float* out, int64_t ld,
                                int fill_pad, int dtype = DAE_DTYPE_F32, float* gmax = nullptr,
                                int64_t ld_gmax = 0, int gmax_per_wave = 0, int bias_sel = 0,
                                const dae_sample_skip* skip = nullptr);      // (taken by the half-row-group sample only)
// gmax_per_wave: 0 = one maximum per (workgroup, round, position) over the workgroup's waves; 1 = every wave slot's value (small
// samples); 3 = per-WAVE groups over all of a wave's tiles, 8 wave slots per workgroup (dae_sample_wave_groups: ld_gmax = 8 nb_rg 32);
// 4 = the same with waves w and w + 4 sharing a group (ld_gmax = 4 nb_rg 32)
// filter epilogue: append (logit, global col) with logit >= tau[row] and col < n_valid_col
// live_cnt / live_list (nullable; the fp32 hidden-256 kernel only -- dae_filter_takes_live): row group rg walks the live_cnt[rg]
// tiles at live_list[rg * ts.n_items ..) instead of ts.list (dae_launch_live_tiles)
int dae_launch_decode_filter_f32(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts,
                                 const float* tau, int n_valid_col, uint2* cand, int* cand_cnt,
                                 int cap, int dtype = DAE_DTYPE_F32, int bias_sel = 0, const int* live_cnt = nullptr,
                                 const int* live_list = nullptr);
// bias_sel (bf16 image prepacked with DAE_DTYPE_BF16_EXACT): 0 = b, 1 = b - eps (lower bounds), 2 = b + eps (upper bounds)

int dae_launch_decode_scaled_T(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts, const float* row_scale,
                               float* outT, int64_t ldT, int dtype = DAE_DTYPE_F32, bool add = false);

// training forward: all tiles; the epilogue takes every element as a negative (target 0), writes dL/dz
// TRANSPOSED ([ncols, ldT]: what both backward GEMMs read) and one loss partial per workgroup
// (DAEs.py:98-100); the positives are redone afterwards by train.hip's loss_fixup_kernel.
int dae_launch_decode_loss_f32(dae_ctx* ctx, const dae_rowgeom& g, int B, float inv_n_batch,
                               float* dzT, int64_t ldT, float* loss_part, int dtype = DAE_DTYPE_F32,
                               int dz16 = 0);

// the loss without a step (loss_rows.hip): ALL tiles of the image of `dtype`, every element a negative, summed per row and
// workgroup into the partial table row_part[g.n_rg][g.nb_rg][g.R_TILE] (decode_f32_kernel's EPI_ROWLOSS); stores nothing else
int dae_launch_decode_rowloss(dae_ctx* ctx, const dae_rowgeom& g, int B, int dtype, float* row_part);
// the mixed loss without a step (mix_loss.hip): the same walk over the TITLE scorer's fp32 image, every element the negative
// term of sigmoid(z) * mix_w[row] + mixT[column * mix_ld + row] (decode_f32_kernel's EPI_MIXROWLOSS); the same partial table
int dae_launch_decode_mixrowloss(dae_ctx* ctx, const dae_rowgeom& g, int B, const float* mixT, int64_t mix_ld, const float* mix_w,
                                 float* row_part);
// loss_rows.hip loss_cost_kernel: cost = (float)(sum_r (double)row_loss[r] / n_batch + lambda * sum of the n_l2 partials)
int dae_launch_loss_cost(dae_ctx* ctx, const float* row_loss, int B, int n_batch, const double* l2_part, int n_l2, float lambda,
                         float* cost_out);

int dae_launch_decode_loss_rowmajor(dae_ctx* ctx, const dae_rowgeom& g, int B, int V, int H, const float* W,
                                    const float* bias, const float* h, float inv_n_batch, float* dzT, int64_t ldT,
                                    float* loss_part);

int dae_launch_decode_loss_dh(dae_ctx* ctx, const dae_rowgeom& g, int B, int V, int H, const float* W, const float* bias,
                              const float* h, float inv_n_batch, float* dzT, int64_t ldT, float* loss_part, float* part, int Bpad64);

// decode_generic.hip: decode_f32_kernel for (epilogue EPI_*, operand type DT_*, row-group height) -- decode_common.h
struct dae_decp;
int dae_launch_decode_generic(dae_ctx* ctx, int epi, int dt, const dae_rowgeom& g, const dae_decp& p);
int dae_launch_decode_gmax_half(dae_ctx* ctx, const dae_rowgeom& g, const dae_decp& p);

// train.hip
int dae_train_step_f32(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
        int V, int H, int B, int n_batch, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* gW_enc, float* gb_enc, float* gW_dec, float* gb_dec, float* cost_out);
int dae_train_shard_encode_f32(dae_ctx* ctx, const int32_t* x_row_ptr, const int32_t* x_col,
                               const float* x_val, const float* W_enc_loc, int col_lo, int col_hi,
                               int H, int B, float ikp, uint32_t seed, float* pre_partial);
int dae_train_shard_decode_f32(dae_ctx* ctx, const float* pre, const float* b_enc,
                               const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                               const float* W_enc_loc, const float* W_dec_loc, const float* b_dec_loc,
                               int col_lo, int col_hi, int H, int B, int n_batch, int tied,
                               float kp, uint32_t seed, float reg_lambda,
                               float* gW_out, float* gb_dec_loc, float* dh_partial, float* cost_partial);
int dae_train_shard_finish_f32(dae_ctx* ctx, const float* dh, const int32_t* x_row_ptr,
                               const int32_t* x_col, const float* x_val,
                               const float* W_enc_loc, const float* b_enc, const float* W_dec_loc,
                               const float* b_dec_loc, int col_lo, int col_hi, int H, int B, int tied,
                               float ikp, float kp, uint32_t seed, float reg_lambda,
                               float* gW_enc_loc, float* gb_enc, float* gW_dec_loc, float* gb_dec_loc);
int dae_launch_grad_h(dae_ctx* ctx, const float* dzT, int64_t ldT, const float* W, int H, int V, int B, float* dh);
// tf.nn.l2_loss partials of the listed tensors (null / empty entries left out), at most 1024 doubles per tensor, side by side
int dae_launch_l2_partials(dae_ctx* ctx, const float* const* ts, const size_t* ns, int n_t, double* l2_part, int* n_l2);

// grad_wdec.hip (K6).  dae_armed_adam: the dense TF1-Adam of the [V, H] tensor p that an armed K6 applies in its epilogue
struct dae_armed_adam { float* p; float* m; float* v; float alpha, b1, b2, eps; };
int dae_launch_k6(dae_ctx* ctx, const float* dzT, int64_t ldT, int dz16, const float* h, int H, int B, int V, float* gW,
                  float* gb, const dae_armed_adam* arm, int small_v, const float* gprev);
int dae_launch_grad_w(dae_ctx* ctx, const float* dzT, int64_t ldT, const float* h, int H, int B, int V,
                      float* gW, float* gb);

// adam.hip
int dae_launch_adam_rows(dae_ctx* ctx, int mode, float* param, float* m, float* v, float* grad, int32_t* last,
                         int32_t* mark, float* lr_tab, int n_rows, int row_len, const int32_t* rows,
                         const int32_t* n_listed_dev, int n_listed_max, float lr_t, float beta1, float beta2,
                         float eps, int step);
int dae_launch_adam(dae_ctx* ctx, float* param, float* m, float* v, const float* grad, int64_t n,
                    float lr_t, float beta1, float beta2, float eps);

// csr.hip
int dae_launch_coo_to_csr(dae_ctx* ctx, const int64_t* positions, const float* values, int values_broadcast,
                          int64_t nnz, int n_rows, int n_cols, int32_t* row_ptr, int32_t* col, float* val,
                          int32_t* status);
// a titled launch's intermediates (score.hip dae_title_prepare / dae_title_rank; device pointers, caller-owned)
struct dae_title_bufs {
    int32_t *rp, *col, *srp, *sc;     // CSR of the feed [B + 1], [nnz]; seed lists [B + 1], [nnz]
    float *val, *h, *feat, *wt, *wp;  // values [nnz]; DAE hidden rows [B][H]; title features [B][ld_feat]; mixing weights [B]
};
int dae_title_bufs_reserve(dae_ctx* tc, int64_t nnz, int B, int H, int ld_feat, dae_title_bufs& b);      // out of tc->title_scratch
int dae_title_prepare(dae_ctx* tc, dae_ctx* dc, const int64_t* positions, const float* values, int values_broadcast, int64_t nnz,
                      int B, int V, const float* W_enc, const float* b_enc, int H, const int32_t* titles, int L, const float* emb,
                      int n_char, int E, const float* conv_w, const float* conv_b, const int32_t* filter_sizes, int n_sizes, int F,
                      int ld_feat, const float* titles_use, int n_tracks, const dae_title_bufs& b, int32_t* csr_status);
int dae_title_rank(dae_ctx* tc, dae_ctx* dc, int dtype, int B, int V, int H, int ld_feat, const dae_title_bufs& b, int n_tracks, int k,
                   float* out_score, int32_t* out_idx, int32_t* guard_out);
int dae_launch_coo64_to_csr_seeds(dae_ctx* ctx, const int64_t* positions, const float* values, int values_broadcast,
                                  int64_t nnz, int n_rows, int n_cols, int32_t* row_ptr, int32_t* col, float* val,
                                  int32_t* status, int n_tracks, int32_t* seed_row_ptr, int32_t* seed_col);
int dae_launch_coo32_to_csr_seeds(dae_ctx* ctx, const int32_t* positions, const float* values, int values_broadcast,
                                  int64_t nnz, int n_rows, int n_cols, int32_t* row_ptr, int32_t* col, float* val,
                                  int32_t* status, int n_tracks, int32_t* seed_row_ptr, int32_t* seed_col);

int dae_launch_seeds_from_csr(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, int B, int n_tracks,
                              int32_t* seed_row_ptr, int32_t* seed_col);

// catalogue.hip, for the pipeline: the seed translation into caller-owned buffers (rp_out [B + 1], cnt [B], sc_out [cap]; any B,
// on the context's stream), and the ranking calls that take the translated (LOCAL) seed lists and end with the map-back
void dae_catalogue_shape(const dae_catalogue* cat, int* device, int* n, int* n_tracks);
int dae_catalogue_translate_seeds(dae_ctx* ctx, const dae_catalogue* cat, const int32_t* srp, const int32_t* sc, int B, int cap,
                                  int32_t* rp_out, int32_t* cnt, int32_t* sc_out);
int dae_score_topk_catalogue_local(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                                   const float* b_enc, int V, int H, int B, int dtype, const dae_catalogue* cat,
                                   const int32_t* local_srp, const int32_t* local_sc, int k, int out_kind, float* out_score,
                                   int32_t* out_idx);
int dae_title_rank_catalogue(dae_ctx* tc, dae_ctx* dc, int dtype, int B, int H, int ld_feat, const dae_title_bufs& b,
                             const dae_catalogue* cat, int k, float* out_score, int32_t* out_idx, int32_t* guard_out);

// title.hip
int dae_launch_title_features(dae_ctx* ctx, const int32_t* titles, int B, int L, const float* emb, int n_char,
                              int E, const float* conv_w, const float* conv_b, const int32_t* filter_sizes,
                              int n_sizes, int F, float kp, uint32_t seed, float* feat, int64_t ld,
                              int32_t* argmax, float* feat_raw);
int dae_launch_title_table(dae_ctx* ctx, const float* emb, int n_char, int E, const float* conv_w, const int32_t* filter_sizes,
                           int n_sizes, int F);
int dae_launch_row_sums(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, int B,
                        float ikp, uint32_t seed, float* out);
int dae_launch_mix_weights(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, int B, float ikp,
                           uint32_t seed, const float* use, float* w_t, float* w_p);
int dae_launch_title_loss_backward(dae_ctx* ctx, const float* zt, int64_t ld_z, const float* dae_score, int64_t ld_d,
                                   const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                                   const float* w_title, const float* w_playlist, int B, int V, int n_batch,
                                   const float* feat, int ld, const float* Output_WT, float* gOutput_WT,
                                   float* gOutput_b, float* dfeat, float* cost_out);
int dae_launch_title_loss_backward_cols(dae_ctx* ctx, const float* zt, int64_t ld_z, const float* dae_score, int64_t ld_d,
                                        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                                        const float* w_title, const float* w_playlist, int B, int col_lo, int col_hi,
                                        int n_batch, const float* feat, int ld, const float* Output_WT_rows,
                                        float* gOutput_WT_rows, float* gOutput_b_rows, float* dfeat_partial,
                                        float* cost_partial);
int dae_launch_title_conv_backward(dae_ctx* ctx, const int32_t* titles, int B, int L, const float* emb, int n_char,
                                   int E, const float* conv_w, const int32_t* filter_sizes, int n_sizes, int F,
                                   const int32_t* argmax, const float* feat_raw, const float* dfeat, int64_t ld,
                                   float kp, uint32_t seed, float* g_emb, float* g_conv_w, float* g_conv_b);
int dae_launch_mix_scores(dae_ctx* ctx, const float* title_score, int64_t ld_t, float* dae_score, int64_t ld_d,
                          const float* w_title, const float* w_playlist, int B, int ncols);

// the exact title mix (DAE_DTYPE_BF16_EXACT under the title mix): mixexact.hip is the call, mix_plan.h its geometry
// mix_prep.hip: the title image's row-scaled bounds (once per image, from prepack.hip)
int dae_launch_mix_title_bounds(dae_ctx* ctx, const float* W, const float* b, int H, int Hp, int col_lo, int col_hi,
                                int ntiles, dae_packed& pk);
struct dae_mix_call {       // the caller's arguments of dae_mix_topk_exact that its launches read
    const float* feat; int64_t ld_feat;           // title features [B][ld_feat]
    const float* h; int64_t ld_h;                 // DAE hidden rows [B][ld_h]
    int B;
    const float* w_title; const float* w_playlist;                    // [B] mixing weights
    const int32_t* seed_row_ptr; const int32_t* seed_col;
    int k; float* out_score; int32_t* out_idx;
};
// The launches of one call, in its order; each reads and writes the title context's scratch, reserved by the caller for pl.
int dae_launch_mix_prep_pack(dae_ctx* tc, const dae_mix_plan& pl, int HD, int HT, const dae_mix_call& c);             // mix_prep.hip
int dae_launch_mix_pass(dae_ctx* tc, const dae_mix_plan& pl, bool sample, const dae_packed& pd, const dae_packed& pt,    // mix_filter.hip
                        const int* order, const dae_mix_call& c);
int dae_launch_mix_refine(dae_ctx* tc, const dae_mix_plan& pl, const dae_packed& pd, const dae_packed& pt, const dae_mix_call& c);   // mix_refine.hip
int dae_launch_mix_audit(dae_ctx* tc, dae_ctx* dc, int n_valid_col, const dae_mix_call& c);                           // audit.hip
void dae_note_plan(const int32_t last[8]);      // score.hip: what dae_last_plan reports
// score.hip: what every ranking call refuses before any launch -- null outputs, an unknown dtype, k beyond the dtype's limit, half a seed CSR
int dae_check_topk_args(dae_ctx* ctx, int dtype, int k, const int32_t* seed_row_ptr, const int32_t* seed_col,
                        const void* out_score, const void* out_idx);
int dae_mix_topk_exact_impl(dae_ctx* tc, dae_ctx* dc, const float* feat, int64_t ld_feat, const float* h, int64_t ld_h, int B,
                            const float* w_title, const float* w_playlist, int n_tracks, const int32_t* seed_row_ptr,
                            const int32_t* seed_col, int k, float* out_score, int32_t* out_idx);

// topk.hip
struct dae_dense_src {      // element p of row r = logits[r*ld + p], p in [0,n)
    const float* logits; int64_t ld; int n;
    int col_base;           // global column of tile 0
    int tile_stride;        // column = col_base + (p/32)*32*tile_stride + p%32
    const int* tile_list;   // non-null: column = col_base + tile_list[p/32]*32 + p%32
};
struct dae_pair_group {     // element (seg, r, i) = base[seg*seg_stride + r*row_stride + i]
    const uint2* base; const int* cnt; int64_t seg_stride; int64_t row_stride;
    int64_t cnt_seg_stride; int nseg; int fixed_cnt;
};
struct dae_topk_args {
    int B, k, out_kind;           // out_kind: DAE_OUT_SCORE / DAE_OUT_LOGIT
    int bitmap_base, bitmap_n;    // seed bitmap covers global columns [base, base+n)
    const int32_t* seed_row_ptr; const int32_t* seed_col;
    float* out_score; int32_t* out_idx;   // [B,k]  (may be null)
    uint2* out_pairs;                     // [B,k] (logit bits, idx) (may be null)
    float* out_tau;                       // [B] k-th logit or -inf (may be null)
    int pairs_stride;             // row stride of out_pairs
    int lean, sort_cap;           // set by the launcher (topk.hip): LDS mode, sort buffer keys
    int prefer_small;             // candidate lists: the 256-thread shape (shares a CU with a bf16 filter workgroup)
    const float* row_min;         // nullable: [B] elements with logit < row_min[row] are absent (an exchanged threshold)
};
int dae_launch_topk_dense(dae_ctx* ctx, const dae_dense_src& src, const dae_topk_args& a);
// tau_select.hip
// Threshold of the fused path + the sample's survivors (tau_select_kernel):
//   tau[row] = a valid lower bound of the row's k-th largest rankable non-seed logit: the (k + n_seeds(row))-th
//   largest of gmax[row][0..n_g) (-inf = absent) to 16 key bits; -inf when the row holds fewer finite maxima;
//   out_pairs[row * pairs_stride + i], i < out_cnt[row]: the (logit, column) of every dense sample logit
//   samp[row][0..n_s) >= tau (column of element q = col_lo + samp_list[q >> 5] * 32 + (q & 31)), unordered
//   live (nullable; the workgroup-per-row kernel of an fp32 launch with a dense sample only -- dae_score_plan::live_in_tau):
//   the launch also builds the live lists of the filter launch that takes these thresholds, as dae_launch_live_tiles would
//   from them: the last workgroup of each 128-row group to finish does it, so nothing waits and no launch is added
//   samp_tab (nullable; the workgroup-per-row kernel only), nb_rg: the decoded-tile table of the half-row-group sample that wrote
//   gmax and samp (dae_sample_skip::tab, n_g == nb_rg * 32): slots the table does not mark are -inf and are never read
struct dae_tau_live {
    const float4* hp; int B, H, G;                               // the packed fp32 hidden image in 128-row groups; G = Hp / 8 = 32
    const float* tile_ub; int ntiles, nrank;                     // dae_packed::tile_ub of the image's ntiles tiles; ranked columns
    const int* list; int n_items;                                // the filter launch's tile list
    unsigned long long* d_row;                                   // [Bpad] scratch: the bits of each row's max |h - 0.5| (double)
    unsigned* arrive;                                            // [n_rg] rows of the group that have published; ZERO between launches
    int* live_cnt; int* live_list; unsigned long long* stat;     // as dae_launch_live_tiles; stat[3] += row groups proved empty
    // THE EMPTY LIST PROVED (nullable, both or neither; the instances with a decoded-tile table only): the {dq, tau_safe} pairs this
    // call's sample launch stored per half group and the envelope of `list` (empty_proof.h).  A group whose pairs prove that the
    // tail would keep nothing gets live_cnt = 0 and the counters from the workgroup of its first row; no workgroup of it arrives
    const float2* pair; const float* env;
};
int dae_launch_tau_select(dae_ctx* ctx, const float* gmax, int64_t ld_g, int n_g, const float* samp, int64_t ld_s,
                          int n_s, const int* samp_list, int col_lo, int B, int k, const int32_t* seed_row_ptr,
                          float* tau, uint2* out_pairs, int64_t pairs_stride, int* out_cnt, const dae_tau_live* live,
                          const unsigned* samp_tab = nullptr, int nb_rg = 0);
int dae_launch_topk_pairs(dae_ctx* ctx, const dae_pair_group& g0, const dae_pair_group& g1,
                          const dae_topk_args& a);
int dae_launch_topk_soa(dae_ctx* ctx, int G, const float* logit, const int32_t* idx,
                        const dae_topk_args& a);
// DAE_DTYPE_BF16_EXACT (refine.hip): the candidate lists of the bf16 filter launch hold upper bounds u of the fp32
// logits; in place, every candidate that can still be among the k best non-seeds gets its logit RECOMPUTED in fp32 --
// the canonical fmaf chain over k = 0..H-1 of h[row][k] * W32[col - col_lo][k], + bias[col - col_lo] -- and every other
// one -inf (absent for the selection kernel)
struct dae_exact_src {
    const float* h; int64_t ld_h; int H;          // fp32 hidden rows [B][ld_h]
    const float* W32; const float* bias; int col_lo;
    const int* row_bad;                           // nullable: rows flagged 1 return no candidates (idx -1)
    const float* eps_max;                         // device scalar: max over the image's columns of eps_c
    const float* eps;                             // [ncols] the per-column bounds (the guard tests each recomputed survivor)
    int* guard;                                   // nullable: device {violations, a violating column} (dae_exact_guard_read)
};
// out / out_cnt / out_cap (nullable): per row a compact list [out_cap] of the survivors' (fp32 logit, column) pairs and its
// length; rows that fit get it filled and their g1 lists emptied (counts zeroed), the others are refined in place.
// fused (nullable; dae_exact_refine_can_fuse): the launch ENDS the scoring call -- seeds removed, the k best of every row in
// order to fused->out_score / out_idx, exactly what dae_launch_topk_pairs over the refined lists returns -- and the lists it
// leaves behind are not meant to be read
// audit.hip: one audit of the exact scoring launch in progress (n_tiles random ranked tiles x all B rows -> the guard words)
int dae_launch_exact_audit(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_exact_src& x, int nrank, int n_tiles);
// (pieces the exact title mix's audit shares: dae_launch_mix_audit) this audit's tile ids + the context's totals; the canonical
// logits of those tiles for rows [0, B) into zout[B][n_tiles * 32]
int dae_audit_pick_tiles(dae_ctx* ctx, int n_rank_tiles, int n_tiles, unsigned long long** stat_out, int** tiles_out);
int dae_launch_audit_chains(dae_ctx* ctx, const float* h, int64_t ld_h, int H, const float* W32, const float* bias, int ncols,
                            int col_bound, int B, const int* tiles, int n_tiles, float* zout);
bool dae_exact_refine_can_fuse(const dae_topk_args& a);
int dae_launch_exact_refine(dae_ctx* ctx, const dae_pair_group& g1, const dae_exact_src& x, int B, int k,
                            const int32_t* seed_row_ptr, uint2* out = nullptr, int* out_cnt = nullptr, int out_cap = 0,
                            int* stat = nullptr, const dae_topk_args* fused = nullptr);
// ensemble.hip -- what the ensemble calls share
// The scorers of an ensemble call, as the entry points take them: M member contexts with their hidden rows, widths and weights
// (HOST arrays of M entries), and the title context (nullable) with the width of its feature rows.  dae_ensemble_check refuses
// what dae_ensemble_topk refuses about them -- a null, doubled, foreign-device or foreign-stream context, one with
// dae_set_score_mix set, one without a plain image of `dtype` over the whole vocabulary, images of different V, an H that is not
// its image's -- with `fn` as the call's name in the message, which goes to rc_ctx; *V_out = the images' column count.  dtype < 0:
// the call reads no image, so none is asked for (*V_out = 0).
int dae_ensemble_check(const char* fn, dae_ctx* rc_ctx, dae_ctx* const* members, int M, const float* const* h, const int* H,
                       const float* const* row_scale, dae_ctx* title_ctx, int ld_feat, int dtype, int* V_out);
// The canonical value y at the listed pairs into out[n_cand], everything on rc_ctx's stream: per scorer the candidate chain with
// the sigmoid into s + i * s_stride (i < M + (feat ? 1 : 0)), then the combining launch.  No check of its own but
// dae_decode_candidates'.
struct dae_ens_tensors {
    int M; const float* const* h; const int* H; const float* const* row_scale; const float* const* W_dec; const float* const* b_dec;
    const float* feat; int ld_feat; const float* OutW_T; const float* Out_b; const float* w_title;      // all null / 0 when untitled
};
int dae_launch_ensemble_candidates(dae_ctx* rc_ctx, const dae_ens_tensors& t, int B, int V, const int32_t* row_ptr, const int32_t* col,
                                   int n_cand, float* s, size_t s_stride, float* out, int32_t* status);
