// candidates.hip -- score and rank CALLER-GIVEN columns: what the model thinks of these columns for this playlist, without the
// [B, V] matrix a dense decode writes to answer it (a reranker over another generator's candidates, held-out answers among
// sampled negatives, a catalogue restricted to a market).
//
// Input: a candidate CSR on the device, cand_row_ptr[B + 1] / cand_col[n_cand], int32 GLOBAL column ids -- tracks and artists,
// any order, duplicates allowed.  Per listed (row r, column c) the launch runs the canonical chain
//     acc = fmaf(h[r][k], W[c][k], acc) over k = 0 .. H-1 from +0, then + b[c]
// -- oracle/dae_oracle.c orc_decode, the operation v_mfma_f32_32x32x2_f32 performs in the fp32 kernels, step 2 of refine.hip --
// against the model's OWN row-major fp32 [V, H] decoder tensor (no prepacked image), so the numbers are bit for bit those of
// dae_decode_dense at [r, c].
//   candidate_logits_kernel : z or the canonical sigmoid of z (out_kind), in the order of cand_col;
//   candidate_mix_kernel    : two chains per candidate (the DAE's, and the title features against Output_W^T), mixed with
//                             mix_scores_kernel's operations in their order (title.hip): dae_decode_dense x 2 + dae_mix_scores.
// A lane owns a candidate and its serial chain; the row's h sits in LDS; the decoder rows are fetched as refine.hip found
// necessary: the 4 lanes of a quad read 64 CONTIGUOUS bytes of one row per instruction, re-distributed through 5 KiB of LDS
// per wave (80-byte row stride), 4 blocks of 16 k in flight per lane, refilled in pairs (the two halves of a 128-byte line).
//
// WORKGROUP -> (row, chunk) without a host read of cand_row_ptr: a workgroup takes DAE_CAND_CHUNK candidates of ONE row, and row r owns
// the workgroup ids [row_ptr[r] / DAE_CAND_CHUNK + r, row_ptr[r + 1] / DAE_CAND_CHUNK + r + 1) -- a strictly increasing function of r, so a
// workgroup finds its row by a search over row_ptr (two rounds of 64 lanes), and floor(b / C) - floor(a / C) + 1 >= ceil((b - a) / C)
// ids are enough for the row's chunks (the surplus ids find nothing to do).  The grid is n_cand / DAE_CAND_CHUNK + B: the caller's
// n_cand, no device read.
//
// IDS.  -1 is padding: its slot receives -inf (what the rankers write beside an index of -1), no flag.  Any other id outside
// [0, V) receives a quiet NaN, is never dereferenced, and ORs bit 0 into the (nullable) device status word.
//
// RANKING adds no selection kernel: candidate_pairs_kernel writes (key, column) pairs, one list per row at a fixed row stride --
// the layout topk.hip's PairSrc takes -- and the existing selection orders them (key descending, column ascending, seeds
// removed, (-1, -inf) beyond the list).  A column listed twice is ranked twice: the caller's contract.
#include "dae_internal.h"

namespace {

constexpr int CD_THREADS = 256;        // 4 waves
constexpr int CD_WAVES = CD_THREADS / 64;
constexpr int CD_ROWSTRIDE = 20;       // dwords per candidate in a wave's transposition buffer (16 data + 4 pad): refine.hip
constexpr int CD_DEPTH = 4;            // blocks of 16 k in flight per lane: one 64-k chunk of the hidden row per trip
constexpr int CD_MAXH = 1024;

// row of workgroup `wg`: the largest r in [0, B] with row_ptr[r] / DAE_CAND_CHUNK + r <= wg (r == B: no work).  Every wave searches
// for itself (uniform result, no barrier): 64 probes a round, two rounds for B <= 4096.
__device__ __forceinline__ int cd_find_row(const int32_t* __restrict__ row_ptr, int B, int wg, int lane)
{
    const int step = (B + 1 + 63) >> 6;                       // <= 65
    const int r1 = lane * step;
    const bool ok1 = r1 <= B && (row_ptr[r1 <= B ? r1 : B] / DAE_CAND_CHUNK + r1) <= wg;
    const int n1 = __popcll(__ballot(ok1));
    if (n1 == 0) return B;                                    // (a row_ptr that does not start at 0: nothing is this workgroup's)
    const int base = (n1 - 1) * step;
    int n = 0;
    for (int i0 = 0; i0 < step; i0 += 64) {
        const int r2 = base + i0 + lane;
        const bool ok2 = i0 + lane < step && r2 <= B && (row_ptr[r2 <= B ? r2 : B] / DAE_CAND_CHUNK + r2) <= wg;
        n += __popcll(__ballot(ok2));
    }
    return base + n - 1;
}

// One group of <= 64 candidates, a lane each: the chain of row-major W[colv][0 .. H) against the LDS row hrow (zero beyond H,
// 1024 floats) -> acc, WITHOUT the bias.  colv is a valid column on every lane (lanes without a candidate pass any).  HT > 0:
// H = 16 HT known at compile time -- no branch around a load, so the ring's waits are exact counts (refine.hip refine_body).
template <int HT>
__device__ __forceinline__ float cd_chain(const float* __restrict__ W, const int H, const float* hrow, float* tbuf,
                                          const int colv, const bool in, const int lane)
{
    const int Q = lane >> 2, q = lane & 3;
    const float4* rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ci = __shfl(colv, 4 * Q + i);
        rp[i] = reinterpret_cast<const float4*>(W + (size_t)ci * H) + q;
    }
    const int H16 = HT > 0 ? HT : (H >> 4);                   // blocks of 16 k
    const int Hrem4 = HT > 0 ? 0 : ((H & 15) >> 2);           // float4 left over after the whole blocks
    float4 v[CD_DEPTH][4];
#pragma unroll
    for (int d = 0; d < CD_DEPTH; ++d)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[d][i] = d < H16 ? rp[i][4 * d] : make_float4(0.f, 0.f, 0.f, 0.f);
    float acc = 0.0f;
#pragma unroll 1                                              // (rolled: unrolled, hipcc hoists the chain's loads -- refine.hip)
    for (int j0 = 0; j0 < H16; j0 += CD_DEPTH) {
        // lane l holds h[16 j0 + l] of this 64-k chunk; every product takes its factor by v_readlane (refine.hip)
        const int hc = (int)__float_as_uint(hrow[(16 * j0 + lane) & (CD_MAXH - 1)]);
#pragma unroll
        for (int dd = 0; dd < CD_DEPTH; ++dd) {
            const int j = j0 + dd;
            if (HT > 0 || j < H16) {                          // wave-uniform
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<float4*>(tbuf + (4 * Q + i) * CD_ROWSTRIDE + 4 * q) = v[dd][i];
                __builtin_amdgcn_wave_barrier();              // (a wave's LDS accesses execute in order; keep the compiler from moving them)
                if (dd & 1) {                                 // the ring is refilled in pairs of blocks: both halves of a line back to back
                    const int jn0 = j - 1 + CD_DEPTH, jn1 = j + CD_DEPTH;
                    if (HT > 0) {
                        const int c0 = jn0 < HT ? jn0 : HT - 1, c1 = jn1 < HT ? jn1 : HT - 1;   // (the last trip re-reads the row's end: never used)
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[dd - 1][i] = rp[i][4 * c0];
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[dd][i] = rp[i][4 * c1];
                    } else {
                        if (jn0 < H16) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[dd - 1][i] = rp[i][4 * jn0];
                        }
                        if (jn1 < H16) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[dd][i] = rp[i][4 * jn1];
                        }
                    }
                }
                float4 w[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) w[t] = *reinterpret_cast<const float4*>(tbuf + lane * CD_ROWSTRIDE + 4 * t);
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int l0 = 16 * dd + 4 * t;
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0)), w[t].x, acc);
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0 + 1)), w[t].y, acc);
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0 + 2)), w[t].z, acc);
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0 + 3)), w[t].w, acc);
                }
            }
        }
    }
    if (Hrem4 && in) {                                        // hidden sizes that are not a multiple of 16: the tail, lane-owned
        const float4* wr = reinterpret_cast<const float4*>(W + (size_t)colv * H);
        for (int t = 0; t < Hrem4; ++t) {
            const float4 wv = wr[4 * H16 + t];
            const int hb = 16 * H16 + 4 * t;
            acc = fmaf(hrow[hb], wv.x, acc);
            acc = fmaf(hrow[hb + 1], wv.y, acc);
            acc = fmaf(hrow[hb + 2], wv.z, acc);
            acc = fmaf(hrow[hb + 3], wv.w, acc);
        }
    }
    return acc;
}

struct CandP {
    const float* h; int64_t ld_h; int H;                      // fp32 hidden rows [B][ld_h]
    const float* W; const float* b; int V;                    // the model's row-major [V][H] decoder tensor and bias
    const float* feat; int64_t ld_feat; int HF;               // mix: title features [B][ld_feat], chain length HF = ld_feat
    const float* WT; const float* bT;                         // mix: Output_W^T [V][HF], Output_b [V]
    const float* w_title; const float* w_playlist;            // mix: [B]
    const int32_t* row_ptr; const int32_t* col; int n_cand, B;
    int out_kind; float* out; int32_t* status;
};

// MIX: candidate_mix_kernel (two chains, the mixed score); otherwise candidate_logits_kernel.  HT: as cd_chain (the DAE's chain).
template <bool MIX, int HT>
__device__ __forceinline__ void cd_body(const CandP& p)
{
    __shared__ __attribute__((aligned(16))) float tb[CD_WAVES * 64 * CD_ROWSTRIDE];
    __shared__ float hrow[CD_MAXH];
    __shared__ float frow[MIX ? CD_MAXH : 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = blockIdx.x;
    const int row = cd_find_row(p.row_ptr, p.B, wg, lane);
    if (row >= p.B) return;                                   // (block-uniform: every wave found the same row)
    const int rb = p.row_ptr[row], re_ = p.row_ptr[row + 1];
    const int chunk = wg - (rb / DAE_CAND_CHUNK + row);
    const int e0 = (rb > 0 ? rb : 0) + chunk * DAE_CAND_CHUNK;
    const int re = re_ < p.n_cand ? re_ : p.n_cand;           // nothing is read or written at or past the caller's n_cand
    if (e0 >= re) return;
    for (int i = tid; i < CD_MAXH; i += CD_THREADS) {
        hrow[i] = i < p.H ? p.h[(size_t)row * p.ld_h + i] : 0.0f;
        if (MIX) frow[i] = i < p.HF ? p.feat[(size_t)row * p.ld_feat + i] : 0.0f;
    }
    __syncthreads();
    const int e = e0 + wave * 64 + lane;
    const bool in = e < re;
    const int c = in ? p.col[e] : -1;
    const bool ok = c >= 0 && c < p.V;
    if (__ballot(ok) == 0ull) {                               // wave-uniform: no chain to run
        if (in) p.out[e] = c == -1 ? -__builtin_inff() : __builtin_nanf("");
        if (in && c != -1 && p.status) atomicOr(p.status, 1);
        return;
    }
    const int colv = ok ? c : 0;                              // lanes without a column fetch row 0 and drop the result
    float* tbuf = tb + wave * (64 * CD_ROWSTRIDE);
    float z = cd_chain<HT>(p.W, p.H, hrow, tbuf, colv, ok, lane) + p.b[colv];
    float y;
    if (MIX) {
        __builtin_amdgcn_wave_barrier();
        const float zt = cd_chain<0>(p.WT, p.HF, frow, tbuf, colv, ok, lane) + p.bT[colv];
        // mix_scores_kernel's operations in its order (title.hip: d = t * a + d * b; no contraction: -ffp-contract=off)
        const float ts = dae_sigmoidf(zt) * p.w_title[row];
        const float pd = dae_sigmoidf(z) * p.w_playlist[row];
        y = ts + pd;
    } else {
        y = p.out_kind == DAE_OUT_SCORE ? dae_sigmoidf(z) : z;
    }
    if (in) p.out[e] = ok ? y : (c == -1 ? -__builtin_inff() : __builtin_nanf(""));
    if (in && !ok && c != -1 && p.status) atomicOr(p.status, 1);
}

template <int HT>
__global__ __launch_bounds__(CD_THREADS) void candidate_logits_kernel(const CandP p) { cd_body<false, HT>(p); }
template <int HT>
__global__ __launch_bounds__(CD_THREADS) void candidate_mix_kernel(const CandP p) { cd_body<true, HT>(p); }

// the candidates of a row as (key, column) pairs at pairs[row * cap + i], i < cnt[row] = min(row length, cap); an id outside
// [0, V) becomes column -1: absent for the selection kernel (topk.hip ckey)
__global__ __launch_bounds__(256) void candidate_pairs_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col,
                                                              const float* __restrict__ key, int V, int cap,
                                                              uint2* __restrict__ pairs, int* __restrict__ cnt)
{
    const int row = blockIdx.y;
    const int rb = row_ptr[row];
    int n = row_ptr[row + 1] - rb;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[row] = n;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const int c = col[rb + i];
        pairs[(size_t)row * cap + i] = make_uint2(__float_as_uint(key[rb + i]), (c >= 0 && c < V) ? (unsigned)c : 0xFFFFFFFFu);
    }
}

// A row's repeated columns -> -1, so that dae_rank_candidates ranks every column once.  One workgroup per row, a bitmap over
// [0, V) in dynamic LDS (bm_words dwords, zeroed by the workgroup); the row is walked in chunks of DAE_CAND_CHUNK, a lane per id.
// ds_or_rtn decides: of all lanes that name a column -- in one chunk or in different ones -- exactly one finds its bit clear
// and keeps the id, every other one writes -1, so no barrier separates the chunks.  -1 and ids outside [0, V) are copied as
// they are.  A lane reads in[e] before it writes out[e] and touches no other slot: in == out is fine.  Bank conflicts: ids of
// one wave that fall into the same dword serialise in the LDS atomic unit; random ids over a bitmap of V / 32 dwords rarely do,
// and a row of one repeated id costs 64 serial atomics per wave -- small next to the 2 x H fetches the row's chains save.
__global__ __launch_bounds__(DAE_CAND_CHUNK) void candidates_unique_kernel(const int32_t* __restrict__ row_ptr, const int32_t* in,
                                                                            int32_t* out, int n_cand, int V, int bm_words)
{
    extern __shared__ unsigned cu_bitmap[];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int rb_ = row_ptr[row], re_ = row_ptr[row + 1];
    const int rb = rb_ > 0 ? rb_ : 0;
    const int re = re_ < n_cand ? re_ : n_cand;                // nothing is read or written at or past the caller's n_cand
    if (re - rb < 2) {                                         // (block-uniform) nothing to compare: the copy alone
        if (tid == 0 && re > rb) out[rb] = in[rb];
        return;
    }
    for (int i = tid; i < bm_words; i += DAE_CAND_CHUNK) cu_bitmap[i] = 0u;
    __syncthreads();
    for (int e = rb + tid; e < re; e += DAE_CAND_CHUNK) {
        int c = in[e];
        if (c >= 0 && c < V) {                                 // (c >> 5 < bm_words = ceil(V / 32))
            const unsigned bit = 1u << (c & 31);
            if (atomicOr(&cu_bitmap[c >> 5], bit) & bit) c = -1;
        }
        out[e] = c;
    }
}

int check_cand_args(dae_ctx* ctx, const void* h, int64_t ld_h, int B, int H, const void* W, const void* b, int V,
                    const void* row_ptr, const void* col, int n_cand, const void* out)
{
    if (!h || !W || !b || !row_ptr || !col || !out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (H <= 0 || (H % 4) != 0 || H > CD_MAXH) return dae_fail(ctx, DAE_ERR_ARG, "H=%d must be a multiple of 4 in [4, %d]", H, CD_MAXH);
    if (B < 1 || B > 4096) return dae_fail(ctx, DAE_ERR_ARG, "B=%d out of [1, 4096]", B);
    if (V <= 0 || n_cand < 0 || ld_h < H) return dae_fail(ctx, DAE_ERR_ARG, "bad shape V=%d n_cand=%d ld_h=%lld", V, n_cand, (long long)ld_h);
    if (reinterpret_cast<uintptr_t>(W) % 16) return dae_fail(ctx, DAE_ERR_ARG, "the decoder tensor must be 16-byte aligned");
    return DAE_OK;
}

int launch_candidates(dae_ctx* ctx, const CandP& p, bool mix)
{
    const unsigned grid = (unsigned)(p.n_cand / DAE_CAND_CHUNK + p.B);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    dae_take_profile_events(ctx, mix ? "candidate_mix_kernel" : "candidate_logits_kernel", e0, e1);
    if (e0) DAE_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
    if (mix) {
        if (p.H == 256) hipLaunchKernelGGL(candidate_mix_kernel<16>, dim3(grid), dim3(CD_THREADS), 0, ctx->stream, p);
        else hipLaunchKernelGGL(candidate_mix_kernel<0>, dim3(grid), dim3(CD_THREADS), 0, ctx->stream, p);
    } else {
        if (p.H == 256) hipLaunchKernelGGL(candidate_logits_kernel<16>, dim3(grid), dim3(CD_THREADS), 0, ctx->stream, p);
        else hipLaunchKernelGGL(candidate_logits_kernel<0>, dim3(grid), dim3(CD_THREADS), 0, ctx->stream, p);
    }
    DAE_CHECK_LAUNCH(ctx, mix ? "candidate_mix_kernel" : "candidate_logits_kernel");
    if (e1) DAE_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    return DAE_OK;
}

}  // namespace

static_assert(DAE_CAND_CHUNK == CD_THREADS, "a lane per candidate: a workgroup's chunk is its thread count");

extern "C" {

int dae_decode_candidates(dae_ctx* ctx, const float* h, int64_t ld_h, int B, int H, const float* W_dec, const float* b_dec, int V,
                          const int32_t* cand_row_ptr, const int32_t* cand_col, int n_cand, int out_kind, float* out,
                          int32_t* status)
{
    if (!ctx) return DAE_ERR_ARG;
    int rc = check_cand_args(ctx, h, ld_h, B, H, W_dec, b_dec, V, cand_row_ptr, cand_col, n_cand, out);
    if (rc) return rc;
    if (out_kind != DAE_OUT_SCORE && out_kind != DAE_OUT_LOGIT) return dae_fail(ctx, DAE_ERR_ARG, "out_kind=%d", out_kind);
    CandP p{};
    p.h = h; p.ld_h = ld_h; p.H = H; p.W = W_dec; p.b = b_dec; p.V = V;
    p.row_ptr = cand_row_ptr; p.col = cand_col; p.n_cand = n_cand; p.B = B;
    p.out_kind = out_kind; p.out = out; p.status = status;
    return launch_candidates(ctx, p, false);
}

int dae_score_candidates(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                         const float* b_enc, int V, int H, int B, const float* W_dec, const float* b_dec,
                         const int32_t* cand_row_ptr, const int32_t* cand_col, int n_cand, int out_kind, float* out,
                         int32_t* status)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !W_enc || !b_enc) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if ((reinterpret_cast<uintptr_t>(W_enc) | reinterpret_cast<uintptr_t>(b_enc)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "W_enc, b_enc must be 16-byte aligned");
    int rc = check_cand_args(ctx, W_enc, H, B, H, W_dec, b_dec, V, cand_row_ptr, cand_col, n_cand, out);
    if (rc) return rc;
    rc = dae_reserve(ctx, ctx->h_scratch, (size_t)B * H * sizeof(float));      // the hidden rows stay in the context, as dae_score_topk's
    if (rc) return rc;
    float* h = static_cast<float*>(ctx->h_scratch.p);
    rc = dae_launch_encode(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, 1.0f, 1.0f, 0u, h, nullptr, 0, 0);
    if (rc) return rc;
    return dae_decode_candidates(ctx, h, H, B, H, W_dec, b_dec, V, cand_row_ptr, cand_col, n_cand, out_kind, out, status);
}

int dae_mix_candidates(dae_ctx* title_ctx, dae_ctx* dae, const float* h, int64_t ld_h, int H, const float* W_dec,
                       const float* b_dec, const float* feat, int64_t ld_feat, const float* OutW_T, const float* Out_b,
                       const float* w_title, const float* w_playlist, int B, int V, const int32_t* cand_row_ptr,
                       const int32_t* cand_col, int n_cand, float* out, int32_t* status)
{
    dae_ctx* ctx = title_ctx;
    if (!ctx || !dae) return DAE_ERR_ARG;
    if (ctx->stream != dae->stream) return dae_fail(ctx, DAE_ERR_STATE, "both contexts must be bound to the same stream");
    int rc = check_cand_args(ctx, h, ld_h, B, H, W_dec, b_dec, V, cand_row_ptr, cand_col, n_cand, out);
    if (rc) return rc;
    if (!feat || !OutW_T || !Out_b || !w_title || !w_playlist) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (ld_feat <= 0 || (ld_feat % 4) != 0 || ld_feat > CD_MAXH)
        return dae_fail(ctx, DAE_ERR_ARG, "ld_feat=%lld must be a multiple of 4 in [4, %d]", (long long)ld_feat, CD_MAXH);
    if (reinterpret_cast<uintptr_t>(OutW_T) % 16) return dae_fail(ctx, DAE_ERR_ARG, "Output_W^T must be 16-byte aligned");
    CandP p{};
    p.h = h; p.ld_h = ld_h; p.H = H; p.W = W_dec; p.b = b_dec; p.V = V;
    p.feat = feat; p.ld_feat = ld_feat; p.HF = (int)ld_feat; p.WT = OutW_T; p.bT = Out_b;
    p.w_title = w_title; p.w_playlist = w_playlist;
    p.row_ptr = cand_row_ptr; p.col = cand_col; p.n_cand = n_cand; p.B = B;
    p.out_kind = DAE_OUT_LOGIT; p.out = out; p.status = status;
    return launch_candidates(ctx, p, true);
}

int dae_candidates_unique(dae_ctx* ctx, int B, int V, const int32_t* cand_row_ptr, const int32_t* cand_col_in, int32_t* cand_col_out,
                          int n_cand)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!cand_row_ptr || !cand_col_in || !cand_col_out) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B < 1 || B > 4096) return dae_fail(ctx, DAE_ERR_ARG, "B=%d out of [1, 4096]", B);
    if (V <= 0 || n_cand < 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape V=%d n_cand=%d", V, n_cand);
    if (V > DAE_CAND_UNIQUE_MAX_V)
        return dae_fail(ctx, DAE_ERR_ARG, "dae_candidates_unique: V=%d is too wide for the LDS bitmap over [0, V) (at most %d columns)", V,
                        DAE_CAND_UNIQUE_MAX_V);
    if (n_cand == 0) return DAE_OK;
    const int bm_words = (V + 31) >> 5;
    const size_t lds = (size_t)bm_words * sizeof(unsigned);
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, candidates_unique_kernel, (size_t)DAE_CAND_UNIQUE_MAX_V / 8));
    hipLaunchKernelGGL(candidates_unique_kernel, dim3(B), dim3(DAE_CAND_CHUNK), lds, ctx->stream, cand_row_ptr, cand_col_in, cand_col_out,
                       n_cand, V, bm_words);
    DAE_CHECK_LAUNCH(ctx, "candidates_unique_kernel");
    return DAE_OK;
}

int dae_rank_candidates(dae_ctx* ctx, int B, int V, const int32_t* cand_row_ptr, const int32_t* cand_col, const float* key,
                        int row_cap, const int32_t* seed_row_ptr, const int32_t* seed_col, int k, int out_kind,
                        float* out_score, int32_t* out_idx)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!cand_row_ptr || !cand_col || !key || !out_score || !out_idx) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (B < 1 || B > 4096) return dae_fail(ctx, DAE_ERR_ARG, "B=%d out of [1, 4096]", B);
    if (V <= 0 || row_cap < 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape V=%d row_cap=%d", V, row_cap);
    if (k < 1 || k > DAE_MAX_K_DEEP) return dae_fail(ctx, DAE_ERR_ARG, "k=%d out of [1,%d]", k, DAE_MAX_K_DEEP);
    if ((seed_row_ptr == nullptr) != (seed_col == nullptr))
        return dae_fail(ctx, DAE_ERR_ARG, "seed_row_ptr and seed_col must both be given or both null");
    const int cap = row_cap > 0 ? row_cap : 1;
    // [B][cap] pairs, then [B] counts
    const size_t pair_bytes = (size_t)B * cap * sizeof(uint2);
    int rc = dae_reserve(ctx, ctx->cand_list, pair_bytes + (size_t)B * sizeof(int));
    if (rc) return rc;
    uint2* pairs = static_cast<uint2*>(ctx->cand_list.p);
    int* cnt = reinterpret_cast<int*>(static_cast<char*>(ctx->cand_list.p) + pair_bytes);
    const int bx = cap >= 256 * 64 ? 64 : (cap + 255) / 256;
    hipLaunchKernelGGL(candidate_pairs_kernel, dim3(bx, B), dim3(256), 0, ctx->stream, cand_row_ptr, cand_col, key, V, cap, pairs,
                       cnt);
    DAE_CHECK_LAUNCH(ctx, "candidate_pairs_kernel");
    dae_topk_args ta;
    memset(&ta, 0, sizeof(ta));
    ta.B = B; ta.k = k; ta.out_kind = out_kind;
    ta.bitmap_base = 0; ta.bitmap_n = V;
    ta.seed_row_ptr = seed_row_ptr; ta.seed_col = seed_col;
    ta.out_score = out_score; ta.out_idx = out_idx;
    dae_pair_group g0{pairs, cnt, 0, cap, 0, 1, 0};
    dae_pair_group g1{nullptr, nullptr, 0, 0, 0, 0, 0};
    return dae_launch_topk_pairs(ctx, g0, g1, ta);
}

}  // extern "C"
