// prepack.hip -- everything that turns the model and a batch into the operand images the decode kernels stream
// (DESIGN.md "HBM layout"): the decoder in MFMA A-operand order (fp32 / bf16, with the bias fragments and, for
// DAE_DTYPE_BF16_EXACT, the per-column bounds), the hidden rows in B-operand order, and the tile lists of the fused path
// (identity, bias order, the sample re-dealt by popularity band).
#include <atomic>

#include "decode_common.h"

namespace {

// ---- prepack: W_dec rows -> MFMA A-operand order ----------------------------------------------
// One workgroup per 32-column tile: the tile's 32 rows of W (32 x H floats, contiguous 4 H bytes each) are read
// with coalesced 16-byte loads into LDS and written out in operand order with coalesced 16-byte stores.
// (A thread gathering its own 4 / 8 strided scalars straight from HBM took 139 us for the 174 MB matrix --
// 2.5 TB/s of traffic; the training step re-tiles the decoder every step.)
//   fp32: out float4 index = (t*G + g)*64 + lane, lane = hi*32 + i; component e = W[col_lo+32t+i][8g + 2e + hi]
//   bf16: out uint4  index = (t*NS + s)*64 + lane: bf16 of W[col_lo+32t+i][16s + 8hi + 0..7]
//         bias fragments: lane (hi = 0, i) of tile t carries b[col_lo + 32 t + i] = e0 + e1 + e2 in k-slots 0..2
// (zero outside the matrix)
constexpr int PP_PAD = 4;          // LDS row stride Hp + 4 floats: rows stay 16-byte aligned

template <int DT>
__global__ __launch_bounds__(256) void prepack_tile_kernel(const float* __restrict__ W,
                                                           const float* __restrict__ b, int H, int Hp,
                                                           int col_lo, int col_hi, int ntiles,
                                                           void* __restrict__ Wp_,
                                                           float* __restrict__ bias,
                                                           uint4* __restrict__ bias16)
{
    extern __shared__ __attribute__((aligned(16))) float pp_tile[];      // [32][Hp + PP_PAD]
    const int tid = threadIdx.x;
    const int ldt = Hp + PP_PAD;
    const int Hp4 = Hp >> 2;
    const bool vec = (H & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int v0 = col_lo + t * 32;
        for (int idx = tid; idx < 32 * Hp4; idx += 256) {
            const int r = idx / Hp4, c4 = idx - r * Hp4;
            const int v = v0 + r, k = 4 * c4;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (v < col_hi) {
                const float* src = W + (size_t)v * H + k;
                if (vec && k + 3 < H) {
                    x = *reinterpret_cast<const float4*>(src);
                } else {
                    if (k < H) x.x = src[0];
                    if (k + 1 < H) x.y = src[1];
                    if (k + 2 < H) x.z = src[2];
                    if (k + 3 < H) x.w = src[3];
                }
            }
            *reinterpret_cast<float4*>(pp_tile + r * ldt + k) = x;
        }
        __syncthreads();
        if (DT == DT_F32) {
            float4* Wp = static_cast<float4*>(Wp_);
            const int G = Hp >> 3;
            for (int o = tid; o < G * 64; o += 256) {
                const int lane = o & 63, g = o >> 6;
                const float* row = pp_tile + (lane & 31) * ldt + 8 * g + (lane >> 5);
                Wp[(size_t)t * G * 64 + o] = make_float4(row[0], row[2], row[4], row[6]);
            }
        } else {
            uint4* Wp = static_cast<uint4*>(Wp_);
            const int NS = Hp >> 4;
            for (int o = tid; o < NS * 64; o += 256) {
                const int lane = o & 63, sidx = o >> 6;
                const float* row = pp_tile + (lane & 31) * ldt + 16 * sidx + 8 * (lane >> 5);
                const float4 lo = *reinterpret_cast<const float4*>(row), hi4 = *reinterpret_cast<const float4*>(row + 4);
                Wp[(size_t)t * NS * 64 + o] =
                    make_uint4(dae_bf16_rne(lo.x) | (dae_bf16_rne(lo.y) << 16), dae_bf16_rne(lo.z) | (dae_bf16_rne(lo.w) << 16),
                               dae_bf16_rne(hi4.x) | (dae_bf16_rne(hi4.y) << 16), dae_bf16_rne(hi4.z) | (dae_bf16_rne(hi4.w) << 16));
            }
        }
        if (tid < 32) bias[t * 32 + tid] = v0 + tid < col_hi ? b[v0 + tid] : 0.0f;
        if (DT == DT_BF16 && tid < 64) {
            const int v = v0 + (tid & 31);
            uint4 f = make_uint4(0u, 0u, 0u, 0u);
            if ((tid >> 5) == 0 && v < col_hi) {
                const float bv = b[v];
                const unsigned e0 = dae_bf16_rne(bv);
                const float r1 = bv - __uint_as_float(e0 << 16);
                const unsigned e1 = dae_bf16_rne(r1);
                const float r2 = r1 - __uint_as_float(e1 << 16);
                const unsigned e2 = dae_bf16_rne(r2);
                f.x = e0 | (e1 << 16); f.y = e2;
            }
            bias16[t * 64 + tid] = f;
        }
        __syncthreads();
    }
}

// ---- DAE_DTYPE_BF16_EXACT: per-column bound of |fp32 logit - bf16 logit| -----------------------------------------
// z32(r, c) = the canonical fp32 chain acc = fmaf(h[k], W[c][k], acc), + b[c]  (oracle orc_decode, DAEs.py:141-145)
// z16(r, c) = what the bf16 decode kernels (decode_f32.hip, decode_generic.hip) leave in an accumulator: bias terms e0 + e1 + e2 and the products
//             bf16(h[k]) * bf16(W[c][k]) (exact in fp32) summed by v_mfma_f32_32x32x16_bf16 in an unspecified order.
// With h[k] in [0, 1] (sigmoid outputs): |bf16(h) - h| <= 2^-9, bf16(h) <= 1, hence against the real-number value
//   | sum bf16(h) bf16(W) - sum h W | <= d_c + 2^-9 n_c,   d_c = sum_k |bf16(W[c][k]) - W[c][k]|,  n_c = sum_k |W[c][k]|
// (d_c is the rounding this image really made: on average a third of the worst case 2^-8 n_c);
//   accumulation, bf16 MFMA: every term runs through at most Hp + 3 additions of unknown order; an addition is taken
//     to err by <= 2^-23 relative (TWICE fp32's unit roundoff: covers a truncating adder), and the total is doubled
//     again: A16 = (Hp + 16) 2^-22 times the sum of the magnitudes (n_c + d_c + |b| + eps);
//     tests/test_gpu_exact.py pins the assumption: measured |z16 - exact| stays below a quarter of this term;
//   accumulation, fp32 chain: (H + 2) 2^-24 (1 + 2^-10) (n_c + |b|)   (standard recursive-summation bound, fma);
//   the three-term bf16 split of b -+ eps: exact to 2^-24 relative (taken as 2^-23).
// Everything in double, rounded away from b when stored.  One 256-thread workgroup per 32-column tile: 8 threads per
// column.  bias16_lo / bias16_hi: bias fragments (see prepack_tile_kernel) of b - eps and b + eps.
__device__ __forceinline__ uint4 bias_fragment(float bv)
{
    const unsigned e0 = dae_bf16_rne(bv);
    const float r1 = bv - __uint_as_float(e0 << 16);
    const unsigned e1 = dae_bf16_rne(r1);
    const float r2 = r1 - __uint_as_float(e1 << 16);
    const unsigned e2 = dae_bf16_rne(r2);
    return make_uint4(e0 | (e1 << 16), e2, 0u, 0u);
}

__global__ __launch_bounds__(256) void exact_bounds_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                           int H, int Hp, int col_lo, int col_hi, int ntiles,
                                                           float* __restrict__ eps, uint4* __restrict__ bias16_lo,
                                                           uint4* __restrict__ bias16_hi, float margin,
                                                           int m_lo, int m_hi, float m_scale)
{
    float* eps_max = eps + (size_t)ntiles * 32;          // zeroed by the launcher; positive floats order like their bits
    const int tid = threadIdx.x;
    const int c = tid >> 3, part = tid & 7;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int v = col_lo + t * 32 + c;
        double n = 0.0, d = 0.0;
        if (v < col_hi) {
            const float* row = W + (size_t)v * H;
            for (int k = part; k < H; k += 8) {
                const float w = row[k];
                const float w16 = __uint_as_float(dae_bf16_rne(w) << 16);
                n += fabs((double)w);
                d += fabs((double)w16 - (double)w);
            }
        }
#pragma unroll
        for (int sh = 1; sh < 8; sh <<= 1) { n += __shfl_xor(n, sh); d += __shfl_xor(d, sh); }
        if (part == 0) {
            float e_f = 0.0f, lo_f = 0.0f, hi_f = 0.0f;
            if (v < col_hi) {
                const double bv = (double)b[v], ab = fabs(bv);
                const double A16 = (double)(Hp + 16) * 0x1p-22;
                const double A32 = (double)(H + 2) * 0x1p-24 * (1.0 + 0x1p-10);
                double e = d + 0x1p-9 * n + A16 * (n + d + 1.01 * ab) + A32 * (n + ab);
                e = e * (1.0 + 4.0 * A16) + 0x1p-23 * (ab + e) + 1e-30;      // eps feeds back through the shifted bias; split error
                e *= 1.0 + 1e-6;
                // dae_set_exact_margin: 1 by default; < 1 voids the bound (the guard's test hook; _range: for some columns only)
                const bool in_range = v >= m_lo && v < m_hi;
                e *= (double)(in_range && m_scale > 0.0f ? m_scale : margin);
                e_f = (float)e;
                if ((double)e_f < e) e_f = __uint_as_float(__float_as_uint(e_f) + 1u);      // e > 0: next float up
                double lo = bv - (double)e_f, hi = bv + (double)e_f;
                if (in_range && m_scale < 0.0f) hi = bv + (double)m_scale;     // (a FORGED filter: the upper bound |scale| logits low)
                lo_f = (float)lo; if ((double)lo_f > lo) lo_f = nextafterf(lo_f, -__builtin_inff());
                hi_f = (float)hi; if ((double)hi_f < hi) hi_f = nextafterf(hi_f, __builtin_inff());
            }
            eps[t * 32 + c] = e_f;
            if (e_f > 0.0f) atomicMax(reinterpret_cast<unsigned*>(eps_max), __float_as_uint(e_f));
            bias16_lo[t * 64 + c] = bias_fragment(lo_f);
            bias16_hi[t * 64 + c] = bias_fragment(hi_f);
            bias16_lo[t * 64 + 32 + c] = make_uint4(0u, 0u, 0u, 0u);
            bias16_hi[t * 64 + 32 + c] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// ---- tile order for the fused path's threshold sample -------------------------------------------
// The sample only has to be SOME subset of the rankable columns (its k-th largest logit is a lower
// bound of the row's k-th largest whatever the subset), but the tighter that bound, the fewer
// candidates phase B has to keep.  Vocabulary ids are popularity ranks and the trained b_dec is the
// popularity prior, so the tiles with the largest bias hold most of every row's winners: sample
// those.  One workgroup: key = (ordered max bias over the tile's rankable columns, ~tile) sorted
// descending by a bitonic network in LDS.
constexpr int ORDER_MAX_TILES = 8192;
__global__ __launch_bounds__(1024) void tile_order_kernel(const float* __restrict__ bias, int ntiles,
                                                          int nrank, int* __restrict__ order)
{
    __shared__ unsigned long long keys[ORDER_MAX_TILES];
    int n2 = 1024;
    while (n2 < ntiles) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += 1024) {
        unsigned long long k = 0ULL;                       // padding sorts last
        if (i < ntiles) {
            float m = -__builtin_inff();
            for (int c = 0; c < 32; ++c) {
                const int col = i * 32 + c;
                if (col < nrank) m = fmaxf(m, bias[col]);
            }
            k = ((unsigned long long)dae_okey(m) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
        }
        keys[i] = k;
    }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < n2; i += 1024) {
                const int jx = i ^ stride;
                if (jx > i) {
                    const unsigned long long a = keys[i], b = keys[jx];
                    const bool desc = (i & size) == 0;
                    if (desc ? (a < b) : (a > b)) { keys[i] = b; keys[jx] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < ntiles; i += 1024)
        order[i] = (int)(0xFFFFFFFFu - (unsigned)(keys[i] & 0xFFFFFFFFULL));
}

__global__ __launch_bounds__(256) void tile_iota_kernel(int n, int* __restrict__ out)
{
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += gridDim.x * 256) out[t] = t;
}

// The threshold sample re-dealt for a launch of several ROUNDS (dae_launch_tile_band).  Phase A takes, per (row, position in the
// tile), the maximum over the `waves` tiles a workgroup decodes together in a round; the threshold is the (k + seeds)-th largest
// of these maxima, so two winners in one group cost one of them.  Item i of the sample goes to round i / n_ws, wave (i % n_ws) /
// nb_rg, workgroup i % nb_rg: with ONE round the group's tiles sit nb_rg places apart in the bias order (128 at batch 256) --
// different popularity bands; with ten rounds (2 048 rows: 16 workgroups per row group) they sit 16 apart, round 0 is the 64 most
// popular tiles in 16 groups of 4, ~550 winners share 512 maxima, the threshold drops into the next round's maxima and 1 155
// candidates per row pass instead of 534.  Here wave w's items (all rounds, all workgroups) take the w-th band of the order.
__global__ __launch_bounds__(256) void tile_band_kernel(const int* __restrict__ order, int ntiles, int n_samp, int nb_rg,
                                                        int waves, int* __restrict__ band)
{
    const int n_ws = nb_rg * waves;
    const int R = n_samp / n_ws, rem_last = n_samp - R * n_ws;
    for (int it = blockIdx.x * 256 + threadIdx.x; it < ntiles; it += gridDim.x * 256) {
        if (it >= n_samp) { band[it] = order[it]; continue; }
        const int round = it / n_ws, rem = it - round * n_ws, w = rem / nb_rg, bir = rem - w * nb_rg;
        int rank = round * nb_rg + bir;                       // items of wave w in front of this one: every lower (round, bir) exists
        for (int wp = 0; wp < w; ++wp) {                      // + all items of the waves before it
            int last = rem_last - wp * nb_rg;
            last = last < 0 ? 0 : (last > nb_rg ? nb_rg : last);
            rank += R * nb_rg + last;
        }
        band[it] = order[rank];
    }
}

// fallback for more than ORDER_MAX_TILES ranked tiles: every S-th tile first, then the others (n_samp = ceil(ntiles / S))
__global__ __launch_bounds__(256) void tile_order_strided_kernel(int ntiles, int n_samp, int S,
                                                                 int* __restrict__ order)
{
    for (int t = blockIdx.x * 256 + threadIdx.x; t < ntiles; t += gridDim.x * 256) {
        if (t % S == 0) order[t / S] = t;
        else order[n_samp + (t / S) * (S - 1) + (t % S) - 1] = t;
    }
}

// ---- pack h [B,H] -> MFMA B-operand order per row group ---------------------------------------
// out float4 index = ((rg*G + g)*RB + rb)*64 + lane, lane = hi*32 + j; component e holds
// h[rg*R_TILE + rb*32 + j][8g + 2e + hi]  (zero outside).
__global__ __launch_bounds__(256) void pack_h_kernel(const float* __restrict__ h, int B, int H,
                                                     int G, int RB, int n_rg,
                                                     float4* __restrict__ hp)
{
    const size_t total = (size_t)n_rg * G * RB * 64;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total;
         o += (size_t)gridDim.x * 256) {
        const int lane = (int)(o & 63);
        size_t x = o >> 6;
        const int rb = (int)(x % RB); x /= RB;
        const int g = (int)(x % G);
        const int rg = (int)(x / G);
        const int hi = lane >> 5, jj = lane & 31;
        const int r = (rg * RB + rb) * 32 + jj;
        float e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 8 * g + 2 * c + hi;
            e[c] = (r < B && k < H) ? h[(size_t)r * H + k] : 0.0f;
        }
        hp[o] = make_float4(e[0], e[1], e[2], e[3]);
    }
}

// out uint4 index = ((rg*NS + s)*RB + rb)*64 + lane: bf16 of h[(rg*RB+rb)*32+j][16s+8hi+0..7]
// row_bad (nullable, zeroed by the launcher): set to 1 for rows with an entry outside [0, 1] (or NaN) -- the
// precondition of DAE_DTYPE_BF16_EXACT's bound
__global__ __launch_bounds__(256) void pack_h_bf16_kernel(const float* __restrict__ h, int B, int H,
                                                          int NS, int RB, int n_rg,
                                                          uint4* __restrict__ hp, int* __restrict__ row_bad)
{
    const size_t total = (size_t)n_rg * NS * RB * 64;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
        const int lane = (int)(o & 63);
        size_t x = o >> 6;
        const int rb = (int)(x % RB); x /= RB;
        const int s = (int)(x % NS);
        const int rg = (int)(x / NS);
        const int hi = lane >> 5, jj = lane & 31;
        const int r = (rg * RB + rb) * 32 + jj;
        unsigned e[8];
        bool bad = false;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int k = 16 * s + 8 * hi + c;
            const float hv = (r < B && k < H) ? h[(size_t)r * H + k] : 0.0f;
            bad = bad || !(hv >= 0.0f && hv <= 1.0f);
            e[c] = dae_bf16_rne(hv);
        }
        if (row_bad && bad) row_bad[r] = 1;
        hp[o] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
}

template <int DT>
int launch_prepack_tiles(dae_ctx* ctx, const float* W, const float* b, int H, int Hp, int col_lo, int col_hi,
                         int ntiles, void* Wp, float* bias, uint4* bias16)
{
    if (ntiles <= 0) return DAE_OK;
    const size_t lds = (size_t)32 * (Hp + PP_PAD) * sizeof(float);
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &prepack_tile_kernel<DT>, 160 * 1024));
    const int blocks = ntiles < 8 * DAE_NUM_CU ? ntiles : 8 * DAE_NUM_CU;
    hipLaunchKernelGGL(prepack_tile_kernel<DT>, dim3(blocks), dim3(256), lds, ctx->stream, W, b, H, Hp, col_lo, col_hi,
                       ntiles, Wp, bias, bias16);
    DAE_CHECK_LAUNCH(ctx, "prepack_tile_kernel");
    return DAE_OK;
}
}  // namespace

int dae_launch_prepack_bf16(dae_ctx* ctx, const float* W, const float* b, int V, int H,
                            int col_lo, int col_hi, int exact)
{
    dae_packed& pk = ctx->pk_bf16;
    pk.valid = false; pk.order_nrank = -1; pk.exact = false;
    if (exact && (H & 3)) return dae_fail(ctx, DAE_ERR_ARG, "DAE_DTYPE_BF16_EXACT needs H %% 4 == 0 (H=%d)", H);
    const int Hp = dae_round_up(H, DAE_HPAD);
    if ((size_t)32 * Hp * 2 > 128 * 1024)
        return dae_fail(ctx, DAE_ERR_ARG, "hidden size %d too large", H);
    const int ntiles = (col_hi - col_lo + DAE_VT - 1) / DAE_VT;
    const int NS = Hp / 16;
    int rc = dae_reserve(ctx, pk.W, (size_t)ntiles * NS * 64 * sizeof(uint4));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.bias, (size_t)ntiles * 32 * sizeof(float));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.bias16, (size_t)ntiles * 64 * sizeof(uint4));
    if (rc) return rc;
    rc = launch_prepack_tiles<DT_BF16>(ctx, W, b, H, Hp, col_lo, col_hi, ntiles, pk.W.p,
                                       static_cast<float*>(pk.bias.p), static_cast<uint4*>(pk.bias16.p));
    if (rc) return rc;
    pk.V = V; pk.H = H; pk.Hp = Hp; pk.col_lo = col_lo; pk.col_hi = col_hi; pk.ntiles = ntiles;
    rc = dae_reserve(ctx, pk.ident, (size_t)(ntiles > 0 ? ntiles : 1) * sizeof(int));
    if (rc) return rc;
    rc = dae_launch_tile_iota(ctx, static_cast<int*>(pk.ident.p), ntiles);
    if (rc) return rc;
    if (exact) {
        rc = dae_reserve(ctx, pk.eps, ((size_t)ntiles * 32 + 1) * sizeof(float));
        if (rc) return rc;
        DAE_HIP_CHECK(ctx, hipMemsetAsync(static_cast<float*>(pk.eps.p) + (size_t)ntiles * 32, 0, sizeof(float), ctx->stream));
        rc = dae_reserve(ctx, pk.bias16_lo, (size_t)ntiles * 64 * sizeof(uint4));
        if (rc) return rc;
        rc = dae_reserve(ctx, pk.bias16_hi, (size_t)ntiles * 64 * sizeof(uint4));
        if (rc) return rc;
        const size_t wbytes = (size_t)(col_hi - col_lo) * H * sizeof(float);
        rc = dae_reserve(ctx, pk.W32, wbytes);
        if (rc) return rc;
        const int blocks = ntiles < 8 * DAE_NUM_CU ? ntiles : 8 * DAE_NUM_CU;
        hipLaunchKernelGGL(exact_bounds_kernel, dim3(blocks), dim3(256), 0, ctx->stream, W, b, H, Hp, col_lo, col_hi,
                           ntiles, static_cast<float*>(pk.eps.p), static_cast<uint4*>(pk.bias16_lo.p),
                           static_cast<uint4*>(pk.bias16_hi.p), ctx->exact_margin, ctx->margin_lo, ctx->margin_hi, ctx->margin_scale);
        DAE_CHECK_LAUNCH(ctx, "exact_bounds_kernel");
        DAE_HIP_CHECK(ctx, hipMemcpyAsync(pk.W32.p, W + (size_t)col_lo * H, wbytes, hipMemcpyDeviceToDevice, ctx->stream));
        // the same image read as the title side of the exact title mix: row-scaled bounds (mixexact.hip)
        rc = dae_launch_mix_title_bounds(ctx, W, b, H, Hp, col_lo, col_hi, ntiles, pk);
        if (rc) return rc;
        pk.exact = true;
    }
    pk.valid = true;
    return DAE_OK;
}

int dae_launch_pack_h_bf16(dae_ctx* ctx, const float* h, int B, int H, const dae_rowgeom& g, int* row_bad)
{
    const int Hp = dae_round_up(H, DAE_HPAD);
    const int NS = Hp / 16, RB = g.R_TILE / 32;
    const size_t total = (size_t)g.n_rg * NS * RB * 64;
    int rc = dae_reserve(ctx, ctx->h_packed16, total * sizeof(uint4));
    if (rc) return rc;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (row_bad) DAE_HIP_CHECK(ctx, hipMemsetAsync(row_bad, 0, (size_t)g.Bpad * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(pack_h_bf16_kernel, dim3(blocks), dim3(256), 0, ctx->stream, h, B, H, NS, RB,
                       g.n_rg, static_cast<uint4*>(ctx->h_packed16.p), row_bad);
    DAE_CHECK_LAUNCH(ctx, "pack_h_bf16_kernel");
    ctx->h16_geom_key = ((long long)B << 32) | ((long long)H << 12) | (long long)g.R_TILE;   // whole image rewritten, pads zero
    ctx->h16_geom_ptr = ctx->h_packed16.p;
    return DAE_OK;
}

int dae_launch_prepack_f32(dae_ctx* ctx, const float* W, const float* b, int V, int H,
                           int col_lo, int col_hi)
{
    dae_packed& pk = ctx->pk_f32;
    pk.valid = false; pk.order_nrank = -1;
    const int Hp = dae_round_up(H, DAE_HPAD);
    if ((size_t)32 * Hp * 4 > 128 * 1024)
        return dae_fail(ctx, DAE_ERR_ARG, "hidden size %d too large (max 1024)", H);
    const int ntiles = (col_hi - col_lo + DAE_VT - 1) / DAE_VT;
    const int G = Hp / DAE_KG;
    int rc = dae_reserve(ctx, pk.W, (size_t)ntiles * G * 64 * sizeof(float4));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.bias, (size_t)ntiles * 32 * sizeof(float));
    if (rc) return rc;
    rc = launch_prepack_tiles<DT_F32>(ctx, W, b, H, Hp, col_lo, col_hi, ntiles, pk.W.p,
                                      static_cast<float*>(pk.bias.p), nullptr);
    if (rc) return rc;
    pk.V = V; pk.H = H; pk.Hp = Hp; pk.col_lo = col_lo; pk.col_hi = col_hi; pk.ntiles = ntiles;
    rc = dae_reserve(ctx, pk.ident, (size_t)(ntiles > 0 ? ntiles : 1) * sizeof(int));
    if (rc) return rc;
    rc = dae_launch_tile_iota(ctx, static_cast<int*>(pk.ident.p), ntiles);
    if (rc) return rc;
    pk.valid = true;
    return DAE_OK;
}

int dae_launch_tile_iota(dae_ctx* ctx, int* dst, int ntiles)
{
    hipLaunchKernelGGL(tile_iota_kernel, dim3((ntiles + 255) / 256 > 0 ? (ntiles + 255) / 256 : 1), dim3(256), 0,
                       ctx->stream, ntiles, dst);
    DAE_CHECK_LAUNCH(ctx, "tile_iota_kernel");
    return DAE_OK;
}

int dae_launch_tile_order(dae_ctx* ctx, dae_packed& pk, int nrank, int n_samp, int S)
{
    if (pk.order_nrank == nrank && pk.order_nsamp == n_samp && pk.order.p) return DAE_OK;
    // the list holds the tiles with a rankable column -- a prefix of the image's -- and its length picks the kernel: a wide
    // image whose ranked part fits the sort still gets the bias order
    int n_rt = (nrank + 31) / 32;
    if (n_rt > pk.ntiles) n_rt = pk.ntiles;
    int rc = dae_reserve(ctx, pk.order, (size_t)(n_rt > 0 ? n_rt : 1) * sizeof(int));
    if (rc) return rc;
    if (n_rt <= 0) {
        // (no list to build)
    } else if (!dae_tile_order_sorted(n_rt)) {
        hipLaunchKernelGGL(tile_order_strided_kernel, dim3((n_rt + 255) / 256), dim3(256), 0, ctx->stream,
                           n_rt, n_samp, S, static_cast<int*>(pk.order.p));
    } else {
        hipLaunchKernelGGL(tile_order_kernel, dim3(1), dim3(1024), 0, ctx->stream,
                           static_cast<const float*>(pk.bias.p), n_rt, nrank, static_cast<int*>(pk.order.p));
    }
    DAE_CHECK_LAUNCH(ctx, "tile_order_kernel");
    pk.order_nrank = nrank; pk.order_nsamp = n_samp;
    static std::atomic<long long> gen{0};
    pk.order_gen = ++gen;
    return DAE_OK;
}

// does a list of n_rank_tiles take the bias sort (whose order does not depend on the sample size)?
bool dae_tile_order_sorted(int n_rank_tiles) { return n_rank_tiles <= ORDER_MAX_TILES; }

int dae_launch_tile_band(dae_ctx* ctx, const int* order, int ntiles, int n_samp, int nb_rg, int waves, int* band)
{
    if (ntiles <= 0) return DAE_OK;
    hipLaunchKernelGGL(tile_band_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, ctx->stream, order, ntiles, n_samp, nb_rg,
                       waves, band);
    DAE_CHECK_LAUNCH(ctx, "tile_band_kernel");
    return DAE_OK;
}

int dae_launch_pack_h(dae_ctx* ctx, const float* h, int B, int H, const dae_rowgeom& g)
{
    const int Hp = dae_round_up(H, DAE_HPAD);
    const int G = Hp / DAE_KG, RB = g.R_TILE / 32;
    const size_t total = (size_t)g.n_rg * G * RB * 64;
    int rc = dae_reserve(ctx, ctx->h_packed, total * sizeof(float4));
    if (rc) return rc;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(pack_h_kernel, dim3(blocks), dim3(256), 0, ctx->stream, h, B, H, G, RB,
                       g.n_rg, static_cast<float4*>(ctx->h_packed.p));
    DAE_CHECK_LAUNCH(ctx, "pack_h_kernel");
    return DAE_OK;
}
