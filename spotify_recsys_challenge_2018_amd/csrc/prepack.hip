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
                                                           uint4* __restrict__ bias16,
                                                           float* __restrict__ tile_ub)
{
    extern __shared__ __attribute__((aligned(16))) float pp_tile[];      // [32][Hp + PP_PAD] | 4 x 2 floats
    const int tid = threadIdx.x;
    const int ldt = Hp + PP_PAD;
    float (*const ub_wave)[2] = reinterpret_cast<float (*)[2]>(pp_tile + 32 * ldt);     // (fp32 image) the waves' maxima of a_c, m_c
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
        if (DT == DT_F32 && tile_ub) {
            // ---- the tile's logit bound (the filter launch of hidden 256 skips tiles by it: live_tiles_kernel below) ----------
            // z32(r, c) = the canonical chain acc = fmaf(h[k], W[c][k], acc) over k < H, + b[c]  (oracle orc_decode): H + 1
            // roundings, so |z32 - z| <= rho (sum_k |h_k W_ck| + |b_c|) with z = b_c + sum_k h_k W_ck in real numbers and
            // rho = (H + 2) 2^-24 (1 + 2^-10), the recursive-summation bound exact_bounds_kernel uses for the same chain, plus
            // (H + 2) 2^-125 in absolute terms for results that underflow (flushed or gradual).  For a hidden row with
            // |h_k - 0.5| <= d for all k, and s = sum_k W_ck, n = sum_k |W_ck|:
            //     z <= b + 0.5 s + d n,     sum_k |h_k W_ck| <= (0.5 + d) n,     hence     z32(r, c) <= a_c + d m_c,
            //     a_c = b + 0.5 s + rho (0.5 n + |b|) + (H + 2) 2^-125,     m_c = (1 + rho) n.
            // s and n are summed in double (H terms: off by <= H 2^-53 n, covered by 2^-40 (n + |b|) and the factor 1 + 2^-40)
            // and a_c, m_c rounded UP to float.  The tile keeps A_t = max_c a_c, M_t = max_c m_c over its columns inside the image
            // (n_tracks is a call-time argument: a superset of the ranked columns is still a bound).  A NaN stays a NaN: the
            // comparison that skips a tile is written so that a NaN keeps it.
            const int c = tid >> 3, part = tid & 7;
            const float* wrow = pp_tile + c * ldt;
            double sw = 0.0, nw = 0.0;
            for (int k = part; k < H; k += 8) { const double w = (double)wrow[k]; sw += w; nw += fabs(w); }
#pragma unroll
            for (int sh = 1; sh < 8; sh <<= 1) { sw += __shfl_xor(sw, sh); nw += __shfl_xor(nw, sh); }
            // The LOWER bound of the same chain (what the threshold sample skips tiles by: sample_bound_kernel below, DESIGN.md
            // section 2): z >= b + 0.5 s - d n and |z32 - z| <= rho (0.5 + d) n + rho |b| + (H + 2) 2^-125 give
            //     z32(r, c) >= lo_c - d m_c,     lo_c = b + 0.5 s - rho (0.5 n + |b|) - (H + 2) 2^-125,
            // with the SAME m_c; the double sums' own error comes off as 2^-40 (n + |b|), and lo_c is rounded DOWN to float.
            float a_f = -__builtin_inff(), m_f = 0.0f, lo_f = -__builtin_inff();      // a column past the image bounds nothing
            if (v0 + c < col_hi) {
                const double bv = (double)b[v0 + c], ab = fabs(bv);
                const double rho = (double)(H + 2) * 0x1p-24 * (1.0 + 0x1p-10);
                const double a = bv + 0.5 * sw + rho * (0.5 * nw + ab) + (double)(H + 2) * 0x1p-125 + 0x1p-40 * (nw + ab);
                const double m = (1.0 + rho) * nw * (1.0 + 0x1p-40);
                a_f = (float)a; if ((double)a_f < a) a_f = nextafterf(a_f, __builtin_inff());
                m_f = (float)m; if ((double)m_f < m) m_f = nextafterf(m_f, __builtin_inff());
                const double lo = bv + 0.5 * sw - rho * (0.5 * nw + ab) - (double)(H + 2) * 0x1p-125 - 0x1p-40 * (nw + ab);
                lo_f = (float)lo; if ((double)lo_f > lo) lo_f = nextafterf(lo_f, -__builtin_inff());
            }
            // (the columns' own pairs behind the tiles': the tile that holds the LAST ranked column of a call is bounded over its
            // ranked columns alone -- live_tiles_kernel -- since its other columns, the first artists, carry the largest biases)
            if (part == 0) {
                tile_ub[2 * (ntiles + t * 32 + c)] = a_f; tile_ub[2 * (ntiles + t * 32 + c) + 1] = m_f;
                tile_ub[(size_t)66 * ntiles + t * 32 + c] = lo_f;
            }
#pragma unroll
            for (int sh = 8; sh < 64; sh <<= 1) {
                a_f = dae_max_nan(a_f, __shfl_xor(a_f, sh));
                m_f = dae_max_nan(m_f, __shfl_xor(m_f, sh));
            }
            if ((tid & 63) == 0) { ub_wave[tid >> 6][0] = a_f; ub_wave[tid >> 6][1] = m_f; }
        }
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
        // (the next tile's maxima are written behind the next barrier, which this thread reaches after these reads)
        if (DT == DT_F32 && tile_ub && tid < 2)
            tile_ub[2 * t + tid] = dae_max_nan(dae_max_nan(ub_wave[0][tid], ub_wave[1][tid]), dae_max_nan(ub_wave[2][tid], ub_wave[3][tid]));
    }
}

// ---- the live lists of the fp32 filter launch (score.hip topk_phase_b; hidden 256 in 128-row groups) ---------------------
// The STANDALONE builder.  A call whose filter launch takes the thresholds its own threshold launch computed gets the lists
// from that launch (tau_select.hip tau_select_kernel<.., LIVE>: dae_score_plan::live_in_tau) and never runs this kernel; it runs
// where the thresholds come from elsewhere (dae_score_topk_finish: exchanged, possibly raised) or the threshold launch is the
// wave-per-row kernel.  Both builders apply ONE test, dae_tile_is_live (decode_common.h), to the same d_max and tau_min, so the
// lists of the two are the same for the same thresholds.
// One workgroup per row group rg.  From the group's packed hidden tile: d_max = max |h[r][k] - 0.5| over its rows r < B and the
// units k < H (the zero padding of the tile is NOT read: it would give 0.5); from the thresholds the filter launch is given:
// tau_min = min over the same rows.  Item i of `list` is live unless U = A_t + d M_t < tau_min (prepack_tile_kernel's bound:
// no column of tile t then reaches the threshold of any row of the group, i.e. the filter epilogue would drop all of it).
// The live tiles go to live_list[rg * n_items ..) in the list's order, their number to live_cnt[rg].
// stat: {launches, planned tiles x row groups, live tiles} of the context (dae_filter_skip_read).
__global__ __launch_bounds__(1024) void live_tiles_kernel(const float4* __restrict__ hp, int B, int H, int G,
                                                          const float* __restrict__ tau, const float* __restrict__ tile_ub,
                                                          int ntiles, int nrank, const int* __restrict__ list, int n_items,
                                                          int* __restrict__ live_cnt, int* __restrict__ live_list,
                                                          unsigned long long* __restrict__ stat)
{
    constexpr int RB = 4, R_TILE = 128, NW = 16;
    __shared__ double sh_d[NW];
    __shared__ float sh_t[NW];
    __shared__ int sh_n[NW];
    const int rg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // hidden tile of the group: float4 index (g * RB + rb) * 64 + l holds h[rg * 128 + rb * 32 + (l & 31)][8 g + 2 e + (l >> 5)]
    double d = 0.0;
    const float4* src = hp + (size_t)rg * G * RB * 64;
    for (int o = tid; o < G * RB * 64; o += 1024) {
        const int l = o & 63, rb = (o >> 6) % RB, g = (o >> 6) / RB;
        if ((rg * RB + rb) * 32 + (l & 31) >= B) continue;
        const float4 v = src[o];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (8 * g + 2 * c + (l >> 5) < H) d = dae_max_nan(d, fabs((double)e[c] - 0.5));
    }
    // the tile that holds the last ranked column (nrank is no multiple of 32): its bound over the ranked columns only
    __shared__ float sh_edge[2];
    const int t_edge = (nrank & 31) ? (nrank >> 5) : -1;
    if (wave == 0 && t_edge >= 0) {
        float ea, em;
        dae_edge_tile_bound(tile_ub, ntiles, nrank, lane, ea, em);
        if (lane == 0) { sh_edge[0] = ea; sh_edge[1] = em; }
    }
    float tm = __builtin_inff();
    if (tid < R_TILE && rg * R_TILE + tid < B) tm = tau[rg * R_TILE + tid];
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        d = dae_max_nan(d, __shfl_xor(d, sh));
        tm = dae_min_nan(tm, __shfl_xor(tm, sh));
    }
    if (lane == 0) { sh_d[wave] = d; sh_t[wave] = tm; }
    __syncthreads();
    for (int w = 0; w < NW; ++w) { d = dae_max_nan(d, sh_d[w]); tm = dae_min_nan(tm, sh_t[w]); }

    int done = 0;
    int* const out = live_list + (size_t)rg * n_items;
    for (int i0 = 0; i0 < n_items; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false;
        int t = 0;
        if (i < n_items) {
            t = list[i];
            keep = dae_tile_is_live(t == t_edge ? sh_edge[0] : tile_ub[2 * t], t == t_edge ? sh_edge[1] : tile_ub[2 * t + 1], d, tm);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) sh_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < NW; ++w) { before += w < wave ? sh_n[w] : 0; all += sh_n[w]; }
        if (keep) out[done + before + __popcll(mask & ((1ull << lane) - 1ull))] = t;
        done += all;
        __syncthreads();
    }
    if (tid == 0) {
        live_cnt[rg] = done;
        if (rg == 0) atomicAdd(&stat[0], 1ull);
        atomicAdd(&stat[1], (unsigned long long)n_items);
        atomicAdd(&stat[2], (unsigned long long)done);
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

// ---- the bound table of the threshold sample (score.hip topk_phase_a; decode_generic.hip decode_f32_kernel's HALF) ------------
// Built once per (tile order, sample geometry).  The sample launch in half row groups decodes item w * nb_rg + bir in wave w of
// workgroup bir and takes, per position c of the tile, the maximum over the workgroup's waves: group (bir, c).
//   ub_out[i]   = {A_t, M_t} of item i's tile, in list order (the edge tile bounded over its ranked columns);
//   beta_out[j] = the j-th largest of beta_g = max lo_c over the RANKED columns of group g (-inf: a group without one), for the
//                 leading n_beta of the nb_rg * 32 groups;
//   head[0]     = mu_max = max M_t over the items -- a NaN if any lo_c or M_t is one, which keeps every tile (the bound says
//                 nothing about an image that holds a NaN).
// One workgroup; the sort is tile_order_kernel's network on 32-bit keys.
constexpr int BOUND_MAX_GROUPS = 8192;              // nb_rg <= DAE_NUM_CU workgroups x 32 positions
__global__ __launch_bounds__(1024) void sample_bound_kernel(const int* __restrict__ list, int n_items, int nb_rg, int waves,
                                                            const float* __restrict__ tile_ub, int ntiles, int nrank,
                                                            float* __restrict__ head, float2* __restrict__ ub_out,
                                                            float* __restrict__ beta_out, int n_beta)
{
    __shared__ unsigned keys[BOUND_MAX_GROUPS];
    __shared__ float sh_edge[2], sh_mu[16];
    __shared__ int sh_nan;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* const lo = tile_ub + (size_t)66 * ntiles;
    const int t_edge = (nrank & 31) ? (nrank >> 5) : -1;
    if (tid == 0) sh_nan = 0;
    if (wave == 0 && t_edge >= 0) {
        float ea, em;
        dae_edge_tile_bound(tile_ub, ntiles, nrank, lane, ea, em);
        if (lane == 0) { sh_edge[0] = ea; sh_edge[1] = em; }
    }
    __syncthreads();
    float mu = 0.0f;
    for (int i = tid; i < n_items; i += 1024) {
        const int t = list[i];
        const float2 ub = t == t_edge ? make_float2(sh_edge[0], sh_edge[1]) : make_float2(tile_ub[2 * t], tile_ub[2 * t + 1]);
        ub_out[i] = ub;
        mu = dae_max_nan(mu, ub.y);
    }
    const int n_groups = nb_rg * 32;
    int n2 = 1024;
    while (n2 < n_groups) n2 <<= 1;
    bool nan = false;
    for (int gi = tid; gi < n2; gi += 1024) {
        unsigned key = 0u;                                  // padding sorts last (below the key of -inf)
        if (gi < n_groups) {
            const int bir = gi >> 5, c = gi & 31;
            float b = -__builtin_inff();
            for (int w = 0; w < waves; ++w) {
                const int item = w * nb_rg + bir;
                if (item >= n_items) continue;
                const int col = list[item] * 32 + c;
                if (col < nrank) b = dae_max_nan(b, lo[col]);
            }
            nan = nan || b != b;
            key = b != b ? 0xFFFFFFFFu : dae_okey(b);
        }
        keys[gi] = key;
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) mu = dae_max_nan(mu, __shfl_xor(mu, sh));
    if (lane == 0) sh_mu[wave] = mu;
    if (nan) sh_nan = 1;
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2; i += 1024) {
                const int jx = i ^ stride;
                if (jx > i) {
                    const unsigned a = keys[i], b = keys[jx];
                    const bool desc = (i & size) == 0;
                    if (desc ? (a < b) : (a > b)) { keys[i] = b; keys[jx] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < n_beta; i += 1024) beta_out[i] = dae_okey_inv(keys[i]);
    if (tid == 0) {
        float m = sh_mu[0];
        for (int w = 1; w < 16; ++w) m = dae_max_nan(m, sh_mu[w]);
        head[0] = sh_nan ? __builtin_nanf("") : m;
    }
}

// THE ENVELOPE OF THE FILTER LIST (empty_proof.h), behind the bound table and rebuilt with it: workgroup j
// takes env[j] = the maximum over the filter launch's items of U_t(d_j), the value dae_tile_is_live compares with tau_min, in
// double, rounded UP to float; the edge tile by its ranked columns' pair.  A NaN pair or M_t < 0 anywhere: env[j] = NaN.
__global__ __launch_bounds__(256) void filter_envelope_kernel(const int* __restrict__ list, int n_items,
                                                              const float* __restrict__ tile_ub, int ntiles, int nrank,
                                                              float* __restrict__ env)
{
    __shared__ float sh_edge[2];
    __shared__ double sh_u[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x;
    const int t_edge = (nrank & 31) ? (nrank >> 5) : -1;
    if (wave == 0 && t_edge >= 0) {
        float ea, em;
        dae_edge_tile_bound(tile_ub, ntiles, nrank, lane, ea, em);
        if (lane == 0) { sh_edge[0] = ea; sh_edge[1] = em; }
    }
    __syncthreads();
    double u = -__builtin_inf();
    for (int i = tid; i < n_items; i += 256) {
        const int t = list[i];
        const float a = t == t_edge ? sh_edge[0] : tile_ub[2 * t], m = t == t_edge ? sh_edge[1] : tile_ub[2 * t + 1];
        u = dae_max_nan(u, dae_proof_item(a, m, j));
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) u = dae_max_nan(u, __shfl_xor(u, sh));
    if (lane == 0) sh_u[wave] = u;
    __syncthreads();
    if (tid == 0) env[j] = dae_proof_float_up(dae_max_nan(dae_max_nan(sh_u[0], sh_u[1]), dae_max_nan(sh_u[2], sh_u[3])));
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

// The same image for a ranking call (score.hip pack_hidden), which also wants the rows' d: one workgroup per (row group, row
// block, quarter of the k groups); wave w takes the quarter's groups w, w + 4, ...
// d_out: [Bpad][4] floats, d_out[r * 4 + q] = max |h[r][k] - 0.5| over the quarter's units k < H of the real row r, in double,
// rounded UP, a NaN if an entry is one (what the threshold sample's skip takes the row's d from, as from the encode kernels:
// decode_generic.hip).  The zero padding takes no part: it would read 0.5.
__global__ __launch_bounds__(256) void pack_h_d_kernel(const float* __restrict__ h, int B, int H,
                                                       int G, int RB, int n_rg,
                                                       float4* __restrict__ hp, float* __restrict__ d_out)
{
    __shared__ double sh_d[4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x & 3, rb = (blockIdx.x >> 2) % RB, rg = (blockIdx.x >> 2) / RB;
    const int hi = lane >> 5, jj = lane & 31;
    const int r = (rg * RB + rb) * 32 + jj;
    const int Gq = G >> 2;                                   // (Hp is a multiple of DAE_HPAD = 32: G of 4)
    double d = 0.0;
    for (int g = q * Gq + wave; g < (q + 1) * Gq; g += 4) {
        float e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int k = 8 * g + 2 * c + hi;
            const bool in = r < B && k < H;
            e[c] = in ? h[(size_t)r * H + k] : 0.0f;
            if (in) d = dae_max_nan(d, fabs((double)e[c] - 0.5));
        }
        hp[(((size_t)rg * G + g) * RB + rb) * 64 + lane] = make_float4(e[0], e[1], e[2], e[3]);
    }
    d = dae_max_nan(d, __shfl_xor(d, 32));
    if (hi == 0) sh_d[wave][jj] = d;
    __syncthreads();
    if (threadIdx.x < 32 && r < B) {
        d = dae_max_nan(dae_max_nan(sh_d[0][jj], sh_d[1][jj]), dae_max_nan(sh_d[2][jj], sh_d[3][jj]));
        float df = (float)d;
        if ((double)df < d) df = nextafterf(df, __builtin_inff());
        d_out[(size_t)r * 4 + q] = df;
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
                         int ntiles, void* Wp, float* bias, uint4* bias16, float* tile_ub = nullptr)
{
    if (ntiles <= 0) return DAE_OK;
    const size_t lds = ((size_t)32 * (Hp + PP_PAD) + 8) * sizeof(float);
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &prepack_tile_kernel<DT>, 160 * 1024));
    const int blocks = ntiles < 8 * DAE_NUM_CU ? ntiles : 8 * DAE_NUM_CU;
    hipLaunchKernelGGL(prepack_tile_kernel<DT>, dim3(blocks), dim3(256), lds, ctx->stream, W, b, H, Hp, col_lo, col_hi,
                       ntiles, Wp, bias, bias16, tile_ub);
    DAE_CHECK_LAUNCH(ctx, "prepack_tile_kernel");
    return DAE_OK;
}
}  // namespace

int dae_launch_prepack_bf16(dae_ctx* ctx, const float* W, const float* b, int V, int H,
                            int col_lo, int col_hi, int exact)
{
    dae_packed& pk = ctx->pk_bf16;
    pk.valid = false; pk.order_nrank = -1; pk.exact = false; pk.cat_id = 0;
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
        // the same image read as the title side of the exact title mix: row-scaled bounds (mix_prep.hip)
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
                           int col_lo, int col_hi, bool bounds)
{
    dae_packed& pk = ctx->pk_f32;
    pk.valid = false; pk.order_nrank = -1; pk.ub_valid = false; pk.cat_id = 0;
    const int Hp = dae_round_up(H, DAE_HPAD);
    if ((size_t)32 * Hp * 4 > 128 * 1024)
        return dae_fail(ctx, DAE_ERR_ARG, "hidden size %d too large (max 1024)", H);
    const int ntiles = (col_hi - col_lo + DAE_VT - 1) / DAE_VT;
    const int G = Hp / DAE_KG;
    int rc = dae_reserve(ctx, pk.W, (size_t)ntiles * G * 64 * sizeof(float4));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.bias, (size_t)ntiles * 32 * sizeof(float));
    if (rc) return rc;
    if (bounds) {
        rc = dae_reserve(ctx, pk.tile_ub, (size_t)(ntiles > 0 ? ntiles : 1) * (33 * 2 + 32) * sizeof(float));      // [ntiles][2] | [ntiles * 32][2] | [ntiles * 32]
        if (rc) return rc;
    }
    rc = launch_prepack_tiles<DT_F32>(ctx, W, b, H, Hp, col_lo, col_hi, ntiles, pk.W.p,
                                      static_cast<float*>(pk.bias.p), nullptr, bounds ? static_cast<float*>(pk.tile_ub.p) : nullptr);
    if (rc) return rc;
    pk.V = V; pk.H = H; pk.Hp = Hp; pk.col_lo = col_lo; pk.col_hi = col_hi; pk.ntiles = ntiles;
    rc = dae_reserve(ctx, pk.ident, (size_t)(ntiles > 0 ? ntiles : 1) * sizeof(int));
    if (rc) return rc;
    rc = dae_launch_tile_iota(ctx, static_cast<int*>(pk.ident.p), ntiles);
    if (rc) return rc;
    pk.valid = true; pk.ub_valid = bounds;
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

int dae_launch_live_tiles(dae_ctx* ctx, const dae_packed& pk, const dae_rowgeom& g, int B, const int* list, int n_items,
                          const float* tau, int nrank, int* live_cnt, int* live_list, unsigned long long* stat)
{
    if (g.R_TILE != 128 || !pk.ub_valid || !pk.tile_ub.p || !ctx->h_packed.p || n_items <= 0)
        return dae_fail(ctx, DAE_ERR_STATE, "live tile lists: fp32 image with tile bounds, 128-row groups");
    hipLaunchKernelGGL(live_tiles_kernel, dim3(g.n_rg), dim3(1024), 0, ctx->stream, static_cast<const float4*>(ctx->h_packed.p),
                       B, pk.H, pk.Hp / DAE_KG, tau, static_cast<const float*>(pk.tile_ub.p), pk.ntiles, nrank, list, n_items, live_cnt, live_list,
                       stat);
    DAE_CHECK_LAUNCH(ctx, "live_tiles_kernel");
    return DAE_OK;
}

int dae_launch_pack_h(dae_ctx* ctx, const float* h, int B, int H, const dae_rowgeom& g, float* d_out)
{
    const int Hp = dae_round_up(H, DAE_HPAD);
    const int G = Hp / DAE_KG, RB = g.R_TILE / 32;
    const size_t total = (size_t)g.n_rg * G * RB * 64;
    int rc = dae_reserve(ctx, ctx->h_packed, total * sizeof(float4));
    if (rc) return rc;
    if (d_out) {
        hipLaunchKernelGGL(pack_h_d_kernel, dim3(g.n_rg * RB * 4), dim3(256), 0, ctx->stream, h, B, H, G, RB,
                           g.n_rg, static_cast<float4*>(ctx->h_packed.p), d_out);
    } else {
        int blocks = (int)((total + 255) / 256);
        if (blocks > 2048) blocks = 2048;
        hipLaunchKernelGGL(pack_h_kernel, dim3(blocks), dim3(256), 0, ctx->stream, h, B, H, G, RB,
                           g.n_rg, static_cast<float4*>(ctx->h_packed.p));
    }
    DAE_CHECK_LAUNCH(ctx, d_out ? "pack_h_d_kernel" : "pack_h_kernel");
    return DAE_OK;
}

int dae_launch_sample_bounds(dae_ctx* ctx, const dae_packed& pk, const int* list, int n_items, int nb_rg, int waves, int nrank,
                             float* head, float2* ub_out, float* beta_out, int n_beta, int n_filter, float* env_out)
{
    if (!pk.ub_valid || !pk.tile_ub.p || n_items <= 0 || nb_rg * 32 > BOUND_MAX_GROUPS || n_beta > nb_rg * 32 || n_filter < 0)
        return dae_fail(ctx, DAE_ERR_STATE, "sample bound table: fp32 image with bounds, at most %d groups", BOUND_MAX_GROUPS);
    hipLaunchKernelGGL(sample_bound_kernel, dim3(1), dim3(1024), 0, ctx->stream, list, n_items, nb_rg, waves,
                       static_cast<const float*>(pk.tile_ub.p), pk.ntiles, nrank, head, ub_out, beta_out, n_beta);
    DAE_CHECK_LAUNCH(ctx, "sample_bound_kernel");
    // (the filter launch's items follow the sample's in the order)
    hipLaunchKernelGGL(filter_envelope_kernel, dim3(DAE_PROOF_ENV), dim3(256), 0, ctx->stream, list + n_items, n_filter,
                       static_cast<const float*>(pk.tile_ub.p), pk.ntiles, nrank, env_out);
    DAE_CHECK_LAUNCH(ctx, "filter_envelope_kernel");
    return DAE_OK;
}
