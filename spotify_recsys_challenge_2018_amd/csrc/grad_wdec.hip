// grad_wdec.hip -- K6 of the training step: the decoder gradient gW_dec = dz^T h (+ gb_dec = the column sums of dz), or, armed
// (dae_arm_decoder_adam), the dense Adam update of W_dec from that gradient without writing it.  Four kernels by operand type
// and orientation, one launcher (dae_launch_k6, at the end) that holds the whole choice between them.
#include "train_common.h"

namespace {

// ---- K6: gW[v, hc] = sum_r dz[r, v] * h[r, hc];  gb[v] = sum_r dz[r, v] ----------------------
// block = 4 waves sharing the LDS image of h[:, hc0 : hc0+128] (K = B <= 256 rows); a wave owns
// tiles of 64 vocabulary columns (2 MFMA tiles, v = v0 + 2 j + b) x 128 hidden units (4 tiles).
struct GwP {
    const float* dzT; int64_t ldT;    // [V, ldT] (dz transposed, rows zero padded to ldT)
    const float* h; int H, B, V;
    float* gW;                        // [V, H]
    float* gb;                        // [V] (written by the hc0 == 0 blocks) or null
    // the ACC instances (a later 256-row panel of a longer batch, train.hip): the [V, H] gradient of the earlier panels, which the
    // tile is added to (partial + tile, element by element) -- gW itself for the unarmed kernels, the context's scratch for the
    // armed ones, which feed the sum to Adam; gb[v] then holds the earlier panels' column sums and has this panel's added
    const float* gprev;
    int n_half, nb_half;              // H / 128 hidden halves, blocks per half
    // dense TF1-Adam of the [V, H] tensor `ad.p` applied in the epilogue instead of writing gW (dae_arm_decoder_adam); read by
    // the kernels that can be armed only: grad_wdec_kernel<4, 8, true> and the two t32 kernels
    dae_armed_adam ad;
};

// which part of the work a workgroup has: blocks q * gs .. (q + 1) * gs - 1 are one block per (hidden half, XCD), so the
// DAE_NUM_XCD blocks that share a half's h columns are dealt to different XCDs.  hw = hidden units per half.
struct K6Block { int half, bir, hc0, Bp; };   // hidden half, block index within the half, its first hidden unit, rows padded to 32
__device__ __forceinline__ K6Block k6_block(const GwP& p, int hw)
{
    const int gs = DAE_NUM_XCD * p.n_half;
    const int q = blockIdx.x / gs, rem = blockIdx.x % gs;
    K6Block b;
    b.half = rem / DAE_NUM_XCD;
    b.bir = q * DAE_NUM_XCD + (rem % DAE_NUM_XCD);
    b.hc0 = b.half * hw;
    b.Bp = (p.B + 31) & ~31;           // rows padded to whole 32-row groups (zero rows)
    return b;
}

// LDS image of h^T for the transposed bf16 kernels: B fragment (s, a, lane (n, hi)) = bf16 of h[16 s + 8 hi + x][hc0 + 4 n + a],
// x = 0..7; rows past B are zero.  S k-steps of 16 playlists, 4 KB each.
__device__ __forceinline__ void k6_fill_ht_bf16(uint4* ldsq, const GwP& p, int hc0, int S, int tid, int n_threads)
{
    for (int f = tid; f < S * 4 * 64; f += n_threads) {
        const int fl = f & 63, fa = (f >> 6) & 3, fs = f >> 8;
        const int r0 = 16 * fs + 8 * (fl >> 5);
        const float* src = p.h + hc0 + 4 * (fl & 31) + fa;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = r0 + e < p.B ? src[(size_t)(r0 + e) * p.H] : 0.0f;
        ldsq[f] = make_uint4(pk_bf16(x[0], x[1]), pk_bf16(x[2], x[3]), pk_bf16(x[4], x[5]), pk_bf16(x[6], x[7]));
    }
}

// The armed pass of the two t32 kernels over a tile of 32 decoder rows: register reg of lane (n, hi) is decoder row
// v0 + acc_row32(reg, hi), hidden hc0 + 4 n + a (a = the 4 accumulators).  Four groups of four rows through two buffers: group
// g + 1 is requested before group g is updated and stored; group 0 is requested by the kernel before its MFMAs.
// ACC: the earlier panels' gradient rows (p.gprev) travel with P / M / V -- requested a group ahead, like them.  A group's rows
// are added into its accumulators (partial + tile) before the next group is requested, so one buffer of them is enough.
template <bool ACC>
struct K6AdamRows {
    float4 P[2][4], M[2][4], V[2][4], G[ACC ? 4 : 1];
    size_t off[2][4];
    bool ok[2][4];
    __device__ __forceinline__ void issue(const GwP& p, int buf, int r4, int v0, int hi, int hcol)
    {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int v = v0 + acc_row32(r4 + u, hi);
            ok[buf][u] = v < p.V;
            off[buf][u] = (size_t)(ok[buf][u] ? v : 0) * p.H + hcol;
            P[buf][u] = nt_ld4(p.ad.p + off[buf][u]);
            M[buf][u] = nt_ld4(p.ad.m + off[buf][u]);
            V[buf][u] = nt_ld4(p.ad.v + off[buf][u]);
            if (ACC) G[ACC ? u : 0] = nt_ld4(p.gprev + off[buf][u]);
        }
    }
    __device__ __forceinline__ void pass(const GwP& p, f32x16 (&acc)[4], int v0, int hi, int hcol)
    {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int cb = g & 1;
            if (ACC) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 g0 = G[ACC ? u : 0];
                    const int reg = 4 * g + u;
                    acc[0][reg] = g0.x + acc[0][reg]; acc[1][reg] = g0.y + acc[1][reg];
                    acc[2][reg] = g0.z + acc[2][reg]; acc[3][reg] = g0.w + acc[3][reg];
                }
            }
            if (g + 1 < 4) issue(p, cb ^ 1, 4 * (g + 1), v0, hi, hcol);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int reg = 4 * g + u;
                float4 pp = P[cb][u], mm = M[cb][u], vv = V[cb][u];
                dae_adam_el4(pp, mm, vv, make_float4(acc[0][reg], acc[1][reg], acc[2][reg], acc[3][reg]), p.ad.alpha, p.ad.b1,
                             p.ad.b2, p.ad.eps);
                if (ok[cb][u]) {
                    nt_st4(p.ad.p + off[cb][u], pp);
                    nt_st4(p.ad.m + off[cb][u], mm);
                    nt_st4(p.ad.v + off[cb][u], vv);
                }
            }
        }
    }
};

// fp32 operands (the bf16 training step's K6 is grad_wdec_t_kernel / grad_wdec_t32_kernel below).
// NA = hidden tiles per wave (4, 2 or 1): a "half" is 32*NA hidden units, hidden = hc0 + NA*i + a
// TR (NA = 4): the two MFMA operands swapped -- D[i = vocabulary row of the lane pair][j = hidden lane] instead of
// D[i = hidden][j = vocabulary row].  Loads, LDS image and column sums are unchanged; what changes is that a lane of the
// accumulators is a hidden unit (hc0 + 4 j + a), so the epilogue writes 512 contiguous bytes of one gW row per half-wave
// instead of 16-byte pieces of 32 rows -- the same shape the transposed bf16 kernel (grad_wdec_t_kernel) has.
// ACC: the tile is added to the earlier panels' gradient at p.gprev (see GwP).  Each of the four kernels is a body with the ACC
// switch and two entry points: the kernel a batch of at most 256 rows has always launched, and its _acc twin for a later panel.
template <int NA, int NW, bool TR, bool ACC>
__device__ __forceinline__ void grad_wdec_body(const GwP& p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];     // [Bp][32*NA] floats
    constexpr int HW = 32 * NA;
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, j = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const K6Block wg = k6_block(p, HW);
    const int half = wg.half, bir = wg.bir, hc0 = wg.hc0, Bp = wg.Bp;

    // LDS image of h[:, hc0 : hc0 + HW]: 8 independent 16-byte loads in flight per thread.  (One 4-byte load ->
    // wait -> ds_write per iteration, 128 iterations per thread, was ~80 us of this kernel's 280: every iteration
    // pays an L2 round trip.)
    if ((reinterpret_cast<uintptr_t>(p.h) & 15) == 0 && (p.H & 3) == 0) {
        constexpr int HW4 = HW / 4, NT = NW * 64;
        const int n4 = Bp * HW4;
        float4* lds4 = reinterpret_cast<float4*>(lds);
        for (int i0 = tid; i0 < n4; i0 += 8 * NT) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * NT, n4 - 1);
                const int r = i / HW4, c4 = i - r * HW4;
                v[u] = *reinterpret_cast<const float4*>(p.h + (size_t)min(r, p.B - 1) * p.H + hc0 + 4 * c4);
                if (r >= p.B) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * NT;
                if (i < n4) lds4[i] = v[u];
            }
        }
    } else {
        for (int i = tid; i < Bp * HW; i += NW * 64) {
            const int r = i / HW, c = i - r * HW;
            lds[i] = r < p.B ? p.h[(size_t)r * p.H + hc0 + c] : 0.0f;
        }
    }
    __syncthreads();

    const int n_tiles = (p.V + 63) / 64;
    const int n_ws = p.nb_half * NW;
    for (int t = bir * NW + wave; t < n_tiles; t += n_ws) {
        const int v0 = t * 64;
        const int vcol = v0 + 2 * j;                                 // this lane's 2 columns
        const bool ok0 = vcol < p.V, ok1 = vcol + 1 < p.V;
        f32x16 acc[NA][2];
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.0f;
        float cs0 = 0.f, cs1 = 0.f;

        // B operand from dz^T [V][ldT]: the tile's 64 columns x B rows are ONE contiguous 64 KiB
        // block there (a strip of row-major dz is 256-byte pieces at a 4*V-byte stride: every piece
        // another DRAM page and TLB entry -- 584 us measured).  A lane owns columns vcol, vcol+1 =
        // two rows of dz^T; one float4 per row carries 4 consecutive playlists = 2 k-steps
        // (playlist 4q + 2*step + hi).
        const float* t0p = p.dzT + (size_t)(ok0 ? vcol : 0) * p.ldT;
        const float* t1p = p.dzT + (size_t)(ok1 ? vcol + 1 : 0) * p.ldT;
// unconditional loads (conditional writes to these arrays sent them to scratch memory): columns
// past V read row 0 and accumulate values that are never stored; the prefetch issued in the last
// iteration re-reads the last group
#define GW_LOAD(T0, T1, R0)                                                                    \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                     \
            const int r4 = min((R0) + 4 * q_, Bp4 - 4);                                        \
            T0[q_] = *reinterpret_cast<const float4*>(t0p + r4);                               \
            T1[q_] = *reinterpret_cast<const float4*>(t1p + r4);                               \
        }
#define GW_STEP(DX, DY, R)                                                                     \
        {                                                                                      \
            const float* ap = lds + (size_t)((R) + hi) * HW + NA * j;                          \
            float av[NA];                                                                      \
            if (NA == 4) {                                                                     \
                const float4 t4 = *reinterpret_cast<const float4*>(ap);                        \
                av[0] = t4.x; av[1 % NA] = t4.y; av[2 % NA] = t4.z; av[3 % NA] = t4.w;         \
            } else if (NA == 2) {                                                              \
                const float2 t2 = *reinterpret_cast<const float2*>(ap);                        \
                av[0] = t2.x; av[1 % NA] = t2.y;                                               \
            } else {                                                                           \
                av[0] = ap[0];                                                                 \
            }                                                                                  \
            cs0 += (DX); cs1 += (DY);                                                          \
            _Pragma("unroll") for (int a = 0; a < NA; ++a)                                     \
                acc[a][0] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32((DX), av[a], acc[a][0], 0, 0, 0) \
                               : __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], (DX), acc[a][0], 0, 0, 0); \
            _Pragma("unroll") for (int a = 0; a < NA; ++a)                                     \
                acc[a][1] = TR ? __builtin_amdgcn_mfma_f32_32x32x2f32((DY), av[a], acc[a][1], 0, 0, 0) \
                               : __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], (DY), acc[a][1], 0, 0, 0); \
        }
// the upper half-wave takes the odd playlist.  A bit blend (v_bfi), NOT `hi ? t.y : t.x`: the
// optimizer turns that into a dynamically indexed vector extract, which lives in scratch memory.
#define GW_SEL(A, Bv) __uint_as_float((__float_as_uint(Bv) & himask) | (__float_as_uint(A) & ~himask))
#define GW_MMA(T0, T1, R0)                                                                     \
        _Pragma("unroll") for (int q_ = 0; q_ < 4; ++q_) {                                     \
            const int r4 = (R0) + 4 * q_;                                                      \
            GW_STEP(GW_SEL(T0[q_].x, T0[q_].y), GW_SEL(T1[q_].x, T1[q_].y), r4)                \
            GW_STEP(GW_SEL(T0[q_].z, T0[q_].w), GW_SEL(T1[q_].z, T1[q_].w), r4 + 2)            \
        }
        const int Bp4 = Bp;                          // dz^T rows are zero padded to a multiple of 64
        const unsigned himask = hi ? 0xFFFFFFFFu : 0u;
        float4 ta0[4], ta1[4], tb0[4], tb1[4];
        GW_LOAD(ta0, ta1, 0)
        for (int r0 = 0; r0 < Bp; r0 += 32) {        // straight-line 16 k-steps per iteration
            GW_LOAD(tb0, tb1, r0 + 16)
            __builtin_amdgcn_sched_barrier(0);       // keep the prefetch AHEAD of the 64 MFMAs below
            GW_MMA(ta0, ta1, r0)                     // (hipcc sinks loads next to their first use)
            __builtin_amdgcn_sched_barrier(0);
            GW_LOAD(ta0, ta1, r0 + 32)               // past the end: re-reads the last group
            __builtin_amdgcn_sched_barrier(0);
            GW_MMA(tb0, tb1, r0 + 16)
            __builtin_amdgcn_sched_barrier(0);
        }
#undef GW_LOAD
#undef GW_STEP
#undef GW_SEL
#undef GW_MMA
        // D[i][j]: hidden unit hc0 + NA * i_idx + a, i_idx = acc_row32(reg, hi); column v0 + 2 j + b.  The NA `a` accumulators
        // of one reg are NA consecutive hidden units.
        if (TR && NA == 4) {
            // register reg of accumulator (a, b) is row v0 + 2 acc_row32(reg, hi) + b; lane j holds hidden units
            // hc0 + 4 j + a: one float4 per (b, reg)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
#pragma unroll
                for (int r4 = 0; r4 < 16; r4 += 4) {
                    if (p.ad.m) {
                        // the gradient tile goes straight into the Adam update of its parameters: W / m / v are read and
                        // written in place, gW never reaches memory (7 passes over the tensor + 1 of the gradient become 6).
                        // 12 loads, compute, 12 stores per group of four rows.
                        float4 pp[4], mm[4], vv[4], gp[ACC ? 4 : 1];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int v = v0 + 2 * acc_row32(r4 + u, hi) + b;
                            const size_t o = (size_t)(v < p.V ? v : 0) * p.H + hc0 + 4 * j;
                            pp[u] = nt_ld4(p.ad.p + o);
                            mm[u] = nt_ld4(p.ad.m + o);
                            vv[u] = nt_ld4(p.ad.v + o);
                            if (ACC) gp[ACC ? u : 0] = nt_ld4(p.gprev + o);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int reg = r4 + u;
                            const int v = v0 + 2 * acc_row32(reg, hi) + b;
                            const size_t o = (size_t)(v < p.V ? v : 0) * p.H + hc0 + 4 * j;
                            float4 gg = make_float4(acc[0][b][reg], acc[1 % NA][b][reg], acc[2 % NA][b][reg], acc[3 % NA][b][reg]);
                            if (ACC) {
                                const float4 g0 = gp[ACC ? u : 0];
                                gg = make_float4(g0.x + gg.x, g0.y + gg.y, g0.z + gg.z, g0.w + gg.w);
                            }
                            dae_adam_el4(pp[u], mm[u], vv[u], gg, p.ad.alpha, p.ad.b1, p.ad.b2, p.ad.eps);
                            if (v < p.V) {
                                nt_st4(p.ad.p + o, pp[u]);
                                nt_st4(p.ad.m + o, mm[u]);
                                nt_st4(p.ad.v + o, vv[u]);
                            }
                        }
                    } else {
                        float4 gp[ACC ? 4 : 1];
                        if (ACC) {                      // the four rows' earlier sums first, then the four stores
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int v = v0 + 2 * acc_row32(r4 + u, hi) + b;
                                gp[ACC ? u : 0] = *reinterpret_cast<const float4*>(p.gprev + (size_t)(v < p.V ? v : 0) * p.H + hc0 + 4 * j);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            const int reg = r4 + u;
                            const int v = v0 + 2 * acc_row32(reg, hi) + b;
                            if (v >= p.V) continue;
                            float4 gg = make_float4(acc[0][b][reg], acc[1 % NA][b][reg], acc[2 % NA][b][reg], acc[3 % NA][b][reg]);
                            if (ACC) {
                                const float4 g0 = gp[ACC ? u : 0];
                                gg = make_float4(g0.x + gg.x, g0.y + gg.y, g0.z + gg.z, g0.w + gg.w);
                            }
                            *reinterpret_cast<float4*>(p.gW + (size_t)v * p.H + hc0 + 4 * j) = gg;
                        }
                    }
                }
            }
        } else
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int v = vcol + b;
            if (v >= p.V) continue;
            float* orow = p.gW + (size_t)v * p.H + hc0;
            const float* prow = p.gprev + (size_t)v * p.H + hc0;          // (read under ACC only)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i_idx = acc_row32(reg, hi);
                if (NA == 4) {
                    float4 gg = make_float4(acc[0][b][reg], acc[1 % NA][b][reg], acc[2 % NA][b][reg], acc[3 % NA][b][reg]);
                    if (ACC) {
                        const float4 g0 = *reinterpret_cast<const float4*>(prow + 4 * i_idx);
                        gg = make_float4(g0.x + gg.x, g0.y + gg.y, g0.z + gg.z, g0.w + gg.w);
                    }
                    *reinterpret_cast<float4*>(orow + 4 * i_idx) = gg;
                } else {
#pragma unroll
                    for (int a = 0; a < NA; ++a) orow[NA * i_idx + a] = ACC ? prow[NA * i_idx + a] + acc[a][b][reg] : acc[a][b][reg];
                }
            }
        }
        if (p.gb && half == 0) {
            cs0 += __shfl_xor(cs0, 32);
            cs1 += __shfl_xor(cs1, 32);
            if (hi == 0) {
                if (ok0) p.gb[vcol] = ACC ? p.gb[vcol] + cs0 : cs0;
                if (ok1) p.gb[vcol + 1] = ACC ? p.gb[vcol + 1] + cs1 : cs1;
            }
        }
    }
}

// ---- K6, transposed orientation (bf16 operands, dz^T stored as bf16, hidden a multiple of 128) --------------------
// Same product gW[v, hc] = sum_r dz[r, v] h[r, hc] with the operand roles swapped: A = dz^T (M = vocabulary rows),
// B = h^T (N = hidden units), so that an accumulator lane is a hidden unit and its registers are vocabulary rows.
// What that buys is memory shape on both sides:
//   * A fragments are plain 16-byte loads from the bf16 dz^T row of the lane (8 consecutive playlists): no selects,
//     no permutes, no conversions;
//   * a store instruction writes, per half-wave, 32 lanes x float4 = 512 contiguous bytes of ONE gW row (hidden =
//     hc0 + 4 n + a), where the other orientation writes 16-byte pieces of 32 rows (57 of its 113 us were the store);
//     the armed Adam update (dae_arm_decoder_adam) reads and writes W / m / v with the same shape.
// LDS holds h^T for the workgroup's 128 hidden units as bf16 B fragments in operand order: 4 KB per k-step of 16
// playlists, 64 KB at B = 256.  gb = dz^T 1 comes out of the matrix pipe as well (a ones fragment as B operand).
template <int NW, bool FULL, bool ACC>
__device__ __forceinline__ void grad_wdec_t_body(const GwP& p)
{
    extern __shared__ __attribute__((aligned(16))) uint4 ldsq[];      // [S][4][64] B fragments
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, n = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const K6Block wg = k6_block(p, 128);
    const int half = wg.half, bir = wg.bir, hc0 = wg.hc0;
    const int S = wg.Bp >> 4;                                          // k-steps of 16 playlists (2..16)
    k6_fill_ht_bf16(ldsq, p, hc0, S, tid, NW * 64);
    __syncthreads();

    const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));
    const unsigned short* dz = reinterpret_cast<const unsigned short*>(p.dzT);
    const int n_tiles = (p.V + 63) / 64;
    const int n_ws = p.nb_half * NW;
    constexpr int RING = 4;                                            // k-steps of A fragments in flight per wave (8: spills)
    for (int t = bir * NW + wave; t < n_tiles; t += n_ws) {
        const int v0 = t * 64;
        const int va = v0 + n, vb = v0 + 32 + n;                       // this lane's two A rows
        const unsigned short* ra = dz + (size_t)(va < p.V ? va : 0) * p.ldT + 8 * hi;
        const unsigned short* rb = dz + (size_t)(vb < p.V ? vb : 0) * p.ldT + 8 * hi;
        f32x16 acc[2][4], accg[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
#pragma unroll
            for (int e = 0; e < 16; ++e) accg[m][e] = 0.0f;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][a][e] = 0.0f;
        }
        uint4 qa[RING], qb[RING];
#pragma unroll
        for (int u = 0; u < RING; ++u) {
            const int su = (FULL || u < S) ? u : S - 1;
            qa[u] = *reinterpret_cast<const uint4*>(ra + 16 * su);
            qb[u] = *reinterpret_cast<const uint4*>(rb + 16 * su);
        }
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) {
            // (FULL: S == 16, a batch of 241 .. 256, known at compile time -- with the wave-uniform tests in the loop hipcc ends
            // every step on s_waitcnt vmcnt(0), i.e. on the ring slot it has just requested)
            if (FULL || s_ < S) {                                      // wave-uniform
                const bf16x8_t fa = __builtin_bit_cast(bf16x8_t, qa[s_ % RING]);
                const bf16x8_t fb = __builtin_bit_cast(bf16x8_t, qb[s_ % RING]);
                if (s_ + RING < 16) {                                  // refill the slot (clamped: values unused past S)
                    const int sn = (FULL || s_ + RING < S) ? s_ + RING : S - 1;
                    qa[s_ % RING] = *reinterpret_cast<const uint4*>(ra + 16 * sn);
                    qb[s_ % RING] = *reinterpret_cast<const uint4*>(rb + 16 * sn);
                }
                uint4 bq[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) bq[a] = ldsq[(s_ * 4 + a) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const bf16x8_t bf = __builtin_bit_cast(bf16x8_t, bq[a]);
                    acc[0][a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, bf, acc[0][a], 0, 0, 0);
                    acc[1][a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, bf, acc[1][a], 0, 0, 0);
                }
                accg[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, ones, accg[0], 0, 0, 0);
                accg[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, ones, accg[1], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (p.gb && half == 0 && n == 0) {                             // every lane holds the row sums; lanes 0 and 32 store
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int v = v0 + 32 * m + acc_row32(reg, hi);
                    if (v < p.V) p.gb[v] = ACC ? p.gb[v] + accg[m][reg] : accg[m][reg];
                }
        }
        // lane n holds hidden units hc0 + 4 n + a (a = the 4 accumulators of a register), register reg the row
        // v0 + 32 m + acc_row32(reg, hi): one float4 per (m, reg), 512 contiguous bytes per half-wave
        if (ACC) {
            // the earlier panels' rows four at a time (the dz^T ring's registers are free by now), then their four stores
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int r4 = 0; r4 < 16; r4 += 4) {
                    float4 gp[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int v = v0 + 32 * m + acc_row32(r4 + u, hi);
                        gp[u] = *reinterpret_cast<const float4*>(p.gprev + (size_t)(v < p.V ? v : 0) * p.H + hc0 + 4 * n);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int reg = r4 + u;
                        const int v = v0 + 32 * m + acc_row32(reg, hi);
                        if (v < p.V)
                            *reinterpret_cast<float4*>(p.gW + (size_t)v * p.H + hc0 + 4 * n) =
                                make_float4(gp[u].x + acc[m][0][reg], gp[u].y + acc[m][1][reg], gp[u].z + acc[m][2][reg],
                                            gp[u].w + acc[m][3][reg]);
                    }
                }
        } else
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int v = v0 + 32 * m + acc_row32(reg, hi);
                if (v < p.V)
                    *reinterpret_cast<float4*>(p.gW + (size_t)v * p.H + hc0 + 4 * n) =
                        make_float4(acc[m][0][reg], acc[m][1][reg], acc[m][2][reg], acc[m][3][reg]);
            }
    }
}

// ---- K6, transposed orientation, the armed-Adam form with its state streams kept in flight (round 6) ---------------------------
// grad_wdec_t_kernel above runs a tile in two phases -- 160 MFMAs with 4 KB of dz^T requests in flight per wave, then the Adam
// pass in groups of 12 x 1 KB loads, compute, 12 stores -- and sits at 5.3 TB/s for 1.14 GB with its waves parked 59 % of the time
// (SQ counters, r06 notes 8): too few bytes in flight, not too many instructions.  At 248 registers it has no room for more.
// This form halves the tile (32 decoder rows: 64 accumulator registers instead of 128 + 32) and spends the registers on the
// streams: the first group of p / m / v rows of a tile is requested BEFORE its MFMAs (under which it arrives), and inside the Adam
// pass group g + 1 is requested before group g is computed and stored (two buffers).  Same operands, same k order per
// element, same update operations as above: the parameters stay bit-identical to dense Adam.
template <int NW, bool FULL, bool ACC>
__device__ __forceinline__ void grad_wdec_t32_body(const GwP& p)
{
    extern __shared__ __attribute__((aligned(16))) uint4 ldsq[];      // [S][4][64] B fragments
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, n = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const K6Block wg = k6_block(p, 128);
    const int half = wg.half, bir = wg.bir, hc0 = wg.hc0;
    const int S = wg.Bp >> 4;                                          // k-steps of 16 playlists (2..16)
    k6_fill_ht_bf16(ldsq, p, hc0, S, tid, NW * 64);
    __syncthreads();

    const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u));
    const unsigned short* dz = reinterpret_cast<const unsigned short*>(p.dzT);
    const int n_tiles = (p.V + 31) / 32;
    const int n_ws = p.nb_half * NW;
    constexpr int RING = 4;
    for (int t = bir * NW + wave; t < n_tiles; t += n_ws) {
        const int v0 = t * 32;
        const int va = v0 + n;
        const unsigned short* ra = dz + (size_t)(va < p.V ? va : 0) * p.ldT + 8 * hi;
        f32x16 acc[4], accg;
#pragma unroll
        for (int e = 0; e < 16; ++e) accg[e] = 0.0f;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][e] = 0.0f;
        uint4 qa[RING];
#pragma unroll
        for (int u = 0; u < RING; ++u) qa[u] = *reinterpret_cast<const uint4*>(ra + 16 * ((FULL || u < S) ? u : S - 1));
        K6AdamRows<ACC> ad;
        ad.issue(p, 0, 0, v0, hi, hc0 + 4 * n);                         // group 0 arrives under the MFMAs
        // (S == 16 -- a batch of 241 .. 256 -- is a template case: with the wave-uniform `s_ < S` tests in the loop hipcc ends every
        // step on s_waitcnt vmcnt(0), i.e. on the ring slot it has just requested: 16 memory round trips per tile instead of a ring)
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) {
            if (FULL || s_ < S) {                                      // wave-uniform
                const bf16x8_t fa = __builtin_bit_cast(bf16x8_t, qa[s_ % RING]);
                if (s_ + RING < 16) {
                    const int sn = (FULL || s_ + RING < S) ? s_ + RING : S - 1;
                    qa[s_ % RING] = *reinterpret_cast<const uint4*>(ra + 16 * sn);
                }
                uint4 bq[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) bq[a] = ldsq[(s_ * 4 + a) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, __builtin_bit_cast(bf16x8_t, bq[a]), acc[a], 0, 0, 0);
                accg = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, ones, accg, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (p.gb && half == 0 && n == 0) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int v = v0 + acc_row32(reg, hi);
                if (v < p.V) p.gb[v] = ACC ? p.gb[v] + accg[reg] : accg[reg];
            }
        }
        ad.pass(p, acc, v0, hi, hc0 + 4 * n);
    }
}

// ---- K6 with fp32 operands (train_dtype = f32), the armed-Adam form with its state streams kept in flight (round 6) -------------
// grad_wdec_t32_kernel's plan on v_mfma_f32_32x32x2_f32: a tile of 32 decoder rows, A = dz^T (fp32 rows; a float4 = 4
// playlists = two k-steps, the lane half hi taking the even / odd one), B = h^T from LDS (one float4 per lane and k-step: the four
// accumulators' hidden units), 512 MFMAs per tile, the row sums (gb) on the VALU; then the Adam pass of section 12 -- the first
// group of p / m / v rows requested before the MFMAs, group g + 1 before group g is computed.  The generic kernel it replaces
// for this case (grad_wdec_kernel<4, 8, true>) ran its two phases back to back at 12 KB in flight per wave: 349 us
// for 180 us of matrix work and 1.22 GB.
template <int NW, bool FULL, bool ACC>
__device__ __forceinline__ void grad_wdec_t32_f32_body(const GwP& p)
{
    extern __shared__ __attribute__((aligned(16))) float4 ldsf[];     // [Bp / 2 k-steps][64 lanes]: h[2 g + hi][hc0 + 4 n .. + 3]
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, n = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const K6Block wg = k6_block(p, 128);
    const int half = wg.half, bir = wg.bir, hc0 = wg.hc0, Bp = wg.Bp;
    const int Q = Bp >> 2;                                             // float4 of a dz^T row (4 playlists each)

    for (int f = tid; f < (Bp >> 1) * 64; f += NW * 64) {
        const int fl = f & 63, g = f >> 6;
        const int r = 2 * g + (fl >> 5);
        ldsf[f] = r < p.B ? *reinterpret_cast<const float4*>(p.h + (size_t)r * p.H + hc0 + 4 * (fl & 31)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();

    const int n_tiles = (p.V + 31) / 32;
    const int n_ws = p.nb_half * NW;
    constexpr int RING = 4;
    const unsigned himask = hi ? 0xFFFFFFFFu : 0u;
    // (Tried: the second wave of each SIMD starting 2 .. 16 x 8 k cycles late, so that one wave's MFMAs run under the other's state
    // streams -- 345 - 352 us at every setting: phases that coincide are not what this launch loses its time to.)
#define K6F_SEL(A, Bv) __uint_as_float((__float_as_uint(Bv) & himask) | (__float_as_uint(A) & ~himask))
    for (int t = bir * NW + wave; t < n_tiles; t += n_ws) {
        const int v0 = t * 32;
        const int va = v0 + n;
        const float4* ra = reinterpret_cast<const float4*>(p.dzT + (size_t)(va < p.V ? va : 0) * p.ldT);
        f32x16 acc[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][e] = 0.0f;
        float cs = 0.0f;
        float4 qa[RING];
#pragma unroll
        for (int u = 0; u < RING; ++u) qa[u] = ra[(FULL || u < Q) ? u : Q - 1];
        K6AdamRows<ACC> ad;
        ad.issue(p, 0, 0, v0, hi, hc0 + 4 * n);                         // group 0 arrives under the 512 MFMAs
        const int q_end = FULL ? 64 : Q;
        for (int q0 = 0; q0 < q_end; q0 += RING) {
#pragma unroll
            for (int u = 0; u < RING; ++u) {
                const int qq = q0 + u;
                const float4 d4 = qa[u];
                {
                    const int qn = qq + RING;
                    qa[u] = ra[(FULL ? qn < 64 : qn < Q) ? qn : q_end - 1];
                }
                const float4 bA = ldsf[(2 * qq) * 64 + lane], bB = ldsf[(2 * qq + 1) * 64 + lane];
                const float dA = K6F_SEL(d4.x, d4.y), dB = K6F_SEL(d4.z, d4.w);
                __builtin_amdgcn_sched_barrier(0);
                cs += dA; cs += dB;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dA, bA.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dA, bA.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(dA, bA.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(dA, bA.w, acc[3], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dB, bB.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dB, bB.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(dB, bB.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(dB, bB.w, acc[3], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        cs += __shfl_xor(cs, 32);                                      // the two lane halves hold the even / odd playlists of the row
        if (p.gb && half == 0 && hi == 0 && va < p.V) p.gb[va] = ACC ? p.gb[va] + cs : cs;
        ad.pass(p, acc, v0, hi, hc0 + 4 * n);
    }
#undef K6F_SEL
}

// the entry points: <...>_kernel as ever, <...>_acc_kernel for a later panel
template <int NA, int NW = 4, bool TR = false>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_kernel(const GwP p) { grad_wdec_body<NA, NW, TR, false>(p); }
template <int NA, int NW = 4, bool TR = false>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_acc_kernel(const GwP p) { grad_wdec_body<NA, NW, TR, true>(p); }
template <int NW, bool FULL = false>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_t_kernel(const GwP p) { grad_wdec_t_body<NW, FULL, false>(p); }
template <int NW, bool FULL = false>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_t_acc_kernel(const GwP p) { grad_wdec_t_body<NW, FULL, true>(p); }
template <int NW, bool FULL>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_t32_kernel(const GwP p) { grad_wdec_t32_body<NW, FULL, false>(p); }
template <int NW, bool FULL>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_t32_acc_kernel(const GwP p) { grad_wdec_t32_body<NW, FULL, true>(p); }
template <int NW, bool FULL>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_t32_f32_kernel(const GwP p) { grad_wdec_t32_f32_body<NW, FULL, false>(p); }
template <int NW, bool FULL>
__global__ __launch_bounds__(NW * 64, 1) void grad_wdec_t32_f32_acc_kernel(const GwP p) { grad_wdec_t32_f32_body<NW, FULL, true>(p); }

}  // namespace

// K6 on caller-provided buffers: gW[v, :] = sum_r dzT[v, r] h[r, :] and gb[v] = sum_r dzT[v, r] (gb nullable), or, with `arm`,
// the Adam update of arm->p from that gradient (gW is not touched).  H % 32 == 0, B <= 256; dz16: dz^T holds bf16 (H % 128 == 0).
// small_v: the caller's V is a few tiles (the title scorer's output layer): the 4-wave untransposed form, as it always took.
// gprev: null, or the [V, H] gradient of the earlier panels of a batch above 256 rows (train.hip): the tile is added to it, gW
// (or the armed update) takes the sum, and gb has this panel's column sums added to what it holds.
int dae_launch_k6(dae_ctx* ctx, const float* dzT, int64_t ldT, int dz16, const float* h, int H, int B, int V, float* gW,
                  float* gb, const dae_armed_adam* arm, int small_v, const float* gprev)
{
    if ((H % 32) != 0 || B < 1 || B > 256) return dae_fail(ctx, DAE_ERR_ARG, "grad_w: H=%d B=%d unsupported", H, B);
    const int NA = (H % 128) == 0 ? 4 : ((H % 64) == 0 ? 2 : 1);
    if ((arm || dz16) && NA != 4) return dae_fail(ctx, DAE_ERR_ARG, "grad_w: armed Adam / bf16 dz^T need H %% 128 == 0 (H=%d)", H);
    if (gprev && small_v) return dae_fail(ctx, DAE_ERR_ARG, "grad_w: no accumulation in the small-V form");
    GwP p;
    p.dzT = dzT; p.ldT = ldT; p.h = h; p.H = H; p.B = B; p.V = V; p.gW = gW; p.gb = gb; p.gprev = gprev;
    p.ad = arm ? *arm : dae_armed_adam{nullptr, nullptr, nullptr, 0.0f, 0.0f, 0.0f, 0.0f};
    p.n_half = H / (32 * NA);
    int nb = (DAE_NUM_CU / p.n_half) / DAE_NUM_XCD * DAE_NUM_XCD;
    if (nb < DAE_NUM_XCD) nb = DAE_NUM_XCD;
    p.nb_half = nb;
    const int Bp32 = (B + 31) & ~31;
    const bool full = Bp32 == 256;
    const size_t lds = (size_t)Bp32 * 32 * NA * sizeof(float);              // grad_wdec_kernel: h[:, half] as fp32
    const size_t lds_t = (size_t)(Bp32 >> 4) * 4 * 64 * sizeof(uint4);      // t / t32: bf16 B fragments of h^T
    const size_t lds_f = (size_t)(Bp32 >> 1) * 64 * sizeof(float4);         // t32_f32: fp32 float4 of h^T
    const dim3 grid(p.n_half * nb), w4(256), w8(512);
    hipStream_t st = ctx->stream;
    // two waves per SIMD on the shared h image: 241 us against 257 us with one (V = 170 000, B = H = 256); the
    // second wave covers the dz^T load latency and the gW stores of the first
    //
    //   dz^T   armed  H == 256  rows == 256   instance
    //   bf16   yes    any       yes / no      grad_wdec_t32_kernel<8, true / false>
    //   bf16   no     any       yes / no      grad_wdec_t_kernel<8, true / false>
    //   fp32   yes    yes       yes / no      grad_wdec_t32_f32_kernel<8, true / false>
    //   fp32   yes    no        any           grad_wdec_kernel<4, 8, true>, armed
    //   fp32   no     any       any           grad_wdec_kernel<4, 8, true> (H % 128 == 0), <2> or <1>;  small_v: <4>, <2> or <1>
    //   gprev (a later panel of a batch above 256 rows): the same choice among the _acc twins; never with small_v
    if (gprev) {
        if (dz16 && arm) {
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_acc_kernel<8, true>, 64 * 1024));
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_acc_kernel<8, false>, 64 * 1024));
            if (full) hipLaunchKernelGGL((grad_wdec_t32_acc_kernel<8, true>), grid, w8, lds_t, st, p);
            else hipLaunchKernelGGL((grad_wdec_t32_acc_kernel<8, false>), grid, w8, lds_t, st, p);
        } else if (dz16) {
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t_acc_kernel<8, true>, 64 * 1024));
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t_acc_kernel<8>, 160 * 1024));
            if (full) hipLaunchKernelGGL((grad_wdec_t_acc_kernel<8, true>), grid, w8, lds_t, st, p);
            else hipLaunchKernelGGL((grad_wdec_t_acc_kernel<8>), grid, w8, lds_t, st, p);
        } else if (arm && H == 256) {
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_f32_acc_kernel<8, true>, 128 * 1024));
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_f32_acc_kernel<8, false>, 128 * 1024));
            if (full) hipLaunchKernelGGL((grad_wdec_t32_f32_acc_kernel<8, true>), grid, w8, lds_f, st, p);
            else hipLaunchKernelGGL((grad_wdec_t32_f32_acc_kernel<8, false>), grid, w8, lds_f, st, p);
        } else if (NA == 4) {
            DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_acc_kernel<4, 8, true>, 160 * 1024));
            hipLaunchKernelGGL((grad_wdec_acc_kernel<4, 8, true>), grid, w8, lds, st, p);
        } else if (NA == 2) hipLaunchKernelGGL(grad_wdec_acc_kernel<2>, grid, w4, lds, st, p);
        else hipLaunchKernelGGL(grad_wdec_acc_kernel<1>, grid, w4, lds, st, p);
    } else if (dz16 && arm) {
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_kernel<8, true>, 64 * 1024));
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_kernel<8, false>, 64 * 1024));
        if (full) hipLaunchKernelGGL((grad_wdec_t32_kernel<8, true>), grid, w8, lds_t, st, p);
        else hipLaunchKernelGGL((grad_wdec_t32_kernel<8, false>), grid, w8, lds_t, st, p);
    } else if (dz16) {
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t_kernel<8, true>, 64 * 1024));
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t_kernel<8>, 160 * 1024));
        if (full) hipLaunchKernelGGL((grad_wdec_t_kernel<8, true>), grid, w8, lds_t, st, p);
        else hipLaunchKernelGGL((grad_wdec_t_kernel<8>), grid, w8, lds_t, st, p);
    } else if (arm && H == 256) {
        // (the ring walks the dz^T row four float4 at a time: whole groups of 16 playlists -- any multiple of 32 rows)
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_f32_kernel<8, true>, 128 * 1024));
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_t32_f32_kernel<8, false>, 128 * 1024));
        if (full) hipLaunchKernelGGL((grad_wdec_t32_f32_kernel<8, true>), grid, w8, lds_f, st, p);
        else hipLaunchKernelGGL((grad_wdec_t32_f32_kernel<8, false>), grid, w8, lds_f, st, p);
    } else if (NA == 4 && !small_v) {
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_kernel<4, 8, true>, 160 * 1024));
        hipLaunchKernelGGL((grad_wdec_kernel<4, 8, true>), grid, w8, lds, st, p);
    } else if (NA == 4) {
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &grad_wdec_kernel<4>, 160 * 1024));
        hipLaunchKernelGGL(grad_wdec_kernel<4>, grid, w4, lds, st, p);
    } else if (NA == 2) hipLaunchKernelGGL(grad_wdec_kernel<2>, grid, w4, lds, st, p);
    else hipLaunchKernelGGL(grad_wdec_kernel<1>, grid, w4, lds, st, p);
    DAE_CHECK_LAUNCH(ctx, "grad_wdec_kernel");
    return DAE_OK;
}

// (the title scorer's output layer, title.hip) fp32 dz^T, never armed
int dae_launch_grad_w(dae_ctx* ctx, const float* dzT, int64_t ldT, const float* h, int H, int B, int V,
                      float* gW, float* gb)
{
    return dae_launch_k6(ctx, dzT, ldT, 0, h, H, B, V, gW, gb, nullptr, 1, nullptr);
}
