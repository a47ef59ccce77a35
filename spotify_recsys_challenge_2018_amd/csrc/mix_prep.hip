// mix_prep.hip -- what the exact title mix (mixexact.hip has the overview) prepares before its two GEMM passes: once per image
// the title side's row-scaled bounds, once per call the rows' feature bounds F_r, their preconditions, and the hidden rows of
// both scorers packed as MFMA operands.
#include "decode_common.h"
#include "mix_common.h"

namespace {

// ---- the title image's row-scaled bounds (mix_common.h has the derivation) ----------------------------------------------
// One 256-thread workgroup per 32-column tile, 8 threads per column (as exact_bounds_kernel).  alpha_hat[c]: the bf16
// value (as a float) the fragments carry; beta[c]: the shift folded into the bias split.
__device__ __forceinline__ uint4 mix_bias_fragment(float bv, unsigned slot3)
{
    const unsigned e0 = dae_bf16_rne(bv);
    const float r1 = bv - __uint_as_float(e0 << 16);
    const unsigned e1 = dae_bf16_rne(r1);
    const float r2 = r1 - __uint_as_float(e1 << 16);
    const unsigned e2 = dae_bf16_rne(r2);
    return make_uint4(e0 | (e1 << 16), e2 | (slot3 << 16), 0u, 0u);
}

__global__ __launch_bounds__(256) void mix_title_bounds_kernel(const float* __restrict__ W, const float* __restrict__ b,
                                                               int H, int Hp, int col_lo, int col_hi, int ntiles,
                                                               float* __restrict__ alpha_hat, float* __restrict__ beta,
                                                               uint4* __restrict__ frag_lo, uint4* __restrict__ frag_hi,
                                                               float margin, int m_lo, int m_hi, float m_scale)
{
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
            float a_f = 0.0f, be_f = 0.0f, lo_f = 0.0f, hi_f = 0.0f;
            unsigned a16 = 0u;
            if (v < col_hi) {
                const double bv = (double)b[v], ab = fabs(bv);
                const double A16 = (double)(Hp + 16) * 0x1p-22;
                const double A32 = (double)(H + 2) * 0x1p-24 * (1.0 + 0x1p-10);
                const double up = 1.0 + 0x1p-8;               // bf16(f) <= F_r (1 + 2^-8); bf16(F_r) and bf16(alpha) round up
                double al = up * d + 0x1p-9 * n + A16 * up * (n + d) + A32 * n;
                double be = (1.01 * A16 + A32 + 0x1p-23) * ab;
                al = al * (1.0 + 4.0 * A16 * up * up) * (1.0 + 1e-6) + 1e-30;      // the shift feeds back through the accumulation
                be = be * (1.0 + 4.0 * A16) * (1.0 + 1e-6) + 0x1p-23 * be + 1e-30;
                // dae_set_exact_margin (< 1 voids the bound: the guard's test hook); _range: some columns only
                const bool in_range = v >= m_lo && v < m_hi;
                const double mg = (double)(in_range && m_scale > 0.0f ? m_scale : margin);
                al *= mg; be *= mg;
                a_f = (float)al;
                if ((double)a_f < al) a_f = __uint_as_float(__float_as_uint(a_f) + 1u);
                a16 = (__float_as_uint(a_f) + 0xFFFFu) >> 16;                     // bf16, rounded up (a_f > 0)
                a_f = __uint_as_float(a16 << 16);
                be_f = (float)be;
                if ((double)be_f < be) be_f = __uint_as_float(__float_as_uint(be_f) + 1u);
                double lo = bv - (double)be_f, hi = bv + (double)be_f;
                if (in_range && m_scale < 0.0f) hi = bv + (double)m_scale;     // (a FORGED filter: the upper bound |scale| logits low)
                lo_f = (float)lo; if ((double)lo_f > lo) lo_f = nextafterf(lo_f, -__builtin_inff());
                hi_f = (float)hi; if ((double)hi_f < hi) hi_f = nextafterf(hi_f, __builtin_inff());
            }
            alpha_hat[t * 32 + c] = a_f;
            beta[t * 32 + c] = be_f;
            frag_lo[t * 64 + c] = v < col_hi ? mix_bias_fragment(lo_f, a16 | 0x8000u) : make_uint4(0u, 0u, 0u, 0u);
            frag_hi[t * 64 + c] = v < col_hi ? mix_bias_fragment(hi_f, a16) : make_uint4(0u, 0u, 0u, 0u);
            frag_lo[t * 64 + 32 + c] = make_uint4(0u, 0u, 0u, 0u);
            frag_hi[t * 64 + 32 + c] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// ---- per row: F_r (bf16, rounded up) and whether the bound's preconditions hold -----------------------------------------
// one wave per row.  row_bad[r] = 1: a DAE hidden entry outside [0, 1], a feature that is not finite, or a mixing weight
// outside [0, 1] -- such rows return no recommendations (idx -1), as in the plain exact mode
__device__ __forceinline__ void mix_rowprep_body(int block, const float* __restrict__ h, int64_t ld_h, int HD,
                                                 const float* __restrict__ feat, int64_t ld_f, int HT,
                                                 const float* __restrict__ w_t, const float* __restrict__ w_p,
                                                 int B, int Bpad, unsigned* __restrict__ fhat, int* __restrict__ row_bad)
{
    const int lane = threadIdx.x & 63;
    const int row = block * 4 + (threadIdx.x >> 6);
    if (row >= Bpad) return;
    float mx = 0.0f;
    bool bad = false;
    if (row < B) {
        for (int k = lane; k < HT; k += 64) {
            const float f = fabsf(feat[(size_t)row * ld_f + k]);
            bad = bad || !(f <= 3.0e38f);
            mx = fmaxf(mx, f);
        }
        for (int k = lane; k < HD; k += 64) {
            const float x = h[(size_t)row * ld_h + k];
            bad = bad || !(x >= 0.0f && x <= 1.0f);
        }
        const float a = w_t[row], c = w_p[row];
        bad = bad || !(a >= 0.0f && a <= 1.0f) || !(c >= 0.0f && c <= 1.0f);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    const bool any_bad = __any(bad);
    if (lane == 0) {
        fhat[row] = mx > 0.0f ? (__float_as_uint(mx) + 0xFFFFu) >> 16 : 0u;
        row_bad[row] = any_bad ? 1 : 0;
    }
}

// hidden rows of both scorers in B-operand order: out uint4 index = ((rg * NS + s) * RB + rb) * 64 + lane holds the bf16 of
// h[r][16 s + 8 hi + 0..7] (s < NSD) or feat[r][16 (s - NSD) + 8 hi + 0..7], r = (rg RB + rb) 32 + j  (zero outside)
__device__ __forceinline__ void mix_pack_body(int block, int n_blocks, const float* __restrict__ h, int64_t ld_h, int HD,
                                              const float* __restrict__ feat, int64_t ld_f, int HT,
                                              int B, int NSD, int NS, int RB, int n_rg, uint4* __restrict__ hp)
{
    const size_t total = (size_t)n_rg * NS * RB * 64;
    for (size_t o = (size_t)block * 256 + threadIdx.x; o < total; o += (size_t)n_blocks * 256) {
        const int lane = (int)(o & 63);
        size_t x = o >> 6;
        const int rb = (int)(x % RB); x /= RB;
        const int s = (int)(x % NS);
        const int rg = (int)(x / NS);
        const int hi = lane >> 5, jj = lane & 31;
        const int r = (rg * RB + rb) * 32 + jj;
        const bool dae = s < NSD;
        const float* src = dae ? h + (size_t)r * ld_h : feat + (size_t)r * ld_f;
        const int k0 = 16 * (dae ? s : s - NSD) + 8 * hi;
        const int Hs = dae ? HD : HT;
        unsigned e[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) e[c] = dae_bf16_rne((r < B && k0 + c < Hs) ? src[k0 + c] : 0.0f);
        hp[o] = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
}

// both in ONE launch (the first `prep_blocks` workgroups prepare rows, the others pack: two launches of ~5 us each sat on the
// launch's critical path -- profiles/r04_title_timeline.txt)
__global__ __launch_bounds__(256) void mix_prep_pack_kernel(const float* __restrict__ h, int64_t ld_h, int HD,
                                                            const float* __restrict__ feat, int64_t ld_f, int HT,
                                                            const float* __restrict__ w_t, const float* __restrict__ w_p, int B,
                                                            int Bpad, unsigned* __restrict__ fhat, int* __restrict__ row_bad,
                                                            int prep_blocks, int NSD, int NS, int RB, int n_rg,
                                                            uint4* __restrict__ hp)
{
    if ((int)blockIdx.x < prep_blocks)
        mix_rowprep_body((int)blockIdx.x, h, ld_h, HD, feat, ld_f, HT, w_t, w_p, B, Bpad, fhat, row_bad);
    else
        mix_pack_body((int)blockIdx.x - prep_blocks, (int)gridDim.x - prep_blocks, h, ld_h, HD, feat, ld_f, HT, B, NSD, NS, RB, n_rg, hp);
}

}  // namespace

int dae_launch_mix_title_bounds(dae_ctx* ctx, const float* W, const float* b, int H, int Hp, int col_lo, int col_hi,
                                int ntiles, dae_packed& pk)
{
    int rc = dae_reserve(ctx, pk.mix_alpha, (size_t)ntiles * 32 * sizeof(float));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.mix_beta, (size_t)ntiles * 32 * sizeof(float));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.mix16_lo, (size_t)ntiles * 64 * sizeof(uint4));
    if (rc) return rc;
    rc = dae_reserve(ctx, pk.mix16_hi, (size_t)ntiles * 64 * sizeof(uint4));
    if (rc) return rc;
    const int blocks = ntiles < 8 * DAE_NUM_CU ? ntiles : 8 * DAE_NUM_CU;
    hipLaunchKernelGGL(mix_title_bounds_kernel, dim3(blocks), dim3(256), 0, ctx->stream, W, b, H, Hp, col_lo, col_hi, ntiles,
                       static_cast<float*>(pk.mix_alpha.p), static_cast<float*>(pk.mix_beta.p),
                       static_cast<uint4*>(pk.mix16_lo.p), static_cast<uint4*>(pk.mix16_hi.p), ctx->exact_margin,
                       ctx->margin_lo, ctx->margin_hi, ctx->margin_scale);
    DAE_CHECK_LAUNCH(ctx, "mix_title_bounds_kernel");
    return DAE_OK;
}

// per row of the call F_r and the preconditions (tc->mix_fhat, tc->row_bad: [Bpad]); the hidden rows of both scorers in
// B-operand order for row groups of pl.RB blocks (tc->h_packed16)
int dae_launch_mix_prep_pack(dae_ctx* tc, const dae_mix_plan& pl, int HD, int HT, const dae_mix_call& c)
{
    const int NS = pl.NSD + pl.NST;
    const size_t total = (size_t)pl.n_rg * NS * pl.RB * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4 * DAE_NUM_CU) blocks = 4 * DAE_NUM_CU;
    const int prep_blocks = (pl.Bpad + 3) / 4;
    hipLaunchKernelGGL(mix_prep_pack_kernel, dim3(prep_blocks + blocks), dim3(256), 0, tc->stream, c.h, c.ld_h, HD, c.feat, c.ld_feat, HT,
                       c.w_title, c.w_playlist, c.B, pl.Bpad, static_cast<unsigned*>(tc->mix_fhat.p), static_cast<int*>(tc->row_bad.p),
                       prep_blocks, pl.NSD, NS, pl.RB, pl.n_rg, static_cast<uint4*>(tc->h_packed16.p));
    DAE_CHECK_LAUNCH(tc, "mix_prep_pack_kernel");
    return DAE_OK;
}
