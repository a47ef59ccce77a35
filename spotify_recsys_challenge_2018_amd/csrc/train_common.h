// train_common.h -- what the training translation units (train.hip, grad_wdec.hip, adam.hip) share: the streamed 16-byte
// accesses of the optimiser state, the bf16 MFMA operand alias, and THE Adam element update.
#pragma once
#include "decode_common.h"

// streamed-once 16-byte accesses (Adam state: every byte is read and written exactly once per step)
typedef float nt4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_ld4(const float* a)
{
    const nt4_t t = __builtin_nontemporal_load(reinterpret_cast<const nt4_t*>(a));
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ void nt_st4(float* a, const float4 x)
{
    const nt4_t t = {x.x, x.y, x.z, x.w};
    __builtin_nontemporal_store(t, reinterpret_cast<nt4_t*>(a));
}

typedef bf16x8 bf16x8_t;

// v_mfma_*_32x32*: accumulator register reg (0..15) of a lane in half hi (lane >> 5) holds row i of D[i][j = lane & 31]
__device__ __forceinline__ int acc_row32(int reg, int hi) { return (reg & 3) + 8 * (reg >> 2) + 4 * hi; }

// TF1 ApplyAdam functor, one element:
//   m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);  var -= (m alpha) / (sqrt(v) + eps)
// Every Adam in the library is this function: the dense kernel (adam.hip adam_kernel), the rows-Adam and its replay of
// missed steps with g = 0 (adam_rows_kernel, adam_rows_flush_kernel), and the update the armed decoder-gradient kernels
// apply in their epilogue instead of writing gW_dec (grad_wdec.hip).  The build runs with -ffp-contract=off, so the three
// statements are the same nine rounded operations in the same order wherever they are inlined: same operations on the
// same inputs => the same bits.  That is the whole argument behind "armed Adam == dense Adam == rows Adam, bit for bit"
// (tests/test_gpu_train.py).
__device__ __forceinline__ void dae_adam_el(float& p, float& m, float& v, float g, float alpha, float b1, float b2, float eps)
{
    m = m + (g - m) * (1.0f - b1);
    v = v + (g * g - v) * (1.0f - b2);
    p = p - (m * alpha) / (sqrtf(v) + eps);
}
// the same on the four elements of a float4
__device__ __forceinline__ void dae_adam_el4(float4& p, float4& m, float4& v, const float4 g, float alpha, float b1, float b2,
                                             float eps)
{
    dae_adam_el(p.x, m.x, v.x, g.x, alpha, b1, b2, eps);
    dae_adam_el(p.y, m.y, v.y, g.y, alpha, b1, b2, eps);
    dae_adam_el(p.z, m.z, v.z, g.z, alpha, b1, b2, eps);
    dae_adam_el(p.w, m.w, v.w, g.w, alpha, b1, b2, eps);
}

// THE positives' chain: the logit of one (row, column) as the fp32 MFMA of the forward GEMM computes it -- fmaf over
// k = 0..H-1 from +0, then + bias -- from the decoder row w ([H4] float4, row-major) and the hidden row sh ([H4] float4 in LDS,
// already rounded under BF16); BF16 rounds W the same way (dae_bf16_value).  loss_fixup_kernel (train.hip, the step) and
// loss_rows_finish_kernel (loss_rows.hip, the loss without a step) both call this, so a positive's logit is the same in both.
template <bool BF16>
__device__ __forceinline__ float dae_positive_logit(const float4* __restrict__ w, const float4* sh, int H4, const float* __restrict__ bias_c)
{
    float z = 0.0f;
    int k = 0;
    for (; k + 16 <= H4; k += 16) {                        // (16 loads in flight: the same chain, half the round trips)
        float4 wv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) wv[u] = w[k + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if (BF16) wv[u] = make_float4(dae_bf16_value(wv[u].x), dae_bf16_value(wv[u].y), dae_bf16_value(wv[u].z), dae_bf16_value(wv[u].w));
            const float4 hv = sh[k + u];
            z = fmaf(wv[u].x, hv.x, z); z = fmaf(wv[u].y, hv.y, z);
            z = fmaf(wv[u].z, hv.z, z); z = fmaf(wv[u].w, hv.w, z);
        }
    }
    for (; k + 8 <= H4; k += 8) {
        float4 wv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) wv[u] = w[k + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (BF16) wv[u] = make_float4(dae_bf16_value(wv[u].x), dae_bf16_value(wv[u].y), dae_bf16_value(wv[u].z), dae_bf16_value(wv[u].w));
            const float4 hv = sh[k + u];
            z = fmaf(wv[u].x, hv.x, z); z = fmaf(wv[u].y, hv.y, z);
            z = fmaf(wv[u].z, hv.z, z); z = fmaf(wv[u].w, hv.w, z);
        }
    }
    for (; k < H4; ++k) {
        float4 wv = w[k];
        const float4 hv = sh[k];
        if (BF16) wv = make_float4(dae_bf16_value(wv.x), dae_bf16_value(wv.y), dae_bf16_value(wv.z), dae_bf16_value(wv.w));
        z = fmaf(wv.x, hv.x, z); z = fmaf(wv.y, hv.y, z); z = fmaf(wv.z, hv.z, z); z = fmaf(wv.w, hv.w, z);
    }
    z += *bias_c;
    return z;
}

// blocks of 256 threads for a grid-stride loop over n elements
inline int grid_for(size_t n) { size_t b = (n + 255) / 256; return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b)); }
