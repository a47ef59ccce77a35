// decode_common.h -- what the decode translation units (decode_f32.hip, decode_generic.hip, prepack.hip) share with each
// other and with the kernels built on the same MFMA fragments (mix_filter.hip, refine.hip, title.hip, train.hip): vector
// types, bf16 helpers, the decode kernels' argument block, and the loss head of the training step.
#pragma once
#include "dae_internal.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

template <int N> struct IntC { static constexpr int value = N; };     // a compile-time int as a generic lambda's argument

__device__ __forceinline__ bf16x8 as_bf16x8(const uint4 u) { return __builtin_bit_cast(bf16x8, u); }

// value of the bf16 nearest (ties to even) to f, as the prepack / pack_h kernels round the MFMA operands
__device__ __forceinline__ float dae_bf16_value(float f) { return __uint_as_float(dae_bf16_rne(f) << 16); }

// two floats -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ unsigned pk_bf16(float a, float b)
{
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}

constexpr int DT_F32 = 0;          // v_mfma_f32_32x32x2_f32, exact fp32 (bit-equal to the oracle)
constexpr int DT_BF16 = 1;         // v_mfma_f32_32x32x16_bf16, fp32 accumulate (BASELINE configs[4])

// bf16 kernels take the bias through the matrix pipe: b = e0 + e1 + e2 (three bf16 terms, exact to
// 2^-25 |b|) sits in k-slots 0..2 of an extra A fragment per tile and is multiplied by this B fragment
// of ones, so the accumulators START at the bias: no bias loads or adds in any epilogue, and every
// bf16 kernel produces the same logits for the same (row, column).
__device__ __forceinline__ uint4 bf16_ones_fragment(int hi)
{
    return hi == 0 ? make_uint4(0x3F803F80u, 0x00003F80u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);
}

constexpr int EPI_DENSE = 0;
constexpr int EPI_FILTER = 1;
constexpr int EPI_LOSS = 2;        // training: logits -> loss + dL/dz (DAEs.py:98-100)
constexpr int EPI_GMAX = 3;        // EPI_DENSE (raw logits) + cross-wave group maxima: the threshold sample (phase A)
constexpr int EPI_TERM_ADD = 4;    // an ensemble member's term ADDED to the transposed buffer: outT[c][r] = outT[c][r] + sigmoid(z) * row_scale[r]
constexpr int EPI_ROWLOSS = 5;     // the loss without a step: every element a negative, summed per ROW; nothing stored per element (loss_rows.hip)
constexpr int EPI_MIXROWLOSS = 6;  // EPI_ROWLOSS of the title scorer's MIXED score: the negative term of sigmoid(z) * mix_w[row] + mixT[col][row] (mix_loss.hip)

struct dae_decp {          // argument block of the decode kernels on the prepacked image (filled by decode_f32.hip fill_common)
    const float4* Wp;      // f32: [ntiles][G][64] float4   bf16: [ntiles][G][64] uint4 (8 bf16)
    const float* bias;     // [ntiles*32]
    const uint4* bias16;   // bf16 image only: [ntiles][64] A-operand fragments holding b as 3 bf16 terms
    const float4* hp;      // f32: [n_rg][G][RB][64] float4  bf16: [n_rg][G][RB][64] uint4
    int G;                 // k groups per tile: Hp / 8 (f32, 4 MFMA each) or Hp / 16 (bf16, 1 MFMA)
    int ncols;             // col_hi - col_lo of the prepacked image
    int col_lo;
    int B, n_rg, nb_rg, Bpad;
    dae_tileset ts;
    // dense epilogue
    float* out; int64_t ld; int apply_sigmoid; int mask_from_col; int fill_pad; int vec_ok;
    // EPI_GMAX (threshold sample, phase A of the fused path): besides the dense logits, the maximum over the NW
    // tiles a workgroup decodes in one round of every (row, position in the tile):
    //   gmax[row * ld_gmax + (round * nb_rg + bir) * 32 + c]  = max over waves of z[row][tile(wave)][c]
    // The groups are disjoint sets of columns, so the maxima are distinct elements of the row and their k-th
    // largest is a valid lower bound of the row's k-th largest logit (tau_select_kernel, tau_select.hip).  The tiles of
    // one workgroup sit nb_rg items apart in the bias-ordered list, i.e. in different popularity bands: with ids
    // = popularity ranks the winners are packed into the first tiles, and a group then holds at most one of them
    // (maxima over neighbouring columns would lose 7 of 8: measured, 4 000 instead of 600 survivors per row).
    float* gmax; int64_t ld_gmax;
    int gmax_per_wave;             // small samples (vocabulary shards): no cross-wave maximum, slot = (round * n_ws + wave * nb_rg + bir)
    // filter epilogue
    const float* tau; int n_valid_col; uint2* cand; int* cand_cnt; int cap;
    // decode_f32_h256_filter_kernel (nullable): row group rg walks live_cnt[rg] tiles at live_list[rg * ts.n_items ..), not ts.list
    const int* live_cnt; const int* live_list;
    dae_sample_skip sk;            // decode_f32_kernel's HALF (the threshold sample in half row groups): tiles skipped by their bound
    // title mix (models/DAEs.py:180 of the reference: y = title_score * w_title + dae_score * w_playlist):
    //   DAE side, EPI_DENSE: outT[column * ld_outT + row] = sigmoid(z) * row_scale[row] -- the second term, transposed
    //   (EPI_TERM_ADD: the same element becomes outT[...] + sigmoid(z) * row_scale[row], a further member of an ensemble)
    //   title side, EPI_GMAX / EPI_FILTER: every value becomes sigmoid(z) * mix_w[row] + mixT[column * mix_ld + row]
    //   before it is stored / compared, i.e. the launch ranks the MIXED score; no [B, V] matrix of either scorer exists
    float* outT; int64_t ld_outT; const float* row_scale;
    const float* mixT; int64_t mix_ld; const float* mix_w; int mix_ncols;   // mixT holds global columns [0, mix_ncols)
    // loss epilogue
    float inv_nb; float* dzT; int64_t ldT; float* loss_part;
    int dz16;                      // dzT holds bf16 (the bf16 backward GEMMs read it as such)
    // EPI_ROWLOSS: loss_part is the partial table [n_rg][nb_rg][R_TILE] -- the negatives' sum of row (rg, i) over the tiles of
    // workgroup `bir` of its row group, at ((rg * nb_rg + bir) * R_TILE + i); no mean folded in (inv_nb, dzT unused)
    // EPI_MIXROWLOSS: the same table; mixT / mix_ld / mix_w (above) are the call's own, never dae_set_score_mix's
};

// ---------------------------------------------------------------------------------------------
// The live lists of the fp32 filter launch: ONE test, shared by the two kernels that build them (tau_select.hip tau_select_kernel's
// tail, prepack.hip live_tiles_kernel).  For a row group: d_max = dae_max_nan over its rows r < B and the units k < H of
// |(double)h[r][k] - 0.5| (the zero padding of the packed tile is NOT read: it would give 0.5), tau_min = dae_min_nan over
// the same rows of their thresholds.  A tile with the bound {A_t, M_t} (prepack_tile_kernel) is live unless
// U = A_t + d M_t < tau_min.  Roundings go the safe way: d_max, the product and the sum in double, d and U pushed up by more
// than their rounding errors; the test is !(U < tau_min), so a NaN anywhere (weights, hidden rows, thresholds) and
// tau = -inf keep the tile.
// ---------------------------------------------------------------------------------------------
// the larger of two values, a NaN if either is one (fmax would drop it)
template <class T>
__device__ __forceinline__ T dae_max_nan(T a, T b) { return (a != a) ? a : ((b > a || b != b) ? b : a); }
template <class T>
__device__ __forceinline__ T dae_min_nan(T a, T b) { return -dae_max_nan(-a, -b); }

__device__ __forceinline__ bool dae_tile_is_live(float A_t, float M_t, double d_max, float tau_min)
{
    const double d = d_max * (1.0 + 0x1p-40);               // (|h - 0.5| in double is off by at most 2^-53 relative)
    const double A = (double)A_t, dm = d * (double)M_t;
    const double U = A + dm + (fabs(A) + fabs(dm)) * 0x1p-48;   // two roundings of 2^-53 (|A| + |d M|) at most
    return !(U < (double)tau_min);
}

// The tile that holds the last ranked column (nrank is no multiple of 32) is bounded over its ranked columns only, from the
// columns' own pairs behind the tiles' in tile_ub.  One whole wave calls this; every lane returns the pair.  t_edge < 0: none.
__device__ __forceinline__ void dae_edge_tile_bound(const float* tile_ub, int ntiles, int nrank, int lane, float& ea, float& em)
{
    const int t_edge = nrank >> 5;
    ea = -__builtin_inff(); em = 0.0f;
    if (lane < (nrank & 31)) { ea = tile_ub[2 * (ntiles + t_edge * 32 + lane)]; em = tile_ub[2 * (ntiles + t_edge * 32 + lane) + 1]; }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { ea = dae_max_nan(ea, __shfl_xor(ea, sh)); em = dae_max_nan(em, __shfl_xor(em, sh)); }
}

__device__ __forceinline__ int tile_of_item(const dae_tileset& ts, int i)
{
    return ts.list[i];          // always a list (the identity for "all tiles"): no branch around a load
}

// ---------------------------------------------------------------------------------------------
// The loss head of the training step (DAEs.py:98-99; DESIGN.md section 4, "The loss head at saturated logits"), per
// element with logit z and target y:
//   p = sigmoid(z), a1 = fl(p + 1e-10f), a0 = fl(fl(1 - p) + 1e-10f)
//   L = -[y ln a1 + 0.55 (1 - y) ln a0],  dz = -(y / a1 - 0.55 (1 - y) / a0) p (1 - p) / n_batch
// Training only (parity by tolerance): hardware exp2 / log2 / rcp instead of the canonical sigmoid and IEEE divides the
// ranking path needs.  The test reference (oracle/dae_numpy.py fp32_head) is derived from the operation sequence below:
// every K5 epilogue and loss_fixup_kernel run exactly this, no contraction.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dae_train_sigmoid(float z)
{
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * z));
}
// a NEGATIVE (y = 0) of probability pr: its loss term 0.55 ln a0 (<= 0; the caller SUBTRACTS it) ...
__device__ __forceinline__ float dae_loss_neg_term(float pr)
{
    return (0.69314718f * 0.55f) * __builtin_amdgcn_logf(1.0f - pr + 1e-10f);
}
// ... and its dL/dz, the mean over n_batch folded in
__device__ __forceinline__ float dae_loss_neg_dz(float pr, float inv_nb)
{
    return 0.55f * __builtin_amdgcn_rcpf(1.0f - pr + 1e-10f) * pr * (1.0f - pr) * inv_nb;
}
// The fused K5 + K7 launch (decode_f32.hip decode_loss_dh_bf16_kernel) writes a negative's dz in the short form
// 0.55 p / n_batch: the quotient (1 - p) / (1 - p + 1e-10) it drops is 1 to 1e-10 / (1 - p), inside the 2^-18 the test
// reference allows the hardware rcp and products, unless 1 - p is below this (a logit above 10.5) -- there the wave takes
// the exact quotient.  (It was 1e-6 until tests/test_gpu_train_saturated.py planted logits 13 and 13.7 with n_batch = 365,
// where an error of 4.4e-5 / 8.9e-5 carries dz across a bf16 midpoint: gb_dec of the column off by B bf16 steps.)
constexpr float DAE_LOSS_SHORT_FORM_MIN_Q = 2.7e-5f;
// an element with target y (train.hip loss_fixup_kernel redoes the positives K5 took as negatives): returns dL/dz and adds
// L(y) - L(0) = -ln2 * y * (log2 a1 - 0.55 log2 a0) to corr
__device__ __forceinline__ float dae_loss_head(float pr, float y, float inv_nb, float& corr)
{
    const float a1 = pr + 1e-10f, a0 = 1.0f - pr + 1e-10f;
    const float l1 = __builtin_amdgcn_logf(a1), l0 = __builtin_amdgcn_logf(a0);
    corr -= 0.69314718f * y * (l1 - 0.55f * l0);
    return -(y * __builtin_amdgcn_rcpf(a1) - 0.55f * (1.0f - y) * __builtin_amdgcn_rcpf(a0)) * pr * (1.0f - pr) * inv_nb;
}
// the loss part of dae_loss_head alone (loss_rows.hip loss_rows_finish_kernel: the loss without a step has no dL/dz): adds
// L(y) - L(0) of an element with target y to corr, in dae_loss_head's operations
__device__ __forceinline__ void dae_loss_pos_corr(float pr, float y, float& corr)
{
    const float a1 = pr + 1e-10f, a0 = 1.0f - pr + 1e-10f;
    const float l1 = __builtin_amdgcn_logf(a1), l0 = __builtin_amdgcn_logf(a0);
    corr -= 0.69314718f * y * (l1 - 0.55f * l0);
}
// the same head on the MIXED score yp of the title scorer (title.hip title_loss_kernel), which is no sigmoid of one logit:
// natural logarithms and IEEE quotients, the whole term L(y) subtracted from `loss`; returns dL/dyp / n_batch
__device__ __forceinline__ float dae_loss_head_mixed(float yp, float y, float inv_nb, float& loss)
{
    const float a1 = yp + 1e-10f, a0 = 1.0f - yp + 1e-10f;
    loss -= y * __logf(a1) + 0.55f * (1.0f - y) * __logf(a0);
    return -(y / a1 - 0.55f * (1.0f - y) / a0) * inv_nb;
}
// a NEGATIVE (y = 0) of the mixed score yp: its term 0.55 ln a0 (<= 0; the caller SUBTRACTS it), the bits dae_loss_head_mixed
// subtracts at y = 0 (there 0 * ln a1 is a zero and 0.55f * 1.0f is 0.55f).  decode_f32_kernel's EPI_MIXROWLOSS sums it per row,
// mix_loss.hip mix_loss_finish_kernel takes it back out of a target's element: the mixed loss without a step has no dL/dyp
__device__ __forceinline__ float dae_loss_neg_term_mixed(float yp)
{
    return 0.55f * __logf(1.0f - yp + 1e-10f);
}
// an element of the mixed score with target y (mix_loss.hip redoes the targets the GEMM took as negatives): adds
// L(y) - L(0) = -y (ln a1 - 0.55 ln a0) to corr; the 0.55 ln a0 taken out is dae_loss_neg_term_mixed of the same yp, bit for bit
__device__ __forceinline__ void dae_loss_pos_corr_mixed(float yp, float y, float& corr)
{
    corr -= y * (__logf(yp + 1e-10f) - dae_loss_neg_term_mixed(yp));
}
// the title step's sigmoid of a title logit (title.hip title_loss_kernel), as the two kernels of the mixed loss repeat it
__device__ __forceinline__ float dae_title_step_sigmoid(float z)
{
    return 1.0f / (1.0f + __expf(-z));
}
