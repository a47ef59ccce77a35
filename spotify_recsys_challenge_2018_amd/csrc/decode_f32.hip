// decode_f32.hip -- K2: decoder GEMM logits[r, c] = h[r,:] . W_dec[c,:] + b_dec[c] in EXACT fp32
// on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32), reference models/DAEs.py:73-77 (tied) and
// :141-145 (untied), and on bf16 operands (v_mfma_f32_32x32x16_bf16).  Here: the kernels of the shipped shape, hidden =
// 256 -- the two filter kernels (keep only (logit, column) pairs with logit >= tau[row]: the fused front half of the
// top-500 ranking, main_challenge.py:28-36; nothing dense reaches HBM), the bf16 per-wave threshold sample, the two K5
// training forwards from the row-major decoder -- and the public launchers (the host planners: score_plan.h), which pass every other
// shape and the dense epilogue (the reference's y_pred, main_train.py:66) on to the generic kernel of decode_generic.hip.
// The operand images all of them stream are built by prepack.hip.
//
// Structure of the kernels on the prepacked image, generic and hidden-256 alike (DESIGN.md "decode kernel"):
//   * v_mfma_f32_32x32x2_f32 is bit-for-bit the fmaf chain acc = fma(a_k, b_k, acc) over
//     ascending k, i.e. exactly oracle/dae_oracle.c:orc_decode.  A = W_dec tile (32 vocabulary
//     columns x 2 k), B = h^T (2 k x 32 playlists); D[i = column][j = playlist], so every lane
//     holds 16 different columns of ONE playlist (j = lane & 31) and the per-playlist threshold
//     lives in one register.
//   * the hidden tile of a row group (R_TILE playlists x H, 128 KiB at 128 x 256) is copied into
//     LDS ONCE per persistent workgroup; the main loop has no LDS writes and no barriers.
//   * W_dec is streamed straight from HBM into VGPRs from the prepacked image (one coalesced
//     1 KiB global_load_dwordx4 per wave per 8 k), through a 4-deep register ring; each wave owns
//     whole 32-column tiles, so W_dec is read exactly once per row group.
//   * the fp32 matrix pipe issues one MFMA per 64 cycles per SIMD; with 4 independent
//     accumulators a single wave per SIMD saturates it (MI355X_MICROARCH.md), so the workgroup
//     is 4 waves = one per SIMD, one workgroup per CU.
//   * blockIdx -> (row group, slot) is XCD-aware: the workgroups that walk the SAME column tiles
//     for different row groups sit on the same XCD (blockIdx % 8), so the second..n-th read of a
//     W tile hits that XCD's L2 instead of HBM.
#include <climits>

#include "decode_common.h"

namespace {

// ---- training forward (K5) straight from the ROW-MAJOR decoder, hidden = 256 -------------------------------------------
// The decoder changes every training step, so the packed image the scoring kernels stream had to be rebuilt every step (65 us
// for 174 MB) only to be read once: K5 reads the matrix as the optimiser leaves it.  Until round 6 a lane read ITS decoder row
// in 16-byte (fp32) / 32-byte (bf16) pieces -- 32 rows, 64 cache lines per load instruction; the two kernels below take a tile's
// rows as plain 1 KB reads through LDS instead.  The k order of a sum differs from the canonical chain: this is the training
// path, compared by tolerance.  Loss epilogue as decode_generic.hip's EPI_LOSS (every element a negative; the positives are redone by train.hip's
// loss_fixup_kernel).
struct LossRmP {
    const float* W; const float* bias; const float* h;       // [V][H], [V], [B][H] row-major
    int V, H, B, n_rg, nb_rg;
    float inv_nb; float* dzT; int64_t ldT; float* loss_part;
};

// ---- K5 + K7 in one launch (bf16 operands, dz^T as bf16, hidden 256, batches <= 256): dh folded into the forward (round 6) ----
// The forward (K5): a workgroup of 8 waves takes a tile of 32 decoder rows x ALL playlists.  (Until round 6 a wave was a tile of
// 32 decoder rows x 128 playlists, every lane reading ITS decoder row in 32-byte pieces: 64 different cache lines per load
// instruction, one tag lookup each -- 90 us with, 48 us without the W loads; profiles/r06_notes.md 8.)
//   * the 8 waves fetch the tile's 32 rows as plain 1 KB row reads (4 per wave), round them to bf16 and put them in LDS
//     ([row][k], 528-byte rows: conflict-free both ways), two tiles in rotation;
//   * a wave is one block of 32 playlists: its hidden fragments (16 k-steps x 16 B) stay on chip for the whole launch, the A
//     fragments (decoder rows) come from LDS, 16 MFMAs per tile, then the epilogue of its 32 x 32 logits;
//   * every W byte is read once per launch by one workgroup.
// K7 (train.hip grad_hidden_kernel) reads the whole decoder a second time and dz^T back from HBM to form dh = dz W_dec.  Here
// the tile of decoder rows is in LDS already and a lane holds its playlist's 16 dz values of the tile when the epilogue ends:
// the wave multiplies them (A operand: straight from the epilogue's packed bf16 pairs -- the MFMA's k-slots are assigned to
// the tile's rows the way the accumulator layout hands them out) by the tile (B operand: a TRANSPOSED bf16 copy of the tile
// in LDS, [hidden unit][row], the rows permuted the same way) into 8 accumulators = dh[its 32 playlists][256], kept for the
// whole launch and left as one partial per workgroup (part[blockIdx.x][playlist][hidden]: the fixed-order reduce of
// hidden_backward_kernel sums them, K7's chunks before).  Every element is still a NEGATIVE here: loss_fixup_kernel<.., CORR>
// adds (dz_positive - dz_negative) W_dec[v] for the ~25 k positives as one more partial.  Products: bf16(dz) x bf16(W), fp32
// accumulate, as K7's.  Registers: 128 (dh) + 32 (half of the hidden fragments; the other half in LDS) + the forward's.
__global__ __launch_bounds__(512, 1) void decode_loss_dh_bf16_kernel(const LossRmP p, float* __restrict__ part, int Bpad64)
{
    constexpr int NW = 8, LDW = 132, LDT = 18;                         // dwords per staged row: forward copy / transposed copy
    extern __shared__ __attribute__((aligned(16))) unsigned dyn[];
    unsigned* const wt = dyn;                                          // [2][32 * LDW]          forward copy  [row v][k]
    unsigned* const wt2 = dyn + 2 * 32 * LDW;                          // [2][256 * LDT]         transposed    [hidden][row, permuted]
    uint4* const hq = reinterpret_cast<uint4*>(dyn + 2 * 32 * LDW + 2 * 256 * LDT);     // [8 steps][8 waves][64]: steps 8 .. 15
    float* const wsum = reinterpret_cast<float*>(hq + 8 * 8 * 64);
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, j = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = wave * 32 + j;
    const int H4 = p.H >> 2;
    const float4* W4 = reinterpret_cast<const float4*>(p.W);
    const int n_tiles = (p.V + 31) >> 5;
    const int nb = gridDim.x;
    const int t_last = n_tiles - 1;

    // hidden fragments of the lane's playlist: steps 0 .. 7 in registers, 8 .. 15 in LDS (zeros past the batch)
    uint4 hb[8];
    {
        const float4* hr = reinterpret_cast<const float4*>(p.h) + (size_t)(row < p.B ? row : 0) * H4 + 2 * hi;
        float4 ha[16], hc[16];
#pragma unroll
        for (int s_ = 0; s_ < 16; ++s_) { ha[s_] = hr[4 * s_]; hc[s_] = hr[4 * s_ + 1]; }
        const unsigned keep = row < p.B ? 0xFFFFFFFFu : 0u;
#define K5D_FRAG(A, B) make_uint4((dae_bf16_rne(A.x) | (dae_bf16_rne(A.y) << 16)) & keep, (dae_bf16_rne(A.z) | (dae_bf16_rne(A.w) << 16)) & keep, \
                                  (dae_bf16_rne(B.x) | (dae_bf16_rne(B.y) << 16)) & keep, (dae_bf16_rne(B.z) | (dae_bf16_rne(B.w) << 16)) & keep)
#pragma unroll
        for (int s_ = 0; s_ < 8; ++s_) hb[s_] = K5D_FRAG(ha[s_], hc[s_]);
#pragma unroll
        for (int s_ = 8; s_ < 16; ++s_) hq[((s_ - 8) * NW + wave) * 64 + lane] = K5D_FRAG(ha[s_], hc[s_]);
#undef K5D_FRAG
    }
    // the wave's four rows of a tile (lane l: floats 4 l .. 4 l + 3 of each), staged twice: as they are ([row][k]) and transposed
    // ([hidden 4 l + c][the wave's 4 rows]: position of row v = 16 s + 4 h + 8 g + i in its 32: (2 s + h) 8 + 4 g + i, with
    // (s, g, h) = bits of the wave index -- the k-slot order of the dh MFMAs below)
    float4 w0, w1, w2, w3;
    const int tpos = (((wave >> 2) << 1) | (wave & 1)) * 4 + ((wave >> 1) & 1) * 2;          // dwords into a transposed row
#define K5D_LOAD(T)                                                                            \
    {                                                                                          \
        const int v_ = (T) * 32 + 4 * wave;                                                    \
        w0 = W4[(size_t)(v_ < p.V ? v_ : p.V - 1) * H4 + lane];                                \
        w1 = W4[(size_t)(v_ + 1 < p.V ? v_ + 1 : p.V - 1) * H4 + lane];                        \
        w2 = W4[(size_t)(v_ + 2 < p.V ? v_ + 2 : p.V - 1) * H4 + lane];                        \
        w3 = W4[(size_t)(v_ + 3 < p.V ? v_ + 3 : p.V - 1) * H4 + lane];                        \
    }
#define K5D_PK(A, B) pk_bf16((A), (B))
#define K5D_STAGE(BUF)                                                                         \
    {                                                                                          \
        unsigned* d_ = wt + (BUF) * 32 * LDW + (4 * wave) * LDW + 2 * lane;                    \
        *reinterpret_cast<uint2*>(d_) = make_uint2(K5D_PK(w0.x, w0.y), K5D_PK(w0.z, w0.w));    \
        *reinterpret_cast<uint2*>(d_ + LDW) = make_uint2(K5D_PK(w1.x, w1.y), K5D_PK(w1.z, w1.w)); \
        *reinterpret_cast<uint2*>(d_ + 2 * LDW) = make_uint2(K5D_PK(w2.x, w2.y), K5D_PK(w2.z, w2.w)); \
        *reinterpret_cast<uint2*>(d_ + 3 * LDW) = make_uint2(K5D_PK(w3.x, w3.y), K5D_PK(w3.z, w3.w)); \
        unsigned* e_ = wt2 + (BUF) * 256 * LDT + (4 * lane) * LDT + tpos;                      \
        *reinterpret_cast<uint2*>(e_) = make_uint2(K5D_PK(w0.x, w1.x), K5D_PK(w2.x, w3.x));    \
        *reinterpret_cast<uint2*>(e_ + LDT) = make_uint2(K5D_PK(w0.y, w1.y), K5D_PK(w2.y, w3.y)); \
        *reinterpret_cast<uint2*>(e_ + 2 * LDT) = make_uint2(K5D_PK(w0.z, w1.z), K5D_PK(w2.z, w3.z)); \
        *reinterpret_cast<uint2*>(e_ + 3 * LDT) = make_uint2(K5D_PK(w0.w, w1.w), K5D_PK(w2.w, w3.w)); \
    }
    auto load_bias = [&](int t) -> float {
        const int c = t * 32 + j;
        return p.bias[c < p.V ? c : p.V - 1];
    };

    f32x16 dh[8];
#pragma unroll
    for (int b = 0; b < 8; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) dh[b][e] = 0.0f;
    float loss_acc = 0.0f;
    float bl, bl_n = 0.0f;
    int t = blockIdx.x;
    K5D_LOAD(t < t_last ? t : t_last)
    bl = load_bias(t < t_last ? t : t_last);
    K5D_STAGE(0)
    K5D_LOAD(t + nb < t_last ? t + nb : t_last)
    __syncthreads();
    const float k1 = 0.55f * p.inv_nb;
    const bool row_in = row < p.B;
    int buf = 0;
    for (; t < n_tiles; t += nb, buf ^= 1) {
        K5D_STAGE(buf ^ 1)                                             // tile t + nb (or a clamped copy nobody reads)
        bl_n = load_bias(t + nb < t_last ? t + nb : t_last);
        K5D_LOAD(t + 2 * nb < t_last ? t + 2 * nb : t_last)
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        const unsigned* wl = wt + buf * 32 * LDW + j * LDW + 4 * hi;
#pragma unroll
        for (int s_ = 0; s_ < 8; ++s_) {
            const uint4 af = *reinterpret_cast<const uint4*>(wl + 8 * s_);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(af), as_bf16x8(hb[s_]), acc, 0, 0, 0);
        }
#pragma unroll
        for (int s_ = 8; s_ < 16; ++s_) {
            const uint4 af = *reinterpret_cast<const uint4*>(wl + 8 * s_);
            const uint4 bf = hq[((s_ - 8) * NW + wave) * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(af), as_bf16x8(bf), acc, 0, 0, 0);
        }
        // epilogue: lane (j, hi) holds, for playlist `row`, the columns t 32 + 4 hi + 8 qd + e; dz of columns past V and of
        // playlists past the batch is 0 (and not stored)
        float dzv[16];
        float q_min = 1.0f;
        const int tcol0 = t * 32 + 4 * hi;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // dae_train_sigmoid and dae_loss_neg_term (decode_common.h) WRITTEN OUT: through the functions hipcc schedules this
                // kernel differently (6 more scalar spills at its 256 registers; profiles/decode_split_notes.md) -- same operations
                const float zz = acc[4 * qd + e] + __shfl(bl, 4 * hi + 8 * qd + e);
                const float pr = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * zz));
                const float q = 1.0f - pr;
                const bool live = row_in && tcol0 + 8 * qd + e < p.V;
                loss_acc -= live ? (0.69314718f * 0.55f) * __builtin_amdgcn_logf(q + 1e-10f) : 0.0f;
                q_min = fminf(q_min, live ? q : 1.0f);
                dzv[4 * qd + e] = live ? k1 * pr : 0.0f;             // the short form (DAE_LOSS_SHORT_FORM_MIN_Q, decode_common.h)
            }
        }
        if (__builtin_expect(__ballot(q_min < DAE_LOSS_SHORT_FORM_MIN_Q) != 0ull, 0)) {   // (a logit above 10.5 somewhere in the wave: the exact form)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float zz = acc[4 * qd + e] + __shfl(bl, 4 * hi + 8 * qd + e);
                    const float pr = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * zz));
                    const float q = 1.0f - pr;
                    const bool live = row_in && tcol0 + 8 * qd + e < p.V;
                    if (live && q < DAE_LOSS_SHORT_FORM_MIN_Q) dzv[4 * qd + e] = k1 * __builtin_amdgcn_rcpf(q + 1e-10f) * pr * q;
                }
        }
        unsigned pk[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) pk[x] = K5D_PK(dzv[2 * x], dzv[2 * x + 1]);
        if (row_in) {
            unsigned short* const d16 = reinterpret_cast<unsigned short*>(p.dzT) + (size_t)t * 32 * p.ldT;
            const unsigned lane_off = (unsigned)(4 * hi) * (unsigned)p.ldT + (unsigned)row;
            if (t * 32 + 32 <= p.V) {
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int c = 8 * (x >> 1) + 2 * (x & 1);              // column offset of the pair's first element
                    (d16 + (size_t)c * p.ldT)[lane_off] = (unsigned short)(pk[x] & 0xFFFFu);
                    (d16 + (size_t)(c + 1) * p.ldT)[lane_off] = (unsigned short)(pk[x] >> 16);
                }
            } else {
#pragma unroll
                for (int x = 0; x < 8; ++x) {
                    const int c = 8 * (x >> 1) + 2 * (x & 1);
                    if (tcol0 + c < p.V) (d16 + (size_t)c * p.ldT)[lane_off] = (unsigned short)(pk[x] & 0xFFFFu);
                    if (tcol0 + c + 1 < p.V) (d16 + (size_t)(c + 1) * p.ldT)[lane_off] = (unsigned short)(pk[x] >> 16);
                }
            }
        }
        // dh[playlist][hidden] += dz[playlist][the tile's rows] W[rows][hidden]: A = dz (k-slot i of lane half hi, step s: row
        // 16 s + 4 hi + i for i < 4, + 8 + (i - 4) above), B = the transposed tile, block b of 32 hidden units
        const uint4 a0 = make_uint4(pk[0], pk[1], pk[2], pk[3]), a1 = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        const unsigned* tl = wt2 + buf * 256 * LDT + j * LDT + 4 * hi;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const uint2 x0 = *reinterpret_cast<const uint2*>(tl + b * 32 * LDT), x1 = *reinterpret_cast<const uint2*>(tl + b * 32 * LDT + 2);
            const uint2 y0 = *reinterpret_cast<const uint2*>(tl + b * 32 * LDT + 8), y1 = *reinterpret_cast<const uint2*>(tl + b * 32 * LDT + 10);
            dh[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a0), as_bf16x8(make_uint4(x0.x, x0.y, x1.x, x1.y)), dh[b], 0, 0, 0);
            dh[b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a1), as_bf16x8(make_uint4(y0.x, y0.y, y1.x, y1.y)), dh[b], 0, 0, 0);
        }
        bl = bl_n;
        __syncthreads();
    }
    // the workgroup's partial of dh: register reg of lane (j, hi), block b = playlist 32 wave + (reg & 3) + 8 (reg >> 2) + 4 hi,
    // hidden 32 b + j
    {
        float* pw = part + (size_t)blockIdx.x * Bpad64 * p.H;
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * hi;
                if (r < Bpad64) pw[(size_t)r * p.H + b * 32 + j] = dh[b][reg];
            }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) loss_acc += __shfl_xor(loss_acc, d);
    if (lane == 0) wsum[wave] = loss_acc;
    __syncthreads();
    if (tid == 0) {
        float sm = 0.0f;
        for (int w = 0; w < NW; ++w) sm += wsum[w];
        p.loss_part[blockIdx.x] = sm * p.inv_nb;
    }
}
#undef K5D_LOAD
#undef K5D_PK
#undef K5D_STAGE

// ---- K5, fp32 operands, hidden 256, batches of at most 256 playlists: the same shape on v_mfma_f32_32x32x2_f32 (round 6) ----
// The row-gathering fp32 kernel it replaces (64 cache lines per load instruction, as the 128-row bf16 kernel's): 219 us for
// 142 us of fp32 matrix work at the nominal clock; this one 209 us.  Here: a workgroup = a tile of 32 decoder rows x all playlists, the rows
// as plain 1 KB reads into LDS (fp32, 1 040-byte rows, two tiles in rotation), a wave = 32 playlists whose hidden row sits in
// 128 registers, the A fragments from LDS (a float4 = four MFMAs).  The k order inside a dot product is the row-major kernel's
// (pairs (8 g + c, 8 g + 4 + c)); training compares by tolerance.
__global__ __launch_bounds__(512, 1) void decode_loss_shared_f32_kernel(const LossRmP p)
{
    constexpr int NW = 8, LDW = 260;                                   // dwords per staged decoder row (256 + 4 of padding)
    extern __shared__ __attribute__((aligned(16))) float wtf[];       // [2][32 * LDW] | wsum[NW]
    float* const wsum = wtf + 2 * 32 * LDW;
    const int tid = threadIdx.x, lane = tid & 63, hi = lane >> 5, j = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row = wave * 32 + j;
    const int H4 = p.H >> 2;
    const float4* W4 = reinterpret_cast<const float4*>(p.W);
    const int n_tiles = (p.V + 31) >> 5;
    const int nb = gridDim.x;

    // hidden row of the lane's playlist: group g = k 8 g + 4 hi .. + 3 (zeros past the batch)
    float4 hb[32];
    {
        const float4* hr = reinterpret_cast<const float4*>(p.h) + (size_t)(row < p.B ? row : 0) * H4 + hi;
#pragma unroll
        for (int g = 0; g < 32; ++g) hb[g] = hr[2 * g];
        if (row >= p.B) {
#pragma unroll
            for (int g = 0; g < 32; ++g) hb[g] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // the wave's four rows of a tile, lane l holding floats 4 l .. 4 l + 3 of each: four named registers (an array behind a
    // lambda's reference stayed in scratch here)
    float4 w0, w1, w2, w3;
#define K5F_LOAD(T)                                                                            \
    {                                                                                          \
        const int v_ = (T) * 32 + 4 * wave;                                                    \
        w0 = W4[(size_t)(v_ < p.V ? v_ : p.V - 1) * H4 + lane];                                \
        w1 = W4[(size_t)(v_ + 1 < p.V ? v_ + 1 : p.V - 1) * H4 + lane];                        \
        w2 = W4[(size_t)(v_ + 2 < p.V ? v_ + 2 : p.V - 1) * H4 + lane];                        \
        w3 = W4[(size_t)(v_ + 3 < p.V ? v_ + 3 : p.V - 1) * H4 + lane];                        \
    }
#define K5F_STAGE(BUF)                                                                         \
    {                                                                                          \
        float* d_ = &wtf[(BUF) * 32 * LDW + (4 * wave) * LDW + 4 * lane];                      \
        *reinterpret_cast<float4*>(d_) = w0;                                                   \
        *reinterpret_cast<float4*>(d_ + LDW) = w1;                                             \
        *reinterpret_cast<float4*>(d_ + 2 * LDW) = w2;                                         \
        *reinterpret_cast<float4*>(d_ + 3 * LDW) = w3;                                         \
    }
    // the tile's 32 bias values, one per lane (lane l: column 32 t + (l & 31)); a lane takes its 16 by shuffle when it needs them
    auto load_bias = [&](int t) -> float {
        const int c = t * 32 + j;
        return p.bias[c < p.V ? c : p.V - 1];
    };
    float loss_acc = 0.0f;
    float bl, bl_n = 0.0f;
    int t = blockIdx.x;
    // (every request is UNCONDITIONAL, on a tile clamped to the last one: a conditionally written register array goes to scratch,
    // and the store to scratch waits for the load it has just issued)
    const int t_last = n_tiles - 1;
    K5F_LOAD(t < t_last ? t : t_last)
    bl = load_bias(t < t_last ? t : t_last);
    K5F_STAGE(0)
    K5F_LOAD(t + nb < t_last ? t + nb : t_last)
    __syncthreads();
    const bool rows_in = wave * 32 + 32 <= p.B;
    // (Tried: the second wave of each SIMD one tile late with its epilogue, so that one wave's MFMAs run under the other's
    // epilogue -- 214 against 209 us: the launch is not losing its time to coinciding phases.)
    auto epilogue = [&](int te, const f32x16& ac, float bv) {
            float4 bq[4];
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
                bq[qd] = make_float4(__shfl(bv, 4 * hi + 8 * qd), __shfl(bv, 4 * hi + 8 * qd + 1), __shfl(bv, 4 * hi + 8 * qd + 2),
                                     __shfl(bv, 4 * hi + 8 * qd + 3));
            if (te * 32 + 32 <= p.V && rows_in) {
                const unsigned lane_off = (unsigned)(4 * hi) * (unsigned)p.ldT + (unsigned)row;
                float* const d32 = p.dzT + (size_t)te * 32 * p.ldT;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float pr = dae_train_sigmoid(ac[4 * qd + e] + zb[e]);
                        loss_acc -= dae_loss_neg_term(pr);
                        (d32 + (size_t)(8 * qd + e) * p.ldT)[lane_off] = dae_loss_neg_dz(pr, p.inv_nb);
                    }
                }
            } else if (row < p.B) {
                const int tcol0 = te * 32 + 4 * hi;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int lc = tcol0 + 8 * qd;
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (lc + e < p.V) {
                            const float pr = dae_train_sigmoid(ac[4 * qd + e] + zb[e]);
                            loss_acc -= dae_loss_neg_term(pr);
                            p.dzT[(size_t)(lc + e) * p.ldT + row] = dae_loss_neg_dz(pr, p.inv_nb);
                        }
                    }
                }
            }
    };
    int buf = 0;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    for (; t < n_tiles; t += nb, buf ^= 1) {
        K5F_STAGE(buf ^ 1)                                             // tile t + nb (or a clamped copy nobody reads)
        bl_n = load_bias(t + nb < t_last ? t + nb : t_last);
        K5F_LOAD(t + 2 * nb < t_last ? t + 2 * nb : t_last)
        __builtin_amdgcn_sched_barrier(0);                             // (hipcc sinks these requests below the 128 MFMAs otherwise)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        const float* wl = &wtf[buf * 32 * LDW + j * LDW + 4 * hi];
        // (one accumulator: a chain of 128 dependent MFMAs per wave, and two -- even / odd groups, summed -- measured the same
        // 209 - 213 us: with two waves per SIMD the pipe is busy either way; the launch is at the fp32 MFMA rate of its clock)
#pragma unroll
        for (int g = 0; g < 32; ++g) {
            const float4 a = *reinterpret_cast<const float4*>(wl + 8 * g);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, hb[g].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, hb[g].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, hb[g].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, hb[g].w, acc, 0, 0, 0);
        }
        epilogue(t, acc, bl);
        bl = bl_n;
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) loss_acc += __shfl_xor(loss_acc, d);
    if (lane == 0) wsum[wave] = loss_acc;
    __syncthreads();
    if (tid == 0) {
        float sm = 0.0f;
        for (int w = 0; w < NW; ++w) sm += wsum[w];
        p.loss_part[blockIdx.x] = sm * p.inv_nb;
    }
}
#undef K5F_LOAD
#undef K5F_STAGE

// ---- fp32, hidden = 256, filter epilogue (phase B of the fused path): the generic kernel (decode_generic.hip) with
// one addition, TAIL BALANCE.  A launch of n tiles over n_ws wave slots runs floor(n / n_ws) whole rounds
// and a last round with `rem` tiles; when that round is at most half full (222 of 512 slots at batch 256,
// i.e. 10 rounds of time for 9.43 rounds of work) each of its tiles is split between TWO waves by row
// blocks (128 playlists -> 2 x 64), so the round costs half a tile time.  The k chain of every output is
// untouched (bit-exact), only which wave owns which row block changes.
template <int DUMMY>
__global__ __launch_bounds__(256, 1) void decode_f32_h256_filter_kernel(const dae_decp p)
{
    constexpr int RB = 4, G = 32, NW = 4, R_TILE = 128;
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;

    const int gs = DAE_NUM_XCD * p.n_rg;
    const int q = blockIdx.x / gs, rem_b = blockIdx.x % gs;
    const int rg = rem_b / DAE_NUM_XCD;
    const int bir = q * DAE_NUM_XCD + (rem_b % DAE_NUM_XCD);

    constexpr int n_h4 = RB * 64 * G;
    // SKIPPED TILES (score.hip topk_phase_b, prepack.hip live_tiles_kernel): with live lists the row group walks the tiles of
    // p.ts whose logit bound reaches the smallest threshold of its rows -- live_cnt[rg] of them, in p.ts's order -- and R, rem,
    // split and item_at below follow that count.  A tile left out holds no logit >= tau[row] for any row of the group: the
    // epilogue would have dropped every element of it.  No live tile: the workgroup's candidate counts are zero, nothing else
    // is read.
    const int* const tlist = p.live_cnt ? p.live_list + (size_t)rg * p.ts.n_items : p.ts.list;
    const int n_items = p.live_cnt ? __builtin_amdgcn_readfirstlane(p.live_cnt[rg]) : p.ts.n_items;
    if (n_items <= 0) {
        if (tid < R_TILE) p.cand_cnt[(size_t)bir * p.Bpad + rg * R_TILE + tid] = 0;
        return;
    }
    // this wave's work: whole tiles ws + r * n_ws (r < R), then possibly one tile -- or half of one -- of
    // the last round
    const int n_ws = p.nb_rg * NW;
    const int ws = wave * p.nb_rg + bir;
    const int R = n_items / n_ws, rem = n_items - R * n_ws;
    const bool split = rem > 0 && 2 * rem <= n_ws;
    const int n_it = R + (ws < (split ? 2 * rem : rem) ? 1 : 0);
    auto item_at = [&](int r) {
        r = r < n_it - 1 ? r : n_it - 1;
        r = r < 0 ? 0 : r;
        const int it = r < R ? ws + r * n_ws : R * n_ws + (split ? (ws >> 1) : ws);
        return it < n_items ? it : 0;
    };
    // the first two tile ids go out ahead of the hidden tile's loads, so that the W ring can start before the workgroup
    // meets (tile, barrier, ids, W was one more dependent trip to memory in front of the first MFMA)
    const int tv_cur = tlist[item_at(0)], tv_nxt = tlist[item_at(1)];
    {
        const float4* src = p.hp + (size_t)rg * n_h4;
        constexpr int NT = NW * 64;
#pragma unroll
        for (int i0 = 0; i0 < n_h4; i0 += 8 * NT) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[i0 + u * NT + tid];
#pragma unroll
            for (int u = 0; u < 8; ++u) lds4[i0 + u * NT + tid] = v[u];
        }
    }
    int* lcnt = reinterpret_cast<int*>(lds4 + n_h4);
    float* ltau = reinterpret_cast<float*>(lcnt + R_TILE);
    if (tid < R_TILE) {
        lcnt[tid] = 0;
        ltau[tid] = rg * R_TILE + tid < p.B ? p.tau[rg * R_TILE + tid] : __builtin_inff();
    }
    float4 wb0, wb1, wb2, wb3;
    float4 bA[RB], bB[RB];
    int t_cur = __builtin_amdgcn_readfirstlane(tv_cur), t_nxt = __builtin_amdgcn_readfirstlane(tv_nxt);
    {
        const float4* w0 = p.Wp + (size_t)t_cur * G * 64 + lane;     // (a wave without work reads a listed tile and drops it)
        wb0 = w0[0]; wb1 = w0[64]; wb2 = w0[128]; wb3 = w0[192];
    }
    __syncthreads();

    float tau_r[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) tau_r[rb] = ltau[rb * 32 + j];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) bA[rb] = lds4[rb * 64 + lane];

    for (int r = 0; r < n_it; ++r) {
        const int t = t_cur;
        const float4* wp = p.Wp + (size_t)t * G * 64 + lane;
        const float4* wn = p.Wp + (size_t)t_nxt * G * 64 + lane;
        const int t_nn_v = tlist[item_at(r + 2)];                     // two tiles ahead (see decode_f32_kernel)
        const float* bp = p.bias + (size_t)t * 32 + 4 * hi;
        float4 bq[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) bq[qd] = *reinterpret_cast<const float4*>(bp + 8 * qd);
        const int tcol0 = t * 32 + 4 * hi;
        const bool rankable = (t * 32 < p.ncols) && (p.col_lo + t * 32 < p.n_valid_col);

        // one tile over row blocks [R0, R0 + RN): GEMM with the 4-deep W ring, then the filter epilogue
        auto tile = [&](auto r0c, auto rnc) {
            constexpr int R0 = decltype(r0c)::value, RN = decltype(rnc)::value;
            f32x16 acc[RN];
#pragma unroll
            for (int i = 0; i < RN; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
#define DAE_STEPR(WB, PF, BC, BN, GNEXT)                                                              \
    {                                                                                                 \
        const float4 a = WB;                                                                          \
        WB = *(PF);                                                                                   \
        const float4* hl = lds4 + (size_t)(GNEXT) * (RB * 64) + lane;                                 \
        _Pragma("unroll") for (int i = 0; i < RN; ++i) BN[R0 + i] = hl[(R0 + i) * 64];                \
        __builtin_amdgcn_sched_barrier(0);                                                            \
        _Pragma("unroll") for (int i = 0; i < RN; ++i)                                                \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, BC[R0 + i].x, acc[i], 0, 0, 0);        \
        _Pragma("unroll") for (int i = 0; i < RN; ++i)                                                \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, BC[R0 + i].y, acc[i], 0, 0, 0);        \
        _Pragma("unroll") for (int i = 0; i < RN; ++i)                                                \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, BC[R0 + i].z, acc[i], 0, 0, 0);        \
        _Pragma("unroll") for (int i = 0; i < RN; ++i)                                                \
            acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, BC[R0 + i].w, acc[i], 0, 0, 0);        \
        __builtin_amdgcn_sched_barrier(0);                                                            \
    }
            int g = 0;
#pragma unroll
            for (; g < G - 4; g += 4) {
                const float4* pf = wp + (size_t)(g + 4) * 64;
                DAE_STEPR(wb0, pf,       bA, bB, g + 1)
                DAE_STEPR(wb1, pf + 64,  bB, bA, g + 2)
                DAE_STEPR(wb2, pf + 128, bA, bB, g + 3)
                DAE_STEPR(wb3, pf + 192, bB, bA, g + 4)
            }
            DAE_STEPR(wb0, wn,       bA, bB, g + 1)
            DAE_STEPR(wb1, wn + 64,  bB, bA, g + 2)
            DAE_STEPR(wb2, wn + 128, bA, bB, g + 3)
            // the next tile may own OTHER row blocks (a full tile's successor is never narrower than
            // ... a half tile is always last): fetch group 0 for ALL row blocks
            {
                const float4 a = wb3;
                wb3 = wn[192];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) bA[rb] = lds4[rb * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < RN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bB[R0 + i].x, acc[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < RN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bB[R0 + i].y, acc[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < RN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bB[R0 + i].z, acc[i], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < RN; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bB[R0 + i].w, acc[i], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
#undef DAE_STEPR
            if (!rankable) return;
#pragma unroll
            for (int i = 0; i < RN; ++i) {
                constexpr int dummy = 0; (void)dummy;
                const int rb = R0 + i;
                const float tv = tau_r[rb];
                float z[16];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    z[4 * qd + 0] = acc[i][4 * qd + 0] + bq[qd].x;
                    z[4 * qd + 1] = acc[i][4 * qd + 1] + bq[qd].y;
                    z[4 * qd + 2] = acc[i][4 * qd + 2] + bq[qd].z;
                    z[4 * qd + 3] = acc[i][4 * qd + 3] + bq[qd].w;
                }
                float mx = z[0];
#pragma unroll
                for (int e = 1; e < 16; ++e) mx = fmaxf(mx, z[e]);
                if (mx >= tv) {
                    unsigned m = 0;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int lc = tcol0 + (e & 3) + 8 * (e >> 2);
                        if (z[e] >= tv && lc < p.ncols && p.col_lo + lc < p.n_valid_col) m |= 1u << e;
                    }
                    if (m) {
                        const int rloc = rb * 32 + j;
                        int base = atomicAdd(&lcnt[rloc], __popc(m));
                        uint2* dst = p.cand + ((size_t)bir * p.Bpad + rg * R_TILE + rloc) * (size_t)p.cap;
#pragma unroll
                        for (int reg = 0; reg < 16; ++reg) {
                            if (m & (1u << reg)) {
                                const int lc = tcol0 + (reg & 3) + 8 * (reg >> 2);
                                dst[base++] = make_uint2(__float_as_uint(z[reg]), (unsigned)(p.col_lo + lc));
                            }
                        }
                    }
                }
            }
        };

        if (!(split && r == R)) tile(IntC<0>{}, IntC<RB>{});
        else if ((ws & 1) == 0) tile(IntC<0>{}, IntC<RB / 2>{});
        else tile(IntC<RB / 2>{}, IntC<RB / 2>{});

        t_cur = t_nxt;
        t_nxt = __builtin_amdgcn_readfirstlane(t_nn_v);
    }
    __syncthreads();
    if (tid < R_TILE) p.cand_cnt[(size_t)bir * p.Bpad + rg * R_TILE + tid] = lcnt[tid];
}

// ---- bf16, hidden = 256, filter epilogue (phase B of the fused path) --------------------------------
// A wave owns NT column tiles x RB row blocks.  Measured (profiles/r01_notes.md, us at batch 256 / 1024):
//   <NT = 1, RB = 4, ring 8, 2 waves per SIMD>  19.9 / 55.7   <- default: 4 accumulators per wave
//   <NT = 1, RB = 4, ring 16, 1 wave per SIMD>  23.9 / 65.3
//   <NT = 2, RB = 4, ring 16, 1 wave per SIMD>  25.6 / 61.5   (a hidden fragment feeds 2 MFMAs)
//   <NT = 1, RB = 8, ring 16, 1 wave per SIMD>  27.6 / 64.1   (256-row groups: W read once at batch 256)
//   3 and 4 waves per SIMD spill (168 / 128 registers) and are slower.
// A micro-benchmark of the inner pattern (scripts/micro/mfma_peak.hip: 4 accumulators, hidden fragments
// from LDS one step ahead, no global memory) reaches 2.3-2.4 PFLOP/s, so neither LDS nor the MFMA issue
// limits it; what the real kernel adds is the W ring, tile indices two groups ahead, the bias MFMA and the
// epilogue (a max-reduction and one compare per row block unless some lane really passes).
// ---- phase A for launches of many rows: per-WAVE group maxima, no exchange ---------------------------------------------------
// The generic phase-A kernel (decode_f32_kernel<4, EPI_GMAX, 16, 4, DT_BF16>) takes the maximum over the tiles the FOUR waves of a
// workgroup decode in a round: row block by row block through LDS, two barriers each, one wave per SIMD (468 registers) -- at
// 2 048 rows the sample (1 / 9 of the tiles) costs 40 us where the filter launch decodes everything in 113.  When a launch's
// sample gives every one of the filter kernel's wave slots (8 per workgroup) at least two tiles, the group can be the tiles ONE
// wave decodes: wave w of workgroup bir takes items w nb_rg + bir + r n_ws, r = 0, 1, ... -- in the plain bias order, so its tiles
// sit n_ws places apart (round r = popularity band r) -- and keeps the running maximum per (row, position in the tile) in
// registers: no LDS traffic beyond the hidden fragments, no barrier after the prologue, two waves per SIMD.  The structure of
// decode_bf16_h256_filter_kernel<1, 4, 8, 8> (same hidden tile, W ring, bias through the matrix pipe: the same logits bit for
// bit) with a static tile assignment and fmax as the epilogue.  Groups are disjoint sets of columns as before: the (k + seeds)-th
// largest of the 8 nb_rg x 32 maxima of a row is a valid threshold.  gmax[row][(wave nb_rg + bir) 32 + position].
__global__ __launch_bounds__(512, 1) void decode_bf16_h256_wavemax_kernel(const dae_decp p)
{
    constexpr int NS = 16, RB = 4, QR = 8, NW = 8;
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;
    const int gs = DAE_NUM_XCD * p.n_rg;
    const int q = blockIdx.x / gs, rem = blockIdx.x % gs;
    const int rg = rem / DAE_NUM_XCD;
    const int bir = q * DAE_NUM_XCD + (rem % DAE_NUM_XCD);
    constexpr int n_h4 = RB * 64 * NS;
    constexpr int NTH = NW * 64;
    constexpr int PER = n_h4 / NTH;                              // 8 uint4 of the hidden tile per thread
    const int n_items = p.ts.n_items;
    const int n_ws = p.nb_rg * NW;
    const int it0 = wave * p.nb_rg + bir;
    const uint4* Wq = reinterpret_cast<const uint4*>(p.Wp);
    const uint4* ldsq = reinterpret_cast<const uint4*>(lds4);
    const uint4 ones = bf16_ones_fragment(hi);
    const bool has = it0 < n_items;
    const int tv0 = tile_of_item(p.ts, has ? it0 : 0);
    const int tv1 = tile_of_item(p.ts, has ? (it0 + n_ws < n_items ? it0 + n_ws : it0) : 0);
    {
        const float4* hsrc = p.hp + (size_t)rg * n_h4;
        float4 hv[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) hv[e] = hsrc[e * NTH + tid];
#pragma unroll
        for (int e = 0; e < PER; ++e) lds4[e * NTH + tid] = hv[e];
    }
    __builtin_amdgcn_sched_barrier(0);
    int t = __builtin_amdgcn_readfirstlane(tv0), u = __builtin_amdgcn_readfirstlane(tv1);
    uint4 wq[QR];
    uint4 cb[2][RB];
    uint4 bfr = p.bias16[(size_t)t * 64 + lane];
#pragma unroll
    for (int k = 0; k < QR; ++k) wq[k] = Wq[(size_t)t * (NS * 64) + k * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) cb[0][rb] = ldsq[rb * 64 + lane];

    f32x16 mx[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx[rb][e] = -__builtin_inff();

    for (int it = it0; it < n_items; it += n_ws) {
        const int it_nn = it + 2 * n_ws;
        const int wv = tile_of_item(p.ts, it_nn < n_items ? it_nn : it);   // consumed at the end of this tile
        const uint4* cur = Wq + (size_t)t * (NS * 64);
        const uint4* nxt = Wq + (size_t)u * (NS * 64);
        f32x16 acc[RB];
        {
            f32x16 zero;
#pragma unroll
            for (int e = 0; e < 16; ++e) zero[e] = 0.0f;
            const uint4 bc = bfr;
            bfr = p.bias16[(size_t)u * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(bc), as_bf16x8(ones), zero, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sn = (s + 1) % NS;
            const uint4 a = wq[s % QR];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(cb[s & 1][rb]), acc[rb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                cb[(s + 1) & 1][rb] = ldsq[(sn * RB + rb) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
            }
            wq[s % QR] = (s + QR < NS) ? cur[(s + QR) * 64 + lane] : nxt[(s + QR - NS) * 64 + lane];
            __builtin_amdgcn_sched_barrier(0);
        }
        // register reg of the tile is column 32 t + (reg & 3) + 8 (reg >> 2) + 4 hi; columns that are not ranked never enter a maximum
        const bool whole = t * 32 + 31 < p.ncols && p.col_lo + t * 32 + 31 < p.mask_from_col;          // wave-uniform
        if (whole) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) mx[rb][reg] = fmaxf(mx[rb][reg], acc[rb][reg]);
        } else {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int lc = t * 32 + 4 * hi + (reg & 3) + 8 * (reg >> 2);
                const bool ok = lc < p.ncols && p.col_lo + lc < p.mask_from_col;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) mx[rb][reg] = ok ? fmaxf(mx[rb][reg], acc[rb][reg]) : mx[rb][reg];
            }
        }
        t = u; u = __builtin_amdgcn_readfirstlane(wv);
    }
    // a wave without a tile leaves -inf: absent for the threshold kernel
    if (p.gmax_per_wave == 4) {
        // few tiles per wave (1 024 rows: 2.3): waves w and w + 4 share a group -- ONE exchange at the end of the launch, through the
        // hidden tile's LDS (dead by now): 4 nb_rg x 32 maxima per row instead of 8 nb_rg x 32, so that the threshold kernel reads
        // 4 096, not 8 192 (its 16-key shape).  Groups of ~4.6 tiles from as many bands, as a wave's own tiles are at 2 048 rows.
        // (Pairing NEIGHBOURING positions instead doubles the candidates: in the hottest tiles every column is a winner.)
        __syncthreads();                                          // every wave is past its last hidden fragment
        float* xl = reinterpret_cast<float*>(lds4);
        if (wave >= 4) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd)
                    *reinterpret_cast<float4*>(xl + ((((wave - 4) * RB + rb) * 4 + qd) * 64 + lane) * 4) =
                        make_float4(mx[rb][4 * qd], mx[rb][4 * qd + 1], mx[rb][4 * qd + 2], mx[rb][4 * qd + 3]);
        }
        __syncthreads();
        if (wave >= 4) return;
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int row = rg * 128 + rb * 32 + j;
            float* gp = p.gmax + (size_t)row * p.ld_gmax + (size_t)(wave * p.nb_rg + bir) * 32 + 4 * hi;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const float4 o = *reinterpret_cast<const float4*>(xl + (((wave * RB + rb) * 4 + qd) * 64 + lane) * 4);
                if (row < p.B)
                    *reinterpret_cast<float4*>(gp + 8 * qd) = make_float4(fmaxf(mx[rb][4 * qd], o.x), fmaxf(mx[rb][4 * qd + 1], o.y),
                                                                          fmaxf(mx[rb][4 * qd + 2], o.z), fmaxf(mx[rb][4 * qd + 3], o.w));
            }
        }
        return;
    }
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int row = rg * 128 + rb * 32 + j;
        if (row >= p.B) continue;
        float* gp = p.gmax + (size_t)row * p.ld_gmax + (size_t)(wave * p.nb_rg + bir) * 32 + 4 * hi;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
            *reinterpret_cast<float4*>(gp + 8 * qd) = make_float4(mx[rb][4 * qd], mx[rb][4 * qd + 1], mx[rb][4 * qd + 2], mx[rb][4 * qd + 3]);
    }
}

template <int NT, int RB, int QR, int NW>
__global__ __launch_bounds__(NW * 64, 1) void decode_bf16_h256_filter_kernel(const dae_decp p)
{
    constexpr int NS = 16, R_TILE = RB * 32;
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;

    const int gs = DAE_NUM_XCD * p.n_rg;
    const int q = blockIdx.x / gs, rem = blockIdx.x % gs;
    const int rg = rem / DAE_NUM_XCD;
    const int bir = q * DAE_NUM_XCD + (rem % DAE_NUM_XCD);

    constexpr int n_h4 = RB * 64 * NS;
    constexpr int NTH = NW * 64;
    constexpr int PER = (n_h4 + NTH - 1) / NTH;                  // float4 of the hidden tile per thread
    constexpr int CH = PER < 8 ? PER : 8;                        // ... of which in flight at once
    const int n_items = p.ts.n_items;
    const int n_grp = (n_items + NT - 1) / NT;                   // groups of NT tiles
    const int n_ws = p.nb_rg * NW;
    const int grp0 = wave * p.nb_rg + bir;
    const uint4* Wq = reinterpret_cast<const uint4*>(p.Wp);      // uniform base; the lane is the index
    const uint4* ldsq = reinterpret_cast<const uint4*>(lds4);
    const uint4 ones = bf16_ones_fragment(hi);
    // item of (group, nt), clamped to the group's first item when the last group is ragged
    auto item_of = [&](int grp, int nt) { const int i = NT * grp + nt; return i < n_items ? i : NT * grp; };

    // ---- prologue: the requests that depend on nothing go out together (tile ids, thresholds, the hidden tile), the W
    // ring as soon as the ids are here and the tile has been handed to LDS -- it streams from HBM while the workgroup
    // meets.  The straight order (tile, barrier, thresholds, ids, W) was one more dependent trip to memory before the
    // first MFMA; keeping the tile's registers live across the ring's loads made the compiler park them in scratch.
    // WHICH groups a wave decodes: its first two by position (wave w: the w-th and the (NW + w)-th group of the workgroup's
    // share {bir + m nb_rg}), every further one CLAIMED from a counter in LDS, two groups ahead of its use.  A wave that
    // drew one of the hottest tiles of the bias-ordered list (nearly every value passes: 16 - 20 k cycles of appends against
    // 4 k for an ordinary tile, stage stamps) then simply takes fewer tiles, instead of setting the end of the
    // launch with the static share it had before (42 k cycles against 32 k for a workgroup without a hot tile).
    int t[NT], u[NT];                                            // tiles of this / the next group (uniform)
    int tv0[NT], tv1[NT];
    const bool has = grp0 < n_grp;
    {
        const int gn = grp0 + n_ws < n_grp ? grp0 + n_ws : grp0;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            tv0[nt] = tile_of_item(p.ts, has ? item_of(grp0, nt) : 0);
            tv1[nt] = tile_of_item(p.ts, has ? item_of(gn, nt) : 0);
        }
    }
    float tau_g[(R_TILE + NTH - 1) / NTH];
#pragma unroll
    for (int e = 0; e < (R_TILE + NTH - 1) / NTH; ++e) {
        const int i = e * NTH + tid;
        tau_g[e] = (i < R_TILE && rg * R_TILE + i < p.B) ? p.tau[rg * R_TILE + i] : __builtin_inff();
    }
    int* lcnt = reinterpret_cast<int*>(lds4 + n_h4);
    float* ltau = reinterpret_cast<float*>(lcnt + R_TILE);
    int* claim = reinterpret_cast<int*>(ltau + R_TILE);          // next unclaimed group of the workgroup (in units of nb_rg)
    if (tid == 0) *claim = 2 * NW;
    {
        const float4* hsrc = p.hp + (size_t)rg * n_h4;
#pragma unroll
        for (int e0 = 0; e0 < PER; e0 += CH) {
            float4 hv[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int i = (e0 + e) * NTH + tid;
                hv[e] = hsrc[i < n_h4 ? i : n_h4 - 1];            // unconditional: a guarded load would push hv[] to scratch
            }
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int i = (e0 + e) * NTH + tid;
                if (e0 + e < PER && i < n_h4) lds4[i] = hv[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < (R_TILE + NTH - 1) / NTH; ++e) {
        const int i = e * NTH + tid;
        if (i < R_TILE) { lcnt[i] = 0; ltau[i] = tau_g[e]; }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint4 wq[NT][QR];
    uint4 cb[2][RB];
    uint4 bfr[NT];                                               // bias fragments of the NEXT group
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        t[nt] = __builtin_amdgcn_readfirstlane(tv0[nt]);
        u[nt] = __builtin_amdgcn_readfirstlane(tv1[nt]);
    }
    // (unconditional: a wave without a tile reads tile list[0]'s fragments and never uses them)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bfr[nt] = p.bias16[(size_t)t[nt] * 64 + lane];
#pragma unroll
    for (int k = 0; k < QR; ++k)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wq[nt][k] = Wq[(size_t)t[nt] * (NS * 64) + k * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    float tau_r[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) tau_r[rb] = ltau[rb * 32 + j];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) cb[0][rb] = ldsq[rb * 64 + lane];

    int g_nxt = grp0 + n_ws;
    for (int grp = grp0; grp < n_grp;) {
        int g_nn;
        {
            int n2 = 0;
            if (lane == 0) n2 = atomicAdd(claim, 1);
            g_nn = __builtin_amdgcn_readfirstlane(n2) * p.nb_rg + bir;
        }
        const int gnn = g_nn < n_grp ? g_nn : grp;                // (a group that exists: its tile id is read, never used)
        int wv[NT];
        const uint4 *cur[NT], *nxt[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            wv[nt] = tile_of_item(p.ts, item_of(gnn, nt));        // consumed at the end of this group
            cur[nt] = Wq + (size_t)t[nt] * (NS * 64);
            nxt[nt] = Wq + (size_t)u[nt] * (NS * 64);
        }

        // the accumulators start at the bias (see bf16_ones_fragment)
        f32x16 acc[NT][RB];
        {
            f32x16 zero;
#pragma unroll
            for (int e = 0; e < 16; ++e) zero[e] = 0.0f;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const uint4 bc = bfr[nt];
                bfr[nt] = p.bias16[(size_t)u[nt] * 64 + lane];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
                    acc[nt][rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(bc), as_bf16x8(ones), zero, 0, 0, 0);
            }
        }

        // One wave per SIMD issues in order: a burst of loads in front of the MFMAs would leave the
        // matrix pipe idle while the burst issues.  So every MFMA (32 cycles in the pipe) is followed
        // by ONE memory instruction of the prefetch -- the next step's hidden fragments from LDS, then
        // the W fragments of step s + QR -- and sched_barrier pins that order.
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sn = (s + 1) % NS;
            uint4 a[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) a[nt] = wq[nt][s % QR];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    acc[nt][rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[nt]), as_bf16x8(cb[s & 1][rb]),
                                                                          acc[nt][rb], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    const int mi = nt * RB + rb;                      // MFMA index within the step
                    if (mi < RB) {                                    // next step's fragment rb = mi
                        cb[(s + 1) & 1][mi] = ldsq[(sn * RB + mi) * 64 + lane];
                    } else if (mi - RB < NT && (mi - RB) <= nt - 1) { // W of step s+QR for a tile already consumed
                        const int w = mi - RB;
                        wq[w][s % QR] = (s + QR < NS) ? cur[w][(s + QR) * 64 + lane] : nxt[w][(s + QR - NS) * 64 + lane];
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // W fragments not yet refilled (their tile's MFMAs of this step had to finish first)
#pragma unroll
            for (int w = 0; w < NT; ++w) {
                const bool done_inline = (NT * RB > RB + w) && (w <= ((RB + w) / RB) - 1);
                if (!done_inline)
                    wq[w][s % QR] = (s + QR < NS) ? cur[w][(s + QR) * 64 + lane] : nxt[w][(s + QR - NS) * 64 + lane];
            }
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- epilogue: lane = playlist j of row block rb; register reg of tile t is column
        // 32 t + (reg & 3) + 8 (reg >> 2) + 4 hi.  The tiles of this launch are the LOW-bias ones:
        // most hold no value above tau at all, so the common case is a max-reduction and one compare
        // per row block; masks, list slots (LDS atomic) and stores only where a lane really passes.
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const float tv = tau_r[rb];
            float mx = acc[0][rb][0];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) mx = fmaxf(mx, acc[nt][rb][reg]);
            if (mx >= tv) {
                unsigned m[NT];
                int cnt = 0;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    m[nt] = 0;
                    const bool live = NT * grp + nt < n_items;            // ragged last group
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int lc = t[nt] * 32 + 4 * hi + (reg & 3) + 8 * (reg >> 2);
                        if (live && acc[nt][rb][reg] >= tv && lc < p.ncols && p.col_lo + lc < p.n_valid_col)
                            m[nt] |= 1u << reg;
                    }
                    cnt += __popc(m[nt]);
                }
                if (cnt) {
                    int at = atomicAdd(&lcnt[rb * 32 + j], cnt);
                    uint2* dst = p.cand + ((size_t)bir * p.Bpad + rg * R_TILE + rb * 32 + j) * (size_t)p.cap;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const int cg = p.col_lo + t[nt] * 32 + 4 * hi;
                        // two neighbouring values that both pass leave as ONE 16-byte store: in the hottest tiles of the
                        // bias-ordered list nearly every value passes, and their 16 scattered 8-byte stores per lane and row
                        // block made those tiles cost 21 k cycles against 4 k (profiles/r03_notes.md) -- the launch's tail
#pragma unroll
                        for (int reg = 0; reg < 16; reg += 2) {
                            const unsigned two = (m[nt] >> reg) & 3u;
                            const uint2 e0 = make_uint2(__float_as_uint(acc[nt][rb][reg]), (unsigned)(cg + (reg & 3) + 8 * (reg >> 2)));
                            const uint2 e1 = make_uint2(__float_as_uint(acc[nt][rb][reg + 1]),
                                                        (unsigned)(cg + ((reg + 1) & 3) + 8 * ((reg + 1) >> 2)));
                            if (two == 3u) {
                                *reinterpret_cast<uint4*>(dst + at) = make_uint4(e0.x, e0.y, e1.x, e1.y);
                                at += 2;
                            } else if (two == 1u) {
                                dst[at++] = e0;
                            } else if (two == 2u) {
                                dst[at++] = e1;
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { t[nt] = u[nt]; u[nt] = __builtin_amdgcn_readfirstlane(wv[nt]); }
        grp = g_nxt; g_nxt = g_nn;
    }
    __syncthreads();
    for (int i = tid; i < R_TILE; i += NW * 64) p.cand_cnt[(size_t)bir * p.Bpad + rg * R_TILE + i] = lcnt[i];
}

// (The variant with the hidden tile in REGISTERS for MFMA-bound batches measured slower and is not kept: profiles/r04_notes.md 6.)

int fill_common(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts, dae_decp& p,
                int dtype = DAE_DTYPE_F32, int bias_sel = 0)
{
    const dae_packed& pk = dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16;
    const dae_buf& hb = dtype == DAE_DTYPE_F32 ? ctx->h_packed : ctx->h_packed16;
    if (!pk.valid) return dae_fail(ctx, DAE_ERR_STATE, "decoder not prepacked (dtype %d)", dtype);
    if (!hb.p) return dae_fail(ctx, DAE_ERR_STATE, "hidden tile not packed");
    memset(&p, 0, sizeof(p));
    p.Wp = static_cast<const float4*>(pk.W.p);
    p.bias = static_cast<const float*>(pk.bias.p);
    p.bias16 = static_cast<const uint4*>(pk.bias16.p);
    if (bias_sel) {                                        // DAE_DTYPE_BF16_EXACT: bounds instead of the logits
        if (dtype != DAE_DTYPE_BF16 || !pk.exact)
            return dae_fail(ctx, DAE_ERR_STATE, "decoder not prepacked with DAE_DTYPE_BF16_EXACT");
        p.bias16 = static_cast<const uint4*>(bias_sel == 1 ? pk.bias16_lo.p : pk.bias16_hi.p);
    }
    p.hp = static_cast<const float4*>(hb.p);
    p.G = dtype == DAE_DTYPE_F32 ? pk.Hp / DAE_KG : pk.Hp / 16;
    p.ncols = pk.col_hi - pk.col_lo;
    p.col_lo = pk.col_lo;
    p.B = B; p.n_rg = g.n_rg; p.nb_rg = g.nb_rg; p.Bpad = g.Bpad;
    p.ts = ts;
    p.mixT = ctx->mixT; p.mix_ld = ctx->mix_ld; p.mix_w = ctx->mix_w; p.mix_ncols = ctx->mix_ncols;      // dae_set_score_mix (GMAX / FILTER epilogues)
    return DAE_OK;
}

}  // namespace

// (which kernel a geometry takes: the predicates of score_plan.h, shared with the plan of a scoring call)
int dae_launch_decode_dense_f32(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts,
                                int apply_sigmoid, int mask_from_col, float* out, int64_t ld,
                                int fill_pad, int dtype, float* gmax, int64_t ld_gmax, int gmax_per_wave, int bias_sel,
                                const dae_sample_skip* skip)
{
    dae_decp p;
    int rc = fill_common(ctx, g, B, ts, p, dtype, bias_sel);
    if (rc) return rc;
    p.out = out; p.ld = ld; p.apply_sigmoid = apply_sigmoid; p.mask_from_col = mask_from_col;
    p.gmax = gmax; p.ld_gmax = ld_gmax; p.gmax_per_wave = gmax_per_wave;
    if (!out && !gmax) return dae_fail(ctx, DAE_ERR_ARG, "dense decode without an output");
    // fill_pad: the (internal) buffer covers whole tiles; columns past the image get -inf
    p.fill_pad = (out && fill_pad && ld >= (int64_t)ts.n_items * 32) ? 1 : 0;
    p.vec_ok = ((ld % 4) == 0 && (reinterpret_cast<uintptr_t>(out) % 16) == 0) ? 1 : 0;
    const int dt = dtype == DAE_DTYPE_F32 ? DT_F32 : DT_BF16;
    if (gmax && (gmax_per_wave == 3 || gmax_per_wave == 4)) {
        // per-wave group maxima (the caller sized gmax for 8 wave slots per workgroup: dae_sample_wave_groups)
        if (dtype != DAE_DTYPE_BF16 || out || p.G != 16 || g.R_TILE != 128 || p.mixT)
            return dae_fail(ctx, DAE_ERR_ARG, "per-wave group maxima: bf16, hidden 256, 128-row groups, maxima only");
        const size_t lds = (size_t)4 * 64 * 16 * sizeof(float4);
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_bf16_h256_wavemax_kernel, 160 * 1024));
        hipLaunchKernelGGL(decode_bf16_h256_wavemax_kernel, dim3(g.grid), dim3(512), lds, ctx->stream, p);
        DAE_CHECK_LAUNCH(ctx, "decode_bf16_h256_wavemax_kernel");
        return DAE_OK;
    }
    if (gmax) {
        if (g.waves != 4) return dae_fail(ctx, DAE_ERR_ARG, "group maxima need 4-wave workgroups");
        if (dae_sample_takes_half(g, dtype, p.G * DAE_KG, p.mixT != nullptr, gmax_per_wave, ts.n_items)) {
            if (skip) p.sk = *skip;                            // (tiles a bound puts below tau: the kernel's prologue)
            return dae_launch_decode_gmax_half(ctx, g, p);     // one round of tiles (the threshold sample at batch <= 256)
        }
        // (a table nobody writes would be read by the threshold launch: the plan gives one to the half-row-group sample only)
        if (skip && skip->tab) return dae_fail(ctx, DAE_ERR_STATE, "a decoded-tile table for a sample launch that is not in half row groups");
        return dae_launch_decode_generic(ctx, EPI_GMAX, dt, g, p);
    }
    return dae_launch_decode_generic(ctx, EPI_DENSE, dt, g, p);
}

// DAE term of the title mix: outT[c * ldT + r] = sigmoid(logit[r, c]) * row_scale[r] for the first n_items tiles
// (add: outT[c * ldT + r] + that, the read-modify-write instances of the kernel -- a further member of an ensemble)
int dae_launch_decode_scaled_T(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts, const float* row_scale,
                               float* outT, int64_t ldT, int dtype, bool add)
{
    dae_decp p;
    int rc = fill_common(ctx, g, B, ts, p, dtype);
    if (rc) return rc;
    p.mixT = nullptr;
    p.outT = outT; p.ld_outT = ldT; p.row_scale = row_scale; p.mask_from_col = INT_MAX;
    return dae_launch_decode_generic(ctx, add ? EPI_TERM_ADD : EPI_DENSE, dtype == DAE_DTYPE_F32 ? DT_F32 : DT_BF16, g, p);
}

// K5 from the row-major decoder (fp32, hidden = 256, 128-row groups); returns DAE_ERR_STATE when the shape does not apply
int dae_launch_decode_loss_rowmajor(dae_ctx* ctx, const dae_rowgeom& g, int B, int V, int H, const float* W,
                                    const float* bias, const float* h, float inv_n_batch, float* dzT, int64_t ldT,
                                    float* loss_part)
{
    if (H != 256 || g.R_TILE != 128 || g.waves != 4) return DAE_ERR_STATE;
    if ((uint64_t)ldT * 4 + (uint64_t)g.Bpad >= (1ull << 30)) return DAE_ERR_STATE;          // (32-bit lane offsets in the epilogues)
    LossRmP p;
    p.W = W; p.bias = bias; p.h = h; p.V = V; p.H = H; p.B = B; p.n_rg = g.n_rg; p.nb_rg = g.nb_rg;
    p.inv_nb = inv_n_batch; p.dzT = dzT; p.ldT = ldT; p.loss_part = loss_part;
    if (B > 256) return DAE_ERR_STATE;
    const size_t lds_s = ((size_t)2 * 32 * 260 + 8) * sizeof(float);
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_loss_shared_f32_kernel, lds_s));
    hipLaunchKernelGGL(decode_loss_shared_f32_kernel, dim3(g.grid), dim3(512), lds_s, ctx->stream, p);
    DAE_CHECK_LAUNCH(ctx, "decode_loss_shared_f32_kernel");
    return DAE_OK;
}

// K5 + K7 fused (decode_loss_dh_bf16_kernel): g.grid partials of dh at `part` ([g.grid][Bpad64][H]); DAE_ERR_STATE when the shape does not apply
int dae_launch_decode_loss_dh(dae_ctx* ctx, const dae_rowgeom& g, int B, int V, int H, const float* W, const float* bias,
                              const float* h, float inv_n_batch, float* dzT, int64_t ldT, float* loss_part, float* part, int Bpad64)
{
    if (H != 256 || B > 256 || g.R_TILE != 128 || g.waves != 4) return DAE_ERR_STATE;
    if ((uint64_t)ldT * 4 + (uint64_t)g.Bpad >= (1ull << 30)) return DAE_ERR_STATE;
    LossRmP p;
    p.W = W; p.bias = bias; p.h = h; p.V = V; p.H = H; p.B = B; p.n_rg = g.n_rg; p.nb_rg = g.nb_rg;
    p.inv_nb = inv_n_batch; p.dzT = dzT; p.ldT = ldT; p.loss_part = loss_part;
    const size_t lds = ((size_t)2 * 32 * 132 + (size_t)2 * 256 * 18) * 4 + (size_t)8 * 8 * 64 * 16 + 64;
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_loss_dh_bf16_kernel, lds));
    hipLaunchKernelGGL(decode_loss_dh_bf16_kernel, dim3(g.grid), dim3(512), lds, ctx->stream, p, part, Bpad64);
    DAE_CHECK_LAUNCH(ctx, "decode_loss_dh_bf16_kernel");
    return DAE_OK;
}

int dae_launch_decode_loss_f32(dae_ctx* ctx, const dae_rowgeom& g, int B, float inv_n_batch,
                               float* dzT, int64_t ldT, float* loss_part, int dtype, int dz16)
{
    dae_decp p;
    const dae_packed& pk = dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16;
    dae_tileset ts{pk.ntiles, 1, 0, static_cast<const int*>(pk.ident.p)};
    int rc = fill_common(ctx, g, B, ts, p, dtype);
    if (rc) return rc;
    p.dzT = dzT; p.ldT = ldT; p.loss_part = loss_part; p.inv_nb = inv_n_batch;
    p.dz16 = (dtype == DAE_DTYPE_BF16 && dz16) ? 1 : 0;
    // (hidden 256 in 128-row groups takes the row-major K5 launches above: train.hip train_plan `rm`)
    return dae_launch_decode_generic(ctx, EPI_LOSS, dtype == DAE_DTYPE_BF16 ? DT_BF16 : DT_F32, g, p);
}

int dae_launch_decode_rowloss(dae_ctx* ctx, const dae_rowgeom& g, int B, int dtype, float* row_part)
{
    dae_decp p;
    const dae_packed& pk = dtype == DAE_DTYPE_F32 ? ctx->pk_f32 : ctx->pk_bf16;
    dae_tileset ts{pk.ntiles, 1, 0, static_cast<const int*>(pk.ident.p)};      // every tile, the artists' included
    int rc = fill_common(ctx, g, B, ts, p, dtype);
    if (rc) return rc;
    p.mixT = nullptr;
    p.loss_part = row_part;
    return dae_launch_decode_generic(ctx, EPI_ROWLOSS, dtype == DAE_DTYPE_BF16 ? DT_BF16 : DT_F32, g, p);
}

int dae_launch_decode_mixrowloss(dae_ctx* ctx, const dae_rowgeom& g, int B, const float* mixT, int64_t mix_ld, const float* mix_w,
                                 float* row_part)
{
    dae_decp p;
    const dae_packed& pk = ctx->pk_f32;
    dae_tileset ts{pk.ntiles, 1, 0, static_cast<const int*>(pk.ident.p)};      // every tile, the artists' included
    int rc = fill_common(ctx, g, B, ts, p, DAE_DTYPE_F32);
    if (rc) return rc;
    // the call's own term buffer and weights: what dae_set_score_mix left in the context is neither read nor changed
    p.mixT = mixT; p.mix_ld = mix_ld; p.mix_w = mix_w; p.mix_ncols = pk.col_hi;
    p.loss_part = row_part;
    return dae_launch_decode_generic(ctx, EPI_MIXROWLOSS, DT_F32, g, p);
}

int dae_launch_decode_filter_f32(dae_ctx* ctx, const dae_rowgeom& g, int B, const dae_tileset& ts,
                                 const float* tau, int n_valid_col, uint2* cand, int* cand_cnt,
                                 int cap, int dtype, int bias_sel, const int* live_cnt, const int* live_list)
{
    dae_decp p;
    int rc = fill_common(ctx, g, B, ts, p, dtype, bias_sel);
    if (rc) return rc;
    p.tau = tau; p.n_valid_col = n_valid_col; p.cand = cand; p.cand_cnt = cand_cnt; p.cap = cap;
    if (live_cnt && !dae_filter_takes_live(g, dtype, p.G * DAE_KG, p.mixT != nullptr))
        return dae_fail(ctx, DAE_ERR_ARG, "live tile lists: the fp32 hidden-256 filter launch only");
    p.live_cnt = live_cnt; p.live_list = live_list;
    if (dae_filter_takes_live(g, dtype, p.G * DAE_KG, p.mixT != nullptr)) {
        const size_t lds = (size_t)4 * 64 * 32 * sizeof(float4) + 128 * sizeof(int) + 128 * sizeof(float);
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_f32_h256_filter_kernel<0>, 160 * 1024));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        dae_take_profile_events(ctx, "decode_f32_h256_filter_kernel<0>", e0, e1);
        hipExtLaunchKernelGGL(decode_f32_h256_filter_kernel<0>, dim3(g.grid), dim3(256), lds, ctx->stream, e0, e1, 0, p);
        DAE_CHECK_LAUNCH(ctx, "decode_f32_h256_filter_kernel");
        return DAE_OK;
    }
    if (bf16_fast_filter(g, dtype, p.G) && !p.mixT) {
        const size_t lds = (size_t)(g.R_TILE / 32) * 64 * 16 * sizeof(float4) + (size_t)g.R_TILE * (sizeof(int) + sizeof(float)) + 16;     // (+ the claim counter)
        DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_bf16_h256_filter_kernel<1, 4, 8, 8>, 160 * 1024));
        hipEvent_t e0 = nullptr, e1 = nullptr;
        dae_take_profile_events(ctx, "decode_bf16_h256_filter_kernel<1, 4, 8, 8>", e0, e1);
        hipExtLaunchKernelGGL((decode_bf16_h256_filter_kernel<1, 4, 8, 8>), dim3(g.grid), dim3(512), lds,
                              ctx->stream, e0, e1, 0, p);
        DAE_CHECK_LAUNCH(ctx, "decode_bf16_h256_filter_kernel");
        return DAE_OK;
    }
    return dae_launch_decode_generic(ctx, EPI_FILTER, dtype == DAE_DTYPE_F32 ? DT_F32 : DT_BF16, g, p);
}
