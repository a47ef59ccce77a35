// train.hip -- the training step of the reference graph (models/DAEs.py:98-102; SURVEY.md 8a
// rows a8-a10, App. B.5), fp32 on the CDNA4 matrix cores (bf16 operands for the three GEMMs under
// dae_set_train_dtype, BASELINE.json configs[3]):
//
//   forward   K1 encode with dropout (encode.hip) -> K5 decode GEMM whose epilogue turns logits
//             into the weighted-BCE loss and dL/dz, every element taken as a negative
//             (decode_f32.hip; decode_generic.hip EPI_LOSS), writing dz^T [V,B]; loss_fixup_kernel redoes the positives
//             of the target CSR (no dense target matrix)
//   K6        gW_dec[v,:] = sum_r dz[r,v] h[r,:]   (+ gb_dec = column sums)      contraction B   (grad_wdec.hip)
//   K7        dh[r,:]     = sum_v dz[r,v] W_dec[v,:]  split over V, partials reduced   contraction V
//   K8        dpre = dh * dropout-mask/kp * s(1-s); gb_enc; gW_enc[c,:] += xhat[r,c] dpre[r,:]
//   K9        TF1 Adam, dense (moments decay on zero-gradient rows too)                            (adam.hip)
//
// This file: the three step entry points and their planning (TrainPlan), loss_fixup_kernel, K7, K8 and the small kernels.
// K7 (grad_hidden_kernel) uses v_mfma_f32_32x32x2_f32 (one 32x32x16 bf16 MFMA per 8 k-steps under dae_set_train_dtype) with
// operands read in their natural row-major layouts because the contraction index is the slow dimension of both; the 4 (2)
// tiles a wave owns along the hidden dimension are interleaved (hidden = hc0 + 4 i + a) so that one float4 (float2) per lane
// feeds 4 (2) MFMAs.  Which MFMA operand the hidden unit is differs by instance (NA = 4 and the transposed K6 forms put it
// on the lane, the others on the register).  Summation orders differ from the oracle's float64 reference: parity is by
// tolerance (tests/test_gpu_train.py), not bitwise.
#include "train_common.h"

namespace {

// eight floats -> the 8 k-slots a lane holds of one 32x32x16 bf16 MFMA operand
__device__ __forceinline__ bf16x8_t pk_bf16x8(float a0, float a1, float a2, float a3, float a4, float a5, float a6,
                                              float a7)
{
    return __builtin_bit_cast(bf16x8_t, make_uint4(pk_bf16(a0, a1), pk_bf16(a2, a3), pk_bf16(a4, a5), pk_bf16(a6, a7)));
}

// ---- the positives of the loss -----------------------------------------------------------------------
// K5 (decode_f32.hip; decode_generic.hip EPI_LOSS) treats all B x V elements as negatives.  A batch holds ~100 positives per row
// out of 170 000 columns, so instead of a dense [B, V] target matrix (174 MB zeroed, scattered into and read
// back per step) each target entry (row, col, y) is redone here: the same logit -- the fmaf chain over
// k = 0..H-1 from +0, then + bias, which is what the fp32 MFMA computes -- then the full loss term and
// dL/dz of DAEs.py:98-99; dL/dz OVERWRITES K5's value and the loss partial holds L(y) - L(0).
// One workgroup per row (h row in LDS), one thread per target entry.  The target CSR holds one entry per
// (row, col) (include/dae_hip.h: the CSR contract), so no two threads own the same element.
constexpr int FIX_MAXH = 1024;
// BF16: the forward GEMM ran on bf16 operands (dae_set_train_dtype): W and h are rounded the same way here
// DZ16: dL/dz is kept as bf16 (the bf16 backward GEMMs read it as such)
// CORR (with BF16 and DZ16: the forward launch has already folded dh = dz W_dec into itself with every element a negative):
// the row's dh correction sum_i (bf16(dz_i) - bf16(dz_i as a negative)) bf16(W_dec[v_i]) goes out as one more partial
// (corr_out[row][k]); the value the forward launch stored is read back before it is overwritten, so the difference is exact.
template <bool BF16, bool DZ16 = false, bool CORR = false>
__global__ __launch_bounds__(256) void loss_fixup_kernel(const int32_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, int B, int H,
                                                         int col_lo, int col_hi,
                                                         const float* __restrict__ h,      // [B, H] after dropout
                                                         const float* __restrict__ Wd,     // [col_hi - col_lo, H]
                                                         const float* __restrict__ bias,   // local column index
                                                         float inv_nb, float* __restrict__ dzT, int64_t ldT,
                                                         float* __restrict__ loss_part, float* __restrict__ corr_out = nullptr)
{
    __shared__ float4 sh[FIX_MAXH / 4];
    __shared__ float wsum[4];
    constexpr int CCAP = CORR ? 1024 : 1;
    __shared__ float cdel[CCAP];
    __shared__ int ccol[CCAP];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int H4 = H >> 2;
    for (int i = tid; i < H4; i += 256) {
        float4 v = reinterpret_cast<const float4*>(h + (size_t)row * H)[i];
        if (BF16) v = make_float4(dae_bf16_value(v.x), dae_bf16_value(v.y), dae_bf16_value(v.z), dae_bf16_value(v.w));
        sh[i] = v;
    }
    __syncthreads();
    float corr = 0.0f;
    // CORR: the row's entries go in windows of CCAP (a row may be of any length): a window's (cdel, ccol) are staged in LDS, then
    // summed into the correction; wave g takes the entries g, g + 4, ... of the row across all windows (CCAP % 4 == 0), each lane
    // its hidden quads k4 = lane + 64 j in registers, so the sums run in entry order whatever the row's length
    constexpr int KJ = CORR ? FIX_MAXH / 256 : 1;
    float4 cacc_r[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) cacc_r[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    const int wlen = CORR ? CCAP : end - beg;
    for (int w0 = beg; w0 < end; w0 += wlen) {
        const int wend = min(w0 + wlen, end);
        for (int i = w0 + tid; i < wend; i += 256) {
            const int c = col[i];
            if (c < col_lo || c >= col_hi) {
                if (CORR) { cdel[i - w0] = 0.0f; ccol[i - w0] = 0; }      // (another shard's entry: nothing to correct)
                continue;
            }
            const int lc = c - col_lo;
            const float y = val[i];
            const float4* w = reinterpret_cast<const float4*>(Wd + (size_t)lc * H);
            const float z = dae_positive_logit<BF16>(w, sh, H4, bias + lc);          // train_common.h: THE positives' chain
            const float dzv = dae_loss_head(dae_train_sigmoid(z), y, inv_nb, corr);
            if (DZ16) {
                unsigned short* dst = reinterpret_cast<unsigned short*>(dzT) + (size_t)lc * ldT + row;
                const unsigned short nw = (unsigned short)(pk_bf16(dzv, 0.0f) & 0xFFFFu);
                if (CORR) { cdel[i - w0] = __uint_as_float((unsigned)nw << 16) - __uint_as_float((unsigned)*dst << 16); ccol[i - w0] = lc; }
                *dst = nw;
            } else dzT[(size_t)lc * ldT + row] = dzv;
        }
        if (CORR) {
            // wave g takes the window's entries g, g + 4, ... (a lane = four hidden units: plain 1 KB row reads, 8 in flight)
            const int n = wend - w0;
            __syncthreads();
            const int wv_ = tid >> 6, ln_ = tid & 63;
#pragma unroll
            for (int j = 0; j < KJ; ++j) {
                const int k4 = ln_ + 64 * j;
                if (k4 >= H4) break;
                float4 a = cacc_r[j];
                int e = wv_;
                for (; e + 28 < n; e += 32) {
                    float4 wv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) wv[u] = reinterpret_cast<const float4*>(Wd + (size_t)ccol[e + 4 * u] * H)[k4];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float d = cdel[e + 4 * u];
                        a.x = fmaf(d, dae_bf16_value(wv[u].x), a.x); a.y = fmaf(d, dae_bf16_value(wv[u].y), a.y);
                        a.z = fmaf(d, dae_bf16_value(wv[u].z), a.z); a.w = fmaf(d, dae_bf16_value(wv[u].w), a.w);
                    }
                }
                for (; e < n; e += 4) {
                    const float4 w1 = reinterpret_cast<const float4*>(Wd + (size_t)ccol[e] * H)[k4];
                    const float d = cdel[e];
                    a.x = fmaf(d, dae_bf16_value(w1.x), a.x); a.y = fmaf(d, dae_bf16_value(w1.y), a.y);
                    a.z = fmaf(d, dae_bf16_value(w1.z), a.z); a.w = fmaf(d, dae_bf16_value(w1.w), a.w);
                }
                cacc_r[j] = a;
            }
            __syncthreads();                                           // (the next window restages cdel / ccol)
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) corr += __shfl_xor(corr, d);
    if ((tid & 63) == 0) wsum[tid >> 6] = corr;
    __syncthreads();
    if (tid == 0) loss_part[row] = (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * inv_nb;
    if (CORR) {
        // the four waves' sums meet in LDS and are added in wave order: a fixed order, whatever the timing
        float4* const cacc = sh;                                    // (the hidden row is no longer needed: [4][H / 4] float4 fit)
        const int wv_ = tid >> 6, ln_ = tid & 63;
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
            const int k4 = ln_ + 64 * j;
            if (k4 < H4) cacc[wv_ * (FIX_MAXH / 16) + k4] = cacc_r[j];
        }
        __syncthreads();
        for (int k4 = tid; k4 < H4; k4 += 256) {
            const float4 p0 = cacc[k4], p1 = cacc[(FIX_MAXH / 16) + k4], p2 = cacc[2 * (FIX_MAXH / 16) + k4], p3 = cacc[3 * (FIX_MAXH / 16) + k4];
            reinterpret_cast<float4*>(corr_out + (size_t)row * H)[k4] =
                make_float4(((p0.x + p1.x) + p2.x) + p3.x, ((p0.y + p1.y) + p2.y) + p3.y, ((p0.z + p1.z) + p2.z) + p3.z,
                            ((p0.w + p1.w) + p2.w) + p3.w);
        }
    }
}

// ---- K7: dh partial [chunk][r][hc] = sum_{v in chunk} dzT[v, r] * W[v, hc] -----------------------
// a wave owns one (hidden half of 128, 64 playlists) output tile for one chunk of V: 8 accumulators;
// A = W rows (float4 per lane: hc0 + 4 i + a), B = dz^T rows (float2 per lane: r0 + 2 j + b); no LDS.
struct DhP {
    const float* dzT; int64_t ldT;     // [V, ldT]  (ldT >= Bpad64)
    const float* W; int H, V;
    float* part;                       // [n_chunk][Bpad64][H]
    int n_chunk, chunk, Bpad64, n_half, n_rblk;
    int fast32;                        // W and dz^T both end below 4 GB: whole chunks take 32-bit byte offsets from the matrix base
};

// BF16 (dae_set_train_dtype, NA = 4 only; dz^T is then stored as bf16, TrainPlan::dz16): the 8 k-steps of a block (16
// vocabulary rows) become ONE v_mfma_f32_32x32x16_bf16 per accumulator: k-slot x of lane half hi is row V0 + 2x + hi in both
// operands; a lane's two playlists (r0 + 2j, r0 + 2j + 1) of a dz^T row are one dword.
template <int NA, bool BF16 = false>
__global__ __launch_bounds__(256, 1) void grad_hidden_kernel(const DhP p)
{
    constexpr int HW = 32 * NA;
    const int lane = threadIdx.x & 63, hi = lane >> 5, j = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_out = p.n_half * p.n_rblk;
    const int total = n_out * p.n_chunk;
    // (Round 6, settled with scripts/probe/fetch_calib.hip: this launch really pulls 430 - 474 MB through the fabric for 261 MB
    // algorithmic -- every W row leaves HBM twice.  A chunk's eight output tiles are two workgroups; dealing the pair to ONE XCD
    // (blocks b, b + 8) changed nothing (FETCH_SIZE 215 113 KB before and after): an XCD streams 16 chunks of 1.36 MB at once
    // through 4 MB of L2, the partner's lines are gone before it arrives.  Reading W once needs the eight tiles in one workgroup
    // with the W block shared through LDS -- not built.)
    for (int w = blockIdx.x * 4 + wave; w < total; w += gridDim.x * 4) {
        const int ot = w % n_out, ch = w / n_out;      // neighbours share the W chunk
        // the four waves of a workgroup take the playlist blocks of ONE hidden half (n_rblk = 4: the shipped batch of 256), so
        // every W byte is read by one workgroup only -- its waves ask for the same lines within a few hundred cycles
        const int half = ot / p.n_rblk, rblk = ot % p.n_rblk;
        const int hc0 = half * HW, r0 = rblk * 64;
        const int v_beg = ch * p.chunk;
        int v_end = v_beg + p.chunk;
        if (v_end > p.V) v_end = p.V;
        f32x16 acc[NA][2];
#pragma unroll
        for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.0f;
        // (byte offsets, 32 bits: the launcher takes the fast form only when both matrices lie below 4 GB)
        const unsigned w_row = (unsigned)p.H * 4u, d_row = (unsigned)p.ldT * (BF16 ? 2u : 4u);
        const unsigned lane_w = (unsigned)(hc0 + NA * j) * 4u + (unsigned)hi * w_row;
        const unsigned lane_d = (unsigned)(r0 + 2 * j) * (BF16 ? 2u : 4u) + (unsigned)hi * d_row;
        const float* Wl = p.W + hc0 + NA * j;
        const float* Dl = p.dzT + r0 + 2 * j;
        const unsigned short* Dl16 = reinterpret_cast<const unsigned short*>(p.dzT) + r0 + 2 * j;
        // 16 vocabulary rows (8 k-steps, 64 MFMAs) per block, two register sets: the loads of block n+1 are
        // issued before the MFMAs of block n (one wave per SIMD: nothing else hides the ~2 us of HBM latency;
        // without the second set this kernel ran at 0.6 of its matrix time).  Rows past the chunk read row
        // v_beg and multiply by 0.
#define DH_LOAD(AV, D, V0)                                                                     \
        _Pragma("unroll") for (int s = 0; s < 8; ++s) {                                        \
            const int v = (V0) + 2 * s + hi;                                                   \
            const bool in = FASTV || v < v_end;                                                \
            const int vc = in ? v : v_beg;                                                     \
            /* FASTV: a wave-uniform row base (scalar registers) + one 32-bit lane offset -- the per-lane form costs a */ \
            /* 64-bit multiply (four quarter-rate instructions) per load, ~700 cycles per block next to 256 of MFMA   */ \
            const float* wr = FASTV ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.W) +     \
                                          ((unsigned)((V0) + 2 * s) * w_row + lane_w))                         \
                                    : Wl + (size_t)vc * p.H;                                   \
            if (NA == 4) {                                                                     \
                const float4 t4 = *reinterpret_cast<const float4*>(wr);                        \
                AV[s][0] = t4.x; AV[s][1 % NA] = t4.y; AV[s][2 % NA] = t4.z; AV[s][3 % NA] = t4.w; \
            } else if (NA == 2) {                                                              \
                const float2 t2 = *reinterpret_cast<const float2*>(wr);                        \
                AV[s][0] = t2.x; AV[s][1 % NA] = t2.y;                                         \
            } else {                                                                           \
                AV[s][0] = wr[0];                                                              \
            }                                                                                  \
            const char* dfast = reinterpret_cast<const char*>(p.dzT) + ((unsigned)((V0) + 2 * s) * d_row + lane_d); \
            if (BF16) D[s].x = __uint_as_float(*reinterpret_cast<const unsigned*>(             \
                FASTV ? dfast : reinterpret_cast<const char*>(Dl16 + (size_t)vc * p.ldT)));    \
            else D[s] = *reinterpret_cast<const float2*>(                                      \
                FASTV ? dfast : reinterpret_cast<const char*>(Dl + (size_t)vc * p.ldT));       \
        }
// the "past the chunk -> 0" select sits HERE, not next to the load: a select on a loaded value in the load
// stage makes the compiler wait for that load before the sched_barrier, i.e. before the MFMAs it should hide under
#define DH_MMA(AV, D, V0)                                                                      \
        if (BF16) {                                                                            \
            unsigned dd[8];                                                                    \
            _Pragma("unroll") for (int s = 0; s < 8; ++s)                                      \
                dd[s] = (FASTV || (V0) + 2 * s + hi < v_end) ? __float_as_uint(D[s].x) : 0u;   \
            const bf16x8_t bx = __builtin_bit_cast(bf16x8_t, make_uint4(                       \
                __builtin_amdgcn_perm(dd[1], dd[0], 0x05040100u), __builtin_amdgcn_perm(dd[3], dd[2], 0x05040100u), \
                __builtin_amdgcn_perm(dd[5], dd[4], 0x05040100u), __builtin_amdgcn_perm(dd[7], dd[6], 0x05040100u))); \
            const bf16x8_t by = __builtin_bit_cast(bf16x8_t, make_uint4(                       \
                __builtin_amdgcn_perm(dd[1], dd[0], 0x07060302u), __builtin_amdgcn_perm(dd[3], dd[2], 0x07060302u), \
                __builtin_amdgcn_perm(dd[5], dd[4], 0x07060302u), __builtin_amdgcn_perm(dd[7], dd[6], 0x07060302u))); \
            _Pragma("unroll") for (int a = 0; a < NA; ++a) {                                   \
                const bf16x8_t af = pk_bf16x8(AV[0][a], AV[1][a], AV[2][a], AV[3][a], AV[4][a], AV[5][a], \
                                              AV[6][a], AV[7][a]);                             \
                acc[a][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bx, af, acc[a][0], 0, 0, 0); \
                acc[a][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(by, af, acc[a][1], 0, 0, 0); \
            }                                                                                  \
        } else                                                                                 \
        _Pragma("unroll") for (int s = 0; s < 8; ++s) {                                        \
            const bool in = FASTV || (V0) + 2 * s + hi < v_end;                                \
            const float dx = in ? D[s].x : 0.f, dy = in ? D[s].y : 0.f;                        \
            _Pragma("unroll") for (int a = 0; a < NA; ++a)                                     \
                acc[a][0] = NA == 4 ? __builtin_amdgcn_mfma_f32_32x32x2f32(dx, AV[s][a], acc[a][0], 0, 0, 0) \
                                    : __builtin_amdgcn_mfma_f32_32x32x2f32(AV[s][a], dx, acc[a][0], 0, 0, 0); \
            _Pragma("unroll") for (int a = 0; a < NA; ++a)                                     \
                acc[a][1] = NA == 4 ? __builtin_amdgcn_mfma_f32_32x32x2f32(dy, AV[s][a], acc[a][1], 0, 0, 0) \
                                    : __builtin_amdgcn_mfma_f32_32x32x2f32(AV[s][a], dy, acc[a][1], 0, 0, 0); \
        }
        // A chunk that is whole (a multiple of 32 rows, and the prefetch past its end stays inside the matrix -- every
        // chunk but the last) needs no "row past the chunk" clamps and selects: its addresses are then a uniform part
        // plus a per-lane constant, and the ~120 VALU instructions per block that a single wave per SIMD executes
        // with the matrix pipe idle shrink accordingly.
        auto body = [&](auto fastc) {
            constexpr bool FASTV = decltype(fastc)::value;
            float avA[8][NA], avB[8][NA];
            float2 dA[8], dB[8];
            DH_LOAD(avA, dA, v_beg)
            for (int v0 = v_beg; v0 < v_end; v0 += 32) {
                DH_LOAD(avB, dB, v0 + 16)
                __builtin_amdgcn_sched_barrier(0);
                DH_MMA(avA, dA, v0)
                __builtin_amdgcn_sched_barrier(0);
                DH_LOAD(avA, dA, v0 + 32)
                __builtin_amdgcn_sched_barrier(0);
                DH_MMA(avB, dB, v0 + 16)
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (((v_end - v_beg) & 31) == 0 && v_end + 16 <= p.V && p.fast32) body(IntC<1>{});
        else body(IntC<0>{});
#undef DH_LOAD
#undef DH_MMA
        float* prow = p.part + ((size_t)ch * p.Bpad64) * p.H + hc0;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int r = r0 + 2 * j + b;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int i_idx = acc_row32(reg, hi);
                if (NA == 4) {
                    // operands swapped (NA = 4): the lane is the hidden unit hc0 + 4 j + a, the register the playlist
                    // r0 + 2 i_idx + b -- 512 contiguous bytes of one partial row per half-wave
                    *reinterpret_cast<float4*>(prow + (size_t)(r0 + 2 * i_idx + b) * p.H + 4 * j) =
                        make_float4(acc[0][b][reg], acc[1 % NA][b][reg], acc[2 % NA][b][reg], acc[3 % NA][b][reg]);
                } else {
#pragma unroll
                    for (int a = 0; a < NA; ++a) prow[(size_t)r * p.H + NA * i_idx + a] = acc[a][b][reg];
                }
            }
        }
    }
}

// ---- K8a: dpre[r, k] = (sum_chunks part) * (h > 0 ? 1/kp : 0) * s (1 - s)  (DAEs.py:67-68) ------
__global__ __launch_bounds__(256) void hidden_backward_kernel(const float* __restrict__ part,
                                                              int n_chunk, int Bpad64, int H, int B,
                                                              const float* __restrict__ h,
                                                              const float* __restrict__ sg, float kp,
                                                              float* __restrict__ dpre)
{
    const size_t n = (size_t)B * H;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (size_t)gridDim.x * 256) {
        float s = 0.f;
        // fixed order; 32 loads in flight per thread (one dependent load per iteration was 32 us for 33 MB, 8 at a time 11 us:
        // 65 536 threads x 128 chunk partials is 16 round trips of 8)
        int c = 0;
        for (; c + 32 <= n_chunk; c += 32) {
            float q[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) q[u] = part[(size_t)(c + u) * Bpad64 * H + o];
#pragma unroll
            for (int u = 0; u < 32; ++u) s += q[u];
        }
        for (; c + 8 <= n_chunk; c += 8) {
            float q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = part[(size_t)(c + u) * Bpad64 * H + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += q[u];
        }
        for (; c < n_chunk; ++c) s += part[(size_t)c * Bpad64 * H + o];
        const float sv = sg[o];
        const float keep = h[o] != 0.0f ? 1.0f / kp : 0.0f;
        dpre[o] = s * keep * sv * (1.0f - sv);
    }
}

// column sums over rows: out[k] = sum_r a[r, k] (+ lambda * base[k])
// one block per 64 columns; 4 row lanes per column, combined in fixed order (deterministic)
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, int B, int H,
                                                     float lambda, const float* __restrict__ base,
                                                     float* __restrict__ out)
{
    __shared__ float part[4][64];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + c;
    float s = 0.f;
    if (k < H) {
        int r = rl;
        for (; r + 28 < B; r += 32) {                // 8 loads in flight, summed in row order
            float q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = a[(size_t)(r + 4 * u) * H + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += q[u];
        }
        for (; r < B; r += 4) s += a[(size_t)r * H + k];
    }
    part[rl][c] = s;
    __syncthreads();
    if (rl == 0 && k < H)
        out[k] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) + (lambda != 0.f ? lambda * base[k] : 0.f);
}

// ---- K8b: gW_enc[c, :] += xhat[r, c] * dpre[r, :]  (row-sparse; several rows may share c) ---------
// xhat is recomputed exactly as the encode kernel does (same dropout draws, same order).
__global__ __launch_bounds__(256) void scatter_gwenc_kernel(const int32_t* __restrict__ row_ptr,
                                                            const int32_t* __restrict__ col,
                                                            const float* __restrict__ val, int B,
                                                            int H, float ikp, uint32_t seed,
                                                            int col_lo, int col_hi,
                                                            const float* __restrict__ dpre,
                                                            float* __restrict__ gW)
{
    // the row's entries (dropped-out value, column) are staged in LDS by all threads at once: walking them with
    // one scalar load per iteration, twice, was ~35 us of dependent-load latency for rows of ~100 entries
    constexpr int CAP = 1024;
    __shared__ float xs[CAP];
    __shared__ int cs[CAP];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (row >= B) return;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    // pass 1: the row sum, in entry order (the order the encode kernel uses)
    float s = 0.0f;
    for (int c0 = beg; c0 < end; c0 += CAP) {
        const int n = min(CAP, end - c0);
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            float x = val[c0 + i];
            const int c = col[c0 + i];
            if (ikp < 1.0f) x = (x / ikp) * floorf(ikp + dae_uniform(seed, 0U, (uint32_t)row, (uint32_t)c));
            xs[i] = x; cs[i] = c;
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) s += xs[i];
    }
    const float denom = s + 1e-10f;
    // pass 2: gW[c, :] += xhat * dpre[row, :]   (a single chunk -- every playlist batch -- is still in LDS)
    for (int c0 = beg; c0 < end; c0 += CAP) {
        const int n = min(CAP, end - c0);
        if (end - beg > CAP) {
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                float x = val[c0 + i];
                const int c = col[c0 + i];
                if (ikp < 1.0f) x = (x / ikp) * floorf(ikp + dae_uniform(seed, 0U, (uint32_t)row, (uint32_t)c));
                xs[i] = x; cs[i] = c;
            }
            __syncthreads();
        }
        // xhat once per entry (the same division, by one thread instead of by every hidden unit's: ~100 IEEE divides per thread)
        __syncthreads();
        for (int i = tid; i < n; i += 256) xs[i] = xs[i] / denom;
        __syncthreads();
        for (int k = tid; k < H; k += 256) {
            const float dv = dpre[(size_t)row * H + k];
            for (int i = 0; i < n; ++i) {
                const float w = xs[i];
                const int c = cs[i];
                if (w != 0.0f && c >= col_lo && c < col_hi) atomicAdd(&gW[(size_t)(c - col_lo) * H + k], w * dv);
            }
        }
    }
}

// ---- vocabulary-sharded training: partial pre-activation of the encoder -------------
// pre[r, k] = sum over this shard's columns of xhat[r, c] * W_loc[c - col_lo, k]; xhat is normalised
// by the row's GLOBAL sum (the CSR carries the whole row on every rank), no bias, no sigmoid.
__global__ __launch_bounds__(256) void encode_partial_kernel(const int32_t* __restrict__ row_ptr,
                                                             const int32_t* __restrict__ col,
                                                             const float* __restrict__ val, int B,
                                                             int H, float ikp, uint32_t seed,
                                                             int col_lo, int col_hi,
                                                             const float* __restrict__ W,
                                                             float* __restrict__ pre)
{
    const int row = blockIdx.x;
    if (row >= B) return;
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    float s = 0.0f;
    for (int i = beg; i < end; ++i) {
        float x = val[i];
        if (ikp < 1.0f) x = (x / ikp) * floorf(ikp + dae_uniform(seed, 0U, (uint32_t)row, (uint32_t)col[i]));
        s += x;
    }
    const float denom = s + 1e-10f;
    for (int k = threadIdx.x; k < H; k += 256) {
        float acc = 0.0f;
        for (int i = beg; i < end; ++i) {
            const int c = col[i];
            if (c < col_lo || c >= col_hi) continue;
            float x = val[i];
            if (ikp < 1.0f) x = (x / ikp) * floorf(ikp + dae_uniform(seed, 0U, (uint32_t)row, (uint32_t)c));
            acc = fmaf(x / denom, W[(size_t)(c - col_lo) * H + k], acc);
        }
        pre[(size_t)row * H + k] = acc;
    }
}

// sg = sigmoid(pre + b_enc); h = dropout(sg, kp) with the encode kernel's draws (DAEs.py:66-68)
__global__ __launch_bounds__(256) void activate_kernel(const float* __restrict__ pre,
                                                       const float* __restrict__ b_enc, int B, int H,
                                                       float kp, uint32_t seed,
                                                       float* __restrict__ h, float* __restrict__ sg)
{
    const size_t n = (size_t)B * H;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (size_t)gridDim.x * 256) {
        const int row = (int)(o / H), hu = (int)(o - (size_t)row * H);
        float hv = dae_sigmoidf(pre[o] + b_enc[hu]);
        sg[o] = hv;
        if (kp < 1.0f) hv = (hv / kp) * floorf(kp + dae_uniform(seed, 1U, (uint32_t)row, (uint32_t)hu));
        h[o] = hv;
    }
}

// dh[o] = sum over the K7 chunks, fixed order
__global__ __launch_bounds__(256) void sum_chunks_kernel(const float* __restrict__ part, int n_chunk,
                                                         size_t chunk_stride, size_t n,
                                                         float* __restrict__ out)
{
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (size_t)gridDim.x * 256) {
        float s = 0.f;
        int c = 0;
        for (; c + 8 <= n_chunk; c += 8) {           // 8 loads in flight, summed in chunk order
            float q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) q[u] = part[(size_t)(c + u) * chunk_stride + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += q[u];
        }
        for (; c < n_chunk; ++c) s += part[(size_t)c * chunk_stride + o];
        out[o] = s;
    }
}

__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ y, const float* __restrict__ x,
                                                   float a, size_t n)
{
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (size_t)gridDim.x * 256)
        y[o] += a * x[o];
}

// sum of squares / 2 of a tensor, one partial per block (tf.nn.l2_loss, DAEs.py:79-82)
__global__ __launch_bounds__(256) void l2_partial_kernel(const float* __restrict__ x, size_t n,
                                                         double* __restrict__ part)
{
    __shared__ double ws[4];
    double s = 0.0;
    for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < n; o += (size_t)gridDim.x * 256)
        s += (double)x[o] * (double)x[o];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = 0.5 * (ws[0] + ws[1] + ws[2] + ws[3]);
}

}  // namespace

// the l2 partials of the listed tensors (null / empty ones left out), side by side at l2_part: at most 1024 per tensor; *n_l2 of
// them.  What the step's cost and the loss without a step (loss_rows.hip) both add up
int dae_launch_l2_partials(dae_ctx* ctx, const float* const* ts, const size_t* ns, int n_t, double* l2_part, int* n_l2)
{
    int n = 0;
    for (int i = 0; i < n_t; ++i) {
        if (!ts[i] || ns[i] == 0) continue;
        const int nb = grid_for(ns[i]) > 1024 ? 1024 : grid_for(ns[i]);
        hipLaunchKernelGGL(l2_partial_kernel, dim3(nb), dim3(256), 0, ctx->stream, ts[i], ns[i], l2_part + n);
        DAE_CHECK_LAUNCH(ctx, "l2_partial_kernel");
        n += nb;
    }
    *n_l2 = n;
    return DAE_OK;
}

namespace {

// cost = sum(loss partials) + lambda * sum(l2 partials), in double, fixed order (lane-strided sums, then
// a shuffle tree): one wave
__global__ __launch_bounds__(64) void finish_cost_kernel(const float* __restrict__ loss_part, int n_loss,
                                                         const double* __restrict__ l2_part, int n_l2, float lambda,
                                                         float* __restrict__ cost)
{
    const int lane = threadIdx.x;
    double s = 0.0, l2 = 0.0;
    for (int i = lane; i < n_loss; i += 64) s += (double)loss_part[i];
    for (int i = lane; i < n_l2; i += 64) l2 += l2_part[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { s += __shfl_xor(s, d); l2 += __shfl_xor(l2, d); }
    if (lane == 0) *cost = (float)(s + (double)lambda * l2);
}

// split of K7's V contraction: about one (output tile of NA * 32 hidden units x 64 playlists, chunk) work item per wave slot
struct K7Plan { int NA, chunk, n_chunk; };
K7Plan k7_plan(int V, int H, int Bpad64)
{
    K7Plan k;
    k.NA = (H % 128) == 0 ? 4 : ((H % 64) == 0 ? 2 : 1);
    const int n_out_tiles = (H / (32 * k.NA)) * (Bpad64 / 64);
    int want_chunks = (DAE_NUM_CU * 4) / n_out_tiles;
    if (want_chunks < 1) want_chunks = 1;
    k.chunk = ((V + want_chunks - 1) / want_chunks + 15) / 16 * 16;
    if (k.chunk < 16) k.chunk = 16;
    k.n_chunk = (V + k.chunk - 1) / k.chunk;
    return k;
}

// K7: the k.n_chunk partials [n_chunk][Bpad64][H] of dh = dz W at `part`.  dz16: dz^T holds bf16 (k.NA == 4)
int launch_k7(dae_ctx* ctx, const float* dzT, int64_t ldT, int dz16, const float* W, int H, int V, int Bpad64, const K7Plan& k,
              float* part)
{
    DhP p;
    p.dzT = dzT; p.ldT = ldT; p.W = W; p.H = H; p.V = V; p.part = part;
    p.n_chunk = k.n_chunk; p.chunk = k.chunk; p.Bpad64 = Bpad64; p.n_half = H / (32 * k.NA);
    p.n_rblk = Bpad64 / 64;
    p.fast32 = ((uint64_t)(V + 32) * (uint64_t)H * 4 < (1ull << 32) && (uint64_t)(V + 32) * (uint64_t)ldT * 4 < (1ull << 32)) ? 1 : 0;
    const int total = p.n_half * p.n_rblk * k.n_chunk;
    int blocks = (total + 3) / 4;
    if (blocks > DAE_NUM_CU) blocks = DAE_NUM_CU;
    if (k.NA == 4 && dz16) hipLaunchKernelGGL((grad_hidden_kernel<4, true>), dim3(blocks), dim3(256), 0, ctx->stream, p);
    else if (k.NA == 4) hipLaunchKernelGGL(grad_hidden_kernel<4>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    else if (k.NA == 2) hipLaunchKernelGGL(grad_hidden_kernel<2>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL(grad_hidden_kernel<1>, dim3(blocks), dim3(256), 0, ctx->stream, p);
    DAE_CHECK_LAUNCH(ctx, "grad_hidden_kernel");
    return DAE_OK;
}

// ---- batches above 256 rows: panels ----------------------------------------------------------------------------------------
// K5, the positives' fix-up, K7 and K6 hold a batch of at most TRAIN_PANEL rows (K6's LDS image of h, the [V, 256] dz^T).  A longer
// batch is cut into panels of TRAIN_PANEL rows and a shorter last one; each panel runs those launches as a batch of its own rows
// would, on h + r0 H, y_row_ptr + r0 (the offsets stay absolute) and the same dz^T scratch.  What is a sum over rows crosses the
// panels: K6 of a later panel adds its tile to the gradient the earlier ones left (grad_wdec.hip ACC), the loss partials of all
// panels lie side by side for finish_cost_kernel, and dh's partials are reduced per panel into the panel's rows of dpre (or of
// the shard's dh).  Encode / activate, the encoder backward, the lambda terms and the cost run once, over all rows: the dropout
// masks are keyed by the row's index in the batch and no kernel that draws them sees a panel.
constexpr int TRAIN_PANEL = 256;
constexpr int TRAIN_MAX_B = 4096;

// what the launches of one batch (or panel) of B <= TRAIN_PANEL rows are: which K5, dz^T's type and row pitch, K7's split
struct TrainShape {
    int G, RB, Bpad64, n_chunk, n_fix, dtype, dz16, rm;
    K7Plan k7;          // (k7.n_chunk: K7's own launch; n_chunk: the partials of dh the step leaves, whoever wrote them)
    int fuse_dh;        // K5 leaves dh's partials itself (decode_f32.hip decode_loss_dh_bf16_kernel): no K7; n_chunk = g.grid + 1
    dae_rowgeom g;
    size_t hp_bytes;
};

// scratch carved for one training step over a [Vl, H] weight (shard) and B rows; stable for a given
// (Vl, H, B), so the stages of a sharded step find h / sg where the earlier stage left them.
// B > TRAIN_PANEL: the TrainShape part is that of a full panel, `last` that of the last one; hbuf / sg / dpre hold all B rows,
// part one panel's partials, loss_part every panel's (n_loss of them); train_panel() is the plan of one panel.
struct TrainPlan : TrainShape {
    size_t bh;
    float *dzT, *hbuf, *sg, *dpre, *part, *loss_part;
    double* l2_part;
    int B, H, n_panel, n_loss;
    TrainShape last;
};

TrainShape train_shape(dae_ctx* ctx, int Vl, int H, int B)
{
    TrainShape t;
    const int Hp = dae_round_up(H, DAE_HPAD);
    t.dtype = ctx->train_dtype;
    // bf16 GEMMs with the 4-tile backward kernels: dL/dz itself is stored as bf16
    t.dz16 = (t.dtype == DAE_DTYPE_BF16 && (H % 128) == 0) ? 1 : 0;
    t.g = t.dtype == DAE_DTYPE_BF16 ? dae_row_geometry_bf16(B, Hp) : dae_row_geometry(B, Hp);
    t.G = Hp / DAE_KG; t.RB = t.g.R_TILE / 32;
    // hidden 256: K5 reads the row-major decoder and hidden activations directly (fp32, or rounded to bf16 in registers) -- no
    // per-step prepack
    t.rm = (H == 256 && t.g.R_TILE == 128 && t.g.waves == 4) ? 1 : 0;
    t.Bpad64 = (B + 63) / 64 * 64;
    t.hp_bytes = (size_t)t.g.n_rg * t.G * t.RB * 64 * sizeof(float4);
    t.k7 = k7_plan(Vl, H, t.Bpad64);
    t.n_chunk = t.k7.n_chunk;
    {   // bf16 GEMMs with dz^T as bf16 at hidden 256: dh comes out of the forward launch, one partial per workgroup + the positives'
        t.fuse_dh = (t.rm && t.dtype == DAE_DTYPE_BF16 && t.dz16) ? 1 : 0;
        if (t.fuse_dh) t.n_chunk = t.g.grid + 1;
    }
    t.n_fix = B;                                   // loss partials of the positives: one per row
    return t;
}

int train_plan(dae_ctx* ctx, int Vl, int H, int B, TrainPlan& t)
{
    if ((H % 32) != 0) return dae_fail(ctx, DAE_ERR_ARG, "training kernels need H %% 32 == 0 (H=%d)", H);
    if (B < 1 || B > TRAIN_MAX_B) return dae_fail(ctx, DAE_ERR_ARG, "training batch %d outside [1, %d]", B, TRAIN_MAX_B);
    if (Vl < 1) return dae_fail(ctx, DAE_ERR_ARG, "empty vocabulary shard");
    int rc;
    t.B = B; t.H = H;
    t.n_panel = (B + TRAIN_PANEL - 1) / TRAIN_PANEL;
    static_cast<TrainShape&>(t) = train_shape(ctx, Vl, H, t.n_panel > 1 ? TRAIN_PANEL : B);
    t.last = t.n_panel > 1 ? train_shape(ctx, Vl, H, B - (t.n_panel - 1) * TRAIN_PANEL) : static_cast<const TrainShape&>(t);
    const int ld_dz = t.n_panel > 1 ? TRAIN_PANEL : t.Bpad64;
    if ((rc = dae_reserve(ctx, ctx->h_packed, t.hp_bytes > t.last.hp_bytes ? t.hp_bytes : t.last.hp_bytes))) return rc;
    if ((rc = dae_reserve(ctx, ctx->train_b, (size_t)Vl * ld_dz * sizeof(float)))) return rc;
    t.bh = (size_t)B * H;
    size_t part_floats = (size_t)t.n_chunk * t.Bpad64 * H;
    if ((size_t)t.last.n_chunk * t.last.Bpad64 * H > part_floats) part_floats = (size_t)t.last.n_chunk * t.last.Bpad64 * H;
    t.n_loss = (t.n_panel - 1) * (t.g.grid + t.n_fix) + t.last.g.grid + t.last.n_fix;
    const size_t c_floats = 3 * t.bh + part_floats + (size_t)t.n_loss + 64;
    if ((rc = dae_reserve(ctx, ctx->train_c, c_floats * sizeof(float) + 4096 * sizeof(double)))) return rc;
    t.dzT = static_cast<float*>(ctx->train_b.p);
    t.hbuf = static_cast<float*>(ctx->train_c.p);
    t.sg = t.hbuf + t.bh;
    t.dpre = t.sg + t.bh;
    t.part = t.dpre + t.bh;
    t.loss_part = t.part + part_floats;
    t.l2_part = reinterpret_cast<double*>(
        (reinterpret_cast<uintptr_t>(t.loss_part + t.n_loss) + 63) & ~(uintptr_t)63);
    return DAE_OK;
}

// the plan of panel i (rows [i TRAIN_PANEL, ...)) of a step: its own shape, its rows of hbuf / sg / dpre, its loss partials
TrainPlan train_panel(const TrainPlan& t, int i)
{
    if (t.n_panel == 1) return t;
    TrainPlan p = t;
    const int r0 = i * TRAIN_PANEL;
    if (i == t.n_panel - 1) static_cast<TrainShape&>(p) = t.last;
    p.B = i == t.n_panel - 1 ? t.B - r0 : TRAIN_PANEL;
    p.bh = (size_t)p.B * t.H;
    p.hbuf += (size_t)r0 * t.H; p.sg += (size_t)r0 * t.H; p.dpre += (size_t)r0 * t.H;
    p.loss_part += (size_t)i * (t.g.grid + t.n_fix);
    p.n_loss = p.g.grid + p.n_fix;
    p.n_panel = 1;
    return p;
}

// One panel (a whole batch of at most TRAIN_PANEL rows is its only panel): K5 loss/dz over the prepacked decoder image + the
// positives' fix-up -> K6 (gW, gb) -> K7 partials of dh.  t: the panel's plan; h (row-major in t.hbuf and tiled in ctx->h_packed)
// and ctx->pk_f32 must be current.  arm: the step is armed (dae_arm_decoder_adam).  first / last: the panel's place in the step.
// A later panel adds to the gradient of the earlier ones; the armed update belongs to the last panel, the earlier ones leave their
// sum in gscr ([Vl, H], ctx->train_d) instead of gWd.
int train_decode_backward_panel(dae_ctx* ctx, const TrainPlan& t, int Vl, int H, int B, int n_batch,
                                const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                                int col_lo, int col_hi, const float* Wd, const float* b_dec, float* gWd, float* gb_dec,
                                const dae_armed_adam* arm, bool first, bool last, float* gscr)
{
    hipStream_t st = ctx->stream;
    int rc;
    if (t.Bpad64 != B)
        DAE_HIP_CHECK(ctx, hipMemsetAsync(t.dzT, 0, (size_t)Vl * t.Bpad64 * (t.dz16 ? sizeof(unsigned short) : sizeof(float)), st));
    float* const corr_part = t.part + (size_t)(t.n_chunk - 1) * t.Bpad64 * H;         // (fuse_dh: the positives' partial, the last one)
    if (t.fuse_dh) {
        rc = dae_launch_decode_loss_dh(ctx, t.g, B, Vl, H, Wd, b_dec, t.hbuf, 1.0f / (float)n_batch, t.dzT, t.Bpad64, t.loss_part,
                                       t.part, t.Bpad64);
        if (rc == DAE_ERR_STATE) return dae_fail(ctx, DAE_ERR_STATE, "the fused K5 + K7 launch does not take this shape");
        if (t.Bpad64 != B) DAE_HIP_CHECK(ctx, hipMemsetAsync(corr_part, 0, (size_t)t.Bpad64 * H * sizeof(float), st));
    } else if (t.rm)
        rc = dae_launch_decode_loss_rowmajor(ctx, t.g, B, Vl, H, Wd, b_dec, t.hbuf, 1.0f / (float)n_batch, t.dzT, t.Bpad64,
                                             t.loss_part);      // (fp32: a bf16 step at hidden 256 takes the fused launch above)
    else
        rc = dae_launch_decode_loss_f32(ctx, t.g, B, 1.0f / (float)n_batch, t.dzT, t.Bpad64, t.loss_part, t.dtype, t.dz16);
    if (rc) return rc;
    auto fixup = [&](auto kernel, float* corr_out) {
        hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, st, y_row_ptr, y_col, y_val, B, H, col_lo, col_hi, t.hbuf, Wd, b_dec,
                           1.0f / (float)n_batch, t.dzT, (int64_t)t.Bpad64, t.loss_part + t.g.grid, corr_out);
    };
    if (t.fuse_dh) fixup(&loss_fixup_kernel<true, true, true>, corr_part);
    else if (t.dz16) fixup(&loss_fixup_kernel<true, true>, nullptr);
    else if (t.dtype == DAE_DTYPE_BF16) fixup(&loss_fixup_kernel<true>, nullptr);
    else fixup(&loss_fixup_kernel<false>, nullptr);
    DAE_CHECK_LAUNCH(ctx, "loss_fixup_kernel");

    // where the gradient of the panels so far lies: gWd, or gscr while an armed step has panels to come
    float* const gsum = (arm && !(first && last)) ? gscr : gWd;
    auto run_k6 = [&](const dae_armed_adam* a) {
        return dae_launch_k6(ctx, t.dzT, t.Bpad64, t.dz16, t.hbuf, H, B, Vl, a ? gWd : gsum, gb_dec, a, 0, first ? nullptr : gsum);
    };
    auto run_k7 = [&]() { return launch_k7(ctx, t.dzT, t.Bpad64, t.dz16, Wd, H, Vl, t.Bpad64, t.k7, t.part); };
    // K6 and K7 are independent (both read dz^T).  With the armed Adam K6 rewrites Wd in place, and K7 multiplies by
    // the weights the forward pass used: K7 first.
    if (arm && last) {          // dae_arm_decoder_adam: update Wd in place instead of writing gWd
        if (!t.fuse_dh) { rc = run_k7(); if (rc) return rc; }
        return run_k6(arm);
    }
    rc = run_k6(nullptr); if (rc) return rc;
    return t.fuse_dh ? DAE_OK : run_k7();
}

// The decode side of a step over all its panels.  after_panel(plan of the panel, its first row): what has to read the panel's
// partials of dh before the next panel overwrites them; called for steps of more than one panel only (the one panel of a shorter
// batch leaves them at t.part, as it always did).
template <class After>
int train_decode_backward(dae_ctx* ctx, const TrainPlan& t, int Vl, int H, int B, int n_batch,
                          const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                          int col_lo, int col_hi, const float* Wd, const float* b_dec, float* gWd, float* gb_dec, After after_panel)
{
    int rc;
    if (H > FIX_MAXH) return dae_fail(ctx, DAE_ERR_ARG, "training kernels need H <= %d (H=%d)", FIX_MAXH, H);
    dae_armed_adam arm = {const_cast<float*>(Wd), ctx->arm_m, ctx->arm_v, ctx->arm_alpha, ctx->arm_b1, ctx->arm_b2, ctx->arm_eps};
    const bool armed = ctx->arm_m != nullptr;
    float* gscr = nullptr;
    if (armed) {
        ctx->arm_m = nullptr; ctx->arm_v = nullptr;         // one step only
        if ((H % 128) != 0) return dae_fail(ctx, DAE_ERR_ARG, "the armed decoder Adam needs H %% 128 == 0 (H=%d)", H);
        if (t.n_panel > 1) {
            // (train_d: otherwise the title scorer's K7 partials, dae_launch_grad_h -- nothing of either outlives its call)
            if ((rc = dae_reserve(ctx, ctx->train_d, (size_t)Vl * H * sizeof(float)))) return rc;
            gscr = static_cast<float*>(ctx->train_d.p);
        }
    }
    for (int i = 0; i < t.n_panel; ++i) {
        const TrainPlan pv = train_panel(t, i);
        const int r0 = i * TRAIN_PANEL;
        if (t.n_panel > 1 && !pv.rm) {                      // the packed K5 reads the panel's rows as a hidden tile of its own
            rc = pv.dtype == DAE_DTYPE_BF16 ? dae_launch_pack_h_bf16(ctx, pv.hbuf, pv.B, H, pv.g) : dae_launch_pack_h(ctx, pv.hbuf, pv.B, H, pv.g);
            if (rc) return rc;
            ctx->h_geom_key = -1;
        }
        rc = train_decode_backward_panel(ctx, pv, Vl, H, pv.B, n_batch, y_row_ptr + r0, y_col, y_val, col_lo, col_hi, Wd, b_dec,
                                         gWd, gb_dec, armed ? &arm : nullptr, i == 0, i == t.n_panel - 1, gscr);
        if (rc) return rc;
        if (t.n_panel > 1 && (rc = after_panel(pv, r0))) return rc;
    }
    return DAE_OK;
}

// cost = sum of the loss partials + lambda * (l2 of the listed tensors)
int train_cost(dae_ctx* ctx, const TrainPlan& t, float reg_lambda, const float* const* ts,
               const size_t* ns, int n_t, float* cost_out)
{
    hipStream_t st = ctx->stream;
    int n_l2 = 0;
    if (reg_lambda != 0.0f) {
        const int rc = dae_launch_l2_partials(ctx, ts, ns, n_t, t.l2_part, &n_l2);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(finish_cost_kernel, dim3(1), dim3(64), 0, st, t.loss_part, t.n_loss, t.l2_part, n_l2,
                       reg_lambda, cost_out);
    DAE_CHECK_LAUNCH(ctx, "finish_cost_kernel");
    return DAE_OK;
}

// dpre of a batch's (or panel's) rows from its n_chunk partials of dh at `part`
int train_hidden_backward(dae_ctx* ctx, const TrainPlan& t, const float* part, int n_chunk, int H, int B, float kp)
{
    hipLaunchKernelGGL(hidden_backward_kernel, dim3(grid_for(t.bh)), dim3(256), 0, ctx->stream, part, n_chunk,
                       t.Bpad64, H, B, t.hbuf, t.sg, kp, t.dpre);
    DAE_CHECK_LAUNCH(ctx, "hidden_backward_kernel");
    return DAE_OK;
}

// dpre from dh (n_chunk partials at `part`; part == null: the panels of the step have left dpre already), gb_enc, the row-sparse
// gW_enc of this column range, and the lambda terms of the weight gradients -- over all B rows of the step
int train_encoder_backward(dae_ctx* ctx, const TrainPlan& t, const float* part, int n_chunk,
                           const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
                           int col_lo, int col_hi, int H, int B, int tied, float ikp, float kp,
                           uint32_t seed, float reg_lambda, const float* W_enc, const float* b_enc,
                           const float* W_dec, const float* b_dec,
                           float* gW_enc, float* gb_enc, float* gW_dec, float* gb_dec)
{
    hipStream_t st = ctx->stream;
    const size_t nW = (size_t)(col_hi - col_lo) * H;
    if (part) {
        const int rc = train_hidden_backward(ctx, t, part, n_chunk, H, B, kp);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(colsum_kernel, dim3((H + 63) / 64), dim3(256), 0, st, t.dpre, B, H, reg_lambda,
                       b_enc, gb_enc);
    DAE_CHECK_LAUNCH(ctx, "colsum_kernel");

    // ---- K8: encoder gradient (row-sparse) -----------------------------------------------------------
    // (the rows-Adam keeps the dense buffer all-zero itself: dae_set_enc_grad_prezeroed)
    if (!tied && !ctx->enc_grad_prezeroed) DAE_HIP_CHECK(ctx, hipMemsetAsync(gW_enc, 0, nW * sizeof(float), st));
    hipLaunchKernelGGL(scatter_gwenc_kernel, dim3(B), dim3(256), 0, st, x_row_ptr, x_col, x_val, B, H,
                       ikp, seed, col_lo, col_hi, t.dpre, gW_enc);
    DAE_CHECK_LAUNCH(ctx, "scatter_gwenc_kernel");

    if (reg_lambda != 0.0f) {
        hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(nW)), dim3(256), 0, st, gW_enc, W_enc, reg_lambda, nW);
        if (!tied)
            hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(nW)), dim3(256), 0, st, gW_dec, W_dec, reg_lambda, nW);
        hipLaunchKernelGGL(axpy_kernel, dim3(grid_for((size_t)(col_hi - col_lo))), dim3(256), 0, st, gb_dec,
                           b_dec, reg_lambda, (size_t)(col_hi - col_lo));
        DAE_CHECK_LAUNCH(ctx, "axpy_kernel");
    }
    return DAE_OK;
}

}  // namespace

// ---- K7 on caller-provided buffers (the title scorer's output layer; its K6 is grad_wdec.hip dae_launch_grad_w) ---
// dh[r, :] = sum_v dzT[v, r] W[v, :]  (split over V into ctx scratch, reduced in fixed order)
int dae_launch_grad_h(dae_ctx* ctx, const float* dzT, int64_t ldT, const float* W, int H, int V, int B, float* dh)
{
    if ((H % 32) != 0 || B < 1 || B > 256) return dae_fail(ctx, DAE_ERR_ARG, "grad_h: H=%d B=%d unsupported", H, B);
    const int Bpad64 = (B + 63) / 64 * 64;
    if (ldT < Bpad64) return dae_fail(ctx, DAE_ERR_ARG, "grad_h: ldT=%lld < %d", (long long)ldT, Bpad64);
    const K7Plan k = k7_plan(V, H, Bpad64);
    const int n_chunk = k.n_chunk;
    int rc = dae_reserve(ctx, ctx->train_d, (size_t)n_chunk * Bpad64 * H * sizeof(float));
    if (rc) return rc;
    float* part = static_cast<float*>(ctx->train_d.p);
    if ((rc = launch_k7(ctx, dzT, ldT, 0, W, H, V, Bpad64, k, part))) return rc;
    const size_t bh = (size_t)B * H;
    hipLaunchKernelGGL(sum_chunks_kernel, dim3(grid_for(bh)), dim3(256), 0, ctx->stream, part, n_chunk,
                       (size_t)Bpad64 * H, bh, dh);
    DAE_CHECK_LAUNCH(ctx, "sum_chunks_kernel");
    return DAE_OK;
}

int dae_train_step_f32(dae_ctx* ctx,
        const int32_t* x_row_ptr, const int32_t* x_col, const float* x_val,
        const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
        const float* W_enc, const float* b_enc, const float* W_dec, const float* b_dec,
        int V, int H, int B, int n_batch, int tied,
        float ikp, float kp, uint32_t seed, float reg_lambda,
        float* gW_enc, float* gb_enc, float* gW_dec, float* gb_dec, float* cost_out)
{
    hipStream_t st = ctx->stream;
    TrainPlan t;
    int rc = train_plan(ctx, V, H, B, t);
    if (rc) return rc;
    if (ctx->arm_m && (tied || reg_lambda != 0.0f)) {
        ctx->arm_m = nullptr; ctx->arm_v = nullptr;
        return dae_fail(ctx, DAE_ERR_ARG, "the armed decoder Adam needs the untied model and reg_lambda = 0");
    }
    const float* Wd = tied ? W_enc : W_dec;
    const bool packed = !t.rm || !t.last.rm;                // some panel takes the packed K5
    const bool panels = t.n_panel > 1;                      // (each panel's hidden tile is then packed from t.hbuf, panel by panel)
    // decoder weights change every step: re-tile them for the forward GEMM
    if (packed) {
        rc = t.dtype == DAE_DTYPE_BF16 ? dae_launch_prepack_bf16(ctx, Wd, b_dec, V, H, 0, V)
                                       : dae_launch_prepack_f32(ctx, Wd, b_dec, V, H, 0, V, false);    // (no logit bounds: a ranking call on this image skips nothing)
        if (rc) return rc;
    }

    // ---- forward ----------------------------------------------------------------------------------
    // the pad rows / pad k of the fp32 image are never written by the encode kernel: zeroed once per geometry and
    // buffer (same key as the scoring path: the two share the image)
    if (t.dtype == DAE_DTYPE_F32 && !t.rm && !panels) {
        const long long key = ((long long)B << 32) | ((long long)H << 12) | (long long)t.g.R_TILE;
        if (ctx->h_geom_key != key || ctx->h_geom_ptr != ctx->h_packed.p) {
            DAE_HIP_CHECK(ctx, hipMemsetAsync(ctx->h_packed.p, 0, t.hp_bytes, st));
            ctx->h_geom_key = key;
            ctx->h_geom_ptr = ctx->h_packed.p;
        }
    }
    if (t.rm || panels) {
        rc = dae_launch_encode(ctx, x_row_ptr, x_col, x_val, W_enc, b_enc, V, H, B, ikp, kp, seed, t.hbuf,
                               nullptr, 0, 0, t.sg, nullptr);
    } else if (t.dtype == DAE_DTYPE_BF16) {
        rc = dae_launch_encode(ctx, x_row_ptr, x_col, x_val, W_enc, b_enc, V, H, B, ikp, kp, seed, t.hbuf,
                               nullptr, 0, 0, t.sg, nullptr);
        if (rc) return rc;
        rc = dae_launch_pack_h_bf16(ctx, t.hbuf, B, H, t.g);
    } else {
        rc = dae_launch_encode(ctx, x_row_ptr, x_col, x_val, W_enc, b_enc, V, H, B, ikp, kp, seed, t.hbuf,
                               static_cast<float*>(ctx->h_packed.p), t.G, t.RB, t.sg, nullptr);
    }
    if (rc) return rc;
    rc = train_decode_backward(ctx, t, V, H, B, n_batch, y_row_ptr, y_col, y_val, 0, V, Wd, b_dec,
                               tied ? gW_enc : gW_dec, gb_dec, [&](const TrainPlan& pv, int) {
                                   return train_hidden_backward(ctx, pv, pv.part, pv.n_chunk, H, pv.B, kp);
                               });
    if (rc) return rc;

    // ---- cost (+ lambda * l2) ----------------------------------------------------------------------
    const float* ts[4] = {W_enc, b_dec, b_enc, tied ? nullptr : W_dec};
    const size_t ns[4] = {(size_t)V * H, (size_t)V, (size_t)H, (size_t)V * H};
    rc = train_cost(ctx, t, reg_lambda, ts, ns, 4, cost_out);
    if (rc) return rc;

    rc = train_encoder_backward(ctx, t, panels ? nullptr : t.part, t.n_chunk, x_row_ptr, x_col, x_val, 0, V, H, B, tied,
                                ikp, kp, seed, reg_lambda, W_enc, b_enc, W_dec, b_dec,
                                gW_enc, gb_enc, gW_dec, gb_dec);
    if (rc) return rc;
    if (packed) (t.dtype == DAE_DTYPE_BF16 ? ctx->pk_bf16 : ctx->pk_f32).valid = true;
    return DAE_OK;
}

// ---- vocabulary-row sharded step: three stages around the caller's two all-reduces ------
int dae_train_shard_encode_f32(dae_ctx* ctx, const int32_t* x_row_ptr, const int32_t* x_col,
                               const float* x_val, const float* W_enc_loc, int col_lo, int col_hi,
                               int H, int B, float ikp, uint32_t seed, float* pre_partial)
{
    hipLaunchKernelGGL(encode_partial_kernel, dim3(B), dim3(256), 0, ctx->stream, x_row_ptr, x_col, x_val,
                       B, H, ikp, seed, col_lo, col_hi, W_enc_loc, pre_partial);
    DAE_CHECK_LAUNCH(ctx, "encode_partial_kernel");
    return DAE_OK;
}

int dae_train_shard_decode_f32(dae_ctx* ctx, const float* pre, const float* b_enc,
                               const int32_t* y_row_ptr, const int32_t* y_col, const float* y_val,
                               const float* W_enc_loc, const float* W_dec_loc, const float* b_dec_loc,
                               int col_lo, int col_hi, int H, int B, int n_batch, int tied,
                               float kp, uint32_t seed, float reg_lambda,
                               float* gW_out, float* gb_dec_loc, float* dh_partial, float* cost_partial)
{
    hipStream_t st = ctx->stream;
    const int Vl = col_hi - col_lo;
    TrainPlan t;
    int rc = train_plan(ctx, Vl, H, B, t);
    if (rc) return rc;
    const float* Wd = tied ? W_enc_loc : W_dec_loc;
    const bool packed = !t.rm || !t.last.rm;
    if (packed) {
        rc = t.dtype == DAE_DTYPE_BF16 ? dae_launch_prepack_bf16(ctx, Wd, b_dec_loc, Vl, H, 0, Vl)
                                       : dae_launch_prepack_f32(ctx, Wd, b_dec_loc, Vl, H, 0, Vl, false);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(activate_kernel, dim3(grid_for(t.bh)), dim3(256), 0, st, pre, b_enc, B, H, kp, seed,
                       t.hbuf, t.sg);
    DAE_CHECK_LAUNCH(ctx, "activate_kernel");
    ctx->h_geom_key = -1;
    if (!t.rm && t.n_panel == 1) {
        rc = t.dtype == DAE_DTYPE_BF16 ? dae_launch_pack_h_bf16(ctx, t.hbuf, B, H, t.g)
                                       : dae_launch_pack_h(ctx, t.hbuf, B, H, t.g);
        if (rc) return rc;
    }
    // dh of this shard: the partials summed in chunk order, a panel's rows after the panel
    auto sum_dh = [&](const TrainPlan& pv, int r0) {
        hipLaunchKernelGGL(sum_chunks_kernel, dim3(grid_for(pv.bh)), dim3(256), 0, st, pv.part, pv.n_chunk,
                           (size_t)pv.Bpad64 * H, pv.bh, dh_partial + (size_t)r0 * H);
        DAE_CHECK_LAUNCH(ctx, "sum_chunks_kernel");
        return (int)DAE_OK;
    };
    rc = train_decode_backward(ctx, t, Vl, H, B, n_batch, y_row_ptr, y_col, y_val, col_lo, col_hi, Wd, b_dec_loc,
                               gW_out, gb_dec_loc, sum_dh);
    if (rc) return rc;
    // b_enc is replicated: its l2 term is counted once, by the shard that owns column 0
    const float* ts[4] = {W_enc_loc, b_dec_loc, col_lo == 0 ? b_enc : nullptr, tied ? nullptr : W_dec_loc};
    const size_t ns[4] = {(size_t)Vl * H, (size_t)Vl, (size_t)H, (size_t)Vl * H};
    rc = train_cost(ctx, t, reg_lambda, ts, ns, 4, cost_partial);
    if (rc) return rc;
    if (t.n_panel == 1 && (rc = sum_dh(t, 0))) return rc;
    if (packed) (t.dtype == DAE_DTYPE_BF16 ? ctx->pk_bf16 : ctx->pk_f32).valid = true;
    return DAE_OK;
}

int dae_train_shard_finish_f32(dae_ctx* ctx, const float* dh, const int32_t* x_row_ptr,
                               const int32_t* x_col, const float* x_val,
                               const float* W_enc_loc, const float* b_enc, const float* W_dec_loc,
                               const float* b_dec_loc, int col_lo, int col_hi, int H, int B, int tied,
                               float ikp, float kp, uint32_t seed, float reg_lambda,
                               float* gW_enc_loc, float* gb_enc, float* gW_dec_loc, float* gb_dec_loc)
{
    TrainPlan t;
    int rc = train_plan(ctx, col_hi - col_lo, H, B, t);       // same carving as the decode stage
    if (rc) return rc;
    return train_encoder_backward(ctx, t, dh, 1, x_row_ptr, x_col, x_val, col_lo, col_hi, H, B, tied,
                                  ikp, kp, seed, reg_lambda, W_enc_loc, b_enc, W_dec_loc, b_dec_loc,
                                  gW_enc_loc, gb_enc, gW_dec_loc, gb_dec_loc);
}
