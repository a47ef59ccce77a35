// rank_of.hip -- the exact rank of GIVEN track columns among all rankable tracks of a row, without the [B, V] matrix a dense
// decode, a sort and a search would take (include/dae_hip.h "rank_of").
//
// THE ORDER.  Column c' precedes column c of a row iff  key(z') > key(z)  or  (key(z') == key(z) and c' < c), key = dae_okey of
// the canonical fp32 logit: the order every ranking call of the library lists by.  Both halves live in ONE 64-bit word,
//     comp(z, c) = (~dae_okey(z) << 32) | c,        c' precedes c  <=>  comp' < comp,
// so ties need no path of their own and a column never precedes itself.
//
// THE LAUNCHES of a call (all on the context's stream, all scratch in the context):
//   1. dae_decode_candidates over the answers: z_a, the canonical logit of every listed (row, column), from the row-major tensors.
//   2. a memset of the global counters and of the row groups' longest-row words;
//   3. rank_of_prep_kernel, a workgroup per row: a row's answers are cut into CHUNKS of C in the caller's order
//      (rank_of_plan.h), each chunk's composites sorted ascending into thr[] at the answers' own CSR offsets, inv[i] = the place
//      of answer i in its chunk.  An answer that cannot be ranked by its id (-1, an artist, out of range) becomes ~0, which
//      sorts behind every real composite.
//   4. rank_of_count_kernel: the fp32 MFMA decode over the tiles that hold a ranked column, hidden tile resident in LDS, W
//      streamed through a register ring as in decode_generic.hip.  Per pass q the workgroup holds chunk q of each of its rows
//      in LDS and drops every logit x of a ranked column into the bucket j = #{a in chunk : comp(a) <= comp(x)}.  x precedes
//      the answer at sorted place p iff j <= p, so that answer's count is the PREFIX sum of the buckets up to p; bucket `len` is
//      never read and not kept.  One compare each against the chunk's first and last threshold settles the common cases
//      (bucket 0 is counted in a register, bucket `len` dropped); only what lies between takes the binary search and an LDS
//      atomic.  The answer's own column gives comp(x) == comp(a) -- the accumulator IS the candidate chain's value -- hence j > p:
//      it is left out by identity.  Workgroups add their buckets to the global ones with integer atomics: sums of integers, the
//      same whatever the order.
//   5. rank_of_finish_kernel, a workgroup per row: prefix sums -> counts; then the row's SEEDS (each distinct seed track once):
//      their canonical logits by the same chain, one subtracted from every answer a seed precedes, and an answer that is a seed
//      becomes (-1, -inf).  Results go out in the caller's order.
//
// THE TITLED CALL (dae_mix_rank_of; DESIGN.md section 4d "Under the title mix") ranks by the MIXED score
//     y[r, c] = sigmoid(z_title[r, c]) * w_title[r] + sigmoid(z_dae[r, c]) * w_playlist[r]                    (mixf, mix_common.h)
// with the same launches on the TITLE scorer's context: y_a from dae_mix_candidates; the DAE's term of the track columns stored
// transposed by dae_decode_mix_term (on the DAE's context); the counting launch is the MIX instantiation of the kernel below
// over the title image (Output_W^T / Output_b against the title features), whose epilogue turns every accumulator element into
// y with the operations and order of the fp32 mix epilogue of decode_generic.hip before it is counted; the finishing launch
// takes the seeds out by their mixed value (both canonical chains per distinct seed).  The composite, the buckets, the prefix
// sums are the plain call's: the kernels are the same templates.
//
// THE ENSEMBLE'S CALL (dae_ensemble_rank_of; DESIGN.md section 4e "Ranks under the ensemble") ranks by the canonical value y of a
// weighted sum of several scorers with the same launches again: y_a and the seeds' values from the candidate chains of
// ensemble.hip, the other scorers' terms in the transposed buffer dae_ensemble_topk builds, the MIX counting kernel over the
// ranking scorer's image, and the GIVEN instantiation of the finishing kernel, which reads the seeds' values instead of
// recomputing chains.
#include "decode_common.h"
#include "mix_common.h"             // mixf
#include "rank_of_plan.h"
#include "ensemble_rank_of_plan.h"

namespace {

constexpr int RO_NW = 4;                       // waves of a counting workgroup: one per SIMD
constexpr int RO_THREADS = RO_NW * 64;
constexpr unsigned long long RO_NONE = ~0ull;  // an answer whose id cannot be ranked
constexpr int RO_MAXH = 1024;

__device__ __forceinline__ unsigned long long ro_comp(float z, int c)
{
    return ((unsigned long long)(~dae_okey(z)) << 32) | (unsigned)c;
}

struct RankP {
    const float4* Wp; const float* bias; const float4* hp;   // the fp32 image over [0, V) and the packed hidden rows
    int G, ntiles_r, n_tracks, V;              // k groups; tiles with a ranked column; ranked columns; all columns
    int B, n_rg, nb_rg, C;
    const int32_t* ans_row_ptr; const int32_t* ans_col; int n_ans;
    const int32_t* seed_row_ptr; const int32_t* seed_col;
    const float* z;                            // [n_ans] candidate logits
    unsigned long long* thr; int* inv;         // [n_ans] sorted composites per chunk; place of an answer in its chunk
    unsigned* gcnt; int* glen;                 // [n_ans] buckets; [n_rg] longest row of a group
    int R_TILE;
    const float* h; int H; const float* W; const float* b;   // row-major tensors (the seeds' chains)
    int32_t* out_rank; float* out_logit;
    // the titled call alone (the MIX instantiations): the DAE's term of the track columns, transposed; the mixing weights; the
    // title scorer's row-major tensors and feature rows (the seeds' second chain).  h / H / W / b above are then the DAE's,
    // Wp / bias / hp / G the title image's, z the mixed values y_a.
    const float* mixT; int64_t mix_ld; const float* w_title; const float* w_playlist;
    const float* feat; int HF; const float* WT; const float* bT;
    // the ensemble's call alone (the GIVEN finish): the seeds' values, one per slot of seed_col, computed before the launch
    const float* seed_y; int n_seed;
};

// a row's answers: [beg, end) of ans_col, clamped to what the caller said exists
__device__ __forceinline__ void ro_row_span(const RankP& p, int row, int& beg, int& end)
{
    const int a = p.ans_row_ptr[row], b = p.ans_row_ptr[row + 1];
    beg = a > 0 ? a : 0;
    end = b < p.n_ans ? b : p.n_ans;
    if (end < beg) end = beg;
}

__global__ __launch_bounds__(256) void rank_of_prep_kernel(const RankP p)
{
    __shared__ unsigned long long comp[DAE_RO_MAX_C];
    const int row = blockIdx.x, tid = threadIdx.x;
    int beg, end;
    ro_row_span(p, row, beg, end);
    if (tid == 0 && end > beg) atomicMax(&p.glen[row / p.R_TILE], end - beg);
    for (int c0 = beg; c0 < end; c0 += p.C) {
        const int len = end - c0 < p.C ? end - c0 : p.C;
        __syncthreads();
        for (int t = tid; t < len; t += 256) {
            const int c = p.ans_col[c0 + t];
            comp[t] = (c >= 0 && c < p.n_tracks) ? ro_comp(p.z[c0 + t], c) : RO_NONE;
        }
        __syncthreads();
        for (int t = tid; t < len; t += 256) {
            const unsigned long long a = comp[t];
            int pos = 0;
            for (int u = 0; u < len; ++u) {
                const unsigned long long o = comp[u];
                pos += (o < a || (o == a && u < t)) ? 1 : 0;
            }
            p.thr[c0 + pos] = a;
            p.inv[c0 + t] = pos;
        }
    }
}

// MIX: the titled call -- the image is the title scorer's, and what is counted is y, not the logit (the mix epilogue below)
template <int RB, int GT, bool MIX>
__global__ __launch_bounds__(RO_THREADS, 1) void rank_of_count_kernel(const RankP p)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    constexpr int R_TILE = RB * 32;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;
    const int G = GT > 0 ? GT : p.G;
    const int C = p.C;

    // XCD-aware block -> (row group, slot in row group), as the decode kernels
    const int gs = DAE_NUM_XCD * p.n_rg;
    const int q = blockIdx.x / gs, rem = blockIdx.x % gs;
    const int rg = rem / DAE_NUM_XCD;
    const int bir = q * DAE_NUM_XCD + (rem % DAE_NUM_XCD);
    if (rg >= p.n_rg || bir >= p.nb_rg) return;

    const int longest = p.glen[rg];                               // block-uniform
    if (longest <= 0) return;                                     // no row of the group asks anything

    const int n_h4 = RB * 64 * G;
    unsigned long long* lthr = reinterpret_cast<unsigned long long*>(lds4 + n_h4);
    unsigned* lcnt = reinterpret_cast<unsigned*>(lthr + (size_t)R_TILE * C);
    int* llen = reinterpret_cast<int*>(lcnt + (size_t)R_TILE * C);
    int* lbeg = llen + R_TILE;

    // ---- hidden tile of this row group -> LDS, once ------------------------------------------
    {
        const float4* src = p.hp + (size_t)rg * n_h4;
        int i = tid;
        for (; i + 7 * RO_THREADS < n_h4; i += 8 * RO_THREADS) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[i + u * RO_THREADS];
#pragma unroll
            for (int u = 0; u < 8; ++u) lds4[i + u * RO_THREADS] = v[u];
        }
        for (; i < n_h4; i += RO_THREADS) lds4[i] = src[i];
    }

    const int n_ws = p.nb_rg * RO_NW;
    const int item0 = wave * p.nb_rg + bir;                       // wave-major: a short tile list is spread over all workgroups

    for (int pass = 0; pass * C < longest; ++pass) {
        // ---- chunk `pass` of every row of the group: thresholds into LDS, buckets zeroed ------
        for (int i = tid; i < R_TILE; i += RO_THREADS) {
            const int row = rg * R_TILE + i;
            int len = 0, beg = 0;
            if (row < p.B) {
                int rb0, re;
                ro_row_span(p, row, rb0, re);
                beg = rb0 + pass * C;
                len = re - beg;
                len = len < 0 ? 0 : (len > C ? C : len);
                // the unrankable answers sort to the chunk's end: they are no thresholds (first index holding RO_NONE)
                int lo = 0, hi2 = len;
                while (lo < hi2) {
                    const int mid = (lo + hi2) >> 1;
                    if (p.thr[beg + mid] == RO_NONE) hi2 = mid; else lo = mid + 1;
                }
                len = lo;
            }
            llen[i] = len; lbeg[i] = beg;
        }
        __syncthreads();
        for (int s = tid; s < R_TILE * C; s += RO_THREADS) {
            const int i = s / C, t = s - i * C;
            lcnt[s] = 0u;
            if (t < llen[i]) lthr[s] = p.thr[lbeg[i] + t];
        }
        __syncthreads();

        int len_r[RB];
        unsigned n0[RB];
        unsigned long long first[RB], last[RB];
        float wt_r[MIX ? RB : 1];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const int i = rb * 32 + j;
            len_r[rb] = llen[i];
            if (MIX) wt_r[rb] = len_r[rb] > 0 ? p.w_title[rg * R_TILE + i] : 0.0f;      // (a row at or past B has no answers)
            n0[rb] = 0u;
            first[rb] = len_r[rb] > 0 ? lthr[(size_t)i * C] : 0ull;                       // (no x is below 0 ...
            last[rb] = len_r[rb] > 0 ? lthr[(size_t)i * C + len_r[rb] - 1] : 0ull;        //  ... and every x is >= 0: nothing counts)
        }

        // ---- the GEMM over the ranked tiles (decode_generic.hip decode_f32_kernel's fp32 body) -
        if (item0 < p.ntiles_r) {
            float4 wb0, wb1, wb2, wb3;
            float4 bA[RB], bB[RB];
            {
                const float4* w0 = p.Wp + (size_t)item0 * G * 64 + lane;
                wb0 = w0[0]; wb1 = w0[64]; wb2 = w0[128]; wb3 = w0[192];
            }
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) bA[rb] = lds4[rb * 64 + lane];

            for (int t = item0; t < p.ntiles_r; t += n_ws) {
                const float4* wp = p.Wp + (size_t)t * G * 64 + lane;
                const int t_n = t + n_ws < p.ntiles_r ? t + n_ws : t;   // (the last tile again: in bounds, unused)
                const float4* wn = p.Wp + (size_t)t_n * G * 64 + lane;
                const float* bp = p.bias + (size_t)t * 32 + 4 * hi;
                float4 bq[4];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) bq[qd] = *reinterpret_cast<const float4*>(bp + 8 * qd);

                // the titled call: the DAE's term of this tile's elements, requested now, consumed in the epilogue (as
                // decode_generic.hip loads mixv).  A half wave reads 32 consecutive rows of one column; a row without
                // answers in this pass -- every row at or past B is one -- and a column that is not ranked form no address
                float mixv[MIX ? RB : 1][16];
                if (MIX) {
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        const int row = rg * R_TILE + rb * 32 + j;
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int lc = t * 32 + 4 * hi + (e & 3) + 8 * (e >> 2);
                            mixv[rb][e] = (len_r[rb] > 0 && lc < p.n_tracks) ? p.mixT[(size_t)lc * p.mix_ld + row] : 0.0f;
                        }
                    }
                }

                f32x16 acc[RB];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb)
#pragma unroll
                    for (int e = 0; e < 16; ++e) acc[rb][e] = 0.0f;

#define RO_STEP(WB, PF, BC, BN, GNEXT)                                                         \
    {                                                                                          \
        const float4 a = WB;                                                                   \
        WB = *(PF);                                                                            \
        const float4* hl = lds4 + (size_t)(GNEXT) * (RB * 64) + lane;                          \
        _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) BN[rb] = hl[rb * 64];                \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        _Pragma("unroll") for (int rb = 0; rb < RB; ++rb)                                      \
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, BC[rb].x, acc[rb], 0, 0, 0);   \
        _Pragma("unroll") for (int rb = 0; rb < RB; ++rb)                                      \
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, BC[rb].y, acc[rb], 0, 0, 0);   \
        _Pragma("unroll") for (int rb = 0; rb < RB; ++rb)                                      \
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, BC[rb].z, acc[rb], 0, 0, 0);   \
        _Pragma("unroll") for (int rb = 0; rb < RB; ++rb)                                      \
            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, BC[rb].w, acc[rb], 0, 0, 0);   \
        __builtin_amdgcn_sched_barrier(0);                                                     \
    }
                int g = 0;
#pragma unroll
                for (; g < G - 4; g += 4) {
                    const float4* pf = wp + (size_t)(g + 4) * 64;
                    RO_STEP(wb0, pf,       bA, bB, g + 1)
                    RO_STEP(wb1, pf + 64,  bB, bA, g + 2)
                    RO_STEP(wb2, pf + 128, bA, bB, g + 3)
                    RO_STEP(wb3, pf + 192, bB, bA, g + 4)
                }
                RO_STEP(wb0, wn,       bA, bB, g + 1)
                RO_STEP(wb1, wn + 64,  bB, bA, g + 2)
                RO_STEP(wb2, wn + 128, bA, bB, g + 3)
                RO_STEP(wb3, wn + 192, bB, bA, 0)
#undef RO_STEP

                // ---- the counting epilogue: lane holds, for row j of row block rb, the columns
                //   tcol0 + (reg & 3) + 8 * (reg >> 2)                                    (reg = 0..15)
                const int tcol0 = t * 32 + 4 * hi;
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    if (len_r[rb] == 0) continue;
                    const unsigned long long* th = lthr + (size_t)(rb * 32 + j) * C;
                    unsigned* cn = lcnt + (size_t)(rb * 32 + j) * C;
#pragma unroll
                    for (int qd = 0; qd < 4; ++qd) {
                        float z4[4] = {acc[rb][4 * qd + 0] + bq[qd].x, acc[rb][4 * qd + 1] + bq[qd].y,
                                       acc[rb][4 * qd + 2] + bq[qd].z, acc[rb][4 * qd + 3] + bq[qd].w};
                        if (MIX) {
                            // THE MIX EPILOGUE: the operations and order of decode_generic.hip's fp32 mix epilogue (title * w_title
                            // + the stored DAE term; two roundings, no contraction), so x == y_a bit for bit at an answer's own column
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const float ts = dae_sigmoidf(z4[e]) * wt_r[rb];
                                z4[e] = ts + mixv[rb][4 * qd + e];
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int col = tcol0 + 8 * qd + e;
                            if (col >= p.n_tracks) continue;     // artists in the last ranked tile, the image's padding
                            const unsigned long long x = ro_comp(z4[e], col);
                            if (x < first[rb]) {
                                ++n0[rb];
                            } else if (x < last[rb]) {
                                // first[] <= x < last[]: the bucket is the first place in [1, len - 1] whose threshold is > x
                                int lo = 1, hi2 = len_r[rb] - 1;
                                while (lo < hi2) {
                                    const int mid = (lo + hi2) >> 1;
                                    if (th[mid] <= x) lo = mid + 1; else hi2 = mid;
                                }
                                atomicAdd(&cn[lo], 1u);
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
            if (n0[rb]) atomicAdd(&lcnt[(size_t)(rb * 32 + j) * C], n0[rb]);
        __syncthreads();
        // ---- this workgroup's buckets -> the global ones ---------------------------------------
        for (int s = tid; s < R_TILE * C; s += RO_THREADS) {
            const int i = s / C, t = s - i * C;
            if (t < llen[i]) {
                const unsigned v = lcnt[s];
                if (v) atomicAdd(&p.gcnt[lbeg[i] + t], v);
            }
        }
        __syncthreads();
    }
}

// the canonical chain of one column over a row held in LDS: acc = fmaf(hrow[k], Wrow[k], acc) over k = 0 .. H-1 from +0 (H % 4 == 0)
__device__ __forceinline__ float ro_chain(const float* hrow, const float* Wrow, int H)
{
    const float4* wr = reinterpret_cast<const float4*>(Wrow);
    float acc = 0.0f;
    const int n4 = H >> 2;
    int k4 = 0;
    for (; k4 + 3 < n4; k4 += 4) {
        float4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wr[k4 + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kb = 4 * (k4 + u);
            acc = fmaf(hrow[kb], w[u].x, acc);
            acc = fmaf(hrow[kb + 1], w[u].y, acc);
            acc = fmaf(hrow[kb + 2], w[u].z, acc);
            acc = fmaf(hrow[kb + 3], w[u].w, acc);
        }
    }
    for (; k4 < n4; ++k4) {
        const float4 w = wr[k4];
        const int kb = 4 * k4;
        acc = fmaf(hrow[kb], w.x, acc);
        acc = fmaf(hrow[kb + 1], w.y, acc);
        acc = fmaf(hrow[kb + 2], w.z, acc);
        acc = fmaf(hrow[kb + 3], w.w, acc);
    }
    return acc;
}

// MIX: the seeds leave by their MIXED value -- both canonical chains and mixf per distinct seed
// GIVEN (dae_ensemble_rank_of; never with MIX): the seeds leave by the value the caller computed for each slot, p.seed_y[] -- no chain
template <bool MIX, bool GIVEN = false>
__global__ __launch_bounds__(256) void rank_of_finish_kernel(const RankP p)
{
    __shared__ float hrow[RO_MAXH];
    __shared__ float frow[MIX ? RO_MAXH : 1];
    __shared__ unsigned long long scomp[256];
    __shared__ int scol[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    int beg, end;
    ro_row_span(p, row, beg, end);
    if (end <= beg) return;
    const float ninf = -__builtin_inff();

    // counts from the buckets; what cannot be ranked by its id
    for (int i = beg + tid; i < end; i += 256) {
        const int c = p.ans_col[i];
        int rank = -1;
        float zl = p.z[i];                                        // (-inf for -1, NaN for an id outside [0, V): candidates.hip)
        if (c >= 0 && c < p.n_tracks) {
            const int c0 = beg + (i - beg) / p.C * p.C;
            const int pos = p.inv[i];
            unsigned s = 0;
            for (int u = 0; u <= pos; ++u) s += p.gcnt[c0 + u];
            rank = (int)s;
        } else if (c >= p.n_tracks && c < p.V) {
            zl = ninf;                                            // an artist column: -inf beside -1
        }
        p.out_rank[i] = rank;
        if (p.out_logit) p.out_logit[i] = zl;
    }
    if (!p.seed_row_ptr) return;
    int sb = p.seed_row_ptr[row], se = p.seed_row_ptr[row + 1];
    if (GIVEN) {                                                  // nothing is read at or past the caller's n_seed
        sb = sb > 0 ? sb : 0;
        se = se < p.n_seed ? se : p.n_seed;
    }
    if (se <= sb) return;
    if (!GIVEN) {
        for (int k = tid; k < RO_MAXH; k += 256) {
            hrow[k] = k < p.H ? p.h[(size_t)row * p.H + k] : 0.0f;
            if (MIX) frow[k] = k < p.HF ? p.feat[(size_t)row * p.HF + k] : 0.0f;
        }
    }
    __syncthreads();                                              // (also orders this workgroup's stores to out_rank before its reads below)

    // the seeds in blocks of 256, a lane each: the canonical chain over the row-major tensor; a seed listed twice counts once
    for (int s0 = sb; s0 < se; s0 += 256) {
        const int si = s0 + tid;
        int c = -1;
        unsigned long long sc = RO_NONE;
        if (si < se) {
            c = p.seed_col[si];
            bool ok = c >= 0 && c < p.n_tracks;
            for (int u = sb; ok && u < si; ++u) ok = p.seed_col[u] != c;
            if (ok && GIVEN) {
                sc = ro_comp(p.seed_y[si], c);
            } else if (ok) {
                const float zd = ro_chain(hrow, p.W + (size_t)c * p.H, p.H) + p.b[c];
                if (MIX) {
                    const float zt = ro_chain(frow, p.WT + (size_t)c * p.HF, p.HF) + p.bT[c];
                    sc = ro_comp(mixf(zt, zd, p.w_title[row], p.w_playlist[row]), c);
                } else {
                    sc = ro_comp(zd, c);
                }
            } else {
                c = -1;
            }
        }
        __syncthreads();
        scomp[tid] = sc; scol[tid] = c;
        __syncthreads();
        const int ns = se - s0 < 256 ? se - s0 : 256;
        for (int i = beg + tid; i < end; i += 256) {
            const int rank = p.out_rank[i];
            if (rank < 0) continue;
            const int ca = p.ans_col[i];
            const unsigned long long a = ro_comp(p.z[i], ca);
            int sub = 0;
            bool is_seed = false;
            for (int u = 0; u < ns; ++u) {
                sub += scomp[u] < a ? 1 : 0;
                is_seed = is_seed || scol[u] == ca;
            }
            if (is_seed) {
                p.out_rank[i] = -1;
                if (p.out_logit) p.out_logit[i] = ninf;
            } else if (sub) {
                p.out_rank[i] = rank - sub;
            }
        }
    }
}

template <int RB, int GT, bool MIX>
int launch_count(dae_ctx* ctx, const dae_ro_plan& pl, const RankP& p)
{
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &rank_of_count_kernel<RB, GT, MIX>, DAE_RO_LDS_BYTES));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    dae_take_profile_events(ctx, "rank_of_count_kernel", e0, e1);
    if (e0) DAE_HIP_CHECK(ctx, hipEventRecord(e0, ctx->stream));
    hipLaunchKernelGGL((rank_of_count_kernel<RB, GT, MIX>), dim3(pl.grid), dim3(RO_THREADS), pl.lds_bytes, ctx->stream, p);
    DAE_CHECK_LAUNCH(ctx, "rank_of_count_kernel");
    if (e1) DAE_HIP_CHECK(ctx, hipEventRecord(e1, ctx->stream));
    return DAE_OK;
}

// the context's fp32 image is a plain one of H-wide rows over [0, V); `who` names the context in the titled call's messages
int check_image(dae_ctx* ctx, const dae_packed& pk, int V, int H, const char* who)
{
    if (!pk.valid) return dae_fail(ctx, DAE_ERR_STATE, "rank_of%s needs a DAE_DTYPE_F32 image of the decoder: none is prepacked", who);
    if (pk.cat_id != 0)
        return dae_fail(ctx, DAE_ERR_STATE, "rank_of%s: the fp32 image is a catalogue image, not one of the vocabulary's own columns", who);
    if (pk.col_lo != 0 || pk.col_hi != V || pk.V != V)
        return dae_fail(ctx, DAE_ERR_STATE, "rank_of%s: the fp32 image is a shard image over [%d, %d) of %d columns, not one over [0, %d)",
                        who, pk.col_lo, pk.col_hi, pk.V, V);
    if (pk.H != H) return dae_fail(ctx, DAE_ERR_ARG, "rank_of%s: H=%d does not match prepacked H=%d", who, H, pk.H);
    return DAE_OK;
}

// everything the entry points refuse, before any launch (the titled call: on the title context, with the title scorer's tensors)
int check_rank_of(dae_ctx* ctx, const void* h_or_enc, int B, int H, const float* W_dec, const float* b_dec, int V, int n_tracks,
                  const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr, const int32_t* ans_col,
                  int n_ans, const int32_t* out_rank, dae_ro_plan* pl, const char* who = "")
{
    if (!h_or_enc || !W_dec || !b_dec || !ans_row_ptr || !ans_col || !out_rank) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (n_ans < 0) return dae_fail(ctx, DAE_ERR_ARG, "n_ans=%d is negative", n_ans);
    if (B < 1 || B > DAE_RO_MAX_B) return dae_fail(ctx, DAE_ERR_ARG, "B=%d out of [1, %d]", B, DAE_RO_MAX_B);
    if (H <= 0 || (H % 4) != 0 || H > RO_MAXH) return dae_fail(ctx, DAE_ERR_ARG, "H=%d must be a multiple of 4 in [4, %d]", H, RO_MAXH);
    if (V <= 0) return dae_fail(ctx, DAE_ERR_ARG, "bad shape V=%d", V);
    if (n_tracks < 1 || n_tracks > V) return dae_fail(ctx, DAE_ERR_ARG, "n_tracks=%d out of [1, V=%d]", n_tracks, V);
    if ((seed_row_ptr == nullptr) != (seed_col == nullptr))
        return dae_fail(ctx, DAE_ERR_ARG, "seed_row_ptr and seed_col must both be given or both null");
    if (reinterpret_cast<uintptr_t>(W_dec) % 16) return dae_fail(ctx, DAE_ERR_ARG, "the decoder tensor must be 16-byte aligned");
    const int rc = check_image(ctx, ctx->pk_f32, V, H, who);
    if (rc) return rc;
    *pl = dae_plan_rank_of(B, H, n_ans);
    if (pl->C <= 0) return dae_fail(ctx, DAE_ERR_ARG, "rank_of: no geometry for B=%d H=%d", B, H);
    return DAE_OK;
}

// the titled call: the DAE's side of the mix (ctx is then the title context, h / H / W_dec / b_dec the title features and tensors)
struct RoMix {
    dae_ctx* dae; const float* h; int H; const float* W_dec; const float* b_dec;
    const float* w_title; const float* w_playlist;
};

// which value is counted and how the seeds leave: the plain logit (their own chain), the title mix (both chains), the ensemble's
// y (the values in p.seed_y)
enum RoMode { RO_PLAIN, RO_MIX, RO_ENSEMBLE };

// The launches every call ends with, once p.z holds the answers' values and the counters are zeroed: the ranking scorer's rows
// h [B][H] packed for this call's row groups, the sort, the count over ctx's fp32 image, the finish.  The caller has filled what
// differs between the calls: the lists, the scratch, the outputs, the row-major tensors and the mix fields of its mode.
int rank_of_launches(dae_ctx* ctx, const dae_ro_plan& pl, RankP& p, const float* h, int B, int H, RoMode mode)
{
    const dae_packed& pk = ctx->pk_f32;
    // the hidden rows in the MFMA operand order, for this call's row groups
    dae_rowgeom g{};
    g.R_TILE = pl.R_TILE; g.n_rg = pl.n_rg; g.Bpad = pl.n_rg * pl.R_TILE; g.nb_rg = pl.nb_rg; g.grid = pl.grid; g.waves = RO_NW;
    // the packed hidden image becomes this call's: its pads are for this geometry (the ranking calls re-zero theirs), no row d
    // belongs to it, and a dae_score_topk_begin waiting for its _finish on this context has lost its rows (it is refused then)
    ctx->row_d_fresh = false;
    ctx->h_geom_key = -1;
    ctx->tk.valid = false;
    int rc = dae_launch_pack_h(ctx, h, B, H, g, nullptr);
    if (rc) return rc;
    p.Wp = static_cast<const float4*>(pk.W.p); p.bias = static_cast<const float*>(pk.bias.p);
    p.hp = static_cast<const float4*>(ctx->h_packed.p);
    p.G = pl.G; p.ntiles_r = (p.n_tracks + 31) / 32;
    p.B = B; p.n_rg = pl.n_rg; p.nb_rg = pl.nb_rg; p.C = pl.C; p.R_TILE = pl.R_TILE;

    hipLaunchKernelGGL(rank_of_prep_kernel, dim3(B), dim3(256), 0, ctx->stream, p);
    DAE_CHECK_LAUNCH(ctx, "rank_of_prep_kernel");
    const bool h256 = pl.G == 32;
    if (mode != RO_PLAIN) {                     // (the run-time k-group count at every width of the ranking scorer's rows)
        switch (pl.R_TILE) {
            case 128: rc = launch_count<4, 0, true>(ctx, pl, p); break;
            case 64:  rc = launch_count<2, 0, true>(ctx, pl, p); break;
            case 32:  rc = launch_count<1, 0, true>(ctx, pl, p); break;
            default:  rc = dae_fail(ctx, DAE_ERR_ARG, "bad R_TILE %d", pl.R_TILE);
        }
    } else {
        switch (pl.R_TILE) {
            case 128: rc = h256 ? launch_count<4, 32, false>(ctx, pl, p) : launch_count<4, 0, false>(ctx, pl, p); break;
            case 64:  rc = h256 ? launch_count<2, 32, false>(ctx, pl, p) : launch_count<2, 0, false>(ctx, pl, p); break;
            case 32:  rc = launch_count<1, 0, false>(ctx, pl, p); break;
            default:  rc = dae_fail(ctx, DAE_ERR_ARG, "bad R_TILE %d", pl.R_TILE);
        }
    }
    if (rc) return rc;
    if (mode == RO_MIX) hipLaunchKernelGGL(rank_of_finish_kernel<true>, dim3(B), dim3(256), 0, ctx->stream, p);
    else if (mode == RO_ENSEMBLE) hipLaunchKernelGGL((rank_of_finish_kernel<false, true>), dim3(B), dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL(rank_of_finish_kernel<false>, dim3(B), dim3(256), 0, ctx->stream, p);
    DAE_CHECK_LAUNCH(ctx, "rank_of_finish_kernel");
    return DAE_OK;
}

int rank_of_core(dae_ctx* ctx, const dae_ro_plan& pl, const float* h, int B, int H, const float* W_dec, const float* b_dec,
                 int V, int n_tracks, const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr,
                 const int32_t* ans_col, int n_ans, int32_t* out_rank, float* out_logit, int32_t* status,
                 const RoMix* mix = nullptr)
{
    if (n_ans == 0) return DAE_OK;
    // scratch: thr [n_ans] u64 | z [n_ans] | inv [n_ans] | gcnt [n_ans] | glen [n_rg]   (gcnt and glen zeroed together)
    const size_t na = (size_t)n_ans;
    const size_t bytes = na * 8 + na * 4 * 3 + (size_t)pl.n_rg * 4;
    int rc = dae_reserve(ctx, ctx->rank_of, bytes);
    if (rc) return rc;
    // the titled call: the DAE's term of the track columns, [n_tracks rounded up to 32, never past the image][B] (dae_title_rank's buffer)
    const size_t nt32 = (size_t)((n_tracks + 31) / 32 * 32 < V ? (n_tracks + 31) / 32 * 32 : V);
    if (mix) {
        rc = dae_reserve(ctx, ctx->title_y1, nt32 * (size_t)B * sizeof(float));
        if (rc) return rc;
    }
    char* base = static_cast<char*>(ctx->rank_of.p);
    RankP p{};
    p.thr = reinterpret_cast<unsigned long long*>(base);
    float* z = reinterpret_cast<float*>(base + na * 8);
    p.z = z;
    p.inv = reinterpret_cast<int*>(base + na * 12);
    p.gcnt = reinterpret_cast<unsigned*>(base + na * 16);
    p.glen = reinterpret_cast<int*>(base + na * 20);

    // (a) the thresholds: the candidate chain(s) over the answers -- the logit, or the mixed value with the DAE's term behind it
    if (mix) {
        rc = dae_mix_candidates(ctx, mix->dae, mix->h, mix->H, mix->H, mix->W_dec, mix->b_dec, h, H, W_dec, b_dec, mix->w_title,
                                mix->w_playlist, B, V, ans_row_ptr, ans_col, n_ans, z, status);
        if (rc) return rc;
        rc = dae_decode_mix_term(mix->dae, mix->h, B, mix->H, DAE_DTYPE_F32, mix->w_playlist, n_tracks,
                                 static_cast<float*>(ctx->title_y1.p), B);
        if (rc) return dae_fail(ctx, rc, "%s", mix->dae->err.c_str());
    } else {
        rc = dae_decode_candidates(ctx, h, H, B, H, W_dec, b_dec, V, ans_row_ptr, ans_col, n_ans, DAE_OUT_LOGIT, z, status);
        if (rc) return rc;
    }
    DAE_HIP_CHECK(ctx, hipMemsetAsync(p.gcnt, 0, na * 4 + (size_t)pl.n_rg * 4, ctx->stream));

    p.n_tracks = n_tracks; p.V = V;
    p.ans_row_ptr = ans_row_ptr; p.ans_col = ans_col; p.n_ans = n_ans;
    p.seed_row_ptr = seed_row_ptr; p.seed_col = seed_col;
    p.h = h; p.H = H; p.W = W_dec; p.b = b_dec;
    p.out_rank = out_rank; p.out_logit = out_logit;
    if (mix) {
        p.h = mix->h; p.H = mix->H; p.W = mix->W_dec; p.b = mix->b_dec;
        p.feat = h; p.HF = H; p.WT = W_dec; p.bT = b_dec;
        p.mixT = static_cast<const float*>(ctx->title_y1.p); p.mix_ld = B;
        p.w_title = mix->w_title; p.w_playlist = mix->w_playlist;
    }
    return rank_of_launches(ctx, pl, p, h, B, H, mix ? RO_MIX : RO_PLAIN);
}

}  // namespace

extern "C" {

int dae_rank_of_plan(int B, int H, int n_ans, int32_t out[4])
{
    if (!out || n_ans < 0) return DAE_ERR_ARG;
    const dae_ro_plan pl = dae_plan_rank_of(B, H, n_ans);
    if (pl.C <= 0) return DAE_ERR_ARG;
    out[0] = pl.R_TILE; out[1] = pl.C; out[2] = pl.n_rg; out[3] = pl.nb_rg;
    return DAE_OK;
}

int dae_decode_rank_of(dae_ctx* ctx, const float* h, int B, int H, const float* W_dec, const float* b_dec, int V, int n_tracks,
                       const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr, const int32_t* ans_col,
                       int n_ans, int32_t* out_rank, float* out_logit, int32_t* status)
{
    if (!ctx) return DAE_ERR_ARG;
    dae_ro_plan pl;
    int rc = check_rank_of(ctx, h, B, H, W_dec, b_dec, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans, out_rank, &pl);
    if (rc) return rc;
    return rank_of_core(ctx, pl, h, B, H, W_dec, b_dec, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans, out_rank,
                        out_logit, status);
}

int dae_score_rank_of(dae_ctx* ctx, const int32_t* row_ptr, const int32_t* col, const float* val, const float* W_enc,
                      const float* b_enc, int V, int H, int B, const float* W_dec, const float* b_dec, int n_tracks,
                      const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr, const int32_t* ans_col,
                      int n_ans, int32_t* out_rank, float* out_logit, int32_t* status)
{
    if (!ctx) return DAE_ERR_ARG;
    if (!row_ptr || !W_enc || !b_enc) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if ((reinterpret_cast<uintptr_t>(W_enc) | reinterpret_cast<uintptr_t>(b_enc)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "W_enc, b_enc must be 16-byte aligned");
    dae_ro_plan pl;
    int rc = check_rank_of(ctx, W_enc, B, H, W_dec, b_dec, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans, out_rank,
                           &pl);
    if (rc) return rc;
    if (n_ans == 0) return DAE_OK;
    rc = dae_reserve(ctx, ctx->h_scratch, (size_t)B * H * sizeof(float));      // the hidden rows stay in the context, as dae_score_candidates'
    if (rc) return rc;
    float* h = static_cast<float*>(ctx->h_scratch.p);
    rc = dae_launch_encode(ctx, row_ptr, col, val, W_enc, b_enc, V, H, B, 1.0f, 1.0f, 0u, h, nullptr, 0, 0);
    if (rc) return rc;
    return rank_of_core(ctx, pl, h, B, H, W_dec, b_dec, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans, out_rank,
                        out_logit, status);
}

int dae_mix_rank_of(dae_ctx* title_ctx, dae_ctx* dae, const float* h, int64_t ld_h, int H, const float* W_dec,
                    const float* b_dec, const float* feat, int64_t ld_feat, const float* OutW_T, const float* Out_b,
                    const float* w_title, const float* w_playlist, int B, int V, int n_tracks,
                    const int32_t* seed_row_ptr, const int32_t* seed_col, const int32_t* ans_row_ptr,
                    const int32_t* ans_col, int n_ans, int32_t* out_rank, float* out_score, int32_t* status)
{
    dae_ctx* ctx = title_ctx;
    if (!ctx) return DAE_ERR_ARG;
    if (!dae || dae == ctx) return dae_fail(ctx, DAE_ERR_ARG, "dae_mix_rank_of: needs the DAE's context");
    if (!h || !W_dec || !b_dec || !w_title || !w_playlist) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (ctx->device != dae->device) return dae_fail(ctx, DAE_ERR_ARG, "dae_mix_rank_of: contexts on different devices");
    if (ctx->stream != dae->stream) return dae_fail(ctx, DAE_ERR_STATE, "both contexts must be bound to the same stream");
    if (ctx->mixT) return dae_fail(ctx, DAE_ERR_STATE, "dae_mix_rank_of sets the mix itself: clear dae_set_score_mix on the title context");
    if (dae->mixT) return dae_fail(ctx, DAE_ERR_STATE, "dae_mix_rank_of: clear dae_set_score_mix on the DAE's context");
    if (H <= 0 || (H % 4) != 0 || H > RO_MAXH) return dae_fail(ctx, DAE_ERR_ARG, "H=%d must be a multiple of 4 in [4, %d]", H, RO_MAXH);
    if (ld_h != H) return dae_fail(ctx, DAE_ERR_ARG, "ld_h=%lld: contiguous hidden rows (ld_h == H = %d) are required", (long long)ld_h, H);
    if (ld_feat <= 0 || (ld_feat % 4) != 0 || ld_feat > RO_MAXH)
        return dae_fail(ctx, DAE_ERR_ARG, "ld_feat=%lld must be a multiple of 4 in [4, %d]", (long long)ld_feat, RO_MAXH);
    if ((reinterpret_cast<uintptr_t>(W_dec) | reinterpret_cast<uintptr_t>(OutW_T)) % 16)
        return dae_fail(ctx, DAE_ERR_ARG, "the decoder tensor and Output_W^T must be 16-byte aligned");
    dae_ro_plan pl;
    int rc = check_rank_of(ctx, feat, B, (int)ld_feat, OutW_T, Out_b, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans,
                           out_rank, &pl, " (the title context)");
    if (rc) return rc;
    rc = check_image(ctx, dae->pk_f32, V, H, " (the DAE's context)");
    if (rc) return rc;
    const RoMix mix{dae, h, H, W_dec, b_dec, w_title, w_playlist};
    return rank_of_core(ctx, pl, feat, B, (int)ld_feat, OutW_T, Out_b, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans,
                        out_rank, out_score, status, &mix);
}

// THE ENSEMBLE'S CALL (DESIGN.md section 4e "Ranks under the ensemble"): the ranks under the canonical value y of a weighted sum
// of M members (+ the title scorer), on the ranking context of dae_ensemble_topk.  The thresholds and the seeds' values come from
// the candidate chains (ensemble.hip), the other scorers' terms from the transposed buffer dae_ensemble_topk builds, and the
// counting launch is the MIX instantiation over the ranking scorer's image: its epilogue, fl(fl(sigmoid(z_rank) * w) + accT), is
// the combining kernel's last two operations on the same operands, so an answer's own column meets its own value.
int dae_ensemble_rank_of(dae_ctx* const* members, int M, const float* const* h, const int* H, const float* const* row_scale,
                         const float* const* W_dec, const float* const* b_dec, dae_ctx* title_ctx, const float* feat, int ld_feat,
                         const float* OutW_T, const float* Out_b, const float* w_title, int B, int V, int n_tracks,
                         const int32_t* seed_row_ptr, const int32_t* seed_col, int n_seed, const int32_t* ans_row_ptr,
                         const int32_t* ans_col, int n_ans, int32_t* out_rank, float* out_score, int32_t* status)
{
    static const char* fn = "dae_ensemble_rank_of";
    if (!members || M < 1 || !members[M - 1]) return dae_fail(title_ctx, DAE_ERR_ARG, "%s: needs M >= 1 member contexts", fn);
    const bool titled = title_ctx != nullptr;
    dae_ctx* ctx = titled ? title_ctx : members[M - 1];                    // the ranking context: it takes the messages too
    if (!h || !H || !row_scale || !W_dec || !b_dec) return dae_fail(ctx, DAE_ERR_ARG, "null pointer");
    if (titled ? (!feat || !w_title || !OutW_T || !Out_b) : (feat || w_title || OutW_T || Out_b))
        return dae_fail(ctx, DAE_ERR_ARG, titled ? "null pointer (feat / Output_W^T / Output_b / w_title of the title context)"
                                                 : "%s: title tensors without a title context", fn);
    int Vimg = 0;
    int rc = dae_ensemble_check(fn, ctx, members, M, h, H, row_scale, title_ctx, ld_feat, DAE_DTYPE_F32, &Vimg);
    if (rc) return rc;
    if (V != Vimg) return dae_fail(ctx, DAE_ERR_ARG, "%s: V=%d, the images hold %d columns", fn, V, Vimg);
    for (int m = 0; m < M; ++m) {
        if (!W_dec[m] || !b_dec[m]) return dae_fail(ctx, DAE_ERR_ARG, "null pointer (W_dec / b_dec of member %d)", m);
        if (H[m] <= 0 || (H[m] % 4) != 0 || H[m] > RO_MAXH)
            return dae_fail(ctx, DAE_ERR_ARG, "H=%d of member %d must be a multiple of 4 in [4, %d]", H[m], m, RO_MAXH);
        if (reinterpret_cast<uintptr_t>(W_dec[m]) % 16)
            return dae_fail(ctx, DAE_ERR_ARG, "the decoder tensor of member %d must be 16-byte aligned", m);
    }
    // the ranking scorer: its rows, row width and row-major tensors
    const float* hr = titled ? feat : h[M - 1];
    const int Hr = titled ? ld_feat : H[M - 1];
    const float* Wr = titled ? OutW_T : W_dec[M - 1];
    const float* br = titled ? Out_b : b_dec[M - 1];
    dae_ro_plan pl;
    rc = check_rank_of(ctx, hr, B, Hr, Wr, br, V, n_tracks, seed_row_ptr, seed_col, ans_row_ptr, ans_col, n_ans, out_rank, &pl,
                       titled ? " (the title context)" : " (the last member's context)");
    if (rc) return rc;
    if (n_seed < 0) return dae_fail(ctx, DAE_ERR_ARG, "n_seed=%d is negative", n_seed);
    if (n_seed > 0 && !seed_col) return dae_fail(ctx, DAE_ERR_ARG, "n_seed=%d without a seed CSR", n_seed);
    if (n_ans == 0) return DAE_OK;
    const bool seeded = seed_col != nullptr && n_seed > 0;

    const int K = M + (titled ? 1 : 0);
    const dae_ens_scratch sp = dae_plan_ensemble_scratch(K, n_ans, seeded ? n_seed : 0, pl.n_rg);
    rc = dae_reserve(ctx, ctx->rank_of, sp.total);
    if (rc) return rc;
    const size_t nt32 = (size_t)((n_tracks + 31) / 32 * 32 < V ? (n_tracks + 31) / 32 * 32 : V);
    rc = dae_reserve(ctx, ctx->title_y1, nt32 * (size_t)B * sizeof(float));
    if (rc) return rc;
    char* base = static_cast<char*>(ctx->rank_of.p);
    float* z = reinterpret_cast<float*>(base + sp.o_z);
    float* seed_y = reinterpret_cast<float*>(base + sp.o_seed_y);
    float* s = reinterpret_cast<float*>(base + sp.o_s);
    float* accT = static_cast<float*>(ctx->title_y1.p);

    // 1. the thresholds, 2. the seeds' values (a status word of their own: none -- an out-of-range seed is ignored, as ever)
    const dae_ens_tensors t{M, h, H, row_scale, W_dec, b_dec, feat, ld_feat, OutW_T, Out_b, w_title};
    rc = dae_launch_ensemble_candidates(ctx, t, B, V, ans_row_ptr, ans_col, n_ans, s, sp.s_stride, z, status);
    if (rc) return rc;
    if (seeded) {
        rc = dae_launch_ensemble_candidates(ctx, t, B, V, seed_row_ptr, seed_col, n_seed, s, sp.s_stride, seed_y, nullptr);
        if (rc) return rc;
    }
    // 3. the other scorers' terms, transposed: dae_ensemble_topk's buffer
    const int n_acc = titled ? M : M - 1;
    if (n_acc == 0)
        DAE_HIP_CHECK(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(accT), (int)0x80000000u, nt32 * (size_t)B, ctx->stream));
    for (int m = 0; m < n_acc; ++m) {
        dae_ctx* c = members[m];
        rc = m == 0 ? dae_decode_mix_term(c, h[m], B, H[m], DAE_DTYPE_F32, row_scale[m], n_tracks, accT, B)
                    : dae_decode_mix_term_add(c, h[m], B, H[m], DAE_DTYPE_F32, row_scale[m], n_tracks, accT, B);
        if (rc) return dae_fail(ctx, rc, "%s", c->err.c_str());
    }
    DAE_HIP_CHECK(ctx, hipMemsetAsync(base + sp.o_gcnt, 0, sp.zero_bytes, ctx->stream));

    // 4. the count over the ranking scorer's image, 5. the finish: the seeds leave by seed_y
    RankP p{};
    p.thr = reinterpret_cast<unsigned long long*>(base + sp.o_thr);
    p.z = z;
    p.inv = reinterpret_cast<int*>(base + sp.o_inv);
    p.gcnt = reinterpret_cast<unsigned*>(base + sp.o_gcnt);
    p.glen = reinterpret_cast<int*>(base + sp.o_glen);
    p.n_tracks = n_tracks; p.V = V;
    p.ans_row_ptr = ans_row_ptr; p.ans_col = ans_col; p.n_ans = n_ans;
    p.seed_row_ptr = seeded ? seed_row_ptr : nullptr; p.seed_col = seeded ? seed_col : nullptr;
    p.seed_y = seed_y; p.n_seed = seeded ? n_seed : 0;
    p.out_rank = out_rank; p.out_logit = out_score;
    p.mixT = accT; p.mix_ld = B;
    p.w_title = titled ? w_title : row_scale[M - 1];
    return rank_of_launches(ctx, pl, p, hr, B, Hr, RO_ENSEMBLE);
}

}  // extern "C"
