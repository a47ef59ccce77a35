// mix_filter.hip -- the two vocabulary-wide passes of the exact title mix (mixexact.hip has the overview): both scorers' GEMMs
// on v_mfma_f32_32x32x16_bf16 in one launch, on BOUNDS of the two logits (mix_common.h).
//   sample (MODE 1): biases shifted down -> the maxima over groups of 4 columns of the lower bounds of y, over the head of the
//          bias-ordered tile list;
//   filter (MODE 0): biases shifted up -> a column is listed with its pair of upper logits when its upper bound can reach tau.
// Two kernels share one tile walk: mix_bf16_kernel, unrolled over the shipped shape's 44 steps, and mix_bf16_steps_kernel,
// whose step counts are run-time values.  Each keeps what is its own -- how the hidden rows are staged into LDS and how the W
// ring walks a tile's steps -- and calls the pieces below for the rest.
#include "decode_common.h"
#include "mix_common.h"

namespace {

struct MixP {
    const uint4* WqD; const uint4* WqT;          // bf16 images [tile][NS][64] of the two scorers (same tiles: column 32 t + i)
    const uint4* biasD; const uint4* biasT;      // [tile][64] bias fragments: the lower or the upper shift
    const uint4* hp;                             // hidden rows of both scorers [n_rg][NSD + NST][RB][64] (mix_prep.hip mix_pack_body)
    const unsigned* fhat;                        // [Bpad] bf16 bits of F_r, rounded up
    const float* w_t; const float* w_p;          // [B]
    const float* tau;                            // [B] (filter)
    const int* list; int n_items;                // tiles of this launch
    int n_valid_col;                             // rankable columns (the images start at column 0)
    int B, n_rg, nb_rg, Bpad;
    uint4* cand; int* cand_cnt; int cap;         // filter: [bir][Bpad][cap] entries (u_t, u_d, column, 0) + [bir][Bpad] counts
    float* samp; int64_t ld_s;                   // sample: [B][ld_s] maxima of 4-column groups, element item * 8 + 4 hi + qd
    int nsD, nsT;                                // mix_bf16_steps_kernel: MFMA steps of the two images (H / 16, both multiples of 4)
};

// ---- the two epilogues of a decoded tile: lane = playlist j of row block rb; register reg is column
// 32 t + 4 hi + (reg & 3) + 8 (reg >> 2)
// filter (MODE 0): the columns whose pair of upper logits can reach the row's threshold go to the row's candidate segment
template <int RB>
__device__ __forceinline__ void mix_filter_epilogue(const MixP& p, const f32x16 (&accD)[RB], const f32x16 (&accT)[RB],
                                                    const float (&tau_r)[RB], const float (&wt_r)[RB], const float (&wp_r)[RB],
                                                    int* lcnt, int t, int rg, int bir, int hi, int j)
{
    constexpr int R_TILE = RB * 32;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const float tv = tau_r[rb], wt = wt_r[rb], wp = wp_r[rb];
        float mT = accT[rb][0], mD = accD[rb][0];
#pragma unroll
        for (int reg = 1; reg < 16; ++reg) { mT = fmaxf(mT, accT[rb][reg]); mD = fmaxf(mD, accD[rb][reg]); }
        // (the pair of maxima bounds every pair of the lane's 16 columns)
        if (mix_can_reach(mT, mD, wt, wp, tv)) {
            // one compare pair per element first (mix_thresholds); the exact test only for the registers in which SOME lane
            // of the wave still has a column in play (wave-uniform: __ballot)
            float th_t, th_d;
            mix_thresholds(mT, mD, wt, wp, tv, th_t, th_d);
            unsigned pm = 0;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                if (accT[rb][reg] >= th_t && accD[rb][reg] >= th_d) pm |= 1u << reg;
            unsigned m = 0;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                if (__ballot((pm >> reg) & 1u)) {
                    const int lc = t * 32 + 4 * hi + (reg & 3) + 8 * (reg >> 2);
                    if (((pm >> reg) & 1u) && mix_can_reach(accT[rb][reg], accD[rb][reg], wt, wp, tv) && lc < p.n_valid_col)
                        m |= 1u << reg;
                }
            }
            if (m) {
                int at = atomicAdd(&lcnt[rb * 32 + j], __popc(m));
                uint4* dst = p.cand + ((size_t)bir * p.Bpad + rg * R_TILE + rb * 32 + j) * (size_t)p.cap;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    if (m & (1u << reg))
                        dst[at++] = make_uint4(__float_as_uint(accT[rb][reg]), __float_as_uint(accD[rb][reg]),
                                               (unsigned)(t * 32 + 4 * hi + (reg & 3) + 8 * (reg >> 2)), 0u);
                }
            }
        }
    }
}
// sample (MODE 1): the maxima of the lower bounds of y over groups of 4 columns, stored per list item `it`
template <int RB>
__device__ __forceinline__ void mix_sample_epilogue(const MixP& p, const f32x16 (&accD)[RB], const f32x16 (&accT)[RB],
                                                    const float (&wt_r)[RB], const float (&wp_r)[RB], int t, int it, int rg, int hi, int j)
{
    constexpr int R_TILE = RB * 32;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int row = rg * R_TILE + rb * 32 + j;
        float o[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {
            float mx = -__builtin_inff();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int lc = t * 32 + 4 * hi + e + 8 * qd;
                const float y = mix_fast_dn(accT[rb][4 * qd + e], accD[rb][4 * qd + e], wt_r[rb], wp_r[rb]);
                if (lc < p.n_valid_col) mx = fmaxf(mx, y);
            }
            o[qd] = mx;
        }
        if (row < p.B)
            *reinterpret_cast<float4*>(p.samp + (size_t)row * p.ld_s + (size_t)it * 8 + 4 * hi) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- the tile walk both kernels share, piece by piece in the order a kernel calls them --------------------------------------
// the workgroups that walk the same tiles for different row groups sit on one XCD (decode_f32.hip)
__device__ __forceinline__ void mix_block_map(const MixP& p, int& rg, int& bir)
{
    const int gs = DAE_NUM_XCD * p.n_rg;
    const int q = blockIdx.x / gs, rem = blockIdx.x % gs;
    rg = rem / DAE_NUM_XCD;
    bir = q * DAE_NUM_XCD + (rem % DAE_NUM_XCD);
}
// a wave's tiles: its first two by position (here), every further one claimed from a counter in LDS (mix_claim; decode_f32.hip)
__device__ __forceinline__ void mix_first_tiles(const MixP& p, int it0, int n_ws, int& tv0, int& tv1)
{
    const bool has = it0 < p.n_items;
    tv0 = p.list[has ? it0 : 0];
    tv1 = p.list[has ? (it0 + n_ws < p.n_items ? it0 + n_ws : it0) : 0];
}
// filter: the threshold of the row thread tid stands for (rows beyond B list nothing)
// (every load of this prologue is UNCONDITIONAL, on a clamped row: a guarded load is a branch, and hipcc ends each guarded
// group on s_waitcnt vmcnt(0) -- eight dependent trips to memory before the first MFMA, round 6's ISA reading)
template <int R_TILE, int MODE>
__device__ __forceinline__ float mix_row_tau(const MixP& p, int rg, int tid)
{
    float tau_g = __builtin_inff();
    if (MODE == 0) {
        const int rr = rg * R_TILE + (tid < R_TILE ? tid : 0);
        const int rc = rr < p.B ? rr : p.B - 1;
        const float tau = p.tau[rc];
        const float a_t = p.w_t[rc], a_p = p.w_p[rc];
        if (tid < R_TILE && rr < p.B) {
            // the compared bound is widened by 2^-20 and rounded twice; tau <= 0 (or -inf: fewer than `need` sample values,
            // or NaN): every column passes
            tau_g = tau > 0.0f ? tau * (1.0f - 0x1p-17f) : 0.0f;
            // a row without input and without title (the padding rows of a reader's last batch, main_challenge.py:75-78): both
            // weights are 0, y is +0 for every column -- nothing is listed, the refine launch writes its list directly
            if (a_t == 0.0f && a_p == 0.0f) tau_g = __builtin_inff();
        }
    }
    return tau_g;
}
// LDS behind the n_h4 uint4 of hidden rows: per row a candidate count and a threshold, then the claim counter (mix_plan.h
// lds_bytes); the counter starts behind the two tiles per wave that go by position
struct MixTail { int* lcnt; float* ltau; int* claim; };
template <int R_TILE, int NW>
__device__ __forceinline__ MixTail mix_lds_tail(float4* lds4, int n_h4, int tid)
{
    MixTail tl;
    tl.lcnt = reinterpret_cast<int*>(lds4 + n_h4);
    tl.ltau = reinterpret_cast<float*>(tl.lcnt + R_TILE);
    tl.claim = reinterpret_cast<int*>(tl.ltau + R_TILE);
    if (tid == 0) *tl.claim = 2 * NW;
    return tl;
}
// a lane's row: its mixing weights (0 beyond B) and oy, the .y word of the title side's "ones" fragment -- k-slot 2 is 1.0,
// k-slot 3 the row's feature bound F_r.  (The arrays' fields by value, not the argument block: the form that leaves the
// kernels' code as it was.)
__device__ __forceinline__ void mix_lane_row(const float* w_t, const float* w_p, const unsigned* fhat, int B, int row, int hi,
                                             float& wt, float& wp, unsigned& oy)
{
    const bool in = row < B;
    const int rc = in ? row : B - 1;
    const float a_t = w_t[rc], a_p = w_p[rc];
    const unsigned fh = fhat[rc];
    wt = in ? a_t : 0.0f;
    wp = in ? a_p : 0.0f;
    oy = hi == 0 ? (0x3F80u | ((in ? fh : 0u) << 16)) : 0u;
}
// the list position of the wave's next tile but one
__device__ __forceinline__ int mix_claim(int* claim, int lane, int nb_rg, int bir)
{
    int n2 = 0;
    if (lane == 0) n2 = atomicAdd(claim, 1);
    return __builtin_amdgcn_readfirstlane(n2) * nb_rg + bir;
}
// a tile's accumulators START at the shifted bias (and, title side, at -+alpha_c F_r): the tile's bias fragment goes through the
// matrix pipe against the row's "ones" fragment
__device__ __forceinline__ f32x16 mix_bias_acc(const uint4 b, const uint4 ones)
{
    f32x16 zero;
#pragma unroll
    for (int e = 0; e < 16; ++e) zero[e] = 0.0f;
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(b), as_bf16x8(ones), zero, 0, 0, 0);
}
// (What ends a tile -- the epilogue by MODE, the wave moving on to its next tile -- and the count store behind the loop are four
// lines each and stay in the kernels: as helpers, in every form tried, they reordered instructions of the filter instances.)

// ---- the shipped shape (hidden 256, rows of 448): both images' step counts are template arguments, the tile unrolled ------
template <int NSD, int NST, int RB, int QR, int NW, int MODE>
__global__ __launch_bounds__(NW * 64, 1) void mix_bf16_kernel(const MixP p)
{
    constexpr int NS = NSD + NST, R_TILE = RB * 32, NTH = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;
    int rg, bir;
    mix_block_map(p, rg, bir);

    constexpr int n_h4 = RB * 64 * NS;
    constexpr int PER = (n_h4 + NTH - 1) / NTH;
    constexpr int CH = PER < 8 ? PER : 8;
    const int n_items = p.n_items;
    const int n_ws = p.nb_rg * NW;
    const int it0 = wave * p.nb_rg + bir;
    const uint4* ldsq = reinterpret_cast<const uint4*>(lds4);

    int tv0, tv1;
    mix_first_tiles(p, it0, n_ws, tv0, tv1);
    static_assert(R_TILE <= NTH, "one thread per row");
    const float tau_g = mix_row_tau<R_TILE, MODE>(p, rg, tid);
    const MixTail tl = mix_lds_tail<R_TILE, NW>(lds4, n_h4, tid);
    {
        const uint4* hsrc = p.hp + (size_t)rg * n_h4;
        uint4* l4 = reinterpret_cast<uint4*>(lds4);
#pragma unroll
        for (int e0 = 0; e0 < PER; e0 += CH) {
            uint4 hv[CH];
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int i = (e0 + e) * NTH + tid;
                hv[e] = hsrc[i < n_h4 ? i : n_h4 - 1];
            }
#pragma unroll
            for (int e = 0; e < CH; ++e) {
                const int i = (e0 + e) * NTH + tid;
                if (e0 + e < PER && i < n_h4) l4[i] = hv[e];
            }
        }
    }
    if (tid < R_TILE) { tl.lcnt[tid] = 0; tl.ltau[tid] = tau_g; }
    // per lane: the mixing weights and the row's feature bound of its RB rows
    float wt_r[RB], wp_r[RB];
    unsigned oy[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) mix_lane_row(p.w_t, p.w_p, p.fhat, p.B, rg * R_TILE + rb * 32 + j, hi, wt_r[rb], wp_r[rb], oy[rb]);
    __builtin_amdgcn_sched_barrier(0);
    int t = __builtin_amdgcn_readfirstlane(tv0), u = __builtin_amdgcn_readfirstlane(tv1);
    // step sg of tile x: the DAE image's steps first, then the title image's
    auto wsrc = [&](int x, int sg) -> const uint4* {
        return sg < NSD ? p.WqD + ((size_t)x * NSD + sg) * 64 + lane : p.WqT + ((size_t)x * NST + (sg - NSD)) * 64 + lane;
    };
    uint4 wq[QR];
    uint4 cb[2][RB];
    uint4 bfD = p.biasD[(size_t)t * 64 + lane], bfT = p.biasT[(size_t)t * 64 + lane];
#pragma unroll
    for (int k = 0; k < QR; ++k) wq[k] = *wsrc(t, k);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    float tau_r[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) tau_r[rb] = tl.ltau[rb * 32 + j];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) cb[0][rb] = ldsq[rb * 64 + lane];
    const uint4 onesD = hi == 0 ? make_uint4(0x3F803F80u, 0x00003F80u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);

    int g_nxt = it0 + n_ws;
    for (int it = it0; it < n_items;) {
        const int g_nn = mix_claim(tl.claim, lane, p.nb_rg, bir);
        const int wv = p.list[g_nn < n_items ? g_nn : it];       // consumed at the end of this tile

        f32x16 accD[RB], accT[RB];
        {
            const uint4 bd = bfD, bt = bfT;                      // this tile's; the next tile's are requested
            bfD = p.biasD[(size_t)u * 64 + lane];
            bfT = p.biasT[(size_t)u * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                accD[rb] = mix_bias_acc(bd, onesD);
                accT[rb] = mix_bias_acc(bt, hi == 0 ? make_uint4(0x3F803F80u, oy[rb], 0u, 0u) : make_uint4(0u, 0u, 0u, 0u));
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int sn = (s + 1) % NS;
            const uint4 a = wq[s % QR];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                if (s < NSD)
                    accD[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(cb[s & 1][rb]), accD[rb], 0, 0, 0);
                else
                    accT[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(cb[s & 1][rb]), accT[rb], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                cb[(s + 1) & 1][rb] = ldsq[(sn * RB + rb) * 64 + lane];
                __builtin_amdgcn_sched_barrier(0);
            }
            wq[s % QR] = (s + QR < NS) ? *wsrc(t, s + QR) : *wsrc(u, s + QR - NS);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (MODE == 0) mix_filter_epilogue<RB>(p, accD, accT, tau_r, wt_r, wp_r, tl.lcnt, t, rg, bir, hi, j);
        else mix_sample_epilogue<RB>(p, accD, accT, wt_r, wp_r, t, it, rg, hi, j);
        t = u; u = __builtin_amdgcn_readfirstlane(wv);
        it = g_nxt; g_nxt = g_nn;
    }
    if (MODE == 0) {
        __syncthreads();
        for (int i = tid; i < R_TILE; i += NTH) p.cand_cnt[(size_t)bir * p.Bpad + rg * R_TILE + i] = tl.lcnt[i];
    }
}

// ---- the same launch at the other supported shapes (dae_mix_shape_ok): step counts at run time ---------------------------
// mix_bf16_kernel is unrolled over its 44 steps; an instance per shape (7 hidden sizes x 8 row lengths x 2 modes) is not an
// option.  Here a tile is two run-time loops -- the DAE image's steps into accD, then the title image's into accT -- over
// CHUNKS of 8 steps, unrolled inside the chunk.  The W ring is one chunk: slot i, once step i has been issued, takes step i
// of the NEXT chunk -- of the same image, of the other image, or of the next tile -- 8 steps ahead as in mix_bf16_kernel,
// with no assumption on the title image's step count but "at least 4, a multiple of 4" (row lengths are multiples of 64).
// REQUIRES nsD >= 8 and a multiple of 4 (hidden >= 128, a multiple of 64: dae_mix_shape_ok): the prologue and the refill
// across the tile boundary load the DAE image's first EIGHT steps of a tile -- with nsD = 4 (hidden 64) they would read past
// the tile's DAE steps; whoever widens the predicate gives those two places the half-chunk addresses first.  An image of 8 m + 4 steps ends on a HALF chunk: steps 4 .. 7 of it multiply nothing, and their slots are loaded
// all the same (slots 4 .. 7 of a half chunk repeat the addresses of slots 0 .. 3) -- EVERY chunk issues its 8 loads, so
// the count of loads in flight is the same on every path and the s_waitcnt vmcnt(n) before a step waits for that step's
// slot only (a skipped load would make it wait for the youngest one: a ring one step deep).
template <int RB, int NW, int MODE>
__global__ __launch_bounds__(NW * 64, 1) void mix_bf16_steps_kernel(const MixP p)
{
    constexpr int R_TILE = RB * 32, NTH = NW * 64;
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;
    const int NSD = p.nsD, NST = p.nsT, NS = NSD + NST;
    int rg, bir;
    mix_block_map(p, rg, bir);

    const int n_h4 = RB * 64 * NS;
    const int n_items = p.n_items;
    const int n_ws = p.nb_rg * NW;
    const int it0 = wave * p.nb_rg + bir;
    const uint4* ldsq = reinterpret_cast<const uint4*>(lds4);

    int tv0, tv1;
    mix_first_tiles(p, it0, n_ws, tv0, tv1);
    static_assert(R_TILE <= NTH, "one thread per row");
    const float tau_g = mix_row_tau<R_TILE, MODE>(p, rg, tid);
    const MixTail tl = mix_lds_tail<R_TILE, NW>(lds4, n_h4, tid);
    {
        // the row group's hidden rows of both scorers, 4 loads in flight per thread and round.  Loads AND stores on the clamped
        // index: no branch (hipcc sinks a load into the branch that guards its store and waits for each there); the threads
        // past the end store the last element a second time
        const uint4* hsrc = p.hp + (size_t)rg * n_h4;
        uint4* l4 = reinterpret_cast<uint4*>(lds4);
        for (int e0 = 0; e0 < n_h4; e0 += 4 * NTH) {
            uint4 hv[4];
            int ic[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = e0 + e * NTH + tid;
                ic[e] = i < n_h4 ? i : n_h4 - 1;
                hv[e] = hsrc[ic[e]];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) l4[ic[e]] = hv[e];
        }
    }
    if (tid < R_TILE) { tl.lcnt[tid] = 0; tl.ltau[tid] = tau_g; }
    // per lane: the mixing weights and the row's feature bound of its RB rows
    float wt_r[RB], wp_r[RB];
    unsigned oy[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) mix_lane_row(p.w_t, p.w_p, p.fhat, p.B, rg * R_TILE + rb * 32 + j, hi, wt_r[rb], wp_r[rb], oy[rb]);
    int t = __builtin_amdgcn_readfirstlane(tv0), u = __builtin_amdgcn_readfirstlane(tv1);
    // this lane's uint4 of step sg of an image, tile x; the following steps of the tile at [64], [128], ...
    auto wD = [&](int x, int sg) -> const uint4* { return p.WqD + ((size_t)x * NSD + sg) * 64 + lane; };
    auto wT = [&](int x, int sg) -> const uint4* { return p.WqT + ((size_t)x * NST + sg) * 64 + lane; };
    uint4 wq[8];
    uint4 cb[2][RB];
    uint4 bfD = p.biasD[(size_t)t * 64 + lane], bfT = p.biasT[(size_t)t * 64 + lane];
    {
        const uint4* a = wD(t, 0);                                // (nsD >= 8)
#pragma unroll
        for (int i = 0; i < 8; ++i) wq[i] = a[i * 64];
    }
    __syncthreads();

    float tau_r[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) tau_r[rb] = tl.ltau[rb * 32 + j];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) cb[0][rb] = ldsq[rb * 64 + lane];
    const uint4 onesD = hi == 0 ? make_uint4(0x3F803F80u, 0x00003F80u, 0u, 0u) : make_uint4(0u, 0u, 0u, 0u);

    int g_nxt = it0 + n_ws;
    for (int it = it0; it < n_items;) {
        const int g_nn = mix_claim(tl.claim, lane, p.nb_rg, bir);
        const int wv = p.list[g_nn < n_items ? g_nn : it];       // consumed at the end of this tile

        f32x16 accD[RB], accT[RB];
        {
            const uint4 bd = bfD, bt = bfT;                      // this tile's; the next tile's are requested
            bfD = p.biasD[(size_t)u * 64 + lane];
            bfT = p.biasT[(size_t)u * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                accD[rb] = mix_bias_acc(bd, onesD);
                accT[rb] = mix_bias_acc(bt, hi == 0 ? make_uint4(0x3F803F80u, oy[rb], 0u, 0u) : make_uint4(0u, 0u, 0u, 0u));
            }
        }
        // a chunk of n (8, or 4: the image's last 4 steps) steps, the first one step s0 of the tile (the order of the rows in
        // LDS); the ring then holds the chunk at `next`, of n_next steps.  Only the multiplications of steps 4 .. 7 depend on n:
        // the loads are straight-line code
        auto chunk = [&](f32x16 (&acc)[RB], int s0, int n, const uint4* next, int n_next) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < 4 || n == 8) {
                    const int s = s0 + i;
                    const uint4* bn = ldsq + (size_t)(s + 1 == NS ? 0 : s + 1) * (RB * 64) + lane;      // the B operands of the step after
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(wq[i]), as_bf16x8(cb[i & 1][rb]), acc[rb], 0, 0, 0);
                        __builtin_amdgcn_sched_barrier(0);
                        cb[(i + 1) & 1][rb] = bn[rb * 64];
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                wq[i] = next[(i < 4 || n_next == 8 ? i : i - 4) * 64];
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        for (int s0 = 0; s0 < NSD; s0 += 8) {                     // the DAE image; after its last chunk: the title image's first
            const int sn = s0 + 8;
            const bool more = sn < NSD;
            chunk(accD, s0, NSD - s0 < 8 ? 4 : 8, more ? wD(t, sn) : wT(t, 0), (more ? NSD - sn : NST) < 8 ? 4 : 8);
        }
        for (int s0 = 0; s0 < NST; s0 += 8) {                     // the title image; after its last chunk: the next tile
            const int sn = s0 + 8;
            const bool more = sn < NST;
            chunk(accT, NSD + s0, NST - s0 < 8 ? 4 : 8, more ? wT(t, sn) : wD(u, 0), (more ? NST - sn : NSD) < 8 ? 4 : 8);
        }
        if (MODE == 0) mix_filter_epilogue<RB>(p, accD, accT, tau_r, wt_r, wp_r, tl.lcnt, t, rg, bir, hi, j);
        else mix_sample_epilogue<RB>(p, accD, accT, wt_r, wp_r, t, it, rg, hi, j);
        t = u; u = __builtin_amdgcn_readfirstlane(wv);
        it = g_nxt; g_nxt = g_nn;
    }
    if (MODE == 0) {
        __syncthreads();
        for (int i = tid; i < R_TILE; i += NTH) p.cand_cnt[(size_t)bir * p.Bpad + rg * R_TILE + i] = tl.lcnt[i];
    }
}

}  // namespace

// One pass of the launch pair over `order`, the DAE image's tiles by their largest bias: the sample over its first pl.n_samp
// tiles (lower bounds; maxima to tc->gmax), or the filter over all pl.ntr (upper bounds against tc->tau; candidates to
// tc->cand / tc->cand_cnt).  The hidden rows and F_r are those dae_launch_mix_prep_pack left in tc.
int dae_launch_mix_pass(dae_ctx* tc, const dae_mix_plan& pl, bool sample, const dae_packed& pd, const dae_packed& pt, const int* order,
                        const dae_mix_call& c)
{
    constexpr int NW = MX_NW, QR = MX_QR;
    MixP p;
    memset(&p, 0, sizeof(p));
    p.WqD = static_cast<const uint4*>(pd.W.p); p.WqT = static_cast<const uint4*>(pt.W.p);
    p.hp = static_cast<const uint4*>(tc->h_packed16.p);
    p.fhat = static_cast<const unsigned*>(tc->mix_fhat.p);
    p.w_t = c.w_title; p.w_p = c.w_playlist;
    p.n_valid_col = pl.n_valid_col;
    p.B = c.B; p.n_rg = pl.n_rg; p.Bpad = pl.Bpad;
    p.nsD = pl.NSD; p.nsT = pl.NST;
    p.list = order;
    if (sample) {
        p.biasD = static_cast<const uint4*>(pd.bias16_lo.p); p.biasT = static_cast<const uint4*>(pt.mix16_lo.p);
        p.n_items = pl.n_samp; p.nb_rg = pl.nb_s;
        p.samp = static_cast<float*>(tc->gmax.p); p.ld_s = pl.ld_s;
    } else {
        p.biasD = static_cast<const uint4*>(pd.bias16_hi.p); p.biasT = static_cast<const uint4*>(pt.mix16_hi.p);
        p.n_items = pl.ntr; p.nb_rg = pl.nb;
        p.tau = static_cast<const float*>(tc->tau.p);
        p.cand = static_cast<uint4*>(tc->cand.p); p.cand_cnt = static_cast<int*>(tc->cand_cnt.p); p.cap = pl.cap;
    }
    // one instance per shape class, row-group height and mode; its LDS limit is raised once
    void (*kern)(MixP);
    if (pl.shipped) kern = sample ? mix_bf16_kernel<16, 28, MX_RB, QR, NW, 1> : mix_bf16_kernel<16, 28, MX_RB, QR, NW, 0>;
    else if (pl.RB == MX_RB) kern = sample ? mix_bf16_steps_kernel<MX_RB, NW, 1> : mix_bf16_steps_kernel<MX_RB, NW, 0>;
    else kern = sample ? mix_bf16_steps_kernel<2, NW, 1> : mix_bf16_steps_kernel<2, NW, 0>;
    DAE_HIP_CHECK(tc, dae_lds_limit_once(tc, kern, pl.lds_attr));
    hipLaunchKernelGGL(kern, dim3(pl.n_rg * p.nb_rg), dim3(NW * 64), pl.lds_bytes, tc->stream, p);
    if (pl.shipped) DAE_CHECK_LAUNCH(tc, sample ? "mix_bf16_kernel<sample>" : "mix_bf16_kernel<filter>");
    else DAE_CHECK_LAUNCH(tc, sample ? "mix_bf16_steps_kernel<sample>" : "mix_bf16_steps_kernel<filter>");
    return DAE_OK;
}
