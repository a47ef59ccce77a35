// tau_select.hip -- the threshold launch of the fused scoring path: tau from the sample's group maxima, the sample's
// survivors, and (fp32, hidden 256) the live tile lists of the filter launch that takes the thresholds.
// Phase A leaves, per row, the dense logits of the sample tiles and the maxima of disjoint groups of sample columns
// (one column from each of the popularity bands a workgroup decodes; non-rankable columns masked to -inf).  The
// maxima are distinct elements of the row, at most n_seeds of them seeds, so the (k + n_seeds)-th largest of them is
// <= the row's k-th largest rankable non-seed logit: a valid threshold for phase B.
// One 256-thread workgroup per row.
//   1. the row's dense sample logits are requested first (up to 16 float4 per thread stay in registers: their
//      latency hides under the search);
//   2. tau: 4-ary search on the 16 leading bits of the order-preserving key for the largest prefix P with
//      count(maxima >= P << 16) >= k + n_seeds (tau_search.h: dae_tau_search, shared with the host test) -- 8 steps, each
//      3 x 16 compares per thread counted with s_bcnt1 on the compare mask and ONE barrier (histogram passes cost more: the
//      logits of a row share a few exponents, so 4 096 LDS atomics land on a handful of addresses -- 12 us; a shuffle
//      reduction per probe 13.7 us).  tau = the float of P << 16 (dae_tau_value): at most 2^-7 (relative) below the element
//      of that rank;
//   3. the sample logits >= tau go out as (logit, column) pairs, one flat list per row (slots from a block-wide
//      exclusive scan of the per-thread counts: no atomics) -- group 0 of the final selection (topk.hip PairSrc).  Phase B
//      never looks at the sample again.
#include <type_traits>

#include "decode_common.h"      // dae_tile_is_live: the live lists tau_select_kernel builds

namespace {

constexpr int TAU_PRE = 16;       // float4 of dense sample logits per thread requested before the search
struct TauP {
    const float* gmax; int64_t ld_g; int n_g;                    // group maxima [B][ld_g], n_g per row
    const float* samp; int64_t ld_s; int n_s;                    // dense sample logits [B][ld_s], n_s per row (% 32 == 0)
    const int* samp_list; int col_lo;                            // column of sample element q = col_lo + list[q >> 5] * 32 + (q & 31)
    const int32_t* seed_row_ptr; int k;
    float* tau; uint2* out_pairs; int64_t pairs_stride; int* out_cnt;
};

// keys >= q among the N register keys of every lane of the wave (wave-uniform).  All compare masks of a probe first, then
// their popcounts: a VALU compare -> SALU popcount pair stalls the (only) wave of the SIMD for the VALU -> SALU hand-over;
// interleaved pair by pair a step cost 2 000 cycles
template <int N>
__device__ __forceinline__ unsigned tau_count_ge(const unsigned (&kreg)[N], unsigned q)
{
    unsigned long long m[N];
    unsigned a = 0;
#pragma unroll
    for (int u = 0; u < N; ++u) m[u] = __ballot(kreg[u] >= q);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < N; ++u) a += (unsigned)__popcll(m[u]);
    return a;
}

// the sample's survivors (never -inf: masked columns and pads are not candidates)
__device__ __forceinline__ bool passes(float z, float tv) { return z >= tv && z > -__builtin_inff(); }
__device__ __forceinline__ unsigned count4(const float4 z, float tv)
{
    return (passes(z.x, tv) ? 1u : 0u) + (passes(z.y, tv) ? 1u : 0u) + (passes(z.z, tv) ? 1u : 0u) + (passes(z.w, tv) ? 1u : 0u);
}
// float4 f of the row's sample, from tile `tile` of the image: its survivors to dst[at ..)
__device__ __forceinline__ void emit4(const TauP& p, uint2* dst, unsigned& at, float tv, const float4 z, int f, int tile)
{
    const unsigned cb = (unsigned)(p.col_lo + tile * 32 + ((4 * f) & 31));
    if (passes(z.x, tv)) dst[at++] = make_uint2(__float_as_uint(z.x), cb);
    if (passes(z.y, tv)) dst[at++] = make_uint2(__float_as_uint(z.y), cb + 1u);
    if (passes(z.z, tv)) dst[at++] = make_uint2(__float_as_uint(z.z), cb + 2u);
    if (passes(z.w, tv)) dst[at++] = make_uint2(__float_as_uint(z.w), cb + 3u);
}

// 256 threads: the sum of v over the threads below this one; wsum[0 .. 4) holds the four waves' sums behind it.  One barrier
// inside; the caller puts one between two calls
__device__ __forceinline__ unsigned block_scan_excl(unsigned v, int lane, int wv, unsigned* wsum)
{
    const unsigned incl = dae_wave_scan_incl(v, lane);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    unsigned at = incl - v;
    for (int w = 0; w < wv; ++w) at += wsum[w];
    return at;
}

// LIVE: the launch also builds the live lists of the fp32 filter launch that takes its thresholds (dae_score_plan::live_in_tau;
// the test and its conventions: decode_common.h dae_tile_is_live, shared with prepack.hip live_tiles_kernel).
//   - the row's own 256 hidden values are requested from the packed image with the dense row's requests (64 float4 per wave,
//     the same in all four) and wave 0 takes d_row = max |h - 0.5| over the units k < H from them behind the search;
//   - behind step 3, one lane publishes {d_row, tau} and counts the row in at arrive[row / 128].  The hand-off between
//     workgroups: payload stored with agent-scope atomic (write-through) stores, drained (s_waitcnt vmcnt(0)) by the storing
//     lane, which then adds to the counter with an agent-scope atomic; the workgroup whose add returns rows_in_group - 1 knows
//     that every row of its group has published, runs ONE agent-scope acquire, and only then -- behind a barrier -- do its
//     waves load the group's payload (with agent-scope atomic loads: vector loads that bypass this CU's L1).  Nobody waits for
//     anybody: a workgroup that is not last ends;
//   - that last workgroup is the group's reducer: d_max and tau_min over the group's rows, the edge tile's bound, the test on
//     every item of the filter launch's list -- a contiguous run of LIVE_PER items per thread, all its list[] loads, then all
//     its bound loads, one block scan of the counts per 256 * LIVE_PER items -- and the kept tiles in the list's order.  It
//     leaves arrive[rg] at zero for the next launch on the stream.
using TauLive = dae_tau_live;      // (dae_internal.h: filled by score.hip topk_phase_a)
struct TauNoLive {};
// SPARSE: the sample launch skipped tiles and stored the decoded ones only (decode_generic.hip decode_f32_kernel's HALF); its
// decoded-tile table (score_plan.h dae_sample_item_slot) says which.  A slot it does not mark holds whatever an earlier call
// left there -- this kernel never reads it and takes the -inf the sample used to store: a maximum whose workgroup decoded
// nothing gets the key that is never counted, a dense float4 of a skipped item is four -inf that passes() never lets through.
struct TauTab { const unsigned* tab; int nb_rg; };               // [2 n_rg][nb_rg]; n_g == nb_rg * 32
struct TauNoTab {};
// where the byte of `item` sits in the kernel's LDS copy: items u * 32 + j (u < 16) of one j side by side
__device__ __forceinline__ int tau_ipos(int item) { return (item >> 9) * 512 + (item & 31) * 16 + ((item >> 5) & 15); }
constexpr int LIVE_PER = 16;       // items per thread and chunk of the reducer

// ---- 4. publish {d_row, tau}, arrive; the group's last workgroup builds its live list ----------------------------
__device__ __forceinline__ void tau_live_tail(const TauP& p, const TauLive& lv, int row, int tid, int lane, int wv, float tv, double d_row,
                                              unsigned* wsum)
{
    __shared__ int sh_last;
    __shared__ double sh_d[4];
    __shared__ float sh_t[4], sh_edge[2];
    const int rg = row >> 7, r0 = rg << 7;
    const int nrows = lv.B - r0 < 128 ? lv.B - r0 : 128;
    unsigned* const tau_bits = reinterpret_cast<unsigned*>(p.tau);
    if (tid == 0) {
        __hip_atomic_store(lv.d_row + row, (unsigned long long)__double_as_longlong(d_row), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(tau_bits + row, __float_as_uint(tv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // both stores have left before the counter moves
        const unsigned before = __hip_atomic_fetch_add(lv.arrive + rg, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = before == (unsigned)(nrows - 1) ? 1 : 0;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // ... and the invalidate has completed before the barrier lets the others load
        }
        sh_last = last;
    }
    __syncthreads();
    if (!sh_last) return;
    double d = 0.0;
    float tm = __builtin_inff();
    if (tid < nrows) {
        d = __longlong_as_double((long long)__hip_atomic_load(lv.d_row + r0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        tm = __uint_as_float(__hip_atomic_load(tau_bits + r0 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        d = dae_max_nan(d, __shfl_xor(d, sh));
        tm = dae_min_nan(tm, __shfl_xor(tm, sh));
    }
    if (lane == 0) { sh_d[wv] = d; sh_t[wv] = tm; }
    const int t_edge = (lv.nrank & 31) ? (lv.nrank >> 5) : -1;
    if (wv == 3 && t_edge >= 0) {                            // (rows sit in waves 0 and 1: this one has nothing in flight)
        float ea, em;
        dae_edge_tile_bound(lv.tile_ub, lv.ntiles, lv.nrank, lane, ea, em);
        if (lane == 0) { sh_edge[0] = ea; sh_edge[1] = em; }
    }
    __syncthreads();
    for (int w = 0; w < 4; ++w) { d = dae_max_nan(d, sh_d[w]); tm = dae_min_nan(tm, sh_t[w]); }
    const float2* const ub2 = reinterpret_cast<const float2*>(lv.tile_ub);
    int* const out = lv.live_list + (size_t)rg * lv.n_items;
    int done = 0;
    for (int c0 = 0; c0 < lv.n_items; c0 += 256 * LIVE_PER) {
        const int i0 = c0 + tid * LIVE_PER;
        int t[LIVE_PER];
        float2 ub[LIVE_PER];
#pragma unroll
        for (int u = 0; u < LIVE_PER; ++u) t[u] = lv.list[i0 + u < lv.n_items ? i0 + u : lv.n_items - 1];
#pragma unroll
        for (int u = 0; u < LIVE_PER; ++u) ub[u] = ub2[t[u]];
        unsigned keep = 0;
#pragma unroll
        for (int u = 0; u < LIVE_PER; ++u) {
            const bool edge = t[u] == t_edge;
            if (i0 + u < lv.n_items && dae_tile_is_live(edge ? sh_edge[0] : ub[u].x, edge ? sh_edge[1] : ub[u].y, d, tm)) keep |= 1u << u;
        }
        int slot = done + (int)block_scan_excl((unsigned)__popc(keep), lane, wv, wsum);
        done += (int)(wsum[0] + wsum[1] + wsum[2] + wsum[3]);
#pragma unroll
        for (int u = 0; u < LIVE_PER; ++u)
            if ((keep >> u) & 1u) out[slot++] = t[u];
        __syncthreads();                                     // (wsum is written again by the next chunk)
    }
    if (tid == 0) {
        lv.live_cnt[rg] = done;
        if (rg == 0) atomicAdd(&lv.stat[0], 1ull);
        atomicAdd(&lv.stat[1], (unsigned long long)lv.n_items);
        atomicAdd(&lv.stat[2], (unsigned long long)done);
        __hip_atomic_store(lv.arrive + rg, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch on the stream counts from zero
    }
}

// HAS_S = false: no dense sample to scan (n_s == 0: the bf16 / exact filter launch decodes every tile itself) -- tau only,
// a third of the registers, so that the workgroup fits on a CU NEXT to a filter workgroup of another batch.
template <int TAU_PER, bool HAS_S = true, bool LIVE = false, bool SPARSE = false>   // TAU_PER: maxima per thread held in registers (rows of <= 256 * TAU_PER maxima in one sweep)
__global__ __launch_bounds__(256) void tau_select_kernel(const TauP p, const std::conditional_t<LIVE, TauLive, TauNoLive> lv,
                                                         const std::conditional_t<SPARSE, TauTab, TauNoTab> tb)
{
    static_assert(!LIVE || HAS_S, "the live lists belong to a filter launch that does not decode the sample again");
    static_assert(!SPARSE || (HAS_S && TAU_PER <= 32), "the table: a dense sample, rows of nb_rg * 32 <= 256 * TAU_PER maxima, nb_rg <= 256 threads");
    // SPARSE: the table of the row's half group, spread out in LDS in the order the threads ask: one byte per workgroup w (it
    // stored its 32 maxima) at lgrp[(w & 7) * TAU_PER + (w >> 3)], one per item (< 4 nb_rg <= 32 TAU_PER) at litem[tau_ipos(item)]
    // -- a thread's TAU_PER groups and its 16 preloaded float4 are 16 contiguous bytes each: one LDS read, not one per register
    __shared__ __attribute__((aligned(16))) unsigned char lgrp[SPARSE ? 8 * TAU_PER : 16];
    __shared__ __attribute__((aligned(16))) unsigned char litem[SPARSE ? 32 * TAU_PER : 16];
    __shared__ unsigned wcnt[2][4][3];
    __shared__ unsigned wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = blockIdx.x;
    const float* g = p.gmax + (size_t)row * p.ld_g;
    const int n = p.n_g;
    const unsigned ns = p.seed_row_ptr ? (unsigned)(p.seed_row_ptr[row + 1] - p.seed_row_ptr[row]) : 0u;
    const unsigned need = (unsigned)p.k + ns;
    // ---- 1. requests: the group maxima ALONE first -- the search needs them and 256 rows asking for their 62 KB of
    // dense logits at the same moment put every row's maxima behind everybody's dense lines (maxima arrived after
    // 8.3 k cycles).  The dense row (TAU_PRE float4 per thread, kept in registers) is requested once the maxima are
    // here and stays in flight under the search.
    const bool one_sweep = n <= 256 * TAU_PER;
    float graw[TAU_PER];
#pragma unroll
    for (int u = 0; u < TAU_PER; ++u) {
        const int i = u * 256 + tid;
        graw[u] = (one_sweep && i < n) ? g[i] : -__builtin_inff();
    }
    // SPARSE: the table word of workgroup `tid` of the row's half group, asked for with the maxima (no trip of its own)
    unsigned tword = 0;
    if constexpr (SPARSE)
        if (tid < tb.nb_rg) tword = tb.tab[(size_t)(row >> 6) * tb.nb_rg + tid];
    // LIVE && SPARSE, THE EMPTY LIST PROVED (empty_proof.h): the {dq, tau_safe} pairs the sample launch stored
    // for the row group's half groups, asked for by every thread with the maxima (a wave-uniform address).  D = max dq >= the d the
    // tail would compute, T = min tau_safe <= every threshold of the group: every workgroup of the group takes the same four floats
    // and reaches the same verdict, so nobody has to arrive anywhere.  A second half group without a real row takes no part.
    constexpr bool PROOF = LIVE && SPARSE;
    float2 pr0 = make_float2(0.0f, 0.0f), pr1 = pr0;
    bool proof_on = false;
    if constexpr (PROOF) {
        proof_on = lv.pair != nullptr;
        if (proof_on) {
            const int hg = (row >> 7) * 2;
            pr0 = lv.pair[hg];
            pr1 = lv.pair[(hg + 1) * 64 < lv.B ? hg + 1 : hg];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    unsigned kreg[TAU_PER];
#pragma unroll
    for (int u = 0; u < TAU_PER; ++u) kreg[u] = dae_okey(graw[u]);     // -inf -> NEG_INF key: never counted
    if constexpr (SPARSE) {
        if (tid < tb.nb_rg) {
            lgrp[(tid & 7) * TAU_PER + (tid >> 3)] = tword != 0u ? 1 : 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) litem[tau_ipos(dae_sample_slot_item(tid, b, tb.nb_rg))] = (unsigned char)((tword >> (8 * b)) & 0xFFu);
        }
        __syncthreads();
        // masked at the KEY: an unmarked slot may hold anything, a NaN included.  Maximum u * 256 + tid belongs to workgroup
        // u * 8 + (tid >> 5); bytes of workgroups >= nb_rg were never written and meet keys that are absent already
#pragma unroll
        for (int q = 0; q < TAU_PER / 16; ++q) {
            const uint4 gb = reinterpret_cast<const uint4*>(lgrp)[(tid >> 5) * (TAU_PER / 16) + q];
            const unsigned gw[4] = {gb.x, gb.y, gb.z, gb.w};
#pragma unroll
            for (int u = 0; u < 16; ++u)
                kreg[q * 16 + u] = ((gw[u >> 2] >> (8 * (u & 3))) & 0xFFu) ? kreg[q * 16 + u] : DAE_KEY_NEG_INF;
        }
    }
    // PROOF: the one envelope entry for D (the pairs arrived with the table word above), asked for here -- ahead of the
    // dense row's requests, so that no wait for it stands in front of the search -- and consumed behind the search
    float genv = __builtin_nanf("");
    float proof_T = -__builtin_inff();
    if constexpr (PROOF) {
        if (proof_on) {
            const float D = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(dae_max_nan(pr0.x, pr1.x))));
            proof_T = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(dae_min_nan(pr0.y, pr1.y))));
            const int jd = dae_proof_index(D);
            if (jd >= 0) genv = lv.env[jd];                      // (no proof for this D: the NaN stands)
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    const float4* srow = reinterpret_cast<const float4*>(p.samp + (size_t)row * p.ld_s);
    const int n4 = HAS_S ? p.n_s >> 2 : 0;
    constexpr int NPRE = HAS_S ? TAU_PRE : 1;
    float4 zpre[NPRE];
    // tiles of the preloaded part (one id per 8 float4) -> LDS: consumed only where something passes
    __shared__ int ltile[HAS_S ? TAU_PRE * 256 / 8 : 1];
    if (HAS_S) {
        // SPARSE: float4 u * 256 + tid belongs to item u * 32 + (tid >> 3) = dae_sample_f4_item(f): the thread's 16 bytes
        static_assert(TAU_PRE == 16, "tau_ipos lays 16 items side by side");
        uint4 ib = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (SPARSE) ib = reinterpret_cast<const uint4*>(litem)[tid >> 3];
        const unsigned iw[4] = {ib.x, ib.y, ib.z, ib.w};
#pragma unroll
        for (int u = 0; u < NPRE; ++u) {
            const int f = u * 256 + tid;
            if constexpr (SPARSE) {                              // a skipped item's float4: no request, four -inf
                zpre[u] = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff());
                if (f < n4 && ((iw[u >> 2] >> (8 * (u & 3))) & 0xFFu)) zpre[u] = srow[f];
            } else {
                zpre[u] = srow[f < n4 ? f : 0];
            }
        }
        for (int i = tid; i < TAU_PRE * 256 / 8; i += 256) ltile[i] = p.samp_list[i < (n4 + 7) / 8 ? i : 0];
    }
    // LIVE: the row's hidden values.  float4 index (g * 4 + rb) * 64 + l of row group rg holds h[rg * 128 + rb * 32 + (l & 31)]
    // [8 g + 2 e + (l >> 5)], e = component (prepack.hip pack_h / the encode kernel): lane j takes g = j >> 1, l >> 5 = j & 1
    // (the 64-key shape has no four registers to spare across the search -- they would cost it a wave per SIMD: it asks behind
    // the search and the latency hides under step 3)
    constexpr bool HV_EARLY = TAU_PER < 64;
    float4 hv = make_float4(0.5f, 0.5f, 0.5f, 0.5f);
    auto load_hv = [&]() {
        // (every wave asks for the same 64 float4, wave 0 uses them: a branch around the request ends in a wait for it -- and
        // for the dense row in front of it -- before the search, which is the latency the early request is there to hide)
        if constexpr (LIVE)
            hv = lv.hp[((size_t)(row >> 7) * lv.G * 4 + (size_t)((lane >> 1) * 4 + ((row >> 5) & 3))) * 64 + (lane & 1) * 32 + (row & 31)];
    };
    if constexpr (LIVE && HV_EARLY) load_hv();
    __builtin_amdgcn_sched_barrier(0);                           // keep every request above ahead of the search
    // ---- 2. tau -------------------------------------------------------------------------------------------------
    // counts of keys >= each of 3 probes over the row (block-uniform results); absent / -inf keys never count
    const unsigned lo = dae_tau_search(need, [&](unsigned q0, unsigned q1, unsigned q2, int it, unsigned (&c)[3]) {
        unsigned a0 = 0, a1 = 0, a2 = 0;
        if (one_sweep) {
            a0 = tau_count_ge(kreg, q0);
            a1 = tau_count_ge(kreg, q1);
            a2 = tau_count_ge(kreg, q2);
        } else {
            for (int i0 = 0; i0 < n; i0 += 256) {
                const unsigned key = i0 + tid < n ? dae_okey(g[i0 + tid]) : 0u;
                a0 += (unsigned)__popcll(__ballot(key >= q0));
                a1 += (unsigned)__popcll(__ballot(key >= q1));
                a2 += (unsigned)__popcll(__ballot(key >= q2));
            }
        }
        if (lane == 0) { wcnt[it & 1][wv][0] = a0; wcnt[it & 1][wv][1] = a1; wcnt[it & 1][wv][2] = a2; }
        __syncthreads();                                         // slots alternate: one barrier per step is enough
#pragma unroll
        for (int e = 0; e < 3; ++e)
            c[e] = wcnt[it & 1][0][e] + wcnt[it & 1][1][e] + wcnt[it & 1][2][e] + wcnt[it & 1][3][e];
    });
    const float tv = dae_tau_value(lo, p.n_s);
    if (!LIVE && tid == 0) p.tau[row] = tv;                      // (LIVE: published at the end, with d_row)
    bool proved = false;                                         // block-uniform
    if constexpr (PROOF) proved = __builtin_amdgcn_readfirstlane((int)(proof_on && dae_proof_holds(genv, proof_T))) != 0;
    double d_row = 0.0;                                          // LIVE, wave 0: max |h - 0.5| over the row's units k < H (the zero pad would read 0.5)
    auto take_d_row = [&]() {
        if constexpr (LIVE) {
            if (wv == 0) {
                // (an opaque use HERE: without it the compiler converts the four values to double right behind their request,
                // i.e. waits for them before the search)
                asm volatile("" : "+v"(hv.x), "+v"(hv.y), "+v"(hv.z), "+v"(hv.w));
                const float e[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (8 * (lane >> 1) + 2 * c + (lane & 1) < lv.H) d_row = dae_max_nan(d_row, fabs((double)e[c] - 0.5));
#pragma unroll
                for (int sh = 1; sh < 64; sh <<= 1) d_row = dae_max_nan(d_row, __shfl_xor(d_row, sh));
            }
        }
    };
    if constexpr (LIVE && HV_EARLY) {
        if (!proved) take_d_row();                               // (a proved group has no tail to give it to)
    }
    if constexpr (LIVE && !HV_EARLY) load_hv();
    if (!HAS_S) {                                                // no sample to scan: the (empty) survivor list
        if (tid == 0) p.out_cnt[row] = 0;
        return;
    }
    // ---- 3. the sample's survivors -----------------------------------------------------------------------------------
    unsigned mine = 0;
    unsigned live = 0;                                           // bit u: some lane of this wave has a survivor in zpre[u]
#pragma unroll
    for (int u = 0; u < NPRE; ++u) {
        const float mx = fmaxf(fmaxf(zpre[u].x, zpre[u].y), fmaxf(zpre[u].z, zpre[u].w));
        if (__ballot(u * 256 + tid < n4 && passes(mx, tv))) {    // wave-uniform: most groups hold nothing above tau
            live |= 1u << u;
            if (u * 256 + tid < n4) mine += count4(zpre[u], tv);
        }
    }
    // rows longer than the preloaded part: read again (SPARSE: the decoded items only)
    auto decoded = [&](int f) -> bool {
        if constexpr (SPARSE) return litem[tau_ipos(dae_sample_f4_item(f))] != 0;
        else return true;
    };
    for (int f = TAU_PRE * 256 + tid; f < n4; f += 256)
        if (decoded(f)) mine += count4(srow[f], tv);
    __syncthreads();
    unsigned at = block_scan_excl(mine, lane, wv, wsum);
    if (tid == 255) p.out_cnt[row] = (int)(at + mine);
    uint2* dst = p.out_pairs + (size_t)row * p.pairs_stride;
#pragma unroll
    for (int u = 0; u < NPRE; ++u)
        if (((live >> u) & 1u) && u * 256 + tid < n4) emit4(p, dst, at, tv, zpre[u], u * 256 + tid, ltile[(u * 256 + tid) >> 3]);
    for (int f = TAU_PRE * 256 + tid; f < n4; f += 256)
        if (decoded(f)) emit4(p, dst, at, tv, srow[f], f, p.samp_list[f >> 3]);
    if constexpr (LIVE) {
        if constexpr (!HV_EARLY) take_d_row();
        if constexpr (PROOF) {
            if (proved) {
                // the answer the arrival tail would have given, from the workgroup of the group's first row: an empty list and the
                // reducer's counters (+ the groups proved).  The arrival counter and lv.d_row are not touched
                if (tid == 0) {
                    p.tau[row] = tv;
                    if ((row & 127) == 0) {
                        const int rg = row >> 7;
                        lv.live_cnt[rg] = 0;
                        if (rg == 0) atomicAdd(&lv.stat[0], 1ull);
                        atomicAdd(&lv.stat[1], (unsigned long long)lv.n_items);
                        atomicAdd(&lv.stat[2], 0ull);
                        atomicAdd(&lv.stat[3], 1ull);
                    }
                }
                return;
            }
        }
        tau_live_tail(p, lv, row, tid, lane, wv, tv, d_row, wsum);
    }
}

// The same for launches of MANY SHORT rows (vocabulary shards, where every rank scores the whole global batch over its
// slice of the columns: 2048 rows x 1952 sample logits at 8 ranks): one WAVE per row, four rows per workgroup.  The
// maxima (<= 64 * KPL) and the dense sample (<= 64 * PRE float4) of a row sit in the registers of its wave; a search
// step is 3 x KPL compare masks and their s_bcnt1 -- the counts are wave-uniform scalars, so there is no LDS, no
// barrier and no other wave to wait for; the survivors' slots come from one wave scan.  Same tau, same survivor set
// (list order differs: the final selection does not depend on it).
template <int KPL, int PRE>
__global__ __launch_bounds__(256) void tau_select_wave_kernel(const TauP p, const int B)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= B) return;                                        // wave-uniform
    const float* g = p.gmax + (size_t)row * p.ld_g;
    const int n = p.n_g;
    const unsigned ns = p.seed_row_ptr ? (unsigned)(p.seed_row_ptr[row + 1] - p.seed_row_ptr[row]) : 0u;
    const unsigned need = (unsigned)p.k + ns;
    float graw[KPL];
#pragma unroll
    for (int u = 0; u < KPL; ++u) {
        const int i = u * 64 + lane;
        graw[u] = i < n ? g[i] : -__builtin_inff();
    }
    const float4* srow = reinterpret_cast<const float4*>(p.samp + (size_t)row * p.ld_s);
    const int n4 = p.n_s >> 2;
    float4 zpre[PRE];
    int tl[PRE];
#pragma unroll
    for (int u = 0; u < PRE; ++u) {
        const int f = u * 64 + lane;
        zpre[u] = srow[f < n4 ? f : 0];
        tl[u] = p.samp_list[(f < n4 ? f : 0) >> 3];
    }
    __builtin_amdgcn_sched_barrier(0);
    unsigned kreg[KPL];
#pragma unroll
    for (int u = 0; u < KPL; ++u) kreg[u] = dae_okey(graw[u]);
    const unsigned lo = dae_tau_search(need, [&](unsigned q0, unsigned q1, unsigned q2, int, unsigned (&c)[3]) {
        c[0] = tau_count_ge(kreg, q0);
        c[1] = tau_count_ge(kreg, q1);
        c[2] = tau_count_ge(kreg, q2);
    });
    const float tv = dae_tau_value(lo, p.n_s);
    if (lane == 0) p.tau[row] = tv;
    unsigned mine = 0;
#pragma unroll
    for (int u = 0; u < PRE; ++u)
        if (u * 64 + lane < n4) mine += count4(zpre[u], tv);
    const unsigned incl = dae_wave_scan_incl(mine, lane);
    unsigned at = incl - mine;
    if (lane == 63) p.out_cnt[row] = (int)incl;
    uint2* dst = p.out_pairs + (size_t)row * p.pairs_stride;
#pragma unroll
    for (int u = 0; u < PRE; ++u)
        if (u * 64 + lane < n4) emit4(p, dst, at, tv, zpre[u], u * 64 + lane, tl[u]);
}

// per = TAU_PER: 16 for rows of <= 4 096 maxima; 32 up to 8 192 (batch 1024 on one GPU: 5 120 maxima per row -- half the
// compares of the 64-key shape); 64 beyond, which has no sample-free instance (it sees n_s == 0 at run time).
// Deep k (<= DAE_MAX_K_DEEP) changes no shape: the plan keeps every sample element as a maximum while a row has fewer than 4 k
// of them, so a row can hold more than 256 * 64 slots (e.g. 4 x 8 192, most of them -inf): the 64-key shape then reads the
// maxima from memory in every search step (one_sweep = false).  A row with fewer than k + n_seeds finite maxima leaves the
// search at DAE_TAU_P_MIN - 1, i.e. tau = -inf (tau_search.h), in this kernel and in the wave-per-row one, which only takes rows
// of <= 64 * 32 maxima whatever k is (dae_tau_wave_per_row).
template <bool HAS_S, bool LIVE, typename Lv>
void launch_tau_per(dae_ctx* ctx, const TauP& p, int B, int per, const Lv& lv)
{
    if (per == 16) hipLaunchKernelGGL((tau_select_kernel<16, HAS_S, LIVE>), dim3(B), dim3(256), 0, ctx->stream, p, lv, TauNoTab{});
    else if (per == 32) hipLaunchKernelGGL((tau_select_kernel<32, HAS_S, LIVE>), dim3(B), dim3(256), 0, ctx->stream, p, lv, TauNoTab{});
    else hipLaunchKernelGGL((tau_select_kernel<64, true, LIVE>), dim3(B), dim3(256), 0, ctx->stream, p, lv, TauNoTab{});
}
// ... with the sample's decoded-tile table (a half-row-group sample: nb_rg <= 256 workgroups, i.e. <= 8 192 maxima per row)
template <bool LIVE, typename Lv>
void launch_tau_sparse(dae_ctx* ctx, const TauP& p, int B, int per, const Lv& lv, const TauTab& tb)
{
    if (per == 16) hipLaunchKernelGGL((tau_select_kernel<16, true, LIVE, true>), dim3(B), dim3(256), 0, ctx->stream, p, lv, tb);
    else hipLaunchKernelGGL((tau_select_kernel<32, true, LIVE, true>), dim3(B), dim3(256), 0, ctx->stream, p, lv, tb);
}

int launch_tau_select(dae_ctx* ctx, const TauP& p, int B, const TauLive* lv, const unsigned* samp_tab, int nb_rg)
{
    if (B <= 0) return DAE_OK;
    // many short rows (>= 4 per CU, <= 2048 maxima and sample logits each: the 8-rank shard of the global batch): a wave
    // per row, everything in registers, no barriers -- 30.1 -> 22.3 us for 2048 rows.  Longer rows lose (4096 maxima per
    // wave = 64 key registers and 128 mask SGPRs per probe: 37 vs 18.6 us at 4 ranks) and keep the workgroup kernel.
    // (score_plan.h dae_tau_wave_per_row: the plan asks the same question before it gives this launch the live lists to build)
    if (dae_tau_wave_per_row(B, p.n_g, p.n_s)) {
        if (lv) return dae_fail(ctx, DAE_ERR_STATE, "the wave-per-row threshold kernel builds no live lists");
        if (samp_tab) return dae_fail(ctx, DAE_ERR_STATE, "the wave-per-row threshold kernel reads the whole sample: no decoded-tile table");
        hipLaunchKernelGGL((tau_select_wave_kernel<32, 8>), dim3((B + 3) / 4), dim3(256), 0, ctx->stream, p, B);
        DAE_CHECK_LAUNCH(ctx, "tau_select_wave_kernel");
        return DAE_OK;
    }
    if (lv && (p.n_s == 0 || lv->G != 32 || lv->n_items <= 0))
        return dae_fail(ctx, DAE_ERR_STATE, "live lists from the threshold launch: fp32 image of hidden 256 with a dense sample only");
    const int per = p.n_g <= 256 * 16 ? 16 : p.n_g <= 256 * 32 ? 32 : 64;
    if (samp_tab) {
        if (p.n_s == 0 || nb_rg <= 0 || nb_rg > 256 || p.n_g != nb_rg * 32 || p.n_s > 4 * nb_rg * 32)
            return dae_fail(ctx, DAE_ERR_STATE, "decoded-tile table: a dense one-round sample of nb_rg <= 256 workgroups per half row group only");
        const TauTab tb{samp_tab, nb_rg};
        if (lv) launch_tau_sparse<true>(ctx, p, B, per, *lv, tb);
        else launch_tau_sparse<false>(ctx, p, B, per, TauNoLive{}, tb);
    }
    else if (lv) launch_tau_per<true, true>(ctx, p, B, per, *lv);
    else if (p.n_s == 0) launch_tau_per<false, false>(ctx, p, B, per, TauNoLive{});
    else launch_tau_per<true, false>(ctx, p, B, per, TauNoLive{});
    DAE_CHECK_LAUNCH(ctx, "tau_select_kernel");
    return DAE_OK;
}

}  // namespace

int dae_launch_tau_select(dae_ctx* ctx, const float* gmax, int64_t ld_g, int n_g, const float* samp, int64_t ld_s,
                          int n_s, const int* samp_list, int col_lo, int B, int k, const int32_t* seed_row_ptr,
                          float* tau, uint2* out_pairs, int64_t pairs_stride, int* out_cnt, const dae_tau_live* live,
                          const unsigned* samp_tab, int nb_rg)
{
    if ((n_s & 31) || (ld_s & 3) || (reinterpret_cast<uintptr_t>(samp) & 15))
        return dae_fail(ctx, DAE_ERR_ARG, "sample rows must be whole tiles, 16-byte aligned");
    TauP p{gmax, ld_g, n_g, samp, ld_s, n_s, samp_list, col_lo, seed_row_ptr, k, tau, out_pairs, pairs_stride, out_cnt};
    return launch_tau_select(ctx, p, B, live, samp_tab, nb_rg);
}
