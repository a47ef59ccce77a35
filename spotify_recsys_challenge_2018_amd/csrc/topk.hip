// topk.hip -- K3/K4: exact top-k ranking of one playlist row per workgroup.
// Reference: main_challenge.py:26-36 (cand_generate) == metrics.py:59-68 (single_eval ranking):
//     cand = argsort(-scores); for s in seed: cand.remove(s); cand = cand[:500]
// numpy's argsort leaves tie order unspecified, so the canonical rule is
//     (fp32 logit descending, column index ascending)
// i.e. descending order of the UNIQUE 64-bit composite key  (okey(logit) << 32) | ~column.
//
// Algorithm per row (one 1024-thread workgroup, everything after the first read stays in LDS):
//   1. seed tracks -> per-row LDS bitmap over the ranked column range (the reference's O(n)
//      list.remove per seed becomes one LDS bit test per element);
//   2. every valid element's composite key is appended to an LDS key buffer (wave-aggregated
//      append), with the running min / max key;
//   3. range-adaptive MSB radix narrowing: histogram (key - lo) >> shift over 2048 bins with shift
//      chosen from the live range [lo, hi], parallel suffix scan to find the bin holding the
//      k-th key, shrink [lo, hi] to that bin; stop as soon as the keys >= lo fit the sort buffer
//      (keys are unique, so no tie handling exists anywhere);
//   4. collect those keys; k <= 512: order them by HISTOGRAM RANK (position = keys in higher bins + keys of the
//      own bin above; one LDS atomic per key, a suffix scan, a count inside the bin); k > 512: hybrid bitonic sort
//      (wave shuffles + LDS stages); emit k.  k > 1024 (<= 4096): the same with a sort buffer of 4096 or 8192 keys, 4 or 8 per
//      thread (the TK_SORT_DEEP instantiation below).
// Rows whose elements do not fit the LDS key buffer (dae_topk_dense over a whole vocabulary row)
// run the same steps with step 3 re-reading the source instead of LDS.
//
// Element sources:
//   dense : a row of logits (dae_topk_dense; small problems of the fused path)
//   pairs : segments of (logit, column) pairs (the sample's survivors from tau_select_kernel + phase-B candidate lists)
//   soa   : [G, B, k] shard lists gathered by RCCL (K4 merge)
#include "rank_lds.h"           // the stages themselves: bin search, narrowing, wave append, histogram-rank ordering

namespace {

constexpr int TK_BINS = DAE_RANK_BINS;
constexpr int TK_MAX_SEG = 1024;
constexpr int TK_SORT_MAX = 2048;
static_assert(TK_SORT_MAX == 2 * DAE_RANK_MAX, "k <= 512 collects what dae_rank_order takes; k > 512 sorts twice as many");
// deep rows (DAE_MAX_K < k <= DAE_MAX_K_DEEP) run an instantiation of their own with a sort buffer of TK_SORT_DEEP keys; the
// instantiations for k <= DAE_MAX_K keep TK_SORT_MAX, and with it their code, registers and LDS (profiles/deep_k_notes.md)
constexpr int TK_SORT_DEEP = 8192;
constexpr size_t TK_LDS_TOTAL = 160 * 1024, TK_LDS_STATIC = 14 * 1024;   // the CU's LDS; hist 8K + seg_prefix 4K + scalars
static_assert(TK_SORT_DEEP >= 2 * DAE_MAX_K_DEEP, "the deep sort buffer holds twice the largest k, as TK_SORT_MAX does for DAE_MAX_K");
static_assert(TK_SORT_DEEP % 1024 == 0 && (TK_SORT_DEEP & (TK_SORT_DEEP - 1)) == 0, "a bitonic network over whole slots of 1024 threads");
// the deep LDS budget: 64 KiB sort buffer + the seed bitmap of the shipped vocabulary (170 000 columns: ~21 KiB) + the static
// part + at least the 8 KiB second buffer / key cache
static_assert((size_t)TK_SORT_DEEP * 8 == 64 * 1024, "deep sort buffer: 64 KiB");
static_assert((size_t)TK_SORT_DEEP * 8 + ((170000 + 31) / 32 * 4 + 15) / 16 * 16 + TK_LDS_STATIC + 8 * 1024 <= TK_LDS_TOTAL,
              "deep sort buffer + seed bitmap over 170 000 columns + static LDS + the smallest key cache fit one CU");
typedef dae_u64 u64;

struct DenseSrc {
    static constexpr int kSegs = 0;
    static constexpr bool kFixedSlots = true;      // for_each visits q = tid, tid + 1024, ... in order
    dae_dense_src s;
    int max_keys() const { return s.n; }                  // host: most keys a row can hold
    template <int NTH> __device__ __forceinline__ void prepare(int, int, int*) const {}
    __device__ __forceinline__ int count(int, const int*) const { return s.n; }
    template <int NTH, typename F>
    __device__ __forceinline__ void for_each(int row, int tid, const int*, F f) const
    {
        const float* rp = s.logits + (size_t)row * s.ld;
        const int step = 32 * s.tile_stride;
        int base = 0;                                  // block-uniform loop bounds
        for (; base + 4 * NTH <= s.n; base += 4 * NTH) {
            float z[4];
            int tb[4];                                 // tile bases: loaded with the logits, not after
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = base + u * NTH + tid;
                z[u] = rp[q];
                tb[u] = s.tile_list ? s.tile_list[q >> 5] * 32 : (q >> 5) * step;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = base + u * NTH + tid;
                f(z[u], s.col_base + tb[u] + (q & 31), true);
            }
        }
        for (; base < s.n; base += NTH) {
            const int q = base + tid;
            const bool in = q < s.n;
            const float z = in ? rp[q] : 0.f;
            const int tb = s.tile_list ? s.tile_list[in ? (q >> 5) : 0] * 32 : (q >> 5) * step;
            f(z, s.col_base + tb + (q & 31), in);
        }
    }
};

struct PairSrc {
    static constexpr int kSegs = TK_MAX_SEG;
    static constexpr bool kFixedSlots = false;
    dae_pair_group g0, g1;
    int max_keys() const { return 2048; }                 // typical rows are far below; larger rows re-read
    __device__ __forceinline__ int seg_count(const dae_pair_group& g, int seg, int row) const
    {
        return g.cnt ? g.cnt[(size_t)seg * g.cnt_seg_stride + row] : g.fixed_cnt;
    }
    // exclusive prefix of segment sizes in LDS: seg_prefix[0..nseg]
    template <int NTH>
    __device__ __forceinline__ void prepare(int row, int tid, int* seg_prefix) const
    {
        const int nseg = g0.nseg + g1.nseg;
        for (int s = tid; s < nseg; s += NTH)
            seg_prefix[s + 1] = s < g0.nseg ? seg_count(g0, s, row) : seg_count(g1, s - g0.nseg, row);
        if (tid == 0) seg_prefix[0] = 0;
        __syncthreads();
        if (tid < 64) {           // one wave scans (nseg <= 1024: 16 chunks of 64)
            int carry = 0;
            for (int base = 0; base < nseg; base += 64) {
                const int i = base + tid;
                const int v = dae_wave_scan_incl(i < nseg ? seg_prefix[i + 1] : 0, tid);
                if (i < nseg) seg_prefix[i + 1] = v + carry;
                carry += __shfl(v, 63);
            }
        }
        __syncthreads();
    }
    __device__ __forceinline__ int count(int, const int* seg_prefix) const
    {
        return seg_prefix[g0.nseg + g1.nseg];
    }
    template <int NTH, typename F>
    __device__ __forceinline__ void for_each(int row, int tid, const int* seg_prefix, F f) const
    {
        constexpr int TK_WAVES = NTH / 64;
        // group 0 (few, long segments: the sample winners): flat over the whole workgroup
        for (int sg = 0; sg < g0.nseg; ++sg) {
            const int cnt = seg_prefix[sg + 1] - seg_prefix[sg];
            const uint2* base = g0.base + (size_t)sg * g0.seg_stride + (size_t)row * g0.row_stride;
            for (int i0 = 0; i0 < cnt; i0 += NTH) {
                const int i = i0 + tid;
                const bool in = i < cnt;
                const uint2 pr = in ? base[i] : make_uint2(0u, 0xFFFFFFFFu);
                f(__uint_as_float(pr.x), (int)pr.y, in);
            }
        }
        // group 1 (many short segments: one candidate list per decode workgroup): a wave per
        // segment, 4 segments in flight, no per-element search
        const int lane = tid & 63, wave = tid >> 6;
        for (int s0 = wave; s0 < g1.nseg; s0 += 4 * TK_WAVES) {
            int cnt[4];
            const uint2* base[4];
            int mx = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int sg = s0 + u * TK_WAVES;
                const bool ok = sg < g1.nseg;
                cnt[u] = ok ? seg_prefix[g0.nseg + sg + 1] - seg_prefix[g0.nseg + sg] : 0;
                base[u] = g1.base + (size_t)(ok ? sg : 0) * g1.seg_stride + (size_t)row * g1.row_stride;
                mx = cnt[u] > mx ? cnt[u] : mx;
            }
            for (int i0 = 0; i0 < mx; i0 += 64) {
                uint2 pr[4];
                bool in[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    in[u] = i0 + lane < cnt[u];
                    pr[u] = in[u] ? base[u][i0 + lane] : make_uint2(0u, 0xFFFFFFFFu);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 < cnt[u]) f(__uint_as_float(pr[u].x), (int)pr[u].y, in[u]);
            }
        }
    }
};

struct SoaSrc {
    static constexpr int kSegs = 0;
    static constexpr bool kFixedSlots = false;
    const float* logit; const int32_t* idx; int G, B, k;
    int max_keys() const { return G * k; }
    template <int NTH> __device__ __forceinline__ void prepare(int, int, int*) const {}
    __device__ __forceinline__ int count(int, const int*) const { return G * k; }
    template <int NTH, typename F>
    __device__ __forceinline__ void for_each(int row, int tid, const int*, F f) const
    {
        const int total = G * k;
        for (int e0 = 0; e0 < total; e0 += NTH) {
            const int e = e0 + tid;
            const bool in = e < total;
            float z = 0.f; int colv = -1;
            if (in) {
                const int g = e / k, i = e - g * k;
                const size_t o = ((size_t)g * B + row) * k + i;
                colv = idx[o]; z = logit[o];
            }
            f(z, colv, in);
        }
    }
};

// NTH threads per row: 1024 for long rows (a phase-A sample, a dense row), 256 for short ones (candidate
// lists, small shards, gathered shard lists) -- a short row is bound by the fixed cost of every stage
// (histogram clears, bin scans, barriers joining 16 waves), which a quarter of the threads cuts to a
// quarter, and up to 8 such workgroups share a CU.  Same stages, same results.
// CAP: the sort buffer's capacity in keys -- TK_SORT_MAX for k <= DAE_MAX_K; TK_SORT_DEEP (1024 threads only) for deeper lists:
// the same stages with a.sort_cap (4096 or 8192) keys collected and sorted, and CAP thread maxima behind the 3a cut.
template <typename Src, int NTH, int CAP = TK_SORT_MAX>
__global__ __launch_bounds__(NTH) void topk_kernel(const Src src, const dae_topk_args a,
                                                   const int key_cap)
{
    static_assert(CAP == TK_SORT_MAX || (CAP == TK_SORT_DEEP && NTH == 1024), "deep rows always take the 1024-thread shape");
    constexpr int TK_WAVES = NTH / 64;
    // per-thread maxima kept for the 3a cut: 1024 in all; deep: CAP in all (the k-th largest of fewer than 2 k maxima cuts nothing)
    constexpr int MAXES = CAP == TK_SORT_MAX ? 1024 / NTH : CAP / NTH;
    constexpr int EMAX = CAP / NTH;                              // sort-buffer keys per thread, at most
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ unsigned hist[TK_BINS];
    __shared__ int seg_prefix[Src::kSegs + 2];
    __shared__ unsigned wave_tot[TK_WAVES];
    __shared__ int s_bin;
    __shared__ unsigned s_above;
    __shared__ unsigned s_cnt, s_cnt2, s_slots;
    __shared__ u64 s_min, s_max, s_min2;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int row = blockIdx.x;
    const int k = a.k;
    // dynamic LDS: [seed bitmap (bitmap mode only)] [skey: sort buffer, sort_cap keys] [key cache]
    const bool lean = a.lean != 0;
    const int bm_words = lean ? 0 : (a.bitmap_n + 31) >> 5;
    unsigned* bitmap = reinterpret_cast<unsigned*>(dyn);
    u64* skey = reinterpret_cast<u64*>(dyn + (((size_t)bm_words * 4 + 15) & ~(size_t)15));
    u64* keys = skey + a.sort_cap;

    // ---- 1. seeds -----------------------------------------------------------------------------------
    // bitmap mode: per-row LDS bitmap over the ranked columns, tested for every element.
    // lean mode (small LDS footprint, so that this kernel can share a CU with the decode workgroups
    // of another batch): no bitmap.  With ns seeds in the row, the (k + ns)-th largest key over ALL
    // elements is a valid cut for the k-th largest non-seed key, so the narrowing stages run seed-blind
    // with rank k + ns, and the seeds are removed once, from the <= sort_n keys that were collected.
    // Rows with k + ns above the sort buffer test every element against the seed list instead.
    const int seed_b = a.seed_col ? a.seed_row_ptr[row] : 0;
    const int seed_e = a.seed_col ? a.seed_row_ptr[row + 1] : 0;
    const int ns = seed_e - seed_b;
    for (int w = tid; w < bm_words; w += NTH) bitmap[w] = 0;
    if (tid == 0) { s_cnt = 0; s_min = ~0ull; s_max = 0ull; s_slots = 0; }
    __syncthreads();
    if (!lean && a.seed_col && bm_words > 0) {
        for (int i = seed_b + tid; i < seed_e; i += NTH) {
            const int pcol = a.seed_col[i] - a.bitmap_base;
            if (pcol >= 0 && pcol < a.bitmap_n) atomicOr(&bitmap[pcol >> 5], 1u << (pcol & 31));
        }
    }
    src.template prepare<NTH>(row, tid, seg_prefix);
    __syncthreads();

    int sort_n = 1;
    while (sort_n < k) sort_n <<= 1;
    if (sort_n < 1024) sort_n = 1024;                            // always <= TK_SORT_MAX (k <= 1024)
    if (k > 512) sort_n = TK_SORT_MAX;
    if (CAP > TK_SORT_MAX) sort_n = a.sort_cap;                  // deep: 4096 (k <= 2048) or 8192, chosen by launch_topk
    const bool seed_blind = lean && ns > 0 && k + ns <= sort_n;  // remove the seeds after the collect
    const bool seed_scan = lean && ns > 0 && !seed_blind;         // (rare) test every element
    auto is_seed = [&](int colv) -> bool {
        bool hit = false;
        for (int i = seed_b; i < seed_e; ++i) hit = hit || (a.seed_col[i] == colv);   // uniform address
        return hit;
    };

    // composite key of one element; 0 = absent (masked seed, -inf padding, missing entry)
    const float row_min = a.row_min ? a.row_min[row] : -__builtin_inff();
    auto ckey = [&](float z, int colv, bool in) -> u64 {
        if (!in || colv < 0 || z < row_min) return 0ull;
        const unsigned key = dae_okey(z);
        if (key <= DAE_KEY_NEG_INF) return 0ull;
        if (!lean) {
            const int pcol = colv - a.bitmap_base;
            if (pcol >= 0 && pcol < a.bitmap_n && ((bitmap[pcol >> 5] >> (pcol & 31)) & 1u)) return 0ull;
        } else if (seed_scan) {
            if (is_seed(colv)) return 0ull;
        }
        return ((u64)key << 32) | (u64)(~(unsigned)colv);
    };

    // ---- 2. first read: keys -> LDS (if they fit), count, min, max ---------------------------------
    // this thread's largest keys, one per class of its elements (class = visit number mod MAXES): MAXES x NTH
    // = 1024 (deep: CAP) distinct elements of the row in all
    u64 tmaxv[MAXES];
#pragma unroll
    for (int c = 0; c < MAXES; ++c) tmaxv[c] = 0ull;
    int visit = 0;
    auto note_max = [&](u64 ck) {
#pragma unroll
        for (int c = 0; c < MAXES; ++c)
            if ((visit % MAXES) == c) tmaxv[c] = ck > tmaxv[c] ? ck : tmaxv[c];
        ++visit;
    };
    {
        u64 mn = ~0ull, mx = 0ull;
        const int n_src = src.count(row, seg_prefix);
        if (Src::kFixedSlots && key_cap > 0 && n_src <= key_cap) {
            // dense source: element q goes to cache slot q (0 = absent) -- no compaction, hence no
            // ballot / leader atomic / shuffle per element group; the count is one atomic per wave
            unsigned cnt = 0;
            int calls = 0;
            src.template for_each<NTH>(row, tid, seg_prefix, [&](float z, int colv, bool in) {
                const u64 ck = ckey(z, colv, in);
                note_max(ck);
                const int slot = tid + NTH * calls++;
                if (slot < n_src) keys[slot] = ck;
                if (ck != 0ull) {
                    ++cnt;
                    mn = ck < mn ? ck : mn;
                    mx = ck > mx ? ck : mx;
                }
            });
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
            if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
            if (tid == 0) s_slots = (unsigned)n_src;
        } else if (key_cap > 0) {
            src.template for_each<NTH>(row, tid, seg_prefix, [&](float z, int colv, bool in) {
                const u64 ck = ckey(z, colv, in);
                note_max(ck);
                const bool v = ck != 0ull;
                // (the wave-aggregated append, open-coded here and in the collect of step 4: through dae_wave_append these
                // per-element loops cost dae_topk_dense +2.2 % -- profiles/topk_split_notes.md)
                const u64 bal = __ballot(v);
                if (bal) {
                    const int leader = __ffsll((long long)__ballot(1)) - 1;
                    unsigned base = 0;
                    if (lane == leader) base = atomicAdd(&s_cnt, (unsigned)__popcll(bal));
                    base = __shfl(base, leader);
                    if (v) {
                        const unsigned slot = base + __popcll(bal & ((1ull << lane) - 1ull));
                        if (slot < (unsigned)key_cap) keys[slot] = ck;
                        mn = ck < mn ? ck : mn;
                        mx = ck > mx ? ck : mx;
                    }
                }
            });
        } else {
            // nothing is cached: count, min and max only -- one atomic per wave instead of one per element group
            unsigned cnt = 0;
            src.template for_each<NTH>(row, tid, seg_prefix, [&](float z, int colv, bool in) {
                const u64 ck = ckey(z, colv, in);
                note_max(ck);
                if (ck != 0ull) {
                    ++cnt;
                    mn = ck < mn ? ck : mn;
                    mx = ck > mx ? ck : mx;
                }
            });
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
            if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const u64 omn = __shfl_xor(mn, d), omx = __shfl_xor(mx, d);
            mn = omn < mn ? omn : mn;
            mx = omx > mx ? omx : mx;
        }
        if (lane == 0) { atomicMin(&s_min, mn); atomicMax(&s_max, mx); }
    }
    __syncthreads();
    const unsigned m = s_cnt;                                   // valid elements
    const unsigned n_cached = s_slots ? s_slots : m;            // cache slots in use (fixed slots: the source size)
    const bool in_lds = key_cap > 0 && n_cached <= (unsigned)key_cap;   // all of them were kept in LDS
    unsigned k_eff = m < (unsigned)k ? m : (unsigned)k;        // outputs of the row (final after seed removal)
    const unsigned k_sel = seed_blind ? (unsigned)(k + ns) : (unsigned)k;
    const unsigned k_rank = m < k_sel ? m : k_sel;               // rank the narrowing stages cut at

    // every valid key, from LDS or (big rows) from the source again.  f(key) is called by WHOLE
    // waves (key == 0 for lanes without an element) so it may use wave-level aggregation.
    auto for_keys = [&](auto f) {
        if (in_lds) {
            for (unsigned i0 = 0; i0 < n_cached; i0 += NTH) {
                const unsigned i = i0 + tid;
                f(i < n_cached ? keys[i] : 0ull);
            }
        } else {
            src.template for_each<NTH>(row, tid, seg_prefix, [&](float z, int colv, bool in) {
                f(ckey(z, colv, in));
            });
        }
    };
    // histogram update with wave-level aggregation: the bulk of a row's logits falls into a
    // handful of bins, and same-address LDS atomics serialise; up to 6 rounds of "leader's bin:
    // one atomic for all lanes that share it", the (few, scattered) rest as plain atomics.
    auto hist_add = [&](unsigned bin, bool valid) {
        u64 todo = __ballot(valid);
        for (int it = 0; it < 6 && todo; ++it) {
            const int leader = __ffsll((long long)todo) - 1;
            const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
            const u64 same = __ballot(valid && bin == lb);
            if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
            if (bin == lb) valid = false;
            todo &= ~same;
        }
        if (valid) atomicAdd(&hist[bin], 1u);
    };

    // ---- 3a. cheap lower bound from ONE value per thread --------------------------------------------
    // The per-thread maxima are distinct elements of the row, so their k-th largest is <= the row's
    // k-th largest key: a valid cut.  With the row spread over 1024 threads it is also tight
    // (~1.4 k keys survive for k = 500), and it costs one histogram over <= 1024 values instead of
    // one over the whole row.
    u64 lo = s_min, hi = s_max;
    unsigned above = 0;                                          // keys > hi
    bool narrowed = false;
    if (m > (unsigned)sort_n) {
        if (tid == 0) { s_cnt2 = 0; s_min2 = ~0ull; }
        __syncthreads();
        {
            unsigned nhas = 0;
            u64 wmn = ~0ull;
#pragma unroll
            for (int c = 0; c < MAXES; ++c) {
                nhas += tmaxv[c] != 0ull ? 1u : 0u;
                wmn = (tmaxv[c] != 0ull && tmaxv[c] < wmn) ? tmaxv[c] : wmn;
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const u64 o = __shfl_xor(wmn, d); wmn = o < wmn ? o : wmn;
                nhas += __shfl_xor(nhas, d);
            }
            if (lane == 0 && nhas) { atomicAdd(&s_cnt2, nhas); atomicMin(&s_min2, wmn); }
        }
        __syncthreads();
        const unsigned n_max = s_cnt2;
        if (n_max >= k_rank) {
            const u64 mlo = s_min2, mhi = s_max;                 // the row maximum is a thread maximum
            const u64 range = mhi - mlo;
            int shift = 64 - 11 - __clzll(range | 1ull);
            if (shift < 0) shift = 0;
            for (int b = tid; b < TK_BINS; b += NTH) hist[b] = 0;
            __syncthreads();
#pragma unroll
            for (int c = 0; c < MAXES; ++c)
                if (tmaxv[c] != 0ull) atomicAdd(&hist[(unsigned)((tmaxv[c] - mlo) >> shift)], 1u);
            __syncthreads();
            dae_rank_find_bin<NTH>(hist, wave_tot, tid, k_rank, &s_bin, &s_above);
            const u64 cut = mlo + ((u64)(unsigned)s_bin << shift);   // <= k-th largest thread maximum
            __syncthreads();
            // count the row's keys >= cut
            unsigned cnt = 0;
            for_keys([&](u64 ck) { cnt += (ck != 0ull && ck >= cut) ? 1u : 0u; });
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
            if (tid == 0) s_cnt2 = 0;
            __syncthreads();
            if (lane == 0) atomicAdd(&s_cnt2, cnt);
            __syncthreads();
            if (s_cnt2 <= (unsigned)sort_n) { lo = cut; narrowed = true; }
            else { lo = cut; }                                   // still a valid cut: narrow inside it
            __syncthreads();
        }
    }

    // ---- 3b. general narrowing of [lo, hi] until the keys >= lo fit the sort buffer ----------------
    if (m > (unsigned)sort_n && !narrowed)
        dae_rank_narrow<NTH>(for_keys, hist_add, lo, hi, above, k_rank, (unsigned)sort_n, hist, wave_tot, &s_bin, &s_above, tid);

    // ---- 4. collect keys >= lo, sort descending, emit -------------------------------------------------
    for (int i = tid; i < sort_n; i += NTH) skey[i] = 0ull;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    if (in_lds) {
        for (unsigned i0 = 0; i0 < n_cached; i0 += NTH) {
            const unsigned i = i0 + tid;
            const u64 ck = i < n_cached ? keys[i] : 0ull;
            const bool v = ck != 0ull && ck >= lo;
            const u64 bal = __ballot(v);
            if (bal) {
                const int leader = __ffsll((long long)__ballot(1)) - 1;
                unsigned base = 0;
                if (lane == leader) base = atomicAdd(&s_cnt, (unsigned)__popcll(bal));
                base = __shfl(base, leader);
                const unsigned slot = base + __popcll(bal & ((1ull << lane) - 1ull));
                if (v && slot < (unsigned)sort_n) skey[slot] = ck;
            }
        }
    } else {
        src.template for_each<NTH>(row, tid, seg_prefix, [&](float z, int colv, bool in) {
            const u64 ck = ckey(z, colv, in);
            const bool v = ck != 0ull && ck >= lo;
            const u64 bal = __ballot(v);
            if (bal) {
                const int leader = __ffsll((long long)__ballot(1)) - 1;
                unsigned base = 0;
                if (lane == leader) base = atomicAdd(&s_cnt, (unsigned)__popcll(bal));
                base = __shfl(base, leader);
                const unsigned slot = base + __popcll(bal & ((1ull << lane) - 1ull));
                if (v && slot < (unsigned)sort_n) skey[slot] = ck;
            }
        });
    }
    __syncthreads();

    // ---- 4a. lean mode: drop the seeds among the collected keys (order is irrelevant here) ------------
    if (seed_blind) {
        u64 kk[EMAX];
        bool keep[EMAX];
        const unsigned c = s_cnt < (unsigned)sort_n ? s_cnt : (unsigned)sort_n;
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const unsigned i = (unsigned)(e * NTH + tid);
            kk[e] = i < c ? skey[i] : 0ull;
            keep[e] = kk[e] != 0ull && !is_seed((int)(~(unsigned)(kk[e] & 0xFFFFFFFFull)));
        }
        __syncthreads();                                         // every skey read is done
        if (tid == 0) s_cnt = 0;
        for (int i = tid; i < sort_n; i += NTH) skey[i] = 0ull;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const unsigned slot = dae_wave_append(&s_cnt, keep[e], lane);
            if (keep[e]) skey[slot] = kk[e];
        }
        __syncthreads();
        // >= k + ns keys were above the cut and <= ns of them were seeds; short rows were collected whole
        k_eff = s_cnt < (unsigned)k ? s_cnt : (unsigned)k;
    }

    // one winner to position i of the row's outputs
    auto emit_key = [&](u64 key, unsigned i) {
        const float z = dae_okey_inv((unsigned)(key >> 32));
        const int colv = (int)(~(unsigned)(key & 0xFFFFFFFFull));
        const size_t o = (size_t)row * k + i;
        if (a.out_idx) a.out_idx[o] = colv;
        if (a.out_score) a.out_score[o] = a.out_kind == DAE_OUT_SCORE ? dae_sigmoidf(z) : z;
        if (a.out_pairs) a.out_pairs[(size_t)row * a.pairs_stride + i] = make_uint2(__float_as_uint(z), (unsigned)colv);
        if (a.out_tau && i == (unsigned)k - 1) a.out_tau[row] = z;
    };
    // ---- 5a. k <= 512 (at most 1024 keys were collected): order by histogram rank (rank_lds.h dae_rank_order) ----------
    if (CAP == TK_SORT_MAX && sort_n == 1024) {
        constexpr int PER = 1024 / NTH;                          // collected keys per thread (slot e * NTH + tid)
        const unsigned c = s_cnt < 1024u ? s_cnt : 1024u;
        u64 mine[PER];
        unsigned rk[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) mine[e] = (unsigned)(e * NTH + tid) < c ? skey[e * NTH + tid] : 0ull;
        for (int b2 = tid; b2 < TK_BINS; b2 += NTH) hist[b2] = 0;
        __syncthreads();                                         // also: every skey read above is done
        // every collected key lies in [lo, s_max].  The `above` table takes the sort buffer (2048 x 4 B = its 1024 x 8 B), the
        // second buffer the key cache region (>= 1024 keys: launch_topk)
        dae_rank_order<NTH>(mine, lo, s_max, hist, reinterpret_cast<unsigned*>(skey), keys, wave_tot, nullptr, tid, rk);
        __syncthreads();                                         // the `above` table is dead: the sort buffer takes the winners
        dae_rank_emit_ordered<NTH>(mine, rk, k_eff, skey, tid, emit_key);
    } else
    // Hybrid bitonic sort, descending.  Thread t holds elements t, t + NTH, ... (E = sort_n / NTH of them,
    // at least one).  Strides < 64 exchange through wave shuffles, larger ones through LDS -- also when both
    // elements of a pair sit in the same thread (every key is in LDS for that step anyway).
    {
        const int E = sort_n > NTH ? sort_n / NTH : 1;
        u64 kr[EMAX];
#pragma unroll
        for (int e = 0; e < EMAX; ++e) kr[e] = (e < E && e * NTH + tid < sort_n) ? skey[e * NTH + tid] : 0ull;
        for (int size = 2; size <= sort_n; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (stride >= 64) {
                    __syncthreads();
#pragma unroll
                    for (int e = 0; e < EMAX; ++e)
                        if (e < E && e * NTH + tid < sort_n) skey[e * NTH + tid] = kr[e];
                    __syncthreads();
#pragma unroll
                    for (int e = 0; e < EMAX; ++e) {
                        if (e < E) {
                            const int i = e * NTH + tid;
                            const u64 other = i < sort_n ? skey[i ^ stride] : 0ull;
                            const bool desc = ((i & size) == 0);
                            const bool lower = ((i & stride) == 0);
                            const u64 mx = kr[e] > other ? kr[e] : other;
                            const u64 mn = kr[e] > other ? other : kr[e];
                            kr[e] = (lower == desc) ? mx : mn;
                        }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EMAX; ++e) {
                        if (e < E) {
                            const int i = e * NTH + tid;
                            const u64 other = __shfl_xor(kr[e], stride);
                            const bool desc = ((i & size) == 0);
                            const bool lower = ((i & stride) == 0);
                            const u64 mx = kr[e] > other ? kr[e] : other;
                            const u64 mn = kr[e] > other ? other : kr[e];
                            kr[e] = (lower == desc) ? mx : mn;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < EMAX; ++e) {
            const unsigned i = (unsigned)(e * NTH + tid);
            if (e < E && i < k_eff) emit_key(kr[e], i);
        }
    }
    // fewer than k valid elements: pad like the reference's cand[:500] of a short list
    for (unsigned i = k_eff + tid; i < (unsigned)k; i += NTH) {
        const size_t o = (size_t)row * k + i;
        if (a.out_idx) a.out_idx[o] = -1;
        if (a.out_score) a.out_score[o] = -__builtin_inff();
        if (a.out_pairs) a.out_pairs[(size_t)row * a.pairs_stride + i] = make_uint2(__float_as_uint(-__builtin_inff()), 0xFFFFFFFFu);
    }
    if (a.out_tau && tid == 0 && k_eff < (unsigned)k) a.out_tau[row] = -__builtin_inff();
}

template <typename Src>
int launch_topk(dae_ctx* ctx, const Src& src, const dae_topk_args& a)
{
    if (a.k < 1 || a.k > DAE_MAX_K_DEEP)
        return dae_fail(ctx, DAE_ERR_ARG, "k=%d out of [1,%d]", a.k, DAE_MAX_K_DEEP);
    if (a.B <= 0) return DAE_OK;
    const bool deep = a.k > DAE_MAX_K;                           // topk_kernel<Src, 1024, TK_SORT_DEEP>
    int sort_n = 1024;
    if (a.k > 512) sort_n = TK_SORT_MAX;
    if (deep) sort_n = a.k > TK_SORT_DEEP / 4 ? TK_SORT_DEEP : TK_SORT_DEEP / 2;
    dae_topk_args aa = a;
    aa.sort_cap = sort_n;
    // Two LDS modes, both covered by the parity tests:
    //   bitmap (default): per-row seed bitmap + a key cache filling the CU's LDS -- fastest alone.
    //   lean: no bitmap (seed-blind narrowing at rank k + n_seeds, seeds removed once
    //     from the collected keys), sort buffer + small cache only: <= 30 KiB and <= 56 registers per
    //     thread, so a workgroup fits on a CU NEXT to a decode workgroup of another batch.  Measured
    //     (profiles/r01_notes.md): the co-resident decode launch slows down by about what the overlap
    //     gains, and the kernel alone is slower (re-reads its source), so it is not the default.
    //     (deep rows: the sort buffer alone is 32 / 64 KiB -- no cache beside it, nothing shares the CU.)
    // a ranked range too wide for the LDS bitmap (> ~1 M columns) takes the bitmap-free mode instead of failing
    aa.lean = (((size_t)((a.bitmap_n + 31) / 32) * 4) + 15) + (size_t)sort_n * 8 + 22 * 1024 > (size_t)160 * 1024 ? 1 : 0;
    const size_t lds_total = TK_LDS_TOTAL, lds_static = TK_LDS_STATIC;
    size_t dyn;
    int key_cap;
    if (aa.lean) {
        const size_t budget = 30 * 1024 - (sizeof(unsigned) * TK_BINS + (Src::kSegs ? (Src::kSegs + 2) * 4 : 8) + 256);
        const size_t sk = (size_t)sort_n * 8;
        key_cap = budget > sk ? (int)((budget - sk) / 8) : 0;
        dyn = sk + (size_t)key_cap * 8;
    } else {
        const size_t bm_bytes = (((size_t)((a.bitmap_n + 31) / 32) * 4) + 15) & ~(size_t)15;
        if (bm_bytes + (size_t)sort_n * 8 + lds_static + 8 * 1024 > lds_total)
            return dae_fail(ctx, DAE_ERR_ARG, "ranked column range %d too wide for the LDS seed bitmap",
                            a.bitmap_n);
        // bitmap + sort buffer + key cache.  The cache is sized to what a row can hold, not to the CU:
        // with many rows of few keys (large batches, vocabulary shards) two workgroups then share a CU.
        const size_t room = lds_total - lds_static - bm_bytes - (size_t)sort_n * 8;
        size_t want = (size_t)(src.max_keys() > 0 ? src.max_keys() : 8192) * 8;
        if (want < 1024 * 8) want = 1024 * 8;                   // the ordering stage's second buffer (1024 keys)
        if (deep) want = room;                                   // one workgroup per CU whatever the cache: a deep row keeps what fits
        if (want > room) want = room;
        key_cap = (int)(want / 8);
        dyn = bm_bytes + (size_t)sort_n * 8 + want;
    }
    static const char attr_set_key = 0, attr_set_key_deep = 0;
    if (deep && dae_first_use(ctx, &attr_set_key_deep))
        DAE_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_kernel<Src, 1024, TK_SORT_DEEP>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(lds_total - lds_static)));
    if (!deep && dae_first_use(ctx, &attr_set_key)) {
        DAE_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_kernel<Src, 1024>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(lds_total - lds_static)));
        DAE_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&topk_kernel<Src, 256>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(lds_total - lds_static)));

    }
    // threads per row: 256 for rows known to be short (see topk_kernel): dense rows of <= 4096 columns (the
    // sample of a small vocabulary shard) and gathered shard lists.  Candidate lists (PairSrc) keep 1024: their
    // cost is walking the per-workgroup segments (one wave per segment), which 4 waves do slower than 16
    // (measured: 407 vs 354 us per step at --sim-world 8).
    const int bound = Src::kSegs ? 0 : src.max_keys();
    // ... and candidate lists when the launch has many rows (>= 4 per CU: large batches, vocabulary shards): a row then
    // holds few candidates, four 256-thread workgroups share a CU, and the per-row fixed cost is what counts
    // (--sim-world 8, 2048 rows: step 322 -> 284 us; at 256 rows 256 threads lose: 22 vs 14 us)
    const bool small = (!Src::kSegs && bound <= 4096) || (Src::kSegs && (a.B >= 1024 || a.prefer_small));
    if (deep)                                                    // never the 256-thread shape: 8192 keys are 8 per thread of 1024
        hipLaunchKernelGGL((topk_kernel<Src, 1024, TK_SORT_DEEP>), dim3(a.B), dim3(1024), dyn, ctx->stream, src, aa, key_cap);
    else if (small)
        hipLaunchKernelGGL((topk_kernel<Src, 256>), dim3(a.B), dim3(256), dyn, ctx->stream, src, aa, key_cap);
    else
        hipLaunchKernelGGL((topk_kernel<Src, 1024>), dim3(a.B), dim3(1024), dyn, ctx->stream, src, aa, key_cap);
    DAE_CHECK_LAUNCH(ctx, "topk_kernel");
    return DAE_OK;
}

}  // namespace

int dae_launch_topk_dense(dae_ctx* ctx, const dae_dense_src& s, const dae_topk_args& a)
{
    DenseSrc src{s};
    return launch_topk(ctx, src, a);
}

int dae_launch_topk_soa(dae_ctx* ctx, int G, const float* logit, const int32_t* idx,
                        const dae_topk_args& a)
{
    SoaSrc src{logit, idx, G, a.B, a.k};
    return launch_topk(ctx, src, a);
}

int dae_launch_topk_pairs(dae_ctx* ctx, const dae_pair_group& g0, const dae_pair_group& g1,
                          const dae_topk_args& a)
{
    if (g0.nseg + g1.nseg > TK_MAX_SEG)
        return dae_fail(ctx, DAE_ERR_ARG, "too many candidate segments (%d)", g0.nseg + g1.nseg);
    PairSrc src{g0, g1};
    return launch_topk(ctx, src, a);
}
