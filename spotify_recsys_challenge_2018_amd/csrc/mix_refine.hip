// mix_refine.hip -- the refine launch of the exact title mix (mixexact.hip has the overview), one 1024-thread workgroup per row:
// (1) the mixed bounds [l, u] of every column the filter launch listed, densely; the need-th largest l is a threshold tau' that
// `need` columns provably reach, so only columns with u >= tau' can be among the k best; (2) those survivors recomputed with
// the canonical fp32 chains and mixed as the fp32 path mixes them, tested against the filter's promise (bound guard), and
// either ordered here (fused selection) or left as one compact (y, column) list per row for the selection kernel.
#include "decode_common.h"
#include "mix_common.h"
#include "rank_lds.h"

namespace {

static_assert(MR_RANK_MAX == DAE_RANK_MAX, "mix_plan.h decides `fuse` by the ordering stage's size");

// ---- refine: bounds of every candidate, the ones that can still be among the k best recomputed in fp32 -------------------
constexpr int MR_THREADS = 1024, MR_WAVES = 16;
// ring of 2 blocks per chain: hipcc waits for every load in flight at each block anyway (run-time bounds around the refills), so a deeper
// ring bought nothing but registers -- at depth 4 the kernel spilled 12 of them into its chains (137 -> 131 us per 750 rows)
constexpr int MR_DEPTH = 2;
constexpr int MR_ROWSTRIDE = 20;       // dwords per candidate in a wave's transposition buffer (refine.hip)
constexpr int MR_BINS = 2048;

struct MixRefP {
    const uint4* base; const int* cnt; int64_t seg_stride, row_stride, cnt_seg_stride; int nseg;
    const float* hD; int64_t ld_hD; int HD; const float* W32D; const float* biasD; const float* epsD;
    const float* hT; int64_t ld_hT; int HT; const float* W32T; const float* biasT; const float* alphaT; const float* betaT;
    const unsigned* fhat; const float* w_t; const float* w_p; const int* row_bad;
    const int32_t* seed_row_ptr; int k; int n_valid_col;
    uint2* out; int* out_cnt; int out_cap;
    int* guard;                        // {violations, a violating column}
    int* stat;                         // [B][2] {candidates, recomputed}
    // FUSED SELECTION (round 5, as refine.hip; k <= 512): the launch ends the call -- the row's seeds out, its k best mixed
    // scores in order (main_challenge.py:26-36 on DAEs.py:180's y) to fo.out_score / out_idx; `out` then only takes the rows
    // with more survivors than the ordering stage holds
    int fuse;
    dae_rank_out fo;
    const int32_t* seed_col;
};

// One group of 64 candidates, a lane each: the canonical chain acc = fmaf(hrow[k], W32[rowidx][k], acc), k = 0 .. H-1, from
// +0 (oracle orc_decode; what v_mfma_f32_32x32x2_f32 performs in the fp32 kernels).  The rows are fetched quad-wise -- the
// 4 lanes of a quad read 64 contiguous bytes of one row per instruction -- and handed to their lanes through the wave's
// LDS buffer; the hidden factors travel by v_readlane (refine.hip rescore_group, which this restates for two scorers).
// H % 16 == 0; hrow zero beyond H up to the next multiple of 64.
template <int DEPTH>
__device__ __forceinline__ float mix_chain64(const float* __restrict__ W32, int H, const float* hrow, float* tbuf, int lane, int rowidx)
{
    const int Q = lane >> 2, q = lane & 3;
    const int H16 = H >> 4;
    const float4* rp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ci = __shfl(rowidx, 4 * Q + i);
        rp[i] = reinterpret_cast<const float4*>(W32 + (size_t)ci * H) + q;
    }
    float4 v[DEPTH][4];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[d][i] = d < H16 ? rp[i][4 * d] : make_float4(0.f, 0.f, 0.f, 0.f);
    float acc = 0.0f;
    constexpr int U = DEPTH < 4 ? 4 : DEPTH;
    for (int j0 = 0; j0 < H16; j0 += U) {
        float hq[U / 4];
#pragma unroll
        for (int c = 0; c < U / 4; ++c) hq[c] = hrow[16 * j0 + 64 * c + lane];
#pragma unroll
        for (int dd = 0; dd < U; ++dd) {
            const int jb = j0 + dd;
            const int d = dd & (DEPTH - 1);
            if (jb < H16) {                                       // wave-uniform
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<float4*>(tbuf + (4 * Q + i) * MR_ROWSTRIDE + 4 * q) = v[d][i];
                __builtin_amdgcn_wave_barrier();
                // the ring is refilled in PAIRS of blocks: the two halves of a row's 128-byte line are requested back to back, so
                // the second finds the line pending instead of fetching it again (refine.hip rescore_group has the measurement)
                if (dd & 1) {
                    const int dp = (dd - 1) & (DEPTH - 1);
                    const int jn0 = jb - 1 + DEPTH, jn1 = jb + DEPTH;
                    if (jn0 < H16) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[dp][i] = rp[i][4 * jn0];
                    }
                    if (jn1 < H16) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[d][i] = rp[i][4 * jn1];
                    }
                }
                float4 w[4];
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) w[tq] = *reinterpret_cast<const float4*>(tbuf + lane * MR_ROWSTRIDE + 4 * tq);
                __builtin_amdgcn_wave_barrier();
                const int hc = (int)__float_as_uint(hq[dd >> 2]);
#pragma unroll
                for (int tq = 0; tq < 4; ++tq) {
                    const int l0 = 16 * (dd & 3) + 4 * tq;
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0)), w[tq].x, acc);
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0 + 1)), w[tq].y, acc);
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0 + 2)), w[tq].z, acc);
                    acc = fmaf(__uint_as_float((unsigned)__builtin_amdgcn_readlane(hc, l0 + 3)), w[tq].w, acc);
                }
            }
        }
    }
    return acc;
}

// two floats further from the value than the rounded subtraction left it
__device__ __forceinline__ float two_down(float x) { return dae_okey_inv(dae_okey(x) - 2u); }

// (The library is built with -fno-vectorize: hipcc's loop vectorizer miscompiled this kernel's per-lane staging loop in round 4 --
// spotify_recsys_challenge_2018_amd/build.py, scripts/probe/vec_repro.hip.)
__global__ __launch_bounds__(MR_THREADS, 1) void mix_refine_kernel(const MixRefP p)
{
    __shared__ int seg_prefix[MR_MAX_SEG + 2];
    __shared__ float hrowD[1024];
    __shared__ float hrowT[1024];
    __shared__ __attribute__((aligned(16))) float tb[MR_WAVES * 64 * MR_ROWSTRIDE];      // the waves' buffers; before: the histogram
    // (static LDS beyond 64 KiB compiles, but its arrays then overlap at run time: the two key arrays are the launch's
    // dynamic LDS, as refine.hip's staging area)
    extern __shared__ __attribute__((aligned(16))) unsigned mr_dyn[];
    unsigned* kl = mr_dyn;                       // keys of the lower bounds; afterwards the survivors' flat indices
    unsigned* ku = mr_dyn + MR_STAGE;            // keys of the upper bounds
    __shared__ unsigned cnts[32];
    __shared__ int s_n;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const int nseg = p.nseg;
    const bool bad = p.row_bad && p.row_bad[row] != 0;
    // fused selection: the row's seeds are requested with the prologue's loads (one per thread in a register; playlists with
    // more than MR_THREADS seed tracks read the rest when the bitmap is built)
    const int seed_b = (p.fuse && p.seed_col) ? p.seed_row_ptr[row] : 0;
    const int seed_e = (p.fuse && p.seed_col) ? p.seed_row_ptr[row + 1] : 0;
    const int my_seed = seed_b + tid < seed_e ? p.seed_col[seed_b + tid] : -1;
    __shared__ unsigned f_range[2];              // {min, max} of the high words of the keys written to LDS
    for (int s = tid; s < nseg; s += MR_THREADS) seg_prefix[s + 1] = p.cnt[(size_t)s * p.cnt_seg_stride + row];
    if (tid == 0) { seg_prefix[0] = 0; s_n = 0; f_range[0] = 0xFFFFFFFFu; f_range[1] = 0u; }
    if (tid < 32) cnts[tid] = (tid == 1 || tid == 3) ? 0xFFFFFFFFu : 0u;      // [1], [3]: minima
    for (int i = tid; i < 1024; i += MR_THREADS) {
        hrowD[i] = i < p.HD ? p.hD[(size_t)row * p.ld_hD + i] : 0.0f;
        hrowT[i] = i < p.HT ? p.hT[(size_t)row * p.ld_hT + i] : 0.0f;
    }
    __syncthreads();
    if (tid < 64) {
        int carry = 0;
        for (int b0 = 0; b0 < nseg; b0 += 64) {
            const int i = b0 + tid;
            const int v = dae_wave_scan_incl(i < nseg ? seg_prefix[i + 1] : 0, tid);
            if (i < nseg) seg_prefix[i + 1] = v + carry;
            carry += __shfl(v, 63);
        }
    }
    __syncthreads();
    const int total = seg_prefix[nseg];
    auto give_up = [&](int code) {
        // a row the launch cannot vouch for (more candidates than its buffers hold): counted like a bound failure -- the
        // callers then re-score the launch with the fp32 kernels
        if (tid == 0) { p.out_cnt[row] = 0; atomicAdd(p.guard, 1); p.guard[1] = code; }
        if (p.fuse) dae_rank_pad<MR_THREADS>(tid, row, 0u, p.fo);
    };
    // ---- fused selection: LDS of the upper-bound keys once they are dead (after step 3; the streamed path never uses them):
    // [keys of the ordering stage: DAE_RANK_MAX x 8 B][seed bitmap over the rankable columns: <= 24 KiB]
    dae_u64* const fkey = reinterpret_cast<dae_u64*>(ku);
    unsigned* const bitmap = ku + 2 * DAE_RANK_MAX;
    const int bm_words = p.fuse ? (p.n_valid_col + 31) >> 5 : 0;
    auto build_bitmap = [&]() {                                   // (every thread; the callers' barrier before it freed the area)
        for (int w = tid; w < bm_words; w += MR_THREADS) bitmap[w] = 0u;
        __syncthreads();
        for (int i = seed_b + tid; i < seed_e; i += MR_THREADS) {
            const int pc = i == seed_b + tid ? my_seed : p.seed_col[i];
            if (pc >= 0 && pc < p.n_valid_col) atomicOr(&bitmap[pc >> 5], 1u << (pc & 31));
        }
        __syncthreads();
    };
    auto fkey_of = [&](float y, int colv) -> dae_u64 {            // composite key of a score; 0 = absent (a seed, -inf)
        const unsigned key = dae_okey(y);
        if (colv < 0 || key <= DAE_KEY_NEG_INF) return 0ull;
        if (colv < p.n_valid_col && ((bitmap[colv >> 5] >> (colv & 31)) & 1u)) return 0ull;
        return ((dae_u64)key << 32) | (dae_u64)(~(unsigned)colv);
    };
    // the ordering stage's buffers: the waves' transposition buffers, free once the recomputation is over
    dae_u64* const sorted = reinterpret_cast<dae_u64*>(tb);
    unsigned* const above = reinterpret_cast<unsigned*>(sorted + DAE_RANK_MAX);
    unsigned* const fhist = above + DAE_RANK_BINS;
    uint2* const orow0 = p.out + (size_t)row * p.out_cap;
    auto select_from_list = [&](int n_list) {                     // the row's list in global memory -> its final lists
        dae_rank_select_emit<MR_THREADS>([&](auto f) {
            for (int e0 = 0; e0 < n_list; e0 += MR_THREADS) {
                const int e = e0 + tid;
                dae_u64 ck = 0ull;
                if (e < n_list) { const uint2 pr = orow0[e]; ck = fkey_of(__uint_as_float(pr.x), (int)pr.y); }
                f(ck);
            }
        }, fkey, sorted, fhist, above, tid, row, p.fo);
    };
    if (!bad && p.w_t[row] == 0.0f && p.w_p[row] == 0.0f) {
        // y = sigmoid(.) * 0 + sigmoid(.) * 0 = +0 for every column: the fp32 path ranks (y desc, column asc), i.e. the first
        // k non-seed columns -- the first k + n_seeds columns cover them
        const int nl = min(p.k + (p.seed_row_ptr ? p.seed_row_ptr[row + 1] - p.seed_row_ptr[row] : 0), min(p.n_valid_col, p.out_cap));
        for (int i = tid; i < nl; i += MR_THREADS) p.out[(size_t)row * p.out_cap + i] = make_uint2(0u, (unsigned)i);
        if (tid == 0) { p.out_cnt[row] = nl; if (p.stat) { p.stat[2 * row] = 0; p.stat[2 * row + 1] = 0; } }
        if (p.fuse) { build_bitmap(); select_from_list(nl); }
        return;
    }
    if (bad || total == 0) {
        if (tid == 0) { p.out_cnt[row] = 0; if (p.stat) { p.stat[2 * row] = total; p.stat[2 * row + 1] = 0; } }
        if (p.fuse) dae_rank_pad<MR_THREADS>(tid, row, 0u, p.fo);
        return;
    }
    const int need = p.k + (p.seed_row_ptr ? p.seed_row_ptr[row + 1] - p.seed_row_ptr[row] : 0);
    const float wt = p.w_t[row], wp = p.w_p[row];
    const float F = __uint_as_float(p.fhat[row] << 16);

    // ---- 1. the mixed bounds of every candidate, as order-preserving keys.  Flat over the row's candidates, four per thread
    // and round with their loads issued together: the entry first, then the three bound terms of its column -- two trips to
    // memory per round.  (A wave per segment, 64 entries at a time, made every 64 entries two DEPENDENT trips: 16 of them
    // per wave and row.)
    auto offset_of = [&](int e) -> int64_t {
        int lo = 0, hi = nseg;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg_prefix[mid] <= e) lo = mid; else hi = mid;
        }
        return (int64_t)lo * p.seg_stride + (int64_t)row * p.row_stride + (e - seg_prefix[lo]);
    };
    constexpr int MR_U = 4;
    // body(i, key of l, key of u) for every candidate i of the round starting at c0
    auto bounds_round = [&](int c0, auto body) {
        uint4 en[MR_U];
#pragma unroll
        for (int q = 0; q < MR_U; ++q) {
            const int i = c0 + q * MR_THREADS + tid;
            en[q] = p.base[offset_of(i < total ? i : 0)];
        }
        float al[MR_U], be[MR_U], ep[MR_U];
#pragma unroll
        for (int q = 0; q < MR_U; ++q) {
            const int col = (int)en[q].z;
            al[q] = p.alphaT[col]; be[q] = p.betaT[col]; ep[q] = p.epsD[col];
        }
#pragma unroll
        for (int q = 0; q < MR_U; ++q) {
            const int i = c0 + q * MR_THREADS + tid;
            const float uT = __uint_as_float(en[q].x), uD = __uint_as_float(en[q].y);
            const float wdT = 2.0f * fmaf(al[q], F, be[q]) * 1.000001f;
            const float wdD = 2.0f * ep[q] * 1.000001f;
            // (the narrowing only needs bounds of the canonical value: the hardware's exp2 / rcp, 2^-15 wider)
            const float up = mix_fast_up(uT, uD, wt, wp);
            const float lo = mix_fast_dn(two_down(uT - wdT), two_down(uD - wdD), wt, wp);
            body(i, i < total, dae_okey(lo), dae_okey(up));
        }
    };
    const bool staged = total <= MR_STAGE;                        // both keys of every candidate fit LDS
    unsigned kmx = 0u, kmn = 0xFFFFFFFFu;
    if (staged) {
        for (int c0 = 0; c0 < total; c0 += MR_U * MR_THREADS)
            bounds_round(c0, [&](int i, bool in, unsigned a, unsigned u) {
                if (in) { kl[i] = a; ku[i] = u; kmx = a > kmx ? a : kmx; kmn = a < kmn ? a : kmn; }
            });
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned a = __shfl_xor(kmx, d), b = __shfl_xor(kmn, d);
        kmx = a > kmx ? a : kmx; kmn = b < kmn ? b : kmn;
    }
    if (lane == 0) { atomicMax(&cnts[0], kmx); atomicMin(&cnts[1], kmn); }
    unsigned* hist = reinterpret_cast<unsigned*>(tb);
    for (int i = tid; i < MR_BINS; i += MR_THREADS) hist[i] = 0u;
    __syncthreads();

    // ---- 2. tau': the need-th largest lower bound (to a 2048-bin histogram over [min, max] of the row's keys and one pass
    // for the smallest key of the selected bin, as refine.hip): `need` distinct columns provably reach it
    unsigned P = 0u;                                             // key of tau' (0: everything survives)
    // the bin that holds the need-th largest key of the histogram, counted from the top (block-uniform, via cnts[2])
    auto select_bin = [&](int need_) -> int {                     // (cnts[5]: how many keys lie in the bins above it)
        constexpr int BPT = MR_BINS / MR_THREADS;
        const int top = MR_BINS - 1 - BPT * tid;
        unsigned hc[BPT], own = 0;
#pragma unroll
        for (int e = 0; e < BPT; ++e) { hc[e] = hist[top - e]; own += hc[e]; }
        unsigned incl = dae_wave_scan_incl(own, lane);
        if (lane == 63) cnts[8 + wave] = incl;
        __syncthreads();
        unsigned pre = 0;
        for (int w = 0; w < wave; ++w) pre += cnts[8 + w];
        incl += pre;
        const unsigned excl = incl - own;
        if (excl < (unsigned)need_ && (unsigned)need_ <= incl) {
            unsigned run = excl;
            bool done = false;
#pragma unroll
            for (int e = 0; e < BPT; ++e) {
                if (!done && run + hc[e] >= (unsigned)need_) { cnts[2] = (unsigned)(top - e); cnts[5] = run; done = true; }
                run += hc[e];
            }
        }
        __syncthreads();
        return (int)cnts[2];
    };
    int* surv = reinterpret_cast<int*>(kl);                       // the survivors' flat indices (the staged path: in kl's place)
    auto append = [&](bool keep, int i) {                         // (whole waves call this)
        const unsigned long long bal = __ballot(keep);
        if (bal) {
            const int leader = __ffsll((long long)bal) - 1;
            int b = 0;
            if (lane == leader) b = atomicAdd(&s_n, __popcll(bal));
            b = __shfl(b, leader);
            const int at = b + __popcll(bal & ((1ull << lane) - 1ull));
            if (keep && at < 2 * MR_STAGE) surv[at] = i;          // (beyond out_cap <= 2 MR_STAGE the row gives up below)
        }
    };
    if (!staged) {
        // STREAMED (a flat DAE bias: the threshold sample says little and a row lists tens of thousands of columns): nothing
        // is staged.  Pass A: histogram of the lower bounds over FIXED bins (1/32 of an octave of y between 2^-40 and 1),
        // A2 inside the bin holding the need-th largest; the lower edge of the sub-bin found is tau'.  Pass B: the bounds
        // again, survivors listed.
        constexpr unsigned K0 = 0x80000000u | 0x2B800000u;        // key of 2^-40
        auto fbin = [&](unsigned key) -> int {
            if (key < K0) return 0;
            const unsigned bq = (key - K0) >> 18;
            return (int)(bq < (unsigned)(MR_BINS - 1) ? bq : (unsigned)(MR_BINS - 1));
        };
        for (int c0 = 0; c0 < total; c0 += MR_U * MR_THREADS)
            bounds_round(c0, [&](int, bool in, unsigned a, unsigned) { if (in) atomicAdd(&hist[fbin(a)], 1u); });
        __syncthreads();
        if (total > need) {
            const int Bsel = select_bin(need);
            P = Bsel > 0 ? K0 + ((unsigned)Bsel << 18) : 0u;
            if (Bsel > 0 && Bsel < MR_BINS - 1) {
                // ... refined: with a flat bias thousands of bounds share that bin (2 % of y wide).  Pass A2: the keys of the
                // selected bin alone, in 2048 sub-bins of 128 key units (1.5e-5 of y)
                const int need2 = need - (int)cnts[5];
                __syncthreads();                                  // (everybody has read cnts[5] and the histogram)
                for (int i = tid; i < MR_BINS; i += MR_THREADS) hist[i] = 0u;
                __syncthreads();
                const unsigned e0 = P;
                for (int c0 = 0; c0 < total; c0 += MR_U * MR_THREADS)
                    bounds_round(c0, [&](int, bool in, unsigned a, unsigned) {
                        if (in && fbin(a) == Bsel) atomicAdd(&hist[(a - e0) >> 7], 1u);
                    });
                __syncthreads();
                const int B2 = select_bin(need2);
                P = e0 + ((unsigned)B2 << 7);
            }
        }
        for (int c0 = 0; c0 < total; c0 += MR_U * MR_THREADS)
            bounds_round(c0, [&](int i, bool in, unsigned, unsigned u) { append(in && u >= P, i); });
    } else if (total > need) {
        const unsigned kmin = cnts[1], kmax = cnts[0];
        const float scale = 2047.999f / ((float)(kmax - kmin) + 1.0f);
        auto bin_of = [&](unsigned key) -> int {
            const unsigned bq = (unsigned)((float)(key - kmin) * scale);
            return (int)(bq < (unsigned)(MR_BINS - 1) ? bq : (unsigned)(MR_BINS - 1));
        };
        for (int i = tid; i < total; i += MR_THREADS) atomicAdd(&hist[bin_of(kl[i])], 1u);
        __syncthreads();
        const int Bsel = select_bin(need);
        unsigned kb = 0xFFFFFFFFu;
        for (int i = tid; i < total; i += MR_THREADS) {
            const unsigned key = kl[i];
            if (bin_of(key) == Bsel) kb = key < kb ? key : kb;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const unsigned o = __shfl_xor(kb, d); kb = o < kb ? o : kb; }
        if (lane == 0 && kb != 0xFFFFFFFFu) atomicMin(&cnts[3], kb);
        __syncthreads();
        if (cnts[3] != 0xFFFFFFFFu) P = cnts[3];
    }
    __syncthreads();                                             // (the last reads of kl and of the histogram)

    // ---- 3. the survivors: upper bound >= tau'.  Their flat indices take kl's place.
    if (staged) {
        for (int c0 = 0; c0 < total; c0 += MR_THREADS) {
            const int i = c0 + tid;
            append(i < total && ku[i] >= P, i);                   // (slot <= i: the list never overtakes the keys still to be read)
        }
    }
    __syncthreads();
    const int n = s_n;
    if (tid == 0 && p.stat) { p.stat[2 * row] = total; p.stat[2 * row + 1] = n; }
    if (n > p.out_cap) { give_up(-3); return; }
    const bool fast = p.fuse && n <= DAE_RANK_MAX;               // the survivors' keys stay in LDS
    if (p.fuse) build_bitmap();

    // ---- 4. recompute the survivors
    float* tbuf = tb + wave * (64 * MR_ROWSTRIDE);
    uint2* orow = p.out + (size_t)row * p.out_cap;
    const int gstep = MR_WAVES * 64;
    uint4 pr = make_uint4(0u, 0u, 0u, 0u);
    int g0 = wave * 64;
    if (g0 < n) pr = p.base[offset_of(surv[g0 + lane < n ? g0 + lane : g0])];
    for (; g0 < n; g0 += gstep) {
        const int e = g0 + lane;
        const bool in = e < n;
        const uint4 cur = pr;
        const int gn = g0 + gstep;
        if (gn < n) pr = p.base[offset_of(surv[gn + lane < n ? gn + lane : gn])];       // the next group's entries, under this group's rows
        const int col = (int)cur.z;
        const float zT = mix_chain64<MR_DEPTH>(p.W32T, p.HT, hrowT, tbuf, lane, col) + p.biasT[col];
        const float zD = mix_chain64<MR_DEPTH>(p.W32D, p.HD, hrowD, tbuf, lane, col) + p.biasD[col];
        const float y = mixf(zT, zD, wt, wp);
        if (in) {
            // BOUND GUARD: the filter launch promised u - width <= z32 <= u for both logits of every listed column
            const float uT = __uint_as_float(cur.x), uD = __uint_as_float(cur.y);
            const float wdT = 2.0f * fmaf(p.alphaT[col], F, p.betaT[col]) * 1.000001f;
            const float wdD = 2.0f * p.epsD[col] * 1.000001f;
            const bool ok = zT <= uT && zT >= two_down(uT - wdT) && zD <= uD && zD >= two_down(uD - wdD);
            if (!ok) { atomicAdd(p.guard, 1); p.guard[1] = col; }
            if (!fast) orow[e] = make_uint2(__float_as_uint(y), (unsigned)col);
        }
        if (fast) {                                               // (whole waves: the range of the keys by two DPP reductions)
            const dae_u64 ck = in ? fkey_of(y, col) : 0ull;
            if (in) fkey[e] = ck;
            const unsigned hi = (unsigned)(ck >> 32);
            const unsigned mx = dae_wave_max_u32(hi), mn = dae_wave_min_u32(ck != 0ull ? hi : 0xFFFFFFFFu);
            if (lane == 0 && mx != 0u) { atomicMin(&f_range[0], mn); atomicMax(&f_range[1], mx); }
        }
    }
    if (tid == 0) p.out_cnt[row] = n;
    if (!p.fuse) return;
    __syncthreads();                                             // the recomputation is over: its buffers become the ordering stage's
    if (fast) {
        for (int b = tid; b < DAE_RANK_BINS; b += MR_THREADS) fhist[b] = 0u;
        dae_rank_emit<MR_THREADS>(fkey, (unsigned)n, sorted, fhist, above, tid, row, p.fo, f_range);
    } else {
        select_from_list(n);
    }
}

}  // namespace

// The candidate segments of the filter launch (tc->cand / tc->cand_cnt: pl.nb per row) -> per row the compact list of its
// recomputed survivors in tc->refined ([Bpad][MX_REF_CAP] pairs, then [Bpad] counts) and, when pl.fuse, the call's lists.
int dae_launch_mix_refine(dae_ctx* tc, const dae_mix_plan& pl, const dae_packed& pd, const dae_packed& pt, const dae_mix_call& c)
{
    uint2* rf = static_cast<uint2*>(tc->refined.p);
    MixRefP r;
    memset(&r, 0, sizeof(r));
    r.base = static_cast<const uint4*>(tc->cand.p); r.cnt = static_cast<const int*>(tc->cand_cnt.p);
    r.seg_stride = (int64_t)pl.Bpad * pl.cap; r.row_stride = pl.cap; r.cnt_seg_stride = pl.Bpad; r.nseg = pl.nb;
    r.hD = c.h; r.ld_hD = c.ld_h; r.HD = pd.H; r.W32D = static_cast<const float*>(pd.W32.p);
    r.biasD = static_cast<const float*>(pd.bias.p); r.epsD = static_cast<const float*>(pd.eps.p);
    r.hT = c.feat; r.ld_hT = c.ld_feat; r.HT = pt.H; r.W32T = static_cast<const float*>(pt.W32.p);
    r.biasT = static_cast<const float*>(pt.bias.p);
    r.alphaT = static_cast<const float*>(pt.mix_alpha.p); r.betaT = static_cast<const float*>(pt.mix_beta.p);
    r.fhat = static_cast<const unsigned*>(tc->mix_fhat.p); r.w_t = c.w_title; r.w_p = c.w_playlist;
    r.row_bad = static_cast<const int*>(tc->row_bad.p);
    r.seed_row_ptr = c.seed_row_ptr; r.k = c.k; r.n_valid_col = pl.n_valid_col;
    r.out = rf; r.out_cnt = reinterpret_cast<int*>(rf + (size_t)pl.Bpad * MX_REF_CAP); r.out_cap = MX_REF_CAP;
    r.guard = static_cast<int*>(tc->guard.p); r.stat = static_cast<int*>(tc->refstat.p);
    r.fuse = pl.fuse ? 1 : 0;
    r.fo = dae_rank_out{c.k, DAE_OUT_LOGIT, c.out_score, c.out_idx};   // (the mixed score is a probability already: it goes out as it is)
    r.seed_col = c.seed_col;
    const size_t lds = 2 * MR_STAGE * sizeof(unsigned);          // the two key arrays
    DAE_HIP_CHECK(tc, dae_lds_limit_once(tc, mix_refine_kernel, lds));
    hipLaunchKernelGGL(mix_refine_kernel, dim3(c.B), dim3(MR_THREADS), lds, tc->stream, r);
    DAE_CHECK_LAUNCH(tc, "mix_refine_kernel");
    return DAE_OK;
}
