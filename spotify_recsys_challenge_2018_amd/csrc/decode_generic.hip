// decode_generic.hip -- K2 on the prepacked image for ANY hidden size and row-group height: the generic decode kernel
// (decode_f32_kernel, fp32 and bf16 MFMA, its compile-time epilogues) and its instance table.  The hidden-256 shapes of the hot paths have
// kernels of their own in decode_f32.hip, whose launchers fall through to dae_launch_decode_generic for every other shape;
// the structure (hidden tile in LDS once per persistent workgroup, W streamed through a register ring, XCD-aware block
// order) is described at the head of that file.
#include "decode_common.h"

namespace {

// GT > 0: hidden size known at compile time (G = GT groups of 8 k) -> the k loop is fully
// unrolled, so no loop header sits between the register-ring loads and their use (hipcc drains
// vmcnt to 0 at every loop header; with the loop gone the waits are exact counted vmcnt(3)).
// HALF (phase A of the fp32 fused path, one round of tiles): the workgroup takes HALF a row group of the packed hidden
// image (RB row blocks of its 2 RB) and two workgroups share a CU -- two waves per SIMD, each with half the rows: the one's
// MFMAs run under the other's prologue (hidden tile -> LDS) and epilogue (exchange, sample store), which a single wave per
// SIMD leaves the matrix pipe idle for (28 us for 13.4 us of matrix work).  The exchange slots take the hidden tile's
// place in LDS (dead after the only round), so two workgroups fit: 2 x 64.5 KiB.  Same groups, same chains, same bits.
template <int RB, int EPI, int GT, int NW, int DT, int HALF = 0>
__global__ __launch_bounds__(NW * 64, HALF ? 2 : NW / 4) void decode_f32_kernel(const dae_decp p)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hi = lane >> 5;
    const int j = lane & 31;
    const int G = GT > 0 ? GT : p.G;
    constexpr int R_TILE = RB * 32;

    // XCD-aware block -> (row group, slot in row group)
    const int gs = DAE_NUM_XCD * p.n_rg;
    const int q = blockIdx.x / gs, rem = blockIdx.x % gs;
    const int rg = rem / DAE_NUM_XCD;
    const int bir = q * DAE_NUM_XCD + (rem % DAE_NUM_XCD);

    // wave-major slots: consecutive tiles go to different workgroups, so a partial round of tiles is
    // spread over all CUs (and, with two waves per SIMD, over all SIMDs) instead of filling a few
    const int n_ws = p.nb_rg * NW;
    const int item0 = dae_sample_slot_item(bir, wave, p.nb_rg);  // = wave * nb_rg + bir (score_plan.h: the decoded-tile table's mapping)
    const bool has0 = item0 < p.ts.n_items;
    // Tile indices come from a list in global memory.  A vector load that the code then waits for
    // drains the WHOLE in-order load queue (s_waitcnt vmcnt(0)), i.e. the W prefetch ring; so the
    // index of a tile is fetched two tiles ahead, before that tile's predecessor issues its W loads --
    // and the first two go out HERE, ahead of the hidden tile's loads, so that the W ring can be started before
    // the workgroup meets (the straight order -- tile, barrier, ids, W -- was one more dependent trip to memory
    // in front of the first MFMA).
    const int tv_cur = tile_of_item(p.ts, has0 ? item0 : 0);
    const int tv_nxt = tile_of_item(p.ts, has0 ? (item0 + n_ws < p.ts.n_items ? item0 + n_ws : item0) : 0);
    const int n_h4 = RB * 64 * G;
    // ---- HALF: tiles a bound puts below every threshold of the half group are not decoded ---------------
    // Before the sample runs, the image's bounds give a lower bound of every row's threshold: each group maximum is >= lo_c -
    // d m_c for each of its members, so the need-th largest maximum of a row is >= x = beta_(need) - d mu_max (beta: the groups'
    // max lo_c, sorted descending; d over the half group's real rows; need = k + the most seeds a row of it has), and the
    // threshold, which tau_select_kernel cuts to 16 key bits, is >= tau_safe = the same cut of x.  A tile with A_t + d M_t <
    // tau_safe holds no element that reaches any row's threshold: its maxima are not counted at the prefix the search returns and
    // none of its logits passes the threshold launch's >= tau -- so the wave stores -inf for it and decodes nothing (with a
    // decoded-tile table, p.sk.tab, it stores nothing at all and the threshold launch supplies the -inf: section 4).  Roundings go
    // the safe way (d rounded up by its producer, x down, U up as in dae_tile_is_live, whose !(U < tau) keeps a tile on any NaN).
    // Every wave takes the half group's d and need itself (64 lanes = its 64 rows; one trip to memory with the window of beta
    // that starts at k - 1 and the wave's own {A_t, M_t}): no LDS and no barrier before the workgroup's vote.
    bool skip_w = false;                                         // wave-uniform: this wave's tile is skipped
    if constexpr (HALF) {
        static_assert(RB == 2 && EPI == EPI_GMAX, "half row groups: the threshold sample, 64 rows");
        if (p.sk.ub) {
            int* const sk_live = reinterpret_cast<int*>(lds4 + n_h4);   // (the R_TILE ints behind the hidden tile: the filter epilogue's)
            const int row = rg * R_TILE + lane;
            const bool real = row < p.B;
            const float4 d4 = real ? reinterpret_cast<const float4*>(p.sk.row_d)[row] : make_float4(0.f, 0.f, 0.f, 0.f);
            int ns = (real && p.sk.seed_row_ptr) ? p.sk.seed_row_ptr[row + 1] - p.sk.seed_row_ptr[row] : 0;
            const int kb = p.sk.k - 1;
            float bw[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = kb + lane + 64 * u;
                bw[u] = idx < p.sk.n_beta ? p.sk.beta[idx] : -__builtin_inff();
            }
            const float mu = *p.sk.mu;
            const float2 ub = p.sk.ub[has0 ? item0 : 0];
            // (the workgroup's own counter word, asked for with the rest: launches of a context run one after the other)
            const unsigned long long cnt_was = tid == 0 ? p.sk.stat[blockIdx.x] : 0ull;
            float dq = dae_max_nan(dae_max_nan(d4.x, d4.y), dae_max_nan(d4.z, d4.w));
            ns = ns < 0 ? 0 : ns;
#pragma unroll
            for (int sh = 1; sh < 64; sh <<= 1) {
                dq = dae_max_nan(dq, __shfl_xor(dq, sh));
                const int o = __shfl_xor(ns, sh);
                ns = o > ns ? o : ns;
            }
            ns = __builtin_amdgcn_readfirstlane(ns);
            float beta_k;
            if (ns < 256) {
                const float sel = ns < 64 ? bw[0] : ns < 128 ? bw[1] : ns < 192 ? bw[2] : bw[3];
                beta_k = __shfl(sel, ns & 63);
            } else {                                             // (more seeds than the window: one more trip)
                beta_k = kb + ns < p.sk.n_beta ? p.sk.beta[kb + ns] : -__builtin_inff();
            }
            const double pm = (double)dq * (double)mu;           // exact: two floats
            double xd = (double)beta_k - pm;
            xd -= (fabs((double)beta_k) + fabs(pm)) * 0x1p-48;   // (more than the one rounding above)
            float xf = (float)xd;
            if ((double)xf > xd) xf = nextafterf(xf, -__builtin_inff());
            const float tau_safe = dae_tau_value(dae_okey(xf) >> 16, 1);      // tau_search.h: the cut tau itself gets
            // (a half group of pad rows alone stores nothing: nothing of it is decoded or counted)
            skip_w = has0 && (rg * R_TILE >= p.B || !dae_tile_is_live(ub.x, ub.y, (double)dq, tau_safe));
            skip_w = __builtin_amdgcn_readfirstlane((int)skip_w) != 0;
            if (lane == 0) sk_live[wave] = (has0 && !skip_w) ? 1 : 0;
            __syncthreads();
            int n_live = 0;
            unsigned word = 0;                                   // the workgroup's word of the decoded-tile table (score_plan.h)
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                n_live += sk_live[w];
                word |= (unsigned)sk_live[w] << (8 * w);
            }
            // (every workgroup of the launch stores its own word, this one included when it is zero: nobody clears the table)
            if (p.sk.tab && tid == 0) p.sk.tab[(size_t)rg * p.nb_rg + bir] = word;
            // ... and workgroup 0 of the half group its {dq, tau_safe}: D >= the d of every row of it, T <= every threshold of it --
            // what the threshold launch proves the filter launch's live list empty from (empty_proof.h), rewritten by every launch
            if (p.sk.pair && bir == 0 && tid == 0) p.sk.pair[rg] = make_float2(dq, tau_safe);
            if (n_live == 0 && p.sk.tab) return;                 // ... and its maxima and dense slots stay as they stand, unread
            if (n_live == 0) {
                // nothing to decode in this workgroup: -inf into its maxima and its dense sample slots (what the exchange
                // stores when no wave holds a tile: gmax_round below), and it ends before the hidden tile is copied
                const float4 ninf = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff());
                for (int sl = tid; sl < 256 * RB; sl += NW * 64) {
                    const int rb = sl >> 8, s2 = sl & 255;
                    const int r2 = rg * R_TILE + rb * 32 + (s2 & 31);
                    if (r2 < p.B)
                        *reinterpret_cast<float4*>(p.gmax + (size_t)r2 * p.ld_gmax + (size_t)bir * 32 + (s2 >> 5) * 4) = ninf;
                }
                for (int t2 = tid; t2 < NW * 64 * RB && p.out; t2 += NW * 64) {
                    const int rb = t2 / (NW * 64), t3 = t2 % (NW * 64);
                    const int w = t3 >> 6, jj = (t3 & 63) >> 1, half = t3 & 1;
                    const int item_w = w * p.nb_rg + bir;
                    const int r2 = rg * R_TILE + rb * 32 + jj;
                    if (item_w < p.ts.n_items && r2 < p.B) {
                        float* orow = p.out + (size_t)r2 * p.ld + (size_t)item_w * 32 + half * 16;
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) *reinterpret_cast<float4*>(orow + 4 * q4) = ninf;
                    }
                }
                return;
            }
            // wave-tiles decoded, into the workgroup's OWN word: a plain store (512 atomics on one address, one per live workgroup
            // of a model that skips nothing, are a queue the launch cannot end before)
            if (tid == 0) p.sk.stat[blockIdx.x] = cnt_was + (unsigned long long)n_live;
        }
    }
    // ---- hidden tile of this row group -> LDS, once ------------------------------------------
    {
        // 8 independent 16 B loads in flight per thread (a load->wait->ds_write chain per element
        // costs one L2 round trip each: ~25k cycles for the 128 KiB tile, measured with SQ_WAIT_ANY)
        const float4* src = p.hp + (HALF ? (size_t)(rg >> 1) * (2 * n_h4) : (size_t)rg * n_h4);
        // HALF: the image is [g][2 RB row blocks][64]; this workgroup's RB blocks of every g
        auto sidx = [&](int i) -> int {
            return HALF ? (i / (RB * 64)) * (2 * RB * 64) + (rg & 1) * (RB * 64) + (i % (RB * 64)) : i;
        };
        constexpr int NT = NW * 64;
        int i = tid;
        for (; i + 7 * NT < n_h4; i += 8 * NT) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[sidx(i + u * NT)];
#pragma unroll
            for (int u = 0; u < 8; ++u) lds4[i + u * NT] = v[u];
        }
        for (; i < n_h4; i += NT) lds4[i] = src[sidx(i)];
    }
    int* lcnt = reinterpret_cast<int*>(lds4 + n_h4);
    float* ltau = reinterpret_cast<float*>(lcnt + R_TILE);
    if (EPI == EPI_FILTER) {
        for (int i = tid; i < R_TILE; i += NW * 64) {
            lcnt[i] = 0;
            ltau[i] = rg * R_TILE + i < p.B ? p.tau[rg * R_TILE + i] : __builtin_inff();
        }
    }

    float loss_acc = 0.0f;
    float row_acc[RB];            // EPI_ROWLOSS: the negatives' sum of row (rb, j) over this lane's column quads of all the wave's tiles
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) row_acc[rb] = 0.0f;
    // W stream: the wave's tiles back to back; the register ring always holds the next 4 groups
    // of that stream, so the prefetch runs across tile boundaries (and under the epilogue).
    float4 wb0, wb1, wb2, wb3;
    float4 bA[RB], bB[RB];
    // bf16: one 16-byte load = the A operand of ONE MFMA (K = 16); the ring holds a whole tile
    // (16 steps at hidden = 256): the next tile streams in while this one is multiplied
    constexpr int QR = 16;
    uint4 wq[QR];
    uint4 cb[2][RB];              // hidden fragments: in use / next step
    uint4 bfrag = make_uint4(0u, 0u, 0u, 0u);                     // bias fragment of the wave's next tile
    const uint4 ones = bf16_ones_fragment(hi);
    const uint4* ldsq = reinterpret_cast<const uint4*>(lds4);
    int t_cur = __builtin_amdgcn_readfirstlane(tv_cur), t_nxt = __builtin_amdgcn_readfirstlane(tv_nxt);
    // the ring's first loads: unconditional (a wave without a tile reads the first listed tile and never uses it)
    {
        const float4* w0 = p.Wp + (size_t)t_cur * G * 64 + lane;
        if (DT == DT_F32) {
            wb0 = w0[0]; wb1 = w0[64]; wb2 = w0[128]; wb3 = w0[192];
        } else {
            bfrag = p.bias16[(size_t)t_cur * 64 + lane];
            const uint4* q0 = reinterpret_cast<const uint4*>(w0);
#pragma unroll
            for (int u = 0; u < QR; ++u) wq[u] = q0[(size_t)(u < G ? u : G - 1) * 64];
        }
    }
    __syncthreads();

    float tau_r[RB];
    if (EPI == EPI_FILTER) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) tau_r[rb] = ltau[rb * 32 + j];
    }
    if (DT == DT_F32) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) bA[rb] = lds4[rb * 64 + lane];
    } else {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) cb[0][rb] = ldsq[rb * 64 + lane];
    }

    // EPI_GMAX: one exchange per round of tiles, joined by EVERY wave of the workgroup (a wave without a tile in
    // the round contributes -inf): row block by row block through 16 B x 256 slots per wave behind the hidden
    // tile -- wave w writes its masked logits as float4 (slot = (quad, half, playlist): conflict-free), thread
    // (quad, half, playlist) takes the maximum over the waves and stores 4 maxima of its playlist's row
    auto gmax_round = [&](bool has, int round, const f32x16* accv, const float4* bqv, int tcol0v) {
        // HALF: the slots ARE the hidden tile's LDS (one round only: every wave is past its k loop at the first barrier)
        float4* xl = HALF ? lds4 : reinterpret_cast<float4*>(lcnt + R_TILE);
        if (p.gmax_per_wave) {
            // a sample too small for groups of NW (a vocabulary shard: 61 tiles for 64 wave slots): every element is
            // its own "group" -- the wave stores its masked logits, -inf where it had no tile this round
            const size_t slot = ((size_t)round * p.nb_rg * NW + (size_t)wave * p.nb_rg + bir) * 32;
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B) continue;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    float4 v = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff());
                    if (has) {
                        const int lc = tcol0v + 8 * qd;
                        float z[4] = {accv[rb][4 * qd + 0] + bqv[qd].x, accv[rb][4 * qd + 1] + bqv[qd].y,
                                      accv[rb][4 * qd + 2] + bqv[qd].z, accv[rb][4 * qd + 3] + bqv[qd].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (p.col_lo + lc + e >= p.mask_from_col || lc + e >= p.ncols) z[e] = -__builtin_inff();
                        v = make_float4(z[0], z[1], z[2], z[3]);
                    }
                    *reinterpret_cast<float4*>(p.gmax + (size_t)row * p.ld_gmax + slot + 4 * hi + 8 * qd) = v;
                }
            }
            return;
        }
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            __syncthreads();                                     // the previous row block's slots were read
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                float4 v = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff());
                if (has) {
                    const int lc = tcol0v + 8 * qd;
                    float z[4] = {accv[rb][4 * qd + 0] + bqv[qd].x, accv[rb][4 * qd + 1] + bqv[qd].y,
                                  accv[rb][4 * qd + 2] + bqv[qd].z, accv[rb][4 * qd + 3] + bqv[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (p.col_lo + lc + e >= p.mask_from_col || lc + e >= p.ncols) z[e] = -__builtin_inff();
                    v = make_float4(z[0], z[1], z[2], z[3]);
                }
                xl[wave * 256 + (qd * 2 + hi) * 32 + j] = v;
            }
            __syncthreads();
            for (int sl = tid; sl < 256; sl += NW * 64) {
                float4 m = xl[sl];
#pragma unroll
                for (int w = 1; w < NW; ++w) {
                    const float4 o = xl[w * 256 + sl];
                    m = make_float4(fmaxf(m.x, o.x), fmaxf(m.y, o.y), fmaxf(m.z, o.z), fmaxf(m.w, o.w));
                }
                const int row = rg * R_TILE + rb * 32 + (sl & 31);
                if (row < p.B)
                    *reinterpret_cast<float4*>(p.gmax + (size_t)row * p.ld_gmax +
                                               ((size_t)round * p.nb_rg + bir) * 32 + (sl >> 5) * 4) = m;
            }
            // the dense sample rows of this row block, from the same slots: thread (tile w, playlist jj, half) writes 64
            // contiguous bytes, a wave 32 whole 128-byte rows -- the accumulator layout itself would store 16-byte
            // pieces of 64 different rows per instruction (4.9 us of the launch, measured with stage stamps)
            for (int t2 = tid; t2 < NW * 64 && p.out; t2 += NW * 64) {   // p.out == null: the launch leaves maxima only
                const int w = t2 >> 6, jj = (t2 & 63) >> 1, half = t2 & 1;
                const int item_w = w * p.nb_rg + bir + round * (p.nb_rg * NW);
                const int row = rg * R_TILE + rb * 32 + jj;
                // HALF with a decoded-tile table: a skipped wave's 32 slots are not stored (sk_live[] sits behind the hidden tile,
                // i.e. behind these exchange slots, which end at 256 NW <= n_h4 float4: still what the vote left there)
                bool stored = true;
                if constexpr (HALF)
                    if (p.sk.tab) stored = reinterpret_cast<const int*>(lds4 + n_h4)[w] != 0;
                if (item_w < p.ts.n_items && row < p.B && stored) {
                    float* orow = p.out + (size_t)row * p.ld + (size_t)item_w * 32 + half * 16;
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4)
                        *reinterpret_cast<float4*>(orow + 4 * q4) = xl[w * 256 + (half * 4 + q4) * 32 + jj];
                }
            }
        }
    };

    // (a wave whose tile is skipped walks nothing and joins the exchange below with -inf, as a wave without a tile does)
    for (int item = skip_w ? p.ts.n_items : item0; item < p.ts.n_items; item += n_ws) {
        const int t = t_cur;
        const float4* wp = p.Wp + (size_t)t * G * 64 + lane;
        // next tile of this wave (or this one again at the end: in-bounds, values unused)
        const int item_n = item + n_ws < p.ts.n_items ? item + n_ws : item;
        const float4* wn = p.Wp + (size_t)t_nxt * G * 64 + lane;
        const int item_nn = item_n + n_ws < p.ts.n_items ? item_n + n_ws : item_n;
        const int t_nn_v = tile_of_item(p.ts, item_nn);            // consumed at the end of this tile

        // bias of the tile's 32 columns, fetched now so the epilogue never waits on memory:
        // lane holds columns v_local(reg) = (reg & 3) + 8 * (reg >> 2) + 4 * hi, reg = 0..15
        const float* bp = p.bias + (size_t)t * 32 + 4 * hi;
        float4 bq[4];
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
            bq[qd] = DT == DT_BF16 ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(bp + 8 * qd);

        // title mix: the other scorer's term of this tile's elements, requested now, consumed in the epilogue
        float mixv[(EPI == EPI_GMAX || EPI == EPI_FILTER) ? RB : 1][16];
        if ((EPI == EPI_GMAX || EPI == EPI_FILTER) && p.mixT) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int lc = t * 32 + 4 * hi + (e & 3) + 8 * (e >> 2);
                    mixv[rb][e] = (row < p.B && lc < p.ncols && p.col_lo + lc < p.mix_ncols)
                                      ? p.mixT[(size_t)(p.col_lo + lc) * p.mix_ld + row] : 0.0f;
                }
            }
        }

        // EPI_MIXROWLOSS: the DAE's term of this tile's elements (ALL columns of the image, the artists' included), requested
        // now like the mix term above
        float mlv[EPI == EPI_MIXROWLOSS ? RB : 1][16];
        if (EPI == EPI_MIXROWLOSS) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int lc = t * 32 + 4 * hi + (e & 3) + 8 * (e >> 2);
                    mlv[EPI == EPI_MIXROWLOSS ? rb : 0][e] =
                        (row < p.B && lc < p.ncols) ? p.mixT[(size_t)(p.col_lo + lc) * p.mix_ld + row] : 0.0f;
                }
            }
        }

        // EPI_TERM_ADD: what the transposed buffer holds of this tile's elements, requested now like the mix term above (a load
        // instruction reads the 32 consecutive rows of one column that the store below it writes)
        float oldv[EPI == EPI_TERM_ADD ? RB : 1][16];
        if (EPI == EPI_TERM_ADD) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int lc = t * 32 + 4 * hi + (e & 3) + 8 * (e >> 2);
                    oldv[EPI == EPI_TERM_ADD ? rb : 0][e] =
                        (row < p.B && lc < p.ncols) ? p.outT[(size_t)(p.col_lo + lc) * p.ld_outT + row] : 0.0f;
                }
            }
        }

        f32x16 acc[RB];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[rb][e] = 0.0f;
        if (DT == DT_BF16) {
            const uint4 bcur = bfrag;
            bfrag = p.bias16[(size_t)t_nxt * 64 + lane];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb)
                acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(bcur), as_bf16x8(ones), acc[rb], 0, 0, 0);
        }

// one k-group (8 k = 4 MFMA steps per accumulator): consume ring slot WB with hidden fragments
// BC, refill the slot from PF, and fetch the NEXT group's hidden fragments into BN.
#define DAE_STEP(WB, PF, BC, BN, GNEXT)                                                        \
    {                                                                                          \
        const float4 a = WB;                                                                   \
        WB = *(PF);                                                                            \
        const float4* hl = lds4 + (size_t)(GNEXT) * (RB * 64) + lane;                          \
        _Pragma("unroll") for (int rb = 0; rb < RB; ++rb) BN[rb] = hl[rb * 64];                \
        __builtin_amdgcn_sched_barrier(0); /* keep the prefetches AHEAD of this group's MFMAs */\
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

        if (DT == DT_BF16) {
            const uint4* wq_cur = reinterpret_cast<const uint4*>(wp);
            const uint4* wq_nxt = reinterpret_cast<const uint4*>(wn);
            if (GT > 0) {
                // hidden size known: fully unrolled, ring slot and fragment buffer are static
#pragma unroll
                for (int s = 0; s < (GT > 0 ? GT : 1); ++s) {
                    const uint4 a = wq[s % QR];
                    wq[s % QR] = (s + QR < GT) ? wq_cur[(size_t)(s + QR) * 64]
                                               : wq_nxt[(size_t)(s + QR - GT) * 64];
                    const int sn = (s + 1) % (GT > 0 ? GT : 1);
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) cb[(s + 1) & 1][rb] = ldsq[(size_t)(sn * RB + rb) * 64 + lane];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb)
                        acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(cb[s & 1][rb]),
                                                                          acc[rb], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
            } else {
                // generic hidden size (G even): two steps per iteration, no deep ring
                for (int s = 0; s < G; s += 2) {
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const uint4 a = wq_cur[(size_t)(s + h2) * 64];
#pragma unroll
                        for (int rb = 0; rb < RB; ++rb) {
                            const uint4 b = ldsq[(size_t)((s + h2) * RB + rb) * 64 + lane];
                            acc[rb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a), as_bf16x8(b),
                                                                              acc[rb], 0, 0, 0);
                        }
                    }
                }
            }
        } else {
        int g = 0;
#pragma unroll
        for (; g < G - 4; g += 4) {
            const float4* pf = wp + (size_t)(g + 4) * 64;
            DAE_STEP(wb0, pf,       bA, bB, g + 1)
            DAE_STEP(wb1, pf + 64,  bB, bA, g + 2)
            DAE_STEP(wb2, pf + 128, bA, bB, g + 3)
            DAE_STEP(wb3, pf + 192, bB, bA, g + 4)
        }
        // last 4 groups of the tile: refill from the next tile, wrap the hidden fragments to g = 0
        DAE_STEP(wb0, wn,       bA, bB, g + 1)
        DAE_STEP(wb1, wn + 64,  bB, bA, g + 2)
        DAE_STEP(wb2, wn + 128, bA, bB, g + 3)
        DAE_STEP(wb3, wn + 192, bB, bA, 0)
        }
#undef DAE_STEP

        // ---- epilogue -----------------------------------------------------------------------
        // lane holds, for playlist j of row block rb, the columns
        //   v_local(reg) = (reg & 3) + 8 * (reg >> 2) + 4 * hi          (reg = 0..15)
        const int tcol0 = t * 32 + 4 * hi;                // local column of reg 0 in the image

        if ((EPI == EPI_GMAX || EPI == EPI_FILTER) && p.mixT) {
            // the accumulators become the mixed scores (same operations, same order as mix_scores_kernel of the
            // unfused path: title * w_title + dae * w_playlist, no contraction); the bias is consumed here
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                const float wt = row < p.B ? p.mix_w[row] : 0.0f;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float ts = dae_sigmoidf(acc[rb][4 * qd + e] + zb[e]) * wt;
                        acc[rb][4 * qd + e] = ts + mixv[rb][4 * qd + e];
                    }
                }
            }
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) bq[qd] = make_float4(0.f, 0.f, 0.f, 0.f);
        }

        if (EPI == EPI_TERM_ADD) {
            // a further member's term joins the transposed buffer: old + sigmoid(z) * scale, two roundings, no contraction
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B) continue;
                const float sc = p.row_scale[row];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int lc = tcol0 + 8 * qd + e;
                        const float term = dae_sigmoidf(acc[rb][4 * qd + e] + zb[e]) * sc;
                        if (lc < p.ncols)
                            p.outT[(size_t)(p.col_lo + lc) * p.ld_outT + row] = oldv[EPI == EPI_TERM_ADD ? rb : 0][4 * qd + e] + term;
                    }
                }
            }
        } else if (EPI == EPI_DENSE && p.outT) {
            // DAE term of the title mix, transposed: a store instruction writes 32 consecutive rows of one column
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B) continue;
                const float sc = p.row_scale[row];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int lc = tcol0 + 8 * qd + e;
                        if (lc < p.ncols)
                            p.outT[(size_t)(p.col_lo + lc) * p.ld_outT + row] = dae_sigmoidf(acc[rb][4 * qd + e] + zb[e]) * sc;
                    }
                }
            }
        } else if (EPI == EPI_DENSE || (EPI == EPI_GMAX && p.gmax_per_wave)) {
            // (EPI_GMAX with the cross-wave exchange stores its dense rows from LDS, inside gmax_round)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B || (EPI == EPI_GMAX && !p.out)) continue;      // maxima only (bf16 whole-launch filter)
                float* orow = p.out + (size_t)row * p.ld + (size_t)item * 32 + 4 * hi;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int lc = tcol0 + 8 * qd;        // first of 4 consecutive local columns
                    float z[4] = {acc[rb][4 * qd + 0] + bq[qd].x, acc[rb][4 * qd + 1] + bq[qd].y,
                                  acc[rb][4 * qd + 2] + bq[qd].z, acc[rb][4 * qd + 3] + bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (p.apply_sigmoid) z[e] = dae_sigmoidf(z[e]);
                        if (p.col_lo + lc + e >= p.mask_from_col || lc + e >= p.ncols)
                            z[e] = -__builtin_inff();
                    }
                    if (lc + 3 < p.ncols || p.fill_pad) {
                        if (p.vec_ok) {
                            *reinterpret_cast<float4*>(orow + 8 * qd) =
                                make_float4(z[0], z[1], z[2], z[3]);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) orow[8 * qd + e] = z[e];
                        }
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (lc + e < p.ncols) orow[8 * qd + e] = z[e];
                    }
                }
            }
            if (EPI == EPI_GMAX) gmax_round(true, (item - item0) / n_ws, acc, bq, tcol0);
        } else if (EPI == EPI_GMAX) {
            gmax_round(true, (item - item0) / n_ws, acc, bq, tcol0);      // maxima AND the dense rows, through LDS
        } else if (EPI == EPI_LOSS) {
            // Every element is treated as a NEGATIVE (target 0) here; the few positives of the batch (~100
            // of 170 000 columns per row) are redone from their own dot products by loss_fixup_kernel
            // (train.hip), so no dense target matrix exists.  dL/dz (mean over n_batch folded in) is
            // written transposed, the layout both backward GEMMs read.
            // The head: decode_common.h (y = 0).
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B) continue;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int lc = tcol0 + 8 * qd;
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (lc + e < p.ncols) {
                            const float pr = dae_train_sigmoid(acc[rb][4 * qd + e] + zb[e]);
                            loss_acc -= dae_loss_neg_term(pr);
                            const float dzv = dae_loss_neg_dz(pr, p.inv_nb);
                            if (DT == DT_BF16 && p.dz16)
                                reinterpret_cast<unsigned short*>(p.dzT)[(size_t)(lc + e) * p.ldT + row] =
                                    (unsigned short)dae_bf16_rne(dzv);
                            else
                                p.dzT[(size_t)(lc + e) * p.ldT + row] = dzv;
                        }
                    }
                }
            }
        } else if (EPI == EPI_ROWLOSS) {
            // The loss without a step: what EPI_LOSS does for the loss (every element a negative, the head of decode_common.h)
            // and nothing else -- no dL/dz, no logits; the sums stay per row.  The positives: loss_rows.hip.
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B) continue;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int lc = tcol0 + 8 * qd;
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (lc + e < p.ncols) {
                            const float pr = dae_train_sigmoid(acc[rb][4 * qd + e] + zb[e]);
                            row_acc[rb] -= dae_loss_neg_term(pr);
                        }
                    }
                }
            }
        } else if (EPI == EPI_MIXROWLOSS) {
            // The mixed loss without a step: the title step's operations in its order on every element, taken as a negative
            // (title.hip title_loss_kernel, dae_loss_head_mixed with y = 0; no contraction), summed per row.  The targets:
            // mix_loss.hip.
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int row = rg * R_TILE + rb * 32 + j;
                if (row >= p.B) continue;
                const float wt = p.mix_w[row];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int lc = tcol0 + 8 * qd;
                    const float zb[4] = {bq[qd].x, bq[qd].y, bq[qd].z, bq[qd].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (lc + e < p.ncols) {
                            const float st = dae_title_step_sigmoid(acc[rb][4 * qd + e] + zb[e]);
                            const float yp = st * wt + mlv[EPI == EPI_MIXROWLOSS ? rb : 0][4 * qd + e];
                            row_acc[rb] -= dae_loss_neg_term_mixed(yp);
                        }
                    }
                }
            }
        } else if ((t * 32 < p.ncols) && (p.col_lo + t * 32 < p.n_valid_col)) {
            // filter: tiles without a rankable column (the artist columns) need no epilogue at all; in
            // the others the common case -- this launch walks the LOW-bias tiles -- is "no value of
            // the row block reaches tau": 16 adds, a max-reduction and one compare.  Masks, the LDS
            // atomic for the list slots and the stores only where a lane really passes.
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const float tv = tau_r[rb];
                float z[16];
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    z[4 * qd + 0] = acc[rb][4 * qd + 0] + bq[qd].x;
                    z[4 * qd + 1] = acc[rb][4 * qd + 1] + bq[qd].y;
                    z[4 * qd + 2] = acc[rb][4 * qd + 2] + bq[qd].z;
                    z[4 * qd + 3] = acc[rb][4 * qd + 3] + bq[qd].w;
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
                        const int row = rg * R_TILE + rloc;
                        int base = atomicAdd(&lcnt[rloc], __popc(m));
                        uint2* dst = p.cand + ((size_t)bir * p.Bpad + row) * (size_t)p.cap;
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
        }
        t_cur = t_nxt;
        t_nxt = __builtin_amdgcn_readfirstlane(t_nn_v);
    }

    if (EPI == EPI_GMAX) {
        // rounds this wave had no tile for: still joins the exchange (block-uniform trip count in total)
        const int rounds = (p.ts.n_items + n_ws - 1) / n_ws;
        const int mine = (item0 < p.ts.n_items && !skip_w) ? (p.ts.n_items - item0 + n_ws - 1) / n_ws : 0;
        f32x16 dummy_acc[RB];
        float4 dummy_b[4];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int e = 0; e < 16; ++e) dummy_acc[rb][e] = 0.0f;
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) dummy_b[qd] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int r = mine; r < rounds; ++r) gmax_round(false, r, dummy_acc, dummy_b, 0);
    }
    if (EPI == EPI_FILTER) {
        __syncthreads();
        if (tid < R_TILE) p.cand_cnt[(size_t)bir * p.Bpad + rg * R_TILE + tid] = lcnt[tid];
    }
    if (EPI == EPI_ROWLOSS || EPI == EPI_MIXROWLOSS) {
        // Fixed order, no atomics: the two half-waves hold the same 32 rows and different column quads -> one shuffle; the
        // waves meet in LDS ([NW][R_TILE] floats behind the hidden tile, which stays untouched) and are added in wave order;
        // one float per row of the group goes to the workgroup's place in the partial table.  A wave without a tile adds +0.
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) row_acc[rb] += __shfl_xor(row_acc[rb], 32);
        float* wrow = reinterpret_cast<float*>(lcnt);
        if (hi == 0) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) wrow[wave * R_TILE + rb * 32 + j] = row_acc[rb];
        }
        __syncthreads();
        for (int i = tid; i < R_TILE; i += NW * 64) {
            float s = wrow[i];
#pragma unroll
            for (int w = 1; w < NW; ++w) s += wrow[w * R_TILE + i];
            p.loss_part[((size_t)rg * p.nb_rg + bir) * R_TILE + i] = s;
        }
    }
    if (EPI == EPI_LOSS) {
        // deterministic: lanes -> wave (shuffle tree), waves -> block (fixed order), one slot/block
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) loss_acc += __shfl_xor(loss_acc, d);
        float* wsum = reinterpret_cast<float*>(lcnt);
        __syncthreads();
        if (lane == 0) wsum[wave] = loss_acc;
        __syncthreads();
        if (tid == 0) {
            float s = 0.0f;
            for (int w = 0; w < NW; ++w) s += wsum[w];
            p.loss_part[blockIdx.x] = s * p.inv_nb;          // reduce_mean over the fixed n_batch
        }
    }
}

template <int RB, int EPI, int GT, int NW, int DT>
int launch_decode(dae_ctx* ctx, const dae_rowgeom& g, const dae_decp& p)
{
    const size_t lds = (size_t)RB * 64 * p.G * sizeof(float4) + (size_t)RB * 32 * sizeof(int) +
                       (EPI == EPI_GMAX ? (size_t)NW * 256 * sizeof(float4) : 0) +
                       (EPI == EPI_FILTER ? (size_t)RB * 32 * sizeof(float) : 0) +
                       ((EPI == EPI_ROWLOSS || EPI == EPI_MIXROWLOSS) ? (size_t)NW * RB * 32 * sizeof(float) : 0);
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_f32_kernel<RB, EPI, GT, NW, DT>, 160 * 1024));
    if (ctx->prof_armed) {
        char name[96];
        snprintf(name, sizeof(name), "decode_f32_kernel<%d, %d, %d, %d, %d>", RB, EPI, GT, NW, DT);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        dae_take_profile_events(ctx, name, e0, e1);
        hipExtLaunchKernelGGL((decode_f32_kernel<RB, EPI, GT, NW, DT>), dim3(g.grid), dim3(NW * 64), lds,
                              ctx->stream, e0, e1, 0, p);
    } else {
        hipLaunchKernelGGL((decode_f32_kernel<RB, EPI, GT, NW, DT>), dim3(g.grid), dim3(NW * 64), lds,
                           ctx->stream, p);
    }
    DAE_CHECK_LAUNCH(ctx, "decode_f32_kernel");
    return DAE_OK;
}

template <int EPI>
int launch_decode_rb(dae_ctx* ctx, const dae_rowgeom& g, const dae_decp& p)
{
    // the shipped configs all use hidden = 256 (config.ini:12): G = 32 gets the unrolled body (not the loss epilogue: hidden
    // 256 in 128-row groups trains through the row-major K5, dae_launch_decode_loss_rowmajor)
    if constexpr (EPI != EPI_LOSS)
        if (g.R_TILE == 128 && p.G == 32) return launch_decode<4, EPI, 32, 4, DT_F32>(ctx, g, p);
    if (g.waves != 4) return dae_fail(ctx, DAE_ERR_ARG, "bad wave count %d", g.waves);
    switch (g.R_TILE) {
        case 128: return launch_decode<4, EPI, 0, 4, DT_F32>(ctx, g, p);
        case 64:  return launch_decode<2, EPI, 0, 4, DT_F32>(ctx, g, p);
        case 32:  return launch_decode<1, EPI, 0, 4, DT_F32>(ctx, g, p);
    }
    return dae_fail(ctx, DAE_ERR_ARG, "bad R_TILE %d", g.R_TILE);
}

template <int EPI>
int launch_decode_rb_bf16(dae_ctx* ctx, const dae_rowgeom& g, const dae_decp& p)
{
    // hidden = 256 -> 16 steps of K = 16: unrolled body with the 8-deep register ring
    // two waves per SIMD here: with 16x faster MFMAs the VALU epilogue of a tile is comparable to
    // its matrix time, and the second wave's MFMAs cover it
    if (g.waves != 4) return dae_fail(ctx, DAE_ERR_ARG, "bad wave count %d", g.waves);
    if constexpr (EPI != EPI_LOSS)                            // (the loss epilogue: as in launch_decode_rb)
        if (g.R_TILE == 128 && p.G == 16) return launch_decode<4, EPI, 16, 4, DT_BF16>(ctx, g, p);
    switch (g.R_TILE) {
        case 128: return launch_decode<4, EPI, 0, 4, DT_BF16>(ctx, g, p);
        case 64:  return launch_decode<2, EPI, 0, 4, DT_BF16>(ctx, g, p);
        case 32:  return launch_decode<1, EPI, 0, 4, DT_BF16>(ctx, g, p);
    }
    return dae_fail(ctx, DAE_ERR_ARG, "bad R_TILE %d", g.R_TILE);
}

}  // namespace

int dae_launch_decode_generic(dae_ctx* ctx, int epi, int dt, const dae_rowgeom& g, const dae_decp& p)
{
    switch (epi) {
        case EPI_DENSE:  return dt == DT_F32 ? launch_decode_rb<EPI_DENSE>(ctx, g, p) : launch_decode_rb_bf16<EPI_DENSE>(ctx, g, p);
        case EPI_FILTER: return dt == DT_F32 ? launch_decode_rb<EPI_FILTER>(ctx, g, p) : launch_decode_rb_bf16<EPI_FILTER>(ctx, g, p);
        case EPI_LOSS:   return dt == DT_F32 ? launch_decode_rb<EPI_LOSS>(ctx, g, p) : launch_decode_rb_bf16<EPI_LOSS>(ctx, g, p);
        case EPI_GMAX:   return dt == DT_F32 ? launch_decode_rb<EPI_GMAX>(ctx, g, p) : launch_decode_rb_bf16<EPI_GMAX>(ctx, g, p);
        case EPI_TERM_ADD: return dt == DT_F32 ? launch_decode_rb<EPI_TERM_ADD>(ctx, g, p) : launch_decode_rb_bf16<EPI_TERM_ADD>(ctx, g, p);
        case EPI_ROWLOSS: return dt == DT_F32 ? launch_decode_rb<EPI_ROWLOSS>(ctx, g, p) : launch_decode_rb_bf16<EPI_ROWLOSS>(ctx, g, p);
        case EPI_MIXROWLOSS:
            // the fp32 image only, at the three row-group heights the geometry can choose (no unrolled hidden-256 body: a title
            // image's K is ld_feat)
            if (dt != DT_F32 || g.waves != 4) break;
            switch (g.R_TILE) {
                case 128: return launch_decode<4, EPI_MIXROWLOSS, 0, 4, DT_F32>(ctx, g, p);
                case 64:  return launch_decode<2, EPI_MIXROWLOSS, 0, 4, DT_F32>(ctx, g, p);
                case 32:  return launch_decode<1, EPI_MIXROWLOSS, 0, 4, DT_F32>(ctx, g, p);
            }
            break;
    }
    return dae_fail(ctx, DAE_ERR_ARG, "bad epilogue %d", epi);
}

// one round of tiles (the threshold sample at batch <= 256; fp32, hidden 256, 128-row groups): half row groups, two
// workgroups per CU (decode_f32_kernel's HALF)
int dae_launch_decode_gmax_half(dae_ctx* ctx, const dae_rowgeom& g, const dae_decp& p_)
{
    dae_decp p = p_;
    p.n_rg = 2 * g.n_rg;
    const size_t lds = (size_t)2 * 64 * p.G * sizeof(float4) + (size_t)2 * 32 * sizeof(int);
    DAE_HIP_CHECK(ctx, dae_lds_limit_once(ctx, &decode_f32_kernel<2, EPI_GMAX, 32, 4, DT_F32, 1>, 160 * 1024));
    hipLaunchKernelGGL((decode_f32_kernel<2, EPI_GMAX, 32, 4, DT_F32, 1>), dim3(2 * g.grid), dim3(256), lds, ctx->stream, p);
    DAE_CHECK_LAUNCH(ctx, "decode_f32_kernel (half row groups)");
    return DAE_OK;
}
