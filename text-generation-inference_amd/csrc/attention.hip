// Paged causal attention for prefill and decode on gfx950 (MFMA 16x16x32, wave64).
// Replaces flash_attn_2_cuda.varlen_fwd as called from utils/flash_attn.py:43-78 for both call shapes of
// custom_modeling/flash_llama_modeling.py:271-295 (prefill: causal over the fresh k/v; decode: q-len 1
// over all cached slots) — here both read the paged cache that tgis_rope_kv_write has just filled.
//
// One workgroup = 4 waves handles one (sequence, kv head, 16-column q tile, key split).  The 16 MFMA
// columns are (q token, q head of the GQA group) pairs, so one K/V stream serves the whole group.
// Groups wider than 16 heads (multi-query attention: 48 q heads on one kv head) take CH 16-head chunks per block:
// the wave keeps CH sets of Q fragments, softmax statistics and O accumulators and applies every K/V fragment it
// loads to all of them, so K/V still stream from HBM once (one block per chunk re-read them once per chunk — the
// chunks land on different XCDs, i.e. different L2s: 47 us per Starcoder-15B launch where the bytes need 11).
// Per 32-token page and wave:
//   S^T[tok][col] = K[tok][:] . Q[col][:]      A = K fragment (1 KiB contiguous loads), B = Q^T
//   online softmax per column: the column's statistics live in lane (l & 15) of every 16-lane row
//   O^T[d][col]  += V^T[d][tok] . P^T[tok][col] A = V^T fragment (1 KiB contiguous loads), B = P^T
// S^T's accumulator layout IS the B-operand layout of the second MFMA and O^T's column index is the
// same lane, so the only cross-lane traffic per page is the 2-step row-max exchange.
//
// Which launch a shape takes (form, waves and chunks per block, PIPE, XCD remap, grid, merge, key splits, workspace) is decided
// in attention_plan.h; this file is the kernels, then the launcher of a plan, then the entry points.
#include <stdio.h>
#include <algorithm>
#include <type_traits>
#include "common.h"
#include "dispatch.h"
#include "attention_args.h"
#include "attention_counters.h"
#include "attention_plan.h"
#include "kv_layout.h"

// tools/floor/attn_unit.hip compiles this unit with per-wave s_memtime stamps (ATTN_STAMP*); the library does not.
#ifndef ATTN_STAMP
#define ATTN_STAMP_DECL
#define ATTN_STAMP(i)
#define ATTN_STAMP_FLUSH
#endif
#ifndef ATTN_BLOCK_REMAP  // tools/floor/attn_unit.hip: which (kv head, sequence) a block id takes, to probe XCD <-> address affinity
#define ATTN_BLOCK_REMAP(by, bz)
#endif

namespace {


// NW = waves per workgroup (the key range of a block is dealt page-by-page to its waves)
// PIPE: two pages of K/V loads in flight per wave (twice the fragment registers)
// KV: the pool's element, T (16-bit cache) or uint8_t (e4m3 codes, kv_layout.h): a one-byte fragment is an 8-byte nontemporal
// load widened to T in registers; the MFMAs, Q and P stay in T
// TREE (tgis_attn_paged_tree: one-chunk blocks of 4 waves, no PIPE): the argument block carries q_mask, one 64-bit word per q
// row.  Keys below ctx - q_len are visible to every row; the key of the sequence's q row j (cache position ctx - q_len + j) is
// visible to q row i when bit j of q_mask[i] is set AND j <= i.  The fully visible pages then end at ctx - q_len and every page
// from there on takes the masked body, which tests one more bit per score.  The mask changes scores only: the pages a block
// walks and every address it loads from are those of the TREE = false kernel for the same ctx_lens and cu_seqlens_q (a page
// that is full but masked goes through load_page_part with nv = 32, which requests what load_page requests).
// WINDOW (tgis_attn_paged_window at one q token per sequence: one-chunk blocks of 4 waves, no PIPE): the argument block carries
// `window`, W keys per q row.  The block's pages begin at the first page its first q row sees (attention_plan.h
// attn_window_first_key) instead of page 0: pages below it are not loaded and their table entries not read, and the key splits
// divide that range.  The first of them, when the window starts inside it, takes the masked body with the lower bound — in
// wave 0 of split 0, in the loop of the partly visible pages — as the page that is being filled takes it with the upper one;
// when both are one page, that page's pass tests both.
//
// Kernel argument preload (csrc/gptq_wide_body.h): the leading scalar parameters — 14 dwords, all the user SGPRs a wave has —
// arrive in SGPRs at wave launch and overrule the same fields of the argument block behind them.  They are what the FIRST
// scalar requests are formed from: which (sequence, split, kv head) this block is (NS, Hkv, HCB, xcd_remap) and where its
// lengths and its block table lie (cu_q, ctx_lens, bt, max_pages); kpool fills the last pair.  Everything else is read from
// the block and arrives with the lengths, one round trip earlier than it did behind a fetch of the block.  Launched through
// launch_attn_kernel only.
template <bool TREE, bool WINDOW>
using AttnArgsOf = std::conditional_t<TREE, AttnTreeArgs, std::conditional_t<WINDOW, AttnWindowArgs, AttnArgs>>;

template <typename T, typename KV, int D, int NW, int CH, bool PIPE, bool TREE = false, bool WINDOW = false>
__global__ __launch_bounds__(64 * NW) void attn_paged_kernel(const int32_t* bt, const int32_t* cu_q, const int32_t* ctx_lens,
                                                             const void* kpool, int64_t max_pages, int NS, int Hkv, int HCB,
                                                             int xcd_remap, AttnArgsOf<TREE, WINDOW> rest) {
    static_assert(!TREE || (CH == 1 && !PIPE), "the tree variant exists for one-chunk blocks without the page pipeline");
    static_assert(!WINDOW || (CH == 1 && !PIPE && !TREE), "the window variant: one-chunk blocks, no page pipeline, no tree");
    using V8 = typename VecT<T>::x8;
    constexpr int KS = D / 32;  // k-steps of the QK^T MFMA
    constexpr int NB = D / 16;  // 16-row blocks of O^T
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    AttnArgsOf<TREE, WINDOW> a = rest;
    a.bt = bt; a.cu_q = cu_q; a.ctx_lens = ctx_lens; a.kpool = kpool; a.max_pages = max_pages;
    a.NS = NS; a.Hkv = Hkv; a.HCB = HCB; a.xcd_remap = xcd_remap;
    ATTN_STAMP_DECL
    ATTN_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the block-table reads become scalar loads
    const int col = lane & 15, c = lane >> 4;
    const int qt = blockIdx.x;
    int by = blockIdx.y, bz = blockIdx.z;
    ATTN_BLOCK_REMAP(by, bz);
    if (a.xcd_remap) {
        // Several blocks per (sequence, split, kv head) group — one per set of 16-head chunks — read the SAME K/V pages.
        // Workgroups go to the 8 XCDs round-robin by linear id, each XCD with its own L2: in grid order the chunk blocks of a
        // group land on different XCDs and every one of them pulls the pages from HBM.  Remapped, XCD x runs the blocks
        // x, x + 8, x + 16, ... and consecutive ones of them are the chunk blocks of one group: the pages cross the fabric
        // once and the other chunk blocks hit that XCD's L2 (MQA 48:1 as three one-chunk blocks, B = 32, ctx 4096:
        // 44 -> 33 us at 4 splits, profiles/r04_mqa_xcd.log).  gridDim.x == 1 and the number of groups is a multiple
        // of 8 — the launcher checks.
        const int L = blockIdx.y + gridDim.y * blockIdx.z;
        const int x = L & 7, i = L >> 3;
        const int grp = x + 8 * (i / a.HCB), cb = i % a.HCB;
        bz = grp / a.Hkv;
        by = (grp % a.Hkv) * a.HCB + cb;
    }
    const int hk = by / a.HCB, hc0 = (by % a.HCB) * CH;  // first 16-head chunk of this block
    const int b = bz / a.NS, split = bz % a.NS;

    // Unsplit launches (NS == 1: every block starts at page 0): this wave's first block-table entry does not depend on the
    // sequence's length, so it is requested together with the lengths instead of behind them — one dependent scalar round trip
    // less in front of the first K / V load (inside a decode step those lines are not in this XCD's L2: the GEMMs of the layer
    // have streamed ~100 MB through it since the last attention launch; profiles/r06_attn_cold.log).
    const int32_t* btrow = a.bt + (int64_t)b * a.max_pages;
    // (WINDOW: a block starts at its first visible page, which the lengths decide)
    const int pg_spec = (!WINDOW && a.NS == 1 && w < a.max_pages) ? btrow[w] : 0;
    const int q0 = a.cu_q[b], q_len = a.cu_q[b + 1] - q0;
    {   // the requests above are formed from preloaded arguments alone.  Every cache line of the argument block the decode path
        // reads is asked for with them (one scalar round trip instead of one per group of fields: tools/floor/wide.hip `pre`)
        const int64_t l0 = a.ld_q;
        const int l1 = a.TQ;
        const void* l2 = a.counters;
        asm volatile("" ::"s"(l0), "s"(l1), "s"(l2));
    }
    const int t0 = qt * a.TQ;
    if (t0 >= q_len) return;
    const int ctx = a.ctx_lens[b];
    const int tq = col >> a.Gp_shift, g = col & (a.Gp - 1);
    bool col_valid[CH];
    int kmax[CH];  // this column may attend to key positions < kmax
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        col_valid[ch] = (g < a.Gc) && ((hc0 + ch) * 16 + g < a.G) && (t0 + tq < q_len);
        kmax[ch] = col_valid[ch] ? (ctx - q_len + t0 + tq + 1) : 0;
    }
    // TREE: this column's mask word; bit j is the key at cache position ctx - q_len + j
    uint64_t qmask = 0;
    if constexpr (TREE) qmask = col_valid[0] ? a.q_mask[q0 + t0 + tq] : 0;
    const int kend = ctx - q_len + min(q_len, t0 + a.TQ);  // keys needed by any column of the tile
    const int pages = (kend + 31) >> 5;
    // WINDOW: keys below klo are hidden from the tile's first q row, so from every row of the tile; this column's bound is kmin
    int klo = 0, kmin = 0;
    if constexpr (WINDOW) {
        klo = attn_window_first_key(ctx, q_len, t0, a.window);
        kmin = attn_window_first_key(ctx, q_len, t0 + tq, a.window);
    }
    const int pfirst = klo >> 5;  // (0 without a window)
    const int pps = (pages - pfirst + a.NS - 1) / a.NS;
    const int pbeg = pfirst + split * pps, pend = min(pages, pbeg + pps);
    ATTN_STAMP(1);  // (the sequence's lengths are in: the stamp macro waits for scalar loads)
    // The first fully visible page's table entry is asked for HERE — as soon as the lengths are in, in front of the q loads and
    // of the partly visible pages: behind them it was a scalar round trip with nothing of this wave in flight (round 5 timeline,
    // profiles/r05_attn_timeline.log: multi-chunk blocks had their first entry 4.8 k ticks after entry, 3.5 k after the lengths).
    const int pg_first = (!WINDOW && a.NS == 1) ? pg_spec : ((pbeg + w < pend) ? btrow[pbeg + w] : 0);

    // Q^T fragments (B operand): lane supplies Q[col][ks*32 + c*8 .. +8]
    V8 qf[CH][KS];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        const int head = hk * a.G + (hc0 + ch) * 16 + g;
        const T* qp = reinterpret_cast<const T*>(a.q) + (int64_t)(q0 + t0 + tq) * a.ld_q + (int64_t)head * D + c * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (col_valid[ch]) {
                qf[ch][ks] = ld16<V8>(qp + ks * 32);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) qf[ch][ks][e] = (T)0.f;
            }
        }
    }
    // (Rotary embedding + cache write of the new token in this prologue was built in round 2, bit-exact, and measured slower
    // than the launch in front: cfg3 104 vs 93 us — experiments/README.md.)

    f32x4 o[CH][NB];
    float m[CH], lsum[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) o[ch][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        m[ch] = NEG_BIG;
        lsum[ch] = 0.f;
    }

    // one page of K (two 16-token halves x KS k-steps) and V^T (NB 16-row blocks): 16 KiB per wave at D = 128
    auto load_page = [&](const int pg, V8 (&kf)[2][KS], V8 (&vf)[NB]) {
        const KV* kb = reinterpret_cast<const KV*>(a.kpool) + ((int64_t)pg * a.Hkv + hk) * (32 * D) + lane * 8;
        const KV* vb = reinterpret_cast<const KV*>(a.vpool) + ((int64_t)pg * a.Hkv + hk) * (32 * D) + c * (D * 8) + col * 8;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[t][ks] = kv_get8_nt<T, KV>(kb + t * (16 * D) + ks * 512);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) vf[nb] = kv_get8_nt<T, KV>(vb + nb * 128);
    };
    // The page a sequence is still filling: only the part its nv written tokens occupy is requested (round 5: the launch
    // cost one whole page per started page — bench.py's steps got 0.1 ms slower the moment the batch crossed a page
    // boundary, and the counters saw 1.016 x the algorithmic bytes).  K: the second 16-token tile is requested only once the
    // sequence has reached it — until then its registers repeat the first tile (finite values, scores masked); a scalar base,
    // the lanes' offsets stay what they are.  V keeps tokens 4 g .. 4 g + 3 of both tiles in column group g and a lane reads one
    // group: the lanes of groups behind the last written token re-read group 0 (lines the wave requests anyway; finite values
    // under a P of exactly 0).  Addresses move, no lane is switched off.  (Redirecting the unwritten tokens INSIDE the tile that
    // is being filled as well costs 6 - 9 more VGPRs — two instead of three waves per SIMD, which the many-block shapes need;
    // tests/test_ops_gpu.py::test_attention_decode_every_fill_of_the_last_page poisons what must not be requested.)
    auto load_page_part = [&](const int pg, const int nv, V8 (&kf)[2][KS], V8 (&vf)[NB]) {
        const KV* kp = reinterpret_cast<const KV*>(a.kpool) + ((int64_t)pg * a.Hkv + hk) * (32 * D);
        const KV* kp1 = kp + (nv > 16 ? 16 * D : 0);  // wave-uniform: a scalar base, the lanes' offsets stay what they are
        const KV* vb = reinterpret_cast<const KV*>(a.vpool) + ((int64_t)pg * a.Hkv + hk) * (32 * D) + col * 8 +
                       ((4 * c < nv) ? c * (D * 8) : 0);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            kf[0][ks] = kv_get8_nt<T, KV>(kp + lane * 8 + ks * 512);
            kf[1][ks] = kv_get8_nt<T, KV>(kp1 + lane * 8 + ks * 512);
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) vf[nb] = kv_get8_nt<T, KV>(vb + nb * 128);
    };
    // FULL: every key of the page is visible to every valid column (all but the last page of a decode step) — no
    // masks.  The softmax reference m[ch] is only moved when a tile maximum exceeds it by more than 2^RESCALE_LOG2
    // (then P <= 2^RESCALE_LOG2, harmless in fp32 / f16 / bf16): the rescale of O — whose accumulators live in AGPRs,
    // so every multiply costs a read and a write-back as well — and of the running sum then runs in a handful of
    // pages per sequence instead of every page, behind a wave-uniform branch.  (MQA, 3 chunks: 697 -> ~250 VALU
    // instructions per page; the loop is issue-bound, not HBM-bound: tools/attn_nw.py.)
    constexpr float RESCALE_LOG2 = 8.f;
    auto apply_page = [&](const int p, const V8 (&kf)[2][KS], const V8 (&vf)[NB], auto full_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        const int kp0 = p * 32 + c * 4;
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            f32x4 s[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) s[t] = mfma16(kf[t][ks], qf[ch][ks], s[t]);
            }
            // scale, causal/length mask, tile max
            float tmax = NEG_BIG;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = s[t][r] * a.scale_log2;
                    if (!FULL) {
                        bool vis = kp0 + t * 16 + r < kmax[ch];
                        if constexpr (TREE) {
                            // (a key at or past kmax may lie 64 or more behind the first q row: the shift count is masked)
                            const int rel = kp0 + t * 16 + r - (ctx - q_len);
                            vis = vis && (rel < 0 || ((qmask >> (rel & 63)) & 1));
                        }
                        if constexpr (WINDOW) vis = vis && kp0 + t * 16 + r >= kmin;
                        v = vis ? v : NEG_BIG;
                    }
                    s[t][r] = v;
                    tmax = fmaxf(tmax, v);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            if (__any(tmax > m[ch] + RESCALE_LOG2)) {
                const float m_new = fmaxf(m[ch], tmax);
                const float alpha = __builtin_amdgcn_exp2f(m[ch] - m_new);  // 0 while m is still NEG_BIG
                m[ch] = m_new;
                lsum[ch] *= alpha;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) o[ch][nb] *= alpha;
            }
            const float mref = m[ch];
            V8 pf;
            float psum = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float pv = __builtin_amdgcn_exp2f(s[t][r] - mref);
                    // masked entries contribute exactly 0 even while m is still NEG_BIG
                    if (!FULL) pv = (s[t][r] > 0.5f * NEG_BIG) ? pv : 0.f;
                    T pt = from_f32<T>(pv);
                    pf[t * 4 + r] = pt;
                    psum += to_f32(pt);  // normaliser from the rounded P, as flash-attention does
                }
            lsum[ch] += psum;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) o[ch][nb] = mfma16(vf[nb], pf, o[ch][nb]);
        }
        ATTN_STAMP(3);  // (kept once: the wave's first page applied)
    };
    // pages below kfull are visible in full to every column of the tile (the tile's first token sees kfull keys)
    // (TREE: the mask may hide any of the sequence's q rows from the tile, row 0 included)
    const int kfull = TREE ? ctx - q_len : ctx - q_len + t0 + 1;
    int p = pbeg + w;
    ATTN_STAMP(2);  // q requested, first table entry in
    // The partly visible pages of this wave (decode: the sequence's last page) go FIRST (round 4): the softmax is order-
    // independent, and their masked body is a second copy of the page code that each wave runs once — at the end of the
    // launch its instruction fetch and its un-overlapped load were part of every block's tail (ctx 1023 vs 1024: +2.6 us
    // per launch before, +1.7 after); at the start both hide under the first pages' latency.
    bool low = false;  // WINDOW: this wave's first page went through the masked loop
    if constexpr (WINDOW) {
        // The same loop with one more page in front for the wave that owns it (wave 0 of split 0): the page the window starts
        // inside, where that is not the sequence's last page anyway.  All of it is written (nv = 32: what load_page requests)
        // and the masked body hides the keys below this column's kmin.
        const int nfullp = kfull >> 5;
        const int pp_top = p + ((max(nfullp - p, 0) + NW - 1) / NW) * NW;
        low = p == pfirst && (klo & 31) != 0 && p < min(pend, nfullp);
        int pp = low ? p : pp_top;
        int pgp = (pp < pend) ? btrow[pp] : 0;
        while (pp < pend) {
            const int nxt = pp < pp_top ? pp_top : pp + NW;
            const int pg_next = (nxt < pend) ? btrow[nxt] : 0;
            V8 kf[2][KS], vf[NB];
            load_page_part(pgp, min(32, ctx - pp * 32), kf, vf);
            apply_page(pp, kf, vf, std::false_type{});
            pgp = pg_next;
            pp = nxt;
        }
        if (low) p += NW;
    } else {
        const int nfullp = kfull >> 5;  // pages [0, nfullp) are fully visible
        int pp = p + ((max(nfullp - p, 0) + NW - 1) / NW) * NW;
        int pgp = (pp < pend) ? btrow[pp] : 0;
        for (; pp < pend; pp += NW) {
            const int pg_next = (pp + NW < pend) ? btrow[pp + NW] : 0;
            V8 kf[2][KS], vf[NB];
            load_page_part(pgp, min(32, ctx - pp * 32), kf, vf);
            apply_page(pp, kf, vf, std::false_type{});
            pgp = pg_next;
        }
    }
    if (PIPE) {
        // Pairs of fully visible pages with two pages of loads in flight: the next page's 16 KiB are requested before
        // the current page is applied.  The body is straight-line (every load it issues is needed, the trip count is
        // wave-uniform) so that hipcc keeps counted vmcnt waits; with a conditional prefetch it drains to vmcnt(0)
        // before every load and nothing overlaps (measured: no gain).  What is left — an odd full page — takes the plain
        // loop below (the partly visible pages ran first).
        const int nfull = (kfull >> 5) > p ? min(((kfull >> 5) - p + NW - 1) / NW, (pend - p + NW - 1) / NW) : 0;
        const int npairs = p < pend ? nfull >> 1 : 0;
        if (npairs > 0) {
            V8 kfa[2][KS], vfa[NB], kfb[2][KS], vfb[NB];
            load_page(pg_first, kfa, vfa);  // pg_first is a page id only when pbeg + w < pend: npairs > 0 says so
            for (int i = 0; i + 1 < npairs; ++i) {
                load_page(btrow[p + NW], kfb, vfb);
                apply_page(p, kfa, vfa, std::true_type{});
                load_page(btrow[p + 2 * NW], kfa, vfa);
                apply_page(p + NW, kfb, vfb, std::true_type{});
                p += 2 * NW;
            }
            load_page(btrow[p + NW], kfb, vfb);
            apply_page(p, kfa, vfa, std::true_type{});
            apply_page(p + NW, kfb, vfb, std::true_type{});
            p += 2 * NW;
        }
    }
    // the fully visible pages — a loop of their own, not one loop with both bodies: the register allocator sizes a loop
    // for the union of what its branches hold (180 vs 122 VGPRs here, i.e. 2 instead of 3 waves per SIMD, which costs
    // the HBM-bound many-block shapes 5 %)
    // (pg_first: valid only when pbeg + w < pend, the loop's p < pend; WINDOW: the loop above may have taken that page)
    int pg = (PIPE || low) ? ((p < pend) ? btrow[p] : 0) : pg_first;
    for (; p < pend && p * 32 + 32 <= kfull; p += NW) {
        const int pg_next = (p + NW < pend) ? btrow[p + NW] : 0;
        V8 kf[2][KS], vf[NB];
        load_page(pg, kf, vf);
        apply_page(p, kf, vf, std::true_type{});
        pg = pg_next;
    }

    ATTN_STAMP(4);  // pages done
    // ---- combine the 4 waves through LDS ----------------------------------------------------------
    float* so = reinterpret_cast<float*>(smem);          // [CH][NW][D][16]
    float* sml = so + CH * NW * D * 16;                  // [CH][NW][2][16]
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
        float ls = lsum[ch];
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            // (row d = nb 16 + c 4 + r sits at nb 16 + r 4 + c: the four 16-lane groups of a store then hit four different
            // groups of 16 banks instead of the same one — round 5: the [d][16] order was a 4-way conflict on every access)
            for (int r = 0; r < 4; ++r) so[((ch * NW + w) * D + nb * 16 + r * 4 + c) * 16 + col] = o[ch][nb][r];
        if (c == 0) {
            sml[((ch * NW + w) * 2 + 0) * 16 + col] = m[ch];
            sml[((ch * NW + w) * 2 + 1) * 16 + col] = ls;
        }
    }
    __syncthreads();
    ATTN_STAMP(5);  // every wave's O and statistics in LDS
    const int grp = blockIdx.x + gridDim.x * (by + gridDim.y * b);  // the NS blocks that share their columns
    __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(a.ws_o, 0, 0x7FFFFFFF, 0x00020000);
    __amdgpu_buffer_rsrc_t rm = __builtin_amdgcn_make_buffer_rsrc(a.ws_ml, 0, 0x7FFFFFFF, 0x00020000);
    // thread -> (chunk, column j, 8 consecutive d)
    for (int item = tid; item < CH * 16 * (D / 8); item += 64 * NW) {
        const int j = item & 15, dc = (item >> 4) % (D / 8), ch = item / (16 * (D / 8));
        const int hc = hc0 + ch;
        const int tqj = j >> a.Gp_shift, gj = j & (a.Gp - 1);
        if (!(gj < a.Gc && hc * 16 + gj < a.G && t0 + tqj < q_len)) continue;
        const float* soc = so + ch * NW * D * 16;
        const float* smc = sml + ch * NW * 2 * 16;
        float mw[NW], mstar = NEG_BIG;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            mw[k] = smc[(k * 2) * 16 + j];
            mstar = fmaxf(mstar, mw[k]);
        }
        float l = 0.f, acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            float f = exp2f(mw[k] - mstar);
            l += smc[(k * 2 + 1) * 16 + j] * f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int d = dc * 8 + e;
                acc[e] += soc[(k * D + ((d & ~15) | ((d & 3) << 2) | ((d >> 2) & 3))) * 16 + j] * f;
            }
        }
        // one-byte cache: V was read as v / v_scale, so the normaliser becomes l / v_scale (every output form and both merges
        // then divide by it as they are)
        if constexpr (kv_is8<T, KV>()) l *= a.inv_v_scale;
        const int64_t tokidx = q0 + t0 + tqj;
        const int headj = hk * a.G + hc * 16 + gj;
        if (a.NS == 1) {
            const float inv = l > 0.f ? 1.f / l : 0.f;
            V8 ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = from_f32<T>(acc[e] * inv);
            st16(reinterpret_cast<T*>(a.out) + (a.out_frag ? xf_off(tokidx, (int64_t)headj * D + dc * 8, (int64_t)a.H * D)
                                                           : (tokidx * a.H + headj) * D + dc * 8), ov);
        } else if (a.counters) {
            // fused combine: the record leaves as 16-byte write-through stores (no other block's record shares a
            // 128-byte line with it: 16 columns x NS x 16 bytes per (group, chunk))
            const int64_t rec = (((int64_t)grp * CH + ch) * 16 + j) * a.NS + split;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{acc[0], acc[1], acc[2], acc[3]}), ro,
                                                   (uint32_t)((rec * D + dc * 8) * 4), 0, 16);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{acc[4], acc[5], acc[6], acc[7]}), ro,
                                                   (uint32_t)((rec * D + dc * 8 + 4) * 4), 0, 16);
            if (dc == 0)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{mstar, l, 0.f, 0.f}), rm,
                                                       (uint32_t)(rec * 16), 0, 16);
        } else {
            float* wo = a.ws_o + ((tokidx * a.H + headj) * a.NS + split) * D + dc * 8;
            *reinterpret_cast<f32x4*>(wo) = f32x4{acc[0], acc[1], acc[2], acc[3]};
            *reinterpret_cast<f32x4*>(wo + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
            if (dc == 0) {
                float* wm = a.ws_ml + ((tokidx * a.H + headj) * a.NS + split) * 2;
                wm[0] = mstar;
                wm[1] = l;
            }
        }
    }
    ATTN_STAMP(6);  // output or split record stored
    ATTN_STAMP_FLUSH
    if (a.NS == 1 || !a.counters) return;

    // ---- the last of the group's NS blocks to get here merges the NS records (what attn_combine_kernel does in a
    //      second launch otherwise).  Protocol of MI355X_MICROARCH.md: write-through (sc1) payload, drained, then an
    //      agent-scope counter; the reader uses sc1 loads on lines its XCD cannot hold yet. ------------------------
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* lastp = reinterpret_cast<int*>(smem);
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.counters + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old + 1u == (unsigned)a.NS;
        if (last) __hip_atomic_store(a.counters + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
        *lastp = last;
    }
    __syncthreads();
    if (!*lastp) return;
    // IB of this thread's items x MB splits are loaded before the first use (one round trip per batch instead of one
    // per split and item); batches are folded with the usual running-maximum rescale.
    constexpr int ITEMS = CH * 16 * (D / 8), THREADS = 64 * NW, ITER = (ITEMS + THREADS - 1) / THREADS;
    // <= 8 records (96 registers) in flight; the three-chunk (MQA) blocks, one per CU anyway, take 12: their four splits
    // arrive in one round trip instead of two
    constexpr int IB = ITER < 4 ? ITER : 4, MB = (CH == 3 && IB == 3 ? 12 : 8) / IB;
    for (int it0 = 0; it0 < ITER; it0 += IB) {
        bool ok[IB];
        int64_t rec0[IB];
        int dcs[IB];
        float mrun[IB], lrun[IB], acc[IB][8];
#pragma unroll
        for (int it = 0; it < IB; ++it) {
            const int item = tid + (it0 + it) * THREADS;
            const int j = item & 15, dc = (item >> 4) % (D / 8), ch = item / (16 * (D / 8));
            const int tqj = j >> a.Gp_shift, gj = j & (a.Gp - 1);
            ok[it] = item < ITEMS && gj < a.Gc && (hc0 + ch) * 16 + gj < a.G && t0 + tqj < q_len;
            rec0[it] = ok[it] ? (((int64_t)grp * CH + ch) * 16 + j) * a.NS : 0;  // (clamped: the loads stay in bounds)
            dcs[it] = dc;
            mrun[it] = NEG_BIG;
            lrun[it] = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[it][e] = 0.f;
        }
        for (int s0 = 0; s0 < a.NS; s0 += MB) {
            f32x4 ml[IB][MB], lo[IB][MB], hi[IB][MB];
#pragma unroll
            for (int it = 0; it < IB; ++it)
#pragma unroll
                for (int k = 0; k < MB; ++k) {
                    const int64_t rec = rec0[it] + min(s0 + k, a.NS - 1);
                    ml[it][k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rm, (uint32_t)(rec * 16), 0, 16));
                    lo[it][k] = __builtin_bit_cast(
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(ro, (uint32_t)((rec * D + dcs[it] * 8) * 4), 0, 16));
                    hi[it][k] = __builtin_bit_cast(
                        f32x4, __builtin_amdgcn_raw_buffer_load_b128(ro, (uint32_t)((rec * D + dcs[it] * 8 + 4) * 4), 0, 16));
                }
#pragma unroll
            for (int it = 0; it < IB; ++it) {
                float mb = mrun[it];
#pragma unroll
                for (int k = 0; k < MB; ++k)
                    if (s0 + k < a.NS) mb = fmaxf(mb, ml[it][k][0]);
                const float fr = exp2f(mrun[it] - mb);  // 0 for the first batch (mrun = NEG_BIG)
                mrun[it] = mb;
                lrun[it] *= fr;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[it][e] *= fr;
#pragma unroll
                for (int k = 0; k < MB; ++k) {
                    if (s0 + k < a.NS) {
                        const float f = exp2f(ml[it][k][0] - mb);
                        lrun[it] += ml[it][k][1] * f;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            acc[it][e] += lo[it][k][e] * f;
                            acc[it][e + 4] += hi[it][k][e] * f;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int it = 0; it < IB; ++it) {
            if (!ok[it]) continue;
            const int item = tid + (it0 + it) * THREADS;
            const int j = item & 15, ch = item / (16 * (D / 8));
            const int tqj = j >> a.Gp_shift, gj = j & (a.Gp - 1);
            const float inv = lrun[it] > 0.f ? 1.f / lrun[it] : 0.f;
            V8 ov;
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = from_f32<T>(acc[it][e] * inv);
            const int64_t tokidx = q0 + t0 + tqj;
            const int headj = hk * a.G + (hc0 + ch) * 16 + gj;
            st16(reinterpret_cast<T*>(a.out) + (a.out_frag ? xf_off(tokidx, (int64_t)headj * D + dcs[it] * 8, (int64_t)a.H * D)
                                                           : (tokidx * a.H + headj) * D + dcs[it] * 8), ov);
        }
    }
}

// out[tok][head][:] = sum_s O_s * 2^(m_s - m*) / sum_s l_s * 2^(m_s - m*);  one wave per (tok, head), four per workgroup.
// MAXS > 0 (NS <= MAXS): every record of the row — {m, l} and the O slice of each split — is requested before the first use,
// so the launch is ONE round trip to the records instead of two dependent passes over them (round 6: the MQA launch pair
// spends 4.5 of its 26 us here); MAXS == 0: any NS, the two-pass loop.  Same expressions in the same order either way.
template <typename T, int D, int MAXS>
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ ws_o,
                                                           const float* __restrict__ ws_ml, T* __restrict__ out,
                                                           int NS, int H, int out_frag, int64_t rows,
                                                           const int32_t* __restrict__ q_end) {
    // lane covers columns i 64 + lane; a D that is not a multiple of 64 (96) leaves the top lanes of its last slice idle
    constexpr int DL = (D + 63) / 64;
    const int64_t th = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // tok*H + head
    if (th >= rows) return;
    // q_len > 1: the grid covers B * max_q_len rows, the sequences may hold fewer (ragged cu_seqlens_q).  Rows from
    // cu_seqlens_q[B] on have no records and no place in `out`; *q_end is that entry (null at q_len 1: rows is exact).
    if (q_end && th >= (int64_t)*q_end * H) return;
    const int lane = threadIdx.x & 63;
    auto in_row = [&](int i) { return D % 64 == 0 || i * 64 + lane < D; };
    float mstar = NEG_BIG;
    float l = 0.f;
    float acc[DL] = {};
    if (MAXS > 0) {
        float ms[MAXS ? MAXS : 1], ls[MAXS ? MAXS : 1], os[MAXS ? MAXS : 1][DL];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            const int64_t r = th * NS + min(s, NS - 1);
            ms[s] = ws_ml[r * 2];
            ls[s] = ws_ml[r * 2 + 1];
#pragma unroll
            for (int i = 0; i < DL; ++i) os[s][i] = in_row(i) ? ws_o[r * D + i * 64 + lane] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < NS) mstar = fmaxf(mstar, ms[s]);
#pragma unroll
        for (int s = 0; s < MAXS; ++s)
            if (s < NS) {
                const float f = exp2f(ms[s] - mstar);
                l += ls[s] * f;
#pragma unroll
                for (int i = 0; i < DL; ++i) acc[i] += os[s][i] * f;
            }
    } else {
        for (int s = 0; s < NS; ++s) mstar = fmaxf(mstar, ws_ml[(th * NS + s) * 2]);
        for (int s = 0; s < NS; ++s) {
            float f = exp2f(ws_ml[(th * NS + s) * 2] - mstar);
            l += ws_ml[(th * NS + s) * 2 + 1] * f;
#pragma unroll
            for (int i = 0; i < DL; ++i)
                if (in_row(i)) acc[i] += ws_o[(th * NS + s) * D + i * 64 + lane] * f;
        }
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int i = 0; i < DL; ++i) {
        if (!in_row(i)) continue;
        const int64_t o = out_frag ? xf_off(th / H, (th % H) * D + i * 64 + lane, (int64_t)H * D) : th * D + i * 64 + lane;
        out[o] = from_f32<T>(acc[i] * inv);
    }
}

// the one place that spells attn_paged_kernel's launch: the preloaded leading parameters, then the whole argument block
template <typename Kernel, typename Args>
static void launch_attn_kernel(Kernel kern, dim3 grid, int nw, size_t lds, hipStream_t st, const Args& a) {
    hipLaunchKernelGGL(kern, grid, dim3(64 * nw), lds, st, a.bt, a.cu_q, a.ctx_lens, a.kpool, a.max_pages, a.NS, a.Hkv, a.HCB,
                       a.xcd_remap, a);
}

// the decode kernel as the plan names it, then the combine launch of a split call that has no arrival counters (multi-chunk
// blocks, or none were free).  That one runs over total_q = B * max_q_len rows: it reads the real count, *q_end.
// (window: the W of a plan of form window, which rides behind the block in an AttnWindowArgs)
template <typename T, typename KV, int D>
static int launch_decode(const AttnPlan& p, const AttnTreeArgs& a, int window, int64_t total_q, const int32_t* q_end,
                         hipStream_t st) {
    const dim3 grid((unsigned)p.grid[0], (unsigned)p.grid[1], (unsigned)p.grid[2]);
    // the instances that exist, as decimal digits (window, tree, PIPE, chunks per block, waves per block)
    const int inst = (p.form == ATTN_WINDOW) * 10000 + (p.form == ATTN_TREE) * 1000 + p.pipe * 100 + p.ch * 10 + p.nw;
    const int rc = by_int<11, 12, 13, 14, 18, 112, 114, 21, 22, 24, 124, 31, 32, 34, 134, 1014, 10014>(
        inst, "tgis_attn_paged: (window, tree, PIPE, chunks, waves)", [&](auto i) {
        constexpr int I = decltype(i)::value, NW = I % 10, CH = I / 10 % 10;
        constexpr bool PIPE = I / 100 % 10 != 0, TREE = I / 1000 % 10 != 0, WINDOW = I / 10000 != 0;
        auto kern = attn_paged_kernel<T, KV, D, NW, CH, PIPE, TREE, WINDOW>;
        static bool attr = false;  // (per instance)
        if (!attr && p.lds_bytes > 48 * 1024) {
            (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
            attr = true;
        }
        if constexpr (WINDOW) {
            AttnWindowArgs wa;
            static_cast<AttnArgs&>(wa) = a;
            wa.window = window;
            launch_attn_kernel(kern, grid, NW, (size_t)p.lds_bytes, st, wa);
        } else {
            launch_attn_kernel(kern, grid, NW, (size_t)p.lds_bytes, st, a);
        }
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
    if (rc != TGIS_OK || a.NS == 1 || a.counters) return rc;
    const int64_t rows = total_q * a.H;
    return by_bool(p.maxs8, [&](auto m8) {
        hipLaunchKernelGGL((attn_combine_kernel<T, D, decltype(m8)::value ? 8 : 0>), dim3((unsigned)cdiv64(rows, 4)), dim3(256),
                           0, st, a.ws_o, a.ws_ml, (T*)a.out, a.NS, a.H, a.out_frag, rows, q_end);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}

// What a shape must satisfy to have a plan, then the plan under `hooks` and its own limit: the checks tgis_attn_paged and
// tgis_debug_attn_plan share.
static int checked_plan(int64_t B, int H, int Hkv, int D, int64_t max_q_len, int num_splits, bool tree, const AttnHooks& hooks,
                        AttnPlan* plan, bool window = false) {
    TGIS_CHECK_ARG(H > 0 && Hkv > 0 && H % Hkv == 0, "tgis_attn_paged: H (%d) must be a multiple of Hkv (%d)", H, Hkv);
    TGIS_CHECK_ARG(D == 64 || D == 96 || D == 128, "tgis_attn_paged: head_dim %d not supported (64, 96, 128)", D);
    TGIS_CHECK_ARG(B >= 0 && max_q_len > 0 && num_splits >= 1, "tgis_attn_paged: bad launch bounds");
    const AttnGeom g = geom(H, Hkv);
    TGIS_CHECK_ARG(!window || num_splits == 1 || max_q_len == 1,
                   "tgis_attn_paged_window: key splits are for one q token per sequence (max_q_len %ld): every other windowed "
                   "call takes the prefill form, which takes none", (long)max_q_len);
    const bool prefill_form = !window && max_q_len * g.Gp > 64;
    TGIS_CHECK_ARG(num_splits == 1 || !prefill_form,
                   "tgis_attn_paged: key splits are for the decode form (max_q_len * padded group size <= 64, here %ld * %d): "
                   "the prefill form takes none", (long)max_q_len, g.Gp);
    TGIS_CHECK_ARG(!tree || !prefill_form,
                   "tgis_attn_paged_tree: only the decode form is served (max_q_len * padded group size <= 64, here %ld * "
                   "%d): one 64-bit mask word per q row", (long)max_q_len, g.Gp);
    *plan = plan_attn(B, H, Hkv, D, max_q_len, num_splits, tree, hooks, window);
    TGIS_CHECK_ARG(plan->grid[0] <= 2147483647LL && plan->grid[1] <= 65535 && plan->grid[2] <= 65535,
                   "tgis_attn_paged: grid too large");
    return TGIS_OK;
}

// the only place that writes an argument block: the geometry and launch form from the plan, the rest from the caller
static AttnTreeArgs fill_args(const AttnPlan& p, int H, int Hkv, int num_splits, const void* q, int64_t ld_q,
                              const void* k_pool, const void* v_pool, const int32_t* block_tables, int64_t max_pages,
                              const int32_t* ctx_lens, const int32_t* cu_seqlens_q, void* out, bool out_frag, float scale_log2,
                              float inv_v_scale, void* workspace, unsigned* counters, const uint64_t* q_mask) {
    AttnTreeArgs a;
    a.q = q, a.ld_q = ld_q, a.kpool = k_pool, a.vpool = v_pool;
    a.bt = block_tables, a.max_pages = max_pages, a.ctx_lens = ctx_lens, a.cu_q = cu_seqlens_q;
    a.out = out, a.out_frag = out_frag, a.H = H, a.Hkv = Hkv, a.NS = num_splits;
    a.G = p.geom.G, a.Gc = p.geom.Gc, a.Gp = p.geom.Gp, a.Gp_shift = p.geom.Gp_shift, a.TQ = p.geom.TQ, a.HC = p.geom.HC;
    a.HCB = p.HCB, a.xcd_remap = p.xcd_remap;
    a.scale_log2 = scale_log2, a.inv_v_scale = inv_v_scale;
    a.ws_o = num_splits > 1 ? (float*)workspace : nullptr;
    a.ws_ml = num_splits > 1 ? a.ws_o + p.ws_o_floats[counters != nullptr] : nullptr;
    a.counters = counters, a.q_mask = q_mask;
    return a;
}

}  // namespace

extern "C" int tgis_attn_num_splits(int64_t B, int Hkv, int H, int64_t max_q_len, int64_t max_ctx) {
    return attn_num_splits(B, Hkv, H, max_q_len, max_ctx, attn_hooks());
}
extern "C" int tgis_attn_num_splits_q(int64_t B, int Hkv, int H, int64_t max_q_len, int64_t max_ctx) {
    return attn_num_splits_q(B, Hkv, H, max_q_len, max_ctx, attn_hooks());
}
extern "C" int64_t tgis_attn_workspace_bytes(int64_t total_q_tokens, int H, int Hkv, int D, int num_splits) {
    return attn_workspace_bytes(total_q_tokens, H, Hkv, D, num_splits, attn_hooks());
}

// debug aid (not part of the documented ABI): the launch tgis_attn_paged (tree != 0: tgis_attn_paged_tree) would make under
// the current hooks, without a launch, a device or a stream.  info[16] = {form (0 prefill, 1 decode, 2 tree), waves per block,
// chunks per block, PIPE, HCB, xcd_remap, grid x, y, z, LDS bytes, fused_ok (NS > 1 and the splits merge in the launch if an
// arrival-counter array is free; else the combine launch), maxs8 (that launch is attn_combine_kernel<MAXS = 8>), Gp, TQ, HC, NS}.
extern "C" int tgis_debug_attn_plan(int64_t B, int H, int Hkv, int D, int64_t max_q_len, int num_splits, int tree, int* info) {
    TGIS_CHECK_ARG(info && B >= 1, "tgis_debug_attn_plan: bad arguments");
    AttnPlan p;
    if (const int rc = checked_plan(B, H, Hkv, D, max_q_len, num_splits, tree != 0, attn_hooks(), &p)) return rc;
    const int v[16] = {p.form, p.nw, p.ch, p.pipe, p.HCB, p.xcd_remap, (int)p.grid[0], (int)p.grid[1], (int)p.grid[2],
                       (int)p.lds_bytes, p.fused_ok, p.maxs8, p.geom.Gp, p.geom.TQ, p.geom.HC, num_splits};
    std::copy(v, v + 16, info);
    return TGIS_OK;
}

// tgis_debug_attn_plan for tgis_attn_paged_window with a window of `window` keys per q row (not part of the documented ABI
// either; host only).  info[16] as above: form 3 is the WINDOW variant of the decode kernel (max_q_len 1), form 0 here the WINDOW
// variant of the prefill kernel (any other max_q_len).  A window no row reaches (max_ctx <= window) is the causal launch, which
// tgis_debug_attn_plan reports.  For each of n sequences of ctx[i] cached tokens, the last q_len[i] of them q rows, under this
// window: first[2 i] = the first page its blocks load (table entries below it are not read), first[2 i + 1] = the first key its
// first q row attends to.
extern "C" int tgis_debug_attn_plan_window(int64_t B, int H, int Hkv, int D, int64_t max_q_len, int num_splits, int64_t window,
                                           int64_t n, const int32_t* ctx, const int32_t* q_len, int* info, int* first) {
    TGIS_CHECK_ARG(info && B >= 1 && n >= 0 && (n == 0 || (ctx && q_len && first)), "tgis_debug_attn_plan_window: bad arguments");
    TGIS_CHECK_ARG(window >= 1, "tgis_attn_paged_window: window %ld must be at least 1", (long)window);
    AttnPlan p;
    if (const int rc = checked_plan(B, H, Hkv, D, max_q_len, num_splits, false, attn_hooks(), &p, true)) return rc;
    const int v[16] = {p.form, p.nw, p.ch, p.pipe, p.HCB, p.xcd_remap, (int)p.grid[0], (int)p.grid[1], (int)p.grid[2],
                       (int)p.lds_bytes, p.fused_ok, p.maxs8, p.geom.Gp, p.geom.TQ, p.geom.HC, num_splits};
    std::copy(v, v + 16, info);
    const int w = (int)std::min<int64_t>(window, 2147483647);
    for (int64_t i = 0; i < n; ++i) {
        TGIS_CHECK_ARG(q_len[i] >= 1 && q_len[i] <= ctx[i], "tgis_debug_attn_plan_window: 1 <= q_len <= ctx");
        first[2 * i + 1] = attn_window_first_key(ctx[i], q_len[i], 0, w);
        first[2 * i] = first[2 * i + 1] >> 5;
    }
    return TGIS_OK;
}

// validate, plan, lease counters where the plan may merge in the launch, fill the argument block, launch
static int attn_paged_impl(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                           const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                           const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                           int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                           void* workspace, int64_t workspace_bytes, void* stream, int kv_dtype, float k_scale,
                           float v_scale, bool tree = false, const uint64_t* q_mask = nullptr,
                           const int64_t* window = nullptr) {
    TGIS_CHECK_ARG(q && k_pool && v_pool && block_tables && ctx_lens && cu_seqlens_q && out,
                   "tgis_attn_paged: null tensor");
    TGIS_CHECK_ARG(!tree || q_mask, "tgis_attn_paged_tree: null q_mask");
    TGIS_CHECK_ARG(!window || *window >= 1, "tgis_attn_paged_window: window %ld must be at least 1", (long)(window ? *window : 0));
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "tgis_attn_paged: bad dtype");
    TGIS_CHECK_KV_ARGS("tgis_attn_paged_kv8", kv_dtype, k_scale, v_scale);
    const bool kv8 = kv_dtype == TGIS_KV_FP8_E4M3;
    TGIS_CHECK_ARG(ld_q % 8 == 0 && ((uintptr_t)q % 16) == 0, "tgis_attn_paged: q must be 16-byte aligned");
    TGIS_CHECK_ARG(max_pages > 0, "tgis_attn_paged: bad launch bounds");
    const AttnHooks hooks = attn_hooks();  // read once per call
    AttnPlan plan;
    if (const int rc = checked_plan(B, H, Hkv, D, max_q_len, num_splits, tree, hooks, &plan, window != nullptr)) return rc;
    // a window that no row of the launch reaches is the causal launch (the refusals above hold for it all the same)
    if (window && max_ctx <= *window) {
        window = nullptr;
        if (const int rc = checked_plan(B, H, Hkv, D, max_q_len, num_splits, tree, hooks, &plan)) return rc;
    }
    const int W = window ? (int)std::min<int64_t>(*window, 2147483647) : 0;  // (positions are 32-bit)
    TGIS_CHECK_ARG(ld_out == 0 || ld_out == (int64_t)H * D ||
                       (ld_out == TGIS_LD_FRAGMENTS && max_q_len == 1 && B <= 64 && ((int64_t)H * D) % 64 == 0),
                   "tgis_attn_paged: out is [tokens, H * D] contiguous (ld_out = 0 or H * D), or — decode, <= 64 sequences — in "
                   "fragment order (ld_out = TGIS_LD_FRAGMENTS)");
    if (B == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    // total q tokens is only needed to size the split workspace; callers pass B*max_q_len rows
    const int64_t total_q = B * max_q_len;
    if (num_splits > 1) {
        const int64_t need = attn_workspace_bytes(total_q, H, Hkv, D, num_splits, hooks);
        TGIS_CHECK_ARG(workspace && workspace_bytes >= need, "tgis_attn_paged: workspace too small (%ld < %ld)",
                       (long)workspace_bytes, (long)need);
    }
    // arrival counters for the in-launch merge, if the plan allows it and an array is free (else: the combine launch)
    CounterLease lease;
    unsigned* counters = plan.fused_ok ? attn_counters(st, &lease.dev, &lease.slot) : nullptr;
    const AttnTreeArgs a = fill_args(plan, H, Hkv, num_splits, q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens,
                                     cu_seqlens_q, out, ld_out == TGIS_LD_FRAGMENTS,
                                     (kv8 ? scale * k_scale : scale) * 1.4426950408889634f, kv8 ? 1.f / v_scale : 1.f, workspace,
                                     counters, q_mask);
    TgisTimedScope timed(TGIS_OP_ATTN, st);
    if (plan.form == ATTN_PREFILL) return tgis_launch_attn_prefill(a, B, Hkv, D, max_q_len, dtype, kv8, st, W);
    const int32_t* q_end = max_q_len > 1 ? cu_seqlens_q + B : nullptr;
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_kv<T>(kv8, [&](auto kv) {  // one-byte cache: the same launch shapes over e4m3 pools
            // D = 96: KS = 3, NB = 6 (gpt-neox-20b)
            return by_int<128, 96, 64>(D, "tgis_attn_paged: head_dim", [&](auto d) {
                return launch_decode<T, type_of<decltype(kv)>, decltype(d)::value>(plan, a, W, total_q, q_end, st);
            });
        });
    });
}

extern "C" int tgis_attn_paged(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                               const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                               const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                               int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    return attn_paged_impl(q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens, cu_seqlens_q, out, ld_out, B, H, Hkv, D,
                           max_q_len, max_ctx, scale, dtype, num_splits, workspace, workspace_bytes, stream, TGIS_KV_MODEL,
                           1.f, 1.f);
}

extern "C" int tgis_attn_paged_kv8(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                                   const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                                   const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                                   int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                                   void* workspace, int64_t workspace_bytes, void* stream, int kv_dtype, float k_scale,
                                   float v_scale) {
    return attn_paged_impl(q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens, cu_seqlens_q, out, ld_out, B, H, Hkv, D,
                           max_q_len, max_ctx, scale, dtype, num_splits, workspace, workspace_bytes, stream, kv_dtype,
                           k_scale, v_scale);
}


// tgis_attn_paged / tgis_attn_paged_kv8 with a per-row mask over the sequence's own q rows (the verify step of speculative
// decoding over several candidates per request: utils/paged.py:162-330 flattens them into one forward).
extern "C" int tgis_attn_paged_tree(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                                    const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                                    const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                                    int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                                    void* workspace, int64_t workspace_bytes, void* stream, const uint64_t* q_mask) {
    return attn_paged_impl(q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens, cu_seqlens_q, out, ld_out, B, H, Hkv, D,
                           max_q_len, max_ctx, scale, dtype, num_splits, workspace, workspace_bytes, stream, TGIS_KV_MODEL,
                           1.f, 1.f, true, q_mask);
}

extern "C" int tgis_attn_paged_tree_kv8(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                                        const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                                        const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv,
                                        int D, int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                                        void* workspace, int64_t workspace_bytes, void* stream, int kv_dtype, float k_scale,
                                        float v_scale, const uint64_t* q_mask) {
    return attn_paged_impl(q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens, cu_seqlens_q, out, ld_out, B, H, Hkv, D,
                           max_q_len, max_ctx, scale, dtype, num_splits, workspace, workspace_bytes, stream, kv_dtype,
                           k_scale, v_scale, true, q_mask);
}

// tgis_attn_paged / tgis_attn_paged_kv8 under a sliding window of `window` keys per q row (Mistral: config.sliding_window).
extern "C" int tgis_attn_paged_window(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                                      const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                                      const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                                      int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                                      void* workspace, int64_t workspace_bytes, void* stream, int64_t window) {
    return attn_paged_impl(q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens, cu_seqlens_q, out, ld_out, B, H, Hkv, D,
                           max_q_len, max_ctx, scale, dtype, num_splits, workspace, workspace_bytes, stream, TGIS_KV_MODEL,
                           1.f, 1.f, false, nullptr, &window);
}

extern "C" int tgis_attn_paged_window_kv8(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                                          const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                                          const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv,
                                          int D, int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                                          void* workspace, int64_t workspace_bytes, void* stream, int kv_dtype, float k_scale,
                                          float v_scale, int64_t window) {
    return attn_paged_impl(q, ld_q, k_pool, v_pool, block_tables, max_pages, ctx_lens, cu_seqlens_q, out, ld_out, B, H, Hkv, D,
                           max_q_len, max_ctx, scale, dtype, num_splits, workspace, workspace_bytes, stream, kv_dtype,
                           k_scale, v_scale, false, nullptr, &window);
}
