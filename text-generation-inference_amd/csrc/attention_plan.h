// Which launch a shape takes in paged attention: the geometry, the tuning hooks, the key-split rules, the workspace size and
// the plan of one tgis_attn_paged call.  Host only, no HIP headers (any C++17 compiler takes it).  attention.hip launches what
// plan_attn returns and tgis_debug_attn_plan reports it without a launch; tests/test_attn_plan_cpu.py restates it.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

static inline int64_t attn_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

static inline int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// G q heads per kv head, in HC chunks of Gc <= 16 heads; a 16-column tile holds TQ q tokens x Gp (Gc padded to a power of two)
struct AttnGeom {
    int G, Gc, Gp, TQ, HC;
    int Gp_shift;  // Gp == 1 << Gp_shift
};
static inline AttnGeom geom(int H, int Hkv) {
    AttnGeom g = {};
    g.G = H / Hkv;
    g.Gc = std::min(g.G, 16);
    g.HC = (g.G + 15) / 16;
    g.Gp = next_pow2(g.Gc);
    g.TQ = 16 / g.Gp;
    while ((1 << g.Gp_shift) < g.Gp) ++g.Gp_shift;
    return g;
}

// The tuning and A/B hooks of the causal launch, all read here.  TGIS_ATTN_NW, TGIS_ATTN_CH and
// TGIS_ATTN_NO_PREFILL_KERNEL are read at EVERY call (tools/attn_nw.py and its kin set them between launches of one
// process); TGIS_ATTN_PIPE, TGIS_ATTN_XCD and TGIS_ATTN_FUSED_COMBINE are read ONCE per process, at the first call (one
// process per value; the tests start a fresh child).  The tree launch follows none but FUSED_COMBINE (plan_attn).
// nw: waves per block (1, 2, 3, 8 as given, anything else asks for 4), 0 = not set; ch: at most this many 16-head chunks per
// block (1 - 3), 0 = not set; pipe: -1 = not set, 0 = never two pages in flight, 2 = also in one-chunk blocks of 2 or 4 waves;
// xcd_off, fused_off: the variable is 0; no_prefill_kernel: the variable exists (long q on the decode kernel).
struct AttnHooks { int nw, ch, pipe; bool xcd_off, fused_off, no_prefill_kernel; };
extern "C" char** environ;
static inline AttnHooks attn_hooks() {
    // one sweep over the environment per call (every launch pays for it: cheaper than one getenv per variable)
    static const char* const names[6] = {"NW", "CH", "NO_PREFILL_KERNEL", "PIPE", "XCD", "FUSED_COMBINE"};
    const char* v[6] = {};
    for (char** e = environ; e && *e; ++e) {
        if (strncmp(*e, "TGIS_ATTN_", 10) != 0) continue;
        for (int i = 0; i < 6; ++i) {
            const size_t n = strlen(names[i]);
            if (!v[i] && strncmp(*e + 10, names[i], n) == 0 && (*e)[10 + n] == '=') v[i] = *e + 10 + n + 1;
        }
    }
    static const int pipe = v[3] ? atoi(v[3]) : -1;  // these three: what the first call saw
    static const bool xcd_off = v[4] && atoi(v[4]) == 0, fused_off = v[5] && atoi(v[5]) == 0;
    const int nw = v[0] ? atoi(v[0]) : 0, ch = v[1] ? atoi(v[1]) : 0;  // tuning hooks (tools/attn_nw.py)
    return {!v[0] ? 0 : (nw == 1 || nw == 2 || nw == 3 || nw == 8) ? nw : 4, (ch >= 1 && ch <= 3) ? ch : 0, pipe, xcd_off,
            fused_off, v[2] != nullptr};
}

// Decode with fewer than 256 (sequence, kv head) groups: blocks of 8 waves that share one group's keys page by page
// (and merge through LDS) instead of more key splits merged across blocks.
static inline bool wide_decode_blocks(int64_t groups, int ch) { return ch == 1 && groups < 256; }

// 16-head chunks one decode block serves (register budget: 3 sets of O accumulators at D = 128)
static inline int chunks_per_block(int HC, int64_t max_q_len, const AttnHooks& hooks) {
    return (max_q_len == 1 && HC > 1) ? std::min(HC, hooks.ch ? hooks.ch : 3) : 1;
}

// Blocks per launch and key split of the decode kernel: one per (sequence, kv head, block of ch chunks, q tile)
static inline int64_t attn_groups(int64_t B, int Hkv, const AttnGeom& g, int ch, int64_t max_q_len) {
    return B * Hkv * attn_cdiv(g.HC, ch) * attn_cdiv(max_q_len, g.TQ);
}
// records of the fused combine: [group = (q tile, kv head, chunk block, sequence)][chunk][16 columns][split]
static inline int64_t attn_records(int64_t groups, int ch, int num_splits) { return groups * ch * 16 * num_splits; }

// tgis_attn_num_splits
static inline int attn_num_splits(int64_t B, int Hkv, int H, int64_t max_q_len, int64_t max_ctx, const AttnHooks& hooks) {
    if (B <= 0 || Hkv <= 0 || H <= 0 || H % Hkv != 0 || max_q_len != 1) return 1;  // splits: decode only
    AttnGeom g = geom(H, Hkv);
    const int ch = chunks_per_block(g.HC, max_q_len, hooks);
    int64_t base = attn_groups(B, Hkv, g, ch, max_q_len);
    int64_t pages = attn_cdiv(std::max<int64_t>(max_ctx, 1), 32);
    // single-chunk blocks, many groups: ~512 blocks fill 256 CUs twice; more, thinner blocks lose to the dispatch ramp
    // and the merge
    int64_t ns;
    if (wide_decode_blocks(base, ch)) {
        // few (sequence, kv head) groups: 8-wave blocks, one round of <= 256 of them, >= 2 pages per wave
        // (tools/attn_nw.py, us: B=16 GQA 8:1 D=64 ctx 512: 6.8 unsplit vs 8.5 at 4 splits of 4 waves;
        //  B=1 MHA D=128 ctx 2048: 14.1 at 8 splits vs 17.7 at 16; B=4 GQA 4:1 ctx 4096: 19.0 at 8 vs 24.0 at 16)
        ns = std::min<int64_t>(attn_cdiv(256, base), pages / 16);
        // Round 6 (profiles/r06_attn_fewgroups.log, first column = the rule above): from 32 pages on, up to 8 splits of >= 8
        // pages pay as long as every block still gets a CU of its own — B 1 MHA ctx 1024 11.6 -> 9.5 us (2 -> 8 splits), B 4
        // GQA 8:1 12.3 -> 10.4, B 8 GQA 8:1 D 64 9.4 -> 8.3, B 2 MHA 12.9 -> 11.8; 96 groups keep 2 (3 would be 288 blocks:
        // 16.4 vs 14.3), 16 pages keep 1 (8.7 vs 10.2), long contexts keep the rule above (>= 16 pages per block).
        if (pages >= 32) ns = std::max<int64_t>(ns, std::min<int64_t>(std::min<int64_t>(256 / base, pages / 8), 8));
        // From 128 groups on the merge costs more than the second half of the CUs gives while the context is short (a 7B rank at
        // TP = 8, B 32 x 4 heads, ctx 1024: 16.0 us unsplit, 16.5 at 2 splits; 64 groups, ctx 2048: 24.0 / 19.2 / 17.7 at
        // 1 / 2 / 4 — profiles/r05_attn_tp8.log).  Round 6 swept it over the context (profiles/r06_attn_base128.log): exactly
        // 128 groups take 2 splits from ctx 2048 on (26.9 vs 29.1 us, 46.0 vs 51.7 at 4096, 166.6 vs 194.8 at 16384: the page
        // walk grows, the merge does not); 129 - 255 groups never do (2 splits would be a second round of blocks: 192 groups
        // 41.2 vs 34.9 at 2048, 272.8 vs 243.5 at 16384).
        if (base >= 128) ns = (base * 2 <= 256 && pages >= 64) ? 2 : 1;
    } else if (ch > 1) {
        // multi-chunk blocks hold three sets of accumulators: one block per CU, one wave per SIMD, so the block's time is
        // its waves' page count (~1 us per page: issue-bound) plus ~12 us.  Their splits are merged by the combine launch,
        // not in the launch (a last-arriving block reads NS x 24 KB through ONE CU: 2.7 us at 4 splits, 5.4 at 8).
        // 48 q heads on 1 kv head, B=32 ctx 4096, us (kernel + combine): 26.7 at 4 splits, 25.1 at 6, 25.3 at 8
        // (in-launch merge: 28.1 / 28.6 / 30.2)
        // round 6: with the combine launch down to one round trip (24.1 vs 25.3 us at 6 splits) 8 splits = 256 blocks edge out
        // 6 (23.9 vs 24.2, profiles/r06_mqa_variants.log)
        ns = std::min<int64_t>(attn_cdiv(256, base), pages / 16);
    } else {
        ns = attn_cdiv(512, base);
        ns = std::min<int64_t>(ns, attn_cdiv(pages, 4));  // at least one page per wave
    }
    ns = std::max<int64_t>(1, std::min<int64_t>(ns, 64));
    return (int)ns;
}

// tgis_attn_num_splits_q.  Key splits of any decode-form launch: attn_num_splits at q_len 1, 1 for the prefill form, and for a
// few q tokens per sequence (a verify step of speculative decoding, a short suffix behind reused prefix pages) the rule below.
static inline int attn_num_splits_q(int64_t B, int Hkv, int H, int64_t max_q_len, int64_t max_ctx, const AttnHooks& hooks) {
    if (max_q_len == 1) return attn_num_splits(B, Hkv, H, max_q_len, max_ctx, hooks);
    if (B <= 0 || Hkv <= 0 || H <= 0 || H % Hkv != 0 || max_q_len < 1) return 1;
    AttnGeom g = geom(H, Hkv);
    if (max_q_len * g.Gp > 64) return 1;  // the prefill form takes no key splits
    const int64_t pages = attn_cdiv(std::max<int64_t>(max_ctx, 1), 32);
    if (max_ctx < 1024) return 1;  // below 1024 keys (32 pages) every q_len > 1 launch stays the one it was
    // One-chunk blocks of 4 waves, one per (sequence, kv head, 16-head chunk, q tile) and split.  Fitted to
    // profiles/attn_qsplit_sweep.log (us per launch, D 128):
    //  - one round of <= 256 blocks (the floor: 11 splits of 24 groups are 264 blocks, 36.9 us where 8 take 30.7), >= 16 pages
    //    per block;
    //  - short contexts: up to 8 splits of >= 4 pages, one per wave (7B B 1 q 4 ctx 1024: 19.9 unsplit, 15.4 at 2, 11.8 at 8;
    //    GQA 8:1 B 1 q 2 ctx 2048: 13.5 at 8, 15.1 at 16);
    //  - 64 - 255 groups: a second round of blocks pays from 32 pages per block on (7B B 4 q 4 ctx 8192: 91.6 at 2, 86.3 at 4;
    //    GQA 8:1 B 4 q 4 ctx 32768: 177.2 at 4, 168.3 at 8); fewer groups lose to the merge (GQA 8:1 B 1 q 4 ctx 32768: 55.9 at
    //    16, 59.2 at 32);
    //  - from 256 groups on the launch stays unsplit: 2 splits give 3 - 8 % from ctx 8192 on and lose below it.
    const int64_t base = attn_groups(B, Hkv, g, chunks_per_block(g.HC, max_q_len, hooks), max_q_len);
    const int64_t one = 256 / base;
    int64_t ns = std::min<int64_t>(one, pages / 16);
    ns = std::max<int64_t>(ns, std::min<int64_t>(std::min<int64_t>(one, pages / 4), 8));
    if (base >= 64 && base < 256) ns = std::max<int64_t>(ns, std::min<int64_t>(512 / base, pages / 32));
    return (int)std::max<int64_t>(1, std::min<int64_t>(ns, 32));  // (no count above 32 was measured)
}

// tgis_attn_workspace_bytes
static inline int64_t attn_workspace_bytes(int64_t total_q_tokens, int H, int Hkv, int D, int num_splits,
                                           const AttnHooks& hooks) {
    if (num_splits <= 1 || Hkv <= 0 || H % Hkv != 0) return 0;
    // the larger of the two layouts: per (token, head, split) {O[D], m, l} for the two-launch combine, or the
    // line-padded records of the fused one (16 columns per group and chunk, {m, l} in 16 bytes)
    const int64_t two_pass = total_q_tokens * H * num_splits * ((int64_t)D + 2) * 4;
    // The fused size is that of total_q_tokens sequences of one token.  It covers B sequences of max_q_len tokens
    // (total_q_tokens = B * max_q_len) as well: their launch has B * ceil(max_q_len / TQ) <= total_q_tokens q tiles per
    // (kv head, chunk block), and one-chunk blocks over all HC <= ceil(HC / ch) * ch chunks.
    AttnGeom g = geom(H, Hkv);
    const int ch = chunks_per_block(g.HC, 1, hooks);
    const int64_t fused = attn_records(attn_groups(total_q_tokens, Hkv, g, ch, 1), ch, num_splits) * ((int64_t)D + 4) * 4;
    return std::max(two_pass, fused);
}

enum AttnForm { ATTN_PREFILL = 0, ATTN_DECODE = 1, ATTN_TREE = 2, ATTN_WINDOW = 3 };

// Sliding-window attention (tgis_attn_paged_window): the q row at cache position p attends to the W positions p - W < j <= p.
// Row t of a sequence's q_len rows sits at p = ctx - q_len + t, so this is the first position it sees; the first page a block
// loads is that of its first row, >> 5.  (constexpr: the kernels call it too.)
constexpr int attn_window_first_key(int ctx, int q_len, int t, int window) {
    return ctx - q_len + t + 1 > window ? ctx - q_len + t + 1 - window : 0;
}

constexpr int64_t ATTN_FUSED_MAX_GROUPS = 1 << 20;  // the in-launch merge counts arrivals per group (attention_counters.h)

struct AttnPlan {
    AttnForm form;    // prefill: attention_prefill.hip; decode / tree / window: attn_paged_kernel<.., nw, ch, pipe, tree, window>
    bool window;      // the WINDOW variant of the form's kernel (form window at one q token per sequence, else form prefill)
    AttnGeom geom;
    int ch, HCB, nw;  // 16-head chunks per block; blocks per kv head along the chunks; waves per block
    bool pipe, xcd_remap;  // two pages in flight per wave; the chunk blocks of a (sequence, split, kv head) group on one XCD
    int64_t grid[3];  // (q tiles, kv heads x HCB, sequences x splits); the launcher refuses y, z > 65535
    int64_t lds_bytes, groups, records;  // groups: blocks per key split; records of the in-launch merge
    bool fused_ok;    // num_splits > 1: the last block of a group may merge the splits in the launch, given arrival counters
    bool maxs8;       // otherwise the combine launch is attn_combine_kernel<MAXS = 8> (else <MAXS = 0>)
    int64_t ws_o_floats[2];  // where ws_ml begins in the workspace: [0] combine launch, [1] in-launch merge
};

// The one chooser.  The arguments are valid (H % Hkv == 0, sizes >= 1) and the prefill form comes unsplit and without a tree.
// window: a windowed call (never a tree) takes the restricted plan of the tree variant at one q token per sequence and the
// prefill form at any other q length, whatever max_q_len * Gp is and whatever TGIS_ATTN_NO_PREFILL_KERNEL says.
static inline AttnPlan plan_attn(int64_t B, int H, int Hkv, int D, int64_t max_q_len, int num_splits, bool tree,
                                 const AttnHooks& hooks, bool window = false) {
    AttnPlan p = {};
    const AttnGeom g = p.geom = geom(H, Hkv);
    const bool prefill_form = max_q_len * g.Gp > 64;
    p.form = tree ? ATTN_TREE : (prefill_form && !hooks.no_prefill_kernel) ? ATTN_PREFILL : ATTN_DECODE;
    if (window) p.form = max_q_len > 1 ? ATTN_PREFILL : ATTN_WINDOW, p.window = true;
    tree = tree || window;  // from here on: the restricted plan, which follows no hook but FUSED_COMBINE
    p.maxs8 = num_splits <= 8;
    if (p.form == ATTN_PREFILL) {
        // long q (prefill): blocks of 128 columns that stage each K/V page once in LDS (attention_prefill.hip)
        p.ch = 1, p.HCB = g.HC, p.nw = 4;
        p.grid[0] = attn_cdiv(max_q_len, g.TQ * 8), p.grid[1] = (int64_t)Hkv * g.HC, p.grid[2] = B;
        p.lds_bytes = (int64_t)2 * 2 * 32 * D * 2;
        p.groups = p.grid[0] * p.grid[1] * p.grid[2];
        return p;
    }
    // the tree variant (and the window variant): one-chunk blocks of 4 waves at any q_len — what the causal launch takes by
    // default at q_len > 1.  It follows none of the NW, CH, PIPE and XCD hooks: a measurement that sets one of them compares the causal launch in
    // another configuration with this one as it always is.
    p.ch = tree ? 1 : chunks_per_block(g.HC, max_q_len, hooks);
    p.HCB = (g.HC + p.ch - 1) / p.ch;
    p.groups = attn_groups(B, Hkv, g, p.ch, max_q_len);
    p.grid[0] = attn_cdiv(max_q_len, g.TQ), p.grid[1] = (int64_t)Hkv * p.HCB, p.grid[2] = B * num_splits;
    p.xcd_remap = !tree && !hooks.xcd_off && max_q_len == 1 && p.grid[0] == 1 && p.HCB > 1 && (B * num_splits * Hkv) % 8 == 0;
    // waves per block: with >= 1024 (sequence, kv head) blocks the chip is full either way and 2-wave blocks halve
    // the page-count imbalance between a block's waves (33 pages over 4 waves = 9/8/8/8; over 2 = 17/16)
    const int64_t nblocks = p.groups * num_splits;
    // (past ~2k blocks the dispatch rate, 7 ns per workgroup, costs more than the imbalance)
    p.nw = 4;
    if (!tree) {
        if (max_q_len == 1 && nblocks >= 1024 && nblocks < 2048) p.nw = 2;
        // wide blocks (8 waves): few (sequence, kv head) groups, the waves of one block share the keys; three waves per
        // SIMD at 1024 blocks is an A/B hook.  Both exist for one-chunk blocks only.
        if (max_q_len == 1 && wide_decode_blocks(p.groups, p.ch)) p.nw = 8;
        if (hooks.nw) p.nw = (p.ch > 1 && (hooks.nw > 4 || hooks.nw == 3)) ? 4 : hooks.nw;
        // Two pages in flight where a block is alone on its CU anyway (multi-chunk blocks: nothing else there hides the load
        // latency; MQA 48:1, B=32, ctx 4096: 30.3 -> 25.8 us).  The 8-wave blocks of few-group shapes measured no different,
        // and the many-block shapes keep the small-register variant.
        p.pipe = p.ch > 1 ? (p.nw == 4 && hooks.pipe != 0) : ((p.nw == 2 || p.nw == 4) && hooks.pipe == 2);
    }
    p.lds_bytes = (int64_t)p.ch * (p.nw * D * 16 + p.nw * 2 * 16) * 4;  // e.g. CH = 3, D = 128, NW = 4: 98 KB of combine scratch
    // one launch: the last block of each (q tile, kv head, chunk block, sequence) group merges the splits (no combine launch).
    // Multi-chunk blocks never do (attn_num_splits).
    p.records = attn_records(p.groups, p.ch, num_splits);
    p.fused_ok = num_splits > 1 && !hooks.fused_off && p.groups <= ATTN_FUSED_MAX_GROUPS &&
                 p.records * D * 4 < (1ll << 31) && p.ch == 1;
    p.ws_o_floats[0] = B * max_q_len * H * num_splits * D;  // [total_q][H][NS][D], total_q = B * max_q_len rows
    p.ws_o_floats[1] = p.records * D;
    return p;
}
