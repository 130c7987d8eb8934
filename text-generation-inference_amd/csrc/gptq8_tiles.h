// The 8-bit GPTQ tile GEMM (any M; meant for forwards past the 64 rows of gptq8_gemm_body.h): out[M, N] = x @ dequant(W)
// (+ bias) over the prepared image of tgis_gptq8_prepare, without the dense f16 copy of W that the dequantise + library GEMM
// path writes and reads back.  Included at the end of gptq8.hip, whose checks and layout helpers the entry point shares.
//
// Grid (column blocks, row tiles).  A block of 4 waves owns one row tile of 32 NB rows (NB = 2 or 4, one 32x32 accumulator
// per 32-row block and wave) x CT column tiles of the image:
//   CT = 4 (from 256 column tiles on: qkv, gate_up)  wave w owns column tile 4 bx + w over the whole k range;
//   CT = 2 (below: o, down)                          wave w owns column tile 2 bx + (w >> 1) and the k64-steps of parity
//                                                    w & 1; the two partial accumulators meet in LDS, part 0 + part 1.
// No k split across blocks, no workspace, no atomics, no reduce launch: the same input gives the same bytes.
//
// The k parts of the CT = 2 form are the even and the odd k64-steps, not the lower and the upper half of k: a stage of the
// activation is then ONE contiguous run of 128 columns per row (256 bytes, two pieces per thread in the same row) in
// place of two runs K / 2 apart, and the two waves of a column tile walk the same 4 KiB of the image at the same time.
//
// Weights: a wave streams its column tile straight from HBM into a register ring, TILE_RING stages (2 KiB each, plus the
// lane's {scale, 1024 + z + 1} word of either 16-row part) ahead, each slot refilled in place once it is consumed.  ONE
// 32x16 B fragment is dequantised at a time (dequant8: one rounding per weight, the bits of tgis_gptq8_dequant_f16) and fed
// to NB MFMAs before the next: a matrix's bytes are read, and its dequantisation paid, once per 32 NB rows.
//
// Activation: the block stages the tile's rows of every stage (one k64-step per k part: 64 or 128 columns — the unit the
// weight ring advances by, so that one barrier serves both; a 256-column chunk would double the 64 KiB of the 128-row CT = 2
// form) once into double-buffered LDS in A-fragment order (fragment i of lane l: row l & 31, columns (l >> 5) * 32 + i * 8
// .. + 8 of the k64-step), so a wave's read is one 16-byte LDS load per MFMA at lane * 16.  Rows past M and columns at or past
// K are staged as zero by a select (a pad byte of the image dequantises to -(z + 1) s, not 0); with PERM the gather of an
// act-order matrix happens here, -1 (a pad row of a padded row shard) reads 0.  One barrier per stage.
//
// Bounds: weight steps are clamped to the image's last real k64-step and groups to G - 1 (what they multiply is staged as
// zero), waves past the last column tile recompute it and never store, x rows are read only below M and columns only below
// K, stores are masked by m < M and n < N.
#pragma once

namespace gptq8 {

struct TileArgs {
    const f16* x;
    int64_t ldx;
    const uint8_t* prep;
    int64_t offB;
    const f16* bias;
    const int32_t* perm;
    f16* out;
    int64_t ldo;
    int M, K, N, G;
    uint32_t gmagic;  // group_magic
    int NT, KS, KSS;
};

// stages of weights a wave keeps in flight: the decode kernel's depth (8 KiB per wave)
#ifndef TGIS_GPTQ8_TILE_RING
#define TGIS_GPTQ8_TILE_RING 4
#endif
constexpr int TILE_RING = TGIS_GPTQ8_TILE_RING;
constexpr int TILE_THREADS = 256;

template <int NB, int CT, bool PERM>
__global__ __launch_bounds__(TILE_THREADS) void gptq8_tile_gemm_kernel(TileArgs a) {
    static_assert((NB == 2 || NB == 4) && (CT == 2 || CT == 4), "row tiles of 64 / 128 rows, 64 / 128 columns per block");
    constexpr int KP = 4 / CT;               // k parts: k64-steps per stage
    constexpr int FRAG = 4 * 64 * 8;         // halves of one 32-row block of one k64-step in A-fragment order (4 KiB)
    constexpr int BUF = NB * KP * FRAG;      // halves per stage buffer
    static_assert((size_t)(KP - 1) * CT * NB * 64 * 16 * sizeof(float) <= (size_t)2 * BUF * sizeof(f16), "finish fits");
    __shared__ __attribute__((aligned(16))) f16 xs[2 * BUF];  // [buffer][32-row block][k part][i][lane][8]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kp = KP == 2 ? (wv & 1) : 0, ct = KP == 2 ? (wv >> 1) : wv;
    const int nt_raw = blockIdx.x * CT + ct;
    const int nt = min(nt_raw, a.NT - 1);
    const int row0 = blockIdx.y * (32 * NB);
    const int nstages = (a.KS + KP - 1) / KP;  // block-uniform

    // ---- weights: ring slot <- k64-step (clamped into the image: a step past K multiplies a zero activation) ----
    const uint8_t* wtile = a.prep + (int64_t)nt * a.KSS * 2048 + lane * 16;
    const uint32_t* sztile = reinterpret_cast<const uint32_t*>(a.prep + a.offB) + (int64_t)nt * a.G * 32 + (lane & 31);
    u32x4 wq[TILE_RING][2];
    uint32_t szr[TILE_RING][2];
    auto ring_load = [&](int slot, int stage) {
        const int ks = min(stage * KP + kp, a.KS - 1);
        const uint8_t* p = wtile + (int64_t)ks * 2048;
        wq[slot][0] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        wq[slot][1] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p + 1024));
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2) {
            const uint32_t k = (uint32_t)(ks * 64 + (lane >> 5) * 32 + p2 * 16);
            const int g = min((int)__umulhi(k, a.gmagic), a.G - 1);
            szr[slot][p2] = sztile[(int64_t)g * 32];
        }
    };

    // ---- activation: thread -> row gm of each 32-row block, the 8 columns gq * 8 .. + 8 of each k64-step of the stage ----
    const int gm = (tid & 7) + 8 * (tid >> 6), gq = (tid >> 3) & 7;
    const int gdst = (((gq & 3) * 64) + (gq >> 2) * 32 + gm) * 8;
    const f16* grow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int m = row0 + j * 32 + gm;
        grow[j] = m < a.M ? a.x + (int64_t)m * a.ldx : nullptr;
    }
    f16x8 g[NB][KP];
    auto gather = [&](int stage) {
        const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int s2 = 0; s2 < KP; ++s2) {
            const int kk = (stage * KP + s2) * 64 + gq * 8;
            const bool inside = kk < a.K;  // K % 8 == 0: a piece is whole or absent
            int src[8];
            if (PERM) {
#pragma unroll
                for (int e = 0; e < 8; ++e) src[e] = inside ? a.perm[kk + e] : -1;
            }
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                f16x8 v = zero;
                if (grow[j] != nullptr) {
                    if (!PERM) {
                        if (inside) v = ld16<f16x8>(grow[j] + kk);
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            if (src[e] >= 0) v[e] = grow[j][src[e]];
                    }
                }
                g[j][s2] = v;
            }
        }
    };
    auto stage_store = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int s2 = 0; s2 < KP; ++s2) st16(xs + buf * BUF + (j * KP + s2) * FRAG + gdst, g[j][s2]);
    };

    uint32_t EXr = 0x64646464u;
    asm volatile("" : "+v"(EXr));
    f32x16 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

    // the (L2-resident) first stage of x goes out before the HBM weight stream it would otherwise queue behind
    gather(0);
#pragma unroll
    for (int s = 0; s < TILE_RING; ++s) ring_load(s, s);
    stage_store(0);
    __syncthreads();
    for (int t0 = 0; t0 < nstages; t0 += TILE_RING) {
#pragma unroll
        for (int r = 0; r < TILE_RING; ++r) {
            const int t = t0 + r;
            if (t < nstages) {  // (block-uniform: every wave meets the barrier below)
                const bool more = t + 1 < nstages;
                if (more) gather(t + 1);
                const f16* xa = xs + (t & 1) * BUF + kp * FRAG + lane * 8;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const u32x4 cur = wq[r][i >> 1];
                    const f16x2 szh = __builtin_bit_cast(f16x2, szr[r][i >> 1]);
                    const f16 nz1 = -szh[1];
                    const f16x2 nz = {nz1, nz1}, sc = {szh[0], szh[0]};
                    const f16x8 b = dequant8(cur[2 * (i & 1)], cur[2 * (i & 1) + 1], nz, sc, EXr);
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        acc[j] = mfma32(*reinterpret_cast<const f16x8*>(xa + j * KP * FRAG + i * 512), b, acc[j]);
                }
                ring_load(r, t + TILE_RING);  // the slot is consumed: refill it in place
                if (more) stage_store((t + 1) & 1);  // (that buffer was last read before the previous barrier)
                __syncthreads();
            }
        }
    }

    // ---- finish: part 1 of a column tile leaves its accumulators in LDS (the x buffers are dead after the last barrier),
    // part 0 adds them to its own (part 0 + part 1) and stores ----
    if constexpr (KP == 2) {
        float* red = reinterpret_cast<float*>(xs) + (((ct * NB) * 64 + lane) << 4);  // [ct][NB][64 lanes][16]
        if (kp == 1) {
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int r = 0; r < 16; r += 4)
                    *reinterpret_cast<f32x4*>(red + j * 1024 + r) = f32x4{acc[j][r], acc[j][r + 1], acc[j][r + 2], acc[j][r + 3]};
        }
        __syncthreads();
        if (kp == 1) return;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; r += 4) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(red + j * 1024 + r);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][r + e] += o[e];
            }
    }
    if (nt_raw >= a.NT) return;
    // accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
    const int n = nt * 32 + (lane & 31);
    if (n >= a.N) return;
    const float bv = a.bias ? (float)a.bias[n] : 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = row0 + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            if (m < a.M) a.out[(int64_t)m * a.ldo + n] = (f16)(acc[j][r] + bv);
        }
}

// Tile height: 64-row tiles up to TILE_ROWS64_MAX rows (twice the blocks on a grid that does not fill the device), 128-row
// tiles above (a fragment's dequantisation and its bytes serve twice the rows).  The macro is the switch of the sweep in
// the 128-column form changes over between 128 and 256 rows (45 against 60 us at 128 rows of qkv, 57 / 60
// at 256, 178 / 153 at 1024); the 64-column form would prefer 64-row tiles up to 512 rows and was left on the same rule.
#ifndef TGIS_GPTQ8_TILE_ROWS64_MAX
#define TGIS_GPTQ8_TILE_ROWS64_MAX 128
#endif
static inline int tile_blocks(int64_t M) { return M <= TGIS_GPTQ8_TILE_ROWS64_MAX ? 2 : 4; }

}  // namespace gptq8

namespace {

template <int NB, int CT, bool PERM>
int tile_launch(const gptq8::TileArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((gptq8::gptq8_tile_gemm_kernel<NB, CT, PERM>),
                       dim3((unsigned)cdiv64(a.NT, CT), (unsigned)cdiv64(a.M, 32 * NB)), dim3(gptq8::TILE_THREADS), 0, st, a);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

}  // namespace

extern "C" int tgis_gptq8_tile_gemm_f16(const void* x, int64_t ldx, const void* prepared, const void* bias, const int32_t* perm,
                                        void* out, int64_t ldo, int64_t M, int64_t K, int64_t N, int64_t groups, void* stream) {
    const char* fn = "tgis_gptq8_tile_gemm_f16";
    TGIS_CHECK_ARG(x && prepared && out, "%s: null tensor", fn);
    TGIS_CHECK_ARG(M >= 1 && M <= (int64_t)1 << 21, "%s: serves 1 <= M <= 2^21 rows (M=%ld)", fn, (long)M);
    const int rc = check_shape(fn, K, N, groups);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ldx >= 0 && ldo >= N,
                   "%s: x needs 16-byte aligned rows, out rows of at least N elements", fn);
    const PrepLayout p = prep_layout(K, N, groups);
    gptq8::TileArgs a;
    a.x = (const f16*)x;
    a.ldx = ldx;
    a.prep = (const uint8_t*)prepared;
    a.offB = p.offB;
    a.bias = (const f16*)bias;
    a.perm = perm;
    a.out = (f16*)out;
    a.ldo = ldo;
    a.M = (int)M, a.K = (int)K, a.N = (int)N, a.G = (int)groups;
    a.gmagic = gptq8::group_magic(K, groups);
    a.NT = (int)p.NT, a.KS = (int)p.KS, a.KSS = (int)p.KSS;
    hipStream_t st = (hipStream_t)stream;
    TgisTimedScope timed(TGIS_OP_GPTQ_GEMM, st);
    return by_int<2, 4>(gptq8::tile_blocks(M), "tgis_gptq8_tile_gemm_f16: tile height", [&](auto nb) {
        return by_bool(p.NT >= 256, [&](auto wide) {
            return by_bool(perm != nullptr, [&](auto pm) {
                constexpr int NB = decltype(nb)::value, CT = decltype(wide)::value ? 4 : 2;
                return tile_launch<NB, CT, decltype(pm)::value>(a, st);
            });
        });
    });
}

// Largest M tgis_gptq8_tile_gemm_f16 should be given for this matrix in place of tgis_gptq8_dequant_f16 + a library GEMM; 64 =
// never (up to 64 rows belong to tgis_gptq8_gemm_f16).  Host only.  Set from profiles/gptq8_tiles_bench.jsonl (DESIGN.md
// section 6): per column form and per plain / act-order, the largest measured M up to which the tile launch is faster by more
// than the spread between repeats on every shape of the class.
extern "C" int64_t tgis_gptq8_tile_rows(int64_t K, int64_t N, int64_t groups, int act_order) {
    if (K <= 0 || N <= 0 || groups <= 0) return 64;
    const bool wide = cdiv64(N, 32) >= 256;
    // 128-column form, plain: 0.87 / 0.77 of the other path at 512 rows (qkv / gate_up of Llama-2-7B), 1.20 / 1.01 at 1024.
    // 64-column form: faster at 128 rows only (down_proj is 1.20 at 65 and 1.54 at 256).  Act-order: 1.6 - 26 times slower
    // everywhere — every column block repeats the element-wise gather of its row tile.
    return wide && !act_order ? 512 : 64;
}
