// The 8-bit GPTQ decode GEMM (1 <= M <= 64): image layout, byte dequantisation, launch plan and the kernel body; the
// kernels and the C ABI around it are in gptq8.hip.
//
// Replaces the Triton QuantLinear that the reference gives every GPTQ width but 4 (utils/gptq/quant_linear.py:130-192,259).
// Normative arithmetic (the same lines): W[k,n] = f16((q[k,n] - (z[g(k),n] + 1)) * s[g(k),n]) with q, z unsigned bytes and
// z + 1 NOT masked back to a byte (a stored 255 is a zero point of 256); y = x @ W, fp32 accumulate, f16 out.
//
// Prepared image, NT = ceil(N/32) column tiles, KS = ceil(K/64) k64-steps (+ one zero pad step per tile,
// so that the tile stride is no multiple of 64 KiB), G groups:
//   A: w8 [NT][KS + 1][2 parts][64 lanes][16 bytes]: lane l of part p holds the bytes of rows
//        k = 64 ks + 32 (l >> 5) + 16 p + 0..15 of column n = 32 nt + (l & 31).  A wave load is one contiguous KiB; bytes
//        8 (i & 1) .. +8 of part i >> 1 are, after dequantisation, the B fragment of the i-th v_mfma_f32_32x32x16_f16 of the
//        step in natural k order (the k order of the int4 image and of the staged activation).
//   B: sz [NT][G][32] u32 = { scale f16, (1024 + z + 1) f16 } — the int4 image's pair (1024 + 256 is an f16).
// Rows are pre-permuted by the act-order permutation when g_idx is not trivial.
#pragma once
#include <algorithm>
#include <type_traits>
#include "common.h"

namespace gptq8 {

struct PrepLayout {
    int64_t NT, KS, KSS, G, offB, total;  // KS real k64-steps, KSS = steps between tiles
};
static inline PrepLayout prep_layout(int64_t K, int64_t N, int64_t G) {
    PrepLayout p;
    p.NT = cdiv64(N, 32);
    p.KS = cdiv64(K, 64);
    p.KSS = p.KS + 1;
    p.G = G;
    p.offB = p.NT * p.KSS * 2048;
    p.total = (p.offB + p.NT * G * 128 + 255) & ~int64_t(255);
    return p;
}

// floor(k / gs) for 0 <= k < K as one v_mul_hi_u32: exact while K * gs < 2^32 (checked by the host); 0 = a single group
static inline uint32_t group_magic(int64_t K, int64_t groups) {
    return groups == 1 ? 0u : (uint32_t)(((uint64_t)1 << 32) / (uint64_t)(K / groups) + 1);
}

// 8 bytes of q (two dwords, natural k order) -> 8 halves (q - (z + 1)) * s.  v_perm_b32 drops each byte under the exponent
// of 1024.0 (0x6400 | q = 1024 + q exactly); adding nz = -(1024 + z + 1) is exact (the result lies in -256..255); the
// product with the f16 scale is the single rounding — the same value as rounding the exact product in fp32.
__device__ __forceinline__ f16x8 dequant8(uint32_t q0, uint32_t q1, f16x2 nz, f16x2 sc, uint32_t EX) {
    const uint32_t a0 = __builtin_amdgcn_perm(EX, q0, 0x04010400u);  // bytes {q.0, 0x64, q.1, 0x64}
    const uint32_t a1 = __builtin_amdgcn_perm(EX, q0, 0x04030402u);
    const uint32_t a2 = __builtin_amdgcn_perm(EX, q1, 0x04010400u);
    const uint32_t a3 = __builtin_amdgcn_perm(EX, q1, 0x04030402u);
    const f16x2 h0 = (__builtin_bit_cast(f16x2, a0) + nz) * sc;
    const f16x2 h1 = (__builtin_bit_cast(f16x2, a1) + nz) * sc;
    const f16x2 h2 = (__builtin_bit_cast(f16x2, a2) + nz) * sc;
    const f16x2 h3 = (__builtin_bit_cast(f16x2, a3) + nz) * sc;
    const u32x4 packed = {__builtin_bit_cast(uint32_t, h0), __builtin_bit_cast(uint32_t, h1),
                          __builtin_bit_cast(uint32_t, h2), __builtin_bit_cast(uint32_t, h3)};
    return __builtin_bit_cast(f16x8, packed);
}

struct GemmArgs {
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
    int KR, S;        // k range of a block (multiple of 256), global k splits
    int NT, KS, KSS;
    float* slabs;     // S > 1: [ceil(M/32)][S][32][NT*32] f32 partial sums, the layout gptq::reduce_slabs sums
};

constexpr int KC = 256;     // k per LDS chunk of x (4 k64-steps)
constexpr int RS = KC + 8;  // LDS row stride in halves (+16 B: conflict-free ds_read_b128 of A fragments)
constexpr int RING = 4;     // k64-steps (2 KiB each) a wave keeps in flight

constexpr size_t lds_bytes(int tn, int wk, int mr) {
    const size_t xb = (size_t)2 * 32 * mr * RS * sizeof(f16), red = (size_t)wk * tn * mr * 64 * 16 * sizeof(float);
    return xb > red ? xb : red;
}

// A block of TN * WK = 8 waves owns 32 TN columns x [split KR, (split + 1) KR) of W, all M rows.  Every 256-row chunk of x
// (gathered by perm, SiLU * up applied for ACT 1, zero past the block's k range) is staged once through LDS by the whole
// block, double-buffered, one barrier per chunk; wave (wn, wk) = (w / WK, w % WK) streams column tile wn and the 4 / WK
// k64-steps wk * (4 / WK) .. of every chunk straight from HBM into registers, RING steps (8 KiB) ahead, each slot refilled
// in place as soon as it is consumed.  One dequantised fragment feeds MR MFMAs (rows 0-31, 32-63).  The WK partial
// accumulators are summed through LDS in fixed order; S > 1 leaves fp32 slabs for the reduce launch.  Bounds: weight and
// {scale, zero} addresses are clamped into the image, x rows to M - 1 and x columns to K - 8; stores are masked by
// m < M, n < N.
template <int TN, int WK, int ACT, bool PERM, int MR>
__device__ __forceinline__ void gemm_unit(const GemmArgs& a, unsigned char* smem) {
    static_assert(TN * WK == 8 && (WK == 2 || WK == 4), "blocks are 8 waves");
    constexpr int SPC = 4 / WK;          // k64-steps of a chunk per wave
    constexpr int U = RING / SPC;        // chunks the ring spans
    constexpr int XR = 32 * MR;          // x rows
    constexpr int NTHR = 64 * TN * WK;
    constexpr int NJ = XR * 32 / NTHR;   // 16-byte x pieces per thread and chunk
    constexpr int RSTEP = NTHR / 32;     // rows between a thread's pieces
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = w / WK, wk = w % WK;
    const int split = blockIdx.y;
    const int kb0 = split * a.KR, kb1 = min(a.K, kb0 + a.KR);
    const int nchunks = max(1, (kb1 - kb0 + KC - 1) / KC);  // block-uniform
    const int nt_raw = blockIdx.x * TN + wn;
    const int nt = min(nt_raw, a.NT - 1);  // waves past the last tile recompute it and never store
    f16* xs = reinterpret_cast<f16*>(smem);  // [2][XR][RS]

    const uint8_t* wtile = a.prep + (int64_t)nt * a.KSS * 2048 + lane * 16;
    const uint32_t* sztile = reinterpret_cast<const uint32_t*>(a.prep + a.offB) + (int64_t)nt * a.G * 32 + (lane & 31);
    const int ks_first = kb0 >> 6;
    const int ks_clamp = max(ks_first, min(a.KS, (kb1 + 63) >> 6) - 1);  // last step with rows of this block
    auto ks_of = [&](int chunk, int s2) { return min(ks_first + chunk * 4 + wk * SPC + s2, ks_clamp); };  // <= KS - 1
    u32x4 wq[RING][2];
    uint32_t szr[RING][2];
    auto ring_load = [&](int slot, int ks) {
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

    // ---- x staging: thread t holds rows (t / 32) + RSTEP j, 16-byte column piece t % 32 of the chunk ----
    const int srow = tid >> 5, scol = (tid & 31) * 8;
    f16x8 xg[NJ], xu[ACT == 1 ? NJ : 1];
    int64_t rowoff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) rowoff[j] = (int64_t)min(srow + RSTEP * j, a.M - 1) * a.ldx;
    auto stage_load = [&](int chunk) {
        const int kreal = kb0 + chunk * KC + scol;
        const bool valid = kreal < kb1;  // K % 8 == 0: a piece is whole or absent
        const int kc = min(kreal, a.K - 8);
        const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const f16* xr = a.x + rowoff[j];
            f16x8 v = zero, u = zero;
            if (!PERM) {
                v = ld16<f16x8>(xr + kc);
                if (ACT == 1) u = ld16<f16x8>(xr + a.K + kc);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int ksrc = a.perm[kc + e];  // -1: a pad row of an act-order row shard (utils/weights.py) reads 0
                    v[e] = ksrc >= 0 ? xr[ksrc] : (f16)0.f;
                    if (ACT == 1) u[e] = ksrc >= 0 ? xr[a.K + ksrc] : (f16)0.f;
                }
            }
            xg[j] = valid ? v : zero;  // a select, not a product: what lies past the range may be anything
            if (ACT == 1) xu[j] = valid ? u : zero;
        }
    };
    auto stage_store = [&](int buf) {
        f16* dst = xs + buf * (XR * RS) + srow * RS + scol;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            f16x8 t = xg[j];
            if (ACT == 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float gte = (float)t[e];
                    const float sl = gte / (1.f + __expf(-gte));
                    // the reference rounds silu(gate) to f16 before the multiply (eager torch ops)
                    t[e] = (f16)((float)(f16)sl * (float)xu[j][e]);
                }
            }
            st16(dst + j * RSTEP * RS, t);
        }
    };

    uint32_t EXr = 0x64646464u;
    asm volatile("" : "+v"(EXr));
    f32x16 acc[MR];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr) acc[mr] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int xoff = (lane & 31) * RS + (lane >> 5) * 32;

    // the (L2-resident) first x chunk goes out before the HBM weight stream it would otherwise queue behind
    stage_load(0);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int s2 = 0; s2 < SPC; ++s2) ring_load(u * SPC + s2, ks_of(u, s2));
    stage_store(0);
    __syncthreads();

    auto chunk_body = [&](const int chunk, auto sb_tag) {
        constexpr int SB = decltype(sb_tag)::value;
        const bool more = chunk + 1 < nchunks;  // block-uniform
        if (more) stage_load(chunk + 1);
        const f16* xbuf = xs + (chunk & 1) * (XR * RS) + xoff + wk * SPC * 64;
#pragma unroll
        for (int s2 = 0; s2 < SPC; ++s2) {
            f16x8 b[4];
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2) {
                const u32x4 cur = wq[SB + s2][p2];
                const f16x2 szh = __builtin_bit_cast(f16x2, szr[SB + s2][p2]);
                const f16 nz1 = -szh[1];
                const f16x2 nz = {nz1, nz1}, sc = {szh[0], szh[0]};
                b[2 * p2] = dequant8(cur[0], cur[1], nz, sc, EXr);
                b[2 * p2 + 1] = dequant8(cur[2], cur[3], nz, sc, EXr);
            }
            ring_load(SB + s2, ks_of(chunk + U, s2));  // the slot is consumed: refill it in place
            const f16* xk = xbuf + s2 * 64;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int mr = 0; mr < MR; ++mr) {
                    const f16x8 av = ld16<f16x8>(xk + mr * (32 * RS) + i * 8);
                    acc[mr] = mfma32(av, b[i], acc[mr]);
                }
        }
        if (more) stage_store((chunk + 1) & 1);
        __syncthreads();
    };
    for (int chunk = 0; chunk < nchunks; chunk += U) {
        chunk_body(chunk, std::integral_constant<int, 0>{});
        if constexpr (U > 1) {
            if (chunk + 1 < nchunks) chunk_body(chunk + 1, std::integral_constant<int, SPC>{});
        }
        if constexpr (U > 2) {
            if (chunk + 2 < nchunks) chunk_body(chunk + 2, std::integral_constant<int, 2 * SPC>{});
            if (chunk + 3 < nchunks) chunk_body(chunk + 3, std::integral_constant<int, 3 * SPC>{});
        }
    }

    // ---- finish: the WK k-parts meet in LDS (the x buffers are dead after the last barrier); wave (wn, wk) sums registers
    // [wk NR, (wk + 1) NR) of tile wn over the k-parts in the fixed order 0..WK-1 and stores those rows ----
    constexpr int NR = 16 / WK;
    float* red = reinterpret_cast<float*>(smem);  // [WK][TN][MR][64 lanes][16]
#pragma unroll
    for (int mr = 0; mr < MR; ++mr) {
        float* dst = red + ((((wk * TN + wn) * MR + mr) * 64 + lane) << 4);
#pragma unroll
        for (int r = 0; r < 16; r += 4)
            *reinterpret_cast<f32x4*>(dst + r) = f32x4{acc[mr][r], acc[mr][r + 1], acc[mr][r + 2], acc[mr][r + 3]};
    }
    __syncthreads();
    if (nt_raw >= a.NT) return;
    float fin[MR][NR];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int k2 = 0; k2 < WK; ++k2) {
            const float* src = red + ((((k2 * TN + wn) * MR + mr) * 64 + lane) << 4) + wk * NR;
#pragma unroll
            for (int j = 0; j < NR; j += 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(src + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) fin[mr][j + e] = k2 == 0 ? t[e] : fin[mr][j + e] + t[e];
            }
        }
    const int n = nt * 32 + (lane & 31);
    auto row_of = [&](int j) {  // row (within the 32-row block) of finished register j
        const int r = wk * NR + j;
        return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    };
    if (a.S == 1) {
        if (n >= a.N) return;
        const float bv = a.bias ? (float)a.bias[n] : 0.f;
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int m = mr * 32 + row_of(j);
                if (m < a.M) a.out[(int64_t)m * a.ldo + n] = (f16)(fin[mr][j] + bv);
            }
    } else {
        const int64_t np = (int64_t)a.NT * 32;
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
            float* sl = a.slabs + ((int64_t)(mr * a.S + split) * 32) * np + n;
#pragma unroll
            for (int j = 0; j < NR; ++j) sl[(int64_t)row_of(j) * np] = fin[mr][j];
        }
    }
}

struct GemmPlan {
    int KR, S, WK, TN, MR;  // rows per block, global k splits, in-block k-parts, column tiles per block, 32-row blocks of x
};

// Derived, not swept: blocks of 8 waves — 128 columns x 2 k-parts from 256 column tiles on (qkv, gate_up), 64 columns x 4
// k-parts below (o, down: the in-block parts cost no slab traffic) — and global k splits until about 384 blocks (1.5 per
// CU, 12 waves of 8 KiB in flight each), every split at least two chunks deep.
static inline GemmPlan plan_gemm(int64_t K, int64_t N, int64_t M) {
    const int64_t tiles = cdiv64(N, 32), kchunks = cdiv64(K, KC);
    const int TN = tiles >= 256 ? 4 : 2, WK = 8 / TN;
    const int64_t colblocks = cdiv64(tiles, TN);
    int64_t S = std::max<int64_t>(1, std::min<int64_t>(kchunks / 2, (384 + colblocks / 2) / colblocks));
    const int64_t per = cdiv64(kchunks, S);
    S = cdiv64(kchunks, per);  // no empty last split
    return {(int)(per * KC), (int)S, WK, TN, M > 32 ? 2 : 1};
}

static inline int64_t slab_bytes(int64_t M, int64_t N, int S) {
    return S > 1 ? cdiv64(M, 32) * S * 32 * cdiv64(N, 32) * 32 * 4 : 0;
}

}  // namespace gptq8
