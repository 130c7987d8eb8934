// Routed expert MLP (Mixtral: a router plus E expert MLPs, top_k of them per token), gfx950 MFMA 32x32x16.
//
//   tgis_moe_route      fp32 router logits [T, E] -> the top_k experts and weights of every token, and the slots
//                       (t * top_k + k) grouped by expert: counts, offsets, slot_rows.  Integer work only for the lists.
//   tgis_moe_gemm_up    h[slot] = T(T(silu(T gate)) * T up) of the slot's token under the slot's expert (act 2's rounding)
//   tgis_moe_gemm_down  y[slot] = (h[slot] @ W2[expert]^T) * expert_w[slot], left as one fp32 slab per k-th choice
//                       (decode form: a native.Partial the next add + RMSNorm finishes) or summed over k in fixed order.
//
// The expert GEMMs read the routing on the device: their grid is (column tiles, E), whatever the routing, so the launches
// can sit in a captured decode graph.  A block owns ONE 32-column tile of ONE expert; it reads offsets[e], returns at once
// when nobody chose the expert (no weight traffic: the reason for these kernels) and otherwise walks the expert's rows in
// 32-row slabs.  Its four waves split the k range; the k-parts are summed through LDS in the fixed order 0..3 and wave wk
// finishes accumulator registers [4 wk, 4 wk + 4).  No float atomics, no cross-block waiting: the same input gives the same
// bytes.
//
// Expert weights are E images of tgis_dense_prepare (dense_gemm_body.h's layout: [NT][KS][4][64 lanes][8 elements], zero
// padded past K and N) at a fixed byte stride: gate|up images with flags bit 0 (a (gate, up) pair sits 16 lanes apart in
// one wave), down images plain.  mfma32, finish_out and the SiLU * up rounding are the dense unit's, by inclusion.
//
//   tgis_moe_gptq_gemm_up / _down  the same two launches over E int4 images of tgis_gptq_prepare (gptq_gemm_body.h's
//                       layout: nibbles [NT][KS'][64 lanes][4 words], then {scale, 1024 + z + 1} pairs [NT][G][32]).  The
//                       kernel is the one above with another weight source: a wave loads 1 KiB per k64-step, dequantises it
//                       with the int4 unit's dequant8 (one rounding to f16) and feeds the same MFMAs; the slab walk, the LDS
//                       exchange and the epilogues are shared.  f16, K a multiple of 64, groups of 64 * 2^n rows or one group.
#include <algorithm>
#include "common.h"
#include "dispatch.h"
#include "dense_gemm_body.h"
#include "gptq_gemm_body.h"

namespace {

constexpr int MOE_WK = 4;        // k-parts (waves) per block
constexpr int MOE_RING = 4;      // k64-steps of weights a wave keeps in flight (4 x 4 KiB)
// The int4 images' ring.  A step is 1 KiB there, a quarter of the dense ring's bytes in flight at the same depth, but 4 / 8 /
// 16 swept with tools/bench_mixtral.py --quantize gptq --ring measured 4 fastest at B 1, 8 and 32: the registers of a deeper
// ring cost a wave per SIMD each time (3 / 2 / 1 waves), which hides more latency than the ring does.
// The macro is that sweep's switch.
#ifndef TGIS_MOE_GPTQ_RING
#define TGIS_MOE_GPTQ_RING 4
#endif
constexpr int MOE_GPTQ_RING = TGIS_MOE_GPTQ_RING;
static_assert(MOE_GPTQ_RING == 4 || MOE_GPTQ_RING == 8 || MOE_GPTQ_RING == 16, "the int4 ring is 4, 8 or 16 k64-steps");
constexpr int MOE_THREADS = 64 * MOE_WK;
constexpr int MOE_LDS = MOE_WK * 64 * 16 * 4;  // the k-part exchange: [WK][64 lanes][16] fp32
constexpr int ROUTE_THREADS = 1024;
constexpr int MOE_MAX_E = 64, MOE_MAX_TOPK = 8;

// ---- routing -------------------------------------------------------------------------------------------------------------
// One block.  Phase 1, a token per thread: softmax over all E, the top_k largest (ties to the lower index), those
// renormalised to sum 1 — transformers' MixtralTopKRouter.  The arithmetic runs in fp64 and is rounded to fp32 once, so each
// weight is the correctly rounded value of what the fp32 sequence approximates.  Phase 2, an expert per wave: the slots that
// chose it are counted (ballot + popcount), offsets are the exclusive prefix sum, and a second walk writes the slots in
// ascending order behind offsets[e].
__global__ __launch_bounds__(ROUTE_THREADS) void moe_route_kernel(const float* __restrict__ logits, int64_t ld, int T, int E,
                                                                 int top_k, int32_t* __restrict__ expert_ids,
                                                                 float* __restrict__ expert_w, int32_t* __restrict__ counts,
                                                                 int32_t* __restrict__ offsets,
                                                                 int32_t* __restrict__ slot_rows) {
    __shared__ int s_cnt[MOE_MAX_E];
    __shared__ int s_off[MOE_MAX_E + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int t = tid; t < T; t += ROUTE_THREADS) {
        const float* row = logits + (int64_t)t * ld;
        float mx = row[0];
        for (int e = 1; e < E; ++e) mx = fmaxf(mx, row[e]);
        double sum = 0.0;
        for (int e = 0; e < E; ++e) sum += exp((double)row[e] - (double)mx);
        uint64_t taken = 0;
        int ids[MOE_MAX_TOPK];
        double pk[MOE_MAX_TOPK];
        double psum = 0.0;
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k) {
            if (k >= top_k) break;
            int best = -1;
            float bestp = 0.f;
            double bestd = 0.0;
            for (int e = 0; e < E; ++e) {
                if ((taken >> e) & 1) continue;
                const double pd = exp((double)row[e] - (double)mx) / sum;
                const float p = (float)pd;  // the order is decided on the fp32 probabilities, as torch.topk sees them
                if (best < 0 || p > bestp) best = e, bestp = p, bestd = pd;
            }
            taken |= 1ull << best;
            ids[k] = best;
            pk[k] = bestd;
            psum += bestd;
        }
#pragma unroll
        for (int k = 0; k < MOE_MAX_TOPK; ++k) {
            if (k >= top_k) break;
            expert_ids[(int64_t)t * top_k + k] = ids[k];
            expert_w[(int64_t)t * top_k + k] = (float)(pk[k] / psum);
        }
    }
    __syncthreads();  // the ids are read back below by other threads of this block
    const int nslots = T * top_k;
    for (int e = wave; e < E; e += ROUTE_THREADS / 64) {
        int c = 0;
        for (int base = 0; base < nslots; base += 64) {
            const int s = base + lane;
            const int id = s < nslots ? expert_ids[s] : -1;
            c += __popcll(__ballot(id == e));
        }
        if (lane == 0) s_cnt[e] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int e = 0; e < E; ++e) {
            s_off[e] = run;
            offsets[e] = run;
            counts[e] = s_cnt[e];
            run += s_cnt[e];
        }
        s_off[E] = run;
        offsets[E] = run;
    }
    __syncthreads();
    for (int e = wave; e < E; e += ROUTE_THREADS / 64) {
        int pos = s_off[e];
        for (int base = 0; base < nslots; base += 64) {
            const int s = base + lane;
            const int id = s < nslots ? expert_ids[s] : -1;
            const uint64_t m = __ballot(id == e);
            if (id == e) slot_rows[pos + __popcll(m & ((1ull << lane) - 1))] = s;
            pos += __popcll(m);
        }
    }
}

// ---- expert GEMMs ---------------------------------------------------------------------------------------------------------
struct MoeArgs {
    const void* x;            // UP: [T, K] activations; DOWN: h [T top_k, K]
    int64_t ldx;
    const uint8_t* images;    // E prepared images, `stride` bytes apart
    int64_t stride;
    const int32_t* offsets;   // [E + 1]
    const int32_t* slot_rows; // [T top_k]
    const float* expert_w;    // DOWN: [T top_k]
    void* out;                // UP: h [T top_k, N / 2], model dtype; DOWN: fp32 slabs (form 0) or fp32 [T top_k, N] (form 1)
    int64_t ldo;              // elements between output rows (form 0: the slab row stride)
    int K, N, NT, KS, top_k;
    int form;                 // DOWN: 0 slabs [T / 32][top_k][32][ldo], 1 one fp32 row per slot
    // int4 images only
    int KSI;                  // k64-steps a tile holds in the image (KS' of gptq::prep_layout: the real ones plus padding)
    int G, spg_shift;         // groups; log2(k64-steps per group), 30 under a single group
    int64_t offB;             // bytes from an image's start to its {scale, zero} table
};

// ---- weight sources: where a wave's B fragments of one k64-step come from ---------------------------------------------------
// A source is built once per wave for (expert, column tile, first k64-step); load(step, slot) asks for the step's bytes and
// frags(slot, b) turns them into the four 32x32x16 B fragments.

// 16-bit image of tgis_dense_prepare: 4 KiB per step, stored as fragments.
template <typename T>
struct DenseSource {
    using V8 = typename VecT<T>::x8;
    static constexpr int RING = MOE_RING;
    static constexpr int NACC = 2;  // accumulators the MFMAs of a step alternate between
    static constexpr int WAVES = 1;  // waves per SIMD the register allocation must leave room for
    struct Step {
        V8 v[4];
    };
    const char* tile;
    uint32_t woff;
    __device__ __forceinline__ DenseSource(const MoeArgs& a, int e, int nt, int ks0, int lane)
        : tile(reinterpret_cast<const char*>(a.images) + (int64_t)e * a.stride + ((int64_t)nt * a.KS + ks0) * 4096),
          woff(lane * 16) {}
    __device__ __forceinline__ void load(int step, Step& dst) const {
        const char* p = tile + (int64_t)step * 4096;
#pragma unroll
        for (int i = 0; i < 4; ++i) dst.v[i] = __builtin_nontemporal_load(reinterpret_cast<const V8*>(p + i * 1024 + woff));
    }
    __device__ __forceinline__ void frags(const Step& s, V8 (&b)[4]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = s.v[i];
    }
};

// int4 image of tgis_gptq_prepare (f16): 1 KiB of nibbles per step, one 16-byte load per lane, and the lane's column's
// {scale, 1024 + z + 1} pair of the step's group, asked for with the nibbles and kept with them in the ring.
struct Int4Source {
    using V8 = f16x8;
    static constexpr int RING = MOE_GPTQ_RING;
    // One accumulator, as the int4 unit of gptq_gemm_body.h: the dequantisation between two MFMAs covers their dependency,
    // and without the second one the kernel fits 128 registers — 4 waves per SIMD, which measured 8 - 18 % faster than 3
    // (DESIGN.md section 6).  A deeper ring does not fit and keeps the allocator's own choice.
    static constexpr int NACC = 1;
    static constexpr int WAVES = MOE_GPTQ_RING == 4 ? 4 : 1;
    struct Step {
        u32x4 q;
        uint32_t sz;
    };
    const char* tile;
    const char* sztile;
    uint32_t woff, szoff, EX, M0, M1;
    int ks0, spg_shift, G;
    __device__ __forceinline__ Int4Source(const MoeArgs& a, int e, int nt, int ks0_, int lane)
        : woff(lane * 16), szoff((lane & 31) * 4), EX(0x64006400u), M0(0x000F000Fu), M1(0x00F000F0u), ks0(ks0_),
          spg_shift(a.spg_shift), G(a.G) {
        const char* image = reinterpret_cast<const char*>(a.images) + (int64_t)e * a.stride;
        tile = image + ((int64_t)nt * a.KSI + ks0) * 1024;
        sztile = image + a.offB + (int64_t)nt * a.G * 128;
        asm volatile("" : "+v"(EX));  // dequant8 takes the exponent pair in a VGPR and the masks in SGPRs
        asm volatile("" : "+s"(M0), "+s"(M1));
    }
    __device__ __forceinline__ void load(int step, Step& dst) const {
        const int g = min((ks0 + step) >> spg_shift, G - 1);
        dst.sz = *reinterpret_cast<const uint32_t*>(sztile + (int64_t)g * 128 + szoff);
        dst.q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(tile + (int64_t)step * 1024 + woff));
    }
    __device__ __forceinline__ void frags(const Step& s, V8 (&b)[4]) const {
        const f16x2 szh = __builtin_bit_cast(f16x2, s.sz);
        const f16 zc1 = szh[1];
        const f16 zd1 = (f16)960.f - zc1;  // -(64 + z + 1), exact
        const f16x2 zc = {zc1, zc1}, zd = {zd1, zd1}, sc = {szh[0], szh[0]};
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = gptq::dequant8(s.q[i], zc, zd, sc, EX, M0, M1);
    }
};

// UP == true: gate|up image, SiLU * up epilogue, rows of x gathered through slot / top_k.
// UP == false: plain image, rows of h are the slots themselves, each finished row scaled by its expert_w in fp32.
// W: the weight source (DenseSource<T> or Int4Source).
template <typename T, bool UP, typename W>
__global__ __launch_bounds__(MOE_THREADS, W::WAVES) void moe_gemm_kernel(MoeArgs a) {
    using V8 = typename VecT<T>::x8;
    using WStep = typename W::Step;
    constexpr int RING = W::RING;
    __shared__ __attribute__((aligned(16))) float red[MOE_WK * 64 * 16];
    const int nt = blockIdx.x, e = blockIdx.y;
    const int row0 = a.offsets[e], cnt = a.offsets[e + 1] - row0;
    if (cnt <= 0) return;  // nobody chose this expert: not one byte of its image is read
    const int tid = threadIdx.x, lane = tid & 63;
    const int wk = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per = (a.KS + MOE_WK - 1) / MOE_WK;
    const int ks0 = min(wk * per, a.KS), ks1 = min(ks0 + per, a.KS);
    const int nsteps = ks1 - ks0;  // (may be 0 under a short K: the wave then contributes zeros)
    const W src_w(a, e, nt, ks0, lane);
    const int c = lane & 31, half_k = (lane >> 5) * 32;

    for (int slab = 0; slab * 32 < cnt; ++slab) {
        const int rows = min(32, cnt - slab * 32);
        // the lane's row of the A operand: rows past the expert's list repeat its last row (their sums are never stored)
        const int slot = a.slot_rows[row0 + slab * 32 + min(c, rows - 1)];
        const int src = UP ? slot / a.top_k : slot;
        const T* xrow = reinterpret_cast<const T*>(a.x) + (int64_t)src * a.ldx;
        auto x_load = [&](int step, V8* dst) {
            const int k = (ks0 + step) * 64 + half_k;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = k + i * 8;  // K % 8 == 0: eight columns are all inside K or all past it
                V8 v = ld16<V8>(xrow + min(kk, a.K - 8));
                if (kk >= a.K) {           // the image is zero there, the activation must be too (0 * NaN)
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
                }
                dst[i] = v;
            }
        };
        f32x16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
        WStep wq[RING];
        V8 xq[2][4];
        if (nsteps > 0) {
            x_load(0, xq[0]);
#pragma unroll
            for (int s = 0; s < RING; ++s)
                if (s < nsteps) src_w.load(s, wq[s]);
        }
        for (int s0 = 0; s0 < nsteps; s0 += RING) {
#pragma unroll
            for (int r = 0; r < RING; ++r) {
                const int s = s0 + r;
                if (s < nsteps) {
                    if (s + 1 < nsteps) x_load(s + 1, xq[(r + 1) & 1]);
                    V8 b[4];
                    src_w.frags(wq[r], b);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if ((i & 1) && W::NACC == 2) acc1 = mfma32(xq[r & 1][i], b[i], acc1);
                        else acc0 = mfma32(xq[r & 1][i], b[i], acc0);
                    }
                    if (s + RING < nsteps) src_w.load(s + RING, wq[r]);  // the slot is consumed: refill it in place
                }
            }
        }
        const f32x16 acc = W::NACC == 2 ? acc0 + acc1 : acc0;
        // ---- k-parts through LDS, summed in the fixed order 0..WK-1 ----------------------------------------------------
        __syncthreads();  // (the previous slab's exchange has been read)
        {
            float* dst = red + ((wk * 64 + lane) << 4);
#pragma unroll
            for (int r = 0; r < 16; r += 4)
                *reinterpret_cast<f32x4*>(dst + r) = f32x4{acc[r], acc[r + 1], acc[r + 2], acc[r + 3]};
        }
        __syncthreads();
        float fin[4];
#pragma unroll
        for (int k2 = 0; k2 < MOE_WK; ++k2) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(red + ((k2 * 64 + lane) << 4) + wk * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) fin[j] = k2 == 0 ? t[j] : fin[j] + t[j];
        }
        // accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = wk * 4 + j;
            const int m = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int oslot = a.slot_rows[row0 + slab * 32 + min(m, rows - 1)];
            if (UP) {
                // (gate, up) pairs sit 16 lanes apart: act 2's epilogue of dense_gemm_unit
                const int half = a.N >> 1, j2 = nt * 16 + (c & 15);
                const float mine = to_f32(from_f32<T>(fin[j]));
                const float other = __shfl_xor(mine, 16, 64);
                if (c < 16 && j2 < half && m < rows) {
                    const float sl = mine / (1.f + __expf(-mine));
                    reinterpret_cast<T*>(a.out)[(int64_t)oslot * a.ldo + j2] = from_f32<T>(to_f32(from_f32<T>(sl)) * other);
                }
            } else {
                const int n = nt * 32 + c;
                if (n < a.N && m < rows) {
                    const float v = fin[j] * a.expert_w[oslot];
                    float* o = reinterpret_cast<float*>(a.out);
                    if (a.form == 0) {
                        const int t = oslot / a.top_k, kth = oslot - t * a.top_k;
                        o[((int64_t)((t >> 5) * a.top_k + kth) * 32 + (t & 31)) * a.ldo + n] = v;
                    } else {
                        o[(int64_t)oslot * a.ldo + n] = v;
                    }
                }
            }
        }
    }
}

// Finished form: out[t] = T(sum over k of y[t top_k + k]) in the fixed order k = 0..top_k-1; a thread per 4 columns.
template <typename T>
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, T* __restrict__ out, int64_t ldo,
                                                          int64_t rows, int N, int top_k) {
    const int n4 = N >> 2;
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * n4) return;
    const int64_t t = idx / n4;
    const int c4 = (int)(idx - t * n4) * 4;
    const float* p = y + (t * top_k) * (int64_t)N + c4;
    f32x4 v = *reinterpret_cast<const f32x4*>(p);
    for (int k = 1; k < top_k; ++k) v += *reinterpret_cast<const f32x4*>(p + (int64_t)k * N);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[t * ldo + c4 + j] = dense::finish_out<T>(v[j], 0);
}

int moe_check_routing(const char* fn, int64_t T, int64_t E, int64_t top_k) {
    TGIS_CHECK_ARG(E >= 2 && E <= MOE_MAX_E, "%s: 2 <= E <= %d (E=%ld)", fn, MOE_MAX_E, (long)E);
    TGIS_CHECK_ARG(top_k >= 1 && top_k <= std::min<int64_t>(E, MOE_MAX_TOPK), "%s: 1 <= top_k <= min(E, %d) (top_k=%ld)", fn,
                   MOE_MAX_TOPK, (long)top_k);
    TGIS_CHECK_ARG(T >= 0 && T * top_k < (1ll << 31), "%s: T (%ld) must be >= 0 with T * top_k below 2^31", fn, (long)T);
    return TGIS_OK;
}

// G == 0: 16-bit images of tgis_dense_prepare; G >= 1: int4 images of tgis_gptq_prepare with G groups.
int moe_check_gemm(const char* fn, const void* x, int64_t ldx, const void* images, int64_t stride, const void* offsets,
                   const void* slot_rows, int64_t T, int64_t K, int64_t N, int64_t E, int64_t top_k, int dtype, int64_t G = 0) {
    const int rc = moe_check_routing(fn, T, E, top_k);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(x && images && offsets && slot_rows, "%s: null tensor", fn);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "%s: bad dtype", fn);
    TGIS_CHECK_ARG(K > 0 && N > 0 && K % 8 == 0 && K < (1ll << 30) && N < (1ll << 30), "%s: K (%ld) must be a positive multiple of 8, N (%ld) positive",
                   fn, (long)K, (long)N);
    TGIS_CHECK_ARG(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x % 16) == 0, "%s: rows of the activation must be 16-byte aligned", fn);
    const int64_t image_bytes = G == 0 ? cdiv64(N, 32) * cdiv64(K, 64) * 4096 : gptq::prep_layout(K, N, G).total;
    TGIS_CHECK_ARG(stride >= image_bytes && stride % 16 == 0 && ((uintptr_t)images % 16) == 0,
                   "%s: the expert stride (%ld) must hold one prepared image", fn, (long)stride);
    TGIS_CHECK_ARG(cdiv64(N, 32) <= 0x7fffffff / 32, "%s: N too large", fn);
    return TGIS_OK;
}

// The shapes the int4 weight source serves: whole k64-steps and column tiles, and a {scale, zero} pair per lane and step —
// one group, or groups of 64 * 2^n rows.  Groups of 32 rows and act-order permutations have no form here.
int moe_check_gptq_shape(const char* fn, int64_t K, int64_t N, int64_t G, int dtype) {
    TGIS_CHECK_ARG(dtype == TGIS_F16, "%s: int4 expert images are served in f16 only", fn);
    TGIS_CHECK_ARG(K > 0 && N > 0 && K % 64 == 0 && N % 32 == 0, "%s: K (%ld) must be a multiple of 64 and N (%ld) of 32", fn,
                   (long)K, (long)N);
    TGIS_CHECK_ARG(G >= 1 && K % G == 0, "%s: %ld groups do not divide K (%ld)", fn, (long)G, (long)K);
    const int64_t gs = K / G;
    TGIS_CHECK_ARG(G == 1 || (gs % 64 == 0 && ((gs / 64) & (gs / 64 - 1)) == 0),
                   "%s: groups of %ld rows are not served (one group, or 64 * 2^n rows)", fn, (long)gs);
    return TGIS_OK;
}

void moe_fill(MoeArgs& a, const void* x, int64_t ldx, const void* images, int64_t stride, const int32_t* offsets,
              const int32_t* slot_rows, const float* expert_w, void* out, int64_t ldo, int64_t K, int64_t N, int top_k,
              int form) {
    a.x = x, a.ldx = ldx, a.images = (const uint8_t*)images, a.stride = stride;
    a.offsets = offsets, a.slot_rows = slot_rows, a.expert_w = expert_w;
    a.out = out, a.ldo = ldo;
    a.K = (int)K, a.N = (int)N, a.NT = (int)cdiv64(N, 32), a.KS = (int)cdiv64(K, 64), a.top_k = top_k, a.form = form;
    a.KSI = 0, a.G = 0, a.spg_shift = 0, a.offB = 0;
}

// the int4 fields, for a shape moe_check_gptq_shape has admitted
void moe_fill_gptq(MoeArgs& a, int64_t K, int64_t N, int64_t G) {
    const gptq::PrepLayout p = gptq::prep_layout(K, N, G);
    a.KSI = (int)p.KS, a.G = (int)G, a.offB = p.offB;
    a.spg_shift = 30;
    if (G > 1)
        for (a.spg_shift = 0; (64ll << a.spg_shift) < K / G; ++a.spg_shift) {}
}

// What both down entry points ask of their arguments beyond moe_check_gemm; scratch is checked by the caller once T > 0.
int moe_check_down(const char* fn, const float* expert_w, int64_t T, int64_t N, int top_k, int form, const void* out, int64_t ldo) {
    TGIS_CHECK_ARG(form == 0 || form == 1, "%s: form must be 0 (slabs) or 1 (finished)", fn);
    TGIS_CHECK_ARG(expert_w, "%s: null expert_w", fn);
    TGIS_CHECK_ARG(form == 1 || cdiv64(T, 32) * top_k * 32 < (1ll << 31), "%s: T too large for the slab form", fn);
    TGIS_CHECK_ARG(form == 0 || (out && ldo >= N && N % 4 == 0), "%s: the finished form needs `out` with rows of N (a multiple of 4) elements", fn);
    return TGIS_OK;
}

}  // namespace

extern "C" int tgis_moe_route(const float* logits, int64_t ld, int64_t T, int E, int top_k, int32_t* expert_ids,
                              float* expert_w, int32_t* counts, int32_t* offsets, int32_t* slot_rows, void* stream) {
    const int rc = moe_check_routing("tgis_moe_route", T, E, top_k);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(counts && offsets && (T == 0 || (logits && expert_ids && expert_w && slot_rows)), "tgis_moe_route: null tensor");
    TGIS_CHECK_ARG(T == 0 || ld >= E, "tgis_moe_route: the logit row stride (%ld) must be at least E", (long)ld);
    hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(ROUTE_THREADS), 0, (hipStream_t)stream, logits, ld, (int)T, E, top_k,
                       expert_ids, expert_w, counts, offsets, slot_rows);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int tgis_moe_gemm_up(const void* x, int64_t ldx, const void* images, int64_t expert_stride, const int32_t* offsets,
                                const int32_t* slot_rows, void* h, int64_t ldh, int64_t T, int64_t K, int64_t N, int E,
                                int top_k, int dtype, void* stream) {
    const int rc = moe_check_gemm("tgis_moe_gemm_up", x, ldx, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(N % 32 == 0, "tgis_moe_gemm_up: the gate|up image needs N / 2 (%ld) to be a multiple of 16", (long)(N / 2));
    TGIS_CHECK_ARG(h && ldh >= N / 2, "tgis_moe_gemm_up: h rows must hold N / 2 elements");
    if (T == 0) return TGIS_OK;
    MoeArgs a;
    moe_fill(a, x, ldx, images, expert_stride, offsets, slot_rows, nullptr, h, ldh, K, N, top_k, 0);
    TgisTimedScope timed(TGIS_OP_DENSE_GEMM, (hipStream_t)stream);
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        hipLaunchKernelGGL((moe_gemm_kernel<T_, true, DenseSource<T_>>), dim3((unsigned)a.NT, (unsigned)E), dim3(MOE_THREADS), 0,
                           (hipStream_t)stream, a);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}

extern "C" int tgis_moe_gptq_gemm_up(const void* x, int64_t ldx, const void* images, int64_t expert_stride, const int32_t* offsets,
                                     const int32_t* slot_rows, void* h, int64_t ldh, int64_t T, int64_t K, int64_t N,
                                     int64_t groups, int E, int top_k, int dtype, void* stream) {
    int rc = moe_check_gptq_shape("tgis_moe_gptq_gemm_up", K, N, groups, dtype);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_gemm("tgis_moe_gptq_gemm_up", x, ldx, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype, groups);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(h && ldh >= N / 2, "tgis_moe_gptq_gemm_up: h rows must hold N / 2 elements");
    if (T == 0) return TGIS_OK;
    MoeArgs a;
    moe_fill(a, x, ldx, images, expert_stride, offsets, slot_rows, nullptr, h, ldh, K, N, top_k, 0);
    moe_fill_gptq(a, K, N, groups);
    TgisTimedScope timed(TGIS_OP_GPTQ_GEMM, (hipStream_t)stream);
    hipLaunchKernelGGL((moe_gemm_kernel<f16, true, Int4Source>), dim3((unsigned)a.NT, (unsigned)E), dim3(MOE_THREADS), 0,
                       (hipStream_t)stream, a);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int64_t tgis_moe_gemm_down_bytes(int64_t T, int64_t N, int top_k, int form) {
    if (T <= 0 || N <= 0 || top_k < 1) return 0;
    if (form == 0) return cdiv64(T, 32) * top_k * 32 * cdiv64(N, 32) * 32 * 4;
    return T * top_k * N * 4;
}

extern "C" int tgis_moe_gemm_down(const void* h, int64_t ldh, const void* images, int64_t expert_stride, const int32_t* offsets,
                                  const int32_t* slot_rows, const float* expert_w, int64_t T, int64_t K, int64_t N, int E,
                                  int top_k, int dtype, int form, float* scratch, int64_t scratch_bytes, void* out, int64_t ldo,
                                  void* stream) {
    const int rc = moe_check_gemm("tgis_moe_gemm_down", h, ldh, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype);
    if (rc != TGIS_OK) return rc;
    const int rc2 = moe_check_down("tgis_moe_gemm_down", expert_w, T, N, top_k, form, out, ldo);
    if (rc2 != TGIS_OK) return rc2;
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(scratch && ((uintptr_t)scratch % 16) == 0 && scratch_bytes >= tgis_moe_gemm_down_bytes(T, N, top_k, form),
                   "tgis_moe_gemm_down: scratch too small (%ld < %ld)", (long)scratch_bytes,
                   (long)tgis_moe_gemm_down_bytes(T, N, top_k, form));
    hipStream_t st = (hipStream_t)stream;
    MoeArgs a;
    moe_fill(a, h, ldh, images, expert_stride, offsets, slot_rows, expert_w, scratch, form == 0 ? cdiv64(N, 32) * 32 : N, K, N,
             top_k, form);
    TgisTimedScope timed(TGIS_OP_DENSE_GEMM, st);
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        hipLaunchKernelGGL((moe_gemm_kernel<T_, false, DenseSource<T_>>), dim3((unsigned)a.NT, (unsigned)E), dim3(MOE_THREADS), 0, st, a);
        TGIS_CHECK_LAUNCH();
        if (form == 1) {
            const int64_t work = T * (N / 4);
            hipLaunchKernelGGL(moe_combine_kernel<T_>, dim3((unsigned)cdiv64(work, 256)), dim3(256), 0, st, scratch, (T_*)out,
                               ldo, T, (int)N, top_k);
            TGIS_CHECK_LAUNCH();
        }
        return TGIS_OK;
    });
}

extern "C" int tgis_moe_gptq_gemm_down(const void* h, int64_t ldh, const void* images, int64_t expert_stride,
                                       const int32_t* offsets, const int32_t* slot_rows, const float* expert_w, int64_t T,
                                       int64_t K, int64_t N, int64_t groups, int E, int top_k, int dtype, int form, float* scratch,
                                       int64_t scratch_bytes, void* out, int64_t ldo, void* stream) {
    int rc = moe_check_gptq_shape("tgis_moe_gptq_gemm_down", K, N, groups, dtype);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_gemm("tgis_moe_gptq_gemm_down", h, ldh, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype, groups);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_down("tgis_moe_gptq_gemm_down", expert_w, T, N, top_k, form, out, ldo);
    if (rc != TGIS_OK) return rc;
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(scratch && ((uintptr_t)scratch % 16) == 0 && scratch_bytes >= tgis_moe_gemm_down_bytes(T, N, top_k, form),
                   "tgis_moe_gptq_gemm_down: scratch too small (%ld < %ld)", (long)scratch_bytes,
                   (long)tgis_moe_gemm_down_bytes(T, N, top_k, form));
    hipStream_t st = (hipStream_t)stream;
    MoeArgs a;
    moe_fill(a, h, ldh, images, expert_stride, offsets, slot_rows, expert_w, scratch, N, K, N, top_k, form);  // (N % 32 == 0)
    moe_fill_gptq(a, K, N, groups);
    TgisTimedScope timed(TGIS_OP_GPTQ_GEMM, st);
    hipLaunchKernelGGL((moe_gemm_kernel<f16, false, Int4Source>), dim3((unsigned)a.NT, (unsigned)E), dim3(MOE_THREADS), 0, st, a);
    TGIS_CHECK_LAUNCH();
    if (form == 1) {
        hipLaunchKernelGGL(moe_combine_kernel<f16>, dim3((unsigned)cdiv64(T * (N / 4), 256)), dim3(256), 0, st, scratch, (f16*)out,
                           ldo, T, (int)N, top_k);
        TGIS_CHECK_LAUNCH();
    }
    return TGIS_OK;
}

// The launch plan of the expert GEMMs without a launch (host-only debug export, kept out of include/tgis_hip.h like
// tgis_debug_gemm_plan).  which: 0 up, 1 down form 0, 2 down form 1.  info[16]:
//   0 grid.x (column tiles)   1 grid.y (experts)   2 threads per block   3 k-parts per block   4 k64-steps per k-part
//   5 k64-steps of weights in flight per wave   6 static LDS bytes   7 rows per slab   8 output columns per block
//   9 second launch (the combine of form 1): blocks, else 0   10 fp32 scratch bytes (low 31 bits)   11 scratch bytes >> 31
extern "C" int tgis_debug_moe_plan(int which, int64_t T, int64_t K, int64_t N, int E, int top_k, int* info) {
    TGIS_CHECK_ARG(info && which >= 0 && which <= 2, "tgis_debug_moe_plan: bad arguments");
    const int rc = moe_check_routing("tgis_debug_moe_plan", T, E, top_k);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(K > 0 && K % 8 == 0 && N > 0 && (which != 0 || N % 32 == 0), "tgis_debug_moe_plan: bad shape");
    for (int i = 0; i < 16; ++i) info[i] = 0;
    const int64_t NT = cdiv64(N, 32), KS = cdiv64(K, 64);
    info[0] = (int)NT, info[1] = E, info[2] = MOE_THREADS, info[3] = MOE_WK, info[4] = (int)cdiv64(KS, MOE_WK);
    info[5] = MOE_RING, info[6] = MOE_LDS, info[7] = 32, info[8] = which == 0 ? 16 : 32;
    info[9] = which == 2 ? (int)cdiv64(T * (N / 4), 256) : 0;
    const int64_t bytes = which == 0 ? 0 : tgis_moe_gemm_down_bytes(T, N, top_k, which - 1);
    info[10] = (int)(bytes & 0x7fffffff), info[11] = (int)(bytes >> 31);
    return TGIS_OK;
}

// The same for the int4 entry points (G groups): tgis_debug_moe_plan's info with info[5] the int4 ring and, in addition,
//   12 bytes between expert images, tgis_gptq_prepared_bytes (low 31 bits)   13 those bytes >> 31
extern "C" int tgis_debug_moe_gptq_plan(int which, int64_t T, int64_t K, int64_t N, int64_t G, int E, int top_k, int* info) {
    int rc = tgis_debug_moe_plan(which, T, K, N, E, top_k, info);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_gptq_shape("tgis_debug_moe_gptq_plan", K, N, G, TGIS_F16);
    if (rc != TGIS_OK) return rc;
    const int64_t stride = gptq::prep_layout(K, N, G).total;
    info[5] = MOE_GPTQ_RING;
    info[12] = (int)(stride & 0x7fffffff), info[13] = (int)(stride >> 31);
    return TGIS_OK;
}
