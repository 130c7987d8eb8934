// GPTQ 8-bit linear for gfx950: one-time repack ("prepare"), fused dequant + MFMA GEMM for decode-sized M (1..64) and a
// full dequant kernel for the large-M (library GEMM) path.  Layout, arithmetic and kernel body: gptq8_gemm_body.h.
//
// Replaces the Triton QuantLinear the reference gives 8-bit checkpoints (utils/gptq/quant_linear.py:130-192,259).
#include <algorithm>
#include "common.h"
#include "dispatch.h"
#include "host_helpers.h"
#include "gptq8_gemm_body.h"

namespace gptq {
// sum of the S split-K slabs (+ bias) -> f16 in fixed order (gptq.hip)
int reduce_slabs(const float* slabs, const f16* bias, f16* out, int64_t ldo, int M, int N, int NP, int S, hipStream_t st);
}

namespace {

using gptq8::GemmArgs;
using gptq8::GemmPlan;
using gptq8::PrepLayout;
using gptq8::plan_gemm;
using gptq8::prep_layout;
using gptq8::slab_bytes;

// one thread per image dword: 4 consecutive rows of one column
__global__ void gptq8_prepare_w_kernel(const int32_t* __restrict__ qweight, const int32_t* __restrict__ perm,
                                       uint32_t* __restrict__ w8, int64_t K, int64_t N, int64_t NT, int64_t KSS) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= NT * KSS * 512) return;
    const int d = idx & 3, l = (idx >> 2) & 63, p = (idx >> 8) & 1;
    const int64_t ks = (idx >> 9) % KSS, nt = (idx >> 9) / KSS;
    const int64_t n = nt * 32 + (l & 31);
    const int64_t k0 = ks * 64 + (l >> 5) * 32 + p * 16 + d * 4;
    uint32_t v = 0;
    if (n < N && k0 < K) {  // K % 4 == 0: a dword is whole or absent
        if (perm == nullptr) {
            v = (uint32_t)qweight[(k0 >> 2) * N + n];
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int64_t ksrc = perm[k0 + b];
                const uint32_t w = (uint32_t)qweight[(ksrc >> 2) * N + n];
                v |= ((w >> (8 * (ksrc & 3))) & 255u) << (8 * b);
            }
        }
    }
    w8[idx] = v;
}

__global__ void gptq8_prepare_sz_kernel(const int32_t* __restrict__ qzeros, const f16* __restrict__ scales,
                                        uint32_t* __restrict__ sz, int64_t N, int64_t NT, int64_t G) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= NT * G * 32) return;
    const int c = idx & 31;
    const int64_t g = (idx >> 5) % G, nt = (idx >> 5) / G;
    const int64_t n = nt * 32 + c;
    f16x2 v = {(f16)0.f, (f16)1025.f};
    if (n < N) {
        const uint32_t w = (uint32_t)qzeros[g * (N / 4) + (n >> 2)];
        v[0] = scales[g * N + n];
        v[1] = (f16)(float)(1024u + ((w >> (8 * (n & 3))) & 255u) + 1u);  // z + 1 unmasked: up to 1280, an f16
    }
    sz[idx] = __builtin_bit_cast(uint32_t, v);
}

// one thread per image dword -> 4 rows of the dense [K, N] f16 matrix (image row order)
__global__ void gptq8_dequant_kernel(const uint8_t* __restrict__ prep, int64_t offB, f16* __restrict__ wout, int K, int N,
                                     int G, int gs, int NT, int KSS) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)NT * KSS * 512) return;
    const int d = idx & 3, l = (idx >> 2) & 63, p = (idx >> 8) & 1;
    const int64_t ks = (idx >> 9) % KSS, nt = (idx >> 9) / KSS;
    const int n = (int)nt * 32 + (l & 31);
    const int k0 = (int)ks * 64 + (l >> 5) * 32 + p * 16 + d * 4;
    if (n >= N || k0 >= K) return;
    const uint32_t q = reinterpret_cast<const uint32_t*>(prep)[idx];
    const int g = min(k0 / gs, G - 1);  // gs % 16 == 0: the four rows share a group
    const f16x2 szh = __builtin_bit_cast(f16x2, reinterpret_cast<const uint32_t*>(prep + offB)[(nt * G + g) * 32 + (l & 31)]);
    const float s = (float)szh[0], z1 = (float)szh[1] - 1024.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float v = ((float)((q >> (8 * b)) & 255u) - z1) * s;  // exact in fp32 (9 x 11 bits): one rounding, to f16
        // the product stays apart from its rounding: fused into one v_fma_mixlo_f16 (a * s + 0), a product of -0 (s = 0
        // under a negative q - z - 1) came out as +0
        asm volatile("" : "+v"(v));
        wout[(int64_t)(k0 + b) * N + n] = (f16)v;
    }
}

template <int TN, int WK, int ACT, bool PERM, int MR>
__global__ __launch_bounds__(64 * TN * WK) void gptq8_gemm_kernel(GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    gptq8::gemm_unit<TN, WK, ACT, PERM, MR>(a, smem);
}

template <int TN, int WK, int ACT, bool PERM, int MR>
int launch_one(dim3 grid, hipStream_t st, const GemmArgs& a) {
    constexpr size_t lds = gptq8::lds_bytes(TN, WK, MR);
    static bool attr_done = false;
    if (!attr_done) {
        TGIS_CHECK_HIP(hipFuncSetAttribute((const void*)gptq8_gemm_kernel<TN, WK, ACT, PERM, MR>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_done = true;
    }
    hipLaunchKernelGGL((gptq8_gemm_kernel<TN, WK, ACT, PERM, MR>), grid, dim3(64 * TN * WK), lds, st, a);
    return TGIS_OK;
}

// what every entry point requires of a matrix; `fn` is the caller's name
int check_shape(const char* fn, int64_t K, int64_t N, int64_t groups) {
    TGIS_CHECK_ARG(K > 0 && N > 0 && K % 32 == 0 && N % 32 == 0, "%s: K (%ld) and N (%ld) must be positive multiples of 32",
                   fn, (long)K, (long)N);
    TGIS_CHECK_ARG(groups > 0 && K % groups == 0, "%s: K %% groups != 0 (K=%ld groups=%ld)", fn, (long)K, (long)groups);
    const int64_t gs = K / groups;
    TGIS_CHECK_ARG(gs % 16 == 0, "%s: group size %ld is not a multiple of 16", fn, (long)gs);
    TGIS_CHECK_ARG(N <= (int64_t)1 << 30 && (groups == 1 ? K <= (int64_t)1 << 30 : K * gs < (int64_t)1 << 32),
                   "%s: matrix too large (K=%ld N=%ld groups=%ld)", fn, (long)K, (long)N, (long)groups);
    return TGIS_OK;
}

}  // namespace

extern "C" int64_t tgis_gptq8_prepared_bytes(int64_t K, int64_t N, int64_t groups) {
    if (K <= 0 || N <= 0 || groups <= 0) return 0;
    return prep_layout(K, N, groups).total;
}

extern "C" int tgis_gptq8_prepare(const int32_t* qweight, const int32_t* qzeros, const void* scales,
                                  const int32_t* g_idx_host, int32_t* perm_out, int64_t K, int64_t N, int64_t groups,
                                  int flags, void* prepared, void* stream) {
    TGIS_CHECK_ARG(qweight && qzeros && scales && prepared, "tgis_gptq8_prepare: null tensor");
    TGIS_CHECK_ARG(flags == 0, "tgis_gptq8_prepare: flags must be 0 (the 8-bit image has no epilogue forms)");
    const int rc = check_shape("tgis_gptq8_prepare", K, N, groups);
    if (rc != TGIS_OK) return rc;
    const int64_t gs = K / groups;
    hipStream_t st = (hipStream_t)stream;
    const int32_t* perm_dev = nullptr;
    if (g_idx_host) {
        const int prc = gptq_act_order_perm("tgis_gptq8_prepare", g_idx_host, perm_out, K, gs, st, &perm_dev);
        if (prc != TGIS_OK) return prc;
    }
    const PrepLayout p = prep_layout(K, N, groups);
    uint8_t* base = (uint8_t*)prepared;
    const int64_t totalA = p.NT * p.KSS * 512;
    hipLaunchKernelGGL(gptq8_prepare_w_kernel, dim3((unsigned)cdiv64(totalA, 256)), dim3(256), 0, st, qweight, perm_dev,
                       (uint32_t*)base, K, N, p.NT, p.KSS);
    TGIS_CHECK_LAUNCH();
    const int64_t totalB = p.NT * groups * 32;
    hipLaunchKernelGGL(gptq8_prepare_sz_kernel, dim3((unsigned)cdiv64(totalB, 256)), dim3(256), 0, st, qzeros,
                       (const f16*)scales, (uint32_t*)(base + p.offB), N, p.NT, groups);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int64_t tgis_gptq8_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N) {
    if (M <= 0 || K <= 0 || N <= 0) return 4096;
    return 4096 + slab_bytes(M, N, plan_gemm(K, N, M).S);
}

extern "C" int tgis_gptq8_gemm_f16(const void* x, int64_t ldx, const void* prepared, const void* bias, const int32_t* perm,
                                   void* out, int64_t ldo, int64_t M, int64_t K, int64_t N, int64_t groups, int act,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    TGIS_CHECK_ARG(x && prepared && out, "tgis_gptq8_gemm_f16: null tensor");
    TGIS_CHECK_ARG(M >= 1 && M <= 64, "tgis_gptq8_gemm_f16: serves 1 <= M <= 64 rows (M=%ld); above, dequantise + library GEMM",
                   (long)M);
    int rc = check_shape("tgis_gptq8_gemm_f16", K, N, groups);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(act == 0 || act == 1, "tgis_gptq8_gemm_f16: act must be 0 or 1");
    TGIS_CHECK_ARG(ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ldx >= 0 && ldo >= N,
                   "tgis_gptq8_gemm_f16: x needs 16-byte aligned rows, out rows of at least N elements");
    const GemmPlan pl = plan_gemm(K, N, M);
    const int64_t need = 4096 + slab_bytes(M, N, pl.S);
    TGIS_CHECK_ARG(pl.S == 1 || (workspace && workspace_bytes >= need), "tgis_gptq8_gemm_f16: workspace too small (%ld < %ld)",
                   (long)workspace_bytes, (long)need);
    const PrepLayout p = prep_layout(K, N, groups);
    GemmArgs a;
    a.x = (const f16*)x;
    a.ldx = ldx;
    a.prep = (const uint8_t*)prepared;
    a.offB = p.offB;
    a.bias = pl.S == 1 ? (const f16*)bias : nullptr;  // S > 1: added by the reduce
    a.perm = perm;
    a.out = (f16*)out;
    a.ldo = ldo;
    a.M = (int)M, a.K = (int)K, a.N = (int)N, a.G = (int)groups;
    a.gmagic = gptq8::group_magic(K, groups);
    a.KR = pl.KR, a.S = pl.S;
    a.NT = (int)p.NT, a.KS = (int)p.KS, a.KSS = (int)p.KSS;
    a.slabs = pl.S > 1 ? (float*)((uint8_t*)workspace + 4096) : nullptr;  // the counter region in front stays untouched
    hipStream_t st = (hipStream_t)stream;
    TgisTimedScope timed(TGIS_OP_GPTQ_GEMM, st);
    const dim3 grid((unsigned)cdiv64(p.NT, pl.TN), (unsigned)pl.S);
    rc = by_pair<pair_c<4, 2>, pair_c<2, 4>>(pl.TN, pl.WK, "tgis_gptq8_gemm_f16: plan (TN, WK)", [&](auto tw) {
        constexpr int TN = decltype(tw)::first, WK = decltype(tw)::second;
        return by_bool(act == 1, [&](auto ac) {
            return by_bool(perm != nullptr, [&](auto pm) {
                constexpr int ACT = decltype(ac)::value ? 1 : 0;
                constexpr bool PERM = decltype(pm)::value;
                return pl.MR == 2 ? launch_one<TN, WK, ACT, PERM, 2>(grid, st, a) : launch_one<TN, WK, ACT, PERM, 1>(grid, st, a);
            });
        });
    });
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_LAUNCH();
    if (pl.S > 1) return gptq::reduce_slabs(a.slabs, (const f16*)bias, a.out, a.ldo, a.M, a.N, a.NT * 32, a.S, st);
    return TGIS_OK;
}

extern "C" int tgis_gptq8_dequant_f16(const void* prepared, void* w_out, int64_t K, int64_t N, int64_t groups, void* stream) {
    TGIS_CHECK_ARG(prepared && w_out, "tgis_gptq8_dequant_f16: null tensor");
    const int rc = check_shape("tgis_gptq8_dequant_f16", K, N, groups);
    if (rc != TGIS_OK) return rc;
    const PrepLayout p = prep_layout(K, N, groups);
    const int64_t total = p.NT * p.KSS * 512;
    hipLaunchKernelGGL(gptq8_dequant_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)prepared, p.offB, (f16*)w_out, (int)K, (int)N, (int)groups, (int)(K / groups), (int)p.NT,
                       (int)p.KSS);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

// debug aid (not part of the documented ABI): the launch tgis_gptq8_gemm_f16 would make, without launching.
// info[8] = {TN, WK, KR, S, MR, reduce launch (0 / 1), PERM, kernel ACT}.
extern "C" int tgis_debug_gptq8_plan(int64_t M, int64_t K, int64_t N, int64_t groups, int act, int act_order, int* info) {
    TGIS_CHECK_ARG(info && M >= 1 && M <= 64 && (act == 0 || act == 1), "tgis_debug_gptq8_plan: bad arguments");
    const int rc = check_shape("tgis_debug_gptq8_plan", K, N, groups);
    if (rc != TGIS_OK) return rc;
    const GemmPlan pl = plan_gemm(K, N, M);
    info[0] = pl.TN, info[1] = pl.WK, info[2] = pl.KR, info[3] = pl.S, info[4] = pl.MR, info[5] = pl.S > 1;
    info[6] = act_order != 0, info[7] = act;
    return TGIS_OK;
}
