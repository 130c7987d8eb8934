// KV page block layout for one (page, kv head), 32 tokens x D elements, and the "partial input" form of
// the qkv activation (fp32 split-K slabs of the qkv GEMM that the consumer sums itself).  Shared by rope_kv.hip (the
// stand-alone rotary + cache-write kernels) and attention.hip (the decode kernel that does both in its prologue).
//   K: [tile=tok>>4][D/8][16 tokens][8]      -> MFMA 16x16x32 A-fragments are 1 KiB contiguous loads
//   V: [4 column groups][D][8], token tok in column v_col(tok) = (i>>2)*8 + tile*4 + (i&3), i = tok&15 (column group =
//      v_col >> 3, slot = v_col & 7) -> a V^T A-fragment (16 rows d x 32 token columns) is four contiguous 256-byte runs of
//      whole cache lines, and the d run of ONE token (a decode step's write) is 16-byte strided: 16 cache lines per head
//      where the [D][32] order of rounds 1-3 touched 64 (round 4: the qkv + rotary launch 15.9 -> 12.6 us with cold pages)
//
// One-byte cache (tgis_*_kv8 entry points, kv_dtype TGIS_KV_FP8_E4M3): the same block in OCP float8_e4m3fn, 32 D bytes per
// (page, kv head), in the SAME token and dim order — k_off / v_off are element offsets, now byte offsets.  A lane's fragment
// load of the decode kernel is then 8 bytes where it was 16.  The pair-interleaved alternative (one 16-byte load holding the
// fragments of two k-steps, or of two V row blocks) was NOT built or measured: no kernel-time A/B between the two orders exists.
// The plain order ships on what was measured of it alone (NOTEBOOK.md, "One-byte KV cache"): at cfg3 the decode attention
// launch takes 49.8 us against 84.5 us on the 16-bit pool (bench.py's eager pass), 0.67 of the HBM peak on its halved bytes.
//   stored = e4m3(sat(x / s)), x the value the 16-bit pool would hold (k after rotary, rounded to the model dtype), s the
//   layer's k_scale / v_scale, sat the clamp to +-448, rounding to nearest even.  The NaN codes 0x7F / 0xFF are never
//   written: every value in the pool stays finite (utils/kv_cache.py).  Readers widen exactly (every e4m3 value is an f16
//   and a bf16) and fold the scales into the softmax: k_scale into scale_log2, 1 / v_scale into the normaliser.
#pragma once
#include <type_traits>
#include "common.h"

__device__ __forceinline__ int64_t k_off(int tok, int d, int D) {
    return ((int64_t)(((tok >> 4) * (D >> 3) + (d >> 3)) * 16 + (tok & 15)) << 3) + (d & 7);
}
__device__ __forceinline__ int v_col(int tok) {
    int i = tok & 15;
    return (i >> 2) * 8 + (tok >> 4) * 4 + (i & 3);
}
// element offset of (token tok, dim d) inside the V block of one (page, kv head)
__device__ __forceinline__ int64_t v_off(int tok, int d, int D) {
    const int cp = v_col(tok);
    return ((int64_t)((cp >> 3) * D + d) << 3) + (cp & 7);
}

template <typename T> struct PartialIn {
    const float* slabs;  // [S][32][slab_ld] fp32 split-K partial sums of the qkv GEMM, or nullptr
    int S;
    int64_t slab_ld;
    const T* bias;
};

// 8 consecutive elements of row t starting at column col: from the model-dtype tensor (hp points at them), or the sum
// of the slabs (+ bias) rounded to the model dtype — bit-identical to reducing first and reading the tensor.
template <typename T>
__device__ __forceinline__ typename VecT<T>::x8 load_chunk(const T* hp, int64_t t, int col, const PartialIn<T>& pin) {
    using V8 = typename VecT<T>::x8;
    if (pin.slabs == nullptr) return ld16<V8>(hp);
    f32x4 lo, hi;
    sum_slabs8(pin.slabs + ((t >> 5) * pin.S * 32 + (t & 31)) * pin.slab_ld + col, 32 * pin.slab_ld, pin.S, lo, hi);
    V8 a;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float b0 = pin.bias ? to_f32(pin.bias[col + e]) : 0.f, b1 = pin.bias ? to_f32(pin.bias[col + 4 + e]) : 0.f;
        a[e] = from_f32<T>(lo[e] + b0);
        a[e + 4] = from_f32<T>(hi[e] + b1);
    }
    return a;
}

// ---- one-byte cache: KV = uint8_t holds e4m3 codes; KV = T is the 16-bit pool ------------------------------------------------
template <typename T, typename KV> constexpr bool kv_is8() { return !std::is_same<T, KV>::value; }

__device__ __forceinline__ float kv8_sat(float x, float s) { return fminf(fmaxf(x / s, -448.f), 448.f); }
// four saturated values -> four e4m3 codes (round to nearest even), byte e = value e
__device__ __forceinline__ uint32_t kv8_pack4(float a, float b, float c, float d) {
    const uint32_t w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
}

// one element of k or v into the pool
template <typename T, typename KV>
__device__ __forceinline__ void kv_put(KV* p, T x, float s) {
    if constexpr (kv_is8<T, KV>())
        *p = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(kv8_sat(to_f32(x), s), 0.f, 0, false) & 0xFF);
    else
        *p = x;
}
// eight consecutive elements (16 bytes of a 16-bit pool, 8 bytes of a one-byte pool)
template <typename T, typename KV>
__device__ __forceinline__ void kv_put8(KV* p, typename VecT<T>::x8 v, float s) {
    if constexpr (kv_is8<T, KV>()) {
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = kv8_sat(to_f32(v[e]), s);
        *reinterpret_cast<u32x2*>(p) = u32x2{kv8_pack4(f[0], f[1], f[2], f[3]), kv8_pack4(f[4], f[5], f[6], f[7])};
    } else {
        st16(p, v);
    }
}

// eight e4m3 codes (byte e = element e) -> eight model-dtype values, exact
template <typename T> __device__ __forceinline__ typename VecT<T>::x8 kv8_widen(u32x2 w);
template <> __device__ __forceinline__ f16x8 kv8_widen<f16>(u32x2 w) {
    const f16x2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[0], 1.f, false);
    const f16x2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[0], 1.f, true);
    const f16x2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[1], 1.f, false);
    const f16x2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[1], 1.f, true);
    return f16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
template <> __device__ __forceinline__ bf16x8 kv8_widen<bf16>(u32x2 w) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], 1.f, false);
    const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[0], 1.f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], 1.f, false);
    const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[1], 1.f, true);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// eight consecutive pool elements as model-dtype values: nontemporal (the decode kernel's streaming loads) or plain
template <typename T, typename KV>
__device__ __forceinline__ typename VecT<T>::x8 kv_get8_nt(const KV* p) {
    using V8 = typename VecT<T>::x8;
    if constexpr (kv_is8<T, KV>())
        return kv8_widen<T>(__builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p)));
    else
        return __builtin_nontemporal_load(reinterpret_cast<const V8*>(p));
}
template <typename T, typename KV>
__device__ __forceinline__ typename VecT<T>::x8 kv_get8(const KV* p) {
    if constexpr (kv_is8<T, KV>())
        return kv8_widen<T>(*reinterpret_cast<const u32x2*>(p));
    else
        return ld16<typename VecT<T>::x8>(p);
}
