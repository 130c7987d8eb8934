// Fused residual-add + RMSNorm / LayerNorm for gfx950.
// Replaces dropout_layer_norm.dropout_add_ln_fwd as called with p=0 from
// custom_modeling/flash_llama_modeling.py:132-152 (RMSNorm) and utils/layers.py:376-396 (LayerNorm):
//   res = x (+ residual)  [sum formed in fp32, stored in the model dtype]
//   y   = norm(res) * weight (+ bias)   [statistics in fp32 from the fp32 sum, one rounding at the end]
// One 256-thread workgroup per row, 16-byte loads, row cached in registers (hidden <= 16384).
#include "common.h"
#include "dispatch.h"
#include "rowwise_plan.h"

namespace {

constexpr int MAX_HIDDEN = 16384;

template <int NT>
__device__ __forceinline__ float block_sum(float v, float* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) t += sh[k];
    return t;
}

// x either as a model-dtype tensor, or (PARTIAL) as S fp32 split-K slabs [S][32][slab_ld] whose sum (+xbias) is
// rounded to the model dtype first — bit-identical to running the split-K reduce kernel and then this one.
// NT threads per row: 256 in general, 512 for decode-sized batches (few rows: latency matters, not occupancy)
template <typename T, bool RMS, bool PARTIAL, int NT>
__global__ __launch_bounds__(NT) void norm_kernel(const T* x, const T* residual,
                                                  const T* __restrict__ weight, const T* __restrict__ bias,
                                                  T* y, T* res_out, int hidden,
                                                  float eps, const float* __restrict__ slabs, int S, int64_t slab_ld,
                                                  const T* __restrict__ xbias, int y_frag) {
    using V8 = typename VecT<T>::x8;
    constexpr int MAXV = MAX_HIDDEN / (NT * 8);
    __shared__ float sh[NT / 64];
    const int64_t row = blockIdx.x;
    const T* xr = PARTIAL ? nullptr : x + row * hidden;
    const T* rr = residual ? residual + row * hidden : nullptr;
    float v[MAXV][8];
    V8 wvs[MAXV], bvs[MAXV];  // weight / bias: asked for with the inputs, not after the row reductions
    const int nchunk = hidden >> 3;  // hidden % 8 == 0
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        int c = threadIdx.x + it * NT;
        if (c < nchunk) {
            wvs[it] = ld16<V8>(weight + c * 8);
            if (bias) bvs[it] = ld16<V8>(bias + c * 8);
            // Round 5: the residual and the bias of the GEMM before are requested HERE, in front of the slabs.  Behind them (in
            // their own basic blocks, after the waits of the slab sum) they were a second and a third dependent round trip to
            // memory in a kernel that is nothing but one round trip.
            V8 b, bv;
            if (rr) b = ld16<V8>(rr + c * 8);
            if (PARTIAL && xbias) bv = ld16<V8>(xbias + c * 8);
            V8 a;
            if (PARTIAL) {
                f32x4 lo, hi;
                // slabs are stored in 32-row units: [row / 32][S][32][slab_ld]
                sum_slabs8(slabs + ((int64_t)(row >> 5) * S * 32 + (row & 31)) * slab_ld + c * 8, 32 * slab_ld, S, lo, hi);
                if (xbias) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        lo[e] += to_f32(bv[e]);
                        hi[e] += to_f32(bv[e + 4]);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = from_f32<T>(lo[e]);
                    a[e + 4] = from_f32<T>(hi[e]);
                }
            } else {
                a = ld16<V8>(xr + c * 8);
            }
            V8 o;
            if (rr) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[it][e] = to_f32(a[e]) + to_f32(b[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[it][e] = to_f32(a[e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = from_f32<T>(v[it][e]);
                s1 += v[it][e];
                s2 += v[it][e] * v[it][e];
            }
            if (res_out) st16(res_out + row * hidden + c * 8, o);
        }
    }
    float mean = 0.f, rstd;
    if (RMS) {
        float tot = block_sum<NT>(s2, sh);
        rstd = rsqrtf(tot / hidden + eps);
    } else {
        mean = block_sum<NT>(s1, sh) / hidden;
        float d2 = 0.f;
#pragma unroll
        for (int it = 0; it < MAXV; ++it) {
            int c = threadIdx.x + it * NT;
            if (c < nchunk) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float d = v[it][e] - mean;
                    d2 += d * d;
                }
            }
        }
        float var = block_sum<NT>(d2, sh) / hidden;
        rstd = rsqrtf(var + eps);
    }
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        int c = threadIdx.x + it * NT;
        if (c < nchunk) {
            const V8 wv = wvs[it];
            V8 o;
            if (bias) {
                const V8 bv = bvs[it];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    o[e] = from_f32<T>((v[it][e] - mean) * rstd * to_f32(wv[e]) + to_f32(bv[e]));
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = from_f32<T>((v[it][e] - mean) * rstd * to_f32(wv[e]));
            }
            // y_frag (RMSNorm in front of an int4 decode GEMM): 32-row fragment order, xf_off in common.h
            st16(y + (y_frag ? xf_off(row, c * 8, hidden) : row * hidden + c * 8), o);
        }
    }
}

template <bool RMS>
static int launch_norm(const void* x, const void* residual, const void* weight, const void* bias, void* y,
                       void* res_out, int64_t rows, int64_t hidden, float eps, int dtype, void* stream,
                       const float* slabs = nullptr, int S = 0, int64_t slab_ld = 0, const void* xbias = nullptr,
                       int64_t ldy = 0) {
    TGIS_CHECK_ARG((x || slabs) && weight && y, "norm: null tensor");
    TGIS_CHECK_ARG(!slabs || (S >= 1 && slab_ld >= hidden && slab_ld % 4 == 0),
                   "norm: partial input needs a slab row stride >= hidden");
    TGIS_CHECK_ARG(hidden > 0 && hidden % 8 == 0 && hidden <= MAX_HIDDEN,
                   "norm: hidden (%ld) must be a multiple of 8 and <= %d", (long)hidden, MAX_HIDDEN);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "norm: bad dtype");
    const int y_frag = ldy == TGIS_LD_FRAGMENTS;
    TGIS_CHECK_ARG(ldy == 0 || ldy == hidden || (y_frag && RMS && rows <= 64 && hidden % 64 == 0),
                   "norm: y is [rows, hidden] contiguous (ldy = 0 or hidden), or — RMSNorm, rows <= 64, hidden %% 64 == 0 — in "
                   "fragment order (ldy = TGIS_LD_FRAGMENTS)");
    if (rows == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    TgisTimedScope timed(TGIS_OP_NORM, st);
    const bool wide = choose_norm(rows, hidden).nt == 512;
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_bool(slabs != nullptr, [&](auto partial) {
            return by_bool(wide, [&](auto w) {
                constexpr int NT = decltype(w)::value ? 512 : 256;
                hipLaunchKernelGGL((norm_kernel<T, RMS, decltype(partial)::value, NT>), dim3((unsigned)rows), dim3(NT), 0,
                                   st, (const T*)x, (const T*)residual, (const T*)weight, (const T*)bias, (T*)y,
                                   (T*)res_out, (int)hidden, eps, slabs, S, slab_ld, (const T*)xbias, y_frag);
                TGIS_CHECK_LAUNCH();
                return TGIS_OK;
            });
        });
    });
}

// Parallel-residual layer boundary of GPT-NeoX (flash_neox_modeling.py:238-259): h' = h + A + B (+ biases) and two
// LayerNorms of h'.  Each addend is a model-dtype tensor, split-K fp32 slabs [S][32][slab_ld] (S may differ between the
// two), or absent; its bias is added to it in fp32.  h' = ((h + A) + B) in fp32, rounded once for res_out; y1 and y2 take
// the same fp32 statistics of the unrounded sum, like norm_kernel.  y2 == nullptr: one LayerNorm (final_layer_norm).
struct Addend {
    const void* x;        // model-dtype [rows, hidden], or nullptr
    const float* slabs;   // or split-K partial sums, or nullptr
    int S;
    int64_t slab_ld;
    const void* bias;     // [hidden] or nullptr
};

template <typename T>
__device__ __forceinline__ void add_addend(float (&v)[8], const Addend& ad, int64_t row, int hidden, int c) {
    using V8 = typename VecT<T>::x8;
    if (ad.slabs) {
        f32x4 lo, hi;
        sum_slabs8(ad.slabs + ((row >> 5) * ad.S * 32 + (row & 31)) * ad.slab_ld + c * 8, 32 * ad.slab_ld, ad.S, lo, hi);
        if (ad.bias) {
            const V8 bv = ld16<V8>(reinterpret_cast<const T*>(ad.bias) + c * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                lo[e] += to_f32(bv[e]);
                hi[e] += to_f32(bv[e + 4]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] += lo[e];
            v[e + 4] += hi[e];
        }
    } else if (ad.x) {
        const V8 a = ld16<V8>(reinterpret_cast<const T*>(ad.x) + row * hidden + c * 8);
        if (ad.bias) {
            const V8 bv = ld16<V8>(reinterpret_cast<const T*>(ad.bias) + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += to_f32(a[e]) + to_f32(bv[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += to_f32(a[e]);
        }
    } else if (ad.bias) {
        const V8 bv = ld16<V8>(reinterpret_cast<const T*>(ad.bias) + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += to_f32(bv[e]);
    }
}

template <typename T, int NT>
__global__ __launch_bounds__(NT) void layernorm2_kernel(const T* h, Addend A, Addend B, const T* __restrict__ w1,
                                                        const T* __restrict__ b1, const T* __restrict__ w2,
                                                        const T* __restrict__ b2, T* y1, T* y2, T* res_out, int hidden,
                                                        float eps) {
    using V8 = typename VecT<T>::x8;
    constexpr int MAXV = MAX_HIDDEN / (NT * 8);
    __shared__ float sh[NT / 64];
    const int64_t row = blockIdx.x;
    float v[MAXV][8];
    const int nchunk = hidden >> 3;
    float s1 = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        const int c = threadIdx.x + it * NT;
        if (c < nchunk) {
            const V8 hv = ld16<V8>(h + row * hidden + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[it][e] = to_f32(hv[e]);
            add_addend<T>(v[it], A, row, hidden, c);
            add_addend<T>(v[it], B, row, hidden, c);
            V8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = from_f32<T>(v[it][e]);
                s1 += v[it][e];
            }
            if (res_out) st16(res_out + row * hidden + c * 8, o);
        }
    }
    const float mean = block_sum<NT>(s1, sh) / hidden;
    float d2 = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        const int c = threadIdx.x + it * NT;
        if (c < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[it][e] - mean;
                d2 += d * d;
            }
        }
    }
    const float rstd = rsqrtf(block_sum<NT>(d2, sh) / hidden + eps);
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        const int c = threadIdx.x + it * NT;
        if (c < nchunk) {
            float n[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) n[e] = (v[it][e] - mean) * rstd;
            const V8 wa = ld16<V8>(w1 + c * 8), ba = ld16<V8>(b1 + c * 8);
            V8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(n[e] * to_f32(wa[e]) + to_f32(ba[e]));
            st16(y1 + row * hidden + c * 8, o);
            if (y2) {
                const V8 wb = ld16<V8>(w2 + c * 8), bb = ld16<V8>(b2 + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(n[e] * to_f32(wb[e]) + to_f32(bb[e]));
                st16(y2 + row * hidden + c * 8, o);
            }
        }
    }
}

static int launch_layernorm2(const void* h, const Addend& A, const Addend& B, const void* w1, const void* b1,
                             const void* w2, const void* b2, void* y1, void* y2, void* res_out, int64_t rows,
                             int64_t hidden, float eps, int dtype, void* stream) {
    TGIS_CHECK_ARG(h && w1 && b1 && y1, "tgis_layernorm2_residual: null tensor");
    TGIS_CHECK_ARG(!y2 || (w2 && b2), "tgis_layernorm2_residual: y2 needs w2 and b2");
    TGIS_CHECK_ARG(!(A.x && A.slabs) && !(B.x && B.slabs), "tgis_layernorm2_residual: an addend is a tensor OR slabs");
    TGIS_CHECK_ARG((!A.slabs || (A.S >= 1 && A.slab_ld >= hidden && A.slab_ld % 4 == 0)) &&
                       (!B.slabs || (B.S >= 1 && B.slab_ld >= hidden && B.slab_ld % 4 == 0)),
                   "tgis_layernorm2_residual: slab input needs S >= 1 and a row stride >= hidden (multiple of 4)");
    TGIS_CHECK_ARG(hidden > 0 && hidden % 8 == 0 && hidden <= MAX_HIDDEN,
                   "tgis_layernorm2_residual: hidden (%ld) must be a multiple of 8 and <= %d", (long)hidden, MAX_HIDDEN);
    TGIS_CHECK_ARG(rows >= 0 && rows <= 2147483647LL, "tgis_layernorm2_residual: bad rows");
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "tgis_layernorm2_residual: bad dtype");
    if (rows == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    TgisTimedScope timed(TGIS_OP_NORM, st);
    const bool wide = choose_norm(rows, hidden).nt == 512;
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_bool(wide, [&](auto w) {
            constexpr int NT = decltype(w)::value ? 512 : 256;
            hipLaunchKernelGGL((layernorm2_kernel<T, NT>), dim3((unsigned)rows), dim3(NT), 0, st, (const T*)h, A, B,
                               (const T*)w1, (const T*)b1, (const T*)w2, (const T*)b2, (T*)y1, (T*)y2, (T*)res_out,
                               (int)hidden, eps);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}

}  // namespace

// 512 threads for decode-sized batches (few rows: latency matters, not occupancy), 256 otherwise
NormPlan choose_norm(int64_t rows, int64_t hidden) {
    const int nt = rows <= 64 && hidden >= 2048 ? 512 : 256;
    return {nt, (int)cdiv64(hidden / 8, nt)};
}

extern "C" int tgis_rmsnorm_residual(const void* x, const void* residual, const void* weight, void* y, int64_t ldy,
                                     void* res_out, int64_t rows, int64_t hidden, float eps, int dtype,
                                     void* stream) {
    return launch_norm<true>(x, residual, weight, nullptr, y, res_out, rows, hidden, eps, dtype, stream, nullptr, 0, 0,
                             nullptr, ldy);
}

extern "C" int tgis_rmsnorm_residual_partial(const float* slabs, int num_slabs, int64_t slab_ld, const void* bias,
                                             const void* residual, const void* weight, void* y, int64_t ldy, void* res_out,
                                             int64_t rows, int64_t hidden, float eps, int dtype, void* stream) {
    TGIS_CHECK_ARG(slabs, "tgis_rmsnorm_residual_partial: null slabs");
    return launch_norm<true>(nullptr, residual, weight, nullptr, y, res_out, rows, hidden, eps, dtype, stream, slabs,
                             num_slabs, slab_ld, bias, ldy);
}

extern "C" int tgis_layernorm_residual_partial(const float* slabs, int num_slabs, int64_t slab_ld, const void* xbias,
                                               const void* residual, const void* weight, const void* bias, void* y,
                                               void* res_out, int64_t rows, int64_t hidden, float eps, int dtype,
                                               void* stream) {
    TGIS_CHECK_ARG(slabs, "tgis_layernorm_residual_partial: null slabs");
    return launch_norm<false>(nullptr, residual, weight, bias, y, res_out, rows, hidden, eps, dtype, stream, slabs,
                              num_slabs, slab_ld, xbias);
}

extern "C" int tgis_layernorm_residual(const void* x, const void* residual, const void* weight,
                                       const void* bias, void* y, void* res_out, int64_t rows, int64_t hidden,
                                       float eps, int dtype, void* stream) {
    return launch_norm<false>(x, residual, weight, bias, y, res_out, rows, hidden, eps, dtype, stream);
}

extern "C" int tgis_layernorm2_residual(const void* residual, const void* a, const void* a_bias, const void* b,
                                        const void* b_bias, const void* w1, const void* b1, const void* w2, const void* b2,
                                        void* y1, void* y2, void* res_out, int64_t rows, int64_t hidden, float eps,
                                        int dtype, void* stream) {
    const Addend A{a, nullptr, 0, 0, a_bias}, B{b, nullptr, 0, 0, b_bias};
    return launch_layernorm2(residual, A, B, w1, b1, w2, b2, y1, y2, res_out, rows, hidden, eps, dtype, stream);
}

extern "C" int tgis_layernorm2_residual_partial(const void* residual, const void* a, const float* a_slabs, int a_num_slabs,
                                                int64_t a_slab_ld, const void* a_bias, const void* b, const float* b_slabs,
                                                int b_num_slabs, int64_t b_slab_ld, const void* b_bias, const void* w1,
                                                const void* b1, const void* w2, const void* b2, void* y1, void* y2,
                                                void* res_out, int64_t rows, int64_t hidden, float eps, int dtype,
                                                void* stream) {
    const Addend A{a, a_slabs, a_num_slabs, a_slab_ld, a_bias}, B{b, b_slabs, b_num_slabs, b_slab_ld, b_bias};
    return launch_layernorm2(residual, A, B, w1, b1, w2, b2, y1, y2, res_out, rows, hidden, eps, dtype, stream);
}
