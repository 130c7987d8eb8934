// MLP speculator, the drafter of speculative decoding: what runs between the dense GEMMs of its heads.  Head i of the
// chain is  s = proj_i x + alpha emb_i[t];  x = gelu(rmsln_i(s));  t = argmax(head_i x).  The two GEMMs are
// tgis_dense_gemm, the argmax is tgis_argmax_logprob; here are the row selection in front of the chain
// (tgis_spec_mlp_input), the arithmetic between a head's GEMMs (tgis_spec_mlp_state) and the transpose behind the chain
// (tgis_spec_mlp_drafts).  Vector loads and stores only.
#include "common.h"
#include "dispatch.h"
#include "rowwise_plan.h"

namespace {

constexpr int MAX_INNER = 16384;  // a row of tgis_spec_mlp_state is cached in registers, as in norm_kernel

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

// One workgroup per request: row b K1 + clamp(n_emit[b], 1, K1) - 1 of hidden, copied (bit for bit) or, SCALE, times
// rsqrt(mean(x^2) + eps) / sqrt(2) with fp32 statistics and one rounding.  The row is read twice rather than cached: E is
// not bounded here, and the second read comes from L2.
template <typename T, bool SCALE>
__global__ __launch_bounds__(256) void spec_mlp_input_kernel(const T* __restrict__ hidden, const int32_t* __restrict__ n_emit,
                                                             int K1, T* __restrict__ out, T* __restrict__ out_copy, int E,
                                                             float eps) {
    using V8 = typename VecT<T>::x8;
    __shared__ float sh[4];
    const int64_t b = blockIdx.x;
    int j = 0;
    if (n_emit) {
        const int n = n_emit[b];
        j = (n < 1 ? 1 : (n > K1 ? K1 : n)) - 1;
    }
    const T* src = hidden + (b * K1 + j) * (int64_t)E;
    const int nchunk = E >> 3;
    float mul = 1.f;
    if (SCALE) {
        float s2 = 0.f;
        for (int c = threadIdx.x; c < nchunk; c += 256) {
            const V8 a = ld16<V8>(src + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) s2 += to_f32(a[e]) * to_f32(a[e]);
        }
        mul = rsqrtf(block_sum<256>(s2, sh) / E + eps) * 0.7071067811865476f;
    }
    for (int c = threadIdx.x; c < nchunk; c += 256) {
        V8 a = ld16<V8>(src + c * 8);
        if (SCALE) {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = from_f32<T>(to_f32(a[e]) * mul);
        }
        st16(out + b * E + c * 8, a);
        if (out_copy) st16(out_copy + b * E + c * 8, a);
    }
}

// One workgroup per row, the shape of norm_kernel: s = p + alpha emb[tok] in fp32, its mean square in fp32, u = s rstd w + b,
// gelu(u) rounded once.  No mean is subtracted (the speculator's LayerNormParameterized is an RMS norm with a bias).
template <typename T, int NT>
__global__ __launch_bounds__(NT) void spec_mlp_state_kernel(const T* __restrict__ proj_out, const int64_t* __restrict__ tok,
                                                            const T* __restrict__ emb, int64_t V, const T* __restrict__ weight,
                                                            const T* __restrict__ bias, float alpha, float eps,
                                                            T* __restrict__ x_out, int inner) {
    using V8 = typename VecT<T>::x8;
    constexpr int MAXV = MAX_INNER / (NT * 8);
    __shared__ float sh[NT / 64];
    const int64_t row = blockIdx.x;
    int64_t t = tok[row];
    t = t < 0 ? 0 : (t >= V ? V - 1 : t);
    const T* pr = proj_out + row * inner;
    const T* er = emb + t * inner;
    float v[MAXV][8];
    V8 wvs[MAXV], bvs[MAXV];
    const int nchunk = inner >> 3;
    float s2 = 0.f;
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        const int c = threadIdx.x + it * NT;
        if (c < nchunk) {
            wvs[it] = ld16<V8>(weight + c * 8);
            bvs[it] = ld16<V8>(bias + c * 8);
            const V8 a = ld16<V8>(pr + c * 8), e8 = ld16<V8>(er + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                v[it][e] = to_f32(a[e]) + alpha * to_f32(e8[e]);
                s2 += v[it][e] * v[it][e];
            }
        }
    }
    const float rstd = rsqrtf(block_sum<NT>(s2, sh) / inner + eps);
#pragma unroll
    for (int it = 0; it < MAXV; ++it) {
        const int c = threadIdx.x + it * NT;
        if (c < nchunk) {
            const V8 wv = wvs[it], bv = bvs[it];
            V8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = from_f32<T>(gelu_f32(v[it][e] * rstd * to_f32(wv[e]) + to_f32(bv[e]), false));
            st16(x_out + row * inner + c * 8, o);
        }
    }
}

__global__ __launch_bounds__(256) void spec_mlp_drafts_kernel(const int64_t* __restrict__ toks, int K,
                                                              int64_t* __restrict__ drafts, int32_t* __restrict__ hits,
                                                              int32_t* __restrict__ hits_copy, int64_t B) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * K) return;
    const int64_t b = r / K;
    const int i = (int)(r - b * K);
    drafts[r] = toks[i * B + b];
    if (i == 0) {
        hits[b] = 1;
        if (hits_copy) hits_copy[b] = 1;
    }
}

}  // namespace

extern "C" int tgis_spec_mlp_input(const void* hidden, const int32_t* n_emit, int64_t K1, void* out, void* out_copy,
                                   int64_t B, int64_t E, int scale_input, float eps, int dtype, void* stream) {
    TGIS_CHECK_ARG(hidden && out && B >= 0 && K1 >= 1 && K1 <= 8, "tgis_spec_mlp_input: bad arguments");
    TGIS_CHECK_ARG(E > 0 && E % 8 == 0 && E < (1ll << 31), "tgis_spec_mlp_input: emb_dim (%ld) must be a multiple of 8",
                   (long)E);
    TGIS_CHECK_ARG(B <= 2147483647LL, "tgis_spec_mlp_input: bad B");
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "tgis_spec_mlp_input: bad dtype");
    if (B == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_bool(scale_input != 0, [&](auto s) {
            hipLaunchKernelGGL((spec_mlp_input_kernel<T, decltype(s)::value>), dim3((unsigned)B), dim3(256), 0, st,
                               (const T*)hidden, n_emit, (int)K1, (T*)out, (T*)out_copy, (int)E, eps);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}

extern "C" int tgis_spec_mlp_state(const void* proj_out, const int64_t* tok, const void* emb, int64_t V,
                                   const void* ln_weight, const void* ln_bias, float alpha, float eps, void* x_out, int64_t B,
                                   int64_t I, int dtype, void* stream) {
    TGIS_CHECK_ARG(proj_out && tok && emb && ln_weight && ln_bias && x_out && V > 0 && B >= 0 && B <= 2147483647LL,
                   "tgis_spec_mlp_state: bad arguments");
    TGIS_CHECK_ARG(I > 0 && I % 8 == 0 && I <= MAX_INNER,
                   "tgis_spec_mlp_state: inner_dim (%ld) must be a multiple of 8 and <= %d", (long)I, MAX_INNER);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "tgis_spec_mlp_state: bad dtype");
    if (B == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool wide = choose_norm(B, I).nt == 512;  // the norms' plan: 512 threads for few long rows
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_bool(wide, [&](auto w) {
            constexpr int NT = decltype(w)::value ? 512 : 256;
            hipLaunchKernelGGL((spec_mlp_state_kernel<T, NT>), dim3((unsigned)B), dim3(NT), 0, st, (const T*)proj_out, tok,
                               (const T*)emb, V, (const T*)ln_weight, (const T*)ln_bias, alpha, eps, (T*)x_out, (int)I);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}

extern "C" int tgis_spec_mlp_drafts(const int64_t* toks, int64_t K, int64_t* drafts, int32_t* hits, int32_t* hits_copy,
                                    int64_t B, void* stream) {
    TGIS_CHECK_ARG(toks && drafts && hits && B >= 0 && B <= (1ll << 24) && K >= 1 && K <= 7,
                   "tgis_spec_mlp_drafts: bad arguments");
    if (B == 0) return TGIS_OK;
    hipLaunchKernelGGL(spec_mlp_drafts_kernel, dim3((unsigned)cdiv64(B * K, 256)), dim3(256), 0, (hipStream_t)stream, toks,
                       (int)K, drafts, hits, hits_copy, B);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}
