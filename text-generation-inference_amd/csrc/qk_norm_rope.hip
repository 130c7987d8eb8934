// Per-head RMSNorm of q and k (Qwen3's self_attn.q_norm / k_norm, weights of size D) built into the rope + cache-write
// launches of rope_kv.hip: a Qwen3 layer has the launches of Llama's unfused path, no separate norm pass.
//
// Arithmetic of one q or k head, x the model-dtype value rope_kv.hip would read (for split-K slabs the rounded sum + bias of
// load_chunk):  rstd = rsqrt(sum_d x^2 / D + eps),  y = (x * rstd) * w[d]  in fp32, then the half-split rotation of y in fp32
// over dims [0, rot), and ONE rounding to the model dtype at the store.  Dims in [rot, D) are normalised and not rotated; v
// heads are copied bit for bit.  The rounded k is what the K page receives (its e4m3 code / k_scale on a one-byte pool).
//
// Both kernels compute a head's statistics the same way, so that they write the same bits for the same token: chunk j (8
// elements, summed in order with fma) sits in lane j of a group of QKN_LANES = 16 lanes, lanes without a chunk (D = 64: 8 of
// them, D = 96: 4) hold zero, and the 16 partial sums are added by an xor butterfly inside the wave: no barrier and no LDS.
#include <algorithm>
#include "common.h"
#include "dispatch.h"
#include "kv_layout.h"
#include "qknorm_plan.h"

namespace {

// sum over the 16 lanes of a head's group; every lane of the group gets the same bits (a + b == b + a at every level)
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = QKN_LANES / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// rstd of a head from the chunk this lane holds (zeros in a lane without one)
template <typename V8>
__device__ __forceinline__ float head_rstd(const V8& a, int D, float eps) {
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(to_f32(a[e]), to_f32(a[e]), ss);
    return rsqrtf(group_sum(ss) / (float)D + eps);
}

__device__ __forceinline__ float normed(float x, float rstd, float w) { return (x * rstd) * w; }
// the rotation of rope_kv_kernel, x1 * cos - x2 * sin and x1 * sin + x2 * cos, with the contraction written out: both kernels
// of this file must round alike
__device__ __forceinline__ float rot_lo(float y1, float y2, float c, float s) { return fmaf(y1, c, -(y2 * s)); }
__device__ __forceinline__ float rot_hi(float y1, float y2, float c, float s) { return fmaf(y1, s, y2 * c); }

// Per token (rope_kv_kernel's role): grid (T, gy), a block takes QKN_HEADS heads of its token per pass.  Lane j of a head's
// group loads chunk j (one 16-byte load, or the slab sum), takes its rotary partner's normalised chunk from lane j +- rot/16
// and stores chunk j (one 16-byte store to qkv, one to the K page).  KV as in rope_kv_kernel.
template <typename T, typename KV>
__global__ __launch_bounds__(256) void qknorm_rope_kv_kernel(T* qkv, int64_t ld, const T* __restrict__ q_w,
                                                             const T* __restrict__ k_w, float eps,
                                                             const T* __restrict__ cosb, const T* __restrict__ sinb,
                                                             const int32_t* __restrict__ positions,
                                                             const int32_t* __restrict__ slots, KV* __restrict__ kpool,
                                                             KV* __restrict__ vpool, int H, int Hkv, int D, int rot,
                                                             PartialIn<T> pin, float k_scale, float v_scale) {
    using V8 = typename VecT<T>::x8;
    const int64_t t = blockIdx.x;
    T* row = qkv + t * ld;
    const int c8 = D >> 3, rh8 = rot >> 4, heads = H + 2 * Hkv;
    const int j = threadIdx.x & (QKN_LANES - 1);
    const bool active = j < c8;
    const int slot = slots ? slots[t] : 0;
    const int page = slot >> 5, tok = slot & 31;
    const T* cr = cosb + (int64_t)positions[t] * (rot >> 1);
    const T* sr = sinb + (int64_t)positions[t] * (rot >> 1);
    // the partner chunk of the rotation: j + rh8 for the first half of the span, j - rh8 for the second, itself behind it
    const bool lo = j < rh8, roped = j < 2 * rh8;
    const int partner = (threadIdx.x & 63 & ~(QKN_LANES - 1)) | (roped ? (lo ? j + rh8 : j - rh8) : j);
    for (int head = blockIdx.y * QKN_HEADS + (threadIdx.x >> 4); head < heads; head += gridDim.y * QKN_HEADS) {
        // (the 16 lanes of a group share `head`: they stay together through the shuffles below)
        T* hp = row + (int64_t)head * D;
        const bool is_v = head >= H + Hkv, is_k = head >= H && !is_v;
        V8 a;
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (T)0.f;
        if (active) a = load_chunk<T>(hp + j * 8, t, head * D + j * 8, pin);
        if (is_v) {
            if (!active) continue;
            if (pin.slabs) st16(hp + j * 8, a);
            if (!vpool) continue;
            KV* vb = vpool + ((int64_t)page * Hkv + (head - H - Hkv)) * 32 * D + v_off(tok, j * 8, D);
#pragma unroll
            for (int e = 0; e < 8; ++e) kv_put<T, KV>(vb + e * 8, a[e], v_scale);
            continue;
        }
        const float rstd = head_rstd(a, D, eps);
        const T* w = is_k ? k_w : q_w;
        float y[8], yp[8];
        V8 wv = a;  // (a lane without a chunk: zeros)
        if (active) wv = ld16<V8>(w + j * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = normed(to_f32(a[e]), rstd, to_f32(wv[e]));
#pragma unroll
        for (int e = 0; e < 8; ++e) yp[e] = __shfl(y[e], partner, 64);
        if (!active) continue;
        V8 o;
        if (roped) {
            const int cj = lo ? j : j - rh8;
            const V8 c = ld16<V8>(cr + cj * 8), s = ld16<V8>(sr + cj * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float cf = to_f32(c[e]), sf = to_f32(s[e]);
                o[e] = from_f32<T>(lo ? rot_lo(y[e], yp[e], cf, sf) : rot_hi(yp[e], y[e], cf, sf));
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = from_f32<T>(y[e]);
        }
        st16(hp + j * 8, o);
        if (is_k && kpool) {
            KV* kb = kpool + ((int64_t)page * Hkv + (head - H)) * 32 * D;
            kv_put8<T, KV>(kb + k_off(tok, j * 8, D), o, k_scale);
        }
    }
}

// Page-wise (rope_kv_prefill_kernel's role, same grid, same preconditions, same stores): one block per (sequence, 32-token
// page, kv head).  A first pass leaves the rstd of the page's 32 k rows in LDS, 16 rows at a time in the lane layout of the
// per-token kernel; then the k rows are normalised, rotated and stored as 256-byte runs and the v rows are transposed through
// LDS, as there.  q goes through the per-token kernel (Hkv = 0).
template <typename T, typename KV>
__global__ __launch_bounds__(256) void qknorm_rope_kv_prefill_kernel(const T* __restrict__ qkv, int64_t ld,
                                                                     const T* __restrict__ k_w, float eps,
                                                                     const T* __restrict__ cosb, const T* __restrict__ sinb,
                                                                     const int32_t* __restrict__ positions,
                                                                     const int32_t* __restrict__ cu,
                                                                     const int32_t* __restrict__ past_lens,
                                                                     const int32_t* __restrict__ bt, int64_t max_pages,
                                                                     KV* __restrict__ kpool, KV* __restrict__ vpool, int H,
                                                                     int Hkv, int D, int rot, int pages_per_seq,
                                                                     float k_scale, float v_scale) {
    using V8 = typename VecT<T>::x8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* vs = reinterpret_cast<T*>(smem);  // [32 tokens][D + 8]
    float* rs = reinterpret_cast<float*>(smem + (size_t)32 * (D + 8) * sizeof(T));  // [32] rstd of the k rows
    const int b = blockIdx.x / pages_per_seq, p = blockIdx.x % pages_per_seq, hk = blockIdx.y;
    const int t0 = cu[b], len = cu[b + 1] - t0;
    const int i0 = p * 32;
    if (i0 >= len) return;
    const int ntok = min(32, len - i0);
    const int tp = (past_lens ? past_lens[b] >> 5 : 0) + p;  // table entry of this page
    if (tp >= max_pages) return;  // (a past_lens the table has no room for: nothing is read or written)
    const int page = bt[(int64_t)b * max_pages + tp];
    const int tid = threadIdx.x;
    const int c8 = D >> 3, rh8 = rot >> 4;
    KV* kb = kpool + ((int64_t)page * Hkv + hk) * 32 * D;
    KV* vb = vpool + ((int64_t)page * Hkv + hk) * 32 * D;
    V8 zero;
#pragma unroll
    for (int e = 0; e < 8; ++e) zero[e] = (T)0.f;

    // ---- statistics: row tok = 16 pass + tid / 16, chunk j = tid % 16 -----------------------------------------------------
    for (int pass = 0; pass < 32 / QKN_HEADS; ++pass) {
        const int tok = pass * QKN_HEADS + (tid >> 4), j = tid & (QKN_LANES - 1);
        V8 a = zero;
        if (tok < ntok && j < c8) a = ld16<V8>(qkv + (int64_t)(t0 + i0 + tok) * ld + (int64_t)(H + hk) * D + j * 8);
        const float rstd = head_rstd(a, D, eps);
        if (j == 0) rs[tok] = rstd;
    }
    __syncthreads();

    // ---- K: item = (token, 8-element chunk j); the rotary partner chunk j + rot/16 is handled with it ----------
    for (int it = tid; it < 32 * c8; it += 256) {
        const int tok = it & 31, j = it >> 5;
        if (j >= rh8 && j < 2 * rh8) continue;
        const bool pair = j < rh8;
        V8 o1 = zero, o2 = zero;
        if (tok < ntok) {
            const int64_t t = t0 + i0 + tok;
            const T* kp = qkv + t * ld + (int64_t)(H + hk) * D;
            const float rstd = rs[tok];
            const V8 x1 = ld16<V8>(kp + j * 8), w1 = ld16<V8>(k_w + j * 8);
            if (pair) {
                const V8 x2 = ld16<V8>(kp + (j + rh8) * 8), w2 = ld16<V8>(k_w + (j + rh8) * 8);
                const T* cr = cosb + (int64_t)positions[t] * (rot >> 1);
                const T* sr = sinb + (int64_t)positions[t] * (rot >> 1);
                const V8 c = ld16<V8>(cr + j * 8), sn = ld16<V8>(sr + j * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float y1 = normed(to_f32(x1[e]), rstd, to_f32(w1[e])), y2 = normed(to_f32(x2[e]), rstd, to_f32(w2[e]));
                    const float cf = to_f32(c[e]), sf = to_f32(sn[e]);
                    o1[e] = from_f32<T>(rot_lo(y1, y2, cf, sf));
                    o2[e] = from_f32<T>(rot_hi(y1, y2, cf, sf));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o1[e] = from_f32<T>(normed(to_f32(x1[e]), rstd, to_f32(w1[e])));
            }
        }
        kv_put8<T, KV>(kb + k_off(tok, j * 8, D), o1, k_scale);
        if (pair) kv_put8<T, KV>(kb + k_off(tok, (j + rh8) * 8, D), o2, k_scale);
    }

    // ---- V: stage [token][d] rows, store [column group][d][8 token columns] runs ----------------------------------------------
    const int rws = D + 8;
    for (int it = tid; it < 32 * c8; it += 256) {
        const int tok = it / c8, j = it - tok * c8;
        V8 v = zero;
        if (tok < ntok) v = ld16<V8>(qkv + (int64_t)(t0 + i0 + tok) * ld + (int64_t)(H + Hkv + hk) * D + j * 8);
        st16(vs + tok * rws + j * 8, v);
    }
    __syncthreads();
    for (int it = tid; it < D * 4; it += 256) {
        const int d = it % D, c = it / D;  // columns c*8 .. c*8+7 of row d = tokens {c*4+e, 16+c*4+e}, e < 4
        V8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = vs[(c * 4 + e) * rws + d];
            o[e + 4] = vs[(16 + c * 4 + e) * rws + d];
        }
        kv_put8<T, KV>(vb + ((int64_t)c * D + d) * 8, o, v_scale);
    }
}

}  // namespace

// What both entry points check of the head shape, the norm and the tables; `fn` is the entry point's name.
#define QKN_CHECK_COMMON(fn)                                                                                             \
    do {                                                                                                                 \
        TGIS_CHECK_ARG(qkv, fn ": null qkv");                                                                            \
        TGIS_CHECK_ARG(D == 64 || D == 96 || D == 128, fn ": head_dim must be 64, 96 or 128, got %d", D);                \
        TGIS_CHECK_ARG(rot_dim > 0 && rot_dim <= D && rot_dim % 16 == 0,                                                 \
                       fn ": rot_dim must be a positive multiple of 16 and <= head_dim, got %d", rot_dim);               \
        TGIS_CHECK_ARG(q_norm_w && k_norm_w, fn ": null q_norm_w / k_norm_w");                                           \
        TGIS_CHECK_ARG(cos && sin && positions, fn ": null cos / sin / positions");                                      \
        TGIS_CHECK_ARG(eps > 0.f && eps < INFINITY, fn ": eps must be positive and finite");                             \
        TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, fn ": bad dtype");                                       \
        TGIS_CHECK_KV_ARGS(fn, kv_dtype, k_scale, v_scale);                                                              \
    } while (0)

static int qknorm_launch(void* qkv, int64_t ld_qkv, const float* slabs, int S, int64_t slab_ld, const void* bias,
                         const void* q_norm_w, const void* k_norm_w, float eps, const void* cos, const void* sin,
                         const int32_t* positions, const int32_t* slots, void* k_pool, void* v_pool, int64_t T, int H, int Hkv,
                         int D, int rot_dim, int dtype, int kv_dtype, float k_scale, float v_scale, hipStream_t st) {
    TgisTimedScope timed(TGIS_OP_ROPE_KV, st);
    const QkNormPlan plan = choose_qknorm(T, H, Hkv, D);
    const dim3 grid((unsigned)T, (unsigned)plan.gy);
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_kv<T>(kv_dtype == TGIS_KV_FP8_E4M3, [&](auto kv) {
            using KV = type_of<decltype(kv)>;
            PartialIn<T> pin{slabs, S, slab_ld, (const T*)bias};
            hipLaunchKernelGGL((qknorm_rope_kv_kernel<T, KV>), grid, dim3(256), 0, st, (T*)qkv, ld_qkv, (const T*)q_norm_w,
                               (const T*)k_norm_w, eps, (const T*)cos, (const T*)sin, positions, slots, (KV*)k_pool,
                               (KV*)v_pool, H, Hkv, D, rot_dim, pin, k_scale, v_scale);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}

extern "C" int tgis_rope_kv_write_qknorm(void* qkv, int64_t ld_qkv, const float* slabs, int num_slabs, int64_t slab_ld,
                                         const void* bias, const void* q_norm_w, const void* k_norm_w, float eps,
                                         const void* cos, const void* sin, const int32_t* positions, const int32_t* slots,
                                         void* k_pool, void* v_pool, int64_t T, int H, int Hkv, int D, int rot_dim, int dtype,
                                         int kv_dtype, float k_scale, float v_scale, void* stream) {
    QKN_CHECK_COMMON("tgis_rope_kv_write_qknorm");
    TGIS_CHECK_ARG(T >= 0 && T <= 2147483647LL && H > 0 && Hkv >= 0, "tgis_rope_kv_write_qknorm: bad sizes");
    TGIS_CHECK_ARG(ld_qkv % 8 == 0 && ld_qkv >= (int64_t)(H + 2 * Hkv) * D, "tgis_rope_kv_write_qknorm: bad row stride");
    TGIS_CHECK_ARG((!k_pool && !v_pool) || slots, "tgis_rope_kv_write_qknorm: cache write needs slots");
    TGIS_CHECK_ARG(!slabs || (num_slabs >= 1 && slab_ld >= (int64_t)(H + 2 * Hkv) * D && slab_ld % 4 == 0),
                   "tgis_rope_kv_write_qknorm: needs a slab row stride >= (H + 2 Hkv) D");
    TGIS_CHECK_ARG(slabs || !bias, "tgis_rope_kv_write_qknorm: a bias needs slabs");
    if (T == 0) return TGIS_OK;
    return qknorm_launch(qkv, ld_qkv, slabs, num_slabs, slab_ld, bias, q_norm_w, k_norm_w, eps, cos, sin, positions, slots,
                         k_pool, v_pool, T, H, Hkv, D, rot_dim, dtype, kv_dtype, k_scale, v_scale, (hipStream_t)stream);
}

extern "C" int tgis_rope_kv_write_prefill_qknorm(void* qkv, int64_t ld_qkv, const void* q_norm_w, const void* k_norm_w,
                                                 float eps, const void* cos, const void* sin, const int32_t* positions,
                                                 const int32_t* cu_seqlens, const int32_t* past_lens,
                                                 const int32_t* block_tables, int64_t max_pages, void* k_pool, void* v_pool,
                                                 int64_t B, int64_t T, int64_t max_len, int H, int Hkv, int D, int rot_dim,
                                                 int dtype, int kv_dtype, float k_scale, float v_scale, void* stream) {
    QKN_CHECK_COMMON("tgis_rope_kv_write_prefill_qknorm");
    TGIS_CHECK_ARG(cu_seqlens && block_tables && k_pool && v_pool, "tgis_rope_kv_write_prefill_qknorm: null tensor");
    TGIS_CHECK_ARG(B >= 0 && T >= 0 && T <= 2147483647LL && max_len >= 0 && max_pages > 0 && H > 0 && Hkv > 0,
                   "tgis_rope_kv_write_prefill_qknorm: bad sizes");
    TGIS_CHECK_ARG(ld_qkv % 8 == 0 && ld_qkv >= (int64_t)(H + 2 * Hkv) * D,
                   "tgis_rope_kv_write_prefill_qknorm: bad row stride");
    if (B == 0 || T == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    const QkNormPrefillPlan plan = choose_qknorm_prefill(max_len, D);
    const int pps = plan.pps;
    // (before the q launch: a refused call has launched nothing)
    TGIS_CHECK_ARG(pps <= max_pages && B * pps <= 2147483647LL && Hkv <= 65535,
                   "tgis_rope_kv_write_prefill_qknorm: grid too large");
    // q heads: normalised and rotated in place by the per-token kernel (no cache traffic: Hkv = 0, no pools)
    int rc = qknorm_launch(qkv, ld_qkv, nullptr, 0, 0, nullptr, q_norm_w, k_norm_w, eps, cos, sin, positions, nullptr, nullptr,
                           nullptr, T, H, 0, D, rot_dim, dtype, TGIS_KV_MODEL, 1.f, 1.f, st);
    if (rc != TGIS_OK) return rc;
    TgisTimedScope timed(TGIS_OP_ROPE_KV, st);
    const dim3 grid((unsigned)(B * pps), (unsigned)Hkv);
    const size_t lds = (size_t)32 * (D + 8) * 2 + 32 * sizeof(float);
    return by_dtype(dtype, [&](auto t) {
        using T = type_of<decltype(t)>;
        return by_kv<T>(kv_dtype == TGIS_KV_FP8_E4M3, [&](auto kv) {
            using KV = type_of<decltype(kv)>;
            hipLaunchKernelGGL((qknorm_rope_kv_prefill_kernel<T, KV>), grid, dim3(256), lds, st, (const T*)qkv, ld_qkv,
                               (const T*)k_norm_w, eps, (const T*)cos, (const T*)sin, positions, cu_seqlens, past_lens,
                               block_tables, max_pages, (KV*)k_pool, (KV*)v_pool, H, Hkv, D, rot_dim, pps, k_scale, v_scale);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}

// Host-only debug export (not in include/tgis_hip.h): the launch form without a launch.
//   op 0, per token: args = {T, H, Hkv, D} -> info = {gy, strided, heads, idle lanes per head group}
//   op 1, page-wise: args = {max_len, D}   -> info = {pages per sequence, statistics passes, k store passes}
extern "C" int tgis_debug_qknorm_plan(int op, const int64_t* args, int64_t* info) {
    TGIS_CHECK_ARG(args && info, "tgis_debug_qknorm_plan: null arguments");
    for (int i = 0; i < 4; ++i) info[i] = 0;
    const int64_t* a = args;
    if (op == 0) {
        TGIS_CHECK_ARG(a[0] >= 0 && a[1] > 0 && a[2] >= 0 && (a[3] == 64 || a[3] == 96 || a[3] == 128),
                       "tgis_debug_qknorm_plan: bad per-token shape");
        const QkNormPlan p = choose_qknorm(a[0], (int)a[1], (int)a[2], (int)a[3]);
        info[0] = p.gy, info[1] = p.strided, info[2] = p.heads, info[3] = p.idle;
        return TGIS_OK;
    }
    if (op == 1) {
        TGIS_CHECK_ARG(a[0] >= 0 && (a[1] == 64 || a[1] == 96 || a[1] == 128), "tgis_debug_qknorm_plan: bad page-wise shape");
        const QkNormPrefillPlan p = choose_qknorm_prefill(a[0], (int)a[1]);
        info[0] = p.pps, info[1] = p.stat_passes, info[2] = p.k_passes;
        return TGIS_OK;
    }
    TGIS_CHECK_ARG(false, "tgis_debug_qknorm_plan: unknown op %d", op);
    return TGIS_EINVAL;
}
