// Statistics of the paged KV cache: tgis_kv_absmax, the per-(k or v, kv head) max |x| over the tokens that a batch of
// sequences holds in one layer's 16-bit pools.  Calibration of the one-byte cache's per-layer scales is built on it
// (utils/kv_cache.py): the model runs with its ordinary cache and this kernel reads what it wrote.
// HBM-bound by construction: every valid 16-byte chunk is loaded once (sum ctx * 2 * Hkv * D * 2 bytes), the chunks of a
// partly filled page that hold no valid token are not loaded at all.
#include "dispatch.h"
#include "kv_layout.h"

namespace {

template <typename T> __device__ __forceinline__ float absmax8(typename VecT<T>::x8 v, uint32_t valid) {
    float m = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (valid >> e & 1) m = fmaxf(m, fabsf(to_f32(v[e])));
    return m;
}

// One block per (sequence b, page p of it, kv head).  Each lane loads 16 bytes: of K a chunk of 8 dims of ONE token (valid
// or not as a whole), of V a chunk of 8 token columns of ONE dim (valid per element, through v_col).  Max in registers, across
// the wave, across the block's 4 waves through LDS, then one atomicMax per block and statistic on the bit pattern of the
// non-negative float (monotone in the float's value).
template <typename T, int D>
__global__ __launch_bounds__(256) void kv_absmax_kernel(const T* __restrict__ kpool, const T* __restrict__ vpool,
                                                        const int32_t* __restrict__ bt, int64_t max_pages,
                                                        const int32_t* __restrict__ ctx_lens, int Hkv,
                                                        uint32_t* __restrict__ out) {
    using V8 = typename VecT<T>::x8;
    constexpr int C8 = D >> 3, CHUNKS = 32 * C8, ITERS = (CHUNKS + 255) / 256;  // K and V: 32 * D / 8 chunks each
    __shared__ int col_tok[32];   // token column of the V block -> token
    __shared__ float red[2][4];
    const int b = (int)(blockIdx.x / max_pages), p = (int)(blockIdx.x % max_pages), hk = blockIdx.y;
    const int ntok = min(32, ctx_lens[b] - p * 32);  // tokens of this page that count
    if (ntok <= 0) return;                           // past the sequence's last page: its table entry is not read
    const int page = bt[(int64_t)b * max_pages + p];
    const int tid = threadIdx.x;
    const T* kb = kpool + ((int64_t)page * Hkv + hk) * 32 * D;
    const T* vb = vpool + ((int64_t)page * Hkv + hk) * 32 * D;
    if (tid < 32) col_tok[v_col(tid)] = tid;
    __syncthreads();

    // every load is issued before the first value is looked at
    V8 kx[ITERS], vx[ITERS];
    uint32_t kval[ITERS], vval[ITERS];
#pragma unroll
    for (int r = 0; r < ITERS; ++r) {
        const int it = tid + r * 256;
        kval[r] = vval[r] = 0;
        if (CHUNKS % 256 != 0 && it >= CHUNKS) continue;
        // K: consecutive lanes = the 16 tokens of a tile, then the dim chunks, then the tile (the order of k_off)
        const int tok = (it / (16 * C8)) * 16 + (it & 15), j = (it >> 4) % C8;
        if (tok < ntok) {
            kval[r] = 0xFF;
            kx[r] = ld16<V8>(kb + k_off(tok, j * 8, D));
        }
        // V: consecutive lanes = the dims of one column group (the order of v_off); column cg * 8 + e holds token col_tok[..]
        const int cg = it / D, d = it - cg * D;
#pragma unroll
        for (int e = 0; e < 8; ++e) vval[r] |= (uint32_t)(col_tok[cg * 8 + e] < ntok) << e;
        if (vval[r]) vx[r] = ld16<V8>(vb + v_off(col_tok[cg * 8], d, D));
    }
    float km = 0.f, vm = 0.f;
#pragma unroll
    for (int r = 0; r < ITERS; ++r) {
        if (kval[r]) km = fmaxf(km, absmax8<T>(kx[r], kval[r]));
        if (vval[r]) vm = fmaxf(vm, absmax8<T>(vx[r], vval[r]));
    }
    km = wave_max(km);
    vm = wave_max(vm);
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = km;
        red[1][tid >> 6] = vm;
    }
    __syncthreads();
    if (tid < 2) {
        const float m = fmaxf(fmaxf(red[tid][0], red[tid][1]), fmaxf(red[tid][2], red[tid][3]));
        atomicMax(out + tid * Hkv + hk, __float_as_uint(m));
    }
}

}  // namespace

extern "C" int tgis_kv_absmax(const void* k_pool, const void* v_pool, const int32_t* block_tables, int64_t max_pages,
                              const int32_t* ctx_lens, int64_t B, int Hkv, int D, int dtype, float* out, void* stream) {
    TGIS_CHECK_ARG(k_pool && v_pool && out && (B <= 0 || (block_tables && ctx_lens)), "tgis_kv_absmax: null tensor");
    TGIS_CHECK_ARG(B >= 0 && max_pages > 0 && Hkv > 0, "tgis_kv_absmax: bad sizes");
    TGIS_CHECK_ARG(D == 64 || D == 96 || D == 128, "tgis_kv_absmax: head_dim %d is not 64, 96 or 128", D);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "tgis_kv_absmax: bad dtype %d (16-bit pools only)", dtype);
    TGIS_CHECK_ARG(B * max_pages <= 2147483647LL && Hkv <= 65535, "tgis_kv_absmax: grid too large");
    if (B == 0) return TGIS_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * max_pages), (unsigned)Hkv);
    return by_int<64, 96, 128>(D, "tgis_kv_absmax: head_dim", [&](auto d) {
        return by_dtype(dtype, [&](auto t) {
            using T = type_of<decltype(t)>;
            hipLaunchKernelGGL((kv_absmax_kernel<T, decltype(d)::value>), grid, dim3(256), 0, st, (const T*)k_pool,
                               (const T*)v_pool, block_tables, max_pages, ctx_lens, Hkv, (uint32_t*)out);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}
