// Per-request LoRA adapters beside a base linear: y[t] = W x[t] + scale_s B_s (A_s x[t]) with s = slot[t], gfx950.
//
//   tgis_lora_group   int32 slot[T] (-1 .. S-1) -> the rows grouped by slot: counts, offsets, rows (ascending inside a slot).
//                     Integer work only; once per forward, read by every linear of every layer.
//   tgis_lora_shrink  v[t, p, :] = A_s[p] x[t] in fp32 for the rows that have a slot (P projections fused into the base linear)
//   tgis_lora_expand  y[t, n] = T(float(y[t, n]) + scale_s sum_r v[t, p(n), r] B_s[n, r]), in place on the base GEMM's output
//
// Both GEMMs read the grouping on the device, as the routed-expert GEMMs of moe.hip read their routing: the grid covers every
// slot whatever the step brings, so the launches can sit in a captured decode graph.  A block reads offsets[s] and ranks[s] and
// returns at once when no row names the slot or the slot's linear holds no adapter: not one byte of that slot's images is
// read.  Of a named slot it reads rank rounded up to 16 rows of A and as many 16-wide granules of B, and nothing behind them.
//
// Slot images (one pair per wrapped linear, S slots `stride` bytes apart, filled by a stream-ordered copy when an adapter is
// loaded; ranks int32 [S] and scales f32 [S] beside them):
//   A  [P][max_rank][K]       row-major in the model dtype; rows from the adapter's rank up to the next multiple of 16 are zero
//   B  [max_rank / 16][N][16] granule g holds columns 16 g .. 16 g + 15 of B [N, r], so that a step reads contiguous granules
//
// shrink: a block owns (32 ranks, one projection, one slot) and walks the slot's rows in 32-row slabs; its 8 waves split the k
// range (MFMA 32x32x16, both operands straight from global memory: nothing is reused inside a block), the k-parts are summed
// through LDS in the fixed order 0..7.  expand: a thread owns one output column, keeps its B row in registers and walks the
// slot's rows, v staged through LDS 16 rows at a time; the sum over r runs in ascending order.  No float atomics and no
// cross-block waiting in either: the same input gives the same bytes, whatever the order of launches.
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int LORA_MAX_T = 64, LORA_MAX_S = 32, LORA_MAX_RANK = 64, LORA_MAX_P = 3;
constexpr int GROUP_THREADS = 1024;
constexpr int SHRINK_WK = 8, SHRINK_THREADS = 64 * SHRINK_WK;
constexpr int EXPAND_THREADS = 128, EXPAND_ROWS = 16;

// ---- grouping -------------------------------------------------------------------------------------------------------------
// One block, a slot per wave (ballot + popcount over the T <= 64 rows), offsets by one thread, then the rows behind offsets[s]
// in ascending order.  A value outside -1 .. S-1 names no slot.
__global__ __launch_bounds__(GROUP_THREADS) void lora_group_kernel(const int32_t* __restrict__ slot, int T, int S,
                                                                   int32_t* __restrict__ counts, int32_t* __restrict__ offsets,
                                                                   int32_t* __restrict__ rows) {
    __shared__ int s_cnt[LORA_MAX_S];
    __shared__ int s_off[LORA_MAX_S + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mine = lane < T ? slot[lane] : -1;
    for (int s = wave; s < S; s += GROUP_THREADS / 64) {
        const int c = __popcll(__ballot(mine == s));
        if (lane == 0) s_cnt[s] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int s = 0; s < S; ++s) {
            s_off[s] = run;
            offsets[s] = run;
            counts[s] = s_cnt[s];
            run += s_cnt[s];
        }
        s_off[S] = run;
        offsets[S] = run;
    }
    __syncthreads();
    for (int s = wave; s < S; s += GROUP_THREADS / 64) {
        const uint64_t m = __ballot(mine == s);
        if (mine == s) rows[s_off[s] + __popcll(m & ((1ull << lane) - 1))] = lane;
    }
}

// ---- shrink ---------------------------------------------------------------------------------------------------------------
struct ShrinkArgs {
    const void* x;
    int64_t ldx;
    const uint8_t* a_images;
    int64_t a_stride;
    const int32_t* ranks;
    const int32_t* offsets;
    const int32_t* rows;
    float* v;  // [T, P max_rank]
    int K, KS, P, max_rank;
};

__device__ __forceinline__ int rank16(int rank, int max_rank) { return min((rank + 15) & ~15, max_rank); }

template <typename T>
__global__ __launch_bounds__(SHRINK_THREADS) void lora_shrink_kernel(ShrinkArgs a) {
    using V8 = typename VecT<T>::x8;
    __shared__ __attribute__((aligned(16))) float red[SHRINK_WK * 64 * 16];
    const int rt = blockIdx.x, p = blockIdx.y, s = blockIdx.z;
    const int row0 = a.offsets[s], cnt = a.offsets[s + 1] - row0;
    if (cnt <= 0) return;  // no row names this slot
    const int rank = a.ranks[s];
    if (rank <= 0) return;  // the slot holds no adapter for this linear
    const int r16 = rank16(rank, a.max_rank);
    if (rt * 32 >= r16) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wk = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per = (a.KS + SHRINK_WK - 1) / SHRINK_WK;
    const int ks0 = min(wk * per, a.KS), ks1 = min(ks0 + per, a.KS);
    const int c = lane & 31, half_k = (lane >> 5) * 32;
    // the lane's row of A_s[p]: ranks past r16 repeat the last one (their sums are never stored)
    const int ar = min(rt * 32 + c, r16 - 1);
    const T* arow = reinterpret_cast<const T*>(a.a_images + (int64_t)s * a.a_stride) + ((int64_t)p * a.max_rank + ar) * a.K;

    for (int slab = 0; slab * 32 < cnt; ++slab) {
        const int nrows = min(32, cnt - slab * 32);
        // rows past the slot's list repeat its last row
        const int t = a.rows[row0 + slab * 32 + min(c, nrows - 1)];
        const T* xrow = reinterpret_cast<const T*>(a.x) + (int64_t)t * a.ldx;
        f32x16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
        for (int ks = ks0; ks < ks1; ++ks) {
            V8 xv[4], av[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = ks * 64 + half_k + i * 8;  // K % 8 == 0: eight columns are all inside K or all past it
                const int kc = min(kk, a.K - 8);
                xv[i] = ld16<V8>(xrow + kc);
                av[i] = ld16<V8>(arow + kc);
                if (kk >= a.K) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[i][j] = (T)0.f, av[i][j] = (T)0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i & 1) acc1 = mfma32(xv[i], av[i], acc1);
                else acc0 = mfma32(xv[i], av[i], acc0);
            }
        }
        const f32x16 acc = acc0 + acc1;
        // ---- k-parts through LDS, summed in the fixed order 0..WK-1 ----------------------------------------------------
        __syncthreads();  // (the previous slab's exchange has been read)
        {
            float* dst = red + ((wk * 64 + lane) << 4);
#pragma unroll
            for (int r = 0; r < 16; r += 4)
                *reinterpret_cast<f32x4*>(dst + r) = f32x4{acc[r], acc[r + 1], acc[r + 2], acc[r + 3]};
        }
        __syncthreads();
        float fin[2];
#pragma unroll
        for (int k2 = 0; k2 < SHRINK_WK; ++k2) {
            const f32x2 part = *reinterpret_cast<const f32x2*>(red + ((k2 * 64 + lane) << 4) + wk * 2);
            fin[0] = k2 == 0 ? part[0] : fin[0] + part[0];
            fin[1] = k2 == 0 ? part[1] : fin[1] + part[1];
        }
        // accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = wk * 2 + j;
            const int m = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int n = rt * 32 + c;
            if (m < nrows && n < r16) {
                const int to = a.rows[row0 + slab * 32 + m];
                a.v[((int64_t)to * a.P + p) * a.max_rank + n] = fin[j];
            }
        }
    }
}

// ---- expand ---------------------------------------------------------------------------------------------------------------
struct ExpandArgs {
    const float* v;  // [T, P max_rank]
    const uint8_t* b_images;
    int64_t b_stride;
    const int32_t* ranks;
    const float* scales;
    const int32_t* offsets;
    const int32_t* rows;
    void* y;
    int64_t ldy;
    int N, P, max_rank;
    int bounds[LORA_MAX_P + 1];
};

// NG granules of 16 ranks: the thread's B row sits in 16 NG registers
template <typename T, int NG>
__device__ __forceinline__ void lora_expand_body(const ExpandArgs& a, float* vs, int s, int row0, int cnt) {
    using V8 = typename VecT<T>::x8;
    constexpr int R = 16 * NG;
    const int tid = threadIdx.x;
    const int n = blockIdx.x * EXPAND_THREADS + tid;
    const bool live = n < a.N;
    int p = 0;
#pragma unroll
    for (int q = 1; q < LORA_MAX_P; ++q)
        if (q < a.P && n >= a.bounds[q]) p = q;
    float b[R];
    const T* bimg = reinterpret_cast<const T*>(a.b_images + (int64_t)s * a.b_stride);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const T* src = bimg + ((int64_t)g * a.N + (live ? n : 0)) * 16;
        const V8 lo = ld16<V8>(src), hi = ld16<V8>(src + 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) b[g * 16 + j] = to_f32(lo[j]), b[g * 16 + 8 + j] = to_f32(hi[j]);
    }
    const float scale = a.scales[s];
    const int vrow = a.P * R;  // floats of one staged row: [P][R]
    for (int base = 0; base < cnt; base += EXPAND_ROWS) {
        const int nrows = min(EXPAND_ROWS, cnt - base);
        __syncthreads();  // (the previous chunk has been read)
        for (int i = tid * 4; i < nrows * vrow; i += EXPAND_THREADS * 4) {
            const int row = i / vrow, rem = i - row * vrow, q = rem / R, r = rem - q * R;
            const int t = a.rows[row0 + base + row];
            *reinterpret_cast<f32x4*>(vs + i) =
                *reinterpret_cast<const f32x4*>(a.v + ((int64_t)t * a.P + q) * a.max_rank + r);
        }
        __syncthreads();
        if (live) {
            for (int row = 0; row < nrows; ++row) {
                const int t = a.rows[row0 + base + row];
                const float* vp = vs + row * vrow + p * R;
                float acc = 0.f;
#pragma unroll
                for (int r = 0; r < R; r += 4) {
                    const f32x4 vv = *reinterpret_cast<const f32x4*>(vp + r);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc += vv[j] * b[r + j];
                }
                T* yp = reinterpret_cast<T*>(a.y) + (int64_t)t * a.ldy + n;
                *yp = from_f32<T>(to_f32(*yp) + scale * acc);
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(EXPAND_THREADS) void lora_expand_kernel(ExpandArgs a) {
    __shared__ __attribute__((aligned(16))) float vs[EXPAND_ROWS * LORA_MAX_P * LORA_MAX_RANK];
    const int s = blockIdx.y;
    const int row0 = a.offsets[s], cnt = a.offsets[s + 1] - row0;
    if (cnt <= 0) return;  // no row names this slot: its rows of y are not touched, its image is not read
    const int rank = a.ranks[s];
    if (rank <= 0) return;
    switch (rank16(rank, a.max_rank) >> 4) {
        case 1: lora_expand_body<T, 1>(a, vs, s, row0, cnt); break;
        case 2: lora_expand_body<T, 2>(a, vs, s, row0, cnt); break;
        case 3: lora_expand_body<T, 3>(a, vs, s, row0, cnt); break;
        default: lora_expand_body<T, 4>(a, vs, s, row0, cnt); break;
    }
}

int lora_check_shape(const char* fn, int64_t T, int P, int S, int max_rank, int dtype) {
    TGIS_CHECK_ARG(T >= 0 && T <= LORA_MAX_T, "%s: 0 <= T <= %d rows (T=%ld)", fn, LORA_MAX_T, (long)T);
    TGIS_CHECK_ARG(S >= 1 && S <= LORA_MAX_S, "%s: 1 <= S <= %d slots (S=%d)", fn, LORA_MAX_S, S);
    TGIS_CHECK_ARG(P >= 1 && P <= LORA_MAX_P, "%s: 1 <= P <= %d fused projections (P=%d)", fn, LORA_MAX_P, P);
    TGIS_CHECK_ARG(max_rank >= 16 && max_rank <= LORA_MAX_RANK && max_rank % 16 == 0,
                   "%s: max_rank (%d) must be a multiple of 16, at most %d", fn, max_rank, LORA_MAX_RANK);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "%s: bad dtype", fn);
    return TGIS_OK;
}

}  // namespace

extern "C" int64_t tgis_lora_a_bytes(int64_t K, int P, int max_rank) {
    if (K <= 0 || P < 1 || max_rank < 1) return 0;
    return (int64_t)P * max_rank * K * 2;
}

extern "C" int64_t tgis_lora_b_bytes(int64_t N, int max_rank) {
    if (N <= 0 || max_rank < 1) return 0;
    return (int64_t)max_rank * N * 2;
}

extern "C" int tgis_lora_group(const int32_t* slot, int64_t T, int S, int32_t* counts, int32_t* offsets, int32_t* rows,
                               void* stream) {
    TGIS_CHECK_ARG(T >= 0 && T <= LORA_MAX_T, "tgis_lora_group: 0 <= T <= %d rows (T=%ld)", LORA_MAX_T, (long)T);
    TGIS_CHECK_ARG(S >= 1 && S <= LORA_MAX_S, "tgis_lora_group: 1 <= S <= %d slots (S=%d)", LORA_MAX_S, S);
    TGIS_CHECK_ARG(counts && offsets && (T == 0 || (slot && rows)), "tgis_lora_group: null tensor");
    hipLaunchKernelGGL(lora_group_kernel, dim3(1), dim3(GROUP_THREADS), 0, (hipStream_t)stream, slot, (int)T, S, counts, offsets,
                       rows);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int tgis_lora_shrink(const void* x, int64_t ldx, const void* a_images, int64_t a_stride, const int32_t* ranks,
                                const int32_t* offsets, const int32_t* rows, float* v, int64_t T, int64_t K, int P, int S,
                                int max_rank, int dtype, void* stream) {
    const int rc = lora_check_shape("tgis_lora_shrink", T, P, S, max_rank, dtype);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(K > 0 && K % 8 == 0 && K < (1ll << 30), "tgis_lora_shrink: K (%ld) must be a positive multiple of 8", (long)K);
    TGIS_CHECK_ARG(a_images && ranks && offsets, "tgis_lora_shrink: null tensor");
    TGIS_CHECK_ARG(a_stride >= tgis_lora_a_bytes(K, P, max_rank) && a_stride % 16 == 0 && ((uintptr_t)a_images % 16) == 0,
                   "tgis_lora_shrink: the slot stride (%ld) must hold one A image, 16-byte aligned", (long)a_stride);
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(x && rows && v, "tgis_lora_shrink: null tensor");
    TGIS_CHECK_ARG(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)v % 16) == 0,
                   "tgis_lora_shrink: rows of the activation and v must be 16-byte aligned");
    ShrinkArgs a;
    a.x = x, a.ldx = ldx, a.a_images = (const uint8_t*)a_images, a.a_stride = a_stride;
    a.ranks = ranks, a.offsets = offsets, a.rows = rows, a.v = v;
    a.K = (int)K, a.KS = (int)cdiv64(K, 64), a.P = P, a.max_rank = max_rank;
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        hipLaunchKernelGGL(lora_shrink_kernel<T_>, dim3((unsigned)cdiv64(max_rank, 32), (unsigned)P, (unsigned)S),
                           dim3(SHRINK_THREADS), 0, (hipStream_t)stream, a);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}

extern "C" int tgis_lora_expand(const float* v, const void* b_images, int64_t b_stride, const int32_t* ranks,
                                const float* scales, const int32_t* offsets, const int32_t* rows, const int64_t* bounds,
                                void* y, int64_t ldy, int64_t T, int64_t N, int P, int S, int max_rank, int dtype,
                                void* stream) {
    const int rc = lora_check_shape("tgis_lora_expand", T, P, S, max_rank, dtype);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(N > 0 && N % 8 == 0 && N < (1ll << 30), "tgis_lora_expand: N (%ld) must be a positive multiple of 8", (long)N);
    TGIS_CHECK_ARG(b_images && ranks && scales && offsets && bounds, "tgis_lora_expand: null tensor");
    TGIS_CHECK_ARG(b_stride >= tgis_lora_b_bytes(N, max_rank) && b_stride % 16 == 0 && ((uintptr_t)b_images % 16) == 0,
                   "tgis_lora_expand: the slot stride (%ld) must hold one B image, 16-byte aligned", (long)b_stride);
    TGIS_CHECK_ARG(bounds[0] == 0 && bounds[P] == N, "tgis_lora_expand: the column bounds must run from 0 to N");
    for (int p = 0; p < P; ++p)
        TGIS_CHECK_ARG(bounds[p + 1] > bounds[p] && bounds[p + 1] % 8 == 0,
                       "tgis_lora_expand: the column bounds must ascend in multiples of 8 (bounds[%d]=%ld)", p + 1,
                       (long)bounds[p + 1]);
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(v && rows && y, "tgis_lora_expand: null tensor");
    TGIS_CHECK_ARG(ldy >= N && ((uintptr_t)v % 16) == 0, "tgis_lora_expand: rows of y must hold N elements, v 16-byte aligned");
    ExpandArgs a;
    a.v = v, a.b_images = (const uint8_t*)b_images, a.b_stride = b_stride, a.ranks = ranks, a.scales = scales;
    a.offsets = offsets, a.rows = rows, a.y = y, a.ldy = ldy;
    a.N = (int)N, a.P = P, a.max_rank = max_rank;
    for (int p = 0; p <= LORA_MAX_P; ++p) a.bounds[p] = (int)bounds[p <= P ? p : P];
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        hipLaunchKernelGGL(lora_expand_kernel<T_>, dim3((unsigned)cdiv64(N, EXPAND_THREADS), (unsigned)S), dim3(EXPAND_THREADS), 0,
                           (hipStream_t)stream, a);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}
