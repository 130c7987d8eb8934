// Per-request LoRA adapters on prefills of any length: the delta of csrc/lora.hip over a TILE TABLE, gfx950.
//
//   tgis_lora_shrink_tiles  v[t, p, :] = A_s[p] x[t] in fp32 for the rows of the tiles
//   tgis_lora_expand_tiles  y[t, n] = T(float(y[t, n]) + scale_s sum_r v[t, p(n), r] B_s[n, r]), in place, for the rows of the tiles
//
// A prefill's rows arrive request by request, so the rows of a slot are contiguous and the host, which knows the requests'
// lengths, lists them: tiles int32 [n_tiles][4] = (row0, nrows, slot, 0) with 1 <= nrows <= 64, no tile across two slots, no
// tile for rows without an adapter.  The grids are sized by n_tiles, nothing is grouped on the device and nothing is read
// back.  The slot images, ranks and scales are those of csrc/lora.hip, read unchanged: of a tile's slot a block reads rank
// rounded up to 16 rows of A and as many 16-wide granules of B, and none of it when ranks[s] <= 0.  A tile that does not
// lie inside the T rows, or names no slot, is skipped (the table is device data: it cannot be checked before the launch).
//
// shrink: one block owns one tile and ALL P projections, so x[tile] leaves HBM once.  Its 8 waves split the k range; per
// half k64-step a wave loads its x fragments (both 32-row halves) once and reuses them across the P r16 / 32 column blocks
// of A_s (MFMA 32x32x16, A_s stays in L2 across the tiles of a slot): up to 2 x 6 accumulators of 16 floats.  The k-parts
// are summed through LDS, one column block per pass, in the fixed order 0..7.  Rows past nrows and ranks past r16 are
// computed on clamped addresses and never stored; the k tail is zeroed.
//
// expand: one block owns one tile x 128 columns, a wave 32 of them.  The tile's v [nrows][P][r16] is staged in LDS once
// (rows 4 floats apart from a multiple of 16, against bank conflicts); the wave's B granules are converted to fp32 in
// registers and multiplied with v_mfma_f32_32x32x2_f32, so v is never rounded: B is the M operand, v the N operand, so that
// a lane's accumulators are runs of 4 columns of ONE row, and one exchange between the wave's halves gives every lane 8
// contiguous columns: y is read, added to in fp32, rounded once and written in 16-byte vectors.  The two ranks of an MFMA
// step are r and r + 8 of a granule (a lane's 8 values of B and of v are then contiguous); a strip of columns that crosses
// a projection bound takes one pass per projection it touches, with the B lanes of the other projections' columns at zero.
//
// No float atomics, no cross-block waiting: the same input gives the same bytes.  The sums run in another order than in
// csrc/lora.hip, so the two paths agree within the contract's bound, not bit for bit.
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int TILE_ROWS = 64, TILES_MAX = 65535, TILES_MAX_S = 32, TILES_MAX_RANK = 64, TILES_MAX_P = 3;
constexpr int SHRINK_WK = 8, SHRINK_THREADS = 64 * SHRINK_WK;
constexpr int EXPAND_WAVES = 4, EXPAND_THREADS = 64 * EXPAND_WAVES, EXPAND_COLS = 32 * EXPAND_WAVES;
constexpr int V_PAD = 4;

struct Tile {
    int row0, nrows, slot;
};

__device__ __forceinline__ bool read_tile(const int32_t* tiles, int i, int64_t T, int S, Tile& t) {
    const int4 e = *reinterpret_cast<const int4*>(tiles + 4 * (int64_t)i);
    t.row0 = e.x, t.nrows = e.y, t.slot = e.z;
    return e.z >= 0 && e.z < S && e.y >= 1 && e.y <= TILE_ROWS && e.x >= 0 && (int64_t)e.x + e.y <= T;
}

__device__ __forceinline__ int tile_rank16(int rank, int max_rank) { return min((rank + 15) & ~15, max_rank); }

// ---- shrink ---------------------------------------------------------------------------------------------------------------
struct ShrinkTilesArgs {
    const void* x;
    int64_t ldx;
    const uint8_t* a_images;
    int64_t a_stride;
    const int32_t* ranks;
    const int32_t* tiles;
    float* v;  // [T, P max_rank]
    int64_t T;
    int K, KS, S, max_rank;
};

// NCB = P * PER column blocks of 32 ranks: PER per projection
template <typename T, int P, int PER>
__device__ __forceinline__ void shrink_tile_body(const ShrinkTilesArgs& a, float* red, const Tile& t, int r16) {
    using V8 = typename VecT<T>::x8;
    constexpr int NCB = P * PER;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wk = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int per_k = (a.KS + SHRINK_WK - 1) / SHRINK_WK;
    const int ks0 = min(wk * per_k, a.KS), ks1 = min(ks0 + per_k, a.KS);
    const int c = lane & 31, half_k = (lane >> 5) * 32;
    const bool two = t.nrows > 32;  // (the whole block agrees)
    // rows past the tile repeat its last row, ranks past r16 repeat the last one: their sums are never stored
    const T* x0 = reinterpret_cast<const T*>(a.x) + (int64_t)(t.row0 + min(c, t.nrows - 1)) * a.ldx;
    const T* x1 = reinterpret_cast<const T*>(a.x) + (int64_t)(t.row0 + min(32 + c, t.nrows - 1)) * a.ldx;
    const T* aimg = reinterpret_cast<const T*>(a.a_images + (int64_t)t.slot * a.a_stride);
    const int ar0 = min(c, r16 - 1), ar1 = min(32 + c, r16 - 1);

    f32x16 acc[2][NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][cb][r] = 0.f, acc[1][cb][r] = 0.f;

    for (int ks = ks0; ks < ks1; ++ks) {
#pragma unroll
        for (int ih = 0; ih < 2; ++ih) {
            V8 xv[2][2];
            int kc[2];
            bool past[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int kk = ks * 64 + half_k + (ih * 2 + i) * 8;  // K % 8 == 0: eight columns are all inside K or all past it
                kc[i] = min(kk, a.K - 8), past[i] = kk >= a.K;
                xv[0][i] = ld16<V8>(x0 + kc[i]);
                xv[1][i] = two ? ld16<V8>(x1 + kc[i]) : xv[0][i];
                if (past[i]) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[0][i][j] = (T)0.f, xv[1][i][j] = (T)0.f;
                }
            }
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const int p = cb / PER, ar = (cb % PER) ? ar1 : ar0;
                const T* arow = aimg + ((int64_t)p * a.max_rank + ar) * a.K;
                V8 av[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    av[i] = ld16<V8>(arow + kc[i]);
                    if (past[i]) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) av[i][j] = (T)0.f;
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    acc[0][cb] = mfma32(xv[0][i], av[i], acc[0][cb]);
                    if (two) acc[1][cb] = mfma32(xv[1][i], av[i], acc[1][cb]);
                }
            }
        }
    }

    // ---- k-parts through LDS, a column block per pass, summed in the fixed order 0..WK-1 --------------------------------
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int p = cb / PER, n = (cb % PER) * 32 + c;
        __syncthreads();  // (the previous pass has been read)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 0 || two) {
                float* dst = red + (((wk * 2 + h) * 64 + lane) << 4);
#pragma unroll
                for (int r = 0; r < 16; r += 4)
                    *reinterpret_cast<f32x4*>(dst + r) = f32x4{acc[h][cb][r], acc[h][cb][r + 1], acc[h][cb][r + 2], acc[h][cb][r + 3]};
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 0 || two) {
                float fin[2];
#pragma unroll
                for (int k2 = 0; k2 < SHRINK_WK; ++k2) {
                    const f32x2 part = *reinterpret_cast<const f32x2*>(red + (((k2 * 2 + h) * 64 + lane) << 4) + wk * 2);
                    fin[0] = k2 == 0 ? part[0] : fin[0] + part[0];
                    fin[1] = k2 == 0 ? part[1] : fin[1] + part[1];
                }
                // accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int r = wk * 2 + j;
                    const int m = h * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    if (m < t.nrows && n < r16) a.v[((int64_t)(t.row0 + m) * P + p) * a.max_rank + n] = fin[j];
                }
            }
        }
    }
}

template <typename T, int P>
__global__ __launch_bounds__(SHRINK_THREADS) void lora_shrink_tiles_kernel(ShrinkTilesArgs a) {
    __shared__ __attribute__((aligned(16))) float red[SHRINK_WK * 2 * 64 * 16];
    Tile t;
    if (!read_tile(a.tiles, blockIdx.x, a.T, a.S, t)) return;
    const int rank = a.ranks[t.slot];
    if (rank <= 0) return;  // the slot holds no adapter for this linear: not one byte of its image is read
    const int r16 = tile_rank16(rank, a.max_rank);
    if (r16 <= 32) shrink_tile_body<T, P, 1>(a, red, t, r16);
    else shrink_tile_body<T, P, 2>(a, red, t, r16);
}

// ---- expand ---------------------------------------------------------------------------------------------------------------
struct ExpandTilesArgs {
    const float* v;  // [T, P max_rank]
    const uint8_t* b_images;
    int64_t b_stride;
    const int32_t* ranks;
    const float* scales;
    const int32_t* tiles;
    void* y;
    int64_t ldy, T;
    int N, P, S, max_rank;
    int vec;  // rows of y are 16-byte aligned
    int bounds[TILES_MAX_P + 1];
};

// y[0 .. 8) = T(float(y) + scale d)
template <typename T>
__device__ __forceinline__ void add_round8(T* yp, const float (&d)[8], float scale, bool vec) {
    using V8 = typename VecT<T>::x8;
    if (vec) {
        V8 yv = ld16<V8>(yp);
#pragma unroll
        for (int j = 0; j < 8; ++j) yv[j] = from_f32<T>(to_f32(yv[j]) + scale * d[j]);
        st16<V8>(yp, yv);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) yp[j] = from_f32<T>(to_f32(yp[j]) + scale * d[j]);
    }
}

// NG granules of 16 ranks: the lane's half of its column's B row sits in 8 NG registers
template <typename T, int NG>
__device__ __forceinline__ void expand_tile_body(const ExpandTilesArgs& a, float* vs, const Tile& t) {
    using V8 = typename VecT<T>::x8;
    constexpr int R = 16 * NG;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int n0 = blockIdx.x * EXPAND_COLS + wave * 32, n = n0 + c;
    const bool live = n0 < a.N;  // (the whole wave agrees)

    // the lane's B values: ranks 8 h .. 8 h + 7 of every granule of column n (a column at or past N repeats the last one)
    float bf[NG * 8];
    if (live) {
        const T* bcol = reinterpret_cast<const T*>(a.b_images + (int64_t)t.slot * a.b_stride) + (int64_t)min(n, a.N - 1) * 16 + h * 8;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const V8 b8 = ld16<V8>(bcol + (int64_t)g * a.N * 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) bf[g * 8 + j] = to_f32(b8[j]);
        }
    }
    // the tile's v into LDS: [nrows][P R] with rows V_PAD floats further apart
    const int vrow = a.P * R, stride = vrow + V_PAD;
    for (int i = tid * 4; i < t.nrows * vrow; i += EXPAND_THREADS * 4) {
        const int row = i / vrow, rem = i - row * vrow, q = rem / R, r = rem - q * R;
        *reinterpret_cast<f32x4*>(vs + row * stride + rem) =
            *reinterpret_cast<const f32x4*>(a.v + ((int64_t)(t.row0 + row) * a.P + q) * a.max_rank + r);
    }
    __syncthreads();
    if (!live) return;

    const bool two = t.nrows > 32;  // (the whole block agrees)
    // rows past the tile repeat its last row: their sums are never stored
    const float* v0 = vs + min(c, t.nrows - 1) * stride + h * 8;
    const float* v1 = vs + min(32 + c, t.nrows - 1) * stride + h * 8;
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.f, acc[1][r] = 0.f;
#pragma unroll
    for (int p = 0; p < TILES_MAX_P; ++p) {
        if (p >= a.P) break;
        const int lo = a.bounds[p], hi = a.bounds[p + 1];
        if (hi <= n0 || lo >= n0 + 32) continue;  // the strip has no column of this projection
        const bool mine = n >= lo && n < hi;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float va[8], vb[8];
#pragma unroll
            for (int j = 0; j < 8; j += 4) {
                const f32x4 q0 = *reinterpret_cast<const f32x4*>(v0 + p * R + g * 16 + j);
                const f32x4 q1 = two ? *reinterpret_cast<const f32x4*>(v1 + p * R + g * 16 + j) : q0;
#pragma unroll
                for (int k = 0; k < 4; ++k) va[j + k] = q0[k], vb[j + k] = q1[k];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float b = mine ? bf[g * 8 + j] : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, va[j], acc[0], 0, 0, 0);
                if (two) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, vb[j], acc[1], 0, 0, 0);
            }
        }
    }

    // accumulator register r of lane (c, h) is column n0 + (r & 3) + 8 (r >> 2) + 4 h of row c: the halves exchange runs of
    // four, so that lane (c, h) holds the column groups 8 q .. 8 q + 7 with q = 2 i + h
    const float scale = a.scales[t.slot];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
        if (hh == 1 && !two) break;
        const int row = hh * 32 + c;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float d[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float own_lo = acc[hh][8 * i + k], own_hi = acc[hh][8 * i + 4 + k];
                const float got = __shfl_xor(h ? own_lo : own_hi, 32, 64);
                d[k] = h ? got : own_lo;
                d[4 + k] = h ? own_hi : got;
            }
            const int col = n0 + 8 * (2 * i + h);  // N % 8 == 0: eight columns are all inside N or all past it
            if (row < t.nrows && col < a.N)
                add_round8<T>(reinterpret_cast<T*>(a.y) + (int64_t)(t.row0 + row) * a.ldy + col, d, scale, a.vec != 0);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(EXPAND_THREADS) void lora_expand_tiles_kernel(ExpandTilesArgs a) {
    extern __shared__ __attribute__((aligned(16))) float vs[];  // TILE_ROWS (P max_rank + V_PAD) floats
    Tile t;
    if (!read_tile(a.tiles, blockIdx.y, a.T, a.S, t)) return;
    const int rank = a.ranks[t.slot];
    if (rank <= 0) return;  // its rows of y are not touched, its image is not read
    switch (tile_rank16(rank, a.max_rank) >> 4) {
        case 1: expand_tile_body<T, 1>(a, vs, t); break;
        case 2: expand_tile_body<T, 2>(a, vs, t); break;
        case 3: expand_tile_body<T, 3>(a, vs, t); break;
        default: expand_tile_body<T, 4>(a, vs, t); break;
    }
}

int tiles_check_shape(const char* fn, int64_t T, int64_t n_tiles, int P, int S, int max_rank, int dtype) {
    TGIS_CHECK_ARG(T >= 0 && T < (1ll << 31) - TILE_ROWS, "%s: 0 <= T < 2^31 - %d rows (T=%ld)", fn, TILE_ROWS, (long)T);
    TGIS_CHECK_ARG(n_tiles >= 0 && n_tiles <= TILES_MAX, "%s: 0 <= n_tiles <= %d (n_tiles=%ld)", fn, TILES_MAX, (long)n_tiles);
    TGIS_CHECK_ARG(S >= 1 && S <= TILES_MAX_S, "%s: 1 <= S <= %d slots (S=%d)", fn, TILES_MAX_S, S);
    TGIS_CHECK_ARG(P >= 1 && P <= TILES_MAX_P, "%s: 1 <= P <= %d fused projections (P=%d)", fn, TILES_MAX_P, P);
    TGIS_CHECK_ARG(max_rank >= 16 && max_rank <= TILES_MAX_RANK && max_rank % 16 == 0,
                   "%s: max_rank (%d) must be a multiple of 16, at most %d", fn, max_rank, TILES_MAX_RANK);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "%s: bad dtype", fn);
    return TGIS_OK;
}

}  // namespace

extern "C" int tgis_lora_shrink_tiles(const void* x, int64_t ldx, const void* a_images, int64_t a_stride, const int32_t* ranks,
                                      const int32_t* tiles, int64_t n_tiles, float* v, int64_t T, int64_t K, int P, int S,
                                      int max_rank, int dtype, void* stream) {
    const int rc = tiles_check_shape("tgis_lora_shrink_tiles", T, n_tiles, P, S, max_rank, dtype);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(K > 0 && K % 8 == 0 && K < (1ll << 30), "tgis_lora_shrink_tiles: K (%ld) must be a positive multiple of 8",
                   (long)K);
    TGIS_CHECK_ARG(a_images && ranks, "tgis_lora_shrink_tiles: null tensor");
    TGIS_CHECK_ARG(a_stride >= tgis_lora_a_bytes(K, P, max_rank) && a_stride % 16 == 0 && ((uintptr_t)a_images % 16) == 0,
                   "tgis_lora_shrink_tiles: the slot stride (%ld) must hold one A image, 16-byte aligned", (long)a_stride);
    if (T == 0 || n_tiles == 0) return TGIS_OK;
    TGIS_CHECK_ARG(x && tiles && v, "tgis_lora_shrink_tiles: null tensor");
    TGIS_CHECK_ARG(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                       ((uintptr_t)tiles % 16) == 0,
                   "tgis_lora_shrink_tiles: rows of the activation, v and the tile table must be 16-byte aligned");
    ShrinkTilesArgs a;
    a.x = x, a.ldx = ldx, a.a_images = (const uint8_t*)a_images, a.a_stride = a_stride;
    a.ranks = ranks, a.tiles = tiles, a.v = v, a.T = T;
    a.K = (int)K, a.KS = (int)cdiv64(K, 64), a.S = S, a.max_rank = max_rank;
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        return by_int<1, 2, 3>(P, "tgis_lora_shrink_tiles", [&](auto p) {
            hipLaunchKernelGGL((lora_shrink_tiles_kernel<T_, decltype(p)::value>), dim3((unsigned)n_tiles), dim3(SHRINK_THREADS), 0,
                               (hipStream_t)stream, a);
            TGIS_CHECK_LAUNCH();
            return TGIS_OK;
        });
    });
}

extern "C" int tgis_lora_expand_tiles(const float* v, const void* b_images, int64_t b_stride, const int32_t* ranks,
                                      const float* scales, const int32_t* tiles, int64_t n_tiles, const int64_t* bounds,
                                      void* y, int64_t ldy, int64_t T, int64_t N, int P, int S, int max_rank, int dtype,
                                      void* stream) {
    const int rc = tiles_check_shape("tgis_lora_expand_tiles", T, n_tiles, P, S, max_rank, dtype);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(N > 0 && N % 8 == 0 && N < (1ll << 30), "tgis_lora_expand_tiles: N (%ld) must be a positive multiple of 8",
                   (long)N);
    TGIS_CHECK_ARG(b_images && ranks && scales && bounds, "tgis_lora_expand_tiles: null tensor");
    TGIS_CHECK_ARG(b_stride >= tgis_lora_b_bytes(N, max_rank) && b_stride % 16 == 0 && ((uintptr_t)b_images % 16) == 0,
                   "tgis_lora_expand_tiles: the slot stride (%ld) must hold one B image, 16-byte aligned", (long)b_stride);
    TGIS_CHECK_ARG(bounds[0] == 0 && bounds[P] == N, "tgis_lora_expand_tiles: the column bounds must run from 0 to N");
    for (int p = 0; p < P; ++p)
        TGIS_CHECK_ARG(bounds[p + 1] > bounds[p] && bounds[p + 1] % 8 == 0,
                       "tgis_lora_expand_tiles: the column bounds must ascend in multiples of 8 (bounds[%d]=%ld)", p + 1,
                       (long)bounds[p + 1]);
    if (T == 0 || n_tiles == 0) return TGIS_OK;
    TGIS_CHECK_ARG(v && tiles && y, "tgis_lora_expand_tiles: null tensor");
    TGIS_CHECK_ARG(ldy >= N && ((uintptr_t)v % 16) == 0 && ((uintptr_t)tiles % 16) == 0 && ((uintptr_t)y % 2) == 0,
                   "tgis_lora_expand_tiles: rows of y must hold N elements, v and the tile table 16-byte aligned");
    ExpandTilesArgs a;
    a.v = v, a.b_images = (const uint8_t*)b_images, a.b_stride = b_stride, a.ranks = ranks, a.scales = scales;
    a.tiles = tiles, a.y = y, a.ldy = ldy, a.T = T;
    a.N = (int)N, a.P = P, a.S = S, a.max_rank = max_rank;
    a.vec = ldy % 8 == 0 && ((uintptr_t)y % 16) == 0;
    for (int p = 0; p <= TILES_MAX_P; ++p) a.bounds[p] = (int)bounds[p <= P ? p : P];
    const size_t lds = sizeof(float) * TILE_ROWS * (P * max_rank + V_PAD);
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        hipLaunchKernelGGL(lora_expand_tiles_kernel<T_>, dim3((unsigned)cdiv64(N, EXPAND_COLS), (unsigned)n_tiles),
                           dim3(EXPAND_THREADS), lds, (hipStream_t)stream, a);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}
