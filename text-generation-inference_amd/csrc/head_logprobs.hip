// Prompt-token scores from the output head without its [T, V] logits, gfx950 (details.input_toks; utils/tokens.py
// get_input_tokens_info: log_softmax + gather + rank compare over all T prompt rows).
//
//   tgis_head_logprobs   z[t, v] = sum_k x[t, k] W[v, k] in fp32, never stored;  per row t with target g = targets[t]:
//                        lse[t] = logsumexp_v z[t, v],  logprob[t] = z[t, g] - lse[t],  rank[t] = 1 + #{v != g : z[t, v] > z[t, g]}
//
// x [T, K] (row stride ldx) and W [V, K] are row-major in the model dtype: W is the head's checkpoint tensor, both operands
// are K-contiguous.  Three launches on the caller's stream, no atomics, no cross-block waiting: the same input gives the
// same bytes.
//
// target: one wave per row, zt[t] = x[t] . W[g] in fp32.  This ONE value is the row's target logit, in logprob and in every
// comparison of the count; the sweep leaves column g out of the count, so the rounding difference between this sum and the
// MFMA's can never make a token outrank itself.  A target outside [0, V) (the host's -1) gives zt = NaN: nothing compares
// greater, and the merge writes logprob NaN, rank 0.
//
// sweep: grid (S vocabulary splits, ceil(T / 128) row tiles), 4 waves.  A block keeps its 128 rows and walks its range of
// 128-column tiles; the k-loop runs on through the tiles (tile, k64-step) so that the next step's 16-byte global loads (four
// of x, four of W per thread) are in flight while the MFMAs of this step read LDS: two buffers, rows 72 elements apart (144
// bytes: the 32 rows of a fragment read then start in 16 different 4-bank groups, twice each), one barrier per step.  The
// product is W x^T with v_mfma_f32_32x32x16: W is the M operand, x the N operand, so a lane holds ONE token (its wave's row
// lane % 32) and 16 of the 32 vocabulary rows of each of the wave's four accumulators.  After a tile's last k-step the lane
// folds its 64 logits into its own running (max, sum of exp(z - max), count(z > zt)) — register-local; columns >= V count
// as -inf.  The two lanes of a token meet once, after the block's last tile, in one exchange across the half-waves, and
// lane % 64 < 32 writes the row's record {max, sum, count} of this split as one 16-byte store.  Rows >= T and columns >= V
// are computed on clamped addresses and never stored; a K that is no multiple of 64 zeroes the pieces past it.
//
// merge: one thread per row folds its S records in the order 0 .. S - 1 and writes lse, logprob, rank.
#include <float.h>
#include <math.h>
#include "common.h"
#include "dispatch.h"

namespace {

constexpr int HL_ROWS = 128, HL_COLS = 128, HL_BK = 64, HL_LD = HL_BK + 8;
constexpr int HL_THREADS = 256, HL_NP = HL_ROWS * (HL_BK / 8) / HL_THREADS;  // 16-byte pieces per thread, operand and step
constexpr int HL_LDS_BYTES = 2 * 2 * HL_ROWS * HL_LD * 2;                    // two buffers of x and of W
// the host rule: as many splits as give every CU two blocks (what fits beside each other there), at most HL_SPLITS_MAX,
// then evened out so that no split is empty
constexpr int HL_BLOCKS = 512, HL_SPLITS_MAX = 128;
static_assert(HL_ROWS == HL_COLS && HL_NP == 4, "the staging maps one piece index onto the rows of x and of W alike");

struct HeadPlan {
    int64_t row_tiles, col_tiles;
    int S, per;  // splits, and the column tiles of each (the last may hold fewer, never none)
};

HeadPlan head_plan(int64_t T, int64_t V) {
    HeadPlan p;
    p.row_tiles = cdiv64(T > 0 ? T : 1, HL_ROWS);
    p.col_tiles = cdiv64(V > 0 ? V : 1, HL_COLS);
    int64_t S = cdiv64(HL_BLOCKS, p.row_tiles);
    if (S > HL_SPLITS_MAX) S = HL_SPLITS_MAX;
    if (S > p.col_tiles) S = p.col_tiles;
    p.per = (int)cdiv64(p.col_tiles, S);
    p.S = (int)cdiv64(p.col_tiles, p.per);
    return p;
}

int64_t head_zt_bytes(int64_t T) { return cdiv64(T * 4, 16) * 16; }

struct HeadArgs {
    const void* x;
    int64_t ldx;
    const void* w;
    const int64_t* targets;
    float* zt;    // [T]
    f32x4* rec;   // [T][S] {max, sum, count as bits, 0}
    float* logprob;
    int32_t* rank;
    float* lse;
    int64_t T;
    int V, K, S, per;
};

// ---- target ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void head_target_kernel(HeadArgs a) {
    using V8 = typename VecT<T>::x8;
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // (the whole wave agrees)
    if (t >= a.T) return;
    const int64_t g = a.targets[t];
    if (g < 0 || g >= a.V) {
        if (lane == 0) a.zt[t] = NAN;
        return;
    }
    const T* xr = reinterpret_cast<const T*>(a.x) + t * a.ldx;
    const T* wr = reinterpret_cast<const T*>(a.w) + g * a.K;
    float s = 0.f;
    for (int k = lane * 8; k < a.K; k += 512) {  // K % 8 == 0: eight columns are all inside K or all past it
        const V8 xv = ld16<V8>(xr + k), wv = ld16<V8>(wr + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += to_f32(xv[j]) * to_f32(wv[j]);
    }
    s = wave_sum(s);
    if (lane == 0) a.zt[t] = s;
}

// ---- sweep -------------------------------------------------------------------------------------------------------------
// (m, s) <- (m, s) and (m2, s2): sums of exp(z - max) under the larger max.  A side that has seen nothing holds (-FLT_MAX, 0);
// columns >= V arrive as -inf, whose exp(-inf - max) is 0.
__device__ __forceinline__ void lse_fold(float& m, float& s, float m2, float s2) {
    const float nm = fmaxf(m, m2);
    s = s * expf(m - nm) + s2 * expf(m2 - nm);
    m = nm;
}

template <typename T>
__global__ __launch_bounds__(HL_THREADS, 2) void head_sweep_kernel(HeadArgs a) {
    using V8 = typename VecT<T>::x8;
    extern __shared__ __attribute__((aligned(16))) unsigned char head_lds[];
    T* xs = reinterpret_cast<T*>(head_lds);  // [2][HL_ROWS][HL_LD]
    T* ws = xs + 2 * HL_ROWS * HL_LD;        // [2][HL_COLS][HL_LD]
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x;
    const int64_t row0 = (int64_t)blockIdx.y * HL_ROWS;
    const int col_tiles = (a.V + HL_COLS - 1) / HL_COLS;
    const int tile0 = split * a.per, tile1 = min(tile0 + a.per, col_tiles);
    const int KS = (a.K + HL_BK - 1) / HL_BK;
    const int steps = (tile1 - tile0) * KS;

    // staging: piece tid + 256 j is row tid / 8 + 32 j, k-columns 8 (tid % 8) ..+8 of the step
    const int pr = tid >> 3, pk = (tid & 7) * 8;
    const T* xrow[HL_NP];
#pragma unroll
    for (int j = 0; j < HL_NP; ++j) {
        const int64_t row = row0 + pr + 32 * j;
        xrow[j] = reinterpret_cast<const T*>(a.x) + (row < a.T ? row : a.T - 1) * a.ldx;
    }
    const T* wbase = reinterpret_cast<const T*>(a.w);
    const int st_off = pr * HL_LD + pk;

    V8 xv[HL_NP], wv[HL_NP];
    auto fetch = [&](int tile, int ks) {
        const int k = ks * HL_BK + pk;
        const bool past = k >= a.K;  // K % 8 == 0: a piece is all inside K or all past it
        const int kc = past ? a.K - 8 : k;
#pragma unroll
        for (int j = 0; j < HL_NP; ++j) {
            xv[j] = ld16<V8>(xrow[j] + kc);
            wv[j] = ld16<V8>(wbase + (int64_t)min(tile * HL_COLS + pr + 32 * j, a.V - 1) * a.K + kc);
            if (past) {
#pragma unroll
                for (int e = 0; e < 8; ++e) xv[j][e] = (T)0.f, wv[j][e] = (T)0.f;
            }
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int j = 0; j < HL_NP; ++j) {
            st16<V8>(xs + (buf * HL_ROWS + 32 * j) * HL_LD + st_off, xv[j]);
            st16<V8>(ws + (buf * HL_COLS + 32 * j) * HL_LD + st_off, wv[j]);
        }
    };

    // the lane's token, its target and the target's logit
    const int64_t t = row0 + wave * 32 + c;
    const bool live = t < a.T;
    const float zt = live ? a.zt[t] : NAN;
    const int64_t g64 = live ? a.targets[t] : -1;
    const int g = g64 >= 0 && g64 < a.V ? (int)g64 : -1;
    float run_m = -FLT_MAX, run_s = 0.f;
    int run_c = 0;

    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

    int tile = tile0, ks = 0;  // of the step being multiplied
    fetch(tile, ks);
    stash(0);
    __syncthreads();
    for (int step = 0; step < steps; ++step) {
        const int buf = step & 1;
        const bool more = step + 1 < steps;
        const bool last_k = ks == KS - 1;
        const int ntile = last_k ? tile + 1 : tile, nks = last_k ? 0 : ks + 1;
        if (more) fetch(ntile, nks);

        const T* xf = xs + (buf * HL_ROWS + wave * 32 + c) * HL_LD + h * 8;
        const T* wf = ws + (buf * HL_COLS + c) * HL_LD + h * 8;
#pragma unroll
        for (int kk = 0; kk < HL_BK / 16; ++kk) {
            const V8 xfrag = *reinterpret_cast<const V8*>(xf + kk * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[j] = mfma32(*reinterpret_cast<const V8*>(wf + 32 * j * HL_LD + kk * 16), xfrag, acc[j]);
        }

        if (more) stash(buf ^ 1);  // (read by the step before this one; everybody has passed its barrier)
        __syncthreads();

        if (last_k) {
            // accumulator register r of lane (c, h) of acc[j] is column v0 + 32 j + (r & 3) + 8 (r >> 2) + 4 h of token c
            const int v0 = tile * HL_COLS + 4 * h;
            const bool ragged = (tile + 1) * HL_COLS > a.V;  // (the whole block agrees)
            float tm = -FLT_MAX;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (ragged && v0 + 32 * j + (r & 3) + 8 * (r >> 2) >= a.V) acc[j][r] = -INFINITY;
                    tm = fmaxf(tm, acc[j][r]);
                }
            const float nm = fmaxf(run_m, tm);
            float s = 0.f;
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float z = acc[j][r];
                    s += expf(z - nm);
                    cnt += (z > zt && v0 + 32 * j + (r & 3) + 8 * (r >> 2) != g) ? 1 : 0;
                    acc[j][r] = 0.f;
                }
            run_s = run_s * expf(run_m - nm) + s;
            run_m = nm;
            run_c += cnt;
        }
        tile = ntile, ks = nks;
    }

    // the token's other 16-row halves sit in lane c + 32
    const float om = __shfl_xor(run_m, 32, 64), os = __shfl_xor(run_s, 32, 64);
    const int oc = __shfl_xor(run_c, 32, 64);
    if (h == 0 && live) {
        lse_fold(run_m, run_s, om, os);
        a.rec[t * a.S + split] = f32x4{run_m, run_s, __int_as_float(run_c + oc), 0.f};
    }
}

// ---- merge -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_merge_kernel(HeadArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.T) return;
    float m = -FLT_MAX, s = 0.f;
    int cnt = 0;
    for (int i = 0; i < a.S; ++i) {
        const f32x4 r = a.rec[t * a.S + i];
        lse_fold(m, s, r[0], r[1]);
        cnt += __float_as_int(r[2]);
    }
    const float lse = m + logf(s);
    const int64_t g = a.targets[t];
    const bool wanted = g >= 0 && g < a.V;
    a.lse[t] = lse;
    a.logprob[t] = wanted ? a.zt[t] - lse : NAN;
    a.rank[t] = wanted ? 1 + cnt : 0;
}

}  // namespace

extern "C" int64_t tgis_head_logprobs_bytes(int64_t T, int64_t V, int* num_splits) {
    const HeadPlan p = head_plan(T, V);
    if (num_splits) *num_splits = p.S;
    if (T <= 0 || V <= 0) return 0;
    return head_zt_bytes(T) + T * p.S * (int64_t)sizeof(f32x4);
}

extern "C" int tgis_head_logprobs(const void* x, int64_t ldx, const void* weight, const int64_t* targets, int64_t T,
                                  int64_t V, int64_t K, int dtype, float* logprob, int32_t* rank, float* lse,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    TGIS_CHECK_ARG(T >= 0 && T <= (int64_t)65535 * HL_ROWS, "tgis_head_logprobs: 0 <= T <= %ld rows (T=%ld)",
                   (long)65535 * HL_ROWS, (long)T);
    TGIS_CHECK_ARG(V >= 1 && V < (1ll << 31) - HL_COLS, "tgis_head_logprobs: 1 <= V < 2^31 - %d (V=%ld)", HL_COLS, (long)V);
    TGIS_CHECK_ARG(K > 0 && K % 16 == 0 && K < (1ll << 30), "tgis_head_logprobs: K (%ld) must be a positive multiple of 16",
                   (long)K);
    TGIS_CHECK_ARG(dtype == TGIS_F16 || dtype == TGIS_BF16, "tgis_head_logprobs: bad dtype");
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(x && weight && targets && logprob && rank && lse && workspace, "tgis_head_logprobs: null tensor");
    TGIS_CHECK_ARG(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)weight % 16) == 0 &&
                       ((uintptr_t)workspace % 16) == 0,
                   "tgis_head_logprobs: rows of x and of the weight and the workspace must be 16-byte aligned (ldx=%ld)",
                   (long)ldx);
    const HeadPlan p = head_plan(T, V);
    TGIS_CHECK_ARG(workspace_bytes >= tgis_head_logprobs_bytes(T, V, nullptr),
                   "tgis_head_logprobs: workspace of %ld bytes, tgis_head_logprobs_bytes asks for %ld", (long)workspace_bytes,
                   (long)tgis_head_logprobs_bytes(T, V, nullptr));
    HeadArgs a;
    a.x = x, a.ldx = ldx, a.w = weight, a.targets = targets;
    a.zt = reinterpret_cast<float*>(workspace);
    a.rec = reinterpret_cast<f32x4*>(reinterpret_cast<uint8_t*>(workspace) + head_zt_bytes(T));
    a.logprob = logprob, a.rank = rank, a.lse = lse;
    a.T = T, a.V = (int)V, a.K = (int)K, a.S = p.S, a.per = p.per;
    hipStream_t st = (hipStream_t)stream;
    TgisTimedScope timed(TGIS_OP_SAMPLE, st);
    return by_dtype(dtype, [&](auto tag) {
        using T_ = type_of<decltype(tag)>;
        static bool attr = false;
        if (!attr) {
            TGIS_CHECK_HIP(hipFuncSetAttribute((const void*)head_sweep_kernel<T_>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               HL_LDS_BYTES));
            attr = true;
        }
        hipLaunchKernelGGL(head_target_kernel<T_>, dim3((unsigned)cdiv64(T, 4)), dim3(256), 0, st, a);
        TGIS_CHECK_LAUNCH();
        hipLaunchKernelGGL(head_sweep_kernel<T_>, dim3((unsigned)p.S, (unsigned)p.row_tiles), dim3(HL_THREADS), HL_LDS_BYTES, st,
                           a);
        TGIS_CHECK_LAUNCH();
        hipLaunchKernelGGL(head_merge_kernel, dim3((unsigned)cdiv64(T, 256)), dim3(256), 0, st, a);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}
