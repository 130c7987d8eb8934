// Int4 (GPTQ) tile expert GEMMs: prefills of a GPTQ Mixtral model past the rows the slab kernels of moe.hip serve well.
// Included at the end of moe.hip, after moe_tiles.h: the entry points below share moe.hip's checks, argument block, int4
// weight source and combine kernel, and moe_tiles.h's tile list.
//
//   tgis_moe_gptq_tile_gemm_up    the contracts of tgis_moe_gptq_gemm_up / _down over the same int4 images of
//   tgis_moe_gptq_tile_gemm_down  tgis_gptq_prepare, walked by the tile list of tgis_moe_route_tiles.
//
// Grid (ceil(NT / 4), tile bound).  A block past tiles[0] returns at once; otherwise it owns one tile (up to TILE_R = 64 rows
// of one expert) x 128 image columns.  Wave w owns column tile 4 blockIdx.x + w over the WHOLE k range (no k split, no LDS
// exchange of partial sums: the same input gives the same bytes).  Per k64-step it takes its 1 KiB of nibbles and the lane's {scale, zero} word
// of the step's group out of a register ring (Int4Source, moe.hip), dequantises ONE 32x16 B fragment at a time with dequant8
// and feeds it to two MFMAs, one per 32-row block of the tile, before it dequantises the next: a dequantised fragment
// serves 64 rows where the slab kernel's serves 32, and an expert's nibbles are read once per 64 of its rows.
//
// The activation rows of the tile are gathered once per block and k64-step into double-buffered LDS in the A-fragment order
// of moe_tile_gemm_kernel (fragment i of lane l: row l & 31, columns step * 64 + (l >> 5) * 32 + i * 8 .. + 8), so a wave's
// read is one 16-byte LDS load per MFMA at lane * 16.  Rows past the tile are zero in LDS and never stored.
//
// A 128-row form (the block of an expert's even-indexed tile also took the tile behind it: four accumulators, a 32 KiB A
// double buffer, 148 registers, 3 waves per SIMD) was built and measured at 64 .. 2048 tokens of 8x7B's shapes: it never beat
// this one (0.98 against 0.81 ms at 512 tokens, equal at 2048) and was deleted.
#pragma once

namespace {

// k64-steps of nibbles a wave keeps in flight.  A ring of 8 costs a wave per SIMD (116 registers, 4 waves, against 94 and 5)
// and measured 3 - 9 % slower at 128, 512 and 2048 tokens; the macro is that sweep's switch.
#ifndef TGIS_MOE_GPTQ_TILE_RING
#define TGIS_MOE_GPTQ_TILE_RING 4
#endif
constexpr int GT_RING = TGIS_MOE_GPTQ_TILE_RING;

template <bool UP>
__global__ __launch_bounds__(TILE_THREADS, 4) void moe_gptq_tile_gemm_kernel(MoeArgs a, const int32_t* __restrict__ tiles) {
    using V8 = f16x8;
    constexpr int ROWS = TILE_R;
    constexpr int NB = ROWS / 32;  // 32-row blocks of the tile: accumulators, and MFMAs per dequantised fragment
    __shared__ __attribute__((aligned(16))) f16 xs[2][NB][4 * 64 * 8];  // [buffer][32-row block][i][lane][8]
    __shared__ int s_slot[ROWS];
    __shared__ float s_wt[ROWS];
    if ((int)blockIdx.y >= tiles[0]) return;
    const int32_t* entry = tiles + 4 * (1 + blockIdx.y);
    const int e = entry[0], first = entry[1], rows = entry[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = blockIdx.x * (TILE_C / 32) + wv;
    const bool active = nt < a.NT;  // (wave-uniform) a wave past the last column tile still gathers
    if (tid < ROWS) {
        const int slot = tid < rows ? a.slot_rows[first + tid] : -1;
        s_slot[tid] = slot;
        s_wt[tid] = (!UP && slot >= 0) ? a.expert_w[slot] : 0.f;
    }
    __syncthreads();

    // gather: thread -> row gm of each 32-row block and the 8 columns gq * 8 .. + 8 of the k64-step (K % 64 == 0: inside K)
    const int gm = (tid & 7) + 8 * (tid >> 6), gq = (tid >> 3) & 7;
    const f16* grow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int slot = s_slot[j * 32 + gm];
        grow[j] = slot < 0 ? nullptr : reinterpret_cast<const f16*>(a.x) + (int64_t)(UP ? slot / a.top_k : slot) * a.ldx;
    }
    const int gdst = (((gq & 3) * 64) + (gq >> 2) * 32 + gm) * 8;
    auto gather = [&](int step, V8* g) {
        const int kk = step * 64 + gq * 8;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            V8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (grow[j] != nullptr) v = ld16<V8>(grow[j] + kk);
            g[j] = v;
        }
    };
    auto stage = [&](int buf, const V8* g) {
#pragma unroll
        for (int j = 0; j < NB; ++j) st16(&xs[buf][j][gdst], g[j]);
    };

    const Int4Source src_w(a, e, active ? nt : 0, 0, lane);
    const int nsteps = a.KS;
    f32x16 acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    Int4Source::Step wq[GT_RING];
    V8 g[NB];
    gather(0, g);
    if (active) {
#pragma unroll
        for (int s = 0; s < GT_RING; ++s)
            if (s < nsteps) src_w.load(s, wq[s]);
    }
    stage(0, g);
    __syncthreads();
    for (int s0 = 0; s0 < nsteps; s0 += GT_RING) {
#pragma unroll
        for (int r = 0; r < GT_RING; ++r) {
            const int s = s0 + r;
            if (s < nsteps) {  // (block-uniform: every wave meets the barrier below)
                if (s + 1 < nsteps) gather(s + 1, g);
                if (active) {
                    const f16x2 szh = __builtin_bit_cast(f16x2, wq[r].sz);
                    const f16 zc1 = szh[1];
                    const f16 zd1 = (f16)960.f - zc1;  // -(64 + z + 1), exact
                    const f16x2 zc = {zc1, zc1}, zd = {zd1, zd1}, sc = {szh[0], szh[0]};
                    const f16* xa = &xs[s & 1][0][lane * 8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const V8 b = gptq::dequant8(wq[r].q[i], zc, zd, sc, src_w.EX, src_w.M0, src_w.M1);
#pragma unroll
                        for (int j = 0; j < NB; ++j)
                            acc[j] = mfma32(*reinterpret_cast<const V8*>(xa + j * 2048 + i * 512), b, acc[j]);
                    }
                    if (s + GT_RING < nsteps) src_w.load(s + GT_RING, wq[r]);  // the slot is consumed: refill it in place
                }
                if (s + 1 < nsteps) stage((s + 1) & 1, g);  // (that buffer was last read before the previous barrier)
                __syncthreads();
            }
        }
    }
    if (!active) return;
    // accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
    const int c = lane & 31;
#pragma unroll
    for (int rb = 0; rb < NB; ++rb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int oslot = s_slot[m];  // -1 past the tile's rows
            const float fin = acc[rb][r];
            if (UP) {
                // (gate, up) pairs sit 16 lanes apart: act 2's epilogue, as moe_gemm_kernel's
                const int half = a.N >> 1, j2 = nt * 16 + (c & 15);
                const float mine = to_f32(from_f32<f16>(fin));
                const float other = __shfl_xor(mine, 16, 64);
                if (c < 16 && j2 < half && oslot >= 0) {
                    const float sl = mine / (1.f + __expf(-mine));
                    reinterpret_cast<f16*>(a.out)[(int64_t)oslot * a.ldo + j2] = from_f32<f16>(to_f32(from_f32<f16>(sl)) * other);
                }
            } else {
                const int n = nt * 32 + c;
                if (n < a.N && oslot >= 0) {
                    const float v = fin * s_wt[m];
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

template <bool UP>
int moe_gptq_tile_launch(const MoeArgs& a, const int32_t* tiles, int64_t tile_bound, hipStream_t st) {
    hipLaunchKernelGGL((moe_gptq_tile_gemm_kernel<UP>), dim3((unsigned)cdiv64(a.NT, TILE_C / 32), (unsigned)tile_bound),
                       dim3(TILE_THREADS), 0, st, a, tiles);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

}  // namespace

extern "C" int tgis_moe_gptq_tile_gemm_up(const void* x, int64_t ldx, const void* images, int64_t expert_stride,
                                          const int32_t* offsets, const int32_t* slot_rows, const int32_t* tiles,
                                          int64_t tile_bound, void* h, int64_t ldh, int64_t T, int64_t K, int64_t N,
                                          int64_t groups, int E, int top_k, int dtype, void* stream) {
    const char* fn = "tgis_moe_gptq_tile_gemm_up";
    int rc = moe_check_gptq_shape(fn, K, N, groups, dtype);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_gemm(fn, x, ldx, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype, groups, TILE_MAX_E);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(h && ldh >= N / 2, "%s: h rows must hold N / 2 elements", fn);
    rc = moe_tile_check_tiles(fn, tiles, tile_bound, T, E, top_k);
    if (rc != TGIS_OK) return rc;
    if (T == 0) return TGIS_OK;
    MoeArgs a;
    moe_fill(a, x, ldx, images, expert_stride, offsets, slot_rows, nullptr, h, ldh, K, N, top_k, 0);
    moe_fill_gptq(a, K, N, groups);
    TgisTimedScope timed(TGIS_OP_GPTQ_GEMM, (hipStream_t)stream);
    return moe_gptq_tile_launch<true>(a, tiles, tile_bound, (hipStream_t)stream);
}

extern "C" int tgis_moe_gptq_tile_gemm_down(const void* h, int64_t ldh, const void* images, int64_t expert_stride,
                                            const int32_t* offsets, const int32_t* slot_rows, const int32_t* tiles,
                                            int64_t tile_bound, const float* expert_w, int64_t T, int64_t K, int64_t N,
                                            int64_t groups, int E, int top_k, int dtype, int form, float* scratch,
                                            int64_t scratch_bytes, void* out, int64_t ldo, void* stream) {
    const char* fn = "tgis_moe_gptq_tile_gemm_down";
    int rc = moe_check_gptq_shape(fn, K, N, groups, dtype);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_gemm(fn, h, ldh, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype, groups, TILE_MAX_E);
    if (rc != TGIS_OK) return rc;
    rc = moe_check_down(fn, expert_w, T, N, top_k, form, out, ldo);
    if (rc != TGIS_OK) return rc;
    rc = moe_tile_check_tiles(fn, tiles, tile_bound, T, E, top_k);
    if (rc != TGIS_OK) return rc;
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(scratch && ((uintptr_t)scratch % 16) == 0 && scratch_bytes >= tgis_moe_tile_gemm_down_bytes(T, N, top_k, form),
                   "%s: scratch too small (%ld < %ld)", fn, (long)scratch_bytes,
                   (long)tgis_moe_tile_gemm_down_bytes(T, N, top_k, form));
    hipStream_t st = (hipStream_t)stream;
    MoeArgs a;
    moe_fill(a, h, ldh, images, expert_stride, offsets, slot_rows, expert_w, scratch, N, K, N, top_k, form);  // (N % 32 == 0)
    moe_fill_gptq(a, K, N, groups);
    TgisTimedScope timed(TGIS_OP_GPTQ_GEMM, st);
    rc = moe_gptq_tile_launch<false>(a, tiles, tile_bound, st);
    if (rc != TGIS_OK || form == 0) return rc;
    hipLaunchKernelGGL(moe_combine_kernel<f16>, dim3((unsigned)cdiv64(T * (N / 4), 256)), dim3(256), 0, st, scratch, (f16*)out, ldo,
                       T, (int)N, top_k);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}
