// Routed expert MLP for many experts (Qwen3-MoE: 128 experts, 8 per token).  Included at the end of moe.hip: the entry
// points below share its checks, its weight source, its combine kernel and, for a few rows, its slab kernel body.
//
//   tgis_moe_route_tiles     tgis_moe_route's five arrays for up to 128 experts, plus a TILE LIST: every expert's rows of
//                            slot_rows cut into consecutive tiles of up to TILE_R rows, experts ascending.
//   tgis_moe_tile_gemm_up    the contracts of tgis_moe_gemm_up / _down over the same images, with a block per
//   tgis_moe_tile_gemm_down  (128 image columns, tile) instead of per (32 image columns, expert).
//
// Route, three launches whose grids depend on T alone:
//   1. a block per RT_TOKENS tokens, a token per wave: lane l holds the logits of experts l and l + 64; the maximum is a wave
//      reduction; the fp64 terms exp(x - max) go through LDS and are summed in expert order (the order tgis_moe_route sums
//      them in: for E <= 64 the two kernels give the same bytes); top_k rounds of a wave arg-max on the fp32 probabilities
//      (ties to the lower index) pick the experts.  The block leaves its expert histogram, integer LDS atomics, as a row of
//      [blocks][E] counts.
//   2. one block, a thread per expert: walks the histogram rows (turning them into each block's base inside the expert's
//      list), then counts, offsets and the tile list.
//   3. a block per RT_TOKENS tokens, a slot per thread: a slot's rank among the block's slots of the same expert is a ballot
//      and a popcount inside its wave plus the waves before it (LDS); slot_rows[offsets[e] + base[block][e] + rank] = slot.
//      Blocks are in token order, so the slots ascend inside every expert.
// No host read, no waiting between blocks, integer work only for the lists.
//
// Tile GEMM: grid (ceil(NT / 4), tile bound).  A block whose index is past n_tiles returns at once; otherwise it owns TILE_R =
// 64 rows of one expert x TILE_C = 128 image columns.  Wave w owns column tile 4 blockIdx.x + w over the WHOLE k range (no k
// split, no LDS exchange of partial sums): it streams the tile's B fragments from global memory in fragment order through
// a ring of MOE_RING k64-steps and holds two 32x32 accumulators (rows 0 - 31 and 32 - 63), so a weight byte feeds 64 rows.  The
// tile's activation rows are gathered ONCE per block and k64-step into LDS (up: row slot / top_k of x, down: row slot of h),
// double-buffered, written in the A-fragment order of xf_off — a wave's read is one ds_read_b128 per MFMA at lane * 16 —
// and read by all four waves: an activation byte is fetched once per 128 columns.  The gather is laid out so that 8 lanes
// fetch the 128 contiguous bytes of one row's k64-step and 8 consecutive lanes write 8 consecutive 16-byte LDS cells.  Rows
// past the tile's row count are zero in LDS and never stored; columns past K are zero as the image is.
#pragma once

namespace {

constexpr int TILE_MAX_E = 128;
constexpr int TILE_R = 64;         // rows of a tile
constexpr int TILE_C = 128;        // image columns of a block (four 32-column tiles, one per wave)
constexpr int TILE_THREADS = 256;
constexpr int TILE_LDS = 2 * TILE_R * 64 * 2 + TILE_R * 8;  // two A buffers of one k64-step, the tile's slots and weights
constexpr int RT_TOKENS = 32;      // tokens of a route block: RT_TOKENS * MOE_MAX_TOPK slots, one per thread of the scatter
constexpr int RT_THREADS = 256;
static_assert(RT_TOKENS * MOE_MAX_TOPK <= RT_THREADS, "the scatter pass gives every slot of a block a thread");
// Tokens up to which the two GEMMs take the slab kernel body of moe.hip instead of the tile kernel (0: never).  Read off
// tools/bench_qwen3_moe.py's table of the routed block under either kernel at Qwen3-30B-A3B's shapes:
// the slab body is 22 %, 17 % and 4 % faster at T = 1, 2 and 4 (8 - 31 tiles x 12 column blocks leave most CUs idle, and each
// wave walks the whole k range alone), the two measure equal at T = 8, where the tile kernel is taken, and the tile kernel wins
// from T = 32 on (at T = 16 the slab body is 2 % ahead; one threshold keeps the tile kernel there).
#ifndef TGIS_MOE_TILE_SLAB_MAX_T
#define TGIS_MOE_TILE_SLAB_MAX_T 4
#endif
int g_tile_force = -1;  // tgis_debug_moe_tile_force: -1 the rule, 0 the tile kernel, 1 the slab kernel body

// ---- route -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RT_THREADS) void moe_tile_route_kernel(const float* __restrict__ logits, int64_t ld, int T, int E,
                                                                   int top_k, int renorm, int32_t* __restrict__ expert_ids,
                                                                   float* __restrict__ expert_w,
                                                                   int32_t* __restrict__ block_counts) {
    __shared__ int s_hist[TILE_MAX_E];
    __shared__ double s_ex[RT_THREADS / 64][TILE_MAX_E];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TILE_MAX_E) s_hist[tid] = 0;
    __syncthreads();
    const int e0 = lane, e1 = lane + 64;
    for (int i = wave; i < RT_TOKENS; i += RT_THREADS / 64) {
        const int t = blockIdx.x * RT_TOKENS + i;
        if (t >= T) break;  // (the same for every lane of the wave)
        const float* row = logits + (int64_t)t * ld;
        const float l0 = e0 < E ? row[e0] : -INFINITY, l1 = e1 < E ? row[e1] : -INFINITY;
        const float mx = wave_max(fmaxf(l0, l1));
        const double x0 = e0 < E ? exp((double)l0 - (double)mx) : 0.0, x1 = e1 < E ? exp((double)l1 - (double)mx) : 0.0;
        s_ex[wave][e0] = x0;
        s_ex[wave][e1] = x1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        double sum = 0.0;  // in expert order, every lane the same additions
        for (int e = 0; e < E; ++e) sum += s_ex[wave][e];
        const double pd0 = x0 / sum, pd1 = x1 / sum;
        // the order is decided on the fp32 probabilities; -1 marks a taken expert, -2 a lane without one
        float p0 = e0 < E ? (float)pd0 : -2.f, p1 = e1 < E ? (float)pd1 : -2.f;
        int myid = 0;
        double mypd = 0.0, psum = 0.0;
        for (int k = 0; k < top_k; ++k) {
            float bp = p0;
            int bi = e0;
            if (p1 > p0) bp = p1, bi = e1;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float op = __shfl_xor(bp, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (op > bp || (op == bp && oi < bi)) bp = op, bi = oi;
            }
            const double bd = __shfl((bi >> 6) ? pd1 : pd0, bi & 63, 64);
            if (lane == k) myid = bi, mypd = bd;
            psum += bd;
            if (bi == e0) p0 = -1.f;
            if (bi == e1) p1 = -1.f;
        }
        if (lane < top_k) {
            myid = min(myid, E - 1);  // (NaN logits leave the arg-max undecided: the id stays one the lists can hold)
            expert_ids[(int64_t)t * top_k + lane] = myid;
            expert_w[(int64_t)t * top_k + lane] = (float)(renorm ? mypd / psum : mypd);
            atomicAdd(&s_hist[myid], 1);
        }
        __builtin_amdgcn_wave_barrier();  // (the sums above have read s_ex before the next token overwrites it)
    }
    __syncthreads();
    if (tid < E) block_counts[(int64_t)blockIdx.x * E + tid] = s_hist[tid];
}

// tiles: int32 quadruples; [0] = {n_tiles, TILE_R, 0, 0}, [1 + i] = {expert, first position in slot_rows, rows, 0}
__global__ __launch_bounds__(TILE_MAX_E) void moe_tile_scan_kernel(int32_t* __restrict__ block_counts, int NB, int E,
                                                                  int32_t* __restrict__ counts, int32_t* __restrict__ offsets,
                                                                  int32_t* __restrict__ tiles, int bound) {
    __shared__ int s_cnt[TILE_MAX_E], s_off[TILE_MAX_E + 1], s_tile[TILE_MAX_E + 1];
    const int e = threadIdx.x;
    int run = 0;
    if (e < E)
        for (int b = 0; b < NB; ++b) {  // (coalesced: the threads read one histogram row together)
            const int c = block_counts[(int64_t)b * E + e];
            block_counts[(int64_t)b * E + e] = run;  // the block's base inside expert e's list
            run += c;
        }
    s_cnt[e] = run;
    __syncthreads();
    if (e == 0) {
        int off = 0, nt = 0;
        for (int i = 0; i < E; ++i) {
            s_off[i] = off, s_tile[i] = nt;
            off += s_cnt[i];
            nt += (s_cnt[i] + TILE_R - 1) / TILE_R;
        }
        s_off[E] = off, s_tile[E] = nt;
        offsets[E] = off;
        tiles[0] = min(nt, bound), tiles[1] = TILE_R, tiles[2] = 0, tiles[3] = 0;
    }
    __syncthreads();
    if (e < E) {
        counts[e] = s_cnt[e];
        offsets[e] = s_off[e];
        for (int i = 0, idx = s_tile[e]; i * TILE_R < s_cnt[e] && idx < bound; ++i, ++idx) {
            int32_t* q = tiles + 4 * (1 + idx);
            q[0] = e, q[1] = s_off[e] + i * TILE_R, q[2] = min(TILE_R, s_cnt[e] - i * TILE_R), q[3] = 0;
        }
    }
}

__global__ __launch_bounds__(RT_THREADS) void moe_tile_scatter_kernel(const int32_t* __restrict__ expert_ids, int nslots, int E,
                                                                     int top_k, const int32_t* __restrict__ block_bases,
                                                                     const int32_t* __restrict__ offsets,
                                                                     int32_t* __restrict__ slot_rows) {
    __shared__ int s_w[RT_THREADS / 64][TILE_MAX_E];  // slots of each expert in each wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < (RT_THREADS / 64) * TILE_MAX_E; i += RT_THREADS) (&s_w[0][0])[i] = 0;
    __syncthreads();
    const int per = RT_TOKENS * top_k;
    const int64_t s = (int64_t)blockIdx.x * per + tid;
    int id = (tid < per && s < nslots) ? expert_ids[s] : -1;
    if (id >= E) id = -1;
    int rank = 0;
    uint64_t pending = __ballot(id >= 0);
    while (pending) {  // (wave-uniform) one round per distinct expert of the wave
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const int lid = __shfl(id, leader, 64);
        const uint64_t m = __ballot(id == lid);
        if (id == lid) {
            rank = __popcll(m & ((1ull << lane) - 1));
            if (lane == leader) s_w[wave][lid] = __popcll(m);
        }
        pending &= ~m;
    }
    __syncthreads();
    if (id >= 0) {
        int pos = offsets[id] + block_bases[(int64_t)blockIdx.x * E + id] + rank;
        for (int w = 0; w < wave; ++w) pos += s_w[w][id];
        slot_rows[pos] = (int32_t)s;
    }
}

// ---- tile GEMM -------------------------------------------------------------------------------------------------------------
template <typename T, bool UP>
__global__ __launch_bounds__(TILE_THREADS, 2) void moe_tile_gemm_kernel(MoeArgs a, const int32_t* __restrict__ tiles) {
    using V8 = typename VecT<T>::x8;
    using W = DenseSource<T>;
    constexpr int RING = W::RING;
    __shared__ __attribute__((aligned(16))) T xs[2][2][4 * 64 * 8];  // [buffer][32-row block][i][lane][8]: xf_off's order
    __shared__ int s_slot[TILE_R];
    __shared__ float s_wt[TILE_R];
    if ((int)blockIdx.y >= tiles[0]) return;
    const int32_t* entry = tiles + 4 * (1 + blockIdx.y);
    const int e = entry[0], first = entry[1], rows = entry[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = blockIdx.x * (TILE_C / 32) + wv;
    const bool active = nt < a.NT;  // (wave-uniform) a wave past the last column tile still gathers
    if (tid < TILE_R) {
        const int slot = tid < rows ? a.slot_rows[first + tid] : -1;
        s_slot[tid] = slot;
        s_wt[tid] = (!UP && slot >= 0) ? a.expert_w[slot] : 0.f;
    }
    __syncthreads();

    // gather: thread -> row gm of each 32-row block and the 8 columns gq * 8 .. + 8 of the k64-step
    const int gm = (tid & 7) + 8 * (tid >> 6), gq = (tid >> 3) & 7;
    const T* grow[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int slot = s_slot[j * 32 + gm];
        grow[j] = slot < 0 ? nullptr : reinterpret_cast<const T*>(a.x) + (int64_t)(UP ? slot / a.top_k : slot) * a.ldx;
    }
    const int gdst = (((gq & 3) * 64) + (gq >> 2) * 32 + gm) * 8;
    auto gather = [&](int step, V8* g) {
        const int kk = step * 64 + gq * 8;  // K % 8 == 0: eight columns are all inside K or all past it
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            V8 v;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (T)0.f;
            if (grow[j] != nullptr && kk < a.K) v = ld16<V8>(grow[j] + kk);
            g[j] = v;
        }
    };
    auto stage = [&](int buf, const V8* g) {
#pragma unroll
        for (int j = 0; j < 2; ++j) st16(&xs[buf][j][gdst], g[j]);
    };

    const W src_w(a, e, active ? nt : 0, 0, lane);
    const int nsteps = a.KS;
    f32x16 acc[2];
    acc[0] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    acc[1] = acc[0];
    typename W::Step wq[RING];
    V8 g[2];
    gather(0, g);
    if (active) {
#pragma unroll
        for (int s = 0; s < RING; ++s)
            if (s < nsteps) src_w.load(s, wq[s]);
    }
    stage(0, g);
    __syncthreads();
    for (int s0 = 0; s0 < nsteps; s0 += RING) {
#pragma unroll
        for (int r = 0; r < RING; ++r) {
            const int s = s0 + r;
            if (s < nsteps) {  // (block-uniform: every wave meets the barrier below)
                if (s + 1 < nsteps) gather(s + 1, g);
                if (active) {
                    V8 b[4];
                    src_w.frags(wq[r], b);
                    const T* xa = &xs[s & 1][0][lane * 8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const V8 a0 = *reinterpret_cast<const V8*>(xa + i * 512);
                        const V8 a1 = *reinterpret_cast<const V8*>(xa + 2048 + i * 512);
                        acc[0] = mfma32(a0, b[i], acc[0]);
                        acc[1] = mfma32(a1, b[i], acc[1]);
                    }
                    if (s + RING < nsteps) src_w.load(s + RING, wq[r]);  // the slot is consumed: refill it in place
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
    for (int rb = 0; rb < 2; ++rb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = rb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const int oslot = s_slot[m];  // -1 past the tile's rows
            const float fin = acc[rb][r];
            if (UP) {
                // (gate, up) pairs sit 16 lanes apart: act 2's epilogue of dense_gemm_unit
                const int half = a.N >> 1, j2 = nt * 16 + (c & 15);
                const float mine = to_f32(from_f32<T>(fin));
                const float other = __shfl_xor(mine, 16, 64);
                if (c < 16 && j2 < half && oslot >= 0) {
                    const float sl = mine / (1.f + __expf(-mine));
                    reinterpret_cast<T*>(a.out)[(int64_t)oslot * a.ldo + j2] =
                        dense::finish_out<T>(to_f32(from_f32<T>(sl)) * other, 0);
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

// ---- host ------------------------------------------------------------------------------------------------------------------
int64_t moe_tile_bound(int64_t T, int64_t E, int64_t top_k) {
    const int64_t slots = T * top_k;
    return slots <= 0 ? 0 : cdiv64(slots, TILE_R) + std::min<int64_t>(E, slots);
}

// The small-T rule: which kernel the two GEMMs launch.  It depends on the shape alone, so a captured step replays the choice
// it was captured with.  Only T decides today: the measured crossover moved with neither K nor N.
bool moe_tile_use_slab(int64_t T, int64_t K, int64_t N, int E, int top_k) {
    (void)K, (void)N, (void)E, (void)top_k;
    if (g_tile_force >= 0) return g_tile_force == 1;
    return T <= TGIS_MOE_TILE_SLAB_MAX_T;
}

int moe_tile_check_tiles(const char* fn, const void* tiles, int64_t tile_bound, int64_t T, int E, int top_k) {
    TGIS_CHECK_ARG(tiles && ((uintptr_t)tiles % 16) == 0, "%s: null or unaligned tile list", fn);
    TGIS_CHECK_ARG(tile_bound >= moe_tile_bound(T, E, top_k), "%s: the tile list holds %ld tiles, tgis_moe_tile_bound asks for %ld",
                   fn, (long)tile_bound, (long)moe_tile_bound(T, E, top_k));
    TGIS_CHECK_ARG(tile_bound <= 65535, "%s: %ld tiles are more than a grid dimension holds: cut the tokens into chunks", fn,
                   (long)tile_bound);
    return TGIS_OK;
}

template <bool UP>
int moe_tile_launch(const MoeArgs& a, const int32_t* tiles, int64_t tile_bound, int64_t T, int E, int dtype, hipStream_t st) {
    const bool slab = moe_tile_use_slab(T, a.K, a.N, E, a.top_k);
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        if (slab)
            hipLaunchKernelGGL((moe_gemm_kernel<T_, UP, DenseSource<T_>>), dim3((unsigned)a.NT, (unsigned)E), dim3(MOE_THREADS), 0,
                               st, a);
        else
            hipLaunchKernelGGL((moe_tile_gemm_kernel<T_, UP>), dim3((unsigned)cdiv64(a.NT, TILE_C / 32), (unsigned)tile_bound),
                               dim3(TILE_THREADS), 0, st, a, tiles);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}

}  // namespace

extern "C" int64_t tgis_moe_tile_bound(int64_t T, int E, int top_k) { return moe_tile_bound(T, E, top_k); }

// bytes of tgis_moe_route_tiles' workspace: the [route blocks][E] histogram
extern "C" int64_t tgis_moe_route_tiles_bytes(int64_t T, int E, int top_k) {
    (void)top_k;
    return T <= 0 || E <= 0 ? 0 : cdiv64(T, RT_TOKENS) * E * 4;
}

extern "C" int tgis_moe_route_tiles(const float* logits, int64_t ld, int64_t T, int E, int top_k, int renorm, int32_t* expert_ids,
                                    float* expert_w, int32_t* counts, int32_t* offsets, int32_t* slot_rows, int32_t* tiles,
                                    int64_t tile_bound, int32_t* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "tgis_moe_route_tiles";
    const int rc = moe_check_routing(fn, T, E, top_k, TILE_MAX_E);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(renorm == 0 || renorm == 1, "%s: renorm must be 0 or 1", fn);
    TGIS_CHECK_ARG(counts && offsets && (T == 0 || (logits && expert_ids && expert_w && slot_rows)), "%s: null tensor", fn);
    TGIS_CHECK_ARG(T == 0 || ld >= E, "%s: the logit row stride (%ld) must be at least E", fn, (long)ld);
    const int rc2 = moe_tile_check_tiles(fn, tiles, tile_bound, T, E, top_k);
    if (rc2 != TGIS_OK) return rc2;
    TGIS_CHECK_ARG(T == 0 || (workspace && workspace_bytes >= tgis_moe_route_tiles_bytes(T, E, top_k)),
                   "%s: workspace too small (%ld < %ld)", fn, (long)workspace_bytes, (long)tgis_moe_route_tiles_bytes(T, E, top_k));
    hipStream_t st = (hipStream_t)stream;
    const int NB = (int)cdiv64(T, RT_TOKENS);
    if (NB > 0) {
        hipLaunchKernelGGL(moe_tile_route_kernel, dim3(NB), dim3(RT_THREADS), 0, st, logits, ld, (int)T, E, top_k, renorm,
                           expert_ids, expert_w, workspace);
        TGIS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(moe_tile_scan_kernel, dim3(1), dim3(TILE_MAX_E), 0, st, workspace, NB, E, counts, offsets, tiles,
                       (int)tile_bound);
    TGIS_CHECK_LAUNCH();
    if (NB > 0) {
        hipLaunchKernelGGL(moe_tile_scatter_kernel, dim3(NB), dim3(RT_THREADS), 0, st, expert_ids, (int)(T * top_k), E, top_k,
                           workspace, offsets, slot_rows);
        TGIS_CHECK_LAUNCH();
    }
    return TGIS_OK;
}

extern "C" int tgis_moe_tile_gemm_up(const void* x, int64_t ldx, const void* images, int64_t expert_stride, const int32_t* offsets,
                                     const int32_t* slot_rows, const int32_t* tiles, int64_t tile_bound, void* h, int64_t ldh,
                                     int64_t T, int64_t K, int64_t N, int E, int top_k, int dtype, void* stream) {
    const char* fn = "tgis_moe_tile_gemm_up";
    const int rc = moe_check_gemm(fn, x, ldx, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype, 0, TILE_MAX_E);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(N % 32 == 0, "%s: the gate|up image needs N / 2 (%ld) to be a multiple of 16", fn, (long)(N / 2));
    TGIS_CHECK_ARG(h && ldh >= N / 2, "%s: h rows must hold N / 2 elements", fn);
    const int rc2 = moe_tile_check_tiles(fn, tiles, tile_bound, T, E, top_k);
    if (rc2 != TGIS_OK) return rc2;
    if (T == 0) return TGIS_OK;
    MoeArgs a;
    moe_fill(a, x, ldx, images, expert_stride, offsets, slot_rows, nullptr, h, ldh, K, N, top_k, 0);
    TgisTimedScope timed(TGIS_OP_DENSE_GEMM, (hipStream_t)stream);
    return moe_tile_launch<true>(a, tiles, tile_bound, T, E, dtype, (hipStream_t)stream);
}

extern "C" int64_t tgis_moe_tile_gemm_down_bytes(int64_t T, int64_t N, int top_k, int form) {
    return tgis_moe_gemm_down_bytes(T, N, top_k, form);
}

extern "C" int tgis_moe_tile_gemm_down(const void* h, int64_t ldh, const void* images, int64_t expert_stride,
                                       const int32_t* offsets, const int32_t* slot_rows, const int32_t* tiles, int64_t tile_bound,
                                       const float* expert_w, int64_t T, int64_t K, int64_t N, int E, int top_k, int dtype,
                                       int form, float* scratch, int64_t scratch_bytes, void* out, int64_t ldo, void* stream) {
    const char* fn = "tgis_moe_tile_gemm_down";
    const int rc = moe_check_gemm(fn, h, ldh, images, expert_stride, offsets, slot_rows, T, K, N, E, top_k, dtype, 0, TILE_MAX_E);
    if (rc != TGIS_OK) return rc;
    const int rc2 = moe_check_down(fn, expert_w, T, N, top_k, form, out, ldo);
    if (rc2 != TGIS_OK) return rc2;
    const int rc3 = moe_tile_check_tiles(fn, tiles, tile_bound, T, E, top_k);
    if (rc3 != TGIS_OK) return rc3;
    if (T == 0) return TGIS_OK;
    TGIS_CHECK_ARG(scratch && ((uintptr_t)scratch % 16) == 0 && scratch_bytes >= tgis_moe_tile_gemm_down_bytes(T, N, top_k, form),
                   "%s: scratch too small (%ld < %ld)", fn, (long)scratch_bytes,
                   (long)tgis_moe_tile_gemm_down_bytes(T, N, top_k, form));
    hipStream_t st = (hipStream_t)stream;
    MoeArgs a;
    moe_fill(a, h, ldh, images, expert_stride, offsets, slot_rows, expert_w, scratch, form == 0 ? cdiv64(N, 32) * 32 : N, K, N,
             top_k, form);
    TgisTimedScope timed(TGIS_OP_DENSE_GEMM, st);
    const int rc4 = moe_tile_launch<false>(a, tiles, tile_bound, T, E, dtype, st);
    if (rc4 != TGIS_OK || form == 0) return rc4;
    return by_dtype(dtype, [&](auto t) {
        using T_ = type_of<decltype(t)>;
        hipLaunchKernelGGL(moe_combine_kernel<T_>, dim3((unsigned)cdiv64(T * (N / 4), 256)), dim3(256), 0, st, scratch, (T_*)out,
                           ldo, T, (int)N, top_k);
        TGIS_CHECK_LAUNCH();
        return TGIS_OK;
    });
}

// Host-only debug exports, kept out of include/tgis_hip.h like tgis_debug_moe_plan.
// tgis_debug_moe_tile_force: -1 the small-T rule, 0 always the tile kernel, 1 always the slab kernel body (benchmarks, tests).
extern "C" int tgis_debug_moe_tile_force(int kernel) {
    TGIS_CHECK_ARG(kernel >= -1 && kernel <= 1, "tgis_debug_moe_tile_force: -1, 0 or 1");
    g_tile_force = kernel;
    return TGIS_OK;
}

// The launch plan of the three entry points without a launch.  which: 0 up, 1 down form 0, 2 down form 1.  info[16]:
//   0 grid.x   1 grid.y   2 threads per block   3 static LDS bytes   4 rows per block (a tile, or a slab)
//   5 image columns per block   6 kernel: 0 tile, 1 slab body   7 second launch (the combine of form 1): blocks, else 0
//   8 fp32 scratch bytes (low 31 bits)   9 scratch bytes >> 31   10 tile bound   11 route blocks   12 tokens per route block
//   13 route workspace bytes (low 31 bits)   14 tokens up to which the rule picks the slab body
extern "C" int tgis_debug_moe_tile_plan(int which, int64_t T, int64_t K, int64_t N, int E, int top_k, int* info) {
    TGIS_CHECK_ARG(info && which >= 0 && which <= 2, "tgis_debug_moe_tile_plan: bad arguments");
    const int rc = moe_check_routing("tgis_debug_moe_tile_plan", T, E, top_k, TILE_MAX_E);
    if (rc != TGIS_OK) return rc;
    TGIS_CHECK_ARG(K > 0 && K % 8 == 0 && N > 0 && (which != 0 || N % 32 == 0), "tgis_debug_moe_tile_plan: bad shape");
    for (int i = 0; i < 16; ++i) info[i] = 0;
    const int64_t NT = cdiv64(N, 32), bound = moe_tile_bound(T, E, top_k);
    const bool slab = moe_tile_use_slab(T, K, N, E, top_k);
    info[0] = slab ? (int)NT : (int)cdiv64(NT, TILE_C / 32), info[1] = slab ? E : (int)bound;
    info[2] = slab ? MOE_THREADS : TILE_THREADS, info[3] = slab ? MOE_LDS : TILE_LDS;
    info[4] = slab ? 32 : TILE_R, info[5] = slab ? 32 : TILE_C, info[6] = slab ? 1 : 0;
    info[7] = which == 2 ? (int)cdiv64(T * (N / 4), 256) : 0;
    const int64_t bytes = which == 0 ? 0 : tgis_moe_tile_gemm_down_bytes(T, N, top_k, which - 1);
    info[8] = (int)(bytes & 0x7fffffff), info[9] = (int)(bytes >> 31);
    info[10] = (int)bound, info[11] = (int)cdiv64(T, RT_TOKENS), info[12] = RT_TOKENS;
    info[13] = (int)(tgis_moe_route_tiles_bytes(T, E, top_k) & 0x7fffffff), info[14] = TGIS_MOE_TILE_SLAB_MAX_T;
    return TGIS_OK;
}
