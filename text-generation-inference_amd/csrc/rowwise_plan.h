// Launch forms of the row-wise kernels: one chooser per kernel family, called by its launcher and reported without a
// launch by tgis_debug_rowwise_plan (elementwise.hip), a host-only debug export kept out of include/tgis_hip.h.
#pragma once
#include <stdint.h>

// norm_kernel / layernorm2_kernel: NT threads per row, each looping over `iters` 16-byte chunks of the row
struct NormPlan {
    int nt;
    int iters;
};
NormPlan choose_norm(int64_t rows, int64_t hidden);  // norm.hip

// rope_kv_kernel: grid (T, gy); `strided` when gy * 256 threads do not cover a token's items in one pass
struct RopePlan {
    int gy;
    bool gen;
    bool strided;
    int items;
};
RopePlan choose_rope(int64_t T, int H, int Hkv, int D, int rot_dim, bool rope);  // rope_kv.hip

// rope_kv_prefill_kernel: pps 32-token pages per sequence in the grid
struct RopePrefillPlan {
    int pps;
    bool gen;
};
RopePrefillPlan choose_rope_prefill(int64_t max_len, int rot_dim, bool rope);  // rope_kv.hip

// argmax_logprob: nseg segments per row through argmax_part_kernel + argmax_merge_kernel (split), else one block per row
struct ArgmaxPlan {
    int nseg;
    bool split;
    int seg_len;
};
ArgmaxPlan choose_argmax(int64_t B, int64_t V, const void* scratch, int64_t scratch_bytes);  // elementwise.hip

// warp_sample: the row in registers (warp_sample_reg_kernel) or re-read from global memory (warp_sample_kernel)
struct SamplerPlan {
    bool reg;
};
SamplerPlan choose_sampler(int64_t V);  // sampler.hip
