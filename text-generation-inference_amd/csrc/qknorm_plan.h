// Launch forms of the q/k RMSNorm + rope + cache-write kernels (qk_norm_rope.hip): the choosers its launchers call, reported
// without a launch by tgis_debug_qknorm_plan, a host-only debug export kept out of include/tgis_hip.h.
#pragma once
#include <stdint.h>

// One head is the work of QKN_LANES consecutive lanes of a wave (lane j: 8-element chunk j; D / 8 = 8, 12 or 16 of them are
// busy), so a 256-thread block takes QKN_HEADS heads per pass.
constexpr int QKN_LANES = 16;
constexpr int QKN_HEADS = 256 / QKN_LANES;

// qknorm_rope_kv_kernel: grid (T, gy); `strided` when gy blocks do not cover a token's H + 2 Hkv heads in one pass
struct QkNormPlan {
    int gy;
    bool strided;
    int heads;
    int idle;  // lanes of a head's QKN_LANES that hold no chunk
};
inline QkNormPlan choose_qknorm(int64_t T, int H, int Hkv, int D) {
    const int heads = H + 2 * Hkv;
    const int need = (heads + QKN_HEADS - 1) / QKN_HEADS;
    const int gy = T <= 64 ? (need < 16 ? need : 16) : 1;  // decode-sized T: one token's heads over several workgroups
    return {gy, gy * QKN_HEADS < heads, heads, QKN_LANES - (D >> 3)};
}

// qknorm_rope_kv_prefill_kernel: pps 32-token pages per sequence in the grid; the block's 32 k rows take `stat_passes` passes
// of QKN_HEADS rows for their statistics and `k_passes` passes of 256 (token, chunk) items for the stores
struct QkNormPrefillPlan {
    int pps;
    int stat_passes;
    int k_passes;
};
inline QkNormPrefillPlan choose_qknorm_prefill(int64_t max_len, int D) {
    return {(int)((max_len + 31) / 32), 32 / QKN_HEADS, (32 * (D >> 3) + 255) / 256};
}
