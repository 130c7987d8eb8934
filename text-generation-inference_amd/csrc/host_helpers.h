// Host-only helpers that more than one translation unit of libtgis_hip.so needs (no device code).  They are `static`: each
// translation unit that uses one keeps its own copy, and no symbol of theirs leaves the library.
#pragma once
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "common.h"

// TGIS_ROPE_MIN_BLOCKS: workgroups the unsplit plan of a fused qkv + rotary launch must still have (default 128).  The int4
// and dense *_rope_ok answers each put their own cap on top of it.
static inline int64_t rope_min_blocks_env() {
    static const int64_t v = getenv("TGIS_ROPE_MIN_BLOCKS") ? atoll(getenv("TGIS_ROPE_MIN_BLOCKS")) : 128;
    return v;
}

// The g_idx of a GPTQ checkpoint (host memory, K entries, group size gs) for a prepare entry point `fn`: *perm_dev stays
// null for a trivial g_idx (row k in group k / gs); an act-order one gives the stable-sorted row permutation, copied to
// perm_out (device, K entries) after the stream has drained.
static inline int gptq_act_order_perm(const char* fn, const int32_t* g_idx_host, int32_t* perm_out, int64_t K, int64_t gs,
                                      hipStream_t st, const int32_t** perm_dev) {
    *perm_dev = nullptr;
    bool trivial = true;
    for (int64_t k = 0; k < K; ++k)
        if (g_idx_host[k] != (int32_t)(k / gs)) { trivial = false; break; }
    if (trivial) return TGIS_OK;
    TGIS_CHECK_ARG(perm_out, "%s: act-order g_idx needs perm_out", fn);
    std::vector<int32_t> perm(K);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return g_idx_host[a] < g_idx_host[b]; });
    // every group must own exactly gs rows (true for GPTQ act-order checkpoints)
    for (int64_t k = 0; k < K; ++k)
        TGIS_CHECK_ARG(g_idx_host[perm[k]] == (int32_t)(k / gs), "%s: g_idx groups are not of uniform size", fn);
    TGIS_CHECK_HIP(hipStreamSynchronize(st));
    TGIS_CHECK_HIP(hipMemcpy(perm_out, perm.data(), K * sizeof(int32_t), hipMemcpyHostToDevice));
    *perm_dev = perm_out;
    return TGIS_OK;
}
