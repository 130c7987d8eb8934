// Arrival counters of in-launch merges: a pool of zeroed device arrays per device, leased per stream.  It knows nothing of
// the launches that count in them (attention.hip: one counter per group of key-split blocks).
#pragma once
#include <stdio.h>
#include <map>
#include <mutex>
#include "common.h"

namespace {
constexpr int64_t ATTN_COUNTERS = 1 << 20;
constexpr int ATTN_COUNTER_SETS = 4;

// Arrival counters of the fused combine, one per group; zero between launches (the last arriver resets its own).
// Owned by the library: a pool of ATTN_COUNTER_SETS arrays per device, handed out per STREAM — two split-key launches that
// overlap on one device are necessarily on different streams, so they never share an array (launches of one stream are
// ordered).  The pool is allocated by the first call that is not inside a stream capture (the eager warm-up step); handing
// an array of the pool to a new stream needs no allocation, so a capture stream gets one too.  A fifth concurrent stream,
// or a capture before any eager call, falls back to the separate combine launch.
struct CounterPool {
    unsigned* sets[ATTN_COUNTER_SETS] = {};
    hipStream_t owner[ATTN_COUNTER_SETS] = {};
    uint64_t last_use[ATTN_COUNTER_SETS] = {};  // launch stamp: the least recently used slot is handed to a new stream
    bool in_graph[ATTN_COUNTER_SETS] = {};      // a captured graph holds this slot's pointer: it never changes hands
    int pending[ATTN_COUNTER_SETS] = {};        // handed out, launch not enqueued yet: an idle owner stream proves nothing
    uint64_t stamp = 0;
    int used = 0;
    bool ready = false;
    bool warned = false;
};
std::mutex g_attn_counters_mu;
std::map<int, CounterPool> g_attn_counters;

// `slot` receives the index to give back with attn_counters_enqueued() once the launch that uses the array is in its
// stream (between this call and the launch a second host thread could see the new owner's stream idle and take
// the same array).
unsigned* attn_counters(hipStream_t st, int* dev_out, int* slot) {
    *slot = -1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    *dev_out = dev;
    std::lock_guard<std::mutex> lock(g_attn_counters_mu);
    CounterPool& pool = g_attn_counters[dev];
    if (!pool.ready) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
            (void)hipGetLastError();
            return nullptr;
        }
        unsigned* p = nullptr;
        const size_t bytes = (size_t)ATTN_COUNTER_SETS * ATTN_COUNTERS * sizeof(unsigned);
        if (hipMalloc((void**)&p, bytes) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        (void)hipDeviceSynchronize();
        for (int i = 0; i < ATTN_COUNTER_SETS; ++i) pool.sets[i] = p + (size_t)i * ATTN_COUNTERS;
        pool.ready = true;
    }
    ++pool.stamp;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool query_failed = hipStreamIsCapturing(st, &cs) != hipSuccess;
    if (query_failed) (void)hipGetLastError();  // not this launch's error: do not leave it for TGIS_CHECK_LAUNCH
    const bool capturing = query_failed || cs != hipStreamCaptureStatusNone;
    for (int i = 0; i < pool.used; ++i)
        if (pool.owner[i] == st) {
            pool.last_use[i] = pool.stamp;
            pool.in_graph[i] |= capturing;
            ++pool.pending[i];
            *slot = i;
            return pool.sets[i];
        }
    if (pool.used < ATTN_COUNTER_SETS) {
        pool.owner[pool.used] = st;
        pool.last_use[pool.used] = pool.stamp;
        pool.in_graph[pool.used] = capturing;
        ++pool.pending[pool.used];
        *slot = pool.used;
        return pool.sets[pool.used++];
    }
    // All slots are owned.  A slot whose stream has no launch in flight can change hands (its counters are zero between
    // launches): take the least recently used one if its stream is idle (hipStreamQuery on a destroyed or capturing stream
    // fails — then the slot stays put and this launch uses the separate combine kernel, which is always correct).
    // (a slot whose pointer sits in a captured graph stays where it is: the graph replays on streams this pool never sees)
    int lru = -1;
    for (int i = 0; i < ATTN_COUNTER_SETS; ++i)
        if (!pool.in_graph[i] && pool.pending[i] == 0 && (lru < 0 || pool.last_use[i] < pool.last_use[lru])) lru = i;
    hipStreamCaptureStatus ocs = hipStreamCaptureStatusNone;
    // (a query on a stream that is being captured would invalidate its capture: ask that first)
    const bool owner_capturing = lru < 0 || hipStreamIsCapturing(pool.owner[lru], &ocs) != hipSuccess ||
                                 ocs != hipStreamCaptureStatusNone;
    if (!capturing && !owner_capturing && hipStreamQuery(pool.owner[lru]) == hipSuccess) {
        pool.owner[lru] = st;
        pool.last_use[lru] = pool.stamp;
        ++pool.pending[lru];
        *slot = lru;
        return pool.sets[lru];
    }
    (void)hipGetLastError();
    if (!pool.warned) {
        pool.warned = true;
        fprintf(stderr, "tgis_attn_paged: more than %d streams use split-key decode attention on device %d; the extra ones "
                        "merge their splits with a second launch\n", ATTN_COUNTER_SETS, dev);
    }
    return nullptr;
}
void attn_counters_enqueued(int dev, int slot) {
    if (slot < 0) return;
    std::lock_guard<std::mutex> lock(g_attn_counters_mu);
    --g_attn_counters[dev].pending[slot];
}
struct CounterLease {  // gives the slot back when the launch is in its stream (or the call fails before it)
    int dev = 0, slot = -1;
    ~CounterLease() { attn_counters_enqueued(dev, slot); }
};
}  // namespace
