// Prompt-lookup speculative decoding, the device side of its bookkeeping: the (K + 1)-row forms of the decode step's
// slot and advance helpers (elementwise.hip) and the n-gram lookup that drafts the next step's tokens.  Nothing here
// touches activations; every kernel is a handful of integer loads and stores per request.
#include "common.h"

namespace {

// Row b * (K + 1) + j of the verify forward: j = 0 is the request's latest token, j > 0 its j-th draft, at position
// pos + j.  A table index past the row's last entry is clamped (the host only verifies requests whose K + 1 positions lie
// inside their tables; the clamp keeps a broken caller inside the table).
__global__ void spec_stage_kernel(const int32_t* __restrict__ positions, const int64_t* __restrict__ latest,
                                  const int64_t* __restrict__ drafts, int K, const int32_t* __restrict__ bt,
                                  int64_t max_pages, int64_t* __restrict__ input_ids, int32_t* __restrict__ pos_out,
                                  int32_t* __restrict__ slots, int32_t* __restrict__ ctx, int64_t B) {
    const int K1 = K + 1;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * K1) return;
    const int64_t b = r / K1;
    const int j = (int)(r - b * K1);
    const int pos = positions[b] + j;
    int64_t pi = pos >> 5;
    pi = pi < 0 ? 0 : (pi >= max_pages ? max_pages - 1 : pi);
    const int page = bt[b * max_pages + pi];
    input_ids[r] = j == 0 ? latest[b] : drafts[b * K + (j - 1)];
    pos_out[r] = pos;
    slots[r] = page * TGIS_KV_PAGE_TOKENS + (pos & 31);
    if (j == 0) ctx[b] = pos + K1;
}

// am_ids / am_lps: the token chosen behind every verify row and its logprob — the argmax (tgis_spec_accept) or whatever
// tgis_warp_sample_verify chose (tgis_spec_accept_sampled, which also passes the streams to advance; null: none).
// One workgroup for the whole batch: the counts of all requests are B * K compares, so the block that needs their prefix
// sums (cu_seqlens) recomputes nothing across workgroups and synchronises with nobody but itself.
__global__ __launch_bounds__(256) void spec_accept_kernel(
    const int64_t* __restrict__ am_ids, const float* __restrict__ am_lps, const int64_t* __restrict__ drafts, int K,
    int32_t* __restrict__ n_emit, int64_t* __restrict__ out_ids, float* __restrict__ out_lps, int64_t* __restrict__ latest,
    int64_t* __restrict__ position_ids, int64_t* __restrict__ all_ids, int64_t ld_all, int32_t* __restrict__ cu_seqlens,
    int64_t* __restrict__ stage_ids, int32_t* __restrict__ stage_pos, const int* __restrict__ do_sample,
    uint64_t* __restrict__ rng, int64_t B) {
    const int K1 = K + 1;
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
        const int64_t* a = am_ids + b * K1;
        int n = 1;  // the row behind the longest accepted prefix is emitted as well: it is the model's own next token
        for (int j = 0; j < K; ++j) {
            if (a[j] != drafts[b * K + j]) break;
            ++n;
        }
        n_emit[b] = n;
        // a sampled request drew once per emitted token (the rows behind the first miss drew for nothing: their draws are
        // made again, at the same offsets, by the steps that emit those positions)
        if (do_sample && do_sample[b]) rng[2 * b + 1] += (uint64_t)n;
        const int64_t pos = position_ids[b];
        for (int j = 0; j < K1; ++j) {
            const bool emit = j < n;
            const int64_t id = a[j];
            if (out_ids) out_ids[b * K1 + j] = emit ? id : -1;
            if (out_lps) out_lps[b * K1 + j] = emit ? am_lps[b * K1 + j] : 0.f;
            const int64_t p = pos + 1 + j;
            if (emit && all_ids && p >= 0 && p < ld_all) all_ids[b * ld_all + p] = id;
        }
        const int64_t last = a[n - 1], new_pos = pos + n;
        position_ids[b] = new_pos;
        if (latest) latest[b] = last;
        if (stage_ids) stage_ids[b] = last;
        if (stage_pos) stage_pos[b] = (int32_t)new_pos;
    }
    if (!cu_seqlens) return;
    __syncthreads();  // n_emit of every request is written (one workgroup: the barrier orders its global stores too)
    for (int64_t b = threadIdx.x; b <= B; b += blockDim.x) {
        int s = (int)b;  // K = 0: every request emitted one token
        if (K > 0) {
            s = 0;
            for (int64_t i = 0; i < b; ++i) s += n_emit[i];
        }
        cu_seqlens[b] += s;  // B + 1 entries
    }
}

// One workgroup per request.  For n = N .. 1: the largest j with j + n < len and tokens[j, j + n) == tokens[len - n, len);
// the first n that finds one wins.  The suffix goes through LDS so that every thread compares against the same registers.
__global__ __launch_bounds__(256) void spec_propose_kernel(const int64_t* __restrict__ all_ids, int64_t ld_all,
                                                           const int64_t* __restrict__ position_ids, int K, int N,
                                                           int64_t* __restrict__ drafts, int32_t* __restrict__ hits,
                                                           int32_t* __restrict__ hits_copy) {
    __shared__ int64_t suf[4];
    __shared__ int best;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t* tok = all_ids + b * ld_all;
    int64_t len64 = position_ids[b] + 1;  // the context ends with the latest token, at position_ids[b]
    len64 = len64 < 0 ? 0 : (len64 > ld_all ? ld_all : len64);
    const int len = (int)len64;
    int hit = 0, start = 0;
    for (int n = N; n >= 1; --n) {
        if (n + 1 > len) continue;  // (uniform) no j >= 0 with j + n < len
        if (tid == 0) best = -1;
        if (tid < n) suf[tid] = tok[len - n + tid];
        __syncthreads();
        int mine = -1;
        for (int j = tid; j + n < len; j += blockDim.x) {
            bool eq = true;
            for (int i = 0; i < n; ++i) eq = eq && tok[j + i] == suf[i];
            if (eq) mine = j;  // j only grows: the last one kept is this thread's largest
        }
        if (mine >= 0) atomicMax(&best, mine);
        __syncthreads();
        const int bj = best;
        __syncthreads();  // everyone has read `best` before a shorter n resets it
        if (bj >= 0) {
            hit = n;
            start = bj + n;
            break;
        }
    }
    if (tid < K) drafts[b * K + tid] = (hit && start + tid < len) ? tok[start + tid] : 0;
    if (tid == 0) {
        hits[b] = hit;
        if (hits_copy) hits_copy[b] = hit;
    }
}

}  // namespace

extern "C" int tgis_spec_stage(const int32_t* positions, const int64_t* latest_ids, const int64_t* drafts, int64_t K,
                               const int32_t* block_tables, int64_t max_pages, int64_t* input_ids, int32_t* positions_out,
                               int32_t* slots, int32_t* ctx_lens, int64_t B, void* stream) {
    TGIS_CHECK_ARG(positions && latest_ids && block_tables && input_ids && positions_out && slots && ctx_lens &&
                       max_pages > 0 && B >= 0 && K >= 0 && K <= 7 && (K == 0 || drafts),
                   "tgis_spec_stage: bad arguments");
    if (B == 0) return TGIS_OK;
    hipLaunchKernelGGL(spec_stage_kernel, dim3((unsigned)cdiv64(B * (K + 1), 64)), dim3(64), 0, (hipStream_t)stream, positions,
                       latest_ids, drafts, (int)K, block_tables, max_pages, input_ids, positions_out, slots, ctx_lens, B);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

namespace {

int spec_accept(const char* what, const int64_t* ids, const float* logprobs, const int64_t* drafts, int64_t K, int32_t* n_emit,
                int64_t* out_ids, float* out_logprobs, int64_t* latest_ids, int64_t* position_ids, int64_t* all_input_ids,
                int64_t ld_all, int32_t* cu_seqlens, int64_t* stage_ids, int32_t* stage_positions, const int* do_sample,
                uint64_t* rng, int64_t B, void* stream) {
    // (an empty batch has no buffers to speak of: a tensor without elements hands over a null pointer)
    TGIS_CHECK_ARG(B >= 0 && K >= 0 && K <= 7 &&
                       (B == 0 || (ids && n_emit && position_ids && (K == 0 || drafts) && (!out_logprobs || logprobs) &&
                                   (!all_input_ids || ld_all > 0) && (!do_sample || rng))),
                   "%s: bad arguments", what);
    if (B == 0) return TGIS_OK;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ids, logprobs, drafts, (int)K, n_emit,
                       out_ids, out_logprobs, latest_ids, position_ids, all_input_ids, ld_all, cu_seqlens, stage_ids,
                       stage_positions, do_sample, rng, B);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

}  // namespace

extern "C" int tgis_spec_accept(const int64_t* argmax_ids, const float* argmax_logprobs, const int64_t* drafts, int64_t K,
                                int32_t* n_emit, int64_t* out_ids, float* out_logprobs, int64_t* latest_ids,
                                int64_t* position_ids, int64_t* all_input_ids, int64_t ld_all, int32_t* cu_seqlens,
                                int64_t* stage_ids, int32_t* stage_positions, int64_t B, void* stream) {
    return spec_accept("tgis_spec_accept", argmax_ids, argmax_logprobs, drafts, K, n_emit, out_ids, out_logprobs, latest_ids,
                       position_ids, all_input_ids, ld_all, cu_seqlens, stage_ids, stage_positions, nullptr, nullptr, B, stream);
}

extern "C" int tgis_spec_accept_sampled(const int64_t* chosen_ids, const float* chosen_logprobs, const int64_t* drafts,
                                        int64_t K, int32_t* n_emit, int64_t* out_ids, float* out_logprobs,
                                        int64_t* latest_ids, int64_t* position_ids, int64_t* all_input_ids, int64_t ld_all,
                                        int32_t* cu_seqlens, int64_t* stage_ids, int32_t* stage_positions,
                                        const int* do_sample, uint64_t* rng, int64_t B, void* stream) {
    return spec_accept("tgis_spec_accept_sampled", chosen_ids, chosen_logprobs, drafts, K, n_emit, out_ids, out_logprobs,
                       latest_ids, position_ids, all_input_ids, ld_all, cu_seqlens, stage_ids, stage_positions, do_sample, rng,
                       B, stream);
}

extern "C" int tgis_spec_propose(const int64_t* all_input_ids, int64_t ld_all, const int64_t* position_ids, int64_t K,
                                 int64_t N, int64_t* drafts, int32_t* hits, int32_t* hits_copy, int64_t B, void* stream) {
    TGIS_CHECK_ARG(all_input_ids && position_ids && drafts && hits && B >= 0 && K >= 1 && K <= 7 && N >= 1 && N <= 4 &&
                       ld_all > 0 && ld_all < (1ll << 31),
                   "tgis_spec_propose: bad arguments");
    if (B == 0) return TGIS_OK;
    hipLaunchKernelGGL(spec_propose_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, all_input_ids, ld_all,
                       position_ids, (int)K, (int)N, drafts, hits, hits_copy);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}
