// Prompt-lookup speculative decoding, the device side of its bookkeeping: the (K + 1)-row forms of the decode step's
// slot and advance helpers (elementwise.hip) and the n-gram lookup that drafts the next step's tokens.  Nothing here
// touches activations; every kernel is a handful of integer loads and stores per request.  The tree forms (several candidates
// per request) add one kernel that does move cache bytes: the commit of a later candidate's keys and values.
#include <type_traits>
#include "common.h"
#include "kv_layout.h"

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

// ---- several candidates per request: the verify step as a token tree ---------------------------------------------------
// R = 1 + C K rows per request.  Row 0 is the latest token (rotary position pos, cache position pos); row 1 + c K + j is
// draft j of candidate c: rotary position pos + 1 + j (its depth), cache position pos + 1 + c K + j (its row).
namespace {

__global__ void spec_tree_stage_kernel(const int32_t* __restrict__ positions, const int64_t* __restrict__ latest,
                                       const int64_t* __restrict__ drafts, int C, int K, const int32_t* __restrict__ bt,
                                       int64_t max_pages, int64_t* __restrict__ input_ids, int32_t* __restrict__ pos_out,
                                       int32_t* __restrict__ slots, int32_t* __restrict__ ctx, int64_t B) {
    const int R = 1 + C * K;
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * R) return;
    const int64_t b = r / R;
    const int j = (int)(r - b * R);
    const int pos0 = positions[b];
    const int depth = j == 0 ? 0 : 1 + (j - 1) % K;
    const int pos = pos0 + j;  // where the row's keys and values go
    int64_t pi = pos >> 5;
    pi = pi < 0 ? 0 : (pi >= max_pages ? max_pages - 1 : pi);
    const int page = bt[b * max_pages + pi];
    input_ids[r] = j == 0 ? latest[b] : drafts[b * (C * K) + (j - 1)];
    pos_out[r] = pos0 + depth;
    slots[r] = page * TGIS_KV_PAGE_TOKENS + (pos & 31);
    if (j == 0) ctx[b] = pos0 + R;
}

// spec_accept_kernel over C candidates: the same bookkeeping along the best candidate's path.
__global__ __launch_bounds__(256) void spec_tree_accept_kernel(
    const int64_t* __restrict__ am_ids, const float* __restrict__ am_lps, const int64_t* __restrict__ drafts, int C, int K,
    int32_t* __restrict__ n_emit, int32_t* __restrict__ best, int64_t* __restrict__ out_ids, float* __restrict__ out_lps,
    int64_t* __restrict__ latest, int64_t* __restrict__ position_ids, int64_t* __restrict__ all_ids, int64_t ld_all,
    int32_t* __restrict__ cu_seqlens, int64_t* __restrict__ stage_ids, int32_t* __restrict__ stage_pos, int64_t B) {
    const int K1 = K + 1, R = 1 + C * K;
    for (int64_t b = threadIdx.x; b < B; b += blockDim.x) {
        const int64_t* a = am_ids + b * R;
        int bc = 0, ba = -1;
        for (int c = 0; c < C; ++c) {
            const int64_t* d = drafts + (b * C + c) * K;
            int acc = 0;  // draft j is right when the choice behind its parent row (row 0, or the candidate's draft j - 1) is it
            for (int j = 0; j < K; ++j) {
                if (a[j == 0 ? 0 : c * K + j] != d[j]) break;
                ++acc;
            }
            if (acc > ba) {  // the first maximum
                ba = acc;
                bc = c;
            }
        }
        const int n = ba + 1;  // the row behind the accepted prefix is emitted as well
        n_emit[b] = n;
        best[b] = bc;
        const int64_t pos = position_ids[b];
        int64_t last = 0;
        for (int j = 0; j < K1; ++j) {
            const bool emit = j < n;
            const int row = j == 0 ? 0 : bc * K + j;  // the path: row 0, then the candidate's drafts 0 .. a - 1
            const int64_t id = emit ? a[row] : -1;
            if (emit) last = id;
            if (out_ids) out_ids[b * K1 + j] = id;
            if (out_lps) out_lps[b * K1 + j] = emit ? am_lps[b * R + row] : 0.f;
            const int64_t p = pos + 1 + j;
            if (emit && all_ids && p >= 0 && p < ld_all) all_ids[b * ld_all + p] = id;
        }
        const int64_t new_pos = pos + n;
        position_ids[b] = new_pos;
        if (latest) latest[b] = last;
        if (stage_ids) stage_ids[b] = last;
        if (stage_pos) stage_pos[b] = (int32_t)new_pos;
    }
    if (!cu_seqlens) return;
    __syncthreads();  // n_emit of every request is written (one workgroup: the barrier orders its global stores too)
    for (int64_t b = threadIdx.x; b <= B; b += blockDim.x) {
        int s = (int)b;
        if (K > 0) {
            s = 0;
            for (int64_t i = 0; i < b; ++i) s += n_emit[i];
        }
        cu_seqlens[b] += s;
    }
}

// One workgroup per (layer, kv head) and request; E = bytes per pool element.  Thread items: (moved token j, one 8-element run
// of K) and (moved token j, one element of V), the orders of kv_layout.h.
template <int E>
__global__ __launch_bounds__(256) void spec_tree_commit_kernel(unsigned char* __restrict__ kpool, unsigned char* __restrict__ vpool,
                                                               int64_t layer_stride, int64_t num_pages,
                                                               const int32_t* __restrict__ bt, int64_t max_pages,
                                                               const int32_t* __restrict__ new_positions,
                                                               const int32_t* __restrict__ best,
                                                               const int32_t* __restrict__ n_emit, int C, int K, int Hkv, int D) {
    const int64_t b = blockIdx.y;
    const int layer = blockIdx.x / Hkv, hk = blockIdx.x % Hkv;
    const int n = min(max(n_emit[b], 1), K + 1);
    const int bc = min(max(best[b], 0), C - 1);
    if (bc == 0 || n == 1) return;  // the first candidate's rows already sit where a chain's would
    const int pos = new_positions[b] - n;  // the latest token of the step that was verified
    const int runs = D >> 3, per_tok = runs + D;
    using KRun = std::conditional_t<E == 2, u32x4, u32x2>;
    using VEl = std::conditional_t<E == 2, uint16_t, uint8_t>;
    const int32_t* btrow = bt + b * max_pages;
    for (int item = threadIdx.x; item < (n - 1) * per_tok; item += blockDim.x) {
        const int j = item / per_tok, i = item - j * per_tok;
        const int ps = pos + 1 + bc * K + j, pd = pos + 1 + j;
        int64_t is = ps >> 5, id = pd >> 5;
        is = is < 0 ? 0 : (is >= max_pages ? max_pages - 1 : is);
        id = id < 0 ? 0 : (id >= max_pages ? max_pages - 1 : id);
        int64_t pgs = btrow[is], pgd = btrow[id];
        pgs = pgs < 0 ? 0 : (pgs >= num_pages ? num_pages - 1 : pgs);
        pgd = pgd < 0 ? 0 : (pgd >= num_pages ? num_pages - 1 : pgd);
        const int64_t bs = (int64_t)layer * layer_stride + (pgs * Hkv + hk) * (32 * (int64_t)D);
        const int64_t bd = (int64_t)layer * layer_stride + (pgd * Hkv + hk) * (32 * (int64_t)D);
        if (i < runs) {
            const KRun v = *reinterpret_cast<const KRun*>(kpool + (bs + k_off(ps & 31, i * 8, D)) * E);
            *reinterpret_cast<KRun*>(kpool + (bd + k_off(pd & 31, i * 8, D)) * E) = v;
        } else {
            const int d = i - runs;
            const VEl v = *reinterpret_cast<const VEl*>(vpool + (bs + v_off(ps & 31, d, D)) * E);
            *reinterpret_cast<VEl*>(vpool + (bd + v_off(pd & 31, d, D)) * E) = v;
        }
    }
}

// spec_propose_kernel for C candidates.  Sites are visited with n from N down to 1 and, within one n, from the latest to the
// earliest; a site is taken when the first token of its continuation (it always has one: j + n < len) differs from that of
// every candidate taken so far.  One scan of the context per candidate and n.
__global__ __launch_bounds__(256) void spec_propose_multi_kernel(const int64_t* __restrict__ all_ids, int64_t ld_all,
                                                                 const int64_t* __restrict__ position_ids, int C, int K,
                                                                 int N, int64_t* __restrict__ drafts,
                                                                 int32_t* __restrict__ hits, int32_t* __restrict__ hits_copy) {
    __shared__ int64_t suf[4];
    __shared__ int64_t first[8];
    __shared__ int starts[8];
    __shared__ int best;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t* tok = all_ids + b * ld_all;
    int64_t len64 = position_ids[b] + 1;
    len64 = len64 < 0 ? 0 : (len64 > ld_all ? ld_all : len64);
    const int len = (int)len64;
    int hit = 0, taken = 0;
    for (int n = N; n >= 1 && taken < C; --n) {
        if (n + 1 > len) continue;  // (uniform) no j >= 0 with j + n < len
        if (tid < n) suf[tid] = tok[len - n + tid];
        int bound = len - n;  // sites below it are still to be visited
        while (taken < C) {   // (uniform: `taken` and `bound` move together in every thread)
            if (tid == 0) best = -1;
            __syncthreads();  // suf, first[0 .. taken) and best are in
            int mine = -1;
            for (int j = tid; j < bound; j += blockDim.x) {
                bool eq = true;
                for (int i = 0; i < n; ++i) eq = eq && tok[j + i] == suf[i];
                const int64_t f = tok[j + n];
                for (int t = 0; t < taken; ++t) eq = eq && f != first[t];
                if (eq) mine = j;  // j only grows: the last one kept is this thread's largest
            }
            if (mine >= 0) atomicMax(&best, mine);
            __syncthreads();
            const int bj = best;
            __syncthreads();  // everyone has read `best` before it is reset
            if (bj < 0) break;
            if (taken == 0) hit = n;
            if (tid == 0) {
                first[taken] = tok[bj + n];
                starts[taken] = bj + n;
            }
            ++taken;
            bound = bj;
        }
        __syncthreads();  // suf is rewritten for a shorter n only after every thread has left this one's scans
    }
    __syncthreads();
    for (int i = tid; i < C * K; i += blockDim.x) {
        const int c = i / K, k = i - c * K;
        drafts[b * (C * K) + i] = (c < taken && starts[c] + k < len) ? tok[starts[c] + k] : 0;
    }
    if (tid == 0) {
        hits[b] = hit;
        if (hits_copy) hits_copy[b] = hit;
    }
}

bool tree_shape_ok(int64_t C, int64_t K) { return C >= 1 && C <= 8 && K >= 0 && K <= 7 && 1 + C * K <= 64 && (C == 1 || K >= 1); }

}  // namespace

extern "C" int tgis_spec_tree_stage(const int32_t* positions, const int64_t* latest_ids, const int64_t* drafts, int64_t C,
                                    int64_t K, const int32_t* block_tables, int64_t max_pages, int64_t* input_ids,
                                    int32_t* positions_out, int32_t* slots, int32_t* ctx_lens, int64_t B, void* stream) {
    TGIS_CHECK_ARG(positions && latest_ids && block_tables && input_ids && positions_out && slots && ctx_lens &&
                       max_pages > 0 && B >= 0 && tree_shape_ok(C, K) && (K == 0 || drafts),
                   "tgis_spec_tree_stage: bad arguments");
    if (B == 0) return TGIS_OK;
    if (K == 0) K = 1, C = 0;  // one row per request (the kernel divides by K)
    hipLaunchKernelGGL(spec_tree_stage_kernel, dim3((unsigned)cdiv64(B * (1 + C * K), 64)), dim3(64), 0, (hipStream_t)stream,
                       positions, latest_ids, drafts, (int)C, (int)K, block_tables, max_pages, input_ids, positions_out, slots,
                       ctx_lens, B);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int tgis_spec_tree_accept(const int64_t* argmax_ids, const float* argmax_logprobs, const int64_t* drafts, int64_t C,
                                     int64_t K, int32_t* n_emit, int32_t* best, int64_t* out_ids, float* out_logprobs,
                                     int64_t* latest_ids, int64_t* position_ids, int64_t* all_input_ids, int64_t ld_all,
                                     int32_t* cu_seqlens, int64_t* stage_ids, int32_t* stage_positions, int64_t B,
                                     void* stream) {
    TGIS_CHECK_ARG(B >= 0 && tree_shape_ok(C, K) &&
                       (B == 0 || (argmax_ids && n_emit && best && position_ids && (K == 0 || drafts) &&
                                   (!out_logprobs || argmax_logprobs) && (!all_input_ids || ld_all > 0))),
                   "tgis_spec_tree_accept: bad arguments");
    if (B == 0) return TGIS_OK;
    hipLaunchKernelGGL(spec_tree_accept_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, argmax_ids, argmax_logprobs, drafts,
                       (int)C, (int)K, n_emit, best, out_ids, out_logprobs, latest_ids, position_ids, all_input_ids, ld_all,
                       cu_seqlens, stage_ids, stage_positions, B);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int tgis_spec_tree_commit(void* k_pool, void* v_pool, int64_t layer_stride, int64_t num_layers, int64_t num_pages,
                                     const int32_t* block_tables, int64_t max_pages, const int32_t* new_positions,
                                     const int32_t* best, const int32_t* n_emit, int64_t C, int64_t K, int64_t B, int Hkv,
                                     int D, int elem_bytes, void* stream) {
    TGIS_CHECK_ARG(B >= 0 && tree_shape_ok(C, K) && K >= 1 && num_layers >= 1 && num_pages >= 1 && max_pages > 0 && Hkv > 0 &&
                       (D == 64 || D == 96 || D == 128) && (elem_bytes == 1 || elem_bytes == 2) && layer_stride >= 0 &&
                       num_layers * Hkv <= 2147483647LL && B <= 65535 &&
                       (B == 0 || (k_pool && v_pool && block_tables && new_positions && best && n_emit)) &&
                       ((uintptr_t)k_pool % 16) == 0 && (layer_stride * elem_bytes) % 16 == 0,
                   "tgis_spec_tree_commit: bad arguments");
    if (B == 0) return TGIS_OK;
    dim3 grid((unsigned)(num_layers * Hkv), (unsigned)B);
    if (elem_bytes == 2)
        hipLaunchKernelGGL(spec_tree_commit_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (unsigned char*)k_pool,
                           (unsigned char*)v_pool, layer_stride, num_pages, block_tables, max_pages, new_positions, best, n_emit,
                           (int)C, (int)K, Hkv, D);
    else
        hipLaunchKernelGGL(spec_tree_commit_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (unsigned char*)k_pool,
                           (unsigned char*)v_pool, layer_stride, num_pages, block_tables, max_pages, new_positions, best, n_emit,
                           (int)C, (int)K, Hkv, D);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}

extern "C" int tgis_spec_propose_multi(const int64_t* all_input_ids, int64_t ld_all, const int64_t* position_ids, int64_t C,
                                       int64_t K, int64_t N, int64_t* drafts, int32_t* hits, int32_t* hits_copy, int64_t B,
                                       void* stream) {
    TGIS_CHECK_ARG(all_input_ids && position_ids && drafts && hits && B >= 0 && tree_shape_ok(C, K) && K >= 1 && N >= 1 &&
                       N <= 4 && ld_all > 0 && ld_all < (1ll << 31),
                   "tgis_spec_propose_multi: bad arguments");
    if (B == 0) return TGIS_OK;
    hipLaunchKernelGGL(spec_propose_multi_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, all_input_ids, ld_all,
                       position_ids, (int)C, (int)K, (int)N, drafts, hits, hits_copy);
    TGIS_CHECK_LAUNCH();
    return TGIS_OK;
}
