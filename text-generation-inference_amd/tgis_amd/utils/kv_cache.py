"""Paged KV cache: one statically allocated page pool per model, 32-token pages, block tables per request.

This replaces the reference's per-batch contiguous `past_key_values[L, total_slots, 2, Hkv, D]` tensor that
is re-concatenated on every decode step, concatenate and prune (models/flash_causal_lm.py:246,281,
307-333,439-447): membership changes and growth become page-table edits, the KV bytes never move.
The *logical* slot index the reference exposes (`cu_seqlens[1:] - 1`, flash_llama_modeling.py:465) is kept
by FlashCausalLMBatch; `PagedKVCache` only maps (request, position) -> physical (page, offset).
Design cue for paging: models/paged_causal_lm.py:300-348 (block size 16 there; 32 here = one MFMA K=32 step).

Where a sequence's pages sit in the pool.  The decode attention's blocks walk their sequences' pages in step, so what the
chip reads at one instant is "page p of every sequence of the batch".  The pool hands out its LOWEST free ids and a batch deals
what it takes PAGE-MAJOR over its sequences (FlashCausalLMBatch.allocate_pages): on a pristine pool those rows are dense runs
(cfg3: 80.7 us per launch against 82.6 for a random order and 88-92 for a sequence's pages side by side,
profiles/r05_attn_page_order.log), and a finished sequence's column of ids is the next one out, so the request that replaces
it inherits it.  Round 6 measured what churn does to that (bench.py --churn, profiles/r06_churn_cfg3.json: requests leaving
and joining every 4-8 steps on a pool aged by random allocations and frees): decode p50 4.149 ms against 4.144 ms on the
pristine pool — lowest-id-first dealing over the holes of an aged pool is still mostly dense.  A channel-aware free list
(one heap per page-id residue class, page p of sequence b from class (b + p) mod C — VERDICT r05 item 2a) was built and
measured on aged pools for C = 2 .. 128 at five shapes: never better than this one, 1-4 % worse for several C
(profiles/r06_page_classes.log; the allocator lives on in tools/attn_page_order.py), so it is not here.

KV cache dtype (opt-in, `kv_dtype="fp8_e4m3"` / TGIS_KV_CACHE_DTYPE): the pool holds one byte per element, OCP float8_e4m3fn
codes of x / k_scale and x / v_scale (csrc/kv_layout.h) in a torch.uint8 tensor of the same shape — half the
bytes per page, so twice the pages for the same memory.  The scales are one float per layer for k and one for v (1.0 until a
calibrated checkpoint supplies others); the native calls take them with `kv_scales=cache.scales(layer)`.
"""
import heapq
import os
from typing import List, Optional, Tuple

import torch

PAGE = 32

# TGIS_KV_CACHE_DTYPE / kv_cache_dtype values: "auto" = the model dtype
KV_CACHE_DTYPES = ("auto", "fp8_e4m3")


def parse_kv_cache_dtype(value: Optional[str] = None) -> str:
    """The KV cache dtype name: `value`, or TGIS_KV_CACHE_DTYPE when it is None (unset: "auto").  Raises on anything else."""
    if value is None:
        value = os.getenv("TGIS_KV_CACHE_DTYPE", "auto")
    name = str(value).strip().lower()
    if name not in KV_CACHE_DTYPES:
        raise ValueError(f"KV cache dtype {value!r} is not supported (one of {', '.join(KV_CACHE_DTYPES)})")
    return name


def kv_pool_dtype(kv_dtype: str, model_dtype: torch.dtype) -> torch.dtype:
    """Element type of the pool tensor: the model dtype, or uint8 holding e4m3 codes."""
    return torch.uint8 if parse_kv_cache_dtype(kv_dtype) == "fp8_e4m3" else model_dtype


def kv_bytes_per_page(num_layers: int, num_kv_heads: int, head_dim: int, elem_bytes: int) -> int:
    """Bytes of one page across every layer, k and v."""
    return num_layers * 2 * num_kv_heads * PAGE * head_dim * elem_bytes


def pages_for_budget(budget_bytes: int, num_layers: int, num_kv_heads: int, head_dim: int, elem_bytes: int,
                     min_pages: int = 64) -> int:
    """How many pages a pool of `elem_bytes`-byte elements gets out of `budget_bytes` (at least `min_pages`)."""
    return max(min_pages, int(budget_bytes) // kv_bytes_per_page(num_layers, num_kv_heads, head_dim, elem_bytes))


class OutOfPages(RuntimeError):
    """Maps to gRPC RESOURCE_EXHAUSTED like a CUDA OOM does in the reference (server.py:48-51)."""


class PagedKVCache:
    def __init__(self, num_layers: int, num_kv_heads: int, head_dim: int, num_pages: int, dtype, device,
                 kv_dtype: str = "auto"):
        self.num_layers, self.num_kv_heads, self.head_dim = num_layers, num_kv_heads, head_dim
        self.num_pages = num_pages
        self.kv_dtype = parse_kv_cache_dtype(kv_dtype)
        dtype = kv_pool_dtype(self.kv_dtype, dtype)
        # per-layer dequantisation scales of a one-byte cache (k, v); 1.0: no calibration yet
        self.k_scales = [1.0] * num_layers
        self.v_scales = [1.0] * num_layers
        # zero-initialised, and every value a kernel ever writes into it is finite: masked slots of a page (the unwritten tail
        # of the page a sequence is filling, stale tokens of a page's previous owner) are multiplied by P = 0 and must never
        # hold NaN / Inf patterns (tests/test_ops_gpu.py::test_attention_decode_every_fill_of_the_last_page runs over stale
        # tails of +-65504).  One page more than `num_pages`: the NULL page (id num_pages), never handed out — the inactive
        # rows of a padded decode graph (FlashCausalLM, batch-size buckets) write their token there and attend to it.
        self.pool = torch.zeros((num_layers, 2, num_pages + 1, num_kv_heads, PAGE * head_dim), dtype=dtype, device=device)
        self.null_page = num_pages
        self._free = list(range(num_pages))  # a heap (heapq), trivially one to begin with

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def bytes_per_token(self) -> int:
        return self.num_layers * 2 * self.num_kv_heads * self.head_dim * self.pool.element_size()

    @property
    def is_fp8(self) -> bool:
        return self.kv_dtype == "fp8_e4m3"

    def scales(self, layer: int) -> Tuple[float, float]:
        """(k_scale, v_scale) of a layer: a one-byte pool holds e4m3(k / k_scale), e4m3(v / v_scale)."""
        return self.k_scales[layer], self.v_scales[layer]

    def k_pool(self, layer: int) -> torch.Tensor:
        return self.pool[layer, 0]

    def v_pool(self, layer: int) -> torch.Tensor:
        return self.pool[layer, 1]

    def alloc(self, n: int) -> List[int]:
        """The n lowest free page ids, ascending.  All or nothing: OutOfPages before anything is taken."""
        if n > len(self._free):
            raise OutOfPages(f"KV cache exhausted: need {n} pages, {len(self._free)} free of {self.num_pages}")
        return [heapq.heappop(self._free) for _ in range(n)]

    def free(self, pages: List[int]):
        for p in pages:
            heapq.heappush(self._free, p)

    @staticmethod
    def pages_for(tokens: int) -> int:
        return (tokens + PAGE - 1) // PAGE
