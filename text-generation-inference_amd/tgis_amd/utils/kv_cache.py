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
bytes per page, so twice the pages for the same memory.  The scales are one float per layer for k and one for v; the native
calls take them with `kv_scales=cache.scales(layer)`.

Calibration of those scales.  A model running its ordinary 16-bit cache measures max |k| and max |v| per layer
over the tokens of calibration prompts (FlashCausalLM.calibrate_kv_scales, the tgis_kv_absmax kernel reading the pages); the
scale of a layer is the smallest power of two s with headroom * absmax / s <= 448 (`scale_from_absmax`): a power of two makes
x / s exact, so e4m3's own rounding is the only one, and it survives JSON; the headroom (2.0, a design constant, not a
measurement) leaves a factor for activations larger than any the prompts produced, and costs nothing, e4m3's relative
precision being flat over its normals.  The result is the file `kv_cache_scales.json` (`save_kv_scales` / `load_kv_scales`)
that FlashCausalLM looks for (`resolve_kv_scales`: its `kv_scales` argument, TGIS_KV_SCALES, the weights' directory) and
applies with `PagedKVCache.set_scales` before any page is written or any graph captured.  Without one the scales stay 1.0.

KV prefix reuse (opt-in, `prefix_reuse=True` / TGIS_KV_PREFIX_REUSE; not the reference's prompt-tuning
`prefix_cache`).  A full page of PROMPT tokens is never rewritten once the prefill has passed it: its owner only writes at
positions >= its prompt length.  Such pages are indexed by content, key (serial of the entry of the page in front of it, the
page's 32 token ids) — a chain, so equal keys mean equal whole prefixes, compared as tuples: no hashes to collide.  Serials
are never reused, so a page whose parent was evicted can never match again.  Pages carry a reference count: 1 from `alloc`,
+1 for every request that maps them through `match`, -1 per `free`.  At 0 an indexed page keeps its contents and waits in
an LRU; `alloc` takes heap pages first and then evicts from it, oldest first.  `free_pages` counts both.  Everything is
host-side and deterministic in the request stream, so tensor-parallel ranks, which see the same stream and hold the same
number of pages, stay in step without talking.
"""
import heapq
import json
import math
import os
from collections import OrderedDict
from typing import Dict, List, Optional, Sequence, Tuple, Union

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


def agree_kv_cache_dtype(group, value: Optional[str] = None) -> str:
    """`parse_kv_cache_dtype(value)`, the same on every rank of `group` (utils/rank_group.py).  Every rank reads and writes its
    shard of the same layers' pages with the same kernels: a rank whose environment asked for another cache dtype is a
    configuration error, raised on every rank rather than served — and a rank whose value does not parse tells its peers
    first, so that they fail with it instead of waiting in a collective."""
    try:
        name, error = parse_kv_cache_dtype(value), None
    except ValueError as e:
        name, error = None, e
    group.fail_together(error, "another tensor-parallel rank was given an unsupported KV cache dtype (TGIS_KV_CACHE_DTYPE)")
    code = KV_CACHE_DTYPES.index(name)
    lo, hi = group.min_int(code), group.max_int(code)
    if lo != hi:
        raise ValueError(f"tensor-parallel ranks disagree on the KV cache dtype (this rank: {name}; "
                         f"ranks use {KV_CACHE_DTYPES[lo]} and {KV_CACHE_DTYPES[hi]}): set TGIS_KV_CACHE_DTYPE alike "
                         f"on every rank")
    return name


def parse_kv_prefix_reuse(value: Union[None, bool, str] = None) -> bool:
    """Whether full prompt pages are shared between requests: `value`, or TGIS_KV_PREFIX_REUSE when it is None (unset:
    false).  A bool, "true" or "false"; anything else raises."""
    if value is None:
        value = os.getenv("TGIS_KV_PREFIX_REUSE", "false")
    if isinstance(value, bool):
        return value
    name = str(value).strip().lower()
    if name not in ("true", "false"):
        raise ValueError(f"KV prefix reuse {value!r} is not supported (true or false)")
    return name == "true"


def agree_kv_prefix_reuse(group, value: Union[None, bool, str] = None) -> bool:
    """`parse_kv_prefix_reuse(value)`, the same on every rank of `group` (utils/rank_group.py), like agree_kv_cache_dtype:
    ranks that disagreed would map different pages for the same request and write different block tables."""
    try:
        flag, error = parse_kv_prefix_reuse(value), None
    except ValueError as e:
        flag, error = False, e
    group.fail_together(error, "another tensor-parallel rank was given an unsupported KV prefix reuse setting "
                               "(TGIS_KV_PREFIX_REUSE)")
    if group.min_int(int(flag)) != group.max_int(int(flag)):
        raise ValueError(f"tensor-parallel ranks disagree on KV prefix reuse (this rank: {str(flag).lower()}): set "
                         f"TGIS_KV_PREFIX_REUSE alike on every rank")
    return flag


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


REUSE_STATS = ("lookups", "hit_pages", "looked_up_pages", "registered", "evictions")


class OutOfPages(RuntimeError):
    """Maps to gRPC RESOURCE_EXHAUSTED like a CUDA OOM does in the reference (server.py:48-51)."""


class PagedKVCache:
    def __init__(self, num_layers: int, num_kv_heads: int, head_dim: int, num_pages: int, dtype, device,
                 kv_dtype: str = "auto", prefix_reuse: bool = False):
        self.num_layers, self.num_kv_heads, self.head_dim = num_layers, num_kv_heads, head_dim
        self.num_pages = num_pages
        self.kv_dtype = parse_kv_cache_dtype(kv_dtype)
        dtype = kv_pool_dtype(self.kv_dtype, dtype)
        # per-layer dequantisation scales of a one-byte cache (k, v); 1.0 unless calibrated ones are set (set_scales)
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
        # KV prefix reuse (module docstring); none of this is looked at when it is off
        self.prefix_reuse = bool(prefix_reuse)
        self._refs: Dict[int, int] = {}  # handed-out page -> holders
        self._index: Dict[Tuple[int, Tuple[int, ...]], Tuple[int, int]] = {}  # (parent serial, tokens) -> (page, serial)
        self._entry: Dict[int, Tuple[Tuple[int, Tuple[int, ...]], int]] = {}  # indexed page -> (its key, its serial)
        self._lru: "OrderedDict[int, None]" = OrderedDict()  # indexed pages nobody holds, oldest first
        self._serial = 0
        self._stats = dict.fromkeys(REUSE_STATS, 0)

    @property
    def free_pages(self) -> int:
        return len(self._free) + len(self._lru)

    def bytes_per_token(self) -> int:
        return self.num_layers * 2 * self.num_kv_heads * self.head_dim * self.pool.element_size()

    @property
    def is_fp8(self) -> bool:
        return self.kv_dtype == "fp8_e4m3"

    def scales(self, layer: int) -> Tuple[float, float]:
        """(k_scale, v_scale) of a layer: a one-byte pool holds e4m3(k / k_scale), e4m3(v / v_scale)."""
        return self.k_scales[layer], self.v_scales[layer]

    def set_scales(self, k_scales, v_scales) -> None:
        """Calibrated per-layer scales of a one-byte pool: two lists of `num_layers` finite positive floats (ValueError
        otherwise, or on a 16-bit pool).  Only while no page is handed out: written pages hold codes of the old scales, and
        captured decode graphs bake the scales in as launch arguments."""
        if not self.is_fp8:
            raise ValueError("KV cache scales apply to the one-byte cache only (kv_cache_dtype='fp8_e4m3')")
        if self.free_pages != self.num_pages:
            raise ValueError("KV cache scales cannot change while pages are handed out")
        k, v = _checked_scales(k_scales, self.num_layers, "k_scales"), _checked_scales(v_scales, self.num_layers, "v_scales")
        self.k_scales, self.v_scales = k, v
        # cached pages hold codes of the old scales: forget them
        for p in self._lru:
            heapq.heappush(self._free, p)
        self._lru.clear()
        self._index.clear()
        self._entry.clear()

    def k_pool(self, layer: int) -> torch.Tensor:
        return self.pool[layer, 0]

    def v_pool(self, layer: int) -> torch.Tensor:
        return self.pool[layer, 1]

    def alloc(self, n: int) -> List[int]:
        """The n lowest free page ids, ascending.  All or nothing: OutOfPages before anything is taken.
        With prefix reuse: heap pages first, then the least recently used cached pages, whose index entries go."""
        if not self.prefix_reuse:
            if n > len(self._free):
                raise OutOfPages(f"KV cache exhausted: need {n} pages, {len(self._free)} free of {self.num_pages}")
            return [heapq.heappop(self._free) for _ in range(n)]
        if n > self.free_pages:
            raise OutOfPages(f"KV cache exhausted: need {n} pages, {self.free_pages} free of {self.num_pages} "
                             f"({len(self._lru)} of them cached)")
        pages = [heapq.heappop(self._free) for _ in range(min(n, len(self._free)))]
        while len(pages) < n:
            p, _ = self._lru.popitem(last=False)
            del self._index[self._entry.pop(p)[0]]
            self._stats["evictions"] += 1
            pages.append(p)
        for p in pages:
            self._refs[p] = 1
        return pages

    def free(self, pages: List[int]):
        """Gives up one hold on each page.  With prefix reuse a page goes on only when its last holder lets go: back to the
        heap, or, indexed, to the young end of the LRU with its contents kept — the pages of one call deepest first, so
        that a chain is evicted from its tail and no page outlives the parent it can only be found through."""
        if not self.prefix_reuse:
            for p in pages:
                heapq.heappush(self._free, p)
            return
        for p in reversed(pages):
            self._refs[p] -= 1
            if self._refs[p] == 0:
                del self._refs[p]
                if p in self._entry:
                    self._lru[p] = None
                else:
                    heapq.heappush(self._free, p)

    # ---- KV prefix reuse ------------------------------------------------------------------------------------------------------
    def match(self, token_ids: Sequence[int]) -> List[int]:
        """The longest chain of indexed pages that holds a prefix of the prompt `token_ids`, at most (len - 1) // 32 of them:
        one prompt token at least is always computed, its logits choose the first generated token.  Every page returned is
        pinned (one more holder, out of the LRU): the caller keeps it or gives it back with `free`."""
        if not self.prefix_reuse:
            return []
        cap = max(len(token_ids) - 1, 0) // PAGE
        self._stats["lookups"] += 1
        self._stats["looked_up_pages"] += cap
        pages, parent = [], 0
        for i in range(cap):
            hit = self._index.get((parent, tuple(token_ids[i * PAGE:(i + 1) * PAGE])))
            if hit is None:
                break
            page, parent = hit
            self._lru.pop(page, None)
            self._refs[page] = self._refs.get(page, 0) + 1
            pages.append(page)
        self._stats["hit_pages"] += len(pages)
        return pages

    def register(self, pages: Sequence[int], token_ids: Sequence[int]) -> None:
        """After a prefill has written them: indexes every full page of the prompt (page p < len // 32 of the request's page
        list `pages`) that is not indexed yet, chained to the page in front of it.  Where the same content is indexed
        already on another page, that entry stays, this page stays private and the chain goes on from the entry."""
        if not self.prefix_reuse:
            return
        parent = 0
        for i in range(len(token_ids) // PAGE):
            page = pages[i]
            if page in self._entry:
                parent = self._entry[page][1]
                continue
            key = (parent, tuple(token_ids[i * PAGE:(i + 1) * PAGE]))
            if key in self._index:
                parent = self._index[key][1]
                continue
            self._serial += 1
            self._index[key] = (page, self._serial)
            self._entry[page] = (key, self._serial)
            self._stats["registered"] += 1
            parent = self._serial

    def reuse_stats(self) -> Dict[str, int]:
        """Counters since construction: `lookups` (match calls), `looked_up_pages` (pages they could have hit), `hit_pages`,
        `registered` (index entries made), `evictions` (entries dropped for their page).  All zero with reuse off."""
        return dict(self._stats)

    @staticmethod
    def pages_for(tokens: int) -> int:
        return (tokens + PAGE - 1) // PAGE


# ---- calibrated scales of the one-byte cache ----------------------------------------------------------------------------------
E4M3_MAX = 448.0
KV_SCALES_FORMAT = "tgis-kv-scales-1"
KV_SCALES_FILE = "kv_cache_scales.json"
KV_SCALES_HEADROOM = 2.0  # a design constant, not a measurement (module docstring)


def _checked_scales(values, num_layers: int, what: str) -> List[float]:
    if not isinstance(values, (list, tuple)) or len(values) != num_layers:
        raise ValueError(f"{what}: expected a list of {num_layers} floats (one per layer)")
    out = []
    for s in values:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s <= 0:
            raise ValueError(f"{what}: {s!r} is not a finite positive float")
        out.append(float(s))
    return out


def scale_from_absmax(absmax: float, headroom: float = KV_SCALES_HEADROOM) -> float:
    """The smallest power of two s with headroom * absmax / s <= 448 (then > 224); 1.0 for absmax == 0."""
    absmax, headroom = float(absmax), float(headroom)
    if not math.isfinite(absmax) or absmax < 0:
        raise ValueError(f"absmax {absmax!r} is not a finite non-negative number")
    if not math.isfinite(headroom) or headroom <= 0:
        raise ValueError(f"headroom {headroom!r} is not a finite positive number")
    if absmax == 0:
        return 1.0
    x = headroom * absmax
    s = math.ldexp(1.0, math.frexp(x / E4M3_MAX)[1])  # within one step of the answer; x / s is exact from here on
    while x / s > E4M3_MAX:
        s *= 2.0
    while s > 2.0 ** -126 and x / (s / 2.0) <= E4M3_MAX:  # the kernels take the scale as a (normal) float: no smaller
        s /= 2.0
    return max(s, 2.0 ** -126)


def kv_scales_stats(k_absmax: List[float], v_absmax: List[float], tokens: int, model_dtype: str,
                    headroom: float = KV_SCALES_HEADROOM) -> Dict:
    """The contents of a scale file from the measured per-layer absmax values."""
    if len(k_absmax) != len(v_absmax):
        raise ValueError("k_absmax and v_absmax differ in length")
    return {
        "format": KV_SCALES_FORMAT, "kv_cache_dtype": "fp8_e4m3", "num_layers": len(k_absmax),
        "k_absmax": [float(a) for a in k_absmax], "v_absmax": [float(a) for a in v_absmax],
        "k_scale": [scale_from_absmax(a, headroom) for a in k_absmax],
        "v_scale": [scale_from_absmax(a, headroom) for a in v_absmax],
        "headroom": float(headroom), "tokens": int(tokens), "model_dtype": str(model_dtype),
    }


def check_kv_scales(stats, num_layers: int) -> Tuple[List[float], List[float]]:
    """(k_scale, v_scale) of a scale file's contents; ValueError on an unknown format, another layer count, wrong lengths or
    a scale that is not finite and positive."""
    if not isinstance(stats, dict) or stats.get("format") != KV_SCALES_FORMAT:
        got = stats.get("format") if isinstance(stats, dict) else type(stats).__name__
        raise ValueError(f"KV cache scales: unknown format {got!r} (expected {KV_SCALES_FORMAT!r})")
    if stats.get("kv_cache_dtype", "fp8_e4m3") != "fp8_e4m3":
        raise ValueError(f"KV cache scales: made for kv_cache_dtype {stats['kv_cache_dtype']!r}, not 'fp8_e4m3'")
    if stats.get("num_layers") != num_layers:
        raise ValueError(f"KV cache scales: made for {stats.get('num_layers')!r} layers, the model has {num_layers}")
    return (_checked_scales(stats.get("k_scale"), num_layers, "KV cache scales: k_scale"),
            _checked_scales(stats.get("v_scale"), num_layers, "KV cache scales: v_scale"))


def save_kv_scales(stats: Dict, path: str) -> None:
    check_kv_scales(stats, stats.get("num_layers"))
    with open(path, "w") as f:
        json.dump(stats, f, indent=1)
        f.write("\n")


def load_kv_scales(path: str, num_layers: int) -> Dict:
    with open(path) as f:
        try:
            stats = json.load(f)
        except ValueError as e:
            raise ValueError(f"KV cache scales: {path} is not JSON ({e})") from None
    check_kv_scales(stats, num_layers)
    return stats


def resolve_kv_scales(kv_scales: Union[None, str, Dict], kv_dtype: str, num_layers: int, model_dir: Optional[str] = None,
                      env: Optional[Dict[str, str]] = None) -> Optional[Tuple[List[float], List[float]]]:
    """Which scales a model's cache gets, (k_scale, v_scale) or None for "stay at 1.0": the explicit `kv_scales` (the
    contents of a scale file, or its path); else the file TGIS_KV_SCALES names; else kv_cache_scales.json in `model_dir`
    (where the weights came from) if there is one.  A 16-bit cache has no scales: an explicit argument is then a ValueError,
    the environment variable and a discovered file are ignored.  Needs no GPU."""
    fp8 = parse_kv_cache_dtype(kv_dtype) == "fp8_e4m3"
    if kv_scales is not None:
        if not fp8:
            raise ValueError("kv_scales was given, but the KV cache is 16-bit (kv_cache_dtype='fp8_e4m3' takes scales)")
        if isinstance(kv_scales, dict):
            return check_kv_scales(kv_scales, num_layers)
        if isinstance(kv_scales, (str, os.PathLike)):
            return check_kv_scales(load_kv_scales(os.fspath(kv_scales), num_layers), num_layers)
        raise ValueError(f"kv_scales: expected a path or a dict, not {type(kv_scales).__name__}")
    if not fp8:
        return None
    path = (os.environ if env is None else env).get("TGIS_KV_SCALES")
    if not path and model_dir and os.path.isfile(os.path.join(model_dir, KV_SCALES_FILE)):
        path = os.path.join(model_dir, KV_SCALES_FILE)
    if not path:
        return None
    return check_kv_scales(load_kv_scales(path, num_layers), num_layers)


def agree_kv_scales(group, kv_scales: Union[None, str, Dict], kv_dtype: str, num_layers: int,
                    model_dir: Optional[str] = None) -> Optional[Tuple[List[float], List[float]]]:
    """`resolve_kv_scales`, the same on every rank of `group` (utils/rank_group.py): rank 0 resolves and every rank gets rank
    0's values.  A rank that fails (an unreadable file on rank 0, an explicit argument with a 16-bit cache anywhere) tells
    its peers first, so that all of them raise instead of one waiting."""
    found, error = None, None
    try:
        if group.rank == 0 or not group.real:
            found = resolve_kv_scales(kv_scales, kv_dtype, num_layers, model_dir)
        elif kv_scales is not None and parse_kv_cache_dtype(kv_dtype) != "fp8_e4m3":
            resolve_kv_scales(kv_scales, kv_dtype, num_layers)  # raises: explicit scales, 16-bit cache
    except (ValueError, OSError) as e:
        error = e
    flat = group.broadcast_from_rank0(None if found is None else found[0] + found[1], 2 * num_layers)
    group.fail_together(error, "another tensor-parallel rank could not resolve the KV cache scales")
    return None if flat is None else (flat[:num_layers], flat[num_layers:])
