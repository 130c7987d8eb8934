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
"""
import heapq
import json
import math
import os
from typing import Dict, List, Optional, Tuple, Union

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
