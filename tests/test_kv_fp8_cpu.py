"""CPU: the one-byte (e4m3) KV cache option — the quantiser restatement, PagedKVCache with kv_dtype "fp8_e4m3", the page
budget arithmetic and TGIS_KV_CACHE_DTYPE parsing."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8_ref as q8  # noqa: E402

from tgis_amd.utils import kv_cache  # noqa: E402
from tgis_amd.utils.kv_cache import PagedKVCache, pages_for_budget, parse_kv_cache_dtype  # noqa: E402


def test_quantiser_known_codes_and_saturation():
    x = torch.tensor([0.0, 1.0, -1.0, 448.0, -448.0, 449.0, 500.0, -1e4, 65504.0, 2.0 ** -9, 0.0625])
    codes = q8.quantize(x)
    assert codes.dtype == torch.uint8
    assert codes.tolist() == [0x00, 0x38, 0xB8, 0x7E, 0xFE, 0x7E, 0x7E, 0xFE, 0x7E, 0x01, 0x18]
    assert not ((codes == 0x7F) | (codes == 0xFF)).any(), "a NaN code"
    back = q8.dequantize(codes)
    assert back.tolist()[:5] == [0.0, 1.0, -1.0, 448.0, -448.0]
    assert torch.isfinite(back).all()


def test_quantiser_clamps_before_the_cast():
    # the reason for the clamp: torch's cast alone gives NaN past the largest finite e4m3 value
    assert torch.isnan(torch.tensor([500.0]).to(torch.float8_e4m3fn).float()).all()
    assert q8.quantize(torch.tensor([500.0])).item() == 0x7E


def test_quantiser_rounds_to_nearest_even_and_scales():
    # 1.0625 lies half-way between 1.0 (0x38) and 1.125 (0x39): ties to the even code; 1.1875 to 1.25 (0x3A)
    assert q8.quantize(torch.tensor([1.0625, 1.1875])).tolist() == [0x38, 0x3A]
    x = torch.tensor([3.0, -6.0], dtype=torch.float16)
    assert q8.dequantize(q8.quantize(x, 2.0), 2.0).tolist() == [3.0, -6.0]
    # every code but the two NaNs survives dequantise -> quantise, -0 (0x80) included
    codes = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=torch.uint8)
    assert torch.equal(q8.quantize(q8.dequantize(codes)), codes)
    # a scale that is not a power of two: x / s, correctly rounded, then the cast (not x times a rounded 1 / s)
    x = torch.tensor([1.0, -3.5, 300.0], dtype=torch.float16)
    assert torch.equal(q8.quantize(x, 0.7), (x.float() / 0.7).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8))


def test_paged_kv_cache_fp8_pool():
    c16 = PagedKVCache(3, 2, 64, 10, torch.float16, torch.device("cpu"))
    c8 = PagedKVCache(3, 2, 64, 10, torch.float16, torch.device("cpu"), kv_dtype="fp8_e4m3")
    assert c8.pool.shape == c16.pool.shape == (3, 2, 11, 2, 32 * 64)
    assert c8.pool.dtype == torch.uint8 and c16.pool.dtype == torch.float16
    assert not c8.pool.any(), "zero-initialised"
    assert c8.bytes_per_token() * 2 == c16.bytes_per_token() == 3 * 2 * 2 * 64 * 2
    assert c8.is_fp8 and not c16.is_fp8 and c16.kv_dtype == "auto"
    assert c8.scales(2) == (1.0, 1.0)
    assert c8.null_page == 10 and c8.k_pool(1).shape == (11, 2, 32 * 64)
    assert c8.alloc(3) == [0, 1, 2]


def test_one_byte_pool_gets_twice_the_pages():
    budget = 40 * 2 ** 30
    p16 = pages_for_budget(budget, 80, 8, 128, 2)
    p8 = pages_for_budget(budget, 80, 8, 128, 1)
    assert p16 == budget // (80 * 2 * 8 * 32 * 128 * 2)
    assert p8 in (2 * p16, 2 * p16 + 1)
    assert pages_for_budget(10, 1, 1, 64, 1) == 64  # the floor
    assert kv_cache.kv_bytes_per_page(2, 4, 64, 1) * 2 == kv_cache.kv_bytes_per_page(2, 4, 64, 2)


def test_kv_cache_dtype_parsing(monkeypatch):
    monkeypatch.delenv("TGIS_KV_CACHE_DTYPE", raising=False)
    assert parse_kv_cache_dtype() == "auto"
    assert parse_kv_cache_dtype("FP8_E4M3") == "fp8_e4m3"
    monkeypatch.setenv("TGIS_KV_CACHE_DTYPE", "fp8_e4m3")
    assert parse_kv_cache_dtype() == "fp8_e4m3"
    assert parse_kv_cache_dtype("auto") == "auto"  # the argument wins over the environment
    for bad in ("fp8", "e5m2", "int8", "fp8_e5m2", ""):
        monkeypatch.setenv("TGIS_KV_CACHE_DTYPE", bad)
        with pytest.raises(ValueError):
            parse_kv_cache_dtype()
    with pytest.raises(ValueError):
        PagedKVCache(1, 1, 64, 4, torch.float16, torch.device("cpu"), kv_dtype="fp16")


def test_flash_causal_lm_rejects_a_bad_kv_dtype_at_construction(monkeypatch):
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    monkeypatch.setenv("TGIS_KV_CACHE_DTYPE", "fp8_e5m2")
    with pytest.raises(ValueError, match="KV cache dtype"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=object())
    monkeypatch.delenv("TGIS_KV_CACHE_DTYPE")
    with pytest.raises(ValueError, match="KV cache dtype"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=object(), kv_cache_dtype="int8")
