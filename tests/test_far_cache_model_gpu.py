"""-m gpu: a model whose requests live on KV pages past 2^31 elements of every layer pool.

The dense tiny Llama (L 2, Hkv 2, D 64) with the one-byte cache and 524288 + 64 pages: a page is 4096 elements per layer
pool, so pages from 524288 on lie past 2^31, and the null page (id num_pages, where the inactive rows of a padded decode graph
write and attend) is the farthest of all.  The low 524288 pages are taken before the batch, so every page the requests get is
a far one.  Ids and logits must equal, bit for bit, those of the same model on a 96-page cache, and the held pages stay zero."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kv_fp8_model_gpu as fp8model  # noqa: E402

pytestmark = pytest.mark.gpu

GIB = 1 << 30
HELD = 524288
PAGES = HELD + 64
LENS = [5, 37, 16]
STEPS = 12


@pytest.fixture(scope="module", autouse=True)
def _enough_memory(gpu_device):
    need = 2 * 2 * (PAGES + 1) * 2 * 32 * 64 + GIB // 4  # the pool [L, 2, pages + 1, Hkv, 32 D] bytes, and the model
    free = torch.cuda.mem_get_info(gpu_device)[0]
    if free < need + GIB:
        pytest.skip(f"{free} bytes of device memory are free, this module needs {need} and 1 GiB to spare")


def test_requests_on_pages_past_2_31_elements_equal_a_small_cache(gpu_device):
    from tgis_amd.models import flash_causal_lm as fcl

    assert fcl.graph_bucket(len(LENS)) > len(LENS), "the batch-size bucket has an inactive row on the null page"
    small, tok, _, _ = fp8model._llama(None, torch.float16, "fp8_e4m3", pages=96)
    want, _, want_logits = fp8model._run(small, tok, LENS, STEPS)
    assert {k[0] for k in small._graphs} == {fcl.graph_bucket(len(LENS))}
    del small
    lm, tok, tcfg, _ = fp8model._llama(None, torch.float16, "fp8_e4m3", pages=PAGES)
    cache = lm.kv_cache
    S = cache.num_kv_heads * 32 * cache.head_dim
    assert (tcfg.num_hidden_layers, cache.num_kv_heads, cache.head_dim) == (2, 2, 64) and cache.pool.dtype == torch.uint8
    assert HELD * S == 1 << 31 and cache.null_page == PAGES and cache.null_page * S > 1 << 31
    held = cache.alloc(HELD)
    assert held[0] == 0 and held[-1] == HELD - 1 and cache.free_pages == PAGES - HELD
    got, _, logits = fp8model._run(lm, tok, LENS, STEPS)
    assert {k[0] for k in lm._graphs} == {fcl.graph_bucket(len(LENS))}, "the decode steps ran on the padded graph"
    assert got == want, "ids or logprobs differ from the 96-page cache"
    assert len(logits) == len(want_logits) == STEPS + 1
    for i, (a, b) in enumerate(zip(logits, want_logits)):
        assert np.array_equal(a, b), f"step {i}: logits differ from the 96-page cache"
    torch.cuda.synchronize()
    for layer in range(2):
        for kv in range(2):
            assert not cache.pool[layer, kv, :HELD].any(), f"layer {layer} {'kv'[kv]}: a held page below 2^31 was written"
            assert cache.pool[layer, kv, HELD:].any(), f"layer {layer} {'kv'[kv]}: nothing was written past 2^31"
    cache.free(held)
