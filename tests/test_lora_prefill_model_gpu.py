"""-m gpu: prefills of more than 64 rows under LoRA adapters take tgis_lora_shrink_tiles / tgis_lora_expand_tiles, end to end on
the Llama flash path: the fixture, bar and helpers of tests/test_lora_model_gpu.py (transformers' fp32 CPU model on merged
weights, tests/golden/llama_lora.npz), with torch.addmm set to raise so that no delta can come from a library GEMM."""
import numpy as np
import pytest
import torch

from tests import lora_tiny
from tests.test_lora_model_gpu import LOGIT_TOL, _build, _check, _fixture, _run, store  # noqa: F401  (store: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_library_gemm(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("torch.addmm under a LoRA prefill: the delta left the HIP kernels")

    monkeypatch.setattr(torch, "addmm", refuse)


def _tile_launches(monkeypatch):
    """Counts the calls of the tile path's expand."""
    from tgis_amd import native

    calls, orig = [], native.lora_expand_tiles
    monkeypatch.setattr(native, "lora_expand_tiles", lambda v, w, tiles, y: calls.append(tiles.n) or orig(v, w, tiles, y))
    return calls


def test_long_prompt_takes_the_tile_kernels(gpu_device, store, monkeypatch):  # noqa: F811
    """100 prompt tokens under the all-module adapter: tiles of 64 + 36 rows in all four linears of both layers."""
    meta, z = _fixture()
    calls = _tile_launches(monkeypatch)
    lm, tok = _build(meta, store)
    got = _run(lm, tok, [meta["long_prompt"]], [meta["long_adapter"]], meta["long_new"], max_new=meta["long_new"])
    _check(got, z["long_ids"][None], z["long_logits"][None], "long prompt")
    assert calls == [2] * (4 * lora_tiny.TinyLlamaConfig().num_hidden_layers)


def test_mixed_batch_prefill_takes_the_tile_kernels(gpu_device, store, monkeypatch):  # noqa: F811
    """The fixture's four requests as one batch of 70 prompt rows (5 without an adapter, then 20, 33 and 12 on three slots):
    one tile per request that carries an adapter."""
    meta, z = _fixture()
    calls = _tile_launches(monkeypatch)
    lm, tok = _build(meta, store)
    got = _run(lm, tok, meta["prompts"], meta["adapters"], 2)
    _check(got, z["ids"], z["logits"], "mixed batch")
    assert calls and set(calls) == {3}


def test_long_prompt_over_the_int4_base(gpu_device, store):  # noqa: F811
    """The 100-token prompt on the tiny GPTQ Llama, against the project's fp32 oracle on the dequantised weights with the
    adapter merged in (as tests/test_lora_model_gpu.py does for its short prompts), fed the model's own ids."""
    from oracle.llama_ref import LlamaRef

    meta, _z = _fixture()
    cfg = lora_tiny.TinyLlamaConfig()
    lm, tok = _build(meta, store, quantize="gptq")
    got = _run(lm, tok, [meta["long_prompt"]], [meta["long_adapter"]], 2, max_new=2)
    tensors = lora_tiny.tiny_llama_tensors(cfg, meta["seed"], quantize="gptq", groupsize=lora_tiny.GROUPSIZE)
    ref = LlamaRef(cfg, lora_tiny.merged_state_dict(cfg, tensors, meta["long_adapter"], meta["seed"]))
    want = ref.generate_greedy([meta["long_prompt"]], len(got), forced=[[g[0][0]] for g in got])
    for i, ((ids, logits), w) in enumerate(zip(got, want)):
        wl = w["logits"].numpy()[0]
        err = float(np.abs(logits[0] - wl).max())
        assert err <= LOGIT_TOL, f"step {i}: max |logit - merged oracle| = {err:.3f} > {LOGIT_TOL}"
        top2 = np.sort(wl)[-2:]
        if top2[1] - top2[0] > 2 * LOGIT_TOL:
            assert ids[0] == int(wl.argmax())
    base = LlamaRef(cfg, lora_tiny.merged_state_dict(cfg, tensors, None, meta["seed"]))
    b0 = base.generate_greedy([meta["long_prompt"]], 1)[0]["logits"].numpy()[0]
    assert float(np.abs(got[0][1][0] - b0).max()) > LOGIT_TOL  # the adapter matters: the base model is far from this row
