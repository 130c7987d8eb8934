"""-m gpu: a GPTQ GPT-BigCode checkpoint directory (safetensors + config.json + quantize_config.json) through
get_model(..., quantize="gptq") and the safetensors `Weights`, against the in-memory engine on the same tensors."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigcode_gptq_ref as bref  # noqa: E402
from fixture_utils import FixtureTokenizer, prompt_text  # noqa: E402
from test_checkpoint_gpu import _write_checkpoint  # noqa: E402

from oracle.tiny_models import TinyBigCodeConfig  # noqa: E402

pytestmark = pytest.mark.gpu
NEW = 4


def _write(path, cfg, tensors):
    _write_checkpoint(path, cfg, tensors, "gptq", bref.GS)  # the tokenizer files, the tensors, quantize_config.json
    conf = {"model_type": "gpt_bigcode", "architectures": ["GPTBigCodeForCausalLM"], "torch_dtype": "float16",
            "vocab_size": cfg.vocab_size, "n_embd": cfg.hidden_size, "n_inner": cfg.n_inner, "n_layer": cfg.num_hidden_layers,
            "n_head": cfg.num_attention_heads, "n_positions": cfg.n_positions, "multi_query": True,
            "layer_norm_epsilon": cfg.layer_norm_epsilon, "activation_function": cfg.activation_function,
            "pad_token_id": 0, "bos_token_id": 1, "eos_token_id": 2, "tie_word_embeddings": True}
    (path / "config.json").write_text(json.dumps(conf))


def _generate(lm, tok, prompts):
    from tgis_amd.pb import generate_pb2 as pb2

    reqs = [pb2.Request(id=i, inputs=prompt_text(p), input_length=len(p), truncate=True, max_output_length=NEW + 2)
            for i, p in enumerate(prompts)]
    with lm.context_manager():
        batch, errs = lm.batch_type.from_pb(pb2.Batch(id=0, requests=reqs), tok, lm.dtype, lm.device, lm.word_embeddings,
                                            None, True)
        assert not errs
        ids = []
        for i in range(NEW):
            toks, _, errs, _ = lm.generate_token(batch, first=(i == 0))
            assert not errs
            ids.append([t.token_id for t in toks])
    batch.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    return ids


def test_checkpoint_directory_equals_the_in_memory_engine(gpu_device, tmp_path, monkeypatch):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models import get_model
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.utils.layers import Ex4bitLinearV2

    monkeypatch.setenv("TGIS_KV_CACHE_FRACTION", "0.01")  # the default pool (85 % of the free memory) is not the subject
    cfg = TinyBigCodeConfig()
    tensors = bref.tiny_bigcode_gptq_tensors(cfg, 5)
    _write(tmp_path, cfg, tensors)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(3, cfg.vocab_size, size=n).tolist() for n in (9, 33, 2)]

    lm = get_model(str(tmp_path), None, "tgis_native", "float16", "gptq", max_sequence_length=256)
    blk = lm.model.transformer.h[0]
    for lin in (blk.attn.c_attn.linear, blk.attn.c_proj.linear, blk.mlp.c_fc.linear, blk.mlp.c_proj.linear):
        assert type(lin) is Ex4bitLinearV2 and lin.q_handle is not None
    from_files = _generate(lm, lm.tokenizer, prompts)

    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, TinyBigCodeConfig(), torch.float16, "gptq", tokenizer=tok,
                          gptq_groupsize=bref.GS)
    mem = FlashCausalLM("synthetic", None, "synthetic", torch.float16, "gptq", engine=eng, kv_cache_pages=64)
    assert from_files == _generate(mem, tok, prompts)


def test_gptq_directory_without_quantize_fails_in_the_loader(gpu_device, tmp_path, monkeypatch):
    """quantize=None on a directory that holds no dense weights: the loader's own error (a missing tensor), not a crash."""
    from tgis_amd.models import get_model

    monkeypatch.setenv("TGIS_KV_CACHE_FRACTION", "0.01")
    cfg = TinyBigCodeConfig()
    _write(tmp_path, cfg, bref.tiny_bigcode_gptq_tensors(cfg, 5))
    with pytest.raises(RuntimeError, match=r"weight transformer\.h\.0\.attn\.\w+\.weight does not exist"):
        get_model(str(tmp_path), None, "tgis_native", "float16", None, max_sequence_length=256)
