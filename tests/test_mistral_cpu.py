"""Mistral on the flash path, the parts that need no GPU: dispatch, `head_dim` and the bias defaults through the loader (kernels
replaced by the oracle through tests/cpu_backend.py) against the head_dim fixture of tests/golden/mistral_window.npz, what a
sliding window refuses, and where the window is put on the KVArgs."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import cpu_backend
from tests.fixture_utils import GOLDEN, FixtureTokenizer, prompt_text
from tests.mistral_tiny import TinyMistralConfig, tiny_mistral_tensors

CPU = torch.device("cpu")


def _fixture():
    z = np.load(os.path.join(GOLDEN, "mistral_window.npz"))
    return json.loads(bytes(z["meta"]).decode()), z


def _config(cfg):
    """What the engine hands the model class for a Mistral config.json: no attention_bias, no mlp_bias."""
    ns = types.SimpleNamespace(model_type="mistral", quantize=None, **cfg.to_dict())
    assert not hasattr(ns, "attention_bias") and not hasattr(ns, "mlp_bias")
    return ns


def _model(cfg, seed):
    from tgis_amd.inference_engine.tgis_native import model_class_for
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.weights import DictWeights

    config = _config(cfg)
    cls, aliases = model_class_for(config)
    assert aliases is None
    return cls(config, DictWeights(tiny_mistral_tensors(cfg, seed), CPU, torch.float16, FakeGroup(0, 1)))


def _lm(monkeypatch, cfg, seed, window):
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.utils.kv_cache import PagedKVCache

    cpu_backend.install(monkeypatch)
    model = _model(cfg, seed)
    attn = model.model.layers[0].self_attn
    lm = FlashCausalLM.__new__(FlashCausalLM)  # the prefill's host code without the GPU-only constructor
    lm.model, lm.device, lm.kv_prefix_reuse = model, CPU, False
    lm.num_heads, lm.num_kv_heads = attn.num_heads, attn.num_key_value_heads
    lm.kv_cache = PagedKVCache(cfg.num_hidden_layers, attn.num_key_value_heads, attn.head_size, 16, torch.float16, CPU)
    if window is not None:
        lm.sliding_window = window
    return lm


def _batch(prompts):
    from tgis_amd.models.flash_causal_lm import FlashCausalLMBatch
    from tgis_amd.pb import generate_pb2 as pb2

    reqs = [pb2.Request(id=i, inputs=prompt_text(p), input_length=len(p), max_output_length=4) for i, p in enumerate(prompts)]
    b, errs = FlashCausalLMBatch.from_pb(pb2.Batch(id=0, requests=reqs), FixtureTokenizer(256), torch.float16, CPU, None, None,
                                         True)
    assert not errs
    return b


def test_dispatch_lists_include_mistral():
    from tgis_amd.inference_engine.tgis_native import FLASH_TYPES, model_class_for
    from tgis_amd.models import FLASH_MODEL_TYPES, _flash_supports
    from tgis_amd.models.custom_modeling.flash_llama_modeling import FlashLlamaForCausalLM

    assert "mistral" in FLASH_MODEL_TYPES and "mistral" in FLASH_TYPES and _flash_supports("mistral", {})
    cls, aliases = model_class_for(_config(TinyMistralConfig()))
    assert cls is FlashLlamaForCausalLM and aliases is None
    tied = _config(TinyMistralConfig())
    tied.tie_word_embeddings = True
    assert model_class_for(tied)[1] == {"lm_head.weight": ["model.embed_tokens.weight"]}


def test_head_dim_and_bias_defaults_through_the_loader(monkeypatch):
    """head_dim 32 on hidden 256 / 4 heads: head size 32 (not 64), o_proj takes H * head_dim = 128 inputs, no bias is looked
    for, and the prefill's logits are the fixture's within the f16 logit bound of the GPU tests."""
    from tgis_amd.models.custom_modeling.flash_common import KVArgs

    meta, z = _fixture()
    cfg = TinyMistralConfig(**{k: meta["headdim_config"][k] for k in ("sliding_window", "head_dim")})
    assert cfg.head_dim == 32 != cfg.hidden_size // cfg.num_attention_heads
    lm = _lm(monkeypatch, cfg, meta["headdim_seed"], cfg.sliding_window)
    attn = lm.model.model.layers[0].self_attn
    assert attn.head_size == 32 and lm.model.model.head_size == 32 and attn.softmax_scale == 32 ** -0.5
    assert attn.o_proj.linear.bias is None and attn.query_key_value.linear.bias is None
    assert lm.model.model.layers[0].mlp.down_proj.linear.bias is None
    assert lm.kv_cache.k_pool(0).shape[-1] == 32 * 32
    prompt = meta["headdim_prompt"]
    batch = _batch([prompt])
    lm._need_all_logits = True
    batch.allocate_pages(lm.kv_cache)
    seen = []
    forward = lm.model.forward
    lm.model.forward = lambda *a, **k: (seen.append(a[5]), forward(*a, **k))[1]
    logits = lm._prefill_fresh_forward(batch)[0]
    assert isinstance(seen[0], KVArgs) and seen[0].window == 40 and seen[0].max_ctx == len(prompt)
    err = float(np.abs(logits.float().numpy() - z["headdim_logits"]).max())
    assert logits.shape == z["headdim_logits"].shape and err <= 0.35, err


@pytest.mark.parametrize("window,n,passed", [(None, 50, None), (40, 30, None), (40, 40, None), (40, 41, 40), (40, 70, 40)])
def test_where_the_window_goes(monkeypatch, window, n, passed):
    """Window off: no `window` on the KVArgs, the causal call.  Window on: it rides on the fresh prefill's KVArgs and `attend`
    passes it to native.attn_paged only when the launch can reach it (max_ctx > W)."""
    from tgis_amd import native

    lm = _lm(monkeypatch, TinyMistralConfig(sliding_window=window), 3, window)
    calls = []
    causal = native.attn_paged  # (the oracle's causal stand-in: only the arguments are under test here)
    monkeypatch.setattr(native, "attn_paged", lambda *a, **k: (calls.append(k), causal(*a))[1])
    seen = []
    forward = lm.model.forward
    lm.model.forward = lambda *a, **k: (seen.append(a[5]), forward(*a, **k))[1]
    batch = _batch([list(range(3, 3 + n)), [5, 6, 7]])
    lm._prefill_forward(batch)
    assert seen[0].window == window and seen[0].num_splits == 1 and seen[0].fresh_prefill
    assert len(calls) == 2 and all(k.get("window") == passed and ("window" in k) == (passed is not None) for k in calls)


def test_sliding_window_is_read_from_the_config():
    from tgis_amd.utils.sliding_window import parse_sliding_window

    ns = types.SimpleNamespace
    assert parse_sliding_window(ns()) is None and parse_sliding_window(ns(sliding_window=None)) is None
    assert parse_sliding_window(ns(sliding_window=0)) is None and parse_sliding_window(ns(sliding_window=4096)) == 4096
    for bad in (-1, 2.5, "4096", True):
        with pytest.raises(ValueError, match="sliding_window"):
            parse_sliding_window(ns(sliding_window=bad))


def test_what_a_window_refuses():
    from tgis_amd.utils.sliding_window import check_window_options

    cfg = types.SimpleNamespace(max_position_embeddings=32768)
    for kw, option in (({"spec_tokens": 3}, "spec_tokens"), ({"kv_prefix_reuse": True}, "kv_prefix_reuse"),
                       ({"calibrate_kv_scales": True}, "calibrate_kv_scales")):
        with pytest.raises(NotImplementedError, match=f"sliding_window = 4096 and {option}"):
            check_window_options(4096, cfg, **kw)
        check_window_options(None, cfg, **kw)    # no window
        check_window_options(32768, cfg, **kw)   # a window no request within the position limit reaches
        with pytest.raises(NotImplementedError, match=option):
            check_window_options(4096, types.SimpleNamespace(), **kw)  # no stated limit
    check_window_options(4096, cfg)
    check_window_options(4096, cfg, spec_tokens=0, kv_prefix_reuse=False)


def test_the_constructor_and_the_calibration_apply_the_rule():
    """FlashCausalLM needs a GPU to construct; what it calls is in its source: the rule right behind the options it refuses,
    before the cache is allocated, and again at the head of calibrate_kv_scales."""
    import inspect

    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    init = inspect.getsource(FlashCausalLM.__init__)
    rule = init.index("check_window_options(self.sliding_window, self.config, self.spec_tokens, self.kv_prefix_reuse)")
    assert init.index("self.sliding_window = parse_sliding_window(self.config)") < rule < init.index("PagedKVCache(")
    assert "check_window_options(self.sliding_window, self.config, calibrate_kv_scales=True)" in \
        inspect.getsource(FlashCausalLM.calibrate_kv_scales)
    assert FlashCausalLM.sliding_window is None


def test_mistral_fixture_is_decisive():
    meta, z = _fixture()
    assert meta["min_margin"] > meta["margin_bound"] == 0.7 and meta["config"]["sliding_window"] == 40
    assert [len(p) for p in meta["prompts"]] == [7, 45, 100] and z["ids"].shape == (3, 50)
    top = np.sort(z["logits"], axis=-1)
    assert float((top[..., -1] - top[..., -2]).min()) == pytest.approx(meta["min_margin"], abs=1e-5)
    assert (z["logits"].argmax(-1) == z["ids"]).all()
