"""Qwen3-MoE on the flash path, the parts that need no GPU: the dispatch, what the loader reads under the published names and
under the fused names transformers >= 5 holds in memory, and the refusals, each by name and before any weight is read."""
import types

import pytest
import torch

from tests.qwen3_moe_tiny import TinyQwen3MoeConfig, fused_names, tiny_qwen3_moe_tensors

CPU = torch.device("cpu")


def _config(**over):
    ns = types.SimpleNamespace(**TinyQwen3MoeConfig().to_dict(), model_type="qwen3_moe", quantize=None)
    for k, v in over.items():
        setattr(ns, k, v)
    return ns


def test_dispatch_picks_the_class():
    from tgis_amd.inference_engine.tgis_native import FLASH_TYPES, model_class_for
    from tgis_amd.models import FLASH_MODEL_TYPES, _flash_supports
    from tgis_amd.models.custom_modeling.flash_llama_modeling import has_qk_norm
    from tgis_amd.models.custom_modeling.flash_qwen3_moe_modeling import FlashQwen3MoeForCausalLM
    from tgis_amd.utils.sliding_window import parse_sliding_window

    assert "qwen3_moe" in FLASH_MODEL_TYPES and tuple(FLASH_MODEL_TYPES) == tuple(FLASH_TYPES) and _flash_supports("qwen3_moe", {})
    cls, aliases = model_class_for(_config())
    assert cls is FlashQwen3MoeForCausalLM and aliases is None
    assert model_class_for(_config(tie_word_embeddings=True))[1] == {"lm_head.weight": ["model.embed_tokens.weight"]}
    assert has_qk_norm(_config()) and parse_sliding_window(_config(sliding_window=4096)) is None
    with pytest.raises(NotImplementedError, match="Qwen3-MoE.*num_experts"):  # the model type alone is not a servable config
        model_class_for(types.SimpleNamespace(model_type="qwen3_moe"))


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_both_namings_load_the_same_expert_tensors(rank, world):
    from tgis_amd.models.custom_modeling.flash_qwen3_moe_modeling import Qwen3MoeExpertTensors
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.weights import DictWeights

    cfg = TinyQwen3MoeConfig("nonorm")
    published = tiny_qwen3_moe_tensors(cfg, 3)
    fused = fused_names(published, cfg)
    assert not any(".experts.0." in k for k in fused)
    I, Il = cfg.moe_intermediate_size, cfg.moe_intermediate_size // world
    for layer in range(cfg.num_hidden_layers):
        a, b = (Qwen3MoeExpertTensors(f"model.layers.{layer}", DictWeights(t, CPU, torch.float16, FakeGroup(rank, world)), I)
                for t in (published, fused))
        assert a.published and not b.published
        assert torch.equal(a.router(), b.router()) and a.router().shape == (cfg.num_experts, cfg.hidden_size)
        for e in range(cfg.num_experts):
            p, lo = f"model.layers.{layer}.mlp.experts.{e}", rank * Il
            gu, dn = a.gate_up(e), a.down(e)
            assert torch.equal(gu, b.gate_up(e)) and torch.equal(dn, b.down(e))
            assert torch.equal(gu[:Il], published[f"{p}.gate_proj.weight"][lo:lo + Il])
            assert torch.equal(gu[Il:], published[f"{p}.up_proj.weight"][lo:lo + Il])
            assert torch.equal(dn, published[f"{p}.down_proj.weight"][:, lo:lo + Il])


@pytest.mark.parametrize("over,name", [
    (dict(decoder_sparse_step=2), "decoder_sparse_step"), (dict(mlp_only_layers=[0]), "mlp_only_layers"),
    (dict(num_experts=129), "num_experts"), (dict(num_experts_per_tok=9), "num_experts_per_tok"),
    (dict(hidden_act="gelu"), "hidden_act"), (dict(use_sliding_window=True), "use_sliding_window"),
    (dict(quantize="gptq"), "gptq"), (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), "rope_scaling"),
])
def test_refusals_name_what_is_refused(over, name):
    from tgis_amd.models.custom_modeling.flash_qwen3_moe_modeling import FlashQwen3MoeForCausalLM

    with pytest.raises(NotImplementedError, match=f"Qwen3-MoE.*{name}"):
        FlashQwen3MoeForCausalLM(_config(**over), object())  # any read of a weight would raise AttributeError


def test_lora_slots_are_refused_and_the_defaults_are_read():
    from tgis_amd.models.custom_modeling.flash_qwen3_moe_modeling import check_qwen3_moe_config
    from tgis_amd.utils.lora import check_lora_model

    with pytest.raises(NotImplementedError, match="qwen3_moe"):
        check_lora_model(1, types.SimpleNamespace(config=_config()))
    assert check_qwen3_moe_config(_config()) == (128, 8, True)
    assert check_qwen3_moe_config(_config(rope_scaling={"type": "linear", "factor": 2.0})) == (128, 8, True)
    cfg = _config(num_experts=16, num_experts_per_tok=4)
    del cfg.norm_topk_prob  # the config's default
    assert check_qwen3_moe_config(cfg) == (16, 4, False)
