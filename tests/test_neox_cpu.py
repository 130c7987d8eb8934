"""GPT-NeoX on the flash path, the parts that need no GPU: dispatch, what is refused at load, the qkv row regrouping
under tensor-parallel sharding, and the rotary settings of both transformers config generations."""
import types

import pytest
import torch

from tests.neox_tiny import TinyNeoXConfig, tiny_neox_tensors


def _cfg(**kw):
    from tgis_amd.models.custom_modeling.flash_neox_modeling import GPTNeoXConfig

    base = dict(vocab_size=256, hidden_size=384, num_hidden_layers=1, num_attention_heads=4, intermediate_size=1536)
    base.update(kw)
    return GPTNeoXConfig(**base)


def test_model_class_for_gpt_neox():
    from tgis_amd.inference_engine.tgis_native import FLASH_TYPES, model_class_for
    from tgis_amd.models import FLASH_MODEL_TYPES
    from tgis_amd.models.custom_modeling.flash_neox_modeling import FlashGPTNeoXForCausalLM

    cls, aliases = model_class_for(_cfg())
    assert cls is FlashGPTNeoXForCausalLM and aliases == {"embed_out.weight": ["lm_head.weight"]}
    assert "gpt_neox" in FLASH_MODEL_TYPES and "gpt_neox" in FLASH_TYPES


def test_gptq_is_refused_at_load():
    from tgis_amd.models.custom_modeling.flash_neox_modeling import FlashGPTNeoXForCausalLM

    with pytest.raises(NotImplementedError, match="gptq"):
        FlashGPTNeoXForCausalLM(_cfg(quantize="gptq"), weights=None)  # refused before any weight is read


@pytest.mark.parametrize("hidden,heads,D", [(2560, 32, 80), (2048, 8, 256)])
def test_unsupported_head_sizes_are_refused_at_load(hidden, heads, D):
    from tgis_amd.models.custom_modeling.flash_neox_modeling import FlashGPTNeoXForCausalLM

    with pytest.raises(NotImplementedError, match=f"head size {D}") as e:
        FlashGPTNeoXForCausalLM(_cfg(hidden_size=hidden, num_attention_heads=heads), weights=None)
    assert "Pythia-2.8B" in str(e.value) and "Pythia-1B" in str(e.value)


def test_unknown_activation_is_refused():
    from tgis_amd.models.custom_modeling.flash_neox_modeling import check_neox_config

    with pytest.raises(NotImplementedError, match="relu"):
        check_neox_config(_cfg(hidden_act="relu"))
    for act in ("gelu", "gelu_fast", "gelu_pytorch_tanh"):
        check_neox_config(_cfg(hidden_act=act))


class _Group:
    def __init__(self, rank, world):
        self._r, self._w = rank, world

    def rank(self):
        return self._r

    def size(self):
        return self._w


@pytest.mark.parametrize("world", [1, 2, 4])
def test_qkv_regrouping_per_shard(world):
    """Rank r's q | k | v rows are the rows of heads [r H / w, (r + 1) H / w) of the unsharded HF weight: q rows of those
    heads, then their k rows, then their v rows (each head's D rows in checkpoint order); the bias likewise."""
    from tgis_amd.models.custom_modeling.flash_neox_modeling import qkv_to_q_k_v
    from tgis_amd.utils.weights import DictWeights

    cfg = TinyNeoXConfig("A")
    cfg.num_attention_heads = 8
    H, E = cfg.num_attention_heads, cfg.hidden_size
    D = E // H
    t = tiny_neox_tensors(cfg, seed=3)
    w_full = t["gpt_neox.layers.0.attention.query_key_value.weight"]
    b_full = t["gpt_neox.layers.0.attention.query_key_value.bias"]
    hf = w_full.view(H, 3, D, E)  # HF: head h, part p (q / k / v), dim d
    hb = b_full.view(H, 3, D)
    Hs = H // world
    for rank in range(world):
        wts = DictWeights({k: v.clone() for k, v in t.items()}, device="cpu", dtype=torch.float32,
                          process_group=_Group(rank, world))
        got_w = qkv_to_q_k_v(wts.get_sharded("gpt_neox.layers.0.attention.query_key_value.weight", dim=0), Hs, D)
        got_b = qkv_to_q_k_v(wts.get_sharded("gpt_neox.layers.0.attention.query_key_value.bias", dim=0), Hs, D)
        heads = range(rank * Hs, (rank + 1) * Hs)
        want_w = torch.cat([hf[h, p] for p in range(3) for h in heads])
        want_b = torch.cat([hb[h, p] for p in range(3) for h in heads])
        assert torch.equal(got_w, want_w) and torch.equal(got_b, want_b)


def test_rotary_settings_of_both_config_generations():
    from tgis_amd.models.custom_modeling.flash_neox_modeling import rotary_inv_freq, rotary_settings

    v4 = types.SimpleNamespace(rotary_pct=0.25, rotary_emb_base=10000)
    v5 = types.SimpleNamespace(rope_parameters={"partial_rotary_factor": 0.25, "rope_theta": 10000.0,
                                                "rope_type": "default"})
    for D, rot in ((96, 24), (128, 32), (64, 16)):
        assert rotary_settings(v4, D) == rotary_settings(v5, D) == (rot, 10000.0)
        f4, f5 = rotary_inv_freq(v4, D), rotary_inv_freq(v5, D)
        assert f4.shape == (rot // 2,) and torch.equal(f4, f5)
        assert torch.allclose(f4, 1.0 / (10000.0 ** (torch.arange(0, rot, 2).float() / rot)))
    # a transformers config object of the installed generation agrees as well
    transformers = pytest.importorskip("transformers")
    hf = transformers.GPTNeoXConfig(hidden_size=384, num_attention_heads=4, rotary_pct=0.25, rotary_emb_base=10000)
    assert rotary_settings(hf, 96) == (24, 10000.0)


def test_checkpoint_inv_freq_wins():
    from tgis_amd.models.custom_modeling.flash_neox_modeling import rotary_inv_freq
    from tgis_amd.utils.weights import DictWeights

    stored = torch.linspace(1.0, 0.01, 12)
    wts = DictWeights({"gpt_neox.layers.0.attention.rotary_emb.inv_freq": stored.clone()}, device="cpu",
                      dtype=torch.float16, process_group=_Group(0, 1))
    cfg = types.SimpleNamespace(rotary_pct=0.25, rotary_emb_base=10000)
    got = rotary_inv_freq(cfg, 96, wts, "gpt_neox.layers.0.attention")
    assert got.dtype == torch.float32 and torch.equal(got, stored)
    assert not torch.equal(rotary_inv_freq(cfg, 96, wts, "gpt_neox.layers.1.attention"), stored)


def test_neox_fixtures_are_decisive():
    from tests.fixture_utils import load_fixture

    for name, variant in (("neox_equal", "A"), ("neox_ragged", "B"), ("neox_continuous", "A")):
        meta, steps = load_fixture(name)
        assert meta["variant"] == variant and meta["min_margin"] >= 0.8 and len(steps) >= 5


def test_unsupported_neox_checkpoints_stay_on_the_padded_path_by_default():
    """With FLASH_ATTENTION unset, a gpt_neox checkpoint the flash port refuses (head size 80 / 256, another activation)
    is not routed to it: CausalLM keeps serving it as before."""
    from tgis_amd.models import _flash_supports

    neox20b = {"model_type": "gpt_neox", "hidden_size": 6144, "num_attention_heads": 64, "hidden_act": "gelu_fast"}
    assert _flash_supports("gpt_neox", neox20b)
    assert not _flash_supports("gpt_neox", {**neox20b, "hidden_size": 2560, "num_attention_heads": 32})  # Pythia-2.8B
    assert not _flash_supports("gpt_neox", {**neox20b, "hidden_size": 2048, "num_attention_heads": 8})  # Pythia-1B
    assert not _flash_supports("gpt_neox", {**neox20b, "hidden_act": "relu"})
    assert _flash_supports("llama", {"model_type": "llama"}) and not _flash_supports("gpt2", {})
