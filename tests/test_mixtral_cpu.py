"""Mixtral on the flash path, the parts that need no GPU: the fp64 restatement of the routed expert MLP (tests/moe_ref.py)
against transformers' MixtralSparseMoeBlock and MixtralTopKRouter in fp32, the dispatch, what the loader reads under the
published names and under the names transformers holds in memory (and what it saves), and the refusals."""
import types

import pytest
import torch

from tests import moe_ref
from tests.mixtral_tiny import TinyMixtralConfig, fused_names, tiny_mixtral_tensors

CPU = torch.device("cpu")
HIDDEN, INTER, E, TOP_K, TOKENS = 64, 48, 8, 2, 40


def _hf_block(seed=0):
    from transformers import MixtralConfig
    from transformers.models.mixtral.modeling_mixtral import MixtralSparseMoeBlock

    g = torch.Generator().manual_seed(seed)
    block = MixtralSparseMoeBlock(MixtralConfig(hidden_size=HIDDEN, intermediate_size=INTER, num_local_experts=E,
                                                num_experts_per_tok=TOP_K)).float().eval()
    with torch.no_grad():
        block.gate.weight.copy_(torch.randn(E, HIDDEN, generator=g) * HIDDEN ** -0.5)
        block.experts.gate_up_proj.copy_(torch.randn(E, 2 * INTER, HIDDEN, generator=g) * HIDDEN ** -0.5)
        block.experts.down_proj.copy_(torch.randn(E, HIDDEN, INTER, generator=g) * INTER ** -0.5)
    x = torch.randn(TOKENS, HIDDEN, generator=g)
    return block, x


def test_restatement_equals_transformers_block():
    """fp32 transformers against the fp64 restatement.  The bar is fp32 roundoff of the block's sums: each output is a sum
    of top_k scaled dot products of length I over hidden-long ones, so |error| <= c u (sum of |terms|) with u = 2^-24 and the
    number of roundings per term c <= hidden + I + 16 (two GEMM chains, SiLU, softmax, scale, add); the bound is evaluated
    on the absolute values."""
    block, x = _hf_block()
    with torch.no_grad():
        got = block(x[None])[0].double()
    gate = block.gate.weight.detach()
    gu, w2 = block.experts.gate_up_proj.detach(), block.experts.down_proj.detach()
    w1, w3 = gu[:, :INTER], gu[:, INTER:]
    ref = moe_ref.moe_block(x, gate, w1, w3, w2, TOP_K)
    # the same expression on absolute values bounds the sum of |terms|
    ids, w = moe_ref.route(x.double() @ gate.double().t(), TOP_K)
    habs = torch.empty((TOKENS * TOP_K, INTER), dtype=torch.float64)
    for t in range(TOKENS):
        for k in range(TOP_K):
            e = int(ids[t, k])
            g = w1[e].double().abs() @ x[t].double().abs()
            habs[t * TOP_K + k] = g * (w3[e].double().abs() @ x[t].double().abs())  # |silu(g)| <= |g|
    mag = moe_ref.expert_down(habs, w2.abs(), ids, w).sum(dim=1)
    tol = (HIDDEN + INTER + 16) * 2.0 ** -24 * mag
    err = (got - ref).abs()
    assert (err <= tol).all(), f"max err {err.max():.3e}, bound there {tol.flatten()[err.argmax()]:.3e}"
    # the bar is an fp32 one: far below the outputs themselves, which a wrong expert or weight would move by their own size
    assert float(tol.max()) < 0.02 * float(ref.abs().mean())


def test_routing_equals_the_transformers_router():
    """Indices exactly and scores to fp32 roundoff (4 ulp) on inputs without near-ties among the three largest."""
    block, _ = _hf_block(1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(400, HIDDEN, generator=g)
    with torch.no_grad():
        logits, scores, indices = block.gate(x)
    top3 = torch.topk(logits, 3, dim=-1).values
    keep = ((top3[:, 0] - top3[:, 1]) > 1e-3) & ((top3[:, 1] - top3[:, 2]) > 1e-3)
    assert int(keep.sum()) > 300
    ids, w = moe_ref.route(logits, TOP_K)
    assert torch.equal(ids[keep], indices[keep])
    ulp = torch.abs(torch.nextafter(scores, torch.ones_like(scores)) - scores).double()
    assert ((w - scores.double()).abs()[keep] <= 4 * ulp[keep]).all()


def test_ties_go_to_the_lower_index_and_lists_are_grouped():
    logits = torch.tensor([[1.0, 3.0, 3.0, 3.0], [0.0, 0.0, 0.0, 0.0], [5.0, 1.0, 5.0, 2.0]])
    ids, w = moe_ref.route(logits, 2)
    assert ids.tolist() == [[1, 2], [0, 1], [0, 2]]
    assert torch.allclose(w, torch.full((3, 2), 0.5, dtype=torch.float64))
    counts, offsets, slot_rows = moe_ref.lists(ids, 4)
    assert counts.tolist() == [2, 2, 2, 0] and offsets.tolist() == [0, 2, 4, 6, 6]
    assert slot_rows.tolist() == [2, 4, 0, 3, 1, 5]


def _config(**over):
    cfg = TinyMixtralConfig()
    ns = types.SimpleNamespace(model_type="mixtral", quantize=None, **cfg.to_dict())
    for k, v in over.items():
        setattr(ns, k, v)
    return ns


def test_dispatch_lists_include_mixtral():
    from tgis_amd.inference_engine.tgis_native import FLASH_TYPES, model_class_for
    from tgis_amd.models import FLASH_MODEL_TYPES, _flash_supports
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import FlashMixtralForCausalLM

    assert "mixtral" in FLASH_MODEL_TYPES and "mixtral" in FLASH_TYPES and _flash_supports("mixtral", {})
    cls, aliases = model_class_for(_config())
    assert cls is FlashMixtralForCausalLM and aliases is None
    assert model_class_for(_config(tie_word_embeddings=True))[1] == {"lm_head.weight": ["model.embed_tokens.weight"]}


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_both_namings_load_the_same_expert_tensors(rank, world):
    """Published names (block_sparse_moe.experts.N.w1 / w3 / w2) and the fused in-memory names of transformers >= 5 give the
    loader the same router and the same per-expert [gate | up] and down tensors, whole and as a shard of two."""
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.weights import DictWeights

    cfg = TinyMixtralConfig()
    published = tiny_mixtral_tensors(cfg, 3)
    fused = fused_names(published, cfg)
    assert not any("block_sparse_moe" in k for k in fused)
    I, Il = cfg.intermediate_size, cfg.intermediate_size // world
    for layer in range(cfg.num_hidden_layers):
        a, b = (ExpertTensors(f"model.layers.{layer}", DictWeights(t, CPU, torch.float16, FakeGroup(rank, world)), I)
                for t in (published, fused))
        assert a.published and not b.published
        assert torch.equal(a.router(), b.router()) and a.router().shape == (cfg.num_local_experts, cfg.hidden_size)
        for e in range(cfg.num_local_experts):
            p = f"model.layers.{layer}.block_sparse_moe.experts.{e}"
            gu, dn = a.gate_up(e), a.down(e)
            assert torch.equal(gu, b.gate_up(e)) and torch.equal(dn, b.down(e))
            lo = rank * Il
            assert torch.equal(gu[:Il], published[f"{p}.w1.weight"][lo:lo + Il])
            assert torch.equal(gu[Il:], published[f"{p}.w3.weight"][lo:lo + Il])
            assert torch.equal(dn, published[f"{p}.w2.weight"][:, lo:lo + Il])


def test_what_transformers_saves_carries_the_published_names(tmp_path):
    """A tiny checkpoint saved by the installed transformers: its tensor names are the ones the loader reads, and they hold
    the fused parameters' values."""
    from safetensors import safe_open
    from transformers import MixtralConfig, MixtralForCausalLM

    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.weights import DictWeights

    model = MixtralForCausalLM(MixtralConfig(vocab_size=32, hidden_size=32, intermediate_size=16, num_hidden_layers=1,
                                             num_attention_heads=2, num_key_value_heads=1, num_local_experts=4,
                                             num_experts_per_tok=2))
    model.save_pretrained(tmp_path)
    with safe_open(str(tmp_path / "model.safetensors"), "pt") as f:
        saved = {k: f.get_tensor(k) for k in f.keys()}
    et = ExpertTensors("model.layers.0", DictWeights(saved, CPU, torch.float32, FakeGroup(0, 1)), 16)
    state = model.state_dict()
    fused_gate_up = state["model.layers.0.mlp.experts.gate_up_proj"]
    assert torch.equal(et.router(), state["model.layers.0.mlp.gate.weight"])
    for e in range(4):
        assert torch.equal(et.gate_up(e), fused_gate_up[e])
        assert torch.equal(et.down(e), state["model.layers.0.mlp.experts.down_proj"][e])


def test_refusals_name_mixtral():
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import FlashMixtralForCausalLM, check_mixtral_config

    class NoWeights:  # any read would raise AttributeError: the refusal comes first
        pass

    with pytest.raises(NotImplementedError, match="Mixtral.*GPTQ"):
        FlashMixtralForCausalLM(_config(quantize="gptq"), NoWeights())
    with pytest.raises(NotImplementedError, match="Mixtral.*hidden_act"):
        check_mixtral_config(_config(hidden_act="gelu"))
    for bad in (dict(num_local_experts=1), dict(num_local_experts=128), dict(num_experts_per_tok=0),
                dict(num_experts_per_tok=9), dict(num_local_experts=4, num_experts_per_tok=5)):
        with pytest.raises(NotImplementedError, match="Mixtral"):
            check_mixtral_config(_config(**bad))
    assert check_mixtral_config(_config()) == (8, 2)


def test_the_path_hook_is_read(monkeypatch):
    from tgis_amd.models.custom_modeling import flash_mixtral_modeling as fm

    for value, want in (("fused", "fused"), ("loop", "loop"), ("auto", None)):
        monkeypatch.setenv("TGIS_MOE_PATH", value)
        assert fm.moe_path_override() == want
    monkeypatch.setenv("TGIS_MOE_PATH", "sometimes")
    with pytest.raises(ValueError):
        fm.moe_path_override()
    assert fm.MOE_FUSED_MAX_TOKENS >= 1
