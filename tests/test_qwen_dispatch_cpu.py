"""CPU: how Qwen2 and Qwen3 checkpoints reach the Llama flash classes: the dispatch lists, the q/k/v / o_proj bias split, the
q / k norm tensors and what they switch off, the `use_sliding_window` rule, the refusals, and flash_common.write_kv handing
`qk_norm` to each of its three launches (the CPU restatements of tests/qknorm_cpu.py stand in for tgis_amd.native)."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qknorm_cpu  # noqa: E402
from qwen_tiny import TinyQwenConfig, tiny_qwen_tensors  # noqa: E402

from tgis_amd import native  # noqa: E402
from tgis_amd.models.custom_modeling import flash_common, flash_llama_modeling  # noqa: E402
from tgis_amd.utils import sliding_window  # noqa: E402
from tgis_amd.utils.kv_cache import PagedKVCache  # noqa: E402


def _ns(model_type, **kw):
    return types.SimpleNamespace(model_type=model_type, **kw)


# ---- dispatch ----------------------------------------------------------------------------------------------------------------
def test_both_types_are_flash_types_and_take_the_llama_class():
    from tgis_amd import models
    from tgis_amd.inference_engine import tgis_native

    for mt in ("qwen2", "qwen3"):
        assert mt in models.FLASH_MODEL_TYPES and mt in tgis_native.FLASH_TYPES
        assert models._flash_supports(mt, {"model_type": mt})
        cls, aliases = tgis_native.model_class_for(_ns(mt, tie_word_embeddings=True))
        assert cls is flash_llama_modeling.FlashLlamaForCausalLM
        assert aliases == {"lm_head.weight": ["model.embed_tokens.weight"]}
        cls, aliases = tgis_native.model_class_for(_ns(mt, tie_word_embeddings=False))
        assert cls is flash_llama_modeling.FlashLlamaForCausalLM and aliases is None
    assert tuple(models.FLASH_MODEL_TYPES) == tuple(tgis_native.FLASH_TYPES)
    with pytest.raises(NotImplementedError, match="qwen2"):  # (the message lists what is served)
        tgis_native.model_class_for(_ns("qwen3_moe"))


def test_bias_split():
    split = flash_llama_modeling.attention_biases
    assert split(_ns("qwen2")) == (True, False)
    assert split(_ns("qwen2", attention_bias=False)) == (True, False)
    assert split(_ns("qwen3", attention_bias=False)) == (False, False)
    for mt in ("llama", "mistral"):
        assert split(_ns(mt)) == (False, False)
        assert split(_ns(mt, attention_bias=True)) == (True, True)
    assert flash_llama_modeling.has_qk_norm(_ns("qwen3")) and not any(
        flash_llama_modeling.has_qk_norm(_ns(mt)) for mt in ("qwen2", "llama", "mistral"))


class _Linear:
    def __init__(self, bias):
        self.bias, self.rope_heads = bias, None

    def declare_rope_heads(self, *heads):
        self.rope_heads = heads


class _Weights:
    """get_tensor from a name -> tensor dict; notes the names asked for."""

    device = "cpu"

    def __init__(self, tensors, world=1):
        self.tensors, self.asked = tensors, []
        self.process_group = types.SimpleNamespace(size=lambda: world, rank=lambda: 0)

    def get_tensor(self, name):
        self.asked.append(name)
        return self.tensors[name]


@pytest.fixture
def stub_linears(monkeypatch):
    made = {}

    def load_multi(config, prefixes, dim, weights, bias):
        made["qkv"] = _Linear(bias)
        return made["qkv"]

    def load(config, prefix, weights, bias):
        made["o"] = _Linear(bias)
        return made["o"]

    monkeypatch.setattr(flash_llama_modeling.TensorParallelColumnLinear, "load_multi", staticmethod(load_multi))
    monkeypatch.setattr(flash_llama_modeling.TensorParallelRowLinear, "load", staticmethod(load))
    monkeypatch.setattr(flash_llama_modeling.PositionRotaryEmbedding, "static", staticmethod(lambda **kw: kw))
    return made


@pytest.mark.parametrize("world", [1, 2])
def test_attention_of_each_type(stub_linears, world):
    """qwen3: the norm weights are loaded whole on every rank with get_tensor, no rope heads are declared (so neither the fused
    GEMM + rope launch nor fragment-order qkv operands are chosen); qwen2: bias (True, False), rope heads declared."""
    cfg3 = TinyQwenConfig("qwen3")
    w = _Weights(tiny_qwen_tensors(cfg3, 1), world)
    att = flash_llama_modeling.FlashLlamaAttention("model.layers.1.self_attn", cfg3, w)
    assert w.asked == ["model.layers.1.self_attn.q_norm.weight", "model.layers.1.self_attn.k_norm.weight"]
    q_w, k_w, eps = att.qk_norm
    assert torch.equal(q_w, w.tensors[w.asked[0]]) and torch.equal(k_w, w.tensors[w.asked[1]]) and eps == cfg3.rms_norm_eps
    assert q_w.shape == (128,) and att.head_size == 128 and (att.num_heads, att.num_key_value_heads) == (4 // world, 2 // world)
    assert stub_linears["qkv"].rope_heads is None and (stub_linears["qkv"].bias, stub_linears["o"].bias) == (False, False)
    assert att.rotary_emb["base"] == cfg3.rope_theta and att.rotary_emb["dim"] == 128

    cfg2 = TinyQwenConfig("qwen2")
    w = _Weights(tiny_qwen_tensors(cfg2, 1), world)
    att = flash_llama_modeling.FlashLlamaAttention("model.layers.0.self_attn", cfg2, w)
    assert att.qk_norm is None and w.asked == [] and att.head_size == 64
    assert stub_linears["qkv"].rope_heads == (4 // world, 2 // world, 64)
    assert (stub_linears["qkv"].bias, stub_linears["o"].bias) == (True, False)


def test_a_head_size_without_a_kernel_is_refused(stub_linears):
    cfg = TinyQwenConfig("qwen3")
    cfg.head_dim = 32
    tensors = {k: (v[:32] if "_norm.weight" in k and "self_attn" in k else v) for k, v in tiny_qwen_tensors(cfg, 1).items()}
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        flash_llama_modeling.FlashLlamaAttention("model.layers.0.self_attn", cfg, _Weights(tensors))


# ---- sliding window and the refusals ---------------------------------------------------------------------------------------------
def test_use_sliding_window_rule():
    window = sliding_window.parse_sliding_window
    for mt in ("qwen2", "qwen3"):
        assert window(_ns(mt, sliding_window=4096, use_sliding_window=False)) is None
        assert window(_ns(mt, sliding_window=4096)) is None  # (the flag's default is false)
        assert window(_ns(mt, sliding_window=None, use_sliding_window=False)) is None
        with pytest.raises(NotImplementedError, match="use_sliding_window") as e:
            window(_ns(mt, sliding_window=4096, use_sliding_window=True, max_window_layers=28))
        assert "layer_types" in str(e.value) and mt in str(e.value)
    # every other type reads the window as before, whatever flag it carries
    assert window(_ns("mistral", sliding_window=4096)) == 4096
    assert window(_ns("mistral", sliding_window=4096, use_sliding_window=False)) == 4096
    assert window(_ns("llama")) is None and window(TinyQwenConfig("qwen3")) is None and window(TinyQwenConfig("qwen2")) is None


def test_lora_is_refused_by_name():
    from tgis_amd.utils.lora import check_lora_model

    for mt in ("qwen2", "qwen3"):
        model = types.SimpleNamespace(config=_ns(mt), enable_lora=lambda *a: None)
        check_lora_model(0, model)
        with pytest.raises(NotImplementedError, match=f"lora_slots=4.*{mt}"):
            check_lora_model(4, model)
    check_lora_model(4, types.SimpleNamespace(config=_ns("llama"), enable_lora=lambda *a: None))


def test_other_rope_scalings_stay_refused():
    with pytest.raises(ValueError, match="yarn"):
        flash_llama_modeling.rope_settings(_ns("qwen3", rope_scaling={"rope_type": "yarn", "factor": 4.0}))
    assert flash_llama_modeling.rope_settings(_ns("qwen3", rope_parameters={"rope_theta": 1e6, "rope_type": "default"})) == (1e6, 1.0)


@pytest.mark.parametrize("model_type", ["qwen3", "qwen2"])
def test_fixtures_are_decisive(model_type):
    """What tests/golden/make_qwen_fixtures.py wrote: every id decided by more than twice the f16 logit bar, and a Llama twin of
    the same tensors (no q / k norm, no q/k/v bias) far from the fixture at the first generated token of every prompt."""
    import json

    import numpy as np

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"{model_type}_tiny.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    assert meta["min_margin"] > meta["margin_bound"] == 0.7 and meta["config"] == TinyQwenConfig(model_type).to_dict()
    assert [len(p) for p in meta["prompts"]] == [7, 45, 100] and z["ids"].shape == (3, 50)
    top = np.sort(z["logits"], axis=-1)
    assert float((top[..., -1] - top[..., -2]).min()) == pytest.approx(meta["min_margin"], abs=1e-5)
    assert (z["logits"].argmax(-1) == z["ids"]).all() and min(meta["llama_twin_diff"]) > 0.35
    assert len(set(z["ids"].reshape(-1).tolist())) > 30  # (not one token repeated: the layers, not the tied embedding, decide)


# ---- write_kv: the three forms with qk_norm passed through ----------------------------------------------------------------------
H, HKV, D, LAYER = 4, 2, 64, 1


def _setup(lens, past=None, **kw):
    from oracle import ops_ref

    g = torch.Generator().manual_seed(5)
    cache = PagedKVCache(2, HKV, D, 8, torch.float16, "cpu")
    for pool in (cache.k_pool(LAYER), cache.v_pool(LAYER)):
        pool.fill_(float("nan"))
    past = past or [0] * len(lens)
    T = sum(lens)
    cu = torch.tensor([0, *torch.tensor(lens).cumsum(0).tolist()], dtype=torch.int32)
    bt = torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]], dtype=torch.int32)[:len(lens)]
    where = [p + torch.arange(n) for p, n in zip(past, lens)]
    slots = torch.cat([bt[b, w // 32] * 32 + w % 32 for b, w in enumerate(where)]).to(torch.int32)
    pos = torch.cat(where).to(torch.int32)
    kv = flash_common.KVArgs(cache=cache, block_tables=bt, ctx_lens=torch.tensor([p + n for p, n in zip(past, lens)],
                                                                                 dtype=torch.int32),
                             slots=slots, max_q_len=max(lens), max_ctx=max(p + n for p, n in zip(past, lens)), **kw)
    qkv = torch.randn((T, (H + 2 * HKV) * D), generator=g).half()
    cos, sin = ops_ref.rope_tables(D, 10000.0, 256, torch.float16)
    qk_norm = ((0.5 + 1.5 * torch.rand(D, generator=g)).half(), (0.5 + 1.5 * torch.rand(D, generator=g)).half(), 1e-6)
    return cache, kv, qkv, cos, sin, pos, cu, qk_norm


def _write(s, qkv, **kw):
    cache, kv, _, cos, sin, pos, cu, _ = s
    return flash_common.write_kv(qkv, kv, LAYER, H, HKV, D, D, cos, sin, pos, cu, **kw)


def test_write_kv_passes_qk_norm_to_each_form(monkeypatch):
    """The same tokens through the per-token, the fresh page-wise and the past_lens form: each launch gets the qk_norm it was
    given, and the three leave the same q and the same pages.  Without qk_norm no launch sees the keyword at all."""
    qknorm_cpu.install(monkeypatch, native)
    lens = [40, 3]
    runs = {}
    for name, kw, past in (("rope_kv_write", {}, None), ("rope_kv_write_prefill", dict(fresh_prefill=True), None),
                           ("rope_kv_write_prefill_at", dict(past_lens=torch.zeros(2, dtype=torch.int32)), None)):
        s = _setup(lens, past, **kw)
        qkv = s[2].clone()
        got = _write(s, qkv, qk_norm=s[7])
        assert got is qkv and qknorm_cpu.CALLS[-1][0] == name and qknorm_cpu.CALLS[-1][1]["qk_norm"] is s[7]
        runs[name] = (got[:, :H * D].clone(), s[0].k_pool(LAYER).clone(), s[0].v_pool(LAYER).clone())
        assert not torch.isnan(runs[name][0]).any()
        # the norm is applied: the plain launch of the same form leaves another q
        plain = _write(_setup(lens, past, **kw), s[2].clone())
        assert qknorm_cpu.CALLS[-1] == (name, dict(qk_norm=None))
        assert (plain[:, :H * D].float() - got[:, :H * D].float()).abs().max() > 0.5
    first = runs["rope_kv_write"]
    for name, run in runs.items():
        for a, b in zip(first, run):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), name


def test_write_kv_without_qk_norm_makes_the_current_calls(monkeypatch):
    seen = []
    for name in ("rope_kv_write", "rope_kv_write_prefill", "rope_kv_write_prefill_at"):
        monkeypatch.setattr(native, name, lambda *a, _n=name, **k: seen.append((_n, k)) or a[0])
    for kw in ({}, dict(fresh_prefill=True), dict(past_lens=torch.zeros(2, dtype=torch.int32))):
        s = _setup([40, 3], **kw)
        _write(s, s[2])
        _write(s, s[2], qk_norm=s[7])
    assert [n for n, _ in seen] == ["rope_kv_write"] * 2 + ["rope_kv_write_prefill"] * 2 + ["rope_kv_write_prefill_at"] * 2
    assert all(k == {} for _, k in seen[0::2]) and all(list(k) == ["qk_norm"] for _, k in seen[1::2])


def test_a_reused_prefix_goes_behind_past_lens(monkeypatch):
    """past_lens = (32, 0): the first sequence's suffix lands on its second page, its first page is not touched."""
    qknorm_cpu.install(monkeypatch, native)
    s = _setup([10, 3], past=[32, 0], past_lens=torch.tensor([32, 0], dtype=torch.int32))
    _write(s, s[2], qk_norm=s[7])
    kp = s[0].k_pool(LAYER)
    assert qknorm_cpu.CALLS[-1][0] == "rope_kv_write_prefill_at"
    assert torch.isnan(kp[0]).all() and not torch.isnan(kp[1]).all() and not torch.isnan(kp[4]).all()
