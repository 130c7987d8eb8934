"""Seeded tiny Qwen3 and Qwen2 checkpoints for the parity tests (the pattern of tests/mistral_tiny.py).  TEST INFRASTRUCTURE.

The tensors are a pure function of (config, seed), so the fixture generator (tests/golden/make_qwen_fixtures.py, which runs
transformers' fp32 CPU Qwen3ForCausalLM / Qwen2ForCausalLM) and the tests rebuild identical weights; only outputs are
committed.  hidden 256, 2 layers, vocab 256, weights rounded to f16, the output head scaled up so that greedy margins sit far
above fp16 noise.
  qwen3: 4 heads on 2 kv heads of head_dim 128 (not hidden / heads: the shape every Qwen3 has), tied embeddings, q_norm / k_norm
         weights drawn from [0.5, 2] and q_proj scaled by 3, so the norm is far from the identity;
  qwen2: head_dim 64 = hidden / heads, q/k/v biases N(0, 0.3), no o_proj bias, an output head of its own.
The tied embedding sits in the residual stream that its own transpose reads, which alone would make every greedy token the
last input token: o_proj and down_proj of the tied model are scaled by 32 so that the layers, not the embedding, decide.
Both carry what their config.json carries: `sliding_window` next to `use_sliding_window: false`."""
from typing import Dict

import torch


class TinyQwenConfig:
    def __init__(self, model_type: str = "qwen3", max_position_embeddings: int = 512):
        assert model_type in ("qwen2", "qwen3")
        self.model_type = model_type
        self.vocab_size = 256
        self.hidden_size = 256
        self.intermediate_size = 512
        self.num_hidden_layers = 2
        self.num_attention_heads = 4
        self.num_key_value_heads = 2
        self.rms_norm_eps = 1e-6
        self.rope_theta = 1000000.0
        self.max_position_embeddings = max_position_embeddings
        self.hidden_act = "silu"
        self.sliding_window = 128
        self.use_sliding_window = False
        self.max_window_layers = 2
        if model_type == "qwen3":
            self.head_dim = 128
            self.attention_bias = False
        self.tie_word_embeddings = model_type == "qwen3"
        self.pad_token_id = 0
        self.bos_token_id = 1
        self.eos_token_id = 2

    def to_dict(self):
        return {k: v for k, v in vars(self).items()}


def tiny_qwen_tensors(cfg: TinyQwenConfig, seed: int, head_scale: float = 40.0) -> Dict[str, torch.Tensor]:
    """f16 HF-named state dict (Llama's tensor names + q_norm / k_norm resp. the q/k/v biases): N(0, 1/sqrt(fan_in)) linears,
    RMSNorm weights near 1.  A tied model's embedding is the scaled head: N(0, head_scale / sqrt(E)), which the first
    RMSNorm normalises away on the input side."""
    g = torch.Generator().manual_seed(seed)
    E, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    D = getattr(cfg, "head_dim", None) or E // H
    qwen3 = cfg.model_type == "qwen3"
    t: Dict[str, torch.Tensor] = {}

    def lin(name, n, k, scale=1.0, bias=False):
        t[f"{name}.weight"] = (torch.randn(n, k, generator=g) * k ** -0.5 * scale).half()
        if bias:
            t[f"{name}.bias"] = (0.3 * torch.randn(n, generator=g)).half()

    def norm(name):
        t[f"{name}.weight"] = (1.0 + 0.1 * torch.randn(E, generator=g)).half()

    def head_norm(name):
        t[f"{name}.weight"] = (0.5 + 1.5 * torch.rand(D, generator=g)).half()

    if qwen3:
        t["model.embed_tokens.weight"] = (torch.randn(V, E, generator=g) * E ** -0.5 * head_scale).half()
    else:
        t["model.embed_tokens.weight"] = torch.randn(V, E, generator=g).half()
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}"
        lin(f"{p}.self_attn.q_proj", H * D, E, scale=3.0 if qwen3 else 1.0, bias=not qwen3)
        lin(f"{p}.self_attn.k_proj", Hkv * D, E, bias=not qwen3)
        lin(f"{p}.self_attn.v_proj", Hkv * D, E, bias=not qwen3)
        lin(f"{p}.self_attn.o_proj", E, H * D, scale=32.0 if qwen3 else 1.0)
        if qwen3:
            head_norm(f"{p}.self_attn.q_norm")
            head_norm(f"{p}.self_attn.k_norm")
        lin(f"{p}.mlp.gate_proj", I, E)
        lin(f"{p}.mlp.up_proj", I, E)
        lin(f"{p}.mlp.down_proj", E, I, scale=32.0 if qwen3 else 1.0)
        norm(f"{p}.input_layernorm")
        norm(f"{p}.post_attention_layernorm")
    norm("model.norm")
    if not qwen3:
        lin("lm_head", V, E, head_scale)
    return t
