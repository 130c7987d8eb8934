"""Seeded tiny Mixtral checkpoints for the routed-expert parity tests (the pattern of tests/mistral_tiny.py).  TEST
INFRASTRUCTURE.

The tensors are a pure function of (config, seed) under the published names (block_sparse_moe.gate, experts.N.w1 / w3 / w2),
so the fixture generator (tests/golden/make_mixtral_fixtures.py, which runs transformers' fp32 CPU MixtralForCausalLM: the
reference project has no Mixtral) and the tests rebuild identical weights; only outputs are committed.  hidden 256, I 512,
4 heads on 2 kv heads, 2 layers, vocab 256, 8 experts, top-2, no sliding window; weights rounded to f16, the output head
scaled up so that greedy margins sit far above f16 noise."""
from typing import Dict, Optional

import torch


class TinyMixtralConfig:
    model_type = "mixtral"

    def __init__(self, sliding_window: Optional[int] = None, max_position_embeddings: int = 512):
        self.vocab_size = 256
        self.hidden_size = 256
        self.intermediate_size = 512
        self.num_hidden_layers = 2
        self.num_attention_heads = 4
        self.num_key_value_heads = 2
        self.num_local_experts = 8
        self.num_experts_per_tok = 2
        self.rms_norm_eps = 1e-5
        self.rope_theta = 10000.0
        self.max_position_embeddings = max_position_embeddings
        self.hidden_act = "silu"
        self.sliding_window = sliding_window
        self.tie_word_embeddings = False
        self.pad_token_id = 0
        self.bos_token_id = 1
        self.eos_token_id = 2

    def to_dict(self):
        return {k: v for k, v in vars(self).items()}


def tiny_mixtral_tensors(cfg: TinyMixtralConfig, seed: int, head_scale: float = 40.0) -> Dict[str, torch.Tensor]:
    """f16 state dict under the published Mixtral names: N(0, 1/sqrt(fan_in)) linears, RMSNorm weights near 1."""
    g = torch.Generator().manual_seed(seed)
    E, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    D = E // H
    t: Dict[str, torch.Tensor] = {}

    def lin(name, n, k, scale=1.0):
        t[f"{name}.weight"] = (torch.randn(n, k, generator=g) * k ** -0.5 * scale).half()

    def norm(name):
        t[f"{name}.weight"] = (1.0 + 0.1 * torch.randn(E, generator=g)).half()

    t["model.embed_tokens.weight"] = torch.randn(V, E, generator=g).half()
    for i in range(cfg.num_hidden_layers):
        p = f"model.layers.{i}"
        lin(f"{p}.self_attn.q_proj", H * D, E)
        lin(f"{p}.self_attn.k_proj", Hkv * D, E)
        lin(f"{p}.self_attn.v_proj", Hkv * D, E)
        lin(f"{p}.self_attn.o_proj", E, H * D)
        lin(f"{p}.block_sparse_moe.gate", cfg.num_local_experts, E)
        for e in range(cfg.num_local_experts):
            lin(f"{p}.block_sparse_moe.experts.{e}.w1", I, E)
            lin(f"{p}.block_sparse_moe.experts.{e}.w3", I, E)
            lin(f"{p}.block_sparse_moe.experts.{e}.w2", E, I)
        norm(f"{p}.input_layernorm")
        norm(f"{p}.post_attention_layernorm")
    norm("model.norm")
    lin("lm_head", V, E, head_scale)
    return t


def fused_names(tensors: Dict[str, torch.Tensor], cfg: TinyMixtralConfig) -> Dict[str, torch.Tensor]:
    """The same checkpoint under the names transformers >= 5 holds in memory: mlp.gate.weight, mlp.experts.gate_up_proj
    [E, 2 I, hidden] (w1 rows, then w3 rows) and mlp.experts.down_proj [E, hidden, I]."""
    out = {k: v for k, v in tensors.items() if ".block_sparse_moe." not in k}
    for i in range(cfg.num_hidden_layers):
        p, q = f"model.layers.{i}.block_sparse_moe", f"model.layers.{i}.mlp"
        out[f"{q}.gate.weight"] = tensors[f"{p}.gate.weight"]
        ex = range(cfg.num_local_experts)
        out[f"{q}.experts.gate_up_proj"] = torch.stack(
            [torch.cat([tensors[f"{p}.experts.{e}.w1.weight"], tensors[f"{p}.experts.{e}.w3.weight"]]) for e in ex])
        out[f"{q}.experts.down_proj"] = torch.stack([tensors[f"{p}.experts.{e}.w2.weight"] for e in ex])
    return out
