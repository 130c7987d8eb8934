"""Seeded tiny Mistral checkpoints for the sliding-window parity tests (the pattern of oracle/tiny_models.py and
tests/neox_tiny.py).  TEST INFRASTRUCTURE.

The tensors are a pure function of (config, seed), so the fixture generator (tests/golden/make_mistral_fixtures.py, which
runs transformers' fp32 CPU MistralForCausalLM: the reference project has no Mistral) and the tests rebuild identical
weights; only outputs are committed.  hidden 256, 4 heads on 2 kv heads, 2 layers, vocab 256, sliding_window 40; the weights
are rounded to f16 (the fp32 reference and the f16 kernels see the same values) and the output head is scaled up (as the tiny
Llama's is) so that greedy margins sit far above fp16 noise.  head_dim: None = hidden / heads = 64; 32 is the variant whose
head size is not hidden / heads (Mistral-Nemo's shape in miniature), which no kernel serves: it is loaded on the CPU only."""
from typing import Dict, Optional

import torch


class TinyMistralConfig:
    model_type = "mistral"

    def __init__(self, sliding_window: Optional[int] = 40, head_dim: Optional[int] = None,
                 max_position_embeddings: int = 512):
        self.vocab_size = 256
        self.hidden_size = 256
        self.intermediate_size = 512
        self.num_hidden_layers = 2
        self.num_attention_heads = 4
        self.num_key_value_heads = 2
        self.rms_norm_eps = 1e-5
        self.rope_theta = 10000.0
        self.max_position_embeddings = max_position_embeddings
        self.hidden_act = "silu"
        self.sliding_window = sliding_window
        if head_dim is not None:
            self.head_dim = head_dim
        self.tie_word_embeddings = False
        self.pad_token_id = 0
        self.bos_token_id = 1
        self.eos_token_id = 2

    def to_dict(self):
        """What a Mistral config.json carries: no attention_bias, no mlp_bias."""
        return {k: v for k, v in vars(self).items()}


def tiny_mistral_tensors(cfg: TinyMistralConfig, seed: int, head_scale: float = 40.0) -> Dict[str, torch.Tensor]:
    """f16 HF-named Mistral state dict (Llama's tensor names): N(0, 1/sqrt(fan_in)) linears, RMSNorm weights near 1."""
    g = torch.Generator().manual_seed(seed)
    E, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    H, Hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    D = getattr(cfg, "head_dim", None) or E // H
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
        lin(f"{p}.mlp.gate_proj", I, E)
        lin(f"{p}.mlp.up_proj", I, E)
        lin(f"{p}.mlp.down_proj", E, I)
        norm(f"{p}.input_layernorm")
        norm(f"{p}.post_attention_layernorm")
    norm("model.norm")
    lin("lm_head", V, E, head_scale)
    return t
