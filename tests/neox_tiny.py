"""Seeded tiny GPT-NeoX checkpoints for the NeoX parity tests (the pattern of oracle/tiny_models.py).  TEST INFRASTRUCTURE.

The tensors are a pure function of (config, seed), so the fixture generator (tests/golden/make_neox_fixtures.py, which
runs the reference's CPU causal_lm) and the GPU tests rebuild identical weights; only outputs are committed.
  A: hidden 384, 4 heads (head size 96, 24 rotary dims), parallel residual, gelu_fast — gpt-neox-20b's layer in miniature.
  B: hidden 256, 4 heads (head size 64, 16 rotary dims), sequential residual, exact gelu.
The output head is scaled up (as the tiny Llama's is) so that greedy margins sit far above fp16 noise."""
from typing import Dict

import torch


class TinyNeoXConfig:
    model_type = "gpt_neox"

    def __init__(self, variant="A"):
        self.variant = variant
        self.vocab_size = 256
        self.hidden_size = 384 if variant == "A" else 256
        self.num_attention_heads = 4
        self.intermediate_size = 4 * self.hidden_size
        self.num_hidden_layers = 2
        self.rotary_pct = 0.25
        self.rotary_emb_base = 10000
        self.use_parallel_residual = variant == "A"
        self.hidden_act = "gelu_fast" if variant == "A" else "gelu"
        self.layer_norm_eps = 1e-5
        self.max_position_embeddings = 512
        self.tie_word_embeddings = False
        self.pad_token_id = 0
        self.bos_token_id = 1
        self.eos_token_id = 2

    def to_dict(self):
        return {k: v for k, v in vars(self).items()}

    def hf_kwargs(self):
        """GPTNeoXConfig keyword arguments (both transformers generations read rotary_pct / rotary_emb_base)."""
        d = self.to_dict()
        d.pop("variant")
        return d


def tiny_neox_tensors(cfg: TinyNeoXConfig, seed: int, head_scale: float = 48.0) -> Dict[str, torch.Tensor]:
    """fp32 HF-named GPT-NeoX state dict: N(0, 1/sqrt(fan_in)) linears with small biases, LayerNorms near identity;
    query_key_value rows in the checkpoint's head-interleaved [H, 3, D] order."""
    g = torch.Generator().manual_seed(seed)
    E, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    t: Dict[str, torch.Tensor] = {}

    def lin(name, n, k, scale=1.0):
        t[f"{name}.weight"] = torch.randn(n, k, generator=g) * k ** -0.5 * scale
        t[f"{name}.bias"] = torch.randn(n, generator=g) * 0.02

    def ln(name):
        t[f"{name}.weight"] = 1.0 + torch.randn(E, generator=g) * 0.05
        t[f"{name}.bias"] = torch.randn(E, generator=g) * 0.02

    t["gpt_neox.embed_in.weight"] = torch.randn(V, E, generator=g)
    for i in range(cfg.num_hidden_layers):
        p = f"gpt_neox.layers.{i}"
        ln(f"{p}.input_layernorm")
        ln(f"{p}.post_attention_layernorm")
        lin(f"{p}.attention.query_key_value", 3 * E, E)
        lin(f"{p}.attention.dense", E, E)
        lin(f"{p}.mlp.dense_h_to_4h", I, E)
        lin(f"{p}.mlp.dense_4h_to_h", E, I)
    ln("gpt_neox.final_layer_norm")
    t["embed_out.weight"] = torch.randn(V, E, generator=g) * E ** -0.5 * head_scale
    return t
