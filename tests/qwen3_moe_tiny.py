"""Seeded tiny Qwen3-MoE checkpoints for the parity tests (the pattern of tests/mixtral_tiny.py).  TEST INFRASTRUCTURE.

The tensors are the synthetic maker's (tgis_amd.inference_engine.synthetic.qwen3_moe_tensors, published names, f16), a pure
function of (config, seed), so the fixture generator (tests/golden/make_qwen3_moe_fixtures.py, which runs transformers' fp32
CPU Qwen3MoeForCausalLM) and the tests rebuild identical weights; only outputs are committed.  2 layers, hidden 64, 2 heads
on 1 kv head of head_dim 64, moe intermediate 32, vocab 64; 128 experts top-8 renormalised, or ("nonorm") 16 experts top-4
with norm_topk_prob false.  The routers are scaled by ROUTER_SCALE so that the gap between the last chosen expert and the
first one left out is wide against what an f16 run moves a router logit, and the head by 40 so that greedy margins are."""
from typing import Dict

import torch

ROUTER_SCALE = 4.0


class TinyQwen3MoeConfig:
    model_type = "qwen3_moe"

    def __init__(self, kind: str = "e128", max_position_embeddings: int = 512):
        assert kind in ("e128", "nonorm")
        self.vocab_size = 64
        self.hidden_size = 64
        self.moe_intermediate_size = 32
        self.intermediate_size = 32
        self.num_hidden_layers = 2
        self.num_attention_heads = 2
        self.num_key_value_heads = 1
        self.head_dim = 64
        self.num_experts, self.num_experts_per_tok = (128, 8) if kind == "e128" else (16, 4)
        self.norm_topk_prob = kind == "e128"
        self.decoder_sparse_step = 1
        self.mlp_only_layers = []
        self.rms_norm_eps = 1e-6
        self.rope_theta = 1000000.0
        self.max_position_embeddings = max_position_embeddings
        self.hidden_act = "silu"
        self.attention_bias = False
        self.sliding_window = None
        self.use_sliding_window = False
        self.tie_word_embeddings = False
        self.pad_token_id = 0
        self.bos_token_id = 1
        self.eos_token_id = 2

    def to_dict(self):
        return {k: v for k, v in vars(self).items()}


def tiny_qwen3_moe_tensors(cfg: TinyQwen3MoeConfig, seed: int, head_scale: float = 40.0) -> Dict[str, torch.Tensor]:
    from tgis_amd.inference_engine.synthetic import qwen3_moe_tensors

    t = qwen3_moe_tensors(cfg, seed, dtype=torch.float16, head_scale=head_scale)
    for i in range(cfg.num_hidden_layers):
        name = f"model.layers.{i}.mlp.gate.weight"
        t[name] = (t[name].float() * ROUTER_SCALE).half()
    return t


def fused_names(tensors: Dict[str, torch.Tensor], cfg: TinyQwen3MoeConfig) -> Dict[str, torch.Tensor]:
    """The same checkpoint under the names transformers >= 5 holds in memory: mlp.experts.gate_up_proj [E, 2 I, hidden]
    (gate_proj rows, then up_proj rows) and mlp.experts.down_proj [E, hidden, I]."""
    out = {k: v for k, v in tensors.items() if ".mlp.experts." not in k}
    for i in range(cfg.num_hidden_layers):
        q, ex = f"model.layers.{i}.mlp.experts", range(cfg.num_experts)
        out[f"{q}.gate_up_proj"] = torch.stack(
            [torch.cat([tensors[f"{q}.{e}.gate_proj.weight"], tensors[f"{q}.{e}.up_proj.weight"]]) for e in ex])
        out[f"{q}.down_proj"] = torch.stack([tensors[f"{q}.{e}.down_proj.weight"] for e in ex])
    return out
