"""Qwen3-MoE (model_type "qwen3_moe": Qwen3-30B-A3B, Qwen3-235B-A22B) forward for prefill and batched decode: Qwen3's
attention (flash_llama_modeling.py: explicit head_dim, per-head q / k RMSNorm in the rope + cache launches) around a routed
expert MLP of up to 128 experts on the kernels of csrc/moe_tiles.h.

The reference project has no such model; transformers' `Qwen3MoeSparseMoeBlock` (models/qwen3_moe/modeling_qwen3_moe.py) is
what `Qwen3MoeSparseMoe` mirrors: a router (softmax over all `num_experts` in fp32, the top `num_experts_per_tok`,
renormalised when `norm_topk_prob` is true and left as they are otherwise) and `num_experts` SiLU MLPs of
`moe_intermediate_size`, of which every token runs the chosen ones.

One forward of the block is the router GEMM, native.moe_route_tiles (three launches that leave the routing and a tile list on
the device) and the two tile GEMMs.  Nothing is read on the host, whatever the token count, so decode steps are captured and
prefills never leave HIP.  A prefill of more than MOE_CHUNK_TOKENS tokens runs the block chunk by chunk — a plain host loop —
so that the fp32 rows the down GEMM leaves for its fixed-order sum (tokens x top_k x hidden x 4 bytes) stay bounded.

The expert weights are native.MoeWeights, the images Mixtral's kernels read; there is no second copy.  Tensor parallelism as
Mixtral's: every expert's moe_intermediate_size is split across ranks, the router is replicated, the output all-reduced once."""
import os

import torch
import torch.distributed

from tgis_amd import native
from tgis_amd.models.custom_modeling.flash_common import FlashForCausalLM, KVArgs
from tgis_amd.models.custom_modeling.flash_llama_modeling import FlashLlamaAttention, LlamaRMSNorm, rope_settings
from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors, FlashMixtralModel
from tgis_amd.utils.graph_segments import collective
from tgis_amd.utils.layers import DEFER_REDUCE, TensorParallelHead, workspace

# tokens of one pass of the routed block: 4096 x 8 x 2048 x 4 bytes = 256 MiB of fp32 rows at Qwen3-30B-A3B's shapes
MOE_CHUNK_TOKENS = int(os.getenv("TGIS_MOE_CHUNK_TOKENS", "4096"))
MAX_EXPERTS, MAX_TOP_K = 128, 8


def refuse(what: str):
    raise NotImplementedError(f"Qwen3-MoE: {what}")


def check_qwen3_moe_config(config, quantize=None):
    """(E, top_k, renorm) of a Qwen3-MoE config, or the refusal, by name, of what has no kernel or no launch here.  Called
    by the dispatch (model_class_for) and again by the model class, both before any weight is read."""
    if quantize == "gptq":
        refuse("quantize=\"gptq\" is not served: the tile GEMMs read 16-bit expert images only")
    if quantize is not None:
        refuse(f"quantization `{quantize}` is not implemented")
    E, top_k = getattr(config, "num_experts", None), getattr(config, "num_experts_per_tok", None)
    if E is None or top_k is None:
        refuse("the config carries no num_experts / num_experts_per_tok, which every qwen3_moe config.json has (dense Qwen "
               "checkpoints are the model types qwen2 / qwen3)")
    if getattr(config, "decoder_sparse_step", 1) != 1:
        refuse(f"decoder_sparse_step {config.decoder_sparse_step!r}: every layer must be a routed block (decoder_sparse_step 1)")
    if getattr(config, "mlp_only_layers", None):
        refuse(f"mlp_only_layers {config.mlp_only_layers!r}: dense layers between the routed ones are not served")
    act = getattr(config, "hidden_act", None)
    if act != "silu":
        refuse(f"hidden_act {act!r}: only silu is wired into the expert kernels")
    if getattr(config, "use_sliding_window", False):
        refuse("use_sliding_window = true is not served: per-layer windows are out of scope (DESIGN.md section 8)")
    try:
        rope_settings(config)
    except ValueError as err:
        refuse(f"{err} (rope scalings other than linear are not served)")
    if not isinstance(E, int) or not isinstance(top_k, int) or not 2 <= E <= MAX_EXPERTS or not 1 <= top_k <= min(E, MAX_TOP_K):
        refuse(f"num_experts {E!r} / num_experts_per_tok {top_k!r} are not served (2 <= experts <= {MAX_EXPERTS}, "
               f"1 <= experts per token <= min(experts, {MAX_TOP_K}))")
    I = getattr(config, "moe_intermediate_size", None)
    if not isinstance(I, int) or I < 16:
        refuse(f"moe_intermediate_size {I!r} must be a positive multiple of 16 per rank")
    return E, top_k, bool(getattr(config, "norm_topk_prob", False))


class Qwen3MoeExpertTensors(ExpertTensors):
    """ExpertTensors under Qwen3-MoE's names, both beneath {prefix}.mlp:
      published   gate.weight, experts.{e}.gate_proj / up_proj / down_proj .weight
      fused       gate.weight, experts.gate_up_proj [E, 2 I, hidden], experts.down_proj [E, hidden, I] (transformers >= 5 in
                  memory; Mixtral's fused form, read by the base class)."""

    def __init__(self, prefix: str, weights, I: int):
        self.weights, self.I, self.quantize = weights, I, None
        tp, self.rank = weights.process_group.size(), weights.process_group.rank()
        if I % tp != 0:
            raise ValueError(f"moe_intermediate_size {I} must be divisible by the shard count {tp}")
        self.Il = I // tp
        self.base = f"{prefix}.mlp"
        self.published = weights.has(f"{self.base}.experts.0.gate_proj.weight")
        if not self.published and not weights.has(f"{self.base}.experts.gate_up_proj"):
            raise RuntimeError(f"weight {self.base}.experts.0.gate_proj.weight does not exist (nor {self.base}.experts.gate_up_proj)")
        self._fused = {}

    def gate_up(self, e: int) -> torch.Tensor:
        if not self.published:
            return super().gate_up(e)
        w = self.weights
        return torch.cat([w.get_sharded(f"{self.base}.experts.{e}.gate_proj.weight", dim=0),
                          w.get_sharded(f"{self.base}.experts.{e}.up_proj.weight", dim=0)], dim=0)

    def down(self, e: int) -> torch.Tensor:
        if not self.published:
            return super().down(e)
        return self.weights.get_sharded(f"{self.base}.experts.{e}.down_proj.weight", dim=1)


class Qwen3MoeSparseMoe:
    def __init__(self, prefix: str, config, weights):
        self.E, self.top_k, self.renorm = check_qwen3_moe_config(config, getattr(config, "quantize", None))
        self.hidden = config.hidden_size
        if self.hidden % 8 != 0:
            refuse(f"hidden_size {self.hidden} must be a multiple of 8")
        self.process_group = weights.process_group
        tensors = Qwen3MoeExpertTensors(prefix, weights, config.moe_intermediate_size)
        if tensors.Il % 16 != 0:
            refuse(f"moe_intermediate_size per rank ({tensors.Il}) must be a multiple of 16")
        self.router = native.DenseWeight(tensors.router().contiguous())  # replicated
        assert (self.router.N, self.router.K) == (self.E, self.hidden)
        self.gate_up = native.MoeWeights(tensors.gate_up, self.E, gate_up=True)
        self.down = native.MoeWeights(tensors.down, self.E)
        tensors._fused.clear()

    def route(self, x: torch.Tensor) -> native.Routing:
        logits = native.dense_gemm(x, self.router, workspace(x.device), out_f32=True)
        return native.moe_route_tiles(logits, self.top_k, renorm=self.renorm)

    def block(self, x: torch.Tensor, partial: bool):
        r = self.route(x)
        h = native.moe_tile_gemm_up(x, self.gate_up, r)
        return native.moe_tile_gemm_down(h, self.down, r, partial=partial)

    def forward(self, x: torch.Tensor):
        """[T, hidden], or (one rank, one chunk of up to PARTIAL_MAX_M tokens) a native.Partial of top_k slabs whose sum the
        next add + RMSNorm finishes."""
        T = x.shape[0]
        tp = self.process_group.size()
        if T <= MOE_CHUNK_TOKENS:
            out = self.block(x, partial=tp == 1 and DEFER_REDUCE and T <= native.PARTIAL_MAX_M)
        else:
            out = torch.cat([self.block(x[t0:t0 + MOE_CHUNK_TOKENS], partial=False) for t0 in range(0, T, MOE_CHUNK_TOKENS)])
        if tp > 1:
            pg = self.process_group
            collective(lambda t=out: torch.distributed.all_reduce(t, group=pg))
        return out

    __call__ = forward


class FlashQwen3MoeLayer:
    def __init__(self, layer_id, config, weights):
        prefix = f"model.layers.{layer_id}"
        self.layer_id = layer_id
        self.self_attn = FlashLlamaAttention(prefix=f"{prefix}.self_attn", config=config, weights=weights)
        self.moe = Qwen3MoeSparseMoe(prefix, config, weights)
        self.input_layernorm = LlamaRMSNorm(prefix=f"{prefix}.input_layernorm", weights=weights, eps=config.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNorm(prefix=f"{prefix}.post_attention_layernorm", weights=weights,
                                                     eps=config.rms_norm_eps)

    def forward(self, hidden_states, residual, cos, sin, position_ids, cu_seqlens_q, kv: KVArgs):
        normed, res = self.input_layernorm(hidden_states, residual)
        attn_output = self.self_attn(normed, cos, sin, position_ids, cu_seqlens_q, self.layer_id, kv)
        normed_attn_res, attn_res = self.post_attention_layernorm(attn_output, res)
        return self.moe(normed_attn_res), attn_res

    __call__ = forward


class FlashQwen3MoeModel(FlashMixtralModel):
    """FlashMixtralModel's embedding, rope tables, layer walk and final norm over FlashQwen3MoeLayer."""
    layer_class = FlashQwen3MoeLayer


class FlashQwen3MoeForCausalLM(FlashForCausalLM):
    def __init__(self, config, weights):
        check_qwen3_moe_config(config, getattr(config, "quantize", None))  # before any weight is read
        if not hasattr(config, "num_key_value_heads") or config.num_key_value_heads is None:
            config.num_key_value_heads = config.num_attention_heads
        self.config = config
        self.model = FlashQwen3MoeModel(config, weights)
        self.lm_head = TensorParallelHead.load(config, prefix="lm_head", weights=weights)
        # the expert weights are held by native.MoeWeights, not by linears
        self.collect_linears((layer.self_attn.query_key_value, layer.self_attn.o_proj) for layer in self.model.layers)

    def get_input_embeddings(self):
        return self.model.embed_tokens
