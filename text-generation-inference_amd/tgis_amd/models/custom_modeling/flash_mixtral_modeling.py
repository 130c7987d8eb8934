"""Mixtral forward for prefill and batched decode: Llama's attention, norms, rotary tables and cache (flash_llama_modeling.py,
unchanged) around a routed expert MLP on the kernels of csrc/moe.hip.

The reference project has no Mixtral; transformers' `MixtralSparseMoeBlock` (models/mixtral/modeling_mixtral.py) is what
`MixtralSparseMoe` mirrors: a router (softmax over all experts in fp32, the top `num_experts_per_tok`, renormalised) and
`num_local_experts` SiLU MLPs of which every token runs the chosen ones, their outputs scaled by the routing weights.

One forward of the block is four launches — router GEMM, route, up, down — that read the routing on the device only, so a
captured decode or verify step holds them.  The same function has a second implementation, the loop path: one host read of
the expert counts, then for each expert that was hit index_select, the dense act 2 and plain GEMMs on that expert's image,
a scale and index_add_ in fp32.  Captured steps always take the kernels; an eager forward takes them up to
MOE_FUSED_MAX_TOKENS tokens (MOE_GPTQ_FUSED_MAX_TOKENS for GPTQ experts) and the loop above (TGIS_MOE_PATH=fused / loop
forces either on eager forwards).

GPTQ checkpoints (4 bits, one group or groups of 64 * 2^n rows, no act-order; q/k/v/o as Llama's): every expert's w1 | w3 and
w2 are int4 images (native.MoeGptqWeights) and the block takes native.moe_gptq_gemm_up / _down, the same kernel over another
weight source; its loop path runs gptq_gemm(act=2) and gptq_gemm on views of the same images.  The router stays 16-bit.

Tensor parallelism: every expert's intermediate size is split across ranks (w1 and w3 by rows, w2 by columns, as Llama's
MLP), the router is replicated, and the block's output is all-reduced once."""
import os

import torch
import torch.distributed

from tgis_amd import native
from tgis_amd.models.custom_modeling.flash_common import FlashForCausalLM, KVArgs, grow_max_positions
from tgis_amd.models.custom_modeling.flash_llama_modeling import FlashLlamaAttention, LlamaRMSNorm
from tgis_amd.utils.graph_segments import collective
from tgis_amd.utils.layers import DEFER_REDUCE, TensorParallelEmbedding, TensorParallelHead, workspace

# tokens up to which an eager forward takes the routed kernels; above, the loop path.  Measured on 8x7B layer shapes
# (profiles/mixtral_bench.jsonl): the kernels win at 64 rows (0.50 against 0.81 ms) and lose at 128
# (0.86 against 0.79 ms) — they re-read an expert's weights once per 32 of its rows, the loop's GEMMs once per 64.
MOE_FUSED_MAX_TOKENS = int(os.getenv("TGIS_MOE_FUSED_MAX_TOKENS", "64"))
# the same threshold for GPTQ experts.  It differs because the int4 crossover does: on the same shapes
# (profiles/mixtral_gptq_bench.jsonl) the int4 kernels still win at 128 rows (0.48 against 0.55 - 0.66 ms for the loop, whose
# per-expert gptq_gemm launches and host read cost what they cost at f16 while the kernels read a quarter of the bytes) and
# lose at 256 (0.93 against 0.76 ms).
MOE_GPTQ_FUSED_MAX_TOKENS = int(os.getenv("TGIS_MOE_GPTQ_FUSED_MAX_TOKENS", "128"))


def moe_path_override():
    """TGIS_MOE_PATH = fused | loop forces one implementation on eager forwards (tests, A/B runs); unset / auto: the rule."""
    v = os.getenv("TGIS_MOE_PATH", "auto").lower()
    if v not in ("auto", "fused", "loop"):
        raise ValueError(f"TGIS_MOE_PATH must be auto, fused or loop, got {v!r}")
    return None if v == "auto" else v


def gptq_params_of(weights):
    """(bits, group size) of a GPTQ checkpoint as its weights object knows them before any weight is read, or None."""
    get = getattr(weights, "_get_gptq_params", None)
    if get is None:
        return None
    try:
        bits, groupsize = get()
    except (RuntimeError, AttributeError, TypeError):
        return None
    return (bits, groupsize) if isinstance(bits, int) and isinstance(groupsize, int) else None


def refuse_gptq(what: str):
    raise NotImplementedError(f"Mixtral: GPTQ checkpoints are served at 4 bits, one group or groups of 64 * 2^n rows, "
                              f"without act-order, under the published tensor names: {what}")


def check_mixtral_config(config, quantize=None, gptq_params=None):
    """(E, top_k) of a Mixtral config, or the refusal: a GPTQ form without a kernel, another activation, expert counts the
    route kernel has no form for.  Called before any weight is read; gptq_params = (bits, group size) of a GPTQ checkpoint
    (gptq_params_of), None when they are not known."""
    if quantize == "gptq":
        if gptq_params is None:
            refuse_gptq("the bits and group size of this checkpoint are not known")
        bits, groupsize = gptq_params
        if bits != 4:
            refuse_gptq(f"{bits}-bit experts have no kernel")
        if not native.moe_gptq_group_ok(groupsize):
            refuse_gptq(f"groups of {groupsize} rows have no form in the expert kernels")
    elif quantize is not None:
        raise NotImplementedError(f"Mixtral: quantization `{quantize}` is not implemented")
    act = getattr(config, "hidden_act", None)
    if act != "silu":
        raise NotImplementedError(f"Mixtral: hidden_act {act!r}: only silu is wired into the expert kernels")
    E, top_k = getattr(config, "num_local_experts", None), getattr(config, "num_experts_per_tok", None)
    if not isinstance(E, int) or not isinstance(top_k, int) or not 2 <= E <= 64 or not 1 <= top_k <= min(E, 8):
        raise NotImplementedError(f"Mixtral: num_local_experts {E!r} / num_experts_per_tok {top_k!r} are not served "
                                  "(2 <= experts <= 64, 1 <= experts per token <= min(experts, 8))")
    return E, top_k


class ExpertTensors:
    """Where a layer's expert tensors are in a checkpoint, under either naming, sliced for this rank:
      published   {prefix}.block_sparse_moe.gate.weight, ...experts.{e}.w1 / w3 / w2 .weight (gate, up, down)
      fused       {prefix}.mlp.gate.weight, ...mlp.experts.gate_up_proj [E, 2 I, hidden], ...mlp.experts.down_proj [E, hidden, I]
                  (transformers >= 5 in memory; what it saves carries the published names again)."""

    def __init__(self, prefix: str, weights, I: int, quantize=None):
        self.weights, self.I, self.quantize = weights, I, quantize
        tp, self.rank = weights.process_group.size(), weights.process_group.rank()
        if I % tp != 0:
            raise ValueError(f"intermediate_size {I} must be divisible by the shard count {tp}")
        self.Il = I // tp
        self.published = weights.has(f"{prefix}.block_sparse_moe.gate.weight")
        self.base = f"{prefix}.block_sparse_moe" if self.published else f"{prefix}.mlp"
        if not self.published and not weights.has(f"{self.base}.experts.gate_up_proj"):
            raise RuntimeError(f"weight {prefix}.block_sparse_moe.gate.weight does not exist (nor {self.base}.experts.gate_up_proj)")
        if quantize == "gptq" and not self.published:
            refuse_gptq(f"{self.base}.experts carries the fused in-memory names, which hold no GPTQ tensors")
        self._fused = {}

    def router(self) -> torch.Tensor:
        return self.weights.get_tensor(f"{self.base}.gate.weight")

    def _fused_full(self, name: str) -> torch.Tensor:
        if name not in self._fused:
            self._fused[name] = self.weights._full(f"{self.base}.experts.{name}")
        return self._fused[name]

    def gate_up(self, e: int) -> torch.Tensor:
        """[2 I / tp, hidden]: this rank's rows of w1, then of w3."""
        w = self.weights
        if self.published:
            return torch.cat([w.get_sharded(f"{self.base}.experts.{e}.w1.weight", dim=0),
                              w.get_sharded(f"{self.base}.experts.{e}.w3.weight", dim=0)], dim=0)
        full, lo = self._fused_full("gate_up_proj")[e], self.rank * self.Il
        return w._finish(torch.cat([full[lo:lo + self.Il], full[self.I + lo:self.I + lo + self.Il]], dim=0))

    def down(self, e: int) -> torch.Tensor:
        """[hidden, I / tp]: this rank's columns of w2."""
        w = self.weights
        if self.published:
            return w.get_sharded(f"{self.base}.experts.{e}.w2.weight", dim=1)
        lo = self.rank * self.Il
        return w._finish(self._fused_full("down_proj")[e][:, lo:lo + self.Il])


    def _gptq_bundle(self, name: str, bundle):
        """(qweight, qzeros, scales, g_idx, bits, groupsize) of one expert matrix as Llama's MLP loader sliced (and, for a
        row shard, regrouped) it, or the refusal of what the expert kernels have no form for, naming the tensor."""
        qweight, qzeros, scales, g_idx, bits, groupsize = bundle[:6]
        K, G = qweight.shape[0] * (32 // bits), qzeros.shape[0]
        if bits != 4:
            refuse_gptq(f"{name} holds {bits}-bit codes")
        if g_idx is not None:
            trivial = not isinstance(g_idx, tuple) and g_idx.numel() == K and K % G == 0
            if trivial:
                gi = g_idx.to("cpu", torch.int64)
                trivial = torch.equal(gi, torch.arange(K) // (K // G)) or (G == 1 and not bool(gi.any()))
            if not trivial:
                refuse_gptq(f"{name} is an act-order matrix (its g_idx permutes the rows)")
        if K % 64 != 0 or K % G != 0 or not native.moe_gptq_group_ok(K // G, K):
            refuse_gptq(f"{name}: {K} rows per rank in {G} groups (the checkpoint's group size is {groupsize})")
        return qweight, qzeros, scales, g_idx, bits, K // G

    def gate_up_gptq(self, e: int):
        """The GPTQ bundle of [w1 | w3]: this rank's columns of each, side by side (Llama's gate_up_proj read)."""
        names = [f"{self.base}.experts.{e}.w1", f"{self.base}.experts.{e}.w3"]
        return self._gptq_bundle(names[0] + " | w3", self.weights.get_multi_weights_col(names, "gptq", dim=1))

    def down_gptq(self, e: int):
        """The GPTQ bundle of w2: this rank's rows (Llama's down_proj read, regrouped when a group straddles the ranks)."""
        name = f"{self.base}.experts.{e}.w2"
        return self._gptq_bundle(name, self.weights.get_multi_weights_row(name, "gptq"))


class ExpertWeights:
    """The expert weights of one layer as the kernels read them: the gate|up images and the down images of all experts
    (native.MoeWeights: E calls of tgis_dense_prepare into one buffer each; native.MoeGptqWeights and tgis_gptq_prepare for
    a GPTQ checkpoint).  The checkpoint-layout tensors are released as their images are made."""

    def __init__(self, tensors: ExpertTensors, E: int):
        if tensors.Il % 16 != 0:
            raise NotImplementedError(f"Mixtral: intermediate size per rank ({tensors.Il}) must be a multiple of 16")
        if tensors.quantize == "gptq":
            self.gate_up = native.MoeGptqWeights(tensors.gate_up_gptq, E, gate_up=True)
            self.down = native.MoeGptqWeights(tensors.down_gptq, E)
        else:
            self.gate_up = native.MoeWeights(tensors.gate_up, E, gate_up=True)
            self.down = native.MoeWeights(tensors.down, E)
        # one expert's images as dense weights (views): the loop path's operands
        self.gate_up_experts = [self.gate_up.expert(e) for e in range(E)]
        self.down_experts = [self.down.expert(e) for e in range(E)]


class MixtralSparseMoe:
    def __init__(self, prefix: str, config, weights):
        self.quantize = getattr(config, "quantize", None)
        self.E, self.top_k = check_mixtral_config(config, self.quantize, gptq_params_of(weights))
        self.hidden = config.hidden_size
        if self.hidden % 8 != 0:
            raise NotImplementedError(f"Mixtral: hidden_size {self.hidden} must be a multiple of 8")
        self.process_group = weights.process_group
        tensors = ExpertTensors(prefix, weights, config.intermediate_size, self.quantize)
        self.router = native.DenseWeight(tensors.router().contiguous())  # replicated
        assert (self.router.N, self.router.K) == (self.E, self.hidden)
        self.experts = ExpertWeights(tensors, self.E)
        tensors._fused.clear()

    def route(self, x: torch.Tensor) -> native.Routing:
        logits = native.dense_gemm(x, self.router, workspace(x.device), out_f32=True)
        return native.moe_route(logits, self.top_k)

    def fused(self, x: torch.Tensor, r: native.Routing, partial: bool):
        if self.quantize == "gptq":
            h = native.moe_gptq_gemm_up(x, self.experts.gate_up, r)
            return native.moe_gptq_gemm_down(h, self.experts.down, r, partial=partial)
        h = native.moe_gemm_up(x, self.experts.gate_up, r)
        return native.moe_gemm_down(h, self.experts.down, r, partial=partial)

    def loop(self, x: torch.Tensor, r: native.Routing) -> torch.Tensor:
        E, k = self.E, self.top_k
        lists = r.lists.tolist()  # the one host read: counts and offsets
        counts, offsets = lists[:E], lists[E:]
        ws = workspace(x.device)
        out = torch.zeros((x.shape[0], self.hidden), dtype=torch.float32, device=x.device)
        flat_w = r.expert_w.view(-1)
        for e in range(E):
            if counts[e] == 0:
                continue
            slots = r.slot_rows[offsets[e]:offsets[e + 1]].long()
            tokens = torch.div(slots, k, rounding_mode="floor")  # (distinct inside one expert: the adds below never collide)
            if self.quantize == "gptq":  # the int4 GEMM leaves f16: scaled and added in fp32 all the same
                h = native.gptq_gemm(x.index_select(0, tokens), self.experts.gate_up_experts[e], ws, act=2)
                y = native.gptq_gemm(h, self.experts.down_experts[e], ws).float()
            else:
                h = native.dense_gemm(x.index_select(0, tokens), self.experts.gate_up_experts[e], ws, act=2)
                y = native.dense_gemm(h, self.experts.down_experts[e], ws, out_f32=True)
            out.index_add_(0, tokens, y * flat_w.index_select(0, slots).unsqueeze(1))
        return out.to(x.dtype)

    def forward(self, x: torch.Tensor):
        """[T, hidden], or (one rank, up to PARTIAL_MAX_M tokens on the kernels) a native.Partial of top_k slabs whose sum the
        next add + RMSNorm finishes."""
        T = x.shape[0]
        tp = self.process_group.size()
        use_fused = T <= (MOE_GPTQ_FUSED_MAX_TOKENS if self.quantize == "gptq" else MOE_FUSED_MAX_TOKENS)
        if torch.cuda.is_current_stream_capturing():
            use_fused = True  # a captured step cannot read the routing
        else:
            forced = moe_path_override()
            if forced is not None:
                use_fused = forced == "fused"
        r = self.route(x)
        if not use_fused:
            out = self.loop(x, r)
        else:
            out = self.fused(x, r, partial=tp == 1 and DEFER_REDUCE and T <= native.PARTIAL_MAX_M)
        if tp > 1:
            pg = self.process_group
            collective(lambda t=out: torch.distributed.all_reduce(t, group=pg))
        return out

    __call__ = forward


class FlashMixtralLayer:
    def __init__(self, layer_id, config, weights):
        prefix = f"model.layers.{layer_id}"
        self.layer_id = layer_id
        self.self_attn = FlashLlamaAttention(prefix=f"{prefix}.self_attn", config=config, weights=weights)
        self.moe = MixtralSparseMoe(prefix, config, weights)
        self.input_layernorm = LlamaRMSNorm(prefix=f"{prefix}.input_layernorm", weights=weights, eps=config.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNorm(prefix=f"{prefix}.post_attention_layernorm", weights=weights,
                                                     eps=config.rms_norm_eps)

    def forward(self, hidden_states, residual, cos, sin, position_ids, cu_seqlens_q, kv: KVArgs):
        normed, res = self.input_layernorm(hidden_states, residual)
        attn_output = self.self_attn(normed, cos, sin, position_ids, cu_seqlens_q, self.layer_id, kv)
        normed_attn_res, attn_res = self.post_attention_layernorm(attn_output, res)
        return self.moe(normed_attn_res), attn_res

    __call__ = forward


class FlashMixtralModel:
    def __init__(self, config, weights):
        self.config = config
        process_group = weights.process_group
        self.tp_rank = process_group.rank()
        self.tp_world_size = process_group.size()
        self.embed_tokens = TensorParallelEmbedding(prefix="model.embed_tokens", weights=weights)
        self.layers = [FlashMixtralLayer(i, config, weights) for i in range(config.num_hidden_layers)]
        self.norm = LlamaRMSNorm(prefix="model.norm", weights=weights, eps=config.rms_norm_eps)
        self.head_size = self.layers[0].self_attn.head_size
        self.num_heads = self.layers[0].self_attn.num_heads
        self.num_key_value_heads = config.num_key_value_heads // process_group.size()
        self.max_positions = 0

    def rope_tables(self, dtype, device, max_s: int):
        self.max_positions = grow_max_positions(self.config, self.max_positions, max_s)
        return self.layers[0].self_attn.rotary_emb.tables(dtype, device, self.max_positions)

    def forward(self, input_ids, position_ids, cu_seqlens_q, max_s, inputs_embeds, kv: KVArgs):
        hidden_states = inputs_embeds if inputs_embeds is not None else self.embed_tokens(input_ids)
        cos, sin = self.rope_tables(hidden_states.dtype, hidden_states.device, max_s)
        residual = None
        for layer in self.layers:
            hidden_states, residual = layer(hidden_states, residual, cos, sin, position_ids, cu_seqlens_q, kv)
        hidden_states, _ = self.norm(hidden_states, residual)
        return hidden_states

    __call__ = forward


class FlashMixtralForCausalLM(FlashForCausalLM):
    def __init__(self, config, weights):
        check_mixtral_config(config, getattr(config, "quantize", None), gptq_params_of(weights))  # before any weight is read
        if not hasattr(config, "num_key_value_heads") or config.num_key_value_heads is None:
            config.num_key_value_heads = config.num_attention_heads
        self.config = config
        self.model = FlashMixtralModel(config, weights)
        self.lm_head = TensorParallelHead.load(config, prefix="lm_head", weights=weights)
        # the expert weights are held by ExpertWeights, not by linears
        self.collect_linears((layer.self_attn.query_key_value, layer.self_attn.o_proj) for layer in self.model.layers)

    def get_input_embeddings(self):
        return self.model.embed_tokens
