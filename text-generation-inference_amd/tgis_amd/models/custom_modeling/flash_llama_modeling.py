"""Llama (MHA / GQA) forward for prefill and batched decode on the gfx950 kernels of libtgis_hip.so.

Mirrors custom_modeling/flash_llama_modeling.py of the reference — `LlamaConfig` (:37-99), `LlamaRMSNorm`
(:102-152), `FlashLlamaAttention` (:183-297), `LlamaMLP` (:300-335), `FlashLlamaLayer` (:338-395),
`FlashLlamaModel` (:398-497), `FlashLlamaForCausalLM` (:500-540) — with these deliberate differences:
  * the KV cache is the paged pool of utils/kv_cache.py instead of a per-batch contiguous tensor, so
    `forward` takes a `KVArgs` (block tables, context lengths, slots) where the reference takes
    `past_key_values` / `pre_allocate_past_size`;
  * RoPE, the KV write and the q/k/v split are one kernel; SiLU*mul is fused into down_proj's operand
    staging; every residual-add is fused into the following RMSNorm (as in the reference);
  * logits are produced in fp32.
Tensor-parallel sharding follows the reference exactly (heads split across ranks, qkv / gate_up
column-parallel, o_proj / down_proj row-parallel + all-reduce, vocab-parallel embedding and head)."""
from tgis_amd import native
from tgis_amd.models.custom_modeling.flash_common import (  # noqa: F401  (KVArgs is re-exported)
    FlashForCausalLM,
    KVArgs,
    attend,
    grow_max_positions,
    layer_pools,
    write_kv,
)
from tgis_amd.utils.layers import (
    PositionRotaryEmbedding,
    TensorParallelColumnLinear,
    TensorParallelEmbedding,
    TensorParallelHead,
    TensorParallelRowLinear,
)


class LlamaConfig:
    """The subset of the HF Llama config the forward needs (reference :37-99; eps default 1e-6 there)."""

    def __init__(self, vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32,
                 num_attention_heads=32, num_key_value_heads=None, hidden_act="silu", max_position_embeddings=2048,
                 rms_norm_eps=1e-6, rope_scaling=None, rope_theta=10000.0, attention_bias=False, mlp_bias=False,
                 pad_token_id=None, bos_token_id=1, eos_token_id=2, tie_word_embeddings=False, quantize=None,
                 **kwargs):
        self.vocab_size = vocab_size
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.num_key_value_heads = num_key_value_heads if num_key_value_heads is not None else num_attention_heads
        self.hidden_act = hidden_act
        self.max_position_embeddings = max_position_embeddings
        self.rms_norm_eps = rms_norm_eps
        self.rope_scaling = rope_scaling
        self.rope_theta = rope_theta
        self.attention_bias = attention_bias
        self.mlp_bias = mlp_bias
        self.pad_token_id = pad_token_id
        self.bos_token_id = bos_token_id
        self.eos_token_id = eos_token_id
        self.tie_word_embeddings = tie_word_embeddings
        self.quantize = quantize
        self.model_type = "llama"
        for k, v in kwargs.items():
            setattr(self, k, v)

    def to_dict(self):
        return dict(vars(self))


# (The persistent decode tail, the rope-in-attention launch and the norm-as-a-GEMM-phase launches of rounds 2 and 3 were all
# measured slower than the launches they replace: experiments/README.md is their ledger.)


def frag_rows(linear, rows: int, kv: "KVArgs", act: int = 0) -> bool:
    """Decode step of <= 64 rows in front of a linear that takes its operand in fragment order (native.FragAct)."""
    return kv.max_q_len == 1 and not kv.fresh_prefill and rows <= 64 and linear.wants_fragments(rows, act)


class LlamaRMSNorm:
    def __init__(self, prefix, weights, eps=1e-6):
        self.weight = weights.get_tensor(f"{prefix}.weight").contiguous()
        self.variance_epsilon = eps

    def forward(self, hidden_states, residual=None, frag: bool = False):
        # returns (normed, res) like the reference; res is hidden_states itself when residual is None
        # frag: the normed activation leaves in fragment order (native.FragAct) for the int4 GEMM behind it
        return native.rmsnorm_residual(hidden_states, residual, self.weight, self.variance_epsilon, frag=frag)

    __call__ = forward


def rope_settings(config):
    """(theta, linear scaling factor) from either config generation: `rope_theta` + `rope_scaling{type, factor}` (the
    reference's transformers 4.40, flash_llama_modeling.py:181-191) or `rope_parameters{rope_theta, rope_type, factor}`
    (transformers >= 5, which dropped the flat attributes)."""
    params = getattr(config, "rope_parameters", None) or {}
    theta = getattr(config, "rope_theta", None)
    if theta is None:
        theta = params.get("rope_theta", 10000.0)
    rs = getattr(config, "rope_scaling", None) or {}
    kind = rs.get("type") or rs.get("rope_type") or params.get("rope_type") or "default"
    if kind in ("default", None):
        return float(theta), 1.0
    if kind == "linear":
        return float(theta), float(rs.get("factor", params.get("factor", 1.0)))
    raise ValueError(f"rope_scaling of type {kind} is not supported")


def attention_biases(config):
    """(q/k/v bias, o_proj bias).  llama and mistral carry one switch, `attention_bias`, for all four projections; Qwen2 has a
    bias on q, k and v and none on o_proj, whatever its config says; Qwen3 follows its `attention_bias` (false in every
    released checkpoint) like llama."""
    if getattr(config, "model_type", None) == "qwen2":
        return True, False
    bias = bool(getattr(config, "attention_bias", False))  # (a Mistral config carries neither bias field)
    return bias, bias


def has_qk_norm(config) -> bool:
    """Qwen3: a per-head RMSNorm (self_attn.q_norm / k_norm, eps rms_norm_eps) between the qkv projection and the rotation."""
    return getattr(config, "model_type", None) == "qwen3"


class FlashLlamaAttention:
    def __init__(self, prefix: str, config, weights):
        self.num_heads = config.num_attention_heads
        self.hidden_size = config.hidden_size
        # (Mistral-Nemo: hidden 5120, 32 heads of `head_dim` 128; q_proj / o_proj are then [H head_dim, E] / [E, H head_dim])
        self.head_size = getattr(config, "head_dim", None) or self.hidden_size // self.num_heads
        theta, scaling = rope_settings(config)
        self.rotary_emb = PositionRotaryEmbedding.static(dim=self.head_size, base=theta,
                                                         device=weights.device, scaling_factor=scaling)
        self.softmax_scale = self.head_size ** -0.5
        tp = weights.process_group.size()
        if self.num_heads % tp != 0:
            raise ValueError(f"`num_heads` must be divisible by `num_shards` (got `num_heads`: {self.num_heads} "
                             f"and `num_shards`: {tp}")
        assert config.num_key_value_heads % tp == 0, "num_key_value_heads must be divisible by the shard count"
        self.num_heads = self.num_heads // tp
        self.num_key_value_heads = config.num_key_value_heads // tp
        qkv_bias, o_bias = attention_biases(config)
        self.query_key_value = TensorParallelColumnLinear.load_multi(
            config, prefixes=[f"{prefix}.q_proj", f"{prefix}.k_proj", f"{prefix}.v_proj"], dim=0, weights=weights,
            bias=qkv_bias)
        self.o_proj = TensorParallelRowLinear.load(config, prefix=f"{prefix}.o_proj", weights=weights, bias=o_bias)
        self.qk_norm = None
        if has_qk_norm(config):
            # [head_dim] each, the same on every tensor-parallel rank, never quantised.  The norm sits between the GEMM and
            # the rotation, so the GEMM + rope launch (and the fragment-order operands it is chosen with) cannot serve this
            # model: no rope heads are declared, every step takes write_kv, whose launches carry the norm.
            self.qk_norm = (weights.get_tensor(f"{prefix}.q_norm.weight").contiguous(),
                            weights.get_tensor(f"{prefix}.k_norm.weight").contiguous(), float(config.rms_norm_eps))
            if self.head_size not in (64, 96, 128):
                raise NotImplementedError(f"q_norm / k_norm with head_dim {self.head_size}: the kernels serve 64, 96 and 128")
        else:
            # where the linear has that launch, decode steps of up to 64 rows rotate q / k and write the cache in the GEMM
            # epilogue
            self.query_key_value.declare_rope_heads(self.num_heads, self.num_key_value_heads, self.head_size)

    def project_qkv(self, hidden_states, cos, sin, position_ids, cu_seqlens_q, layer_id: int, kv: KVArgs):
        """qkv GEMM, rotation of q and k in place, k and v scattered to their page slots (reference :251-268,282)."""
        H, Hkv, D = self.num_heads, self.num_key_value_heads, self.head_size
        if isinstance(hidden_states, native.FragAct) or (
                kv.slots is not None and not kv.fresh_prefill and kv.max_q_len == 1 and cos.shape[1] * 2 == D
                and self.query_key_value.rope_serves(hidden_states.shape[0])):
            # one launch: GEMM + rotary embedding + cache write
            k_pool, v_pool, scales = layer_pools(kv, layer_id)
            return self.query_key_value.forward_rope(hidden_states, cos, sin, position_ids, kv.slots, k_pool, v_pool,
                                                     **scales)
        # [T, (H + 2 Hkv) D]; at decode sizes the split-K sum of the GPTQ GEMM is finished inside the rope kernel
        qkv = self.query_key_value(hidden_states, partial=True)
        return write_kv(qkv, kv, layer_id, H, Hkv, D, D, cos, sin, position_ids, cu_seqlens_q, qk_norm=self.qk_norm)

    def attend(self, qkv, cu_seqlens_q, layer_id: int, kv: KVArgs):
        """Attention of the rotated q over the layer's cache pages (reference :271-295): [T, H D]."""
        # decode: the o_proj GEMM reads its operand in fragment order
        return attend(qkv, kv, layer_id, self.num_heads, self.num_key_value_heads, self.head_size, self.softmax_scale,
                      cu_seqlens_q, frag_out=frag_rows(self.o_proj, qkv.shape[0], kv))

    def forward(self, hidden_states, cos, sin, position_ids, cu_seqlens_q, layer_id: int, kv: KVArgs, lora=None):
        if lora is not None:
            return self.forward_lora(hidden_states, cos, sin, position_ids, cu_seqlens_q, layer_id, kv, lora)
        qkv = self.project_qkv(hidden_states, cos, sin, position_ids, cu_seqlens_q, layer_id, kv)
        attn_output = self.attend(qkv, cu_seqlens_q, layer_id, kv)
        # may be a native.Partial: the following fused add+RMSNorm finishes the split-K sum
        return self.o_proj(attn_output, partial=True)

    def forward_lora(self, hidden_states, cos, sin, position_ids, cu_seqlens_q, layer_id: int, kv: KVArgs, lora):
        """A step that carries adapter rows (utils/lora.py): the plain GEMMs, each followed by its delta, which must land
        before the rotation and before the add + norm — none of the fused forms."""
        H, Hkv, D = self.num_heads, self.num_key_value_heads, self.head_size
        qkv = self.query_key_value.forward_lora(hidden_states, lora)
        qkv = write_kv(qkv, kv, layer_id, H, Hkv, D, D, cos, sin, position_ids, cu_seqlens_q)
        attn_output = attend(qkv, kv, layer_id, H, Hkv, D, self.softmax_scale, cu_seqlens_q)
        return self.o_proj.forward_lora(attn_output, lora)

    __call__ = forward


class LlamaMLP:
    def __init__(self, prefix, config, weights):
        if config.hidden_act != "silu":
            raise NotImplementedError(f"hidden_act {config.hidden_act}: only silu is wired into the fused kernel")
        mlp_bias = getattr(config, "mlp_bias", False)
        self.gate_up_proj = TensorParallelColumnLinear.load_multi(
            config, prefixes=[f"{prefix}.gate_proj", f"{prefix}.up_proj"], weights=weights, dim=0, bias=mlp_bias)
        self.down_proj = TensorParallelRowLinear.load(config, prefix=f"{prefix}.down_proj", weights=weights, bias=mlp_bias)
        self.intermediate_size = config.intermediate_size // weights.process_group.size()
        # GPTQ: SiLU(gate)*up runs in the gate_up GEMM epilogue (columns interleaved at prepare time);
        # dense: it runs while down_proj stages its operand.  Reference: eager ops at :332-335.
        self.fused_epilogue = self.intermediate_size % 16 == 0 and self.gate_up_proj.fuse_gate_up()

    def forward(self, hidden_states, lora=None):
        if lora is not None:
            # unfused [T, 2 I] -> delta -> SiLU * up -> down_proj on the activated tensor, the operand of its shrink too
            gate_up_states = self.gate_up_proj.forward_lora(hidden_states, lora)
            act = native.act_mul(gate_up_states, self.intermediate_size)
            return self.down_proj.forward_lora(act, lora)
        if self.fused_epilogue:
            if isinstance(hidden_states, native.FragAct):  # decode: SiLU * up leaves in the layout down_proj reads
                rows = hidden_states.shape[0]
                act = self.gate_up_proj(hidden_states, out_frag=self.down_proj.wants_fragments(rows))
                return self.down_proj(act, partial=True)
            act = self.gate_up_proj(hidden_states)  # [T, I], already silu(gate) * up
            return self.down_proj(act, partial=True)
        gate_up_states = self.gate_up_proj(hidden_states)  # [T, 2, I]
        return self.down_proj(gate_up_states, act=1, partial=True)

    __call__ = forward


class FlashLlamaLayer:
    def __init__(self, layer_id, config, weights):
        prefix = f"model.layers.{layer_id}"
        self.layer_id = layer_id
        self.self_attn = FlashLlamaAttention(prefix=f"{prefix}.self_attn", config=config, weights=weights)
        self.mlp = LlamaMLP(prefix=f"{prefix}.mlp", config=config, weights=weights)
        self.input_layernorm = LlamaRMSNorm(prefix=f"{prefix}.input_layernorm", weights=weights,
                                            eps=config.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNorm(prefix=f"{prefix}.post_attention_layernorm", weights=weights,
                                                     eps=config.rms_norm_eps)

    def forward(self, hidden_states, residual, cos, sin, position_ids, cu_seqlens_q, kv: KVArgs, lora=None):
        if lora is not None:  # (utils/lora.py LoraArgs: row-major activations throughout, the shrink reads them)
            normed_hidden_states, res = self.input_layernorm(hidden_states, residual)
            attn_output = self.self_attn(normed_hidden_states, cos, sin, position_ids, cu_seqlens_q, self.layer_id, kv, lora)
            normed_attn_res_output, attn_res = self.post_attention_layernorm(attn_output, res)
            return self.mlp(normed_attn_res_output, lora), attn_res
        rows = hidden_states.shape[0]
        att = self.self_attn
        # decode steps of <= 64 rows hand the int4 GEMMs their operands in fragment order (native.FragAct): the qkv + rotary
        # launch when it serves the step, the MLP when the SiLU * up epilogue does
        qkv_frag = (kv.slots is not None and cos.shape[1] * 2 == att.head_size
                    and frag_rows(att.query_key_value, rows, kv, act=3))
        normed_hidden_states, res = self.input_layernorm(hidden_states, residual, frag=qkv_frag)
        attn_output = att(normed_hidden_states, cos, sin, position_ids, cu_seqlens_q, self.layer_id, kv)
        mlp_frag = self.mlp.fused_epilogue and frag_rows(self.mlp.gate_up_proj, rows, kv, act=2)
        normed_attn_res_output, attn_res = self.post_attention_layernorm(attn_output, res, frag=mlp_frag)
        mlp_output = self.mlp(normed_attn_res_output)
        return mlp_output, attn_res

    __call__ = forward


class FlashLlamaModel:
    def __init__(self, config, weights):
        self.config = config
        process_group = weights.process_group
        self.tp_rank = process_group.rank()
        self.tp_world_size = process_group.size()
        self.embed_tokens = TensorParallelEmbedding(prefix="model.embed_tokens", weights=weights)
        self.layers = [FlashLlamaLayer(i, config, weights) for i in range(config.num_hidden_layers)]
        self.norm = LlamaRMSNorm(prefix="model.norm", weights=weights, eps=config.rms_norm_eps)
        self.head_size = self.layers[0].self_attn.head_size
        self.num_heads = self.layers[0].self_attn.num_heads
        self.num_key_value_heads = config.num_key_value_heads // process_group.size()
        self.max_positions = 0

    def rope_tables(self, dtype, device, max_s: int):
        self.max_positions = grow_max_positions(self.config, self.max_positions, max_s)
        return self.layers[0].self_attn.rotary_emb.tables(dtype, device, self.max_positions)

    def forward(self, input_ids, position_ids, cu_seqlens_q, max_s, inputs_embeds, kv: KVArgs, lora=None):
        hidden_states = inputs_embeds if inputs_embeds is not None else self.embed_tokens(input_ids)
        cos, sin = self.rope_tables(hidden_states.dtype, hidden_states.device, max_s)
        residual = None
        for layer in self.layers:
            hidden_states, residual = layer(hidden_states, residual, cos, sin, position_ids, cu_seqlens_q, kv, lora)
        hidden_states, _ = self.norm(hidden_states, residual)
        return hidden_states

    __call__ = forward


class FlashLlamaForCausalLM(FlashForCausalLM):
    def __init__(self, config, weights):
        self.config = config
        self.model = FlashLlamaModel(config, weights)
        self.lm_head = TensorParallelHead.load(config, prefix="lm_head", weights=weights)
        self.collect_linears((layer.self_attn.query_key_value, layer.self_attn.o_proj, layer.mlp.gate_up_proj,
                              layer.mlp.down_proj) for layer in self.model.layers)

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def enable_lora(self, slots: int, max_rank: int, dtype, device):
        """Before post_init: wraps the four projections of every layer in a utils.lora.LoraLinear with `slots` adapter
        slots (allocated here, once) and takes the SiLU * up epilogue out of gate_up, whose delta must land in front of it.
        Returns the wrappers."""
        from tgis_amd.utils.lora import LoraLinear

        cfg, wrapped = self.config, []
        for layer in self.model.layers:
            att, mlp = layer.self_attn, layer.mlp
            E, q, kvw, inter = cfg.hidden_size, att.num_heads * att.head_size, att.num_key_value_heads * att.head_size, \
                mlp.intermediate_size
            mlp.gate_up_proj.linear.unfuse_gate_up()
            mlp.fused_epilogue = False

            def wrap(proj, modules, bounds, K):
                w = LoraLinear(proj, layer.layer_id, modules, bounds, K, slots, max_rank, dtype, device)
                wrapped.append(w)
                return w

            att.query_key_value = wrap(att.query_key_value, ("q_proj", "k_proj", "v_proj"), (0, q, q + kvw, q + 2 * kvw), E)
            att.o_proj = wrap(att.o_proj, ("o_proj",), (0, E), q)
            mlp.gate_up_proj = wrap(mlp.gate_up_proj, ("gate_proj", "up_proj"), (0, inter, 2 * inter), E)
            mlp.down_proj = wrap(mlp.down_proj, ("down_proj",), (0, E), inter)
        return wrapped
