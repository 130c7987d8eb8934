"""GPT-NeoX (gpt-neox-20b, Pythia) forward for prefill and batched decode on the gfx950 kernels of libtgis_hip.so.

Mirrors custom_modeling/flash_neox_modeling.py of the reference: `load_row` (:42-56: row-linear biases on rank 0 only),
`load_qkv` (:58-80: the checkpoint's head-interleaved [H, 3, D] rows regrouped to q | k | v per shard), `FlashNeoxAttention`
(:83-163, partial rotary over the first `rotary_pct * D` dims of each head), `FlashMLP` (:166-196), `FlashNeoXLayer`
(:199-283) and `FlashGPTNeoXForCausalLM` (:286-392).  Differences are those of the Llama port (paged KV through `KVArgs`,
fp32 logits) plus one: with `use_parallel_residual` the boundary between two layers — `h + attn + mlp` and the next layer's
two LayerNorms of that sum — is ONE launch (tgis_layernorm2_residual), which also finishes both row linears' split-K sums;
under tensor parallelism the attention and MLP outputs are added first and all-reduced once per layer (reference :254-259)."""
from typing import Optional

import torch
import torch.distributed

from tgis_amd import native
from tgis_amd.models.custom_modeling.flash_common import (
    FastLayerNorm,
    FlashForCausalLM,
    KVArgs,
    attend,
    grow_max_positions,
    write_kv,
)
from tgis_amd.utils.graph_segments import collective
from tgis_amd.utils.layers import (
    PositionRotaryEmbedding,
    TensorParallelColumnLinear,
    TensorParallelEmbedding,
    TensorParallelHead,
    TensorParallelRowLinear,
    get_linear,
)

SUPPORTED_HEAD_SIZES = (64, 96, 128)


class GPTNeoXConfig:
    """The subset of the HF GPT-NeoX config the forward needs (transformers 4.x attribute names)."""

    def __init__(self, vocab_size=50432, hidden_size=6144, num_hidden_layers=44, num_attention_heads=64,
                 intermediate_size=24576, hidden_act="gelu_fast", rotary_pct=0.25, rotary_emb_base=10000,
                 max_position_embeddings=2048, layer_norm_eps=1e-5, use_parallel_residual=True, bos_token_id=0,
                 eos_token_id=0, pad_token_id=None, tie_word_embeddings=False, quantize=None, **kwargs):
        self.vocab_size = vocab_size
        self.hidden_size = hidden_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.intermediate_size = intermediate_size
        self.hidden_act = hidden_act
        self.rotary_pct = rotary_pct
        self.rotary_emb_base = rotary_emb_base
        self.max_position_embeddings = max_position_embeddings
        self.layer_norm_eps = layer_norm_eps
        self.use_parallel_residual = use_parallel_residual
        self.bos_token_id = bos_token_id
        self.eos_token_id = eos_token_id
        self.pad_token_id = pad_token_id
        self.tie_word_embeddings = tie_word_embeddings
        self.quantize = quantize
        self.model_type = "gpt_neox"
        for k, v in kwargs.items():
            setattr(self, k, v)

    def to_dict(self):
        return dict(vars(self))


def check_neox_config(config, quantize: Optional[str] = None) -> None:
    """What this port refuses at load, before any weight is read."""
    quantize = quantize if quantize is not None else getattr(config, "quantize", None)
    if quantize == "gptq":
        # the reference's load_qkv permutes the bias but not the packed int4 weight (:62-74): no behaviour to match
        raise NotImplementedError("gpt_neox with quantize='gptq' is not supported: the head-interleaved [H, 3, D] "
                                  "query_key_value rows of a packed int4 weight are not regrouped to q | k | v")
    D = config.hidden_size // config.num_attention_heads
    if config.hidden_size % config.num_attention_heads or D not in SUPPORTED_HEAD_SIZES:
        raise NotImplementedError(f"gpt_neox head size {D} is not supported (attention kernels exist for "
                                  f"{list(SUPPORTED_HEAD_SIZES)}); this excludes e.g. Pythia-2.8B (head size 80) and "
                                  "Pythia-1B (head size 256)")
    act = getattr(config, "hidden_act", None)
    if act not in ("gelu", "gelu_fast", "gelu_pytorch_tanh"):
        raise NotImplementedError(f"gpt_neox hidden_act {act!r}: only gelu (erf), gelu_fast and gelu_pytorch_tanh "
                                  "(tanh) are wired into the GEMM epilogue")


def rotary_settings(config, head_size: int):
    """(rot_dim, base) from either config generation: `rotary_pct` + `rotary_emb_base` (transformers 4.x, gpt-neox-20b's
    config.json) or `rope_parameters{partial_rotary_factor, rope_theta}` (transformers 5.x)."""
    params = getattr(config, "rope_parameters", None) or {}
    pct = getattr(config, "rotary_pct", None)
    if pct is None:
        pct = params.get("partial_rotary_factor", getattr(config, "partial_rotary_factor", 1.0))
    base = getattr(config, "rotary_emb_base", None)
    if base is None:
        base = params.get("rope_theta", getattr(config, "rope_theta", 10000.0))
    return int(head_size * float(pct)), float(base)


def rotary_inv_freq(config, head_size: int, weights=None, prefix: Optional[str] = None) -> torch.Tensor:
    """fp32 inv_freq [rot_dim / 2]: the checkpoint's `{prefix}.rotary_emb.inv_freq` when it has one (the reference's
    PositionRotaryEmbedding.load), computed from the config otherwise."""
    rot, base = rotary_settings(config, head_size)
    name = f"{prefix}.rotary_emb.inv_freq"
    if weights is not None and prefix is not None and weights.has(name):
        inv_freq = weights._full(name).to(torch.float32)
        assert inv_freq.numel() * 2 == rot, f"{name} has {inv_freq.numel()} entries, rot_dim is {rot}"
        return inv_freq.to(weights.device)
    device = weights.device if weights is not None else "cpu"
    return 1.0 / (base ** (torch.arange(0, rot, 2, device=device, dtype=torch.float32) / rot))


def qkv_to_q_k_v(t: torch.Tensor, num_heads: int, head_size: int) -> torch.Tensor:
    """Rows of one shard's query_key_value weight [Hs * 3 * D, ...] (or bias) from the checkpoint's [Hs, 3, D] order to
    q | k | v (reference :66-74)."""
    rest = t.shape[1:]
    return t.reshape(num_heads, 3, head_size, *rest).transpose(0, 1).reshape(3 * num_heads * head_size, *rest)


def load_qkv(config, prefix: str, weights, num_heads: int, head_size: int):
    """This rank's heads (contiguous [H/w, 3, D] rows of the checkpoint) as a q | k | v column-parallel linear."""
    weight = qkv_to_q_k_v(weights.get_sharded(f"{prefix}.weight", dim=0), num_heads, head_size).contiguous()
    bias = qkv_to_q_k_v(weights.get_sharded(f"{prefix}.bias", dim=0), num_heads, head_size).contiguous()
    return TensorParallelColumnLinear(get_linear(weight, bias, config.quantize))


def load_row(config, prefix: str, weights):
    """Row-parallel linear, bias on rank 0 only (reference :42-56).  Parallel residual: the plain linear (the layer adds
    attention and MLP outputs and reduces the sum once); sequential: reduced on its own."""
    weight = weights.get_multi_weights_row(prefix, quantize=config.quantize)
    bias = weights.get_tensor(f"{prefix}.bias") if weights.process_group.rank() == 0 else None
    linear = get_linear(weight, bias, config.quantize)
    if config.use_parallel_residual:
        return linear
    return TensorParallelRowLinear(linear, process_group=weights.process_group)


class FlashNeoxAttention:
    def __init__(self, config, prefix, weights):
        self.hidden_size = config.hidden_size
        self.head_size = config.hidden_size // config.num_attention_heads
        tp = weights.process_group.size()
        if config.num_attention_heads % tp != 0:
            raise ValueError(f"`num_heads` must be divisible by `num_shards` (got `num_heads`: "
                             f"{config.num_attention_heads} and `num_shards`: {tp}")
        self.num_heads = config.num_attention_heads // tp
        self.rot_dim, _ = rotary_settings(config, self.head_size)
        self.rotary_emb = PositionRotaryEmbedding(rotary_inv_freq(config, self.head_size, weights, prefix))
        self.softmax_scale = self.head_size ** -0.5
        self.query_key_value = load_qkv(config, f"{prefix}.query_key_value", weights, self.num_heads, self.head_size)
        self.dense = load_row(config, f"{prefix}.dense", weights)

    def forward(self, hidden_states, cos, sin, position_ids, cu_seqlens_q, layer_id: int, kv: KVArgs, partial: bool):
        H, D = self.num_heads, self.head_size
        # [T, 3 H D]; at decode sizes the split-K sum (and the bias) is finished inside the rotary + cache-write kernel
        qkv = self.query_key_value(hidden_states, partial=True)
        qkv = write_kv(qkv, kv, layer_id, H, H, D, self.rot_dim, cos, sin, position_ids, cu_seqlens_q)
        attn_output = attend(qkv, kv, layer_id, H, H, D, self.softmax_scale, cu_seqlens_q)
        return self.dense(attn_output, partial=partial)

    __call__ = forward


class FlashMLP:
    def __init__(self, config, prefix, weights):
        self.tanh = config.hidden_act in ("gelu_fast", "gelu_pytorch_tanh")  # reference :173-187
        self.dense_h_to_4h = TensorParallelColumnLinear.load(config, prefix=f"{prefix}.dense_h_to_4h", weights=weights,
                                                             bias=True)
        self.dense_4h_to_h = load_row(config, f"{prefix}.dense_4h_to_h", weights)

    def forward(self, hidden_states, partial: bool):
        # GELU (act 4 erf / act 5 tanh) where the GEMM finishes its output
        h = self.dense_h_to_4h.forward_gelu(hidden_states, self.tanh)
        return self.dense_4h_to_h(h, partial=partial)

    __call__ = forward


class FlashNeoXLayer:
    def __init__(self, layer_id, config, weights):
        prefix = f"gpt_neox.layers.{layer_id}"
        self.layer_id = layer_id
        self.use_parallel_residual = config.use_parallel_residual
        self.process_group = weights.process_group
        self.input_layernorm = FastLayerNorm(f"{prefix}.input_layernorm", weights, config.layer_norm_eps)
        self.post_attention_layernorm = FastLayerNorm(f"{prefix}.post_attention_layernorm", weights,
                                                      config.layer_norm_eps)
        self.attention = FlashNeoxAttention(config, f"{prefix}.attention", weights)
        self.mlp = FlashMLP(config, f"{prefix}.mlp", weights)

    def forward_parallel(self, ln1, ln2, cos, sin, position_ids, cu_seqlens_q, kv: KVArgs):
        """attn(ln1) and mlp(ln2) of one parallel-residual layer: the two addends of the next boundary (Partials at decode
        sizes on one rank; under TP their sum, all-reduced once, and None)."""
        tp = self.process_group.size() > 1
        attn = self.attention(ln1, cos, sin, position_ids, cu_seqlens_q, self.layer_id, kv, partial=not tp)
        mlp = self.mlp(ln2, partial=not tp)
        if not tp:
            return attn, mlp
        intermediate = mlp.add_(attn)  # mlp_output + attn_output, then ONE all-reduce (reference :254-257)
        pg = self.process_group
        collective(lambda t=intermediate: torch.distributed.all_reduce(t, group=pg))
        return intermediate, None

    def forward_sequential(self, hidden_states, residual, cos, sin, position_ids, cu_seqlens_q, kv: KVArgs):
        hidden_states, residual = self.input_layernorm(hidden_states, residual)
        hidden_states = self.attention(hidden_states, cos, sin, position_ids, cu_seqlens_q, self.layer_id, kv,
                                       partial=True)
        hidden_states, residual = self.post_attention_layernorm(hidden_states, residual)
        return self.mlp(hidden_states, partial=True), residual


class FlashGPTNeoXModel:
    def __init__(self, config, weights):
        self.config = config
        self.process_group = weights.process_group
        self.embed_in = TensorParallelEmbedding(prefix="gpt_neox.embed_in", weights=weights)
        self.layers = [FlashNeoXLayer(i, config, weights) for i in range(config.num_hidden_layers)]
        self.final_layer_norm = FastLayerNorm("gpt_neox.final_layer_norm", weights, config.layer_norm_eps)
        self.use_parallel_residual = config.use_parallel_residual
        self.head_size = self.layers[0].attention.head_size
        self.num_heads = self.layers[0].attention.num_heads
        self.num_key_value_heads = self.num_heads
        self.max_positions = 0

    def rope_tables(self, dtype, device, max_s: int):
        """cos / sin [positions, rot_dim / 2], sized once for the model's position range (grow_max_positions)."""
        self.max_positions = grow_max_positions(self.config, self.max_positions, max_s)
        return self.layers[0].attention.rotary_emb.tables(dtype, device, self.max_positions)

    def forward(self, input_ids, position_ids, cu_seqlens_q, max_s, inputs_embeds, kv: KVArgs):
        hidden_states = inputs_embeds if inputs_embeds is not None else self.embed_in(input_ids)
        cos, sin = self.rope_tables(hidden_states.dtype, hidden_states.device, max_s)
        fln = self.final_layer_norm
        if not self.use_parallel_residual:
            residual = None
            for layer in self.layers:
                hidden_states, residual = layer.forward_sequential(hidden_states, residual, cos, sin, position_ids,
                                                                   cu_seqlens_q, kv)
            hidden_states, _ = fln(hidden_states, residual)
            return hidden_states
        # h' = h + attn + mlp of the layer before and both LayerNorms of this one: one launch per boundary
        a = b = None
        for layer in self.layers:
            ln1, ln2 = layer.input_layernorm, layer.post_attention_layernorm
            y1, y2, hidden_states = native.layernorm2_residual(hidden_states, a, b, ln1.weight, ln1.bias, ln1.eps,
                                                               ln2.weight, ln2.bias)
            a, b = layer.forward_parallel(y1, y2, cos, sin, position_ids, cu_seqlens_q, kv)
        y, _, _ = native.layernorm2_residual(hidden_states, a, b, fln.weight, fln.bias, fln.eps)
        return y

    __call__ = forward


class FlashGPTNeoXForCausalLM(FlashForCausalLM):
    def __init__(self, config, weights):
        check_neox_config(config)
        self.config = config
        self.gpt_neox = FlashGPTNeoXModel(config, weights)
        self.embed_out = TensorParallelHead.load(config, prefix="embed_out", weights=weights)

    @property
    def model(self):
        return self.gpt_neox

    @property
    def lm_head(self):
        return self.embed_out

    def post_init(self):
        pass  # dense weights only: their GEMM images are built at load

    def get_input_embeddings(self):
        return self.gpt_neox.embed_in

