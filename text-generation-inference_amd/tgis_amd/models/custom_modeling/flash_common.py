"""What the Llama, GPT-NeoX and Santacoder forwards share: how a layer writes its keys and values into the paged cache and
attends over it, the fused add + LayerNorm, the growth rule of the rotary tables and the tail of the `*ForCausalLM` classes.

A change to the cache (another element type, per-head scales, a clamp on write) is made here once; the model files differ
only in `(H, Hkv, D, rot_dim)` and in whether they rotate at all.  Every `native` function is looked up when it is called:
tests replace them on the module."""
from dataclasses import dataclass
from typing import Optional

import torch

from tgis_amd import native
from tgis_amd.utils.layers import workspace


@dataclass
class KVArgs:
    """Where this forward's keys/values live in the paged cache."""
    cache: "object"                    # utils.kv_cache.PagedKVCache
    block_tables: torch.Tensor         # [B, max_pages] int32 (device)
    ctx_lens: Optional[torch.Tensor]   # [B] int32, tokens per sequence incl. this forward's (prefill); decode: filled in
    slots: Optional[torch.Tensor]      # [T] int32 physical slot per token (prefill); decode: filled in
    max_q_len: int                     # longest q run in this forward (1 for decode)
    max_ctx: int                       # upper bound of ctx_lens (launch shaping only)
    num_splits: int = 1                # attention key splits (decode)
    fresh_prefill: bool = False        # every sequence starts at cache position 0: page-wise cache writes
    past_lens: Optional[torch.Tensor] = None  # [B] int32: tokens already cached on reused pages (multiples of 32) in
    #                                    front of this prefill's: page-wise cache writes starting behind them
    q_mask: Optional[torch.Tensor] = None  # [T] int64, one 64-bit word per q row: which of its sequence's q rows the row
    #                                    attends to (a tree verify step; native.attn_paged's q_mask).  None: causal
    window: Optional[int] = None       # sliding-window attention (Mistral's config.sliding_window): a q row attends to this
    #                                    many cache positions up to its own (native.attn_paged's window).  None: causal.
    #                                    `num_splits` is then the count for min(max_ctx, window + 31) keys (decode) or 1


def layer_pools(kv: KVArgs, layer_id: int):
    """(k_pool, v_pool, keyword arguments) of the native cache writers and readers for one layer: the scales of a one-byte
    cache; a 16-bit one's calls carry no `kv_scales` keyword at all."""
    cache = kv.cache
    scales = {"kv_scales": cache.scales(layer_id)} if cache.is_fp8 else {}
    return cache.k_pool(layer_id), cache.v_pool(layer_id), scales


def write_kv(qkv, kv: KVArgs, layer_id: int, H: int, Hkv: int, D: int, rot_dim: int, cos, sin, position_ids, cu_seqlens_q,
             qk_norm=None):
    """Rotates q and k of `qkv` [T, (H + 2 Hkv) D] (cos is None: no rotary) and scatters k and v to their page slots;
    returns the activation whose first H D columns attention reads.  A fresh prefill writes page-wise, and so does one
    behind reused pages (`past_lens`); everything else per token, which at decode sizes also finishes the split-K sum (and
    the bias) of a `native.Partial`.  qk_norm = (q_w, k_w, eps): the per-head RMSNorm of q and k in front of the rotation
    (Qwen3), done by the same launch in each of the three forms."""
    k_pool, v_pool, scales = layer_pools(kv, layer_id)
    if qk_norm is not None:
        scales = dict(scales, qk_norm=qk_norm)
    if kv.fresh_prefill and not isinstance(qkv, native.Partial):
        return native.rope_kv_write_prefill(qkv, cos, sin, position_ids, cu_seqlens_q, kv.block_tables, k_pool, v_pool,
                                            kv.max_q_len, H, Hkv, D, rot_dim, **scales)
    if kv.past_lens is not None and not isinstance(qkv, native.Partial):
        return native.rope_kv_write_prefill_at(qkv, cos, sin, position_ids, cu_seqlens_q, kv.block_tables, k_pool, v_pool,
                                               kv.max_q_len, H, Hkv, D, rot_dim, kv.past_lens, **scales)
    return native.rope_kv_write(qkv, cos, sin, position_ids, kv.slots, k_pool, v_pool, H, Hkv, D, rot_dim, **scales)


def attend(qkv, kv: KVArgs, layer_id: int, H: int, Hkv: int, D: int, scale: float, cu_seqlens_q, frag_out: bool = False):
    """Attention of the rotated q over the layer's cache pages: [T, H D], in fragment order (native.FragAct) for the int4
    GEMM behind it when `frag_out`."""
    k_pool, v_pool, scales = layer_pools(kv, layer_id)
    T = qkv.shape[0]
    if frag_out:
        attn_output = native.FragAct.empty(T, H * D, qkv.device)
    else:
        attn_output = torch.empty((T, H * D), dtype=qkv.dtype, device=qkv.device)
    ws = None
    if kv.num_splits > 1:
        ws = workspace(qkv.device)
        # the launcher sizes its records for B * max_q_len rows: T itself except behind ragged suffixes (prefix reuse)
        rows = max(T, kv.block_tables.shape[0] * kv.max_q_len)
        ws.ensure(native.attn_workspace_bytes(rows, H, Hkv, D, kv.num_splits))
    if kv.q_mask is not None:
        scales = dict(scales, q_mask=kv.q_mask)
    if kv.window is not None and kv.max_ctx > kv.window:  # (a window no row reaches: the causal call, as for every other model)
        scales = dict(scales, window=kv.window)
    native.attn_paged(qkv, qkv.stride(0), k_pool, v_pool, kv.block_tables, kv.ctx_lens, cu_seqlens_q, attn_output,
                      kv.block_tables.shape[0], H, Hkv, D, kv.max_q_len, kv.max_ctx, scale, kv.num_splits, ws, **scales)
    return attn_output


class FastLayerNorm:
    def __init__(self, prefix, weights, eps):
        self.weight = weights.get_tensor(f"{prefix}.weight").contiguous()
        self.bias = weights.get_tensor(f"{prefix}.bias").contiguous()
        self.eps = eps

    def forward(self, hidden_states, residual=None):
        return native.layernorm_residual(hidden_states, residual, self.weight, self.bias, self.eps)

    __call__ = forward


def grow_max_positions(config, max_positions: int, max_s: int) -> int:
    """How many positions the cos / sin tables of a model cover once a forward needs `max_s` of them.
    Sized once for the model's whole position range, so the tables normally never move.  A longer request still works:
    PositionRotaryEmbedding keeps the replaced tables allocated, because decode graphs captured earlier hold their raw
    pointers (and only ever index positions inside the table they captured)."""
    if max_s <= max_positions:
        return max_positions
    declared = min(int(getattr(config, "max_position_embeddings", 0) or 0), 1 << 17)
    return max(max_s, 2 * max_positions, declared, 2048)


class FlashForCausalLM:
    """Tail of the three `*ForCausalLM` classes: `self.model` is the decoder stack, `self.lm_head` the output head,
    `self.linears` the projections of the layers and `self.gptq_linears` the quantised ones among them."""

    def collect_linears(self, layers):
        """`layers`: per decoder layer, its projections (the tensor-parallel wrappers of utils/layers.py)."""
        self.linears = [proj.linear for projections in layers for proj in projections]
        self.gptq_linears = [lin for lin in self.linears if lin.quantized]

    def post_init(self):
        """Repack every linear for the kernels (the reference does this in serve(), server.py:334-358)."""
        for lin in self.linears:
            lin.post_init()

    @property
    def num_layers(self):
        return len(self.model.layers)

    def forward(self, input_ids, position_ids, cu_seqlens_q, max_s, inputs_embeds=None, kv: KVArgs = None,
                lm_head_indices: Optional[torch.Tensor] = None, return_embeds: bool = False, lora=None):
        """position_ids int32 [T]; returns fp32 logits [T or len(lm_head_indices), vocab]; with `return_embeds` (the
        reference's paged_llama_modeling.py:443-462) the pair (logits, hidden_states), the rows that went into lm_head.
        lora: a utils.lora.LoraArgs when rows of this forward carry adapters (the Llama class alone takes one)."""
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("You cannot specify both input_ids and inputs_embeds at the same time")
        if lora is not None:
            hidden_states = self.model(input_ids, position_ids, cu_seqlens_q, max_s, inputs_embeds, kv, lora)
        else:
            hidden_states = self.model(input_ids, position_ids, cu_seqlens_q, max_s, inputs_embeds, kv)
        if lm_head_indices is not None:
            hidden_states = hidden_states.index_select(0, lm_head_indices)
        logits = self.lm_head(hidden_states)
        return (logits, hidden_states) if return_embeds else logits

    __call__ = forward
