"""FlashCausalLMBatch + FlashCausalLM: the batched prefill/decode hot path on the MI355X kernels.

Mirrors models/flash_causal_lm.py of the reference: batch fields and `from_pb` (:28-194), `concatenate`
(:196-285), `prune` (:290-353), `generate_token` (:405-460), `_process_prefill/_decode/_new_tokens`
(:462-588).  Same names, same argument meaning, same returned tuple, same logical bookkeeping
(`cu_seqlens`, `cu_seqlens_q`, `max_seqlen`, `position_ids`, `all_input_ids_tensor`, `input_lengths`).

What is different by design:
  * `past_key_values` is always None: KV lives in the model's PagedKVCache and a batch owns a list of page
    ids per request.  The reference re-concatenates the whole KV tensor on every decode step for B > 1
    (:439-447) and on every concatenate/prune; here those are page-table edits.
  * the decode step (embedding -> layers -> head -> greedy) is replayed from a captured HIP graph keyed by
    (batch size, block-table width); the only host<->device traffic per step is three small input copies
    and, for plain greedy batches, one copy of `[B]` token ids (+ logprobs) instead of B `.item()` syncs
    (reference :546-586 / utils/tokens.py:394).
"""
import logging
import os
import time
from collections import OrderedDict, deque
from dataclasses import dataclass, field
from operator import itemgetter
from typing import Any, List, Optional, Tuple, Type, Union

import numpy as np
import torch

from tgis_amd import native
from tgis_amd.models.custom_modeling.flash_common import KVArgs
from tgis_amd.models.decode_graph import (LORA_KEY, _DecodeGraph, _LoraDecodeGraph, _TreeVerifyGraph, _VerifyGraph,
                                          renew_unheld_pool)
from tgis_amd.models.model import Model
from tgis_amd.models.speculation import LookupDrafter, MLPDrafter, spec_step
from tgis_amd.models.types import Batch, GenerateError
from tgis_amd.pb import generate_pb2
from tgis_amd.utils import mlp_speculator
from tgis_amd.utils.kv_cache import (KV_SCALES_HEADROOM, PAGE, OutOfPages, PagedKVCache, agree_kv_cache_dtype,
                                     agree_kv_prefix_reuse, agree_kv_scales, kv_pool_dtype, kv_scales_stats,
                                     pages_for_budget, parse_kv_cache_dtype, parse_kv_prefix_reuse)
from tgis_amd.utils.lora import (LoraAdapter, LoraArgs, LoraSlots, check_lora_model, check_lora_world, module_shapes,
                                 parse_lora_max_rank, parse_lora_slots, release_slots)
from tgis_amd.utils.rank_group import RankGroup
from tgis_amd.utils.sliding_window import check_window_options, parse_sliding_window
from tgis_amd.utils.spec_decode import (check_spec_candidates, check_spec_world, check_tree_rows, fallback_cause,
                                        may_ever_verify, new_stats, parse_spec_candidates, parse_spec_ngram,
                                        parse_spec_sampling, parse_spec_tokens)
from tgis_amd.utils.token_types import InputTokens, TokenInfo
from tgis_amd.utils.tokens import HeterogeneousNextTokenChooser, get_input_tokens_info, get_token_info

USE_GRAPHS = os.getenv("TGIS_DISABLE_GRAPHS", "false").lower() not in ("1", "true")


@dataclass
class FlashCausalLMBatch(Batch):
    batch_id: int
    requests: List[generate_pb2.Request]

    # tensors hold the sequences of the batch concatenated: [sum(seq_lengths)] (prefill) / [B] (decode)
    input_ids: Optional[torch.Tensor]
    position_ids: torch.Tensor
    inputs_embeds: Optional[torch.Tensor]
    # cumulative (logical) sequence lengths, and cumulative query lengths (decode only)
    cu_seqlens: torch.Tensor
    cu_seqlens_q: Optional[torch.Tensor]
    # kept for the servicer's clean_attribute("past_key_values") call; always None (paged cache)
    past_key_values: Optional[torch.Tensor]
    # maximum of the input lengths across the batch (including prefix)
    max_seqlen: int

    all_input_ids_tensor: torch.Tensor
    input_lengths: List[int]
    # (truncated) input length + prefix length + max output tokens: sizes all_input_ids_tensor and the pages
    total_lengths: List[int]
    pad_token_id: int

    next_token_chooser: HeterogeneousNextTokenChooser

    # paged-KV ownership: page ids per request, filled by the prefill generate_token
    kv_cache: Optional[PagedKVCache] = None
    pages: Optional[List[List[int]]] = None
    block_tables: Optional[torch.Tensor] = None
    # KV prefix reuse (utils/kv_cache.py): the prompts' token ids on the host, from `from_pb` to the prefill, which is their
    # only consumer; and, from `allocate_pages`, how many leading tokens of each request sit on pages it shares
    prompt_token_ids: Optional[List[List[int]]] = None
    reused_lengths: Optional[List[int]] = None
    # speculative decoding (models/speculation.py), set by the prefill of a model that has it on: K, the model's drafter, and
    # on the device the K tokens drafted for each request's next step [B, K] and the suffix length their lookup matched [B]
    # (0 = none; an MLP drafter's are all ones)
    spec_tokens: int = 0
    spec_model: Optional[Any] = None
    # candidates per request (1: one chain, `spec_drafts` [B, K]; C > 1: a token tree, `spec_drafts` [B, C, K])
    spec_candidates: int = 1
    spec_drafts: Optional[torch.Tensor] = None
    spec_hits: Optional[torch.Tensor] = None
    # with a drafter that needs it (the MLP speculator): per request the post-norm hidden state that predicted its latest
    # token [B, E] — the reference's `batch.embeds` (paged_causal_lm.py:192,261)
    spec_hidden: Optional[torch.Tensor] = None
    # (spec_hits, its host list) as last read or noted, and whether a step left the drafts stale (`spec_hits_host`)
    _spec_seen: Optional[tuple] = field(default=None, repr=False)
    _spec_stale: bool = field(default=False, repr=False)
    # the host copy of `block_tables` (`_rebuild_block_tables`), which `grow_pages` edits and uploads again
    _bt_host: Optional[np.ndarray] = field(default=None, repr=False)
    # LoRA adapters (utils/lora.py): per request the device slot its adapter is pinned in (-1: none), None when no request
    # of the batch carries one; the slot table the pins go back to; and the slots on the device, int32 [B], made on demand
    lora_slots: Optional[List[int]] = None
    lora_table: Optional[Any] = None
    _lora_dev: Optional[torch.Tensor] = field(default=None, repr=False)

    def has_lora(self) -> bool:
        return self.lora_slots is not None and any(s >= 0 for s in self.lora_slots)

    def lora_slots_device(self) -> torch.Tensor:
        """`lora_slots` as int32 [B] on the device; the same tensor until concatenate or prune change the batch."""
        if self._lora_dev is None or self._lora_dev.numel() != len(self.lora_slots):
            self._lora_dev = torch.tensor(self.lora_slots, dtype=torch.int32).to(self.position_ids.device, non_blocking=True)
        return self._lora_dev

    def get_id(self) -> int:
        return self.batch_id

    def __len__(self):
        return len(self.requests)

    # ---- page ownership --------------------------------------------------------------------------
    def allocate_pages(self, kv_cache: PagedKVCache):
        """Pages for the prompt and the first generated token.  The cache then grows one page at a time as sequences
        cross page boundaries (`grow_pages`), like the reference's KV grows with the tokens produced — the router's
        batch-weight model (router/src/batch_types.rs:46-118) counts tokens present, not max_output_length."""
        assert self.pages is None
        need = [PagedKVCache.pages_for(n + 1) for n in self.input_lengths]
        # KV prefix reuse: the leading pages a request shares with an earlier one come first in its list (pinned by
        # `match`), the pool deals only the rest.  Tensor-parallel ranks need no collective here: every rank sees the same
        # request stream and holds the same number of pages (FlashCausalLM, ranks.min_int), and the index is a
        # deterministic function of the two, so every rank maps the same pages.
        shared = [[] for _ in need]
        if getattr(kv_cache, "prefix_reuse", False) and self.reuse_lookup_ok():
            # (a request that carries a LoRA adapter neither looks up nor registers pages: its keys differ)
            adapted = self.lora_slots or [-1] * len(need)
            shared = [kv_cache.match(ids) if s < 0 else [] for ids, s in zip(self.prompt_token_ids, adapted)]
        own = [n - len(s) for n, s in zip(need, shared)]
        try:
            flat = kv_cache.alloc(sum(own))  # raises OutOfPages before anything is taken
        except OutOfPages:
            for s in shared:
                kv_cache.free(s)
            raise
        self.kv_cache = kv_cache
        self.reused_lengths = [len(s) * PAGE for s in shared]
        # page-major: page p of every sequence, then page p + 1 (kv_cache.py: the pages the decode blocks read at the same
        # time are then neighbours in the pool)
        self.pages, it = shared, iter(flat)
        for p in range(max(own, default=0)):
            for i in range(len(own)):
                if p < own[i]:
                    self.pages[i].append(next(it))
        self._rebuild_block_tables()

    def reuse_lookup_ok(self) -> bool:
        """Whether this batch's prefill may start behind cached pages.  Not with prompt-tuning prefixes (`inputs_embeds`:
        the pad ids in their place do not describe the content), and not when a request wants `details.input_toks`: every
        prompt position's logits are then needed, and `_process_new_tokens` indexes them by the logical `cu_seqlens`."""
        return (self.prompt_token_ids is not None and self.inputs_embeds is None
                and not any(r.details.input_toks for r in self.requests))

    def register_prompt_pages(self):
        """After the prefill: the full prompt pages become findable (not those of prompt-tuning prefixes)."""
        ids, self.prompt_token_ids = self.prompt_token_ids, None
        if ids is None or self.inputs_embeds is not None or not getattr(self.kv_cache, "prefix_reuse", False):
            return
        adapted = self.lora_slots or [-1] * len(ids)
        for pages, toks, s in zip(self.pages, ids, adapted):
            if s < 0:
                self.kv_cache.register(pages, toks)

    def grow_pages(self, ahead: int = 0):
        """Before a decode step: every sequence owns the page its next token (position input_length - 1) lands on, and
        those of the `ahead` positions behind it (a verify step writes its drafts' keys and values there)."""
        short = [i for i, (p, n) in enumerate(zip(self.pages, self.input_lengths)) if len(p) * PAGE < n + ahead]
        if not short:
            return
        need = {i: PagedKVCache.pages_for(self.input_lengths[i] + ahead) - len(self.pages[i]) for i in short}
        flat = iter(self.kv_cache.alloc(sum(need[i] for i in short)))  # all or nothing: OutOfPages leaves the batch as it was
        for i in short:
            self.pages[i].extend(next(flat) for _ in range(need[i]))
        width = self.block_tables.shape[1]
        if max(len(self.pages[i]) for i in short) > width or self._bt_host is None:
            self._rebuild_block_tables()
        else:  # edit the host copy and upload the few KB again (the same copy the prefill made: nothing new to load)
            for i in short:
                have = len(self.pages[i])
                self._bt_host[i, have - need[i]:have] = self.pages[i][-need[i]:]
            self.block_tables = torch.from_numpy(self._bt_host).to(self.block_tables.device, non_blocking=True)

    # ---- speculative decoding ---------------------------------------------------------------------
    def redraft(self):
        """Drafts anew from the batch's own tensors: concatenate and prune rebuilt what the drafter reads, or a step left
        the drafts stale.  A no-op with the option off."""
        if self.spec_tokens:
            self.spec_model.redraft(self)

    def can_verify(self) -> bool:
        """Whether a batch of this size can verify at all (its bucket times 1 + C K rows): if not, nobody drafts for it."""
        return may_ever_verify(self.spec_tokens, graph_bucket(len(self)), self.spec_candidates)

    def ensure_spec_buffers(self, emb_dim: int = 0, dtype=None):
        """The batch's own `spec_drafts` / `spec_hits` for its present size (and `spec_hidden`, given its width)."""
        B, dev = len(self), self.position_ids.device
        if self.spec_drafts is None or self.spec_drafts.shape[0] != B:
            shape = (B, self.spec_tokens) if self.spec_candidates == 1 else (B, self.spec_candidates, self.spec_tokens)
            self.spec_drafts = torch.zeros(shape, dtype=torch.int64, device=dev)
            self.spec_hits = torch.zeros(B, dtype=torch.int32, device=dev)
        if emb_dim and (self.spec_hidden is None or self.spec_hidden.shape[0] != B):
            self.spec_hidden = torch.zeros((B, emb_dim), dtype=dtype, device=dev)

    def drafts_renewed(self):
        self._spec_seen = None
        self._spec_stale = False

    def drafts_are_stale(self):
        """A step that could not lead to a verify step (sampling or details in the batch, a bucket too wide) skips the
        lookup; the step rule drafts anew before it looks at the hits, should the batch ever get that far."""
        self._spec_stale = True

    def spec_hits_host(self) -> List[int]:
        """`spec_hits` on the host.  A greedy step brings them along in its one copy (`note_spec_hits`); only a tensor the
        batch has not seen yet is fetched: after a prefill, concatenate or prune, or one a caller put in its place (whoever
        wants other drafts verified assigns new `spec_drafts` / `spec_hits` tensors rather than writing into these)."""
        if self._spec_stale:
            self.redraft()
        t = self.spec_hits
        seen = self._spec_seen
        if seen is None or seen[0] is not t:
            seen = self._spec_seen = (t, t.tolist())
        return seen[1]

    def note_spec_hits(self, hits: List[int]):
        self._spec_seen = (self.spec_hits, hits)

    def _rebuild_block_tables(self):
        # as wide as the longest sequence can ever get (pages themselves are taken lazily): the decode graph of a batch
        # is keyed by (size, table width), so the width must not creep up while the batch generates
        width = max(max(len(p) for p in self.pages), max(PagedKVCache.pages_for(t) for t in self.total_lengths))
        width = (width + 7) // 8 * 8  # few distinct widths -> few captured graphs
        bt = np.zeros((len(self.pages), width), dtype=np.int32)
        for i, p in enumerate(self.pages):
            bt[i, :len(p)] = p
        self._bt_host = bt
        self.block_tables = torch.from_numpy(bt).to(self.cu_seqlens.device, non_blocking=True)

    def release(self):
        if self.pages is not None and self.kv_cache is not None:
            for p in self.pages:
                self.kv_cache.free(p)
        self.pages = None
        self.block_tables = None
        slots, self.lora_slots = self.lora_slots, None
        release_slots(self.lora_table, slots)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    # ---- construction ---------------------------------------------------------------------------------
    @classmethod
    def from_pb(cls, pb: generate_pb2.Batch, tokenizer, dtype: torch.dtype, device: torch.device,
                embeddings_lookup: Optional, prefix_cache: Optional, use_position_ids: bool = True,
                ) -> Tuple[Optional["FlashCausalLMBatch"], List[GenerateError]]:
        lora_slots: List[int] = []  # the requests' LoRA slots, pinned as they are found: they go back if no batch results
        try:
            return cls._from_pb(pb, tokenizer, dtype, device, embeddings_lookup, prefix_cache, use_position_ids, lora_slots)
        except BaseException:
            release_slots(getattr(prefix_cache, "lora", None), lora_slots)
            raise

    @classmethod
    def _from_pb(cls, pb, tokenizer, dtype, device, embeddings_lookup, prefix_cache, use_position_ids, lora_slots):
        errors: List[GenerateError] = []
        requests, batch_inputs, prefix_embeds_by_index = [], [], {}
        input_lengths, total_lengths = [], []
        cu_seqlens = [0]
        lora_table = getattr(prefix_cache, "lora", None)
        for r in pb.requests:
            input_length = r.input_length
            slot = -1
            if r.prefix_id:
                try:
                    prefix_embeds = prefix_cache.get(r.prefix_id)
                    if isinstance(prefix_embeds, LoraAdapter):
                        # a LoRA adapter adds no tokens: the request pins a device slot (every slot pinned: an error)
                        slot = lora_table.acquire(prefix_embeds)
                except Exception as exc:
                    message = f"Prefix lookup error for request #{r.id}, prefix id {r.prefix_id}"
                    if isinstance(exc, ValueError) and "LoRA" in str(exc):
                        message += f": {exc}"  # (names the refused variant, the missing option or the busy slots)
                    logging.error(message)
                    errors.append(GenerateError(request_id=r.id, message=message))
                    continue  # the request is left out of the batch
                if slot < 0:
                    prefix_embeds_by_index[len(requests)] = prefix_embeds
                    input_length += prefix_embeds.shape[0]  # input_lengths include the prefix
            lora_slots.append(slot)
            requests.append(r)
            batch_inputs.append(r.inputs)
            input_lengths.append(input_length)
            total_lengths.append(input_length + r.max_output_length)
            cu_seqlens.append(cu_seqlens[-1] + input_length)
        if not requests:
            return None, errors
        max_seqlen = max(input_lengths)

        # no padding: sequences are concatenated across the batch
        tokenized = tokenizer(batch_inputs, truncation=True, max_length=max_seqlen,
                              return_token_type_ids=False)["input_ids"]
        all_input_ids_tensor = torch.full((len(requests), max(total_lengths)), tokenizer.pad_token_id,
                                          dtype=torch.int64, device=device)
        input_ids, position_ids, chooser_params, return_logprobs, prompt_token_ids = [], [], [], [], []
        for i, (r, toks, input_length) in enumerate(zip(requests, tokenized, input_lengths)):
            if r.truncate:
                toks = toks[-r.input_length:]
                if getattr(tokenizer, "add_bos_token", False):
                    toks[0] = tokenizer.bos_token_id  # keep a BOS at the front after left-truncation
            prompt_token_ids.append([int(t) for t in toks])
            toks = all_input_ids_tensor.new_tensor(toks)
            # a prefix occupies the first (input_length - r.input_length) positions as pad ids
            all_input_ids_tensor[i, input_length - r.input_length:input_length] = toks
            input_ids.append(toks if input_length == r.input_length else all_input_ids_tensor[i, :input_length])
            chooser_params.append(r.parameters)
            return_logprobs.append(r.details.logprobs)
            position_ids.append(torch.arange(0, input_length))
        input_ids = torch.cat(input_ids)

        if prefix_embeds_by_index:
            inputs_embeds = embeddings_lookup(input_ids)
            input_ids = None
            for i, p in prefix_embeds_by_index.items():
                inputs_embeds[cu_seqlens[i]:cu_seqlens[i] + p.shape[0], :] = p
        else:
            inputs_embeds = None

        next_token_chooser = HeterogeneousNextTokenChooser.from_pb(
            pb=chooser_params,
            model_eos_token_id=getattr(tokenizer, "model_eos_token_id", tokenizer.eos_token_id),
            model_pad_token_id=tokenizer.pad_token_id,
            return_logprobs=return_logprobs, dtype=torch.float32, device=device)

        return cls(
            batch_id=pb.id, requests=requests, input_ids=input_ids, inputs_embeds=inputs_embeds,
            position_ids=torch.cat(position_ids).to(device, non_blocking=True),
            cu_seqlens=torch.tensor(cu_seqlens, dtype=torch.int32, device=device), cu_seqlens_q=None,
            max_seqlen=max_seqlen, past_key_values=None, input_lengths=input_lengths,
            total_lengths=total_lengths, all_input_ids_tensor=all_input_ids_tensor,
            next_token_chooser=next_token_chooser, pad_token_id=tokenizer.pad_token_id,
            prompt_token_ids=prompt_token_ids,
            lora_slots=list(lora_slots) if any(s >= 0 for s in lora_slots) else None, lora_table=lora_table,
        ), errors

    @classmethod
    def concatenate(cls, batches: List["FlashCausalLMBatch"]) -> "FlashCausalLMBatch":
        first = batches[0]
        device = first.cu_seqlens_q.device
        requests, input_lengths, total_lengths, pages = [], [], [], []
        chooser_params, ntc_current_tokens, ntc_samplings, ntc_return_logprobs = [], [], [], []
        input_ids, position_ids = [], []
        cu_seqlens = [torch.tensor([0], dtype=torch.int32, device=device)]
        new_batch_size = sum(len(b) for b in batches)
        max_total_length = max(t for b in batches for t in b.total_lengths)
        all_input_ids_tensor = first.all_input_ids_tensor.new_full((new_batch_size, max_total_length),
                                                                   first.pad_token_id)
        cumulative_length = torch.tensor(0, device=device)
        start, max_seqlen = 0, 0
        for batch in batches:
            requests.extend(batch.requests)
            input_lengths.extend(batch.input_lengths)
            total_lengths.extend(batch.total_lengths)
            chooser_params.extend(r.parameters for r in batch.requests)
            ntc_current_tokens.extend(batch.next_token_chooser.current_tokens)
            ntc_samplings.extend(batch.next_token_chooser.samplings)
            ntc_return_logprobs.extend(batch.next_token_chooser.return_logprobs)
            cu_seqlens.append(batch.cu_seqlens[1:] + cumulative_length)
            input_ids.append(batch.input_ids)
            position_ids.append(batch.position_ids)
            # no KV bytes move (reference: torch.cat of the pasts); ownership of the pages changes hands below, once
            # the merged batch exists — an exception before that leaves every page with its source batch
            pages.extend(batch.pages)
            end = start + len(batch)
            all_input_ids_tensor[start:end, :batch.all_input_ids_tensor.shape[1]] = batch.all_input_ids_tensor
            start = end
            max_seqlen = max(max_seqlen, batch.max_seqlen)
            cumulative_length += batch.cu_seqlens[-1]

        ntc0 = first.next_token_chooser
        next_token_chooser = HeterogeneousNextTokenChooser.from_pb(
            pb=chooser_params, model_eos_token_id=ntc0.eos_token_id, model_pad_token_id=ntc0.pad_token_id,
            return_logprobs=ntc_return_logprobs, dtype=ntc0.dtype, device=ntc0.device,
            samplings=ntc_samplings, current_tokens=ntc_current_tokens)

        merged = FlashCausalLMBatch(
            batch_id=first.batch_id, requests=requests, input_ids=torch.cat(input_ids), inputs_embeds=None,
            position_ids=torch.cat(position_ids), cu_seqlens=torch.cat(cu_seqlens),
            cu_seqlens_q=torch.arange(len(requests) + 1, device=device, dtype=torch.int32),
            max_seqlen=max_seqlen, past_key_values=None, input_lengths=input_lengths,
            total_lengths=total_lengths, all_input_ids_tensor=all_input_ids_tensor,
            next_token_chooser=next_token_chooser, pad_token_id=first.pad_token_id,
            kv_cache=first.kv_cache, pages=None, spec_tokens=first.spec_tokens, spec_model=first.spec_model,
            spec_candidates=first.spec_candidates,
            spec_hidden=torch.cat([b.spec_hidden for b in batches]) if first.spec_hidden is not None else None)
        merged.pages = pages
        try:
            merged._rebuild_block_tables()
        except BaseException:
            merged.pages = None  # the sources still own them
            raise
        if any(b.lora_slots is not None for b in batches):  # the pins change hands with the pages
            merged.lora_slots = [s for b in batches for s in (b.lora_slots or [-1] * len(b))]
            merged.lora_table = next(b.lora_table for b in batches if b.lora_slots is not None)
        for batch in batches:
            batch.pages = None
            batch.block_tables = None
            batch.lora_slots = None
        merged.redraft()
        return merged

    @classmethod
    def prune(cls, batch: "FlashCausalLMBatch", completed_ids: List[int]) -> Optional["FlashCausalLMBatch"]:
        """Drop completed requests; their pages go back to the pool."""
        if not completed_ids:
            return batch
        keep_indices = Model.get_indices_to_keep(batch.requests, completed_ids)
        new_size = len(keep_indices)
        if new_size == 0:
            batch.release()
            return None
        keep = set(keep_indices)
        for i, p in enumerate(batch.pages):
            if i not in keep:
                batch.kv_cache.free(p)
        pick = (lambda l: [l[i] for i in keep_indices])
        if batch.lora_slots is not None:  # the completed requests' adapter slots are unpinned
            release_slots(batch.lora_table, [s for i, s in enumerate(batch.lora_slots) if i not in keep])
            batch.lora_slots, batch._lora_dev = pick(batch.lora_slots), None
        batch.pages = pick(batch.pages)
        batch.input_lengths = pick(batch.input_lengths)
        batch.total_lengths = pick(batch.total_lengths)
        batch.requests = pick(batch.requests)
        batch.next_token_chooser = batch.next_token_chooser.filter(keep_indices)
        batch.max_seqlen = max(batch.input_lengths)
        batch.input_ids = batch.input_ids[keep_indices]
        batch.position_ids = batch.position_ids[keep_indices]
        batch.all_input_ids_tensor = batch.all_input_ids_tensor[keep_indices, :max(batch.total_lengths)]
        if new_size == 1:
            batch.cu_seqlens = batch.cu_seqlens.new_tensor([0, batch.input_lengths[0]])
        else:
            # logical slot layout after re-packing: every kept sequence followed by its free slot
            cu = batch.cu_seqlens[:new_size + 1].clone()
            cu[1:] = batch.position_ids
            cu[1:].add_(1)
            batch.cu_seqlens = torch.cumsum(cu, dim=0, dtype=torch.int32)
        batch.cu_seqlens_q = batch.cu_seqlens_q[:new_size + 1]
        batch._rebuild_block_tables()
        batch.spec_drafts = batch.spec_hits = None
        if batch.spec_hidden is not None:
            batch.spec_hidden = batch.spec_hidden[keep_indices]
        batch.redraft()
        return batch


# page-wise cache writes in prefill (tgis_rope_kv_write_prefill); "false" keeps the per-token kernel for A/B checks
FRESH_PREFILL_KV = os.getenv("TGIS_PREFILL_KV", "true").lower() not in ("0", "false")


# A captured decode step serves every batch size of its BUCKET (round 6): the rows past the batch are inactive — position 0,
# every table entry the pool's null page (utils/kv_cache.py), their token written there and attended to alone, their ids
# never read.  A router that lets a batch wander over 24..32 requests then replays ONE graph instead of capturing nine (a
# capture is a warm-up step + the capture itself: tens of ms in the middle of serving; bench.py --churn reports them).
GRAPH_BUCKETS = os.getenv("TGIS_GRAPH_BUCKETS", "true").lower() not in ("0", "false")


def graph_bucket(B: int) -> int:
    """Rows of the decode graph that serves B requests: powers of two up to 8, then multiples of 8 (the GEMMs cost the same
    up to 32 rows and from 33 to 64; an inactive row costs the attention one page)."""
    if not GRAPH_BUCKETS:
        return B
    if B <= 8:
        return 1 << (B - 1).bit_length()
    return (B + 7) // 8 * 8


class FlashCausalLM(Model):
    # the drafter of speculative decoding (models/speculation.py; set by the constructor): None with the option off, else the
    # prompt lookup or the MLP speculator on the device, which is then `speculator` too
    spec_drafter = "lookup"
    drafter = speculator = None
    # whether batches that sample or carry processors verify drafts too (set by the constructor)
    spec_sampling = False
    # draft chains a greedy request brings to a verify step (set by the constructor); 1 = the single chain
    spec_candidates = 1
    # sliding-window attention: W keys per q row (config.sliding_window, Mistral), None = causal (set by the constructor)
    sliding_window = None
    # LoRA adapters per request (utils/lora.py; set by the constructor): S device slots (0 = off) for ranks up to
    # lora_max_rank, and the table that maps adapter ids to them
    lora_slots = 0
    lora_max_rank = 64
    lora_table = None

    def __init__(self, model_name: str, revision: Optional[str], deployment_framework: str, dtype: torch.dtype,
                 quantize: Optional[str], model_config: Union[Any] = None, auto_model_class=None,
                 max_sequence_length: Optional[int] = None, engine=None, kv_cache_pages: Optional[int] = None,
                 kv_cache_dtype: Optional[str] = None, kv_scales: Union[None, str, dict] = None,
                 kv_prefix_reuse: Optional[bool] = None, spec_tokens: Optional[int] = None,
                 spec_ngram: Optional[int] = None, speculator: Union[None, str, Any] = None,
                 spec_sampling: Optional[bool] = None, spec_candidates: Optional[int] = None,
                 lora_slots: Optional[int] = None, lora_max_rank: Optional[int] = None):
        # KV cache element: "auto" (the model dtype) or "fp8_e4m3" (one byte, utils/kv_cache.py); None reads
        # TGIS_KV_CACHE_DTYPE.  Checked before anything is loaded — except on a rank of a tensor-parallel group, which loads
        # its shard and then tells its peers (agree_kv_cache_dtype below): they sit in a collective only it can release.
        # kv_prefix_reuse: requests share the cached pages of a common prompt prefix (utils/kv_cache.py); None reads
        # TGIS_KV_PREFIX_REUSE (true / false, default false).  Checked and agreed on like the cache dtype.
        if (getattr(engine, "world_size", 1) or 1) == 1:
            parse_kv_cache_dtype(kv_cache_dtype)
            parse_kv_prefix_reuse(kv_prefix_reuse)
        # spec_tokens: K > 0 turns prompt-lookup speculative decoding on (utils/spec_decode.py): greedy batches verify K
        # drafted tokens per request and step; None reads TGIS_SPEC_TOKENS (0 / unset = off, 1 .. 7).  spec_ngram: the
        # longest suffix looked up (TGIS_SPEC_NGRAM, default 3, 1 .. 4).  Not under tensor parallelism.
        self.spec_tokens = parse_spec_tokens(spec_tokens)
        self.spec_ngram = parse_spec_ngram(spec_ngram)
        check_spec_world(self.spec_tokens, getattr(engine, "world_size", 1) or 1)
        # spec_sampling: batches that are not plain greedy (sampling, warpers, penalties, an unmet min_new_tokens) verify
        # drafts as well, every row chosen by the fused chooser with the draw its plain step would have made; None reads
        # TGIS_SPEC_SAMPLING (true / false, default false).  It means something only with spec_tokens > 0.
        self.spec_sampling = parse_spec_sampling(spec_sampling) and self.spec_tokens > 0
        # speculator: the checkpoint directory of an MLP speculator (utils/mlp_speculator.py), the drafter in place of the
        # lookup; None reads TGIS_SPECULATOR, unset = the lookup.  It needs spec_tokens in 1 .. min(n_predict, 7) and ignores
        # spec_ngram.  Its config, tensor names and shapes are checked here, before any weight is on the device.
        # (tools hand over a checkpoint they made in memory, a mlp_speculator.SpeculatorCheckpoint, in place of the directory)
        # (an engine built here is checked against the base model below, as soon as its config is read)
        spec_ckpt = mlp_speculator.checked_checkpoint(speculator, self.spec_tokens, getattr(engine, "_config", None))
        self.spec_drafter = "lookup" if spec_ckpt is None else "mlp"
        # spec_candidates: C > 1 lets a greedy request bring up to C looked-up chains of K drafts to a verify step, verified in
        # one forward as a token tree of 1 + C K rows (utils/spec_decode.py); None reads TGIS_SPEC_CANDIDATES (unset / 1 = one
        # chain, 2 .. 4).  It needs spec_tokens > 0, the lookup drafter and no spec_sampling.
        self.spec_candidates = parse_spec_candidates(spec_candidates)
        check_spec_candidates(self.spec_candidates, self.spec_tokens, spec_ckpt is not None, self.spec_sampling)
        # lora_slots: S > 0 lets every request name a LoRA adapter with its prefix_id (utils/lora.py): S adapters are
        # resident on the device at once, requests with different adapters or none share a batch; None reads TGIS_LORA_SLOTS
        # (0 / unset = off, 1 .. 32).  lora_max_rank: the largest rank a slot holds (TGIS_LORA_MAX_RANK, default 64, a
        # multiple of 16 up to 64).  Llama class only; not under tensor parallelism, not with spec_tokens.
        self.lora_slots = parse_lora_slots(lora_slots)
        self.lora_max_rank = parse_lora_max_rank(lora_max_rank)
        check_lora_world(self.lora_slots, getattr(engine, "world_size", 1) or 1, self.spec_tokens)
        # kv_scales: the calibrated per-layer scales of a one-byte cache, the contents of a kv_cache_scales.json or its path
        # (utils/kv_cache.py, resolve_kv_scales); None looks at TGIS_KV_SCALES, then next to the weights, else they stay 1.0
        if not torch.cuda.is_available():
            raise NotImplementedError("FlashCausalLM is only available on GPU")
        if engine is None:
            from tgis_amd.inference_engine import get_inference_engine_class
            from tgis_amd.utils.hub import get_model_path

            model_path = get_model_path(model_name, revision)
            engine = get_inference_engine_class(deployment_framework)(
                model_path, auto_model_class, dtype, quantize, model_config, max_sequence_length)
        super().__init__(engine, dtype, max_sequence_length)
        self.use_position_ids = True
        tok = self.tokenizer
        if tok is not None:
            if getattr(self.config, "pad_token_id", None) is not None:
                tok.pad_token_id = self.config.pad_token_id
            elif tok.pad_token_id is None:
                if getattr(self.config, "eos_token_id", None) is not None:
                    tok.pad_token_id = self.config.eos_token_id
                elif tok.eos_token_id is not None:
                    tok.pad_token_id = tok.eos_token_id
                else:
                    tok.add_special_tokens({"pad_token": "[PAD]"})

        inner = self.model.model  # FlashLlamaModel / FlashSantacoderModel
        self.num_heads = inner.num_heads
        self.num_kv_heads = inner.num_key_value_heads
        self.head_size = inner.head_size
        self.num_layers = len(inner.layers)
        if self.lora_slots:
            # before post_init (the gate_up image loses its SiLU * up epilogue) and before the pool is sized: the slot
            # images are allocated here, once, and their bytes come out of the page budget
            check_lora_model(self.lora_slots, self.model)
            self.lora_linears = self.model.enable_lora(self.lora_slots, self.lora_max_rank, dtype, self.device)
            self.lora_table = LoraSlots(self.lora_slots, self.lora_max_rank, module_shapes(self.config), self.num_layers, dtype,
                                        upload=self._load_adapter)
            if self.prefix_cache is not None:
                self.prefix_cache.lora = self.lora_table
        if hasattr(self.model, "post_init"):
            self.model.post_init()
        # what tensor-parallel ranks must agree on, in this order on every rank: cache dtype, prefix reuse, pages, scales,
        # graph mode, seed
        self.ranks = RankGroup(engine, self.device)
        check_spec_world(self.spec_tokens, self.ranks.world)
        check_lora_world(self.lora_slots, self.ranks.world, self.spec_tokens)
        check_tree_rows(self.spec_candidates, self.spec_tokens, self.num_heads, self.num_kv_heads)
        self._spec_stats = new_stats()
        if spec_ckpt is not None:
            # before the pool is sized: the speculator's bytes come out of the page budget
            mlp_speculator.check_base(spec_ckpt.cfg, self.config.hidden_size, self.config.vocab_size)
            self.drafter = self.speculator = MLPDrafter(spec_ckpt, self.spec_tokens, dtype, self.device)
        elif self.spec_tokens:
            self.drafter = LookupDrafter(self.spec_tokens, self.spec_ngram, self.spec_candidates)
        self.kv_cache_dtype = agree_kv_cache_dtype(self.ranks, kv_cache_dtype)
        self.kv_prefix_reuse = agree_kv_prefix_reuse(self.ranks, kv_prefix_reuse)
        # config.sliding_window (None / 0 = off): the fresh prefill and the decode graphs attend under it
        # (utils/sliding_window.py); the options whose launches do not are refused before any page is allocated
        self.sliding_window = parse_sliding_window(self.config)
        check_window_options(self.sliding_window, self.config, self.spec_tokens, self.kv_prefix_reuse)
        if kv_cache_pages is None:
            kv_cache_pages = self._default_kv_pages()
        # Tensor parallel: every rank must hold the SAME number of pages.  Each rank sizes its pool from its own free
        # memory, and `grow_pages` raises OutOfPages before a decode step: a rank with fewer pages would leave the step
        # while the others enter its all-reduces (a hang instead of RESOURCE_EXHAUSTED), and the memory model a rank
        # reports to the router would differ from its peers'.  The smallest pool decides.
        kv_cache_pages = self.ranks.min_int(kv_cache_pages)
        self.kv_cache = PagedKVCache(self.num_layers, self.num_kv_heads, self.head_size, kv_cache_pages, dtype,
                                     self.device, kv_dtype=self.kv_cache_dtype, prefix_reuse=self.kv_prefix_reuse)
        # before any page is written and any graph captured: both hold the scales
        scales = agree_kv_scales(self.ranks, kv_scales, self.kv_cache_dtype, self.num_layers,
                                 getattr(engine, "model_path", None))
        if scales is not None:
            self.kv_cache.set_scales(*scales)
        # tp > 1, TGIS_TP_GRAPHS = auto (default) | full | segments | false:
        #   full      one graph per step with the RCCL all-reduces / all-gather inside it (RCCL is capture-aware);
        #   segments  a chain of graphs with the collectives launched between them (utils/graph_segments.py);
        #   false     every kernel launched eagerly (host-bound: 4.4 ms/step whatever the shard size);
        #   auto      full if a one-collective probe graph captures, replays and reduces correctly on every rank of an
        #             RCCL group, else segments.
        # One rank's step at TP=8 shapes, collectives on a world-size-1 RCCL group (tools/tp_segments_rccl1.py):
        # 2.0 ms full, 3.2 ms segments, 4.4 ms eager.
        tp = self.tp_world = self.ranks.world
        tp_mode = os.getenv("TGIS_TP_GRAPHS", "auto").lower()
        if tp == 1 or tp_mode in ("full", "1", "true"):
            self.graph_mode = "full"
        elif tp_mode in ("auto", "segments"):
            self.graph_mode = tp_mode
        else:
            self.graph_mode = None
        self.use_graphs = USE_GRAPHS and self.graph_mode is not None
        if self.ranks.real:
            # requests without a seed must still draw the same tokens on every rank
            from tgis_amd.utils import tokens

            base = tokens.seed_base()
            hi, lo = self.ranks.broadcast_int64_pair(base >> 32, base & 0xFFFFFFFF)
            tokens.set_seed_base((hi << 32) | lo)
        # captured decode steps, least recently used first; they share one memory pool (a step's intermediates are dead
        # once it has run, and its outputs are consumed before the next replay), and the number kept is bounded
        self._graphs = OrderedDict()
        self.graph_captures = deque(maxlen=4096)  # (rows, pages per row, capture ms, K: 0 = plain step) of the latest captures
        self.max_graphs = int(os.getenv("TGIS_MAX_DECODE_GRAPHS", "48"))
        self.graph_pool = torch.cuda.graph_pool_handle() if self.use_graphs else None

    def calibrate_kv_scales(self, batches, decode_steps: int = 0, headroom: float = KV_SCALES_HEADROOM) -> dict:
        """The contents of a kv_cache_scales.json (utils/kv_cache.py) measured on this model: every generate_pb2.Batch of
        `batches` is prefilled and decoded for `decode_steps` steps on the ordinary 16-bit cache, tgis_kv_absmax reads max |k|
        and max |v| of its cached tokens layer by layer, and its pages go back to the pool.  Tensor parallel: every rank
        runs it on the same batches; the heads of all ranks are reduced, every rank returns the same dict."""
        if self.kv_cache.is_fp8:
            raise ValueError("calibrate_kv_scales measures the 16-bit cache: build the model with kv_cache_dtype='auto'")
        check_window_options(self.sliding_window, self.config, calibrate_kv_scales=True)
        L, Hkv, D = self.num_layers, self.num_kv_heads, self.head_size
        stats = torch.zeros((L, 2, Hkv), dtype=torch.float32, device=self.device)
        tokens = 0
        with self.context_manager():
            for pb in batches:
                if decode_steps and min(r.max_output_length for r in pb.requests) <= decode_steps:
                    raise ValueError(f"{decode_steps} decode steps need requests with max_output_length > {decode_steps}")
                batch, errs = self.batch_type.from_pb(pb, self.tokenizer, self.dtype, self.device, self.word_embeddings,
                                                      self.prefix_cache, self.use_position_ids)
                if errs:
                    raise ValueError(f"calibration batch {pb.id}: {errs[0].message}")
                try:
                    self.generate_token(batch, first=True)
                    for _ in range(decode_steps):
                        self.generate_token(batch)
                    cached = [n - 1 for n in batch.input_lengths]  # the token chosen last is not in the cache yet
                    ctx = torch.tensor(cached, dtype=torch.int32, device=self.device)
                    for l in range(L):
                        native.kv_absmax(self.kv_cache.k_pool(l), self.kv_cache.v_pool(l), batch.block_tables, ctx, Hkv, D,
                                         stats[l])
                    tokens += sum(cached)
                finally:
                    batch.release()
            # [L, 2] over this rank's heads, then over the ranks (outside any capture)
            absmax = self.ranks.max_reduce(stats.amax(dim=2)).cpu().tolist()
        return kv_scales_stats([a[0] for a in absmax], [a[1] for a in absmax], tokens, str(self.dtype).replace("torch.", ""),
                               headroom)

    def spec_stats(self) -> dict:
        """Counters of speculative decoding since construction (all zero with the option off): decode steps, those that
        verified drafts (and, of these, those of batches that are not plain greedy: spec_sampling), the plain steps of a
        speculating model by cause (utils/spec_decode.py FALLBACK_CAUSES), tokens drafted, drafts accepted, tokens emitted by
        decode steps."""
        return dict(self._spec_stats)

    def _default_kv_pages(self) -> int:
        free, _total = torch.cuda.mem_get_info(self.device)
        frac = float(os.getenv("TGIS_KV_CACHE_FRACTION", "0.85"))
        elem = torch.empty((), dtype=kv_pool_dtype(self.kv_cache_dtype, self.dtype)).element_size()
        return pages_for_budget(int(free * frac), self.num_layers, self.num_kv_heads, self.head_size, elem)

    @property
    def batch_type(self) -> Type[FlashCausalLMBatch]:
        return FlashCausalLMBatch

    # ---- the hot path -------------------------------------------------------------------------------------
    def generate_token(self, batch: FlashCausalLMBatch, first: bool = False, for_concat: bool = False,
                       ) -> Tuple[List[TokenInfo], Optional[List[InputTokens]], List[GenerateError], int]:
        start_time = time.time_ns()
        spec_before = None
        if self.spec_tokens and not first and logging.getLogger().isEnabledFor(logging.DEBUG):
            spec_before = self.spec_stats()
        if first:
            (out, embeds), fused = self._prefill(batch), None
        else:
            out, fused = self._decode_forward(batch)
        forward_time_ns = time.time_ns() - start_time

        if first:
            generated_tokens, input_token_infos, decode_errors = self._process_prefill(batch, out)
        else:
            generated_tokens, decode_errors = self._process_decode(batch, out, fused)
            input_token_infos = None

        # logical slot bookkeeping of the reference: one more slot per sequence (:457-458); a decode step has done the
        # addition on the device already (tgis_decode_advance)
        if first:
            batch.cu_seqlens.add_(batch.cu_seqlens_q)
        batch.max_seqlen = max(batch.input_lengths)  # one more token; a verify step adds up to K + 1 to a request
        if first and self.spec_tokens:
            self.drafter.start(batch, embeds)
        if spec_before is not None:
            after = self.spec_stats()
            logging.debug("speculative decoding, batch %s: %s", batch.batch_id,
                          {k: after[k] - spec_before[k] for k in after})
        return generated_tokens, input_token_infos, decode_errors, forward_time_ns

    def _prefill_forward(self, batch: FlashCausalLMBatch):
        """The prompts' logits alone."""
        return self._prefill(batch)[0]

    def _prefill(self, batch: FlashCausalLMBatch):
        """(logits, the rows that went into lm_head if the drafter needs them, else None) of the batch's prompts."""
        before = self.kv_cache.reuse_stats() if self.kv_prefix_reuse else None
        batch.allocate_pages(self.kv_cache)
        self._need_all_logits = any(r.details.input_toks for r in batch.requests)
        if any(batch.reused_lengths):
            out = self._prefill_suffix_forward(batch)
        else:
            out = self._prefill_fresh_forward(batch)
        batch.register_prompt_pages()
        if before is not None and logging.getLogger().isEnabledFor(logging.DEBUG):
            after = self.kv_cache.reuse_stats()
            logging.debug("KV prefix reuse, batch %s: %s", batch.batch_id, {k: after[k] - before[k] for k in after})
        return out

    def _prefill_suffix_forward(self, batch: FlashCausalLMBatch):
        """The prefill of a batch of which at least one request found its leading pages in the cache (KV prefix reuse): only
        the tokens behind them go through the model, at their true positions, attending over the whole context; their k and
        v are written page-wise starting at the first own page.  `batch.cu_seqlens`, `position_ids` and the rest of the
        reference's logical slot contract stay those of the whole prompts."""
        lens, hits = batch.input_lengths, batch.reused_lengths
        starts = np.cumsum([0] + lens[:-1])
        take = np.concatenate([s + np.arange(h, l) for s, h, l in zip(starts, hits, lens)])
        positions = np.concatenate([np.arange(h, l) for h, l in zip(hits, lens)]).astype(np.int32)
        slots = np.concatenate([
            np.asarray(p, dtype=np.int64)[np.arange(h, l) // PAGE] * PAGE + np.arange(h, l) % PAGE
            for p, h, l in zip(batch.pages, hits, lens)]).astype(np.int32)
        suffix = [l - h for h, l in zip(hits, lens)]
        cu_q = np.concatenate([[0], np.cumsum(suffix)]).astype(np.int32)
        dev = self.device
        up = (lambda a: torch.from_numpy(a).to(dev, non_blocking=True))
        cu_q = up(cu_q)
        max_q, max_ctx = max(suffix), max(lens)
        # a few tokens over a long cached context are the decode forms of the attention: their key splits apply
        kv = KVArgs(cache=self.kv_cache, block_tables=batch.block_tables,
                    ctx_lens=torch.tensor(lens, dtype=torch.int32, device=dev), slots=up(slots),
                    max_q_len=max_q, max_ctx=max_ctx,
                    num_splits=native.attn_q_splits(len(lens), self.num_kv_heads, self.num_heads, max_q, max_ctx),
                    past_lens=native.past_lens_tensor(hits, dev) if FRESH_PREFILL_KV else None)
        return self._forward_prefill(batch.input_ids.index_select(0, up(take)), up(positions), cu_q, batch.max_seqlen, None,
                                     kv, (cu_q[1:] - 1).long(), lora=self._prefill_lora(batch, suffix))

    def _forward_prefill(self, *args, lora=None):
        """(logits, hidden rows or None): the model's forward; a drafter that needs them also gets the rows that went into
        lm_head (`return_embeds`).  lora: the LoraArgs of a prefill that carries adapter rows."""
        if lora is not None:
            return self.model.forward(*args, lora=lora), None
        if self.drafter is not None and self.drafter.needs_hidden:
            return self.model.forward(*args, return_embeds=True)
        return self.model.forward(*args), None

    def _load_adapter(self, slot: int, adapter: LoraAdapter):
        """The slot table's upload: the adapter's tensors into `slot` of every wrapped linear, as copies on the current
        stream (a captured decode graph reads the slot images at fixed addresses and sees them on its next replay)."""
        for lin in self.lora_linears:
            lin.load(slot, adapter)

    def _prefill_lora(self, batch: FlashCausalLMBatch, rows_per_request: List[int]) -> Optional[LoraArgs]:
        """The LoraArgs of a prefill whose request i brings rows_per_request[i] rows, None when no request carries an
        adapter.  Up to 64 rows take the kernels (grouped on the device); longer forwards loop on the host over the
        requests that carry one, whose rows are contiguous."""
        if not batch.has_lora():
            return None
        slots = np.repeat(np.asarray(batch.lora_slots, dtype=np.int32), rows_per_request)
        dev_slots = torch.from_numpy(slots).to(self.device, non_blocking=True)
        if slots.size <= native.LORA_MAX_T:
            return LoraArgs.grouped(dev_slots, self.lora_slots)
        starts = np.concatenate([[0], np.cumsum(rows_per_request)])
        ranges = [(int(starts[i]), int(starts[i + 1]), s) for i, s in enumerate(batch.lora_slots)
                  if s >= 0 and rows_per_request[i] > 0]
        return LoraArgs(slots=dev_slots, ranges=ranges)

    def _prefill_fresh_forward(self, batch: FlashCausalLMBatch):
        lens = batch.input_lengths
        slots = np.concatenate([
            np.asarray(p, dtype=np.int64)[np.arange(l) // PAGE] * PAGE + np.arange(l) % PAGE
            for p, l in zip(batch.pages, lens)]).astype(np.int32)
        dev = self.device
        kv = KVArgs(cache=self.kv_cache, block_tables=batch.block_tables,
                    ctx_lens=torch.tensor(lens, dtype=torch.int32, device=dev),
                    slots=torch.from_numpy(slots).to(dev, non_blocking=True),
                    max_q_len=max(lens), max_ctx=max(lens), num_splits=1, fresh_prefill=FRESH_PREFILL_KV,
                    window=self.sliding_window)
        lm_head_indices = None if self._need_all_logits else (batch.cu_seqlens[1:] - 1).long()
        return self._forward_prefill(batch.input_ids, batch.position_ids.to(torch.int32), batch.cu_seqlens,
                                     batch.max_seqlen, batch.inputs_embeds, kv, lm_head_indices,
                                     lora=self._prefill_lora(batch, lens))

    def _decode_forward(self, batch: FlashCausalLMBatch):
        verify = self.spec_tokens > 0 and self._grow_for_verify(batch)
        if not verify:
            batch.grow_pages()
        key = (graph_bucket(len(batch)), batch.block_tables.shape[1])
        tree = verify and self.spec_candidates > 1
        if verify:
            key += (self.spec_tokens, self.spec_candidates) if tree else (self.spec_tokens,)
        # a step in which some row carries a LoRA adapter runs its own graph (the unfused linears plus the deltas, over a
        # static slot buffer); batches without adapters keep the plain key and the plain graph
        lora = self.lora_slots > 0 and batch.has_lora()
        if lora:
            key += (LORA_KEY,)
        g = self._graphs.get(key)
        if g is None:
            while len(self._graphs) >= self.max_graphs:
                self._graphs.popitem(last=False)
            renew_unheld_pool(self)
            kind = _LoraDecodeGraph if lora else _TreeVerifyGraph if tree else _VerifyGraph if verify else _DecodeGraph
            g = self._graphs[key] = kind(self, *key)
        else:
            self._graphs.move_to_end(key)
        if lora:
            logits, ids, lps = g.run(batch.input_ids, batch.position_ids, batch.block_tables, batch.lora_slots_device())
        elif verify:
            logits, ids, lps = g.run(batch.input_ids, batch.position_ids, batch.block_tables, batch.spec_drafts)
        else:
            logits, ids, lps = g.run(batch.input_ids, batch.position_ids, batch.block_tables)
        return logits, (ids, lps, g)

    def _grow_for_verify(self, batch: FlashCausalLMBatch) -> bool:
        """Whether this decode step verifies the batch's drafts (utils/spec_decode.py, fallback_cause); if so its requests
        own the pages of K + 1 more tokens afterwards (C K + 1 with C candidates per request: one cache position per row).  A
        pool that cannot provide them is one more cause to run the plain step, which grows by one token as it always did:
        speculation never exhausts the pool by itself."""
        K, C, st = self.spec_tokens, self.spec_candidates, self._spec_stats
        st["decode_steps"] += 1
        ntc = batch.next_token_chooser
        plain_greedy = ntc.is_plain_greedy
        # spec_sampling: what the step rule needs is a chooser for K + 1 rows per request on the device, and the fused one
        # serves every batch (`_process_spec_tokens`); top-n tokens and ranks remain a cause of their own
        greedy = (plain_greedy or self.spec_sampling) and batch.spec_hits is not None
        cause = fallback_cause(
            K, graph_bucket(len(batch)), greedy, any(r.details.top_n_toks or r.details.ranks for r in batch.requests),
            [t - n for t, n in zip(batch.total_lengths, batch.input_lengths)], batch.spec_hits_host, C)
        if cause is None:
            try:
                batch.grow_pages(ahead=C * K)
            except OutOfPages:
                cause = "pages"
        if cause is not None:
            st["fallback_" + cause] += 1
            return False
        st["verify_steps"] += 1
        if not plain_greedy:
            st["verify_steps_sampled"] += 1
        return True

    def _process_prefill(self, batch: FlashCausalLMBatch, out):
        generated_tokens: List[TokenInfo] = []
        input_token_infos: List[InputTokens] = []
        decode_errors: List[GenerateError] = []
        # position ids of the first generated token, set before input lengths are incremented
        batch.position_ids = batch.position_ids.new_tensor(batch.input_lengths)
        batch.input_ids = self._process_new_tokens(batch, out, generated_tokens, decode_errors, input_token_infos,
                                                   True, None)
        batch.inputs_embeds = None
        batch.cu_seqlens_q = torch.arange(len(batch) + 1, device=self.device, dtype=torch.int32)
        return generated_tokens, input_token_infos, decode_errors

    def _process_decode(self, batch: FlashCausalLMBatch, out, fused):
        generated_tokens: List[TokenInfo] = []
        decode_errors: List[GenerateError] = []
        # position_ids += 1, the scatter into all_input_ids and cu_seqlens += cu_seqlens_q happen in _process_new_tokens
        batch.input_ids = self._process_new_tokens(batch, out, generated_tokens, decode_errors, None, False, fused)
        return generated_tokens, decode_errors

    def _process_new_tokens(self, batch: FlashCausalLMBatch, out, generated_tokens: List[TokenInfo],
                            decode_errors: List[GenerateError], input_token_infos: Optional[List[InputTokens]],
                            prefill: bool, fused):
        if prefill and self._need_all_logits:
            logits = out[batch.cu_seqlens[1:] - 1, :]  # out is [sum(lengths), vocab]
        else:
            logits = out  # already one row per request

        ntc = batch.next_token_chooser
        details = any(r.details.top_n_toks or r.details.ranks for r in batch.requests)
        plain_greedy = ntc.is_plain_greedy
        simple = plain_greedy and not details
        graph = None if prefill else fused[2]  # the prefill is the one caller without a captured step
        if self.spec_tokens and not prefill:
            self._spec_stats["emitted"] += len(batch)  # (a verify step adds the drafts it accepted)
            if batch.spec_hits is not None and not details and (plain_greedy or self.spec_sampling):
                # verify or plain (K = 0).  spec_sampling: the fused chooser behind every row in place of the captured argmax
                return spec_step(self, batch, fused, generated_tokens, logits=None if plain_greedy else logits)
        read_host = None
        if not simple:
            # EOS mask / length penalty, repetition penalty, warpers, argmax or draw, log-softmax at the chosen id:
            # one launch (tgis_warp_sample) and, below, one device->host copy for the whole batch
            next_token_ids, next_logprobs, lse, next_token_scores = ntc.choose_fused(
                batch.all_input_ids_tensor[:, :batch.max_seqlen], logits)
        elif prefill:
            next_token_ids, next_logprobs = ntc.choose_greedy_fused(logits)
        else:
            # one kernel (already part of the decode graph), one device->host copy for the whole batch
            next_token_ids, next_logprobs = fused[:2]
            read_host = graph.fetch_greedy()  # the copy is on its way while the bookkeeping launch below runs

        if prefill:
            batch.all_input_ids_tensor.scatter_(dim=1, index=batch.position_ids[:, None], src=next_token_ids[:, None])
        else:
            # reference :499 `position_ids += 1`, :533 the scatter, :457 `cu_seqlens.add_`, and the copy of the ids out of
            # the buffer the next step overwrites — one launch, which also leaves the next step's inputs in the static
            # buffers of the graph that will run it
            next_token_ids = native.decode_advance(
                next_token_ids, batch.position_ids, batch.all_input_ids_tensor, batch.cu_seqlens, batch.cu_seqlens_q,
                stage_ids=graph.input_ids[:len(batch)], stage_positions=graph.positions[:len(batch)])
            graph.staged_ids, graph.staged_pos = next_token_ids, batch.position_ids
            if self.spec_tokens:  # (a batch below its min_new_tokens turns plain greedy without being rebuilt)
                self.drafter.after_step(batch, graph, next_token_ids, None, 1, None, False)

        if read_host is not None:
            ids_host, lps_host = read_host(any(ntc.return_logprobs))
        else:
            ids_host = next_token_ids.tolist()
            lps_host = next_logprobs.tolist() if any(ntc.return_logprobs) else None
        for i, request in enumerate(batch.requests):
            try:
                if not simple and (request.details.top_n_toks or request.details.ranks):
                    # top-n tokens and ranks are read from the warped scores of this row (tokens.py:388-425)
                    row = next_token_scores[i:i + 1]
                    info = get_token_info(request, row, next_token_ids[i:i + 1],
                                          row - lse[i] if request.details.logprobs else None)
                else:
                    info = TokenInfo(request_id=request.id, token_id=ids_host[i])
                    if lps_host is not None and request.details.logprobs:
                        info.logprob = lps_host[i]
                generated_tokens.append(info)
                if prefill and request.details.input_toks:
                    self._append_input_tokens(batch, out, i, request, input_token_infos)
            except Exception as e:
                logging.exception(f"token decoding error for request #{request.id}")
                decode_errors.append(GenerateError(request_id=request.id,
                                                   message=f"Token decoding error: {str(e)}"))
            batch.input_lengths[i] += 1
        return next_token_ids

    @staticmethod
    def _append_input_tokens(batch, out, i, request, input_token_infos):
        start = int(batch.cu_seqlens[i])
        input_length = batch.input_lengths[i]
        # the last position's logits predict the generated token, not an input token
        logits = out[start:start + input_length - 1, :]
        input_token_infos.append(get_input_tokens_info(request, batch.all_input_ids_tensor[i, :input_length], logits))
