"""Speculative decoding on the model's side (the host rules are utils/spec_decode.py): who drafts, and the
decode step of a speculating model.  FlashCausalLM holds one drafter (`lm.drafter`, None with the option off) and every batch
it prefilled points at it (`batch.spec_model`).  A drafter has

    needs_hidden                whether the forward must also return the rows that fed lm_head (`return_embeds`)
    start(batch, embeds)        behind the prefill: the batch's speculation fields and its first drafts; `embeds` is what the
                                forward returned with `return_embeds`, or None
    redraft(batch)              drafts from the batch's own tensors: behind concatenate and prune, and when stale drafts are
                                asked for (`batch.spec_hits_host`)
    after_step(batch, graph, latest_ids, n_emit, stride, hits_copy, drafting)
                                behind tgis_spec_accept* (n_emit [B], stride K + 1) or tgis_decode_advance (None, 1): the
                                next step's drafts if `drafting`, else they are marked stale

and there are two: the prompt lookup and the MLP speculator.  `spec_step` is what follows a decode step whose tokens
tgis_spec_accept* emits."""
import time
from typing import List, Optional

import numpy as np
import torch

from tgis_amd import native
from tgis_amd.utils.graph_segments import no_gc_during_capture
from tgis_amd.utils.mlp_speculator import MLPSpeculator
from tgis_amd.utils.token_types import TokenInfo


class LookupDrafter:
    """Drafts looked up in the request's own context (tgis_spec_propose): the tokens behind the latest earlier occurrence of
    its longest suffix of up to `ngram` tokens.  With `candidates` = C > 1 (tgis_spec_propose_multi) up to C chains per
    request, `batch.spec_drafts` [B, C, K]: further sites, latest first and longest suffix first, whose continuations start
    with a token no chain taken before starts with."""
    needs_hidden = False

    def __init__(self, spec_tokens: int, ngram: int, candidates: int = 1):
        self.K, self.ngram, self.C = spec_tokens, ngram, candidates

    def start(self, batch, embeds):
        batch.spec_tokens, batch.spec_model, batch.spec_candidates = self.K, self, self.C
        self.redraft(batch)

    def redraft(self, batch, hits_copy: Optional[torch.Tensor] = None):
        batch.ensure_spec_buffers()
        propose = native.spec_propose_multi if self.C > 1 else native.spec_propose
        propose(batch.all_input_ids_tensor, batch.position_ids, self.ngram, batch.spec_drafts, batch.spec_hits, hits_copy)
        batch.drafts_renewed()

    def after_step(self, batch, graph, latest_ids, n_emit, stride, hits_copy, drafting):
        if drafting:
            self.redraft(batch, hits_copy)
        else:
            batch.drafts_are_stale()


class MLPDrafter(MLPSpeculator):
    """The MLP speculator (utils/mlp_speculator.py) as the drafter: it predicts from `batch.spec_hidden`, per request the
    post-norm state that predicted its latest token, and the latest ids; its hits are all ones.  A bucket that can never
    verify (`batch.can_verify`) keeps the states and drafts nothing: the step rule answers `rows`, nobody reads drafts."""
    needs_hidden = True

    def start(self, batch, embeds):
        batch.spec_tokens, batch.spec_model = self.K, self
        if embeds.shape[0] != len(batch):  # details.input_toks: every prompt position went through lm_head
            ends = np.cumsum([n - 1 for n in batch.input_lengths]) - 1  # (input_lengths count the generated token by now)
            embeds = embeds.index_select(0, torch.from_numpy(ends).to(embeds.device))
        # the batch's own tensor: the state behind each prompt's last token
        batch.spec_hidden = native.spec_mlp_input(
            embeds.contiguous(), None, 1, torch.empty((len(batch), embeds.shape[1]), dtype=embeds.dtype, device=embeds.device))
        self.redraft(batch)

    def redraft(self, batch):
        batch.ensure_spec_buffers()
        if batch.can_verify():
            self.draft(batch.spec_hidden, batch.input_ids, batch.spec_drafts, batch.spec_hits)
        batch.drafts_renewed()

    def after_step(self, batch, graph, latest_ids, n_emit, stride, hits_copy, drafting):
        """The state behind each request's last emitted token into `batch.spec_hidden` (a step whose chooser samples or
        reports details leaves it too); then, `drafting`, the next drafts into `batch.spec_drafts`, ones into
        `batch.spec_hits` and `hits_copy`, which travels to the host.  Behind a captured step the two launches are a
        captured graph of their own, `graph.chain`; otherwise they are launched one by one."""
        batch.ensure_spec_buffers(self.cfg.emb_dim, graph.hidden.dtype)
        if not drafting:
            native.spec_mlp_input(graph.hidden, n_emit, stride, batch.spec_hidden)
            batch.drafts_are_stale()
            return
        if graph.lm.use_graphs and graph.graph is not None:
            if graph.chain is None:
                graph.chain = _DraftChain(self, graph)
            graph.chain.run(batch)
        else:
            self.state_then_draft(graph.hidden, n_emit, stride, batch.spec_hidden, latest_ids, batch.spec_drafts,
                                  batch.spec_hits, hits_copy)
        batch.drafts_renewed()

    def state_then_draft(self, hidden, n_emit, stride, state, latest_ids, drafts, hits, hits_copy, bufs=None):
        native.spec_mlp_input(hidden, n_emit, stride, state)
        self.draft(state, latest_ids, drafts, hits, hits_copy=hits_copy, bufs=bufs)


class _DraftChain:
    """The MLP drafter's launches behind one captured step, as a captured graph of their own: it reads that step's static
    `hidden`, `spec_out.n_emit` and `input_ids` (where tgis_spec_accept left the new latest ids) and writes buffers of its
    own, for every row of the bucket.  A row past the batch drafts from what the inactive row computed and token 0; nobody
    reads its drafts.  The chain belongs to its step graph: it is no key of `lm._graphs`, it goes when that graph is
    evicted, and its capture time is added to that graph's `graph_captures` entry."""

    def __init__(self, drafter: MLPDrafter, g):
        dev = g.lm.device
        self.drafter, self.g = drafter, g
        self.bufs = drafter.buffers(g.rows)
        self.raw = torch.zeros((g.rows, drafter.cfg.emb_dim), dtype=g.hidden.dtype, device=dev)
        self.drafts = torch.zeros((g.rows, drafter.K), dtype=torch.int64, device=dev)
        self.hits = torch.zeros(g.rows, dtype=torch.int32, device=dev)
        self.graph = None

    def _launch(self):
        g = self.g
        self.drafter.state_then_draft(g.hidden, g.spec_out.n_emit, g.K + 1, self.raw, g.input_ids, self.drafts, self.hits,
                                      g.spec_out.hits, self.bufs)

    def run(self, batch):
        g, lm = self.g, self.g.lm
        if self.graph is None:
            t_capture = time.perf_counter()
            self._launch()  # warm-up: sizes the GEMM workspace outside the capture (and drafts for real, once)
            torch.cuda.current_stream().synchronize()
            graph = torch.cuda.CUDAGraph()
            with no_gc_during_capture(), torch.cuda.graph(graph, pool=lm.graph_pool):
                self._launch()
            self.graph = graph
            caps, ms = lm.graph_captures, (time.perf_counter() - t_capture) * 1e3
            for i in range(len(caps) - 1, -1, -1):
                if caps[i] is g._capture_entry:
                    r, w, t, k = caps[i]
                    caps[i] = g._capture_entry = (r, w, t + ms, k)
                    break
        self.graph.replay()
        B = len(batch)
        # the batch's own tensors: another batch may run this graph next
        batch.spec_drafts.copy_(self.drafts[:B])
        batch.spec_hits.copy_(self.hits[:B])
        batch.spec_hidden.copy_(self.raw[:B])


def spec_step(lm, batch, fused, generated_tokens: List[TokenInfo], logits: Optional[torch.Tensor] = None):
    """What follows a decode step of a speculating model, verify (K drafts per request) or plain (K = 0): one launch
    accepts and does the bookkeeping of `_process_new_tokens` for up to K + 1 tokens per request (tgis_spec_accept),
    the drafter drafts the next step, one copy brings ids, logprobs, counts and the drafter's hits to the host.  Request i
    contributes n_emit[i] TokenInfos, in order; returns the latest ids [B].
    logits: None for a plain-greedy batch, whose rows the captured argmax chose.  Otherwise (spec_sampling) the step's
    logits [B (K + 1), V]: the fused chooser chooses behind every row as the plain step of that position would
    (tgis_warp_sample_verify: the request's parameters, its context plus the drafts in front of the row, the draw
    (seed, offset + j)), a draft is accepted while the chosen token equals it — for a deterministic drafter the
    rejection rule, accept with probability p(draft) — and tgis_spec_accept_sampled also advances each sampled
    request's stream by what it emitted.
    A tree verify step (graph.C > 1 candidates per request, greedy only): tgis_spec_tree_accept emits along the best
    candidate's path and tgis_spec_tree_commit, on the same stream, moves that candidate's keys and values to where a single
    chain would have written them, so that the cache and every later step are those of a chain step."""
    ids, lps, graph = fused
    B, K, K1, out = len(batch), graph.K, graph.K + 1, graph.spec_out
    C = graph.C
    ntc = batch.next_token_chooser
    outputs = dict(out_ids=out.ids[:B * K1], out_logprobs=out.lps[:B * K1], all_input_ids=batch.all_input_ids_tensor,
                   cu_seqlens=batch.cu_seqlens, stage_ids=graph.input_ids[:B], stage_positions=graph.positions[:B])
    drafts = batch.spec_drafts if K else None
    if C > 1:
        next_token_ids = native.spec_tree_accept(ids, lps, drafts, out.n_emit[:B], out.best[:B], batch.position_ids, **outputs)
        # (the positions tgis_spec_tree_accept just staged: the step's own are those minus n_emit)
        native.spec_tree_commit(lm.kv_cache.pool, batch.block_tables, graph.positions[:B], out.best[:B], out.n_emit[:B], C, K)
    elif logits is None:
        next_token_ids = native.spec_accept(ids, lps, drafts, out.n_emit[:B], batch.position_ids, **outputs)
    else:
        ids, lps, _lse, _scores = ntc.choose_fused_verify(batch.all_input_ids_tensor[:, :batch.max_seqlen], logits,
                                                          drafts, K)
        do_sample, rng = ntc.fused_streams(logits.device)
        next_token_ids = native.spec_accept_sampled(ids.view(-1), lps.view(-1), drafts, out.n_emit[:B],
                                                    batch.position_ids, do_sample=do_sample, rng=rng, **outputs)
    graph.staged_ids, graph.staged_pos = next_token_ids, batch.position_ids
    drafting = batch.can_verify()
    # (an MLP drafter's chain reads the latest ids tgis_spec_accept just wrote)
    lm.drafter.after_step(batch, graph, next_token_ids, out.n_emit[:B], K1, out.hits[:B], drafting)
    out.fetch()
    ids_host, lps_host, n_emit, hits = out.read(B, any(ntc.return_logprobs))
    if drafting:
        batch.note_spec_hits(hits)
    if logits is not None:
        ntc.commit_verify(n_emit)
    for i, request in enumerate(batch.requests):
        for j in range(i * K1, i * K1 + n_emit[i]):
            info = TokenInfo(request_id=request.id, token_id=ids_host[j])
            if lps_host is not None and request.details.logprobs:
                info.logprob = lps_host[j]
            generated_tokens.append(info)
        batch.input_lengths[i] += n_emit[i]
    if K:
        st = lm._spec_stats
        st["drafted"] += C * K * B  # every request's draft rows are verified, the zero drafts of a lookup that missed too
        st["accepted"] += sum(n_emit) - B
        st["emitted"] += sum(n_emit) - B
        if C > 1:  # what the later candidates bought: steps a request would have ended at its first chain's miss
            st["won_by_later_candidate"] += sum(1 for c, n in zip(out.read_best(B), n_emit) if c > 0 and n > 1)
    return next_token_ids
