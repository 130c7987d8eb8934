"""The captured decode step of FlashCausalLM: static buffers + HIP graph per (batch-size bucket, table width), the choice
between one graph and a chain of segments under tensor parallelism, and the memory pool the captures share.  With
speculative decoding on (utils/spec_decode.py) the verify step is captured the same way, per (bucket, table width, K) — with
several candidates per request per (bucket, table width, K, C), a token tree of 1 + C K rows per request; what drafts and what
follows such a step is models/speculation.py.

The state stays on the model, where bench.py, the tests and tools/ read and set it: `lm._graphs`, `lm.graph_captures`,
`lm.use_graphs`, `lm.max_graphs`, `lm.graph_mode`, `lm.graph_pool`, `lm.tp_world`, `lm.ranks` (utils/rank_group.py)."""
import logging
import time

import torch

from tgis_amd import native
from tgis_amd.models.custom_modeling.flash_common import KVArgs
from tgis_amd.utils.graph_segments import SegmentedGraph, no_gc_during_capture
from tgis_amd.utils.kv_cache import PAGE
from tgis_amd.utils.spec_decode import tree_q_mask, tree_rows

logger = logging.getLogger(__name__)


def renew_unheld_pool(lm):
    """The allocator retires a graph pool with the last captured graph that holds it (every graph evicted, or a failed full
    capture that took the pool's only graph with it): captures that follow start a new one."""
    if lm.use_graphs and not any(d.graph is not None for d in lm._graphs.values()):
        lm.graph_pool = torch.cuda.graph_pool_handle()


def resolve_graph_mode(lm) -> str:
    """"full" or "segments"; `auto` is settled once, identically on every rank."""
    if lm.graph_mode == "auto":
        try:
            works = _collective_capture_works(lm)
        except Exception as exc:  # an unusable probe must not take the server down: segments need no capture of RCCL
            logger.warning("probing RCCL graph capture failed (%s)", exc)
            works = False
        lm.graph_mode = "full" if works else "segments"
        logger.info("tensor-parallel decode graphs: %s", lm.graph_mode)
    return lm.graph_mode


def _collective_capture_works(lm) -> bool:
    if not lm.ranks.nccl:
        return False  # host-mediated collectives synchronise: they can never be inside a capture
    pg = lm.ranks.process_group
    world = pg.size()
    t = torch.ones(1024, device=lm.device, dtype=torch.float32)
    try:
        torch.distributed.all_reduce(t, group=pg)  # communicator up before any capture
        torch.cuda.synchronize(lm.device)
        t.fill_(1.0)
        g = torch.cuda.CUDAGraph()
        with no_gc_during_capture(), torch.cuda.graph(g, capture_error_mode="thread_local"):
            torch.distributed.all_reduce(t, group=pg)
        g.replay()
        g.replay()
        torch.cuda.synchronize(lm.device)
        ok = bool((t == float(world * world)).all().item())
    except Exception as exc:
        logger.warning("RCCL inside a captured graph is not usable here (%s)", exc)
        native.clear_error()
        ok = False
    return lm.ranks.all_true(ok)


class _SpecOut:
    """What a greedy step of a speculating model sends to the host, in ONE device buffer and one copy to its pinned mirror:
    the emitted ids int64 [B, K + 1] and their logprobs f32 [B, K + 1] (tgis_spec_accept), how many of them count, n_emit
    int32 [B], and the hits int32 [B] of the lookup that drafted the next step (tgis_spec_propose).  `best`: a tree verify
    step adds the winning candidate int32 [B] (tgis_spec_tree_accept) behind them."""

    def __init__(self, B: int, K: int, dev, best: bool = False):
        R = B * (K + 1)
        self.K1 = K + 1
        size = R * 12 + B * (12 if best else 8)
        self.buf = torch.zeros(size, dtype=torch.uint8, device=dev)
        self.host = torch.zeros(size, dtype=torch.uint8).pin_memory()
        self.ids, self.lps, self.n_emit, self.hits = self._views(self.buf, B, R)
        self.best = self.buf[R * 12 + B * 8:].view(torch.int32) if best else None
        self.ready = torch.cuda.Event()

    @staticmethod
    def _views(buf, B, R):
        return (buf[:R * 8].view(torch.int64), buf[R * 8:R * 12].view(torch.float32),
                buf[R * 12:R * 12 + B * 4].view(torch.int32), buf[R * 12 + B * 4:R * 12 + B * 8].view(torch.int32))

    def read_best(self, n: int):
        """best [n] of the first n requests as a host list (behind `read`, which waited for the copy)."""
        B = self.n_emit.numel()
        return self.host[B * self.K1 * 12 + B * 8:].view(torch.int32)[:n].tolist()

    def fetch(self):
        self.host.copy_(self.buf, non_blocking=True)
        self.ready.record()

    def read(self, n: int, want_logprobs: bool):
        """(ids [n * (K + 1)], logprobs or None, n_emit [n], hits [n]) of the first n requests, as host lists."""
        self.ready.synchronize()
        B = self.n_emit.numel()
        ids, lps, n_emit, hits = self._views(self.host, B, B * self.K1)
        return (ids[:n * self.K1].tolist(), lps[:n * self.K1].tolist() if want_logprobs else None, n_emit[:n].tolist(),
                hits[:n].tolist())


class _DecodeGraph:
    """Static buffers + captured HIP graph of one decode step for a (batch-size bucket, table width) pair."""

    K = 0  # drafts per request: none in the plain step
    C = 1  # draft chains per request (more than one: _TreeVerifyGraph)

    def __init__(self, lm, B: int, width: int):
        self._init_buffers(lm, B, width, B)
        dev = lm.device
        self.ctx = torch.ones(B, dtype=torch.int32, device=dev)
        self.cu_q = torch.arange(B + 1, dtype=torch.int32, device=dev)
        # sliding-window attention: a graph whose table cannot hold more than W keys is the causal graph; a wider one makes
        # the windowed launch, its key splits sized for the keys a step can see (W of them over at most W + 31 slots of pages)
        W = getattr(lm, "sliding_window", None)
        self.window = W if W is not None and self.max_ctx > W else None
        keys = self.max_ctx if self.window is None else min(self.max_ctx, self.window + PAGE - 1)
        self.num_splits = native.attn_num_splits(B, lm.num_kv_heads, lm.num_heads, 1, keys)
        # a speculating model's plain steps report through tgis_spec_accept (K = 0) too: the next lookup's hits ride along
        self.spec_out = _SpecOut(B, 0, dev) if lm.spec_tokens else None

    def _init_buffers(self, lm, B: int, width: int, R: int):
        """What the plain and the verify step share: the per-request inputs, and R rows of slots and greedy outputs."""
        dev = lm.device
        self.rows = B
        self.active = 0  # rows [0, active) hold a batch's sequences, the rest are inactive
        self.input_ids = torch.zeros(B, dtype=torch.int64, device=dev)
        self.positions = torch.zeros(B, dtype=torch.int32, device=dev)
        self.block_tables = torch.full((B, width), lm.kv_cache.null_page, dtype=torch.int32, device=dev)
        self.slots = torch.zeros(R, dtype=torch.int32, device=dev)
        self.max_ctx = width * PAGE
        self.lm = lm
        self.graph = None
        self.logits = self.ids = self.logprobs = None
        # greedy ids (int64) and their logprobs (f32) in ONE device buffer: one copy to the (pinned) host mirror per step
        self.out_buf = torch.zeros(R * 12, dtype=torch.uint8, device=dev)
        self.ids_buf = self.out_buf[:R * 8].view(torch.int64)
        self.lps_buf = self.out_buf[R * 8:].view(torch.float32)
        self.argmax_scratch = native.argmax_scratch(R, dev)
        self.host_buf = torch.zeros(R * 12, dtype=torch.uint8).pin_memory()
        self.host_ready = torch.cuda.Event()
        # whose next-step inputs the static buffers already hold (tgis_decode_advance wrote them): identity of the
        # batch's tensors, so that a pruned / concatenated / other batch always stages its own
        self.staged_ids = self.staged_pos = self.staged_bt = None
        # a drafter that needs them (models/speculation.py) reads the rows that went into lm_head: `hidden` [R, E] is what the
        # latest step left there, `_static_hidden` the tensor the captured step writes; `chain` is the drafter's, its launches
        # behind this step as a captured graph that goes with this one
        self.hidden = self._static_hidden = self.chain = self._capture_entry = None

    def _forward(self, ids, positions, kv):
        lm = self.lm
        if lm.drafter is None or not lm.drafter.needs_hidden:
            return lm.model.forward(ids, positions, self.cu_q, self.max_ctx, None, kv)
        logits, self.hidden = lm.model.forward(ids, positions, self.cu_q, self.max_ctx, None, kv, return_embeds=True)
        return logits

    def fetch_greedy(self):
        """ids and logprobs of the step that just ran, as host lists: one device->host copy, one wait."""
        self.host_buf.copy_(self.out_buf, non_blocking=True)
        self.host_ready.record()
        return self._read_host

    def _read_host(self, want_logprobs: bool):
        self.host_ready.synchronize()
        B = self.ids_buf.numel()
        ids = self.host_buf[:B * 8].view(torch.int64).tolist()
        return ids, (self.host_buf[B * 8:].view(torch.float32).tolist() if want_logprobs else None)

    def _step(self):
        lm = self.lm
        native.decode_slots(self.positions, self.block_tables, self.slots, self.ctx)
        kv = KVArgs(cache=lm.kv_cache, block_tables=self.block_tables, ctx_lens=self.ctx, slots=self.slots,
                    max_q_len=1, max_ctx=self.max_ctx, num_splits=self.num_splits, window=self.window)
        logits = self._forward(self.input_ids, self.positions, kv)
        ids, lps = native.argmax_logprob(logits, ids_out=self.ids_buf, logprob_out=self.lps_buf, scratch=self.argmax_scratch)
        return logits, ids, lps

    def run(self, input_ids, position_ids, block_tables):
        """One decode step of a batch of n <= rows sequences; returns (logits, ids, logprobs) of its n rows."""
        n = self._stage(input_ids, position_ids, block_tables)
        logits, ids, lps = self._run()
        return (logits, ids, lps) if n == self.rows else (logits[:n], ids[:n], lps[:n])

    def _stage(self, input_ids, position_ids, block_tables) -> int:
        """The batch's inputs into the static buffers (those the launch after the last step left there are skipped)."""
        n = input_ids.numel()
        if n < self.active:  # rows a larger batch used before: inactive again
            self.positions[n:self.active].zero_()
            self.input_ids[n:self.active].zero_()
            self.block_tables[n:self.active].fill_(self.lm.kv_cache.null_page)
        self.active = n
        if input_ids is not self.staged_ids or position_ids is not self.staged_pos:
            self.input_ids[:n].copy_(input_ids, non_blocking=True)
            self.positions[:n].copy_(position_ids, non_blocking=True)
        if block_tables is not self.staged_bt:
            self.block_tables[:n].copy_(block_tables, non_blocking=True)
            self.staged_bt = block_tables
        self.staged_ids = self.staged_pos = None
        return n

    def _run(self):
        if not self.lm.use_graphs:
            return self._step()
        if self.graph is None:
            t_capture = time.perf_counter()
            # warm-up: sizes the workspaces, builds rope tables and (tp > 1) initialises the RCCL communicators outside
            # the capture
            self._step()
            torch.cuda.current_stream().synchronize()
            g = None
            if resolve_graph_mode(self.lm) == "full":
                g = torch.cuda.CUDAGraph()
                # tp > 1: RCCL's proxy and watchdog threads may call the runtime while this thread captures
                kw = {"capture_error_mode": "thread_local"} if self.lm.tp_world > 1 else {}
                ok = True
                try:
                    with no_gc_during_capture(), torch.cuda.graph(g, pool=self.lm.graph_pool, **kw):
                        self.logits, self.ids, self.logprobs = self._step()
                except Exception as exc:
                    if self.lm.tp_world == 1:
                        raise
                    logger.warning("capturing the tensor-parallel step with RCCL inside failed (%s)", exc)
                    native.clear_error()
                    ok = False
                if self.lm.tp_world > 1 and not self.lm.ranks.all_true(ok):
                    # one rank failing is every rank's failure: all of them leave `full` together, or their collective
                    # sequences would diverge (a capture issues no collective, so nobody is waiting inside one here)
                    self.lm.graph_mode = "segments"
                    g = None
            if g is None:
                renew_unheld_pool(self.lm)
                g = SegmentedGraph(self.lm.device, pool=self.lm.graph_pool)
                try:
                    self.logits, self.ids, self.logprobs = g.record(self._step)
                except Exception as exc:  # keep serving: the eager step needs nothing the capture set up
                    logger.warning("segmented capture of the decode step failed (%s); running eagerly", exc)
                    native.clear_error()
                    self.lm.use_graphs = False
                    return self._step()
            self.graph = g
            self._static_hidden = self.hidden
            # (rows, table width, host ms of warm-up step + capture, K): what a new (bucket, width[, K]) key costs a serving step
            self._capture_entry = (self.rows, self.block_tables.shape[1], (time.perf_counter() - t_capture) * 1e3, self.K)
            self.lm.graph_captures.append(self._capture_entry)
        self.graph.replay()
        if self._static_hidden is not None:
            self.hidden = self._static_hidden  # (an eager step in between, lm.use_graphs switched off, left its own there)
        return self.logits, self.ids, self.logprobs


LORA_KEY = "lora"  # the trailing marker of the graph key of a step in which some row carries a LoRA adapter


class _LoraDecodeGraph(_DecodeGraph):
    """The decode step of a batch in which some request carries a LoRA adapter (utils/lora.py), for a (batch-size bucket,
    table width, LORA_KEY) key: the plain step's buffers plus a static `lora_slots` int32 [bucket], staged per run with the
    inactive rows at -1.  The captured step groups the rows by slot on the device (tgis_lora_group) and every wrapped linear
    adds its delta from the slot images, so a replay follows whatever slots, and whatever adapters in them, a step brings."""

    def __init__(self, lm, B: int, width: int, marker: str = LORA_KEY):
        assert marker == LORA_KEY
        super().__init__(lm, B, width)
        self.lora_slots = torch.full((B,), -1, dtype=torch.int32, device=lm.device)
        self.staged_slots = None

    def _forward(self, ids, positions, kv):
        from tgis_amd.utils.lora import LoraArgs

        lm = self.lm
        return lm.model.forward(ids, positions, self.cu_q, self.max_ctx, None, kv,
                                lora=LoraArgs.grouped(self.lora_slots, lm.lora_slots))

    def run(self, input_ids, position_ids, block_tables, slots):
        """One decode step of a batch of n <= rows sequences whose adapter slots are `slots` int32 [n] (device)."""
        n = input_ids.numel()
        if n < self.active:
            self.lora_slots[n:self.active].fill_(-1)
        if slots is not self.staged_slots or n != self.active:
            self.lora_slots[:n].copy_(slots, non_blocking=True)
            self.staged_slots = slots
        return super().run(input_ids, position_ids, block_tables)


class _VerifyGraph(_DecodeGraph):
    """The verify step of speculative decoding for a (batch-size bucket, table width, K) triple: K + 1 rows per request, its
    latest token and its K drafts, through the generic q_len > 1 forward (rotary and cache write per token, the attention's
    decode form, with key splits from 1024 keys on), then the greedy choice behind every row.  `input_ids` / `positions` stay the
    per-request inputs, as in the plain step, so that the launch after either step can leave the next inputs in them."""

    def __init__(self, lm, B: int, width: int, K: int, C: int = 1):
        """C > 1 is _TreeVerifyGraph's: C chains per request, 1 + C K rows, drafts [B, C, K]."""
        R1 = tree_rows(C, K)  # rows per request (K + 1 for the one chain)
        R = B * R1
        self._init_buffers(lm, B, width, R)
        dev = lm.device
        self.K, self.C, self.R1 = K, C, R1
        self.drafts = torch.zeros((B, K) if C == 1 else (B, C, K), dtype=torch.int64, device=dev)
        self.row_ids = torch.zeros(R, dtype=torch.int64, device=dev)
        self.row_positions = torch.zeros(R, dtype=torch.int32, device=dev)
        self.ctx = torch.full((B,), R1, dtype=torch.int32, device=dev)
        self.cu_q = torch.arange(B + 1, dtype=torch.int32, device=dev) * R1
        # the decode form takes key splits over a long context (tgis_attn_num_splits_q); captured and eager steps share them
        self.num_splits = native.attn_q_splits(B, lm.num_kv_heads, lm.num_heads, R1, self.max_ctx)
        self.spec_out = _SpecOut(B, K, dev, best=C > 1)

    def _step(self):
        lm = self.lm
        native.spec_stage(self.positions, self.input_ids, self.drafts, self.block_tables, self.row_ids, self.row_positions,
                          self.slots, self.ctx)
        kv = KVArgs(cache=lm.kv_cache, block_tables=self.block_tables, ctx_lens=self.ctx, slots=self.slots,
                    max_q_len=self.K + 1, max_ctx=self.max_ctx, num_splits=self.num_splits)
        logits = self._forward(self.row_ids, self.row_positions, kv)
        ids, lps = native.argmax_logprob(logits, ids_out=self.ids_buf, logprob_out=self.lps_buf, scratch=self.argmax_scratch)
        return logits, ids, lps

    def run(self, input_ids, position_ids, block_tables, drafts):
        """One verify step of a batch of n <= rows sequences; returns (logits, ids, logprobs) of its n (K + 1) rows."""
        n = input_ids.numel()
        if n < self.active:
            self.drafts[n:self.active].zero_()
        self.drafts[:n].copy_(drafts, non_blocking=True)
        self._stage(input_ids, position_ids, block_tables)
        logits, ids, lps = self._run()
        r = n * self.R1
        return logits[:r], ids[:r], lps[:r]


class _TreeVerifyGraph(_VerifyGraph):
    """The verify step over C candidates per request for a (batch-size bucket, table width, K, C) key: R = 1 + C K rows per
    request as a token tree (utils/spec_decode.py: row 0 the latest token, row 1 + c K + j draft j of candidate c, rotary
    position by depth, cache position by row), through the same generic q_len > 1 forward; the attention takes the static
    `q_mask` (tgis_attn_paged_tree) under which a row sees the cache, row 0 and its own candidate up to itself.  `run` is
    _VerifyGraph's, on drafts [n, C, K]."""

    def __init__(self, lm, B: int, width: int, K: int, C: int):
        super().__init__(lm, B, width, K, C)
        # built once on the host: every request of the bucket has the same tree
        self.q_mask = torch.tensor(tree_q_mask(C, K) * B, dtype=torch.int64, device=lm.device)

    def _step(self):
        lm = self.lm
        native.spec_tree_stage(self.positions, self.input_ids, self.drafts, self.block_tables, self.row_ids,
                               self.row_positions, self.slots, self.ctx)
        kv = KVArgs(cache=lm.kv_cache, block_tables=self.block_tables, ctx_lens=self.ctx, slots=self.slots,
                    max_q_len=self.R1, max_ctx=self.max_ctx, num_splits=self.num_splits, q_mask=self.q_mask)
        logits = self._forward(self.row_ids, self.row_positions, kv)
        ids, lps = native.argmax_logprob(logits, ids_out=self.ids_buf, logprob_out=self.lps_buf, scratch=self.argmax_scratch)
        return logits, ids, lps
