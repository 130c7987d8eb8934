"""CPU: prompt-lookup speculative decoding on the host (utils/spec_decode.py and what FlashCausalLM / FlashCausalLMBatch do
with it): the options and their errors, which decode steps verify drafts and every cause of a plain step on its own, the
page look-ahead of `grow_pages` and its fallback on a CPU pool, and the numpy restatement (tests/spec_ref.py) on cases whose
answers are written out by hand.  No kernel runs."""
import numpy as np
import pytest
import torch

from tests import spec_ref
from tests.fixture_utils import FixtureTokenizer, prompt_text
from tgis_amd.models.flash_causal_lm import FlashCausalLM, FlashCausalLMBatch, graph_bucket
from tgis_amd.pb import generate_pb2 as pb2
from tgis_amd.utils import spec_decode as sd
from tgis_amd.utils.kv_cache import OutOfPages, PagedKVCache

CPU = torch.device("cpu")


# ---- options ----------------------------------------------------------------------------------------------------------------
def test_options_from_arguments_and_environment(monkeypatch):
    monkeypatch.delenv("TGIS_SPEC_TOKENS", raising=False)
    monkeypatch.delenv("TGIS_SPEC_NGRAM", raising=False)
    assert sd.parse_spec_tokens() == 0 and sd.parse_spec_ngram() == 3, "unset: off, and the default n-gram"
    assert [sd.parse_spec_tokens(k) for k in (0, 1, 7, "3", " 5 ")] == [0, 1, 7, 3, 5]
    assert [sd.parse_spec_ngram(n) for n in (1, 4, "2")] == [1, 4, 2]
    monkeypatch.setenv("TGIS_SPEC_TOKENS", "4")
    monkeypatch.setenv("TGIS_SPEC_NGRAM", "2")
    assert sd.parse_spec_tokens() == 4 and sd.parse_spec_ngram() == 2
    assert sd.parse_spec_tokens(0) == 0 and sd.parse_spec_ngram(1) == 1, "the argument wins over the environment"
    monkeypatch.setenv("TGIS_SPEC_TOKENS", "")
    assert sd.parse_spec_tokens() == 0


@pytest.mark.parametrize("bad", [-1, 8, 100, "x", "1.5", 2.0, True])
def test_bad_spec_tokens_raise(bad, monkeypatch):
    with pytest.raises(ValueError, match="spec_tokens"):
        sd.parse_spec_tokens(bad)
    if isinstance(bad, (int, str)) and not isinstance(bad, bool):
        monkeypatch.setenv("TGIS_SPEC_TOKENS", str(bad))
        with pytest.raises(ValueError, match="TGIS_SPEC_TOKENS"):
            sd.parse_spec_tokens()


@pytest.mark.parametrize("bad", [0, 5, -2, "n", 1.0])
def test_bad_spec_ngram_raise(bad, monkeypatch):
    with pytest.raises(ValueError, match="spec_ngram"):
        sd.parse_spec_ngram(bad)
    monkeypatch.setenv("TGIS_SPEC_NGRAM", str(bad))
    with pytest.raises(ValueError, match="TGIS_SPEC_NGRAM"):
        sd.parse_spec_ngram()


class _Engine:
    def __init__(self, world_size):
        self.world_size = world_size


def test_the_constructor_checks_the_options_before_anything_else(monkeypatch):
    """Bad values and tensor parallelism are refused before a weight is loaded or the GPU looked at."""
    monkeypatch.delenv("TGIS_SPEC_TOKENS", raising=False)
    with pytest.raises(ValueError, match="spec_tokens"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=_Engine(1), spec_tokens=8)
    with pytest.raises(ValueError, match="spec_ngram"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=_Engine(1), spec_tokens=3, spec_ngram=5)
    with pytest.raises(NotImplementedError, match="tensor parallelism is out of scope"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=_Engine(2), spec_tokens=3)
    monkeypatch.setenv("TGIS_SPEC_TOKENS", "2")
    with pytest.raises(NotImplementedError, match="tensor parallelism is out of scope"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=_Engine(4))
    sd.check_spec_world(0, 8)  # off: any world
    sd.check_spec_world(7, 1)


# ---- the step rule ------------------------------------------------------------------------------------------------------------
OK = dict(K=3, rows=4, plain_greedy=True, details=False, remaining=[9, 4, 30], hits=[0, 2, 0])


def test_a_step_that_meets_every_condition_verifies():
    assert sd.fallback_cause(**OK) is None


@pytest.mark.parametrize("change,cause", [
    (dict(plain_greedy=False), "not_greedy"),
    (dict(details=True), "details"),
    (dict(rows=24), "rows"),             # 24 * 4 = 96 > 64
    (dict(remaining=[9, 3, 30]), "remaining"),  # one request has K tokens left: one short of K + 1
    (dict(hits=[0, 0, 0]), "no_match"),
])
def test_each_cause_of_a_plain_step_on_its_own(change, cause):
    assert cause in sd.FALLBACK_CAUSES
    assert sd.fallback_cause(**{**OK, **change}) == cause


def test_the_row_bound_is_64_rows_of_the_bucket():
    assert sd.fallback_cause(**{**OK, "rows": 16}) is None            # 16 * 4 = 64
    assert sd.fallback_cause(**{**OK, "K": 7, "rows": 8, "remaining": [8]}) is None  # 8 * 8 = 64
    assert sd.fallback_cause(**{**OK, "K": 7, "rows": 16, "remaining": [8]}) == "rows"
    assert graph_bucket(9) == 16 and sd.fallback_cause(**{**OK, "K": 4, "rows": graph_bucket(9), "remaining": [8]}) == "rows"


def test_stats_have_one_counter_per_cause():
    st = sd.new_stats()
    assert set(st) == set(sd.SPEC_STATS) and not any(st.values())
    assert all("fallback_" + c in st for c in sd.FALLBACK_CAUSES)
    assert {"decode_steps", "verify_steps", "drafted", "accepted", "emitted"} <= set(st)


# ---- pages --------------------------------------------------------------------------------------------------------------------
def _batch(lens, max_new=40):
    reqs = [pb2.Request(id=i, inputs=prompt_text([5 + (j % 7) for j in range(n)]), input_length=n, max_output_length=max_new)
            for i, n in enumerate(lens)]
    b, errs = FlashCausalLMBatch.from_pb(pb2.Batch(id=0, requests=reqs), FixtureTokenizer(4096), torch.float16, CPU, None,
                                         None, True)
    assert not errs
    return b


def _after_prefill(b, cache):
    b.allocate_pages(cache)
    b.input_lengths = [n + 1 for n in b.input_lengths]  # the prefill chose one token


def test_grow_pages_without_look_ahead_is_what_it_was():
    c = PagedKVCache(1, 1, 64, 16, torch.float16, CPU)
    b = _batch([31, 32, 10])
    _after_prefill(b, c)           # lengths 32, 33, 11: pages for 32, 33 and 11 tokens are there
    assert [len(p) for p in b.pages] == [1, 2, 1]
    b.grow_pages()
    assert [len(p) for p in b.pages] == [1, 2, 1]
    b.input_lengths[0] += 1        # 33 tokens: the next one lands on a second page
    b.grow_pages()
    assert [len(p) for p in b.pages] == [2, 2, 1] and b.block_tables[0, :2].tolist() == b.pages[0]
    b.release()
    assert c.free_pages == c.num_pages


def test_grow_pages_looks_ahead_by_k_tokens():
    c = PagedKVCache(1, 1, 64, 16, torch.float16, CPU)
    b = _batch([28, 29, 10, 60])
    _after_prefill(b, c)           # lengths 29, 30, 11, 61: latest tokens at positions 28, 29, 10, 60
    assert [len(p) for p in b.pages] == [1, 1, 1, 2]
    free = c.free_pages
    b.grow_pages(ahead=3)          # positions .. 31, .. 32, .. 13, .. 63: only the second crosses a page
    assert [len(p) for p in b.pages] == [1, 2, 1, 2] and c.free_pages == free - 1
    b.grow_pages(ahead=7)          # .. 35, .. 36, .. 17, .. 67
    assert [len(p) for p in b.pages] == [2, 2, 1, 3] and c.free_pages == free - 3
    for i, p in enumerate(b.pages):
        assert b.block_tables[i, :len(p)].tolist() == p and len(p) * 32 >= b.input_lengths[i] + 7
    b.release()
    assert c.free_pages == c.num_pages


def test_a_look_ahead_the_pool_cannot_serve_leaves_the_batch_as_it_was():
    c = PagedKVCache(1, 1, 64, 3, torch.float16, CPU)
    b = _batch([30, 30, 30])
    _after_prefill(b, c)           # three pages, the pool is empty; every latest token sits at position 30
    pages = [list(p) for p in b.pages]
    with pytest.raises(OutOfPages):
        b.grow_pages(ahead=3)      # position 33 would need a second page each
    assert b.pages == pages and c.free_pages == 0
    b.grow_pages()                 # the plain step still fits
    assert b.pages == pages
    b.release()


def _host_lm(K, N=3):
    lm = FlashCausalLM.__new__(FlashCausalLM)  # the step rule's host code without the GPU-only constructor
    lm.spec_tokens, lm.spec_ngram, lm._spec_stats = K, N, sd.new_stats()
    return lm


def _spec_batch(lens, K, hits, cache, max_new=40):
    b = _batch(lens, max_new)
    _after_prefill(b, cache)
    b.spec_tokens = K
    b.spec_drafts = torch.zeros((len(lens), K), dtype=torch.int64)
    b.spec_hits = torch.tensor(hits, dtype=torch.int32)
    return b


def test_a_pool_too_small_for_the_look_ahead_falls_back_without_an_error():
    c = PagedKVCache(1, 1, 64, 2, torch.float16, CPU)
    lm = _host_lm(3)
    b = _spec_batch([30, 30], 3, [2, 0], c)
    assert c.free_pages == 0
    assert lm._grow_for_verify(b) is False
    st = lm.spec_stats()
    assert st["fallback_pages"] == 1 and st["verify_steps"] == 0 and st["decode_steps"] == 1
    b.grow_pages()                 # what the plain step does next: nothing to grow, no error
    b.release()


def test_the_model_counts_each_cause_and_grows_only_when_it_verifies():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    lm = _host_lm(3)
    b = _spec_batch([30, 12], 3, [0, 0], c)
    assert lm._grow_for_verify(b) is False and lm.spec_stats()["fallback_no_match"] == 1
    assert [len(p) for p in b.pages] == [1, 1], "a plain step's pages are grown by grow_pages(), not here"
    b.spec_hits = torch.tensor([0, 3], dtype=torch.int32)   # a tensor the batch has not seen: read again
    assert lm._grow_for_verify(b) is True
    assert [len(p) for p in b.pages] == [2, 1] and lm.spec_stats()["verify_steps"] == 1
    b.spec_hits = torch.zeros(2, dtype=torch.int32)
    assert lm._grow_for_verify(b) is False and lm.spec_stats()["fallback_no_match"] == 2
    b.spec_hits = torch.ones(2, dtype=torch.int32)
    b.requests[1].details.top_n_toks = 2
    assert lm._grow_for_verify(b) is False and lm.spec_stats()["fallback_details"] == 1
    b.requests[1].details.top_n_toks = 0
    b.total_lengths[1] = b.input_lengths[1] + 3             # K tokens left
    assert lm._grow_for_verify(b) is False and lm.spec_stats()["fallback_remaining"] == 1
    b.total_lengths[1] += 1
    assert lm._grow_for_verify(b) is True
    st = lm.spec_stats()
    assert st["decode_steps"] == 6 and st["verify_steps"] == 2
    b.release()
    assert c.free_pages == c.num_pages


def test_a_sampling_request_keeps_the_batch_on_the_plain_step():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    lm = _host_lm(3)
    b = _spec_batch([5, 6], 3, [3, 3], c)
    assert b.next_token_chooser.is_plain_greedy and lm._grow_for_verify(b) is True
    reqs = [pb2.Request(id=i, inputs=prompt_text([5, 6, 7]), input_length=3, max_output_length=20) for i in range(2)]
    reqs[1].parameters.temperature = 0.7
    s, errs = FlashCausalLMBatch.from_pb(pb2.Batch(id=1, requests=reqs), FixtureTokenizer(4096), torch.float16, CPU, None,
                                         None, True)
    assert not errs and not s.next_token_chooser.is_plain_greedy
    _after_prefill(s, c)
    s.spec_tokens, s.spec_drafts, s.spec_hits = 3, torch.zeros((2, 3), dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    assert lm._grow_for_verify(s) is False and lm.spec_stats()["fallback_not_greedy"] == 1
    b.release()
    s.release()


# ---- the batch and its drafter ------------------------------------------------------------------------------------------------
class _RecordingDrafter:
    """The three methods of a drafter (models/speculation.py); `redraft` records what the batch looked like when called and
    drafts the way a drafter must: the batch's own buffers, and renewed."""

    def __init__(self):
        self.calls = []

    def redraft(self, batch):
        self.calls.append((batch, batch.spec_drafts, batch.spec_hits))
        batch.ensure_spec_buffers()
        batch.drafts_renewed()


class _CountedHits:
    """A `spec_hits` stand-in that counts how often the batch reads it to the host."""

    def __init__(self, hits):
        self.hits, self.reads = hits, 0

    def tolist(self):
        self.reads += 1
        return list(self.hits)


def _decode_form(b):
    """What the prefill's bookkeeping leaves: one id, one position per request."""
    B = len(b)
    b.cu_seqlens_q = torch.arange(B + 1, dtype=torch.int32)
    b.position_ids = torch.tensor([n - 1 for n in b.input_lengths])
    b.input_ids = torch.arange(B, dtype=torch.int64) + 7
    return b


def _drafted_batch(cache, drafter, hidden=None, first_id=0):
    b = _decode_form(_spec_batch([30, 12], 3, [0, 0], cache))
    for i, r in enumerate(b.requests):
        r.id = first_id + i
    b.spec_model, b.spec_hidden = drafter, hidden
    return b


def test_stale_drafts_are_drafted_anew_once_when_the_hits_are_asked_for():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    d = _RecordingDrafter()
    b = _drafted_batch(c, d)
    first = b.spec_hits = _CountedHits([0, 2])
    b.drafts_are_stale()
    assert d.calls == [] and first.reads == 0, "marking drafts stale drafts nothing"
    assert b.spec_hits_host() == [0, 2] and len(d.calls) == 1 and d.calls[0][0] is b
    assert b.spec_hits_host() == [0, 2] and len(d.calls) == 1 and first.reads == 1, "neither drafted nor read twice"
    second = b.spec_hits = _CountedHits([3, 0])
    assert b.spec_hits_host() == [3, 0] and b.spec_hits_host() == [3, 0]
    assert second.reads == 1 and first.reads == 1 and len(d.calls) == 1, "a new tensor is read again, once, without a redraft"
    b.release()


def test_prune_drafts_anew_on_dropped_buffers_and_keeps_the_kept_rows_state():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    d = _RecordingDrafter()
    hidden = torch.arange(8, dtype=torch.float16).reshape(2, 4)
    b = _drafted_batch(c, d, hidden.clone())
    kept = FlashCausalLMBatch.prune(b, [0])
    assert kept is b and [r.id for r in b.requests] == [1]
    assert len(d.calls) == 1 and d.calls[0] == (b, None, None), "one redraft, on a batch whose drafts and hits were dropped"
    assert b.spec_drafts.shape == (1, 3) and b.spec_hits.shape == (1,)
    assert torch.equal(b.spec_hidden, hidden[1:2]), "the kept request's state is carried over"
    # the lookup's batches have no state to carry
    b2 = _drafted_batch(c, d, None, first_id=2)
    FlashCausalLMBatch.prune(b2, [3])
    assert len(d.calls) == 2 and d.calls[1] == (b2, None, None) and b2.spec_hidden is None
    b.release()
    b2.release()
    assert c.free_pages == c.num_pages


def test_concatenate_drafts_anew_once_on_the_merged_batch():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    d = _RecordingDrafter()
    ha, hb = torch.arange(8, dtype=torch.float16).reshape(2, 4), 10 + torch.arange(8, dtype=torch.float16).reshape(2, 4)
    a, b = _drafted_batch(c, d, ha.clone()), _drafted_batch(c, d, hb.clone(), first_id=2)
    m = FlashCausalLMBatch.concatenate([a, b])
    assert len(d.calls) == 1 and d.calls[0] == (m, None, None), "one redraft, on the merged batch"
    assert [r.id for r in m.requests] == [0, 1, 2, 3] and m.spec_tokens == 3 and m.spec_model is d
    assert torch.equal(m.spec_hidden, torch.cat([ha, hb])), "the states in request order"
    assert m.spec_drafts.shape == (4, 3) and m.spec_hits.shape == (4,)
    m.release()
    assert c.free_pages == c.num_pages


# ---- the restatement, on cases written out by hand ----------------------------------------------------------------------------
def _ctx(tokens, width=24):
    row = np.full(width, 999, dtype=np.int64)  # what lies behind the context is never looked at
    row[:len(tokens)] = tokens
    return row, len(tokens) - 1


@pytest.mark.parametrize("tokens,K,N,want_drafts,want_hit", [
    ([7, 8], 3, 3, [0, 0, 0], 0),                               # shorter than n + 1 for n = 3, 2; n = 1 finds nothing
    ([7], 3, 1, [0, 0, 0], 0),                                  # one token: no j at all
    ([1, 2, 3, 9, 9, 1, 2, 3], 3, 3, [9, 9, 1], 3),             # a match at index 0
    ([4, 5, 6, 4, 5, 7, 4, 5], 2, 2, [7, 4], 2),                # several matches: the latest (j = 3) wins over j = 0
    ([1, 2, 3, 4, 9, 3, 8, 1, 2, 3], 2, 3, [4, 9], 3),          # n = 3 at j = 0 beats the later n = 1 match at j = 5
    ([5, 6, 7, 5, 6], 4, 2, [7, 5, 6, 0], 2),                   # the continuation runs into the context's end
    ([1, 2, 3, 4, 5], 3, 3, [0, 0, 0], 0),                      # no match at all
    ([3, 3], 2, 3, [3, 0], 1),                                  # j + n < len: the suffix itself is not a match, j = 0 is
])
def test_propose_restated(tokens, K, N, want_drafts, want_hit):
    row, pos = _ctx(tokens)
    drafts, hits = spec_ref.propose(row[None], [pos], K, N)
    assert drafts.tolist() == [want_drafts] and hits.tolist() == [want_hit]


def test_accept_restated():
    am = np.array([[10, 11, 12, 13], [10, 11, 12, 13], [10, 11, 12, 13]])
    lps = -np.arange(12, dtype=np.float32).reshape(3, 4)
    drafts = np.array([[99, 11, 12], [10, 11, 77], [10, 11, 12]])  # none, two, all three accepted
    all_ids = np.zeros((3, 12), dtype=np.int64)
    got = spec_ref.accept(am, lps, drafts, [2, 4, 7], all_ids, [0, 3, 8, 16])
    assert got["n_emit"].tolist() == [1, 3, 4]
    assert got["out_ids"].tolist() == [[10, -1, -1, -1], [10, 11, 12, -1], [10, 11, 12, 13]]
    assert got["out_lps"][1].tolist() == [-4.0, -5.0, -6.0, 0.0]
    assert got["latest"].tolist() == [10, 12, 13] and got["positions"].tolist() == [3, 7, 11]
    assert got["all_ids"][0, 3] == 10 and got["all_ids"][1, 5:8].tolist() == [10, 11, 12]
    assert got["all_ids"][2, 8:12].tolist() == [10, 11, 12, 13] and got["all_ids"].sum() == 10 + 33 + 46
    assert got["cu_seqlens"].tolist() == [0, 4, 12, 24], "entry b grows by what the requests in front of it emitted"
    # K = 0: one token each, cu_seqlens += arange
    got = spec_ref.accept(am[:, :1], lps[:, :1], [[], [], []], [2, 4, 7], all_ids, [0, 3, 8, 16])
    assert got["n_emit"].tolist() == [1, 1, 1] and got["cu_seqlens"].tolist() == [0, 4, 10, 19]


def test_stage_restated():
    bt = np.array([[4, 9, 2], [7, 7, 7]])
    ids, pos, slots, ctx = spec_ref.stage([30, 0], [50, 60], [[51, 52, 53], [0, 0, 0]], bt)
    assert ids.tolist() == [50, 51, 52, 53, 60, 0, 0, 0] and pos.tolist() == [30, 31, 32, 33, 0, 1, 2, 3]
    assert slots.tolist() == [4 * 32 + 30, 4 * 32 + 31, 9 * 32, 9 * 32 + 1, 224, 225, 226, 227] and ctx.tolist() == [34, 4]
