"""CPU: KV prefix reuse on the host (utils/kv_cache.py): the page index keyed by (parent serial, the page's 32 token ids),
shared ownership by reference count, the LRU of cached pages nobody holds, and how FlashCausalLMBatch.allocate_pages and the
FlashCausalLM option use them.  The pool lives on the CPU device; no kernel runs."""
import threading

import pytest
import torch

from tests.fixture_utils import FixtureTokenizer, prompt_text
from tgis_amd.models.flash_causal_lm import FlashCausalLMBatch
from tgis_amd.pb import generate_pb2 as pb2
from tgis_amd.utils.kv_cache import OutOfPages, PagedKVCache, agree_kv_prefix_reuse, parse_kv_prefix_reuse
from tgis_amd.utils.rank_group import RankGroup

CPU = torch.device("cpu")
ZERO_STATS = {"lookups": 0, "hit_pages": 0, "looked_up_pages": 0, "registered": 0, "evictions": 0}


def pool(num_pages=8, reuse=True, kv_dtype="auto"):
    return PagedKVCache(1, 1, 64, num_pages, torch.float16, CPU, kv_dtype=kv_dtype, prefix_reuse=reuse)


def toks(n, base=0):
    """n distinct token ids, another sequence for another `base`."""
    return [base + i for i in range(n)]


def state(c):
    return (sorted(c._free), list(c._lru), dict(c._index), dict(c._entry), dict(c._refs), c.free_pages)


def serve(c, prompt):
    """One request's life up to its prefill: match, allocate the rest, register.  Returns its page list."""
    shared = c.match(prompt)
    pages = shared + c.alloc(PagedKVCache.pages_for(len(prompt) + 1) - len(shared))
    c.register(pages, prompt)
    return pages


# ---- reuse off --------------------------------------------------------------------------------------------------------------
def test_reuse_off_hands_out_the_ids_it_always_did():
    c = pool(8, reuse=False)
    assert c.alloc(3) == [0, 1, 2] and c.alloc(2) == [3, 4]
    c.free([1, 3])
    assert c.alloc(3) == [1, 3, 5] and c.free_pages == 2
    c.free([5, 0])
    assert c.alloc(1) == [0] and c.alloc(3) == [5, 6, 7] and c.free_pages == 0
    with pytest.raises(OutOfPages):
        c.alloc(1)
    c.free([7, 6, 5, 4, 3, 2, 1, 0])
    assert c.free_pages == 8 and c.alloc(8) == list(range(8))
    # the new calls are inert, and nothing was counted
    c.register([0, 1], toks(64))
    assert c.match(toks(70)) == [] and c.reuse_stats() == ZERO_STATS and not c._index and not c._refs and not c._lru


def test_default_is_off():
    assert PagedKVCache(1, 1, 64, 4, torch.float16, CPU).prefix_reuse is False


# ---- match after register ---------------------------------------------------------------------------------------------------
def test_match_returns_the_longest_chain_capped_one_token_short():
    c = pool(16)
    a = toks(70)
    pa = serve(c, a)                                  # 3 pages, 2 of them full
    assert pa == [0, 1, 2] and c.reuse_stats()["registered"] == 2
    assert c.match(a[:64] + toks(10, 500)) == [0, 1]  # longest chain
    assert c.match(a[:64]) == [0]                     # 64 tokens: (64 - 1) // 32 = 1, one token at least is computed
    assert c.match(a[:65]) == [0, 1]                  # 65 tokens: 2
    assert c.match(a[:32]) == [] and c.match(a[:1]) == [] and c.match([]) == []
    other = list(a)
    other[40] += 1000                                 # differs inside page 1
    assert c.match(other) == [0]
    other = list(a)
    other[3] += 1000                                  # differs inside page 0: page 1's equal tokens do not help
    assert c.match(other) == []
    s = c.reuse_stats()
    # (the first lookup was A's own, a miss over 2 pages)
    assert s["lookups"] == 9 and s["hit_pages"] == 2 + 1 + 2 + 1 and s["looked_up_pages"] == 2 + (2 + 1 + 2 + 0 + 0 + 0 + 2 + 2)


def test_register_keeps_the_first_entry_of_equal_content():
    c = pool(16)
    a = toks(70)
    p1, p2 = c.alloc(3), c.alloc(3)   # two requests of one batch: both missed, both prefilled
    c.register(p1, a)
    c.register(p2, a)
    assert c.reuse_stats()["registered"] == 2 and set(c._entry) == {0, 1}
    assert c.match(a) == [0, 1]
    c.free([0, 1])
    c.free(p1)
    c.free(p2)                        # p2's pages were never indexed: straight back to the heap
    assert sorted(c._free) == [2, 3, 4, 5] + list(range(6, 16)) and list(c._lru) == [1, 0] and c.free_pages == 16
    # registering twice changes nothing
    c.register(p1, a)
    assert c.reuse_stats()["registered"] == 2


# ---- sharing ----------------------------------------------------------------------------------------------------------------
def test_a_shared_page_is_free_only_after_both_holders_let_go():
    c = pool(8)
    a = toks(70)
    pa = serve(c, a)
    pb = serve(c, a[:64] + toks(10, 900))
    assert pb[:2] == pa[:2] and pb[2] not in pa and c._refs[pa[0]] == 2 and c._refs[pa[2]] == 1
    assert c.free_pages == 8 - 4
    c.free(pa)
    assert pa[0] not in c._free and pa[0] not in c._lru and pa[1] not in c._lru  # B still holds them
    assert pa[2] in c._free and c.free_pages == 8 - 3
    c.free(pb)
    assert set(c._lru) == {pa[0], pa[1]} and not c._refs and c.free_pages == c.num_pages == 8


# ---- eviction ---------------------------------------------------------------------------------------------------------------
def test_eviction_takes_heap_pages_first_then_the_oldest_cached():
    c = pool(6)
    x, y = toks(40, 0), toks(40, 1000)
    px = serve(c, x)          # pages 0 (indexed), 1
    py = serve(c, y)          # pages 2 (indexed), 3
    c.free(px)
    c.free(py)
    assert list(c._lru) == [0, 2] and sorted(c._free) == [1, 3, 4, 5] and c.free_pages == 6
    assert c.alloc(4) == [1, 3, 4, 5] and c.reuse_stats()["evictions"] == 0      # heap first
    c.free([1, 3, 4, 5])
    hit = c.match(x)          # a hit refreshes recency
    assert hit == [0]
    c.free(hit)
    assert list(c._lru) == [2, 0]
    got = c.alloc(5)
    assert got == [1, 3, 4, 5, 2] and c.reuse_stats()["evictions"] == 1          # then the oldest cached page: y's
    assert c.match(y) == [] and c.match(x) == [0]                                # evicted: gone; x's page is pinned now
    with pytest.raises(OutOfPages):
        c.alloc(1)            # a held page is never evicted
    c.free([0])
    assert c.alloc(1) == [0] and c.match(x) == [] and c.reuse_stats()["evictions"] == 2


def test_a_chain_is_evicted_from_its_tail():
    c = pool(4)
    a = toks(100)
    pa = serve(c, a)          # 4 pages, 3 indexed
    c.free(pa)
    assert list(c._lru) == [2, 1, 0] and sorted(c._free) == [3]
    assert c.alloc(2) == [3, 2]
    assert c.match(a) == [0, 1]


def test_a_child_of_an_evicted_parent_never_matches_again():
    c = pool(4)
    a = toks(70)
    pa = serve(c, a)                        # 0, 1 indexed; 2
    c.free([pa[0]])
    c.free([pa[1], pa[2]])                  # the parent is now the oldest cached page
    assert list(c._lru) == [0, 1] and sorted(c._free) == [2, 3]
    got = c.alloc(3)                        # both heap pages, then the parent's
    assert got == [2, 3, 0] and c.reuse_stats()["evictions"] == 1
    assert c.match(a) == []                 # the chain starts at the evicted parent
    c.free(got)
    fresh = c.alloc(2)                      # the same first page again, written anew: a new serial
    assert fresh == [0, 2]
    c.register(fresh, a[:40])
    assert 1 in c._entry                    # the child still sits in the index, under the old parent's serial
    assert c.match(a) == [0]                # ... which nothing can ever present again
    c.free([0])
    c.free(fresh)
    assert c.free_pages == 4


# ---- OutOfPages -------------------------------------------------------------------------------------------------------------
def test_out_of_pages_with_pinned_pages_changes_nothing():
    c = pool(6)
    a = toks(70)
    pa = serve(c, a)
    c.free(pa)                              # 2 cached, 4 on the heap
    pinned = c.match(a)
    assert pinned == [0, 1]
    before = state(c)
    with pytest.raises(OutOfPages):
        c.alloc(5)                          # 4 heap pages, the 2 cached ones are held
    assert state(c) == before and c.reuse_stats()["evictions"] == 0
    c.free(pinned)
    assert c.free_pages == 6


def _pb(prompts, max_new, first_id=0, batch_id=0, input_toks=False):
    reqs = [pb2.Request(id=first_id + i, inputs=prompt_text(p), input_length=len(p), max_output_length=max_new,
                        details=pb2.RequestedDetails(input_toks=input_toks)) for i, p in enumerate(prompts)]
    return pb2.Batch(id=batch_id, requests=reqs)


def _batch(prompts, max_new=4, **kw):
    b, errs = FlashCausalLMBatch.from_pb(_pb(prompts, max_new, **kw), FixtureTokenizer(4096), torch.float16, CPU, None, None,
                                         True)
    assert not errs
    return b


def test_from_pb_keeps_the_prompt_ids_on_the_host():
    b = _batch([toks(5, 7), toks(3, 100)])
    assert b.prompt_token_ids == [toks(5, 7), toks(3, 100)] and b.reused_lengths is None


def test_allocate_pages_maps_shared_pages_first_and_deals_the_rest_page_major():
    c = pool(16)
    a = toks(70, 10)
    first = _batch([a], batch_id=1)
    first.allocate_pages(c)
    assert first.pages == [[0, 1, 2]] and first.reused_lengths == [0]
    first.register_prompt_pages()
    assert first.prompt_token_ids is None and c.reuse_stats()["registered"] == 2
    # one hit of two pages next to a miss: own pages page-major over the two requests
    nxt = _batch([a[:64] + toks(40, 700), toks(40, 2000)], first_id=5, batch_id=2)
    nxt.allocate_pages(c)
    assert nxt.reused_lengths == [64, 0]
    assert nxt.pages == [[0, 1, 3, 5], [4, 6]]
    assert nxt.block_tables[0, :4].tolist() == [0, 1, 3, 5]
    # two requests of one batch that share a prefix nobody registered: both miss
    twins = _batch([toks(70, 3000), toks(70, 3000)], first_id=9, batch_id=3)
    twins.allocate_pages(c)
    assert twins.reused_lengths == [0, 0] and not set(twins.pages[0]) & set(twins.pages[1])
    for b in (first, nxt, twins):
        b.release()
    assert c.free_pages == c.num_pages


def test_a_batch_that_wants_input_token_details_does_not_look_up_but_registers():
    c = pool(16)
    a = toks(70, 10)
    first = _batch([a], batch_id=1)
    first.allocate_pages(c)
    first.register_prompt_pages()
    lookups = c.reuse_stats()["lookups"]
    b = _batch([a[:64] + toks(10, 700)], first_id=3, batch_id=2, input_toks=True)
    b.allocate_pages(c)
    assert b.reused_lengths == [0] and c.reuse_stats()["lookups"] == lookups and not set(b.pages[0]) & {0, 1}
    b.register_prompt_pages()          # equal content is indexed already: its own pages stay private
    assert c.reuse_stats()["registered"] == 2
    d = _batch([toks(70, 5000)], first_id=4, batch_id=3, input_toks=True)
    d.allocate_pages(c)
    d.register_prompt_pages()
    assert c.reuse_stats()["registered"] == 4
    for x in (first, b, d):
        x.release()
    assert c.free_pages == c.num_pages


def test_a_batch_with_prompt_tuning_embeddings_neither_looks_up_nor_registers():
    c = pool(16)
    b = _batch([toks(70, 10)], batch_id=1)
    b.inputs_embeds = torch.zeros((70, 8))  # what from_pb leaves when a request carries a prefix_id
    b.allocate_pages(c)
    b.register_prompt_pages()
    assert c.reuse_stats() == ZERO_STATS
    b.release()
    assert c.free_pages == c.num_pages


def test_a_failed_allocate_pages_gives_back_its_pins():
    c = pool(6)
    a = toks(70, 10)
    first = _batch([a], batch_id=1)
    first.allocate_pages(c)
    first.register_prompt_pages()
    first.release()                         # pages 0, 1 cached; 4 on the heap
    before = state(c)
    big = _batch([a[:64] + toks(150, 700)], first_id=2, batch_id=2)   # 7 pages, 2 of them shared: 5 > 4
    with pytest.raises(OutOfPages):
        big.allocate_pages(c)
    assert big.pages is None and c.reuse_stats()["hit_pages"] == 2
    after = state(c)
    assert after[0] == before[0] and sorted(after[1]) == sorted(before[1]) and after[2:] == before[2:]
    assert not c._refs and c.free_pages == 6
    ok = _batch([a[:64] + toks(10, 700)], first_id=3, batch_id=3)
    ok.allocate_pages(c)
    assert ok.pages == [[0, 1, 2]]
    ok.release()


# ---- scales -----------------------------------------------------------------------------------------------------------------
def test_set_scales_drops_the_index():
    c = pool(8, kv_dtype="fp8_e4m3")
    a = toks(70)
    pa = serve(c, a)
    with pytest.raises(ValueError):
        c.set_scales([0.5], [2.0])          # a page is handed out
    c.free(pa)
    assert len(c._lru) == 2 and c.free_pages == 8
    c.set_scales([0.5], [2.0])
    assert not c._lru and not c._index and not c._entry and sorted(c._free) == list(range(8)) and c.free_pages == 8
    assert c.match(a) == [] and c.scales(0) == (0.5, 2.0)


# ---- the option -------------------------------------------------------------------------------------------------------------
def test_flag_parsing(monkeypatch):
    monkeypatch.delenv("TGIS_KV_PREFIX_REUSE", raising=False)
    assert parse_kv_prefix_reuse() is False and parse_kv_prefix_reuse(True) is True and parse_kv_prefix_reuse(False) is False
    assert parse_kv_prefix_reuse("TRUE ") is True and parse_kv_prefix_reuse("false") is False
    monkeypatch.setenv("TGIS_KV_PREFIX_REUSE", "true")
    assert parse_kv_prefix_reuse() is True and parse_kv_prefix_reuse(False) is False
    for bad in ("1", "yes", "", "on"):
        with pytest.raises(ValueError, match="KV prefix reuse"):
            parse_kv_prefix_reuse(bad)
    monkeypatch.setenv("TGIS_KV_PREFIX_REUSE", "maybe")
    with pytest.raises(ValueError, match="maybe"):
        parse_kv_prefix_reuse()


class _PairedGroup(RankGroup):
    """One of two fake ranks run on two threads: every reduction meets the peer's at a barrier, so a rank that issued
    another sequence of collectives than its peer would break the barrier (timeout) instead of passing."""

    def __init__(self, rank, shared):
        self.world, self.rank, self.process_group, self.real, self.nccl, self.device = 2, rank, None, True, False, CPU
        self.shared = shared

    def _reduce_int(self, v, op):
        s = self.shared
        s["vals"][self.rank] = (int(v), op)
        s["barrier"].wait(timeout=20)
        (a, op_a), (b, op_b) = s["vals"]
        assert op_a == op_b, "the ranks are in different collectives"
        s["barrier"].wait(timeout=20)
        return min(a, b) if op == torch.distributed.ReduceOp.MIN else max(a, b)


def _on_two_fake_ranks(values):
    shared = {"vals": [None, None], "barrier": threading.Barrier(2)}
    out = [None, None]

    def run(r):
        try:
            out[r] = agree_kv_prefix_reuse(_PairedGroup(r, shared), values[r])
        except Exception as e:  # noqa: BLE001 (reported to the asserting thread)
            out[r] = e

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30)
    assert not any(t.is_alive() for t in threads)
    return out


def test_ranks_agree_on_the_flag():
    assert _on_two_fake_ranks([True, "true"]) == [True, True]
    assert _on_two_fake_ranks([False, False]) == [False, False]
    got = _on_two_fake_ranks([True, False])
    assert all(isinstance(e, ValueError) and "disagree on KV prefix reuse" in str(e) for e in got)
    got = _on_two_fake_ranks([True, "perhaps"])   # the rank that cannot parse tells its peer: both raise, nobody waits
    assert all(isinstance(e, ValueError) for e in got)
    assert "another tensor-parallel rank" in str(got[0]) and "perhaps" in str(got[1])


def test_one_rank_needs_no_group():
    assert agree_kv_prefix_reuse(RankGroup(object(), CPU), True) is True
    with pytest.raises(ValueError):
        agree_kv_prefix_reuse(RankGroup(object(), CPU), "2")


# ---- which cache writer a layer calls (flash_common.write_kv) ----------------------------------------------------------------
def test_write_kv_picks_the_writer_by_case(monkeypatch):
    from tgis_amd import native
    from tgis_amd.models.custom_modeling import flash_common

    calls = []
    for name in ("rope_kv_write", "rope_kv_write_prefill", "rope_kv_write_prefill_at"):
        monkeypatch.setattr(native, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)) or a[0])
    H, HKV, D = 4, 2, 64
    cache = PagedKVCache(2, HKV, D, 4, torch.float16, CPU, kv_dtype="fp8_e4m3", prefix_reuse=True)
    cache.k_scales[1], cache.v_scales[1] = 0.5, 2.0
    cu = torch.tensor([0, 3, 5], dtype=torch.int32)
    past = torch.tensor([32, 0], dtype=torch.int32)
    qkv = torch.zeros((5, (H + 2 * HKV) * D), dtype=torch.float16)

    def kv(**kw):
        return flash_common.KVArgs(cache=cache, block_tables=torch.tensor([[0, 1], [2, 3]], dtype=torch.int32),
                                   ctx_lens=torch.tensor([35, 2], dtype=torch.int32), slots=torch.arange(5, dtype=torch.int32),
                                   max_q_len=3, max_ctx=35, **kw)

    def write(x, args):
        return flash_common.write_kv(x, args, 1, H, HKV, D, D, None, None, None, cu)

    behind = kv(past_lens=past)
    assert write(qkv, behind) is qkv
    write(qkv, kv(fresh_prefill=True))
    write(qkv, kv())
    part = native.Partial(torch.zeros(8, dtype=torch.float32), 2, qkv.shape[1], 5, qkv.shape[1], None)
    write(part, behind)   # a split-K sum is finished by the per-token kernel, whatever the case
    assert [c[0] for c in calls] == ["rope_kv_write_prefill_at", "rope_kv_write_prefill", "rope_kv_write", "rope_kv_write"]
    name, args, kw = calls[0]
    assert args[0] is qkv and args[4] is cu and args[5] is behind.block_tables and args[8:] == (3, H, HKV, D, D, past)
    assert args[13] is past and kw == {"kv_scales": (0.5, 2.0)}
    assert calls[3][1][4] is behind.slots
