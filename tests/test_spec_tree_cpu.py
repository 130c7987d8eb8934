"""CPU: several draft candidates per request — the option and its refusals, the step rule with 1 + C K rows, the mask
builder against a brute-force ancestor walk, the non-overlap claim of tgis_spec_tree_commit by enumeration, and the accept
restatement (tests/spec_tree_ref.py) against the rule of the reference's process_outputs_with_speculation.

What runs project code here: the option, the refusals, the step rule, `tree_q_mask` and the library's argument checks.  The
tests of the layout, of `commit_moves`, of the accept rule and of the lookup check the RESTATEMENTS in tests/spec_tree_ref.py
(they pass without the feature): they are the enumeration and the rule the kernels are then held to on the GPU.  In
particular the non-overlap enumeration proves the claim for `ref.commit_moves`, not for the index arithmetic of
`spec_tree_commit_kernel`; the two are tied together only by the whole-pool comparison of tests/test_spec_tree_ops_gpu.py."""
import numpy as np
import pytest
import torch

from tests import spec_tree_ref as ref
from tests.test_spec_decode_cpu import CPU, _host_lm, _spec_batch
from tgis_amd.utils import spec_decode as sd
from tgis_amd.utils.kv_cache import PagedKVCache

SHAPES = [(C, K) for C in range(1, 5) for K in range(1, 8) if 1 + C * K <= 64]


# ---- the option ---------------------------------------------------------------------------------------------------------------
def test_parse_spec_candidates(monkeypatch):
    monkeypatch.delenv("TGIS_SPEC_CANDIDATES", raising=False)
    assert sd.parse_spec_candidates() == 1 and sd.parse_spec_candidates(1) == 1 and sd.parse_spec_candidates("3") == 3
    assert sd.parse_spec_candidates(sd.MAX_SPEC_CANDIDATES) == 4
    monkeypatch.setenv("TGIS_SPEC_CANDIDATES", "2")
    assert sd.parse_spec_candidates() == 2 and sd.parse_spec_candidates(4) == 4, "the argument wins over the environment"
    monkeypatch.setenv("TGIS_SPEC_CANDIDATES", " ")
    assert sd.parse_spec_candidates() == 1
    for bad in (0, 5, -1, "two", 2.0, True):
        with pytest.raises(ValueError, match="spec_candidates"):
            sd.parse_spec_candidates(bad)
    monkeypatch.setenv("TGIS_SPEC_CANDIDATES", "7")
    with pytest.raises(ValueError, match="TGIS_SPEC_CANDIDATES"):
        sd.parse_spec_candidates()


def test_what_several_candidates_need_of_the_other_options():
    sd.check_spec_candidates(1, 0, True, True)  # one candidate asks nothing
    sd.check_spec_candidates(3, 3, False, False)
    with pytest.raises(ValueError, match="needs spec_tokens > 0"):
        sd.check_spec_candidates(2, 0, False, False)
    with pytest.raises(NotImplementedError, match="MLP speculator"):
        sd.check_spec_candidates(2, 3, True, False)
    with pytest.raises(NotImplementedError, match="spec_sampling"):
        sd.check_spec_candidates(2, 3, False, True)
    # the decode form of the attention: rows * padded group size <= 64
    sd.check_tree_rows(4, 7, 32, 32)       # MHA: 29 rows
    sd.check_tree_rows(2, 3, 32, 4)        # GQA 8:1: 7 rows * 8
    sd.check_tree_rows(3, 1, 48, 1)        # MQA: 4 rows * 16
    sd.check_tree_rows(1, 7, 48, 1)        # one candidate is never refused here
    with pytest.raises(ValueError, match="decode form"):
        sd.check_tree_rows(3, 3, 32, 4)    # 10 rows * 8
    with pytest.raises(ValueError, match="decode form"):
        sd.check_tree_rows(2, 2, 48, 1)    # 5 rows * 16
    with pytest.raises(NotImplementedError, match="tensor parallelism"):
        sd.check_spec_world(3, 2)          # (stays refused as it is)


def test_the_constructor_refuses_before_it_loads_anything(monkeypatch):
    """The refusals sit in front of the GPU check and of any engine: they raise the same way on a machine without a GPU."""
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    def build(**kw):
        return FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=object(), **kw)

    monkeypatch.delenv("TGIS_SPEC_CANDIDATES", raising=False)
    with pytest.raises(ValueError, match="spec_candidates"):
        build(spec_tokens=3, spec_candidates=5)
    with pytest.raises(ValueError, match="needs spec_tokens > 0"):
        build(spec_candidates=2)
    with pytest.raises(NotImplementedError, match="spec_sampling"):
        build(spec_tokens=3, spec_candidates=2, spec_sampling=True)
    monkeypatch.setenv("TGIS_SPEC_CANDIDATES", "9")
    with pytest.raises(ValueError, match="TGIS_SPEC_CANDIDATES"):
        build(spec_tokens=3)


# ---- the step rule ------------------------------------------------------------------------------------------------------------
def test_step_rule_with_r_rows():
    hits = [1, 0]
    # rows: bucket * (1 + C K) <= 64
    assert sd.fallback_cause(3, 8, True, False, [20, 20], hits, C=2) is None          # 56 rows
    assert sd.fallback_cause(3, 16, True, False, [20, 20], hits, C=2) == "rows"       # 112
    assert sd.fallback_cause(3, 8, True, False, [20, 20], hits, C=3) == "rows"        # 80
    assert sd.fallback_cause(7, 2, True, False, [40, 40], hits, C=4) is None          # 58
    # remaining: C K + 1 tokens left
    assert sd.fallback_cause(3, 2, True, False, [7, 9], hits, C=2) is None
    assert sd.fallback_cause(3, 2, True, False, [6, 9], hits, C=2) == "remaining"
    assert sd.fallback_cause(3, 2, True, False, [6, 9], hits) is None, "one candidate: K + 1 as before"
    assert sd.fallback_cause(3, 2, True, False, [20, 20], [0, 0], C=2) == "no_match"
    assert sd.fallback_cause(3, 2, False, False, [20, 20], hits, C=2) == "not_greedy"
    assert sd.fallback_cause(3, 2, True, True, [20, 20], hits, C=2) == "details"
    assert sd.may_ever_verify(3, 8, 2) and not sd.may_ever_verify(3, 16, 2) and sd.may_ever_verify(3, 16)
    assert not sd.may_ever_verify(0, 1, 4)
    assert "won_by_later_candidate" in sd.SPEC_STATS and sd.new_stats()["won_by_later_candidate"] == 0


def test_the_model_grows_c_k_positions_ahead_or_stays_plain():
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    lm = _host_lm(3)
    lm.spec_candidates = 2
    b = _spec_batch([27, 12], 3, [2, 1], c)   # the latest tokens sit at positions 27 and 12
    b.spec_candidates = 2
    assert lm._grow_for_verify(b) is True     # rows up to position 27 + 6 = 33: a second page; 12 + 6 stays on the first
    assert [len(p) for p in b.pages] == [2, 1] and lm.spec_stats()["verify_steps"] == 1
    b.total_lengths[1] = b.input_lengths[1] + 6  # C K tokens left: one short
    assert lm._grow_for_verify(b) is False and lm.spec_stats()["fallback_remaining"] == 1
    b.release()
    # a pool that cannot serve the look-ahead: the plain step, no error
    c = PagedKVCache(1, 1, 64, 2, torch.float16, CPU)
    b = _spec_batch([27, 27], 3, [2, 1], c)
    b.spec_candidates = 2
    assert c.free_pages == 0 and lm._grow_for_verify(b) is False and lm.spec_stats()["fallback_pages"] == 1
    b.release()
    # the batch's own buffers
    c = PagedKVCache(1, 1, 64, 8, torch.float16, CPU)
    b = _spec_batch([5, 6, 7], 3, [0, 0, 0], c)
    b.position_ids = torch.tensor([4, 5, 6])
    b.spec_drafts = None
    b.ensure_spec_buffers()
    assert b.spec_drafts.shape == (3, 3), "one candidate keeps [B, K]"
    b.spec_candidates, b.spec_drafts = 4, None
    b.ensure_spec_buffers()
    assert b.spec_drafts.shape == (3, 4, 3) and b.spec_hits.shape == (3,)
    assert b.can_verify()                     # bucket 4 * 13 rows
    b.release()


# ---- the mask and the layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", SHAPES)
def test_mask_builder_against_the_ancestor_walk(C, K):
    par = ref.parents(C, K)
    assert len(par) == sd.tree_rows(C, K) == ref.rows(C, K)
    brute = ref.mask_from_parents(par)
    assert sd.tree_q_mask(C, K) == brute == ref.q_mask(C, K)
    dep = ref.depths(C, K)
    for r, w in enumerate(brute):
        assert w >> (r + 1) == 0, "ancestors have lower row numbers: the causal bound stays an upper bound"
        assert bin(w).count("1") == dep[r] + 1, "a row sees itself and one ancestor per depth"
        assert w & 1, "every row sees row 0"
    assert all(0 <= w < 2 ** 63 for w in brute), "the words fit an int64 tensor"


@pytest.mark.parametrize("C,K", SHAPES)
def test_commit_moves_never_overlap(C, K):
    """By enumeration: over every best >= 1 and n_emit, no destination position is a source, every source lies at least K
    behind its destination, at most K positions move, and all of them lie inside the step's rows."""
    pos = 100
    for best in range(C):
        for n in range(1, K + 2):
            moves = ref.commit_moves(pos, C, K, best, n)
            if best == 0 or n == 1:
                assert moves == []
                continue
            src, dst = [m[0] for m in moves], [m[1] for m in moves]
            assert len(moves) == n - 1 <= K and not set(src) & set(dst)
            assert all(s - d == best * K >= K for s, d in moves)
            assert min(dst) == pos + 1 and max(src) <= pos + C * K
            assert src == [pos + 1 + best * K + j for j in range(n - 1)]


# ---- the accept rule ----------------------------------------------------------------------------------------------------------
def _drawn(rng, C, K, mode):
    R = ref.rows(C, K)
    am = rng.integers(3, 40, size=R).astype(np.int64)
    drafts = rng.integers(50, 90, size=(C, K)).astype(np.int64)  # disjoint from the choices: wrong unless set
    if mode == "none":
        return am, drafts
    depth = [int(rng.integers(0, K + 1)) for _ in range(C)]
    if mode == "ties":
        depth = [max(depth)] * C
    for c in range(C):
        for j in range(depth[c]):
            drafts[c, j] = am[0 if j == 0 else 1 + c * K + j - 1]
    return am, drafts


@pytest.mark.parametrize("C,K", [(1, 3), (2, 3), (3, 1), (4, 3), (4, 7), (2, 7)])
def test_accept_restatement_is_the_references_rule(C, K):
    rng = np.random.default_rng(10 * C + K)
    seen = set()
    for i in range(200):
        mode = ("drawn", "ties", "none")[i % 3]
        am, drafts = _drawn(rng, C, K, mode)
        got = ref.accept(am[None], np.zeros((1, ref.rows(C, K)), dtype=np.float32), drafts[None], [5], np.zeros((1, 64)), [0, 9])
        bc, nc = ref.reference_best(am, drafts)
        assert int(got["best"][0]) == bc and int(got["n_emit"][0]) == nc + 1, (mode, am, drafts)
        a = ref.n_correct(am, drafts)
        assert bc == a.index(max(a))
        path = [am[0]] + [am[1 + bc * K + j] for j in range(nc)]
        assert got["out_ids"][0, :nc + 1].tolist() == path and (got["out_ids"][0, nc + 1:] == -1).all()
        assert got["all_ids"][0, 6:6 + nc + 1].tolist() == path and got["positions"][0] == 5 + nc + 1
        if mode == "none":
            assert nc == 0 and bc == 0, "no candidate right anywhere: the first one, one token"
        seen.add((mode, bc > 0, nc))
    if C > 1:
        assert any(m == "ties" and not later and n > 0 for m, later, n in seen), "a tie goes to the first candidate"
        assert any(later and n > 0 for _m, later, n in seen), "a later candidate wins somewhere"


def test_accept_restated_by_hand():
    # C = 2, K = 3: rows [latest, c0d0, c0d1, c0d2, c1d0, c1d1, c1d2]
    am = np.array([[10, 11, 12, 13, 21, 22, 23]])
    lps = -np.arange(7, dtype=np.float32)[None]
    drafts = np.array([[[10, 99, 12], [10, 21, 77]]])  # candidate 0: one right; candidate 1: two right
    got = ref.accept(am, lps, drafts, [2], np.zeros((1, 12), dtype=np.int64), [0, 3])
    assert got["best"].tolist() == [1] and got["n_emit"].tolist() == [3]
    assert got["out_ids"].tolist() == [[10, 21, 22, -1]] and got["out_lps"].tolist() == [[0.0, -4.0, -5.0, 0.0]]
    assert got["latest"].tolist() == [22] and got["positions"].tolist() == [5] and got["cu_seqlens"].tolist() == [0, 6]
    assert ref.commit_moves(2, 2, 3, 1, 3) == [(6, 3), (7, 4)]
    ids, pos, slots, ctx = ref.stage([30], [50], [[[51, 52, 53], [61, 62, 63]]], np.array([[4, 9]]))
    assert ids.tolist() == [50, 51, 52, 53, 61, 62, 63] and pos.tolist() == [30, 31, 32, 33, 31, 32, 33]
    assert slots.tolist() == [4 * 32 + 30, 4 * 32 + 31, 9 * 32, 9 * 32 + 1, 9 * 32 + 2, 9 * 32 + 3, 9 * 32 + 4] and ctx.tolist() == [37]


def test_propose_multi_restated_by_hand():
    tok = [21, 22, 30, 9, 21, 22, 30, 8, 22, 40, 5, 21, 22]
    row = np.full((1, 24), 999, dtype=np.int64)
    row[0, :len(tok)] = tok
    d, h = ref.propose_multi(row, [len(tok) - 1], 3, 2, 2)
    # n = 2: the sites 4 and 0 both continue with 30 (the later one is taken); n = 1: site 8 continues with 40; then none
    assert d.tolist() == [[[30, 8], [40, 5], [0, 0]]] and h.tolist() == [2]
    d, h = ref.propose_multi(row, [len(tok) - 1], 1, 2, 2)
    assert d.tolist() == [[[30, 8]]] and h.tolist() == [2]


# ---- the entry points check their arguments before touching the device --------------------------------------------------------
def test_the_library_refuses_bad_tree_arguments_without_a_gpu():
    from tgis_amd import native

    lib = native.load_library()
    rc = lib.tgis_attn_paged_tree(None, 0, None, None, None, 1, None, None, None, 0, 1, 4, 4, 64, 1, 1, 0.125, native.F16, 1,
                                  None, 0, None, None)
    assert rc == -1 and b"tgis_attn_paged" in lib.tgis_last_error()
    assert lib.tgis_spec_tree_stage(None, None, None, 2, 3, None, 1, None, None, None, None, 1, None) == -1
    assert b"tgis_spec_tree_stage" in lib.tgis_last_error()
    assert lib.tgis_spec_tree_accept(None, None, None, 9, 7, None, None, None, None, None, None, None, 0, None, None, None, 1,
                                     None) == -1 and b"tgis_spec_tree_accept" in lib.tgis_last_error()
    assert lib.tgis_spec_tree_commit(None, None, 0, 1, 1, None, 1, None, None, None, 2, 3, 1, 1, 64, 2, None) == -1
    assert b"tgis_spec_tree_commit" in lib.tgis_last_error()
    assert lib.tgis_spec_propose_multi(None, 8, None, 2, 3, 2, None, None, None, 1, None) == -1
    assert b"tgis_spec_propose_multi" in lib.tgis_last_error()
    # B = 0 returns TGIS_OK without a launch
    assert lib.tgis_spec_tree_commit(None, None, 0, 1, 1, None, 1, None, None, None, 2, 3, 0, 1, 64, 2, None) == 0
    assert lib.tgis_spec_tree_accept(None, None, None, 2, 3, None, None, None, None, None, None, None, 0, None, None, None, 0,
                                     None) == 0
    lib.tgis_clear_error()
