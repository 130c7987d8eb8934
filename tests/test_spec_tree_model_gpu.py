"""-m gpu: several draft candidates per request on the product path (FlashCausalLM(spec_tokens=K, spec_candidates=C)).

Like tests/test_spec_model_gpu.py, whose Runner, forced prompts and models these tests use: speculation must change no
token.  The forced prompts' first 21 tokens are decided by 0.9 logits or more, so an id that differs from the plain run's is
an error.  A step's candidates are forced: per request one candidate (drawn, or none) holds the true continuation, wrong from
a drawn index on; the others hold junk whose first token is not the true one.  Each request must then get exactly the tokens
that candidate earns, and the steps behind a step won by a later candidate read the keys and values tgis_spec_tree_commit
moved."""
import numpy as np
import pytest
import torch

from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests.fixture_utils import FixtureTokenizer, load_fixture
from tests.test_spec_model_gpu import (BIGCODE_TOL, FORCED_TOKENS, LOGIT_TOL, WIDE_LENS, WIDE_SEED, WIDE_TOKENS, Runner, _delta,
                                       _forced_models, _forced_prompts, _loop, _parting, _plain_streams, _request)

pytestmark = pytest.mark.gpu

K = 3


def _tree_llama(C, k=K, kv="auto", pages=96, **kw):
    """tests/test_spec_model_gpu.py's dense TinyLlama with spec_candidates (None: the argument is left out)."""
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyLlamaConfig()
    tensors = tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64)
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({n: v.clone() for n, v in tensors.items()}, LlamaConfig(**cfg.to_dict()), torch.float16, None,
                          tokenizer=tok, gptq_groupsize=64)
    if C is not None:
        kw["spec_candidates"] = C
    return FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=pages,
                         kv_cache_dtype=kv, spec_tokens=k, **kw), tok


def _force_tree(batch, run, plain, rng, C, k, pick=None):
    """New drafts [B, C, K] for the batch; returns ({request id: tokens the step must give it}, how many requests a later
    candidate wins).  pick(request id) -> (which candidate holds the truth or -1, first wrong index or K) overrides the draw."""
    drafts, expect, wins = [], {}, 0
    for r in batch.requests:
        e = len(run.ids[r.id])
        true = list(plain.ids[r.id][e:e + k])
        assert len(true) == k
        which, wrong = pick(r.id) if pick else (int(rng.integers(-1, C)), int(rng.integers(0, k + 1)))
        cands = []
        for c in range(C):
            if c == which:
                d = list(true)
                if wrong < k:
                    d[wrong] = (d[wrong] + 1) % 256  # the drafts behind it stay true: acceptance must stop at the first miss
            else:
                d = rng.integers(3, 256, size=k).tolist()
                if d[0] == true[0]:  # (junk that happens to start right would be accepted)
                    d[0] = (d[0] + 1) % 256
            cands.append(d)
        n = wrong + 1 if which >= 0 else 1
        expect[r.id] = n
        wins += int(which > 0 and n > 1)
        drafts.append(cands)
    dev = batch.spec_hits.device
    batch.spec_drafts = torch.tensor(drafts, dtype=torch.int64, device=dev)
    batch.spec_hits = torch.ones(len(drafts), dtype=torch.int32, device=dev)  # new tensors: the batch reads them again
    return expect, wins


def _tree_run(lm, tok, plain, prompts, C, steps, k=K, tokens=FORCED_TOKENS, tol=LOGIT_TOL, seed=5):
    """`steps` tree verify steps with forced candidates — in the first the LAST candidate is right, wholly or but for its last
    draft, so a later candidate wins it and every later step reads what the commit moved — then the batch decodes on with
    its own lookups to `tokens` tokens (at least 4 more steps at 21 tokens)."""
    run = Runner(lm, tok)
    batch = run.batch([_request(i, p, tokens) for i, p in enumerate(prompts)])
    batch, _ = run.step(batch, first=True)
    before = lm.spec_stats()
    rng = np.random.default_rng(seed)
    wins = 0
    for s in range(steps):
        pick = (lambda rid: (C - 1, k - rid % 2 if k > 1 else k)) if s == 0 else None
        expect, w = _force_tree(batch, run, plain, rng, C, k, pick)
        wins += w
        assert batch.spec_drafts.shape == (len(batch), C, k)
        batch, got = run.step(batch)
        assert got == expect, f"step {s}: tokens per request {got}, expected {expect}"
    d = _delta(lm, before)
    assert d["verify_steps"] == steps and d["decode_steps"] == steps, d
    assert d["won_by_later_candidate"] == wins and wins > 0, (d, wins)
    assert d["drafted"] == steps * len(prompts) * C * k, d
    after_forced = lm.spec_stats()["decode_steps"]
    while batch is not None:
        batch, _ = run.step(batch)
    if tokens == FORCED_TOKENS:
        behind = steps - 1 + lm.spec_stats()["decode_steps"] - after_forced
        assert behind >= 4, "too few steps behind the first step's win to show a wrong commit"
    for rid, want in plain.ids.items():
        assert run.ids[rid] == want, f"request {rid} {run.ids[rid]} != plain run {want} {_parting(run, plain, rid)}"
        np.testing.assert_allclose(run.lps[rid], plain.lps[rid], atol=tol, err_msg=f"request {rid} logprobs")
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages, "pages leaked"
    return run


@pytest.fixture(scope="module")
def plain(gpu_device):
    (lm0, tok0), _ = _forced_models(k=0)
    prompts = _forced_prompts()
    return _plain_streams(lm0, tok0, prompts, FORCED_TOKENS), prompts


# ---- forced candidates -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3])
def test_forced_candidates_emit_what_they_must_and_change_no_token(plain, C):
    """Requests of 27, 5 and 30 prompt tokens: the first and the last cross a page boundary inside the 1 + C K rows.  Three
    forced steps: each needs C K + 1 tokens left of the 21."""
    streams, prompts = plain
    lm, tok = _tree_llama(C)
    assert lm.spec_candidates == C
    _tree_run(lm, tok, streams, prompts, C, steps=3)
    assert all(len(key) in (2, 4) for key in lm._graphs), list(lm._graphs)
    assert any(len(key) == 4 and key[2:] == (K, C) for key in lm._graphs)


def test_the_option_from_the_environment(plain, monkeypatch):
    streams, prompts = plain
    monkeypatch.setenv("TGIS_SPEC_CANDIDATES", "2")
    lm, tok = _tree_llama(None)
    monkeypatch.delenv("TGIS_SPEC_CANDIDATES")
    assert lm.spec_candidates == 2
    _tree_run(lm, tok, streams, prompts, 2, steps=2, seed=9)


def test_forced_candidates_on_the_e4m3_cache_match_its_plain_run(gpu_device):
    (lm0, tok0), _ = _forced_models(kv="fp8_e4m3", k=0)
    prompts = _forced_prompts()
    streams = _plain_streams(lm0, tok0, prompts, FORCED_TOKENS)
    lm, tok = _tree_llama(3, kv="fp8_e4m3")
    assert lm.kv_cache.is_fp8
    _tree_run(lm, tok, streams, prompts, 3, steps=3)


def test_the_tree_graph_equals_the_eager_tree_step(plain):
    streams, prompts = plain
    lm, tok = _tree_llama(2)
    assert lm.use_graphs
    captured = _tree_run(lm, tok, streams, prompts, 2, steps=3)
    assert any(len(key) == 4 and g.graph is not None for key, g in lm._graphs.items()), "no tree verify step was captured"
    lm.use_graphs = False
    try:
        eager = _tree_run(lm, tok, streams, prompts, 2, steps=3)
    finally:
        lm.use_graphs = True
    assert len(captured.logits) == len(eager.logits)
    assert any(lg.shape[0] == 3 * (1 + 2 * K) for lg in captured.logits)
    for s, (a, b) in enumerate(zip(captured.logits, eager.logits)):
        assert a.shape == b.shape and torch.equal(a, b), f"step {s}: captured and eager logits differ"


def test_eight_requests_fill_56_rows(gpu_device):
    (lm0, tok0), _ = _forced_models(k=0)
    rng = np.random.default_rng(WIDE_SEED)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in WIDE_LENS]
    streams = _plain_streams(lm0, tok0, prompts, WIDE_TOKENS)
    lm, tok = _tree_llama(2)
    run = _tree_run(lm, tok, streams, prompts, 2, steps=2, tokens=WIDE_TOKENS)
    assert any(lg.shape[0] == 8 * (1 + 2 * K) for lg in run.logits), "no tree verify forward of the full bucket ran"


def test_santacoder_multi_query(gpu_device):
    """Multi-query attention, learned positions by depth, no rotary; C = 3, K = 1: four rows per request.  The fixture's
    model and prompts (its six tokens are decided by 0.55 logits or more): one forced step — the next has fewer than
    C K + 1 tokens left — which the last candidate wins for every request, then plain steps behind the commit."""
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    meta, _steps = load_fixture("bigcode_equal")
    cfg = TinyBigCodeConfig()
    tensors = tiny_bigcode_tensors(cfg, seed=meta["seed"], embed_scale=meta["embed_scale"])
    cfg.quantize = None
    tok = FixtureTokenizer(cfg.vocab_size)

    def build(**kw):
        eng = InferenceEngine({n: v.clone() for n, v in tensors.items()}, cfg, torch.float16, None, tokenizer=tok)
        return FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=64, **kw)

    streams = _plain_streams(build(), tok, meta["prompts"], meta["max_new"])
    lm = build(spec_tokens=1, spec_candidates=3)
    _tree_run(lm, tok, streams, meta["prompts"], 3, steps=1, k=1, tokens=meta["max_new"], tol=BIGCODE_TOL)
    assert lm.spec_stats()["fallback_remaining"] >= 1


MQA16_SEED, MQA16_EMBED_SCALE, MQA16_TOKENS, MQA16_MARGIN = 21, 3.0, 10, 0.5


def test_santacoder_multi_query_sixteen_heads(gpu_device):
    """C = 3, K = 1 on a Santacoder of 16 heads over one kv head (hidden 1024, D 64): R = 4 rows per request with Gp = 16,
    so R Gp = 64 sits exactly on the bound of the attention's decode form (`check_tree_rows`), one q token per tile and four
    q tiles per request; learned positions by depth, the commit at Hkv = 1.  The yardstick is the model's own plain run
    over the forced prompts (tests/test_spec_model_gpu.py): with weights of seed 21 and embed_scale 3.0 its first ten tokens
    per request are decided by 0.85 logits or more (measured on an MI355X; the test asserts 0.5, more than six times
    BIGCODE_TOL), so an id that differs is an error and not a near-tie, and the streams are not constant (request 1 goes
    159 x 4 then 170, request 2 127 then 216).  Two forced steps, the first won by the last candidate for every request,
    then plain steps behind the commit (a third tree step would have fewer than C K + 1 tokens left)."""
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyBigCodeConfig(hidden_size=1024, n_inner=2048, num_attention_heads=16)
    tensors = tiny_bigcode_tensors(cfg, seed=MQA16_SEED, embed_scale=MQA16_EMBED_SCALE)
    cfg.quantize = None
    tok = FixtureTokenizer(cfg.vocab_size)

    def build(**kw):
        eng = InferenceEngine({n: v.clone() for n, v in tensors.items()}, cfg, torch.float16, None, tokenizer=tok)
        return FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=64, **kw)

    prompts = _forced_prompts()
    streams = _plain_streams(build(), tok, prompts, MQA16_TOKENS)
    margins = []
    for lg in streams.logits:
        top = lg.float().topk(2, dim=-1).values
        margins += (top[:, 0] - top[:, 1]).tolist()
    print(f"\n[mqa16] plain run: min top-2 margin {min(margins):.3f} over {len(margins)} rows; ids {streams.ids}")
    assert min(margins) >= MQA16_MARGIN, f"the plain run decides a token by {min(margins):.3f} logits: choose other weights"
    assert any(len(set(ids)) > 1 for ids in streams.ids.values()), "constant streams would hide a wrong commit"
    lm = build(spec_tokens=1, spec_candidates=3)
    assert (lm.num_heads, lm.num_kv_heads, lm.head_size) == (16, 1, 64)
    _tree_run(lm, tok, streams, prompts, 3, steps=2, k=1, tokens=MQA16_TOKENS, tol=BIGCODE_TOL)
    assert any(key[2:] == (1, 3) and g.R1 == 4 and g.num_splits == 1 for key, g in lm._graphs.items())


# ---- fallbacks -------------------------------------------------------------------------------------------------------------
def _same_as_off(requests_of, C=2, pages=96, steps=None, force_hits=False):
    """The same requests through a model with the option off and one with C candidates; returns (lm on, its stats)."""
    runs = []
    for lm, tok in (_tree_llama(None, k=0, pages=pages), _tree_llama(C, pages=pages)):
        run = Runner(lm, tok)
        batch = run.batch(requests_of())
        if steps is None:
            run.run(batch)
        else:
            batch, _ = run.step(batch, first=True)
            for _ in range(steps):
                if force_hits and lm.spec_tokens:
                    batch.spec_hits = torch.ones_like(batch.spec_hits)
                batch, _ = run.step(batch)
            batch.release()
        runs.append((lm, run))
    (lm0, off), (lm, on) = runs
    assert on.ids == off.ids, "a fallback step changed a token"
    for rid in on.lps:
        assert on.lps[rid] == off.lps[rid], "the plain step of a speculating model is the plain step"
    assert lm0.spec_stats() == dict.fromkeys(lm0.spec_stats(), 0)
    return lm, lm.spec_stats()


def _only(st, cause):
    assert st["verify_steps"] == 0 and st["decode_steps"] > 0, st
    assert st["fallback_" + cause] == st["decode_steps"], st
    assert st["drafted"] == st["accepted"] == st["won_by_later_candidate"] == 0


def test_seventeen_requests_stay_plain(gpu_device):
    _lm, st = _same_as_off(lambda: [_request(i, _loop(4 + i, base=20 + i), 4) for i in range(17)], pages=64)  # bucket 24
    _only(st, "rows")


def test_requests_with_fewer_than_c_k_plus_1_tokens_left_stay_plain(gpu_device):
    # C K = 6 left after the prefill, one short; a chain (K + 1 = 4) would have verified
    _lm, st = _same_as_off(lambda: [_request(0, _loop(9), 2 * K + 1), _request(1, _loop(7), 2 * K + 1)])
    _only(st, "remaining")


def test_a_pool_too_small_for_the_look_ahead_raises_nothing(gpu_device):
    lm, st = _same_as_off(lambda: [_request(0, _loop(30), 12), _request(1, _loop(30, base=40), 12)], pages=2, steps=2,
                          force_hits=True)
    _only(st, "pages")
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


# ---- the batch ---------------------------------------------------------------------------------------------------------------
def test_concatenate_and_prune_keep_the_candidates(gpu_device):
    C = 3
    lm, tok = _tree_llama(C)
    run = Runner(lm, tok)
    a = run.batch([_request(0, _loop(9), 12), _request(1, _loop(7, base=40), 12)], batch_id=1)
    a, _ = run.step(a, first=True)
    assert a.spec_candidates == C and a.spec_drafts.shape == (2, C, K) and a.spec_hits.shape == (2,)
    a, _ = run.step(a)
    b = run.batch([_request(2, _loop(11, base=60), 12)], batch_id=2)
    b, _ = run.step(b, first=True)
    with lm.context_manager():
        merged = lm.batch_type.concatenate([a, b])
    assert merged.spec_candidates == C and merged.spec_drafts.shape == (3, C, K) and merged.spec_hits.shape == (3,)
    merged, _ = run.step(merged)
    with lm.context_manager():
        merged = lm.batch_type.prune(merged, [0])
    assert merged.spec_drafts.shape == (len(merged), C, K)
    merged, _ = run.step(merged)
    merged.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


# ---- one candidate is the path without the option -----------------------------------------------------------------------------
def test_one_candidate_is_the_chain(gpu_device):
    """spec_candidates=1 builds only (bucket, width) and (bucket, width, K) graphs, and its streams are those of a model
    built without the argument, ids and logprobs exactly (the same launches on the same inputs)."""
    reqs = lambda: [_request(0, _loop(9), 14), _request(1, _loop(7, base=40), 14), _request(2, _loop(12, base=60), 14)]  # noqa: E731
    runs = []
    for C in (None, 1):
        lm, tok = _tree_llama(C)
        run = Runner(lm, tok)
        batch, _ = run.step(run.batch(reqs()), first=True)
        for _ in range(2):  # whatever the lookups drafted is verified: every lookup is made to look like a hit
            batch.spec_hits = torch.ones_like(batch.spec_hits)
            batch, _ = run.step(batch)
        while batch is not None:
            batch, _ = run.step(batch)
        assert lm.spec_candidates == 1 and all(len(key) in (2, 3) for key in lm._graphs), list(lm._graphs)
        assert any(len(key) == 3 for key in lm._graphs)
        runs.append((lm, run))
    (lm_a, a), (lm_b, b) = runs
    assert a.ids == b.ids and a.lps == b.lps
    assert lm_a.spec_stats() == lm_b.spec_stats() and lm_a.spec_stats()["verify_steps"] >= 1
