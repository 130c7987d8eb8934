"""-m gpu: prompt-lookup speculative decoding on the product path (FlashCausalLM(spec_tokens=K)).

Speculation must change no token: the yardsticks are the golden fixtures of tests/test_model_gpu.py (every id, logprobs
within its bars) and, for drafts the tests force, the plain run of the same model.  The prompts of the forced-draft tests
are drawn (FORCED_SEED) so that the fp32 CPU oracle, with and without the e4m3 quantiser on its keys and values, decides
each of their first 21 tokens by 0.9 logits or more (1.38 with the quantiser), and to the same ids: as the golden fixtures
are drawn (>= 0.8), more than twice the 0.35 by which test_model_gpu.py bounds a whole fp16 step's error, so an id that
differs is an error and not a near-tie."""
import numpy as np
import pytest
import torch

from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests.fixture_utils import FixtureTokenizer, load_fixture, prompt_text

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35    # tests/test_model_gpu.py, Llama f16
BIGCODE_TOL = 0.08  # tests/test_model_gpu.py, Santacoder f16
K = 3
FORCED_SEED, FORCED_LENS, FORCED_TOKENS = 113, [27, 5, 30], 21


def _llama(tensors, cfg, quantize, spec, pages=96, kv="auto", ngram=None):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, LlamaConfig(**cfg.to_dict()), torch.float16, quantize,
                          tokenizer=tok, gptq_groupsize=64)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=pages,
                       kv_cache_dtype=kv, spec_tokens=spec, spec_ngram=ngram)
    return lm, tok


def _request(rid, prompt, max_new, temperature=None, seed=None, top_n=0):
    from tgis_amd.pb import generate_pb2 as pb2

    r = pb2.Request(id=rid, inputs=prompt_text(prompt), input_length=len(prompt), truncate=False, max_output_length=max_new)
    r.details.logprobs = True
    r.details.top_n_toks = top_n
    if temperature is not None:
        r.parameters.temperature = temperature
        r.parameters.seed = seed
    return r


class Runner:
    """Drives generate_token the way the servicer does: a request that has all its tokens is pruned.  Keeps every request's
    id and logprob stream, how many tokens each step gave each request, and checks the slot contract after every step."""

    def __init__(self, lm, tok):
        self.lm, self.tok = lm, tok
        self.ids, self.lps, self.max_new, self.logits = {}, {}, {}, []
        orig = lm.__dict__.get("_untapped") or lm._process_new_tokens  # (a model serves several runners: one tap at a time)
        lm._untapped = orig

        def tapped(batch, out, *a, **kw):
            self.logits.append(out.detach().clone())
            return orig(batch, out, *a, **kw)

        lm._process_new_tokens = tapped

    def batch(self, requests, batch_id=0):
        from tgis_amd.pb import generate_pb2 as pb2

        lm = self.lm
        with lm.context_manager():
            b, errs = lm.batch_type.from_pb(pb2.Batch(id=batch_id, requests=requests), self.tok, lm.dtype, lm.device,
                                            lm.word_embeddings, None, True)
        assert not errs
        for r in requests:
            self.ids[r.id], self.lps[r.id], self.max_new[r.id] = [], [], r.max_output_length
        return b

    def step(self, batch, first=False, prune=True):
        """One generate_token; returns (the batch that goes on, or None, {request id: tokens this step gave it})."""
        lm = self.lm
        with lm.context_manager():
            toks, _in, errs, _ns = lm.generate_token(batch, first=first, for_concat=first)
        assert not errs
        got = {}
        for t in toks:
            got[t.request_id] = got.get(t.request_id, 0) + 1
            self.ids[t.request_id].append(t.token_id)
            self.lps[t.request_id].append(t.logprob)
        assert [r.id for r in batch.requests] == list(dict.fromkeys(t.request_id for t in toks)), "request-major order"
        # the reference's logical slot of every request's latest token: cu_seqlens[1:] - 1
        assert (batch.cu_seqlens[1:] - 1).tolist() == (np.cumsum(batch.input_lengths) - 1).tolist(), "slot contract"
        assert batch.position_ids.tolist() == [n - 1 for n in batch.input_lengths]
        assert batch.max_seqlen == max(batch.input_lengths)
        for r in batch.requests:
            assert len(self.ids[r.id]) <= self.max_new[r.id], "more tokens than the request may have"
        done = [r.id for r in batch.requests if len(self.ids[r.id]) >= self.max_new[r.id]]
        if prune and done:
            with lm.context_manager():
                batch = lm.batch_type.prune(batch, done)
        return batch, got

    def run(self, batch, limit=64):
        batch, _ = self.step(batch, first=True)
        while batch is not None and limit:
            batch, _ = self.step(batch)
            limit -= 1
        assert batch is None
        assert self.lm.kv_cache.free_pages == self.lm.kv_cache.num_pages, "pages leaked"


def _delta(lm, before):
    after = lm.spec_stats()
    return {k: after[k] - before[k] for k in after}


def _fixture_streams(steps):
    ids, lps = {}, {}
    for s in steps:
        for r, i, lp in zip(s["request_ids"].tolist(), s["ids"].tolist(), s["logprobs"].tolist()):
            ids.setdefault(r, []).append(i)
            lps.setdefault(r, []).append(lp)
    return ids, lps


def _check_against_fixture(run, want_ids, want_lps, tol, what, whole=True):
    for rid, want in want_ids.items():
        got = run.ids[rid]
        n = len(want) if whole else min(len(want), len(got))
        assert n >= 1 and got[:n] == want[:n], f"{what}: request {rid} ids {got} != fixture {want}"
        if whole:
            assert len(got) == len(want)
        err = float(np.abs(np.array(run.lps[rid][:n]) - np.array(want_lps[rid][:n])).max())
        assert err <= tol, f"{what}: request {rid} max |logprob - fixture| = {err:.4f} > {tol}"


# ---- golden fixtures ----------------------------------------------------------------------------------------------------------
def _fixture_cfg(meta):
    return TinyLlamaConfig(**{k: v for k, v in meta["config"].items() if k in (
        "vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
        "num_key_value_heads", "rms_norm_eps", "rope_theta", "max_position_embeddings")})


@pytest.mark.parametrize("variant", ["dense", "gptq"])
@pytest.mark.parametrize("scenario", ["equal", "ragged"])
def test_llama_fixture_streams_are_unchanged(gpu_device, variant, scenario):
    """(Without the fixtures' top-n and rank details, which keep a batch on the plain step: the ids are the same.)
    Whether a step verifies here is up to the lookups, and incidental: on these short random streams one step per scenario
    does, and gptq/equal drafts nothing at all, so that case runs the K = 0 accept path only.  No bar is set on it; the
    forced-draft tests below carry the weight of the verify step."""
    meta, steps = load_fixture(f"llama_{variant}_{scenario}")
    cfg = _fixture_cfg(meta)
    tensors = tiny_llama_tensors(cfg, seed=meta["seed"], quantize=meta["quantize"], groupsize=meta["groupsize"])
    lm, tok = _llama(tensors, cfg, meta["quantize"], K)
    run = Runner(lm, tok)
    run.run(run.batch([_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts"])]))
    _check_against_fixture(run, *_fixture_streams(steps), LOGIT_TOL, f"{variant}/{scenario}")
    st = lm.spec_stats()
    print(f"\n[spec {variant}/{scenario}] {st}")
    assert st["emitted"] == sum(len(v) - 1 for v in run.ids.values()) and st["decode_steps"] >= 1
    assert st["decode_steps"] == st["verify_steps"] + sum(v for k, v in st.items() if k.startswith("fallback_"))


@pytest.mark.parametrize("variant", ["dense", "gptq"])
def test_llama_continuous_batching_fixture_is_unchanged(gpu_device, variant):
    """Prefill A, decode x2, prefill B, concatenate, decode x2, prune id 0, decode x2: concatenate and prune draft anew."""
    meta, steps = load_fixture(f"llama_{variant}_continuous")
    cfg = _fixture_cfg(meta)
    tensors = tiny_llama_tensors(cfg, seed=meta["seed"], quantize=meta["quantize"], groupsize=meta["groupsize"])
    lm, tok = _llama(tensors, cfg, meta["quantize"], K)
    run = Runner(lm, tok)
    a = run.batch([_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts_a"])], batch_id=1)
    a, _ = run.step(a, first=True)
    for _ in range(2):
        a, _ = run.step(a)
    b = run.batch([_request(2, meta["prompts_b"][0], meta["max_new"])], batch_id=2)
    b, _ = run.step(b, first=True)
    with lm.context_manager():
        merged = lm.batch_type.concatenate([a, b])
    assert merged.spec_tokens == K and merged.spec_drafts.shape == (3, K) and merged.spec_hits.shape == (3,)
    for _ in range(2):
        merged, _ = run.step(merged)
    if any(r.id == 0 for r in merged.requests):
        with lm.context_manager():
            merged = lm.batch_type.prune(merged, [0])
    assert merged.spec_drafts.shape == (len(merged), K)
    for _ in range(2):
        if merged is not None:
            merged, _ = run.step(merged)
    if merged is not None:
        merged.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    _check_against_fixture(run, *_fixture_streams(steps), LOGIT_TOL, f"{variant}/continuous", whole=False)
    print(f"\n[spec {variant}/continuous] {lm.spec_stats()}")


def test_santacoder_fixture_stream_is_unchanged(gpu_device):
    """Multi-query attention, learned positions, no rotary: the verify rows take the same generic forward."""
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    meta, steps = load_fixture("bigcode_equal")
    cfg = TinyBigCodeConfig()
    tensors = tiny_bigcode_tensors(cfg, seed=meta["seed"], embed_scale=meta["embed_scale"])
    cfg.quantize = None
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, cfg, torch.float16, None, tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=64, spec_tokens=K)
    run = Runner(lm, tok)
    run.run(run.batch([_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts"])]))
    _check_against_fixture(run, *_fixture_streams(steps), BIGCODE_TOL, "bigcode/equal")
    print(f"\n[spec bigcode/equal] {lm.spec_stats()}")


# ---- forced drafts ------------------------------------------------------------------------------------------------------------
def _forced_prompts():
    rng = np.random.default_rng(FORCED_SEED)
    return [rng.integers(3, 256, size=n).tolist() for n in FORCED_LENS]


def _forced_models(kv="auto", k=K):
    cfg = TinyLlamaConfig()
    tensors = tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64)
    return _llama(tensors, cfg, None, 0, kv=kv), _llama(tensors, cfg, None, k, kv=kv)


def _plain_streams(lm, tok, prompts, n):
    run = Runner(lm, tok)
    run.run(run.batch([_request(i, p, n) for i, p in enumerate(prompts)]))
    assert lm.spec_stats() == dict.fromkeys(lm.spec_stats(), 0), "option off: nothing is counted"
    return run


def _force(batch, run, plain, wrong_at, K=K):
    """Overwrites the batch's drafts with each request's true continuation, wrong from index wrong_at(request id) on its
    first wrong entry only (K: none is wrong); returns {request id: tokens the step must give it}."""
    drafts, expect = [], {}
    for r in batch.requests:
        e = len(run.ids[r.id])
        d = list(plain.ids[r.id][e:e + K])
        assert len(d) == K
        j = wrong_at(r.id)
        if j < K:
            d[j] = (d[j] + 1) % 256  # the drafts behind it stay the true ones: acceptance must stop at the first miss
        drafts.append(d)
        expect[r.id] = j + 1
    dev = batch.spec_hits.device
    batch.spec_drafts = torch.tensor(drafts, dtype=torch.int64, device=dev)
    batch.spec_hits = torch.ones(len(drafts), dtype=torch.int32, device=dev)  # new tensors: the batch reads them again
    return expect


def _parting(run, plain, rid):
    """Where request rid left the plain run's stream, and by how much the plain run itself decided that token."""
    t = next((i for i, (a, b) in enumerate(zip(run.ids[rid], plain.ids[rid])) if a != b), None)
    if t is None or t >= len(plain.logits):
        return "(streams of different length)"
    top = plain.logits[t][rid].float().topk(2).values
    return f"first at token {t}, where the plain run's top-2 margin is {float(top[0] - top[1]):.3f}"


def _forced_run(lm, tok, plain, prompts, mode, steps=4, K=K, tokens=FORCED_TOKENS):
    """`steps` verify steps with forced drafts, then the batch decodes on with its own lookups to `tokens` tokens."""
    run = Runner(lm, tok)
    batch = run.batch([_request(i, p, tokens) for i, p in enumerate(prompts)])
    batch, _ = run.step(batch, first=True)
    before = lm.spec_stats()
    rng = np.random.default_rng(5)
    for s in range(steps):
        if mode == "correct":
            wrong_at = (lambda rid: K)
        elif mode == "garbage":
            wrong_at = (lambda rid: 0)
        else:  # every request another index, another one every step; K (all right) among them
            picks = {r.id: int(rng.integers(0, K + 1)) for r in batch.requests}
            wrong_at = picks.__getitem__
        expect = _force(batch, run, plain, wrong_at, K)
        if mode == "garbage":
            junk = rng.integers(3, 256, size=(len(batch), K))
            for i, r in enumerate(batch.requests):  # (a random id that happens to be the true one would be accepted)
                if int(junk[i, 0]) == plain.ids[r.id][len(run.ids[r.id])]:
                    junk[i, 0] += 1
            batch.spec_drafts = torch.from_numpy(junk).to(batch.spec_hits.device)
        batch, got = run.step(batch)
        assert got == expect, f"{mode} step {s}: tokens per request {got}, expected {expect}"
    d = _delta(lm, before)
    assert d["verify_steps"] == steps and d["decode_steps"] == steps, d
    while batch is not None:
        batch, _ = run.step(batch)
    for rid, want in plain.ids.items():
        assert run.ids[rid] == want, f"{mode}: request {rid} {run.ids[rid]} != plain run {want} {_parting(run, plain, rid)}"
        np.testing.assert_allclose(run.lps[rid], plain.lps[rid], atol=LOGIT_TOL, err_msg=f"{mode}: request {rid} logprobs")
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    return run


@pytest.fixture(scope="module")
def forced(gpu_device):
    (lm0, tok0), (lm, tok) = _forced_models()
    prompts = _forced_prompts()
    return lm, tok, _plain_streams(lm0, tok0, prompts, FORCED_TOKENS), prompts


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
def test_forced_drafts_emit_what_they_must_and_change_no_token(forced, mode):
    """Requests of 27, 5 and 30 prompt tokens: the first and the last cross a page boundary inside the verified rows, and
    the steps behind rejected rows overwrite the keys and values those rows left in the cache."""
    lm, tok, plain, prompts = forced
    before = lm.spec_stats()
    _forced_run(lm, tok, plain, prompts, mode)
    d = _delta(lm, before)
    print(f"\n[forced {mode}] {d}")
    if mode == "correct":  # 4 steps x 3 requests x K drafts, all accepted: 1 + 16 tokens each, the rest by lookups
        assert d["accepted"] >= 4 * 3 * K and d["drafted"] >= 4 * 3 * K
    assert d["emitted"] == 3 * (FORCED_TOKENS - 1)


@pytest.fixture(scope="module")
def forced_plain(gpu_device):
    """The plain run of the three forced prompts, for the models with another K."""
    (lm0, tok0), _ = _forced_models(k=0)
    prompts = _forced_prompts()
    return _plain_streams(lm0, tok0, prompts, FORCED_TOKENS), prompts


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
@pytest.mark.parametrize("k,steps", [(1, 4), (7, 2)], ids=["K1", "K7"])
def test_forced_drafts_at_the_ends_of_the_k_range(forced_plain, k, steps, mode):
    """K = 1 (two rows per request) and K = 7 (eight: the attention's q_len = 8, 32 verify rows in the bucket of four)."""
    plain, prompts = forced_plain
    _, (lm, tok) = _forced_models(k=k)
    _forced_run(lm, tok, plain, prompts, mode, steps=steps, K=k)


# eight requests fill the bucket of 8: 32 verify rows at K = 3 and, at K = 7, the 64 rows the step rule allows at the most.
# Drawn like the three prompts above: the fp32 oracle decides each of their first WIDE_TOKENS tokens by >= 0.94 logits.
WIDE_SEED, WIDE_LENS, WIDE_TOKENS = 589, [27, 5, 30, 12, 31, 9, 20, 3], 13


@pytest.fixture(scope="module")
def wide_plain(gpu_device):
    (lm0, tok0), _ = _forced_models(k=0)
    rng = np.random.default_rng(WIDE_SEED)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in WIDE_LENS]
    return _plain_streams(lm0, tok0, prompts, WIDE_TOKENS), prompts


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
@pytest.mark.parametrize("k,steps", [(3, 3), (7, 1)], ids=["K3-32rows", "K7-64rows"])
def test_forced_drafts_fill_the_row_bound(wide_plain, k, steps, mode):
    plain, prompts = wide_plain
    _, (lm, tok) = _forced_models(k=k)
    run = _forced_run(lm, tok, plain, prompts, mode, steps=steps, K=k, tokens=WIDE_TOKENS)
    assert any(lg.shape[0] == 8 * (k + 1) for lg in run.logits), "no verify forward of the full bucket ran"


def test_forced_drafts_on_the_e4m3_cache_match_its_plain_run(gpu_device):
    (lm0, tok0), (lm, tok) = _forced_models(kv="fp8_e4m3")
    assert lm.kv_cache.is_fp8
    prompts = _forced_prompts()
    plain = _plain_streams(lm0, tok0, prompts, FORCED_TOKENS)
    _forced_run(lm, tok, plain, prompts, "mixed")


def test_the_verify_graph_equals_the_eager_verify_step(forced):
    lm, tok, plain, prompts = forced
    assert lm.use_graphs
    captured = _forced_run(lm, tok, plain, prompts, "mixed")
    assert any(len(k) == 3 and g.graph is not None for k, g in lm._graphs.items()), "no verify step was captured"
    lm.use_graphs = False
    try:
        eager = _forced_run(lm, tok, plain, prompts, "mixed")
    finally:
        lm.use_graphs = True
    assert len(captured.logits) == len(eager.logits)
    assert any(lg.shape[0] == 3 * (K + 1) for lg in captured.logits)
    for s, (a, b) in enumerate(zip(captured.logits, eager.logits)):
        assert a.shape == b.shape and torch.equal(a, b), f"step {s}: captured and eager logits differ"


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------
def _loop(n, base=20):
    """A prompt that repeats itself: its lookup always hits."""
    return [base + i % 3 for i in range(n)]


def _same_as_off(requests_of, pages=96, steps=None, force_hits=False):
    """Runs the same requests through a model with the option off and one with it on; returns (lm on, its stats).
    force_hits: every lookup of the speculating model is made to look like a hit before each decode step."""
    cfg = TinyLlamaConfig()
    tensors = tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64)
    runs = []
    for spec in (0, K):
        lm, tok = _llama(tensors, cfg, None, spec, pages=pages)
        run = Runner(lm, tok)
        batch = run.batch(requests_of())
        if steps is None:
            run.run(batch)
        else:
            batch, _ = run.step(batch, first=True)
            for _ in range(steps):
                if force_hits and spec:
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
    assert st["drafted"] == st["accepted"] == 0


def test_a_sampling_request_keeps_its_batch_on_the_plain_step(gpu_device):
    _lm, st = _same_as_off(lambda: [_request(0, _loop(9), 6), _request(1, _loop(7), 6, temperature=0.8, seed=11)])
    _only(st, "not_greedy")


def test_a_request_with_top_n_tokens_keeps_its_batch_on_the_plain_step(gpu_device):
    _lm, st = _same_as_off(lambda: [_request(0, _loop(9), 6), _request(1, _loop(7), 6, top_n=2)])
    _only(st, "details")


def test_a_batch_whose_bucket_times_k_plus_1_exceeds_64_rows_stays_plain(gpu_device):
    _lm, st = _same_as_off(lambda: [_request(i, _loop(4 + i, base=20 + i), 4) for i in range(17)], pages=64)  # bucket 24
    _only(st, "rows")


def test_requests_with_fewer_than_k_plus_1_tokens_left_stay_plain(gpu_device):
    _lm, st = _same_as_off(lambda: [_request(0, _loop(9), K + 1), _request(1, _loop(7), K + 1)])  # K left after the prefill
    _only(st, "remaining")


def test_a_pool_too_small_for_the_look_ahead_raises_nothing(gpu_device):
    """Two requests whose latest token sits at position 30 of their only page, and no page left: the look-ahead to position
    33 cannot be served; the plain steps at positions 30 and 31 need no page and run as they always did."""
    lm, st = _same_as_off(lambda: [_request(0, _loop(30), 12), _request(1, _loop(30, base=40), 12)], pages=2, steps=2,
                          force_hits=True)
    _only(st, "pages")
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


def test_lookups_alone_speed_a_repeating_request_up(gpu_device):
    """No forcing: a request whose greedy continuation settles into a cycle is drafted from its own context.  The ragged
    fixture's one-token prompt repeats id 21; with the option on it needs fewer steps than tokens."""
    meta, steps = load_fixture("llama_dense_ragged")
    cfg = _fixture_cfg(meta)
    tensors = tiny_llama_tensors(cfg, seed=meta["seed"], quantize=None, groupsize=meta["groupsize"])
    lm, tok = _llama(tensors, cfg, None, K, ngram=1)
    run = Runner(lm, tok)
    run.run(run.batch([_request(3, meta["prompts"][3], meta["max_new"])]))
    want, _ = _fixture_streams(steps)
    assert run.ids[3] == want[3] == [21] * 6
    st = lm.spec_stats()
    assert st["verify_steps"] >= 1 and st["accepted"] >= 1 and st["decode_steps"] < 5, st


def test_stale_lookups_are_drafted_anew_once_the_batch_turns_greedy(gpu_device):
    """The same request with min_new_tokens = 3: below it the EOS mask keeps the batch off the plain-greedy path, the steps
    are plain and leave the drafts stale; the first greedy step drafts anew from the context before it looks at the hits,
    and the cycle is verified as above.  Every id and logprob is the one the option off gives.
    The request may have 3 + K + 1 = 7 tokens, one more than the fixture's 6: with 6, the first greedy step has K tokens
    left, one short of what a verify step needs (`fallback_remaining`), and no request of that fixture could verify."""
    meta, _steps = load_fixture("llama_dense_ragged")
    cfg = _fixture_cfg(meta)
    tensors = tiny_llama_tensors(cfg, seed=meta["seed"], quantize=None, groupsize=meta["groupsize"])
    runs = []
    for spec in (0, K):
        lm, tok = _llama(tensors, cfg, None, spec, ngram=1)
        request = _request(3, meta["prompts"][3], 3 + K + 1)
        request.parameters.min_new_tokens = 3
        run = Runner(lm, tok)
        run.run(run.batch([request]))
        runs.append((lm, run))
    (lm0, off), (lm, on) = runs
    print(f"\n[stale then redraft] ids {on.ids[3]} / {off.ids[3]}, max |logprob on - off| = "
          f"{max(abs(a - b) for a, b in zip(on.lps[3], off.lps[3])):.3g}, {lm.spec_stats()}")
    assert on.ids == off.ids and on.lps == off.lps and on.ids[3][:6] == [21] * 6
    assert lm0.spec_stats() == dict.fromkeys(lm0.spec_stats(), 0)
    st = lm.spec_stats()
    assert st["fallback_not_greedy"] >= 1, st
    assert st["verify_steps"] >= 1 and st["accepted"] >= 1, st
