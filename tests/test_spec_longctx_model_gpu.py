"""-m gpu: speculative decoding and prefix reuse over contexts long enough for the attention's key splits at more than
one q token per sequence (tgis_attn_num_splits_q): the tiny Llama (4 q heads on 2 kv heads, D 64, dense f16) behind prompts
of 1100 - 1200 tokens, whose verify graphs hold 40-page tables and take two splits.

Speculation must change no token: the yardstick is the plain run (options off) of the same requests, with drafts forced
the way tests/test_spec_model_gpu.py forces them.  The prompts (and the sampled request's seed) are drawn on the CPU
(tests/golden/make_spec_longctx_prompts.py) so that the fp32 oracle decides every compared token: a greedy request's first
TOKENS tokens by >= 0.9 logits, also with the e4m3 round trip on its keys and values and to the same ids; the sampled
request's races by >= 2 LOGIT_TOL / T = 0.875 in warped-score units, one of them at least against the argmax.  Achieved
margins, the minimum over a request's TOKENS tokens (greedy: over both caches):
  greedy    0.929, 1.960, 5.830
  sampled   2.720
Prefix reuse: suffixes of 3 and 2 tokens in one batch behind a registered header of 1056 tokens (33 pages); their
first-token logits against the fp32 oracle on the full sequences, within tests/test_model_gpu.py's f16 bar."""
import numpy as np
import pytest
import torch

from oracle.llama_ref import LlamaRef
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests.fixture_utils import FixtureTokenizer
from tests.test_prefix_reuse_model_gpu import Driver
from tests.test_spec_model_gpu import LOGIT_TOL, Runner, _delta, _force, _forced_run, _plain_streams, _request

pytestmark = pytest.mark.gpu

K, TOKENS, T = 3, 13, 0.8
PROMPT_SEED = 8192
# per request: prompt length and the draw the search settled on (prompt number and, for the sampled request, its seed)
SCENARIOS = {
    "greedy": [dict(length=1150, draw=0), dict(length=1101, draw=1), dict(length=1190, draw=0)],
    "sampled": [dict(length=1170, draw=23, temperature=T)],
}
HEADER_SEED, HEADER_TOKENS = 77, 1056


def tiny_config():
    return TinyLlamaConfig(max_position_embeddings=2048)


def drawn_prompt(length, draw):
    return np.random.default_rng([PROMPT_SEED, length, draw]).integers(3, 256, size=length).tolist()


def oracle_params(r):
    return dict(temperature=r.get("temperature", 1.0), rep_penalty=1.0, eos_id=2, sample=int("temperature" in r))


def bound_of(r):
    return 2 * LOGIT_TOL / r["temperature"] if "temperature" in r else 0.9


_TENSORS = {}


def _model(spec=0, sampling=None, kv="auto", reuse=False):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = tiny_config()
    if not _TENSORS:
        _TENSORS.update(tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64))
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in _TENSORS.items()}, LlamaConfig(**cfg.to_dict()), torch.float16, None,
                          tokenizer=tok, gptq_groupsize=64)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=176,
                       kv_cache_dtype=kv, spec_tokens=spec, spec_sampling=sampling, kv_prefix_reuse=reuse)
    return lm, tok


def _prompts(name, n=None):
    return [drawn_prompt(r["length"], r["draw"]) for r in SCENARIOS[name][:n]]


def _verify_graphs(lm):
    return [g for key, g in lm._graphs.items() if len(key) == 3]


def _check_split_graphs(lm, k):
    """Every verify graph of the model held a table of >= 40 pages and asked for more than one key split."""
    graphs = _verify_graphs(lm)
    assert graphs, "no verify step ran"
    for g in graphs:
        assert g.K == k and g.block_tables.shape[1] >= 40 and g.num_splits > 1, \
            (g.K, tuple(g.block_tables.shape), g.num_splits)


_PLAIN = {}


def _plain(n, kv="auto"):
    """The plain run (options off) of the first n greedy prompts, computed once and left unchanged."""
    if (n, kv) not in _PLAIN:
        lm0, tok0 = _model(kv=kv)
        _PLAIN[n, kv] = _plain_streams(lm0, tok0, _prompts("greedy", n), TOKENS)
    return _PLAIN[n, kv]


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
@pytest.mark.parametrize("k,n,steps", [(3, 1, 3), (3, 3, 3), (7, 1, 1)], ids=["K3-B1", "K3-B3", "K7-B1"])
def test_forced_drafts_over_split_keys_change_no_token(gpu_device, k, n, steps, mode):
    """All right emits K + 1 tokens, first wrong at a drawn index j emits j + 1, garbage emits 1 (_forced_run asserts it
    per step), and every id is the plain run's."""
    lm, tok = _model(k)
    _forced_run(lm, tok, _plain(n), _prompts("greedy", n), mode, steps=steps, K=k, tokens=TOKENS)
    _check_split_graphs(lm, k)


def test_the_split_verify_graph_equals_the_eager_verify_step(gpu_device):
    lm, tok = _model(K)
    assert lm.use_graphs
    plain, prompts = _plain(3), _prompts("greedy", 3)
    captured = _forced_run(lm, tok, plain, prompts, "mixed", tokens=TOKENS, steps=3)
    assert any(g.graph is not None for g in _verify_graphs(lm)), "no verify step was captured"
    _check_split_graphs(lm, K)
    lm.use_graphs = False
    try:
        eager = _forced_run(lm, tok, plain, prompts, "mixed", tokens=TOKENS, steps=3)
    finally:
        lm.use_graphs = True
    assert len(captured.logits) == len(eager.logits)
    assert any(lg.shape[0] == 3 * (K + 1) for lg in captured.logits)
    for s, (a, b) in enumerate(zip(captured.logits, eager.logits)):
        assert a.shape == b.shape and torch.equal(a, b), f"step {s}: captured and eager logits differ"


def test_forced_drafts_over_split_keys_on_the_e4m3_cache_match_its_plain_run(gpu_device):
    lm, tok = _model(K, kv="fp8_e4m3")
    assert lm.kv_cache.is_fp8
    _forced_run(lm, tok, _plain(3, kv="fp8_e4m3"), _prompts("greedy", 3), "mixed", tokens=TOKENS, steps=3)
    _check_split_graphs(lm, K)


def _sampled_requests():
    return [_request(i, drawn_prompt(r["length"], r["draw"]), TOKENS, temperature=r["temperature"], seed=r["draw"])
            for i, r in enumerate(SCENARIOS["sampled"])]


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
def test_a_seeded_sampled_request_over_split_keys_emits_its_plain_stream(gpu_device, mode):
    lm0, tok0 = _model()
    plain = Runner(lm0, tok0)
    plain.run(plain.batch(_sampled_requests()))
    lm, tok = _model(K, sampling=True)
    run = Runner(lm, tok)
    batch, _ = run.step(run.batch(_sampled_requests()), first=True)
    before = lm.spec_stats()
    rng = np.random.default_rng(5)
    for s in range(3):
        j = {"correct": K, "garbage": 0}.get(mode, int(rng.integers(0, K + 1)))
        expect = _force(batch, run, plain, lambda rid: j, K)
        if mode == "garbage":
            junk = rng.integers(3, 256, size=(len(batch), K))
            if int(junk[0, 0]) == plain.ids[0][len(run.ids[0])]:  # (a random id that happens to be the true one)
                junk[0, 0] += 1
            batch.spec_drafts = torch.from_numpy(junk).to(batch.spec_hits.device)
        batch, got = run.step(batch)
        assert got == expect, f"sampled/{mode} step {s}: tokens per request {got}, expected {expect}"
    d = _delta(lm, before)
    assert d["verify_steps"] == d["verify_steps_sampled"] == d["decode_steps"] == 3, d
    while batch is not None:
        batch, _ = run.step(batch)
    assert run.ids[0] == plain.ids[0], f"sampled/{mode}: {run.ids[0]} != plain run {plain.ids[0]}"
    np.testing.assert_allclose(run.lps[0], plain.lps[0], atol=LOGIT_TOL)
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages, "pages leaked"
    _check_split_graphs(lm, K)


def test_short_suffixes_behind_a_long_registered_header_split_their_keys(gpu_device, monkeypatch):
    """Suffixes of 3 and 2 tokens in one batch (ragged cu_seqlens_q: 5 rows where the launcher counts 2 x 3) behind 1056
    reused tokens: the suffix forward asks for more than one split, and the first-token logits hold the f16 bar."""
    from tgis_amd import native

    cfg = tiny_config()
    lm, tok = _model(reuse=True)
    ref = LlamaRef(cfg, _TENSORS)
    d = Driver(lm, tok, lambda seqs: ref.generate_greedy(seqs, 1)[0]["logits"].numpy(), torch.float16, LOGIT_TOL,
               check_tokens=False)
    rng = np.random.default_rng(HEADER_SEED)
    header = rng.integers(3, 256, size=HEADER_TOKENS).tolist()
    first = d.batch([header + rng.integers(3, 256, size=3).tolist()], 0, 1)
    d.step(first, "header request", first=True)
    first.release()
    calls = []
    orig = native.attn_paged

    def spy(*a, **kw):
        calls.append((a[8], a[12], a[13], a[15]))  # B, max_q_len, max_ctx, num_splits
        return orig(*a, **kw)

    monkeypatch.setattr(native, "attn_paged", spy)
    b = d.batch([header + rng.integers(3, 256, size=n).tolist() for n in (3, 2)], 1, 2)
    d.step(b, "suffixes 3, 2 behind 1056 reused tokens", first=True)
    assert b.reused_lengths == [HEADER_TOKENS, HEADER_TOKENS]
    assert calls and all(c[:3] == (2, 3, HEADER_TOKENS + 3) and c[3] > 1 for c in calls), calls
    assert len(calls) == cfg.num_hidden_layers
    b.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
