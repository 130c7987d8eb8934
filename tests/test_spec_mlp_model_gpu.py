"""-m gpu: the MLP speculator drafter on the product path (FlashCausalLM(speculator=DIR, spec_tokens=K)).

A drafter may change no token: the golden fixtures of tests/test_model_gpu.py stay the yardstick for the ids and logprobs.
What the drafter itself must do is checked three ways: a speculator whose drafts are known by construction (the successor
speculator: t + 1, t + 3, t + 6 behind token t, each head decided by sqrt(V) = 16), the hidden rows it reads compared bit
for bit with the rows that fed lm_head, and a random speculator with wide heads against the fp64 restatement
(tests/spec_mlp_ref.py) fed with the device's own states.  The runner is a copy of tests/test_spec_model_gpu.py's."""
import numpy as np
import pytest
import torch

from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests import spec_mlp_ref as ref
from tests.fixture_utils import FixtureTokenizer, load_fixture, prompt_text

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35    # tests/test_model_gpu.py, Llama f16: the bar for a whole f16 step
BIGCODE_TOL = 0.08  # tests/test_model_gpu.py, Santacoder f16
K = 3
E = V = 256         # the tiny fixture models
FORCED_SEED, FORCED_LENS, FORCED_TOKENS = 113, [27, 5, 30], 21  # tests/test_spec_model_gpu.py: decided by >= 0.9 logits
# the speculator of test_drafts_equal_the_specification: heads drawn wide, so that typical top-2 gaps are several logits while
# the f16 error of its logits stays near 0.03.  tests/test_spec_mlp_cpu.py checks the seed on stand-in states.
WIDE_SEED, WIDE_INNER, WIDE_HEAD_STD, UNDECIDED_SHARE = 3, 64, 4.0, 0.25


def _spec_dir(tmp_path_factory, spec, name):
    return ref.write_checkpoint(str(tmp_path_factory.mktemp(name)), spec)


@pytest.fixture(scope="module")
def random_dir(tmp_path_factory):
    return _spec_dir(tmp_path_factory, ref.make_random(E, 64, V, 3, seed=11), "random")


@pytest.fixture(scope="module")
def successor_dir(tmp_path_factory):
    return _spec_dir(tmp_path_factory, ref.make_successor(E, V, 3), "successor")


def _llama(tensors, cfg, quantize, speculator=None, spec=K, pages=96, kv="auto", reuse=None):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, LlamaConfig(**cfg.to_dict()), torch.float16, quantize,
                          tokenizer=tok, gptq_groupsize=64)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=pages,
                       kv_cache_dtype=kv, spec_tokens=spec, speculator=speculator, kv_prefix_reuse=reuse)
    return lm, tok


def _dense(speculator=None, spec=K, **kw):
    cfg = TinyLlamaConfig()
    return _llama(tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64), cfg, None, speculator, spec, **kw)


def _request(rid, prompt, max_new, temperature=None, seed=None, input_toks=False):
    from tgis_amd.pb import generate_pb2 as pb2

    r = pb2.Request(id=rid, inputs=prompt_text(prompt), input_length=len(prompt), truncate=False, max_output_length=max_new)
    r.details.logprobs = True
    r.details.input_toks = input_toks
    if temperature is not None:
        r.parameters.temperature = temperature
        r.parameters.seed = seed
    return r


class Runner:
    """Drives generate_token the way the servicer does: a request that has all its tokens is pruned.  Keeps every request's
    id and logprob stream and how many tokens each step gave each request; `after` is called with the batch behind every
    step (and prune)."""

    def __init__(self, lm, tok, after=None):
        self.lm, self.tok, self.after = lm, tok, after
        self.ids, self.lps, self.max_new = {}, {}, {}

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
        lm = self.lm
        with lm.context_manager():
            toks, _in, errs, _ns = lm.generate_token(batch, first=first, for_concat=first)
        assert not errs
        got = {}
        for t in toks:
            got[t.request_id] = got.get(t.request_id, 0) + 1
            self.ids[t.request_id].append(t.token_id)
            self.lps[t.request_id].append(t.logprob)
        assert (batch.cu_seqlens[1:] - 1).tolist() == (np.cumsum(batch.input_lengths) - 1).tolist(), "slot contract"
        assert batch.position_ids.tolist() == [n - 1 for n in batch.input_lengths]
        if self.after is not None:
            self.after(batch, got, "prefill" if first else "step")
        done = [r.id for r in batch.requests if len(self.ids[r.id]) >= self.max_new[r.id]]
        if prune and done:
            with lm.context_manager():
                batch = lm.batch_type.prune(batch, done)
            if batch is not None and self.after is not None:
                self.after(batch, None, "prune")
        return batch, got

    def run(self, batch, limit=64):
        batch, _ = self.step(batch, first=True)
        while batch is not None and limit:
            batch, _ = self.step(batch)
            limit -= 1
        assert batch is None
        assert self.lm.kv_cache.free_pages == self.lm.kv_cache.num_pages, "pages leaked"


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


def _fixture_cfg(meta):
    return TinyLlamaConfig(**{k: v for k, v in meta["config"].items() if k in (
        "vocab_size", "hidden_size", "intermediate_size", "num_hidden_layers", "num_attention_heads",
        "num_key_value_heads", "rms_norm_eps", "rope_theta", "max_position_embeddings")})


def _mlp_stats_ok(lm, what):
    st = lm.spec_stats()
    print(f"\n[spec mlp {what}] {st}")
    assert st["verify_steps"] > 0 and st["fallback_no_match"] == 0, st
    assert st["decode_steps"] == st["verify_steps"] + sum(v for k, v in st.items() if k.startswith("fallback_"))
    assert all(len(k) in (2, 3) for k in lm._graphs), "the draft chain is no key of the step graphs"
    assert len(lm.graph_captures) == len(lm._graphs), "the chain's capture is no entry of its own"


# ---- 1. no token changes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["dense", "gptq"])
@pytest.mark.parametrize("scenario", ["equal", "ragged"])
def test_llama_fixture_streams_are_unchanged(gpu_device, random_dir, variant, scenario):
    meta, steps = load_fixture(f"llama_{variant}_{scenario}")
    cfg = _fixture_cfg(meta)
    tensors = tiny_llama_tensors(cfg, seed=meta["seed"], quantize=meta["quantize"], groupsize=meta["groupsize"])
    lm, tok = _llama(tensors, cfg, meta["quantize"], random_dir)
    assert lm.spec_drafter == "mlp" and lm.speculator.K == K
    run = Runner(lm, tok)
    run.run(run.batch([_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts"])]))
    _check_against_fixture(run, *_fixture_streams(steps), LOGIT_TOL, f"{variant}/{scenario}")
    _mlp_stats_ok(lm, f"{variant}/{scenario}")
    assert lm.spec_stats()["emitted"] == sum(len(v) - 1 for v in run.ids.values())


@pytest.mark.parametrize("variant", ["dense", "gptq"])
def test_llama_continuous_batching_fixture_is_unchanged(gpu_device, random_dir, variant):
    """Prefill A, decode x2, prefill B, concatenate, decode x2, prune id 0, decode x2."""
    meta, steps = load_fixture(f"llama_{variant}_continuous")
    cfg = _fixture_cfg(meta)
    tensors = tiny_llama_tensors(cfg, seed=meta["seed"], quantize=meta["quantize"], groupsize=meta["groupsize"])
    lm, tok = _llama(tensors, cfg, meta["quantize"], random_dir)
    run = Runner(lm, tok)
    a = run.batch([_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts_a"])], batch_id=1)
    a, _ = run.step(a, first=True)
    for _ in range(2):
        a, _ = run.step(a)
    b = run.batch([_request(2, meta["prompts_b"][0], meta["max_new"])], batch_id=2)
    b, _ = run.step(b, first=True)
    with lm.context_manager():
        merged = lm.batch_type.concatenate([a, b])
    assert merged.spec_drafts.shape == (3, K) and merged.spec_hidden.shape == (3, E) and merged.spec_model is lm.speculator
    for _ in range(2):
        merged, _ = run.step(merged)
    if any(r.id == 0 for r in merged.requests):
        with lm.context_manager():
            merged = lm.batch_type.prune(merged, [0])
    assert merged.spec_drafts.shape == (len(merged), K) and merged.spec_hidden.shape == (len(merged), E)
    for _ in range(2):
        if merged is not None:
            merged, _ = run.step(merged)
    if merged is not None:
        merged.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    _check_against_fixture(run, *_fixture_streams(steps), LOGIT_TOL, f"{variant}/continuous", whole=False)
    _mlp_stats_ok(lm, f"{variant}/continuous")


def test_santacoder_fixture_stream_is_unchanged(gpu_device, random_dir):
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    meta, steps = load_fixture("bigcode_equal")
    cfg = TinyBigCodeConfig()
    tensors = tiny_bigcode_tensors(cfg, seed=meta["seed"], embed_scale=meta["embed_scale"])
    cfg.quantize = None
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, cfg, torch.float16, None, tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=64, spec_tokens=K,
                       speculator=random_dir)
    run = Runner(lm, tok)
    run.run(run.batch([_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts"])]))
    _check_against_fixture(run, *_fixture_streams(steps), BIGCODE_TOL, "bigcode/equal")
    _mlp_stats_ok(lm, "bigcode/equal")


# ---- 2. the chain is wired right ------------------------------------------------------------------------------------------------
def _forced_prompts():
    rng = np.random.default_rng(FORCED_SEED)
    return [rng.integers(3, 256, size=n).tolist() for n in FORCED_LENS]


def test_the_successor_speculator_drafts_what_it_must(gpu_device, successor_dir):
    """Through a prefill, verify steps, the plain steps at the end of a request (fewer than K + 1 tokens left), a step whose
    chooser samples (the drafts go stale and are made anew when asked for), a concatenate and a prune."""
    lm, tok = _dense(successor_dir)
    seen = []

    def after(batch, got, what):
        batch.spec_hits_host()  # (drafts anew if the step left them stale)
        drafts = batch.spec_drafts.tolist()
        for i, r in enumerate(batch.requests):
            want = ref.successor_drafts(run.ids[r.id][-1], K, V)
            assert drafts[i] == want, f"{what}: request {r.id} behind token {run.ids[r.id][-1]}: {drafts[i]} != {want}"
        assert batch.spec_hits.tolist() == [1] * len(batch)
        seen.append(what)

    run = Runner(lm, tok, after)
    prompts = _forced_prompts()
    a = run.batch([_request(0, prompts[0], 9), _request(1, prompts[1], 20)], batch_id=1)
    a, _ = run.step(a, first=True)
    for _ in range(2):
        a, _ = run.step(a)
    b = run.batch([_request(2, prompts[2], 12, temperature=0.7, seed=5)], batch_id=2)
    b, _ = run.step(b, first=True)
    with lm.context_manager():
        merged = lm.batch_type.concatenate([a, b])
    after(merged, None, "concatenate")
    while merged is not None:
        merged, _ = run.step(merged)  # (request 2 samples: plain steps until it is pruned, then verify steps again)
    st = lm.spec_stats()
    print(f"\n[spec mlp successor] {st} {sorted(set(seen))}")
    assert {"prefill", "step", "prune", "concatenate"} <= set(seen)
    assert st["verify_steps"] > 0 and st["fallback_not_greedy"] > 0 and st["fallback_remaining"] > 0, st
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


# ---- 3. the right hidden row ----------------------------------------------------------------------------------------------------
def _tap_lm_head(lm):
    """Records what goes into lm_head (eager forwards only mean something: a replayed graph calls nothing)."""
    seen, orig = [], lm.model.lm_head

    def tapped(x):
        seen.append(x)
        return orig(x)

    lm.model.lm_head = tapped
    return seen


def _bits(t):
    return t.contiguous().view(torch.int16)


def _latest_graph(lm):
    return next(reversed(lm._graphs.values()))


@pytest.mark.parametrize("mode", ["correct", "mixed", "garbage"])
def test_spec_hidden_is_the_row_behind_the_last_emitted_token(gpu_device, random_dir, mode):
    lm0, tok0 = _dense(None, 0)
    prompts = _forced_prompts()
    plain = Runner(lm0, tok0)
    plain.run(plain.batch([_request(i, p, FORCED_TOKENS) for i, p in enumerate(prompts)]))
    lm, tok = _dense(random_dir)
    fed = _tap_lm_head(lm)
    run = Runner(lm, tok)
    batch = run.batch([_request(i, p, FORCED_TOKENS) for i, p in enumerate(prompts)])
    batch, _ = run.step(batch, first=True)
    assert fed[-1].shape == (3, E) and torch.equal(_bits(batch.spec_hidden), _bits(fed[-1])), "prefill"
    assert run.ids == {i: plain.ids[i][:1] for i in range(3)}
    rng = np.random.default_rng(5)
    before = lm.spec_stats()
    for s in range(4):
        drafts, expect = [], {}
        for r in batch.requests:
            e = len(run.ids[r.id])
            d = list(plain.ids[r.id][e:e + K])
            j = {"correct": K, "garbage": 0}.get(mode, int(rng.integers(0, K + 1)))
            if j < K:
                d[j] = (d[j] + 1) % 256
            drafts.append(d)
            expect[r.id] = j + 1
        batch.spec_drafts = torch.tensor(drafts, dtype=torch.int64, device=lm.device)
        batch.spec_hits = torch.ones(len(drafts), dtype=torch.int32, device=lm.device)
        batch, got = run.step(batch)
        assert got == expect, f"{mode} step {s}: tokens per request {got}, expected {expect}"
        g = _latest_graph(lm)
        assert g.K == K and g.hidden.shape == (g.rows * (K + 1), E)
        for b, r in enumerate(batch.requests):
            row = b * (K + 1) + got[r.id] - 1
            assert torch.equal(_bits(batch.spec_hidden[b]), _bits(g.hidden[row])), f"{mode} step {s} request {r.id}"
    after = lm.spec_stats()
    assert after["verify_steps"] - before["verify_steps"] == 4
    while batch is not None:
        was = batch
        batch, got = run.step(batch, prune=False)
        g = _latest_graph(lm)
        rows = [b * (g.K + 1) + got[r.id] - 1 for b, r in enumerate(was.requests)]
        assert torch.equal(_bits(was.spec_hidden), _bits(g.hidden[rows])), "a step behind the forced ones"
        done = [r.id for r in was.requests if len(run.ids[r.id]) >= FORCED_TOKENS]
        with lm.context_manager():
            batch = lm.batch_type.prune(was, done)
    assert lm.spec_stats()["fallback_remaining"] > 0, "no plain step ran"
    for rid, want in plain.ids.items():
        assert run.ids[rid] == want, f"{mode}: request {rid} {run.ids[rid]} != plain run {want}"


def test_spec_hidden_behind_prefills_of_every_kind_and_a_sampling_step(gpu_device, random_dir):
    lm, tok = _dense(random_dir, reuse=True)
    fed = _tap_lm_head(lm)
    run = Runner(lm, tok)
    rng = np.random.default_rng(9)
    shared = rng.integers(3, 256, size=40).tolist()
    # every prompt position goes through lm_head (details.input_toks): the rows behind the prompts' last tokens are picked
    lens = [7, 33]
    batch = run.batch([_request(i, rng.integers(3, 256, size=n).tolist(), 4, input_toks=True) for i, n in enumerate(lens)])
    batch, _ = run.step(batch, first=True)
    assert fed[-1].shape == (sum(lens), E)
    assert torch.equal(_bits(batch.spec_hidden), _bits(fed[-1][[lens[0] - 1, sum(lens) - 1]])), "input_toks prefill"
    batch.release()
    # behind a reused prefix: the second batch prefills only what follows the shared page
    first = run.batch([_request(10, shared + [5, 6, 7], 4)], batch_id=1)
    first, _ = run.step(first, first=True)
    second = run.batch([_request(11, shared + [9, 8], 6, temperature=0.8, seed=3), _request(12, shared[:35], 6)], batch_id=2)
    second, _ = run.step(second, first=True)
    assert second.reused_lengths == [32, 32] and fed[-1].shape == (2, E)
    assert torch.equal(_bits(second.spec_hidden), _bits(fed[-1])), "suffix prefill"
    # request 11 samples: the plain step of the general chooser keeps the state too
    second, _ = run.step(second)
    g = _latest_graph(lm)
    assert g.K == 0 and lm.spec_stats()["fallback_not_greedy"] == 1
    assert torch.equal(_bits(second.spec_hidden), _bits(g.hidden[:2])), "sampling step"
    first.release()
    second.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


# ---- 4. drafts equal the specification ------------------------------------------------------------------------------------------
def _collect_drafts(lm, tok, prompts, tokens):
    """[(spec_hidden, latest ids, spec_drafts)] on the host, behind every step of one run."""
    out = []

    def after(batch, got, what):
        if what != "prune":
            out.append((batch.spec_hidden.double().cpu().numpy(), [run.ids[r.id][-1] for r in batch.requests],
                        batch.spec_drafts.cpu().numpy()))

    run = Runner(lm, tok, after)
    run.run(run.batch([_request(i, p, tokens) for i, p in enumerate(prompts)]))
    return out, run


def test_drafts_equal_the_specification(gpu_device, tmp_path_factory):
    spec = ref.make_random(E, WIDE_INNER, V, 3, seed=WIDE_SEED, head_std=WIDE_HEAD_STD)
    lm, tok = _dense(_spec_dir(tmp_path_factory, spec, "wide"))
    rng = np.random.default_rng(21)
    prompts = [rng.integers(3, 256, size=n).tolist() for n in (27, 5, 30, 12)]
    steps, _ = _collect_drafts(lm, tok, prompts, 16)
    pairs = undecided = 0
    for s, (hidden, latest, drafts) in enumerate(steps):
        want, margins = spec.draft(hidden, latest, K)
        for b in range(len(latest)):
            pairs += 1
            if margins[b].min() < LOGIT_TOL:
                undecided += 1
                continue
            assert drafts[b].tolist() == want[b].tolist(), (
                f"step {s} request row {b}: drafts {drafts[b].tolist()} != specification {want[b].tolist()} "
                f"(margins {margins[b].round(2).tolist()})")
    print(f"\n[spec mlp specification] {pairs} (request, step) pairs, {undecided} under {LOGIT_TOL} logits")
    assert pairs >= 30 and undecided <= UNDECIDED_SHARE * pairs


# ---- 5. captured == eager -------------------------------------------------------------------------------------------------------
def test_the_captured_chain_equals_the_eager_chain(gpu_device, random_dir):
    lm, tok = _dense(random_dir)
    assert lm.use_graphs
    prompts = _forced_prompts()
    captured, run_c = _collect_drafts(lm, tok, prompts, 12)
    chains = [g.chain for g in lm._graphs.values() if g.chain is not None and g.chain.graph is not None]
    assert chains, "no draft chain was captured"
    assert len(lm.graph_captures) == len(lm._graphs)
    lm.use_graphs = False
    try:
        eager, run_e = _collect_drafts(lm, tok, prompts, 12)
    finally:
        lm.use_graphs = True
    assert run_c.ids == run_e.ids and len(captured) == len(eager)
    for s, (a, b) in enumerate(zip(captured, eager)):
        assert np.array_equal(a[0], b[0]), f"step {s}: spec_hidden differs"
        assert np.array_equal(a[2], b[2]), f"step {s}: drafts differ: {a[2].tolist()} != {b[2].tolist()}"


# ---- 6. the e4m3 cache ----------------------------------------------------------------------------------------------------------
def test_the_mlp_drafter_on_the_e4m3_cache_matches_its_plain_run(gpu_device, random_dir):
    lm0, tok0 = _dense(None, 0, kv="fp8_e4m3")
    lm, tok = _dense(random_dir, kv="fp8_e4m3")
    assert lm.kv_cache.is_fp8
    prompts = _forced_prompts()
    plain, run = Runner(lm0, tok0), Runner(lm, tok)
    plain.run(plain.batch([_request(i, p, FORCED_TOKENS) for i, p in enumerate(prompts)]))
    run.run(run.batch([_request(i, p, FORCED_TOKENS) for i, p in enumerate(prompts)]))
    assert run.ids == plain.ids
    for rid in run.lps:
        np.testing.assert_allclose(run.lps[rid], plain.lps[rid], atol=LOGIT_TOL)
    _mlp_stats_ok(lm, "e4m3")


# ---- 7. refusals and the loaded speculator --------------------------------------------------------------------------------------
def test_construction_refusals_on_the_product_path(gpu_device, random_dir, tmp_path_factory):
    with pytest.raises(ValueError, match=r"spec_tokens.*speculator.*n_predict = 3"):
        _dense(random_dir, 4)
    with pytest.raises(ValueError, match=r"speculator.*spec_tokens"):
        _dense(random_dir, 0)
    narrow = _spec_dir(tmp_path_factory, ref.make_random(64, 64, V, 3, seed=1), "narrow")
    with pytest.raises(ValueError, match="emb_dim 64 != the base model's hidden size 256"):
        _dense(narrow)
    vocab = _spec_dir(tmp_path_factory, ref.make_random(E, 64, 128, 3, seed=1), "vocab")
    with pytest.raises(ValueError, match="vocab_size 128 != the base model's vocab_size 256"):
        _dense(vocab)
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyLlamaConfig()
    eng = InferenceEngine(tiny_llama_tensors(cfg, seed=7), LlamaConfig(**cfg.to_dict()), torch.float16, None,
                          tokenizer=FixtureTokenizer(V))
    eng.world_size = 2
    with pytest.raises(NotImplementedError, match="tensor parallelism is out of scope"):
        FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=16, spec_tokens=K,
                      speculator=random_dir)


def test_defaults_and_tied_weights_on_the_device(gpu_device, tmp_path_factory, monkeypatch):
    monkeypatch.delenv("TGIS_SPECULATOR", raising=False)
    lm, _ = _dense(None, K)
    assert lm.spec_drafter == "lookup" and lm.speculator is None
    tied = ref.make_random(E, 64, V, 4, seed=2, tie_weights=True, scale=True)
    path = ref.write_checkpoint(str(tmp_path_factory.mktemp("tied")), tied, prefix="speculator.", store_tied_once=True)
    monkeypatch.setenv("TGIS_SPECULATOR", path)
    lm, tok = _dense(None, 4)  # the environment names the speculator
    assert lm.spec_drafter == "mlp" and lm.speculator.cfg.scale_input
    h = lm.speculator.heads
    assert len(h) == 4 and all(x.emb is h[0].emb and x.head is h[0].head and x.ln_weight is h[0].ln_weight for x in h)
    assert h[1].proj is h[2].proj is h[3].proj and h[0].proj is not h[1].proj
    # and it drafts what the specification drafts, scale_input and K = 4 included
    rng = np.random.default_rng(3)
    steps, _ = _collect_drafts(lm, tok, [rng.integers(3, 256, size=n).tolist() for n in (9, 20)], 8)
    agree = total = 0
    for hidden, latest, drafts in steps:
        want, margins = tied.draft(hidden, latest, 4)
        for b in range(len(latest)):
            if margins[b].min() >= LOGIT_TOL:
                total += 1
                agree += drafts[b].tolist() == want[b].tolist()
    assert total >= 4 and agree == total, (agree, total)
