"""-m gpu: a Mistral checkpoint (model_type "mistral", sliding_window 40) end to end on the flash path against transformers'
fp32 CPU MistralForCausalLM (tests/golden/mistral_window.npz, made by tests/golden/make_mistral_fixtures.py on the seeded tiny
checkpoint of tests/mistral_tiny.py): prompts of 7, 45 and 100 tokens in one batch, 50 greedy tokens each, so the prefill runs
the windowed prefill form, every decode step the windowed decode form, and the short request crosses the window and a page
edge while it decodes.

test_mistral_at_a_window_of_1000_keys runs the same checkpoint at a window of 31 pages (prompts of 7, 990 and 1100 tokens):
there the waves of the windowed decode form walk several pages each, its key splits are live in the captured graphs and the
prefill takes most pages mask-free; the reference is the windowed fp32 oracle of test_mistral_over_the_e4m3_cache."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests.fixture_utils import GOLDEN, FixtureTokenizer
from tests.mistral_tiny import TinyMistralConfig, tiny_mistral_tensors
from tests.test_neox_model_gpu import _from_pb, _LogitTap, _pb, _step

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35       # tests/test_model_gpu.py's f16 bar; the fixture's margins are more than twice that: ids are exact
KV_FP8_LOGIT_TOL = 1.4  # tests/test_kv_fp8_model_gpu.py's f16 bar


def _fixture():
    z = np.load(os.path.join(GOLDEN, "mistral_window.npz"))
    return json.loads(bytes(z["meta"]).decode()), z["ids"], z["logits"]


def _build(meta, sliding_window=40, model_type="mistral", use_graphs=True, max_position_embeddings=512, kv_cache_pages=64,
           **kw):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyMistralConfig(sliding_window=sliding_window, max_position_embeddings=max_position_embeddings)
    if model_type == "mistral":  # what a Mistral config.json carries: no bias fields
        config = types.SimpleNamespace(model_type="mistral", **cfg.to_dict())
    else:
        fields = cfg.to_dict()
        fields.pop("sliding_window")
        config = LlamaConfig(**fields)
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tiny_mistral_tensors(cfg, meta["seed"]), config, torch.float16, None, tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=kv_cache_pages, **kw)
    lm.use_graphs = use_graphs
    return lm, tok


def _run(lm, tok, meta, steps):
    """[(ids [3], logits [3, vocab])] of the prefill and steps - 1 decode steps of the fixture's batch."""
    tap = _LogitTap(lm)
    batch = _from_pb(lm, tok, _pb(meta["prompts"], meta["max_new"]))
    got = []
    for i in range(steps):
        toks, logits = _step(lm, batch, tap, first=(i == 0))
        assert [t.request_id for t in toks] == [0, 1, 2]
        got.append(([t.token_id for t in toks], logits))
    return got


def test_mistral_matches_transformers_graph_and_eager(gpu_device):
    """f16: every id equals the fixture's and every logit is within the Llama fixtures' bar; the captured windowed decode graph
    reproduces the eager steps bit for bit."""
    meta, ids, logits = _fixture()
    steps = ids.shape[1]
    runs = {}
    for use_graphs in (True, False):
        lm, tok = _build(meta, use_graphs=use_graphs)
        assert lm.sliding_window == 40
        got = runs[use_graphs] = _run(lm, tok, meta, steps)
        if use_graphs:
            assert lm._graphs and all(g.window == 40 and g.max_ctx > 40 for g in lm._graphs.values())
        worst = 0.0
        for i, (got_ids, got_logits) in enumerate(got):
            err = float(np.abs(got_logits - logits[:, i]).max())
            worst = max(worst, err)
            assert got_ids == ids[:, i].tolist(), f"graphs={use_graphs} step {i}: ids {got_ids} != {ids[:, i].tolist()}"
            assert err <= LOGIT_TOL, f"graphs={use_graphs} step {i}: max |logit - reference| = {err:.3f} > {LOGIT_TOL}"
        print(f"graphs={use_graphs}: max |logit - reference| over {steps} steps = {worst:.4f}")
    for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
        assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"


def test_the_window_is_what_makes_it_match(gpu_device):
    """The same weights without the window leave the fixture once a request is past 40 tokens: the prefill of the 45- and the
    100-token prompts already does (the feature's test: it fails on a build that ignores sliding_window)."""
    meta, ids, logits = _fixture()
    lm, tok = _build(meta, sliding_window=None)
    _got_ids, got_logits = _run(lm, tok, meta, 1)[0]
    err = np.abs(got_logits - logits[:, 0]).max(axis=1)
    assert err[0] <= LOGIT_TOL and err[1] > LOGIT_TOL and err[2] > LOGIT_TOL, err


def test_window_off_equals_the_llama_path(gpu_device):
    """model_type "mistral" with sliding_window null makes Llama's launches: logits bit for bit, prefill and decode."""
    meta, _ids, _logits = _fixture()
    runs = []
    for model_type in ("mistral", "llama"):
        lm, tok = _build(meta, sliding_window=None, model_type=model_type)
        assert lm.sliding_window is None
        runs.append(_run(lm, tok, meta, 8))
        assert all(g.window is None for g in lm._graphs.values())
    for i, ((im, lm_), (il, ll)) in enumerate(zip(*runs)):
        assert im == il and np.array_equal(lm_, ll), f"step {i}: mistral without a window and llama differ"


def test_mistral_over_the_e4m3_cache(gpu_device, monkeypatch):
    """kv_cache_dtype fp8_e4m3 through the windowed launches, within the KV-fp8 model test's f16 bar of that test's kind of
    reference: the project's fp32 Llama oracle (oracle/llama_ref.py) fed the model's own ids, its attention replaced by the
    windowed restatement (tests/attn_window_ref.py) over K / V rounded to f16, quantised to e4m3 and dequantised with scales 1,
    which is what the one-byte cache hands the kernels.  The same oracle without the quantisation is first held against the
    transformers fixture, so it is the fixture's model."""
    import attn_window_ref
    import kv_fp8_ref as q8
    from oracle import ops_ref
    from oracle.llama_ref import LlamaRef

    meta, ids, logits = _fixture()
    cfg = TinyMistralConfig()
    quantise = [False]

    def windowed(q, k, v, cu_q, cu_k, scale):
        assert list(cu_q) == [0, q.shape[0]] and list(cu_k) == [0, k.shape[0]]  # one sequence per call
        if quantise[0]:
            k = q8.dequantize(q8.quantize(k.to(torch.float16)))
            v = q8.dequantize(q8.quantize(v.to(torch.float16)))
        return attn_window_ref.window_attention(q, k, v, cfg.sliding_window, scale).float()

    monkeypatch.setattr(ops_ref, "attention_varlen", windowed)
    ref = LlamaRef(cfg, tiny_mistral_tensors(cfg, meta["seed"]))
    steps = ids.shape[1]
    forced = [ids[:, i].tolist() for i in range(steps)]
    for i, w in enumerate(ref.generate_greedy(meta["prompts"], steps, forced=forced)):
        err = float(np.abs(w["logits"].numpy() - logits[:, i]).max())
        assert err <= 1e-2, f"step {i}: the windowed oracle is {err:.4f} from the transformers fixture"

    lm, tok = _build(meta, kv_cache_dtype="fp8_e4m3")
    assert lm.kv_cache.is_fp8
    got = _run(lm, tok, meta, ids.shape[1])
    quantise[0] = True
    want = ref.generate_greedy(meta["prompts"], len(got), forced=[g[0] for g in got])
    worst = 0.0
    for i, ((_ids, got_logits), w) in enumerate(zip(got, want)):
        err = float(np.abs(got_logits - w["logits"].numpy()).max())
        worst = max(worst, err)
        assert err <= KV_FP8_LOGIT_TOL, f"step {i}: max |logit - quantised-KV oracle| = {err:.3f} > {KV_FP8_LOGIT_TOL}"
    print(f"e4m3 cache: max |logit - quantised-KV oracle| over {len(got)} steps = {worst:.4f}")


WIDE_WINDOW = 1000            # 31 pages and a bit: a step sees up to 33 pages, 8 or 9 per wave when the launch is not split
WIDE_PROMPT_LENS = (7, 990, 1100)  # below the window; crossing it while it decodes; beyond it, so that the prefill is windowed
WIDE_STEPS = 40
WIDE_BUILD = dict(max_position_embeddings=2048, kv_cache_pages=128)  # 2 + 33 + 36 pages are in use at the last step


def test_mistral_at_a_window_of_1000_keys(gpu_device, monkeypatch):
    """sliding_window 1000: every captured decode graph is a windowed one with the key splits the rule gives its W + 31 keys
    (more than one), graph and eager runs agree bit for bit, every logit is within the f16 bar of the windowed fp32 oracle fed
    the model's own ids, every id is the oracle's argmax wherever the oracle's top-2 margin exceeds twice the bar, and the
    same weights without a window leave the oracle at the 1100-token prompt's prefill.  The oracle is LlamaRef with its attention
    replaced by tests/attn_window_ref.py at this W: test_mistral_over_the_e4m3_cache holds it to 1e-2 of the transformers
    fixture at W 40, and the width is a parameter of the same restatement."""
    import attn_window_ref
    from oracle import ops_ref
    from oracle.llama_ref import LlamaRef
    from tgis_amd import native

    seed = _fixture()[0]["seed"]
    rng = np.random.default_rng(WIDE_WINDOW)
    meta = {"seed": seed, "prompts": [rng.integers(3, 256, size=n).tolist() for n in WIDE_PROMPT_LENS], "max_new": WIDE_STEPS}
    cfg = TinyMistralConfig(sliding_window=WIDE_WINDOW, max_position_embeddings=WIDE_BUILD["max_position_embeddings"])

    runs = {}
    for use_graphs in (True, False):
        lm, tok = _build(meta, sliding_window=WIDE_WINDOW, use_graphs=use_graphs, **WIDE_BUILD)
        assert lm.sliding_window == WIDE_WINDOW
        runs[use_graphs] = _run(lm, tok, meta, WIDE_STEPS)
        if use_graphs:
            assert lm._graphs
            for g in lm._graphs.values():
                assert g.graph is not None and g.window == WIDE_WINDOW and g.max_ctx > WIDE_WINDOW
                rule = native.attn_num_splits(g.rows, lm.num_kv_heads, lm.num_heads, 1, min(g.max_ctx, WIDE_WINDOW + 31))
                assert g.num_splits == rule > 1, (g.rows, g.max_ctx, g.num_splits, rule)
    for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
        assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"

    def windowed(q, k, v, cu_q, cu_k, scale):
        assert list(cu_q) == [0, q.shape[0]] and list(cu_k) == [0, k.shape[0]]  # one sequence per call
        return attn_window_ref.window_attention(q, k, v, WIDE_WINDOW, scale).float()

    monkeypatch.setattr(ops_ref, "attention_varlen", windowed)
    ref = LlamaRef(cfg, tiny_mistral_tensors(cfg, seed))
    got = runs[True]
    want = ref.generate_greedy(meta["prompts"], WIDE_STEPS, forced=[ids for ids, _ in got])
    worst, decided = 0.0, 0
    for i, ((got_ids, got_logits), w) in enumerate(zip(got, want)):
        wl = w["logits"].numpy()
        err = float(np.abs(got_logits - wl).max())
        worst = max(worst, err)
        top2 = np.sort(wl, axis=1)[:, -2:]
        for r in range(len(got_ids)):
            if top2[r, 1] - top2[r, 0] > 2 * LOGIT_TOL:
                decided += 1
                assert got_ids[r] == int(wl[r].argmax()), f"step {i} request {r}: id {got_ids[r]} != oracle {int(wl[r].argmax())}"
        assert err <= LOGIT_TOL, f"step {i}: max |logit - windowed oracle| = {err:.3f} > {LOGIT_TOL}"
    print(f"W {WIDE_WINDOW}: max |logit - windowed oracle| over {WIDE_STEPS} steps = {worst:.4f}; {decided} of "
          f"{3 * WIDE_STEPS} ids decided by a margin above {2 * LOGIT_TOL}")
    assert decided >= 2 * WIDE_STEPS  # (the head is scaled so that margins sit far above the bar: most ids are checked)

    # the feature check at this width: without the window the 1100-token prompt's prefill is another model's
    lm, tok = _build(meta, sliding_window=None, **WIDE_BUILD)
    _ids, causal_logits = _run(lm, tok, meta, 1)[0]
    err = np.abs(causal_logits - want[0]["logits"].numpy()).max(axis=1)
    assert err[0] <= LOGIT_TOL and err[1] <= LOGIT_TOL and err[2] > LOGIT_TOL, err
