"""-m gpu: Qwen3-MoE checkpoints (model_type "qwen3_moe") end to end on the flash path against transformers' fp32 CPU
Qwen3MoeForCausalLM (tests/golden/qwen3_moe_tiny.npz, made by tests/golden/make_qwen3_moe_fixtures.py on the seeded tiny
checkpoints of tests/qwen3_moe_tiny.py).  "e128": 128 experts, top-8, renormalised; prompts of 5, 20 and 33 tokens in one batch
with the routed block cut into chunks of 55 tokens, so the prefill's 58 tokens cross the chunk and the small-T rule (55
through the tile kernel, 3 through the slab kernel body) and every decode step routes three.  "nonorm": 16 experts, top-4, norm_topk_prob
false.  Every top-2 margin of the fixture exceeds twice LOGIT_TOL, so exact ids are a fair demand of an f16 run."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.fixture_utils import GOLDEN, FixtureTokenizer
from tests.qwen3_moe_tiny import TinyQwen3MoeConfig, tiny_qwen3_moe_tensors
from tests.test_neox_model_gpu import _from_pb, _LogitTap, _pb, _step

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35  # tests/test_mixtral_model_gpu.py's bar against its fixture
CHUNK = 55


def _fixture(kind):
    z = np.load(os.path.join(GOLDEN, "qwen3_moe_tiny.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta["seed"], meta["runs"][kind], z[f"ids_{kind}"], z[f"logits_{kind}"]


def _build(kind, seed, use_graphs):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyQwen3MoeConfig(kind)
    config = types.SimpleNamespace(**cfg.to_dict(), model_type="qwen3_moe")
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tiny_qwen3_moe_tensors(cfg, seed), config, torch.float16, None, tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=64)
    lm.use_graphs = use_graphs
    return lm, tok


@pytest.mark.parametrize("kind", ("e128", "nonorm"))
def test_qwen3_moe_matches_transformers_graph_and_eager(gpu_device, monkeypatch, kind):
    from tgis_amd import native
    from tgis_amd.models.custom_modeling import flash_qwen3_moe_modeling as fq

    monkeypatch.setattr(fq, "MOE_CHUNK_TOKENS", CHUNK)
    routed = []
    real = native.moe_route_tiles
    monkeypatch.setattr(native, "moe_route_tiles", lambda logits, *a, **kw: routed.append(logits.shape[0]) or real(logits, *a, **kw))
    seed, run, ids, logits = _fixture(kind)
    steps, runs = ids.shape[1], {}
    for use_graphs in (True, False):
        lm, tok = _build(kind, seed, use_graphs)
        assert isinstance(lm.model, fq.FlashQwen3MoeForCausalLM) and lm.sliding_window is None
        tap = _LogitTap(lm)
        batch = _from_pb(lm, tok, _pb(run["prompts"], run["max_new"]))
        got = runs[use_graphs] = []
        for i in range(steps):
            toks, step_logits = _step(lm, batch, tap, first=(i == 0))
            got.append(([t.token_id for t in toks], step_logits))
            err = float(np.abs(step_logits - logits[:, i]).max())
            print(f"{kind} graphs={use_graphs} step {i}: max |logit - reference| = {err:.4f}")
            assert got[-1][0] == ids[:, i].tolist(), f"graphs={use_graphs} step {i}: ids {got[-1][0]} != {ids[:, i].tolist()}"
            assert err <= LOGIT_TOL, f"graphs={use_graphs} step {i}: max |logit - reference| = {err:.3f} > {LOGIT_TOL}"
        assert not use_graphs or lm._graphs
    for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
        assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"
    if kind == "e128":  # the prefill crossed the chunk, and its two passes sit on either side of the small-T rule
        assert routed[:4] == [CHUNK, 58 - CHUNK, CHUNK, 58 - CHUNK], routed[:4]
        assert not native.moe_tile_plan(0, CHUNK, 64, 64, 128, 8)["slab_body"]
        assert native.moe_tile_plan(0, 58 - CHUNK, 64, 64, 128, 8)["slab_body"]
