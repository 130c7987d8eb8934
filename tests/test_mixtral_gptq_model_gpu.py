"""-m gpu: a GPTQ Mixtral checkpoint (4 bits, group size 64: q/k/v/o and every expert's w1 / w3 / w2; router, norms, embeddings
and head in f16) end to end on the flash path against transformers' fp32 CPU MixtralForCausalLM on the dequantised weights
(tests/golden/mixtral_gptq_top2.npz, made by tests/golden/make_mixtral_gptq_fixtures.py on the seeded tiny checkpoint of
tests/mixtral_gptq_tiny.py).  Prompts of 5, 20 and 33 tokens in one batch: the prefill routes 58 tokens through the int4 expert
kernels and every decode step three, as slabs that the next add + RMSNorm sums.

The fixture's seed was searched until every top-2 logit margin exceeds twice LOGIT_TOL and every router's 2nd-to-3rd logit gap
exceeds 8 times what a float16 run moves a router logit, so exact ids and exact routing are fair demands."""
import json
import os
import time
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fixture_utils import GOLDEN, FixtureTokenizer
from tests.mixtral_gptq_tiny import GS, TinyMixtralConfig, tiny_mixtral_gptq_tensors
from tests.test_mixtral_model_gpu import LOGIT_TOL, _check, _free_port, _RouteTap, _run

pytestmark = pytest.mark.gpu

TP_TIME_LIMIT = 240.0  # seconds for the two ranks of test_tp2_matches_the_fixture, from spawn to join


def _fixture():
    z = np.load(os.path.join(GOLDEN, "mixtral_gptq_top2.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, z["ids"], z["logits"], [z[f"router_idx_{i}"] for i in range(len(meta["prompts"]))]


def _build(meta, use_graphs=True, **kw):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyMixtralConfig()
    config = types.SimpleNamespace(model_type="mixtral", **cfg.to_dict())
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tiny_mixtral_gptq_tensors(cfg, meta["seed"]), config, torch.float16, "gptq", tokenizer=tok,
                          gptq_groupsize=GS)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, "gptq", engine=eng, kv_cache_pages=64, **kw)
    lm.use_graphs = use_graphs
    return lm, tok


def test_gptq_mixtral_matches_transformers_graph_and_eager(gpu_device, monkeypatch):
    """Every id equals the fixture's and every logit is within LOGIT_TOL, with graphs and eager; the captured decode graph
    reproduces the eager steps bit for bit; the prefill routes every token as transformers did; the experts are int4 images."""
    from tgis_amd import native
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import FlashMixtralForCausalLM

    monkeypatch.delenv("TGIS_MOE_PATH", raising=False)
    meta, ids, logits, router_idx = _fixture()
    steps = ids.shape[1]
    runs = {}
    for use_graphs in (True, False):
        lm, tok = _build(meta, use_graphs=use_graphs)
        assert isinstance(lm.model, FlashMixtralForCausalLM)
        experts = lm.model.model.layers[0].moe.experts
        assert isinstance(experts.gate_up, native.MoeGptqWeights) and isinstance(experts.down, native.MoeGptqWeights)
        assert (experts.gate_up.groups, experts.down.groups) == (256 // GS, 512 // GS)
        tap = _RouteTap(monkeypatch) if not use_graphs else None
        runs[use_graphs] = _run(lm, tok, meta, steps)
        if use_graphs:
            assert steps == 1 or (lm._graphs and all(g.graph is not None for g in lm._graphs.values()))
        else:
            want = [np.concatenate([r[layer, :len(p)] for r, p in zip(router_idx, meta["prompts"])]) for layer in range(2)]
            for layer in range(2):
                assert np.array_equal(tap.calls[layer].expert_ids.cpu().numpy(), want[layer]), f"layer {layer} routing"
        worst = _check(runs[use_graphs], ids, logits, f"gptq graphs={use_graphs}")
        print(f"gptq graphs={use_graphs}: max |logit - reference| over {steps} steps = {worst:.4f}")
    for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
        assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"


def test_the_loop_path_gives_the_same_tokens(gpu_device, monkeypatch):
    """TGIS_MOE_PATH=loop (eager forwards): gptq_gemm(act=2) and gptq_gemm on the experts' views, no routed launch."""
    from tgis_amd import native

    meta, ids, logits, _ = _fixture()
    monkeypatch.setenv("TGIS_MOE_PATH", "loop")
    calls = {"up": 0}
    real_up = native.moe_gptq_gemm_up
    monkeypatch.setattr(native, "moe_gptq_gemm_up",
                        lambda *a, **kw: (calls.__setitem__("up", calls["up"] + 1), real_up(*a, **kw))[1])
    lm, tok = _build(meta, use_graphs=False)
    _check(_run(lm, tok, meta, ids.shape[1]), ids, logits, "gptq loop")
    assert calls["up"] == 0, "the forced loop path launched the routed kernels"


def _tp_worker(rank, world, port, seed, prompts, max_new, steps, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1")
    os.environ.pop("TGIS_MOE_PATH", None)
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    lm, tok = _build({"seed": seed})
    assert lm.tp_world == world
    assert lm.model.model.layers[0].moe.experts.down.K == 512 // world
    ret[rank] = _run(lm, tok, {"prompts": prompts, "max_new": max_new}, steps)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_matches_the_fixture(gpu_device):
    """Two ranks on one device: every expert's w1 | w3 split by columns and w2 by rows of the int4 matrices, the router
    replicated; ids are the fixture's, logits within LOGIT_TOL, both ranks hold the same logits."""
    meta, ids, logits, _ = _fixture()
    steps = ids.shape[1]
    mgr = mp.get_context("spawn").Manager()
    ret = mgr.dict()
    keys = ("OMP_NUM_THREADS", "MKL_NUM_THREADS")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ[k] = str(max(1, min(8, (os.cpu_count() or 8) // 2)))
    try:
        ctx = mp.spawn(_tp_worker, args=(2, _free_port(), meta["seed"], meta["prompts"], meta["max_new"], steps, ret),
                       nprocs=2, join=False)
        deadline = time.monotonic() + TP_TIME_LIMIT
        while not ctx.join(timeout=2.0):
            if time.monotonic() > deadline:
                for p in ctx.processes:
                    p.kill()
                pytest.fail(f"the two ranks did not finish within {TP_TIME_LIMIT:.0f} s")
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for (i0, l0), (i1, l1) in zip(ret[0], ret[1]):
        assert i0 == i1 and np.array_equal(l0, l1), "ranks must hold identical logits"
    _check(ret[0], ids, logits, "gptq tp2")
