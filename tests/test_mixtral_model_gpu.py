"""-m gpu: a Mixtral checkpoint (model_type "mixtral", 8 experts, top-2) end to end on the flash path against transformers'
fp32 CPU MixtralForCausalLM (tests/golden/mixtral_top2.npz, made by tests/golden/make_mixtral_fixtures.py on the seeded tiny
checkpoint of tests/mixtral_tiny.py): prompts of 5, 20 and 33 tokens in one batch, so the prefill routes 58 tokens through
the expert kernels and every decode step three, each time as slabs that the next add + RMSNorm sums.

The fixture's seed was searched until every top-2 logit margin exceeds twice LOGIT_TOL and every router's 2nd-to-3rd logit
gap exceeds 8 times what a float16 run moves a router logit (meta: router_margin), so exact ids and exact routing are fair
demands of an f16 run."""
import json
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fixture_utils import GOLDEN, FixtureTokenizer
from tests.mixtral_tiny import TinyMixtralConfig, tiny_mixtral_tensors
from tests.test_neox_model_gpu import _from_pb, _LogitTap, _pb, _step

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35  # tests/test_model_gpu.py's f16 bar; the fixture's margins are more than twice that: ids are exact


def _fixture():
    z = np.load(os.path.join(GOLDEN, "mixtral_top2.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, z["ids"], z["logits"], [z[f"router_idx_{i}"] for i in range(len(meta["prompts"]))]


def _build(meta, use_graphs=True, **kw):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyMixtralConfig()
    config = types.SimpleNamespace(model_type="mixtral", **cfg.to_dict())
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tiny_mixtral_tensors(cfg, meta["seed"]), config, torch.float16, None, tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=64, **kw)
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


def _check(got, ids, logits, what):
    worst = 0.0
    for i, (got_ids, got_logits) in enumerate(got):
        err = float(np.abs(got_logits - logits[:, i]).max())
        worst = max(worst, err)
        print(f"{what} step {i}: max |logit - reference| = {err:.4f}")
        assert got_ids == ids[:, i].tolist(), f"{what} step {i}: ids {got_ids} != {ids[:, i].tolist()}"
        assert err <= LOGIT_TOL, f"{what} step {i}: max |logit - reference| = {err:.3f} > {LOGIT_TOL}"
    return worst


class _RouteTap:
    """Records the expert ids of every native.moe_route call (layer by layer, forward by forward)."""

    def __init__(self, monkeypatch, rewrite=None):
        from tgis_amd import native

        self.calls = []
        real = native.moe_route

        def tapped(logits, top_k):
            if rewrite is not None:
                logits = rewrite(logits)
            r = real(logits, top_k)
            self.calls.append(r)
            return r

        monkeypatch.setattr(native, "moe_route", tapped)


def test_mixtral_matches_transformers_graph_and_eager(gpu_device, monkeypatch):
    """f16: every id equals the fixture's and every logit is within the Llama fixtures' bar, with graphs and eager; the
    captured decode graph reproduces the eager steps bit for bit; the prefill routes every token as transformers did."""
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import FlashMixtralForCausalLM

    monkeypatch.delenv("TGIS_MOE_PATH", raising=False)
    meta, ids, logits, router_idx = _fixture()
    steps = ids.shape[1]
    runs = {}
    for use_graphs in (True, False):
        lm, tok = _build(meta, use_graphs=use_graphs)
        assert isinstance(lm.model, FlashMixtralForCausalLM) and lm.sliding_window is None
        tap = _RouteTap(monkeypatch) if not use_graphs else None
        runs[use_graphs] = _run(lm, tok, meta, steps)
        if use_graphs:
            assert steps == 1 or (lm._graphs and all(g.graph is not None for g in lm._graphs.values()))
        else:
            # the prefill's routing, layer by layer: the prompts' tokens in batch order
            want = [np.concatenate([r[layer, :len(p)] for r, p in zip(router_idx, meta["prompts"])]) for layer in range(2)]
            for layer in range(2):
                assert np.array_equal(tap.calls[layer].expert_ids.cpu().numpy(), want[layer]), f"layer {layer} routing"
        worst = _check(runs[use_graphs], ids, logits, f"graphs={use_graphs}")
        print(f"graphs={use_graphs}: max |logit - reference| over {steps} steps = {worst:.4f}")
    for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
        assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"


def test_the_loop_path_gives_the_same_tokens(gpu_device, monkeypatch):
    """TGIS_MOE_PATH=loop (eager forwards): one host read of the counts, the dense GEMMs per expert that was hit."""
    from tgis_amd import native

    meta, ids, logits, _ = _fixture()
    monkeypatch.setenv("TGIS_MOE_PATH", "loop")
    calls = {"up": 0}
    real_up = native.moe_gemm_up
    monkeypatch.setattr(native, "moe_gemm_up", lambda *a, **kw: (calls.__setitem__("up", calls["up"] + 1), real_up(*a, **kw))[1])
    lm, tok = _build(meta, use_graphs=False)
    _check(_run(lm, tok, meta, ids.shape[1]), ids, logits, "loop")
    assert calls["up"] == 0, "the forced loop path launched the routed kernels"


def test_routing_is_what_makes_it_match(gpu_device, monkeypatch):
    """The feature's test: the same weights with every token sent to experts 0 and 1 (the other experts' logits at -inf, so
    the two weights are their renormalised softmax) leave the fixture."""
    meta, ids, logits, _ = _fixture()

    def only_0_and_1(router_logits):
        forced = router_logits.clone()
        forced[:, 2:] = float("-inf")
        return forced

    tap = _RouteTap(monkeypatch, rewrite=only_0_and_1)
    lm, tok = _build(meta, use_graphs=False)
    _got_ids, got_logits = _run(lm, tok, meta, 1)[0]
    assert all(sorted(set(c.expert_ids.flatten().tolist())) == [0, 1] for c in tap.calls)
    err = np.abs(got_logits - logits[:, 0]).max(axis=1)
    assert (err > LOGIT_TOL).all(), err


REPETITIVE = [7, 19, 33] * 4 + [7, 19]  # a prompt the lookup drafter always finds a continuation for


def test_lookup_speculation_emits_the_plain_ids(gpu_device, monkeypatch):
    """spec_tokens = 3 (lookup drafter, greedy): the verify steps run the expert kernels over 1 + K rows per request.  The
    fixture's requests emit the fixture's ids; a repetitive prompt, which makes sure that drafts are verified, emits the plain
    run's ids for as long as the plain run's top-2 margin stays above twice LOGIT_TOL (below that an f16 near-tie may fall
    either way, whatever the step's shape)."""
    from tests.test_spec_model_gpu import Runner, _request

    monkeypatch.delenv("TGIS_MOE_PATH", raising=False)
    meta, ids, _logits, _ = _fixture()
    new = 12
    lm, tok = _build(meta)
    plain = Runner(lm, tok)
    plain.run(plain.batch([_request(0, REPETITIVE, new)]))
    decided = 0
    for row in plain.logits:
        top = torch.topk(row[0].float(), 2).values
        if float(top[0] - top[1]) <= 2 * LOGIT_TOL:
            break
        decided += 1
    want_plain = list(plain.ids[0])
    del lm, plain
    lm, tok = _build(meta, spec_tokens=3)
    run = Runner(lm, tok)
    requests = [_request(i, p, meta["max_new"]) for i, p in enumerate(meta["prompts"])] + [_request(3, REPETITIVE, new)]
    run.run(run.batch(requests))
    for i in range(len(meta["prompts"])):
        assert run.ids[i] == ids[i].tolist(), f"request {i}"
    stats = lm.spec_stats()
    print("spec stats:", stats, "ids decided by the margin:", decided)
    assert stats["verify_steps"] > 0 and stats["drafted"] > 0
    assert len(run.ids[3]) == new and run.ids[3][:decided] == want_plain[:decided], (run.ids[3], want_plain, decided)


# ---- world size 2 on one device, over gloo (the pattern of tests/test_tp_gpu.py) ---------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
    got = _run(lm, tok, {"prompts": prompts, "max_new": max_new}, steps)
    ret[rank] = got
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_matches_the_fixture(gpu_device):
    """Two ranks on one device: every expert's intermediate size split in two, the router replicated, one all-reduce per
    block; ids are the fixture's, logits within LOGIT_TOL, and both ranks hold the same logits."""
    meta, ids, logits, _ = _fixture()
    steps = ids.shape[1]
    mgr = mp.get_context("spawn").Manager()
    ret = mgr.dict()
    keys = ("OMP_NUM_THREADS", "MKL_NUM_THREADS")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ[k] = str(max(1, min(8, (os.cpu_count() or 8) // 2)))
    try:
        mp.spawn(_tp_worker, args=(2, _free_port(), meta["seed"], meta["prompts"], meta["max_new"], steps, ret), nprocs=2,
                 join=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for (i0, l0), (i1, l1) in zip(ret[0], ret[1]):
        assert i0 == i1 and np.array_equal(l0, l1), "ranks must hold identical logits"
    _check(ret[0], ids, logits, "tp2")
