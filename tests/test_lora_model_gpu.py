"""-m gpu: per-request LoRA adapters end to end on the Llama flash path against transformers' fp32 CPU LlamaForCausalLM on
MERGED weights (tests/golden/llama_lora.npz, made by tests/golden/make_llama_lora_fixtures.py on the seeded tiny Llama and the
three seeded adapters of tests/lora_tiny.py): prompts of 5, 20, 33 and 12 tokens for no adapter, `qv` (r 8 on q and v), `all` (r 16
on all seven modules) and `od` (r 4 on o and down), 12 greedy tokens each, plus a prompt of 100 tokens under `all`.  The
fixture's top-2 margins all exceed 0.7 = 2 LOGIT_TOL, so f16 runs must reproduce every id.  The adapters are real peft
directories written into tmp_path and named by `prefix_id`."""
import json
import os

import numpy as np
import pytest
import torch

from tests import lora_tiny
from tests.fixture_utils import GOLDEN, FixtureTokenizer, prompt_text
from tests.test_neox_model_gpu import _LogitTap, _step

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35  # tests/test_model_gpu.py's f16 bar


def _fixture():
    z = np.load(os.path.join(GOLDEN, "llama_lora.npz"))
    return json.loads(bytes(z["meta"]).decode()), z


def _build(meta, store, lora_slots=4, quantize=None, use_graphs=True, **kw):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.prompt_cache import PrefixCache

    cfg = lora_tiny.TinyLlamaConfig()
    tok = FixtureTokenizer(cfg.vocab_size)
    tensors = lora_tiny.tiny_llama_tensors(cfg, meta["seed"], quantize=quantize, groupsize=lora_tiny.GROUPSIZE)
    eng = InferenceEngine(tensors, LlamaConfig(**cfg.to_dict()), torch.float16, quantize, tokenizer=tok,
                          gptq_groupsize=lora_tiny.GROUPSIZE)
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=64,
                       lora_slots=lora_slots, **kw)
    lm.use_graphs = use_graphs
    lm.prefix_cache = PrefixCache(lm.device, lm.dtype, 64, cfg.hidden_size, store=store)
    lm.prefix_cache.lora = lm.lora_table
    return lm, tok


@pytest.fixture()
def store(tmp_path):
    meta, _ = _fixture()
    cfg = lora_tiny.TinyLlamaConfig()
    for name in lora_tiny.ADAPTER_NAMES:
        lora_tiny.write_adapter(tmp_path / name, name, cfg, meta["seed"])
    return tmp_path


def _pb(prompts, adapters, max_new, first_id=0, batch_id=0):
    from tgis_amd.pb import generate_pb2 as pb2

    reqs = []
    for i, (p, a) in enumerate(zip(prompts, adapters)):
        r = pb2.Request(id=first_id + i, inputs=prompt_text(p), input_length=len(p), truncate=False, max_output_length=max_new)
        if a:
            r.prefix_id = a
        r.details.logprobs = True
        reqs.append(r)
    return pb2.Batch(id=batch_id, requests=reqs)


def _from_pb(lm, tok, pb):
    with lm.context_manager():
        return lm.batch_type.from_pb(pb, tok, lm.dtype, lm.device, lm.word_embeddings, lm.prefix_cache, True)


def _run(lm, tok, prompts, adapters, steps, max_new=12, mutate=None):
    """[(ids [B], logits [B, vocab])] of the prefill and steps - 1 decode steps of one batch."""
    tap = _LogitTap(lm)
    batch, errs = _from_pb(lm, tok, _pb(prompts, adapters, max_new))
    assert not errs
    if mutate is not None:
        mutate(batch)
    got = []
    for i in range(steps):
        toks, logits = _step(lm, batch, tap, first=(i == 0))
        got.append(([t.token_id for t in toks], logits))
    batch.release()
    return got


def _check(got, ids, logits, what):
    """got: [(ids [B], logits [B, vocab])] per step; ids [B, steps], logits [B, steps, vocab] of the fixture."""
    worst = 0.0
    for i, (got_ids, got_logits) in enumerate(got):
        err = float(np.abs(got_logits - logits[:, i]).max())
        worst = max(worst, err)
        assert got_ids == ids[:, i].tolist(), f"{what} step {i}: ids {got_ids} != {ids[:, i].tolist()}"
        assert err <= LOGIT_TOL, f"{what} step {i}: max |logit - reference| = {err:.3f} > {LOGIT_TOL}"
    print(f"{what}: max |logit - reference| over {len(got)} steps = {worst:.4f}")


def test_mixed_batch_matches_the_merged_models_graph_and_eager(gpu_device, store):
    """The four requests as ONE batch (70 prompt rows: the prefill loops on the host over the three requests that carry an
    adapter; every decode step takes the kernels): every request's ids equal its own merged model's, logits within the f16
    bar; the captured steps equal the eager ones bit for bit."""
    meta, z = _fixture()
    runs = {}
    for use_graphs in (True, False):
        lm, tok = _build(meta, store, use_graphs=use_graphs)
        got = runs[use_graphs] = _run(lm, tok, meta["prompts"], meta["adapters"], meta["max_new"])
        _check(got, z["ids"], z["logits"], f"graphs={use_graphs}")
        if use_graphs:
            assert [k for k in lm._graphs if k[-1] == "lora"] and all(g.graph is not None for g in lm._graphs.values())
        assert lm.lora_table.pins == [0] * 4 and lm.lora_table.loads == 3
    for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
        assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"


def test_without_the_slots_it_is_the_base_model(gpu_device, store):
    """The feature's test: the same batch with every slot forced to -1 gives the base model's ids for all four requests and
    misses the adapter rows' logits by more than the bar."""
    meta, z = _fixture()
    lm, tok = _build(meta, store)

    def drop(batch):
        slots, batch.lora_slots = batch.lora_slots, None
        for s in slots:
            lm.lora_table.release(s)

    got = _run(lm, tok, meta["prompts"], meta["adapters"], meta["max_new"], mutate=drop)
    _check(got, z["base_ids"], z["base_logits"], "slots at -1")
    err = np.abs(got[0][1] - z["logits"][:, 0]).max(axis=1)
    assert err[0] <= LOGIT_TOL and (err[1:] > LOGIT_TOL).all(), err
    assert not [k for k in lm._graphs if k[-1] == "lora"]


def test_a_batch_without_adapters_keeps_the_plain_graph(gpu_device, store):
    """On the LoRA-enabled model (its MLP without the fused SiLU * up epilogue) a batch without adapters runs the plain key's
    graph and matches the base model on all four prompts."""
    meta, z = _fixture()
    lm, tok = _build(meta, store)
    got = _run(lm, tok, meta["prompts"], [None] * 4, meta["max_new"])
    _check(got, z["base_ids"], z["base_logits"], "no adapters")
    assert lm._graphs and all(len(k) == 2 for k in lm._graphs) and lm.lora_table.loads == 0


def test_long_prompt_takes_the_host_loop(gpu_device, store):
    """100 prompt tokens under the all-module adapter: past the 64 rows of the kernel path."""
    meta, z = _fixture()
    lm, tok = _build(meta, store)
    got = _run(lm, tok, [meta["long_prompt"]], [meta["long_adapter"]], meta["long_new"], max_new=meta["long_new"])
    _check(got, z["long_ids"][None], z["long_logits"][None], "long prompt")


def test_concatenate_prune_and_slot_reuse(gpu_device, store):
    """lora_slots=2 and three adapters: a second batch joins after 3 steps (its 33-row prefill takes the kernels), a third
    adapter's request is refused while both slots are pinned and served once a prune has freed one; the slot images stay
    where they are."""
    meta, z = _fixture()
    lm, tok = _build(meta, store, lora_slots=2)
    prompts, ids, logits = meta["prompts"], z["ids"], z["logits"]
    where = [(lin.images.A.data_ptr(), lin.images.B.data_ptr(), lin.images.ranks.data_ptr()) for lin in lm.lora_linears]
    tap = _LogitTap(lm)
    seen = {}  # request id -> tokens checked so far
    variant = {0: 1, 1: 0, 2: 2, 3: 3}  # request id -> fixture row: qv, none, all, od

    def step(batch, first=False):
        toks, rows = _step(lm, batch, tap, first=first)
        for t, row in zip(toks, rows):
            v, i = variant[t.request_id], seen.get(t.request_id, 0)
            err = float(np.abs(row - logits[v, i]).max())
            assert t.token_id == int(ids[v, i]) and err <= LOGIT_TOL, (t.request_id, i, t.token_id, int(ids[v, i]), err)
            seen[t.request_id] = i + 1

    a, errs = _from_pb(lm, tok, _pb([prompts[1], prompts[0]], ["qv", None], 12, first_id=0, batch_id=1))
    assert not errs and a.lora_slots == [0, -1]
    step(a, first=True)  # 25 rows: the kernels serve this prefill
    for _ in range(3):
        step(a)
    b, errs = _from_pb(lm, tok, _pb([prompts[2]], ["all"], 12, first_id=2, batch_id=2))
    assert not errs and b.lora_slots == [1]
    step(b, first=True)
    m = lm.batch_type.concatenate([a, b])
    assert m.lora_slots == [0, -1, 1] and lm.lora_table.pins == [1, 1]
    step(m)
    none, errs = _from_pb(lm, tok, _pb([prompts[3]], ["od"], 12, first_id=3, batch_id=3))
    assert none is None and len(errs) == 1 and "pinned by live requests" in errs[0].message
    step(m)
    m = lm.batch_type.prune(m, [0])
    assert m.lora_slots == [-1, 1] and lm.lora_table.pins == [0, 1]
    c, errs = _from_pb(lm, tok, _pb([prompts[3]], ["od"], 12, first_id=3, batch_id=4))
    assert not errs and c.lora_slots == [0] and lm.lora_table.ids == ["od", "all"]
    step(c, first=True)
    m = lm.batch_type.concatenate([m, c])
    for _ in range(4):
        step(m)
    assert seen[1] == 10 and seen[2] == 7 and seen[3] == 5 and seen[0] == 6
    m.release()
    assert lm.lora_table.pins == [0, 0]
    assert where == [(lin.images.A.data_ptr(), lin.images.B.data_ptr(), lin.images.ranks.data_ptr())
                     for lin in lm.lora_linears]


def test_adapter_over_the_int4_base(gpu_device, store):
    """The tiny GPTQ Llama of the existing fixtures under the all-module adapter, against the project's fp32 oracle
    (oracle/llama_ref.py) on the DEQUANTISED weights with the adapter merged in (transformers cannot merge into int4), fed
    the model's own ids: logits within the f16 bar, and the ids where the oracle decides by more than twice the bar.
    (A deviation from the issue's wording, which asks for an fp64 restatement: the oracle computes in fp32.  It is an
    independent restatement of the model on the CPU, its own error is orders of magnitude below the bar, and the bar is the
    issue's.)"""
    from oracle.llama_ref import LlamaRef

    meta, _z = _fixture()
    cfg = lora_tiny.TinyLlamaConfig()
    lm, tok = _build(meta, store, quantize="gptq")
    prompts = [meta["prompts"][2], meta["prompts"][3]]
    got = _run(lm, tok, prompts, ["all", None], 6)
    tensors = lora_tiny.tiny_llama_tensors(cfg, meta["seed"], quantize="gptq", groupsize=lora_tiny.GROUPSIZE)
    worst = 0.0
    for r, name in enumerate(("all", None)):
        ref = LlamaRef(cfg, lora_tiny.merged_state_dict(cfg, tensors, name, meta["seed"]))
        want = ref.generate_greedy([prompts[r]], len(got), forced=[[g[0][r]] for g in got])
        for i, ((got_ids, got_logits), w) in enumerate(zip(got, want)):
            wl = w["logits"].numpy()[0]
            err = float(np.abs(got_logits[r] - wl).max())
            worst = max(worst, err)
            assert err <= LOGIT_TOL, f"request {r} step {i}: max |logit - oracle| = {err:.3f} > {LOGIT_TOL}"
            top2 = np.sort(wl)[-2:]
            if top2[1] - top2[0] > 2 * LOGIT_TOL:
                assert got_ids[r] == int(wl.argmax())
    print(f"int4 base: max |logit - merged oracle| = {worst:.4f}")
    # the adapter matters here too: the base oracle is far from the adapter row
    base = LlamaRef(cfg, lora_tiny.merged_state_dict(cfg, tensors, None, meta["seed"]))
    b0 = base.generate_greedy([prompts[0]], 1)[0]["logits"].numpy()[0]
    assert float(np.abs(got[0][1][0] - b0).max()) > LOGIT_TOL
