"""-m gpu: GPTQ GPT-BigCode end to end (TinyBigCodeConfig, group size 64, f16) against the oracle: SantacoderRef on the
dequantised dense tensors (tests/bigcode_gptq_ref.py), forced to the product's tokens as tests/test_gptq8_model_gpu.py does.

Ids equal the oracle's unless its top-2 margin is below the tie margin of the int4 Llama tests (0.75).  The logit bars start
from the dense f16 BigCode bar of tests/test_model_gpu.py (0.08): the oracle sees the same dequantised weights, so only f16
rounding separates the two; see LOGIT_TOL below for the measured values.  The fp8 cache keeps the bar
tests/test_kv_fp8_model_gpu.py sets for BigCode against the quantised-KV oracle."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bigcode_gptq_ref as bref  # noqa: E402
import test_kv_fp8_model_gpu as kv8  # noqa: E402
from test_kv_fp8_model_gpu import quantised_oracle  # noqa: E402,F401  (fixture)
from test_tp_gpu import PROMPTS, STEPS, _free_port, _spawn  # noqa: E402

from oracle.santacoder_ref import SantacoderRef  # noqa: E402
from oracle.tiny_models import TinyBigCodeConfig  # noqa: E402

pytestmark = pytest.mark.gpu
GS = bref.GS
TIE_MARGIN = 0.75
# max |logit - oracle| per scenario is printed by every test (-s).  Measured on MI355X: equal 0.0180,
# ragged 0.0177, act-order 0.0179, long prompt 0.0163, 8-bit 0.0195, two ranks 0.0199, fp8 cache 0.2088 (its own bar, 0.32):
# nothing exceeds the dense f16 BigCode bar, which therefore holds unchanged, for two ranks too.
LOGIT_TOL, TP_TOL = 0.08, 0.08

_TENSORS = {}


def _tensors(seed, act_order=False, bits=4):
    key = (seed, act_order, bits)
    if key not in _TENSORS:
        cfg = TinyBigCodeConfig()
        t = bref.tiny_bigcode_gptq_tensors(cfg, seed, GS, act_order, bits)
        _TENSORS[key] = (cfg, t, SantacoderRef(cfg, bref.dense_tensors(t, GS, bits)))
    return _TENSORS[key]


def _lm(cfg, tensors, use_graphs=True, kv="auto", pages=64, bits=4):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer
    from tgis_amd.utils.layers import Ex4bitLinearV2, Gptq8Linear

    pcfg = TinyBigCodeConfig()  # the engine writes `quantize` into its config: not into the oracle's
    assert pcfg.to_dict() == {k: v for k, v in cfg.to_dict().items() if k != "quantize"}
    tok = SyntheticTokenizer(pcfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, pcfg, torch.float16, "gptq", tokenizer=tok,
                          gptq_bits=bits, gptq_groupsize=GS)
    lm = FlashCausalLM("synthetic", None, "synthetic", torch.float16, "gptq", engine=eng, kv_cache_pages=pages,
                       kv_cache_dtype=kv)
    lm.use_graphs = use_graphs
    blk = lm.model.transformer.h[0]
    for lin in (blk.attn.c_attn.linear, blk.attn.c_proj.linear, blk.mlp.c_fc.linear, blk.mlp.c_proj.linear):
        assert type(lin) is (Ex4bitLinearV2 if bits == 4 else Gptq8Linear) and lin.q_handle is not None
    return lm, tok


def _check(got, logits, want, tol, what):
    """got: [(request id, token id, logprob)] per step; want: the oracle's steps, forced to the product's tokens."""
    worst = 0.0
    for i, (s, lg, w) in enumerate(zip(got, logits, want)):
        err = float(np.abs(lg - w["logits"].numpy()).max())
        worst = max(worst, err)
        print(f"{what} step {i}: max |logit - oracle| = {err:.4f}")
        top2 = torch.topk(w["logits"], 2, dim=-1).values
        for j, (_, tid, _) in enumerate(s):
            if tid != int(w["token_ids"][j]):  # only a near-tie of the fp32 oracle may flip in fp16
                assert float(top2[j, 0] - top2[j, 1]) < TIE_MARGIN, f"{what} step {i} row {j}: {tid} vs {int(w['token_ids'][j])}"
    print(f"{what}: max |logit - oracle| over {len(got)} steps = {worst:.4f} (bar {tol})")
    assert worst <= tol, f"{what}: max |logit - oracle| = {worst:.4f} > {tol}"


def _generate_and_check(lens, seed, what, act_order=False, steps=4, use_graphs=True, bits=4):
    cfg, tensors, ref = _tensors(seed, act_order, bits)
    lm, tok = _lm(cfg, tensors, use_graphs, bits=bits)
    got, prompts, logits = kv8._run(lm, tok, lens, steps)
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    want = ref.generate_greedy(prompts, len(got), forced=[[t[1] for t in s] for s in got])
    _check(got, logits, want, LOGIT_TOL, what)
    return lm


@pytest.mark.parametrize("use_graphs", [True, False], ids=["graphs", "eager"])
@pytest.mark.parametrize("scenario,lens", [("equal", [16, 16, 16]), ("ragged", [5, 37, 16])])
def test_prompts_match_oracle(gpu_device, scenario, lens, use_graphs):
    lm = _generate_and_check(lens, 7, f"{scenario} {'graphs' if use_graphs else 'eager'}", use_graphs=use_graphs)
    assert lm.use_graphs == use_graphs and (lm._graphs or not use_graphs), "no decode graph was captured"


def test_decode_graph_is_bit_equal_to_eager(gpu_device):
    cfg, tensors, _ = _tensors(7)
    lens = [5, 37, 16, 64]
    lm, tok = _lm(cfg, tensors, True)
    got_g, _, lg_g = kv8._run(lm, tok, lens, 6)
    assert lm._graphs, "no decode graph was captured"
    lme, toke = _lm(cfg, tensors, False)
    got_e, _, lg_e = kv8._run(lme, toke, lens, 6)
    assert got_g == got_e, "graph replay and eager steps differ"
    for a, b in zip(lg_g, lg_e):
        assert np.array_equal(a, b), "graph and eager logits differ"


def test_fused_gelu_launch_is_bit_equal_to_two_launches(gpu_device, monkeypatch):
    """The whole model with TGIS_FUSED_GELU_GEMM on and off: the same logits bit for bit (eager, so that every step takes
    the switch as it is set)."""
    from tgis_amd.utils import layers

    cfg, tensors, _ = _tensors(7)
    runs = []
    for on in (True, False):
        monkeypatch.setattr(layers, "FUSED_GELU_GEMM", on)
        lm, tok = _lm(cfg, tensors, False)
        runs.append(kv8._run(lm, tok, [5, 37, 16], 4))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(a, b), "fused and two-launch logits differ"


def test_decode_step_takes_the_forms_of_the_dense_model(gpu_device, monkeypatch):
    """One eager decode step: every c_attn leaves its split-K sum to the cache-write kernel (no rotary), both c_proj leave
    theirs and their bias to the add + LayerNorm behind them, and c_fc + GELU is one launch."""
    from tgis_amd import native
    from tgis_amd.testing import make_batch_pb

    cfg, tensors, _ = _tensors(7)
    lm, tok = _lm(cfg, tensors, use_graphs=False)
    L = cfg.num_hidden_layers
    calls = {"kv": [], "ln": [], "gemm": [], "gelu": 0}

    def spy(name, note):
        real = getattr(native, name)

        def wrapped(*a, **kw):
            note(a, kw)
            return real(*a, **kw)
        monkeypatch.setattr(native, name, wrapped)

    with lm.context_manager():
        batch, errs = lm.batch_type.from_pb(make_batch_pb([5, 37, 16], max_new=4), tok, lm.dtype, lm.device, lm.word_embeddings,
                                            None, True)
        assert not errs
        lm.generate_token(batch, first=True)
        spy("rope_kv_write", lambda a, kw: calls["kv"].append((isinstance(a[0], native.Partial), a[1] is None)))
        spy("layernorm_residual", lambda a, kw: calls["ln"].append(isinstance(a[0], native.Partial) and a[0].bias is not None))
        spy("gptq_gemm", lambda a, kw: calls["gemm"].append(kw.get("act", 0)))
        spy("gelu", lambda a, kw: calls.__setitem__("gelu", calls["gelu"] + 1))
        lm.generate_token(batch)
    batch.release()
    assert calls["kv"] == [(True, True)] * L, calls["kv"]
    assert calls["ln"] == [False] + [True] * (2 * L), calls["ln"]  # ln_1 of layer 0 reads the embeddings
    assert calls["gemm"] == [5] * L and calls["gelu"] == 0, calls


def test_continuous_batching_matches_oracle(gpu_device):
    """Two batches prefilled apart, concatenated, one request pruned: every request's logits match the oracle's run of that
    request alone, forced to the product's tokens."""
    from tgis_amd.testing import make_batch_pb

    cfg, tensors, ref = _tensors(7)
    lm, tok = _lm(cfg, tensors)
    tap = kv8._Tap(lm)
    seen, prompts = {0: [], 1: [], 2: []}, {}

    def record(toks):
        rows = tap.rows[-1]
        assert rows.shape[0] == len(toks)
        for j, t in enumerate(toks):
            seen[t.request_id].append((t.token_id, rows[j]))

    with lm.context_manager():
        def prefill(lens, first, bid):
            pb = make_batch_pb(lens, max_new=7, batch_id=bid, first_request_id=first, logprobs=True)
            b, errs = lm.batch_type.from_pb(pb, tok, lm.dtype, lm.device, lm.word_embeddings, None, True)
            assert not errs
            for i, n in enumerate(lens):
                prompts[first + i] = b.all_input_ids_tensor[i, :n].tolist()
            record(lm.generate_token(b, first=True, for_concat=True)[0])
            return b

        a = prefill([9, 40], 0, 1)
        record(lm.generate_token(a)[0])
        b = prefill([33], 2, 2)
        merged = lm.batch_type.concatenate([a, b])
        for _ in range(2):
            record(lm.generate_token(merged)[0])
        merged = lm.batch_type.prune(merged, [0])
        for _ in range(2):
            record(lm.generate_token(merged)[0])
        merged.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    assert [len(seen[r]) for r in (0, 1, 2)] == [4, 6, 5]  # request 0 leaves with the prune
    for rid, steps in seen.items():
        want = ref.generate_greedy([prompts[rid]], len(steps), forced=[[tid] for tid, _ in steps])
        _check([[(rid, tid, 0.0)] for tid, _ in steps], [lg[None] for _, lg in steps], want, LOGIT_TOL, f"continuous request {rid}")


def test_act_order_matches_oracle(gpu_device):
    lm = _generate_and_check([7, 40, 1], 11, "act-order", act_order=True)
    blk = lm.model.transformer.h[0]
    assert blk.mlp.c_fc.linear.q_handle.perm is not None and blk.mlp.c_proj.linear.q_handle.perm is not None


def test_prompt_of_more_than_256_tokens(gpu_device):
    """300 + 5 rows of prefill: c_fc takes the tall kernel (or dequantise + library GEMM) and tgis_gelu; decode stays fused."""
    _generate_and_check([300, 5], 7, "long prompt", steps=3)


def test_fp8_kv_cache_matches_quantised_kv_oracle(gpu_device, quantised_oracle):
    cfg, tensors, ref = _tensors(7)
    lm, tok = _lm(cfg, tensors, kv="fp8_e4m3")
    assert lm.kv_cache.is_fp8
    got, prompts, logits = kv8._run(lm, tok, [5, 37, 16], 4)
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    quantised_oracle(torch.float16)
    want = ref.generate_greedy(prompts, len(got), forced=[[t[1] for t in s] for s in got])
    _check(got, logits, want, kv8.BIGCODE_TOL[torch.float16], "fp8 cache")


def test_8_bit_checkpoint_through_the_default_forward_gelu(gpu_device):
    from tgis_amd.utils.layers import Gptq8Linear, Linear

    assert Gptq8Linear.forward_gelu is Linear.forward_gelu
    _generate_and_check([5, 37, 16], 7, "8-bit", bits=8)


def _tp_worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import bigcode_gptq_ref as ref4
    from tests.fixture_utils import FixtureTokenizer, prompt_text
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.pb import generate_pb2 as pb2
    from tgis_amd.utils.layers import Ex4bitLinearV2

    cfg = TinyBigCodeConfig()
    tensors = ref4.tiny_bigcode_gptq_tensors(cfg, 21, GS, True)
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, cfg, torch.float16, "gptq", tokenizer=tok, gptq_bits=4, gptq_groupsize=GS)
    assert eng.world_size == world
    lm = FlashCausalLM("tp", None, "synthetic", torch.float16, "gptq", engine=eng, kv_cache_pages=32)
    blk = lm.model.transformer.h[0]
    lins = (blk.attn.c_attn.linear, blk.attn.c_proj.linear, blk.mlp.c_fc.linear, blk.mlp.c_proj.linear)
    assert all(type(lin) is Ex4bitLinearV2 and lin.q_handle is not None for lin in lins)
    shapes = [(lin.q_handle.in_features, lin.q_handle.N) for lin in lins]
    rows = {}
    orig = lm._process_new_tokens

    def tapped(batch, out, *a, **kw):
        rows["logits"] = out.detach().float().cpu().numpy().copy()
        return orig(batch, out, *a, **kw)

    lm._process_new_tokens = tapped
    reqs = [pb2.Request(id=i, inputs=prompt_text(p), input_length=len(p), truncate=False, max_output_length=STEPS + 2)
            for i, p in enumerate(PROMPTS)]
    with lm.context_manager():
        batch, errs = lm.batch_type.from_pb(pb2.Batch(id=0, requests=reqs), tok, lm.dtype, lm.device, lm.word_embeddings,
                                            None, True)
        assert not errs
        ids, logits = [], []
        for i in range(STEPS):
            toks, _, errs, _ = lm.generate_token(batch, first=(i == 0))
            assert not errs
            ids.append([t.token_id for t in toks])
            logits.append(rows["logits"])
    batch.release()
    ret[rank] = (ids, logits, shapes, (blk.attn.c_proj.linear.bias is not None, blk.mlp.c_proj.linear.bias is not None),
                 lm.kv_cache.free_pages == lm.kv_cache.num_pages)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_act_order_on_one_gpu_matches_oracle(gpu_device):
    """World size 2 on one device (gloo collectives), act-order: q columns sharded with the k / v head on both ranks, c_fc a
    column shard, both c_proj act-order row shards with their bias on rank 0."""
    mgr = mp.get_context("spawn").Manager()  # never fork a process that has run gRPC (or CUDA) threads
    ret = mgr.dict()
    _spawn(_tp_worker, (2, _free_port(), ret), 2)
    ids0, logits0, shapes0, bias0, free0 = ret[0]
    ids1, logits1, shapes1, bias1, free1 = ret[1]
    assert ids0 == ids1 and all(np.array_equal(a, b) for a, b in zip(logits0, logits1))
    assert free0 and free1
    cfg = TinyBigCodeConfig()
    E, I, D = cfg.hidden_size, cfg.n_inner, cfg.hidden_size // cfg.num_attention_heads
    assert shapes0 == shapes1 == [(E, E // 2 + 2 * D), (E // 2, E), (E, I // 2), (I // 2, E)]
    assert bias0 == (True, True) and bias1 == (False, False)
    _, _, ref = _tensors(21, True)
    want = ref.generate_greedy(PROMPTS, STEPS, forced=ids0)
    got = [[(j, tid, 0.0) for j, tid in enumerate(s)] for s in ids0]
    _check(got, logits0, want, TP_TOL, "tp2")
