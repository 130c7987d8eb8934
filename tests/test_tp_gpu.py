"""-m gpu, world_size 2 on ONE device: the tensor-parallel product path with the real HIP kernels (sharded GPTQ and
dense linears incl. the row-parallel K/tp rule, per-rank KV heads, vocab-parallel embedding and head) driven through
FlashCausalLM.generate_token exactly as `bench.py --gpus 2` drives it.  Collectives go through gloo (host-mediated)
because a single-GPU box cannot host two RCCL ranks; everything above and below the collective is the shipped code."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle.llama_ref import LlamaRef
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors

pytestmark = pytest.mark.gpu

PROMPTS = [[5, 9, 31, 44, 12, 7, 3, 18, 25], [11, 6, 40, 8], [22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
                                                                36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49,
                                                                50, 51, 52, 53, 54, 55, 56]]
STEPS = 4
MAX_RANKS = 4  # processes holding one shared GPU at once: the test process + at most four ranks


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(fn, args, nprocs):
    """mp.spawn with the host threads of every rank capped: ranks that each start a full OpenMP / MKL team while they
    import torch, build tensors and create their HIP context spend most of their start-up fighting for the cores.
    At most MAX_RANKS ranks: they and the test process all hold the one GPU open."""
    assert nprocs <= MAX_RANKS, f"{nprocs} ranks + the test process would hold the shared GPU open at once"
    keys = ("OMP_NUM_THREADS", "MKL_NUM_THREADS")
    old = {k: os.environ.get(k) for k in keys}
    for k in keys:
        os.environ[k] = str(max(1, (os.cpu_count() or 8) // nprocs))
    try:
        mp.spawn(fn, args=args, nprocs=nprocs, join=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _graph_info(lm):
    """(mode, captured segments per decode graph) of the model's decode graphs."""
    if not lm.use_graphs:
        return ("eager", [])
    return (lm.graph_mode, [getattr(g.graph, "num_segments", 1) for g in lm._graphs.values() if g.graph is not None])


def _worker(rank, world, port, quantize, inter, ret, cfg_kw=None):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1")
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tests.fixture_utils import FixtureTokenizer, prompt_text
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.pb import generate_pb2 as pb2

    cfg = TinyLlamaConfig(intermediate_size=inter, **{k: v for k, v in (cfg_kw or {}).items() if not k.startswith("_")})
    tensors = tiny_llama_tensors(cfg, seed=21, quantize=quantize, groupsize=64)
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, LlamaConfig(**cfg.to_dict()), torch.float16, quantize, tokenizer=tok, gptq_groupsize=64)
    assert eng.world_size == world
    lm = FlashCausalLM("tp", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=32)
    rows = {}
    orig = lm._process_new_tokens

    def tapped(batch, out, *a, **kw):
        rows["logits"] = out.detach().float().cpu().numpy().copy()
        return orig(batch, out, *a, **kw)

    lm._process_new_tokens = tapped
    reqs = [pb2.Request(id=i, inputs=prompt_text(p), input_length=len(p), truncate=False, max_output_length=STEPS + 2)
            for i, p in enumerate(PROMPTS)]
    if (cfg_kw or {}).get("_sample"):
        # request 0 seeded, request 1 WITHOUT a seed (ranks must still agree), the rest greedy
        reqs[0].parameters.temperature, reqs[0].parameters.top_k, reqs[0].parameters.seed = 0.9, 20, 7
        reqs[1].parameters.temperature, reqs[1].parameters.top_p = 1.1, 0.9
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
    ret[rank] = (ids, logits)
    ret[f"graph{rank}"] = _graph_info(lm)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


# inter=448: 224 rows of down_proj per rank = 3.5 groups of 64 -> the loader regroups into sub-groups of 32
# (llama-7B at tp=4/8 is in that situation: 11008/4 = 21.5 groups of 128)
@pytest.mark.parametrize("quantize,inter", [(None, 512), ("gptq", 512), ("gptq", 448)])
def test_tp2_product_path_matches_oracle(gpu_device, quantize, inter):
    mgr = mp.get_context("spawn").Manager()  # never fork a process that has run gRPC (or CUDA) threads
    ret = mgr.dict()
    _spawn(_worker, (2, _free_port(), quantize, inter, ret), 2)
    ids0, logits0 = ret[0]
    ids1, logits1 = ret[1]
    assert ids0 == ids1, "ranks must stay in lock-step without a broadcast"
    for a, b in zip(logits0, logits1):
        assert np.array_equal(a, b), "every rank holds identical logits after the all-gather"
    cfg = TinyLlamaConfig(intermediate_size=inter)
    ref = LlamaRef(cfg, tiny_llama_tensors(cfg, seed=21, quantize=quantize, groupsize=64), quantize=quantize, groupsize=64)
    want = ref.generate_greedy(PROMPTS, STEPS, forced=ids0)
    for i in range(STEPS):
        err = np.abs(logits0[i] - want[i]["logits"].numpy()).max()
        assert err < 0.5, f"step {i}: max |logit - oracle| = {err:.3f}"
        margin_ok = want[i]["token_ids"].tolist() == ids0[i]
        if not margin_ok:  # only a near-tie of the fp32 oracle may flip in fp16
            top2 = torch.topk(want[i]["logits"], 2, dim=-1).values
            flipped = [j for j, (a, b) in enumerate(zip(want[i]["token_ids"].tolist(), ids0[i])) if a != b]
            assert all(float(top2[j, 0] - top2[j, 1]) < 0.75 for j in flipped), f"step {i}: ids {ids0[i]}"


def test_tp4_one_head_per_rank_matches_oracle(gpu_device):
    """Four ranks on one device, the per-rank situation of llama-7B at tp=8: one q/kv head per rank, down_proj shards of
    352 rows = 5.5 groups of 64 (regrouped to 32), vocab and embedding split four ways."""
    kw = dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=4)
    inter = 1408
    mgr = mp.get_context("spawn").Manager()  # never fork a process that has run gRPC (or CUDA) threads
    ret = mgr.dict()
    _spawn(_worker, (4, _free_port(), "gptq", inter, ret, kw), 4)
    ids0, logits0 = ret[0]
    for r in range(1, 4):
        assert ret[r][0] == ids0
        assert all(np.array_equal(a, b) for a, b in zip(ret[r][1], logits0))
    cfg = TinyLlamaConfig(intermediate_size=inter, **kw)
    ref = LlamaRef(cfg, tiny_llama_tensors(cfg, seed=21, quantize="gptq", groupsize=64), quantize="gptq", groupsize=64)
    want = ref.generate_greedy(PROMPTS, STEPS, forced=ids0)
    for i in range(STEPS):
        err = np.abs(logits0[i] - want[i]["logits"].numpy()).max()
        assert err < 0.5, f"step {i}: max |logit - oracle| = {err:.3f}"


def _bigcode_worker(rank, world, port, dtype_name, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1")
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors
    from tests.fixture_utils import FixtureTokenizer, prompt_text
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.pb import generate_pb2 as pb2

    dtype = getattr(torch, dtype_name)
    cfg = TinyBigCodeConfig()
    cfg.quantize = None
    tensors = {k: v.float().to(dtype) for k, v in tiny_bigcode_tensors(cfg, seed=31).items()}
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, cfg, dtype, None, tokenizer=tok)
    lm = FlashCausalLM("tp", None, "synthetic", dtype, None, engine=eng, kv_cache_pages=32)
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
                                            None, lm.use_position_ids)
        assert not errs
        ids, logits = [], []
        for i in range(STEPS):
            toks, _, errs, _ = lm.generate_token(batch, first=(i == 0))
            assert not errs
            ids.append([t.token_id for t in toks])
            logits.append(rows["logits"])
    batch.release()
    ret[rank] = (ids, logits)
    ret[f"graph{rank}"] = _graph_info(lm)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_tp_santacoder_mqa_matches_oracle(gpu_device, world):
    """cfg5 family under tensor parallelism: q heads split, the single kv head replicated on every rank (each rank keeps
    its own copy of the KV pages), vocab-parallel tied embedding/head."""
    from oracle.santacoder_ref import SantacoderRef
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors

    mgr = mp.get_context("spawn").Manager()  # never fork a process that has run gRPC (or CUDA) threads
    ret = mgr.dict()
    _spawn(_bigcode_worker, (world, _free_port(), "float16", ret), world)
    ids0, logits0 = ret[0]
    for r in range(1, world):
        assert ret[r][0] == ids0 and all(np.array_equal(a, b) for a, b in zip(ret[r][1], logits0))
    cfg = TinyBigCodeConfig()
    want = SantacoderRef(cfg, tiny_bigcode_tensors(cfg, seed=31)).generate_greedy(PROMPTS, STEPS, forced=ids0)
    for i in range(STEPS):
        err = np.abs(logits0[i] - want[i]["logits"].numpy()).max()
        assert err < 0.1, f"step {i}: max |logit - oracle| = {err:.3f}"


def test_tp2_segmented_graphs_equal_eager(gpu_device, monkeypatch):
    """The default TP decode step is a chain of captured segments with the collectives between them
    (utils/graph_segments.py): one segment per all-reduce seam, and bit-identical logits to the eager step."""
    from oracle.tiny_models import TinyLlamaConfig

    got = {}
    for mode in ("segments", "false"):
        monkeypatch.setenv("TGIS_TP_GRAPHS", mode)
        mgr = mp.get_context("spawn").Manager()
        ret = mgr.dict()
        _spawn(_worker, (2, _free_port(), "gptq", 512, ret), 2)
        got[mode] = (ret[0], ret["graph0"], ret["graph1"])
    (ids_s, logits_s), info_s, info_s1 = got["segments"]
    (ids_e, logits_e), info_e, _ = got["false"]
    assert info_e[0] == "eager" and info_s[0] == info_s1[0] == "segments"
    layers = TinyLlamaConfig().num_hidden_layers
    # embedding reduce + two reductions per layer + the head's all-gather -> that many seams, one more segment
    assert info_s[1] and all(n == 2 * layers + 3 for n in info_s[1]), info_s
    assert ids_s == ids_e
    for a, b in zip(logits_s, logits_e):
        assert np.array_equal(a, b)


def test_tp2_sampling_ranks_agree(gpu_device):
    """Sampled requests under tensor parallelism: every rank draws the same tokens — with a request seed (same Philox
    stream everywhere) and without one (rank 0's seed base is broadcast at start-up; seedless requests take
    mix(base, arrival number))."""
    mgr = mp.get_context("spawn").Manager()
    ret = mgr.dict()
    _spawn(_worker, (2, _free_port(), "gptq", 512, ret, {"_sample": True}), 2)
    ids0, logits0 = ret[0]
    ids1, logits1 = ret[1]
    assert ids0 == ids1
    assert all(np.array_equal(a, b) for a, b in zip(logits0, logits1))
    greedy = [[int(np.argmax(l[r])) for r in range(2, len(PROMPTS))] for l in logits0]
    assert [row[2:] for row in ids0] == greedy  # the greedy neighbours are untouched by the sampled rows


@pytest.mark.parametrize("K,N,gs,world,M", [(4096, 4096, 128, 2, 32), (11008, 4096, 128, 4, 7), (1024, 96, 128, 2, 70),
                                             (4096, 512, 128, 2, 2000)])
def test_act_order_row_parallel_shards_on_the_kernels(gpu_device, K, N, gs, world, M):
    """Act-order GPTQ under row tensor parallelism through the real kernels: every rank's shard (rows sorted by group, runs
    padded to 32 rows with the gather index -1, scales / zeros from the full tables: utils/weights.py, the reference's
    g_idx fallback utils/weights.py:150-156,190-196) run one after the other on this GPU, partial results summed as the
    all-reduce would, against ops_ref.gptq_linear on the whole matrix with its random g_idx.  M = 70: 64-row passes;
    M = 2000: the dequantise + library GEMM path."""
    import types

    from oracle import ops_ref
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.layers import TensorParallelRowLinear
    from tgis_amd.utils.weights import DictWeights

    qw, qz, sc, gi = ops_ref.make_gptq_tensors(K, N, gs, seed=K + N, act_order=True)
    t = {"p.qweight": torch.from_numpy(qw), "p.qzeros": torch.from_numpy(qz), "p.scales": torch.from_numpy(sc),
         "p.g_idx": torch.from_numpy(gi).to(torch.int32)}
    g = torch.Generator().manual_seed(M)
    x = (torch.randn(M, K, generator=g) * 0.5).half()
    want = ops_ref.gptq_linear(x, qw, qz, sc, gi, gs, None).float()
    rows = K // world
    total = torch.zeros((M, N), dtype=torch.float32)
    for rank in range(world):
        w = DictWeights(t, gpu_device, torch.float16, FakeGroup(rank, world))
        w.gptq_bits, w.gptq_groupsize = 4, gs
        lin = TensorParallelRowLinear.load(types.SimpleNamespace(quantize="gptq"), "p", w, bias=False).linear
        y = lin(x[:, rank * rows:(rank + 1) * rows].contiguous().to(gpu_device))
        assert lin.q_handle.perm is not None and lin.q_handle.in_features == rows
        total += y.float().cpu()
    err = (total - want).abs()
    bound = 4e-3 * want.abs() + 4e-3 * float(want.abs().mean()) + 1e-3  # world f16 roundings of partial sums
    assert bool((err <= bound).all()), f"max err {float(err.max()):.4g}"
