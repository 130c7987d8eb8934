"""GPT-NeoX served the way a deployment serves it: tensor parallel (two ranks sharing one GPU, as tests/test_tp_gpu.py
does) with one all-reduce per parallel-residual layer, and a safetensors checkpoint directory loaded by the tgis_native
engine behind the gRPC servicer.  Both against the reference's fixtures (tests/golden/neox_*.npz)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.fixture_utils import check_ids, load_fixture
from tests.neox_tiny import TinyNeoXConfig, tiny_neox_tensors
from tests.test_tp_gpu import _free_port, _spawn

pytestmark = pytest.mark.gpu


def _tp_worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1")
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist

    from tests.fixture_utils import FixtureTokenizer, load_fixture, prompt_text
    from tests.neox_tiny import TinyNeoXConfig, tiny_neox_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling import flash_neox_modeling
    from tgis_amd.models.custom_modeling.flash_neox_modeling import GPTNeoXConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.pb import generate_pb2 as pb2

    meta, steps = load_fixture("neox_equal")
    cfg = TinyNeoXConfig(meta["variant"])
    tensors = {k: v.to(torch.float16) for k, v in tiny_neox_tensors(cfg, seed=meta["seed"]).items()}
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, GPTNeoXConfig(**cfg.hf_kwargs()), torch.float16, None, tokenizer=tok)
    lm = FlashCausalLM("tp", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=32)
    lm.use_graphs = False  # every all-reduce of a step is a call of this process
    # all-reduces issued from inside the decoder layers, counted per generate_token call
    calls = {"layers": 0}
    layer_forward = flash_neox_modeling.FlashNeoXLayer.forward_parallel
    orig_all_reduce = dist.all_reduce
    inside = {"on": False}

    def counting_all_reduce(*a, **kw):
        if inside["on"]:
            calls["layers"] += 1
        return orig_all_reduce(*a, **kw)

    def traced_forward(self, *a, **kw):
        inside["on"] = True
        try:
            return layer_forward(self, *a, **kw)
        finally:
            inside["on"] = False

    dist.all_reduce = counting_all_reduce
    flash_neox_modeling.FlashNeoXLayer.forward_parallel = traced_forward
    rows = {}
    orig = lm._process_new_tokens

    def tapped(batch, out, *a, **kw):
        rows["logits"] = out.detach().float().cpu().numpy().copy()
        return orig(batch, out, *a, **kw)

    lm._process_new_tokens = tapped
    reqs = []
    for i, p in enumerate(meta["prompts"]):
        r = pb2.Request(id=i, inputs=prompt_text(p), input_length=len(p), truncate=False,
                        max_output_length=meta["max_new"])
        r.details.logprobs = True
        reqs.append(r)
    out = []
    with lm.context_manager():
        batch, errs = lm.batch_type.from_pb(pb2.Batch(id=0, requests=reqs), tok, lm.dtype, lm.device, lm.word_embeddings,
                                            None, True)
        assert not errs
        for i in range(len(steps)):
            calls["layers"] = 0
            toks, _, errs, _ = lm.generate_token(batch, first=(i == 0))
            assert not errs
            out.append(([t.request_id for t in toks], [t.token_id for t in toks], rows["logits"], calls["layers"]))
    batch.release()
    ret[rank] = (out, lm.num_layers)
    dist.barrier()
    dist.destroy_process_group()


def test_neox_tp2_matches_reference_with_one_all_reduce_per_layer(gpu_device):
    """Two ranks, heads split, dense / dense_4h_to_h biases on rank 0 only: both ranks return the fixture's tokens and
    the same logits, within the fixture tolerance of the reference, and every parallel-residual layer issues exactly
    one all-reduce per step (attention + MLP summed first, reference flash_neox_modeling.py:254-257)."""
    meta, steps = load_fixture("neox_equal")
    mgr = mp.get_context("spawn").Manager()
    ret = mgr.dict()
    _spawn(_tp_worker, (2, _free_port(), ret), 2)
    (out0, layers), (out1, _) = ret[0], ret[1]
    for i, ((req0, ids0, lg0, n0), (req1, ids1, lg1, n1), want) in enumerate(zip(out0, out1, steps)):
        assert ids0 == ids1 and np.array_equal(lg0, lg1), f"step {i}: ranks disagree"
        assert req0 == want["request_ids"].tolist()
        check_ids(ids0, want, f"tp2 step {i}")
        err = np.abs(lg0 - want["logits"]).max()
        assert err <= 0.35, f"tp2 step {i}: max |logit - reference| = {err:.3f}"
        assert n0 == n1 == layers, f"step {i}: {n0} / {n1} all-reduces inside {layers} decoder layers"


def _write_checkpoint(path, cfg, tensors):
    """A gpt_neox directory as the hub ships one: config.json (transformers 4.x keys), model.safetensors with the
    checkpoint's own names (gpt_neox.*, embed_out), a word-level tokenizer of the fixture vocabulary."""
    from safetensors.torch import save_file
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    os.makedirs(path, exist_ok=True)
    conf = dict(cfg.hf_kwargs(), model_type="gpt_neox", architectures=["GPTNeoXForCausalLM"], torch_dtype="float16")
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(conf, f)
    save_file({k: v.to(torch.float16).contiguous() for k, v in tensors.items()}, os.path.join(path, "model.safetensors"))
    vocab = {"<pad>": 0, "<s>": 1, "</s>": 2}
    for i in range(3, cfg.vocab_size):
        vocab[f"t{i}"] = i
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<pad>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    PreTrainedTokenizerFast(tokenizer_object=tk, eos_token="</s>", bos_token="<s>", unk_token="<pad>",
                            pad_token="<pad>").save_pretrained(path)


def test_neox_grpc_shard_from_a_safetensors_directory(gpu_device, tmp_path):
    """get_model on a written tiny gpt_neox directory (tgis_native engine, safetensors Weights, the config as
    transformers parses it) behind the gRPC servicer: Prefill A -> NextToken -> Prefill B -> NextToken(A, B)
    (concatenate) -> NextToken with id 0 completed (prune) returns the continuous fixture's tokens."""
    import asyncio

    import grpc

    from tgis_amd.cache import Cache
    from tgis_amd.models import get_model
    from tgis_amd.models.custom_modeling.flash_neox_modeling import FlashGPTNeoXForCausalLM
    from tgis_amd.pb import generate_pb2 as pb
    from tgis_amd.pb import generate_pb2_grpc
    from tgis_amd.server import MemoryScalingModel, TextGenerationService
    from tests.fixture_utils import prompt_text

    meta, steps = load_fixture("neox_continuous")
    cfg = TinyNeoXConfig(meta["variant"])
    path = str(tmp_path / "neox")
    _write_checkpoint(path, cfg, tiny_neox_tensors(cfg, seed=meta["seed"]))
    lm = get_model(path, None, "tgis_native", "float16", None, 256)
    assert isinstance(lm.model, FlashGPTNeoXForCausalLM) and lm.head_size == 96

    def batch(prompts, first_id, bid):
        reqs = []
        for i, p in enumerate(prompts):
            r = pb.Request(id=first_id + i, inputs=prompt_text(p), input_length=len(p), truncate=False,
                           max_output_length=meta["max_new"])
            r.details.logprobs = True
            reqs.append(r)
        return pb.Batch(id=bid, requests=reqs)

    def cached(bid, done):
        cb = pb.CachedBatch(batch_id=bid)
        cb.status.completed_ids.extend(done)
        return cb

    async def run():
        got = []
        url = f"unix://{tmp_path}/shard-0"
        server = grpc.aio.server()
        svc = TextGenerationService(lm, Cache(), [url], MemoryScalingModel(lm.kv_cache.num_pages * 32))
        generate_pb2_grpc.add_TextGenerationServiceServicer_to_server(svc, server)
        server.add_insecure_port(url)
        await server.start()
        async with grpc.aio.insecure_channel(url) as ch:
            stub = generate_pb2_grpc.TextGenerationServiceStub(ch)
            got.append((await stub.Prefill(pb.PrefillRequest(batch=batch(meta["prompts_a"], 0, 1)))).result)
            got.append((await stub.NextToken(pb.NextTokenRequest(batches=[cached(1, [])]))).result)
            got.append((await stub.Prefill(pb.PrefillRequest(batch=batch(meta["prompts_b"], 2, 2)))).result)
            got.append((await stub.NextToken(pb.NextTokenRequest(batches=[cached(1, []), cached(2, [])]))).result)
            got.append((await stub.NextToken(pb.NextTokenRequest(batches=[cached(1, [0])]))).result)
        await server.stop(0)
        return got

    got = asyncio.run(run())
    assert len(got) == len(steps)
    for i, (res, want) in enumerate(zip(got, steps)):
        assert [t.request_id for t in res.output_tokens] == want["request_ids"].tolist(), f"step {i}"
        check_ids([t.token_id for t in res.output_tokens], want, f"grpc step {i}")
        assert res.forward_time_ns > 0 and not res.errors
