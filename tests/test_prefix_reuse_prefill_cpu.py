"""CPU: the prefill behind a reused prefix (FlashCausalLM._prefill_forward -> _prefill_suffix_forward) with the kernels replaced
by the oracle through tests/cpu_backend.py, as tests/test_tp_gloo.py runs the model: what is under test is the host side —
which tokens, positions, slots, cu_seqlens_q, ctx_lens and head rows a hit batch feeds the model, and that the logical
bookkeeping of the batch stays the whole prompt's.  The GPU twin is tests/test_prefix_reuse_model_gpu.py."""
import numpy as np
import pytest
import torch

from oracle.llama_ref import LlamaRef
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests import cpu_backend
from tests.fixture_utils import FixtureTokenizer, prompt_text

CPU = torch.device("cpu")
TOL = 0.5  # tests/test_tp_gloo.py's bar for this stand-in backend (activations rounded to f16 between ops, logits ~ 60)


def _prefill_at(qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, max_len, H, Hkv, D, rot_dim, past_lens):
    # by contract the per-token kernel with slot(b, i) = block_tables[b][(past + i) // 32] * 32 + (past + i) % 32
    cu, past = [int(v) for v in cu_seqlens], [int(v) for v in past_lens]
    assert all(p % 32 == 0 for p in past) and max(cu[b + 1] - cu[b] for b in range(len(past))) == max_len
    slots = torch.tensor([int(block_tables[b, (past[b] + i) // 32]) * 32 + (past[b] + i) % 32
                          for b in range(len(past)) for i in range(cu[b + 1] - cu[b])], dtype=torch.int32)
    return cpu_backend._rope_kv_write(qkv, cos, sin, positions, slots, k_pool, v_pool, H, Hkv, D, rot_dim)


@pytest.fixture
def lm(monkeypatch):
    from tgis_amd import native
    from tgis_amd.models.custom_modeling.flash_llama_modeling import FlashLlamaForCausalLM, LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.kv_cache import PagedKVCache
    from tgis_amd.utils.weights import DictWeights

    cpu_backend.install(monkeypatch)
    calls = []
    monkeypatch.setattr(native, "rope_kv_write_prefill_at", lambda *a: calls.append(a) or _prefill_at(*a))
    cfg = TinyLlamaConfig()
    tensors = tiny_llama_tensors(cfg, seed=7, quantize=None, groupsize=64)
    pcfg = LlamaConfig(**cfg.to_dict())
    pcfg.quantize = None
    model = FlashLlamaForCausalLM(pcfg, DictWeights(tensors, CPU, torch.float16, FakeGroup(0, 1)))
    attn = model.model.layers[0].self_attn
    lm = FlashCausalLM.__new__(FlashCausalLM)  # the prefill's host code without the GPU-only constructor
    lm.model, lm.device, lm.kv_prefix_reuse = model, CPU, True
    lm.num_heads, lm.num_kv_heads = attn.num_heads, attn.num_key_value_heads
    lm.kv_cache = PagedKVCache(cfg.num_hidden_layers, attn.num_key_value_heads, attn.head_size, 16, torch.float16, CPU,
                               prefix_reuse=True)
    lm.at_calls = calls
    lm.ref = LlamaRef(cfg, tensors, quantize=None, groupsize=64)
    return lm


def _batch(prompts, first_id=0, batch_id=0):
    from tgis_amd.models.flash_causal_lm import FlashCausalLMBatch
    from tgis_amd.pb import generate_pb2 as pb2

    reqs = [pb2.Request(id=first_id + i, inputs=prompt_text(p), input_length=len(p), max_output_length=4)
            for i, p in enumerate(prompts)]
    b, errs = FlashCausalLMBatch.from_pb(pb2.Batch(id=batch_id, requests=reqs), FixtureTokenizer(256), torch.float16, CPU,
                                         None, None, True)
    assert not errs
    return b


def _check(lm, out, prompts, what):
    want = lm.ref.generate_greedy(prompts, 1)[0]
    err = float((out.float() - want["logits"]).abs().max())
    assert out.shape == want["logits"].shape and err < TOL, f"{what}: max |logit - oracle| = {err:.3f}"
    assert out.argmax(-1).tolist() == want["token_ids"].tolist(), what


def test_a_hit_batch_feeds_only_the_suffix_and_matches_the_oracle(lm):
    rng = np.random.default_rng(31)
    draw = (lambda n: rng.integers(3, 256, size=n).tolist())
    A = draw(70)
    a = _batch([A], 0, 1)
    _check(lm, lm._prefill_forward(a), [A], "A, fresh")
    assert not lm.at_calls and a.reused_lengths == [0] and lm.kv_cache.reuse_stats()["registered"] == 2
    # one request behind A's two pages, one behind its first only, one miss: suffixes of 10, 40 and 50 tokens
    prompts = [A[:64] + draw(10), A[:32] + draw(40), draw(50)]
    b = _batch(prompts, 1, 2)
    cu_before, pos_before = b.cu_seqlens.clone(), b.position_ids.clone()
    out = lm._prefill_forward(b)
    assert b.reused_lengths == [64, 32, 0] and b.pages[0][:2] == a.pages[0][:2] and b.pages[1][:1] == a.pages[0][:1]
    _check(lm, out, prompts, "B, behind A's pages")
    # what the layers' writer was given: the suffix tokens only, at their true positions
    assert len(lm.at_calls) == 2  # one per layer
    qkv, _cos, _sin, positions, cu_q, bt, _k, _v, max_len, *_rest, past = lm.at_calls[0]
    assert qkv.shape[0] == 10 + 40 + 50 and cu_q.tolist() == [0, 10, 50, 100] and max_len == 50
    assert positions.tolist() == list(range(64, 74)) + list(range(32, 72)) + list(range(50))
    assert past.tolist() == [64, 32, 0] and past.dtype == torch.int32 and bt is b.block_tables
    # the reference's logical contract is the whole prompt's
    assert torch.equal(b.cu_seqlens, cu_before) and b.cu_seqlens.tolist() == [0, 74, 146, 196]
    assert torch.equal(b.position_ids, pos_before) and b.prompt_token_ids is None
    # A's pages were read, never written: its own continuation still matches the oracle on them
    store = cpu_backend._POOLS[lm.kv_cache.k_pool(0).data_ptr()]
    assert all(p * 32 + o in store for p in a.pages[0][:2] for o in range(32))
    for x in (a, b):
        x.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages
    # a third request finds the header in the LRU; its single new token is the decode-sized forward
    c = _batch([A[:64] + draw(1)], 9, 3)
    _check(lm, lm._prefill_forward(c), [c.all_input_ids_tensor[0, :65].tolist()], "C, one token behind the header")
    assert c.reused_lengths == [64]
    c.release()


def test_reuse_off_takes_the_fresh_path(lm, monkeypatch):
    from tgis_amd.utils.kv_cache import PagedKVCache

    old = lm.kv_cache
    lm.kv_cache = PagedKVCache(old.num_layers, old.num_kv_heads, old.head_dim, 16, torch.float16, CPU)
    lm.kv_prefix_reuse = False
    rng = np.random.default_rng(37)
    A = rng.integers(3, 256, size=70).tolist()
    for i in range(2):
        b = _batch([A], i, i)
        _check(lm, lm._prefill_forward(b), [A], f"run {i}")
        assert b.reused_lengths == [0] and b.pages == [[0, 1, 2]]
        b.release()
    assert not lm.at_calls and lm.kv_cache.reuse_stats() == dict.fromkeys(lm.kv_cache.reuse_stats(), 0)
