"""-m gpu: KV prefix reuse on the product path (FlashCausalLM(kv_prefix_reuse=True)).

The yardstick of every logit is the fp32 CPU oracle run on the request's FULL token sequence (prompt + what was generated so
far), whatever part of it the product found in its cache: oracle/llama_ref.py, oracle/santacoder_ref.py, and for GPT-NeoX,
which oracle/ has no model of, transformers' GPTNeoXForCausalLM in fp32 (what the NeoX fixtures were drawn from).  The bars
are those of fresh prefills: tests/test_model_gpu.py's LOGIT_TOL (Llama, NeoX), its BigCode bar, tests/test_kv_fp8_model_gpu.py's
for the one-byte cache; ids go through check_ids with the same tie rule (none for f16)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import ops_ref
from oracle.llama_ref import LlamaRef
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors
from tests.fixture_utils import FixtureTokenizer, check_ids, prompt_text

pytestmark = pytest.mark.gpu

LOGIT_TOL = {torch.float16: 0.35, torch.bfloat16: 2.5}   # tests/test_model_gpu.py
BIGCODE_TOL = {torch.float16: 0.08, torch.bfloat16: 0.6}  # tests/test_model_gpu.py, Santacoder
FP8_TOL = {torch.float16: 1.4}                            # tests/test_kv_fp8_model_gpu.py
VOCAB = 256


def _rand(rng, n):
    """n random token ids.  (The seeds below are ones at which the ORACLE decides every token a test compares by more than
    twice the logit bar, as the golden fixtures are drawn: an id that differs is then an error, not a near-tie.)"""
    return rng.integers(3, VOCAB, size=n).tolist()


# ---- models and their oracles -----------------------------------------------------------------------------------------------
def _llama(quantize=None, dtype=torch.float16, pages=96, kv="auto", reuse=True):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    tcfg = TinyLlamaConfig()
    assert tcfg.vocab_size == VOCAB
    tensors = tiny_llama_tensors(tcfg, seed=7, quantize=quantize, groupsize=64, dtype=dtype)
    tok = FixtureTokenizer(tcfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, LlamaConfig(**tcfg.to_dict()), dtype, quantize,
                          tokenizer=tok, gptq_groupsize=64)
    lm = FlashCausalLM("fixture", None, "synthetic", dtype, quantize, engine=eng, kv_cache_pages=pages, kv_cache_dtype=kv,
                       kv_prefix_reuse=reuse)
    ref = LlamaRef(tcfg, tensors, quantize=quantize, groupsize=64)
    return lm, tok, (lambda seqs: ref.generate_greedy(seqs, 1)[0]["logits"].numpy()), ref


def _santacoder(dtype=torch.float16):
    from oracle.santacoder_ref import SantacoderRef
    from oracle.tiny_models import TinyBigCodeConfig, tiny_bigcode_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyBigCodeConfig()
    tensors = tiny_bigcode_tensors(cfg, seed=11)
    cfg.quantize = None
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, cfg, dtype, None, tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", dtype, None, engine=eng, kv_cache_pages=64, kv_prefix_reuse=True)
    ref = SantacoderRef(cfg, tensors)
    return lm, tok, (lambda seqs: ref.generate_greedy(seqs, 1)[0]["logits"].numpy())


def _neox(dtype=torch.float16):
    from transformers import GPTNeoXConfig as HFConfig, GPTNeoXForCausalLM

    from tests.neox_tiny import TinyNeoXConfig, tiny_neox_tensors
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_neox_modeling import GPTNeoXConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyNeoXConfig("A")  # head size 96, 24 rotary dims: the general rotary path of the writer
    tensors = tiny_neox_tensors(cfg, seed=11)
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.to(dtype) for k, v in tensors.items()}, GPTNeoXConfig(**cfg.hf_kwargs()), dtype, None,
                          tokenizer=tok)
    lm = FlashCausalLM("fixture", None, "synthetic", dtype, None, engine=eng, kv_cache_pages=64, kv_prefix_reuse=True)
    hf = GPTNeoXForCausalLM(HFConfig(**cfg.hf_kwargs()))
    sd = tensors
    if hasattr(hf, "lm_head"):  # transformers 5 names the checkpoint's embed_out `lm_head`
        sd = {("lm_head.weight" if k == "embed_out.weight" else k): v for k, v in tensors.items()}
    missing, unexpected = hf.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in m or "inv_freq" in m or "masked_bias" in m or ".attention.bias" in m
                                  for m in missing), (missing, unexpected)
    hf = hf.float().eval()

    def oracle(seqs):
        with torch.no_grad():
            return np.stack([hf(torch.tensor([s])).logits[0, -1].float().numpy() for s in seqs])

    return lm, tok, oracle


# ---- the driver ---------------------------------------------------------------------------------------------------------------
class Driver:
    """Runs requests through generate_token and holds every logit row against the oracle on the request's full sequence."""

    def __init__(self, lm, tok, oracle, dtype, tol, check_tokens=True):
        self.lm, self.tok, self.oracle, self.dtype, self.tol, self.check_tokens = lm, tok, oracle, dtype, tol, check_tokens
        self.seqs, self.rows, self.worst = {}, None, 0.0
        orig = lm._process_new_tokens

        def tapped(batch, out, *a, **kw):
            self.rows = out.detach().float().cpu().numpy().copy()
            return orig(batch, out, *a, **kw)

        lm._process_new_tokens = tapped

    def stats(self):
        return self.lm.kv_cache.reuse_stats()

    def batch(self, prompts, first_id, batch_id, max_new=12, input_toks=False, prefix_id=None, prefix_cache=None):
        from tgis_amd.pb import generate_pb2 as pb2

        reqs = []
        for i, p in enumerate(prompts):
            r = pb2.Request(id=first_id + i, inputs=prompt_text(p), input_length=len(p), truncate=False,
                            max_output_length=max_new)
            r.details.logprobs = True
            r.details.input_toks = input_toks
            if prefix_id:
                r.prefix_id = prefix_id
            reqs.append(r)
            self.seqs[first_id + i] = list(p)
        lm = self.lm
        with lm.context_manager():
            b, errs = lm.batch_type.from_pb(pb2.Batch(id=batch_id, requests=reqs), self.tok, lm.dtype, lm.device,
                                            lm.word_embeddings, prefix_cache, True)
        assert not errs
        return b

    def step(self, batch, what, first=False, check=True):
        with self.lm.context_manager():
            toks, in_toks, errs, _ = self.lm.generate_token(batch, first=first, for_concat=first)
        assert not errs
        rows = self.rows if self.rows.shape[0] == len(toks) else None  # (all-position logits: checked by the caller)
        if check and rows is not None:
            want = self.oracle([self.seqs[t.request_id] for t in toks])
            err = float(np.abs(rows - want).max())
            self.worst = max(self.worst, err)
            print(f"{what}: max |logit - oracle| = {err:.4f} (bar {self.tol})")
            assert err <= self.tol, f"{what}: max |logit - oracle| = {err:.4f} > {self.tol}"
            if self.check_tokens:
                check_ids([t.token_id for t in toks], {"logits": want, "ids": want.argmax(-1)}, what,
                          tie_margin=None if self.dtype == torch.float16 else 2 * self.tol)
        for t in toks:
            self.seqs[t.request_id].append(t.token_id)
        return toks, in_toks

    def prefill(self, prompts, first_id, batch_id, what, **kw):
        b = self.batch(prompts, first_id, batch_id, **kw)
        self.step(b, f"{what} prefill", first=True)
        return b

    def decode(self, batch, n, what):
        for i in range(n):
            self.step(batch, f"{what} decode {i}")


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _scenario_ab(d, rng):
    """A (70 tokens) prefilled and decoded; B = A's first 64 tokens + 10 others hits A's two full pages; both decode side by
    side; A leaves, B goes on, B leaves; C with the same header still hits the two pages, now from the LRU."""
    lm, cache = d.lm, d.lm.kv_cache
    A = _rand(rng, 70)
    B, C = A[:64] + _rand(rng, 10), A[:64] + _rand(rng, 5)
    a = d.prefill([A], 0, 1, "A")
    assert a.reused_lengths == [0] and d.stats()["registered"] == 2
    d.decode(a, 3, "A")
    s0 = d.stats()
    b = d.prefill([B], 1, 2, "B")
    got = _delta(d.stats(), s0)
    assert got["lookups"] == 1 and got["hit_pages"] == 2 and got["looked_up_pages"] == 2, got
    assert b.reused_lengths == [64] and b.pages[0][:2] == a.pages[0][:2] and b.pages[0][2] not in a.pages[0]
    assert b.block_tables[0, :2].tolist() == a.block_tables[0, :2].tolist()
    assert b.cu_seqlens.tolist() == [0, 75], "the logical slot contract counts the whole prompt"
    d.decode(b, 3, "B")
    with lm.context_manager():
        merged = lm.batch_type.concatenate([a, b])
    d.decode(merged, 3, "A+B")           # (one-token writes of both next to the shared pages)
    shared = merged.pages[0][:2]
    with lm.context_manager():
        merged = lm.batch_type.prune(merged, [0])
    assert all(cache._refs[p] == 1 for p in shared), "B still holds the pages A shared with it"
    d.decode(merged, 2, "B after A left")
    with lm.context_manager():
        assert lm.batch_type.prune(merged, [1]) is None
    assert cache.free_pages == cache.num_pages
    s0 = d.stats()
    c = d.prefill([C], 2, 3, "C")
    assert _delta(d.stats(), s0)["hit_pages"] == 2 and c.pages[0][:2] == shared
    d.decode(c, 1, "C")
    c.release()
    assert cache.free_pages == cache.num_pages


@pytest.mark.parametrize("family,quantize,dtype", [("llama", None, torch.float16), ("llama", "gptq", torch.float16),
                                                   ("llama", None, torch.bfloat16), ("neox", None, torch.float16),
                                                   ("santacoder", None, torch.float16)],
                         ids=["llama-dense-f16", "llama-gptq-f16", "llama-dense-bf16", "neox-partial-rotary-f16",
                              "santacoder-mqa-no-rotary-f16"])
def test_a_request_behind_a_shared_header_matches_the_oracle(gpu_device, family, quantize, dtype):
    if family == "llama":
        lm, tok, oracle, _ = _llama(quantize, dtype)
        tol = LOGIT_TOL[dtype]
    elif family == "neox":
        lm, tok, oracle = _neox(dtype)
        tol = LOGIT_TOL[dtype]
    else:
        lm, tok, oracle = _santacoder(dtype)
        tol = BIGCODE_TOL[dtype]
    _scenario_ab(Driver(lm, tok, oracle, dtype, tol), np.random.default_rng(31))


def test_fp8_cache_behind_a_shared_header_matches_the_quantised_kv_oracle(gpu_device, monkeypatch):
    """The one-byte cache: B attends over A's e4m3 codes.  The oracle's K / V pass through the quantiser, as in
    tests/test_kv_fp8_model_gpu.py (scales 1), and its bar holds; ids are not held against a lossy cache there either."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import kv_fp8_ref as q8

    lm, tok, oracle, _ = _llama(None, torch.float16, kv="fp8_e4m3")
    assert lm.kv_cache.is_fp8 and lm.kv_cache.prefix_reuse
    orig = ops_ref.attention_varlen

    def attn(q, k, v, cu_q, cu_k, scale):
        k8 = q8.dequantize(q8.quantize(k.to(torch.float16)))
        v8 = q8.dequantize(q8.quantize(v.to(torch.float16)))
        return orig(q, k8, v8, cu_q, cu_k, scale)

    monkeypatch.setattr(ops_ref, "attention_varlen", attn)
    _scenario_ab(Driver(lm, tok, oracle, torch.float16, FP8_TOL[torch.float16], check_tokens=False),
                 np.random.default_rng(31))


# ---- one dense f16 Llama for the cases below --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def llama(gpu_device):
    lm, tok, oracle, ref = _llama(None, torch.float16)
    d = Driver(lm, tok, oracle, torch.float16, LOGIT_TOL[torch.float16])
    d.ref = ref
    return d


def _register(d, prompt, rid, bid):
    """One request that leaves its full prompt pages in the index and goes."""
    b = d.prefill([prompt], rid, bid, f"header request {rid}")
    b.release()
    assert d.lm.kv_cache.free_pages == d.lm.kv_cache.num_pages


def test_a_prompt_equal_to_a_registered_one_still_computes_its_last_page(llama):
    d, rng = llama, np.random.default_rng(41)
    P = _rand(rng, 64)
    _register(d, P + _rand(rng, 6), 100, 100)
    s0 = d.stats()
    b = d.prefill([P], 101, 101, "64 tokens, all registered")
    assert _delta(d.stats(), s0)["hit_pages"] == 1 and b.reused_lengths == [32]
    d.decode(b, 2, "64 tokens")
    b.release()


def test_short_suffixes_over_a_long_header_and_a_long_suffix_next_to_a_miss(llama):
    """1-3 tokens over 96 cached ones are the decode forms of the attention (q > 1, and q = 1 with the key splits
    attn_num_splits returns); a 40-token suffix beside a miss is its prefill form."""
    d, rng = llama, np.random.default_rng(1013)
    H = _rand(rng, 96)
    _register(d, H + _rand(rng, 3), 110, 110)
    s0 = d.stats()
    b = d.prefill([H + _rand(rng, n) for n in (1, 2, 3)], 111, 111, "suffixes 1, 2, 3")
    assert b.reused_lengths == [96, 96, 96] and _delta(d.stats(), s0)["hit_pages"] == 9
    d.decode(b, 2, "suffixes 1, 2, 3")
    b.release()
    b = d.prefill([H + _rand(rng, 1), H[:64] + _rand(rng, 1)], 115, 112, "suffixes 1, 1")
    assert b.reused_lengths == [96, 64]
    d.decode(b, 2, "suffixes 1, 1")
    b.release()
    b = d.prefill([H + _rand(rng, 40), _rand(rng, 50)], 120, 113, "suffix 40 + miss 50")
    assert b.reused_lengths == [96, 0]
    d.decode(b, 2, "suffix 40 + miss 50")
    b.release()
    assert d.lm.kv_cache.free_pages == d.lm.kv_cache.num_pages


def test_input_token_details_switch_the_lookup_off_for_the_batch(llama):
    d, rng = llama, np.random.default_rng(47)
    P = _rand(rng, 70)
    _register(d, P, 130, 130)
    s0 = d.stats()
    Q = P[:32] + _rand(rng, 41)   # its first page is in the index (a lookup would hit it), its second is new content
    b = d.batch([Q], 131, 131, input_toks=True)
    toks, in_toks = d.step(b, "input_toks", first=True, check=False)
    got = _delta(d.stats(), s0)
    assert got["lookups"] == 0 and got["hit_pages"] == 0 and b.reused_lengths == [0]
    assert d.rows.shape[0] == len(Q), "every prompt position's logits were computed"
    (info,) = in_toks
    assert len(info.tokens) == len(Q) and [t.token_id for t in info.tokens] == Q
    # all-position oracle logits: row i predicts token i + 1
    state = d.ref.new_state(1)
    want = d.ref.forward(torch.tensor(Q), torch.arange(len(Q)), [0] * len(Q), state).float()
    err = float((torch.from_numpy(d.rows) - want).abs().max())
    print(f"input_toks: max |logit - oracle| over all positions = {err:.4f}")
    assert err <= d.tol
    lp = torch.log_softmax(want, -1)[torch.arange(len(Q) - 1), torch.tensor(Q[1:])]
    np.testing.assert_allclose([t.logprob for t in info.tokens[1:]], lp.numpy(), atol=d.tol)
    assert got["registered"] == 1, "the batch registers afterwards all the same: its second page was new content"
    b.release()


def test_a_prompt_tuning_prefix_bypasses_lookup_and_registers_nothing(llama, tmp_path):
    from tgis_amd.prompt_cache import PrefixCache

    d, rng = llama, np.random.default_rng(53)
    cfg = TinyLlamaConfig()
    (tmp_path / "soft").mkdir()
    torch.save(torch.randn(3, cfg.hidden_size), tmp_path / "soft" / "decoder.pt")
    pc = PrefixCache(d.lm.device, d.lm.dtype, max_length=16, hidden_size=cfg.hidden_size, store=tmp_path, budget_mb=8)
    s0 = d.stats()
    b = d.batch([_rand(rng, 70)], 140, 140, prefix_id="soft", prefix_cache=pc)
    assert b.input_lengths == [73] and b.inputs_embeds is not None  # 3 prefix rows + 70 tokens
    d.step(b, "prefix_id", first=True, check=False)
    assert b.input_lengths == [74] and b.reused_lengths == [0]       # (one more: the token just generated)
    assert _delta(d.stats(), s0) == dict.fromkeys(s0, 0), "a prompt-tuning batch looked up or registered"
    b.release()
    assert d.lm.kv_cache.free_pages == d.lm.kv_cache.num_pages


def test_an_evicted_header_misses_and_is_computed_again(gpu_device):
    lm, tok, oracle, _ = _llama(None, torch.float16, pages=8)
    d, rng = Driver(lm, tok, oracle, torch.float16, LOGIT_TOL[torch.float16]), np.random.default_rng(59)
    H = _rand(rng, 70)
    _register(d, H, 0, 0)                      # 2 cached pages, 6 on the heap
    s0 = d.stats()
    b = d.prefill([H[:64] + _rand(rng, 3)], 1, 1, "hit before eviction")
    assert _delta(d.stats(), s0)["hit_pages"] == 2
    b.release()
    b = d.prefill([_rand(rng, 100), _rand(rng, 100)], 2, 2, "the pool filled by others")  # 2 x 4 pages: all 8
    assert d.stats()["evictions"] >= 2 and lm.kv_cache.free_pages == 0
    b.release()
    s0 = d.stats()
    b = d.prefill([H[:64] + _rand(rng, 4)], 4, 3, "miss after eviction")
    got = _delta(d.stats(), s0)
    assert got["hit_pages"] == 0 and got["lookups"] == 1 and b.reused_lengths == [0]
    d.decode(b, 2, "miss after eviction")
    b.release()
    assert lm.kv_cache.free_pages == lm.kv_cache.num_pages


def test_reuse_off_counts_nothing(gpu_device):
    lm, tok, oracle, _ = _llama(None, torch.float16, reuse=False)
    d, rng = Driver(lm, tok, oracle, torch.float16, LOGIT_TOL[torch.float16]), np.random.default_rng(61)
    P = _rand(rng, 70)
    _register(d, P, 0, 0)
    b = d.prefill([P[:64] + _rand(rng, 5)], 1, 1, "reuse off")
    assert b.reused_lengths == [0] and d.stats() == dict.fromkeys(d.stats(), 0) and not lm.kv_prefix_reuse
    b.release()


# ---- tensor parallel: two ranks on one GPU, as tests/test_tp_gpu.py sets them up -----------------------------------------
TP_SEED = 67


def _tp_prompts():
    rng = np.random.default_rng(TP_SEED)
    A = _rand(rng, 70)
    return A, A[:64] + _rand(rng, 10)


def _tp_worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1", TGIS_KV_PREFIX_REUSE="true",
                      TGIS_DIST_TIMEOUT_S="60")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.pb import generate_pb2 as pb2

    cfg = TinyLlamaConfig(intermediate_size=512)
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tiny_llama_tensors(cfg, seed=21, quantize=None, groupsize=64), LlamaConfig(**cfg.to_dict()),
                          torch.float16, None, tokenizer=tok, gptq_groupsize=64)
    lm = FlashCausalLM("tp", None, "synthetic", torch.float16, None, engine=eng, kv_cache_pages=32)
    assert lm.kv_prefix_reuse
    rows = {}
    orig = lm._process_new_tokens

    def tapped(batch, out, *a, **kw):
        rows["logits"] = out.detach().float().cpu().numpy().copy()
        return orig(batch, out, *a, **kw)

    lm._process_new_tokens = tapped
    out = {"ids": [], "logits": [], "hits": []}
    with lm.context_manager():
        for rid, prompt in enumerate(_tp_prompts()):
            req = pb2.Request(id=rid, inputs=prompt_text(prompt), input_length=len(prompt), truncate=False,
                              max_output_length=6)
            b, errs = lm.batch_type.from_pb(pb2.Batch(id=rid, requests=[req]), tok, lm.dtype, lm.device, lm.word_embeddings,
                                            None, True)
            assert not errs
            for i in range(3):
                toks, _, errs, _ = lm.generate_token(b, first=(i == 0))
                assert not errs
                out["ids"].append(toks[0].token_id)
                out["logits"].append(rows["logits"])
            out["hits"].append((list(b.reused_lengths), b.pages[0][:2], lm.kv_cache.reuse_stats()))
            if rid == 1:
                b.release()
            else:
                keep = b  # A stays alive while B maps its pages
        keep.release()
    ret[rank] = out
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_tp2_ranks_map_the_same_pages_and_match_the_oracle(gpu_device):
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        from tests.test_tp_gpu import _free_port

        port = _free_port()
        procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, ret)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(150)
        hung = [r for r, p in enumerate(procs) if p.is_alive()]
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
        assert not hung, f"ranks {hung} did not finish"
        assert [p.exitcode for p in procs] == [0, 0]
        r0, r1 = ret[0], ret[1]
    assert r0["hits"] == r1["hits"] and r0["ids"] == r1["ids"], "the ranks' indexes went apart"
    assert r0["hits"][0][0] == [0] and r0["hits"][1][0] == [64] and r0["hits"][1][2]["hit_pages"] == 2
    assert r0["hits"][0][1] == r0["hits"][1][1]
    cfg = TinyLlamaConfig(intermediate_size=512)
    ref = LlamaRef(cfg, tiny_llama_tensors(cfg, seed=21, quantize=None, groupsize=64), quantize=None, groupsize=64)
    tol, k = LOGIT_TOL[torch.float16], 0
    for prompt in _tp_prompts():
        seq = list(prompt)
        for i in range(3):
            want = ref.generate_greedy([seq], 1)[0]["logits"].numpy()
            err = float(np.abs(r0["logits"][k] - want).max())
            print(f"tp2 request {k // 3} step {i}: max |logit - oracle| = {err:.4f}")
            assert err <= tol, f"request {k // 3} step {i}: {err:.4f} > {tol}"
            check_ids([r0["ids"][k]], {"logits": want, "ids": want.argmax(-1)}, f"tp2 request {k // 3} step {i}")
            seq.append(r0["ids"][k])
            k += 1
