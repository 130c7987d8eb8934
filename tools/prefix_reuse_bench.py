"""Prefill time with and without KV prefix reuse (utils/kv_cache.py) on the synthetic cfg3 engine, built as bench.py builds it.

One warm request registers a shared header of S tokens; then B requests whose prompts share those S tokens and differ in
their last T - S are prefilled, device sync on both sides of generate_token(first=True).  Median of --runs runs (one
untimed run in front), reuse off and reuse on, one JSON line per (B, T, S).

    python tools/prefix_reuse_bench.py [--runs 5] [--config llama2-7b-gptq] > profiles/NAME.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "text-generation-inference_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from tgis_amd import native  # noqa: E402
from tgis_amd.inference_engine.synthetic import InferenceEngine, llama_tensors  # noqa: E402
from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig  # noqa: E402
from tgis_amd.models.flash_causal_lm import FlashCausalLM  # noqa: E402
from tgis_amd.pb import generate_pb2  # noqa: E402
from tgis_amd.utils.kv_cache import PagedKVCache  # noqa: E402

CASES = [(1, 1024, 992), (8, 1024, 896), (8, 1024, 512)]


class IdTokenizer:
    """'t17 t203' -> [17, 203]: prompts are given as the ids themselves, so that two of them can share a prefix."""

    def __init__(self, vocab_size):
        self.vocab_size, self.pad_token_id, self.bos_token_id, self.eos_token_id = vocab_size, 0, 1, 2
        self.add_bos_token = False

    def __call__(self, texts, truncation=True, max_length=None, return_token_type_ids=False, **kw):
        return {"input_ids": [[int(w[1:]) for w in t.split()] for t in texts]}


def batch_pb(prompts, batch_id, first_id):
    reqs = [generate_pb2.Request(id=first_id + i, inputs=" ".join(f"t{t}" for t in p), input_length=len(p), truncate=False,
                                 max_output_length=4) for i, p in enumerate(prompts)]
    return generate_pb2.Batch(id=batch_id, requests=reqs)


def prefill_ms(lm, tok, prompts, batch_id):
    batch, errs = lm.batch_type.from_pb(batch_pb(prompts, batch_id, 0), tok, lm.dtype, lm.device, lm.word_embeddings, None,
                                        True)
    assert not errs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lm.generate_token(batch, first=True)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    reused = list(batch.reused_lengths)
    batch.release()
    return ms, reused


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="llama2-7b-gptq", choices=sorted(bench.CONFIGS))
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    assert args.runs >= 5, "median of at least 5 runs"
    kw, quantize, dtype_s, _, _ = bench.CONFIGS[args.config]
    cfg, dtype, dev = LlamaConfig(**kw), getattr(torch, dtype_s), torch.device("cuda:0")
    tensors = llama_tensors(cfg, quantize, seed=1234, device=dev, dtype=dtype)
    tok = IdTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, cfg, dtype, quantize, tokenizer=tok)
    del tensors
    pages = 2 * max(B * PagedKVCache.pages_for(T + 8) for B, T, _ in CASES) + 64
    # the two models share the engine's weights; each has its own page pool
    lms = {reuse: FlashCausalLM("synthetic", None, "synthetic", dtype, quantize, engine=eng, kv_cache_pages=pages,
                                kv_prefix_reuse=reuse) for reuse in (False, True)}
    rng = np.random.default_rng(2024)
    draw = (lambda n: rng.integers(3, cfg.vocab_size, size=n).tolist())
    H, Hkv = lms[True].num_heads, lms[True].num_kv_heads
    for B, T, S in CASES:
        header = draw(S)
        res = {"config": args.config, "B": B, "T": T, "S": S, "runs": args.runs}
        for reuse, lm in lms.items():
            with lm.context_manager():
                prefill_ms(lm, tok, [header + draw(1)], 0)  # the warm request: registers the header's S / 32 pages
                times = []
                for run in range(args.runs + 1):
                    ms, reused = prefill_ms(lm, tok, [header + draw(T - S) for _ in range(B)], run + 1)
                    assert reused == [S if reuse else 0] * B, reused
                    times.append(ms)
            key = "hit" if reuse else "miss"
            res[f"{key}_ms"] = round(statistics.median(times[1:]), 3)
            res[f"{key}_ms_all"] = [round(t, 3) for t in times[1:]]
        q = T - S
        res["ratio_miss_over_hit"] = round(res["miss_ms"] / res["hit_ms"], 2)
        res["hit_attention"] = {"max_q_len": q, "max_ctx": T, "num_splits": native.attn_num_splits(B, Hkv, H, q, T),
                                "form": "prefill" if q * max(1, H // Hkv) > 64 else "decode, q > 1"}
        res["reuse_stats"] = lms[True].kv_cache.reuse_stats()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
