"""The 8-bit GPTQ decode GEMM next to its two neighbours, and one cfg3 decode step of an 8-bit Llama-2-7B.

Per cfg3 projection (K x N, group size 128) and M in {1, 32, 64}: the median over --reps launches, each bracketed by its
own pair of HIP events after --warm untimed ones, of (a) tgis_gptq8_gemm_f16, (b) tgis_gptq_gemm_f16 on an int4 weight of
the same shape, (c) tgis_dense_gemm on an f16 weight of the same shape — all in one process on one device — and the fraction
of 8 TB/s that (a) reaches on K N + groups N 4 bytes.  Then the step: a synthetic 8-bit Llama-2-7B (B 32, ctx 1024) through
the synthetic InferenceEngine(gptq_bits=8), median of three blocks of --steps decode steps, wall clock around a device
synchronize.  One JSON line per measurement.

    python tools/gptq8_bench.py [--reps 200] [--skip-step] > profiles/NAME.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "text-generation-inference_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
from tgis_amd import native  # noqa: E402
from tgis_amd.inference_engine.synthetic import InferenceEngine, llama_tensors  # noqa: E402
from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig  # noqa: E402
from tgis_amd.models.flash_causal_lm import FlashCausalLM  # noqa: E402
from tgis_amd.testing import SyntheticTokenizer, make_batch_pb  # noqa: E402
from tgis_amd.utils.kv_cache import PagedKVCache  # noqa: E402

SHAPES = [("qkv", 4096, 12288), ("o", 4096, 4096), ("gate_up", 4096, 22016), ("down", 11008, 4096)]
GS = 128
HBM = 8.0e12


def median_us(fn, warm, reps):
    for _ in range(warm):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in evs) * 1e3


def weights(K, N, dev):
    g = torch.Generator(device=dev).manual_seed(K + N)
    G = K // GS

    def ints(*shape):
        return torch.randint(-2**31, 2**31 - 1, shape, generator=g, device=dev, dtype=torch.int32)

    s = (torch.rand((G, N), generator=g, device=dev) * 1e-3 + 1e-3).half()
    w8 = native.Gptq8Weight(ints(K // 4, N), ints(G, N // 4), s, None, 8, GS)
    w4 = native.GptqWeight(ints(K // 8, N), ints(G, N // 8), s, None, 4, GS)
    wd = native.DenseWeight((torch.randn((N, K), generator=g, device=dev) * 0.02).half())
    return w8, w4, wd


def projections(args, dev):
    ws = native.Workspace(64 << 20, dev)
    for name, K, N in SHAPES:
        w8, w4, wd = weights(K, N, dev)
        for M in (1, 32, 64):
            x = (torch.randn((M, K), device=dev) * 0.1).half()
            o = torch.empty((M, N), dtype=torch.float16, device=dev)
            t8 = median_us(lambda: native.gptq8_gemm(x, w8, ws, out=o), args.warm, args.reps)
            t4 = median_us(lambda: native.gptq_gemm(x, w4, ws, out=o), args.warm, args.reps)
            td = median_us(lambda: native.dense_gemm(x, wd, ws, out=o), args.warm, args.reps)
            nbytes = K * N + (K // GS) * N * 4
            print(json.dumps({"proj": name, "K": K, "N": N, "M": M, "gptq8_us": round(t8, 2), "gptq4_us": round(t4, 2),
                              "dense_f16_us": round(td, 2), "gptq8_bytes": nbytes,
                              "gptq8_fraction_of_8TBs": round(nbytes / (t8 * 1e-6) / HBM, 3),
                              "gptq8_over_dense": round(t8 / td, 3)}), flush=True)
        del w8, w4, wd
        torch.cuda.empty_cache()


def step(args, dev):
    kw, quantize, dtype_s, B, ctx = bench.CONFIGS["llama2-7b-gptq"]
    cfg = LlamaConfig(**kw)
    tensors = llama_tensors(cfg, "gptq", seed=1234, device=dev, dtype=torch.float16, bits=8)
    tok = SyntheticTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, cfg, torch.float16, "gptq", tokenizer=tok, gptq_bits=8)
    del tensors
    K, W = args.steps, 10
    L_in = max(1, ctx - W - K // 2 - 1)
    lm = FlashCausalLM("synthetic", None, "synthetic", torch.float16, "gptq", engine=eng,
                       kv_cache_pages=B * PagedKVCache.pages_for(L_in + W + K + 8) + 8)
    torch.cuda.empty_cache()
    blocks = []
    with lm.context_manager():
        for _ in range(3):
            batch, errs = lm.batch_type.from_pb(make_batch_pb([L_in] * B, max_new=W + K + 8), tok, lm.dtype, lm.device,
                                                lm.word_embeddings, None, True)
            assert not errs
            lm.generate_token(batch, first=True)
            for _ in range(W):
                lm.generate_token(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                lm.generate_token(batch)
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) / K * 1e3)
            batch.release()
    print(json.dumps({"step": "llama2-7b gptq 8-bit", "B": B, "ctx": ctx, "steps": K, "graphs": bool(lm.use_graphs),
                      "ms_per_step": round(statistics.median(blocks), 4), "ms_per_step_blocks": [round(b, 4) for b in blocks]}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-projections", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    native.load_library()
    if not args.skip_projections:
        projections(args, dev)
    if not args.skip_step:
        step(args, dev)


if __name__ == "__main__":
    main()
