"""Qwen3-8B decode on one MI355X: synthetic weights at the real layer shapes (hidden 4096, 32 heads on 8 KV heads, head_dim 128,
I 12288, vocab 151936) with --layers layers (default 8; the full model has 36), f16 and int4 GPTQ (group size 128), B in
{1, 8, 32}, mean context 1024.  One JSON line per measurement (keep them under profiles/):

  {"kind": "step", "variant": ...}  ms per decode step (median of timed blocks, synchronised on both sides) of three models of
        the same shapes and weights: "qwen3" (q / k norm inside the rope + cache-write launch), "llama" (no norm; the qkv GEMM +
        rope launch where the linear's rule chooses it) and "llama-unfused" (TGIS_FUSED_ROPE_GEMM off: the launches of qwen3
        without the norm)
  {"kind": "launch", "form": "per-token"}  tgis_rope_kv_write_qknorm alone next to tgis_rope_kv_write_partial on the same
        split-K slabs (the qkv GEMM's own, at B rows), and their ratio
  {"kind": "launch", "form": "page-wise"}  tgis_rope_kv_write_prefill_qknorm next to tgis_rope_kv_write_prefill on one
        4096-token prefill, and their ratio

Every comparison runs in this one process on one device, after a warm-up, as medians.

    python tools/bench_qwen.py [--layers 8 --steps 32 --warmup 3 --blocks 3 --quantize none,gptq --batches 1,8,32]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "text-generation-inference_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

E, H, HKV, D, INTER, VOCAB, EPS = 4096, 32, 8, 128, 12288, 151936, 1e-6
PREFILL_TOKENS = 4096


def timed_ms(fn, iters, rounds=5):
    """Median over `rounds` of the mean ms of `iters` back-to-back calls, between events on the current stream."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def build(variant, layers, quantize, device, pages):
    """FlashCausalLM of the Qwen3-8B layer shapes: as model_type qwen3, or the same tensors as a llama."""
    from tgis_amd.inference_engine.synthetic import InferenceEngine, llama_tensors
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer
    from tgis_amd.utils import layers as layers_mod

    layers_mod.FUSED_ROPE_GEMM = variant != "llama-unfused"
    cfg = LlamaConfig(vocab_size=VOCAB, hidden_size=E, intermediate_size=INTER, num_hidden_layers=layers,
                      num_attention_heads=H, num_key_value_heads=HKV, rms_norm_eps=EPS, rope_theta=1000000.0,
                      max_position_embeddings=40960, head_dim=D)
    cfg.model_type = "qwen3" if variant == "qwen3" else "llama"
    tensors = llama_tensors(cfg, quantize, seed=1234, device=device, dtype=torch.float16)
    g = torch.Generator(device=device).manual_seed(99)
    for i in range(layers):
        for n in ("q_norm", "k_norm"):
            tensors[f"model.layers.{i}.self_attn.{n}.weight"] = (0.5 + 1.5 * torch.rand(D, generator=g, device=device)).half()
    tok = SyntheticTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, cfg, torch.float16, quantize, tokenizer=tok, gptq_groupsize=128)
    tensors.clear()
    lm = FlashCausalLM("synthetic", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=pages)
    torch.cuda.empty_cache()
    return lm, tok


def step_ms(lm, tok, B, L_in, W, K, blocks):
    from tgis_amd.testing import make_batch_pb

    out = []
    with lm.context_manager():
        batch = None
        for _ in range(blocks):
            if batch is not None:
                batch.release()
            batch, errs = lm.batch_type.from_pb(make_batch_pb([L_in] * B, max_new=W + K + 10), tok, lm.dtype, lm.device,
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
            out.append((time.perf_counter() - t0) * 1e3 / K)
        batch.release()
    return out


def launches_alone(lm, quantize, batches, device):
    """The two norm + rope launches next to the plain ones on the same inputs."""
    from tgis_amd import native

    att = lm.model.model.layers[0].self_attn
    g = torch.Generator(device=device).manual_seed(5)
    cos, sin = lm.model.model.rope_tables(torch.float16, device, PREFILL_TOKENS)
    pages = PREFILL_TOKENS // 32
    kp, vp = (torch.zeros((pages, HKV, 32 * D), dtype=torch.float16, device=device) for _ in range(2))
    for B in batches:
        x = torch.randn((B, E), generator=g, device=device).half()
        qkv = att.query_key_value(x, partial=True)
        pos = torch.full((B,), 1024, dtype=torch.int32, device=device)
        slots = (torch.arange(B, dtype=torch.int32, device=device) * 32 + 7)
        tail = (cos, sin, pos, slots, kp, vp, H, HKV, D, D)
        plain = timed_ms(lambda: native.rope_kv_write(qkv, *tail), 50)
        normed = timed_ms(lambda: native.rope_kv_write(qkv, *tail, qk_norm=att.qk_norm), 50)
        print(json.dumps({"kind": "launch", "form": "per-token", "quantize": quantize, "rows": B,
                          "input": f"split-K slabs, S = {qkv.S}" if isinstance(qkv, native.Partial) else "in place",
                          "plain_us": round(plain * 1e3, 3), "qknorm_us": round(normed * 1e3, 3),
                          "ratio": round(normed / plain, 3)}), flush=True)
    T = PREFILL_TOKENS
    qkv = torch.randn((T, (H + 2 * HKV) * D), generator=g, device=device).half()
    pos = torch.arange(T, dtype=torch.int32, device=device)
    cu = torch.tensor([0, T], dtype=torch.int32, device=device)
    bt = torch.arange(pages, dtype=torch.int32, device=device)[None].contiguous()
    tail = (cos, sin, pos, cu, bt, kp, vp, T, H, HKV, D, D)
    plain = timed_ms(lambda: native.rope_kv_write_prefill(qkv, *tail), 10)
    normed = timed_ms(lambda: native.rope_kv_write_prefill(qkv, *tail, qk_norm=att.qk_norm), 10)
    moved = T * (H + 2 * HKV) * D * 2 + T * H * D * 2 + 2 * T * HKV * D * 2  # qkv read, q written, k and v pages written
    print(json.dumps({"kind": "launch", "form": "page-wise", "quantize": quantize, "tokens": T, "plain_us": round(plain * 1e3, 2),
                      "qknorm_us": round(normed * 1e3, 2), "ratio": round(normed / plain, 3), "bytes_moved": moved,
                      "qknorm_bytes_per_s": round(moved / (normed * 1e-3), 0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=1024, help="mean context length over the timed steps")
    ap.add_argument("--quantize", default="none,gptq")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--skip-steps", action="store_true", help="only the launches alone")
    args = ap.parse_args()

    from tgis_amd.utils.kv_cache import PagedKVCache

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    K, W = args.steps, args.warmup
    batches = [int(b) for b in args.batches.split(",")]
    L_in = max(1, args.ctx - W - K // 2 - 1)
    pages = max(batches) * PagedKVCache.pages_for(L_in + W + K + 10) + 8
    for qname in args.quantize.split(","):
        quantize = None if qname == "none" else qname
        for variant in ("qwen3", "llama", "llama-unfused"):
            lm, tok = build(variant, args.layers, quantize, device, pages)
            if variant == "qwen3":
                launches_alone(lm, quantize, batches, device)
            for B in ([] if args.skip_steps else batches):
                blocks = step_ms(lm, tok, B, L_in, W, K, args.blocks)
                print(json.dumps({"kind": "step", "variant": variant, "quantize": quantize, "layers": args.layers, "batch": B,
                                  "mean_ctx": L_in + W + (K + 1) / 2, "steps": K, "warmup": W,
                                  "ms_per_step": round(statistics.median(blocks), 4),
                                  "ms_per_step_blocks": [round(b, 4) for b in blocks], "hip_graph": bool(lm.use_graphs),
                                  "data": "synthetic (seeded weights at the Qwen3-8B layer shapes; KV from a real prefill)"}),
                      flush=True)
            del lm
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
