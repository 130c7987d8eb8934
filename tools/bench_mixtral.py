"""Mixtral-8x7B decode on one MI355X: synthetic weights at the real layer shapes (hidden 4096, I 14336, 32 heads on 8 KV heads,
D 128, 8 experts, top-2, vocab 32000) with --layers layers (default 8; the full model has 32), bf16 and f16, B in {1, 8, 32},
mean context 1024.  One JSON line per configuration (keep them under profiles/):

  {"kind": "step", ...}   ms per decode step (median of timed blocks, synchronised on both sides), the mean number of distinct
                          experts hit per layer (read back from one eager step behind the timed region) and the step's HBM
                          roofline computed from the experts actually hit: attention + router + head weights, hit experts'
                          weights and the KV read, at 8 TB/s
  {"kind": "moe", ...}    one layer's routed block alone at T rows: the four launches (router GEMM, route, up, down) timed one
                          by one and together, and the loop path for the same rows; T in the decode sizes and in
                          {64, 128, 256, 512, 1024}, the table behind MOE_FUSED_MAX_TOKENS

Both sides of every comparison run in this one process on one device, after a warm-up, as medians.

    python tools/bench_mixtral.py [--layers 8 --steps 32 --warmup 3 --blocks 3 --dtypes bf16,f16 --batches 1,8,32]

--quantize gptq: the same rows for a synthetic int4 GPTQ checkpoint (4 bits, group size 128, f16: q/k/v/o and the experts
quantised, router and head dense) AND, first, for the f16 model it is compared with, in the same run; every line carries
"quantize".  The roofline counts the bytes the int4 kernels read: half a byte per weight plus 4 bytes per (group, column).
Keep the lines in profiles/mixtral_gptq_bench.jsonl.  --moe-tokens 64,128,256 replaces the row counts of the "moe" lines (the
crossover behind MOE_FUSED_MAX_TOKENS); --ring N loads lib/libtgis_hip_ring<N>.so, a library built with another int4 weight
ring (TGIS_LIB_SUFFIX=_ring<N> tools/build.sh -DTGIS_MOE_GPTQ_RING=<N>), for the sweep of DESIGN.md section 6.

    python tools/bench_mixtral.py --quantize gptq [--skip-steps] [--moe-tokens 1,8,32] [--ring 16]"""
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

HBM_PEAK = 8.0e12
MOE_ROWS = (1, 8, 32, 64, 128, 256, 512, 1024)


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


def weight_bytes(K, N, quantize, groupsize=128):
    """Bytes a GEMM reads of a [K, N] weight: 2 per element, or the int4 image's nibbles and {scale, zero} pairs."""
    return K * N // 2 + (K // groupsize) * N * 4 if quantize == "gptq" else K * N * 2


def moe_alone(moe, T, dtype, device, seed):
    """One layer's routed block at T rows: each launch alone, the four together, and the loop path."""
    from tgis_amd import native
    from tgis_amd.utils.layers import workspace

    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((T, moe.hidden), generator=g, device=device).to(dtype)
    ws = workspace(device)
    logits = native.dense_gemm(x, moe.router, ws, out_f32=True)
    r = native.moe_route(logits, moe.top_k)
    up, down = ((native.moe_gptq_gemm_up, native.moe_gptq_gemm_down) if moe.quantize == "gptq" else
                (native.moe_gemm_up, native.moe_gemm_down))
    h = up(x, moe.experts.gate_up, r)
    partial = T <= native.PARTIAL_MAX_M
    iters = 20 if T <= 64 else 5
    hit = int((r.counts > 0).sum())
    res = {
        "kind": "moe", "rows": T, "dtype": str(dtype).replace("torch.", ""), "quantize": moe.quantize, "experts_hit": hit,
        "down_form": "slabs" if partial else "finished",
        "router_gemm_ms": timed_ms(lambda: native.dense_gemm(x, moe.router, ws, out_f32=True), iters),
        "route_ms": timed_ms(lambda: native.moe_route(logits, moe.top_k), iters),
        "up_ms": timed_ms(lambda: up(x, moe.experts.gate_up, r), iters),
        "down_ms": timed_ms(lambda: down(h, moe.experts.down, r, partial=partial), iters),
        "fused_ms": timed_ms(lambda: moe.fused(x, moe.route(x), partial), iters),
        "loop_ms": timed_ms(lambda: moe.loop(x, moe.route(x)), iters),
    }
    expert_bytes = hit * 3 * weight_bytes(moe.hidden, moe.experts.down.K, moe.quantize)
    res["expert_weight_bytes_hit"] = expert_bytes
    res["fused_frac_of_hbm_peak"] = round(expert_bytes / HBM_PEAK * 1e3 / res["fused_ms"], 4)
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}


def experts_hit_per_layer(lm, batch):
    """Mean number of distinct experts per layer in one eager decode step (host reads, outside any timed region)."""
    from tgis_amd import native

    seen, real, graphs = [], native.moe_route, lm.use_graphs

    def tapped(logits, top_k):
        r = real(logits, top_k)
        seen.append(r.counts)
        return r

    native.moe_route, lm.use_graphs = tapped, False
    try:
        lm.generate_token(batch)
        torch.cuda.synchronize()
    finally:
        native.moe_route, lm.use_graphs = real, graphs
    return statistics.mean(int((c > 0).sum()) for c in seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=1024, help="mean context length over the timed steps")
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--skip-moe", action="store_true", help="only the decode steps")
    ap.add_argument("--skip-steps", action="store_true", help="only the routed block alone")
    ap.add_argument("--quantize", default=None, choices=("gptq",),
                    help="f16 only: the f16 model, then the synthetic int4 GPTQ model (group size 128), in one run")
    ap.add_argument("--moe-tokens", default=None, help="row counts of the routed block alone, e.g. 64,128,256")
    ap.add_argument("--ring", type=int, default=None, choices=(4, 8, 16),
                    help="load lib/libtgis_hip_ring<N>.so: the library built with an int4 weight ring of N k64-steps")
    args = ap.parse_args()
    if args.ring is not None:  # before tgis_amd.native is imported: it reads TGIS_HIP_LIB once
        lib = os.path.join(ROOT, "text-generation-inference_amd", "lib", f"libtgis_hip_ring{args.ring}.so")
        if not os.path.exists(lib):
            sys.exit(f"{lib} not found: TGIS_LIB_SUFFIX=_ring{args.ring} tools/build.sh -DTGIS_MOE_GPTQ_RING={args.ring}")
        os.environ["TGIS_HIP_LIB"] = lib

    from tgis_amd.inference_engine.synthetic import InferenceEngine, MixtralConfig, mixtral_tensors
    from tgis_amd.models.custom_modeling import flash_mixtral_modeling as fm
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer, make_batch_pb
    from tgis_amd.utils.kv_cache import PagedKVCache

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    K, W = args.steps, args.warmup
    batches = [int(b) for b in args.batches.split(",")]
    L_in = max(1, args.ctx - W - K // 2 - 1)
    total_len = L_in + W + K + 10
    moe_rows = MOE_ROWS if args.moe_tokens is None else tuple(int(t) for t in args.moe_tokens.split(","))
    configs = [(name, None) for name in args.dtypes.split(",")] if args.quantize is None else [("f16", None), ("f16", "gptq")]
    ring = None
    if args.quantize is not None:
        import ctypes

        from tgis_amd import native

        info = (ctypes.c_int * 16)()
        native.load_library().tgis_debug_moe_gptq_plan(0, 1, 4096, 64, 32, 8, 2, info)
        ring = info[5]
        assert args.ring in (None, ring), f"the loaded library's int4 ring is {ring}, not {args.ring}"
    for name, quantize in configs:
        dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[name]
        cfg = MixtralConfig(num_hidden_layers=args.layers)
        tok = SyntheticTokenizer(cfg.vocab_size)
        tensors = mixtral_tensors(cfg, seed=1234, device=device, dtype=dtype, quantize=quantize)
        eng = InferenceEngine(tensors, cfg, dtype, quantize, tokenizer=tok, gptq_groupsize=128)
        tensors.clear()
        del tensors
        lm = FlashCausalLM("synthetic", None, "synthetic", dtype, quantize, engine=eng,
                           kv_cache_pages=max(batches) * PagedKVCache.pages_for(total_len) + 8)
        torch.cuda.empty_cache()
        E, I, L, H = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads
        Hkv, D = cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads
        dense_bytes = (L * (weight_bytes(E, (H + 2 * Hkv) * D, quantize) + weight_bytes(H * D, E, quantize)
                            + cfg.num_local_experts * E * 2) + cfg.vocab_size * E * 2)
        for B in ([] if args.skip_steps else batches):
            blocks = []
            with lm.context_manager():
                batch = None
                for _ in range(args.blocks):
                    if batch is not None:
                        batch.release()
                    batch, errs = lm.batch_type.from_pb(make_batch_pb([L_in] * B, max_new=W + K + 10), tok, lm.dtype,
                                                        lm.device, lm.word_embeddings, None, True)
                    assert not errs
                    lm.generate_token(batch, first=True)  # prefill (untimed; the loop path above MOE_FUSED_MAX_TOKENS)
                    for _ in range(W):
                        lm.generate_token(batch)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(K):
                        lm.generate_token(batch)
                    torch.cuda.synchronize()
                    blocks.append((time.perf_counter() - t0) * 1e3 / K)
                hit = experts_hit_per_layer(lm, batch)
                batch.release()
            ms = statistics.median(blocks)
            ctx_mean = L_in + W + (K + 1) / 2
            expert_bytes = int(L * hit * 3 * weight_bytes(E, I, quantize))
            kv_bytes = int(L * 2 * Hkv * D * 2 * B * ctx_mean)
            roof_ms = (dense_bytes + expert_bytes + kv_bytes) / HBM_PEAK * 1e3
            print(json.dumps({
                "kind": "step", "metric": f"decode ms per step (Mixtral-8x7B layer shapes, {L} layers, {name})",
                "dtype": name, "quantize": quantize, "int4_ring": ring, "layers": L, "batch": B, "mean_ctx": ctx_mean, "steps": K, "warmup": W,
                "ms_per_step": round(ms, 4), "ms_per_step_blocks": [round(b, 4) for b in blocks],
                "tokens_per_s": round(B / ms * 1e3, 2), "hip_graph": bool(lm.use_graphs),
                "experts_hit_per_layer": round(hit, 3), "moe_fused_max_tokens": fm.MOE_GPTQ_FUSED_MAX_TOKENS if quantize == "gptq" else fm.MOE_FUSED_MAX_TOKENS,
                "step_roofline": {"dense_weight_bytes": dense_bytes, "expert_weight_bytes_hit": expert_bytes,
                                  "kv_read_bytes": kv_bytes, "ms_at_hbm_peak": round(roof_ms, 4),
                                  "frac_of_hbm_peak": round(roof_ms / ms, 4)},
                "data": "synthetic (seeded weights at the real layer shapes; KV from a real prefill of seeded token ids)",
            }), flush=True)
        if not args.skip_moe:
            moe = lm.model.model.layers[0].moe
            for T in moe_rows:
                print(json.dumps(dict(moe_alone(moe, T, dtype, device, seed=T), int4_ring=ring)), flush=True)
        del lm, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
