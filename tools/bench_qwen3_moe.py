"""Qwen3-30B-A3B on one MI355X: synthetic weights at the real layer shapes (hidden 2048, 32 heads on 4 KV heads of 128, 128
experts, 8 per token, moe intermediate 768, vocab 151936) with --layers layers (default 8; the full model has 48), bf16, mean
context 1024.  One JSON line per row (keep them in profiles/qwen3_moe_bench.jsonl):

  {"kind": "step", ...}   ms per decode step at B 1 / 8 / 32 (median of timed blocks, synchronised on both sides), the mean
                          number of distinct experts hit per layer and the step's HBM roofline computed from the experts
                          actually hit: attention + router + head weights, hit experts' weights and the KV read, at 8 TB/s
  {"kind": "moe", ...}    one layer's routed block alone (router GEMM, route, up, down) at T rows under the tile kernel and
                          under the slab kernel body (tgis_debug_moe_tile_force), the two alternating round by round: the
                          table the small-T rule of csrc/moe_tiles.h is read off
  {"kind": "route", ...}  the three route launches alone at T = 32 and 4096

    python tools/bench_qwen3_moe.py [--layers 8 --steps 32 --warmup 3 --blocks 3 --batches 1,8,32 --skip-steps --skip-moe]"""
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
MOE_ROWS = (1, 2, 4, 8, 16, 32, 64, 128, 256, 1024, 4096)
ROUTE_ROWS = (32, 4096)


def event_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def moe_alone(moe, T, dtype, device, rounds=5):
    """The routed block at T rows under either kernel, alternating; medians and ranges over the rounds."""
    from tgis_amd import native

    g = torch.Generator(device=device).manual_seed(T)
    x = torch.randn((T, moe.hidden), generator=g, device=device).to(dtype)
    partial = T <= native.PARTIAL_MAX_M
    iters = 20 if T <= 64 else (5 if T <= 256 else 2)
    times = {0: [], 1: []}
    try:
        for kernel in (0, 1):  # warm-up of both
            native.moe_tile_force(kernel)
            moe.block(x, partial)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for kernel in (0, 1):
                native.moe_tile_force(kernel)
                times[kernel].append(event_ms(lambda: moe.block(x, partial), iters))
    finally:
        native.moe_tile_force(-1)
    hit = int((moe.route(x).counts > 0).sum())
    expert_bytes = hit * 3 * moe.hidden * moe.down.K * 2
    tile, slab = statistics.median(times[0]), statistics.median(times[1])
    return {"kind": "moe", "rows": T, "dtype": str(dtype).replace("torch.", ""), "experts_hit": hit,
            "down_form": "slabs" if partial else "finished", "tile_ms": round(tile, 4), "slab_body_ms": round(slab, 4),
            "tile_ms_range": [round(min(times[0]), 4), round(max(times[0]), 4)],
            "slab_body_ms_range": [round(min(times[1]), 4), round(max(times[1]), 4)],
            "rule_picks": "slab_body" if native.moe_tile_plan(0, T, moe.hidden, moe.gate_up.N, moe.E, moe.top_k)["slab_body"] else "tile",
            "expert_weight_bytes_hit": expert_bytes,
            "tile_frac_of_hbm_peak": round(expert_bytes / HBM_PEAK * 1e3 / tile, 4),
            "slab_body_frac_of_hbm_peak": round(expert_bytes / HBM_PEAK * 1e3 / slab, 4)}


def route_alone(moe, T, device, rounds=5):
    from tgis_amd import native

    logits = torch.randn((T, moe.E), generator=torch.Generator(device=device).manual_seed(T), device=device) * 2.0
    native.moe_route_tiles(logits, moe.top_k, renorm=moe.renorm)
    torch.cuda.synchronize()
    ms = [event_ms(lambda: native.moe_route_tiles(logits, moe.top_k, renorm=moe.renorm), 20) for _ in range(rounds)]
    return {"kind": "route", "rows": T, "experts": moe.E, "top_k": moe.top_k, "launches": 3,
            "route_ms": round(statistics.median(ms), 4), "route_ms_range": [round(min(ms), 4), round(max(ms), 4)]}


def experts_hit_per_layer(lm, batch):
    """Mean number of distinct experts per layer in one eager decode step (host reads, outside any timed region)."""
    from tgis_amd import native

    seen, real, graphs = [], native.moe_route_tiles, lm.use_graphs

    def tapped(*a, **kw):
        r = real(*a, **kw)
        seen.append(r.counts)
        return r

    native.moe_route_tiles, lm.use_graphs = tapped, False
    try:
        lm.generate_token(batch)
        torch.cuda.synchronize()
    finally:
        native.moe_route_tiles, lm.use_graphs = real, graphs
    return statistics.mean(int((c > 0).sum()) for c in seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--ctx", type=int, default=1024, help="mean context length over the timed steps")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--skip-moe", action="store_true", help="only the decode steps")
    ap.add_argument("--skip-steps", action="store_true", help="only the routed block and the route launches alone")
    args = ap.parse_args()

    from tgis_amd.inference_engine.synthetic import InferenceEngine, Qwen3MoeConfig, qwen3_moe_tensors
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer, make_batch_pb
    from tgis_amd.utils.kv_cache import PagedKVCache

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    K, W, dtype = args.steps, args.warmup, torch.bfloat16
    batches = [int(b) for b in args.batches.split(",")]
    L_in = max(1, args.ctx - W - K // 2 - 1)
    total_len = L_in + W + K + 10
    cfg = Qwen3MoeConfig(num_hidden_layers=args.layers)
    tok = SyntheticTokenizer(cfg.vocab_size)
    tensors = qwen3_moe_tensors(cfg, seed=1234, device=device, dtype=dtype)
    eng = InferenceEngine(tensors, cfg, dtype, None, tokenizer=tok)
    tensors.clear()
    del tensors
    lm = FlashCausalLM("synthetic", None, "synthetic", dtype, None, engine=eng,
                       kv_cache_pages=max(batches) * PagedKVCache.pages_for(total_len) + 8)
    torch.cuda.empty_cache()
    E, I, L, H = cfg.hidden_size, cfg.moe_intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads
    Hkv, D = cfg.num_key_value_heads, cfg.head_dim
    dense_bytes = L * (E * (H + 2 * Hkv) * D + H * D * E + cfg.num_experts * E) * 2 + cfg.vocab_size * E * 2
    for B in ([] if args.skip_steps else batches):
        blocks = []
        with lm.context_manager():
            batch = None
            for _ in range(args.blocks):
                if batch is not None:
                    batch.release()
                batch, errs = lm.batch_type.from_pb(make_batch_pb([L_in] * B, max_new=W + K + 10), tok, lm.dtype, lm.device,
                                                    lm.word_embeddings, None, True)
                assert not errs
                lm.generate_token(batch, first=True)  # prefill, untimed
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
        expert_bytes = int(L * hit * 3 * E * I * 2)
        kv_bytes = int(L * 2 * Hkv * D * 2 * B * ctx_mean)
        roof_ms = (dense_bytes + expert_bytes + kv_bytes) / HBM_PEAK * 1e3
        print(json.dumps({
            "kind": "step", "metric": f"decode ms per step (Qwen3-30B-A3B layer shapes, {L} layers, bf16)", "layers": L,
            "batch": B, "mean_ctx": ctx_mean, "steps": K, "warmup": W, "ms_per_step": round(ms, 4),
            "ms_per_step_blocks": [round(b, 4) for b in blocks], "tokens_per_s": round(B / ms * 1e3, 2),
            "hip_graph": bool(lm.use_graphs), "experts_hit_per_layer": round(hit, 3),
            "step_roofline": {"dense_weight_bytes": dense_bytes, "expert_weight_bytes_hit": expert_bytes,
                              "kv_read_bytes": kv_bytes, "ms_at_hbm_peak": round(roof_ms, 4),
                              "frac_of_hbm_peak": round(roof_ms / ms, 4),
                              "expert_bytes_frac_of_hbm_peak": round(expert_bytes / HBM_PEAK * 1e3 / ms, 4)},
            "data": "synthetic (seeded weights at the real layer shapes; KV from a real prefill of seeded token ids)",
        }), flush=True)
    if not args.skip_moe:
        moe = lm.model.model.layers[0].moe
        for T in MOE_ROWS:
            print(json.dumps(moe_alone(moe, T, dtype, device)), flush=True)
        for T in ROUTE_ROWS:
            print(json.dumps(route_alone(moe, T, device)), flush=True)


if __name__ == "__main__":
    main()
