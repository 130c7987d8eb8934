"""gpt-neox-20b decode on one MI355X: synthetic fp16 weights at the real shapes (44 layers, hidden 6144, 64 heads of 96,
intermediate 24576, vocab 50432, 24 rotary dims, gelu_fast, parallel residual), B 32, mean context 1024.
Prints one JSON line in bench.py's shape: ms/step (median of timed blocks, synchronised on both sides), tok/s and the
step roofline computed from the shapes (weights + KV read at 8 TB/s).

    python tools/bench_neox.py [--steps 32 --warmup 3 --blocks 3]
    rocprofv3 --kernel-trace --stats -d OUT -o neox -- python tools/bench_neox.py --blocks 1   (profiles/neox20b_*)"""
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
NEOX_20B = dict(vocab_size=50432, hidden_size=6144, num_hidden_layers=44, num_attention_heads=64, intermediate_size=24576,
                hidden_act="gelu_fast", rotary_pct=0.25, rotary_emb_base=10000, max_position_embeddings=2048,
                layer_norm_eps=1e-5, use_parallel_residual=True)


def params(cfg) -> int:
    E, I, V, L = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_hidden_layers
    layer = (3 * E * E + 3 * E) + (E * E + E) + (I * E + I) + (E * I + E) + 4 * E
    return 2 * V * E + L * layer + 2 * E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--ctx", type=int, default=1024, help="mean context length over the timed steps")
    args = ap.parse_args()

    from tgis_amd.inference_engine.synthetic import InferenceEngine, neox_tensors
    from tgis_amd.models.custom_modeling.flash_neox_modeling import GPTNeoXConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer, make_batch_pb
    from tgis_amd.utils.kv_cache import PagedKVCache

    cfg = GPTNeoXConfig(**NEOX_20B)
    dtype = torch.float16
    B, K, W = args.batch, args.steps, args.warmup
    L_in = max(1, args.ctx - W - K // 2 - 1)
    total_len = L_in + W + K + 8
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = SyntheticTokenizer(cfg.vocab_size)
    eng = InferenceEngine(neox_tensors(cfg, seed=1234, device=device, dtype=dtype), cfg, dtype, None, tokenizer=tok)
    lm = FlashCausalLM("synthetic", None, "synthetic", dtype, None, engine=eng,
                       kv_cache_pages=B * PagedKVCache.pages_for(total_len) + 8)
    torch.cuda.empty_cache()

    blocks, ctx_means = [], []
    with lm.context_manager():
        batch = None
        for _ in range(args.blocks):
            if batch is not None:
                batch.release()
            batch, errs = lm.batch_type.from_pb(make_batch_pb([L_in] * B, max_new=W + K + 8), tok, lm.dtype, lm.device,
                                                lm.word_embeddings, None, True)
            assert not errs
            lm.generate_token(batch, first=True)  # prefill (untimed)
            for _ in range(W):
                lm.generate_token(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                lm.generate_token(batch)
            torch.cuda.synchronize()
            blocks.append((time.perf_counter() - t0) * 1e3 / K)
        ctx_mean = L_in + W + (K + 1) / 2  # context (incl. the new token) averaged over the timed steps
    ms = statistics.median(blocks)
    E, L = cfg.hidden_size, cfg.num_hidden_layers
    w_bytes = (params(cfg) - cfg.vocab_size * E) * 2  # every weight but embed_in, which a step reads B rows of
    kv_bytes = int(L * 2 * E * 2 * B * ctx_mean)
    roof_ms = (w_bytes + kv_bytes) / HBM_PEAK * 1e3
    print(json.dumps({
        "metric": "decode tokens/sec (gpt-neox-20b fp16, batch 32, ctx 1024) + ms per step",
        "value": round(B / ms * 1e3, 2), "unit": "tokens/s", "n_gpus": 1, "steps": K, "warmup": W,
        "ms_per_step": round(ms, 4), "timed_blocks": len(blocks), "ms_per_step_blocks": [round(b, 4) for b in blocks],
        "higher_is_better": True, "dtype": "f16", "hip_graph": bool(lm.use_graphs),
        "data": "synthetic (seeded weights at the real shapes; KV from a real prefill of seeded token ids)",
        "config": {"workload": f"gpt-neox-20b decode, B={B}, mean ctx {ctx_mean:.1f}", "params": params(cfg),
                   "rot_dim": 24, "head_size": 96},
        "step_roofline": {"weight_bytes": w_bytes, "kv_read_bytes": kv_bytes, "ms_at_hbm_peak": round(roof_ms, 3),
                          "frac_of_hbm_peak": round(roof_ms / ms, 4)},
    }))


if __name__ == "__main__":
    main()
