"""What per-request LoRA adapters cost a decode step, on synthetic Llama-2-7B shapes (B 32, ctx 1024), f16 and int4.

Four configurations of the same step, alternating block by block in ONE process (so that drift hits all of them alike), after
a warm-up, with the spread over the blocks next to each median:
  off        lora_slots = 0: the model as it always was
  on_none    lora_slots = 8, no row carries an adapter: the plain graph, but the MLP without its fused SiLU * up epilogue
  on_one     every row on one r 16 all-module adapter
  on_eight   the rows spread over 8 such adapters
and the shrink and expand launches alone on the four projections' shapes at 32 rows (one slot / 8 slots).  The adapters are
made in memory (random f16 A and B) and pinned through the model's own slot table.  One JSON line per measurement on stdout,
all of them together in --out.

    python tools/bench_lora.py [--steps 20] [--blocks 5] [--dtypes f16,int4] [--out profiles/lora_bench.json]"""
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
from tgis_amd.utils import lora  # noqa: E402
from tgis_amd.utils.kv_cache import PagedKVCache  # noqa: E402

SLOTS, RANK, WARM = 8, 16, 10
# (name, K, the column bounds) of the four wrapped linears of Llama-2-7B
SHAPES = [("qkv", 4096, (0, 4096, 8192, 12288)), ("o", 4096, (0, 4096)), ("gate_up", 4096, (0, 11008, 22016)),
          ("down", 11008, (0, 4096))]


def median_us(fn, warm, reps):
    for _ in range(warm):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return statistics.median(ts), ts[len(ts) // 10], ts[-1 - len(ts) // 10]


def launches(args, dev, emit):
    """tgis_lora_shrink and tgis_lora_expand alone: 32 rows on one r 16 slot, and spread over 8."""
    T = 32
    for name, K, bounds in SHAPES:
        P, N = len(bounds) - 1, bounds[-1]
        w = native.LoraImages(K, bounds, SLOTS, 64, torch.float16, dev)
        for s in range(SLOTS):
            w.load(s, [torch.randn(RANK, K) * K ** -0.5] * P, [torch.randn(bounds[p + 1] - bounds[p], RANK) for p in range(P)], 2.0)
        x = (torch.randn((T, K), device=dev) * 0.1).half()
        y = torch.zeros((T, N), dtype=torch.float16, device=dev)
        for label, slot in (("one_slot", [0] * T), ("eight_slots", [t % SLOTS for t in range(T)])):
            g = native.lora_group(torch.tensor(slot, dtype=torch.int32, device=dev), SLOTS)
            v = native.lora_shrink(x, w, g)
            sh = median_us(lambda: native.lora_shrink(x, w, g, v), args.warm, args.reps)
            ex = median_us(lambda: native.lora_expand(v, w, g, y), args.warm, args.reps)
            emit({"launch": name, "K": K, "N": N, "P": P, "rows": T, "rank": RANK, "slots": label,
                  "shrink_us": round(sh[0], 2), "shrink_p10_p90": [round(sh[1], 2), round(sh[2], 2)],
                  "expand_us": round(ex[0], 2), "expand_p10_p90": [round(ex[1], 2), round(ex[2], 2)]})
        del w
        torch.cuda.empty_cache()


def adapter(cfg, name):
    """An all-module r 16 adapter of random f16 tensors, as utils.lora.build_adapter would leave it."""
    shapes = lora.module_shapes(cfg)
    g = torch.Generator().manual_seed(int(name[1:]))
    tensors = {(layer, m): ((torch.randn(RANK, i, generator=g) * i ** -0.5).half(), (torch.randn(o, RANK, generator=g) * 0.02).half())
               for layer in range(cfg.num_hidden_layers) for m, (o, i) in shapes.items()}
    return lora.LoraAdapter(name, RANK, 2.0, tensors)


def steps(args, dev, dtype_s, emit):
    kw, _quantize, _dtype, B, ctx = bench.CONFIGS["llama2-7b-gptq"]  # the flagship's shapes, as int4 or as dense f16
    quantize = "gptq" if dtype_s == "int4" else None
    cfg = LlamaConfig(**kw)
    tok = SyntheticTokenizer(cfg.vocab_size)
    K, n_blocks = args.steps, args.blocks
    new = WARM + K * n_blocks + 8
    L_in = max(1, ctx - new // 2)
    pages = B * PagedKVCache.pages_for(L_in + new) + 8

    def model(slots, batches):
        tensors = llama_tensors(cfg, quantize, seed=1234, device=dev, dtype=torch.float16)
        eng = InferenceEngine(tensors, cfg, torch.float16, quantize, tokenizer=tok)
        del tensors
        return FlashCausalLM("synthetic", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=pages * batches,
                             lora_slots=slots)

    off, on = model(0, 1), model(SLOTS, 3)
    torch.cuda.empty_cache()
    names = [f"a{i}" for i in range(SLOTS)]
    for name in names:  # loaded through the slot table, as a first request would; the batches below pin them as theirs do
        on.lora_table.release(on.lora_table.acquire(adapter(cfg, name)))

    def batch(lm, adapters, bid):
        b, errs = lm.batch_type.from_pb(make_batch_pb([L_in] * B, max_new=new, batch_id=bid), tok, lm.dtype, lm.device,
                                        lm.word_embeddings, None, True)
        assert not errs
        if adapters is not None:  # what from_pb does for a request whose prefix_id names a resident adapter
            table = lm.lora_table
            b.lora_slots, b.lora_table = [table.acquire(table.resident(a)) for a in adapters], table
        lm.generate_token(b, first=True)
        for _ in range(WARM):
            lm.generate_token(b)
        return b

    with off.context_manager():
        variants = [("off", off, batch(off, None, 0)), ("on_none", on, batch(on, None, 1)),
                    ("on_one", on, batch(on, [names[0]] * B, 2)),
                    ("on_eight", on, batch(on, [names[i % SLOTS] for i in range(B)], 3))]
        times = {name: [] for name, _, _ in variants}
        for _ in range(n_blocks):
            for name, lm, b in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(K):
                    lm.generate_token(b)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / K * 1e3)
        for _, _, b in variants:
            b.release()
    base = statistics.median(times["off"])
    for name, _, _ in variants:
        med = statistics.median(times[name])
        emit({"step": f"llama2-7b {dtype_s}", "config": name, "B": B, "ctx": ctx, "steps_per_block": K, "blocks": n_blocks,
              "graphs": bool(on.use_graphs), "ms_per_step": round(med, 4), "ms_min_max": [round(min(times[name]), 4),
                                                                                           round(max(times[name]), 4)],
              "over_off": round(med / base, 4)})
    del off, on, variants
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--dtypes", default="f16,int4")
    ap.add_argument("--skip-launches", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    native.load_library()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    if not args.skip_launches:
        launches(args, dev, emit)
    for dtype_s in [d for d in args.dtypes.split(",") if d]:
        steps(args, dev, dtype_s, emit)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
