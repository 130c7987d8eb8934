"""What scoring the prompt tokens of an input_toks request costs, in time and in memory, on head shapes K 4096 with V 32000
(Llama-2) and V 128256 (Llama-3) at T 512 / 2048 / 8192 rows, f16:

  logits   the path without the option: the library GEMM to fp32 [T, V] (FastLinear.forward over all rows), then
           log_softmax, gather and the rank compare of utils/tokens.py get_input_tokens_info, restated here
  fused    native.head_logprobs: the same three results per row, z never stored

Both run in ONE process, alternating block by block after a warm-up of each shape; times are device events around the whole
path, the median over the blocks with the spread next to it; memory is torch.cuda.max_memory_allocated above what was
allocated before the call (the inputs and the weight are not counted).  The two paths' results are compared on the same
seeded inputs.  One JSON object per (V, T) on stdout and in --out.

    python tools/bench_input_logprobs.py [--blocks 7] [--reps 3] [--out profiles/input_logprobs_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "text-generation-inference_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tgis_amd import native  # noqa: E402

K = 4096
VOCABS = (32000, 128256)
ROWS = (512, 2048, 8192)


def logits_path(x, w, targets):
    """lm_head over all rows to fp32, then what get_input_tokens_info does with logprobs and ranks asked for."""
    logits = F.linear(x, w).float()
    all_lp = torch.log_softmax(logits, -1)
    tok_lp = all_lp.gather(1, targets.unsqueeze(-1))
    ranks = (all_lp > tok_lp).sum(dim=1) + 1
    return tok_lp.squeeze(-1), ranks


def timed_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "input_logprobs_bench.jsonl"))
    ap.add_argument("--vocabs", default=",".join(map(str, VOCABS)))
    ap.add_argument("--rows", default=",".join(map(str, ROWS)))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_input_logprobs.py measures on the GPU: none found")
    native.load_library()
    dev = torch.device("cuda:0")
    lines = []
    for V in map(int, args.vocabs.split(",")):
        g = torch.Generator(device=dev).manual_seed(V)
        w = (torch.randn((V, K), device=dev, generator=g) * K ** -0.5).half()
        for T in map(int, args.rows.split(",")):
            # rows of unit scale against a weight of K^-1/2: logits of unit scale, as behind a final norm
            x = torch.randn((T, K), device=dev, generator=g).half()
            targets = torch.randint(0, V, (T,), device=dev, generator=g)
            paths = {"logits": lambda: logits_path(x, w, targets), "fused": lambda: native.head_logprobs(x, w, targets)[:2]}
            (lp0, rk0), (lp1, rk1) = paths["logits"](), paths["fused"]()
            lp_err = float((lp0 - lp1).abs().max())
            rank_same = float((rk0 == rk1).float().mean())
            del lp0, rk0, lp1, rk1
            mem = {name: peak_bytes(fn) for name, fn in paths.items()}
            for fn in paths.values():  # (warm: both have run twice by now)
                timed_ms(fn, 1)
            ms = {name: [] for name in paths}
            for _ in range(args.blocks):
                for name, fn in paths.items():
                    ms[name].append(timed_ms(fn, args.reps))
            line = {"K": K, "V": V, "T": T, "dtype": "f16", "blocks": args.blocks, "reps": args.reps,
                    "max_abs_logprob_diff": lp_err, "ranks_equal_share": rank_same}
            for name in paths:
                line[f"{name}_ms"] = round(statistics.median(ms[name]), 4)
                line[f"{name}_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
                line[f"{name}_peak_bytes"] = mem[name]
            line["fused_tflops"] = round(2.0 * T * V * K / (line["fused_ms"] * 1e-3) / 1e12, 1)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del x, targets
            torch.cuda.empty_cache()
        del w
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
