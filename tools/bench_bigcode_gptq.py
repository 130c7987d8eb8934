"""Starcoder-15B-shaped int4 GPTQ decode on one MI355X: synthetic weights at BigCodeConfig's default shapes (40 layers, hidden
6144, 48 heads over one kv head, n_inner 24576, vocab 49152), group size 128, f16, B 32.  Prints ONE JSON line:

  "step":   ms/step, tokens/s and the share of the step's HBM roofline (bench.algorithmic_bytes_per_step at 8 TB/s) at mean
            ctx 1024 and 4096, median of --blocks timed blocks of --steps decode steps (wall clock around a synchronize);
  "step_ab": the ctx 1024 step with TGIS_FUSED_GELU_GEMM on and off, each value in a fresh child process, alternated twice;
  "c_fc":   the c_fc launch (6144 x 24576) alone at 1, 8, 32 and 64 rows: fused (act 5) against GEMM then tgis_gelu,
            alternated inside one process, warmed, each window of --reps (>= 200) launches (captured once, replayed as one
            graph, so that the host's launch cost stays out) bracketed by device events, --windows windows per side; us per
            launch as the median window, with the windows' min and max as its spread.

The process that prints the line does not touch the GPU: every measurement runs in a child of its own.

    python tools/bench_bigcode_gptq.py > profiles/bigcode_gptq_bench.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "text-generation-inference_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GS = 128
B = 32


def child_step(args):
    import torch

    import bench
    from tgis_amd.inference_engine.synthetic import BigCodeConfig, InferenceEngine, bigcode_tensors
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer, make_batch_pb
    from tgis_amd.utils import layers
    from tgis_amd.utils.kv_cache import PagedKVCache

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = BigCodeConfig()
    K, W = args.steps, args.warmup
    L_in = max(1, args.ctx - W - K // 2 - 1)
    tok = SyntheticTokenizer(cfg.vocab_size)
    tensors = bigcode_tensors(cfg, seed=1234, device=dev, dtype=torch.float16, quantize="gptq", groupsize=GS)
    eng = InferenceEngine(tensors, cfg, torch.float16, "gptq", tokenizer=tok, gptq_groupsize=GS)
    del tensors
    lm = FlashCausalLM("synthetic", None, "synthetic", torch.float16, "gptq", engine=eng,
                       kv_cache_pages=B * PagedKVCache.pages_for(L_in + W + K + 8) + 8)
    torch.cuda.empty_cache()
    blocks = []
    with lm.context_manager():
        for _ in range(args.blocks):
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
            blocks.append((time.perf_counter() - t0) / K * 1e3)
            batch.release()
    ms = statistics.median(blocks)
    ctx_mean = L_in + W + (K + 1) / 2
    ab = bench.algorithmic_bytes_per_step(cfg, "gptq", B, ctx_mean, 1, GS)
    roof_ms = ab["total"] / (bench.HBM_PEAK_GBS * 1e9) * 1e3
    print(json.dumps({"ctx_mean": ctx_mean, "fused_gelu_gemm": bool(layers.FUSED_GELU_GEMM), "graphs": bool(lm.use_graphs),
                      "ms_per_step": round(ms, 4), "ms_per_step_blocks": [round(b, 4) for b in blocks],
                      "tokens_per_s": round(B / ms * 1e3, 1), "algorithmic_bytes_per_step": int(ab["total"]),
                      "ms_at_hbm_peak": round(roof_ms, 4), "frac_of_hbm_peak": round(roof_ms / ms, 4)}))


def child_launch(args):
    import torch

    from tgis_amd import native
    from tgis_amd.inference_engine.synthetic import BigCodeConfig, _random_gptq

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = BigCodeConfig()
    K, N = cfg.hidden_size, cfg.n_inner
    gen = torch.Generator(device=dev).manual_seed(1234)
    t = {}
    _random_gptq(t, "c_fc", N, K, gen, dev, GS, 4)
    w = native.GptqWeight(t["c_fc.qweight"], t["c_fc.qzeros"], t["c_fc.scales"], None, 4, GS)
    bias = (torch.randn(N, generator=gen, device=dev) * 0.02).half()
    ws = native.Workspace(64 << 20, dev)
    out = {}
    for M in (1, 8, 32, 64):
        x = (torch.randn((M, K), generator=gen, device=dev) * 0.5).half()
        o = torch.empty((M, N), dtype=torch.float16, device=dev)
        o2 = torch.empty_like(o)

        def fused():
            native.gptq_gemm(x, w, ws, bias=bias, act=5, out=o)

        def two():
            native.gptq_gemm(x, w, ws, bias=bias, act=0, out=o)
            native.gelu(o, True, out=o2)

        def captured(fn):  # one window = one graph of --reps launches: device time, free of the host's launch cost
            for _ in range(args.warm):
                fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(args.reps):
                    fn()
            return g

        def window(g):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) * 1e3 / args.reps

        graphs = {"fused": captured(fused), "two": captured(two)}
        for g in graphs.values():
            window(g)
        wins = {"fused": [], "two": []}
        for _ in range(args.windows):  # alternated: drift of the clocks hits both sides alike
            wins["fused"].append(window(graphs["fused"]))
            wins["two"].append(window(graphs["two"]))
        fused()  # `two` ran last: o2 holds the GELU of the act 0 output
        torch.cuda.synchronize()
        assert torch.equal(o.view(torch.int16), o2.view(torch.int16)), "fused and two-launch bits differ"
        out[str(M)] = {side: {"us": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                       for side, v in wins.items()}
        out[str(M)]["launches_per_window"] = args.reps
        out[str(M)]["windows"] = args.windows
    print(json.dumps(out))


def run_child(argv, env=None):
    e = dict(os.environ)
    e.update(env or {})
    # (a child that runs past its limit is killed and ends the tool: nothing more is started on the device)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), *argv], env=e, capture_output=True, text=True, timeout=600)
    sys.stderr.write(f"child {' '.join(argv)} {env or ''}: exit {p.returncode}\n")
    sys.stderr.flush()
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {argv} failed with {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["step", "launch"])
    ap.add_argument("--ctx", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--skip-4096", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 200, "a window holds at least 200 launches"
    if args.child == "step":
        return child_step(args)
    if args.child == "launch":
        return child_launch(args)
    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--blocks", str(args.blocks)]
    launch = run_child(["--child", "launch", "--reps", str(args.reps), "--warm", str(args.warm), "--windows", str(args.windows)])
    ab = {"on": [], "off": []}
    for _ in range(2):
        for name, val in (("on", "true"), ("off", "false")):
            ab[name].append(run_child(["--child", "step", "--ctx", "1024", *common], {"TGIS_FUSED_GELU_GEMM": val}))
    steps = {"1024": ab["on"][0]}
    if not args.skip_4096:
        steps["4096"] = run_child(["--child", "step", "--ctx", "4096", *common], {"TGIS_FUSED_GELU_GEMM": "true"})
    print(json.dumps({
        "metric": "decode ms per step and tokens/s (Starcoder-15B shapes, int4 GPTQ group 128, f16, batch 32)",
        "data": "synthetic (seeded random GPTQ tensors at the real shapes; KV from a real prefill of seeded token ids)",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "timed_blocks": args.blocks,
        "step": steps,
        "step_ab": {k: {"ms_per_step": [r["ms_per_step"] for r in v], "ms_per_step_blocks": [r["ms_per_step_blocks"] for r in v]}
                    for k, v in ab.items()},
        "c_fc": launch,
    }))


if __name__ == "__main__":
    main()
