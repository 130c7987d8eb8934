"""What a verify step of prompt-lookup speculative decoding (FlashCausalLM(spec_tokens=K)) costs next to the plain decode step,
on the synthetic cfg3 engine built as bench.py builds it, context 1024 (--ctx: another one; from 1024 keys on the verify
step's attention takes the key splits of tgis_attn_num_splits_q, which `verify_num_splits` reports).

Per (B, K), in one process: the median ms of the captured plain step and of the captured verify step (HIP events around graph
replays); their ratio is the break-even number of tokens a verify step must emit.  Then two runs through generate_token, host
clock with a device sync on both sides, in tokens/s: one whose drafts are forced to the model's own continuation (every
draft accepted wherever the two launch forms agree on the token; the count is reported) and one whose drafts are garbage (none
accepted: the cost of speculating in vain).  The plain run of the same requests is the third figure.  An untimed pass of a few
steps in front of every timed run pays the captures of the graphs it uses; forced drafts are gathered on the device and the
hits are told to the batch (note_spec_hits), so no timed step reads the device beyond its one copy of the results.

Random weights at this size decide many tokens by less than fp16 rounding, and a verify forward of B (K + 1) rows takes other
GEMM plans than a plain step of B rows: a forced run may leave the plain run's id stream.  For every request that does, the
tool records the first such token, the plain step's own top-2 logit margin there and max |the verify row's logits - the plain
step's|, and the largest such distance over all tokens on which the streams agree, so that a near-tie is shown, not supposed.

SYNTHETIC WEIGHTS SAY NOTHING ABOUT REAL ACCEPTANCE RATES: the forced runs bracket what the mechanism costs and can give; how
often a lookup's drafts are right depends on the model and the prompts, and is not measured here.

With --speculator E,I,P the drafter is a synthetic MLP speculator (utils/mlp_speculator.py; seeded random weights made in
memory, E = the base model's hidden size) and K = min(P, 7).  Every greedy step of such a model is followed by the drafter's
captured chain, so the figures are: `draft_chain_ms`, the chain alone (HIP events around replays of the chain behind the
verify step; `draft_chain_after_plain_ms` the one behind the plain step); `break_even_tokens_per_verify_step` = (verify step
+ chain) / (plain step + chain); and the same three runs, whose `plain` one is the plain steps of the speculating model,
chain included.  RANDOM SPECULATOR WEIGHTS DRAFT GARBAGE: acceptance on real text is not measured here.

With --sampled the requests sample (temperature 0.8 and top-p 0.9, seeded) and the speculating model has spec_sampling on:
B = 8, K = 3.  One JSON line: ms per step through generate_token (host clock, device sync on both sides) of the plain
sampled step of a model without speculation — the step as it was before the option existed — of the speculating model's
plain (K = 0) step, and of its verify step with every draft forced right and with none; the same two verify runs for greedy
requests on the same model (the captured argmax in place of the chooser); and the chooser's launch alone (HIP events) on
B and on B (K + 1) rows.  Seeded streams are reproducible, so the forced drafts are the plain run's own tokens.

With --candidates C,C,... every (B, K) is measured once per C (spec_candidates=C; 1 = the single chain): the verify step is
then a token tree of 1 + C K rows per request.  The forced run puts the true continuation into the LAST candidate and junk
into the others, so every accepted token is won by a later candidate and passes through tgis_spec_tree_commit.  Added per
line: `commit_ms` (that launch alone, every request moving K positions), and the attention launch alone at the verify
step's (B, q_len = 1 + C K, ctx) with the tree's mask (`attn_tree_launch_ms`) next to the causal launch of the same shape
(`attn_chain_launch_ms_same_shape`), both at the verify step's key splits.

    python tools/spec_decode_bench.py [--config llama2-7b-gptq] [--tokens 32] [--ctx 1024] > profiles/spec_decode_bench.json
    python tools/spec_decode_bench.py --candidates 1,2,4 --bs 1,4,8 --ks 3 > profiles/spec_tree_bench.json
    python tools/spec_decode_bench.py --speculator 4096,4096,3 > profiles/spec_mlp_bench.json
    python tools/spec_decode_bench.py --sampled > profiles/spec_sampled_bench.json"""
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
from tgis_amd.inference_engine.synthetic import InferenceEngine, llama_tensors  # noqa: E402
from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig  # noqa: E402
from tgis_amd.models.flash_causal_lm import FlashCausalLM, graph_bucket  # noqa: E402
from tgis_amd.pb import generate_pb2  # noqa: E402
from tgis_amd.utils import mlp_speculator  # noqa: E402
from tgis_amd.utils.kv_cache import PagedKVCache  # noqa: E402
from tgis_amd.utils.spec_decode import MAX_VERIFY_ROWS, tree_q_mask, tree_rows  # noqa: E402

CTX, BS, KS = 1024, [1, 4, 8, 16], [3, 7]


class IdTokenizer:
    """'t17 t203' -> [17, 203]."""

    def __init__(self, vocab_size):
        self.vocab_size, self.pad_token_id, self.bos_token_id, self.eos_token_id = vocab_size, 0, 1, 2
        self.add_bos_token = False

    def __call__(self, texts, truncation=True, max_length=None, return_token_type_ids=False, **kw):
        return {"input_ids": [[int(w[1:]) for w in t.split()] for t in texts]}


def prefill(lm, tok, prompts, max_new, sampled=False):
    reqs = [generate_pb2.Request(id=i, inputs=" ".join(f"t{t}" for t in p), input_length=len(p), truncate=False,
                                 max_output_length=max_new) for i, p in enumerate(prompts)]
    for i, r in enumerate(reqs if sampled else []):
        r.parameters.temperature, r.parameters.top_p, r.parameters.seed = 0.8, 0.9, 100 + i
    batch, errs = lm.batch_type.from_pb(generate_pb2.Batch(id=0, requests=reqs), tok, lm.dtype, lm.device, lm.word_embeddings,
                                        None, True)
    assert not errs
    toks = lm.generate_token(batch, first=True)[0]
    return batch, {t.request_id: [t.token_id] for t in toks}


class Tap:
    """Keeps the fp32 logits of the latest generate_token call (what the model hands to the chooser)."""

    def __init__(self, lm):
        self.rows = None
        orig = lm._process_new_tokens

        def tapped(batch, out, *a, **kw):
            self.rows = out
            return orig(batch, out, *a, **kw)

        lm._process_new_tokens = tapped


def decode(lm, batch, streams, tokens, force=None, tap=None, keep=None, against=None, path=None):
    """Decode steps until every request has `tokens` tokens; `force(batch, streams)` sets the drafts before each step.
    keep: a list that receives every step's logits (the plain run; one row per request and token).  against = (plain
    streams, plain logits): every emitted token is held against the plain run until its request's stream parts from it.
    Returns (seconds, steps, tokens emitted, partings) — one record per request that parted: the token index, the plain
    run's top-2 logit margin there, and max |this run's logits row - the plain run's| for that token.
    path: the rows of a request, in order, behind which its tokens are emitted (a tree step whose last candidate holds the
    forced drafts); None: rows 0, 1, ..."""
    torch.cuda.synchronize()
    t0, steps, emitted, trace = time.perf_counter(), 0, 0, []
    while min(len(s) for s in streams.values()) < tokens:
        if force is not None:
            force(batch, streams)
        before = {r.id: len(streams[r.id]) for r in batch.requests}
        toks = lm.generate_token(batch)[0]
        if keep is not None:
            keep.append(tap.rows.clone())
        for t in toks:
            streams[t.request_id].append(t.token_id)
            emitted += 1
        if against is not None:  # (a device copy; it is looked at after the clock has stopped)
            trace.append((tap.rows.clone(), before, {rid: len(streams[rid]) for rid in before}, list(before)))
        steps += 1
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    parted, partings, worst = set(), [], 0.0
    for rows, before, after, order in trace:
        plain, plain_logits = against
        per = rows.shape[0] // len(order)
        for i, rid in enumerate(order):
            for j in range(per if path is None else len(path)):
                t = before[rid] + j
                if rid in parted or t >= after[rid] or t >= len(plain[rid]) or t - 1 >= len(plain_logits):
                    break  # (rows behind a rejected draft say nothing)
                ref = plain_logits[t - 1][rid]  # the plain step that chose token t (token 0 is the prefill's)
                diff = float((rows[i * per + (j if path is None else path[j])] - ref).abs().max())
                if streams[rid][t] != plain[rid][t]:
                    top = ref.topk(2).values
                    partings.append({"request": rid, "token": t, "plain_top2_margin": round(float(top[0] - top[1]), 4),
                                     "max_abs_logit_diff": round(diff, 4)})
                    parted.add(rid)
                else:
                    worst = max(worst, diff)
    return sec, steps, emitted, partings, round(worst, 4)


def replay_ms(g, n=30):
    """Median ms of n replays of a captured step (its static inputs stay what the last step left: same shapes, same work)."""
    assert g.graph is not None
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for _ in range(3):
        g.graph.replay()
    for a, b in ev:
        a.record()
        g.graph.replay()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def launch_ms(call, n=30):
    """Median ms of n launches of `call` (HIP events), three untimed ones in front."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for _ in range(3):
        call()
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return round(statistics.median(a.elapsed_time(b) for a, b in ev), 4)


def tree_launches_ms(lm, g, B, C, K, ctx, dev):
    """(tgis_spec_tree_commit alone with every request moving K positions from the last candidate, the attention launch
    of the verify step's shape with the tree's mask, the causal launch of the same shape) on layer 0's pools as they are."""
    from tgis_amd import native
    from tgis_amd.utils.layers import workspace

    R1 = tree_rows(C, K)
    H, Hkv, D = lm.num_heads, lm.num_kv_heads, lm.head_size
    width = PagedKVCache.pages_for(ctx + R1)
    bt = (torch.arange(B * width, dtype=torch.int32, device=dev) % lm.kv_cache.num_pages).reshape(B, width).contiguous()
    new_pos = torch.full((B,), ctx + K, dtype=torch.int32, device=dev)
    best = torch.full((B,), C - 1, dtype=torch.int32, device=dev)
    n_emit = torch.full((B,), K + 1, dtype=torch.int32, device=dev)
    commit = launch_ms(lambda: native.spec_tree_commit(lm.kv_cache.pool, bt, new_pos, best, n_emit, C, K))
    q = torch.randn(B * R1, H * D, device=dev).to(lm.dtype)
    out = torch.empty_like(q)
    ctx_lens = torch.full((B,), ctx + R1, dtype=torch.int32, device=dev)
    cu = torch.arange(B + 1, dtype=torch.int32, device=dev) * R1
    mask = torch.tensor(tree_q_mask(C, K) * B, dtype=torch.int64, device=dev)
    ns = native.attn_q_splits(B, Hkv, H, R1, width * 32)
    ws = None
    if ns > 1:
        ws = workspace(dev)
        ws.ensure(native.attn_workspace_bytes(B * R1, H, Hkv, D, ns))
    k_pool, v_pool = lm.kv_cache.k_pool(0), lm.kv_cache.v_pool(0)

    def attn(**kw):
        native.attn_paged(q, q.stride(0), k_pool, v_pool, bt, ctx_lens, cu, out, B, H, Hkv, D, R1, width * 32, D ** -0.5, ns,
                          ws, **kw)

    return commit, launch_ms(lambda: attn(q_mask=mask)), launch_ms(attn)


def synthetic_speculator(E, I, P, V, dtype):
    """A seeded random speculator as an in-memory checkpoint: unit-normal embeddings and heads, fan-in-scaled projections."""
    cfg = mlp_speculator.SpeculatorConfig(E, I or E, V, P)
    names = {mlp_speculator.TENSOR_NAMES[kind].format(i=i): (kind, i) for i in range(P) for kind in mlp_speculator.TENSOR_NAMES}

    def load(name):
        kind, i = names[name]
        shape = cfg.shape_of(kind, i)
        g = torch.Generator().manual_seed(1000 + 10 * i + sorted(mlp_speculator.TENSOR_NAMES).index(kind))
        if kind == "ln_weight":
            return torch.ones(shape, dtype=dtype)
        if kind == "ln_bias":
            return torch.zeros(shape, dtype=dtype)
        t = torch.randn(shape, generator=g)
        return (t / shape[1] ** 0.5 if kind == "proj" else t).to(dtype)

    return mlp_speculator.SpeculatorCheckpoint(cfg, {n: cfg.shape_of(*ki) for n, ki in names.items()}, load)


def chooser_ms(V, B, K, dev, n=30):
    """Median ms of the chooser's launch alone, temperature + top-p, every row sampled: (tgis_warp_sample on B rows,
    tgis_warp_sample_verify on B (K + 1) rows)."""
    from tgis_amd import native

    g = torch.Generator().manual_seed(0)
    logits = (torch.randn(B * (K + 1), V, generator=g) * 3).to(dev)
    temp = torch.full((B,), 0.8, device=dev)
    cut = torch.full((B,), float(np.float32(1) - np.float32(0.9)), device=dev)
    flags = torch.ones(B, dtype=torch.int32, device=dev)
    rng = torch.tensor([[100 + b, 0] for b in range(B)], dtype=torch.int64, device=dev)
    drafts = torch.full((B, K), 3, dtype=torch.int64, device=dev)
    calls = (lambda: native.warp_sample(logits[:B], temperature=temp, top_p_cut=cut, do_sample=flags, rng=rng),
             lambda: native.warp_sample_verify(logits, drafts, K, temperature=temp, top_p_cut=cut, do_sample=flags, rng=rng))
    out = []
    for call in calls:
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for _ in range(3):
            call()
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        out.append(round(statistics.median(a.elapsed_time(b) for a, b in ev), 4))
    return out


def sampled_main(args, eng, cfg, dtype, quantize, tok, dev):
    B, K, T = 8, 3, args.tokens
    max_new = T + 16
    pages = B * PagedKVCache.pages_for(CTX + max_new) + 8
    prompts = [np.random.default_rng(2025).integers(3, cfg.vocab_size, size=CTX).tolist() for _ in range(B)]
    ones, zeros = [1] * B, [0] * B
    res = {"config": args.config, "ctx": CTX, "B": B, "K": K, "V": cfg.vocab_size, "tokens_per_request": T,
           "sampling": "temperature 0.8, top_p 0.9, seeded",
           "note": "synthetic weights: says nothing about real acceptance rates; ms per step through generate_token"}

    def no_drafts(batch, streams):
        batch.spec_hits = torch.zeros_like(batch.spec_hits)
        batch.note_spec_hits(zeros)

    def garbage(batch, streams):
        batch.spec_drafts = torch.full_like(batch.spec_drafts, 3)
        batch.spec_hits = torch.ones_like(batch.spec_hits)
        batch.note_spec_hits(ones)

    def run(lm, force, n, sampled):
        for timed in (False, True):  # an untimed pass pays the captures
            batch, streams = prefill(lm, tok, prompts, max_new, sampled=sampled)
            before = lm.spec_stats()
            sec, steps, emitted, _, _ = decode(lm, batch, streams, n if timed else 1 + 2 * (K + 1), force=force)
            batch.release()
        return sec, steps, emitted, streams, {k: v - before[k] for k, v in lm.spec_stats().items()}

    def report(name, out, plain=None):
        sec, steps, emitted, streams, d = out
        res[f"{name}_ms_per_step"] = round(sec / steps * 1e3, 4)
        res[f"{name}_tokens_per_s"] = round(emitted / sec, 1)
        res[f"{name}_tokens_per_step_and_request"] = round(emitted / steps / B, 3)
        if plain is not None:
            res[f"{name}_stats"] = {k: d[k] for k in ("verify_steps", "verify_steps_sampled", "fallback_not_greedy", "drafted",
                                                      "accepted")}
            res[f"{name}_ids_equal_plain"] = all(streams[i][:T] == plain[i][:T] for i in streams)

    lm0 = FlashCausalLM("synthetic", None, "synthetic", dtype, quantize, engine=eng, kv_cache_pages=pages)
    with lm0.context_manager():
        out = run(lm0, None, T + K, True)
        report("plain_sampled_step_without_speculation", out)
        plain_s = out[3]
        out = run(lm0, None, T + K, False)
        report("plain_greedy_step_without_speculation", out)
        plain_g = out[3]
    lm0._graphs.clear()
    del lm0
    torch.cuda.empty_cache()
    lm = FlashCausalLM("synthetic", None, "synthetic", dtype, quantize, engine=eng, kv_cache_pages=pages, spec_tokens=K,
                       spec_sampling=True)
    offs = torch.arange(K, device=dev)[None]
    with lm.context_manager():
        for kind, sampled, plain in (("sampled", True, plain_s), ("greedy", False, plain_g)):
            plain_dev = torch.tensor([plain[i] + [3] * K for i in range(B)], dtype=torch.int64, device=dev)

            def truth(batch, streams):
                at = torch.tensor([len(streams[r.id]) for r in batch.requests], device=dev)[:, None] + offs
                batch.spec_drafts = plain_dev.gather(1, at.clamp_(max=plain_dev.shape[1] - 1))
                batch.spec_hits = torch.ones_like(batch.spec_hits)
                batch.note_spec_hits(ones)

            report(f"{kind}_plain_step_of_the_speculating_model", run(lm, no_drafts, T, sampled), plain)
            report(f"{kind}_verify_accept_all", run(lm, truth, T, sampled), plain)
            report(f"{kind}_verify_accept_none", run(lm, garbage, T, sampled), plain)
    res["chooser_ms_plain_B_rows"], res["chooser_ms_verify_B_K1_rows"] = chooser_ms(cfg.vocab_size, B, K, dev)
    res["not_measured"] = "acceptance on real text; other B, K, V and warpers; the MLP drafter with sampled requests"
    print(json.dumps(res), flush=True)


def main():
    global CTX, BS, KS
    ap = argparse.ArgumentParser()
    ap.add_argument("--speculator", default=None, metavar="E,I,P",
                    help="draft with a synthetic MLP speculator of these sizes (e.g. 4096,4096,3) instead of the lookup")
    ap.add_argument("--sampled", action="store_true",
                    help="sampled requests (temperature + top-p) on a model with spec_sampling: B = 8, K = 3")
    ap.add_argument("--config", default="llama2-7b-gptq", choices=sorted(bench.CONFIGS))
    ap.add_argument("--tokens", type=int, default=32, help="tokens generated per request in the timed runs")
    ap.add_argument("--ctx", type=int, default=CTX, help="prompt tokens per request")
    ap.add_argument("--bs", default=None, metavar="B,B,...", help="batch sizes (default 1,4,8,16)")
    ap.add_argument("--ks", default=None, metavar="K,K,...", help="drafts per request (default 3,7)")
    ap.add_argument("--candidates", default="1", metavar="C,C,...",
                    help="draft chains per request (spec_candidates; default 1 = the single chain), e.g. 1,2,4")
    args = ap.parse_args()
    CTX = args.ctx
    BS = [int(b) for b in args.bs.split(",")] if args.bs else BS
    KS = [int(k) for k in args.ks.split(",")] if args.ks else KS
    CS = [int(c) for c in args.candidates.split(",")]
    assert CS == [1] or not (args.speculator or args.sampled), "--candidates > 1 goes with the lookup and greedy requests"
    kw, quantize, dtype_s, _, _ = bench.CONFIGS[args.config]
    cfg, dtype, dev = LlamaConfig(**kw), getattr(torch, dtype_s), torch.device("cuda:0")
    tensors = llama_tensors(cfg, quantize, seed=1234, device=dev, dtype=dtype)
    tok = IdTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors, cfg, dtype, quantize, tokenizer=tok)
    del tensors
    if args.sampled:
        return sampled_main(args, eng, cfg, dtype, quantize, tok, dev)
    T = args.tokens
    max_new = T + max(16, max(CS) * max(KS) + 1)  # every timed step keeps K + 1 (C K + 1) tokens in hand
    pages = max(BS) * PagedKVCache.pages_for(CTX + max_new) + 8
    rng = np.random.default_rng(2025)
    spec, ks = None, KS
    if args.speculator:
        E, I, P = (int(x) for x in args.speculator.split(","))
        spec = synthetic_speculator(E, I, P, cfg.vocab_size, dtype)
        ks = [min(P, 7)]
    for K, C in [(K, C) for K in ks for C in CS]:
        lm = FlashCausalLM("synthetic", None, "synthetic", dtype, quantize, engine=eng, kv_cache_pages=pages, spec_tokens=K,
                           speculator=spec, spec_candidates=C)
        assert lm.use_graphs
        tap = Tap(lm)
        for B in BS:
            res = {"config": args.config, "ctx": CTX, "B": B, "K": K, "C": C, "tokens_per_request": T,
                   "note": "synthetic weights: says nothing about real acceptance rates"}
            if spec is not None:
                res["drafter"] = f"mlp {args.speculator}"
                res["speculator_bytes"] = lm.speculator.nbytes
            if graph_bucket(B) * tree_rows(C, K) > MAX_VERIFY_ROWS:
                res["skipped"] = (f"graph_bucket(B) * (1 + C K) = {graph_bucket(B) * tree_rows(C, K)} > {MAX_VERIFY_ROWS}: "
                                  "such a batch never verifies")
                print(json.dumps(res), flush=True)
                continue
            prompts = [rng.integers(3, cfg.vocab_size, size=CTX).tolist() for _ in range(B)]

            ones, zeros = [1] * B, [0] * B

            def no_drafts(batch, streams):  # every step the plain one; the host learns the hits without a read
                batch.spec_hits = torch.zeros_like(batch.spec_hits)
                batch.note_spec_hits(zeros)

            def garbage(batch, streams):
                batch.spec_drafts = torch.full_like(batch.spec_drafts, 3)
                batch.spec_hits = torch.ones_like(batch.spec_hits)
                batch.note_spec_hits(ones)

            def run(force, n, **kw):
                """An untimed pass of a few steps in front (it pays the captures of the graphs the mode uses), then the
                timed one."""
                for timed in (False, True):
                    batch, streams = prefill(lm, tok, prompts, max_new)
                    before = lm.spec_stats()
                    out = decode(lm, batch, streams, n if timed else 1 + 2 * (K + 1), force=force, tap=tap,
                                 **(kw if timed else {}))
                    width = batch.block_tables.shape[1]
                    batch.release()
                return out, streams, {k: v - before[k] for k, v in lm.spec_stats().items()}, width

            with lm.context_manager():
                # the plain run: the model's own continuation and its logits
                plain_logits = []
                (sec, steps, emitted, _, _), plain, _, width = run(no_drafts, T + K, keep=plain_logits)
                res["plain_tokens_per_s"] = round(emitted / sec, 1)
                key = (graph_bucket(B), width)
                res["plain_step_ms"] = round(replay_ms(lm._graphs[key]), 4)
                plain_dev = torch.tensor([plain[i] + [3] * K for i in range(B)], dtype=torch.int64, device=dev)
                offs = torch.arange(K, device=dev)[None]

                def truth(batch, streams):  # the plain run's next K tokens of every request, gathered on the device
                    at = torch.tensor([len(streams[r.id]) for r in batch.requests], device=dev)[:, None] + offs
                    right = plain_dev.gather(1, at.clamp_(max=plain_dev.shape[1] - 1))
                    if C > 1:  # the last candidate holds them, the others junk: every accepted token goes through the commit
                        right = torch.cat([torch.full((B, C - 1, K), 3, dtype=torch.int64, device=dev), right[:, None]], 1)
                    batch.spec_drafts = right
                    batch.spec_hits = torch.ones_like(batch.spec_hits)
                    batch.note_spec_hits(ones)

                for name, force in (("accept_all", truth), ("accept_none", garbage)):
                    path = None if C == 1 else [0] + [1 + (C - 1) * K + j for j in range(K)]
                    (sec, steps, emitted, partings, worst), streams, d, _ = run(force, T, against=(plain, plain_logits),
                                                                                path=path)
                    res[f"{name}_tokens_per_s"] = round(emitted / sec, 1)
                    res[f"{name}_steps"] = steps
                    res[f"{name}_tokens_per_step_and_request"] = round(emitted / max(1, steps) / B, 3)
                    res[f"{name}_stats"] = {k: d[k] for k in ("verify_steps", "drafted", "accepted", "emitted",
                                                              "won_by_later_candidate")}
                    res[f"{name}_ids_equal_plain"] = all(streams[i][:T] == plain[i][:T] for i in streams)
                    # where a stream left the plain run's: how narrowly the plain run decided that token, and how far the
                    # two launch forms' logits are apart there; and the largest such distance over the tokens that agreed
                    res[f"{name}_partings"] = partings
                    res[f"{name}_max_abs_logit_diff_where_equal"] = worst
                vkey = key + ((K,) if C == 1 else (K, C))
                res["verify_step_ms"] = round(replay_ms(lm._graphs[vkey]), 4)
                res["plain_num_splits"] = lm._graphs[key].num_splits
                res["verify_num_splits"] = lm._graphs[vkey].num_splits
                if C > 1:
                    res["commit_ms"], res["attn_tree_launch_ms"], res["attn_chain_launch_ms_same_shape"] = tree_launches_ms(
                        lm, lm._graphs[vkey], B, C, K, CTX, dev)
            if spec is None:
                res["break_even_tokens_per_verify_step"] = round(res["verify_step_ms"] / res["plain_step_ms"], 3)
            else:
                res["draft_chain_ms"] = chain = round(replay_ms(lm._graphs[vkey].chain), 4)
                res["draft_chain_after_plain_ms"] = chain0 = round(replay_ms(lm._graphs[key].chain), 4)
                res["break_even_tokens_per_verify_step"] = round(
                    (res["verify_step_ms"] + chain) / (res["plain_step_ms"] + chain0), 3)
            print(json.dumps(res), flush=True)
        lm._graphs.clear()
        del lm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
