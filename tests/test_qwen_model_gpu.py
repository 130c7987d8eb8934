"""-m gpu: Qwen3 (model_type "qwen3": per-head q / k RMSNorm, head_dim 128 on hidden 256, tied embeddings) and Qwen2 ("qwen2":
q/k/v bias, no o_proj bias) checkpoints end to end on the flash path against transformers' fp32 CPU Qwen3ForCausalLM /
Qwen2ForCausalLM (tests/golden/qwen3_tiny.npz, qwen2_tiny.npz, made by tests/golden/make_qwen_fixtures.py on the seeded tiny
checkpoints of tests/qwen_tiny.py): prompts of 7, 45 and 100 tokens in one batch, 50 greedy tokens each, so the prefill takes the
page-wise norm + rope launch and every decode step the per-token one.  The options that reach the cache through write_kv run on
Qwen3: KV prefix reuse (the past_lens form) and prompt-lookup speculation (verify rows) are held to the plain run, GPTQ to the
f16 model of the dequantised weights, two tensor-parallel ranks to the fixture.  (The e4m3 cache is held to its codes at the
launches, tests/test_qknorm_ops_gpu.py: there is no quantised-KV oracle of this model to hold a whole run to.)"""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests.fixture_utils import GOLDEN, FixtureTokenizer
from tests.qwen_tiny import TinyQwenConfig, tiny_qwen_tensors
from tests.test_neox_model_gpu import _from_pb, _LogitTap, _pb, _step

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.35       # tests/test_model_gpu.py's f16 bar; the fixtures' margins are more than twice that: ids are exact
GPTQ_SEED = None       # None: the fixture's seed (its dequantised model keeps more than half of the steps above 2 LOGIT_TOL)
GROUPSIZE = 64


def _fixture(model_type):
    z = np.load(os.path.join(GOLDEN, f"{model_type}_tiny.npz"))
    return json.loads(bytes(z["meta"]).decode()), z["ids"], z["logits"]


def _tensors(cfg, seed):
    t = tiny_qwen_tensors(cfg, seed)
    if cfg.tie_word_embeddings:  # (the synthetic engine takes a plain dict: the alias of model_class_for, written out)
        t["lm_head.weight"] = t["model.embed_tokens.weight"]
    return t


def _build(model_type, seed, use_graphs=True, as_type=None, tensors=None, quantize=None, kv_cache_pages=64, engine_kw=None,
           **kw):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    cfg = TinyQwenConfig(model_type)
    fields = cfg.to_dict()
    fields["model_type"] = as_type or model_type
    config = types.SimpleNamespace(**fields)  # what a config.json carries, nothing else
    tok = FixtureTokenizer(cfg.vocab_size)
    eng = InferenceEngine(tensors if tensors is not None else _tensors(cfg, seed), config, torch.float16, quantize,
                          tokenizer=tok, **(engine_kw or {}))
    lm = FlashCausalLM("fixture", None, "synthetic", torch.float16, quantize, engine=eng, kv_cache_pages=kv_cache_pages, **kw)
    lm.use_graphs = use_graphs
    return lm, tok


def _run(lm, tok, prompts, max_new, steps):
    """[(ids [B], logits [B, vocab])] of the prefill and steps - 1 decode steps of one batch."""
    tap = _LogitTap(lm)
    batch = _from_pb(lm, tok, _pb(prompts, max_new))
    got = []
    for i in range(steps):
        toks, logits = _step(lm, batch, tap, first=(i == 0))
        assert [t.request_id for t in toks] == list(range(len(prompts)))
        got.append(([t.token_id for t in toks], logits))
    return got


def _count_fused(monkeypatch):
    """Counts the calls of the two GEMM + rope launches (made while a graph is captured as well as eagerly)."""
    from tgis_amd import native

    calls = []
    for name in ("dense_gemm_rope", "gptq_gemm_rope"):
        orig = getattr(native, name)
        monkeypatch.setattr(native, name, lambda *a, _o=orig, _n=name, **k: calls.append(_n) or _o(*a, **k))
    return calls


def _against_fixture(model_type, monkeypatch, graph_modes=(True, False)):
    """Both runs against the fixture; returns (runs, fused launches, the models' qkv linears)."""
    meta, ids, logits = _fixture(model_type)
    steps = ids.shape[1]
    fused = _count_fused(monkeypatch)
    runs, linears = {}, []
    for use_graphs in graph_modes:
        lm, tok = _build(model_type, meta["seed"], use_graphs=use_graphs)
        assert lm.sliding_window is None  # (the config carries sliding_window 128 next to use_sliding_window false)
        linears += [layer.self_attn.query_key_value.linear for layer in lm.model.model.layers]
        got = runs[use_graphs] = _run(lm, tok, meta["prompts"], meta["max_new"], steps)
        assert not use_graphs or lm._graphs
        worst = 0.0
        for i, (got_ids, got_logits) in enumerate(got):
            err = float(np.abs(got_logits - logits[:, i]).max())
            worst = max(worst, err)
            assert got_ids == ids[:, i].tolist(), f"graphs={use_graphs} step {i}: ids {got_ids} != {ids[:, i].tolist()}"
            assert err <= LOGIT_TOL, f"graphs={use_graphs} step {i}: max |logit - reference| = {err:.3f} > {LOGIT_TOL}"
        print(f"{model_type} graphs={use_graphs}: max |logit - reference| over {steps} steps = {worst:.4f}")
    if len(runs) == 2:
        for i, ((ig, lg), (ie, le)) in enumerate(zip(runs[True], runs[False])):
            assert ig == ie and np.array_equal(lg, le), f"step {i}: graph and eager differ"
    return runs, fused, linears


def test_qwen3_matches_transformers_graph_and_eager(gpu_device, monkeypatch):
    """f16: every id equals the fixture's, every logit is within the Llama fixtures' bar, graph and eager agree bit for bit,
    and no GEMM + rope launch was made (the Python entry of either is never called, while a graph is captured or eagerly) or
    prepared (no rope image): the norm sits between the two."""
    _runs, fused, linears = _against_fixture("qwen3", monkeypatch)
    assert fused == [] and all(lin.rope_handle is None and lin.rope_heads is None for lin in linears)


def test_the_q_k_norm_is_what_makes_it_match(gpu_device):
    """The Qwen3 tensors loaded as model_type "llama" (the norm tensors ignored) leave the fixture at the first step: the
    feature's test, it fails on a build that skips the norm."""
    meta, _ids, logits = _fixture("qwen3")
    lm, tok = _build("qwen3", meta["seed"], as_type="llama")
    _got_ids, got_logits = _run(lm, tok, meta["prompts"], meta["max_new"], 1)[0]
    err = np.abs(got_logits - logits[:, 0]).max(axis=1)
    assert (err > LOGIT_TOL).all(), err


def test_qwen2_matches_transformers_graph_and_eager(gpu_device, monkeypatch):
    """As for Qwen3.  Whether a decode step takes the GEMM + rope launch (with the q/k/v bias in its epilogue) is the linear's
    own rule, which at this size says no unless TGIS_ROPE_MIN_BLOCKS is lowered: the launches counted are those the rule
    chose; test_qwen2_takes_the_fused_rope_launch runs the other side."""
    _runs, fused, linears = _against_fixture("qwen2", monkeypatch)
    assert all(lin.rope_heads == (4, 2, 64) and lin.bias is not None for lin in linears)
    assert bool(fused) == any(lin.rope_handle is not None for lin in linears)


def _qwen2_child():
    """In a fresh process with TGIS_ROPE_MIN_BLOCKS=1 (read once per process): the Qwen2 fixture over the GEMM + rope launch."""
    mp = pytest.MonkeyPatch()
    try:
        _runs, fused, linears = _against_fixture("qwen2", mp, graph_modes=(True,))
    finally:
        mp.undo()
    assert fused and set(fused) == {"dense_gemm_rope"} and all(lin.rope_handle is not None for lin in linears), fused
    print("ok", len(fused), flush=True)


def test_qwen2_takes_the_fused_rope_launch(gpu_device):
    """Qwen2 declares its rope heads, so where the launch rule allows it decode steps take the GEMM + rope launch: one was made,
    and ids and logits are still the fixture's."""
    env = dict(os.environ, TGIS_ROPE_MIN_BLOCKS="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [root, os.path.join(root, "text-generation-inference_amd")]
    code = f"import sys; sys.path[:0] = {paths!r}; import tests.test_qwen_model_gpu as t; t._qwen2_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240, cwd=root)
    assert r.returncode == 0 and "ok" in r.stdout, f"child: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"


def test_qwen3_behind_a_shared_header(gpu_device):
    """kv_prefix_reuse: B shares A's first 64 tokens, so its prefill writes behind past_lens = 64 (the page-wise form with
    past_lens) and attends over A's pages.  Held to the option-off run of the same requests by the bar the prefix-reuse model
    test holds its runs to."""
    meta, _ids, _logits = _fixture("qwen3")
    rng = np.random.default_rng(7)
    A = rng.integers(3, 256, size=70).tolist()
    B = A[:64] + rng.integers(3, 256, size=10).tolist()
    runs = {}
    for reuse in (True, False):
        lm, tok = _build("qwen3", meta["seed"], kv_prefix_reuse=reuse)
        tap = _LogitTap(lm)
        a = _from_pb(lm, tok, _pb([A], 8))
        _step(lm, a, tap, first=True)
        b = _from_pb(lm, tok, _pb([B], 8, first_id=1, batch_id=1))
        rows = [_step(lm, b, tap, first=True)]
        assert b.reused_lengths == ([64] if reuse else [0])  # (set when the prefill takes its pages)
        rows += [_step(lm, b, tap) for _ in range(5)]
        runs[reuse] = [([t.token_id for t in toks], logits) for toks, logits in rows]
    for i, ((ir, lr), (ip, lp)) in enumerate(zip(runs[True], runs[False])):
        err = float(np.abs(lr - lp).max())
        assert err <= LOGIT_TOL and ir == ip, f"step {i}: reuse on vs off: ids {ir} / {ip}, max |logit difference| {err:.3f}"


def test_qwen3_with_prompt_lookup_speculation(gpu_device):
    """spec_tokens = 3 (lookup drafter, greedy): verify steps carry 4 rows per request through the per-token launch; all 50 ids
    each request emits are the fixture's, which are the plain run's (test_qwen3_matches_transformers_graph_and_eager)."""
    meta, ids, _logits = _fixture("qwen3")
    lm, tok = _build("qwen3", meta["seed"], spec_tokens=3)
    batch = _from_pb(lm, tok, _pb(meta["prompts"], meta["max_new"]))
    out = {i: [] for i in range(len(meta["prompts"]))}
    first, limit = True, 3 * meta["max_new"]
    while batch is not None and limit:
        with lm.context_manager():
            toks, _in, errs, _ns = lm.generate_token(batch, first=first, for_concat=first)
        first, limit = False, limit - 1
        assert not errs
        for t in toks:
            out[t.request_id].append(t.token_id)
        done = [r.id for r in batch.requests if len(out[r.id]) >= meta["max_new"]]
        if done:
            with lm.context_manager():
                batch = lm.batch_type.prune(batch, done)
    assert batch is None and lm.kv_cache.free_pages == lm.kv_cache.num_pages
    stats = lm.spec_stats()
    print(f"spec: {stats}")
    for r, got in out.items():
        assert got == ids[r].tolist(), f"request {r}: {got} != {ids[r].tolist()}"


def _gptq_pair(seed):
    """(GPTQ tensors, f16 tensors of their dequantisation) of the Qwen3 checkpoint: q/k/v/o and the MLP quantised by the helper
    of the tiny GPTQ tests (oracle.tiny_models.quantize_gptq), everything else as it is."""
    from oracle.tiny_models import dense_state_dict, quantize_gptq

    cfg = TinyQwenConfig("qwen3")
    q = {}
    for name, v in tiny_qwen_tensors(cfg, seed).items():
        if name.endswith("_proj.weight"):
            qw, qz, sc, gi = quantize_gptq(v.float().t().contiguous(), GROUPSIZE)
            base = name[:-len(".weight")]
            q.update({f"{base}.qweight": torch.from_numpy(qw), f"{base}.qzeros": torch.from_numpy(qz),
                      f"{base}.scales": torch.from_numpy(sc), f"{base}.g_idx": torch.from_numpy(gi)})
        else:
            q[name] = v
    dense = {k: v.half() for k, v in dense_state_dict(cfg, q, GROUPSIZE).items()}
    for t in (q, dense):
        t["lm_head.weight"] = t["model.embed_tokens.weight"]
    return q, dense


def test_qwen3_gptq_matches_the_f16_model_of_its_dequantised_weights(gpu_device):
    """GPTQ q/k/v/o and MLP (the int4 GEMM leaves its split-K sum to the norm + rope launch) against the f16 model built from
    the dequantised weights: logits within the bar, ids equal wherever that model's top-2 margin exceeds 0.7, and more than
    half of the rows are decided by such a margin."""
    meta, _ids, _logits = _fixture("qwen3")
    seed = meta["seed"] if GPTQ_SEED is None else GPTQ_SEED
    q, dense = _gptq_pair(seed)
    steps = 20
    lm, tok = _build("qwen3", seed, tensors=dense)
    want = _run(lm, tok, meta["prompts"], meta["max_new"], steps)
    lm, tok = _build("qwen3", seed, tensors=q, quantize="gptq", engine_kw=dict(gptq_groupsize=GROUPSIZE))
    got = _run(lm, tok, meta["prompts"], meta["max_new"], steps)
    decided, worst = 0, 0.0
    for i, ((gi, gl), (wi, wl)) in enumerate(zip(got, want)):
        err = float(np.abs(gl - wl).max())
        worst = max(worst, err)
        assert err <= LOGIT_TOL, f"step {i}: max |logit - f16 model| = {err:.3f} > {LOGIT_TOL}"
        top2 = np.sort(wl, axis=1)[:, -2:]
        clear = top2[:, 1] - top2[:, 0] > 2 * LOGIT_TOL
        decided += int(clear.sum())
        assert all(g == w for g, w, c in zip(gi, wi, clear) if c), f"step {i}: ids {gi} != {wi} (clear margins: {clear})"
        if gi != wi:
            break  # (a near-tie went the other way: the sequences differ from here on)
    print(f"gptq: max |logit - f16 model| = {worst:.4f}; {decided} of {3 * steps} rows decided by a margin above {2 * LOGIT_TOL}")
    assert decided > 3 * steps // 2


def _tp_worker(rank, world, port, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    meta, ids, _logits = _fixture("qwen3")
    lm, tok = _build("qwen3", meta["seed"], kv_cache_pages=32)
    assert lm.ranks.world == world and lm.num_heads == 4 // world and lm.num_kv_heads == 2 // world
    got = _run(lm, tok, meta["prompts"], meta["max_new"], 6)
    ret[rank] = got
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_qwen3_on_two_tensor_parallel_ranks(gpu_device):
    """World size 2 on one device (tests/test_tp_gpu.py's harness: gloo collectives): the norm weights are whole on both
    ranks, each normalises its own heads; ranks agree bit for bit and are within the bar of the fixture."""
    import torch.multiprocessing as mp

    from tests.test_tp_gpu import _free_port, _spawn

    meta, ids, logits = _fixture("qwen3")
    ret = mp.get_context("spawn").Manager().dict()
    _spawn(_tp_worker, (2, _free_port(), ret), 2)
    for i, ((i0, l0), (i1, l1)) in enumerate(zip(ret[0], ret[1])):
        assert i0 == i1 and np.array_equal(l0, l1), f"step {i}: the ranks differ"
        err = float(np.abs(l0 - logits[:, i]).max())
        assert i0 == ids[:, i].tolist() and err <= LOGIT_TOL, f"step {i}: ids {i0}, max |logit - reference| = {err:.3f}"
