"""-m gpu: which native launch serves each projection of one Llama decoder layer, for every weight format.

One FlashLlamaLayer forward per case runs under a recorder that wraps the real `native` functions and calls through.  The
recorded sequence (function, act, layout of the operand, layout of the result) must equal the sequence spelled out in
`_expected`, which is built from the library's own host-only answers (tgis_gptq_rope_ok, tgis_gptq_fragments_ok,
tgis_dense_rope_ok, tgis_gptq_gemm_fused_rows) and from the row thresholds of the default environment — never from a run of
the layer.  The layer's output is compared with oracle/llama_ref.py at the f16 tolerance of tests/test_model_gpu.py.

Shapes: hidden 1024, 8 heads and 8 kv heads of 128, group size 128, f16; intermediate size 1024, and 512 once.  There every
fused form is taken at some row count and refused at another (`_preconditions` asserts it), so both sides of each decision
are pinned: decode steps of 1, 32, 33, 64 and 65 rows over a 3-token context, a fresh prefill of 40 tokens in two
sequences, and one of 300 tokens (prefill-sized M: the tall kernel, or dequantise + library GEMM)."""
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gptq8_ref  # noqa: E402

from oracle import ops_ref  # noqa: E402
from oracle.llama_ref import LlamaRef  # noqa: E402
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors  # noqa: E402

pytestmark = pytest.mark.gpu

E, H, D, GS = 1024, 8, 128, 128
G = E // GS
TOL = 0.35  # tests/test_model_gpu.py LOGIT_TOL[torch.float16]
PARTIAL_MAX_M = SKINNY_MAX_M = 256  # rows up to which a GEMM defers its split-K sum / the dense streaming kernel runs
GPTQ8_MAX_M = 64
CONTEXT = 3  # tokens every sequence of a decode case has in the cache
KINDS = {"int4": 1024, "int4-act-order": 1024, "int8": 1024, "dense": 1024, "int4-i512": 512}
STEPS = [("decode", [1] * r) for r in (1, 32, 33, 64, 65)] + [("prefill", [25, 15]), ("prefill", [200, 100])]
RECORDED = ("rmsnorm_residual", "gptq_gemm", "gptq_gemm_partial", "gptq_gemm_rope", "gptq8_gemm", "dense_gemm",
            "dense_gemm_partial", "dense_gemm_rope", "act_mul", "rope_kv_write", "rope_kv_write_prefill", "attn_paged")


def _layout(native, t):
    return "frag" if isinstance(t, native.FragAct) else "partial" if isinstance(t, native.Partial) else "rows"


class _Recorder:
    """Wraps the real functions of RECORDED on the `native` module; each call goes through and leaves
    (name, act, layout of the first operand, layout of the result)."""

    def __init__(self, native, monkeypatch):
        self.native, self.calls = native, []
        for name in RECORDED:
            monkeypatch.setattr(native, name, self._wrap(name, getattr(native, name)))

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def call(*a, **kw):
            out = real(*a, **kw)
            args = sig.bind(*a, **kw).arguments
            res = args["out"] if name == "attn_paged" else out[0] if isinstance(out, tuple) else out
            self.calls.append((name, args.get("act", 0), _layout(self.native, next(iter(args.values()))),
                               _layout(self.native, res)))
            return out

        return call


def _answers(lib, kind, I):
    """The library's host-only answers for this layer's int4 / dense projections, by row count."""
    ao = int(kind == "int4-act-order")
    frag = lambda rows, K, N, act: bool(rows <= 64 and lib.tgis_gptq_fragments_ok(rows, K, N, K // GS, ao, act))
    if kind == "dense":
        rope = lambda rows: bool(lib.tgis_dense_rope_ok(rows, E, 3 * E, D))
    else:
        rope = lambda rows: bool(lib.tgis_gptq_rope_ok(rows, E, 3 * E, G, ao, D))
    image = any(rope(m) for m in (1, 32, 64))  # the rope image is only built where it serves some decode batch
    return dict(rope=lambda rows: image and rows <= 64 and rope(rows), qkv_frag=lambda rows: image and frag(rows, E, 3 * E, 3),
                o_frag=lambda rows: frag(rows, E, E, 0), mlp_frag=lambda rows: frag(rows, E, 2 * I, 2),
                down_frag=lambda rows: frag(rows, I, E, 0),
                fused_rows=lambda K, act: lib.tgis_gptq_gemm_fused_rows(K, K // GS, ao, act))


def _preconditions(lib):
    """Every fused form is taken on one side and refused on the other at these shapes."""
    a, ao, d, small = (_answers(lib, k, KINDS[k]) for k in ("int4", "int4-act-order", "dense", "int4-i512"))
    for x in (a, d):
        assert [x["rope"](r) for r in (1, 32, 33, 64)] == [True, True, False, False]
    assert not any(ao["rope"](r) or ao["qkv_frag"](r) or ao["o_frag"](r) for r in (1, 32, 64))
    assert [a["qkv_frag"](r) for r in (1, 32, 33, 64)] == [True, True, False, False]
    assert all(a["mlp_frag"](r) for r in (1, 32, 33, 64)) and not a["mlp_frag"](65)
    assert not any(small["mlp_frag"](r) for r in (1, 32, 33, 64, 65))
    for f in (a["o_frag"], a["down_frag"], small["down_frag"]):
        assert all(f(r) for r in (1, 32, 33, 64)) and not f(65)
    assert [a["fused_rows"](E, act) for act in (0, 1, 2)] == [3072, 256, 3072]
    assert [ao["fused_rows"](E, act) for act in (0, 1, 2)] == [256, 256, 256]


def _expected(lib, kind, I, step, rows):
    """The launches of one layer forward, in order: (native function, act, operand layout, result layout)."""
    decode = step == "decode"
    ans = _answers(lib, kind, I)
    seq = []

    def linear(K, act=0, operand="rows"):
        """A projection asked for partial=True (not the [gate | up] one); returns the layout of its result."""
        if kind == "dense":
            if rows <= PARTIAL_MAX_M:
                seq.append(("dense_gemm_partial", act, operand, "partial"))
                return "partial"
            if act:
                seq.append(("act_mul", 0, "rows", "rows"))  # then the library GEMM
        elif kind == "int8":
            if rows <= GPTQ8_MAX_M:
                seq.append(("gptq8_gemm", act, operand, "rows"))
            elif act:
                seq.append(("act_mul", 0, "rows", "rows"))  # then dequantise + library GEMM
        elif rows <= PARTIAL_MAX_M:
            seq.append(("gptq_gemm_partial", act, operand, "partial"))
            return "partial"
        elif rows <= ans["fused_rows"](K, act):
            seq.append(("gptq_gemm", act, operand, "rows"))
        elif act:
            seq.append(("act_mul", 0, "rows", "rows"))
        return "rows"

    fragments = decode and kind.startswith("int4")
    qkv_frag = fragments and ans["qkv_frag"](rows)
    seq.append(("rmsnorm_residual", 0, "rows", "frag" if qkv_frag else "rows"))
    if qkv_frag or (decode and kind != "int8" and ans["rope"](rows)):
        seq.append(("dense_gemm_rope" if kind == "dense" else "gptq_gemm_rope", 0, "frag" if qkv_frag else "rows", "rows"))
    else:
        qkv = linear(E)
        page_wise = not decode and qkv != "partial"  # a fresh prefill writes the cache page-wise unless the sum is deferred
        seq.append(("rope_kv_write_prefill" if page_wise else "rope_kv_write", 0, qkv, "rows"))
    o_frag = fragments and ans["o_frag"](rows)
    seq.append(("attn_paged", 0, "rows", "frag" if o_frag else "rows"))
    attn_out = linear(E, operand="frag" if o_frag else "rows")
    if kind == "int8":  # no SiLU * up epilogue: down_proj takes [gate | up] with act 1
        seq.append(("rmsnorm_residual", 0, attn_out, "rows"))
        linear(E)
        linear(I, act=1)
        return seq
    mlp_frag = fragments and ans["mlp_frag"](rows)
    seq.append(("rmsnorm_residual", 0, attn_out, "frag" if mlp_frag else "rows"))
    down_frag = mlp_frag and ans["down_frag"](rows)
    if kind == "dense":
        seq.append(("dense_gemm", 2, "rows", "rows") if rows <= SKINNY_MAX_M else ("act_mul", 0, "rows", "rows"))
    elif mlp_frag or rows <= ans["fused_rows"](E, 2):
        seq.append(("gptq_gemm", 2, "frag" if mlp_frag else "rows", "frag" if down_frag else "rows"))
    else:
        seq.append(("act_mul", 0, "rows", "rows"))  # behind dequantise + library GEMM
    linear(I, operand="frag" if down_frag else "rows")
    return seq


_LAYERS = {}


def _layer(kind, device):
    """(FlashLlamaLayer, oracle, config) of one weight kind, built once."""
    if kind not in _LAYERS:
        from tgis_amd.models.custom_modeling.flash_llama_modeling import FlashLlamaLayer, LlamaConfig
        from tgis_amd.utils.dist import FakeGroup
        from tgis_amd.utils.weights import DictWeights

        cfg = TinyLlamaConfig(vocab_size=32, hidden_size=E, intermediate_size=KINDS[kind], num_hidden_layers=1,
                              num_attention_heads=H, num_key_value_heads=H)
        if kind == "dense":
            tensors = tiny_llama_tensors(cfg, 3)
            ref = LlamaRef(cfg, tensors)
        elif kind == "int8":
            tensors = gptq8_ref.tiny_llama8_tensors(cfg, 3, GS)
            ref = LlamaRef(cfg, gptq8_ref.dense_tensors(tensors, GS))
        else:
            tensors = tiny_llama_tensors(cfg, 3, quantize="gptq", groupsize=GS, act_order=kind == "int4-act-order")
            ref = LlamaRef(cfg, tensors, quantize="gptq", groupsize=GS)
        pcfg = LlamaConfig(**cfg.to_dict())
        pcfg.quantize = None if kind == "dense" else "gptq"
        weights = DictWeights({k: v.clone() for k, v in tensors.items()}, device, torch.float16, FakeGroup(0, 1))
        weights.gptq_bits, weights.gptq_groupsize = (8 if kind == "int8" else 4), GS
        _LAYERS[kind] = (FlashLlamaLayer(0, pcfg, weights), ref, cfg)
    return _LAYERS[kind]


def _forward(native, layer, ref, cfg, state, cache, block_tables, x, lens, past, fresh):
    """One forward of `layer` and of the oracle over sum(lens) tokens: sequence b's tokens sit at cache positions
    past .. past + lens[b] - 1.  Returns (product hidden stream after the layer, the oracle's), both fp32 on the host."""
    from tgis_amd.models.custom_modeling.flash_llama_modeling import KVArgs

    dev = x.device
    pos = torch.cat([torch.arange(past, past + n) for n in lens]).int()
    seq = [b for b, n in enumerate(lens) for _ in range(n)]
    slots = (block_tables.cpu()[torch.tensor(seq), pos.long() // 32].long() * 32 + pos.long() % 32).int()
    cu = torch.tensor([0] + lens, dtype=torch.int32).cumsum(0).int()
    kv = KVArgs(cache=cache, block_tables=block_tables, ctx_lens=torch.tensor([past + n for n in lens], dtype=torch.int32, device=dev),
                slots=slots.to(dev), max_q_len=max(lens), max_ctx=past + max(lens), num_splits=1, fresh_prefill=fresh)
    cos, sin = layer.self_attn.rotary_emb.tables(torch.float16, dev, 512)
    out, res = layer(x, None, cos, sin, pos.to(dev), cu.to(dev), kv)
    # the next layer's add + RMSNorm finishes a deferred split-K sum: its residual output is the hidden stream
    _, hidden = native.rmsnorm_residual(out, res, torch.ones(E, dtype=torch.float16, device=dev), cfg.rms_norm_eps)
    torch.cuda.synchronize()
    rcos, rsin = ops_ref.rope_tables(D, cfg.rope_theta, 512, torch.float32)
    want, want_res = ref._layer(0, x.float().cpu(), None, rcos[pos.long()], rsin[pos.long()], seq, state, None)
    return hidden.float().cpu(), want + want_res


@pytest.mark.parametrize("kind", list(KINDS))
def test_layer_launches_and_output(gpu_device, monkeypatch, kind):
    from tgis_amd import native
    from tgis_amd.utils.kv_cache import PagedKVCache

    lib = native.load_library()
    _preconditions(lib)
    layer, ref, cfg = _layer(kind, gpu_device)
    g = torch.Generator().manual_seed(17)
    for step, lens in STEPS:
        B, rows = len(lens), sum(lens)
        pages = [(CONTEXT + n + 31) // 32 if step == "decode" else (n + 31) // 32 for n in lens]
        cache = PagedKVCache(1, H, D, sum(pages), torch.float16, gpu_device)
        block_tables = torch.zeros((B, max(pages)), dtype=torch.int32)
        first = 0
        for b, n in enumerate(pages):
            block_tables[b, :n] = torch.arange(first, first + n)
            first += n
        block_tables = block_tables.to(gpu_device)
        state = ref.new_state(B)
        past = 0
        if step == "decode":  # the context goes in through the same layer, unrecorded
            ctx = torch.randn(B * CONTEXT, E, generator=g).half().to(gpu_device)
            got, want = _forward(native, layer, ref, cfg, state, cache, block_tables, ctx, [CONTEXT] * B, 0, True)
            assert (got - want).abs().max() <= TOL
            past = CONTEXT
        x = torch.randn(rows, E, generator=g).half().to(gpu_device)
        with monkeypatch.context() as m:
            rec = _Recorder(native, m)
            got, want = _forward(native, layer, ref, cfg, state, cache, block_tables, x, lens, past, step == "prefill")
        calls = rec.calls[:-1]  # the last one is _forward's own closing add + RMSNorm
        err = float((got - want).abs().max())
        print(f"{kind} {step} {rows} rows: max |hidden - oracle| = {err:.4f}; " + " ".join(c[0] for c in calls))
        assert calls == _expected(lib, kind, KINDS[kind], step, rows), f"{kind}, {step} of {rows} rows"
        assert err <= TOL, f"{kind}, {step} of {rows} rows: max |hidden - oracle| = {err:.4f} > {TOL}"
