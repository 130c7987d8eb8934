"""-m gpu: the one-byte (e4m3) KV cache on its kernels.

Writers: every cache writer's *_kv8 form writes, into a pool that starts as a sentinel byte, exactly the codes of the restated
quantiser (kv_fp8_ref.quantize) of what its 16-bit form writes into a NaN-filled pool, and nothing else; q and the qkv
activation are bit for bit those of the 16-bit form.  Attention: the launch forms of test_attention_edges_gpu.py over e4m3
pools packed on the host, against the fp32 oracle on the dequantised K / V, with unwritten slots holding +-448."""
import functools
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
import kv_fp8_ref as q8  # noqa: E402
import test_attention_edges_gpu as edges  # noqa: E402
import test_gemm_edges_gpu as gemm_edges  # noqa: E402

from oracle import ops_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
SENTINEL = 0x5A  # 3.25 in e4m3: a byte no writer produces from these inputs by accident at the checked places


def _nat():
    from tgis_amd import native

    native.load_library()
    return native


def _pools(pages, Hkv, D, dtype, dev):
    k16 = torch.full((pages, Hkv, 32 * D), float("nan"), dtype=dtype, device=dev)
    k8 = torch.full((pages, Hkv, 32 * D), SENTINEL, dtype=torch.uint8, device=dev)
    return k16, k16.clone(), k8, k8.clone()


def _check_pools(p16, p8, scale, what):
    """p8 holds quantize(p16 / scale) wherever the 16-bit writer wrote, the sentinel elsewhere."""
    p16, p8 = p16.cpu(), p8.cpu()
    written = ~torch.isnan(p16.float())
    assert written.any(), f"{what}: nothing written"
    want = torch.where(written, q8.quantize(torch.nan_to_num(p16), scale), torch.tensor(SENTINEL, dtype=torch.uint8))
    bad = want != p8
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} bytes differ (first at {bad.nonzero()[0].tolist()}: "
                           f"{int(p8[bad][0])} vs {int(want[bad][0])})")
    assert not ((p8 == 0x7F) | (p8 == 0xFF)).any(), f"{what}: a NaN code in the pool"


# (name, dtype, H, Hkv, D, rot or None (no rotary), k_scale, v_scale, lens)
WRITERS = [
    ("llama-gqa-d128-f16", F16, 8, 2, 128, 128, 1.0, 1.0, [1, 31, 32, 33, 70]),
    ("llama-mha-d64-bf16-scaled", BF16, 4, 4, 64, 64, 0.5, 2.0, [3, 64, 17]),
    ("neox-d96-rot24-f16", F16, 4, 4, 96, 24, 1.0, 1.0, [5, 40]),  # partial span off the 16-element grid (GEN)
    ("neox-d64-rot16-bf16", BF16, 4, 4, 64, 16, 0.25, 4.0, [33, 2]),  # partial span on the grid
    ("bigcode-mqa-d128-f16-norope", F16, 8, 1, 128, None, 1.0, 1.0, [1, 45, 32]),  # cos == NULL (santacoder)
    ("bigcode-mqa-d64-bf16-norope-big", BF16, 8, 1, 64, None, 0.125, 0.125, [9, 100]),  # |x / s| past 448: saturates
    ("llama-d128-f16-scale0.7", F16, 8, 2, 128, 128, 0.7, 1.3, [4, 33]),  # x / s correctly rounded, not a reciprocal
    # the launch forms of choose_rope (csrc/rope_kv.hip): T <= 64 spreads a token over gy = ceil(items / 256) <= 16 blocks,
    # and past gy * 256 items the blocks stride; T > 64 takes one block per token, striding from 256 items on
    ("gy3-gqa-d128-f16", F16, 32, 8, 128, 128, 0.7, 0.7, [1, 5, 20]),  # 768 items: 3 blocks per token
    ("gy16-strided-d128-bf16", BF16, 256, 8, 128, 128, 1.0, 1.0, [2, 3]),  # 4352 items > 16 x 256
    ("one-block-strided-d128-f16", F16, 32, 32, 128, 128, 0.7, 1.3, [70]),  # T 70: 1536 items on one block
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,rot,ks,vs,lens", WRITERS, ids=[w[0] for w in WRITERS])
def test_rope_writers_write_the_quantised_bytes(gpu_device, name, dtype, H, Hkv, D, rot, ks, vs, lens):
    nat = _nat()
    dev = gpu_device
    W = (H + 2 * Hkv) * D
    T = sum(lens)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    mag = 200.0 if name.endswith("big") else 0.5
    Kx = min(W // 2, 512)
    x = (torch.randn(T, Kx, generator=g) * 0.5).to(dtype)
    w = (torch.randn(W, Kx, generator=g) * mag * Kx ** -0.5).to(dtype)
    bias = (torch.randn(W, generator=g) * 0.1).to(dtype)
    npg = [(n + 31) // 32 for n in lens]
    pages = sum(npg) + 2
    perm = torch.randperm(pages, generator=g)
    bt = torch.full((len(lens), max(npg)), int(perm[-1]), dtype=torch.int32)
    o = 0
    for b, n in enumerate(npg):
        bt[b, :n] = perm[o:o + n].int()
        o += n
    pos = torch.cat([torch.arange(n) for n in lens]).int()
    slots = torch.cat([bt[b, torch.arange(n) // 32].long() * 32 + torch.arange(n) % 32 for b, n in enumerate(lens)]).int()
    cu = torch.tensor([0] + torch.tensor(lens).cumsum(0).tolist(), dtype=torch.int32)
    if rot is not None:
        cos, sin = (t.to(dev) for t in ops_ref.rope_tables(rot, 10000.0, 128, dtype))
        r = rot
    else:
        cos = sin = None
        r = D
    dpos, dslots, dcu, dbt = pos.to(dev), slots.to(dev), cu.to(dev), bt.to(dev)
    dw = nat.DenseWeight(w.to(dev))
    qkv = nat.dense_gemm(x.to(dev), dw, nat.Workspace(0, dev), bias=bias.to(dev))
    sc = (ks, vs)
    # per-token writer (qkv in place)
    k16, v16, k8, v8 = _pools(pages, Hkv, D, dtype, dev)
    a16, a8 = qkv.clone(), qkv.clone()
    nat.rope_kv_write(a16, cos, sin, dpos if cos is not None else None, dslots, k16, v16, H, Hkv, D, r)
    nat.rope_kv_write(a8, cos, sin, dpos if cos is not None else None, dslots, k8, v8, H, Hkv, D, r, kv_scales=sc)
    torch.cuda.synchronize()
    assert torch.equal(a16.view(torch.int16), a8.view(torch.int16)), f"{name}: qkv differs from the 16-bit writer"
    _check_pools(k16, k8, ks, f"{name} rope_kv_write k")
    _check_pools(v16, v8, vs, f"{name} rope_kv_write v")
    # split-K partial input
    part = nat.dense_gemm_partial(x.to(dev), dw, bias=bias.to(dev))
    k16, v16, k8, v8 = _pools(pages, Hkv, D, dtype, dev)
    b16 = nat.rope_kv_write(part, cos, sin, dpos if cos is not None else None, dslots, k16, v16, H, Hkv, D, r)
    b8 = nat.rope_kv_write(part, cos, sin, dpos if cos is not None else None, dslots, k8, v8, H, Hkv, D, r, kv_scales=sc)
    torch.cuda.synchronize()
    assert torch.equal(b16.view(torch.int16), b8.view(torch.int16)), f"{name}: partial qkv differs"
    _check_pools(k16, k8, ks, f"{name} rope_kv_write_partial k")
    _check_pools(v16, v8, vs, f"{name} rope_kv_write_partial v")
    # prefill page-wise writer (zeroes the tail of a last partial page)
    k16, v16, k8, v8 = _pools(pages, Hkv, D, dtype, dev)
    c16, c8 = qkv.clone(), qkv.clone()
    nat.rope_kv_write_prefill(c16, cos, sin, dpos if cos is not None else None, dcu, dbt, k16, v16, max(lens), H, Hkv, D, r)
    nat.rope_kv_write_prefill(c8, cos, sin, dpos if cos is not None else None, dcu, dbt, k8, v8, max(lens), H, Hkv, D, r,
                              kv_scales=sc)
    torch.cuda.synchronize()
    assert torch.equal(c16.view(torch.int16), c8.view(torch.int16)), f"{name}: prefill q differs"
    _check_pools(k16, k8, ks, f"{name} rope_kv_write_prefill k")
    _check_pools(v16, v8, vs, f"{name} rope_kv_write_prefill v")


ROPE_CASES = [c for c in gc.CASES if c["entry"] in ("gptq_rope", "dense_rope")]


@pytest.mark.parametrize("case", ROPE_CASES, ids=[c["id"] for c in ROPE_CASES])
def test_fused_qkv_rope_gemm_writes_the_quantised_bytes(gpu_device, case):
    """tgis_gptq_gemm_rope_f16_kv8 / tgis_dense_gemm_rope_kv8 at every plan tests/gemm_cases.py pins for the fused
    launch: q bit for bit the 16-bit launch's, k / v the codes of what it writes (scales 0.7 / 2)."""
    nat = _nat()
    c, dev = case, gpu_device
    gen = torch.Generator(device=dev)
    gen.manual_seed(zlib.crc32(c["id"].encode()))
    dense = c["entry"] == "dense_rope"
    w, _W = gemm_edges._dense_weight(c, gen, dev) if dense else gemm_edges._int4_weight(c, gen, dev)
    dt = w.dtype if dense else F16
    M, H, Hkv, D = c["M"], c["H"], c["Hkv"], c["D"]
    x = gemm_edges._activation(M, c["K"], dt, gen, dev)
    bias = (torch.randn(c["N"], generator=gen, device=dev) * 0.1).to(dt) if c.get("bias") else None
    cos, sin = (t.to(dev) for t in ops_ref.rope_tables(D, 10000.0, 4096, dt))
    pos = torch.randint(0, 4096, (M,), generator=gen, device=dev, dtype=torch.int32)
    pages = (M + 31) // 32 + 2
    slots = torch.randperm(pages * 32, generator=gen, device=dev)[:M].to(torch.int32)
    xa = nat.FragAct.from_rows(x.contiguous()) if c.get("frag_in") else x
    fn = nat.dense_gemm_rope if dense else nat.gptq_gemm_rope
    k16, v16, k8, v8 = _pools(pages, Hkv, D, dt, dev)
    q16 = fn(xa, w, bias, cos, sin, pos, slots, k16, v16, H, Hkv, D)
    q8_ = fn(xa, w, bias, cos, sin, pos, slots, k8, v8, H, Hkv, D, kv_scales=(0.7, 2.0))
    torch.cuda.synchronize()
    assert torch.equal(q16[:, :H * D].view(torch.int16), q8_[:, :H * D].view(torch.int16)), f"{c['id']}: q differs"
    _check_pools(k16, k8, 0.7, f"{c['id']} k")
    _check_pools(v16, v8, 2.0, f"{c['id']} v")


# ---- attention over e4m3 pools ------------------------------------------------------------------------------------------
def _to_fp8(c, ks, vs):
    """Turn an edges._Case into its one-byte form: K / V replaced by their dequantised codes (what the oracle sees), the pools
    by e4m3 pools of +-448 (the largest finite code) with the real tokens' codes packed on the host."""
    g = torch.Generator().manual_seed(len(c.seqs) * 7 + c.D)
    total, Hkv, D = c.kpool.shape[0], c.Hkv, c.D

    def poisoned():
        sign = torch.randint(0, 2, (total, Hkv, 32 * D), generator=g, dtype=torch.uint8)
        return torch.where(sign == 1, torch.tensor(0x7E, dtype=torch.uint8), torch.tensor(0xFE, dtype=torch.uint8))

    k8, v8 = poisoned(), poisoned()
    bt = c.bt.cpu()
    for b, (_ql, ctx) in enumerate(c.seqs):
        Kc, Vc = q8.quantize(c.K[b], ks), q8.quantize(c.V[b], vs)
        c.K[b] = q8.dequantize(Kc, ks).to(c.dtype)  # exact: e4m3 times a power of two is an f16 / bf16 value
        c.V[b] = q8.dequantize(Vc, vs).to(c.dtype)
        for j in range((ctx + 31) // 32):
            ops_ref.kv_page_pack(k8, v8, int(bt[b, j]), Kc[32 * j:32 * j + 32], Vc[32 * j:32 * j + 32])
    c.kpool, c.vpool = k8.to(c.dev), v8.to(c.dev)
    return c


@pytest.fixture
def scaled_attn(monkeypatch):
    """edges._Case.run calls native.attn_paged without scales: bind them for the test."""
    nat = _nat()
    orig = nat.attn_paged

    def bind(ks, vs):
        monkeypatch.setattr(nat, "attn_paged", functools.partial(orig, kv_scales=(ks, vs)))
    return bind


SCALES = [(1.0, 1.0), (0.5, 2.0)]


@pytest.mark.parametrize("ks,vs", SCALES, ids=["unit", "scaled"])
@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens", edges.SHORT, ids=[c[0] for c in edges.SHORT])
def test_fp8_short_prefill_on_the_decode_kernel(gpu_device, scaled_attn, name, dtype, H, Hkv, D, lens, ks, vs):
    c = _to_fp8(edges._Case(gpu_device, dtype, H, Hkv, D, [(l, l) for l in lens], seed=H * D + len(lens)), ks, vs)
    scaled_attn(ks, vs)
    c.check(c.run(1), c.want(), name)


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens", edges.PREFILL, ids=[c[0] for c in edges.PREFILL])
def test_fp8_multi_tile_prefill_kernel(gpu_device, scaled_attn, name, dtype, H, Hkv, D, lens):
    c = _to_fp8(edges._Case(gpu_device, dtype, H, Hkv, D, [(l, l) for l in lens], seed=H + Hkv + D), 2.0, 0.5)
    scaled_attn(2.0, 0.5)
    assert edges._form(H, Hkv, c.max_q, 1) == "prefill"
    c.check(c.run(1), c.want(), name)


FILL = [("mha-d128-f16", F16, 8, 8, 128), ("gqa8-d64-bf16", BF16, 32, 4, 64), ("neox-d96-f16", F16, 8, 8, 96),
        ("mqa48-d128-bf16", BF16, 48, 1, 128)]


@pytest.mark.parametrize("name,dtype,H,Hkv,D", FILL, ids=[f[0] for f in FILL])
def test_fp8_decode_every_fill_of_the_last_page(gpu_device, scaled_attn, name, dtype, H, Hkv, D):
    """q_len 1 over ctx 33 .. 64 (every fill of a second page, its unwritten tail +-448) and over 1 .. 32."""
    scaled_attn(0.5, 2.0)
    for lo in (1, 33):
        c = _to_fp8(edges._Case(gpu_device, dtype, H, Hkv, D, [(1, n) for n in range(lo, lo + 32)], seed=lo + D), 0.5, 2.0)
        c.check(c.run(1), c.want(), f"{name} ctx {lo}..{lo + 31}")


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens", [
    ("g1-d128-f16", F16, 16, 16, 128, [(5, 300), (1, 77), (40, 41)]),
    ("g8-d64-bf16", BF16, 32, 4, 64, [(3, 129), (8, 1000), (1, 2)]),
    ("mqa48-d96-f16", F16, 48, 1, 96, [(2, 64), (1, 500)]),
    ("prefill-g1-d128-bf16", BF16, 8, 8, 128, [(100, 400), (70, 70)]),
], ids=lambda v: v if isinstance(v, str) else None)
def test_fp8_new_tokens_over_a_longer_context(gpu_device, scaled_attn, name, dtype, H, Hkv, D, lens):
    c = _to_fp8(edges._Case(gpu_device, dtype, H, Hkv, D, lens, seed=D + len(lens)), 0.5, 0.5)
    scaled_attn(0.5, 0.5)
    c.check(c.run(1), c.want(), name)


# the long-context cases of the 16-bit tests at 9 - 33 splits, and 64 splits over a shorter context (2 - 4 pages per split)
SPLITS = [s for s in edges.SPLITS if "ns64" not in s[0] and "ctx16384" not in s[0]] + [
    ("g8-fused-explicit-ns64", F16, 8, 1, 128, [8192], 64, False),
    ("g8x8kv-fused-explicit-ns64", BF16, 64, 8, 64, [4096, 2000], 64, False),
    ("mqa48-combine-explicit-ns64", BF16, 48, 1, 128, [4096], 64, False),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens,ns,by_rule", SPLITS, ids=[s[0] for s in SPLITS])
def test_fp8_split_decode(gpu_device, scaled_attn, name, dtype, H, Hkv, D, lens, ns, by_rule):
    """9 - 33 key splits through the in-launch merge (single-chunk groups) and the combine launch (MQA), and splits a
    sequence does not reach; NaN guards behind `out` and the workspace are checked by edges._Case.run."""
    c = _to_fp8(edges._Case(gpu_device, dtype, H, Hkv, D, [(1, l) for l in lens], seed=ns + D + len(lens)), 0.5, 2.0)
    scaled_attn(0.5, 2.0)
    if by_rule:
        assert _nat().attn_num_splits(len(lens), Hkv, H, 1, max(lens)) == ns
    c.check(c.run(ns), c.want(), name, long=True)
