"""-m gpu: every launch that addresses a KV pool by page id, and the key-split workspace, at offsets on both sides of 2^31
and 2^32 elements.

The small cases of the existing GPU files run twice: on their ordinary pools ("near") and moved, data and launch unchanged, to
far page ids inside one device arena (tests/far_pool.py, whose arithmetic tests/test_far_pool_cpu.py checks).  The arena holds
the pool dtype's NaN pattern everywhere else and reaches 2^31 elements below the pools' base, so an offset computed in 32 bits
reads NaN, or writes where the check of the rest of the arena finds it, instead of leaving memory the test owns.

Readers: the far output is bit-identical to the near one (nothing in the arithmetic depends on a page id) and meets the case's
existing oracle at its existing bar.  Writers: every returned activation is bit-equal, the far blocks gathered by far id equal
the near pool's pages bit for bit, and every other word of the arena still holds the fill.  The split workspace runs at the
two batch sizes on either side of the 2 GiB guard of its 32-bit record offsets (csrc/attention_plan.h)."""
import functools
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases  # noqa: E402
import attn_window_ref as wref  # noqa: E402
import far_pool as fp  # noqa: E402
import spec_tree_ref as tref  # noqa: E402
import test_attention_edges_gpu as edges  # noqa: E402
import test_attn_qsplit_gpu as qsplit  # noqa: E402
import test_attn_window_gpu as window  # noqa: E402
import test_gemm_edges_gpu as gemm_edges  # noqa: E402
import test_kv_absmax_gpu as absmax  # noqa: E402
import test_kv_fp8_ops_gpu as fp8ops  # noqa: E402
import test_spec_tree_ops_gpu as tree  # noqa: E402

from oracle import ops_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, U8 = torch.float16, torch.bfloat16, torch.uint8
FP8_SCALES = (0.5, 2.0)
WS_CASE_BYTES = 5 * fp.GIB // 2  # section "split workspace": a 2.06 GiB workspace, its activations and outputs


def _nat():
    return edges._nat()


@pytest.fixture(scope="module")
def arena(gpu_device):
    need = fp.ARENA_BYTES + WS_CASE_BYTES
    free = torch.cuda.mem_get_info(gpu_device)[0]
    if free < need + fp.GIB:
        pytest.skip(f"{free} bytes of device memory are free, this module needs {need} and 1 GiB to spare")
    a = fp.Arena(gpu_device)
    yield a
    a.release()
    del a
    torch.cuda.empty_cache()


@pytest.fixture
def fp8_scales(monkeypatch):
    """The e4m3 cases: edges._Case.run and its kin call native.attn_paged without scales."""
    def bind():
        nat = _nat()
        monkeypatch.setattr(nat, "attn_paged", functools.partial(nat.attn_paged, kv_scales=FP8_SCALES))
    return bind


def _bits(t):
    return fp._bits(t)


# ---- readers ------------------------------------------------------------------------------------------------------------------
def _relocate(arena, c, npages, first=()):
    """Move the pools and the block table of a case object (kpool, vpool, bt, Hkv, D) to far pages; the page map."""
    geom = fp.Geometry(c.Hkv, c.D, c.kpool.element_size())
    bt = c.bt.cpu()
    m = fp.page_map(geom, bt, npages, first=first)
    kfar, vfar = arena.pools(geom, c.kpool.dtype)
    arena.scatter(c.kpool, c.vpool, m)
    c.kpool, c.vpool, c.bt = kfar, vfar, fp.remap(bt, m).to(c.bt.device)
    used = sorted(set(m.values()))
    geom.check_aliases(used)
    geom.assert_crosses(used)
    if len(used) > len(geom.required()):
        geom.assert_mixed(used)
    return geom, m


def _near_far(arena, c, launches, first=()):
    """Every launch on the near pools, then on the far ones: bit-equal and finite.  The far outputs, the geometry, the map."""
    npages = [(s[1] + 31) // 32 for s in c.seqs]
    near = [run(c) for run in launches]
    geom, m = _relocate(arena, c, npages, first)
    far = [run(c) for run in launches]
    for i, (n, f) in enumerate(zip(near, far)):
        assert torch.isfinite(f).all(), f"launch {i}: non-finite output over the far pool: a load from a wrong address"
        assert torch.equal(n, f), (f"launch {i}: the far pool's output differs from the near pool's in "
                                   f"{int((n != f).sum())} of {n.numel()} values")
    return far, geom, m


HKV8 = [("hkv8-d128", 32, 8, 128), ("hkv8-d96", 32, 8, 96)]
# (form name, sequences, split counts, the launch form, the case class, the bound of `check` over long contexts)
FORMS = [
    ("decode", [(1, 1), (1, 33), (1, 97)], (1,), "decode", edges._Case, False),
    ("decode-2-and-5-splits", [(1, 1), (1, 97), (1, 200)], (2, 5), "fused merge", edges._Case, False),
    ("decode-q2-q5", [(2, 70), (5, 70)], (1,), "decode q>1", edges._Case, False),
    ("verify-rows-3-splits", [(4, 1027), (2, 1055)], (1, 3), "decode q>1", qsplit._QCase, True),
    ("prefill", [(97, 97), (200, 200), (5, 150)], (1,), "prefill", edges._Case, False),
]
ATTN = [(f"{g[0]}-{f[0]}-{dn}-{'e4m3' if fp8 else 'kv16'}", g, f, dt, fp8)
        for g in HKV8 for f in FORMS for dn, dt in (("f16", F16), ("bf16", BF16)) for fp8 in (False, True)
        if dt == F16 or f[0] in ("decode", "prefill")]
ATTN += [(f"mqa48-d128-combine-launch-{dn}-{'e4m3' if fp8 else 'kv16'}", ("mqa48-d128", 48, 1, 128),
          ("combine", [(1, 97), (1, 33), (1, 200)], (2,), "combine", edges._Case, False), dt, fp8)
         for dn, dt in (("f16", F16), ("bf16", BF16)) for fp8 in (False, True)]


@pytest.mark.parametrize("name,geom,form,dtype,fp8", ATTN, ids=[a[0] for a in ATTN])
def test_attn_paged(arena, gpu_device, fp8_scales, name, geom, form, dtype, fp8):
    _, H, Hkv, D = geom
    fname, seqs, splits, launch, cls, long = form
    c = cls(gpu_device, dtype, H, Hkv, D, seqs, seed=zlib.crc32(name.encode()) % 1000)
    if fp8:
        c = fp8ops._to_fp8(c, *FP8_SCALES)
        fp8_scales()
    for ns in splits:
        assert edges._form(H, Hkv, c.max_q, ns) == launch
    want = c.want()
    far, g, m = _near_far(arena, c, [functools.partial(cls.run, ns=ns) for ns in splits])
    for ns, got in zip(splits, far):
        c.check(got, want, f"{name}: far pool, {ns} split(s) against the oracle", long=long)
    if long:  # contexts of 1024 and more: a middle page of every sequence is a far page, not only its ends
        for b, (_ql, ctx) in enumerate(seqs):
            assert any(g.is_far(p) for p in c.bt[b, 1:(ctx + 31) // 32 - 1].tolist())


L23 = ("layout", 2, 3)
TREE = [(f"{g[0]}-{'split' if split else 'unsplit'}-{'e4m3' if fp8 else 'kv16'}", g, split, fp8)
        for g in HKV8 for split in (False, True) for fp8 in (False, True)]


@pytest.mark.parametrize("name,geom,split,fp8", TREE, ids=[t[0] for t in TREE])
def test_attn_paged_tree(arena, gpu_device, name, geom, split, fp8):
    """C 2, K 3 verify steps (7 rows) under spec_tree_ref.q_mask, unsplit and at 2 key splits."""
    _, H, Hkv, D = geom
    seqs = [(7, 1031, L23), (7, 1100, L23)] if split else [(7, 71, L23), (7, 102, L23), (7, 40, L23)]
    c = tree._TreeCase(gpu_device, F16, H, Hkv, D, seqs, seed=11 + split)
    assert c.words[0] == tref.q_mask(2, 3)
    if fp8:
        c = fp8ops._to_fp8(c, *FP8_SCALES)
        c.kv_scales = FP8_SCALES
    want = c.want()
    far, _, _ = _near_far(arena, c, [functools.partial(tree._TreeCase.run, ns=2 if split else 1)])
    c.check(far[0], want, f"{name}: far pool against the masked oracle", long=split)


WINDOW = [(f"w{W}-{mode}-{'e4m3' if fp8 else 'kv16'}", W, mode, fp8)
          for W in (40, 95) for mode in ("decode", "decode-2-splits", "prefill") for fp8 in (False, True)]


@pytest.mark.parametrize("name,W,mode,fp8", WINDOW, ids=[w[0] for w in WINDOW])
def test_attn_paged_window(arena, gpu_device, fp8_scales, name, W, mode, fp8):
    """The first visible page of every sequence is a far page; the table entries of the hidden pages name a NaN page."""
    H, Hkv, D = 32, 8, 128
    seqs = [(97, 97), (5, 150)] if mode == "prefill" else [(1, 300), (1, W + 1), (1, 136)]
    c = window._WCase(gpu_device, F16, H, Hkv, D, seqs, W, seed=W + len(mode),
                      to_fp8=(lambda x: fp8ops._to_fp8(x, *FP8_SCALES)) if fp8 else None)
    if fp8:
        fp8_scales()
    assert c.hidden_pages and window._form(c)["form"] == ("prefill" if mode == "prefill" else "window")
    ns = 2 if mode == "decode-2-splits" else 1
    firsts = [wref.first_visible_page(ctx, ql, W) for ql, ctx in seqs]
    first_near = [int(c.bt[b, f]) for b, f in enumerate(firsts)]
    want = c.want()
    far, g, m = _near_far(arena, c, [functools.partial(window._WCase.run, ns=ns)], first=first_near)
    c.check(far[0], want, f"{name}: far pool against the windowed restatement")
    for b, f in enumerate(firsts):
        assert g.is_far(int(c.bt[b, f])), "the first visible page is a far page"
        assert (c.bt[b, :f] == m[c.nan_page]).all()
    nan_block = arena.block(m[c.nan_page] * g.S)
    assert (nan_block == 0x7F).all() if fp8 else torch.isnan(nan_block.float()).all()


ABSMAX = [(f"hkv{Hkv}-d{D}-{dn}", Hkv, D, dt) for Hkv, D in ((8, 128), (8, 96), (1, 128)) for dn, dt in (("f16", F16), ("bf16", BF16))]


# eight sequences of one page each, then 2, 4 and 2 pages.  A maximum ignores NaN, so a page read from a wrong address does not
# show by itself: it shows where the page that was missed holds the maximum.  Every sequence keeps its largest |k| and |v| in
# its last token and is measured alone, so each of the one-page sequences' pages (they get the threshold pages) must be read.
ABSMAX_CTX = [32, 17, 1, 31, 16, 15, 9, 25, 33, 97, 64]


@pytest.mark.parametrize("name,Hkv,D,dtype", ABSMAX, ids=[a[0] for a in ABSMAX])
def test_kv_absmax(arena, gpu_device, name, Hkv, D, dtype):
    c = absmax._Case(gpu_device, dtype, Hkv, D, ABSMAX_CTX, seed=3 + D + Hkv)
    rows = [None] + [[b] for b in range(len(ABSMAX_CTX))]

    def launches():
        outs = []
        for r in rows:
            region, out = c.new_out()
            c.run(out, r)
            c.check(region, out, c.want(r), f"{name} rows {r}")  # bit-equal to the host recomputation, guards intact
            outs.append(out.cpu())
        return torch.stack(outs)

    near = launches()
    assert (near > 0).all()
    one_page = [int(c.bt[b, 0]) for b, n in enumerate(ABSMAX_CTX) if n <= 32]
    g, m = _relocate(arena, c, [(n + 31) // 32 for n in c.ctxs], first=one_page)
    assert {m[p] for p in one_page} >= set(g.required()[:len(g.required()) - 2]), "the one-page sequences sit on the far pages"
    assert torch.equal(launches(), near)


# ---- writers ------------------------------------------------------------------------------------------------------------------
def _near_pool(pages, Hkv, D, dtype, dev):
    p = torch.empty((pages, Hkv, 32 * D), dtype=dtype, device=dev)
    _bits(p).fill_(fp.FILL[dtype])
    return p


def _writer(arena, Hkv, D, pool_dtype, bt, npages, slots, call, what):
    """call(kpool, vpool, block table, slots) -> activations, on near pools of the fill pattern and on the arena."""
    dev = arena.words.device
    geom = fp.Geometry(Hkv, D, 1 if pool_dtype == U8 else 2)
    pages = int(bt.max()) + 1
    kn, vn = _near_pool(pages, Hkv, D, pool_dtype, dev), _near_pool(pages, Hkv, D, pool_dtype, dev)
    near = call(kn, vn, bt.to(dev), None if slots is None else slots.to(dev))
    m = fp.page_map(geom, bt, npages)
    kf, vf = arena.pools(geom, pool_dtype)
    far = call(kf, vf, fp.remap(bt, m).to(dev), None if slots is None else fp.remap(slots, m, per=32).to(dev))
    torch.cuda.synchronize()
    assert len(near) == len(far) and len(near) > 0
    for a, b in zip(near, far):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: an activation differs between the near and the far call"
    ids = sorted(m)
    koff, voff = [m[p] * geom.S for p in ids], [(m[p] + fp.VSHIFT) * geom.S for p in ids]
    for pool, offs, kv in ((kn, koff, "k"), (vn, voff, "v")):
        nb = _bits(pool)[ids].flatten(1)
        assert (nb != fp.FILL[pool_dtype]).any(), f"{what}: nothing was written to the near {kv} pool"
        bad = (arena.gather(offs) != nb).any(1).nonzero().flatten().tolist()
        assert not bad, f"{what}: far {kv} pages {[m[ids[i]] for i in bad]} differ from the near pool's {[ids[i] for i in bad]}"
    arena.restore(koff + voff)
    assert arena.untouched(), f"{what}: the arena outside the case's own page blocks was written"
    used = sorted(set(m.values()))
    geom.check_aliases(used)
    geom.assert_crosses(used)
    return geom, m


def _tables(lens_pages):
    """A block table of consecutive near pages, rows of lens_pages[b] pages, one spare page behind the unused entries."""
    total = sum(lens_pages)
    bt = torch.full((len(lens_pages), max(lens_pages) + 1), total, dtype=torch.int32)
    o = 0
    for b, n in enumerate(lens_pages):
        bt[b, :n] = torch.arange(o, o + n, dtype=torch.int32)
        o += n
    return bt


ROPE = [(f"hkv8-d{D}-rot{rot}-{dn}-{'e4m3' if fp8 else 'kv16'}", D, rot, dt, fp8)
        for D, rot in ((128, 128), (96, 24)) for dn, dt in (("f16", F16), ("bf16", BF16)) for fp8 in (False, True)]


@pytest.mark.parametrize("name,D,rot,dtype,fp8", ROPE, ids=[r[0] for r in ROPE])
def test_rope_kv_writers(arena, gpu_device, name, D, rot, dtype, fp8):
    """tgis_rope_kv_write, _partial, _prefill and _prefill_at (and their _kv8 forms): 5 decode tokens on five far pages,
    prefills of 33 and 70 tokens, the same behind 32 and 64 cached tokens."""
    nat, dev = _nat(), gpu_device
    H = Hkv = 8
    N = (H + 2 * Hkv) * D
    pool_dtype = U8 if fp8 else dtype
    kw = {"kv_scales": FP8_SCALES} if fp8 else {}
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    cos, sin = (t.to(dev) for t in ops_ref.rope_tables(rot, 10000.0, 256, dtype))
    # decode: token i at some offset of page i
    bt5 = _tables([5])
    slots5 = (torch.arange(5) * 32 + torch.tensor([3, 31, 0, 17, 8])).int()
    pos5 = torch.tensor([3, 63, 64, 113, 200], dtype=torch.int32, device=dev)
    x5 = (torch.randn(5, N, generator=g) * 1.5).to(dtype).to(dev)

    def per_token(kp, vp, bt, slots):
        a = x5.clone()
        nat.rope_kv_write(a, cos, sin, pos5, slots, kp, vp, H, Hkv, D, rot, **kw)
        return [a]

    _writer(arena, Hkv, D, pool_dtype, bt5, [5], slots5, per_token, f"{name} rope_kv_write")
    xin = (torch.randn(5, 256, generator=g) * 0.5).to(dtype).to(dev)
    w = nat.DenseWeight((torch.randn(N, 256, generator=g) * 0.06).to(dtype).to(dev))
    part = nat.dense_gemm_partial(xin, w, bias=(torch.randn(N, generator=g) * 0.1).to(dtype).to(dev))

    def partial(kp, vp, bt, slots):
        return [nat.rope_kv_write(part, cos, sin, pos5, slots, kp, vp, H, Hkv, D, rot, **kw)]

    _writer(arena, Hkv, D, pool_dtype, bt5, [5], slots5, partial, f"{name} rope_kv_write_partial")
    # prefill of 33 and 70 tokens: the tails of the last pages are zeroed, and count as written
    lens = [33, 70]
    T = sum(lens)
    x = (torch.randn(T, N, generator=g) * 1.5).to(dtype).to(dev)
    cu = torch.tensor([0, 33, 103], dtype=torch.int32, device=dev)
    pos = torch.cat([torch.arange(n) for n in lens]).int().to(dev)

    def prefill(kp, vp, bt, slots):
        a = x.clone()
        nat.rope_kv_write_prefill(a, cos, sin, pos, cu, bt, kp, vp, max(lens), H, Hkv, D, rot, **kw)
        return [a]

    _writer(arena, Hkv, D, pool_dtype, _tables([2, 3]), [2, 3], None, prefill, f"{name} rope_kv_write_prefill")
    pasts = [32, 64]
    pos_at = torch.cat([p + torch.arange(n) for p, n in zip(pasts, lens)]).int().to(dev)

    def prefill_at(kp, vp, bt, slots):
        a = x.clone()
        nat.rope_kv_write_prefill_at(a, cos, sin, pos_at, cu, bt, kp, vp, max(lens), H, Hkv, D, rot, pasts, **kw)
        return [a]

    _writer(arena, Hkv, D, pool_dtype, _tables([3, 5]), [3, 5], None, prefill_at, f"{name} rope_kv_write_prefill_at")


def _gemm_slots(M):
    """M tokens dealt over 8 pages (M 3: three pages), at offsets that differ per page."""
    i = torch.arange(M)
    return ((i % 8) * 32 + (i // 8 * 7 + i % 8 * 5) % 32).int()


GEMM = [(f"{entry}{'-fragments' if frag else ''}-m{M}-hkv8-d{D}-{dn}-{'e4m3' if fp8 else 'kv16'}", entry, frag, M, D, dn, fp8)
        for entry, frag, dn in (("gptq_rope", False, "f16"), ("gptq_rope", True, "f16"), ("dense_rope", False, "f16"),
                                ("dense_rope", False, "bf16"))
        for M in (3, 33) for D in (128, 96) for fp8 in (False, True)]


@pytest.mark.parametrize("name,entry,frag,M,D,dn,fp8", GEMM, ids=[c[0] for c in GEMM])
def test_qkv_rope_gemms(arena, gpu_device, name, entry, frag, M, D, dn, fp8):
    """tgis_gptq_gemm_rope_f16 through both bodies (row-major x: gptq_gemm_body.h, fragment-order x: gptq_wide_body.h) and
    tgis_dense_gemm_rope, and their _kv8 forms, at the smallest K the entry points take (64: one group of 64 rows) and
    N = (8 + 2 * 8) D."""
    nat, dev = _nat(), gpu_device
    H = Hkv = 8
    c = dict(entry=entry, K=64, N=(H + 2 * Hkv) * D, groups=1, act=3, H=H, Hkv=Hkv, D=D, dtype=dn)
    gen = torch.Generator(device=dev)
    gen.manual_seed(zlib.crc32(name.encode()))
    dense = entry == "dense_rope"
    w, _ = gemm_edges._dense_weight(c, gen, dev) if dense else gemm_edges._int4_weight(c, gen, dev)
    dt = gemm_edges.DT[dn]
    x = gemm_edges._activation(M, c["K"], dt, gen, dev)
    bias = (torch.randn(c["N"], generator=gen, device=dev) * 0.1).to(dt)
    cos, sin = (t.to(dev) for t in ops_ref.rope_tables(D, 10000.0, 4096, dt))
    pos = torch.randint(0, 4096, (M,), generator=gen, device=dev, dtype=torch.int32)
    xa = nat.FragAct.from_rows(x.contiguous()) if frag else x
    fn = nat.dense_gemm_rope if dense else nat.gptq_gemm_rope
    kw = {"kv_scales": FP8_SCALES} if fp8 else {}
    npg = min(M, 8)

    def call(kp, vp, bt, slots):
        return [fn(xa, w, bias, cos, sin, pos, slots, kp, vp, H, Hkv, D, **kw)[:, :H * D].contiguous()]

    _writer(arena, Hkv, D, U8 if fp8 else dt, _tables([npg]), [npg], _gemm_slots(M), call, name)


@pytest.mark.parametrize("pool_dtype", [F16, U8], ids=["16bit", "e4m3"])
def test_spec_tree_commit(arena, gpu_device, pool_dtype):
    """The arena as one pool [L, 2, P, Hkv, 32 D]: the last layer's V pool begins past 2^32 elements (one byte) or 2^31
    (16-bit) from layer 0's K pool.  C 3, K 3, best 2, n_emit 3: two positions move, from one page to another."""
    nat, dev = _nat(), gpu_device
    Hkv, D, C, K = 2, 64, 3, 3
    cg = fp.CommitGeometry(Hkv, D, 1 if pool_dtype == U8 else 2)
    L, P, S = cg.L, cg.P, cg.S
    assert cg.arena_bytes() <= arena.nbytes
    far_pages = cg.pages()
    cg.check_aliases(far_pages)
    assert cg.offset(L - 1, 1, 0) >= cg.T and cg.offset(0, 0, max(far_pages)) < cg.T
    # (pos, best, n_emit): destinations 29 30 | 31 32 (they straddle a page edge, 37 -> 31 crosses it) | 61 62, sources 6 further
    reqs = [(28, 2, 3), (30, 2, 3), (60, 2, 3)]
    for p, bc, n in reqs:
        moves = tref.commit_moves(p, C, K, bc, n)
        assert len(moves) == 2 and any(s // 32 != d // 32 for s, d in moves), "a source and its destination on different pages"
    B, width = len(reqs), 3
    g = torch.Generator().manual_seed(5)
    bt = torch.arange(B * width, dtype=torch.int32).reshape(B, width)
    if pool_dtype == U8:
        near = torch.randint(0, 256, (L, 2, B * width, Hkv, 32 * D), generator=g, dtype=U8).to(dev)
    else:
        near = torch.randn((L, 2, B * width, Hkv, 32 * D), generator=g).to(pool_dtype).to(dev)
    m = dict(zip(range(B * width), far_pages))
    arena.fill(pool_dtype)
    arena.geom = cg
    offs = [cg.offset(layer, kv, m[p]) for layer in range(L) for kv in (0, 1) for p in range(B * width)]
    for o, blk in zip(offs, near.reshape(-1, S)):
        arena.block(o).copy_(blk)
    far = arena.typed()[fp.BASE:fp.BASE + L * 2 * P * S].view(L, 2, P, Hkv, 32 * D)
    before = near.cpu().clone()
    assert torch.equal(arena.gather(offs).cpu(), _bits(before).reshape(-1, S))
    args = [torch.tensor([r[i] for r in reqs], dtype=torch.int32, device=dev) for i in range(3)]
    new_pos, best, n_emit = args[0] + args[2], args[1], args[2]
    nat.spec_tree_commit(near, bt.to(dev), new_pos, best, n_emit, C, K)
    nat.spec_tree_commit(far, fp.remap(bt, m).to(dev), new_pos, best, n_emit, C, K)
    torch.cuda.synchronize()
    # spec_tree_ref's moves on the blocks as they were
    want = before.clone()
    for layer in range(L):
        for b, (p, bc, n) in enumerate(reqs):
            for src, dst in tref.commit_moves(p, C, K, bc, n):
                Ks, Vs = ops_ref.kv_page_unpack(before[layer, 0], before[layer, 1], int(bt[b, src // 32]), Hkv, D)
                pg = int(bt[b, dst // 32])
                Kd, Vd = (t.clone() for t in ops_ref.kv_page_unpack(want[layer, 0], want[layer, 1], pg, Hkv, D))
                Kd[dst % 32], Vd[dst % 32] = Ks[src % 32], Vs[src % 32]
                ops_ref.kv_page_pack(want[layer, 0], want[layer, 1], pg, Kd, Vd)
    assert not torch.equal(_bits(want), _bits(before))
    got = arena.gather(offs).cpu()
    assert torch.equal(got, _bits(want).reshape(-1, S)), "the far blocks differ from spec_tree_ref's commit"
    assert torch.equal(got, _bits(near.cpu()).reshape(-1, S)), "the far blocks differ from the near pool's"
    arena.restore(offs)
    assert arena.untouched(), "the arena outside the case's own page blocks was written"


# ---- the split workspace at its 2 GiB guard ----------------------------------------------------------------------------------
class _SharedPages(edges._Case):
    """B one-token sequences of H 8 / Hkv 8 / D 128 whose contexts cycle through CTXS; all sequences of one context share
    its pages, so the pools stay tiny while the workspace grows with B."""
    CTXS = (5, 33, 40, 64)

    def __init__(self, dev, B):
        g = torch.Generator().manual_seed(B)
        self.dev, self.dtype, self.H, self.Hkv, self.D = dev, F16, 8, 8, 128
        H, Hkv, D = self.H, self.Hkv, self.D
        npages = [(c + 31) // 32 for c in self.CTXS]
        total = sum(npages) + 1
        sign = torch.randint(0, 2, (2, total, Hkv, 32 * D), generator=g, dtype=torch.int8) * 2 - 1
        kpool, vpool = (sign.float() * edges.POISON).to(F16)
        rows = torch.full((len(self.CTXS), max(npages)), total - 1, dtype=torch.int32)
        self.Ks, self.Vs, o = [], [], 0
        for i, ctx in enumerate(self.CTXS):
            K = torch.randn(ctx, Hkv, D, generator=g).to(F16)
            V = (torch.randn(ctx, Hkv, D, generator=g) + 1.0).to(F16)
            self.Ks.append(K)
            self.Vs.append(V)
            for j in range(npages[i]):
                rows[i, j] = o
                ops_ref.kv_page_pack(kpool, vpool, o, K[32 * j:32 * j + 32], V[32 * j:32 * j + 32])
                o += 1
        self.kind = torch.arange(B) % len(self.CTXS)
        self.seqs = [(1, self.CTXS[k]) for k in self.kind.tolist()]
        self.T, self.max_q, self.max_ctx = B, 1, max(self.CTXS)
        self.qh = (torch.randn(B, H, D, generator=g) * 2.0).to(F16)
        qa = torch.full((B, (H + 2 * Hkv) * D), float("nan"), dtype=F16)
        qa[:, :H * D] = self.qh.reshape(B, H * D)
        self.qa, self.kpool, self.vpool = qa.to(dev), kpool.to(dev), vpool.to(dev)
        self.bt = rows[self.kind].contiguous().to(dev)
        self.ctx = torch.tensor([c for _, c in self.seqs], dtype=torch.int32, device=dev)
        self.cu = torch.arange(B + 1, dtype=torch.int32, device=dev)

    def want(self):
        """Softmax attention in fp64 for all rows that share a context at once (H == Hkv: head h reads kv head h)."""
        out = torch.empty(self.T, self.H, self.D, dtype=torch.float64)
        for i in range(len(self.CTXS)):
            rows = self.kind == i
            q, K, V = self.qh[rows].double(), self.Ks[i].double(), self.Vs[i].double()
            p = torch.softmax(torch.einsum("nhd,chd->nhc", q, K) * self.D ** -0.5, dim=-1)
            out[rows] = torch.einsum("nhc,chd->nhd", p, V)
        return out.float()


@pytest.mark.parametrize("B,merge", [(16383, "fused"), (16384, "combine8")], ids=["b16383-merged-in-the-launch", "b16384-combine-launch"])
def test_split_workspace_at_the_2gib_guard(arena, gpu_device, B, merge):
    """records * D * 4 = 2 147 352 576 < 2^31 at B 16383: the in-launch merge, whose record offsets are 32-bit byte offsets,
    runs right below its guard; at B 16384 the product is exactly 2^31 and the plan takes the combine launch."""
    nat = _nat()
    H, Hkv, D, ns = 8, 8, 128, 2
    assert B * Hkv * 16 * ns * D * 4 == (2147352576 if B == 16383 else 1 << 31)
    plan = attn_cases.plan_fields(attn_cases.query_plan(nat.load_library(), B, H, Hkv, D, 1, ns))
    assert plan["merge"] == merge, plan
    assert nat.attn_workspace_bytes(B, H, Hkv, D, ns) > 2 * fp.GIB
    c = _SharedPages(gpu_device, B)
    want = c.want()
    for b in (0, 1, 2, 3, B - 1):  # the vectorised oracle is the oracle
        K, V = c.Ks[int(c.kind[b])], c.Vs[int(c.kind[b])]
        one = ops_ref.attention_varlen(c.qh[b:b + 1], K, V, [0, 1], [0, K.shape[0]], D ** -0.5)
        assert (one - want[b:b + 1]).abs().max() < 1e-5
    got = c.run(ns)  # NaN workspace, NaN guards behind it and behind `out`; finite output
    c.check(got, want, f"B {B}: 2 splits against the oracle")
    c.check(got, c.run(1), f"B {B}: 2 splits against one")
    assert torch.equal(got, c.run(ns)), f"B {B}: the second launch differs from the first"
