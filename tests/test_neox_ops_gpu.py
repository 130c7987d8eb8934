"""GPT-NeoX kernels: decode / prefill attention at head size 96, partial rotary spans off the 16-element grid (24 of 96),
the parallel-residual add + two LayerNorms launch, and the argument checks that guard them."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ops_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat(gpu_device):
    from tgis_amd import native

    native.load_library()
    return native


def _close(got, want, tol, what):
    err = (got.float().cpu() - want.float()).abs().max().item()
    assert err <= tol * (1 + want.float().abs().max().item()), f"{what}: max err {err}"


def _pool_with_context(nat, dev, dtype, ctxs, Hkv, D, g):
    """Pages for every sequence (shuffled), filled with random k / v through the no-rotation cache write."""
    pages_per = [(c + 31) // 32 for c in ctxs]
    total = sum(pages_per) + 2
    perm = torch.randperm(total, generator=g).tolist()
    bt = torch.zeros((len(ctxs), max(pages_per)), dtype=torch.int32)
    pi = 0
    for b, n in enumerate(pages_per):
        for j in range(n):
            bt[b, j] = perm[pi]
            pi += 1
    T = sum(ctxs)
    k = (torch.randn(T, Hkv, D, generator=g)).to(dtype)
    v = (torch.randn(T, Hkv, D, generator=g)).to(dtype)
    slots = torch.cat([bt[b, torch.arange(c) // 32].long() * 32 + torch.arange(c) % 32 for b, c in enumerate(ctxs)]).int()
    kpool = torch.zeros((total, Hkv, 32 * D), dtype=dtype, device=dev)
    vpool = torch.zeros_like(kpool)
    qkv = torch.cat([k.view(T, -1), k.view(T, -1), v.view(T, -1)], dim=1).to(dev)  # q part unused (H = Hkv here)
    nat.rope_kv_write(qkv, None, None, None, slots.to(dev), kpool, vpool, Hkv, Hkv, D, D)
    return bt, kpool, vpool, k, v


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 7, 33])
@pytest.mark.parametrize("H,Hkv", [(8, 8), (48, 1)])
def test_decode_attention_head_size_96(nat, gpu_device, dtype, B, H, Hkv):
    """One decode token per sequence over contexts 1, 31, 32, 33 and ~1000, unsplit and split (the split rule's own
    choice and forced splits), against the varlen oracle.  MHA (8 heads) merges its splits inside the attention launch;
    48 q heads on one kv head (three 16-head chunks per block) merge them in attn_combine_kernel: <= 8 splits in its
    one-round-trip form, 11 in its two-pass form."""
    D = 96
    g = torch.Generator().manual_seed(96 + B)
    ctxs = [[1, 31, 32, 33, 1000][i % 5] for i in range(B)]
    bt, kpool, vpool, k, v = _pool_with_context(nat, gpu_device, dtype, ctxs, Hkv, D, g)
    q = torch.randn(B, H, D, generator=g).to(dtype)
    cuk = [0] + np.cumsum(ctxs).tolist()
    want = ops_ref.attention_varlen(q, k, v, torch.arange(B + 1), cuk, D ** -0.5)
    dq = q.view(B, H * D).to(gpu_device)
    ctx = torch.tensor(ctxs, dtype=torch.int32, device=gpu_device)
    cuq = torch.arange(B + 1, dtype=torch.int32, device=gpu_device)
    auto = nat.attn_num_splits(B, Hkv, H, 1, max(ctxs))
    tol = 4e-3 if dtype == torch.float16 else 2e-2
    for ns in sorted({1, auto, 4, 11}):
        out = torch.full((B, H * D), float("nan"), dtype=dtype, device=gpu_device)
        ws = nat.Workspace(nat.attn_workspace_bytes(B, H, Hkv, D, ns), gpu_device) if ns > 1 else None
        nat.attn_paged(dq, dq.stride(0), kpool, vpool, bt.to(gpu_device), ctx, cuq, out, B, H, Hkv, D, 1, max(ctxs),
                       D ** -0.5, ns, ws)
        assert not torch.isnan(out).any(), f"splits={ns}: unwritten output columns"
        _close(out.view(B, H, D), want, tol, f"decode D=96 splits={ns}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_prefill_attention_head_size_96(nat, gpu_device, dtype):
    """Prefill-sized q (> 64 columns: the LDS-staged kernel) with 24 rotary dims, against rotary + varlen oracle."""
    H = Hkv = 4
    D, rot = 96, 24
    lens = [45, 1, 32, 97, 70]
    g = torch.Generator().manual_seed(7)
    B, T = len(lens), sum(lens)
    pages_per = [(n + 31) // 32 for n in lens]
    total = sum(pages_per) + 2
    perm = torch.randperm(total, generator=g).tolist()
    bt = torch.zeros((B, max(pages_per)), dtype=torch.int32)
    pi = 0
    for b, n in enumerate(pages_per):
        for j in range(n):
            bt[b, j] = perm[pi]
            pi += 1
    qkv = (torch.randn(T, 3 * H * D, generator=g) * 0.7).to(dtype)
    cos, sin = ops_ref.rope_tables(rot, 10000.0, 128, dtype)
    pos = torch.cat([torch.arange(n) for n in lens]).int()
    cu = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    qr = ops_ref.apply_rope(qkv[:, :H * D].view(T, H, D), cos[pos.long()], sin[pos.long()]).to(dtype)
    kr = ops_ref.apply_rope(qkv[:, H * D:2 * H * D].view(T, H, D), cos[pos.long()], sin[pos.long()]).to(dtype)
    want = ops_ref.attention_varlen(qr, kr, qkv[:, 2 * H * D:].view(T, H, D), cu, cu, D ** -0.5)
    kpool = torch.zeros((total, Hkv, 32 * D), dtype=dtype, device=gpu_device)
    vpool = torch.zeros_like(kpool)
    dq = qkv.to(gpu_device)
    nat.rope_kv_write_prefill(dq, cos.to(gpu_device), sin.to(gpu_device), pos.to(gpu_device), cu.to(gpu_device),
                              bt.to(gpu_device), kpool, vpool, max(lens), H, Hkv, D, rot)
    out = torch.empty((T, H * D), dtype=dtype, device=gpu_device)
    nat.attn_paged(dq, dq.stride(0), kpool, vpool, bt.to(gpu_device), torch.tensor(lens, dtype=torch.int32,
                   device=gpu_device), cu.to(gpu_device), out, B, H, Hkv, D, max(lens), max(lens), D ** -0.5, 1, None)
    _close(out.view(T, H, D), want, 4e-3 if dtype == torch.float16 else 2e-2, "prefill D=96")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("D,rot", [(64, 16), (96, 24), (96, 32), (128, 32), (96, 96), (64, 10)])
def test_rope_kernels_partial_span(nat, gpu_device, dtype, D, rot):
    """tgis_rope_kv_write, _partial and _prefill over the first `rot` dims of every q / k head: q in place against
    ops_ref.apply_rope (cos of width rot / 2), the cache holding the rotated k and the untouched v bit for bit, and the
    three kernels agreeing bit for bit."""
    H, Hkv = 4, 2
    W = (H + 2 * Hkv) * D
    lens = [3, 40]
    T = sum(lens)
    g = torch.Generator().manual_seed(D + rot)
    x = (torch.randn(T, W // 2, generator=g) * 0.5).to(dtype)
    w = (torch.randn(W, W // 2, generator=g) * (W // 2) ** -0.5).to(dtype)
    bias = (torch.randn(W, generator=g) * 0.1).to(dtype)
    cos, sin = ops_ref.rope_tables(rot, 10000.0, 64, dtype)
    pos = torch.cat([torch.arange(n) for n in lens]).int()
    cu = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    bt = torch.tensor([[0, 0], [1, 2]], dtype=torch.int32)
    slots = torch.cat([bt[b, torch.arange(n) // 32].long() * 32 + torch.arange(n) % 32 for b, n in enumerate(lens)]).int()
    dev = gpu_device
    dcos, dsin, dpos, dslots = cos.to(dev), sin.to(dev), pos.to(dev), slots.to(dev)
    dw = nat.DenseWeight(w.to(dev))
    qkv = nat.dense_gemm(x.to(dev), dw, nat.Workspace(0, dev), bias=bias.to(dev))
    raw = qkv.cpu()
    pools = []
    # per-token kernel (in place), split-K partial input, prefill page-wise writer
    a = qkv.clone()
    kp, vp = torch.zeros((3, Hkv, 32 * D), dtype=dtype, device=dev), torch.zeros((3, Hkv, 32 * D), dtype=dtype, device=dev)
    nat.rope_kv_write(a, dcos, dsin, dpos, dslots, kp, vp, H, Hkv, D, rot)
    pools.append((kp, vp))
    part = nat.dense_gemm_partial(x.to(dev), dw, bias=bias.to(dev))
    kp2, vp2 = torch.zeros_like(kp), torch.zeros_like(vp)
    b_ = nat.rope_kv_write(part, dcos, dsin, dpos, dslots, kp2, vp2, H, Hkv, D, rot)
    pools.append((kp2, vp2))
    c = qkv.clone()
    kp3, vp3 = torch.zeros_like(kp), torch.zeros_like(vp)
    nat.rope_kv_write_prefill(c, dcos, dsin, dpos, cu.to(dev), bt.to(dev), kp3, vp3, max(lens), H, Hkv, D, rot)
    pools.append((kp3, vp3))
    # both forms against the oracle's rotation of the GEMM output; the partial form sums the slabs itself (another
    # summation order than the GEMM's own reduce: one more rounding of slack)
    ulp = 1e-3 if dtype == torch.float16 else 8e-3
    qr = ops_ref.apply_rope(raw[:, :H * D].view(T, H, D), cos[pos.long()], sin[pos.long()])
    kr = ops_ref.apply_rope(raw[:, H * D:(H + Hkv) * D].view(T, Hkv, D), cos[pos.long()], sin[pos.long()])
    for name, got, tol in (("rope_kv_write", a, ulp), ("rope_kv_write_partial", b_, 3 * ulp)):
        _close(got[:, :H * D].view(T, H, D), qr, tol, f"{name} q")
        _close(got[:, H * D:(H + Hkv) * D].view(T, Hkv, D), kr, tol, f"{name} k")
        _close(got[:, (H + Hkv) * D:], raw[:, (H + Hkv) * D:], tol, f"{name} v")
    assert torch.equal(a[:, (H + Hkv) * D:].cpu(), raw[:, (H + Hkv) * D:]), "rope_kv_write: v changed"
    assert torch.equal(c[:, :H * D], a[:, :H * D]), "prefill q != per-token q"
    kdev = a[:, H * D:(H + Hkv) * D].view(T, Hkv, D).cpu()
    vdev = raw[:, (H + Hkv) * D:].view(T, Hkv, D)
    for (kpool, vpool), what in zip(pools[::2], ("per-token", "prefill")):
        for b, n in enumerate(lens):
            for j in range((n + 31) // 32):
                K, V = ops_ref.kv_page_unpack(kpool.cpu(), vpool.cpu(), int(bt[b, j]), Hkv, D)
                m = min(32, n - j * 32)
                t0 = int(cu[b]) + j * 32
                assert torch.equal(K[:m], kdev[t0:t0 + m]), f"{what}: K page content"
                assert torch.equal(V[:m], vdev[t0:t0 + m]), f"{what}: V page content"
    kb = b_[:, H * D:(H + Hkv) * D].view(T, Hkv, D).cpu()
    for b, n in enumerate(lens):
        K, _ = ops_ref.kv_page_unpack(kp2.cpu(), vp2.cpu(), int(bt[b, 0]), Hkv, D)
        m = min(32, n)
        assert torch.equal(K[:m], kb[int(cu[b]):int(cu[b]) + m]), "partial: K page content"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("rows,hidden,form", [(5, 384, "tensor"), (33, 6144, "slabs"), (3, 256, "mixed"),
                                              (7, 384, "single")])
def test_layernorm2_residual(nat, gpu_device, dtype, rows, hidden, form):
    """h' = h + A + B (+ biases) once in fp32, y1 / y2 = two LayerNorms of it, against ops_ref.layernorm_residual on the
    oracle's h'.  Addends as tensors, as split-K slabs of two GEMMs with different K, or one of each; `single` is the
    final_layer_norm form (no y2)."""
    dev = gpu_device
    g = torch.Generator().manual_seed(rows * hidden)
    h = torch.randn(rows, hidden, generator=g).to(dtype)
    w1, w2 = [(1 + 0.1 * torch.randn(hidden, generator=g)).to(dtype) for _ in range(2)]
    b1, b2 = [(0.1 * torch.randn(hidden, generator=g)).to(dtype) for _ in range(2)]
    ba, bb = [(0.1 * torch.randn(hidden, generator=g)).to(dtype) for _ in range(2)]
    addends, want_sum = [], h.float()
    for K, bias in ((hidden, ba), (4 * hidden, bb)):
        if form == "slabs" or (form == "mixed" and K == hidden):
            x = torch.randn(rows, K, generator=g).to(dtype)
            w = (torch.randn(hidden, K, generator=g) * K ** -0.5).to(dtype)
            p = nat.dense_gemm_partial(x.to(dev), nat.DenseWeight(w.to(dev)), bias=bias.to(dev))
            ref = nat.dense_gemm(x.to(dev), nat.DenseWeight(w.to(dev)),
                                 nat.Workspace(0, dev)).float().cpu()
            addends.append(p)
            want_sum = want_sum + ref + bias.float()
        else:
            t = torch.randn(rows, hidden, generator=g).to(dtype)
            addends.append((t.to(dev), bias.to(dev)))
            want_sum = want_sum + t.float() + bias.float()
    a, b = addends
    kw = {}
    if isinstance(a, tuple):
        a, kw["a_bias"] = a
    if isinstance(b, tuple):
        b, kw["b_bias"] = b
    single = form == "single"
    y1, y2, res = nat.layernorm2_residual(h.to(dev), a, b, w1.to(dev), b1.to(dev), 1e-5,
                                          None if single else w2.to(dev), None if single else b2.to(dev), **kw)
    want1, _ = ops_ref.layernorm_residual(want_sum, None, w1, b1, 1e-5)
    tol = 2e-2 if dtype == torch.float16 else 6e-2
    _close(res, want_sum, 4e-3 if dtype == torch.float16 else 1e-2, "h'")
    _close(y1, want1, tol, "y1")
    if single:
        assert y2 is None
    else:
        want2, _ = ops_ref.layernorm_residual(want_sum, None, w2, b2, 1e-5)
        _close(y2, want2, tol, "y2")
        # both LayerNorms come from one set of statistics: with equal weights they are equal bit for bit
        y1b, y2b, _ = nat.layernorm2_residual(h.to(dev), None, None, w1.to(dev), b1.to(dev), 1e-5, w1.to(dev), b1.to(dev))
        assert torch.equal(y1b, y2b)


def test_bad_head_size_and_rot_dim_are_refused(nat, gpu_device):
    lib = nat.load_library()
    dev = gpu_device
    D = 96
    qkv = torch.zeros((2, 3 * D), dtype=torch.float16, device=dev)
    cos = torch.zeros((8, 48), dtype=torch.float16, device=dev)
    pos = torch.zeros(2, dtype=torch.int32, device=dev)
    slots = torch.zeros(2, dtype=torch.int32, device=dev)
    pool = torch.zeros((1, 1, 32 * D), dtype=torch.float16, device=dev)
    s = nat._stream()
    for rot in (23, 0, 98):  # odd, empty, wider than the head
        rc = lib.tgis_rope_kv_write(qkv.data_ptr(), 3 * D, cos.data_ptr(), cos.data_ptr(), pos.data_ptr(),
                                    slots.data_ptr(), pool.data_ptr(), pool.data_ptr(), 2, 1, 1, D, rot, 0, s)
        assert rc == -1, f"rot_dim {rot}: rc {rc}"
        lib.tgis_clear_error()
    bt = torch.zeros((1, 1), dtype=torch.int32, device=dev)
    ctx = torch.ones(1, dtype=torch.int32, device=dev)
    cu = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    out = torch.zeros((1, 160), dtype=torch.float16, device=dev)
    for Dbad in (80, 256, 32):
        rc = lib.tgis_attn_paged(qkv.data_ptr(), 3 * D, pool.data_ptr(), pool.data_ptr(), bt.data_ptr(), 1,
                                 ctx.data_ptr(), cu.data_ptr(), out.data_ptr(), 0, 1, 1, 1, Dbad, 1, 1,
                                 ctypes.c_float(0.1), 0, 1, None, 0, s)
        assert rc == -1 and b"head_dim" in lib.tgis_last_error(), f"D={Dbad}: rc {rc}"
        lib.tgis_clear_error()
    torch.cuda.synchronize()
