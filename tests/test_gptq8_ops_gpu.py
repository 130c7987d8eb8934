"""GPU: the 8-bit GPTQ kernels (csrc/gptq8.hip) on their own, over the case table of tests/gptq8_cases.py.

Dequantisation is checked bit for bit against ((q - z - 1).float() * s.float()).half(): the fp32 product of a 9-bit and an
11-bit number is exact.  In the plain / trivial / act_order / perm weight forms the scales are drawn >= 2^-10, so that no
product is subnormal (asserted); the "subnormal" form draws column scales 2^-10 .. 2^-24 and one column s = 0, so that the
products are normal values, subnormals, the smallest subnormal and signed zeros, and its expectation is built on the host
in fp64 (the product has <= 20 significant bits: the one rounding to f16 is exact).  The decode GEMM is checked
against fp64 with the bound, the constants and the protections of tests/test_gemm_edges_gpu.py (imported from it):
  |got - ref| <= 2 u16 |ref| + 2 K 2^-24 (|x| @ |W|) + 2^-24   (+ its act 1 slack: one rounding flip of the staged operand)
x is a strided view in a NaN buffer, out a view in a NaN buffer whose margins must stay NaN, the library is told a
workspace of exactly workspace_bytes(M) bytes inside a larger buffer whose tail must stay untouched, the slabs are NaN-filled
and the counters are zero afterwards, and a second call on the same workspace gives identical bits.  Every case asserts
the plan (tgis_debug_gptq8_plan) it names: {TN, WK, KR, S, MR, reduce, PERM, ACT}.  The subnormal GEMM cases first prove
that the bound tells a flushed weight from the true one: see test_gemm_keeps_subnormal_weights."""
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gptq8_cases as g8  # noqa: E402
import test_gemm_edges_gpu as ge  # noqa: E402  (the bound: _reference / _check / A_OUT / B_ACC / U / TINY, and the guards)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from tgis_amd import native

    return native.load_library()


def _wrap32(v):
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def _pack_rows8(q):
    K, N = q.shape
    sh = (torch.arange(4, device=q.device, dtype=torch.int64) * 8).view(1, 4, 1)
    return _wrap32((q.view(K // 4, 4, N).to(torch.int64) << sh).sum(1))


def _pack_cols8(z):
    G, N = z.shape
    sh = (torch.arange(4, device=z.device, dtype=torch.int64) * 8).view(1, 1, 4)
    return _wrap32((z.view(G, N // 4, 4).to(torch.int64) << sh).sum(2))


def _subnormal_codes(K, N, G):
    """Host tensors (q [K, N], z [G, N], s [G, N] f16, W16 [K, N] f16) of the "subnormal" weight form: the scale of column n
    is an f16 in [2^-e, 2^(1-e)), e = 10 + n % 15, with a random mantissa per group (subnormal scales from e = 15 on;
    e = 24 rounds to 2^-24 or 2^-23), and column 15 has s = 0.  W16 is the one rounding of the exact product."""
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("subnormal", K, N, G)).encode()))
    q = torch.randint(0, 256, (K, N), generator=gen, dtype=torch.int32)
    z = torch.randint(0, 256, (G, N), generator=gen, dtype=torch.int32)
    q[0], q[1], q[K - 1, ::2] = 0, 255, 255
    z[:, 0], z[:, 1], z[G - 1, 2], z[0, 3] = 0, 255, 255, 0
    s = ((torch.rand((G, N), generator=gen, dtype=torch.float64) + 1.0)
         * torch.pow(2.0, -(10.0 + (torch.arange(N) % 15).double())).view(1, N)).half()
    s[:, 15] = 0
    gl = torch.arange(K) // (K // G)
    W16 = ((q - z[gl] - 1).double() * s.double()[gl]).half()
    return q, z, s, W16


_WEIGHTS = {}


def _weight(K, N, G, mode="plain", pads=0):
    """(Gptq8Weight, W16 [K, N] f16: the exact expected dequantisation in IMAGE row order, Wx [x columns, N] fp64: the same
    values scattered to the activation's column order), built once per key.  mode: plain (g_idx None), trivial (the trivial
    g_idx tensor), act_order (a shuffled g_idx), perm (rows in image order + an explicit gather with `pads` entries -1)."""
    key = (K, N, G, mode, pads)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    from tgis_amd import native

    gs = K // G
    if mode == "subnormal":
        q, z, sc, W16 = (t.to(DEV) for t in _subnormal_codes(K, N, G))
        w = native.Gptq8Weight(_pack_rows8(q), _pack_cols8(z), sc, None, 8, gs)
        assert w.perm is None
        _WEIGHTS[key] = (w, W16, W16.double())
        return _WEIGHTS[key]
    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32(repr(key).encode()))
    q = torch.randint(0, 256, (K, N), generator=gen, device=DEV, dtype=torch.int32)
    z = torch.randint(0, 256, (G, N), generator=gen, device=DEV, dtype=torch.int32)  # stored zeros (zero point z + 1)
    q[0], q[1], q[K - 1, ::2] = 0, 255, 255                                        # the extremes of q ...
    z[:, 0], z[:, 1], z[G - 1, 2], z[0, 3] = 0, 255, 255, 0                        # ... and of z, against each other
    s = ((torch.rand((1, N), generator=gen, device=DEV) + 1.0) * 2.0 ** -10
         * torch.pow(2.0, (torch.arange(G, device=DEV) % 4).float()).view(G, 1)).half()  # >= 2^-10, groups 2^k apart
    g_idx = torch.arange(K, device=DEV, dtype=torch.int32) // gs
    if mode == "act_order":
        g_idx = torch.empty(K, dtype=torch.int32, device=DEV)
        g_idx[torch.randperm(K, generator=gen, device=DEV)] = torch.arange(K, device=DEV, dtype=torch.int32) // gs
    gl = g_idx.long()
    W16 = ((q - z[gl] - 1).float() * s.float()[gl]).half()  # source row order
    form = {"plain": None, "trivial": g_idx.cpu(), "act_order": g_idx.cpu()}.get(mode)
    if mode == "perm":
        cols = K - pads
        slots = torch.randperm(K, generator=gen, device=DEV)
        perm = torch.full((K,), -1, dtype=torch.int32, device=DEV)
        perm[slots[:cols]] = torch.randperm(cols, generator=gen, device=DEV).to(torch.int32)
        form = ("perm", perm.cpu(), cols)
    w = native.Gptq8Weight(_pack_rows8(q), _pack_cols8(z), s, form, 8, gs)
    if mode == "perm":
        keep = w.perm >= 0
        Wx = torch.zeros((cols, N), dtype=torch.float64, device=DEV)
        Wx[w.perm[keep].long()] = W16[keep].double()
    elif mode == "act_order":
        assert w.perm is not None
        Wx = W16.double()
        W16 = W16[w.perm.long()]  # image row k' holds source row perm[k']
    else:
        assert w.perm is None
        Wx = W16.double()
    _WEIGHTS[key] = (w, W16, Wx)
    return _WEIGHTS[key]


# ---- dequantisation ------------------------------------------------------------------------------------------------------
DEQUANT = [(K, N, G, mode, pads) for mode, pads in [("plain", 0), ("trivial", 0), ("act_order", 0), ("perm", 24)]
           for K, N, G in [(128, 64, 1), (128, 64, 2), (128, 64, 4), (96, 32, 2)]] + [
    (1312, 8224, 82, "act_order", 0),  # gs 16, a k64 tail, 257 column tiles
    (1568, 64, 98, "plain", 0),        # gs 16, a k64 tail, 98 groups
    (96, 8224, 2, "plain", 0),         # gs 48 over a single padded k64-step pair
    (4096, 96, 32, "perm", 24),        # 64 k64-steps of a padded row shard
]


@pytest.mark.parametrize("K,N,G,mode,pads", DEQUANT)
def test_dequant_is_bit_equal(K, N, G, mode, pads):
    from tgis_amd import native

    if mode == "act_order" and G == 1:
        mode = "trivial"  # one group: every g_idx is trivial
    w, W16, _ = _weight(K, N, G, mode, pads)
    buf = torch.full((K + 2, N), float("nan"), dtype=torch.float16, device=DEV)
    got = native.gptq8_dequant(w, out=buf[:K])
    torch.cuda.synchronize()
    assert torch.isnan(buf[K:]).all(), "rows past K written"
    assert torch.equal(got.view(torch.int16), W16.view(torch.int16))
    mag = W16.float().abs()
    assert mag[mag > 0].min() >= 2.0 ** -14, "a subnormal product: the denormal mode would matter"


# ---- GEMM ----------------------------------------------------------------------------------------------------------------
WS_GUARD = 1 << 16  # bytes behind the workspace the library is told of


def _run_gemm(c, w, Wx, xv):
    """One case on a prepared weight: the plan it names, the guards around x, out and the workspace, the bound against
    fp64 on Wx, and a second call on the same workspace.  Returns (ref, tol, got)."""
    from tgis_amd import native

    lib = _lib()
    M, K, N, act = c["M"], c["K"], c["N"], c.get("act", 0)
    TN, WK, KR, S = c["plan"]
    perm_form = g8.perm_form(c)
    assert g8.case_plan(c, lib) == (TN, WK, KR, S, 2 if M > 32 else 1, int(S > 1), int(perm_form), act) == g8.named_plan(c), c["id"]
    assert (w.perm is not None) == perm_form
    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32((c["id"] + "/bias").encode()))
    cols = w.in_features
    Kx = 2 * cols if act == 1 else cols
    assert xv.shape == (M, Kx)
    xbuf, x = ge._nan_view(M, Kx, 3, 64, torch.float16, DEV)
    x.copy_(xv)
    bias = (torch.randn(N, generator=gen, device=DEV) * 0.1).half() if c.get("bias") else None
    nbytes = w.workspace_bytes(M)
    assert nbytes >= 4096 and (S > 1) == (nbytes > 4096)
    # the library is told `nbytes` bytes; the tail behind them must stay untouched
    wsbuf = torch.full((nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    wsbuf[:4096] = 0  # the arrival counters: zeroed once, left at zero by every call

    def call():
        wsbuf[4096:nbytes] = 0xFF  # NaN in every fp32 slab word
        obuf, out = ge._nan_view(M, N, 3, 32, torch.float16, DEV)
        rc = lib.tgis_gptq8_gemm_f16(x.data_ptr(), x.stride(0), w.image.data_ptr(), bias.data_ptr() if bias is not None else None,
                                     w.perm.data_ptr() if w.perm is not None else None, out.data_ptr(), out.stride(0), M, w.K, w.N,
                                     w.groups, act, wsbuf.data_ptr(), nbytes, native._stream())
        assert rc == 0, lib.tgis_last_error().decode()
        torch.cuda.synchronize()
        return obuf, out

    obuf, got = call()
    assert (wsbuf[nbytes:] == 0xFF).all(), f"{c['id']}: the workspace was written past tgis_gptq8_gemm_workspace_bytes"
    assert not wsbuf[:4096].any(), f"{c['id']}: counters not left at zero"
    assert torch.isnan(xbuf[M:]).all() and torch.isnan(xbuf[:, Kx:]).all(), f"{c['id']}: x padding written"
    assert torch.isnan(obuf[M:]).all() and torch.isnan(obuf[:, N:]).all(), f"{c['id']}: out margins written"
    assert act != 1 or cols == K
    ref, tol = ge._reference(dict(K=K, N=N, act=act), xv, Wx, bias, torch.float16)  # K: the rows the kernel accumulates over
    assert ref.shape == got.shape == (M, N)
    print(f"{c['id']}: worst err / tol {float(((got.double() - ref).abs() / tol).max()):.3f}")
    ge._check(got, ref, tol, c["id"])
    _, again = call()
    assert (wsbuf[nbytes:] == 0xFF).all() and not wsbuf[:4096].any()
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), f"{c['id']}: second call on the same workspace differs"
    return ref, tol, got


@pytest.mark.parametrize("c", g8.CASES, ids=lambda c: c["id"])
def test_gemm(c):
    w, _, Wx = _weight(c["K"], c["N"], c["groups"], c.get("mode", "plain"), c.get("pads", 0))
    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32(c["id"].encode()))
    Kx = (2 if c.get("act", 0) == 1 else 1) * w.in_features
    _run_gemm(c, w, Wx, ge._activation(c["M"], Kx, torch.float16, gen, DEV))


# ---- subnormal products --------------------------------------------------------------------------------------------------
F16_MIN_NORMAL = 2.0 ** -14


def _subnormal_case_inputs(c):
    """Host tensors (W16 [K, N] f16, x [M, K] f16) of a case of gptq8_cases.SUBNORMAL."""
    _, _, _, W16 = _subnormal_codes(c["K"], c["N"], c["groups"])
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    return W16, ge._activation(c["M"], c["K"], torch.float16, gen, "cpu")


def _flush_is_seen(c, W16, xv):
    """(all-subnormal columns, those of them in which the reference on a weight with every subnormal entry flushed to
    zero lies outside the bound around the true reference in at least one row); any device."""
    Wd = W16.double()
    mag = Wd.abs()
    sub = (mag > 0) & (mag < F16_MIN_NORMAL)
    cols = (sub.any(0) & ~(mag >= F16_MIN_NORMAL).any(0)).nonzero().flatten()
    ref, tol = ge._reference(dict(K=c["K"], N=c["N"], act=0), xv, Wd, None, torch.float16)
    flushed, _ = ge._reference(dict(K=c["K"], N=c["N"], act=0), xv, torch.where(sub, torch.zeros_like(Wd), Wd), None, torch.float16)
    outside = ((flushed - ref).abs() > tol).any(0)
    return cols, cols[outside[cols]]


@pytest.mark.parametrize("K,N,G", [(512, 64, 4), (512, 8192, 4)])
def test_dequant_of_subnormal_products_is_bit_equal(K, N, G):
    from tgis_amd import native

    w, W16, _ = _weight(K, N, G, "subnormal")
    mag = W16.double().abs()
    bits = W16.view(torch.int16)
    assert (mag >= F16_MIN_NORMAL).any() and ((mag > 0) & (mag < F16_MIN_NORMAL)).any() and (mag == 2.0 ** -24).any()
    assert (bits == 0).any() and (bits == -0x8000).any(), "both zeros: s = 0 under a positive and a negative q - z - 1"
    buf = torch.full((K + 2, N), float("nan"), dtype=torch.float16, device=DEV)
    got = native.gptq8_dequant(w, out=buf[:K])
    torch.cuda.synchronize()
    assert torch.isnan(buf[K:]).all(), "rows past K written"
    diff = got.view(torch.int16) != bits
    assert not diff.any(), (f"{int(diff.sum())} of {diff.numel()} differ; first at {diff.nonzero()[0].tolist()}: got "
                            f"{got[diff][0].item():.6g} want {W16[diff][0].item():.6g}")


@pytest.mark.parametrize("c", g8.SUBNORMAL, ids=lambda c: c["id"])
def test_gemm_keeps_subnormal_weights(c):
    """W is the f16 image with its subnormal entries: a v_pk_mul_f16 or an MFMA that flushed them would give x @ (W with
    those entries zero).  Before the kernel runs, that flushed reference must lie outside the bound in every
    all-subnormal column, or the case could not tell."""
    W16h, xh = _subnormal_case_inputs(c)
    w, W16, Wx = _weight(c["K"], c["N"], c["groups"], "subnormal")
    assert torch.equal(W16.cpu().view(torch.int16), W16h.view(torch.int16))
    xv = xh.to(DEV)
    cols, seen = _flush_is_seen(c, W16, xv)
    assert cols.numel() >= c["N"] // 15 - 1, "too few all-subnormal columns"
    assert torch.equal(cols, seen), f"{c['id']}: a flushed weight stays inside the bound in columns {sorted(set(cols.tolist()) - set(seen.tolist()))}"
    _run_gemm(c, w, Wx, xv)


@pytest.mark.parametrize("what", ["rows", "group_size", "workspace_short", "ldx", "ldo", "act"])
def test_bad_arguments_are_refused_and_write_nothing(what):
    from tgis_amd import native

    lib = _lib()
    K, N = (1280, 64) if what == "workspace_short" else (256, 64)  # 1280 x 64 splits k in two
    groups = {"workspace_short": 10, "group_size": 32}.get(what, 2)  # group_size: groups of 8 rows
    w, _, _ = _weight(K, N, 10 if what == "workspace_short" else 2)
    M = 65 if what == "rows" else 8
    ldx = K + 4 if what == "ldx" else K
    ldo = N - 8 if what == "ldo" else N
    act = 2 if what == "act" else 0
    x = torch.ones((M, 2 * K + 8), dtype=torch.float16, device=DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
    ws = native.Workspace(1 << 20, DEV)
    ws.buf[4096:] = 0xFF
    need = lib.tgis_gptq8_gemm_workspace_bytes(8, K, N)
    assert what != "workspace_short" or 4096 < need <= ws.nbytes
    told = need - 1 if what == "workspace_short" else ws.nbytes
    rc = lib.tgis_gptq8_gemm_f16(x.data_ptr(), ldx, w.image.data_ptr(), None, None, out.data_ptr(), ldo, M, K, N, groups, act, ws.ptr,
                                 told, native._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"tgis_gptq8_gemm_f16" in lib.tgis_last_error()
    why = {"rows": b"1 <= M <= 64", "group_size": b"multiple of 16", "workspace_short": b"workspace too small",
           "ldx": b"16-byte aligned rows", "ldo": b"at least N elements", "act": b"act must be 0 or 1"}[what]
    assert why in lib.tgis_last_error(), lib.tgis_last_error()
    assert torch.isnan(out).all() and (ws.buf[4096:] == 0xFF).all() and not ws.buf[:4096].any()
    if what == "group_size":
        with pytest.raises(native.TgisHipError, match="multiple of 16"):
            native.Gptq8Weight(torch.zeros((K // 4, N), dtype=torch.int32, device=DEV),
                               torch.zeros((32, N // 4), dtype=torch.int32, device=DEV),
                               torch.ones((32, N), dtype=torch.float16, device=DEV), None, 8, 8)
    lib.tgis_clear_error()
