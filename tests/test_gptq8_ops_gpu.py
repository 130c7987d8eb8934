"""GPU: the 8-bit GPTQ kernels (csrc/gptq8.hip) on their own.

Dequantisation is checked bit for bit against ((q - z - 1).float() * s.float()).half(): the fp32 product of a 9-bit and an
11-bit number is exact, and the scales are drawn >= 2^-10 so that no product is subnormal.  The decode GEMM is checked
against fp64 with the bound, the constants and the protections of tests/test_gemm_edges_gpu.py (imported from it):
  |got - ref| <= 2 u16 |ref| + 2 K 2^-24 (|x| @ |W|) + 2^-24   (+ its act 1 slack: one rounding flip of the staged operand)
x is a strided view in a NaN buffer, out a view in a NaN buffer whose margins must stay NaN, the workspace past the counters
is NaN-filled and the counters are zero afterwards, and a second call on the same workspace gives identical bits.  Every
case asserts the plan (tgis_debug_gptq8_plan) it names: {TN, WK, KR, S, MR}."""
import ctypes
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
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


_WEIGHTS = {}


def _weight(K, N, G, mode="plain", pads=0):
    """(Gptq8Weight, W16 [K, N] f16: the exact expected dequantisation in IMAGE row order, Wx [x columns, N] fp64: the same
    values scattered to the activation's column order), built once per key.  mode: plain (g_idx None), trivial (the trivial
    g_idx tensor), act_order (a shuffled g_idx), perm (rows in image order + an explicit gather with `pads` entries -1)."""
    key = (K, N, G, mode, pads)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    from tgis_amd import native

    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32(repr(key).encode()))
    gs = K // G
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
@pytest.mark.parametrize("mode,pads", [("plain", 0), ("trivial", 0), ("act_order", 0), ("perm", 24)])
@pytest.mark.parametrize("K,N,G", [(128, 64, 1), (128, 64, 2), (128, 64, 4), (96, 32, 2)])
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
def _C(M, K, N, plan, G=None, gs=128, **kw):
    G = G if G is not None else K // gs
    tag = "".join(f"-{k}{'' if v is True else v}" for k, v in kw.items())
    return dict(id=f"m{M}-k{K}-n{N}-g{G}{tag}", M=M, K=K, N=N, groups=G, plan=plan, entry="gptq8", **kw)


P_TINY_A = (2, 4, 256, 1)     # (TN, WK, KR, S) of 256 x 512
P_TINY_B = (2, 4, 512, 1)     # 512 x 256
P_O = (2, 4, 768, 6)          # 4096 x 4096: 64-column blocks, six splits, the last one chunk short of the others' three
P_QKV = (4, 2, 1024, 4)       # 4096 x 12288: 128-column blocks
P_DOWN = (2, 4, 2048, 6)      # 11008 x 4096: the last split holds 3 of 8 chunks
GRID = (
    # every instance (TN, WK, MR) and split form on M x {tiny model shapes, cfg3 layer shapes}
    [_C(M, 256, 512, P_TINY_A, gs=64) for M in (1, 16, 17, 32, 33, 64)]
    + [_C(M, 512, 256, P_TINY_B, gs=64) for M in (32, 33)]
    + [_C(M, 4096, 4096, P_O) for M in (1, 16, 17, 32, 33, 64)]
    + [_C(M, 4096, 12288, P_QKV) for M in (1, 32, 33, 64)]
    + [_C(M, 11008, 4096, P_DOWN) for M in (32, 33)]
)
EDGES = [
    _C(17, 96, 64, (2, 4, 256, 1), G=1),                                  # a k64 tail, a single group
    _C(33, 96, 64, (2, 4, 256, 1), G=2),                                  # groups of 48 rows: not a power of two
    _C(5, 128, 32, (2, 4, 256, 1), G=4, bias=True),                       # N = 32: one tile, group size 32
    _C(40, 256, 96, (2, 4, 256, 1), G=2),                                 # N = 96: the last block holds one tile
    _C(32, 1280, 64, (2, 4, 768, 2), G=10, bias=True),                    # a global split whose last part is short, + bias
    _C(64, 1280, 64, (2, 4, 768, 2), G=10, act=1),                        # SiLU * up while staging, split
    _C(17, 512, 64, (2, 4, 512, 1), G=8, act=1, bias=True),
    _C(33, 512, 96, (2, 4, 512, 1), G=8, mode="act_order"),
    _C(16, 1280, 64, (2, 4, 768, 2), G=20, mode="act_order", act=1),
    _C(9, 256, 64, (2, 4, 256, 1), G=8, mode="perm", pads=56),            # a padded row shard: -1 reads a zero
    _C(64, 1280, 32, (2, 4, 768, 2), G=40, mode="perm", pads=88, bias=True),
    _C(3, 4096, 8192, (4, 2, 768, 6), G=1),                               # 256 tiles: the first 128-column plan
]


def _plan(c, lib):
    info = (ctypes.c_int * 8)()
    rc = lib.tgis_debug_gptq8_plan(c["M"], c["K"], c["N"], c["groups"], c.get("act", 0), int(c.get("mode") in ("act_order", "perm")),
                                   info)
    assert rc == 0, lib.tgis_last_error().decode()
    return tuple(info)


@pytest.mark.parametrize("c", GRID + EDGES, ids=lambda c: c["id"])
def test_gemm(c):
    from tgis_amd import native

    lib = _lib()
    M, K, N, act = c["M"], c["K"], c["N"], c.get("act", 0)
    TN, WK, KR, S = c["plan"]
    perm_form = c.get("mode") in ("act_order", "perm")
    assert _plan(c, lib) == (TN, WK, KR, S, 2 if M > 32 else 1, int(S > 1), int(perm_form), act), c["id"]
    w, _, Wx = _weight(K, N, c["groups"], c.get("mode", "plain"), c.get("pads", 0))
    assert (w.perm is not None) == perm_form
    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32(c["id"].encode()))
    cols = w.in_features
    Kx = 2 * cols if act == 1 else cols
    xv = ge._activation(M, Kx, torch.float16, gen, DEV)
    xbuf, x = ge._nan_view(M, Kx, 3, 64, torch.float16, DEV)
    x.copy_(xv)
    bias = (torch.randn(N, generator=gen, device=DEV) * 0.1).half() if c.get("bias") else None
    nbytes = max(w.workspace_bytes(M), 4096)
    ws = native.Workspace(nbytes, DEV)

    def call():
        ws.buf[4096:] = 0xFF  # NaN in every fp32 slab word
        obuf, out = ge._nan_view(M, N, 3, 32, torch.float16, DEV)
        native.gptq8_gemm(x, w, ws, bias=bias, act=act, out=out)
        torch.cuda.synchronize()
        return obuf, out

    obuf, got = call()
    assert ws.nbytes == nbytes, "the workspace grew: its size query is too small"
    assert not ws.buf[:4096].any(), f"{c['id']}: counters not left at zero"
    assert torch.isnan(xbuf[M:]).all() and torch.isnan(xbuf[:, Kx:]).all(), f"{c['id']}: x padding written"
    assert torch.isnan(obuf[M:]).all() and torch.isnan(obuf[:, N:]).all(), f"{c['id']}: out margins written"
    assert act != 1 or cols == K
    ref, tol = ge._reference(dict(K=K, N=N, act=act), xv, Wx, bias, torch.float16)  # K: the rows the kernel accumulates over
    assert ref.shape == got.shape == (M, N)
    ge._check(got, ref, tol, c["id"])
    _, again = call()
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), f"{c['id']}: second call on the same workspace differs"


@pytest.mark.parametrize("what", ["rows", "group_size"])
def test_bad_arguments_are_refused_and_write_nothing(what):
    from tgis_amd import native

    lib = _lib()
    K, N = 256, 64
    w, _, _ = _weight(K, N, 2)
    M, groups = (65, 2) if what == "rows" else (8, 32)  # 65 rows; groups of 8 rows
    x = torch.ones((M, K), dtype=torch.float16, device=DEV)
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
    ws = native.Workspace(1 << 20, DEV)
    ws.buf[4096:] = 0xFF
    rc = lib.tgis_gptq8_gemm_f16(x.data_ptr(), K, w.image.data_ptr(), None, None, out.data_ptr(), N, M, K, N, groups, 0, ws.ptr,
                                 ws.nbytes, native._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"tgis_gptq8_gemm_f16" in lib.tgis_last_error()
    assert torch.isnan(out).all() and (ws.buf[4096:] == 0xFF).all() and not ws.buf[:4096].any()
    if what == "group_size":
        with pytest.raises(native.TgisHipError, match="multiple of 16"):
            native.Gptq8Weight(torch.zeros((K // 4, N), dtype=torch.int32, device=DEV),
                               torch.zeros((32, N // 4), dtype=torch.int32, device=DEV),
                               torch.ones((32, N), dtype=torch.float16, device=DEV), None, 8, 8)
    lib.tgis_clear_error()
