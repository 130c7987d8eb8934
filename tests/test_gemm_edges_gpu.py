"""GPU: every GEMM case of tests/gemm_cases.py against an fp64 reference, with NaN guards around what it may touch.

Each case builds its weight on the device (int4 codes and zeros over 0..15, group scales a power of two apart from group to
group; or a dense f16 / bf16 weight), an activation with a non-zero mean per 256-column chunk, and checks
  |got - ref| <= A_OUT u_out |ref| + B_ACC K 2^-24 (|x| @ |W|) (+ the smallest subnormal of the output type)
where ref is x.double() @ W.double() (+ bias), W the f16 image of the int4 weight, and the epilogue is applied at the
product's rounding points (SiLU * up and GELU round their input to the model dtype first).  Around the call:
  - x is a view with ldx = K + 64 (2K + 64 for act 1) into a NaN-filled buffer with 3 NaN rows below it;
  - out is a [M, N] view into a NaN-filled [M + 3, N + 32] buffer: rows >= M and columns >= N must stay NaN;
  - the workspace past its 4096 bytes of arrival counters and the partial slab buffers are NaN-filled: a split that reads
    slabs nobody wrote fails; the counters must be zero again after the call;
  - tgis_debug_gemm_plan reports the case's variant, and a second call on the same workspace gives identical bits.
The fused qkv + rotary + cache-write launches (rope entries) are checked as GEMM, rounding to the model dtype, rotation in
fp64: q rows, and k / v in each row's cache slot; q outside [M, H D] and every cache slot no row owns must stay NaN.
Partial forms are checked through their consumer (rmsnorm_residual, layernorm_residual, layernorm2_residual): the reduced
residual stream they return is sum + bias + residual.  Variants only A/B knobs reach run in fresh child processes."""
import ctypes
import os
import subprocess
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu

A_OUT = 2.0  # unit roundoffs of the output per |ref|
B_ACC = 2.0  # fp32 accumulation: K 2^-24 per unit of |x| @ |W|
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}
DT = {"f16": torch.float16, "bf16": torch.bfloat16}


def _lib():
    from tgis_amd import native

    return native.load_library()


def _pack_rows(q):
    """[K, N] codes 0..15 -> [K / 8, N] int32, row k in nibble k % 8 (GPTQ qweight)."""
    K, N = q.shape
    sh = (torch.arange(8, device=q.device, dtype=torch.int64) * 4).view(1, 8, 1)
    v = (q.view(K // 8, 8, N).to(torch.int64) << sh).sum(1)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def _pack_cols(z):
    """[G, N] codes -> [G, N / 8] int32, column n in nibble n % 8 (GPTQ qzeros)."""
    G, N = z.shape
    sh = (torch.arange(8, device=z.device, dtype=torch.int64) * 4).view(1, 1, 8)
    v = (z.view(G, N // 8, 8).to(torch.int64) << sh).sum(2)
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def _int4_weight(c, gen, dev):
    """(GptqWeight, W [K, N] fp64: the f16 image of the dequantised weight in original row order)."""
    from tgis_amd import native

    K, N, G = c["K"], c["N"], c["groups"]
    gs = K // G
    q = torch.randint(0, 16, (K, N), generator=gen, device=dev, dtype=torch.int32)
    z = torch.randint(0, 16, (G, N), generator=gen, device=dev, dtype=torch.int32)  # stored zeros (zero point z + 1)
    base = (torch.rand((1, N), generator=gen, device=dev) + 0.5) * (2.0 / 15.0) * 0.05
    s = (base * torch.pow(2.0, -(torch.arange(G, device=dev) % 4).float()).view(G, 1)).half()  # groups 2^k apart
    if c.get("act_order"):
        g_idx = torch.empty(K, dtype=torch.int32, device=dev)
        g_idx[torch.randperm(K, generator=gen, device=dev)] = torch.arange(K, device=dev, dtype=torch.int32) // gs
    else:
        g_idx = torch.arange(K, device=dev, dtype=torch.int32) // gs
    gl = g_idx.long()
    W = ((q - z[gl] - 1).double() * s.double()[gl]).half().double()
    w = native.GptqWeight(_pack_rows(q), _pack_cols(z), s, g_idx.cpu() if c.get("act_order") else None, 4, gs,
                          gate_up=c.get("act", 0) == 2, rope=_rope_image(c))
    return w, W


def _dense_weight(c, gen, dev):
    from tgis_amd import native

    dt = DT[c["dtype"]]
    Wt = (torch.randn((c["N"], c["K"]), generator=gen, device=dev) * 0.05).to(dt)
    return native.DenseWeight(Wt, gate_up=c.get("act", 0) == 2, rope=_rope_image(c)), Wt.double().t()


def _rope_image(c):
    return (c["D"], c["H"] + c["Hkv"]) if c["entry"].endswith("_rope") else None


def _activation(M, Kx, dt, gen, dev):
    x = torch.randn((M, Kx), generator=gen, device=dev) * 0.5
    mean = 0.25 + 0.25 * (torch.arange(Kx, device=dev) // 256 % 4).float()  # non-zero mean per 256-column chunk
    return ((x + mean) * min(1.0, 32.0 / Kx ** 0.5)).to(dt)  # sums stay O(10) at any K: SiLU * up must not overflow f16


def _nan_view(rows, cols, pad_rows, pad_cols, dt, dev):
    buf = torch.full((rows + pad_rows, cols + pad_cols), float("nan"), dtype=dt, device=dev)
    return buf, buf[:rows, :cols]


def _rnd(t, dt):
    return t.to(dt).double()


def _silu(v):
    return v / (1.0 + torch.exp(-v))


def _check(got, ref, tol, what):
    got = got.double()
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    bad = err > tol
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {i}: got "
                             f"{got[tuple(i)].item():.6g} ref {ref[tuple(i)].item():.6g} tol {tol[tuple(i)].item():.3g}")


def _reference(c, x, W, bias, dt_out):
    """(ref, tol) of the finished output in fp64."""
    K, act = c["K"], c.get("act", 0)
    dt = x.dtype
    u = U[dt]
    xd = x.double()
    xa = xd.abs()
    slack = 0.0
    if act == 1:  # operand silu(gate) * up, rounded as the eager reference rounds it
        g, up = xd[:, :K], xd[:, K:]
        xd = _rnd(_rnd(_silu(g), dt) * up, dt)
        xa = xd.abs()
        slack = 2 * u  # one rounding flip of the staged operand
    y = xd @ W
    A = xa @ W.abs()
    if bias is not None:
        y = y + bias.double()
        A = A + bias.double().abs()
    e = B_ACC * K * 2.0 ** -24 * A + slack * A
    if act == 2:
        half = c["N"] // 2
        g, up, eg, eu = y[:, :half], y[:, half:], e[:, :half], e[:, half:]
        gr, ur = _rnd(g, dt), _rnd(up, dt)
        sl = _rnd(_silu(gr), dt)
        ref = _rnd(sl * ur, dt)
        dg = 2 * (eg + u * g.abs()) + TINY[dt]
        du = 2 * (eu + u * up.abs()) + TINY[dt]
        tol = A_OUT * u * ref.abs() + ur.abs() * (1.1 * dg + 2 * u * sl.abs()) + (sl.abs() + 1.1 * dg) * du + TINY[dt]
        return ref, tol
    gelu = {4: "none", 5: "tanh"}.get(act)
    if gelu:
        yr = _rnd(y, dt)
        ref = _rnd(torch.nn.functional.gelu(yr, approximate=gelu), dt)
        tol = A_OUT * u * ref.abs() + 1.2 * (e + A_OUT * u * y.abs()) + TINY[dt]
        return ref, tol
    uo = U[dt_out]
    return y, A_OUT * uo * y.abs() + e + TINY[dt_out]


def _plan_check(c, lib):
    got = gc.variant_key(c, lib)
    assert got == tuple(c["key"]), f"{c['id']}: lands on {gc.key_str(got)}, not {gc.key_str(c['key'])}"


def _full_call(c, w, x, bias, ws, lib):
    """Run the finished form; returns (result tensor, the NaN-guard buffer or None)."""
    from tgis_amd import native

    M, N, act = c["M"], c["N"], c.get("act", 0)
    Nout = N // 2 if act == 2 else N
    if c["entry"] == "dense":
        dt_out = torch.float32 if c.get("out_f32") else w.dtype
        buf, out = _nan_view(M, Nout, 3, 32, dt_out, x.device)
        native.dense_gemm(x, w, ws, bias=bias, out_f32=bool(c.get("out_f32")), act=act, out=out)
        return out, buf
    if c.get("frag_in"):
        xf = native.FragAct.from_rows(x.contiguous())
        if c.get("frag_out"):
            return native.gptq_gemm(xf, w, ws, bias=bias, act=act, out_frag=True).to_rows(), None
        buf, out = _nan_view(M, Nout, 3, 32, torch.float16, x.device)
        native.gptq_gemm(xf, w, ws, bias=bias, act=act, out=out)
        return out, buf
    buf, out = _nan_view(M, Nout, 3, 32, torch.float16, x.device)
    native.gptq_gemm(x, w, ws, bias=bias, act=act, out=out)
    return out, buf


def _partial_call(c, w, x, lib):
    """The partial form on a NaN-filled slab buffer of the size the library asks for; returns a native.Partial."""
    from tgis_amd import native

    M, K, N = c["M"], c["K"], c["N"]
    S, ld = ctypes.c_int(), ctypes.c_int64()
    if c["entry"] == "gptq_partial":
        nbytes = lib.tgis_gptq_gemm_partial_bytes(M, K, N)
        slabs = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=x.device)
        if c.get("frag_in"):
            xf = native.FragAct.from_rows(x.contiguous())
            xp, ldx = xf.buf.data_ptr(), native.LD_FRAGMENTS
        else:
            xp, ldx = x.data_ptr(), x.stride(0)
        rc = lib.tgis_gptq_gemm_f16_partial(xp, ldx, w.image.data_ptr(), native._ptr(w.perm), M, K, N, w.groups,
                                            c.get("act", 0), slabs.data_ptr(), nbytes, ctypes.byref(S), ctypes.byref(ld),
                                            native._stream())
        dt = torch.float16
    else:
        nbytes = lib.tgis_dense_gemm_partial_bytes(M, K, N)
        slabs = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=x.device)
        rc = lib.tgis_dense_gemm_partial(x.data_ptr(), x.stride(0), w.image.data_ptr(), M, K, N, native.dtype_code(w.dtype),
                                         c.get("act", 0), slabs.data_ptr(), nbytes, ctypes.byref(S), ctypes.byref(ld),
                                         native._stream())
        dt = w.dtype
    assert rc == 0, lib.tgis_last_error().decode()
    p = native.Partial(slabs, S.value, ld.value, M, N, None)
    p.dtype = dt
    return p


def _consume(c, p, bias, residual, dev):
    """The reduced residual stream (sum + bias + residual) the consumer kernel returns."""
    from tgis_amd import native

    N, dt = c["N"], residual.dtype
    p.bias = bias
    w1 = torch.ones(N, dtype=dt, device=dev)
    b1 = torch.zeros(N, dtype=dt, device=dev)
    if c["consumer"] == "rms":
        return native.rmsnorm_residual(p, residual, w1, 1e-5)[1]
    if c["consumer"] == "ln":
        return native.layernorm_residual(p, residual, w1, b1, 1e-5)[1]
    return native.layernorm2_residual(residual, p, None, w1, b1, 1e-5)[2]


def run_case(c, lib=None):
    from tgis_amd import native

    lib = lib or _lib()
    for fn in (lib.tgis_gptq_gemm_partial_bytes, lib.tgis_dense_gemm_partial_bytes, lib.tgis_gptq_gemm_workspace_bytes,
               lib.tgis_dense_gemm_workspace_bytes):
        fn.restype = ctypes.c_int64
    _plan_check(c, lib)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(zlib.crc32(c["id"].encode()))
    M, K, N, act = c["M"], c["K"], c["N"], c.get("act", 0)
    dense = c["entry"].startswith("dense")
    w, W = _dense_weight(c, gen, dev) if dense else _int4_weight(c, gen, dev)
    dt = w.dtype if dense else torch.float16
    Kx = 2 * K if act == 1 else K
    xv = _activation(M, Kx, dt, gen, dev)
    xbuf, x = _nan_view(M, Kx, 3, 64, dt, dev)
    x.copy_(xv)
    Nb = N // 2 if act == 2 else N
    bias = (torch.randn(N, generator=gen, device=dev) * 0.1).to(dt) if c.get("bias") else None

    if c["entry"].endswith("_partial"):
        residual = (torch.randn((M, N), generator=gen, device=dev) * 0.5).to(dt)
        ref, tol = _reference(c, xv, W, bias, dt)
        ref = ref + residual.double()
        tol = tol + U[dt] * A_OUT * ref.abs() + TINY[dt]
        p = _partial_call(c, w, x, lib)
        got = _consume(c, p, bias, residual, dev).clone()
        torch.cuda.synchronize()
        _check(got, ref, tol, c["id"])
        again = _consume(c, _partial_call(c, w, x, lib), bias, residual, dev)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), again.view(torch.int16)), f"{c['id']}: second call differs"
        return

    if c["entry"].endswith("_rope"):
        _run_rope(c, w, W, x, xv, bias, dt, gen, dev)
        return

    nbytes = max(w.workspace_bytes(M), 4096)  # (the size query includes the 4096 bytes of arrival counters)
    ws = native.Workspace(nbytes, dev)
    ws.buf[4096:] = 0xFF  # NaN in every fp32 slab word
    got, obuf = _full_call(c, w, x, bias, ws, lib)
    got = got.clone()
    torch.cuda.synchronize()
    assert ws.nbytes == nbytes, "the workspace grew: its size query is too small"
    assert not ws.buf[:4096].any(), f"{c['id']}: arrival counters not left at zero"
    assert torch.isnan(xbuf[M:]).all() and torch.isnan(xbuf[:, Kx:]).all(), f"{c['id']}: x padding written"
    if obuf is not None:
        assert torch.isnan(obuf[M:]).all(), f"{c['id']}: rows >= M of out written"
        assert torch.isnan(obuf[:, got.shape[1]:]).all(), f"{c['id']}: columns >= N of out written"
    ref, tol = _reference(c, xv, W, None if bias is None else bias[:N], got.dtype)
    assert ref.shape == got.shape == (M, Nb)
    _check(got, ref, tol, c["id"])
    ws.buf[4096:] = 0xFF
    again, _ = _full_call(c, w, x, bias, ws, lib)
    torch.cuda.synchronize()
    bits = torch.int32 if got.dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(bits), again.view(bits)), f"{c['id']}: second call on the same workspace differs"


def _rope_call(c, w, x, bias, cos, sin, pos, slots, pages, dev):
    """One fused qkv + rotary + cache-write launch on NaN-filled q rows and cache pools: (q guard buffer, k pool, v pool)."""
    from tgis_amd import native

    M, H, Hkv, D = c["M"], c["H"], c["Hkv"], c["D"]
    qbuf, q = _nan_view(M, H * D, 3, 32, x.dtype, dev)
    kp = torch.full((pages, Hkv, 32 * D), float("nan"), dtype=x.dtype, device=dev)
    vp = torch.full_like(kp, float("nan"))
    xa = native.FragAct.from_rows(x.contiguous()) if c.get("frag_in") else x
    fn = native.dense_gemm_rope if c["entry"] == "dense_rope" else native.gptq_gemm_rope
    fn(xa, w, bias, cos, sin, pos, slots, kp, vp, H, Hkv, D, out=q)
    torch.cuda.synchronize()
    return qbuf, kp, vp


def _run_rope(c, w, W, x, xv, bias, dt, gen, dev):
    """q rows, then k and v of each row in its cache slot, against GEMM -> round to the model dtype -> rotate in fp64.
    Cache slots no row was given and q columns / rows outside [M, H D] must stay NaN."""
    import oracle.ops_ref as ops_ref

    M, K, H, Hkv, D = c["M"], c["K"], c["H"], c["Hkv"], c["D"]
    u, r = U[dt], D // 2
    cos, sin = (t.to(dev) for t in ops_ref.rope_tables(D, 10000.0, 4096, dt))
    pos = torch.randint(0, 4096, (M,), generator=gen, device=dev, dtype=torch.int32)
    pages = (M + 31) // 32 + 2
    slots = torch.randperm(pages * 32, generator=gen, device=dev)[:M].to(torch.int32)
    qbuf, kp, vp = _rope_call(c, w, x, bias, cos, sin, pos, slots, pages, dev)

    y = xv.double() @ W
    A = xv.double().abs() @ W.abs()
    if bias is not None:
        y, A = y + bias.double(), A + bias.double().abs()
    yr = _rnd(y, dt)
    d = B_ACC * K * 2.0 ** -24 * A + 2 * u * y.abs() + TINY[dt]  # a flip of the kernel's own rounding of the sum
    cs, sn = cos.double()[pos.long()][:, None, :], sin.double()[pos.long()][:, None, :]

    def rotate(t, dt_):
        t1, t2 = t[..., :r], t[..., r:]
        return torch.cat([t1 * cs - t2 * sn, t1 * sn + t2 * cs], -1), torch.cat([dt_[..., :r] + dt_[..., r:]] * 2, -1)

    want_q, dq = rotate(yr[:, :H * D].view(M, H, D), d[:, :H * D].view(M, H, D))
    want_k, dk = rotate(yr[:, H * D:(H + Hkv) * D].view(M, Hkv, D), d[:, H * D:(H + Hkv) * D].view(M, Hkv, D))
    want_v, dv = yr[:, (H + Hkv) * D:].view(M, Hkv, D), d[:, (H + Hkv) * D:].view(M, Hkv, D)
    want_q, want_k = _rnd(want_q, dt), _rnd(want_k, dt)

    q = qbuf[:M, :H * D].view(M, H, D)
    assert torch.isnan(qbuf[M:]).all() and torch.isnan(qbuf[:, H * D:]).all(), f"{c['id']}: q written outside [M, H D]"
    _check(q, want_q, A_OUT * u * want_q.abs() + dq, c["id"] + " q")
    kpc, vpc = kp.cpu(), vp.cpu()
    Ks, Vs = zip(*(ops_ref.kv_page_unpack(kpc, vpc, pg, Hkv, D) for pg in range(pages)))
    Kall, Vall = torch.cat(Ks).to(dev), torch.cat(Vs).to(dev)  # [pages * 32, Hkv, D] by slot
    sl = slots.long()
    _check(Kall[sl], want_k, A_OUT * u * want_k.abs() + dk, c["id"] + " k cache")
    _check(Vall[sl], want_v, A_OUT * u * want_v.abs() + dv, c["id"] + " v cache")
    free = torch.ones(pages * 32, dtype=torch.bool, device=dev)
    free[sl] = False
    assert torch.isnan(Kall[free]).all() and torch.isnan(Vall[free]).all(), f"{c['id']}: a cache slot no row owns was written"
    again = _rope_call(c, w, x, bias, cos, sin, pos, slots, pages, dev)
    for a, b, what in zip((qbuf, kp, vp), again, ("q", "k pool", "v pool")):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{c['id']}: second call differs ({what})"


@pytest.mark.parametrize("case", gc.CASES, ids=[c["id"] for c in gc.CASES])
def test_case(case):
    run_case(case)


# ---- variants only the documented A/B knobs reach: fresh child processes (the knobs are read once into statics) --------
def _E(**kw):
    return gc.K_(**kw)


ENV_RUNS = {
    "tall_bmr2": ({"TGIS_TALL_MIN_M": "33"}, [
        dict(id="tall-bmr2-split", entry="gptq", M=40, K=1024, N=512, groups=8, bias=True,
             key=_E(family="tall", mr=2, tw=1, g64=1)),
        dict(id="tall-bmr2-silu", entry="gptq", M=64, K=1024, N=1024, groups=8, act=2, bias=True,
             key=_E(family="tall", mr=2, tw=1, act=2, g64=1)),
        dict(id="tall-bmr2-partial", entry="gptq_partial", M=40, K=1024, N=512, groups=8, bias=False, consumer="rms",
             key=_E(family="tall", mr=2, tw=1, g64=1)),
        dict(id="tall-bmr4-m100", entry="gptq", M=100, K=512, N=256, groups=1, bias=False,
             key=_E(family="tall", mr=4, tw=1, g64=1)),
    ]),
    "tall_tw2": ({"TGIS_TALL_TW": "2"}, [
        dict(id="tall-tw2-split", entry="gptq", M=300, K=1024, N=2048, groups=8, bias=True,
             key=_E(family="tall", mr=4, tw=2, g64=1)),
        dict(id="tall-tw2-silu", entry="gptq", M=300, K=1024, N=2048, groups=8, act=2, bias=False,
             key=_E(family="tall", mr=4, tw=2, act=2, g64=1)),
    ]),
    "gptq_plan_tn3_wk2": ({"TGIS_GPTQ_PLAN": "512,2,2,3"}, [
        dict(id="plan-32-tn3wk2", entry="gptq", M=20, K=1024, N=2048, groups=8, bias=True,
             key=_E(family="stream", tn=3, wk=2, g64=1)),
        dict(id="plan-64-tn3wk2-act1-ao", entry="gptq", M=40, K=1024, N=2048, groups=8, act=1, act_order=True, bias=False,
             key=_E(family="stream", tn=3, wk=2, mr=2, act=1, g64=1, perm=1)),
        dict(id="plan-32-tn3wk2-act1-g32", entry="gptq", M=20, K=1024, N=2048, groups=32, act=1, bias=True,
             key=_E(family="stream", tn=3, wk=2, act=1)),
    ]),
    "gptq_plan_silu": ({"TGIS_GPTQ_PLAN": "1024,1,2,3"}, [
        dict(id="plan-64-tn3wk2-silu", entry="gptq", M=40, K=1024, N=2048, groups=8, act=2, bias=True,
             key=_E(family="stream", tn=3, wk=2, mr=2, act=2, g64=1)),
    ]),
    "dense_plan": ({"TGIS_DENSE_PLAN": "3,2,2"}, [
        dict(id="dplan-s3-bf16", entry="dense", M=8, K=4096, N=8192, dtype="bf16", bias=True,
             key=_E(family="dense", tn=2, wk=2, r16=1, dtype="bf16")),
        dict(id="dplan-s3-act1", entry="dense", M=8, K=4096, N=8192, dtype="f16", act=1, bias=False,
             key=_E(family="dense", tn=2, wk=2, r16=1, act=1, dtype="f16")),
    ]),
    "silu_split_always": ({"TGIS_SILU_SPLIT_BELOW": "100000"}, [
        dict(id="silu-split-wide-shard", entry="gptq", M=8, K=1024, N=8192, groups=8, act=2, bias=True,
             key=_E(family="split_silu", tn=4, wk=2, g64=1)),
    ]),
    "silu_split_never": ({"TGIS_SILU_SPLIT_BELOW": "0"}, [
        dict(id="silu-fused-narrow-ao", entry="gptq", M=33, K=1056, N=2048, groups=33, act=2, act_order=True, bias=True,
             key=_E(family="stream", tn=2, wk=2, mr=2, act=2, perm=1)),
    ]),
}


def _child(name):
    for c in ENV_RUNS[name][1]:
        run_case(c)
        print("ok", c["id"], flush=True)


@pytest.mark.parametrize("name", sorted(ENV_RUNS))
def test_env_variant(name):
    env = dict(os.environ)
    env.update(ENV_RUNS[name][0])
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "text-generation-inference_amd")]
    code = f"import sys; sys.path[:0] = {paths!r}; import test_gemm_edges_gpu as t; t._child({name!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    assert r.stdout.count("ok ") == len(ENV_RUNS[name][1]), r.stdout
