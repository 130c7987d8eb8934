"""GPU: tgis_rope_kv_write_qknorm and tgis_rope_kv_write_prefill_qknorm on every case of tests/qknorm_cases.py against the fp64
restatement of tests/qknorm_ref.py, whose docstring derives the bound (one rounding of the output type on |ref| plus
2^-20-relative fp32 terms; nothing measured).

The harness is that of tests/test_rowwise_edges_gpu.py: the output is a view into a NaN-filled buffer with extra rows and 16
extra columns that must stay NaN, slab padding is NaN input, the pools are NaN (one-byte pools: the code 0x7F, which the
writers never store) and every slot no token owns must stay so; v heads are bit-exact copies; each owned slot holds the bits the
same call wrote to qkv (one-byte pools: tests/kv_fp8_ref.quantize of them); a second call on fresh copies gives the same bits.
The page-wise form must write, for the same tokens, the bits the per-token form writes (q in qkv, k and v in the pages), leave
k / v inside qkv alone, zero the tail slots of a last page and touch no page in front of past_lens."""
import itertools
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8_ref as q8  # noqa: E402
import qknorm_cases as qc  # noqa: E402
import qknorm_ref  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
DEV = "cuda:0"
MAX_POS = 4096
KV_MODEL, KV_FP8 = 0, 1
NAN8 = 0x7F  # the e4m3 NaN code: never written by the cache writers


def _lib():
    from tgis_amd import native

    return native.load_library()


def _stream():
    from tgis_amd import native

    return native._stream()


def _code(dt):
    from tgis_amd import native

    return native.dtype_code(dt)


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(cid):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(cid.encode()))
    return g


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def _bits(t):
    return t.view({torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}.get(t.dtype, t.dtype))


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


def _ok(rc_, what):
    assert rc_ == 0, f"{what}: {_lib().tgis_last_error().decode()}"


def _check(got, ref, tol, what):
    got = got.double()
    assert not torch.isnan(got).any(), f"{what}: NaN in the output"
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {i}: got "
                             f"{got[tuple(i)].item():.8g} ref {ref[tuple(i)].item():.8g} tol {tol[tuple(i)].item():.3g}")


def _exact(got, want, what):
    if not _same(got, want):
        d = (_bits(got.contiguous()) != _bits(want.contiguous())).nonzero()
        i = d[0].tolist()
        raise AssertionError(f"{what}: {d.shape[0]} elements differ in their bits; first at {i}: got "
                             f"{got[tuple(i)].item()!r} want {want[tuple(i)].item()!r}")


def _pools(pages, Hkv, D, dt, kv8):
    if not Hkv:
        return None, None
    if kv8:
        return tuple(torch.full((pages, Hkv, 32 * D), NAN8, dtype=torch.uint8, device=DEV) for _ in range(2))
    return _nan((pages, Hkv, 32 * D), dt), _nan((pages, Hkv, 32 * D), dt)


def _unpack(kp, vp, Hkv, D):
    """[pages * 32, Hkv, D] by slot, on the host."""
    import oracle.ops_ref as ops_ref

    kpc, vpc = kp.cpu(), vp.cpu()
    Ks, Vs = zip(*(ops_ref.kv_page_unpack(kpc, vpc, pg, Hkv, D) for pg in range(kp.shape[0])))
    return torch.cat(Ks), torch.cat(Vs)


def _untouched(pool_rows):
    if pool_rows.dtype == torch.uint8:
        return bool((pool_rows == NAN8).all())
    return bool(torch.isnan(pool_rows).all())


def _tables(rot, dt):
    import oracle.ops_ref as ops_ref

    cos, sin = ops_ref.rope_tables(rot, 10000.0, MAX_POS, dt)
    return cos.to(DEV), sin.to(DEV)


def _weights(D, dt, gen):
    """q_norm / k_norm weights in [0.5, 2]: far from the identity."""
    return tuple((0.5 + 1.5 * torch.rand(D, generator=gen, device=DEV)).to(dt) for _ in range(2))


def _kv_args(c):
    return (KV_FP8, *qc.KV8_SCALES) if c["kv8"] else (KV_MODEL, 1.0, 1.0)


def _cache_expect(out_rows, scale, kv8):
    """What a pool must hold for the rounded rows the call wrote to qkv."""
    return q8.quantize(out_rows, scale) if kv8 else out_rows


# ---- per token --------------------------------------------------------------------------------------------------------------
def _rewrite_slabs(buf, vals, rows, hidden):
    """vals [S, rows, hidden] into slabs stored in 32-row units [rows / 32][S][32][ld]; the rest stays NaN."""
    for blk in range(buf.shape[0]):
        r0, r1 = blk * 32, min(rows, blk * 32 + 32)
        buf[blk, :, :r1 - r0, :hidden] = vals[:, r0:r1]


def _slab_sum(vals, bias):
    """fp32, s = 0..S-1 in order, then the bias."""
    acc = vals[0].clone()
    for s in range(1, vals.shape[0]):
        acc = acc + vals[s]
    if bias is not None:
        acc = acc + bias.float()
    return acc


def _token_data(c, gen):
    T, H, Hkv, D, dt = c["T"], c["H"], c["Hkv"], c["D"], DT[c["dtype"]]
    N = (H + 2 * Hkv) * D
    d = dict(N=N, ld=N + 16)
    pos = torch.randint(0, MAX_POS, (T,), generator=gen, device=DEV, dtype=torch.int32)
    pos[0] = MAX_POS - 1  # the last row of the cos / sin tables
    d["pos"] = pos
    d["pages"] = -(-T // 32) + 2
    d["slots"] = torch.randperm(d["pages"] * 32, generator=gen, device=DEV)[:T].to(torch.int32) if Hkv else None
    d["cos"], d["sin"] = _tables(c["rot"], dt)
    d["qw"], d["kw"] = _weights(D, dt, gen)
    if c["S"]:
        S, sl = c["S"], N + c["slab_pad"]
        d["slabs"] = torch.full((-(-T // 32), S, 32, sl), float("nan"), device=DEV)
        d["vals"] = torch.randn((S, T, N), generator=gen, device=DEV) * (1.5 / S ** 0.5)
        _rewrite_slabs(d["slabs"], d["vals"], T, N)
        d["bias"] = (torch.randn(N, generator=gen, device=DEV) * 0.3).to(dt) if c["bias"] else None
        d["x"] = _slab_sum(d["vals"], d["bias"]).to(dt)
    else:
        x = torch.randn((T, N), generator=gen, device=DEV) * 1.5
        if c["special"]:
            x[0, :D] = 0.0  # an all-zero q head: rstd = eps^-1/2, the output stays zero
            if dt == torch.float16:  # a row whose squares (up to 9e8) exist only in fp32
                mag = (0.5 + 0.5 * torch.rand(N, generator=gen, device=DEV)) * 3e4
                x[1] = torch.where(x[1] < 0, -mag, mag)
        d["x"] = x.to(dt)
    return d


def _token_call(c, d, T=None):
    """One launch on a fresh copy of the input (no slabs: in place) and untouched pools: (rc, out buffer [T + 3, ld], k, v)."""
    lib, dt = _lib(), DT[c["dtype"]]
    T = c["T"] if T is None else T
    H, Hkv, D, N = c["H"], c["Hkv"], c["D"], d["N"]
    buf = _nan((c["T"] + 3, d["ld"]), dt)
    kp, vp = _pools(d["pages"], Hkv, D, dt, c["kv8"])
    if c["S"]:
        src = (_p(d["slabs"]), c["S"], N + c["slab_pad"], _p(d["bias"]))
    else:
        buf[:c["T"], :N] = d["x"]
        src = (None, 0, 0, None)
    r = lib.tgis_rope_kv_write_qknorm(_p(buf), d["ld"], *src, _p(d["qw"]), _p(d["kw"]), qc.EPS, _p(d["cos"]), _p(d["sin"]),
                                      _p(d["pos"]), _p(d["slots"]), _p(kp), _p(vp), T, H, Hkv, D, c["rot"], _code(dt),
                                      *_kv_args(c), _stream())
    torch.cuda.synchronize()
    return r, buf, kp, vp


@pytest.mark.parametrize("c", qc.TOKEN_CASES, ids=[c["id"] for c in qc.TOKEN_CASES])
def test_per_token(c):
    assert qc.case_form(c, _lib()) == tuple(c["form"])
    T, H, Hkv, D = c["T"], c["H"], c["Hkv"], c["D"]
    d = _token_data(c, _gen(c["id"]))
    N = d["N"]
    r, buf, kp, vp = _token_call(c, d)
    _ok(r, c["id"])
    assert torch.isnan(buf[T:]).all() and torch.isnan(buf[:, N:]).all(), f"{c['id']}: qkv padding written"
    out = buf[:T, :N].view(T, H + 2 * Hkv, D)
    x = d["x"].view(T, H + 2 * Hkv, D)
    ref, tol = qknorm_ref.expect(x, d["qw"], d["kw"], qc.EPS, d["cos"], d["sin"], d["pos"], H, Hkv, c["rot"])
    _exact(out[:, H + Hkv:], x[:, H + Hkv:], c["id"] + " v heads")
    _check(out, ref, tol, c["id"])
    if c["special"]:
        assert (_bits(out[0, 0]) & 0x7FFF == 0).all(), f"{c['id']}: the all-zero q head is not zero"
    if Hkv:
        Kall, Vall = _unpack(kp, vp, Hkv, D)
        sl = d["slots"].long().cpu()
        oc = out.cpu()
        ks, vs = qc.KV8_SCALES
        _exact(Kall[sl], _cache_expect(oc[:, H:H + Hkv], ks, c["kv8"]), c["id"] + " k cache")
        _exact(Vall[sl], _cache_expect(oc[:, H + Hkv:], vs, c["kv8"]), c["id"] + " v cache")
        free = torch.ones(d["pages"] * 32, dtype=torch.bool)
        free[sl] = False
        assert _untouched(Kall[free]) and _untouched(Vall[free]), f"{c['id']}: a slot no token owns was written"
    if c["S"]:
        assert torch.isnan(d["slabs"].view(-1, 32, N + c["slab_pad"])[:, :, N:]).all()  # (slab padding stays NaN input)
    r2, buf2, kp2, vp2 = _token_call(c, d)
    _ok(r2, c["id"])
    assert _same(buf, buf2) and (not Hkv or (_same(kp, kp2) and _same(vp, vp2))), f"{c['id']}: second call differs"


def test_per_token_zero_tokens():
    for c in (qc.TOKEN_CASES[0], next(x for x in qc.TOKEN_CASES if x["S"] and x["Hkv"])):
        d = _token_data(c, _gen(c["id"]))
        r, buf, kp, vp = _token_call(c, d, T=0)
        _ok(r, c["id"] + " T = 0")
        assert _untouched(kp) and _untouched(vp), f"{c['id']}: T = 0 wrote the cache"
        if c["S"]:
            assert torch.isnan(buf).all(), f"{c['id']}: T = 0 wrote the output"
        else:
            assert _same(buf[:c["T"], :d["N"]], d["x"]), f"{c['id']}: T = 0 changed qkv"


# ---- page-wise ----------------------------------------------------------------------------------------------------------------
def _page_setup(c, gen):
    lens, H, Hkv, D, dt = c["lens"], c["H"], c["Hkv"], c["D"], DT[c["dtype"]]
    past = c["past"] or [0] * len(lens)
    B, T, N = len(lens), sum(lens), (H + 2 * Hkv) * D
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=DEV)
    npg = [(p + n + 31) // 32 for p, n in zip(past, lens)]  # table entries of a sequence: its reused pages, then its own
    pages = sum(npg) + 3  # 3 pages no sequence owns
    max_pages = max(max(p // 32 for p in past) + c["form"][0], max(npg)) + 1
    perm = torch.randperm(pages, generator=gen, device=DEV).tolist()
    spare = perm[sum(npg)]
    bt = torch.full((B, max_pages), spare, dtype=torch.int32)  # entries past a sequence's pages: a page nobody owns
    k = 0
    for b, n in enumerate(npg):
        bt[b, :n] = torch.tensor(perm[k:k + n], dtype=torch.int32)
        k += n
    where = [p + torch.arange(n) for p, n in zip(past, lens)]  # cache positions of the tokens
    pos = torch.cat([w.to(torch.int32) + (MAX_POS - int(w[-1]) - 1 if b == 0 else 0) for b, w in enumerate(where)])
    slots = torch.cat([bt[b, w // 32] * 32 + w % 32 for b, w in enumerate(where)])
    reused = torch.cat([bt[b, :p // 32] for b, p in enumerate(past)]).long()  # pages in front of past_lens
    x = (torch.randn((T, N), generator=gen, device=DEV) * 1.5).to(dt)
    cos, sin = _tables(c["rot"], dt)
    qw, kw = _weights(D, dt, gen)
    past_dev = torch.tensor(past, dtype=torch.int32, device=DEV) if c["past"] else None
    return dict(B=B, T=T, N=N, ld=N + 16, cu=cu, bt=bt.to(DEV), pages=pages, pos=pos.to(DEV), slots=slots.to(torch.int32),
                x=x, cos=cos, sin=sin, qw=qw, kw=kw, past=past_dev, reused=reused, where=where)


def _page_call(c, s, T=None):
    lib, dt = _lib(), DT[c["dtype"]]
    H, Hkv, D = c["H"], c["Hkv"], c["D"]
    buf = _nan((s["T"] + 3, s["ld"]), dt)
    buf[:s["T"], :s["N"]] = s["x"]
    kp, vp = _pools(s["pages"], Hkv, D, dt, c["kv8"])
    r = lib.tgis_rope_kv_write_prefill_qknorm(_p(buf), s["ld"], _p(s["qw"]), _p(s["kw"]), qc.EPS, _p(s["cos"]), _p(s["sin"]),
                                              _p(s["pos"]), _p(s["cu"]), _p(s["past"]), _p(s["bt"]), s["bt"].shape[1], _p(kp),
                                              _p(vp), s["B"], s["T"] if T is None else T, c["max_len"], H, Hkv, D, c["rot"],
                                              _code(dt), *_kv_args(c), _stream())
    torch.cuda.synchronize()
    return r, buf, kp, vp


@pytest.mark.parametrize("c", qc.PAGE_CASES, ids=[c["id"] for c in qc.PAGE_CASES])
def test_page_wise(c):
    assert qc.case_form(c, _lib()) == tuple(c["form"])
    H, Hkv, D = c["H"], c["Hkv"], c["D"]
    s = _page_setup(c, _gen(c["id"]))
    T, N = s["T"], s["N"]
    r, buf, kp, vp = _page_call(c, s)
    _ok(r, c["id"])
    assert torch.isnan(buf[T:]).all() and torch.isnan(buf[:, N:]).all(), f"{c['id']}: qkv padding written"
    # the fp64 restatement: q in qkv, k in the pages (16-bit pools; one-byte pools are held to the per-token form below)
    x = s["x"].view(T, H + 2 * Hkv, D)
    ref, tol = qknorm_ref.expect(x, s["qw"], s["kw"], qc.EPS, s["cos"], s["sin"], s["pos"], H, Hkv, c["rot"])
    _check(buf[:T, :H * D].view(T, H, D), ref[:, :H], tol[:, :H], c["id"] + " q")
    _exact(buf[:T, H * D:N], s["x"][:, H * D:], c["id"] + " k / v input left alone")
    K, V = _unpack(kp, vp, Hkv, D)
    sl = s["slots"].long()
    if not c["kv8"]:
        _check(K[sl].to(DEV), ref[:, H:H + Hkv], tol[:, H:H + Hkv], c["id"] + " k pages")
    # the per-token form over the same slots writes the same bits
    tc = dict(c, T=T, S=0, special=False)
    td = dict(N=N, ld=s["ld"], pos=s["pos"], pages=s["pages"], slots=s["slots"].to(DEV), cos=s["cos"], sin=s["sin"], x=s["x"],
              qw=s["qw"], kw=s["kw"])
    r1, tbuf, tk, tv = _token_call(tc, td)
    _ok(r1, c["id"] + " per-token")
    _exact(buf[:T, :H * D], tbuf[:T, :H * D], c["id"] + " q vs the per-token form")
    Kt, Vt = _unpack(tk, tv, Hkv, D)
    _exact(K[sl], Kt[sl], c["id"] + " k slots vs the per-token form")
    _exact(V[sl], Vt[sl], c["id"] + " v slots vs the per-token form")
    vs = qc.KV8_SCALES[1]
    _exact(V[sl], _cache_expect(x[:, H + Hkv:].cpu(), vs, c["kv8"]), c["id"] + " v slots")
    tail = torch.zeros(s["pages"] * 32, dtype=torch.bool)
    bt = s["bt"].cpu()
    for b, w in enumerate(s["where"]):
        end = int(w[-1]) + 1
        if end % 32:
            last = int(bt[b, (end - 1) // 32])
            tail[last * 32 + end % 32:last * 32 + 32] = True
    assert (_bits(K[tail]) == 0).all() and (_bits(V[tail]) == 0).all(), f"{c['id']}: tail slots of a last page not +0"
    free = torch.ones(s["pages"] * 32, dtype=torch.bool)
    free[sl] = False
    free[tail] = False
    assert _untouched(K[free]) and _untouched(V[free]), f"{c['id']}: a slot no sequence owns was written"
    if c["past"]:
        front = (s["reused"][:, None] * 32 + torch.arange(32)).reshape(-1)
        assert front.numel() and free[front].all(), f"{c['id']}: the case has no page in front of past_lens"
    r2, buf2, kp2, vp2 = _page_call(c, s)
    _ok(r2, c["id"])
    assert _same(buf, buf2) and _same(kp, kp2) and _same(vp, vp2), f"{c['id']}: second call differs"


def test_page_wise_zero_tokens():
    c = qc.PAGE_CASES[0]
    s = _page_setup(c, _gen(c["id"]))
    r, buf, kp, vp = _page_call(c, s, T=0)
    _ok(r, "page-wise T = 0")
    assert _untouched(kp) and _untouched(vp) and _same(buf[:s["T"], :s["N"]], s["x"])
