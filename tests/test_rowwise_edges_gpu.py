"""GPU: every row-wise case of tests/rowwise_cases.py against a plain high-precision reference, with NaN guards.

Bounds (u_out the unit roundoff of the output type, tiny its smallest subnormal):
  - bit-exact: the residual streams (res_out of every norm form, h' of layernorm2), restated on the host in fp32 in the
    kernel's add order (slabs s = 0..S-1, then the bias, rounded to the model dtype, then the residual; adds only), the
    unrotated parts of rope (dims >= rot, v heads, every dim without rope), each owned cache slot (the kernel's own k / v),
    embedding rows, decode slots and argmax ids;
  - norm outputs: fp64 statistics of that fp32 sum, |y - ref| <= u_out |ref| + 2^-16 (|n w| + |b|) + tiny, plus for
    LayerNorm 2^-17 mean|v| rstd |w| for the rounding of its fp32 mean (LN_MEAN, derived there).  Row 0 of a
    case is all zeros, row 1 constant (LayerNorm: y == bias) and row 2 sits at a mean 256+ standard deviations from zero,
    which a one-pass variance cannot resolve;
  - rope: fp64 rotation of the dtype-rounded input by the dtype cos / sin tables, u_out |ref| + 2^-20 (|x1 c| + |x2 s|) + tiny;
  - act_mul: fp64 with the kernel's two rounding points, 2 u_out |ref| + 2^-20 |g u| + tiny; gelu u_out |ref| + 2^-20 |x| + tiny;
  - argmax logprob: 1e-5 (1 + |ref|).
Every output is a view into a NaN-filled buffer with extra rows (and columns where the API takes a row stride) that must
stay NaN; input padding and slab padding are NaN so that an over-read shows up in the output.  A second call gives identical
bits, zero rows / T = 0 leave every output untouched, and the sampler's global-row kernel (a fresh child process with
TGIS_SAMPLER_GLOBAL_ROWS=1) is bit-identical to the register kernel."""
import itertools
import os
import subprocess
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowwise_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
EPS = 1e-5
EINVAL = -1
DEV = "cuda:0"
MAX_POS = 4096
# LayerNorm subtracts its fp32 mean from every element, so the mean's own error is an absolute error of n (times rstd),
# not one relative to n: near n = 0 it is all there is.  The kernel forms the row sum in at most 64 sequential adds per
# thread, 6 butterfly levels and 8 wave partials, then divides: |mean error| <= (64 + 6 + 8 + 1) 2^-24 mean|v| < 2^-17 mean|v|
# (the recursive-summation bound).  RMSNorm has no such term: its statistic errs relative to n only.
LN_MEAN = 2.0 ** -17


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


def _in_nan(data, pad_rows, pad_cols=0):
    """(buffer, view): `data` copied into a NaN-filled buffer with extra rows and columns."""
    R, C = data.shape
    buf = _nan((R + pad_rows, C + pad_cols), data.dtype)
    buf[:R, :C] = data
    return buf, buf[:R, :C]


def _pad_nan(buf, R, C, what):
    assert torch.isnan(buf[R:]).all() and torch.isnan(buf[:, C:]).all(), f"{what}: padding written"


# ---- norms ------------------------------------------------------------------------------------------------------------------
def _special_rows(c):
    """Rows 0 (zeros), 1 (constant), 2 (mean 256+ standard deviations from zero) when every input but the first is zeroed
    there: plain inputs without a GEMM bias."""
    if c["rows"] < 3 or c.get("xbias"):
        return False
    return not (c["op"] == "ln2" and (c["A"][1] or c["B"][1]))


def _offset_row(hidden, dt, gen):
    """A centre of 2048 (f16) or 256 (bf16) with 1 in 64 elements one ulp of it (2) above or below, balanced: the fp32 sums,
    the mean and the variance are exact, and from hidden 128 on the mean is 8192 (f16) or 1024 (bf16) standard deviations
    of 0.25 from zero (at least 256 below that).  E[x^2]
    in fp32 has a quantum of 1/2 (f16) or 1/128 (bf16) there, so E[x^2] - mean^2 cannot come near the variance of 1/16."""
    centre = 2048.0 if dt == torch.float16 else 256.0
    k = torch.zeros(hidden, device=DEV)
    m = max(hidden // 128, 1)
    idx = torch.randperm(hidden, generator=gen, device=DEV)[:2 * m]
    k[idx[:m]], k[idx[m:]] = 1.0, -1.0
    return (centre + 2.0 * k).to(dt)


def _norm_data(c, gen):
    rows, hidden, dt = c["rows"], c["hidden"], DT[c["dtype"]]
    mean = (torch.arange(rows, device=DEV) % 5 - 2).float().view(rows, 1) * 0.5

    def act(scale=0.7):
        return (torch.randn((rows, hidden), generator=gen, device=DEV) * scale + mean).to(dt)

    def vec(scale, shift=0.0):
        return (torch.randn(hidden, generator=gen, device=DEV) * scale + shift).to(dt)

    def slabs(S):
        buf = torch.full((-(-rows // 32), S, 32, hidden + c["slab_pad"]), float("nan"), device=DEV)
        val = torch.randn((S, rows, hidden), generator=gen, device=DEV) * (0.7 / S ** 0.5) + mean / S
        _rewrite_slabs(buf, val, rows, hidden)
        return buf, val

    d = dict(w=vec(0.3, 1.0), b=vec(0.2), w2=vec(0.3, -1.0), b2=vec(0.2))
    special = _special_rows(c)
    sp = None
    if special:
        sp = torch.stack([torch.zeros(hidden, device=DEV, dtype=dt), torch.full((hidden,), 1.5, device=DEV, dtype=dt),
                          _offset_row(hidden, dt, gen)])
    op = c["op"]
    if op in ("rms", "ln"):
        d["x"] = act()
        if special:
            d["x"][:3] = sp
    if op in ("rms", "ln", "rms_partial", "ln_partial"):
        d["res"] = act(0.5) if c["residual"] else None
        if special and d["res"] is not None:
            d["res"][:3] = 0
    if op.endswith("_partial"):
        d["slabs"], d["slab_vals"] = slabs(c["S"])
        d["xbias"] = vec(0.2) if c["xbias"] else None
        if special:
            d["slab_vals"][:, :3] = 0
            d["slab_vals"][0, :3] = sp.float()
            _rewrite_slabs(d["slabs"], d["slab_vals"], rows, hidden)
    if op == "ln2":
        d["h"] = act(0.5)
        if special:
            d["h"][:3] = sp
        for name, S in (("A", c["SA"]), ("B", c["SB"])):
            kind, has_bias = c[name]
            d[name + "bias"] = vec(0.2) if has_bias else None
            d[name] = d[name + "slabs"] = d[name + "vals"] = None
            if kind == "tensor":
                d[name] = act(0.5)
                if special:
                    d[name][:3] = 0
            elif kind == "slabs":
                d[name + "slabs"], d[name + "vals"] = slabs(S)
                if special:
                    d[name + "vals"][:, :3] = 0
                    _rewrite_slabs(d[name + "slabs"], d[name + "vals"], rows, hidden)
    return d


def _rewrite_slabs(buf, vals, rows, hidden):
    """vals [S, rows, hidden] into slabs stored in 32-row units [rows / 32][S][32][ld]; the rest stays as it is (NaN)."""
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


def _norm_stream(c, d):
    """The fp32 sum the kernel normalises (its rounding is res_out)."""
    dt, op = DT[c["dtype"]], c["op"]
    if op == "ln2":
        v = d["h"].float()
        for name in ("A", "B"):
            kind = c[name][0]
            if kind == "tensor":
                v = v + (d[name].float() + d[name + "bias"].float() if d[name + "bias"] is not None else d[name].float())
            elif kind == "slabs":
                v = v + _slab_sum(d[name + "vals"], d[name + "bias"])
            elif kind == "bias":
                v = v + d[name + "bias"].float()
        return v
    a = _slab_sum(d["slab_vals"], d["xbias"]).to(dt).float() if op.endswith("_partial") else d["x"].float()
    return a + d["res"].float() if d["res"] is not None else a


def _norm_ref(c, v, w, b):
    vd = v.double()
    mean_err = 0.0
    if c["op"].startswith("rms"):
        n = vd / torch.sqrt((vd * vd).mean(1, keepdim=True) + EPS)
    else:
        mu = vd.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((vd - mu) ** 2).mean(1, keepdim=True) + EPS)
        n = (vd - mu) * rstd
        mean_err = LN_MEAN * vd.abs().mean(1, keepdim=True) * rstd * w.double().abs()  # see LN_MEAN
    nw = n * w.double()
    ref = nw + b.double() if b is not None else nw
    dt = DT[c["dtype"]]
    tol = U[dt] * ref.abs() + 2.0 ** -16 * (nw.abs() + (b.double().abs() if b is not None else 0.0)) + mean_err + TINY[dt]
    return ref, tol


def _norm_call(c, d, rows=None):
    """One launch on fresh NaN-filled outputs [rows + 3, hidden]; returns (rc, {name: buffer})."""
    lib, dt = _lib(), DT[c["dtype"]]
    rows = c["rows"] if rows is None else rows
    hidden, op = c["hidden"], c["op"]
    out = {k: _nan((c["rows"] + 3, hidden), dt) for k in ("y", "res")}
    if op == "ln2" and c["y2"]:
        out["y2"] = _nan((c["rows"] + 3, hidden), dt)
    args = (rows, hidden, EPS, _code(dt), _stream())
    if op == "rms":
        r = lib.tgis_rmsnorm_residual(_p(d["x"]), _p(d["res"]), _p(d["w"]), _p(out["y"]), hidden, _p(out["res"]), *args)
    elif op == "ln":
        r = lib.tgis_layernorm_residual(_p(d["x"]), _p(d["res"]), _p(d["w"]), _p(d["b"] if c["bias"] else None),
                                        _p(out["y"]), _p(out["res"]), *args)
    elif op == "rms_partial":
        r = lib.tgis_rmsnorm_residual_partial(_p(d["slabs"]), c["S"], hidden + c["slab_pad"], _p(d["xbias"]), _p(d["res"]),
                                              _p(d["w"]), _p(out["y"]), hidden, _p(out["res"]), *args)
    elif op == "ln_partial":
        r = lib.tgis_layernorm_residual_partial(_p(d["slabs"]), c["S"], hidden + c["slab_pad"], _p(d["xbias"]),
                                                _p(d["res"]), _p(d["w"]), _p(d["b"] if c["bias"] else None), _p(out["y"]),
                                                _p(out["res"]), *args)
    else:
        ld = hidden + c["slab_pad"]
        r = lib.tgis_layernorm2_residual_partial(
            _p(d["h"]), _p(d["A"]), _p(d["Aslabs"]), c["SA"], ld, _p(d["Abias"]), _p(d["B"]), _p(d["Bslabs"]), c["SB"], ld,
            _p(d["Bbias"]), _p(d["w"]), _p(d["b"]), _p(d["w2"] if c["y2"] else None), _p(d["b2"] if c["y2"] else None),
            _p(out["y"]), _p(out.get("y2")), _p(out["res"]), *args)
    torch.cuda.synchronize()
    return r, out


def _norm_inputs_in_nan(c, d):
    """Row-major inputs as views into buffers with 3 NaN rows below them (the API has no input row stride)."""
    for k in ("x", "res", "h", "A", "B"):
        if d.get(k) is not None:
            d[k + "_buf"], d[k] = _in_nan(d[k], 3)


@pytest.mark.parametrize("c", rc.NORM_CASES, ids=[c["id"] for c in rc.NORM_CASES])
def test_norm(c):
    assert rc.case_form(c, _lib()) == tuple(c["form"])
    rows, hidden, dt = c["rows"], c["hidden"], DT[c["dtype"]]
    d = _norm_data(c, _gen(c["id"]))
    _norm_inputs_in_nan(c, d)
    v = _norm_stream(c, d)
    r, out = _norm_call(c, d)
    _ok(r, c["id"])
    for k, buf in out.items():
        _pad_nan(buf, rows, hidden, f"{c['id']} {k}")
    _exact(out["res"][:rows], v.to(dt), c["id"] + " res_out")
    is_ln = c["op"] != "rms" and c["op"] != "rms_partial"
    bias = d["b"] if (c["op"] == "ln2" or c.get("bias")) else None
    ys = [("y", d["w"], bias)] + ([("y2", d["w2"], d["b2"])] if "y2" in out else [])
    for name, w, b in ys:
        y = out[name][:rows]
        ref, tol = _norm_ref(c, v, w, b)
        _check(y, ref, tol, f"{c['id']} {name}")
        if _special_rows(c):
            want = b if b is not None else torch.zeros(hidden, dtype=dt, device=DEV)  # (values: 0 * -w is -0)
            assert torch.equal(y[0], want), f"{c['id']} {name}: zero row is not the bias"
            if is_ln:
                assert torch.equal(y[1], want), f"{c['id']} {name}: constant row is not the bias"
    for k in ("x", "res", "h", "A", "B"):
        if d.get(k + "_buf") is not None:
            assert torch.isnan(d[k + "_buf"][rows:]).all(), f"{c['id']}: input padding {k} written"
    r2, again = _norm_call(c, d)
    _ok(r2, c["id"])
    for k in out:
        assert _same(out[k], again[k]), f"{c['id']}: second call differs ({k})"


@pytest.mark.parametrize("kind", rc.NORM_KINDS)
def test_norm_zero_rows_and_refused_shapes(kind):
    c = next(x for x in rc.NORM_CASES if x["op"] == kind and x["rows"] == 64 and x["hidden"] == 2048)
    d = _norm_data(c, _gen(c["id"]))
    r, out = _norm_call(c, d, rows=0)
    _ok(r, f"{kind} rows = 0")
    assert all(torch.isnan(b).all() for b in out.values()), f"{kind}: rows = 0 wrote an output"
    big = dict(c, hidden=16392, rows=1, slab_pad=8)
    dbig = _norm_data(big, _gen(c["id"]))
    for hidden in (16392, 2052):
        r, out = _norm_call(dict(big, hidden=hidden), dbig, rows=1)
        assert r == EINVAL, f"{kind}: hidden {hidden} not refused ({r})"
        assert all(torch.isnan(b).all() for b in out.values())


# ---- rope + cache write, per token ------------------------------------------------------------------------------------------
def _rope_tables(rot, dt):
    import oracle.ops_ref as ops_ref

    if rot == 0:
        return None, None
    cos, sin = ops_ref.rope_tables(rot, 10000.0, MAX_POS, dt)
    return cos.to(DEV), sin.to(DEV)


def _unpack(kp, vp, Hkv, D):
    import oracle.ops_ref as ops_ref

    kpc, vpc = kp.cpu(), vp.cpu()
    Ks, Vs = zip(*(ops_ref.kv_page_unpack(kpc, vpc, pg, Hkv, D) for pg in range(kp.shape[0])))
    return torch.cat(Ks), torch.cat(Vs)  # [pages * 32, Hkv, D] by slot


def _rope_data(c, gen):
    T, H, Hkv, D, dt = c["T"], c["H"], c["Hkv"], c["D"], DT[c["dtype"]]
    N = (H + 2 * Hkv) * D
    d = dict(N=N, ld=N + 16)
    pos = torch.randint(0, MAX_POS, (T,), generator=gen, device=DEV, dtype=torch.int32)
    pos[0] = MAX_POS - 1  # the last row of the cos / sin tables
    d["pos"] = pos
    d["pages"] = -(-T // 32) + 2
    d["slots"] = torch.randperm(d["pages"] * 32, generator=gen, device=DEV)[:T].to(torch.int32) if Hkv else None
    d["cos"], d["sin"] = _rope_tables(c["rot"], dt)
    if c["S"]:
        S, sl = c["S"], N + c["slab_pad"]
        nb = -(-T // 32)
        d["slabs"] = torch.full((nb, S, 32, sl), float("nan"), device=DEV)
        d["vals"] = torch.randn((S, T, N), generator=gen, device=DEV) * (1.5 / S ** 0.5)
        _rewrite_slabs(d["slabs"], d["vals"], T, N)
        d["bias"] = (torch.randn(N, generator=gen, device=DEV) * 0.3).to(dt) if c["bias"] else None
        d["x"] = _slab_sum(d["vals"], d["bias"]).to(dt)
    else:
        d["x"] = (torch.randn((T, N), generator=gen, device=DEV) * 1.5).to(dt)
    return d


def _rope_call(c, d, T=None):
    """One launch on a fresh copy of the input (plain: in place) and NaN pools: (out buffer [T + 3, ld], k pool, v pool)."""
    lib, dt = _lib(), DT[c["dtype"]]
    T = c["T"] if T is None else T
    H, Hkv, D, N = c["H"], c["Hkv"], c["D"], d["N"]
    buf = _nan((c["T"] + 3, d["ld"]), dt)
    kp = vp = None
    if Hkv:
        kp, vp = _nan((d["pages"], Hkv, 32 * D), dt), _nan((d["pages"], Hkv, 32 * D), dt)
    tail = (_p(d["cos"]), _p(d["sin"]), _p(d["pos"]), _p(d["slots"]), _p(kp), _p(vp), T, H, Hkv, D, c["rot"], _code(dt),
            _stream())
    if c["S"]:
        r = lib.tgis_rope_kv_write_partial(_p(d["slabs"]), c["S"], N + c["slab_pad"], _p(d["bias"]), _p(buf), d["ld"],
                                           *tail)
    else:
        buf[:c["T"], :N] = d["x"]
        r = lib.tgis_rope_kv_write(_p(buf), d["ld"], *tail)
    torch.cuda.synchronize()
    return r, buf, kp, vp


def _rope_expect(c, d):
    """(ref, tol) fp64 of the whole [T, heads, D] output; tol 0 where the output must be an exact copy."""
    T, H, Hkv, D, rot = c["T"], c["H"], c["Hkv"], c["D"], c["rot"]
    dt = DT[c["dtype"]]
    x = d["x"].double().view(T, H + 2 * Hkv, D)
    ref, tol = x.clone(), torch.zeros_like(x)
    if rot:
        r = rot // 2
        cs = d["cos"].double()[d["pos"].long()][:, None, :]
        sn = d["sin"].double()[d["pos"].long()][:, None, :]
        x1, x2 = x[:, :H + Hkv, :r], x[:, :H + Hkv, r:rot]
        o1, o2 = x1 * cs - x2 * sn, x1 * sn + x2 * cs
        ref[:, :H + Hkv, :r], ref[:, :H + Hkv, r:rot] = o1, o2
        tol[:, :H + Hkv, :r] = U[dt] * o1.abs() + 2.0 ** -20 * ((x1 * cs).abs() + (x2 * sn).abs()) + TINY[dt]
        tol[:, :H + Hkv, r:rot] = U[dt] * o2.abs() + 2.0 ** -20 * ((x1 * sn).abs() + (x2 * cs).abs()) + TINY[dt]
    return ref, tol


@pytest.mark.parametrize("c", rc.ROPE_CASES, ids=[c["id"] for c in rc.ROPE_CASES])
def test_rope(c):
    assert rc.case_form(c, _lib()) == tuple(c["form"])
    T, H, Hkv, D, dt = c["T"], c["H"], c["Hkv"], c["D"], DT[c["dtype"]]
    d = _rope_data(c, _gen(c["id"]))
    N = d["N"]
    r, buf, kp, vp = _rope_call(c, d)
    _ok(r, c["id"])
    _pad_nan(buf, T, N, c["id"] + " qkv")
    out = buf[:T, :N].view(T, H + 2 * Hkv, D)
    ref, tol = _rope_expect(c, d)
    copy = tol == 0
    _exact(out[copy], d["x"].view(T, H + 2 * Hkv, D)[copy], c["id"] + " unrotated part")
    _check(out, ref, tol, c["id"])
    if Hkv:
        Kall, Vall = _unpack(kp, vp, Hkv, D)
        sl = d["slots"].long().cpu()
        oc = out.cpu()
        _exact(Kall[sl], oc[:, H:H + Hkv], c["id"] + " k cache")
        _exact(Vall[sl], oc[:, H + Hkv:], c["id"] + " v cache")
        free = torch.ones(d["pages"] * 32, dtype=torch.bool)
        free[sl] = False
        assert torch.isnan(Kall[free]).all() and torch.isnan(Vall[free]).all(), f"{c['id']}: a slot no token owns was written"
    if c["S"]:
        assert torch.isnan(d["slabs"].view(-1, 32, N + c["slab_pad"])[:, :, N:]).all()  # (slab padding stays NaN input)
    r2, buf2, kp2, vp2 = _rope_call(c, d)
    _ok(r2, c["id"])
    assert _same(buf, buf2) and (not Hkv or (_same(kp, kp2) and _same(vp, vp2))), f"{c['id']}: second call differs"


def test_rope_zero_tokens():
    for c in (rc.ROPE_CASES[0], next(x for x in rc.ROPE_CASES if x["S"])):
        d = _rope_data(c, _gen(c["id"]))
        r, buf, kp, vp = _rope_call(c, d, T=0)
        _ok(r, c["id"] + " T = 0")
        assert torch.isnan(kp).all() and torch.isnan(vp).all(), f"{c['id']}: T = 0 wrote the cache"
        if c["S"]:
            assert torch.isnan(buf).all(), f"{c['id']}: T = 0 wrote the output"
        else:
            assert _same(buf[:c["T"], :d["N"]], d["x"]), f"{c['id']}: T = 0 changed qkv"


# ---- rope + cache write, prefill --------------------------------------------------------------------------------------------
def _prefill_setup(c, gen):
    lens, H, Hkv, D, dt = c["lens"], c["H"], c["Hkv"], c["D"], DT[c["dtype"]]
    B, T, N = len(lens), sum(lens), (H + 2 * Hkv) * D
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=DEV)
    npg = [-(-n // 32) for n in lens]
    pages = sum(npg) + 3  # 3 pages no sequence owns
    max_pages = c["form"][0] + 1
    perm = torch.randperm(pages, generator=gen, device=DEV).tolist()
    spare = perm[sum(npg)]
    bt = torch.full((B, max_pages), spare, dtype=torch.int32)  # entries past a sequence's pages: a page nobody owns
    k = 0
    for b, n in enumerate(npg):
        bt[b, :n] = torch.tensor(perm[k:k + n], dtype=torch.int32)
        k += n
    pos = torch.cat([torch.arange(n, dtype=torch.int32) + (MAX_POS - n if b == 0 else 0) for b, n in enumerate(lens)])
    slots = torch.cat([bt[b, torch.arange(n) // 32] * 32 + torch.arange(n) % 32 for b, n in enumerate(lens)])
    x = (torch.randn((T, N), generator=gen, device=DEV) * 1.5).to(dt)
    cos, sin = _rope_tables(c["rot"], dt)
    return dict(B=B, T=T, N=N, ld=N + 16, cu=cu, bt=bt.to(DEV), pages=pages, pos=pos.to(DEV), slots=slots.to(torch.int32),
                x=x, cos=cos, sin=sin)


def _prefill_call(c, s, T=None):
    lib, dt = _lib(), DT[c["dtype"]]
    H, Hkv, D = c["H"], c["Hkv"], c["D"]
    buf = _nan((s["T"] + 3, s["ld"]), dt)
    buf[:s["T"], :s["N"]] = s["x"]
    kp, vp = _nan((s["pages"], Hkv, 32 * D), dt), _nan((s["pages"], Hkv, 32 * D), dt)
    r = lib.tgis_rope_kv_write_prefill(_p(buf), s["ld"], _p(s["cos"]), _p(s["sin"]), _p(s["pos"]), _p(s["cu"]),
                                       _p(s["bt"]), s["bt"].shape[1], _p(kp), _p(vp), s["B"], s["T"] if T is None else T,
                                       c["max_len"], H, Hkv, D, c["rot"], _code(dt), _stream())
    torch.cuda.synchronize()
    return r, buf, kp, vp


@pytest.mark.parametrize("c", rc.PREFILL_CASES, ids=[c["id"] for c in rc.PREFILL_CASES])
def test_rope_prefill(c):
    assert rc.case_form(c, _lib()) == tuple(c["form"])
    H, Hkv, D, dt = c["H"], c["Hkv"], c["D"], DT[c["dtype"]]
    s = _prefill_setup(c, _gen(c["id"]))
    T, N = s["T"], s["N"]
    r, buf, kp, vp = _prefill_call(c, s)
    _ok(r, c["id"])
    _pad_nan(buf, T, N, c["id"] + " qkv")
    # the per-token kernel over the same slots is the reference of q and of every owned slot
    tc = dict(op="rope", T=T, H=H, Hkv=Hkv, D=D, rot=c["rot"], dtype=c["dtype"], S=0)
    td = dict(N=N, ld=s["ld"], pos=s["pos"], pages=s["pages"], slots=s["slots"].to(DEV), cos=s["cos"], sin=s["sin"],
              x=s["x"])
    r1, tbuf, tk, tv = _rope_call(tc, td)
    _ok(r1, c["id"] + " per-token")
    _exact(buf[:T, :H * D], tbuf[:T, :H * D], c["id"] + " q vs the per-token kernel")
    _exact(buf[:T, H * D:N], s["x"][:, H * D:], c["id"] + " k / v input left alone")
    K, V = _unpack(kp, vp, Hkv, D)
    Kt, Vt = _unpack(tk, tv, Hkv, D)
    sl = s["slots"].long()
    _exact(K[sl], Kt[sl], c["id"] + " k slots vs the per-token kernel")
    _exact(V[sl], Vt[sl], c["id"] + " v slots vs the per-token kernel")
    tail = torch.zeros(s["pages"] * 32, dtype=torch.bool)
    bt = s["bt"].cpu()
    for b, n in enumerate(c["lens"]):
        if n % 32:
            last = int(bt[b, (n - 1) // 32])
            tail[last * 32 + n % 32:last * 32 + 32] = True
    assert (_bits(K[tail]) == 0).all() and (_bits(V[tail]) == 0).all(), f"{c['id']}: tail slots of a last page not +0"
    free = torch.ones(s["pages"] * 32, dtype=torch.bool)
    free[sl] = False
    free[tail] = False
    assert torch.isnan(K[free]).all() and torch.isnan(V[free]).all(), f"{c['id']}: a slot no sequence owns was written"
    r2, buf2, kp2, vp2 = _prefill_call(c, s)
    _ok(r2, c["id"])
    assert _same(buf, buf2) and _same(kp, kp2) and _same(vp, vp2), f"{c['id']}: second call differs"


def test_rope_prefill_zero_tokens():
    c = rc.PREFILL_CASES[0]
    s = _prefill_setup(c, _gen(c["id"]))
    r, buf, kp, vp = _prefill_call(c, s, T=0)
    _ok(r, "prefill T = 0")
    assert torch.isnan(kp).all() and torch.isnan(vp).all() and _same(buf[:s["T"], :s["N"]], s["x"])


# ---- argmax + logprob -------------------------------------------------------------------------------------------------------
def _argmax_data(c, gen):
    B, V, dt = c["B"], c["V"], DT[c["dtype"]]
    x = (torch.randn((B, V), generator=gen, device=DEV) * 2).clamp(-7, 7).to(dt)
    nseg = c["nseg"] if c["form"][1] else 2
    seg = -(-V // nseg)
    last0 = (nseg - 1) * seg
    want = []
    for b in range(B):
        kind = b % 4
        if kind == 0:
            at = [0, V - 1]  # first and last element of the row
        elif kind == 1:
            at = [seg - 1, seg]  # across a segment boundary
        elif kind == 2:
            at = [last0 + 1, V - 2] if V - 2 > last0 + 1 else [V - 2, V - 1]  # inside the short last segment
        else:
            at = [V - 1]
        x[b, at] = 8.0
        want.append(min(at))
    return x, torch.tensor(want, dtype=torch.int64)


def _argmax_call(c, x, scratch, B=None):
    lib = _lib()
    B_ = c["B"] if B is None else B
    ids = torch.full((c["B"] + 2,), -7, dtype=torch.int64, device=DEV)
    lp = _nan((c["B"] + 2,), torch.float32)
    f32 = x.dtype == torch.float32
    r = lib.tgis_argmax_logprob(_p(x), x.stride(0), B_, c["V"], int(f32), 0 if f32 else _code(x.dtype), _p(ids), _p(lp),
                                _p(scratch), scratch.numel() if scratch is not None else 0, _stream())
    torch.cuda.synchronize()
    return r, ids, lp


@pytest.mark.parametrize("c", rc.ARGMAX_CASES, ids=[c["id"] for c in rc.ARGMAX_CASES])
def test_argmax(c):
    assert rc.case_form(c, _lib()) == tuple(c["form"])
    B, V = c["B"], c["V"]
    x, want = _argmax_data(c, _gen(c["id"]))
    xbuf, xv = _in_nan(x, 2, c["ld_pad"])
    nbytes = rc.scratch_bytes(c)
    scratch = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV) if nbytes >= 0 else None
    r, ids, lp = _argmax_call(c, xv, scratch)
    _ok(r, c["id"])
    assert (ids[B:] == -7).all() and torch.isnan(lp[B:]).all(), f"{c['id']}: wrote past row B"
    assert torch.equal(ids[:B].cpu(), want), f"{c['id']}: ids {ids[:B].tolist()[:8]} want {want.tolist()[:8]}"
    xd = x.double()
    ref = -torch.log(torch.exp(xd - xd.max(1, keepdim=True).values).sum(1))
    _check(lp[:B], ref, 1e-5 * (1 + ref.abs()), c["id"] + " logprob")
    if scratch is not None and not c["form"][1]:
        assert (scratch == 0xFF).all(), f"{c['id']}: the one-block form wrote the scratch"
    _pad_nan(xbuf, B, V, c["id"] + " logits")
    r2, ids2, lp2 = _argmax_call(c, xv, scratch)
    assert torch.equal(ids, ids2) and _same(lp, lp2), f"{c['id']}: second call differs"


def test_argmax_zero_rows():
    c = rc.ARGMAX_CASES[0]
    x, _ = _argmax_data(c, _gen(c["id"]))
    r, ids, lp = _argmax_call(c, x, None, B=0)
    _ok(r, "argmax B = 0")
    assert (ids == -7).all() and torch.isnan(lp).all()


# ---- sampler: both kernels at the V threshold, and bit-identical to each other ----------------------------------------------
# every row set of test_sampler_gpu on both sides of V = 32768, except typical-p at 32768: with that test's seed for it, the
# fp32 oracle's sequential cumulative mass crosses 0.95 one element late (the fp64 mass passes it 4.4e-7 earlier, where the
# kernel cuts), a photo finish of the oracle rather than a property of either kernel
SAMPLER_THRESHOLD = [(V, name) for V in (32768, 32769) for name in ("all", "eos", "repetition", "temperature", "top_k", "top_p",
                                                                    "typical") if (V, name) != (32768, "typical")]


@pytest.mark.parametrize("V,name", SAMPLER_THRESHOLD)
def test_sampler_threshold(V, name):
    import test_sampler_gpu as ts
    from tgis_amd import native

    native.load_library()
    c = next(x for x in rc.CASES if x["op"] == "sampler" and x["V"] == V)
    assert rc.case_form(c, _lib()) == tuple(c["form"])
    ts.test_warped_scores_and_greedy_choice_match_oracle(native, torch.device(DEV), name, V)


SAMPLER_AB_V = (41, 32000, 32768)


def _sampler_ab_runs():
    """{V: (ids, logprob, lse, scores, rng after)} of fixed greedy + sampled rows (the rows of test_sampler_gpu's "all")."""
    import numpy as np
    import test_sampler_gpu as ts
    from tgis_amd import native

    native.load_library()
    out = {}
    for V in SAMPLER_AB_V:
        rows = ts.ROWSETS["all"] + [dict(r, sample=1) for r in ts.ROWSETS["all"]]
        rs = np.random.RandomState(V)
        logits = (rs.randn(len(rows), V) * 3).astype(np.float32)
        ids = rs.randint(0, V, size=(len(rows), 37)).astype(np.int64)
        rng = torch.tensor([[1000 + b, 5] for b in range(len(rows))], dtype=torch.int64, device=DEV)
        res = ts._run(native, torch.device(DEV), logits, rows, ids, exclude_id=3, eos_id=7 % V, rng=rng)
        torch.cuda.synchronize()
        out[V] = [t.cpu() for t in res] + [rng.cpu()]
    return out


def _sampler_child(path):
    for V in SAMPLER_AB_V:
        assert rc.query(_lib(), "sampler", V)[0] == 0, "TGIS_SAMPLER_GLOBAL_ROWS did not select the global-row kernel"
    torch.save(_sampler_ab_runs(), path)
    print("ok", flush=True)


def test_sampler_global_rows_bit_identical(tmp_path):
    for V in SAMPLER_AB_V:
        assert rc.query(_lib(), "sampler", V)[0] == 1
    mine = _sampler_ab_runs()
    path = str(tmp_path / "global_rows.pt")
    env = dict(os.environ, TGIS_SAMPLER_GLOBAL_ROWS="1")
    here = os.path.dirname(os.path.abspath(__file__))
    paths = [here, os.path.dirname(here), os.path.join(os.path.dirname(here), "text-generation-inference_amd")]
    code = f"import sys; sys.path[:0] = {paths!r}; import test_rowwise_edges_gpu as t; t._sampler_child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "ok" in r.stdout, f"child: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    theirs = torch.load(path)
    for V in SAMPLER_AB_V:
        for what, a, b in zip(("ids", "logprob", "lse", "scores", "rng"), mine[V], theirs[V]):
            assert _same(a, b), f"V={V}: {what} of the global-row kernel differs from the register kernel"


# ---- act_mul, gelu, embedding, decode_slots ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("T,I", rc.ACT_MUL)
def test_act_mul(T, I, dtype):
    dt, lib = DT[dtype], _lib()
    gen = _gen(f"act{T}-{I}-{dtype}")
    g = (torch.randn((T, I), generator=gen, device=DEV) * 3).clamp(-10, 10)
    u = torch.randn((T, I), generator=gen, device=DEV) * 2
    gbuf, gu = _in_nan(torch.cat([g, u], 1).to(dt), 3)
    obuf = _nan((T + 3, I), dt)

    def call(t):
        r = lib.tgis_act_mul(_p(gu), _p(obuf), t, I, 1, _code(dt), _stream())
        torch.cuda.synchronize()
        return r

    _ok(call(T), "act_mul")
    assert torch.isnan(obuf[T:]).all() and torch.isnan(gbuf[T:]).all()
    gd, ud = gu[:, :I].double(), gu[:, I:].double()
    sl = (gd / (1 + torch.exp(-gd))).to(dt).double()
    ref = (sl * ud).to(dt).double()
    _check(obuf[:T], ref, 2 * U[dt] * ref.abs() + 2.0 ** -20 * (gd * ud).abs() + TINY[dt], f"act_mul {T}x{I}")
    first = obuf.clone()
    _ok(call(T), "act_mul")
    assert _same(first, obuf), "act_mul: second call differs"
    obuf.fill_(float("nan"))
    _ok(call(0), "act_mul T = 0")
    assert torch.isnan(obuf).all()


@pytest.mark.parametrize("tanh", [False, True])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("n", rc.GELU_N)
def test_gelu(n, dtype, tanh):
    dt, lib = DT[dtype], _lib()
    gen = _gen(f"gelu{n}-{dtype}")
    x = (torch.randn(n, generator=gen, device=DEV) * 3).clamp(-10, 10)
    x[:8] = torch.tensor([0.0, -0.0, 10.0, -10.0, 1e-3, -1e-3, 5.5, -5.5])
    if dt == torch.bfloat16 and n >= 16:
        x[8:16] = torch.tensor([100.0, -100.0, 99.0, -99.0, 100.0, -100.0, 64.0, -64.0])
    xbuf = _nan((n + 64,), dt)
    xbuf[:n] = x.to(dt)
    obuf = _nan((n + 64,), dt)

    def call(m):
        r = lib.tgis_gelu(_p(xbuf), _p(obuf), m, int(tanh), _code(dt), _stream())
        torch.cuda.synchronize()
        return r

    _ok(call(n), "gelu")
    assert torch.isnan(obuf[n:]).all()
    xd = xbuf[:n].double()
    if tanh:
        ref = 0.5 * xd * (1 + torch.tanh((2 / torch.pi) ** 0.5 * (xd + 0.044715 * xd ** 3)))
    else:
        ref = 0.5 * xd * (1 + torch.erf(xd / 2 ** 0.5))
    _check(obuf[:n], ref, U[dt] * ref.abs() + 2.0 ** -20 * xd.abs() + TINY[dt], f"gelu n={n} tanh={tanh}")
    first = obuf.clone()
    _ok(call(n), "gelu")
    assert _same(first, obuf)
    obuf.fill_(float("nan"))
    _ok(call(0), "gelu n = 0")
    assert torch.isnan(obuf).all()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("E,with_pos", rc.EMBED)
def test_embedding_shard(E, with_pos, dtype):
    """A tensor-parallel vocab shard: rows 200..299 of the vocab; ids outside it give zeros (before the position rows)."""
    dt, lib = DT[dtype], _lib()
    gen = _gen(f"emb{E}-{with_pos}-{dtype}")
    rows, off = 100, 200
    table = (torch.randn((rows, E), generator=gen, device=DEV)).to(dt)
    ids = torch.tensor([199, 200, 299, 300, -1, 250, 0, 1000, -200, 201], dtype=torch.int64, device=DEV)
    T = ids.numel()
    pos = torch.tensor([0, 31, 32, 63, 64, 2047, 5, 1, 2046, 33], dtype=torch.int32, device=DEV)
    ptab = (torch.randn((2048, E), generator=gen, device=DEV)).to(dt) if with_pos else None
    obuf = _nan((T + 3, E), dt)

    def call(t):
        r = lib.tgis_embedding(_p(ids), _p(table), _p(pos) if with_pos else None, _p(ptab), _p(obuf), t, E, rows, off,
                               _code(dt), _stream())
        torch.cuda.synchronize()
        return r

    _ok(call(T), "embedding")
    assert torch.isnan(obuf[T:]).all()
    local = ids - off
    valid = (local >= 0) & (local < rows)
    want = torch.zeros((T, E), dtype=dt, device=DEV)
    want[valid] = table[local[valid]]
    if with_pos:
        want = (want.float() + ptab[pos.long()].float()).to(dt)
    _exact(obuf[:T], want, f"embedding E={E}")
    first = obuf.clone()
    _ok(call(T), "embedding")
    assert _same(first, obuf)
    obuf.fill_(float("nan"))
    _ok(call(0), "embedding T = 0")
    assert torch.isnan(obuf).all()


@pytest.mark.parametrize("B", rc.DECODE_SLOTS_B)
def test_decode_slots(B):
    lib = _lib()
    gen = _gen(f"slots{B}")
    edges = torch.tensor([31, 32, 0, 63, 64, 95, 96, 1], dtype=torch.int32, device=DEV)
    pos = torch.randint(0, 8 * 32, (B,), generator=gen, device=DEV, dtype=torch.int32)
    pos[:min(B, 8)] = edges[:min(B, 8)]
    bt = torch.randperm(B * 9, generator=gen, device=DEV).to(torch.int32).view(B, 9)
    slots = torch.full((B + 3,), -7, dtype=torch.int32, device=DEV)
    ctx = torch.full((B + 3,), -7, dtype=torch.int32, device=DEV)

    def call(b):
        r = lib.tgis_decode_slots(_p(pos), _p(bt), 9, _p(slots), _p(ctx), b, _stream())
        torch.cuda.synchronize()
        return r

    _ok(call(B), "decode_slots")
    pl = pos.long()
    want = bt.long()[torch.arange(B, device=DEV), pl // 32] * 32 + pl % 32
    assert torch.equal(slots[:B].long(), want) and torch.equal(ctx[:B].long(), pl + 1)
    assert (slots[B:] == -7).all() and (ctx[B:] == -7).all()
    slots.fill_(-7)
    ctx.fill_(-7)
    _ok(call(0), "decode_slots B = 0")
    assert (slots == -7).all() and (ctx == -7).all()
