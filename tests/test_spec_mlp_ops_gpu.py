"""-m gpu: the kernels of the MLP speculator (csrc/spec_mlp.hip) against tests/spec_mlp_ref.py in fp64, f16 and bf16.

Every output is a view into a NaN-filled buffer whose extra rows must stay NaN; inputs are padded with NaN rows, so an
over-read shows up in the output.  Bounds (U the unit roundoff of the model dtype, TINY its smallest subnormal, both from
tests/test_rowwise_edges_gpu.py):
  - tgis_spec_mlp_input: bit-equal rows; with scale_input  U |ref| + 2^-16 |ref| + TINY;
  - tgis_spec_mlp_state, u = n w + b:  U |ref| + 1.13 * 2^-16 (|n w| + |b|) + 2^-21 |u| + TINY.  2^-16 (|n w| + |b|) is the
    RMS norms' bound on u; 1.13 is the largest slope of GELU (at u = sqrt(2)), so it carries that bound through; erff errs
    by a few fp32 ulps of erf, which is all of 1 + erf where the two cancel (u << 0): 2^-21 |u|;
  - tgis_spec_mlp_drafts: exact.
The state kernel takes the norms' plan (choose_norm): 512 threads per row for rows <= 64 and I >= 2048, else 256, and
8 NT columns per pass.  STATE_SHAPES has both sides of each: I 2040 | 2048, rows 64 | 65, one pass | two (4096 | 4104 at
512 threads, 2048 | 2056 at 256), and the 16384 the registers hold."""
import zlib

import numpy as np
import pytest
import torch

from tests import spec_mlp_ref as ref

pytestmark = pytest.mark.gpu

U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}
DTYPES = [torch.float16, torch.bfloat16]
DEV = "cuda:0"
EINVAL = -1
V = 11

STATE_SHAPES = [(rows, I) for I in (8, 72, 1024, 2040, 2048, 4096, 4104) for rows in (1, 3, 16, 64)] + [
    (65, 2048), (65, 2056), (2, 16384)]
WORST = {}  # dtype -> (err / tol, case) over the state cases that ran


def _native():
    from tgis_amd import native

    return native


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def _in_nan(data, pad=3):
    buf = _nan((data.shape[0] + pad,) + tuple(data.shape[1:]), data.dtype)
    buf[:data.shape[0]] = data
    return buf, buf[:data.shape[0]]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _f64(t):
    return t.double().cpu().numpy()


def _gen(*key):
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


def _within(got, want, tol, what):
    got = _f64(got)
    assert not np.isnan(got).any(), f"{what}: NaN in the output"
    ratio = np.abs(got - want) / tol
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: err / tol = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


# ---- tgis_spec_mlp_input --------------------------------------------------------------------------------------------------------
def _n_emit(B, K1):
    vals = [1, K1, 0, -5, K1 + 3, 1000, max(1, K1 // 2)]
    return [vals[b % len(vals)] for b in range(B)]


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("K1", [1, 4, 8])
@pytest.mark.parametrize("E", [8, 72, 2056, 4096])
def test_input_selects_rows_bit_for_bit(gpu_device, dt, K1, E):
    native = _native()
    B = 9
    hidden = torch.randn((B * K1, E), generator=_gen("in", K1, E)).to(dt).to(DEV)
    hbuf, h = _in_nan(hidden)
    n_emit = _n_emit(B, K1)
    want = torch.stack([hidden[b * K1 + min(max(n, 1), K1) - 1] for b, n in enumerate(n_emit)])
    obuf, cbuf = _nan((B + 3, E), dt), _nan((B + 3, E), dt)
    native.spec_mlp_input(h, torch.tensor(n_emit, dtype=torch.int32, device=DEV), K1, obuf[:B], cbuf[:B])
    assert torch.equal(_bits(obuf[:B]), _bits(want)), "row selection"
    assert torch.equal(_bits(cbuf[:B]), _bits(obuf[:B])), "out_copy != out"
    assert torch.isnan(obuf[B:]).all() and torch.isnan(cbuf[B:]).all(), "guard rows written"
    # n_emit NULL: row b K1; out_copy NULL: skipped
    obuf.fill_(float("nan"))
    native.spec_mlp_input(h, None, K1, obuf[:B])
    assert torch.equal(_bits(obuf[:B]), _bits(hidden[::K1])) and torch.isnan(obuf[B:]).all()


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("K1,E", [(1, 8), (4, 72), (1, 2056), (8, 4096)])
def test_input_scales_within_the_norm_bound(gpu_device, dt, K1, E):
    native = _native()
    B = 5
    hidden = (torch.randn((B * K1, E), generator=_gen("sc", K1, E)) * 3.0).to(dt)
    hidden[0] = 0  # an all-zero state stays zero (and finite)
    hbuf, h = _in_nan(hidden.to(DEV))
    n_emit = _n_emit(B, K1)
    n_emit[0] = 1
    rows = [b * K1 + min(max(n, 1), K1) - 1 for b, n in enumerate(n_emit)]
    want = ref.scale_input(_f64(hidden)[rows])
    obuf, cbuf = _nan((B + 3, E), dt), _nan((B + 3, E), dt)
    native.spec_mlp_input(h, torch.tensor(n_emit, dtype=torch.int32, device=DEV), K1, obuf[:B], cbuf[:B], scale_input=True,
                          eps=ref.EPS)
    tol = U[dt] * np.abs(want) + 2.0 ** -16 * np.abs(want) + TINY[dt]
    _within(obuf[:B], want, tol, "scale_input")
    assert torch.equal(_bits(cbuf[:B]), _bits(obuf[:B])) and torch.isnan(obuf[B:]).all() and torch.isnan(cbuf[B:]).all()
    assert (obuf[0] == 0).all()


# ---- tgis_spec_mlp_state --------------------------------------------------------------------------------------------------------
def _state_case(rows, I, dt):
    g = _gen("state", rows, I)
    alpha = ref.constants(3, I)[2]
    proj = torch.randn((rows, I), generator=g).to(dt)
    emb = torch.randn((V, I), generator=g).to(dt)
    w = (1.0 + 0.2 * torch.randn(I, generator=g)).to(dt)
    b = (0.3 * torch.randn(I, generator=g)).to(dt)
    tok = torch.randint(0, V, (rows,), generator=g)
    tok[0] = 0
    tok[-1] = V - 1
    if rows >= 3:
        tok[1] = V + 5   # out of range: clamped to V - 1
        tok[2] = -3      # clamped to 0
    return proj, emb, w, b, tok, alpha


def _run_state(proj, emb, w, b, tok, alpha, dt, what):
    native = _native()
    rows, I = proj.shape
    pbuf, p = _in_nan(proj.to(DEV))
    ebuf, e = _in_nan(emb.to(DEV))  # rows past V are NaN: an id that is not clamped shows
    xbuf = _nan((rows + 3, I), dt)
    native.spec_mlp_state(p, tok.to(DEV), e, w.to(DEV), b.to(DEV), alpha, xbuf[:rows], eps=ref.EPS)
    want, nw, u = ref.state(_f64(proj), tok.numpy(), _f64(emb), _f64(w), _f64(b), alpha)
    tol = (U[dt] * np.abs(want) + 1.13 * 2.0 ** -16 * (np.abs(nw) + np.abs(_f64(b))) + 2.0 ** -21 * np.abs(u) + TINY[dt])
    worst = _within(xbuf[:rows], want, tol, what)
    assert torch.isnan(xbuf[rows:]).all(), f"{what}: guard rows written"
    if worst > WORST.get(dt, (0.0, ""))[0]:
        WORST[dt] = (worst, what)
    return xbuf[:rows]


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("rows,I", STATE_SHAPES, ids=[f"{r}x{i}" for r, i in STATE_SHAPES])
def test_state_matches_fp64(gpu_device, dt, rows, I):
    proj, emb, w, b, tok, alpha = _state_case(rows, I, dt)
    _run_state(proj, emb, w, b, tok, alpha, dt, f"state {rows}x{I}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("I", [8, 72, 4096, 4104])
def test_state_zero_and_huge_rows(gpu_device, dt, I):
    """Row 0: proj_out and the embedding row all zero (s = 0: rstd = 1 / sqrt(eps), x = gelu(bias), finite).  Row 1: +-60000,
    whose squares overflow f16 and must be summed in fp32.  Row 2: an ordinary one."""
    proj, emb, w, b, tok, alpha = _state_case(3, I, dt)
    emb[0] = 0
    proj[0] = 0
    tok[0] = 0
    sign = torch.where(torch.arange(I) % 3 == 0, -1.0, 1.0)
    proj[1] = (60000.0 * sign).to(dt)
    x = _run_state(proj, emb, w, b, tok, alpha, dt, f"state special rows I={I}")
    assert torch.isfinite(x.float()).all()
    assert np.allclose(_f64(x[0]), ref.gelu(_f64(b)), rtol=2 * U[dt], atol=1e-6)


def test_the_worst_state_error_is_reported(gpu_device):
    """(Runs behind the cases above in file order; DESIGN.md §6 records the figure.)"""
    for dt, (worst, what) in WORST.items():
        print(f"\n[spec mlp state] {dt}: worst err / tol = {worst:.3f} ({what})")
        assert worst <= 1.0


# ---- tgis_spec_mlp_drafts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_drafts_transposes_and_sets_hits(gpu_device, K, B):
    native = _native()
    toks = torch.randint(0, 2 ** 40, (K, B), generator=_gen("d", K, B), dtype=torch.int64).to(DEV)
    drafts = torch.full((B + 2, K), -7, dtype=torch.int64, device=DEV)
    hits = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    copy = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    native.spec_mlp_drafts(toks, drafts[:B], hits[:B], copy[:B])
    assert torch.equal(drafts[:B], toks.t()) and (drafts[B:] == -7).all()
    assert (hits[:B] == 1).all() and (copy[:B] == 1).all() and (hits[B:] == -7).all() and (copy[B:] == -7).all()
    hits.fill_(-7)
    native.spec_mlp_drafts(toks, drafts[:B], hits[:B])  # hits_copy NULL: skipped
    assert (hits[:B] == 1).all() and (hits[B:] == -7).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_bad_sizes_are_refused_and_empty_batches_are_ok(gpu_device):
    native = _native()
    lib, st = native.load_library(), native._stream()
    t = torch.zeros(64, dtype=torch.float16, device=DEV)
    out = _nan((4, 16), torch.float16)
    ids = torch.zeros(8, dtype=torch.int64, device=DEV)
    hits = torch.zeros(8, dtype=torch.int32, device=DEV)
    p = (lambda x: x.data_ptr())
    assert lib.tgis_spec_mlp_input(p(t), None, 1, p(out), None, 2, 12, 0, 1e-6, 0, st) == EINVAL
    assert b"emb_dim (12) must be a multiple of 8" in lib.tgis_last_error()
    assert lib.tgis_spec_mlp_input(p(t), None, 9, p(out), None, 2, 16, 0, 1e-6, 0, st) == EINVAL
    assert lib.tgis_spec_mlp_state(p(t), p(ids), p(t), 4, p(t), p(t), 1.0, 1e-6, p(out), 2, 12, 0, st) == EINVAL
    assert b"inner_dim (12) must be a multiple of 8" in lib.tgis_last_error()
    assert lib.tgis_spec_mlp_state(p(t), p(ids), p(t), 4, p(t), p(t), 1.0, 1e-6, p(out), 2, 16392, 0, st) == EINVAL
    assert lib.tgis_spec_mlp_state(p(t), p(ids), p(t), 4, p(t), p(t), 1.0, 1e-6, p(out), 2, 16, 7, st) == EINVAL
    assert lib.tgis_spec_mlp_drafts(p(ids), 8, p(ids), p(hits), None, 1, st) == EINVAL
    assert lib.tgis_spec_mlp_drafts(p(ids), 0, p(ids), p(hits), None, 1, st) == EINVAL
    lib.tgis_clear_error()
    # B = 0: TGIS_OK, nothing written
    assert lib.tgis_spec_mlp_input(p(t), None, 1, p(out), None, 0, 16, 1, 1e-6, 0, st) == 0
    assert lib.tgis_spec_mlp_state(p(t), p(ids), p(t), 4, p(t), p(t), 1.0, 1e-6, p(out), 0, 16, 0, st) == 0
    assert lib.tgis_spec_mlp_drafts(p(ids), 3, p(ids), p(hits), None, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and (hits == 0).all()
