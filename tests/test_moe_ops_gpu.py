"""-m gpu: the routed-expert kernels (csrc/moe.hip: tgis_moe_route, tgis_moe_gemm_up, tgis_moe_gemm_down) against the fp64
restatement of tests/moe_ref.py.

Route: ids and lists exactly, weights within 4 ulp of fp32, ties to the lower index.  Up and down: hidden 320 (5 k64-steps:
the four k-parts get 2, 2, 1 and 0 of them), I 80 and 528 (N tails, one and many tiles, a K tail inside a k64-step for the
down GEMM), f16 and bf16, every row count around the 32-row slab, and routing patterns forced through hand-written logits.
The images of experts nobody chose are filled with NaN: a block that read them would show.

Per-element bounds are derived as tests/test_gemm_edges_gpu.py derives them (restated here): fp32 accumulation costs
B_ACC K 2^-24 per unit of |x| @ |W|, an output rounding A_OUT unit roundoffs of |ref|; the SiLU * up epilogue propagates the
two sums' errors through T(T(silu(T g)) * T up)."""
import ctypes

import pytest
import torch

from tests import moe_cases as mc
from tests import moe_ref

pytestmark = pytest.mark.gpu

A_OUT = 2.0  # unit roundoffs of the output per |ref|
B_ACC = 2.0  # fp32 accumulation: K 2^-24 per unit of |x| @ |W|
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}
DTYPES = (torch.float16, torch.bfloat16)
E, TOP_K, HIDDEN = mc.E, mc.TOP_K, mc.HIDDEN


# ---- routing ----------------------------------------------------------------------------------------------------------------
def _check_routing(logits_cpu, r, E, top_k):
    ids, w = moe_ref.route(logits_cpu, top_k)
    counts, offsets, slot_rows = moe_ref.lists(ids, E)
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    assert torch.equal(r.counts.cpu().long(), counts) and torch.equal(r.offsets.cpu().long(), offsets)
    assert torch.equal(r.slot_rows.cpu().long(), slot_rows)
    got = r.expert_w.cpu()
    wf = w.float()
    ulp = (torch.nextafter(wf, torch.full_like(wf, 2.0)) - wf).double()
    err = (got.double() - w).abs()
    assert (err <= 4 * ulp).all(), f"routing weight off by {float((err / ulp).max()):.2f} ulp"
    assert torch.allclose(got.sum(dim=1), torch.ones(got.shape[0]), atol=1e-6, rtol=0)


@pytest.mark.parametrize("E_,top_k", mc.ROUTE_CASES, ids=lambda v: str(v))
def test_route_matches_the_restatement(gpu_device, E_, top_k):
    from tgis_amd import native

    g = torch.Generator().manual_seed(100 * E_ + top_k)
    for T in mc.ROUTE_TOKENS:
        logits = torch.randn(T, E_, generator=g) * 2.0
        r = native.moe_route(logits.to(gpu_device), top_k)
        _check_routing(logits, r, E_, top_k)
        again = native.moe_route(logits.to(gpu_device), top_k)
        for name in ("expert_ids", "expert_w", "lists", "slot_rows"):
            assert torch.equal(getattr(r, name), getattr(again, name)), name


def test_route_reads_a_strided_logit_matrix_and_serves_no_tokens(gpu_device):
    from tgis_amd import native

    g = torch.Generator().manual_seed(9)
    wide = torch.randn(33, 16, generator=g)
    r = native.moe_route(wide.to(gpu_device)[:, :8], 2)  # row stride 16
    _check_routing(wide[:, :8], r, 8, 2)
    r = native.moe_route(torch.empty((0, 8), dtype=torch.float32, device=gpu_device), 2)
    assert r.counts.tolist() == [0] * 8 and r.offsets.tolist() == [0] * 9


def test_route_ties_go_to_the_lower_index(gpu_device):
    from tgis_amd import native

    logits = torch.tensor([[1.0, 3.0, 3.0, 3.0, 0.0, 3.0, -1.0, 2.0],
                           [0.0] * 8,
                           [5.0, 1.0, 5.0, 2.0, 5.0, 0.0, 0.0, 0.0],
                           [-2.0, -2.0, -2.0, -2.0, -2.0, -2.0, -2.0, 7.0]])
    r = native.moe_route(logits.to(gpu_device), 2)
    assert r.expert_ids.tolist() == [[1, 2], [0, 1], [0, 2], [7, 0]]
    assert r.expert_w[:3].tolist() == [[0.5, 0.5]] * 3
    _check_routing(logits, r, 8, 2)


# ---- expert GEMMs -----------------------------------------------------------------------------------------------------------
_WEIGHTS = {}


def _weights(I, dt, dev):
    """(w1, w3, w2 on the CPU in dt, gate|up images, down images) of 8 experts, made once per (I, dtype)."""
    key = (I, dt)
    if key not in _WEIGHTS:
        from tgis_amd import native

        g = torch.Generator().manual_seed(1000 + I)
        w1 = (torch.randn(E, I, HIDDEN, generator=g) * HIDDEN ** -0.5).to(dt)
        w3 = (torch.randn(E, I, HIDDEN, generator=g) * HIDDEN ** -0.5).to(dt)
        w2 = (torch.randn(E, HIDDEN, I, generator=g) * I ** -0.5).to(dt)
        up = native.MoeWeights(lambda e: torch.cat([w1[e], w3[e]]).to(dev), E, gate_up=True)
        down = native.MoeWeights(lambda e: w2[e].to(dev), E)
        _WEIGHTS[key] = (w1, w3, w2, up, down)
    return _WEIGHTS[key]


def _poisoned(mw, chosen):
    """A copy of the images with NaN in every expert outside `chosen`."""
    from tgis_amd import native

    twin = native.MoeWeights.__new__(native.MoeWeights)
    twin.__dict__.update(mw.__dict__)
    twin.image = mw.image.clone()
    for e in range(E):
        if e not in chosen:
            twin.image[e].view(mw.dtype).fill_(float("nan"))
    return twin


def _logits_for(ids):
    """Hand-written router logits whose top-2 are ids[t] = (first, second): 4 and 3 there, noise in [-1, 0) elsewhere."""
    T = ids.shape[0]
    g = torch.Generator().manual_seed(T)
    logits = -torch.rand(T, E, generator=g)
    logits.scatter_(1, ids[:, :1], 4.0)
    logits.scatter_(1, ids[:, 1:], 3.0)
    return logits


def _pattern(name, T):
    """Expert ids [T, 2] of a routing pattern, or None where T cannot hold it."""
    g = torch.Generator().manual_seed(T + len(name))
    if name == "uniform":
        return torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(T)])
    if name == "same_two":  # lists of T rows for experts 2 and 5 (longer than one and two slabs at T 33 / 65); six experts idle
        return torch.tensor([[5, 2]]).repeat(T, 1)
    if name == "exactly_32":  # expert 3 holds exactly 32 rows, the others share the rest
        if T < 32:
            return None
        others = [e for e in range(E) if e != 3]
        ids = torch.tensor([[others[t % 7], others[(t + 3) % 7]] for t in range(T)])
        ids[:32, 1] = 3
        return ids
    if name == "last_token_alone":  # expert 7 holds only the last token
        ids = torch.tensor([[t % 3, 3 + t % 4] for t in range(T)])
        ids[T - 1, 0] = 7
        return ids
    raise KeyError(name)


PATTERNS = ("uniform", "same_two", "exactly_32", "last_token_alone")


def _x(T, dt, gen):
    return ((torch.randn(T, HIDDEN, generator=gen) * 0.5 + 0.25)).to(dt)


def _up_reference(x, w1, w3, ids, dt):
    u = U[dt]
    g, up = moe_ref.expert_up(x, w1, w3, ids, absolute=True)
    ag, au = moe_ref.expert_up(x.double().abs(), w1.double().abs(), w3.double().abs(), ids, absolute=True)
    eg, eu = B_ACC * HIDDEN * 2.0 ** -24 * ag, B_ACC * HIDDEN * 2.0 ** -24 * au
    rnd = lambda t: t.to(dt).double()  # noqa: E731
    gr, ur = rnd(g), rnd(up)
    sl = rnd(moe_ref.silu(gr))
    ref = rnd(sl * ur)
    dg = 2 * (eg + u * g.abs()) + TINY[dt]
    du = 2 * (eu + u * up.abs()) + TINY[dt]
    tol = A_OUT * u * ref.abs() + ur.abs() * (1.1 * dg + 2 * u * sl.abs()) + (sl.abs() + 1.1 * dg) * du + TINY[dt]
    return ref, tol


def _down_reference(h, w2, ids, w):
    """(y, tol) [T, top_k, hidden] of the scaled fp32 rows, from the h the kernel was given."""
    K = h.shape[1]
    y0 = moe_ref.expert_down(h, w2, ids)
    a0 = moe_ref.expert_down(h.double().abs(), w2.double().abs(), ids)
    wd = w.double().reshape(ids.shape[0], ids.shape[1], 1)
    u32 = U[torch.float32]
    tol = (B_ACC * K * 2.0 ** -24 * a0 + A_OUT * u32 * y0.abs()) * wd + u32 * (y0 * wd).abs() + TINY[torch.float32]
    return y0 * wd, tol


def _close(got, ref, tol, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > tol
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {i}: got "
                             f"{got[i].item():.6g} ref {ref[i].item():.6g} tol {tol[i].item():.3g}")


def _slab_rows(p, T):
    """[T, top_k, N] view of a decode-form Partial's slabs."""
    s = p.slabs.view(-1, p.S, 32, p.ld)
    return s.permute(0, 2, 1, 3).reshape(-1, p.S, p.ld)[:T, :, :p.N]


def _run_case(dev, I, dt, T, pattern):
    from tgis_amd import native

    ids = _pattern(pattern, T)
    if ids is None:
        return False
    w1, w3, w2, up_w, down_w = _weights(I, dt, dev)
    chosen = set(ids.reshape(-1).tolist())
    up_w, down_w = _poisoned(up_w, chosen), _poisoned(down_w, chosen)
    gen = torch.Generator().manual_seed(T * 7 + I)
    x = _x(T, dt, gen)
    logits = _logits_for(ids)
    r = native.moe_route(logits.to(dev), TOP_K)
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    what = f"I {I} {dt} T {T} {pattern}"

    h = native.moe_gemm_up(x.to(dev), up_w, r)
    ref, tol = _up_reference(x, w1, w3, ids, dt)
    _close(h, ref, tol, what + " up")

    p = native.moe_gemm_down(h, down_w, r, partial=True)
    assert p.S == TOP_K and p.shape == (T, HIDDEN) and p.ld == HIDDEN
    yref, ytol = _down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    _close(_slab_rows(p, T), yref, ytol, what + " down slabs")

    out = native.moe_gemm_down(h, down_w, r, partial=False)
    total = yref.sum(dim=1)
    ftol = ytol.sum(dim=1) + U[torch.float32] * yref.abs().sum(dim=1) + A_OUT * U[dt] * total.abs() + TINY[dt]
    _close(out, total.to(dt).double(), ftol, what + " down finished")
    # the deferred sum and the finished one are the same fp32 additions in the same order
    rows = _slab_rows(p, T)
    assert torch.equal((rows[:, 0] + rows[:, 1]).to(dt), out), what

    # two runs, the same bytes
    h2 = native.moe_gemm_up(x.to(dev), up_w, r)
    p2 = native.moe_gemm_down(h2, down_w, r, partial=True)
    assert torch.equal(h, h2) and torch.equal(_slab_rows(p, T), _slab_rows(p2, T)), what
    return True


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("I", mc.INTERMEDIATES)
@pytest.mark.parametrize("T", mc.TOKENS)
def test_up_and_down_under_every_pattern(gpu_device, I, dt, T):
    ran = [name for name in PATTERNS if _run_case(gpu_device, I, dt, T, name)]
    assert len(ran) >= 3


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("T", mc.FINISHED_TOKENS)
def test_finished_form_at_many_rows(gpu_device, dt, T):
    """T 130 and 700 (past PARTIAL_MAX_M): the finished form alone, uniform routing and one list of every token."""
    from tgis_amd import native

    I = mc.INTERMEDIATES[1]
    w1, w3, w2, up_w, down_w = _weights(I, dt, gpu_device)
    for pattern in ("uniform", "same_two"):
        ids = _pattern(pattern, T)
        gen = torch.Generator().manual_seed(T)
        x = _x(T, dt, gen)
        r = native.moe_route(_logits_for(ids).to(gpu_device), TOP_K)
        h = native.moe_gemm_up(x.to(gpu_device), up_w, r)
        ref, tol = _up_reference(x, w1, w3, ids, dt)
        _close(h, ref, tol, f"{dt} T {T} {pattern} up")
        out = native.moe_gemm_down(h, down_w, r, partial=False)
        yref, ytol = _down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
        total = yref.sum(dim=1)
        ftol = ytol.sum(dim=1) + U[torch.float32] * yref.abs().sum(dim=1) + A_OUT * U[dt] * total.abs() + TINY[dt]
        _close(out, total.to(dt).double(), ftol, f"{dt} T {T} {pattern} finished")


@pytest.mark.parametrize("T", (1, 33, 65))
def test_every_slot_is_written_exactly_where_it_belongs(gpu_device, T):
    """The slab form into a NaN-filled buffer: every (t, k) row of every slab is finite in its N columns afterwards, and the
    rows past T and the pad columns are untouched.  (Each slot sits in exactly one expert's list, so it is written once.)"""
    from tgis_amd import native

    dt, I = torch.float16, mc.INTERMEDIATES[0]
    _w1, _w3, _w2, up_w, down_w = _weights(I, dt, gpu_device)
    lib = native.load_library()
    ids = _pattern("uniform", T)
    r = native.moe_route(_logits_for(ids).to(gpu_device), TOP_K)
    h = native.moe_gemm_up(_x(T, dt, torch.Generator().manual_seed(T)).to(gpu_device), up_w, r)
    N = 300  # a down projection with an N tail: the first 300 rows of the same images' columns (ld 320)
    narrow = native.MoeWeights(lambda e: _w2[e][:N].to(gpu_device), E)
    nbytes = lib.tgis_moe_gemm_down_bytes(T, N, TOP_K, 0)
    ld = (N + 31) // 32 * 32
    assert nbytes == (T + 31) // 32 * TOP_K * 32 * ld * 4
    slabs = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=gpu_device)
    rc = lib.tgis_moe_gemm_down(h.data_ptr(), h.stride(0), narrow.image.data_ptr(), narrow.stride, r.offsets.data_ptr(),
                                r.slot_rows.data_ptr(), r.expert_w.data_ptr(), T, I, N, E, TOP_K, native.F16, 0,
                                slabs.data_ptr(), nbytes, None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.tgis_last_error()
    torch.cuda.synchronize()
    s = slabs.view(-1, TOP_K, 32, ld).permute(0, 2, 1, 3).reshape(-1, TOP_K, ld).cpu()
    assert torch.isfinite(s[:T, :, :N]).all()
    assert torch.isnan(s[T:]).all() and torch.isnan(s[:, :, N:]).all()
    yref, ytol = _down_reference(h.cpu(), _w2[:, :N], ids, r.expert_w.cpu())
    _close(s[:T, :, :N], yref, ytol, f"T {T} N {N} slabs")


def _norm_reference(total, total_tol, residual, weight, eps, dt):
    """(res, res_tol, y, y_tol) of the add + RMSNorm behind the block, from the fp64 sum `total` known to `total_tol`."""
    u = U[dt]
    x = total.to(dt).double()
    dx = total_tol + A_OUT * u * total.abs() + TINY[dt]
    res = (x + residual.double())
    res_r = res.to(dt).double()
    dres = dx + A_OUT * u * res.abs() + TINY[dt]
    hidden = res.shape[1]
    s2 = (res * res).sum(dim=1, keepdim=True)
    rstd = torch.rsqrt(s2 / hidden + eps)
    # d(rstd) / rstd = -1/2 d(s2) / (s2 + hidden eps), d(s2) <= 2 sum |res| dres, plus fp32 roundoff of the sum
    drel = ((res.abs() * dres).sum(dim=1, keepdim=True) / (s2 + hidden * eps)) + hidden * 2.0 ** -24
    y = res * rstd * weight.double()
    dy = (rstd * weight.double().abs()) * dres + y.abs() * drel + A_OUT * u * y.abs() + TINY[dt]
    return res_r, dres, y.to(dt).double(), dy


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_partial_into_the_norm(gpu_device, dt):
    """The decode form's Partial through rmsnorm_residual: the residual stream and the normed rows are the reference's within
    the propagated bound, and bit for bit what the norm gives on the finished form's tensor."""
    from tgis_amd import native

    I, T, eps = mc.INTERMEDIATES[1], 33, 1e-5
    w1, w3, w2, up_w, down_w = _weights(I, dt, gpu_device)
    ids = _pattern("uniform", T)
    gen = torch.Generator().manual_seed(77)
    x = _x(T, dt, gen)
    residual = torch.randn(T, HIDDEN, generator=gen).to(dt)
    weight = (1.0 + 0.1 * torch.randn(HIDDEN, generator=gen)).to(dt)
    r = native.moe_route(_logits_for(ids).to(gpu_device), TOP_K)
    h = native.moe_gemm_up(x.to(gpu_device), up_w, r)
    p = native.moe_gemm_down(h, down_w, r, partial=True)
    out = native.moe_gemm_down(h, down_w, r, partial=False)
    y_p, res_p = native.rmsnorm_residual(p, residual.to(gpu_device), weight.to(gpu_device), eps)
    y_f, res_f = native.rmsnorm_residual(out, residual.to(gpu_device), weight.to(gpu_device), eps)
    assert torch.equal(y_p, y_f) and torch.equal(res_p, res_f)
    yref, ytol = _down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    total_tol = ytol.sum(dim=1) + U[torch.float32] * yref.abs().sum(dim=1)
    res, dres, y, dy = _norm_reference(yref.sum(dim=1), total_tol, residual, weight, eps, dt)
    _close(res_p, res, dres, f"{dt} residual stream")
    _close(y_p, y, dy, f"{dt} normed")


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_captured_launches_follow_the_routing_of_each_replay(gpu_device, dt):
    """route + up + down (both forms) captured in one graph over a static logit buffer: routing that changes between
    replays gives each replay's own reference."""
    from tgis_amd import native

    I, T = mc.INTERMEDIATES[1], 33
    w1, w3, w2, up_w, down_w = _weights(I, dt, gpu_device)
    gen = torch.Generator().manual_seed(5)
    x = _x(T, dt, gen)
    xg = x.to(gpu_device)
    static_logits = torch.zeros((T, E), dtype=torch.float32, device=gpu_device)

    def step():
        r = native.moe_route(static_logits, TOP_K)
        h = native.moe_gemm_up(xg, up_w, r)
        return r, h, native.moe_gemm_down(h, down_w, r, partial=True), native.moe_gemm_down(h, down_w, r, partial=False)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r, h, p, out = step()
    for pattern in ("same_two", "uniform", "last_token_alone"):
        ids = _pattern(pattern, T)
        static_logits.copy_(_logits_for(ids))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.expert_ids.cpu().long(), ids), pattern
        ref, tol = _up_reference(x, w1, w3, ids, dt)
        _close(h, ref, tol, f"{dt} replay {pattern} up")
        yref, ytol = _down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
        _close(_slab_rows(p, T), yref, ytol, f"{dt} replay {pattern} slabs")
        total = yref.sum(dim=1)
        ftol = ytol.sum(dim=1) + U[torch.float32] * yref.abs().sum(dim=1) + A_OUT * U[dt] * total.abs() + TINY[dt]
        _close(out, total.to(dt).double(), ftol, f"{dt} replay {pattern} finished")
