"""-m gpu: the routed-expert kernels (csrc/moe.hip: tgis_moe_route, tgis_moe_gemm_up, tgis_moe_gemm_down) against the fp64
restatement of tests/moe_ref.py.

Route: ids and lists exactly, weights within 4 ulp of fp32, ties to the lower index.  Up and down: hidden 320 (5 k64-steps:
the four k-parts get 2, 2, 1 and 0 of them), I 80 and 528 (N tails, one and many tiles, a K tail inside a k64-step for the
down GEMM), f16 and bf16, every row count around the 32-row slab, and routing patterns forced through hand-written logits.
The images of experts nobody chose are filled with NaN: a block that read them would show.

Per-element bounds are derived as tests/test_gemm_edges_gpu.py derives them (restated in tests/moe_bounds.py, which this file
shares with tests/test_moe_edges_gpu.py): fp32 accumulation costs B_ACC K 2^-24 per unit of |x| @ |W|, an output rounding A_OUT
unit roundoffs of |ref|; the SiLU * up epilogue propagates the two sums' errors through T(T(silu(T g)) * T up).

tests/test_moe_edges_gpu.py takes the same kernels where these shapes do not reach: k-parts deeper than the weight ring, short
and ragged K, every admitted top_k and E, row strides, prefills of more than 1024 tokens, near-tied and underflowing routers,
and expert images past 2^31 and 2^32 bytes."""
import ctypes

import pytest
import torch

from tests import moe_bounds as mb
from tests import moe_cases as mc

pytestmark = pytest.mark.gpu

DTYPES = mb.DTYPES
E, TOP_K, HIDDEN = mc.E, mc.TOP_K, mc.HIDDEN
PATTERNS = mb.PATTERNS


def _logits_for(ids):
    return mb.logits_for(ids, E)


# ---- routing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E_,top_k", mc.ROUTE_CASES, ids=lambda v: str(v))
def test_route_matches_the_restatement(gpu_device, E_, top_k):
    from tgis_amd import native

    g = torch.Generator().manual_seed(100 * E_ + top_k)
    for T in mc.ROUTE_TOKENS:
        logits = torch.randn(T, E_, generator=g) * 2.0
        r = native.moe_route(logits.to(gpu_device), top_k)
        mb.check_routing(logits, r, E_, top_k)
        again = native.moe_route(logits.to(gpu_device), top_k)
        for name in ("expert_ids", "expert_w", "lists", "slot_rows"):
            assert torch.equal(getattr(r, name), getattr(again, name)), name


def test_route_reads_a_strided_logit_matrix_and_serves_no_tokens(gpu_device):
    from tgis_amd import native

    g = torch.Generator().manual_seed(9)
    wide = torch.randn(33, 16, generator=g)
    r = native.moe_route(wide.to(gpu_device)[:, :8], 2)  # row stride 16
    mb.check_routing(wide[:, :8], r, 8, 2)
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
    mb.check_routing(logits, r, 8, 2)


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


def _x(T, dt, gen):
    return ((torch.randn(T, HIDDEN, generator=gen) * 0.5 + 0.25)).to(dt)


def _run_case(dev, I, dt, T, pattern):
    from tgis_amd import native

    ids = mb.pattern(pattern, T)
    if ids is None:
        return False
    w1, w3, w2, up_w, down_w = _weights(I, dt, dev)
    chosen = set(ids.reshape(-1).tolist())
    up_w, down_w = mb.poisoned(up_w, chosen), mb.poisoned(down_w, chosen)
    gen = torch.Generator().manual_seed(T * 7 + I)
    x = _x(T, dt, gen)
    logits = _logits_for(ids)
    r = native.moe_route(logits.to(dev), TOP_K)
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    what = f"I {I} {dt} T {T} {pattern}"

    h = native.moe_gemm_up(x.to(dev), up_w, r)
    ref, tol = mb.up_reference(x, w1, w3, ids, dt)
    mb.close(h, ref, tol, what + " up")

    p = native.moe_gemm_down(h, down_w, r, partial=True)
    assert p.S == TOP_K and p.shape == (T, HIDDEN) and p.ld == HIDDEN
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    mb.close(mb.slab_rows(p, T), yref, ytol, what + " down slabs")

    out = native.moe_gemm_down(h, down_w, r, partial=False)
    mb.close(out, *mb.finished_reference(yref, ytol, dt), what + " down finished")
    # the deferred sum and the finished one are the same fp32 additions in the same order
    rows = mb.slab_rows(p, T)
    assert torch.equal((rows[:, 0] + rows[:, 1]).to(dt), out), what

    # two runs, the same bytes
    h2 = native.moe_gemm_up(x.to(dev), up_w, r)
    p2 = native.moe_gemm_down(h2, down_w, r, partial=True)
    assert torch.equal(h, h2) and torch.equal(mb.slab_rows(p, T), mb.slab_rows(p2, T)), what
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
        ids = mb.pattern(pattern, T)
        gen = torch.Generator().manual_seed(T)
        x = _x(T, dt, gen)
        r = native.moe_route(_logits_for(ids).to(gpu_device), TOP_K)
        h = native.moe_gemm_up(x.to(gpu_device), up_w, r)
        ref, tol = mb.up_reference(x, w1, w3, ids, dt)
        mb.close(h, ref, tol, f"{dt} T {T} {pattern} up")
        out = native.moe_gemm_down(h, down_w, r, partial=False)
        yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
        mb.close(out, *mb.finished_reference(yref, ytol, dt), f"{dt} T {T} {pattern} finished")


@pytest.mark.parametrize("T", (1, 33, 65))
def test_every_slot_is_written_exactly_where_it_belongs(gpu_device, T):
    """The slab form into a NaN-filled buffer: every (t, k) row of every slab is finite in its N columns afterwards, and the
    rows past T and the pad columns are untouched.  (Each slot sits in exactly one expert's list, so it is written once.)"""
    from tgis_amd import native

    dt, I = torch.float16, mc.INTERMEDIATES[0]
    _w1, _w3, _w2, up_w, down_w = _weights(I, dt, gpu_device)
    lib = native.load_library()
    ids = mb.pattern("uniform", T)
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
    yref, ytol = mb.down_reference(h.cpu(), _w2[:, :N], ids, r.expert_w.cpu())
    mb.close(s[:T, :, :N], yref, ytol, f"T {T} N {N} slabs")


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_partial_into_the_norm(gpu_device, dt):
    """The decode form's Partial through rmsnorm_residual: the residual stream and the normed rows are the reference's within
    the propagated bound, and bit for bit what the norm gives on the finished form's tensor."""
    from tgis_amd import native

    I, T, eps = mc.INTERMEDIATES[1], 33, 1e-5
    w1, w3, w2, up_w, down_w = _weights(I, dt, gpu_device)
    ids = mb.pattern("uniform", T)
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
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    total_tol = mb.sum_tol(yref, ytol)
    res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), total_tol, residual, weight, eps, dt)
    mb.close(res_p, res, dres, f"{dt} residual stream")
    mb.close(y_p, y, dy, f"{dt} normed")


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
        ids = mb.pattern(pattern, T)
        static_logits.copy_(_logits_for(ids))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.expert_ids.cpu().long(), ids), pattern
        ref, tol = mb.up_reference(x, w1, w3, ids, dt)
        mb.close(h, ref, tol, f"{dt} replay {pattern} up")
        yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
        mb.close(mb.slab_rows(p, T), yref, ytol, f"{dt} replay {pattern} slabs")
        mb.close(out, *mb.finished_reference(yref, ytol, dt), f"{dt} replay {pattern} finished")
