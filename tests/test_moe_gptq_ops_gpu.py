"""-m gpu: the int4 routed-expert GEMMs (csrc/moe.hip: tgis_moe_gptq_gemm_up, tgis_moe_gptq_gemm_down) against the fp64
restatement of tests/moe_ref.py on the dequantised weights.

The reference weight is W16 = f16((q - z - 1) * s), which the kernel's dequant8 reproduces exactly, so the references and the
per-element bounds are tests/moe_bounds.py's (fp32 accumulation over K, one output rounding, the SiLU * up propagation) with
no new constants.  E 8, top-2, f16.  tests/moe_gptq_cases.py lists the shapes: every k-part split, group boundaries inside a
k-part and a wave that starts mid-group, k deeper than any ring depth, every row count around the 32-row slab under the routing
patterns of moe_bounds.  The images of experts nobody chose are 0xFF bytes."""
import ctypes

import pytest
import torch

from tests import moe_bounds as mb
from tests import moe_gptq_cases as gc

pytestmark = pytest.mark.gpu

DT = torch.float16
E, TOP_K = gc.E, gc.TOP_K
_IMAGES = {}


def _up(K, I, gs, dev):
    key = ("up", K, I, gs)
    if key not in _IMAGES:
        bundles, w1, w3 = gc.up_experts(K, I, gs)
        _IMAGES[key] = (w1, w3, gc.moe_weights(bundles, gs, dev, gate_up=True))
    return _IMAGES[key]


def _down(K, N, gs, dev):
    key = ("down", K, N, gs)
    if key not in _IMAGES:
        bundles, w2 = gc.down_experts(K, N, gs)
        _IMAGES[key] = (w2, gc.moe_weights(bundles, gs, dev))
    return _IMAGES[key]


def _route(ids, dev):
    from tgis_amd import native

    r = native.moe_route(mb.logits_for(ids, E).to(dev), TOP_K)
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    return r


def _patterns(T):
    return [(name, ids) for name, ids in ((n, mb.pattern(n, T)) for n in mb.PATTERNS) if ids is not None]


def _check_up(dev, K, I, gs, T, name, ids):
    from tgis_amd import native

    w1, w3, mw = _up(K, I, gs, dev)
    assert (mw.K, mw.N, mw.groups, mw.flags) == (K, 2 * I, gc.groups_of(K, gs), 1)
    mw = gc.poisoned(mw, set(ids.reshape(-1).tolist()))
    x = mb.up_input(T, K, DT)
    r = _route(ids, dev)
    h = native.moe_gptq_gemm_up(x.to(dev), mw, r)
    assert h.shape == (T * TOP_K, I) and h.dtype == DT
    ref, tol = mb.up_reference(x, w1, w3, ids, DT)
    mb.close(h, ref, tol, f"up K {K} I {I} gs {gs} T {T} {name}")
    assert torch.equal(h, native.moe_gptq_gemm_up(x.to(dev), mw, r)), "two runs, the same bytes"


def _check_down(dev, K, N, gs, T, name, ids, slabs=True):
    from tgis_amd import native

    w2, mw = _down(K, N, gs, dev)
    assert (mw.K, mw.N, mw.groups, mw.flags) == (K, N, gc.groups_of(K, gs), 0)
    mw = gc.poisoned(mw, set(ids.reshape(-1).tolist()))
    h = mb.down_input(T, TOP_K, K, DT)
    r = _route(ids, dev)
    what = f"down K {K} N {N} gs {gs} T {T} {name}"
    yref, ytol = mb.down_reference(h, w2, ids, r.expert_w.cpu())
    out = native.moe_gptq_gemm_down(h.to(dev), mw, r, partial=False)
    assert out.shape == (T, N) and out.dtype == DT
    mb.close(out, *mb.finished_reference(yref, ytol, DT), what + " finished")
    if not slabs:
        return
    p = native.moe_gptq_gemm_down(h.to(dev), mw, r, partial=True)
    assert isinstance(p, native.Partial) and p.S == TOP_K and p.shape == (T, N) and p.ld == N
    rows = mb.slab_rows(p, T)
    mb.close(rows, yref, ytol, what + " slabs")
    # the deferred sum and the finished one are the same fp32 additions in the same order
    assert torch.equal(mb.slab_sum(rows).to(DT), out), what
    p2 = native.moe_gptq_gemm_down(h.to(dev), mw, r, partial=True)
    assert torch.equal(rows, mb.slab_rows(p2, T)), what + ": two runs, the same bytes"


@pytest.mark.parametrize("K,I,gs", gc.UP_CASES, ids=lambda v: str(v))
def test_up_under_every_pattern(gpu_device, K, I, gs):
    for T in gc.TOKENS:
        ran = _patterns(T)
        assert len(ran) >= 3
        for name, ids in ran:
            _check_up(gpu_device, K, I, gs, T, name, ids)


@pytest.mark.parametrize("K,N,gs", gc.DOWN_CASES, ids=lambda v: str(v))
def test_down_under_every_pattern(gpu_device, K, N, gs):
    for T in gc.TOKENS:
        ran = _patterns(T)
        assert len(ran) >= 3
        for name, ids in ran:
            _check_down(gpu_device, K, N, gs, T, name, ids)


@pytest.mark.parametrize("K,N,gs", gc.DEEP_CASES, ids=lambda v: str(v))
def test_deep_k_refills_the_ring(gpu_device, K, N, gs):
    """k-parts of 5, 5, 5, 2 steps and of 17 steps each: past a ring of 4, and past the ring that is kept (and one of 16)."""
    for T in (1, 33):
        for name in ("uniform", "same_two"):
            ids = mb.pattern(name, T)
            _check_up(gpu_device, K, N // 2, gs, T, name, ids)
            _check_down(gpu_device, K, N, gs, T, name, ids)


def test_finished_form_at_130_rows(gpu_device):
    K, N, gs = gc.DOWN_CASES[2]
    for name in ("uniform", "same_two"):
        ids = mb.pattern(name, gc.FINISHED_TOKENS)
        _check_up(gpu_device, *gc.UP_CASES[2], gc.FINISHED_TOKENS, name, ids)
        _check_down(gpu_device, K, N, gs, gc.FINISHED_TOKENS, name, ids, slabs=False)


@pytest.mark.parametrize("gs", (64, -1))
def test_partial_into_the_norm(gpu_device, gs):
    """The Partial through rmsnorm_residual: bit for bit the norm of the finished tensor, both within norm_reference's bound."""
    from tgis_amd import native

    K, N, T, eps, dev = 576, 320, 33, 1e-5, gpu_device
    w2, mw = _down(K, N, gs, dev)
    ids = mb.pattern("uniform", T)
    gen = torch.Generator().manual_seed(77)
    h = mb.down_input(T, TOP_K, K, DT)
    residual = torch.randn(T, N, generator=gen).to(DT)
    weight = (1.0 + 0.1 * torch.randn(N, generator=gen)).to(DT)
    r = _route(ids, dev)
    p = native.moe_gptq_gemm_down(h.to(dev), mw, r, partial=True)
    out = native.moe_gptq_gemm_down(h.to(dev), mw, r, partial=False)
    y_p, res_p = native.rmsnorm_residual(p, residual.to(dev), weight.to(dev), eps)
    y_f, res_f = native.rmsnorm_residual(out, residual.to(dev), weight.to(dev), eps)
    assert torch.equal(y_p, y_f) and torch.equal(res_p, res_f)
    yref, ytol = mb.down_reference(h, w2, ids, r.expert_w.cpu())
    res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, eps, DT)
    for got_res, got_y in ((res_p, y_p), (res_f, y_f)):
        mb.close(got_res, res, dres, f"gs {gs} residual stream")
        mb.close(got_y, y, dy, f"gs {gs} normed")


@pytest.mark.parametrize("K,I,gs", [(320, 576, 64), (384, 64, 128), (320, 64, -1)], ids=lambda v: str(v))
def test_an_expert_alone_equals_the_int4_gemm_on_its_view(gpu_device, K, I, gs):
    """Every token through expert e and one other: the rows of e against gptq_gemm(act=2) on .expert(e) — the view shares the
    image's bytes, perm is None — both within the up bound of the same reference."""
    from tgis_amd import native
    from tgis_amd.utils.layers import workspace

    dev, T = gpu_device, 33
    w1, w3, mw = _up(K, I, gs, dev)
    x = mb.up_input(T, K, DT)
    for e in (0, 5, 7):
        other = (e + 3) % E
        ids = torch.tensor([[e, other]]).repeat(T, 1)
        r = _route(ids, dev)
        h = native.moe_gptq_gemm_up(x.to(dev), mw, r).view(T, TOP_K, I)[:, 0]
        view = mw.expert(e)
        assert view.perm is None and view.image.data_ptr() == mw.image[e].data_ptr() and view.image.numel() == mw.stride
        assert (view.K, view.N, view.groups, view.flags) == (mw.K, mw.N, mw.groups, 1)
        alone = native.gptq_gemm(x.to(dev), view, workspace(dev), act=2)
        ref, tol = mb.up_reference(x, w1, w3, ids, DT)
        ref, tol = ref.view(T, TOP_K, I)[:, 0], tol.view(T, TOP_K, I)[:, 0]
        mb.close(h, ref, tol, f"expert {e} behind the routing")
        mb.close(alone, ref, tol, f"expert {e} through gptq_gemm on its view")


def test_captured_launches_follow_the_routing_of_each_replay(gpu_device):
    """route + up + down (both forms) captured in one graph over a static logit buffer: routing that changes between replays
    gives each replay's own reference."""
    from tgis_amd import native

    dev, T = gpu_device, 33
    K, I, gs = 320, 576, 64
    w1, w3, up_w = _up(K, I, gs, dev)
    w2, down_w = _down(I, 320, gs, dev)
    x = mb.up_input(T, K, DT)
    xg = x.to(dev)
    static_logits = torch.zeros((T, E), dtype=torch.float32, device=dev)

    def step():
        r = native.moe_route(static_logits, TOP_K)
        h = native.moe_gptq_gemm_up(xg, up_w, r)
        return (r, h, native.moe_gptq_gemm_down(h, down_w, r, partial=True),
                native.moe_gptq_gemm_down(h, down_w, r, partial=False))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r, h, p, out = step()
    for name in ("same_two", "uniform", "last_token_alone"):
        ids = mb.pattern(name, T)
        static_logits.copy_(mb.logits_for(ids, E))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(r.expert_ids.cpu().long(), ids), name
        ref, tol = mb.up_reference(x, w1, w3, ids, DT)
        mb.close(h, ref, tol, f"replay {name} up")
        yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
        mb.close(mb.slab_rows(p, T), yref, ytol, f"replay {name} slabs")
        mb.close(out, *mb.finished_reference(yref, ytol, DT), f"replay {name} finished")


def test_entry_points_refuse_without_launching(gpu_device):
    """K 96, N 48, groups of 32 rows, a stride below one image and bf16: an error code, and outputs filled with NaN stay NaN."""
    from tgis_amd import native

    lib, dev, T = native.load_library(), gpu_device, 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = _route(mb.pattern("uniform", T), dev)
    image = torch.zeros(E * (1 << 20), dtype=torch.uint8, device=dev)
    x = torch.ones((T * TOP_K, 1024), dtype=DT, device=dev)
    out = torch.full((T * TOP_K, 1024), float("nan"), dtype=DT, device=dev)
    scratch = torch.full((T * TOP_K * 1024,), float("nan"), dtype=torch.float32, device=dev)

    def up(K, N, G, stride=1 << 20, dtype=native.F16):
        return lib.tgis_moe_gptq_gemm_up(x.data_ptr(), 1024, image.data_ptr(), stride, r.offsets.data_ptr(),
                                         r.slot_rows.data_ptr(), out.data_ptr(), 1024, T, K, N, G, E, TOP_K, dtype, stream)

    def down(K, N, G, stride=1 << 20, dtype=native.F16, form=0):
        return lib.tgis_moe_gptq_gemm_down(x.data_ptr(), 1024, image.data_ptr(), stride, r.offsets.data_ptr(),
                                           r.slot_rows.data_ptr(), r.expert_w.data_ptr(), T, K, N, G, E, TOP_K, dtype, form,
                                           scratch.data_ptr(), scratch.numel() * 4, out.data_ptr(), 1024, stream)

    small = lib.tgis_gptq_prepared_bytes(320, 64, 5) - 16
    for fn in (up, down):
        for bad in (dict(K=96, N=64, G=1), dict(K=320, N=48, G=5), dict(K=320, N=64, G=10),
                    dict(K=320, N=64, G=5, stride=small), dict(K=320, N=64, G=5, dtype=native.BF16)):
            assert fn(**bad) != 0, (fn.__name__, bad)
            assert lib.tgis_last_error()
            lib.tgis_clear_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(scratch).all()
    # the same calls at a served shape launch (zero images: finite outputs)
    assert up(320, 64, 5, stride=small + 16) == 0 and down(320, 64, 5, stride=small + 16) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:, :32]).all()
