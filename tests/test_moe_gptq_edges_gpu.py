"""-m gpu: the int4 routed-expert GEMMs (csrc/moe.hip: Int4Source behind tgis_moe_gptq_gemm_up / _down) where the shapes of
tests/test_moe_gptq_ops_gpu.py do not reach (tests/moe_gptq_cases.py holds the tables, tests/test_moe_gptq_edges_cpu.py checks
without a GPU that they reach what they claim):

  1. every admitted group size from 128 to 16384 rows (spg_shift 1 to 8) and a single group written as groupsize == K, under
     activations that are zero outside one k64-step, so that a step dequantised under a neighbouring group's scale leaves the
     bound however deep K is;
  2. hand-packed matrices that hold every (nibble, zero point) pair in every nibble position and lane half, read back row by
     row through the identity: bit for bit in the down GEMM;
  3. every admitted kind of (E, top_k) through the gather, the slab address, the combine and the add + RMSNorm;
  4. row strides wider than the rows, an expert stride wider than an image, the image's own padding overwritten, T == 0;
  5. expert images whose byte offsets e * stride lie past 2^31 and 2^32, in an arena that holds 0xFF everywhere else.

References are tests/moe_ref.py in fp64 on W16 = f16((q - z - 1) * s) and the bounds are tests/moe_bounds.py's, unchanged.
f16 throughout.  The images of experts nobody chose are 0xFF bytes."""
import ctypes

import pytest
import torch

from tests import far_pool as fp
from tests import moe_bounds as mb
from tests import moe_cases as mc
from tests import moe_gptq_cases as gc
from tests import moe_ref

pytestmark = pytest.mark.gpu

DT = gc.DT
E, TOP_K, HIDDEN = gc.E, gc.TOP_K, mc.HIDDEN
CASE_IDS = [f"K{K}-gs{gs}" for K, gs in gc.GROUP_CASES]
_IMAGES = {}


def _cached(key, make):
    if key not in _IMAGES:
        _IMAGES[key] = make()
    return _IMAGES[key]


def _chosen(ids):
    return set(ids.reshape(-1).tolist())


def _route_to(ids, E_, dev):
    """The kernel's routing of hand-written logits whose choices are `ids`."""
    from tgis_amd import native

    r = native.moe_route(mb.logits_for(ids, E_).to(dev), ids.shape[1])
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    return r


def _down_checks(dev, h, mw, r, w2, ids, what):
    """Both forms of the down GEMM against the reference; the finished rows equal the slabs' sum; two runs, the same bytes.
    Returns (slab rows [T, top_k, N], finished [T, N])."""
    from tgis_amd import native

    T, top_k = ids.shape
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    hg = h.to(dev)
    p = native.moe_gptq_gemm_down(hg, mw, r, partial=True)
    assert isinstance(p, native.Partial) and p.S == top_k and p.shape == (T, mw.N) and p.ld == mw.N
    rows = mb.slab_rows(p, T)
    mb.close(rows, yref, ytol, what + " down slabs")
    out = native.moe_gptq_gemm_down(hg, mw, r, partial=False)
    assert out.shape == (T, mw.N) and out.dtype == DT
    mb.close(out, *mb.finished_reference(yref, ytol, DT), what + " down finished")
    # the deferred sum and the finished one are the same fp32 additions in the same order, k = 0..top_k-1
    assert torch.equal(mb.slab_sum(rows).to(DT), out), what
    p2 = native.moe_gptq_gemm_down(hg, mw, r, partial=True)
    assert torch.equal(rows, mb.slab_rows(p2, T)) and torch.equal(out, native.moe_gptq_gemm_down(hg, mw, r, partial=False)), what
    return rows, out


# ---- 1. every group size, under step probes ---------------------------------------------------------------------------------
def _group_images(which, K, gs, dev):
    return _cached(("group", which, K, gs), lambda: gc.poisoned(
        gc.moe_weights(gc.group_bundles(which, K, gs), gs, dev, gate_up=which == "up"), set(gc.GROUP_IDS)))


@pytest.mark.parametrize("K,gs", gc.GROUP_CASES, ids=CASE_IDS)
def test_up_takes_every_step_s_own_group(gpu_device, K, gs):
    """Each probe row sees one k64-step of the gate|up matrix: the first and last step of the groups and of the k-parts and
    the first refill of every ring slot.  Its bound is one step's, so the scale of a neighbouring group shows."""
    from tgis_amd import native

    mw = _group_images("up", K, gs, gpu_device)
    assert (mw.K, mw.N, mw.groups, mw.flags) == (K, 2 * gc.GROUP_I, gc.groups_of(K, gs), 1)
    T = gc.probe_tokens(K, gs)
    ids = gc.group_ids(T)
    r = _route_to(ids, E, gpu_device)
    assert r.counts.tolist() == [T if e in gc.GROUP_IDS else 0 for e in range(E)] and T > 32
    x = gc.probe_input(K, gs, 1)
    w1, w3 = gc.stack_up({e: w16 for e, (_b, w16) in gc.group_experts("up", K, gs).items()}, gc.GROUP_I)
    h = native.moe_gptq_gemm_up(x.to(gpu_device), mw, r)
    assert h.shape == (T * TOP_K, gc.GROUP_I) and h.dtype == DT
    mb.close(h, *mb.up_reference(x, w1, w3, ids, DT), f"up K {K} gs {gs}")
    assert torch.equal(h, native.moe_gptq_gemm_up(x.to(gpu_device), mw, r)), "two runs, the same bytes"


@pytest.mark.parametrize("K,gs", gc.GROUP_CASES, ids=CASE_IDS)
def test_down_takes_every_step_s_own_group(gpu_device, K, gs):
    """The same probes as the two slot rows of every token, through the slab form and the finished form."""
    mw = _group_images("down", K, gs, gpu_device)
    assert (mw.K, mw.N, mw.groups, mw.flags) == (K, gc.GROUP_DOWN_N, gc.groups_of(K, gs), 0)
    T = gc.probe_tokens(K, gs)
    ids = gc.group_ids(T)
    r = _route_to(ids, E, gpu_device)
    w2 = gc.stack_down({e: w16 for e, (_b, w16) in gc.group_experts("down", K, gs).items()})
    _down_checks(gpu_device, gc.probe_input(K, gs, TOP_K), mw, r, w2, ids, f"K {K} gs {gs}")


# ---- 2. dequantisation, bit for bit -----------------------------------------------------------------------------------------
def _dequant_images(K, gs, gate_up, dev):
    """Expert DEQUANT_EXPERT holds the hand-packed matrix; expert 0 is 0xFF bytes."""
    def make():
        bundle, w16 = gc.dequant_expert(K, gs, gate_up)
        mw = gc.moe_weights([bundle] * gc.DEQUANT_E, gs, dev, gate_up=gate_up)
        return w16, gc.poisoned(mw, {gc.DEQUANT_EXPERT})
    return _cached(("dequant", K, gs, gate_up), make)


@pytest.mark.parametrize("K,gs", gc.DEQUANT_CASES, ids=lambda v: str(v))
def test_down_over_the_identity_returns_the_dequantised_matrix(gpu_device, K, gs):
    """x is the K x K identity, top_k 1, every token at expert 1 with weight exactly 1: fp32 row t of the slabs is row t of
    W16 = f16((q - z - 1) * s) and the finished tensor is W16 itself, compared with torch.equal.  Every (nibble, zero point)
    pair occurs in each of the 8 nibble positions and both lane halves, the scales span 2^-14 to 4094.  This is the one check
    of the image's row order [k0, k2, k4, k6, k1, k3, k5, k7] and of the k-part exchange row by row.  Products below the
    smallest normal f16 are left out on purpose (|q - z - 1| >= 1 times a scale >= 2^-14): how the MFMA treats f16 subnormal
    inputs on this part has not been measured, and nothing here asserts on them."""
    from tgis_amd import native

    w16, mw = _dequant_images(K, gs, False, gpu_device)
    assert (mw.K, mw.N, mw.groups, mw.E) == (K, gc.DEQUANT_N, gc.groups_of(K, gs), gc.DEQUANT_E)
    ids = gc.dequant_ids(K)
    r = _route_to(ids, gc.DEQUANT_E, gpu_device)
    assert torch.equal(r.expert_w.cpu(), torch.ones(K, 1)), "pk / psum with one term"
    assert r.counts.tolist() == [0, K]
    eye = torch.eye(K, dtype=DT, device=gpu_device)
    p = native.moe_gptq_gemm_down(eye, mw, r, partial=True)
    rows = mb.slab_rows(p, K)
    assert rows.shape == (K, 1, gc.DEQUANT_N) and rows.dtype == torch.float32
    got, want = rows[:, 0].cpu(), w16.float()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        k, n = bad[0].tolist()
        raise AssertionError(f"{len(bad)} of {got.numel()} elements differ; first at row {k} column {n}: got {got[k, n].item()!r} "
                             f"W16 {want[k, n].item()!r}; rows {sorted(set(bad[:, 0].tolist()))[:16]}")
    out = native.moe_gptq_gemm_down(eye, mw, r, partial=False)
    assert out.dtype == DT and torch.equal(out.cpu(), w16)


@pytest.mark.parametrize("K,gs", gc.DEQUANT_CASES, ids=lambda v: str(v))
def test_up_over_the_identity(gpu_device, K, gs):
    """The identity through the hand-packed gate|up matrix: h[t] = silu(W16[t, gate]) * W16[t, up] within up_reference's bound
    (the SiLU goes through __expf, so by bound and not by bytes)."""
    from tgis_amd import native

    w16, mw = _dequant_images(K, gs, True, gpu_device)
    ids = gc.dequant_ids(K)
    r = _route_to(ids, gc.DEQUANT_E, gpu_device)
    eye = torch.eye(K, dtype=DT)
    w1, w3 = gc.stack_up({gc.DEQUANT_EXPERT: w16}, gc.DEQUANT_N // 2)
    h = native.moe_gptq_gemm_up(eye.to(gpu_device), mw, r)
    assert h.shape == (K, gc.DEQUANT_N // 2)
    mb.close(h, *mb.up_reference(eye, w1, w3, ids, DT), f"identity K {K} gs {gs} up")


# ---- 3. every admitted routing ------------------------------------------------------------------------------------------------
def _mix_images(dev, E_, ids=None):
    """(w1, w3, w2, up images, down images) of E_ experts at hidden 320, I 64, groups of 64 rows; ids: poison the others."""
    def make():
        ub, w1, w3 = gc.up_experts(HIDDEN, gc.MIX_I, gc.MIX_GS, E_)
        db, w2 = gc.down_experts(gc.MIX_I, HIDDEN, gc.MIX_GS, E_)
        return w1, w3, w2, gc.moe_weights(ub, gc.MIX_GS, dev, gate_up=True), gc.moe_weights(db, gc.MIX_GS, dev)
    w1, w3, w2, up_w, down_w = _cached(("mix", E_), make)
    assert (up_w.groups, down_w.groups, up_w.E) == (HIDDEN // gc.MIX_GS, 1, E_)
    if ids is not None:
        up_w, down_w = gc.poisoned(up_w, _chosen(ids)), gc.poisoned(down_w, _chosen(ids))
    return w1, w3, w2, up_w, down_w


def _mix_route(dev, T, E_, top_k):
    """Seeded random logits through the route kernel, checked against the restatement: (r, ids)."""
    from tgis_amd import native

    logits = mb.mix_logits(T, E_, top_k)
    r = native.moe_route(logits.to(dev), top_k)
    mb.check_routing(logits, r, E_, top_k)
    return r, moe_ref.route(logits, top_k)[0]


@pytest.mark.parametrize("E_,top_k", mc.MIX_ROUTINGS, ids=lambda v: str(v))
def test_every_admitted_routing_through_the_int4_gemms(gpu_device, E_, top_k):
    from tgis_amd import native

    ran = 0
    for T in mc.MIX_TOKENS:
        what = f"E {E_} top_k {top_k} T {T}"
        r, ids = _mix_route(gpu_device, T, E_, top_k)
        w1, w3, w2, up_w, down_w = _mix_images(gpu_device, E_, ids)
        if (E_, top_k, T) == (64, 2, 1):
            assert len(_chosen(ids)) == 2  # 62 images hold 0xFF
        x = mb.up_input(T, HIDDEN, DT)
        h = native.moe_gptq_gemm_up(x.to(gpu_device), up_w, r)
        assert h.shape == (T * top_k, gc.MIX_I)
        mb.close(h, *mb.up_reference(x, w1, w3, ids, DT), what + " up")
        assert torch.equal(h, native.moe_gptq_gemm_up(x.to(gpu_device), up_w, r)), what + ": two runs, the same bytes"
        _down_checks(gpu_device, h, down_w, r, w2, ids, what)
        ran += 1
    assert ran == len(mc.MIX_TOKENS) == 3


@pytest.mark.parametrize("top_k", gc.NORM_TOP_K)
def test_partial_of_any_top_k_into_the_norm(gpu_device, top_k):
    """A Partial with S = top_k slabs through rmsnorm_residual (sum_slabs8's buckets of 1, 4 and 8): within the propagated
    bound of the reference, and bit for bit what the norm gives on the finished form's tensor."""
    from tgis_amd import native

    T, eps, dev = gc.NORM_T, 1e-5, gpu_device
    r, ids = _mix_route(dev, T, E, top_k)
    _w1, _w3, w2, up_w, down_w = _mix_images(dev, E, ids)
    gen = torch.Generator().manual_seed(77 + top_k)
    residual = torch.randn(T, HIDDEN, generator=gen).to(DT)
    weight = (1.0 + 0.1 * torch.randn(HIDDEN, generator=gen)).to(DT)
    h = native.moe_gptq_gemm_up(mb.up_input(T, HIDDEN, DT).to(dev), up_w, r)
    p = native.moe_gptq_gemm_down(h, down_w, r, partial=True)
    assert p.S == top_k
    out = native.moe_gptq_gemm_down(h, down_w, r, partial=False)
    y_p, res_p = native.rmsnorm_residual(p, residual.to(dev), weight.to(dev), eps)
    y_f, res_f = native.rmsnorm_residual(out, residual.to(dev), weight.to(dev), eps)
    assert torch.equal(y_p, y_f) and torch.equal(res_p, res_f)
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, eps, DT)
    mb.close(res_p, res, dres, f"top_k {top_k} residual stream")
    mb.close(y_p, y, dy, f"top_k {top_k} normed")


# ---- 4. strides and bytes the kernel must not read ------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _c_up(x, image, stride, r, mw, T, hbuf):
    """tgis_moe_gptq_gemm_up on raw pointers: x and hbuf with their own row strides, `image` at `stride` bytes per expert."""
    from tgis_amd import native

    lib = native.load_library()
    rc = lib.tgis_moe_gptq_gemm_up(x.data_ptr(), x.stride(0), image.data_ptr(), stride, r.offsets.data_ptr(),
                                   r.slot_rows.data_ptr(), hbuf.data_ptr(), hbuf.stride(0), T, mw.K, mw.N, mw.groups, mw.E,
                                   r.top_k, native.F16, _stream())
    if rc == 0:
        torch.cuda.synchronize()
    return rc


def _c_down(h, image, stride, r, mw, T, form, scratch, obuf=None):
    from tgis_amd import native

    lib = native.load_library()
    rc = lib.tgis_moe_gptq_gemm_down(h.data_ptr(), h.stride(0), image.data_ptr(), stride, r.offsets.data_ptr(),
                                     r.slot_rows.data_ptr(), r.expert_w.data_ptr(), T, mw.K, mw.N, mw.groups, mw.E, r.top_k,
                                     native.F16, form, scratch.data_ptr(), scratch.numel() * 4,
                                     None if obuf is None else obuf.data_ptr(), 0 if obuf is None else obuf.stride(0), _stream())
    if rc == 0:
        torch.cuda.synchronize()
    return rc


def _scratch(T, N, top_k, form, dev):
    from tgis_amd import native

    return torch.full((native.load_library().tgis_moe_gemm_down_bytes(T, N, top_k, form) // 4,), float("nan"),
                      dtype=torch.float32, device=dev)


def _stride_case(dev):
    T = gc.STRIDE_T
    ids = mb.pattern("uniform", T)
    return T, ids, _route_to(ids, E, dev)


def test_row_strides_wider_than_the_rows(gpu_device):
    """x with ldx = K + 8 out of a NaN-filled matrix, h written with ldh = I + 16 into a NaN-filled buffer and read back with
    that stride by the down GEMM, the finished rows written with ldo = N + 4: the values hold their bounds and every pad
    element still holds NaN."""
    from tgis_amd import native

    dev, pads, I = gpu_device, gc.STRIDE_PADS, gc.MIX_I
    T, ids, r = _stride_case(dev)
    w1, w3, w2, up_w, down_w = _mix_images(dev, E, ids)
    x = mb.up_input(T, HIDDEN, DT)
    xg = mb.padded(x.to(dev), pads["x"])
    assert xg.stride(0) == HIDDEN + 8
    hbuf = torch.full((T * TOP_K, I + pads["h"]), float("nan"), dtype=DT, device=dev)
    assert _c_up(xg, up_w.image, up_w.stride, r, up_w, T, hbuf) == 0, native.load_library().tgis_last_error()
    assert torch.isnan(hbuf[:, I:]).all(), "the up GEMM wrote into the pad of h"
    h = hbuf[:, :I]
    mb.close(h, *mb.up_reference(x, w1, w3, ids, DT), "strided up")
    assert torch.equal(h, native.moe_gptq_gemm_up(x.to(dev), up_w, r)), "the same bytes as at the tight strides"

    N = HIDDEN
    obuf = torch.full((T, N + pads["out"]), float("nan"), dtype=DT, device=dev)
    assert _c_down(h, down_w.image, down_w.stride, r, down_w, T, 1, _scratch(T, N, TOP_K, 1, dev), obuf) == 0
    assert h.stride(0) == I + 16 and torch.isnan(obuf[:, N:]).all(), "the finished form wrote into the pad of out"
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    mb.close(obuf[:, :N], *mb.finished_reference(yref, ytol, DT), "strided down")
    assert torch.equal(obuf[:, :N], native.moe_gptq_gemm_down(h.contiguous(), down_w, r, partial=False))


def _run_all(dev, x, h, up_image, up_stride, down_image, down_stride, up_w, down_w, r, T):
    """(h, slabs, finished) of the three launches over the given images, as raw tensors."""
    hbuf = torch.full((T * TOP_K, up_w.N // 2), float("nan"), dtype=DT, device=dev)
    assert _c_up(x, up_image, up_stride, r, up_w, T, hbuf) == 0
    slabs = _scratch(T, down_w.N, TOP_K, 0, dev)
    assert _c_down(h, down_image, down_stride, r, down_w, T, 0, slabs) == 0
    obuf = torch.full((T, down_w.N), float("nan"), dtype=DT, device=dev)
    assert _c_down(h, down_image, down_stride, r, down_w, T, 1, _scratch(T, down_w.N, TOP_K, 1, dev), obuf) == 0
    return hbuf, slabs, obuf


def _same_bytes(a, b, what):
    for name, u, v in zip(("up", "down slabs", "down finished"), a, b):
        assert torch.equal(u.view(torch.int16 if u.dtype == DT else torch.int32), v.view(torch.int16 if v.dtype == DT else torch.int32)), \
            f"{what}: {name} differs"


def test_an_expert_stride_wider_than_an_image(gpu_device):
    """The images one image plus 4096 bytes apart, 0xFF in the gap behind every image: the same bytes as at the tight stride
    (the slabs' rows past T stay NaN in both)."""
    dev = gpu_device
    T, ids, r = _stride_case(dev)
    w1, w3, w2, up_w, down_w = _mix_images(dev, E, ids)
    x = mb.up_input(T, HIDDEN, DT).to(dev)
    h = mb.down_input(T, TOP_K, gc.MIX_I, DT).to(dev)
    tight = _run_all(dev, x, h, up_w.image, up_w.stride, down_w.image, down_w.stride, up_w, down_w, r, T)
    mb.close(tight[0], *mb.up_reference(x.cpu(), w1, w3, ids, DT), "tight stride up")
    wide = []
    for mw in (up_w, down_w):
        buf = torch.full((E, mw.stride + gc.STRIDE_GAP), 0xFF, dtype=torch.uint8, device=dev)
        buf[:, :mw.stride] = mw.image
        wide.append(buf)
    got = _run_all(dev, x, h, wide[0], up_w.stride + gc.STRIDE_GAP, wide[1], down_w.stride + gc.STRIDE_GAP, up_w, down_w, r, T)
    _same_bytes(got, tight, "wide expert stride")
    for buf, mw in zip(wide, (up_w, down_w)):
        assert (buf[:, mw.stride:] == 0xFF).all()


def test_the_image_s_padding_is_never_read(gpu_device):
    """At K 320 a tile holds 9 k64-steps in the image (whole 256-row chunks plus one pad step) and 5 are real.  Steps 5..8 of
    every tile of every expert overwritten with 0xFF (nibbles of 15 that would dequantise to non-zero weights) give the same
    bytes as the untouched images: no wave reads past its k-part, neither the last wave past K nor any wave's ring refill."""
    dev = gpu_device
    T, ids, r = _stride_case(dev)
    K = gc.PAD_K
    w1, w3, _w2, up_w, _down = _mix_images(dev, E, ids)
    def make():
        db, w2 = gc.down_experts(K, gc.PAD_DOWN_N, gc.MIX_GS)
        return w2, gc.moe_weights(db, gc.MIX_GS, dev)
    w2, down_w = _cached(("pad down",), make)
    down_w = gc.poisoned(down_w, _chosen(ids))
    x = mb.up_input(T, K, DT).to(dev)
    h = mb.down_input(T, TOP_K, K, DT).to(dev)
    clean = _run_all(dev, x, h, up_w.image, up_w.stride, down_w.image, down_w.stride, up_w, down_w, r, T)
    mb.close(clean[0], *mb.up_reference(x.cpu(), w1, w3, ids, DT), "K 320 up")
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    mb.close(clean[2], *mb.finished_reference(yref, ytol, DT), "K 320 down finished")
    real, held = mc.cdiv(K, 64), gc.image_steps(K)
    assert (real, held) == (5, 9)
    dirty = []
    for mw in (up_w, down_w):
        image = mw.image.clone()
        NT = mw.N // 32
        assert mw.stride == gc.prepared_bytes(K, mw.N, mw.groups) >= NT * held * 1024
        nibbles = image[:, :NT * held * 1024].view(E, NT, held, 1024)
        nibbles[:, :, real:] = 0xFF
        assert not torch.equal(image, mw.image)
        dirty.append(image)
    got = _run_all(dev, x, h, dirty[0], up_w.stride, dirty[1], down_w.stride, up_w, down_w, r, T)
    _same_bytes(got, clean, "0xFF in the padding steps")


def test_an_empty_batch_launches_nothing(gpu_device):
    """T == 0: both entry points return 0 and NaN-filled outputs stay NaN."""
    dev = gpu_device
    _T, ids, r = _stride_case(dev)
    _w1, _w3, _w2, up_w, down_w = _mix_images(dev, E, ids)
    x = torch.zeros((8, HIDDEN), dtype=DT, device=dev)
    hbuf = torch.full((8 * TOP_K, gc.MIX_I), float("nan"), dtype=DT, device=dev)
    assert _c_up(x, up_w.image, up_w.stride, r, up_w, 0, hbuf) == 0
    scratch = torch.full((8 * TOP_K * HIDDEN,), float("nan"), dtype=torch.float32, device=dev)
    obuf = torch.full((8, HIDDEN), float("nan"), dtype=DT, device=dev)
    for form in (0, 1):
        assert _c_down(hbuf, down_w.image, down_w.stride, r, down_w, 0, form, scratch, obuf) == 0
    torch.cuda.synchronize()
    assert torch.isnan(hbuf).all() and torch.isnan(scratch).all() and torch.isnan(obuf).all()


# ---- 5. expert images past 2^31 and 2^32 bytes ----------------------------------------------------------------------------------
class _FarWeights:
    """What native.moe_gptq_gemm_up / _down read of a MoeGptqWeights: the image is a view of the arena, the stride the wide
    one."""

    def __init__(self, image, K, N, flags):
        self.image, self.K, self.N, self.flags = image, K, N, flags
        self.E, self.stride, self.groups, self.dtype = mc.FAR_E, mc.FAR_STRIDE, gc.FAR_G, DT


@pytest.fixture(scope="module")
def far_images(gpu_device):
    """Five int4 gate|up images and, FAR_DOWN_SHIFT bytes behind each, five down images, written by tgis_gptq_prepare straight
    into their places in an arena of 0xFF bytes: (w1, w3, w2, up images, down images)."""
    from tgis_amd import native

    lib, dev = native.load_library(), gpu_device
    arena = fp.Arena(dev, mc.FAR_ARENA_BYTES)
    arena.words.fill_(-1)  # 0xFF in every byte
    raw = arena.words.view(torch.uint8)
    ub, w1, w3 = gc.up_experts(gc.FAR_K, gc.FAR_I, gc.FAR_GS, mc.FAR_E)
    db, w2 = gc.down_experts(gc.FAR_K, gc.FAR_DOWN_N, gc.FAR_GS, mc.FAR_E)
    assert lib.tgis_gptq_prepared_bytes(gc.FAR_K, 2 * gc.FAR_I, gc.FAR_G) == gc.FAR_IMAGE_BYTES
    assert lib.tgis_gptq_prepared_bytes(gc.FAR_K, gc.FAR_DOWN_N, gc.FAR_G) == gc.FAR_IMAGE_BYTES <= mc.FAR_DOWN_SHIFT
    for e in range(mc.FAR_E):
        for shift, bundle, N, flags in ((0, ub[e], 2 * gc.FAR_I, 1), (mc.FAR_DOWN_SHIFT, db[e], gc.FAR_DOWN_N, 0)):
            qw, qz, sc = (t.to(dev).contiguous() for t in bundle[:3])
            off = mc.FAR_BASE + shift + e * mc.FAR_STRIDE
            assert off + gc.FAR_IMAGE_BYTES <= arena.nbytes
            rc = lib.tgis_gptq_prepare(qw.data_ptr(), qz.data_ptr(), sc.to(DT).data_ptr(), None, None, gc.FAR_K, N, gc.FAR_G,
                                       flags, raw.data_ptr() + off, _stream())
            assert rc == 0, lib.tgis_last_error()
            torch.cuda.synchronize()
    # the bytes right behind and right in front of an image are still the fill
    off = mc.FAR_BASE + 4 * mc.FAR_STRIDE
    assert (raw[off + gc.FAR_IMAGE_BYTES:off + mc.FAR_DOWN_SHIFT] == 0xFF).all() and (raw[off - 4096:off] == 0xFF).all()
    up = _FarWeights(raw[mc.FAR_BASE:], gc.FAR_K, 2 * gc.FAR_I, 1)
    down = _FarWeights(raw[mc.FAR_BASE + mc.FAR_DOWN_SHIFT:], gc.FAR_K, gc.FAR_DOWN_N, 0)
    yield w1, w3, w2, up, down
    del up, down, raw
    arena.release()
    del arena
    torch.cuda.empty_cache()


def test_up_reads_int4_images_past_4_gib(gpu_device, far_images):
    """Experts 2 and 3 begin past 2^31 bytes from the first image, expert 4 past 2^32: an offset e * stride cut to 32 bits lands
    in 0xFF bytes (tests/test_moe_gptq_edges_cpu.py checks every such landing place): NaN scales."""
    from tgis_amd import native

    w1, w3, _w2, up, _down = far_images
    ids = torch.tensor(mc.FAR_IDS)
    T = ids.shape[0]
    r = _route_to(ids, mc.FAR_E, gpu_device)
    assert r.counts.tolist() == [2] * mc.FAR_E
    x = mb.up_input(T, gc.FAR_K, DT)
    h = native.moe_gptq_gemm_up(x.to(gpu_device), up, r)
    mb.close(h, *mb.up_reference(x, w1, w3, ids, DT), "far int4 images, up")


def test_down_reads_int4_images_past_4_gib(gpu_device, far_images):
    _w1, _w3, w2, _up, down = far_images
    ids = torch.tensor(mc.FAR_IDS)
    r = _route_to(ids, mc.FAR_E, gpu_device)
    h = mb.down_input(ids.shape[0], mc.FAR_TOP_K, gc.FAR_K, DT)
    _down_checks(gpu_device, h, down, r, w2, ids, "far int4 images,")
