"""-m gpu: the routed-expert kernels (csrc/moe.hip) on the code paths that tests/test_moe_ops_gpu.py's shapes do not reach,
each at the smallest shape that reaches it (tests/moe_cases.py holds the tables, tests/test_moe_edges_cpu.py checks without a
GPU that they reach what they claim):

  1. k-parts of more than MOE_RING = 4 k64-steps: the weight ring is refilled in place, once and twice per slot;
  2. K of one step or less per wave, and K tails that end in either half of a k64-step, the activations' pad holding NaN;
  3. every admitted kind of (E, top_k) through the gather, the slab address, the combine and the add + RMSNorm;
  4. row strides wider than the rows at the C entry points;
  5. route: more than 1024 tokens (a thread's second and third), E = 2 / 5 / 64, near-tied and underflowing probabilities,
     a NaN row among good ones;
  6. expert images whose byte offsets e * stride lie past 2^31 and 2^32, in an arena that holds NaN everywhere else.

References are tests/moe_ref.py in fp64 and the bounds are tests/moe_bounds.py's (one derivation with test_moe_ops_gpu.py, the
case's own K in it).  The images of experts nobody chose are filled with NaN."""
import ctypes

import pytest
import torch

from tests import far_pool as fp
from tests import moe_bounds as mb
from tests import moe_cases as mc
from tests import moe_ref

pytestmark = pytest.mark.gpu

DT_IDS = ("f16", "bf16")
E, TOP_K, HIDDEN = mc.E, mc.TOP_K, mc.HIDDEN
U32 = mb.U[torch.float32]

_IMAGES = {}


def _up_images(E_, I, K, dt, dev):
    """(w1, w3 on the CPU, gate|up images) of E_ experts, made once per shape and dtype."""
    key = ("up", E_, I, K, dt)
    if key not in _IMAGES:
        from tgis_amd import native

        w1, w3 = mb.up_weights(E_, I, K, dt)
        _IMAGES[key] = (w1, w3, native.MoeWeights(lambda e: torch.cat([w1[e], w3[e]]).to(dev), E_, gate_up=True))
    return _IMAGES[key]


def _down_images(E_, N, K, dt, dev, rows=None):
    """(w2 on the CPU, down images) of E_ experts; rows: only the first `rows` output rows of the same weights."""
    key = ("down", E_, N, K, dt, rows)
    if key not in _IMAGES:
        from tgis_amd import native

        w2 = mb.down_weights(E_, N, K, dt)[:, :rows]
        _IMAGES[key] = (w2, native.MoeWeights(lambda e: w2[e].to(dev), E_))
    return _IMAGES[key]


def _route_to(ids, E_, dev):
    """The kernel's routing of hand-written logits whose choices are `ids`."""
    from tgis_amd import native

    r = native.moe_route(mb.logits_for(ids, E_).to(dev), ids.shape[1])
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    return r


def _chosen(ids):
    return set(ids.reshape(-1).tolist())


def _check_up(dev, dt, K, I, T, ids, r, what):
    """The up GEMM over x [T, K] handed over as the first K columns of a wider NaN-filled matrix."""
    from tgis_amd import native

    E_ = r.E
    w1, w3, img = _up_images(E_, I, K, dt, dev)
    x = mb.up_input(T, K, dt)
    h = native.moe_gemm_up(mb.padded(x.to(dev), mc.K_PAD), mb.poisoned(img, _chosen(ids)), r)
    mb.close(h, *mb.up_reference(x, w1, w3, ids, dt), what + " up")
    return h


def _check_down(dev, dt, K, N, T, ids, r, what):
    """Both forms of the down GEMM over a random h [T top_k, K] in the model dtype, its pad columns NaN."""
    from tgis_amd import native

    top_k = ids.shape[1]
    w2, img = _down_images(r.E, N, K, dt, dev)
    img = mb.poisoned(img, _chosen(ids))
    h = mb.down_input(T, top_k, K, dt)
    hg = mb.padded(h.to(dev), mc.K_PAD)
    yref, ytol = mb.down_reference(h, w2, ids, r.expert_w.cpu())
    p = native.moe_gemm_down(hg, img, r, partial=True)
    assert p.S == top_k and p.shape == (T, N) and p.ld == mc.cdiv(N, 32) * 32
    mb.close(mb.slab_rows(p, T), yref, ytol, what + " down slabs")
    out = native.moe_gemm_down(hg, img, r, partial=False)
    mb.close(out, *mb.finished_reference(yref, ytol, dt), what + " down finished")
    assert torch.equal(mb.slab_sum(mb.slab_rows(p, T)).to(dt), out), what


# ---- 1. deep k: the ring's refill ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", mb.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", mc.DEEP_UP_K)
def test_up_refills_the_weight_ring(gpu_device, K, dt):
    ran = 0
    for T, name in mc.DEEP_ROWS:
        ids = mb.pattern(name, T)
        _check_up(gpu_device, dt, K, mc.DEEP_I, T, ids, _route_to(ids, E, gpu_device), f"K {K} {dt} T {T} {name}")
        ran += 1
    assert ran == len(mc.DEEP_ROWS) == 3


@pytest.mark.parametrize("dt", mb.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", mc.DEEP_DOWN_K)
def test_down_refills_the_weight_ring(gpu_device, K, dt):
    ran = 0
    for T, name in mc.DEEP_ROWS:
        ids = mb.pattern(name, T)
        _check_down(gpu_device, dt, K, mc.DEEP_DOWN_N, T, ids, _route_to(ids, E, gpu_device), f"K {K} {dt} T {T} {name}")
        ran += 1
    assert ran == len(mc.DEEP_ROWS) == 3


# ---- 2. short and ragged K ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", mb.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K", tuple(mc.SHORT_K))
def test_short_and_ragged_k(gpu_device, K, dt):
    """The lanes past K load a clamped column and are zeroed; the NaN behind column K of every row is never part of a sum."""
    ran = 0
    for T in mc.SHORT_TOKENS:
        ids = mb.pattern("uniform", T)
        r = _route_to(ids, E, gpu_device)
        _check_up(gpu_device, dt, K, mc.SHORT_I, T, ids, r, f"K {K} {dt} T {T}")
        _check_down(gpu_device, dt, K, mc.SHORT_DOWN_N, T, ids, r, f"K {K} {dt} T {T}")
        ran += 1
    assert ran == len(mc.SHORT_TOKENS) == 2


# ---- 3. every admitted top_k and E through the GEMMs ----------------------------------------------------------------------------
def _mix_route(dev, T, E_, top_k):
    """Seeded random logits through the route kernel: (r, ids), the ids checked against the restatement's."""
    from tgis_amd import native

    logits = mb.mix_logits(T, E_, top_k)
    r = native.moe_route(logits.to(dev), top_k)
    ids, _w = moe_ref.route(logits, top_k)
    assert torch.equal(r.expert_ids.cpu().long(), ids), f"T {T} E {E_} top_k {top_k}: ids"
    return r, ids


def _mix_images(dev, dt, E_, ids):
    w1, w3, up_w = _up_images(E_, mc.MIX_I, HIDDEN, dt, dev)
    w2, down_w = _down_images(E_, HIDDEN, mc.MIX_I, dt, dev)
    chosen = _chosen(ids)
    return w1, w3, w2, mb.poisoned(up_w, chosen), mb.poisoned(down_w, chosen)


@pytest.mark.parametrize("dt", mb.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("E_,top_k", mc.MIX_ROUTINGS, ids=lambda v: str(v))
def test_every_admitted_routing_through_the_gemms(gpu_device, E_, top_k, dt):
    from tgis_amd import native

    ran = 0
    for T in mc.MIX_TOKENS:
        what = f"E {E_} top_k {top_k} {dt} T {T}"
        r, ids = _mix_route(gpu_device, T, E_, top_k)
        w1, w3, w2, up_w, down_w = _mix_images(gpu_device, dt, E_, ids)
        if (E_, top_k, T) == (64, 2, 1):
            assert len(_chosen(ids)) == 2  # 62 images hold NaN
        x = mb.up_input(T, HIDDEN, dt)
        xg = x.to(gpu_device)
        h = native.moe_gemm_up(xg, up_w, r)
        assert h.shape == (T * top_k, mc.MIX_I)
        mb.close(h, *mb.up_reference(x, w1, w3, ids, dt), what + " up")

        p = native.moe_gemm_down(h, down_w, r, partial=True)
        assert p.S == top_k and p.shape == (T, HIDDEN) and p.ld == HIDDEN
        yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
        rows = mb.slab_rows(p, T)
        mb.close(rows, yref, ytol, what + " down slabs")
        out = native.moe_gemm_down(h, down_w, r, partial=False)
        mb.close(out, *mb.finished_reference(yref, ytol, dt), what + " down finished")
        # the deferred sum and the finished one are the same fp32 additions in the same order, k = 0..top_k-1
        assert torch.equal(mb.slab_sum(rows).to(dt), out), what

        # two runs, the same bytes
        h2 = native.moe_gemm_up(xg, up_w, r)
        p2 = native.moe_gemm_down(h2, down_w, r, partial=True)
        out2 = native.moe_gemm_down(h2, down_w, r, partial=False)
        assert torch.equal(h, h2) and torch.equal(rows, mb.slab_rows(p2, T)) and torch.equal(out, out2), what
        ran += 1
    assert ran == len(mc.MIX_TOKENS) == 3


@pytest.mark.parametrize("dt", mb.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("top_k", mc.NORM_TOP_K)
def test_partial_of_any_top_k_into_the_norm(gpu_device, top_k, dt):
    """A Partial with S = top_k slabs through rmsnorm_residual (sum_slabs8's buckets of 1, 4 and 8): within the propagated
    bound of the reference, and bit for bit what the norm gives on the finished form's tensor."""
    from tgis_amd import native

    T, eps = mc.NORM_T, 1e-5
    r, ids = _mix_route(gpu_device, T, E, top_k)
    w1, w3, w2, up_w, down_w = _mix_images(gpu_device, dt, E, ids)
    gen = torch.Generator().manual_seed(77 + top_k)
    residual = torch.randn(T, HIDDEN, generator=gen).to(dt)
    weight = (1.0 + 0.1 * torch.randn(HIDDEN, generator=gen)).to(dt)
    h = native.moe_gemm_up(mb.up_input(T, HIDDEN, dt).to(gpu_device), up_w, r)
    p = native.moe_gemm_down(h, down_w, r, partial=True)
    assert p.S == top_k
    out = native.moe_gemm_down(h, down_w, r, partial=False)
    y_p, res_p = native.rmsnorm_residual(p, residual.to(gpu_device), weight.to(gpu_device), eps)
    y_f, res_f = native.rmsnorm_residual(out, residual.to(gpu_device), weight.to(gpu_device), eps)
    assert torch.equal(y_p, y_f) and torch.equal(res_p, res_f)
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, eps, dt)
    mb.close(res_p, res, dres, f"top_k {top_k} {dt} residual stream")
    mb.close(y_p, y, dy, f"top_k {top_k} {dt} normed")


@pytest.mark.parametrize("T", mc.SLAB_TOKENS)
@pytest.mark.parametrize("top_k", mc.SLAB_TOP_K)
def test_slabs_of_one_and_three_choices_are_written_where_they_belong(gpu_device, top_k, T):
    """The slab form into a NaN-filled buffer: every (t, k) row of every slab is finite in its N columns afterwards, and the
    rows past T and the pad columns are untouched."""
    from tgis_amd import native

    dt, N = torch.float16, mc.SLAB_N
    lib = native.load_library()
    r, ids = _mix_route(gpu_device, T, E, top_k)
    _w1, _w3, _w2, up_w, _down = _mix_images(gpu_device, dt, E, ids)
    w2, narrow = _down_images(E, HIDDEN, mc.MIX_I, dt, gpu_device, rows=N)  # a down projection with an N tail (ld 320)
    narrow = mb.poisoned(narrow, _chosen(ids))
    h = native.moe_gemm_up(mb.up_input(T, HIDDEN, dt).to(gpu_device), up_w, r)
    nbytes = lib.tgis_moe_gemm_down_bytes(T, N, top_k, 0)
    ld = mc.cdiv(N, 32) * 32
    assert nbytes == mc.cdiv(T, 32) * top_k * 32 * ld * 4
    slabs = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=gpu_device)
    rc = lib.tgis_moe_gemm_down(h.data_ptr(), h.stride(0), narrow.image.data_ptr(), narrow.stride, r.offsets.data_ptr(),
                                r.slot_rows.data_ptr(), r.expert_w.data_ptr(), T, mc.MIX_I, N, E, top_k, native.F16, 0,
                                slabs.data_ptr(), nbytes, None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.tgis_last_error()
    torch.cuda.synchronize()
    s = slabs.view(-1, top_k, 32, ld).permute(0, 2, 1, 3).reshape(-1, top_k, ld).cpu()
    assert torch.isfinite(s[:T, :, :N]).all()
    assert torch.isnan(s[T:]).all() and torch.isnan(s[:, :, N:]).all()
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    mb.close(s[:T, :, :N], yref, ytol, f"top_k {top_k} T {T} N {N} slabs")


# ---- 4. row strides at the C entry points ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", mb.DTYPES, ids=DT_IDS)
def test_row_strides_wider_than_the_rows(gpu_device, dt):
    """x with ldx = K + 8 out of a NaN-filled matrix, h written with ldh = I + 16 into a NaN-filled buffer and read back with
    that stride by the down GEMM, the finished rows written with ldo = N + 4: the values hold their bounds and every pad
    column still holds NaN."""
    from tgis_amd import native

    T, I, pads = mc.STRIDE_T, mc.STRIDE_I, mc.STRIDE_PADS
    lib, code = native.load_library(), native.dtype_code(dt)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ids = mb.pattern("uniform", T)
    r = _route_to(ids, E, gpu_device)
    w1, w3, up_w = _up_images(E, I, HIDDEN, dt, gpu_device)
    w2, down_w = _down_images(E, HIDDEN, I, dt, gpu_device)
    up_w, down_w = mb.poisoned(up_w, _chosen(ids)), mb.poisoned(down_w, _chosen(ids))
    x = mb.up_input(T, HIDDEN, dt)
    xg = mb.padded(x.to(gpu_device), pads["x"])
    assert xg.stride(0) == HIDDEN + 8
    hbuf = torch.full((T * TOP_K, I + pads["h"]), float("nan"), dtype=dt, device=gpu_device)
    rc = lib.tgis_moe_gemm_up(xg.data_ptr(), xg.stride(0), up_w.image.data_ptr(), up_w.stride, r.offsets.data_ptr(),
                              r.slot_rows.data_ptr(), hbuf.data_ptr(), hbuf.stride(0), T, HIDDEN, 2 * I, E, TOP_K, code, stream)
    assert rc == 0, lib.tgis_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(hbuf[:, I:]).all(), "the up GEMM wrote into the pad of h"
    h = hbuf[:, :I]
    mb.close(h, *mb.up_reference(x, w1, w3, ids, dt), f"{dt} strided up")

    N = HIDDEN
    nbytes = lib.tgis_moe_gemm_down_bytes(T, N, TOP_K, 1)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=gpu_device)
    obuf = torch.full((T, N + pads["out"]), float("nan"), dtype=dt, device=gpu_device)
    rc = lib.tgis_moe_gemm_down(hbuf.data_ptr(), hbuf.stride(0), down_w.image.data_ptr(), down_w.stride, r.offsets.data_ptr(),
                                r.slot_rows.data_ptr(), r.expert_w.data_ptr(), T, I, N, E, TOP_K, code, 1, scratch.data_ptr(),
                                nbytes, obuf.data_ptr(), obuf.stride(0), stream)
    assert rc == 0, lib.tgis_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(obuf[:, N:]).all(), "the finished form wrote into the pad of out"
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    mb.close(obuf[:, :N], *mb.finished_reference(yref, ytol, dt), f"{dt} strided down")


# ---- 5. route -------------------------------------------------------------------------------------------------------------------
def _route_twice(dev, logits_dev, logits_cpu, E_, top_k):
    from tgis_amd import native

    r = native.moe_route(logits_dev, top_k)
    mb.check_routing(logits_cpu, r, E_, top_k)
    again = native.moe_route(logits_dev, top_k)
    for name in ("expert_ids", "expert_w", "lists", "slot_rows"):
        assert torch.equal(getattr(r, name), getattr(again, name)), name
    return r


@pytest.mark.parametrize("E_,top_k", mc.EDGE_ROUTE_CASES, ids=lambda v: str(v))
def test_route_of_more_tokens_than_threads(gpu_device, E_, top_k):
    ran = 0
    for T in mc.EDGE_ROUTE_TOKENS:
        logits = mb.mix_logits(T, E_, top_k)
        _route_twice(gpu_device, logits.to(gpu_device), logits, E_, top_k)
        ran += 1
    assert ran == len(mc.EDGE_ROUTE_TOKENS) == 4


@pytest.mark.parametrize("E_,top_k", mc.EDGE_ROUTE_SMALL, ids=lambda v: str(v))
def test_route_of_a_single_choice_at_the_expert_limits(gpu_device, E_, top_k):
    ran = 0
    for T in mc.EDGE_ROUTE_SMALL_TOKENS:
        logits = mb.mix_logits(T, E_, top_k)
        _route_twice(gpu_device, logits.to(gpu_device), logits, E_, top_k)
        ran += 1
    assert ran == 2


def test_route_reads_64_experts_from_rows_80_apart(gpu_device):
    E_, top_k, ld = mc.EDGE_ROUTE_STRIDED
    wide = torch.randn(1025, ld, generator=torch.Generator().manual_seed(64))
    view = wide.to(gpu_device)[:, :E_]
    assert view.stride(0) == ld
    _route_twice(gpu_device, view, wide[:, :E_], E_, top_k)


def _rows_by_top_k(table):
    """{top_k: (logits [n, 8], wanted ids [n, top_k])} of a table of hand-written rows whose last entry is the ids."""
    out = {}
    for row in table:
        out.setdefault(row[1], []).append(row)
    return {k: (torch.tensor([r[0] for r in rows], dtype=torch.float32), torch.tensor([r[-1] for r in rows]))
            for k, rows in out.items()}


def test_route_near_ties_go_to_the_lower_index(gpu_device):
    """Logits that differ in fp32 and whose probabilities differ only in fp64: the order is decided on the fp32 probabilities,
    so the lower index wins although the higher ones hold the larger logits."""
    seen = 0
    for top_k, (logits, want) in _rows_by_top_k(mc.NEAR_TIES).items():
        r = _route_twice(gpu_device, logits.to(gpu_device), logits, E, top_k)
        assert r.expert_ids.cpu().long().tolist() == want.tolist()
        seen += logits.shape[0]
        for n, (_l, _k, tied, ids) in enumerate(row for row in mc.NEAR_TIES if row[1] == top_k):
            if set(ids) <= set(tied):  # every choice inside the tie: equal shares, within 4 ulp below 1 / top_k
                err = (r.expert_w[n].cpu().double() - 1.0 / top_k).abs()
                assert (err <= 4 * U32 / 2).all(), f"row {n} top_k {top_k}: weights {r.expert_w[n].tolist()}"
    assert seen == len(mc.NEAR_TIES)


def test_route_underflowing_probabilities(gpu_device):
    """One dominant logit, every other fp32 probability 0: the later choices are ties at zero and go to the lowest free
    index; their weights (below 2^-150) round to 0 and the dominant one's to 1."""
    seen = 0
    for top_k, (logits, want) in _rows_by_top_k(mc.UNDERFLOW).items():
        r = _route_twice(gpu_device, logits.to(gpu_device), logits, E, top_k)
        assert r.expert_ids.cpu().long().tolist() == want.tolist()
        w = r.expert_w.cpu()
        assert (w[:, 0] == 1.0).all() and (w[:, 1:] == 0.0).all(), w.tolist()
        seen += logits.shape[0]
    assert seen == len(mc.UNDERFLOW)


def test_route_keeps_a_nan_row_inside_the_lists(gpu_device):
    """Route only (no GEMM runs on this): a row of NaN and a row with one NaN among good rows.  No comparison with NaN is
    true, so such a row takes the first untaken indices: every id stays in range and distinct, the lists stay a grouping of
    all slots, and every other row is the reference's."""
    from tgis_amd import native

    T, top_k = 70, 3
    logits = mb.mix_logits(T, E, top_k)
    bad = (5, 37)
    logits[bad[0]] = float("nan")
    logits[bad[1], 3] = float("nan")
    r = native.moe_route(logits.to(gpu_device), top_k)
    ids = r.expert_ids.cpu().long()
    assert ((ids >= 0) & (ids < E)).all()
    assert all(len(set(row)) == top_k for row in ids.tolist())
    counts, offsets, slot_rows = r.counts.cpu().long(), r.offsets.cpu().long(), r.slot_rows.cpu().long()
    assert int(counts.sum()) == T * top_k
    assert torch.equal(offsets[1:], torch.cumsum(counts, 0)) and int(offsets[0]) == 0
    assert torch.equal(torch.sort(slot_rows).values, torch.arange(T * top_k))
    flat = ids.reshape(-1)
    for e in range(E):
        mine = slot_rows[int(offsets[e]):int(offsets[e + 1])]
        assert (flat[mine] == e).all() and (mine[1:] > mine[:-1]).all(), f"expert {e}"
    good = [t for t in range(T) if t not in bad]
    want_ids, want_w = moe_ref.route(logits[good], top_k)
    assert torch.equal(ids[good], want_ids)
    mb.check_weights(r.expert_w.cpu()[good], want_w)


# ---- 6. expert images past 2^31 and 2^32 bytes ----------------------------------------------------------------------------------
class _FarWeights:
    """What native.moe_gemm_up / _down read of a MoeWeights: the image is a view of the arena, the stride the wide one."""

    def __init__(self, image, N, K, flags):
        self.image, self.N, self.K, self.flags = image, N, K, flags
        self.E, self.stride, self.dtype = mc.FAR_E, mc.FAR_STRIDE, torch.float16


@pytest.fixture(scope="module")
def far_images(gpu_device):
    """Five gate|up images and, FAR_DOWN_SHIFT bytes behind each, five down images, written by tgis_dense_prepare straight
    into their places in a NaN-filled arena: (w1, w3, w2, up images, down images)."""
    from tgis_amd import native

    lib, dt = native.load_library(), torch.float16
    arena = fp.Arena(gpu_device, mc.FAR_ARENA_BYTES)
    arena.fill(dt)
    raw = arena.typed(torch.uint8)
    w1, w3 = mb.up_weights(mc.FAR_E, mc.FAR_I, mc.FAR_K, dt)
    w2 = mb.down_weights(mc.FAR_E, mc.FAR_DOWN_N, mc.FAR_K, dt)
    assert lib.tgis_dense_prepared_bytes(2 * mc.FAR_I, mc.FAR_K) == mc.FAR_IMAGE_BYTES
    assert lib.tgis_dense_prepared_bytes(mc.FAR_DOWN_N, mc.FAR_K) == mc.FAR_IMAGE_BYTES
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for e in range(mc.FAR_E):
        for shift, w, flags in ((0, torch.cat([w1[e], w3[e]]), 1), (mc.FAR_DOWN_SHIFT, w2[e], 0)):
            wg = w.to(gpu_device).contiguous()
            off = mc.FAR_BASE + shift + e * mc.FAR_STRIDE
            assert off + mc.FAR_IMAGE_BYTES <= arena.nbytes
            rc = lib.tgis_dense_prepare(wg.data_ptr(), wg.shape[0], wg.shape[1], native.F16, flags, raw.data_ptr() + off, stream)
            assert rc == 0, lib.tgis_last_error()
            torch.cuda.synchronize()
    up = _FarWeights(raw[mc.FAR_BASE:], 2 * mc.FAR_I, mc.FAR_K, 1)
    down = _FarWeights(raw[mc.FAR_BASE + mc.FAR_DOWN_SHIFT:], mc.FAR_DOWN_N, mc.FAR_K, 0)
    yield w1, w3, w2, up, down
    del up, down, raw
    arena.release()
    del arena
    torch.cuda.empty_cache()


def test_up_reads_expert_images_past_4_gib(gpu_device, far_images):
    """Experts 2 and 3 begin past 2^31 bytes from the first image, expert 4 past 2^32: an offset e * stride cut to 32 bits lands
    in NaN (tests/test_moe_edges_cpu.py checks every such landing place)."""
    from tgis_amd import native

    w1, w3, _w2, up, _down = far_images
    dt, ids = torch.float16, torch.tensor(mc.FAR_IDS)
    T = ids.shape[0]
    r = _route_to(ids, mc.FAR_E, gpu_device)
    assert r.counts.tolist() == [2] * mc.FAR_E
    x = mb.up_input(T, mc.FAR_K, dt)
    h = native.moe_gemm_up(x.to(gpu_device), up, r)
    mb.close(h, *mb.up_reference(x, w1, w3, ids, dt), "far images, up")


def test_down_reads_expert_images_past_4_gib(gpu_device, far_images):
    from tgis_amd import native

    _w1, _w3, w2, _up, down = far_images
    dt, ids = torch.float16, torch.tensor(mc.FAR_IDS)
    T = ids.shape[0]
    r = _route_to(ids, mc.FAR_E, gpu_device)
    h = mb.down_input(T, mc.FAR_TOP_K, mc.FAR_K, dt)
    yref, ytol = mb.down_reference(h, w2, ids, r.expert_w.cpu())
    p = native.moe_gemm_down(h.to(gpu_device), down, r, partial=True)
    mb.close(mb.slab_rows(p, T), yref, ytol, "far images, down slabs")
    out = native.moe_gemm_down(h.to(gpu_device), down, r, partial=False)
    mb.close(out, *mb.finished_reference(yref, ytol, dt), "far images, down finished")
