"""-m gpu: the int4 tile expert GEMMs (csrc/moe_gptq_tiles.h: tgis_moe_gptq_tile_gemm_up, tgis_moe_gptq_tile_gemm_down) over a
routing of tgis_moe_route_tiles, against the fp64 restatement on the dequantised weights.  The weights dequantise exactly
(tests/moe_gptq_cases.py), so the references and per-element bounds are tests/moe_bounds.py's with no new constant.

Rows: test_moe_tiles_ops_gpu's routing (experts of 0, 1, 63, 64, 65 and 130 rows: a tile one row short, full, one row over,
and two tiles and two rows).  Shapes: one k64-step with three idle waves (N 32), a group change every step and a column block with one live
wave (N 160), groups of 2 and 4 steps, and 17 steps: past the weight ring and across the image's 256-row chunk padding.  The
images of experts nobody chose are 0xFF bytes."""
import ctypes

import pytest
import torch

from tests import moe_bounds as mb
from tests import moe_gptq_cases as gc
from tests.test_moe_tiles_ops_gpu import _row_count_ids

pytestmark = pytest.mark.gpu

DT = torch.float16
UP_CASES = [(64, 16, 64), (320, 80, 64), (512, 48, 128), (512, 48, 256), (1088, 16, -1), (1088, 16, 64)]
DOWN_N = (64, 160, 640)


def _route(ids, E, dev):
    from tgis_amd import native

    r = native.moe_route_tiles(mb.logits_for(ids, E).to(dev), ids.shape[1])
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    return r


def _check_up(dev, ids, K, I, gs, E=gc.E):
    from tgis_amd import native

    bundles, w1, w3 = gc.up_experts(K, I, gs, E)
    mw = gc.poisoned(gc.moe_weights(bundles, gs, dev, gate_up=True), set(ids.reshape(-1).tolist()))
    x = mb.up_input(ids.shape[0], K, DT)
    r = _route(ids, E, dev)
    ref, tol = mb.up_reference(x, w1, w3, ids, DT)
    h = native.moe_gptq_tile_gemm_up(x.to(dev), mw, r)
    mb.close(h, ref, tol, f"up K {K} I {I} gs {gs} T {ids.shape[0]}")
    assert torch.equal(h, native.moe_gptq_tile_gemm_up(x.to(dev), mw, r)), "two runs, the same bytes"


def _check_down(dev, ids, K, N, gs, E=gc.E):
    from tgis_amd import native

    T, top_k = ids.shape
    bundles, w2 = gc.down_experts(K, N, gs, E)
    mw = gc.poisoned(gc.moe_weights(bundles, gs, dev), set(ids.reshape(-1).tolist()))
    h = mb.down_input(T, top_k, K, DT)
    r = _route(ids, E, dev)
    yref, ytol = mb.down_reference(h, w2, ids, r.expert_w.cpu())
    gen = torch.Generator().manual_seed(77)
    residual = torch.randn(T, N, generator=gen).to(DT)
    weight = (1.0 + 0.1 * torch.randn(N, generator=gen)).to(DT)
    what = f"down K {K} N {N} gs {gs} T {T}"
    out = native.moe_gptq_tile_gemm_down(h.to(dev), mw, r, partial=False)
    mb.close(out, *mb.finished_reference(yref, ytol, DT), what + " finished")
    assert torch.equal(out, native.moe_gptq_tile_gemm_down(h.to(dev), mw, r, partial=False)), what + ": the same bytes"
    p = native.moe_gptq_tile_gemm_down(h.to(dev), mw, r, partial=True)
    assert isinstance(p, native.Partial) and p.S == top_k and p.shape == (T, N) and p.ld == N
    slabs = mb.slab_rows(p, T)
    mb.close(slabs, yref, ytol, what + " slabs")
    assert torch.equal(mb.slab_sum(slabs).to(DT), out), what + ": the deferred sum is the finished one"
    # the slab form finished by the add + RMSNorm behind the block
    y_p, res_p = native.rmsnorm_residual(p, residual.to(dev), weight.to(dev), 1e-5)
    res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, 1e-5, DT)
    mb.close(res_p, res, dres, what + " residual stream")
    mb.close(y_p, y, dy, what + " normed")


@pytest.mark.parametrize("K,I,gs", UP_CASES, ids=lambda v: str(v))
def test_up_at_every_row_count(gpu_device, K, I, gs):
    _check_up(gpu_device, _row_count_ids(), K, I, gs)


@pytest.mark.parametrize("N", DOWN_N)
@pytest.mark.parametrize("K,gs", [(K, gs) for K, _I, gs in UP_CASES], ids=lambda v: str(v))
def test_down_at_every_row_count(gpu_device, K, gs, N):
    _check_down(gpu_device, _row_count_ids(), K, N, gs)


def test_over_128_experts(gpu_device):
    g = torch.Generator().manual_seed(33)  # [33, 8] over 128 experts: most tiles hold 0 - 3 rows
    ids = torch.stack([torch.randperm(128, generator=g)[:8] for _ in range(33)])
    _check_up(gpu_device, ids, 128, 48, 64, E=128)
    _check_down(gpu_device, ids, 128, 160, 64, E=128)


def test_entry_points_refuse_without_launching(gpu_device):
    """K 96, N 48, groups of 32 rows, bf16, a stride 16 bytes short and a tile bound below tgis_moe_tile_bound: an error code,
    and outputs filled with NaN stay NaN."""
    from tgis_amd import native

    lib, dev, T, E, top_k = native.load_library(), gpu_device, 8, gc.E, gc.TOP_K
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = _route(mb.pattern("uniform", T), E, dev)
    image = torch.zeros(E * (1 << 20), dtype=torch.uint8, device=dev)
    x = torch.ones((T * top_k, 1024), dtype=DT, device=dev)
    out = torch.full((T * top_k, 1024), float("nan"), dtype=DT, device=dev)
    scratch = torch.full((T * top_k * 1024,), float("nan"), dtype=torch.float32, device=dev)

    def up(K, N, G, stride=1 << 20, dtype=native.F16, bound=r.tile_bound):
        return lib.tgis_moe_gptq_tile_gemm_up(x.data_ptr(), 1024, image.data_ptr(), stride, r.offsets.data_ptr(),
                                              r.slot_rows.data_ptr(), r.tiles.data_ptr(), bound, out.data_ptr(), 1024, T, K, N,
                                              G, E, top_k, dtype, stream)

    def down(K, N, G, stride=1 << 20, dtype=native.F16, bound=r.tile_bound):
        return lib.tgis_moe_gptq_tile_gemm_down(x.data_ptr(), 1024, image.data_ptr(), stride, r.offsets.data_ptr(),
                                                r.slot_rows.data_ptr(), r.tiles.data_ptr(), bound, r.expert_w.data_ptr(), T, K,
                                                N, G, E, top_k, dtype, 0, scratch.data_ptr(), scratch.numel() * 4,
                                                out.data_ptr(), 1024, stream)

    small = lib.tgis_gptq_prepared_bytes(320, 64, 5) - 16
    for fn in (up, down):
        for bad in (dict(K=96, N=64, G=1), dict(K=320, N=48, G=5), dict(K=320, N=64, G=10), dict(K=320, N=64, G=5, stride=small),
                    dict(K=320, N=64, G=5, dtype=native.BF16), dict(K=320, N=64, G=5, bound=r.tile_bound - 1)):
            assert fn(**bad) != 0, (fn.__name__, bad)
            assert lib.tgis_last_error()
            lib.tgis_clear_error()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(scratch).all()
    # the same calls at a served shape launch (zero images: finite outputs)
    assert up(320, 64, 5, stride=small + 16) == 0 and down(320, 64, 5, stride=small + 16) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:, :32]).all()
