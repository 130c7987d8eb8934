"""-m gpu: the GELU finish of the int4 GEMM (tgis_gptq_gemm_f16 act 4: erf form, act 5: tanh approximation).

For every M in ROWS x (K, N) in SHAPES x groups in {1, K / 64} x act-order x bias x GELU form:
  1. the result has the bits of gptq_gemm(act 0) followed by native.gelu (the plan is the one of act 0 and the activation
     reads the rounded sum back, as tgis_gelu would);
  2. it is within the bound tests/test_gemm_edges_gpu.py::_reference defines for the dense act 4 / 5, against the fp64
     reference on oracle.ops_ref.gptq_dequant weights (rounded to f16 once, as the kernels round (q - z) * s);
  3. out is a [M, N] view (ldo = N + 32) into a NaN-filled buffer whose padding stays NaN.
SHAPES are the smallest at which each finishing path and edge occurs: (256, 1024) the tiny model's c_fc, unsplit; (256, 96)
three column tiles, fewer than a block's; (4096, 64) splits over k at every row count (the reduce applies the GELU; checked
with tgis_debug_gemm_plan); (1024, 2080) 65 column tiles, a ragged last block.  ROWS are the edges of the 32-row blocks and
the 64-row passes, up to the 256 rows the forms serve.  Then the refusals, and Ex4bitLinearV2.forward_gelu."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
import test_gemm_edges_gpu as edges  # noqa: E402

from oracle import ops_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 64, 65, 96, 256)
SHAPES = ((256, 1024), (256, 96), (4096, 64), (1024, 2080))
WEIGHTS = [(K, N, groups, ao) for K, N in SHAPES for groups in (1, K // 64) for ao in (False, True)]


def _weight(K, N, groups, ao, dev, gate_up=False):
    """(GptqWeight, W [K, N] fp64 on the device, the checkpoint tensors)."""
    from tgis_amd import native

    gs = K // groups
    qw, qz, sc, gi = ops_ref.make_gptq_tensors(K, N, gs, seed=K + N + groups + ao, act_order=ao, w_std=0.05)
    W = ops_ref.gptq_dequant(qw, qz, sc, gi if ao else None, gs).half().double().to(dev)
    t = (torch.from_numpy(qw).to(dev), torch.from_numpy(qz).to(dev), torch.from_numpy(sc).to(dev),
         torch.from_numpy(gi) if ao else None)
    w = native.GptqWeight(*t, 4, gs, gate_up=gate_up)
    assert (w.perm is not None) == (ao and groups > 1)  # one group: every g_idx is the trivial map, no permutation
    return w, W, t


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("K,N,groups,ao", WEIGHTS, ids=[f"K{K}-N{N}-g{g}{'-ao' if ao else ''}" for K, N, g, ao in WEIGHTS])
def test_gelu_finish_has_the_bits_of_two_launches_and_meets_the_reference(gpu_device, K, N, groups, ao):
    from tgis_amd import native
    from tgis_amd.utils.layers import workspace

    dev, lib = gpu_device, native.load_library()
    gen = torch.Generator(device=dev).manual_seed(K * 31 + N)
    w, W, _ = _weight(K, N, groups, ao, dev)
    bias_t = (torch.randn(N, generator=gen, device=dev) * 0.5).half()
    ws = workspace(dev)
    seen = set()
    for M in ROWS:
        plan = gc.plan_fields(gc.query_plan(lib, "gptq", M, K, N, groups, 4, w.perm is not None))
        assert plan["family"] == "stream" and plan["gelu"] == 1 and plan["act"] == 0
        if K == 4096:
            assert plan["s"] > 1, f"(4096, 64) at M = {M} no longer splits over k: pick another shape"
        if K == 256:
            assert plan["s"] == 1
        seen.add((plan["s"] > 1, plan["mr"]))
        xbuf, x = edges._nan_view(M, K, 3, 64, torch.float16, dev)
        x.copy_(edges._activation(M, K, torch.float16, gen, dev))
        for bias in (None, bias_t):
            plain = native.gptq_gemm(x, w, ws, bias=bias, act=0)
            c = {"K": K, "N": N}
            for act, tanh in ((4, False), (5, True)):
                what = f"M={M} K={K} N={N} groups={groups} act-order={ao} bias={bias is not None} act={act}"
                buf, out = edges._nan_view(M, N, 3, 32, torch.float16, dev)
                native.gptq_gemm(x, w, ws, bias=bias, act=act, out=out)
                two = native.gelu(plain, tanh)
                assert torch.equal(_bits(out), _bits(two)), \
                    f"{what}: {int((_bits(out) != _bits(two)).sum())} elements differ from act 0 + tgis_gelu"
                ref, tol = edges._reference(dict(c, act=act), x, W, bias, torch.float16)
                err = (out.double() - ref).abs()
                print(f"{what}: max |got - ref| = {err.max().item():.3e}, max err / tol = {(err / tol).max().item():.3f}")
                edges._check(out, ref, tol, what)
                assert torch.isnan(buf[M:]).all() and torch.isnan(buf[:M, N:]).all(), f"{what}: wrote outside [M, N]"
        assert torch.isnan(xbuf[M:]).all()
    assert {mr for _, mr in seen} == {1, 2}, seen


def test_refused_forms_name_themselves(gpu_device):
    from tgis_amd import native
    from tgis_amd.utils.layers import workspace

    dev, lib = gpu_device, native.load_library()
    K, N, groups = 256, 1024, 4
    w, _, t = _weight(K, N, groups, False, dev)
    ws = workspace(dev)
    x = torch.zeros((32, K), dtype=torch.float16, device=dev)
    out = torch.empty((32, N), dtype=torch.float16, device=dev)
    ws.ensure(w.workspace_bytes(32))
    for act in (4, 5):
        # fragment-order activation / output (native.gptq_gemm asserts before the library is asked: call it directly)
        xf = native.FragAct.from_rows(x)
        for ldx, ldo, xp in ((native.LD_FRAGMENTS, N, xf.buf.data_ptr()), (K, native.LD_FRAGMENTS, x.data_ptr())):
            with pytest.raises(native.TgisHipError, match=r"act 4 / 5 \(GELU\) take a row-major activation.*fragment order"):
                native._check(lib.tgis_gptq_gemm_f16(xp, ldx, w.image.data_ptr(), None, None, out.data_ptr(), ldo, 32, K, N,
                                                     groups, act, ws.ptr, ws.nbytes, None), "tgis_gptq_gemm_f16")
        with pytest.raises(AssertionError, match="row-major"):
            native.gptq_gemm(xf, w, ws, act=act)
        with pytest.raises(native.TgisHipError, match=r"tgis_gptq_gemm_f16_partial: act 4 / 5 \(GELU\) need the finished sum"):
            native.gptq_gemm_partial(x, w, act=act)
        with pytest.raises(native.TgisHipError, match=r"act 4 / 5 \(GELU\) serve up to 256 rows"):
            native.gptq_gemm(torch.zeros((257, K), dtype=torch.float16, device=dev), w, ws, act=act)
    wg = native.GptqWeight(*t, 4, K // groups, gate_up=True)
    for act in (4, 5):
        with pytest.raises(native.TgisHipError, match=r"act 4 / 5 \(GELU\) on a gate\|up image"):
            native.gptq_gemm(x, wg, ws, act=act)
    # nothing above left an error behind or touched the output path: the plain call still works
    native.gptq_gemm(x, w, ws, act=4, out=out)
    torch.cuda.synchronize()


@pytest.mark.parametrize("ao", [False, True], ids=["", "act-order"])
def test_forward_gelu_of_the_int4_linear(gpu_device, monkeypatch, ao):
    """One launch up to q.fused_rows(4) = 256 rows, GEMM then tgis_gelu above and with TGIS_FUSED_GELU_GEMM off: the same
    bits either way."""
    from tgis_amd import native
    from tgis_amd.utils import layers

    dev = gpu_device
    K, N, groups = 256, 1024, 4
    qw, qz, sc, gi = ops_ref.make_gptq_tensors(K, N, K // groups, seed=5, act_order=ao, w_std=0.05)
    gen = torch.Generator(device=dev).manual_seed(17)
    bias = (torch.randn(N, generator=gen, device=dev) * 0.5).half()
    lin = layers.Ex4bitLinearV2(torch.from_numpy(qw).to(dev), torch.from_numpy(qz).to(dev), torch.from_numpy(sc).to(dev),
                                torch.from_numpy(gi), bias, 4, K // groups)
    calls = []
    real_gelu, real_gemm = native.gelu, native.gptq_gemm
    monkeypatch.setattr(native, "gelu", lambda *a, **kw: (calls.append("gelu"), real_gelu(*a, **kw))[1])
    monkeypatch.setattr(native, "gptq_gemm", lambda *a, **kw: (calls.append(("gemm", kw.get("act", 0))), real_gemm(*a, **kw))[1])
    for rows in (1, 64, 256, 300):
        x = edges._activation(rows, K, torch.float16, gen, dev)
        for tanh in (False, True):
            two = real_gelu(lin.forward(x), tanh)
            assert lin.q_handle.fused_rows(4) == 256
            del calls[:]
            monkeypatch.setattr(layers, "FUSED_GELU_GEMM", True)
            got = lin.forward_gelu(x, tanh)
            if rows <= 256:
                assert calls == [("gemm", 5 if tanh else 4)], (rows, calls)
            else:  # the tall kernel (act 0) or, with act-order, dequantise + library GEMM; then tgis_gelu
                assert calls in ([("gemm", 0), "gelu"], ["gelu"]), (rows, calls)
            assert torch.equal(_bits(got), _bits(two)), (rows, tanh)
            del calls[:]
            monkeypatch.setattr(layers, "FUSED_GELU_GEMM", False)
            off = lin.forward_gelu(x, tanh)
            assert calls in ([("gemm", 0), "gelu"], ["gelu"]) and (rows > 256 or len(calls) == 2), (rows, calls)
            assert torch.equal(_bits(off), _bits(two)), (rows, tanh)
