"""GPU: the 8-bit GPTQ tile GEMM (tgis_gptq8_tile_gemm_f16, csrc/gptq8_tiles.h) on its own, against fp64 on the exact
dequantised weights with the bound of tests/test_gemm_edges_gpu.py:
  |got - ref| <= 2 u16 |ref| + 2 K 2^-24 (|x| @ |W|) + 2^-24
The weights are those tests/test_gptq8_ops_gpu.py builds (and checks bit for bit against the dequantisation).  x is a strided
view in a NaN buffer, out a view in a NaN buffer whose margins must stay NaN, and a second call gives identical bits."""
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gemm_edges_gpu import _activation, _check, _nan_view, _reference  # noqa: E402
from test_gptq8_ops_gpu import _weight  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (M, K, N, groups, weight form, pads, bias) -> the kernel instance <rows per tile, columns per block, PERM> it reaches.
# Tiles are 64 rows up to M = 128 and 128 above; blocks are 128 columns wide from 256 column tiles (N >= 8192) on, 64 below.
CASES = [
    (1, 128, 64, 1, "plain", 0, False),         # <64, 64, plain>   one group, one row, fewer k64-steps than the ring
    (63, 128, 64, 2, "act_order", 0, True),     # <64, 64, PERM>    one tile, not full
    (128, 128, 64, 4, "plain", 0, True),        # <64, 64, plain>   two full tiles
    (65, 96, 32, 2, "plain", 0, True),          # <64, 64, plain>   a one-row last tile; a k64 tail over non-zero pad bytes;
    #                                                               one column tile: the block's second pair of waves idles
    (129, 96, 32, 2, "perm", 24, False),        # <128, 64, PERM>   a one-row last tile; 24 gather entries of -1
    (257, 1568, 64, 98, "plain", 0, False),     # <128, 64, plain>  three tiles; 25 k64-steps: the odd part ends a step early
    (128, 4096, 96, 32, "perm", 24, True),      # <64, 64, PERM>    64 k64-steps; 3 column tiles: a half-empty last block
    (257, 4096, 96, 32, "perm", 24, False),     # <128, 64, PERM>
    (65, 96, 8224, 2, "plain", 0, True),        # <64, 128, plain>  257 column tiles: a one-tile last block
    (129, 96, 8224, 2, "plain", 0, False),      # <128, 128, plain>
    (128, 1312, 8224, 82, "act_order", 0, False),  # <64, 128, PERM>   groups of 16 rows, a k64 tail
    (257, 1312, 8224, 82, "act_order", 0, True),   # <128, 128, PERM>  three tiles
]


@pytest.mark.parametrize("M,K,N,G,mode,pads,with_bias", CASES)
def test_tile_gemm(M, K, N, G, mode, pads, with_bias):
    from tgis_amd import native

    lib = native.load_library()
    what = f"M{M} K{K} N{N} G{G} {mode}"
    w, _, Wx = _weight(K, N, G, mode, pads)
    assert (w.perm is not None) == (mode != "plain")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32(what.encode()))
    cols = w.in_features
    xv = _activation(M, cols, torch.float16, gen, DEV)
    xbuf, x = _nan_view(M, cols, 3, 64, torch.float16, DEV)
    x.copy_(xv)
    bias = (torch.randn(N, generator=gen, device=DEV) * 0.1).half() if with_bias else None

    def call():
        obuf, out = _nan_view(M, N, 3, 32, torch.float16, DEV)
        rc = lib.tgis_gptq8_tile_gemm_f16(x.data_ptr(), x.stride(0), w.image.data_ptr(), bias.data_ptr() if with_bias else None,
                                          w.perm.data_ptr() if w.perm is not None else None, out.data_ptr(), out.stride(0), M,
                                          w.K, w.N, w.groups, native._stream())
        assert rc == 0, lib.tgis_last_error().decode()
        torch.cuda.synchronize()
        return obuf, out

    obuf, got = call()
    assert torch.isnan(xbuf[M:]).all() and torch.isnan(xbuf[:, cols:]).all(), f"{what}: x padding written"
    assert torch.isnan(obuf[M:]).all() and torch.isnan(obuf[:, N:]).all(), f"{what}: out margins written"
    ref, tol = _reference(dict(K=K, N=N, act=0), xv, Wx, bias, torch.float16)  # K: the rows the kernel accumulates over
    assert ref.shape == got.shape == (M, N)
    print(f"{what}: worst err / tol {float(((got.double() - ref).abs() / tol).max()):.3f}")
    _check(got, ref, tol, what)
    _, again = call()
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), f"{what}: a second call differs"
