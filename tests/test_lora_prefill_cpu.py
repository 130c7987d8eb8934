"""No GPU: the argument checks of tgis_lora_shrink_tiles / tgis_lora_expand_tiles (csrc/lora_prefill.hip), which refuse before
any launch, and the host's tile table of a prefill (utils.lora.lora_tile_table)."""
import ctypes

import pytest

from tgis_amd import native
from tgis_amd.utils.lora import lora_tile_table


def test_tile_entry_points_check_their_arguments_without_a_gpu():
    lib = native.load_library()
    bounds = (ctypes.c_int64 * 4)(0, 256, 384, 512)
    p = 4096  # a non-null, 16-byte aligned address that is never read: every call below is refused first or launches nothing
    A, B = lib.tgis_lora_a_bytes(320, 3, 64), lib.tgis_lora_b_bytes(512, 64)

    def shrink(T=100, n=2, K=320, P=3, S=4, R=64, dtype=0, stride=A, ldx=320, x=p, a=p, tiles=p):
        return lib.tgis_lora_shrink_tiles(x, ldx, a, stride, p, tiles, n, p, T, K, P, S, R, dtype, None)

    def expand(T=100, n=2, N=512, P=3, S=4, R=64, dtype=0, stride=B, ldy=512, bnd=bounds, y=p, b=p, tiles=p):
        return lib.tgis_lora_expand_tiles(p, b, stride, p, p, tiles, n, bnd, y, ldy, T, N, P, S, R, dtype, None)

    def refused(rc, fn, words):
        msg = lib.tgis_last_error().decode()
        assert rc == -1 and fn in msg and words in msg, (rc, msg)

    refused(shrink(T=-1), "tgis_lora_shrink_tiles", "0 <= T")
    refused(shrink(n=-1), "tgis_lora_shrink_tiles", "0 <= n_tiles")
    refused(shrink(n=1 << 16), "tgis_lora_shrink_tiles", "0 <= n_tiles")
    refused(shrink(a=None), "tgis_lora_shrink_tiles", "null tensor")
    refused(shrink(x=None), "tgis_lora_shrink_tiles", "null tensor")
    refused(shrink(tiles=4104), "tgis_lora_shrink_tiles", "16-byte aligned")
    refused(shrink(dtype=2), "tgis_lora_shrink_tiles", "bad dtype")
    refused(shrink(K=324), "tgis_lora_shrink_tiles", "multiple of 8")
    refused(shrink(P=4), "tgis_lora_shrink_tiles", "1 <= P <= 3")
    refused(shrink(S=33), "tgis_lora_shrink_tiles", "1 <= S <= 32")
    refused(shrink(R=24), "tgis_lora_shrink_tiles", "multiple of 16")
    refused(shrink(stride=A - 16), "tgis_lora_shrink_tiles", "must hold one A image")
    refused(shrink(ldx=312), "tgis_lora_shrink_tiles", "16-byte aligned")
    refused(expand(T=-1), "tgis_lora_expand_tiles", "0 <= T")
    refused(expand(b=None), "tgis_lora_expand_tiles", "null tensor")
    refused(expand(y=None), "tgis_lora_expand_tiles", "null tensor")
    refused(expand(dtype=-1), "tgis_lora_expand_tiles", "bad dtype")
    refused(expand(N=516), "tgis_lora_expand_tiles", "multiple of 8")
    refused(expand(R=80), "tgis_lora_expand_tiles", "at most 64")
    refused(expand(stride=B - 16), "tgis_lora_expand_tiles", "must hold one B image")
    refused(expand(ldy=500), "tgis_lora_expand_tiles", "rows of y must hold N")
    refused(expand(bnd=(ctypes.c_int64 * 4)(0, 256, 384, 520)), "tgis_lora_expand_tiles", "from 0 to N")
    refused(expand(bnd=(ctypes.c_int64 * 4)(0, 260, 384, 512)), "tgis_lora_expand_tiles", "multiples of 8")
    refused(expand(bnd=(ctypes.c_int64 * 4)(0, 384, 256, 512)), "tgis_lora_expand_tiles", "must ascend")
    lib.tgis_clear_error()
    # nothing to do is no error and no launch: no rows, or no tile (then the table may be null)
    assert shrink(T=0) == 0 and expand(T=0) == 0 and shrink(n=0, tiles=None) == 0 and expand(n=0, tiles=None) == 0


@pytest.mark.parametrize("slots, rows", [
    ([2], [65]), ([0, -1, 1, 3, 2], [1, 7, 64, 63, 2]), ([3, 0], [130, 5]), ([1, 2, 1], [70, 3, 129]), ([-1, -1], [40, 90]),
    ([0, 1, -1, 2], [0, 128, 0, 1]), ([], []),
])
def test_tile_table(slots, rows):
    want, row = [], 0
    for s, n in zip(slots, rows):
        want += [[row + r, min(64, n - r), s, 0] for r in range(0, n, 64) if s >= 0]
        row += n
    got = lora_tile_table(slots, rows)
    assert got.dtype.name == "int32" and got.shape == (len(want), 4) and got.flags["C_CONTIGUOUS"] and got.tolist() == want
