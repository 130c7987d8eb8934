"""CPU: what the 8-bit GPTQ tile GEMM decides on the host — the refusals of tgis_gptq8_tile_gemm_f16 (arguments are
checked before the device is touched), the row rule tgis_gptq8_tile_rows and the TGIS_GPTQ8_PATH switch."""
import pytest

X, W, OUT = 0x1000, 0x2000, 0x3000  # never dereferenced: every call below is refused


@pytest.mark.parametrize("what,why,args", [
    ("null tensor", b"null tensor", (X, 256, None, None, None, OUT, 64, 65, 256, 64, 2)),
    ("no rows", b"1 <= M", (X, 256, W, None, None, OUT, 64, 0, 256, 64, 2)),
    ("K % 32", b"multiples of 32", (X, 272, W, None, None, OUT, 64, 65, 272, 64, 1)),
    ("group size 8", b"multiple of 16", (X, 256, W, None, None, OUT, 64, 65, 256, 64, 32)),
    ("misaligned ldx", b"16-byte aligned rows", (X, 260, W, None, None, OUT, 64, 65, 256, 64, 2)),
    ("misaligned x", b"16-byte aligned rows", (X + 2, 256, W, None, None, OUT, 64, 65, 256, 64, 2)),
    ("ldo < N", b"at least N elements", (X, 256, W, None, None, OUT, 56, 65, 256, 64, 2)),
])
def test_bad_arguments_are_refused(what, why, args):
    from tgis_amd import native

    lib = native.load_library()
    lib.tgis_clear_error()
    assert lib.tgis_gptq8_tile_gemm_f16(*args, None) == -1, f"{what}: accepted"
    err = lib.tgis_last_error()
    assert b"tgis_gptq8_tile_gemm_f16" in err and why in err, err
    lib.tgis_clear_error()


@pytest.mark.parametrize("K,N,groups", [(4096, 12288, 32), (4096, 4096, 32), (4096, 22016, 32), (11008, 4096, 86),
                                        (96, 32, 1), (2048, 8192, 128)])
@pytest.mark.parametrize("act_order", [0, 1])
def test_tile_rows_is_a_multiple_of_64(K, N, groups, act_order):
    from tgis_amd import native

    rows = native.load_library().tgis_gptq8_tile_rows(K, N, groups, act_order)
    assert rows >= 64 and rows % 64 == 0, rows


def test_path_switch_refuses_unknown_values(monkeypatch):
    from tgis_amd.utils import layers

    for v, want in (("auto", None), ("tiles", "tiles"), ("DEQUANT", "dequant")):
        monkeypatch.setenv("TGIS_GPTQ8_PATH", v)
        assert layers.gptq8_path_override() == want
    monkeypatch.delenv("TGIS_GPTQ8_PATH")
    assert layers.gptq8_path_override() is None
    monkeypatch.setenv("TGIS_GPTQ8_PATH", "sometimes")
    with pytest.raises(ValueError, match="TGIS_GPTQ8_PATH"):
        layers.gptq8_path_override()
