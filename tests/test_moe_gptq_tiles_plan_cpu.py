"""CPU: the argument refusals of the int4 tile expert GEMMs (csrc/moe_gptq_tiles.h: tgis_moe_gptq_tile_gemm_up / _down), made
before the device is touched, and T == 0."""
import ctypes


def test_entry_points_refuse_bad_arguments():
    from tgis_amd import native

    lib = native.load_library()
    p = ctypes.c_void_p(4096)  # never dereferenced: the checks come first
    stride_up, stride_dn = lib.tgis_gptq_prepared_bytes(320, 160, 5), lib.tgis_gptq_prepared_bytes(128, 320, 1)
    bound = lib.tgis_moe_tile_bound(4, 128, 8)
    # both entry points' good arguments in call order; a case replaces some of them
    good = {
        "tgis_moe_gptq_tile_gemm_up": dict(x=p, ldx=320, images=p, stride=stride_up, offsets=p, slot_rows=p, tiles=p, bound=bound,
                                           h=p, ldh=80, T=4, K=320, N=160, G=5, E=128, top_k=8, dtype=native.F16),
        "tgis_moe_gptq_tile_gemm_down": dict(h=p, ldh=128, images=p, stride=stride_dn, offsets=p, slot_rows=p, tiles=p,
                                             bound=bound, w=p, T=4, K=128, N=320, G=1, E=128, top_k=8, dtype=native.F16, form=0,
                                             scratch=p, nbytes=1 << 30, out=p, ldo=320),
    }
    bad = {
        "tgis_moe_gptq_tile_gemm_up": (dict(E=129), dict(top_k=0), dict(top_k=9), dict(K=96), dict(N=48), dict(G=10),
                                       dict(dtype=native.BF16), dict(stride=stride_up - 16), dict(x=None), dict(images=None),
                                       dict(tiles=None), dict(bound=bound - 1), dict(ldx=312), dict(ldh=79), dict(h=None)),
        "tgis_moe_gptq_tile_gemm_down": (dict(E=129), dict(top_k=9), dict(K=96), dict(N=48), dict(G=4), dict(form=2),
                                         dict(dtype=native.BF16), dict(w=None), dict(tiles=None), dict(bound=bound - 1),
                                         dict(stride=stride_dn - 16), dict(nbytes=1024), dict(scratch=None),
                                         dict(form=1, out=None), dict(form=1, ldo=300)),
    }
    for name, cases in bad.items():
        for case in cases:
            assert getattr(lib, name)(*{**good[name], **case}.values(), None) == -1 and name.encode() in lib.tgis_last_error(), (name, case)
        # T == 0 is served and launches nothing
        assert getattr(lib, name)(*{**good[name], "T": 0, "bound": 0}.values(), None) == 0
    lib.tgis_clear_error()
