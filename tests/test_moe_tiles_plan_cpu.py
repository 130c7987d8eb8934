"""CPU: the launch plan of the routing and tile GEMMs for up to 128 experts (csrc/moe_tiles.h) restated here against
tgis_debug_moe_tile_plan for the shapes of tests/test_moe_tiles_ops_gpu.py and Qwen3-30B-A3B's, and the argument refusals of
the three entry points, which are made before the device is touched (no GPU needed)."""
import ctypes

import pytest

R, C, ROUTE_TOKENS = 64, 128, 32


def cdiv(a, b):
    return (a + b - 1) // b


def _plan(which, T, K, N, E, top_k, slab_max):
    """The restated plan: the slab kernel body of csrc/moe.hip up to slab_max tokens, the tile kernel above."""
    bound = cdiv(T * top_k, R) + min(E, T * top_k)
    scratch = 0 if which == 0 else (cdiv(T, 32) * top_k * 32 * cdiv(N, 32) * 32 * 4 if which == 1 else T * top_k * N * 4)
    slab = T <= slab_max
    return dict(grid_x=cdiv(N, 32) if slab else cdiv(cdiv(N, 32), C // 32), grid_y=E if slab else bound, threads=256,
                lds_bytes=4 * 64 * 16 * 4 if slab else 2 * R * 64 * 2 + R * 8, rows=32 if slab else R, columns=32 if slab else C,
                slab_body=int(slab), combine_blocks=cdiv(T * (N // 4), 256) if which == 2 else 0, tile_bound=bound,
                route_blocks=cdiv(T, ROUTE_TOKENS), route_tokens=ROUTE_TOKENS, route_bytes=cdiv(T, ROUTE_TOKENS) * E * 4,
                slab_max_tokens=slab_max, scratch_bytes=scratch)


CASES = [(w, 200, K, N, 8, 2) for K, I in ((64, 16), (136, 48), (768, 80)) for w, N in ((0, 2 * I), (1, K), (2, K))]
CASES += [(0, 33, 136, 96, 128, 8), (2, 33, 48, 136, 128, 8), (0, 5, 136, 96, 8, 2), (1, 5, 48, 136, 8, 2)]
CASES += [(w, T, K, N, 128, 8) for T in (1, 8, 32, 64, 256, 4096) for w, K, N in ((0, 2048, 1536), (1, 768, 2048), (2, 768, 2048))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "which{}-T{}-K{}-N{}-E{}-k{}".format(*c))
def test_plan_is_the_restated_one(case):
    from tgis_amd import native

    got = native.moe_tile_plan(*case)
    assert got == _plan(*case, got["slab_max_tokens"])
    lib = native.load_library()
    assert lib.tgis_moe_tile_bound(case[1], case[4], case[5]) == got["tile_bound"]
    assert lib.tgis_moe_route_tiles_bytes(case[1], case[4], case[5]) == got["route_bytes"]
    assert lib.tgis_moe_tile_gemm_down_bytes(case[1], case[3], case[5], 1) == case[1] * case[5] * case[3] * 4


def test_entry_points_refuse_bad_arguments():
    from tgis_amd import native

    lib = native.load_library()
    p, one = ctypes.c_void_p(4096), ctypes.c_void_p(16)  # never dereferenced: the checks come first
    stride_up, stride_dn = lib.tgis_dense_prepared_bytes(160, 320), lib.tgis_dense_prepared_bytes(320, 80)
    # every entry point's good arguments in call order; a case replaces some of them
    good = {
        "tgis_moe_route_tiles": dict(logits=one, ld=128, T=4, E=128, top_k=8, renorm=1, ids=one, w=one, counts=one, offsets=one,
                                     rows=one, tiles=one, bound=lib.tgis_moe_tile_bound(4, 128, 8), ws=one, ws_bytes=1 << 20),
        "tgis_moe_tile_gemm_up": dict(x=p, ldx=320, images=p, stride=stride_up, offsets=p, slot_rows=p, tiles=p, bound=128, h=p,
                                      ldh=80, T=4, K=320, N=160, E=128, top_k=8, dtype=0),
        "tgis_moe_tile_gemm_down": dict(h=p, ldh=80, images=p, stride=stride_dn, offsets=p, slot_rows=p, tiles=p, bound=128, w=p,
                                        T=4, K=80, N=320, E=128, top_k=8, dtype=1, form=0, scratch=p, nbytes=1 << 30, out=p,
                                        ldo=320),
    }
    bad = {
        "tgis_moe_route_tiles": (dict(E=129), dict(E=1), dict(top_k=0), dict(top_k=9), dict(renorm=2), dict(ld=127),
                                 dict(logits=None), dict(tiles=None), dict(bound=3), dict(ws=None), dict(ws_bytes=8), dict(T=-1)),
        "tgis_moe_tile_gemm_up": (dict(E=129), dict(top_k=0), dict(top_k=9), dict(K=324), dict(N=176), dict(dtype=2),
                                  dict(stride=stride_up - 4096), dict(x=None), dict(tiles=None), dict(bound=3), dict(ldx=312),
                                  dict(ldh=79), dict(x=ctypes.c_void_p(4098))),
        "tgis_moe_tile_gemm_down": (dict(E=129), dict(top_k=9), dict(K=84), dict(form=2), dict(w=None), dict(bound=3),
                                    dict(stride=stride_dn - 4096), dict(nbytes=1024), dict(scratch=None), dict(form=1, out=None),
                                    dict(form=1, N=322), dict(form=1, ldo=300)),
    }
    for name, cases in bad.items():
        for case in cases:
            assert getattr(lib, name)(*{**good[name], **case}.values(), None) == -1 and name.encode() in lib.tgis_last_error(), (name, case)
    for name in ("tgis_moe_tile_gemm_up", "tgis_moe_tile_gemm_down"):  # T == 0 is served and launches nothing
        assert getattr(lib, name)(*{**good[name], "T": 0, "bound": 0}.values(), None) == 0
    lib.tgis_clear_error()
