"""CPU: the launch plan of the routed-expert GEMMs (csrc/moe.hip) restated in tests/moe_cases.py against
tgis_debug_moe_plan for the shapes of the GPU cases and Mixtral-8x7B's, and the argument refusals of the three entry points,
which are made before the device is touched (no GPU needed)."""
import ctypes

import pytest

from tests import moe_cases as mc


def _lib():
    from tgis_amd import native

    lib = native.load_library()
    fn = lib.tgis_debug_moe_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_int)]
    return lib


def _case_id(c):
    """The cases at E 8, top_k 2 keep the ids they had before the tuples carried E and top_k."""
    return "which{}-T{}-K{}-N{}".format(*c) + ("" if c[4:] == (mc.E, mc.TOP_K) else "-E{}-k{}".format(*c[4:]))


@pytest.mark.parametrize("case", mc.plan_cases(), ids=_case_id)
def test_plan_is_the_restated_one(case):
    which, T, K, N, E, top_k = case
    lib = _lib()
    info = (ctypes.c_int * 16)()
    assert lib.tgis_debug_moe_plan(which, T, K, N, E, top_k, info) == 0, lib.tgis_last_error()
    assert list(info)[:12] == mc.plan(which, T, K, N, E, top_k)
    assert list(info)[12:] == [0, 0, 0, 0]


def test_the_grid_does_not_depend_on_the_rows():
    """What lets the launches sit in a captured graph: T changes no grid dimension of the up and slab-form down launches."""
    lib = _lib()
    seen = set()
    for T in (1, 8, 64, 256):
        for which, K, N in ((0, 4096, 28672), (1, 14336, 4096)):
            info = (ctypes.c_int * 16)()
            assert lib.tgis_debug_moe_plan(which, T, K, N, 8, 2, info) == 0
            seen.add((which,) + tuple(info)[:10])
    assert len(seen) == 2


def test_down_bytes_is_the_plan():
    lib = _lib()
    for T, N, k in ((1, 320, 2), (33, 320, 2), (130, 4096, 2), (700, 320, 4)):
        assert lib.tgis_moe_gemm_down_bytes(T, N, k, 0) == mc.cdiv(T, 32) * k * 32 * mc.cdiv(N, 32) * 32 * 4
        assert lib.tgis_moe_gemm_down_bytes(T, N, k, 1) == T * k * N * 4
    assert lib.tgis_moe_gemm_down_bytes(0, 320, 2, 0) == 0


@pytest.mark.parametrize("E,top_k,T", [(1, 1, 4), (65, 2, 4), (8, 0, 4), (8, 9, 4), (4, 5, 4), (8, 2, -1), (8, 8, 1 << 29)])
def test_route_refuses_bad_routing_shapes(E, top_k, T):
    lib = _lib()
    one = ctypes.c_void_p(16)  # never dereferenced: the check comes first
    rc = lib.tgis_moe_route(one, E, T, E, top_k, one, one, one, one, one, None)
    assert rc == -1 and b"tgis_moe_route" in lib.tgis_last_error()
    lib.tgis_clear_error()


def test_gemms_refuse_bad_arguments():
    lib = _lib()
    p = ctypes.c_void_p(4096)  # never dereferenced
    stride_up = lib.tgis_dense_prepared_bytes(160, 320)
    stride_dn = lib.tgis_dense_prepared_bytes(320, 80)

    def up(**kw):
        a = dict(x=p, ldx=320, images=p, stride=stride_up, offsets=p, slot_rows=p, h=p, ldh=80, T=4, K=320, N=160, E=8,
                 top_k=2, dtype=0)
        a.update(kw)
        return lib.tgis_moe_gemm_up(a["x"], a["ldx"], a["images"], a["stride"], a["offsets"], a["slot_rows"], a["h"], a["ldh"],
                                    a["T"], a["K"], a["N"], a["E"], a["top_k"], a["dtype"], None)

    def down(**kw):
        a = dict(h=p, ldh=80, images=p, stride=stride_dn, offsets=p, slot_rows=p, w=p, T=4, K=80, N=320, E=8, top_k=2, dtype=1,
                 form=0, scratch=p, nbytes=1 << 30, out=p, ldo=320)
        a.update(kw)
        return lib.tgis_moe_gemm_down(a["h"], a["ldh"], a["images"], a["stride"], a["offsets"], a["slot_rows"], a["w"], a["T"],
                                      a["K"], a["N"], a["E"], a["top_k"], a["dtype"], a["form"], a["scratch"], a["nbytes"],
                                      a["out"], a["ldo"], None)

    for bad in (dict(E=1), dict(top_k=9), dict(T=-1), dict(K=324), dict(N=176), dict(dtype=2), dict(stride=stride_up - 4096),
                dict(x=None), dict(offsets=None), dict(ldx=312), dict(ldh=79), dict(x=ctypes.c_void_p(4098))):
        assert up(**bad) == -1 and b"tgis_moe_gemm_up" in lib.tgis_last_error(), bad
    for bad in (dict(E=65), dict(top_k=0), dict(K=84), dict(form=2), dict(w=None), dict(stride=stride_dn - 4096),
                dict(nbytes=1024), dict(scratch=None), dict(form=1, out=None), dict(form=1, N=322), dict(form=1, ldo=300)):
        assert down(**bad) == -1 and b"tgis_moe_gemm_down" in lib.tgis_last_error(), bad
    # T == 0 is served and launches nothing
    assert up(T=0) == 0 and down(T=0) == 0
    lib.tgis_clear_error()
