"""The launch plan of the int4 routed-expert GEMMs (tgis_debug_moe_gptq_plan, host only) against its restatement in
tests/moe_gptq_cases.py: the grid, the k split, the int4 ring, the scratch of both down forms and the stride between expert
images, at the shapes the GPU tests launch and at Mixtral-8x7B's.  tgis_debug_moe_plan itself is untouched: the dense plan
still reports its own ring."""
import ctypes

import pytest

from tests import moe_cases as mc
from tests import moe_gptq_cases as gc


@pytest.fixture(scope="module")
def lib():
    from tgis_amd import native

    lib = native.load_library()
    lib.tgis_debug_moe_gptq_plan.restype = ctypes.c_int
    lib.tgis_debug_moe_gptq_plan.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.tgis_debug_moe_plan.restype = ctypes.c_int
    lib.tgis_debug_moe_plan.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return lib


def _plan(lib, which, T, K, N, G, E=gc.E, top_k=gc.TOP_K):
    info = (ctypes.c_int * 16)()
    rc = lib.tgis_debug_moe_gptq_plan(which, T, K, N, G, E, top_k, info)
    return rc, list(info)


SHAPES = ([(K, 2 * I, gs) for K, I, gs in gc.UP_CASES] + gc.DOWN_CASES + gc.DEEP_CASES)


@pytest.mark.parametrize("K,N,gs", SHAPES + gc.BIG_SHAPES, ids=lambda v: str(v))
def test_plan_equals_the_restatement(lib, K, N, gs):
    G = gc.groups_of(K, gs)
    tokens = gc.BIG_TOKENS if (K, N, gs) in gc.BIG_SHAPES else gc.TOKENS + (gc.FINISHED_TOKENS,)
    for T in tokens:
        for which in (0, 1, 2):
            rc, info = _plan(lib, which, T, K, N, G)
            assert rc == 0, lib.tgis_last_error()
            assert info[:14] == gc.plan(which, T, K, N, G), (which, T, K, N, G)
            assert info[14:] == [0, 0]
    # the stride is tgis_gptq_prepared_bytes, which is what MoeGptqWeights allocates per expert
    assert lib.tgis_gptq_prepared_bytes(K, N, G) == gc.prepared_bytes(K, N, G)


def test_plan_of_every_edge_launch_equals_the_restatement(lib):
    """Every launch of tests/test_moe_gptq_edges_gpu.py: group sizes 128 to 16384 at K up to 32768, (E, top_k) from (2, 1) to
    (64, 8), the identity's 128 and 256 rows, the far images' five experts."""
    cases = gc.edge_cases()
    assert len(cases) == len(set(cases)) > 100
    assert {c[5:] for c in cases} >= {(2, 1), (64, 8), (5, 2)} and {c[4] for c in cases} >= {1, 2, 3, 5, 28}
    for which, T, K, N, G, E, top_k in cases:
        rc, info = _plan(lib, which, T, K, N, G, E, top_k)
        assert rc == 0, lib.tgis_last_error()
        assert info[:14] == gc.plan(which, T, K, N, G, E, top_k), (which, T, K, N, G, E, top_k)
        assert info[14:] == [0, 0]
        assert info[4] == max(mc.k_parts(K)) and lib.tgis_gptq_prepared_bytes(K, N, G) == gc.prepared_bytes(K, N, G)


def test_k_parts_of_the_gpu_cases(lib):
    """The k-part sizes the GPU cases are named after: steps per wave = ceil(ceil(K / 64) / 4)."""
    for K, per in ((64, 1), (320, 2), (384, 2), (576, 3), (640, 3), (1088, 5), (4352, 17), (4096, 16), (14336, 56)):
        rc, info = _plan(lib, 1, 1, K, 64, 1)
        assert rc == 0 and info[4] == per and info[3] == 4
    assert gc.DEEP_CASES[-1][0] // 64 // 4 > gc.RING  # the deepest case refills every ring slot


def test_the_dense_plan_is_unchanged(lib):
    info = (ctypes.c_int * 16)()
    assert lib.tgis_debug_moe_plan(1, 33, 320, 320, gc.E, gc.TOP_K, info) == 0
    assert info[5] == 4 and list(info)[12:] == [0, 0, 0, 0]


@pytest.mark.parametrize("K,N,G", [(96, 64, 1), (320, 48, 1), (320, 64, 10), (320, 64, 3), (640, 64, 0)],
                         ids=("K96", "N48", "group32", "groups_not_dividing", "no_groups"))
def test_plan_refuses_what_the_kernels_do_not_serve(lib, K, N, G):
    rc, _ = _plan(lib, 1, 8, K, N, G)
    assert rc != 0
    lib.tgis_clear_error()
