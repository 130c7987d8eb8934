"""CPU: the launch choice of tgis_gptq_gemm_f16 with act 4 / 5 (GELU of the finished sum), asked of the library's host
entry points as test_gemm_plans_cpu.py asks them (no GPU).

The GELU forms take the plan of act 0 for the same (M, K, N, groups, act-order) — the same summation order over k is what
makes them bit-identical to act 0 followed by tgis_gelu — and report themselves in info[14] (1 erf, 2 tanh) only; the tall
kernel has no GELU finish, so tgis_gptq_gemm_fused_rows(act 4 | 5) stays at 256."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

ROWS = (1, 31, 32, 33, 64, 65, 96, 256)
# tiny c_fc, N below a tile multiple, a deep narrow shape (splits over k), ragged wide N, the Starcoder-15B c_fc and its TP 2 shard
SHAPES = ((256, 1024), (256, 96), (4096, 64), (1024, 2080), (6144, 24576), (6144, 12288))


def _groups(K):
    return sorted({1, K // 64, K // 128})


def grid():
    return [(M, K, N, groups, ao) for K, N in SHAPES for M in ROWS for groups in _groups(K) for ao in (False, True)
            if not (ao and groups == 1)]


@pytest.fixture(scope="module")
def lib():
    from tgis_amd import native

    return native.load_library()


def test_gelu_takes_the_plan_of_act_0(lib):
    classes = {"unsplit": 0, "split": 0, "rows_above_64": 0, "act_order": 0}
    for M, K, N, groups, ao in grid():
        plain = gc.query_plan(lib, "gptq", M, K, N, groups, 0, ao)
        assert plain is not None and plain[14] == 0, (M, K, N, groups, ao)
        for act, flag in ((4, 1), (5, 2)):
            got = gc.query_plan(lib, "gptq", M, K, N, groups, act, ao)
            assert got is not None, f"tgis_debug_gemm_plan refused act {act} at {(M, K, N, groups, ao)}"
            assert got[14] == flag and got[8] == 0, (got, act)
            assert got[:14] + got[15:] == plain[:14] + plain[15:], f"act {act} at {(M, K, N, groups, ao)}: {got} != {plain}"
        p = gc.plan_fields(plain)
        assert p["family"] == "stream", (M, K, N, groups, ao, p)
        classes["split" if p["s"] > 1 else "unsplit"] += 1
        classes["rows_above_64"] += M > 64
        classes["act_order"] += ao
        assert p["reduce"] == (p["s"] > 1)
    # a change of the planner must not empty a class silently
    assert all(classes.values()), classes
    assert gc.plan_fields(gc.query_plan(lib, "gptq", 32, 4096, 64, 64, 4, False))["s"] > 1, "(4096, 64) no longer splits"


def test_fused_rows_of_the_gelu_forms_is_256(lib):
    for K, _ in SHAPES:
        for groups in _groups(K):
            for ao in (0, 1):
                for act in (4, 5):
                    assert lib.tgis_gptq_gemm_fused_rows(K, groups, ao, act) == 256, (K, groups, ao, act)
    # ... while act 0 still reaches the tall kernel where it serves the shape
    assert lib.tgis_gptq_gemm_fused_rows(6144, 48, 0, 0) > 256


def test_forms_without_a_gelu_finish_are_refused(lib):
    assert gc.query_plan(lib, "gptq", 257, 256, 1024, 4, 4) is None  # the tall kernel / library path: act 0, then tgis_gelu
    assert "256 rows" in lib.tgis_last_error().decode()
    assert gc.query_plan(lib, "gptq_partial", 32, 256, 1024, 4, 5) is None  # a GELU needs the finished sum
    assert gc.query_plan(lib, "gptq", 32, 256, 1024, 4, 4, False, True) is None  # fragment-order activation
