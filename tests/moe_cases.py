"""Shapes of the routed-expert op tests (tests/test_moe_ops_gpu.py) and the restated launch plan of csrc/moe.hip that
tests/test_moe_plan_cpu.py holds against tgis_debug_moe_plan.  TEST INFRASTRUCTURE."""

HIDDEN = 320            # 5 k64-steps: a k tail against the 256-wide chunk of the dense unit, uneven k-parts here (2, 2, 1, 0)
INTERMEDIATES = (80, 528)  # N tails of the up image (160 / 1056 rows = 5 / 33 tiles) and a K tail of the down GEMM (80 = 64 + 16)
TOKENS = (1, 31, 32, 33, 64, 65, 130)
FINISHED_TOKENS = (130, 700)
E, TOP_K = 8, 2
ROUTE_CASES = ((8, 2), (4, 1), (16, 4))
ROUTE_TOKENS = (1, 2, 33, 64, 130, 700)

WK, RING, THREADS, LDS_BYTES = 4, 4, 256, 4 * 64 * 16 * 4


def cdiv(a, b):
    return (a + b - 1) // b


def plan(which: int, T: int, K: int, N: int, E: int, top_k: int):
    """info[0:12] of tgis_debug_moe_plan.  which: 0 up (N = 2 I rows of the gate|up image), 1 down as slabs, 2 down finished.
    The grid is (column tiles, experts) whatever T and the routing are; a block's four waves split the k64-steps."""
    NT, KS = cdiv(N, 32), cdiv(K, 64)
    if which == 0:
        scratch = 0
    elif which == 1:
        scratch = cdiv(T, 32) * top_k * 32 * NT * 32 * 4
    else:
        scratch = T * top_k * N * 4
    return [NT, E, THREADS, WK, cdiv(KS, WK), RING, LDS_BYTES, 32, 16 if which == 0 else 32,
            cdiv(T * (N // 4), 256) if which == 2 else 0, scratch & 0x7FFFFFFF, scratch >> 31]


def plan_cases():
    """(which, T, K, N) of every launch the GPU cases make, and Mixtral-8x7B's."""
    out = []
    for I in INTERMEDIATES:
        for T in TOKENS:
            out += [(0, T, HIDDEN, 2 * I), (1, T, I, HIDDEN)]
        for T in FINISHED_TOKENS:
            out += [(0, T, HIDDEN, 2 * I), (2, T, I, HIDDEN)]
    for T in (1, 8, 32, 256):
        out += [(0, T, 4096, 2 * 14336), (1, T, 14336, 4096), (2, T, 14336, 4096)]
    return out
