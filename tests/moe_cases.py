"""Shapes of the routed-expert op tests (tests/test_moe_ops_gpu.py, tests/test_moe_edges_gpu.py) and the restated launch plan
of csrc/moe.hip that tests/test_moe_plan_cpu.py holds against tgis_debug_moe_plan.  TEST INFRASTRUCTURE."""

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


def k_parts(K: int):
    """k64-steps of the four waves of a block, by the kernel's rule: per = ceil(KS / 4), wave wk takes steps
    [min(wk per, KS), min(wk per + per, KS))."""
    KS = cdiv(K, 64)
    per = cdiv(KS, WK)
    return tuple(min(min(wk * per, KS) + per, KS) - min(wk * per, KS) for wk in range(WK))


def last_step_columns(K: int):
    """Columns of K inside its last k64-step (64: no tail)."""
    return K - (cdiv(K, 64) - 1) * 64


# ---- the cases of tests/test_moe_edges_gpu.py --------------------------------------------------------------------------------
# 1. Deep k.  A wave keeps RING = 4 steps of weights in flight and refills slot r with step s + 4 once step s is used, so
# the refill runs only in a k-part of more than 4 steps: K > 1024.  K -> (steps per k-part, columns of the last step).
DEEP_K = {
    1024: ((4, 4, 4, 4), 64),  # the ring exactly full, no refill
    1064: ((5, 5, 5, 2), 40),  # one refill; the tail ends in the upper half of the step (i = 0 valid, i = 1..3 zeroed there)
    2048: ((8, 8, 8, 8), 64),  # every slot refilled once, the second pass full
    2056: ((9, 9, 9, 6), 8),   # a slot refilled twice
    2104: ((9, 9, 9, 6), 56),  # (down only)
}
DEEP_UP_K = (1024, 1064, 2048, 2056)
DEEP_DOWN_K = (1024, 1064, 2048, 2056, 2104)
DEEP_I = 48        # the up image has N = 96: three tiles
DEEP_DOWN_N = 72   # three tiles, the last 8 columns wide
DEEP_ROWS = ((1, "uniform"), (33, "same_two"), (33, "uniform"))  # same_two: one expert's 33 rows prime the ring twice

# 2. Short and ragged K.
SHORT_K = {
    8: ((1, 0, 0, 0), 8),     # one step, every load clamped to column 0, three waves idle
    64: ((1, 0, 0, 0), 64),   # one full step
    72: ((1, 1, 0, 0), 8),    # waves 0 and 1 have a step each
    200: ((1, 1, 1, 1), 8),   # four k-parts of one step
    296: ((2, 2, 1, 0), 40),
}
SHORT_I, SHORT_DOWN_N, SHORT_TOKENS = 16, 40, (1, 33)
K_PAD = 8  # NaN columns behind the K columns of the activations the K-tail cases hand to the kernel

# 3. Every admitted top_k and E through the GEMMs (hidden HIDDEN, I MIX_I).
MIX_I = 80
MIX_TOKENS = (1, 33, 65)
MIX_ROUTINGS = ((2, 1), (2, 2), (8, 1), (8, 3), (8, 8), (64, 2), (64, 8))
NORM_TOP_K, NORM_T = (1, 3, 8), 33          # sum_slabs8's buckets 1, 4 and 8 behind the slab form
SLAB_TOP_K, SLAB_TOKENS, SLAB_N = (1, 3), (1, 33), 300

# 4. Row strides at the C entry points.
STRIDE_T, STRIDE_I = 33, 80
STRIDE_PADS = dict(x=8, h=16, out=4)

# 5. Route.
EDGE_ROUTE_TOKENS = (1024, 1025, 2049, 3000)   # phase 1 gives a thread its second and third token
EDGE_ROUTE_CASES = ((8, 2), (64, 8), (2, 2), (5, 3))
EDGE_ROUTE_SMALL = ((64, 1), (2, 1))           # at EDGE_ROUTE_SMALL_TOKENS
EDGE_ROUTE_SMALL_TOKENS = (1, 65)
EDGE_ROUTE_STRIDED = (64, 8, 80)               # E, top_k, row stride of the logit matrix

# Near ties (E = 8): logits that differ in fp32, probabilities that differ in fp64 and collide in fp32 at the indices
# `tied`, the larger logits at the higher indices.  (logits, top_k, tied indices, ids)
NEAR_TIES = (
    ((0.0, 1e-9, -1.0, -2.0, 3e-9, -3.0, -1.0, -2.0), 2, (0, 1, 4), (0, 1)),
    ((0.0, 1e-9, -1.0, -2.0, 3e-9, -3.0, -1.0, -2.0), 3, (0, 1, 4), (0, 1, 4)),
    ((-1.0, 0.0, -3.0, 1e-9, -2.0, 2e-9, -1.25, 4e-9), 2, (1, 3, 5, 7), (1, 3)),
    ((-1.0, 0.0, -3.0, 1e-9, -2.0, 2e-9, -1.25, 4e-9), 3, (1, 3, 5, 7), (1, 3, 5)),
    ((0.0, -2.0, 5.0, 1e-9, -1.0, 2e-9, -4.0, 3e-9), 3, (0, 3, 5, 7), (2, 0, 3)),   # the tie is for second place
    ((-2.0, -1.0, -3.0, -2.5, -1.5, 0.0, 2e-9, 5e-9), 2, (5, 6, 7), (5, 6)),
)
# Underflow (E = 8): one dominant logit, the others 110 to 200 below it: exp(-110) < 2^-150, so every other fp32 probability
# and weight is 0 and the later choices are ties at zero.  (logits, top_k, ids)
UNDERFLOW = (
    ((-120.0, 0.0, -110.0, -130.0, -150.0, -200.0, -115.0, -140.0), 2, (1, 0)),
    ((-110.0, -120.0, -200.0, -130.0, -150.0, 0.0, -160.0, -111.0), 3, (5, 0, 1)),
    ((3.0, -117.0, -107.0, -197.0, -110.0, -150.0, -125.0, -108.0), 2, (0, 1)),
    ((-190.0, -180.0, -170.0, -160.0, -150.0, -140.0, -130.0, 0.0), 3, (7, 0, 1)),
)

# 6. Expert images past 2^31 and 2^32 bytes: five 16 KiB images FAR_STRIDE apart, the first FAR_BASE bytes above the start
# of an arena that holds NaN everywhere else.  The gate|up images sit there and the down images FAR_DOWN_SHIFT bytes behind
# them, so one fill of the arena serves both GEMMs.
FAR_E, FAR_TOP_K, FAR_K, FAR_I, FAR_DOWN_N = 5, 2, 128, 32, 64
FAR_BASE = 1 << 31
FAR_STRIDE = (1 << 30) + (64 << 10)
FAR_IMAGE_BYTES = 2 * 2 * 4096  # cdiv(64, 32) tiles x cdiv(128, 64) steps x 4 KiB, for the up (N = 2 I) and the down image
FAR_IDS = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 0))
FAR_DOWN_SHIFT = 32 << 10
FAR_ARENA_BYTES = FAR_BASE + FAR_DOWN_SHIFT + (FAR_E - 1) * FAR_STRIDE + FAR_IMAGE_BYTES  # 6 GiB + 304 KiB


def edge_gemm_cases():
    """(which, T, K, N, E, top_k) of every GEMM launch of tests/test_moe_edges_gpu.py, each once."""
    out = []
    for T, _pattern in DEEP_ROWS:
        out += [(0, T, K, 2 * DEEP_I, E, TOP_K) for K in DEEP_UP_K]
        out += [(w, T, K, DEEP_DOWN_N, E, TOP_K) for K in DEEP_DOWN_K for w in (1, 2)]
    for T in SHORT_TOKENS:
        for K in SHORT_K:
            out += [(0, T, K, 2 * SHORT_I, E, TOP_K), (1, T, K, SHORT_DOWN_N, E, TOP_K), (2, T, K, SHORT_DOWN_N, E, TOP_K)]
    for E_, k in MIX_ROUTINGS:
        for T in MIX_TOKENS:
            out += [(0, T, HIDDEN, 2 * MIX_I, E_, k), (1, T, MIX_I, HIDDEN, E_, k), (2, T, MIX_I, HIDDEN, E_, k)]
    for k in SLAB_TOP_K:
        for T in SLAB_TOKENS:
            out += [(0, T, HIDDEN, 2 * MIX_I, E, k), (1, T, MIX_I, SLAB_N, E, k)]
    out += [(0, STRIDE_T, HIDDEN, 2 * STRIDE_I, E, TOP_K), (2, STRIDE_T, STRIDE_I, HIDDEN, E, TOP_K)]
    T = len(FAR_IDS)
    out += [(0, T, FAR_K, 2 * FAR_I, FAR_E, FAR_TOP_K), (1, T, FAR_K, FAR_DOWN_N, FAR_E, FAR_TOP_K),
            (2, T, FAR_K, FAR_DOWN_N, FAR_E, FAR_TOP_K)]
    return list(dict.fromkeys(out))


def plan_cases():
    """(which, T, K, N, E, top_k) of every launch the GPU cases make, and Mixtral-8x7B's."""
    out = []
    for I in INTERMEDIATES:
        for T in TOKENS:
            out += [(0, T, HIDDEN, 2 * I), (1, T, I, HIDDEN)]
        for T in FINISHED_TOKENS:
            out += [(0, T, HIDDEN, 2 * I), (2, T, I, HIDDEN)]
    for T in (1, 8, 32, 256):
        out += [(0, T, 4096, 2 * 14336), (1, T, 14336, 4096), (2, T, 14336, 4096)]
    out = [c + (E, TOP_K) for c in out]
    return out + [c for c in edge_gemm_cases() if c not in out]
