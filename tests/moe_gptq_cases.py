"""Shapes, quantised weights and the launch-plan restatement shared by the int4 routed-expert tests
(tests/test_moe_gptq_ops_gpu.py, tests/test_moe_gptq_plan_cpu.py).  TEST INFRASTRUCTURE: importing this file needs no GPU.

Weights are quantised min/max with oracle.tiny_models.quantize_gptq, as tests/bigcode_gptq_ref.py does.  The reference weight
is W16 = oracle.ops_ref.gptq_dequant(...).half(): (q - z - 1) * s rounded once to f16, which the kernel's dequant8 reproduces
exactly, so the op references and bounds are tests/moe_bounds.py's on W16, with no new constants.  In every matrix column
FORCED_COLUMN has zero point 15 in every group (z + 1 = 16 is not masked back to 4 bits) and nibbles 0 and 15 in its first two
rows.

Group sizes: a group size is listed for a K it divides (quantize_gptq and the entry points both ask for that); -1 is a single
group.  K 64 and K 576 are no multiples of 128, so the 128-row groups of the down GEMM are exercised at K 640 and the deep K
4352; at K 64 the group of 64 rows is the single group."""
import functools

import numpy as np
import torch

from oracle import ops_ref
from oracle.tiny_models import quantize_gptq

E, TOP_K = 8, 2
FORCED_COLUMN = 3
RING = 4  # k64-steps of int4 weights a wave keeps in flight (csrc/moe.hip: TGIS_MOE_GPTQ_RING)

# (K, I, group size): the up GEMM reads a [K, 2 I] gate|up matrix
UP_CASES = [(320, 64, 64), (320, 64, -1), (320, 576, 64), (320, 576, -1),  # k-parts of 2, 2, 1, 0 steps; 4 and 36 tiles
            (384, 64, 128), (384, 576, 128)]                                # a group boundary inside a k-part
# (K, N, group size)
DOWN_CASES = [(64, 320, 64), (64, 320, -1),     # one step, three idle waves
              (576, 320, 64), (576, 320, -1),   # k-parts of 3, 3, 3, 0 steps
              (640, 320, 128)]                  # wave 1 starts mid-group (k-parts of 3, 3, 3, 1 steps, groups of 2)
# deep k: K 1088 = 17 steps (k-parts 5, 5, 5, 2) past a ring of 4; K 4352 = 68 steps, 17 per wave, past a ring of 16 (and of the
# RING kept): every slot of the ring is refilled at least once
DEEP_CASES = [(1088, 64, 64), (1088, 64, -1), (4352, 64, 128)]
TOKENS = (1, 31, 32, 33, 65)
FINISHED_TOKENS = 130
# 8x7B's expert shapes (hidden 4096, I 14336) at group 128 and as one group
BIG_SHAPES = [(4096, 2 * 14336, 128), (4096, 2 * 14336, -1), (14336, 4096, 128), (14336, 4096, -1)]
BIG_TOKENS = (1, 8, 32, 256)


def groups_of(K, gs):
    return 1 if gs == -1 else K // gs


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def quantize_forced(w_kn: torch.Tensor, gs: int):
    """(qweight, qzeros, scales, g_idx) as torch tensors for W [K, N], with FORCED_COLUMN's zero points set to 15 and its
    first two nibbles to 0 and 15, and W16 [K, N]: the dequantisation rounded once to f16."""
    K = w_kn.shape[0]
    size = K if gs == -1 else gs
    qw, qz, sc, gi = quantize_gptq(w_kn, size)
    qw, qz = _u32(qw).copy(), _u32(qz).copy()
    c = FORCED_COLUMN
    qz[:, c // 8] |= np.uint32(15 << (4 * (c % 8)))
    qw[0, c] = (qw[0, c] & np.uint32(0xFFFFFF00)) | np.uint32(0xF0)
    qw, qz = qw.view(np.int32), qz.view(np.int32)
    if gs == -1:
        gi = np.zeros(K, dtype=np.int32)  # one group: the all-zero g_idx AutoGPTQ writes for group_size -1
    w16 = ops_ref.gptq_dequant(qw, qz, sc, gi, size).half()
    col = w16[:, c].float() / torch.from_numpy(np.asarray(sc, dtype=np.float32))[:, c].repeat_interleave(size)
    assert float(col[0]) == -16.0 and float(col[1]) == -1.0, "the forced column holds (0 - 16) s and (15 - 16) s"
    return (torch.from_numpy(qw), torch.from_numpy(qz), torch.from_numpy(np.asarray(sc)), torch.from_numpy(gi)), w16


@functools.lru_cache(maxsize=None)
def up_experts(K, I, gs):
    """(bundles, w1, w3): per expert the GPTQ tensors of [gate | up] as a [K, 2 I] matrix, and W16 as w1 / w3 [E, I, K] f16."""
    g = torch.Generator().manual_seed(1000 * K + 8 * I + (gs % 1000))
    bundles, w1, w3 = [], [], []
    for _ in range(E):
        w = torch.randn(K, 2 * I, generator=g) * K ** -0.5
        b, w16 = quantize_forced(w, gs)
        bundles.append(b)
        w1.append(w16[:, :I].t().contiguous())
        w3.append(w16[:, I:].t().contiguous())
    return bundles, torch.stack(w1), torch.stack(w3)


@functools.lru_cache(maxsize=None)
def down_experts(K, N, gs):
    """(bundles, w2): per expert the GPTQ tensors of a [K, N] down matrix, and W16 as w2 [E, N, K] f16."""
    g = torch.Generator().manual_seed(1000 * K + 8 * N + (gs % 1000) + 1)
    bundles, w2 = [], []
    for _ in range(E):
        b, w16 = quantize_forced(torch.randn(K, N, generator=g) * K ** -0.5, gs)
        bundles.append(b)
        w2.append(w16.t().contiguous())
    return bundles, torch.stack(w2)


def moe_weights(bundles, gs, dev, gate_up=False):
    """native.MoeGptqWeights of the bundles of up_experts / down_experts."""
    from tgis_amd import native

    return native.MoeGptqWeights(lambda e: tuple(t.to(dev) for t in bundles[e]) + (4, gs), E, gate_up=gate_up)


def poisoned(mw, chosen):
    """A copy of the int4 images with 0xFF bytes (NaN scales and zero points, nibbles of 15) in every expert outside
    `chosen`: a block that read the scale table or dequantised would show."""
    from tgis_amd import native

    twin = native.MoeGptqWeights.__new__(native.MoeGptqWeights)
    twin.__dict__.update(mw.__dict__)
    twin.image = mw.image.clone()
    for e in range(mw.E):
        if e not in chosen:
            twin.image[e].fill_(0xFF)
    return twin


# ---- the launch plan, restated ----------------------------------------------------------------------------------------------
def prepared_bytes(K, N, G):
    """tgis_gptq_prepared_bytes: [NT][KS'][1 KiB] of nibbles (whole 256-row chunks plus one pad step), then [NT][G][32] pairs
    of 4 bytes, rounded up to 256."""
    NT = (N + 31) // 32
    KS = (K + 255) // 256 * 4 + 1
    return (NT * KS * 1024 + NT * G * 128 + 255) // 256 * 256


def plan(which, T, K, N, G, E_=E, top_k=TOP_K, ring=RING):
    """info[0:14] of tgis_debug_moe_gptq_plan.  which: 0 up, 1 down form 0, 2 down form 1."""
    NT, KS = (N + 31) // 32, (K + 63) // 64
    if which == 0:
        scratch = 0
    elif which == 1:
        scratch = (T + 31) // 32 * top_k * 32 * NT * 32 * 4
    else:
        scratch = T * top_k * N * 4
    stride = prepared_bytes(K, N, G)
    return [NT, E_, 256, 4, (KS + 3) // 4, ring, 4 * 64 * 16 * 4, 32, 16 if which == 0 else 32,
            (T * (N // 4) + 255) // 256 if which == 2 else 0, scratch & 0x7fffffff, scratch >> 31,
            stride & 0x7fffffff, stride >> 31]
