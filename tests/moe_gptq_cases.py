"""Shapes, quantised weights and the launch-plan restatement shared by the int4 routed-expert tests
(tests/test_moe_gptq_ops_gpu.py, tests/test_moe_gptq_edges_gpu.py, tests/test_moe_gptq_edges_cpu.py,
tests/test_moe_gptq_plan_cpu.py).  TEST INFRASTRUCTURE: importing this file needs no GPU.

Weights are quantised min/max with oracle.tiny_models.quantize_gptq, as tests/bigcode_gptq_ref.py does.  The reference weight
is W16 = oracle.ops_ref.gptq_dequant(...).half(): (q - z - 1) * s rounded once to f16, which the kernel's dequant8 reproduces
exactly, so the op references and bounds are tests/moe_bounds.py's on W16, with no new constants.  In every matrix column
FORCED_COLUMN has zero point 15 in every group (z + 1 = 16 is not masked back to 4 bits) and nibbles 0 and 15 in its first two
rows.

Group sizes: a group size is listed for a K it divides (quantize_gptq and the entry points both ask for that); -1 is a single
group.  K 64 and K 576 are no multiples of 128, so the 128-row groups of the down GEMM are exercised at K 640 and the deep K
4352; at K 64 the group of 64 rows is the single group.

The second half of the file holds the tables of tests/test_moe_gptq_edges_gpu.py: every admitted group size under step-probe
activations, hand-packed matrices that hold every (nibble, zero point) pair, every admitted routing, strides, and the int4
twin of the far expert images of tests/moe_cases.py."""
import functools

import numpy as np
import torch

from oracle import ops_ref
from oracle.tiny_models import quantize_gptq
from tests import moe_bounds as mb
from tests import moe_cases as mc

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
    return 1 if gs in (-1, K) else K // gs


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
def up_experts(K, I, gs, E_=E):
    """(bundles, w1, w3): per expert the GPTQ tensors of [gate | up] as a [K, 2 I] matrix, and W16 as w1 / w3 [E_, I, K] f16."""
    g = torch.Generator().manual_seed(1000 * K + 8 * I + (gs % 1000) + (0 if E_ == E else 7919 * E_))
    bundles, w1, w3 = [], [], []
    for _ in range(E_):
        w = torch.randn(K, 2 * I, generator=g) * K ** -0.5
        b, w16 = quantize_forced(w, gs)
        bundles.append(b)
        w1.append(w16[:, :I].t().contiguous())
        w3.append(w16[:, I:].t().contiguous())
    return bundles, torch.stack(w1), torch.stack(w3)


@functools.lru_cache(maxsize=None)
def down_experts(K, N, gs, E_=E):
    """(bundles, w2): per expert the GPTQ tensors of a [K, N] down matrix, and W16 as w2 [E_, N, K] f16."""
    g = torch.Generator().manual_seed(1000 * K + 8 * N + (gs % 1000) + 1 + (0 if E_ == E else 7919 * E_))
    bundles, w2 = [], []
    for _ in range(E_):
        b, w16 = quantize_forced(torch.randn(K, N, generator=g) * K ** -0.5, gs)
        bundles.append(b)
        w2.append(w16.t().contiguous())
    return bundles, torch.stack(w2)


def moe_weights(bundles, gs, dev, gate_up=False):
    """native.MoeGptqWeights of the bundles of up_experts / down_experts, one expert per bundle."""
    from tgis_amd import native

    return native.MoeGptqWeights(lambda e: tuple(t.to(dev) for t in bundles[e]) + (4, gs), len(bundles), gate_up=gate_up)


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


# ---- the cases of tests/test_moe_gptq_edges_gpu.py --------------------------------------------------------------------------
DT = torch.float16

# 1. Every admitted group size.  (K, group size): K // 64 steps in k-parts of mc.k_parts(K), groups of gs // 64 steps.
GROUP_CASES = [
    (512, 256),       # k-parts of 2: a group is exactly a k-part pair
    (768, 256),       # k-parts of 3: wave 1 starts on step 3 inside group 0 and crosses into group 1 on step 4
    (1024, 512),      # k-parts of 4, groups of 8 steps: waves 1 and 3 start mid-group
    (1536, 512),      # k-parts of 6: every wave but wave 0 starts mid-group
    (2048, 1024),
    (4096, 2048),
    (8192, 4096),     # spg_shift 6, 7 and 8, two groups each
    (16384, 8192),
    (32768, 16384),
    (1024, 1024),     # one group, written as groupsize == K
    (3584, 128),      # 56 steps in k-parts of 14, 28 groups: 8x7B's down geometry at a quarter of its depth
]
GROUP_I, GROUP_DOWN_N = 32, 64   # two column tiles each: the tile strides nt * KSI and nt * G * 128 are used
GROUP_IDS = (5, 2)               # the two experts every row of a case routes to
GROUP_MAX_PROBED = 8             # more groups than this: only groups 0, 1, G - 2 and G - 1 are probed
GROUP_HOWS = ("half_shift", "no_ks0", "shift_1")


def spg_shift(K, gs):
    """moe_fill_gptq's log2(k64-steps per group): 30 under a single group."""
    G = groups_of(K, gs)
    if G == 1:
        return 30
    shift = 0
    while (64 << shift) < K // G:
        shift += 1
    assert 64 << shift == K // G
    return shift


def part_starts(K):
    """First k64-step (the kernel's ks0) of each of the four waves."""
    starts, at = [], 0
    for n in mc.k_parts(K):
        starts.append(at)
        at += n
    return tuple(starts)


def wave_start(K, step):
    """ks0 of the wave that holds `step`."""
    return max(s0 for s0, n in zip(part_starts(K), mc.k_parts(K)) if n and s0 <= step)


def mid_group_waves(K, gs):
    """The waves whose first step is not the first step of a group."""
    shift = spg_shift(K, gs)
    return tuple(wk for wk, (s0, n) in enumerate(zip(part_starts(K), mc.k_parts(K))) if n and shift < 30 and s0 % (1 << shift))


def group_of(K, gs, step, how="kernel"):
    """The group whose {scale, zero} pair a step is dequantised with.  kernel: Int4Source::load's (ks0 + step) >> spg_shift.
    half_shift: the shift one too small.  no_ks0: the wave's local step alone.  shift_1: the shift capped at 1.  Each is
    clamped to G - 1, as the kernel clamps."""
    G, shift = groups_of(K, gs), spg_shift(K, gs)
    if how == "kernel":
        g = step >> shift
    elif how == "half_shift":
        assert shift >= 1
        g = step >> (shift - 1)
    elif how == "no_ks0":
        g = (step - wave_start(K, step)) >> shift
    elif how == "shift_1":
        g = step >> min(shift, 1)
    else:
        raise KeyError(how)
    return min(g, G - 1)


def probe_steps(K, gs):
    """The probed k64-steps: the first and last step of every group (of groups 0, 1, G - 2, G - 1 when there are more than
    GROUP_MAX_PROBED), the first and last step of every k-part, and step r + RING of every ring slot r of every k-part that
    is that long: the first step each slot is refilled with."""
    G, KS = groups_of(K, gs), K // 64
    per_group = KS // G
    steps = set()
    for g in (range(G) if G <= GROUP_MAX_PROBED else (0, 1, G - 2, G - 1)):
        steps |= {g * per_group, (g + 1) * per_group - 1}
    for s0, n in zip(part_starts(K), mc.k_parts(K)):
        if n:
            steps |= {s0, s0 + n - 1} | {s0 + RING + r for r in range(RING) if RING + r < n}
    return sorted(steps)


def probe_rows(K, gs):
    """The step each probe token probes: every probed step the same number of times, 32 rows or more in all, so that with
    the dense row each of the two experts walks a second 32-row slab."""
    steps = probe_steps(K, gs)
    return [s for s in steps for _ in range(-(-32 // len(steps)))]


def probe_tokens(K, gs):
    return len(probe_rows(K, gs)) + 1


def probe_input(K, gs, per):
    """[T per, K] f16: the `per` rows of token t hold mb.activations values inside k64-step probe_rows[t] and exact zeros
    elsewhere; the last token's rows are dense.  per = 1: the x of the up GEMM; per = TOP_K: the h of the down GEMM."""
    rows = probe_rows(K, gs)
    gen = torch.Generator().manual_seed(31 * K + (gs % 1000) + per)
    x = torch.zeros((len(rows) + 1) * per, K, dtype=DT)
    for t, s in enumerate(rows):
        x[t * per:(t + 1) * per, s * 64:(s + 1) * 64] = mb.activations(per, 64, DT, gen)
    x[len(rows) * per:] = mb.activations(per, K, DT, gen)
    return x


def group_ids(T):
    return torch.tensor([GROUP_IDS]).repeat(T, 1)


@functools.lru_cache(maxsize=None)
def group_experts(which, K, gs):
    """{e: (bundle, W16 [K, N])} for the two experts of GROUP_IDS.  which "up": N = 2 GROUP_I, "down": N = GROUP_DOWN_N.
    The rows of group g are uniform in +-(3 / K)^1/2 (the variance of the other cases' weights) times 2^(g mod 3), so the
    scales of adjacent groups differ by a factor of 2 to 4; uniform, because the range of 128 Gaussian rows varies by more
    than that factor leaves room for."""
    N = 2 * GROUP_I if which == "up" else GROUP_DOWN_N
    G = groups_of(K, gs)
    gen = torch.Generator().manual_seed(1000 * K + 8 * N + (gs % 1000) + 17)
    step_up = (2.0 ** ((torch.arange(K) // (K // G)) % 3)).view(K, 1)
    out = {}
    for e in GROUP_IDS:
        w = (torch.rand(K, N, generator=gen) * 2 - 1) * (3.0 / K) ** 0.5 * step_up
        out[e] = quantize_forced(w, gs)
    return out


def group_bundles(which, K, gs):
    """E bundles for moe_weights: the experts nobody chooses borrow a chosen one's tensors (their images are poisoned)."""
    ex = group_experts(which, K, gs)
    return [ex[e][0] if e in ex else ex[GROUP_IDS[0]][0] for e in range(E)]


def dequant_as(bundle, K, gs, how):
    """W16 of a bundle with every k64-step dequantised under group_of(.., how)."""
    qw, qz, sc, _gi = bundle
    g_of_step = torch.tensor([group_of(K, gs, s, how) for s in range(K // 64)])
    gi = g_of_step.repeat_interleave(64).numpy().astype(np.int32)
    return ops_ref.gptq_dequant(qw.numpy(), qz.numpy(), sc.numpy(), gi, K // groups_of(K, gs)).half()


def stack_up(w16s, I):
    """(w1, w3) [E, I, K] of {e: W16 [K, 2 I]}; the experts without an entry hold NaN."""
    K = next(iter(w16s.values())).shape[0]
    w1 = torch.full((max(E, max(w16s) + 1), I, K), float("nan"), dtype=DT)
    w3 = w1.clone()
    for e, w in w16s.items():
        w1[e], w3[e] = w[:, :I].t(), w[:, I:].t()
    return w1, w3


def stack_down(w16s):
    """w2 [E, N, K] of {e: W16 [K, N]}; the experts without an entry hold NaN."""
    K, N = next(iter(w16s.values())).shape
    w2 = torch.full((max(E, max(w16s) + 1), N, K), float("nan"), dtype=DT)
    for e, w in w16s.items():
        w2[e] = w.t()
    return w2


# 2. Dequantisation, bit for bit.  (K, group size); N 64 (I 32 for the gate|up matrix).
DEQUANT_CASES = [(128, 64), (256, -1)]
DEQUANT_N, DEQUANT_E, DEQUANT_EXPERT = 64, 2, 1
SCALE_LOG2 = (-14, 7)
SCALE_CORNERS = (2.0 ** -14, 4094.0)  # the smallest normal f16, and the largest scale whose 16-fold is finite
BIG_COLUMN = 15  # the column of scale 4094: its stored zero point in group 0 is 15, so it holds (0 - 16) * 4094 = -65504


def hand_nibbles(K, gs, N=DEQUANT_N):
    """(q uint8 [K, N], z uint8 [G, N]) written by hand, no quantiser: the stored zero point of column n in group g is
    (n + 5 g) mod 16, and inside one group the rows that share a nibble position k mod 8 and a lane half (k mod 64) // 32,
    numbered r = 0.. , hold nibble (r + 4 (n // 16) + rot) mod 16 in column n.  r and n // 16 both run over 0..3 at least, so
    each zero point meets all 16 nibbles in every position and half; rot mixes position, half, group and zero point in.
    Every nibble value is equally frequent."""
    G = groups_of(K, gs)
    size = K // G
    k, n = np.arange(K)[:, None], np.arange(N)[None, :]
    pos, half, g = k % 8, (k % 64) // 32, k // size
    r = (k % size) // 64 * 4 + (k % 32) // 8
    z = (np.arange(N)[None, :] + 5 * np.arange(G)[:, None]) % 16
    zk = (n + 5 * g) % 16
    q = (r + 4 * (n // 16) + 3 * pos + 7 * half + 5 * g + 11 * zk) % 16
    return q.astype(np.uint8), z.astype(np.uint8)


def hand_scales(G, N, gen, gate_up):
    """Scales [G, N] f16, log-uniform in [2^-14, 2^7], and SCALE_CORNERS in columns 0 and BIG_COLUMN.  gate_up: the I gate scales and the
    I up scales of a group are paired smallest with largest (the pairs then shuffled), so that silu(gate) * up stays finite
    in f16 (|q - z - 1| <= 16 on either side; asserted below); the 4094 sits in gate column BIG_COLUMN, 2^-14 in its up
    column and in gate column 0, which keeps its partner."""
    lo, hi = SCALE_LOG2
    s = (2.0 ** (lo + (hi - lo) * torch.rand(G, N, generator=gen))).half()
    if gate_up:
        I = N // 2
        for g in range(G):
            perm = torch.randperm(I, generator=gen)
            gate, up = s[g, :I].sort().values, s[g, I:].sort(descending=True).values
            s[g, perm], s[g, I + perm] = gate, up
        s[:, 0], s[:, BIG_COLUMN], s[:, I + BIG_COLUMN] = SCALE_CORNERS[0], SCALE_CORNERS[1], SCALE_CORNERS[0]
        assert (16 * s[:, :I].double() * 16 * s[:, I:].double() < 65504 / 2).all()
    else:
        s[:, 0], s[:, BIG_COLUMN] = SCALE_CORNERS
    assert (s >= 2.0 ** lo).all() and (s <= SCALE_CORNERS[1]).all()
    return s


@functools.lru_cache(maxsize=None)
def dequant_expert(K, gs, gate_up):
    """(bundle, W16 [K, DEQUANT_N]) of the hand-packed matrix."""
    G = groups_of(K, gs)
    q, z = hand_nibbles(K, gs)
    qw, qz = ops_ref.gptq_pack(q, z.astype(np.int64) + 1)
    sc = hand_scales(G, DEQUANT_N, torch.Generator().manual_seed(K + G + int(gate_up)), gate_up)
    gi = (np.arange(K) // (K // G)).astype(np.int32)
    w16 = ops_ref.gptq_dequant(qw, qz, sc.numpy(), gi, K // G).half()
    return (torch.from_numpy(qw), torch.from_numpy(qz), sc, torch.from_numpy(gi)), w16


def dequant_ids(K):
    return torch.full((K, 1), DEQUANT_EXPERT)


# 3. Every admitted routing: mc.MIX_ROUTINGS at mc.MIX_TOKENS, hidden mc.HIDDEN; the down GEMM's K 64 is one group.
MIX_I, MIX_GS = 64, 64
NORM_TOP_K, NORM_T = mc.NORM_TOP_K, mc.NORM_T

# 4. Strides and bytes the kernel must not read (E 8, top-2, the matrices of section 3).
STRIDE_T = 33
STRIDE_PADS = dict(x=8, h=16, out=4)
STRIDE_GAP = 4096                   # bytes of 0xFF between the images under the wide expert stride
PAD_K, PAD_DOWN_N = mc.HIDDEN, 64   # K 320: 9 steps per tile in the image, 5 of them real


def image_steps(K):
    """k64-steps a column tile holds in the image (gptq::prep_layout's KS'): whole 256-row chunks plus one pad step."""
    return (K + 255) // 256 * 4 + 1


# 5. Images past 2^31 and 2^32 bytes: mc's arena geometry, the int4 images of K 128 at groups of 64.
FAR_K, FAR_I, FAR_DOWN_N, FAR_GS = mc.FAR_K, mc.FAR_I, mc.FAR_DOWN_N, 64
FAR_G = FAR_K // FAR_GS
FAR_IMAGE_BYTES = prepared_bytes(FAR_K, FAR_DOWN_N, FAR_G)  # the gate|up matrix is as wide: 2 FAR_I columns


def edge_cases():
    """(which, T, K, N, G, E, top_k) of every GEMM launch of tests/test_moe_gptq_edges_gpu.py, each once."""
    out = []
    for K, gs in GROUP_CASES:
        T, G = probe_tokens(K, gs), groups_of(K, gs)
        out += [(0, T, K, 2 * GROUP_I, G, E, TOP_K), (1, T, K, GROUP_DOWN_N, G, E, TOP_K), (2, T, K, GROUP_DOWN_N, G, E, TOP_K)]
    for K, gs in DEQUANT_CASES:
        out += [(w, K, K, DEQUANT_N, groups_of(K, gs), DEQUANT_E, 1) for w in (0, 1, 2)]
    H, GH = mc.HIDDEN, mc.HIDDEN // MIX_GS
    for E_, k in mc.MIX_ROUTINGS:
        for T in mc.MIX_TOKENS:
            out += [(0, T, H, 2 * MIX_I, GH, E_, k), (1, T, MIX_I, H, 1, E_, k), (2, T, MIX_I, H, 1, E_, k)]
    out += [(0, NORM_T, H, 2 * MIX_I, GH, E, k) for k in NORM_TOP_K] + [(w, NORM_T, MIX_I, H, 1, E, k) for k in NORM_TOP_K for w in (1, 2)]
    T = STRIDE_T
    out += [(0, T, H, 2 * MIX_I, GH, E, TOP_K), (1, T, MIX_I, H, 1, E, TOP_K), (2, T, MIX_I, H, 1, E, TOP_K)]
    out += [(1, T, PAD_K, PAD_DOWN_N, PAD_K // MIX_GS, E, TOP_K), (2, T, PAD_K, PAD_DOWN_N, PAD_K // MIX_GS, E, TOP_K)]
    T = len(mc.FAR_IDS)
    out += [(0, T, FAR_K, 2 * FAR_I, FAR_G, mc.FAR_E, mc.FAR_TOP_K), (1, T, FAR_K, FAR_DOWN_N, FAR_G, mc.FAR_E, mc.FAR_TOP_K),
            (2, T, FAR_K, FAR_DOWN_N, FAR_G, mc.FAR_E, mc.FAR_TOP_K)]
    return list(dict.fromkeys(out))
