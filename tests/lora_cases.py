"""Shapes, slot patterns, input builders and the error bound shared by the LoRA kernel tests (tests/test_lora_ops_gpu.py,
tests/test_lora_cpu.py).  TEST INFRASTRUCTURE: importing this file needs no GPU.

The reference is tests/lora_ref.py in fp64.  The per-element bound is built as tests/moe_bounds.py builds its own, from three
parts: the shrink's fp32 accumulation over K (B_ACC K 2^-24 per unit of |scale| sum_r (|A| |x|)_r |B[n, r]|), the expand's fp32
accumulation over the r16 ranks it reads (B_ACC r16 2^-24 per unit of |scale| sum_r |v_r| |B[n, r]|, plus the fp32 roundoffs of
the scaling and of the addition to the base output), and one rounding of base + delta to the model dtype (A_OUT unit roundoffs
of |ref|)."""
import functools

import torch

from tests import lora_ref
from tests.moe_bounds import A_OUT, B_ACC, TINY, U

S = 4
K = 320                      # 5 k64-steps over the shrink's 8 k-parts: uneven, three of them empty
MAX_RANK = 64
RANKS = (1, 4, 16, 24, 64)
TS = (0, 1, 2, 31, 32, 33, 64)
# (bounds): N 80 as one projection and as two, N 528 (no multiple of the expand's 128-column blocks) as two, and q|k|v of
# 256 | 128 | 128 columns
BOUNDS = {"n80_p1": (0, 80), "n80_p2": (0, 40, 80), "n528_p2": (0, 264, 528), "qkv_p3": (0, 256, 384, 512)}
PATTERNS = ("all_none", "all_one", "round_robin", "last_alone", "mixed")


def pattern(name, T):
    """int32 [T] slots of a row pattern over S = 4 slots."""
    if name == "all_none":
        slot = [-1] * T
    elif name == "all_one":
        slot = [2] * T
    elif name == "round_robin":  # every row another slot, in turn
        slot = [t % S for t in range(T)]
    elif name == "last_alone":  # slot 3 holds only the last row
        slot = [t % 2 for t in range(T)]
        if T:
            slot[-1] = 3
    elif name == "mixed":  # slots mixed with -1
        g = torch.Generator().manual_seed(T + 17)
        slot = (torch.randint(0, S + 1, (T,), generator=g) - 1).tolist()
    else:
        raise KeyError(name)
    return torch.tensor(slot, dtype=torch.int32)


def activations(T, Kx, dt, seed=0):
    """[T, K] in dt with a non-zero mean (tests/moe_bounds.py activations)."""
    g = torch.Generator().manual_seed(7 * T + Kx + seed)
    return (torch.randn(T, Kx, generator=g) * 0.5 + 0.25).to(dt)


def base_output(T, N, dt, seed=0):
    """[T, N] in dt: what the base GEMM left, of the delta's size."""
    g = torch.Generator().manual_seed(13 * T + N + seed)
    return torch.randn(T, N, generator=g).to(dt)


@functools.lru_cache(maxsize=None)
def adapters(ranks, bounds, dt, Kx=K):
    """One adapter per slot, (A [P, r, K], B [N, r], scale) on the CPU in dt: A of standard deviation K^-1/2, B of 1, scales
    of either sign."""
    out = []
    for s, r in enumerate(ranks):
        g = torch.Generator().manual_seed(1000 * r + 10 * len(bounds) + s + bounds[-1])
        A = (torch.randn(len(bounds) - 1, r, Kx, generator=g) * Kx ** -0.5).to(dt)
        B = torch.randn(bounds[-1], r, generator=g).to(dt)
        out.append((A, B, (2.0, -0.5, 0.25, 1.5)[s % 4]))
    return tuple(out)


def images(adps, bounds, dt, device, named=None, Kx=K, max_rank=MAX_RANK):
    """The slot images of `adps` on the device.  named: the slots some row names — every other slot's image is filled with
    NaN, and so is everything in a named slot's image past its rank rounded up to 16 (a kernel that reads any of it shows)."""
    from tgis_amd import native

    w = native.LoraImages(Kx, bounds, len(adps), max_rank, dt, device)
    for s, (A, B, scale) in enumerate(adps):
        w.load(s, [A[p] for p in range(A.shape[0])], [B[bounds[p]:bounds[p + 1]] for p in range(A.shape[0])], scale)
    if named is not None:
        nan = float("nan")
        for s, (A, _B, _scale) in enumerate(adps):
            r16 = (A.shape[1] + 15) // 16 * 16
            if s in named:
                w.A[s, :, r16:].fill_(nan)
                w.B[s, r16 // 16:].fill_(nan)
            else:
                w.A[s].fill_(nan)
                w.B[s].fill_(nan)
    return w


def reference(y0, x, adps, slot, bounds, dt):
    """(ref, tol) [T, N]: the contract's output rounded to dt, and the per-element bound of the module docstring."""
    d, sh, ex = lora_ref.delta(x, adps, slot, bounds)
    total = y0.double() + d
    u32 = U[torch.float32]
    r16 = torch.tensor([0 if s < 0 else (adps[s][0].shape[1] + 15) // 16 * 16 for s in slot.tolist()],
                       dtype=torch.float64).reshape(-1, 1)
    tol = (B_ACC * x.shape[1] * u32 * sh + B_ACC * r16 * u32 * ex + 2 * u32 * (y0.double().abs() + d.abs())
           + A_OUT * U[dt] * total.abs() + TINY[dt])
    return total.to(dt).double(), tol
