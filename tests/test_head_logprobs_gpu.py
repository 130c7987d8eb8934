"""-m gpu: native.head_logprobs (tgis_head_logprobs) against the three formulas restated in fp64 on the CPU, from the same
16-bit inputs.  Tolerances come from the inputs: products of two 16-bit numbers are exact in fp32, what remains is the
summation and the exp / log error, bound[t] = (K + 2 log2 V) 2^-23 max_v sum_k |x[t,k] W[v,k]|.

Most rows take one of the row's three highest reference logits as target (there the logits lie far apart and the reference
rank is one value), rows 0 .. 2 columns 0, V - 1 and one of the last partial tile (the bulk), rows 3, 4 and the last -1."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SPLITS = "S"  # V = 128 S (+ 1): S the splits of the host rule for that T, every split one tile (then one with a lone column)
CASES = [  # T, V, K, dtype, ldx - K, log2 of the scale of x
    (1, 1, 16, torch.float16, 0, 0),
    (1, 32003, 1024, torch.bfloat16, 0, 0),
    (63, 127, 208, torch.bfloat16, 0, 0),
    (63, (SPLITS, 1), 16, torch.float16, 0, 0),
    (63, (SPLITS, 0), 1024, torch.float16, 0, 0),
    (129, 1000, 1024, torch.float16, 0, 0),
    (129, (SPLITS, 1), 208, torch.float16, 0, 0),
    (129, 127, 1024, torch.float16, 0, 6),  # |z| reaches about 1e4: exp(z) without the running max overflows
    (260, 1, 208, torch.float16, 0, 0),
    (260, 1000, 1024, torch.bfloat16, 24, 0),
    (260, (SPLITS, 0), 16, torch.bfloat16, 0, 0),
    (260, 32003, 208, torch.float16, 0, 0),
]


def _splits(T, V):
    from tgis_amd import native

    s = ctypes.c_int()
    native.load_library().tgis_head_logprobs_bytes(T, V, ctypes.byref(s))
    return s.value


def _inputs(T, V, K, dtype, pad, scale, seed):
    g = torch.Generator().manual_seed(seed)
    xp = (torch.randn(T, K + pad, generator=g) * 2.0 ** scale).to(dtype)  # rows ldx = K + pad apart
    w = torch.randn(V, K, generator=g).to(dtype)
    z = xp[:, :K].double() @ w.double().T
    targets = z.topk(min(3, V), dim=1).indices[torch.arange(T), torch.arange(T) % min(3, V)]
    if T > 8:
        targets[0], targets[1], targets[2] = 0, V - 1, V - 1 - (V % 128) // 2
        targets[3] = targets[4] = targets[-1] = -1
    return xp, w, z, targets


@pytest.mark.parametrize("T,V,K,dtype,pad,scale", CASES)
def test_head_logprobs_matches_fp64(gpu_device, T, V, K, dtype, pad, scale):
    from tgis_amd import native

    if isinstance(V, tuple):
        V = 128 * _splits(T, 1 << 30) + V[1]
    xp, w, z, targets = _inputs(T, V, K, dtype, pad, scale, seed=T + K)
    bound = (K + 2 * math.log2(V)) * 2.0 ** -23 * (xp[:, :K].double().abs() @ w.double().abs().T).amax(dim=1)
    wanted = targets >= 0
    zt = z.gather(1, targets.clamp(min=0)[:, None])
    ref_lse = torch.logsumexp(z, dim=1)
    lo = 1 + (z > zt + 2 * bound[:, None]).sum(dim=1)
    hi = 1 + ((z >= zt - 2 * bound[:, None]).sum(dim=1) - 1)  # (the target itself is within its own margin)
    assert (lo == hi)[wanted].double().mean() >= 0.9, "the case must pin the rank of at least 90 % of its rows"

    dev = [xp.to(gpu_device)[:, :K], w.to(gpu_device), targets.to(gpu_device)]
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    lp, rank, lse = native.head_logprobs(*dev)
    if (T, V) == (260, 32003):  # the logits are never stored
        assert torch.cuda.max_memory_allocated() - before < T * V * 4
    lp, rank, lse = lp.cpu().double(), rank.cpu().long(), lse.cpu().double()
    print(f"max |lse - ref| / bound = {((lse - ref_lse).abs() / bound).max():.3g}, "
          f"max |logprob - ref| / bound = {((lp - (zt[:, 0] - ref_lse)).abs() / bound)[wanted].max():.3g}")
    assert ((lse - ref_lse).abs() <= bound).all()
    assert ((lp - (zt[:, 0] - ref_lse)).abs() <= 2 * bound)[wanted].all()
    assert ((rank >= lo) & (rank <= hi))[wanted].all()
    assert lp[~wanted].isnan().all() and (rank[~wanted] == 0).all()
    assert not scale or z.abs().max() > 5e3

