"""fp64 restatement of the LoRA kernels' contract (include/tgis_hip.h, csrc/lora.hip).  TEST INFRASTRUCTURE: needs no GPU.

A wrapped linear gives y[t] = W x[t] + scale_s B_s (A_s x[t]) with s = slot[t]; a row with slot[t] = -1 gives W x[t].  An adapter
of a linear is (A [P, r, K], B [N, r], scale): P projections fused into the base linear share the input, projection p owns the
output columns bounds[p] .. bounds[p + 1]."""
import torch


def group(slot, S):
    """(counts [S], offsets [S + 1], rows): the rows that name a slot, grouped by slot, ascending inside each."""
    slot = torch.as_tensor(slot).long()
    counts = torch.tensor([int((slot == s).sum()) for s in range(S)], dtype=torch.long)
    offsets = torch.zeros(S + 1, dtype=torch.long)
    offsets[1:] = torch.cumsum(counts, 0)
    rows = torch.cat([(slot == s).nonzero().flatten() for s in range(S)]) if S else torch.zeros(0, dtype=torch.long)
    return counts, offsets, rows


def shrink(x, adapters, slot):
    """{t: v [P, r_s] in fp64} for the rows that have a slot: v[p] = A_s[p] x[t]."""
    out = {}
    for t, s in enumerate(torch.as_tensor(slot).tolist()):
        if s >= 0:
            A = adapters[s][0].double()
            out[t] = torch.einsum("prk,k->pr", A, x[t].double())
    return out


def delta(x, adapters, slot, bounds):
    """(d, sh, ex) fp64 [T, N], zero rows where slot[t] = -1:
         d[t, n]  = scale_s sum_r v[t, p(n), r] B_s[n, r], the delta;
         sh[t, n] = |scale_s| sum_r (|A_s[p]| |x[t]|)_r |B_s[n, r]|: what an error of the shrink's sums over K is proportional to;
         ex[t, n] = |scale_s| sum_r |v[t, p, r]| |B_s[n, r]|: what an error of the expand's sum over r is proportional to."""
    T, N = x.shape[0], bounds[-1]
    d, sh, ex = (torch.zeros(T, N, dtype=torch.float64) for _ in range(3))
    for t, s in enumerate(torch.as_tensor(slot).tolist()):
        if s < 0:
            continue
        A, B, scale = adapters[s]
        A, B = A.double(), B.double()
        v = torch.einsum("prk,k->pr", A, x[t].double())
        va = torch.einsum("prk,k->pr", A.abs(), x[t].double().abs())
        for p in range(len(bounds) - 1):
            n0, n1 = bounds[p], bounds[p + 1]
            d[t, n0:n1] = scale * (B[n0:n1] @ v[p])
            sh[t, n0:n1] = abs(scale) * (B[n0:n1].abs() @ va[p])
            ex[t, n0:n1] = abs(scale) * (B[n0:n1].abs() @ v[p].abs())
    return d, sh, ex


def linear(y0, x, adapters, slot, bounds):
    """fp64 [T, N]: the base GEMM's output y0 plus every row's delta."""
    return y0.double() + delta(x, adapters, slot, bounds)[0]
