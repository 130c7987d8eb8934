"""References, error bounds and input builders shared by the routed-expert GPU tests (tests/test_moe_ops_gpu.py,
tests/test_moe_edges_gpu.py).  TEST INFRASTRUCTURE: importing this file needs no GPU (tests/test_moe_edges_cpu.py runs every
reference on the CPU).

All references are tests/moe_ref.py in fp64.  Per-element bounds are derived as tests/test_gemm_edges_gpu.py derives them: fp32
accumulation over K columns costs B_ACC K 2^-24 per unit of |x| @ |W|, an output rounding A_OUT unit roundoffs of |ref|; the
SiLU * up epilogue propagates the two sums' errors through T(T(silu(T g)) * T up).  K is always the case's own: the second
dimension of the activation the kernel was given."""
import functools

import torch

from tests import moe_ref

A_OUT = 2.0  # unit roundoffs of the output per |ref|
B_ACC = 2.0  # fp32 accumulation: K 2^-24 per unit of |x| @ |W|
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}
DTYPES = (torch.float16, torch.bfloat16)


# ---- routing ----------------------------------------------------------------------------------------------------------------
def check_weights(got, w):
    """Routing weights `got` (fp32) against the fp64 ones: within 4 ulp of fp32, rows summing to 1."""
    wf = w.float()
    ulp = (torch.nextafter(wf, torch.full_like(wf, 2.0)) - wf).double()
    err = (got.double() - w).abs()
    assert (err <= 4 * ulp).all(), f"routing weight off by {float((err / ulp).max()):.2f} ulp"
    assert torch.allclose(got.sum(dim=1), torch.ones(got.shape[0]), atol=1e-6, rtol=0)


def check_routing(logits_cpu, r, E, top_k):
    ids, w = moe_ref.route(logits_cpu, top_k)
    counts, offsets, slot_rows = moe_ref.lists(ids, E)
    assert torch.equal(r.expert_ids.cpu().long(), ids)
    assert torch.equal(r.counts.cpu().long(), counts) and torch.equal(r.offsets.cpu().long(), offsets)
    assert torch.equal(r.slot_rows.cpu().long(), slot_rows)
    check_weights(r.expert_w.cpu(), w)


def logits_for(ids, E):
    """Hand-written router logits whose top-k are ids[t] in order: top_k + 2 down to 3 there (4 and 3 for a pair), noise in
    [-1, 0) elsewhere."""
    T, top_k = ids.shape
    g = torch.Generator().manual_seed(T)
    logits = -torch.rand(T, E, generator=g)
    for k in range(top_k):
        logits.scatter_(1, ids[:, k:k + 1], float(top_k + 2 - k))
    return logits


def pattern(name, T, E=8):
    """Expert ids [T, 2] of a routing pattern over 8 experts, or None where T cannot hold it."""
    assert E == 8
    g = torch.Generator().manual_seed(T + len(name))
    if name == "uniform":
        return torch.stack([torch.randperm(E, generator=g)[:2] for _ in range(T)])
    if name == "same_two":  # lists of T rows for experts 2 and 5 (longer than one and two slabs at T 33 / 65); six experts idle
        return torch.tensor([[5, 2]]).repeat(T, 1)
    if name == "exactly_32":  # expert 3 holds exactly 32 rows, the others share the rest
        if T < 32:
            return None
        others = [e for e in range(E) if e != 3]
        ids = torch.tensor([[others[t % 7], others[(t + 3) % 7]] for t in range(T)])
        ids[:32, 1] = 3
        return ids
    if name == "last_token_alone":  # expert 7 holds only the last token
        ids = torch.tensor([[t % 3, 3 + t % 4] for t in range(T)])
        ids[T - 1, 0] = 7
        return ids
    raise KeyError(name)


PATTERNS = ("uniform", "same_two", "exactly_32", "last_token_alone")


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def activations(T, K, dt, gen):
    """[T, K] in dt with a non-zero mean: a weight step that is skipped, doubled or swapped moves the sums by far more than
    the bound."""
    return ((torch.randn(T, K, generator=gen) * 0.5 + 0.25)).to(dt)


def padded(x, pad):
    """x as the first columns of a matrix `pad` columns wider whose other columns are NaN: a view with row stride K + pad."""
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=x.device)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


@functools.lru_cache(maxsize=None)
def up_weights(E, I, K, dt):
    """(w1, w3) [E, I, K] on the CPU in dt, i.i.d. with standard deviation K^-1/2; made once per shape and dtype."""
    g = torch.Generator().manual_seed(1000 * K + 8 * I + E)
    w1 = (torch.randn(E, I, K, generator=g) * K ** -0.5).to(dt)
    w3 = (torch.randn(E, I, K, generator=g) * K ** -0.5).to(dt)
    return w1, w3


@functools.lru_cache(maxsize=None)
def down_weights(E, N, K, dt):
    """w2 [E, N, K] on the CPU in dt, i.i.d. with standard deviation K^-1/2; made once per shape and dtype."""
    g = torch.Generator().manual_seed(1000 * K + 8 * N + E + 1)
    return (torch.randn(E, N, K, generator=g) * K ** -0.5).to(dt)


def up_input(T, K, dt):
    """The x [T, K] of the edge cases' up GEMMs."""
    return activations(T, K, dt, torch.Generator().manual_seed(7 * T + K))


def down_input(T, top_k, K, dt):
    """The h [T top_k, K] of the edge cases' down GEMMs: random in the model dtype, not an up GEMM's output."""
    return activations(T * top_k, K, dt, torch.Generator().manual_seed(11 * T + K + top_k))


def mix_logits(T, E, top_k):
    """Seeded random router logits [T, E] at the scale of the route tests."""
    g = torch.Generator().manual_seed(10007 * T + 100 * E + top_k)
    return torch.randn(T, E, generator=g) * 2.0


def poisoned(mw, chosen):
    """A copy of the images with NaN in every expert outside `chosen`."""
    from tgis_amd import native

    twin = native.MoeWeights.__new__(native.MoeWeights)
    twin.__dict__.update(mw.__dict__)
    twin.image = mw.image.clone()
    for e in range(mw.E):
        if e not in chosen:
            twin.image[e].view(mw.dtype).fill_(float("nan"))
    return twin


# ---- references and bounds --------------------------------------------------------------------------------------------------
def up_reference(x, w1, w3, ids, dt):
    """(h, tol) [T top_k, I] of SiLU(gate) * up with the kernel's rounding points, from x [T, K], w1 / w3 [E, I, K]."""
    u, K = U[dt], x.shape[1]
    g, up = moe_ref.expert_up(x, w1, w3, ids, absolute=True)
    ag, au = moe_ref.expert_up(x.double().abs(), w1.double().abs(), w3.double().abs(), ids, absolute=True)
    eg, eu = B_ACC * K * 2.0 ** -24 * ag, B_ACC * K * 2.0 ** -24 * au
    rnd = lambda t: t.to(dt).double()  # noqa: E731
    gr, ur = rnd(g), rnd(up)
    sl = rnd(moe_ref.silu(gr))
    ref = rnd(sl * ur)
    dg = 2 * (eg + u * g.abs()) + TINY[dt]
    du = 2 * (eu + u * up.abs()) + TINY[dt]
    tol = A_OUT * u * ref.abs() + ur.abs() * (1.1 * dg + 2 * u * sl.abs()) + (sl.abs() + 1.1 * dg) * du + TINY[dt]
    return ref, tol


def down_reference(h, w2, ids, w):
    """(y, tol) [T, top_k, N] of the scaled fp32 rows, from the h [T top_k, K] the kernel was given and w2 [E, N, K]."""
    K = h.shape[1]
    y0 = moe_ref.expert_down(h, w2, ids)
    a0 = moe_ref.expert_down(h.double().abs(), w2.double().abs(), ids)
    wd = w.double().reshape(ids.shape[0], ids.shape[1], 1)
    u32 = U[torch.float32]
    tol = (B_ACC * K * 2.0 ** -24 * a0 + A_OUT * u32 * y0.abs()) * wd + u32 * (y0 * wd).abs() + TINY[torch.float32]
    return y0 * wd, tol


def sum_tol(yref, ytol):
    """The bound of the fp32 sum over k of rows known to ytol: the rows' own bounds, and one fp32 roundoff of at most the sum
    of |y| for each of the top_k - 1 additions (one for a pair, none for a single row)."""
    return ytol.sum(dim=1) + (yref.shape[1] - 1) * U[torch.float32] * yref.abs().sum(dim=1)


def finished_reference(yref, ytol, dt):
    """(out, tol) [T, N] of the finished form: the sum over k rounded once to dt."""
    total = yref.sum(dim=1)
    return total.to(dt).double(), sum_tol(yref, ytol) + A_OUT * U[dt] * total.abs() + TINY[dt]


def norm_reference(total, total_tol, residual, weight, eps, dt):
    """(res, res_tol, y, y_tol) of the add + RMSNorm behind the block, from the fp64 sum `total` known to `total_tol`."""
    u = U[dt]
    x = total.to(dt).double()
    dx = total_tol + A_OUT * u * total.abs() + TINY[dt]
    res = (x + residual.double())
    res_r = res.to(dt).double()
    dres = dx + A_OUT * u * res.abs() + TINY[dt]
    hidden = res.shape[1]
    s2 = (res * res).sum(dim=1, keepdim=True)
    rstd = torch.rsqrt(s2 / hidden + eps)
    # d(rstd) / rstd = -1/2 d(s2) / (s2 + hidden eps), d(s2) <= 2 sum |res| dres, plus fp32 roundoff of the sum
    drel = ((res.abs() * dres).sum(dim=1, keepdim=True) / (s2 + hidden * eps)) + hidden * 2.0 ** -24
    y = res * rstd * weight.double()
    dy = (rstd * weight.double().abs()) * dres + y.abs() * drel + A_OUT * u * y.abs() + TINY[dt]
    return res_r, dres, y.to(dt).double(), dy


def close(got, ref, tol, what):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got - ref).abs()
    bad = err > tol
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at {i}: got "
                             f"{got[i].item():.6g} ref {ref[i].item():.6g} tol {tol[i].item():.3g}")


def slab_rows(p, T):
    """[T, top_k, N] view of a decode-form Partial's slabs."""
    s = p.slabs.view(-1, p.S, 32, p.ld)
    return s.permute(0, 2, 1, 3).reshape(-1, p.S, p.ld)[:T, :, :p.N]


def slab_sum(rows):
    """The fp32 sum of slab rows [T, top_k, N] in the order k = 0..top_k-1: the combine kernel's and the norm's additions."""
    total = rows[:, 0].clone()
    for k in range(1, rows.shape[1]):
        total = total + rows[:, k]
    return total
