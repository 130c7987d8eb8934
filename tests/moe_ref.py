"""fp64 restatement of the routed expert MLP (csrc/moe.hip): routing, the list builder and the experts, with the kernels'
rounding points as an option.  TEST INFRASTRUCTURE: pure torch on the CPU, shared by the CPU and the GPU tests.

Semantics are transformers' MixtralTopKRouter / MixtralExperts: softmax over all E experts, the top_k largest (ties to the
lower index here; torch.topk leaves ties open), those renormalised to sum 1; every token runs its top_k experts' SiLU MLPs,
scaled by the weights and summed."""
import torch


def route(logits: torch.Tensor, top_k: int):
    """(ids int64 [T, top_k], weights fp64 [T, top_k]) of router logits [T, E], evaluated in fp64.  The order is decided
    on the probabilities rounded to fp32 (what torch.topk sees in transformers), ties going to the lower index."""
    p = torch.softmax(logits.double(), dim=-1)
    order = p.float().double()
    T, E = p.shape
    ids = torch.empty((T, top_k), dtype=torch.int64)
    for k in range(top_k):
        # argmax of a stable descending sort = the first (lowest) index among equals
        best = torch.sort(order, dim=-1, descending=True, stable=True).indices[:, 0]
        ids[:, k] = best
        order.scatter_(1, best[:, None], -1.0)
    w = p.gather(1, ids)
    return ids, w / w.sum(dim=-1, keepdim=True)


def lists(ids: torch.Tensor, E: int):
    """(counts [E], offsets [E + 1], slot_rows [T top_k]) of expert ids [T, top_k]: the slots t * top_k + k grouped by
    expert, ascending inside each expert."""
    flat = ids.reshape(-1)
    counts = torch.bincount(flat, minlength=E)[:E]
    offsets = torch.zeros(E + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    slot_rows = torch.sort(flat, stable=True).indices
    return counts, offsets, slot_rows


def silu(v: torch.Tensor) -> torch.Tensor:
    return v / (1.0 + torch.exp(-v))


def _rnd(t: torch.Tensor, dt) -> torch.Tensor:
    return t if dt is None else t.to(dt).double()


def expert_up(x, w1, w3, ids, dt=None, absolute=False):
    """h fp64 [T top_k, I]: silu(x W1[e]^T) * (x W3[e]^T) per slot.  x [T, hidden], w1 / w3 [E, I, hidden].  dt: the model
    dtype whose rounding points the kernel has — T(T(silu(T gate)) * T up); None: exact.  absolute: instead return the pair
    (x W1[e]^T, x W3[e]^T) per slot, unrounded, for a caller that derives error bounds from |x| and |W|."""
    T, top_k = ids.shape
    xd, flat = x.double(), ids.reshape(-1)
    tokens = torch.arange(T * top_k) // top_k
    g = torch.empty((T * top_k, w1.shape[1]), dtype=torch.float64)
    u = torch.empty_like(g)
    for e in flat.unique().tolist():
        rows = (flat == e).nonzero()[:, 0]
        g[rows] = xd[tokens[rows]] @ w1[e].double().t()
        u[rows] = xd[tokens[rows]] @ w3[e].double().t()
    if absolute:
        return g, u
    return _rnd(_rnd(silu(_rnd(g, dt)), dt) * _rnd(u, dt), dt)


def expert_down(h, w2, ids, w=None):
    """y fp64 [T, top_k, hidden]: (h[slot] W2[e]^T) * w[slot], unrounded (w None: unscaled).  w2 [E, hidden, I]."""
    T, top_k = ids.shape
    hd, flat = h.double(), ids.reshape(-1)
    y = torch.empty((T * top_k, w2.shape[1]), dtype=torch.float64)
    for e in flat.unique().tolist():
        rows = (flat == e).nonzero()[:, 0]
        y[rows] = hd[rows] @ w2[e].double().t()
    if w is not None:
        y = y * w.double().reshape(-1, 1)
    return y.reshape(T, top_k, -1)


def moe_block(x, gate, w1, w3, w2, top_k, dt=None, ids=None):
    """The whole block in fp64: [T, hidden].  ids: override the routing's choice (the weights stay the router's for those
    experts, renormalised)."""
    logits = x.double() @ gate.double().t()
    rid, rw = route(logits, top_k)
    if ids is not None:
        p = torch.softmax(logits, dim=-1).gather(1, ids)
        rid, rw = ids, p / p.sum(dim=-1, keepdim=True)
    h = expert_up(x, w1, w3, rid, dt)
    return expert_down(h, w2, rid, rw).sum(dim=1)
