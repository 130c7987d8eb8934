"""-m gpu: routing and grouped expert GEMMs for up to 128 experts (csrc/moe_tiles.h: tgis_moe_route_tiles,
tgis_moe_tile_gemm_up, tgis_moe_tile_gemm_down) against the fp64 restatement of tests/moe_ref.py, with the bounds of
tests/moe_bounds.py.

Route: a route block holds 32 tokens, so T 63 / 64 / 65 puts the last token one short of, on and one past a block boundary.
GEMMs: a tile holds 64 rows and a block 128 image columns; the hand-written routing gives experts 0, 1, 63, 64, 65 and 130 rows,
the up N (2 I = 32, 96, 160) and the down N (64, 136, 768) are below one column block or leave its last one partly empty, and
K 136 ends inside a k64-step.  The images of experts nobody chose hold NaN."""
import pytest
import torch

from tests import moe_bounds as mb
from tests import moe_ref

pytestmark = pytest.mark.gpu

ROUTE_CASES = ((2, 1), (64, 8), (65, 8), (128, 8), (128, 1))
ROUTE_TOKENS = (1, 63, 64, 65)


@pytest.fixture(autouse=True)
def _the_rule_decides():
    yield
    from tgis_amd import native

    native.moe_tile_force(-1)


def _route_logits(pattern, T, E, top_k):
    g = torch.Generator().manual_seed(131 * T + E + top_k)
    if pattern == "random":
        return torch.randn(T, E, generator=g) * 2.0
    if pattern == "ties":
        return torch.randn(T, 1, generator=g).expand(T, E).contiguous()
    ids = torch.arange(E - top_k, E).flip(0).repeat(T, 1)  # "same": one expert list per chosen expert holds all T tokens
    return mb.logits_for(ids, E)


def _check_tiles(r, E):
    """The tile list cuts every expert's range of slot_rows into consecutive tiles of up to R rows, experts ascending."""
    tiles, counts, offsets = r.tiles.cpu().tolist(), r.counts.tolist(), r.offsets.tolist()
    n, R = tiles[0][0], tiles[0][1]
    want = [[e, offsets[e] + i, min(R, counts[e] - i)] for e in range(E) for i in range(0, counts[e], R)]
    assert R == 64 and n == len(want) <= r.tile_bound == -(-r.T * r.top_k // R) + min(E, r.T * r.top_k)
    assert [t[:3] for t in tiles[1:1 + n]] == want


@pytest.mark.parametrize("renorm", (1, 0))
@pytest.mark.parametrize("pattern", ("random", "ties", "same"))
@pytest.mark.parametrize("E,top_k", ROUTE_CASES, ids=lambda v: str(v))
def test_route_tiles_matches_the_restatement(gpu_device, E, top_k, pattern, renorm):
    from tgis_amd import native

    for T in ROUTE_TOKENS:
        logits = _route_logits(pattern, T, E, top_k)
        r = native.moe_route_tiles(logits.to(gpu_device), top_k, renorm=bool(renorm))
        ids, w = moe_ref.route(logits, top_k)
        w = w if renorm else torch.softmax(logits.double(), dim=-1).gather(1, ids)  # the full softmax's, as they are
        counts, offsets, slot_rows = moe_ref.lists(ids, E)
        assert torch.equal(r.expert_ids.cpu().long(), ids), T
        assert torch.equal(r.counts.cpu().long(), counts) and torch.equal(r.offsets.cpu().long(), offsets), T
        assert torch.equal(r.slot_rows.cpu().long(), slot_rows), T
        wf = w.float()  # within 4 ulp of fp32 of the fp64 weight: tests/moe_bounds.check_weights' criterion
        ulp = (torch.nextafter(wf, torch.full_like(wf, 2.0)) - wf).double()
        assert ((r.expert_w.cpu().double() - w).abs() <= 4 * ulp).all(), T
        _check_tiles(r, E)
        if E <= 64 and renorm:  # the same bytes as tgis_moe_route
            old = native.moe_route(logits.to(gpu_device), top_k)
            for name in ("expert_ids", "expert_w", "lists", "slot_rows"):
                assert torch.equal(getattr(r, name), getattr(old, name)), (T, name)


# ---- tile GEMMs -------------------------------------------------------------------------------------------------------------
def _row_count_ids():
    """[200, 2] over 8 experts: expert 0 gets no row, 1 one, 2 R - 1 = 63, 3 R = 64, 4 R + 1 = 65, 5 2 R + 2 = 130 (6 and 7: the rest)."""
    first = [5] * 130 + [4] * 65 + [6] * 5
    second = [3] * 64 + [2] * 63 + [1] + [7] * 72
    return torch.tensor([first, second]).t().contiguous()


def _run(dev, ids, E, K, I, dt, what):
    from tgis_amd import native

    T, top_k = ids.shape
    w1, w3 = mb.up_weights(E, I, K, dt)
    w2 = mb.down_weights(E, K, I, dt)
    chosen = set(ids.reshape(-1).tolist())
    up_w = mb.poisoned(native.MoeWeights(lambda e: torch.cat([w1[e], w3[e]]).to(dev), E, gate_up=True), chosen)
    down_w = mb.poisoned(native.MoeWeights(lambda e: w2[e].to(dev), E), chosen)
    x = mb.up_input(T, K, dt)
    r = native.moe_route_tiles(mb.logits_for(ids, E).to(dev), top_k)
    assert torch.equal(r.expert_ids.cpu().long(), ids)

    h = native.moe_tile_gemm_up(x.to(dev), up_w, r)
    mb.close(h, *mb.up_reference(x, w1, w3, ids, dt), what + " up")
    yref, ytol = mb.down_reference(h.cpu(), w2, ids, r.expert_w.cpu())
    out = native.moe_tile_gemm_down(h, down_w, r, partial=False)
    mb.close(out, *mb.finished_reference(yref, ytol, dt), what + " down finished")
    p = native.moe_tile_gemm_down(h, down_w, r, partial=True)
    assert p.S == top_k and p.shape == (T, K)
    mb.close(mb.slab_rows(p, T), yref, ytol, what + " down slabs")
    # the slab form finished by the add + RMSNorm behind the block
    gen = torch.Generator().manual_seed(77)
    residual = torch.randn(T, K, generator=gen).to(dt)
    weight = (1.0 + 0.1 * torch.randn(K, generator=gen)).to(dt)
    y_p, res_p = native.rmsnorm_residual(p, residual.to(dev), weight.to(dev), 1e-5)
    res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, 1e-5, dt)
    mb.close(res_p, res, dres, what + " residual stream")
    mb.close(y_p, y, dy, what + " normed")
    # a down projection over a deep k: random h [T top_k, K] through images [E, 2 I, K]
    h2, w2b = mb.down_input(T, top_k, K, dt), mb.down_weights(E, 2 * I, K, dt)
    deep_w = mb.poisoned(native.MoeWeights(lambda e: w2b[e].to(dev), E), chosen)
    out2 = native.moe_tile_gemm_down(h2.to(dev), deep_w, r, partial=False)
    mb.close(out2, *mb.finished_reference(*mb.down_reference(h2, w2b, ids, r.expert_w.cpu()), dt), what + " deep down")
    # two runs, the same bytes
    again = native.moe_tile_gemm_up(x.to(dev), up_w, r)
    assert torch.equal(h, again) and torch.equal(out, native.moe_tile_gemm_down(again, down_w, r, partial=False)), what


@pytest.mark.parametrize("dt", mb.DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("I", (16, 48, 80))
@pytest.mark.parametrize("K", (64, 136, 768))
def test_tile_gemms_at_every_row_count(gpu_device, K, I, dt):
    from tgis_amd import native

    assert not native.moe_tile_plan(0, 200, K, 2 * I, 8, 2)["slab_body"]
    _run(gpu_device, _row_count_ids(), 8, K, I, dt, f"K {K} I {I} {dt} rows 0..130")


@pytest.mark.parametrize("dt", mb.DTYPES, ids=("f16", "bf16"))
def test_tile_gemms_over_128_experts(gpu_device, dt):
    g = torch.Generator().manual_seed(33)  # [33, 8] over 128 experts: most experts get 0 - 3 rows
    ids = torch.stack([torch.randperm(128, generator=g)[:8] for _ in range(33)])
    _run(gpu_device, ids, 128, 136, 48, dt, f"E 128 top-8 T 33 {dt}")


@pytest.mark.parametrize("dt", mb.DTYPES, ids=("f16", "bf16"))
@pytest.mark.parametrize("force", (-1, 0, 1), ids=("rule", "tile", "slab"))
def test_both_kernels_behind_a_few_rows(gpu_device, force, dt):
    """T = 5 under the small-T rule, under the tile kernel (tiles of 1 - 3 rows) and under the slab kernel body."""
    from tgis_amd import native

    native.moe_tile_force(force)
    assert force < 0 or native.moe_tile_plan(0, 5, 136, 96, 8, 2)["slab_body"] == force
    _run(gpu_device, mb.pattern("uniform", 5), 8, 136, 48, dt, f"T 5 {dt} force {force}")
