"""CPU: the case tables of tests/test_moe_edges_gpu.py (tests/moe_cases.py) reach what they claim, checked without a GPU: the
k64-steps per k-part by the kernel's rule, the near-tied and underflowing router rows' properties, the landing places of a far
expert image's offset cut to 32 bits, and that every GPU case's reference runs and gives finite, positive bounds."""
import pytest
import torch

from tests import far_pool as fp
from tests import moe_bounds as mb
from tests import moe_cases as mc
from tests import moe_ref


# ---- k-parts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", sorted({**mc.DEEP_K, **mc.SHORT_K}))
def test_steps_per_k_part_are_the_claimed_ones(K):
    steps, tail = {**mc.DEEP_K, **mc.SHORT_K}[K]
    assert mc.k_parts(K) == steps and sum(steps) == mc.cdiv(K, 64)
    assert mc.last_step_columns(K) == tail and K % 8 == 0


def test_the_deep_cases_reach_every_state_of_the_ring():
    """A k-part of exactly RING steps (no refill), RING + 1 (one refill), 2 RING (every slot refilled, a full second pass)
    and 2 RING + 1 (a slot refilled twice); tails that end in the lower and in the upper 32 k-slots of a step."""
    assert set(mc.DEEP_UP_K) | set(mc.DEEP_DOWN_K) == set(mc.DEEP_K) and set(mc.DEEP_UP_K) <= set(mc.DEEP_DOWN_K)
    for K in mc.DEEP_K:
        assert K > 1024 or max(mc.k_parts(K)) == mc.RING
    for up_or_down in (mc.DEEP_UP_K, mc.DEEP_DOWN_K):
        deepest = {max(mc.k_parts(K)) for K in up_or_down}
        assert deepest == {mc.RING, mc.RING + 1, 2 * mc.RING, 2 * mc.RING + 1}
        tails = {mc.last_step_columns(K) for K in up_or_down}
        assert any(t <= 32 for t in tails) and any(32 < t < 64 for t in tails) and 64 in tails
    # the refill is never reached by the shapes of tests/test_moe_ops_gpu.py, which is why these cases exist
    assert all(max(mc.k_parts(K)) <= mc.RING for K in (mc.HIDDEN,) + mc.INTERMEDIATES)
    assert mc.DEEP_ROWS == ((1, "uniform"), (33, "same_two"), (33, "uniform"))
    assert mc.cdiv(2 * mc.DEEP_I, 32) == 3 and mc.cdiv(mc.DEEP_DOWN_N, 32) == 3 and mc.DEEP_DOWN_N % 32 == 8


def test_the_short_cases_reach_idle_waves_and_both_halves_of_a_step():
    parts = {K: mc.k_parts(K) for K in mc.SHORT_K}
    assert parts[8] == parts[64] == (1, 0, 0, 0) and parts[72] == (1, 1, 0, 0) and parts[200] == (1, 1, 1, 1)
    assert any(0 in p for p in parts.values())
    assert mc.last_step_columns(72) == mc.last_step_columns(200) == 8 and mc.last_step_columns(296) == 40
    assert mc.SHORT_I % 16 == 0 and mc.SHORT_DOWN_N % 4 == 0 and mc.SHORT_DOWN_N % 32 != 0


def test_the_routings_are_the_admitted_corners():
    assert {(2, 1), (2, 2), (8, 8), (64, 8)} <= set(mc.MIX_ROUTINGS)  # E and top_k at both ends of check_mixtral_config's range
    assert all(2 <= E <= 64 and 1 <= k <= min(E, 8) for E, k in mc.MIX_ROUTINGS + mc.EDGE_ROUTE_CASES + mc.EDGE_ROUTE_SMALL)
    assert {k for _E, k in mc.MIX_ROUTINGS} >= set(mc.NORM_TOP_K) | set(mc.SLAB_TOP_K)
    assert min(mc.EDGE_ROUTE_TOKENS) == 1024 and max(mc.EDGE_ROUTE_TOKENS) > 2 * 1024 > max(mc.ROUTE_TOKENS)
    assert mc.EDGE_ROUTE_STRIDED[2] > mc.EDGE_ROUTE_STRIDED[0] == 64


# ---- hand-written router rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(len(mc.NEAR_TIES)))
def test_near_tied_rows_collide_in_fp32_only(n):
    row, top_k, tied, ids = mc.NEAR_TIES[n]
    logits = torch.tensor([row], dtype=torch.float32)
    tied = list(tied)
    assert len(set(logits[0, tied].tolist())) == len(tied), "the fp32 logits must differ"
    assert (logits[0, tied][1:] > logits[0, tied][:-1]).all(), "the larger logits sit at the higher indices"
    p = torch.softmax(logits.double(), dim=-1)[0]
    assert len(set(p[tied].tolist())) == len(tied), "the fp64 probabilities must differ"
    assert len(set(p.float()[tied].tolist())) == 1, "the fp32 probabilities must collide"
    got, w = moe_ref.route(logits, top_k)
    assert got[0].tolist() == list(ids)
    # what an order decided in fp64 would have chosen differs: the test can tell the two apart
    assert torch.topk(p, top_k).indices.tolist() != list(ids)
    if set(ids) <= set(tied):
        assert torch.allclose(w[0], torch.full((top_k,), 1.0 / top_k, dtype=torch.float64), atol=1e-8, rtol=0)


def test_the_issue_row_has_the_reported_probability():
    p = torch.softmax(torch.tensor(mc.NEAR_TIES[0][0], dtype=torch.float32).double(), dim=-1).float()
    assert p[0] == p[1] == p[4] and abs(float(p[0]) - 0.246535167) < 1e-8
    assert any(len(row[3]) == 3 and set(row[3]) <= set(row[2]) for row in mc.NEAR_TIES)  # top_k = 3 taking all three


@pytest.mark.parametrize("n", range(len(mc.UNDERFLOW)))
def test_underflowing_rows_leave_one_fp32_probability(n):
    row, top_k, ids = mc.UNDERFLOW[n]
    logits = torch.tensor([row], dtype=torch.float32)
    top = max(row)
    assert all(v == top or 110 <= top - v <= 200 for v in row) and row.count(top) == 1
    p = torch.softmax(logits.double(), dim=-1)[0]
    assert (p > 0).all() and int((p.float() > 0).sum()) == 1
    assert float(p.sort().values[-2]) < 2.0 ** -150  # rounds to zero in fp32, flushed or not
    got, w = moe_ref.route(logits, top_k)
    free = [e for e in range(len(row)) if e != row.index(top)]
    assert got[0].tolist() == list(ids) == [row.index(top)] + free[:top_k - 1]
    assert w.float()[0].tolist() == [1.0] + [0.0] * (top_k - 1) and float(w.sum()) == 1.0


# ---- far expert images ----------------------------------------------------------------------------------------------------------
def test_far_image_offsets_cut_to_32_bits_land_in_the_fill():
    """Offsets are bytes from the first gate|up image, FAR_BASE bytes above the arena's start.  Every 4 KiB block of every
    image, as e * stride alone and as the whole offset, cut to 32 bits (signed or unsigned) stays inside the arena and meets
    no image of either set."""
    images = [shift + e * mc.FAR_STRIDE for shift in (0, mc.FAR_DOWN_SHIFT) for e in range(mc.FAR_E)]
    n = mc.FAR_IMAGE_BYTES
    assert n == mc.cdiv(2 * mc.FAR_I, 32) * mc.cdiv(mc.FAR_K, 64) * 4096 == mc.cdiv(mc.FAR_DOWN_N, 32) * mc.cdiv(mc.FAR_K, 64) * 4096
    assert mc.FAR_ARENA_BYTES % 8 == 0 and mc.FAR_ARENA_BYTES <= 9 * fp.GIB and mc.FAR_ARENA_BYTES == mc.FAR_BASE + max(images) + n
    assert 2 * mc.FAR_STRIDE >= 1 << 31 and 4 * mc.FAR_STRIDE >= 1 << 32 and mc.FAR_STRIDE < 1 << 31
    assert sorted({e for pair in mc.FAR_IDS for e in pair}) == list(range(mc.FAR_E))  # every expert is read
    looked = 0
    for shift in (0, mc.FAR_DOWN_SHIFT):
        for e in range(mc.FAR_E):
            off = e * mc.FAR_STRIDE
            lands = []
            for w in fp.wrapped(off, 1):  # the product alone is cut, the rest of the address is right
                lands += [(shift + w + b, 4096) for b in range(0, n, 4096)]
            for b in range(0, n, 4096):   # the whole offset of a block is cut
                lands += fp.wrapped_ranges(shift + off + b, 4096, 1)
                lands += [(shift + lo, m) for lo, m in fp.wrapped_ranges(off + b, 4096, 1)]
            if e >= 2:
                assert lands, f"expert {e}: no 32-bit cut changes its offset"
            for lo, m in lands:
                looked += 1
                assert -mc.FAR_BASE <= lo and lo + m <= mc.FAR_ARENA_BYTES - mc.FAR_BASE, f"expert {e}: [{lo}, {lo + m}) leaves the arena"
                for im in images:
                    assert lo + m <= im or im + n <= lo, f"expert {e}: [{lo}, {lo + m}) meets the image at {im}"
    assert looked >= 2 * 3 * 4


# ---- every GPU case's reference -------------------------------------------------------------------------------------------------
def _positive(ref, tol, what):
    assert torch.isfinite(ref).all() and torch.isfinite(tol).all() and (tol > 0).all(), what
    assert (tol < 0.05 * (ref.abs().max() + 1)).all(), f"{what}: a bound as wide as the values checks nothing"


def _up(dt, T, K, I, E, ids):
    w1, w3 = mb.up_weights(E, I, K, dt)
    _positive(*mb.up_reference(mb.up_input(T, K, dt), w1, w3, ids, dt), f"up {dt} T {T} K {K} I {I} E {E}")


def _down(dt, T, K, N, E, ids, w):
    yref, ytol = mb.down_reference(mb.down_input(T, ids.shape[1], K, dt), mb.down_weights(E, N, K, dt), ids, w)
    _positive(yref, ytol, f"down {dt} T {T} K {K} N {N} E {E}")
    _positive(*mb.finished_reference(yref, ytol, dt), f"finished {dt} T {T} K {K} N {N} E {E}")
    return yref, ytol


@pytest.mark.parametrize("dt", mb.DTYPES, ids=("f16", "bf16"))
def test_every_gpu_case_has_a_reference_and_finite_positive_bounds(dt):
    ran = []
    for T, name in mc.DEEP_ROWS:
        ids = mb.pattern(name, T)
        w = moe_ref.route(mb.logits_for(ids, mc.E), mc.TOP_K)[1]
        for K in mc.DEEP_UP_K:
            _up(dt, T, K, mc.DEEP_I, mc.E, ids)
            ran.append((0, T, K, 2 * mc.DEEP_I, mc.E, mc.TOP_K))
        for K in mc.DEEP_DOWN_K:
            _down(dt, T, K, mc.DEEP_DOWN_N, mc.E, ids, w)
            ran += [(f, T, K, mc.DEEP_DOWN_N, mc.E, mc.TOP_K) for f in (1, 2)]
    for T in mc.SHORT_TOKENS:
        ids = mb.pattern("uniform", T)
        w = moe_ref.route(mb.logits_for(ids, mc.E), mc.TOP_K)[1]
        for K in mc.SHORT_K:
            _up(dt, T, K, mc.SHORT_I, mc.E, ids)
            _down(dt, T, K, mc.SHORT_DOWN_N, mc.E, ids, w)
            ran += [(0, T, K, 2 * mc.SHORT_I, mc.E, mc.TOP_K)] + [(f, T, K, mc.SHORT_DOWN_N, mc.E, mc.TOP_K) for f in (1, 2)]
    for E, top_k in mc.MIX_ROUTINGS:
        for T in mc.MIX_TOKENS:
            ids, w = moe_ref.route(mb.mix_logits(T, E, top_k), top_k)
            _up(dt, T, mc.HIDDEN, mc.MIX_I, E, ids)
            yref, ytol = _down(dt, T, mc.MIX_I, mc.HIDDEN, E, ids, w)
            ran += [(f, T, (mc.HIDDEN, mc.MIX_I)[f > 0], (2 * mc.MIX_I, mc.HIDDEN)[f > 0], E, top_k) for f in (0, 1, 2)]
            if E == mc.E and top_k in mc.NORM_TOP_K and T == mc.NORM_T:
                gen = torch.Generator().manual_seed(77 + top_k)
                residual = torch.randn(T, mc.HIDDEN, generator=gen).to(dt)
                weight = (1.0 + 0.1 * torch.randn(mc.HIDDEN, generator=gen)).to(dt)
                res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, 1e-5, dt)
                _positive(res, dres, f"residual stream top_k {top_k}")
                _positive(y, dy, f"normed top_k {top_k}")
    for top_k in mc.SLAB_TOP_K:
        for T in mc.SLAB_TOKENS:
            ids, w = moe_ref.route(mb.mix_logits(T, mc.E, top_k), top_k)
            h = mb.down_input(T, top_k, mc.MIX_I, dt)
            _positive(*mb.down_reference(h, mb.down_weights(mc.E, mc.HIDDEN, mc.MIX_I, dt)[:, :mc.SLAB_N], ids, w), "narrow slabs")
            ran += [(0, T, mc.HIDDEN, 2 * mc.MIX_I, mc.E, top_k), (1, T, mc.MIX_I, mc.SLAB_N, mc.E, top_k)]
    ids = mb.pattern("uniform", mc.STRIDE_T)
    w = moe_ref.route(mb.logits_for(ids, mc.E), mc.TOP_K)[1]
    _up(dt, mc.STRIDE_T, mc.HIDDEN, mc.STRIDE_I, mc.E, ids)
    _down(dt, mc.STRIDE_T, mc.STRIDE_I, mc.HIDDEN, mc.E, ids, w)
    ran += [(0, mc.STRIDE_T, mc.HIDDEN, 2 * mc.STRIDE_I, mc.E, mc.TOP_K), (2, mc.STRIDE_T, mc.STRIDE_I, mc.HIDDEN, mc.E, mc.TOP_K)]
    ids = torch.tensor(mc.FAR_IDS)
    logits = mb.logits_for(ids, mc.FAR_E)
    got, w = moe_ref.route(logits, mc.FAR_TOP_K)
    assert torch.equal(got, ids)
    _up(dt, len(mc.FAR_IDS), mc.FAR_K, mc.FAR_I, mc.FAR_E, ids)
    _down(dt, len(mc.FAR_IDS), mc.FAR_K, mc.FAR_DOWN_N, mc.FAR_E, ids, w)
    ran += [(f, len(mc.FAR_IDS), mc.FAR_K, 64, mc.FAR_E, mc.FAR_TOP_K) for f in (0, 1, 2)]
    # every launch the plan test holds against tgis_debug_moe_plan is one of these, and the other way round
    assert set(ran) == set(mc.edge_gemm_cases()) and set(mc.edge_gemm_cases()) <= set(mc.plan_cases())


def test_hand_written_logits_give_the_patterns_they_were_written_for():
    for T, name in mc.DEEP_ROWS + tuple((T, "uniform") for T in mc.SHORT_TOKENS):
        ids = mb.pattern(name, T)
        assert torch.equal(moe_ref.route(mb.logits_for(ids, mc.E), mc.TOP_K)[0], ids)
    counts = moe_ref.lists(mb.pattern("same_two", 33), mc.E)[0]
    assert counts.tolist() == [0, 0, 33, 0, 0, 33, 0, 0]  # 33 rows: two slabs, the ring primed twice
    ids = moe_ref.route(mb.mix_logits(1, 64, 2), 2)[0]
    assert len(set(ids.reshape(-1).tolist())) == 2  # 62 of 64 images hold NaN
