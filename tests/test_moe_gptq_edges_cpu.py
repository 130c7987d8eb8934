"""CPU: the case tables of tests/test_moe_gptq_edges_gpu.py (tests/moe_gptq_cases.py) reach what they claim, checked without a
GPU: the k-part splits, the waves that start mid-group and the probed steps of every group-size case against
tests/moe_cases.k_parts; that adjacent groups' scales differ by more than a rounding; that a reference which takes a probed
step's group wrongly (the shift one too small, the wave's first step left out, the shift capped at 1) leaves the bound of the
right one in every probe row whose group it changes; that the hand-packed matrices hold all 256 (nibble, zero point) pairs in
every nibble position and lane half; where a far image's offset cut to 32 bits lands; and that every GPU case's reference runs
and gives finite, positive bounds."""
import numpy as np
import pytest
import torch

from tests import far_pool as fp
from tests import moe_bounds as mb
from tests import moe_cases as mc
from tests import moe_gptq_cases as gc
from tests import moe_ref

DT = gc.DT
E, TOP_K = gc.E, gc.TOP_K
CASE_IDS = [f"K{K}-gs{gs}" for K, gs in gc.GROUP_CASES]

# (K, gs) -> (k64-steps per k-part, spg_shift, waves that start mid-group, groups)
GROUP_TABLE = {
    (512, 256): ((2, 2, 2, 2), 2, (1, 3), 2),
    (768, 256): ((3, 3, 3, 3), 2, (1, 2, 3), 3),
    (1024, 512): ((4, 4, 4, 4), 3, (1, 3), 2),
    (1536, 512): ((6, 6, 6, 6), 3, (1, 2, 3), 3),
    (2048, 1024): ((8, 8, 8, 8), 4, (1, 3), 2),
    (4096, 2048): ((16, 16, 16, 16), 5, (1, 3), 2),
    (8192, 4096): ((32, 32, 32, 32), 6, (1, 3), 2),
    (16384, 8192): ((64, 64, 64, 64), 7, (1, 3), 2),
    (32768, 16384): ((128, 128, 128, 128), 8, (1, 3), 2),
    (1024, 1024): ((4, 4, 4, 4), 30, (), 1),
    (3584, 128): ((14, 14, 14, 14), 1, (), 28),
}


# ---- 1. the group-size tables -------------------------------------------------------------------------------------------------
def test_the_group_cases_are_the_issue_s():
    from tgis_amd import native

    assert list(GROUP_TABLE) == gc.GROUP_CASES
    sizes = {gs for _K, gs in gc.GROUP_CASES}
    assert sizes <= set(native.MOE_GPTQ_GROUP_SIZES) and all(native.moe_gptq_group_ok(gs, K) for K, gs in gc.GROUP_CASES)
    # with 64 and 128 of tests/test_moe_gptq_ops_gpu.py every admitted size runs, so every spg_shift 0..8 and 30
    assert sizes | {64, 128} == set(native.MOE_GPTQ_GROUP_SIZES)
    assert {gc.spg_shift(K, gs) for K, gs in gc.GROUP_CASES} == {1, 2, 3, 4, 5, 6, 7, 8, 30}
    assert gc.RING == mc.RING == 4 and gc.GROUP_I in (16, 32) and gc.GROUP_DOWN_N in (32, 64)


@pytest.mark.parametrize("K,gs", gc.GROUP_CASES, ids=CASE_IDS)
def test_k_parts_groups_and_probed_steps(K, gs):
    parts, shift, mid, G = GROUP_TABLE[(K, gs)]
    KS = K // 64
    assert mc.k_parts(K) == parts and sum(parts) == KS and gc.groups_of(K, gs) == G
    assert gc.spg_shift(K, gs) == shift and (G == 1 or (1 << shift) * G == KS)
    assert gc.mid_group_waves(K, gs) == mid
    starts = gc.part_starts(K)
    assert starts == tuple(wk * parts[0] for wk in range(4))
    # the restated group rule is the quantiser's grouping: rows k // gs
    size = K // G
    assert [gc.group_of(K, gs, s) for s in range(KS)] == [s * 64 // size for s in range(KS)]
    steps = gc.probe_steps(K, gs)
    assert steps == sorted(set(steps)) and 0 <= steps[0] and steps[-1] == KS - 1
    per_group = KS // G
    for g in (range(G) if G <= 8 else (0, 1, G - 2, G - 1)):
        assert {g * per_group, (g + 1) * per_group - 1} <= set(steps), f"group {g}"
    for s0, n in zip(starts, parts):
        assert {s0, s0 + n - 1} <= set(steps)
        assert {s0 + 4 + r for r in range(4) if 4 + r < n} <= set(steps), "the first refill of every ring slot"
    # a wave that starts in another group than 0 shows on its first step that the group is not its local index's; one that
    # starts inside group 0 and leaves it shows on its last; both steps are probed
    for wk in range(1, 4):
        first, last = starts[wk], starts[wk] + parts[wk] - 1
        differs = [s for s in (first, last) if gc.group_of(K, gs, s) != gc.group_of(K, gs, s, "no_ks0")]
        assert differs if gc.group_of(K, gs, last) > 0 else not differs
        assert not differs or gc.group_of(K, gs, first) == 0 or differs[0] == first
    rows = gc.probe_rows(K, gs)
    T = gc.probe_tokens(K, gs)
    assert set(rows) == set(steps) and 33 <= T == len(rows) + 1 <= 130, "two slabs per expert, at most 130 tokens"
    x, h = gc.probe_input(K, gs, 1), gc.probe_input(K, gs, TOP_K)
    assert x.shape == (T, K) and h.shape == (T * TOP_K, K)
    for t, s in enumerate(rows):
        for row in (x[t], h[2 * t], h[2 * t + 1]):
            inside = row[s * 64:(s + 1) * 64]
            assert int((row != 0).sum()) == int((inside != 0).sum()) >= 60, "values inside one k64-step, exact zeros elsewhere"
    assert int((x[-1] != 0).sum()) > K - K // 50 and int((h[-1] != 0).sum()) > K - K // 50  # the dense row


def test_the_named_geometries():
    assert gc.part_starts(768)[1] == 3 and gc.group_of(768, 256, 3) == 0 and gc.group_of(768, 256, 4) == 1
    assert gc.mid_group_waves(1536, 512) == (1, 2, 3)
    # 8x7B's down GEMM: K 14336 at groups of 128 is 224 steps in k-parts of 56; the case is a quarter of that depth
    assert mc.k_parts(14336) == (56, 56, 56, 56) and mc.k_parts(3584) == (14, 14, 14, 14) and 4 * 3584 == 14336
    assert 14 > 3 * gc.RING, "the ring of 4 is refilled three times"
    assert [gc.group_of(3584, 128, s) for s in range(6)] == [0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("K,gs", gc.GROUP_CASES, ids=CASE_IDS)
def test_adjacent_groups_have_scales_a_wrong_group_would_show(K, gs):
    for which in ("up", "down"):
        for e, (bundle, _w16) in gc.group_experts(which, K, gs).items():
            sc = bundle[2].double()
            assert sc.shape[0] == gc.groups_of(K, gs) and (sc > 0).all()
            ratio = sc[1:] / sc[:-1]
            assert ((ratio < 0.75) | (ratio > 1.5)).all(), f"{which} expert {e}: ratios {float(ratio.min())} .. {float(ratio.max())}"


def _changed(K, gs, how):
    """Per probe token: whether `how` takes its step's group wrongly."""
    return [gc.group_of(K, gs, s, how) != gc.group_of(K, gs, s) for s in gc.probe_rows(K, gs)]


def _route_weights(ids, E_):
    got, w = moe_ref.route(mb.logits_for(ids, E_), ids.shape[1])
    assert torch.equal(got, ids)
    return w


@pytest.mark.parametrize("K,gs", gc.GROUP_CASES, ids=CASE_IDS)
def test_a_wrong_group_leaves_the_bound_in_every_probe_row_it_changes(K, gs):
    """The power of the probe rows.  The right reference and its bound, then the reference under each wrong group rule:
    every slot row of every probe token whose step's group the rule changes has an element outside the bound, in the up
    GEMM's h, in the down GEMM's slabs and in the finished rows; the probe rows it does not change are unchanged."""
    T, G = gc.probe_tokens(K, gs), gc.groups_of(K, gs)
    ids = gc.group_ids(T)
    w = _route_weights(ids, E)
    up, down = gc.group_experts("up", K, gs), gc.group_experts("down", K, gs)
    for e in gc.GROUP_IDS:  # group_of("kernel") dequantises to the quantiser's own W16
        assert torch.equal(gc.dequant_as(up[e][0], K, gs, "kernel"), up[e][1])
        assert torch.equal(gc.dequant_as(down[e][0], K, gs, "kernel"), down[e][1])
    x, h = gc.probe_input(K, gs, 1), gc.probe_input(K, gs, TOP_K)
    w1, w3 = gc.stack_up({e: up[e][1] for e in up}, gc.GROUP_I)
    href, htol = mb.up_reference(x, w1, w3, ids, DT)
    yref, ytol = mb.down_reference(h, gc.stack_down({e: down[e][1] for e in down}), ids, w)
    fref, ftol = mb.finished_reference(yref, ytol, DT)
    for t in (href, htol, yref, ytol, fref, ftol):
        assert torch.isfinite(t).all()
    assert (htol > 0).all() and (ytol > 0).all() and (ftol > 0).all()
    shown = 0
    for how in gc.GROUP_HOWS:
        changed = torch.tensor(_changed(K, gs, how))
        if G == 1 or (how == "shift_1" and gc.spg_shift(K, gs) <= 1):  # (a cap at 1 is right for groups of 64 and 128 rows)
            assert not changed.any()
            continue
        assert changed.any(), f"{how}: no probed step shows it"
        w1m, w3m = gc.stack_up({e: gc.dequant_as(up[e][0], K, gs, how) for e in up}, gc.GROUP_I)
        hbad = mb.up_reference(x, w1m, w3m, ids, DT)[0]
        ybad = mb.down_reference(h, gc.stack_down({e: gc.dequant_as(down[e][0], K, gs, how) for e in down}), ids, w)[0]
        fbad = mb.finished_reference(ybad, ytol, DT)[0]
        out_h = ((hbad - href).abs() > htol).any(dim=1).view(T, TOP_K)[:-1]
        out_y = ((ybad - yref).abs() > ytol).any(dim=2)[:-1]
        out_f = ((fbad - fref).abs() > ftol).any(dim=1)[:-1]
        for name, out in (("up", out_h), ("slabs", out_y), ("finished", out_f[:, None])):
            missed = changed[:, None] & ~out
            assert not missed.any(), f"{how} {name}: probe tokens {missed.any(dim=1).nonzero()[:, 0].tolist()} stay inside the bound"
            assert not (out & ~changed[:, None]).any(), f"{how} {name}: an unchanged probe row moved"
        shown += int(changed.sum())
    assert shown > 0 or G == 1


# ---- 2. the hand-packed matrices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,gs", gc.DEQUANT_CASES, ids=lambda v: str(v))
def test_every_nibble_meets_every_zero_point_in_every_position(K, gs):
    G = gc.groups_of(K, gs)
    for gate_up in (False, True):
        (qw, qz, sc, gi), w16 = gc.dequant_expert(K, gs, gate_up)
        N = gc.DEQUANT_N
        assert qw.shape == (K // 8, N) and qz.shape == (G, N // 8) and sc.shape == (G, N) and sc.dtype == torch.float16
        words, zwords = qw.numpy().view(np.uint32), qz.numpy().view(np.uint32)
        k = np.arange(K)
        nib = (words[k // 8] >> (4 * (k % 8))[:, None].astype(np.uint32)) & 15                      # [K, N]
        n = np.arange(N)
        zero = ((zwords[:, n // 8] >> (4 * (n % 8))[None, :].astype(np.uint32)) & 15)[gi.numpy()]  # [K, N]
        for pos in range(8):
            for half in (0, 1):
                rows = (k % 8 == pos) & ((k % 64 >= 32) == bool(half))
                pairs = set((nib[rows] * 16 + zero[rows]).reshape(-1).tolist())
                assert len(pairs) == 256, f"K {K} position {pos} half {half}: {len(pairs)} of 256 pairs"
        assert np.bincount(nib.reshape(-1), minlength=16).tolist() == [K * N // 16] * 16  # no quantiser's mid-range cluster
        d = nib.astype(np.int64) - zero.astype(np.int64) - 1
        assert d.min() == -16 and d.max() == 14
        s = sc.double()
        assert (s >= 2.0 ** -14).all() and (s <= 4094.0).all() and float(s.min()) == 2.0 ** -14 and float(s.max()) == 4094.0
        inner = s[(s > 2.0 ** -14) & (s < 4094.0)]
        assert inner.max() <= 2.0 ** 7 and inner.log2().min() < -12 and inner.log2().max() > 5
        # W16 is the integer times the scale, rounded once; no product is subnormal, none overflows
        want = (torch.from_numpy(d).double() * s[gi.long()]).half()
        assert torch.equal(w16, want) and torch.isfinite(w16).all()
        assert ((w16 == 0) | (w16.abs() >= 2.0 ** -14)).all() and float(w16.abs().max()) == 65504.0
        assert ((w16 == 0) == torch.from_numpy(d == 0)).all()


@pytest.mark.parametrize("K,gs", gc.DEQUANT_CASES, ids=lambda v: str(v))
def test_the_identity_through_the_hand_packed_matrices_has_references(K, gs):
    ids = gc.dequant_ids(K)
    w = _route_weights(ids, gc.DEQUANT_E)
    assert torch.equal(w, torch.ones(K, 1, dtype=torch.float64))
    eye = torch.eye(K, dtype=DT)
    _b, w16 = gc.dequant_expert(K, gs, False)
    yref, ytol = mb.down_reference(eye, gc.stack_down({gc.DEQUANT_EXPERT: w16}), ids, w)
    assert torch.equal(yref[:, 0], w16.double()), "row t of the down GEMM over the identity is row t of W16"
    _b, wgu = gc.dequant_expert(K, gs, True)
    w1, w3 = gc.stack_up({gc.DEQUANT_EXPERT: wgu}, gc.DEQUANT_N // 2)
    ref, tol = mb.up_reference(eye, w1, w3, ids, DT)
    assert torch.isfinite(ref).all() and torch.isfinite(tol).all() and (tol > 0).all()
    assert float(ref.abs().max()) > 1 and int((ref != 0).sum()) > ref.numel() // 4


# ---- 5. far images ----------------------------------------------------------------------------------------------------------------
def test_far_int4_image_offsets_cut_to_32_bits_land_in_the_fill():
    """The layout of the far int4 images restated: image e of the gate|up set sits e * FAR_STRIDE bytes above the first,
    which sits FAR_BASE bytes above the arena's start; the down set FAR_DOWN_SHIFT behind.  e * stride cut to 32 bits, signed
    or unsigned, alone or with the offset of a 256-byte piece of the image (nibbles and {scale, zero} table alike), lands for
    every expert inside the arena and outside every image of either set: a truncated offset reads 0xFF bytes and nothing
    else."""
    n = gc.FAR_IMAGE_BYTES
    assert n == gc.prepared_bytes(gc.FAR_K, 2 * gc.FAR_I, gc.FAR_G) == 2 * 5 * 1024 + 2 * gc.FAR_G * 128 and n % 256 == 0
    assert n <= mc.FAR_DOWN_SHIFT and mc.FAR_DOWN_SHIFT + n <= mc.FAR_STRIDE and mc.FAR_STRIDE % 16 == 0
    images = [shift + e * mc.FAR_STRIDE for shift in (0, mc.FAR_DOWN_SHIFT) for e in range(mc.FAR_E)]
    assert mc.FAR_BASE + max(images) + n <= mc.FAR_ARENA_BYTES <= 9 * fp.GIB
    assert 2 * mc.FAR_STRIDE >= 1 << 31 and 4 * mc.FAR_STRIDE >= 1 << 32 and mc.FAR_STRIDE < 1 << 31
    assert sorted({e for pair in mc.FAR_IDS for e in pair}) == list(range(mc.FAR_E))  # every expert is read
    looked = 0
    for shift in (0, mc.FAR_DOWN_SHIFT):
        for e in range(mc.FAR_E):
            off = e * mc.FAR_STRIDE
            lands = []
            for w in fp.wrapped(off, 1):  # the product alone is cut, the rest of the address is right
                lands.append((shift + w, n))
            for b in range(0, n, 256):    # the whole offset of a piece is cut
                lands += fp.wrapped_ranges(shift + off + b, 256, 1)
                lands += [(shift + lo, m) for lo, m in fp.wrapped_ranges(off + b, 256, 1)]
            if e >= 2:
                assert lands, f"expert {e}: no 32-bit cut changes its offset"
            for lo, m in lands:
                looked += 1
                assert -mc.FAR_BASE <= lo and lo + m <= mc.FAR_ARENA_BYTES - mc.FAR_BASE, f"expert {e}: [{lo}, {lo + m}) leaves the arena"
                for im in images:
                    assert lo + m <= im or im + n <= lo, f"expert {e}: [{lo}, {lo + m}) meets the image at {im}"
    assert looked >= 2 * 3 * 4


# ---- every GPU case's reference, and the list the plan test holds ---------------------------------------------------------------
def _positive(ref, tol, what):
    assert torch.isfinite(ref).all() and torch.isfinite(tol).all() and (tol > 0).all(), what
    assert (tol < 0.05 * (ref.abs().max() + 1)).all(), f"{what}: a bound as wide as the values checks nothing"


def _up(T, K, I, gs, E_, ids):
    _b, w1, w3 = gc.up_experts(K, I, gs, E_)
    _positive(*mb.up_reference(mb.up_input(T, K, DT), w1, w3, ids, DT), f"up T {T} K {K} I {I} E {E_}")


def _down(T, K, N, gs, E_, ids, w):
    _b, w2 = gc.down_experts(K, N, gs, E_)
    yref, ytol = mb.down_reference(mb.down_input(T, ids.shape[1], K, DT), w2, ids, w)
    _positive(yref, ytol, f"down T {T} K {K} N {N} E {E_}")
    _positive(*mb.finished_reference(yref, ytol, DT), f"finished T {T} K {K} N {N} E {E_}")
    return yref, ytol


def test_every_gpu_case_has_a_reference_and_is_in_the_list_of_the_plan_test():
    ran = []
    for K, gs in gc.GROUP_CASES:  # (their references run in the power test above)
        T, G = gc.probe_tokens(K, gs), gc.groups_of(K, gs)
        ran += [(0, T, K, 2 * gc.GROUP_I, G, E, TOP_K)] + [(f, T, K, gc.GROUP_DOWN_N, G, E, TOP_K) for f in (1, 2)]
    for K, gs in gc.DEQUANT_CASES:
        ran += [(f, K, K, gc.DEQUANT_N, gc.groups_of(K, gs), gc.DEQUANT_E, 1) for f in (0, 1, 2)]
    H, I, gs = mc.HIDDEN, gc.MIX_I, gc.MIX_GS
    assert gc.groups_of(H, gs) == 5 and gc.groups_of(I, gs) == 1
    for E_, top_k in mc.MIX_ROUTINGS:
        for T in mc.MIX_TOKENS:
            ids, w = moe_ref.route(mb.mix_logits(T, E_, top_k), top_k)
            _up(T, H, I, gs, E_, ids)
            yref, ytol = _down(T, I, H, gs, E_, ids, w)
            ran += [(0, T, H, 2 * I, 5, E_, top_k), (1, T, I, H, 1, E_, top_k), (2, T, I, H, 1, E_, top_k)]
            if E_ == E and top_k in gc.NORM_TOP_K and T == gc.NORM_T:
                gen = torch.Generator().manual_seed(77 + top_k)
                residual = torch.randn(T, H, generator=gen).to(DT)
                weight = (1.0 + 0.1 * torch.randn(H, generator=gen)).to(DT)
                res, dres, y, dy = mb.norm_reference(yref.sum(dim=1), mb.sum_tol(yref, ytol), residual, weight, 1e-5, DT)
                _positive(res, dres, f"residual stream top_k {top_k}")
                _positive(y, dy, f"normed top_k {top_k}")
    assert {k for _E, k in mc.MIX_ROUTINGS if _E == E} >= set(gc.NORM_TOP_K) and gc.NORM_T in mc.MIX_TOKENS
    T = gc.STRIDE_T
    ids = mb.pattern("uniform", T)
    w = _route_weights(ids, E)
    _up(T, H, I, gs, E, ids)
    _down(T, I, H, gs, E, ids, w)
    _down(T, gc.PAD_K, gc.PAD_DOWN_N, gs, E, ids, w)
    ran += [(0, T, H, 2 * I, 5, E, TOP_K), (1, T, I, H, 1, E, TOP_K), (2, T, I, H, 1, E, TOP_K)]
    ran += [(f, T, gc.PAD_K, gc.PAD_DOWN_N, 5, E, TOP_K) for f in (1, 2)]
    assert gc.image_steps(gc.PAD_K) == 9 and mc.cdiv(gc.PAD_K, 64) == 5 and gc.PAD_K == H
    ids = torch.tensor(mc.FAR_IDS)
    w = _route_weights(ids, mc.FAR_E)
    T = len(mc.FAR_IDS)
    _up(T, gc.FAR_K, gc.FAR_I, gc.FAR_GS, mc.FAR_E, ids)
    _down(T, gc.FAR_K, gc.FAR_DOWN_N, gc.FAR_GS, mc.FAR_E, ids, w)
    ran += [(f, T, gc.FAR_K, 64, gc.FAR_G, mc.FAR_E, mc.FAR_TOP_K) for f in (0, 1, 2)]
    cases = gc.edge_cases()
    assert len(cases) == len(set(cases)) and set(ran) == set(cases)
    identity = [c for c in cases if c[1] == c[2]]  # T = K rows of the identity
    assert len(identity) == 3 * len(gc.DEQUANT_CASES) and all(c[1] <= 130 for c in cases if c not in identity)
