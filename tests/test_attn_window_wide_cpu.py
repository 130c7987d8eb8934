"""CPU: the cases of tests/test_attn_window_wide_gpu.py (sliding windows wider than four pages) reach the loops they are there
for.  The page walk of both windowed kernels is restated in tests/attn_window_walk.py; here it is held against the library's
plan (tgis_debug_attn_plan_window) and the fp64 restatement's visibility (tests/attn_window_ref.py), and the coverage
conditions of the GPU grid (tests/attn_window_wide_cases.py) are asserted from it: conditions on the cases, not measurements
of a kernel.

Two conditions hold in a narrower form than one might wish, for arithmetic reasons:
  * a window of 129 keys shows at most 5 pages, so no wave visits more than 2 of them: the W 129 cases are held to 2 pages per
    wave (the first window at which a wave loops at all), every wider one to 3;
  * a prefill "case" is one (window, geometry) with its three batches.  With q_len = ctx a GQA block (32 q rows or fewer) never
    straddles a page edge, so only the suffix batch can skip a page by the upper bound."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_window_ref as ref  # noqa: E402
import attn_window_walk as wk  # noqa: E402
import attn_window_wide_cases as wc  # noqa: E402
import pytest  # noqa: E402
from attn_window_plan import query_window_plan  # noqa: E402
from test_kv_layout_cpu import _cdiv, _library_or_skip  # noqa: E402

NS_GRID = (1,) + wc.EXPLICIT_SPLITS


@pytest.fixture(scope="module")
def lib():
    return _library_or_skip()


def _all_decode_ctxs(W):
    return sorted(set(wc.window_ctxs(W)) | set(wc.split_ctxs(W)))


# ---- the helper against the library and the restatement -------------------------------------------------------------------------
def test_decode_walk_first_page_and_key(lib):
    for W in wc.WINDOWS:
        seqs = [(1, c) for c in _all_decode_ctxs(W)]
        got = query_window_plan(lib, 3, 8, 2, 128, 1, 1, W, seqs)
        assert got is not None, lib.tgis_last_error()
        for (_, ctx), (page, key) in zip(seqs, got["first"]):
            walk = wk.decode_walk(ctx, W)
            assert walk.klo == key == ref.first_visible_key(ctx, 1, 0, W), (ctx, W)
            assert walk.pfirst == page == ref.first_visible_page(ctx, 1, W), (ctx, W)
            assert 1 <= walk.pages - walk.pfirst <= _cdiv(W + 31, 32), (ctx, W)


def test_decode_walk_visits_every_visible_page_once():
    """The division itself: over the waves of all splits, each page of [pfirst, pages) exactly once; the masked loop takes the
    page the window starts inside and the page that is being filled, the mask-free loop only pages every key of which the q row
    sees."""
    for W in wc.WINDOWS:
        vis_rows = {}
        for ctx in _all_decode_ctxs(W):
            vis = vis_rows[ctx] = ref.visible(ctx, 1, W)[0]
            for ns in NS_GRID:
                walk = wk.decode_walk(ctx, W, ns)
                assert wk.visited(walk) == list(range(walk.pfirst, walk.pages)), (ctx, W, ns)
                assert walk.splits[0].pbeg == walk.pfirst and all(s.pend <= walk.pages for s in walk.splits)
                for s in walk.splits:
                    assert s.pend - s.pbeg <= walk.pps
                    for w in range(wk.NW):
                        for p in s.full[w]:
                            assert 32 * p + 32 <= ctx and bool(vis[32 * p:32 * p + 32].all()), (ctx, W, ns, p)
                        for p in s.masked[w]:
                            assert bool(vis[32 * p:32 * p + 32].any()), (ctx, W, ns, p)
            assert not bool(vis[:32 * wk.decode_walk(ctx, W).pfirst].any())


def test_prefill_walk_against_the_visibility_matrix():
    """Brute force: a skipped page holds no key any row of the wave sees, a mask-free page only keys every row of the wave sees,
    and no row of a block sees a key outside the block's page loop."""
    seen = {wk.SKIP_LO: 0, wk.SKIP_HI: 0, wk.MASKED: 0, wk.FREE: 0}
    for W in wc.PREFILL_WINDOWS:
        for ql, ctx in sorted({s for batch in wc.PREFILL_BATCHES for s in batch}):
            vis = ref.visible(ctx, ql, W)
            for H, Hkv in wc.GEOMS:
                Gp, TQ = wk.geom(H, Hkv)
                for blk in wk.prefill_walk(ql, ctx, W, Gp, TQ):
                    rows = [t for wv in blk.waves for t in wv.rows]
                    assert rows and rows[0] == blk.t0
                    assert not bool(vis[rows, :32 * blk.p0].any()) and not bool(vis[rows, 32 * blk.pages:].any())
                    assert blk.p0 == ref.first_visible_key(ctx, ql, blk.t0, W) // 32
                    for wv in blk.waves:
                        for p, form in wv.forms.items():
                            if not wv.rows:
                                assert form == wk.SKIP_HI  # a wave past the sequence's rows computes nothing
                                continue
                            page = vis[wv.rows, 32 * p:32 * p + 32]
                            seen[form] += 1
                            if form in (wk.SKIP_LO, wk.SKIP_HI):
                                assert not bool(page.any()), (W, ql, ctx, H, Hkv, blk.t0, p, form)
                            elif form == wk.FREE:
                                assert page.shape[1] == 32 and bool(page.all()), (W, ql, ctx, H, Hkv, blk.t0, p)
                            else:
                                assert bool(page.any())  # (a masked page that no row sees would be wasted, not wrong)
    assert all(seen.values()), seen


# ---- the plan at the new windows ------------------------------------------------------------------------------------------------
def test_decode_form_plan_at_wide_windows(lib):
    for H, Hkv in wc.GEOMS:
        Gp, TQ = wk.geom(H, Hkv)
        HC = (H // Hkv + 15) // 16
        for D in (64, 96, 128):
            for W in wc.WINDOWS:
                for B in (3, 5):
                    for ns in NS_GRID:
                        got = query_window_plan(lib, B, H, Hkv, D, 1, ns, W)
                        assert got is not None, lib.tgis_last_error()
                        p = got["plan"]
                        want = {"form": "window", "nw": wk.NW, "ch": 1, "pipe": 0, "hcb": HC, "xcd_remap": 0,
                                "grid": (1, Hkv * HC, B * ns), "lds": (4 * D * 16 + 4 * 2 * 16) * 4,
                                "merge": "none" if ns == 1 else "fused", "gp": Gp, "tq": TQ, "hc": HC, "ns": ns}
                        assert {k: p[k] for k in want} == want, (H, Hkv, D, W, B, ns)


def test_prefill_form_plan_at_wide_windows(lib):
    for _name, _dt, H, Hkv, D in wc.PREFILL:
        Gp, TQ = wk.geom(H, Hkv)
        HC = (H // Hkv + 15) // 16
        for W in wc.PREFILL_WINDOWS:
            for batch in wc.PREFILL_BATCHES:
                q = max(ql for ql, _ in batch)
                got = query_window_plan(lib, len(batch), H, Hkv, D, q, 1, W, list(batch))
                assert got is not None, lib.tgis_last_error()
                p = got["plan"]
                assert (p["form"], p["grid"], p["lds"], p["merge"]) == ("prefill", (_cdiv(q, TQ * 8), Hkv * HC, len(batch)),
                                                                         2 * 2 * 32 * D * 2, "none"), (H, Hkv, W, q)
                for (ql, ctx), (page, key) in zip(batch, got["first"]):
                    assert key == ref.first_visible_key(ctx, ql, 0, W) and page == ref.first_visible_page(ctx, ql, W)
                    assert page == wk.prefill_walk(ql, ctx, W, Gp, TQ)[0].p0


# ---- what the GPU cases rely on -------------------------------------------------------------------------------------------------
def test_every_decode_case_has_a_wave_that_loops():
    for W in wc.WINDOWS:
        need = 2 if W == 129 else 3  # (129 keys show at most 5 pages: 2 for wave 0, and no window shows that wave fewer loops)
        for batch in wc.decode_batches(W):
            assert max(batch) > W  # a windowed launch
            assert max(wk.max_pages_per_wave(wk.decode_walk(c, W)) for c in batch) >= need, (W, batch)
    assert max(wk.max_pages_per_wave(wk.decode_walk(c, 129)) for c in wc.window_ctxs(129)) == 2
    assert wk.max_pages_per_wave(wk.decode_walk(2 * 4096 + 5, 4096)) == 33  # the production width: 129 pages over 4 waves


def test_decode_cases_reach_the_low_page_paths():
    walks = [(W, c, wk.decode_walk(c, W)) for W in wc.WINDOWS for c in wc.window_ctxs(W)]
    # wave 0 of split 0 goes on into the mask-free loop behind the `low` page, with a reloaded table entry and a prefetch
    assert any(wk.full_after_low(wlk) >= 2 for _, _, wlk in walks)
    for W in wc.WINDOWS[1:]:
        assert any(wk.full_after_low(wk.decode_walk(c, W)) >= 2 for c in wc.window_ctxs(W)), W
    # ... and its masked loop jumps from the `low` page to its partly filled last page (nxt = pp_top)
    jumps = [(W, c) for W, c, wlk in walks
             if wlk.splits[0].low[0] and len(wlk.splits[0].masked[0]) == 2 and wlk.splits[0].masked[0][1] - wlk.pfirst > wk.NW]
    assert jumps, "no case in which wave 0 owns the low page, mask-free pages and the last page"
    # the window starting on a page edge or not x the sequence ending on one or not
    combos = {(wlk.klo % 32 == 0, c % 32 == 0) for W, c, wlk in walks if c > W}
    assert combos == {(True, True), (True, False), (False, True), (False, False)}, combos
    for W in wc.WINDOWS:
        if W % 32:
            c = wc.aligned_ctx(W)
            assert (c - W) % 32 == 0 and c % 32 != 0 and c in wc.window_ctxs(W)
            assert not wk.low_exists(wk.decode_walk(c, W))
    # a `low` page exists exactly when the window starts inside a page that is not the sequence's last
    for W, c, wlk in walks:
        assert wk.low_exists(wlk) == (wlk.klo % 32 != 0 and wlk.pfirst < c >> 5), (W, c)


def test_split_cases_own_many_pages_and_leave_splits_empty():
    for W, _name, _dt, _H, _Hkv, _D, ctxs, _splits in wc.split_cases():
        assert {1, 31, 33} < set(ctxs) and max(ctxs) > W
    W = 1000
    ctxs = wc.split_ctxs(W)
    top = wk.decode_walk(max(ctxs), W)
    assert top.pages - top.pfirst >= 32
    for ns in wc.EXPLICIT_SPLITS:
        for c in ctxs:
            wlk = wk.decode_walk(c, W, ns)
            if c in (1, 31, 33):  # one page (33: two, one per split): every split behind them is unreached
                assert wk.empty_splits(wlk) == list(range(_cdiv(c, 32), ns)), (c, ns)
    assert wk.decode_walk(max(ctxs), W, 2).pps > wk.NW and wk.decode_walk(max(ctxs), W, 5).pps > wk.NW  # a split's waves loop
    assert wk.max_pages_per_wave(wk.decode_walk(max(ctxs), W, 2)) >= 3
    assert len(wk.empty_splits(wk.decode_walk(max(ctxs), W, 40))) >= 1 and wk.decode_walk(max(ctxs), W, 40).pps == 1
    assert any(n > 8 for n in wc.EXPLICIT_SPLITS)  # the merge in batches of 8 records
    # at the production width even the rule's splits (8 at most for these shapes) own more than four pages each
    assert wk.decode_walk(2 * 4096 + 5, 4096, 8).pps > wk.NW


def test_prefill_cases_mostly_take_the_mask_free_form():
    for W in wc.PREFILL_WINDOWS:
        for name, _dt, H, Hkv, _D in wc.PREFILL:
            Gp, TQ = wk.geom(H, Hkv)
            total = {wk.SKIP_LO: 0, wk.SKIP_HI: 0, wk.MASKED: 0, wk.FREE: 0}
            for batch in wc.PREFILL_BATCHES:
                assert max(ctx for _, ctx in batch) > W
                for ql, ctx in batch:
                    for form, n in wk.prefill_counts(wk.prefill_walk(ql, ctx, W, Gp, TQ)).items():
                        total[form] += n
            assert 2 * total[wk.FREE] >= total[wk.FREE] + total[wk.MASKED], (W, name, total)
            assert total[wk.SKIP_LO] >= 1 and total[wk.SKIP_HI] >= 1, (W, name, total)
    # mask-free pages UNDER A LOWER BOUND (lo_full > 0): what a window of 40 never reaches with MHA
    for W in wc.PREFILL_WINDOWS:
        for H, Hkv in wc.GEOMS:
            n = sum(1 for blk in wk.prefill_walk(700, 700, W, *wk.geom(H, Hkv)) for wv in blk.waves
                    if wv.lo_full > 0 for f in wv.forms.values() if f == wk.FREE)
            assert n >= 20, (W, H, Hkv, n)
    # (a full MHA wave, 32 rows: the keys all of them see under W 40 are 9, never a page)
    assert not any(f == wk.FREE for blk in wk.prefill_walk(200, 200, 40, 1, 16) for wv in blk.waves
                   if wv.lo_full > 0 and len(wv.rows) == 32 for f in wv.forms.values())
