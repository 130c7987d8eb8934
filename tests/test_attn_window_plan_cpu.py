"""CPU: the launch plan of sliding-window attention (csrc/attention_plan.h plan_attn with a window, reported by
tgis_debug_attn_plan_window): the form, the grid and, per (ctx, q_len, W), the first visible page and key against the
restatement tests/attn_window_ref.py over the grid of tests/test_attn_window_gpu.py and, for the decode form, the windows of
tests/test_attn_window_wide_gpu.py; its refusals; and that
tgis_debug_attn_plan still answers what the commit before the window did (tests/golden/attn_plan_parent.npz: its info[16] at
every point tests/test_attn_plan_cpu.py asks, recorded from that commit's library)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402
import attn_window_ref as ref  # noqa: E402
import pytest  # noqa: E402
from attn_window_plan import query_window_plan  # noqa: E402
from test_attn_plan_cpu import grid_points  # noqa: E402
from test_kv_layout_cpu import _cdiv, _library_or_skip  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_plan_parent.npz")

# the grid of the GPU file, restated (importing it would import torch and the GPU fixtures)
WINDOWS = (1, 32, 40, 64, 95)
WIDE_WINDOWS = (129, 300, 1000, 1024, 4096)  # tests/test_attn_window_wide_gpu.py's (its own grid: test_attn_window_wide_cpu.py)
GEOMS = ((4, 4), (8, 2), (8, 1), (20, 1))


def window_ctxs(W):
    return sorted({c for c in (1, W - 1, W, W + 1, W + 31, W + 32, 3 * W + 5) if c >= 1})


@pytest.fixture(scope="module")
def lib():
    return _library_or_skip()


def _geom(H, Hkv):
    G = H // Hkv
    Gc = min(G, 16)
    Gp = 1 << (Gc - 1).bit_length()
    return Gp, 16 // Gp, (G + 15) // 16


def test_decode_form_plan_and_visible_range(lib):
    for H, Hkv in GEOMS:
        Gp, TQ, HC = _geom(H, Hkv)
        for D in (64, 96, 128):
            for W in WINDOWS + WIDE_WINDOWS:
                seqs = [(1, c) for c in window_ctxs(W)]
                for ns in (1, 2, 5):
                    got = query_window_plan(lib, 3, H, Hkv, D, 1, ns, W, seqs)
                    assert got is not None, lib.tgis_last_error()
                    p = got["plan"]
                    # the restricted plan: one-chunk blocks of 4 waves, no page pipeline, no XCD remap; the splits of one-chunk
                    # blocks merge in the launch
                    want = {"form": "window", "nw": 4, "ch": 1, "pipe": 0, "hcb": HC, "xcd_remap": 0,
                            "grid": (1, Hkv * HC, 3 * ns), "lds": (4 * D * 16 + 4 * 2 * 16) * 4,
                            "merge": "none" if ns == 1 else "fused", "gp": Gp, "tq": TQ, "hc": HC, "ns": ns}
                    assert {k: p[k] for k in want} == want, (H, Hkv, D, W, ns)
                    for (_, ctx), (page, key) in zip(seqs, got["first"]):
                        assert key == max(0, ctx - W) == ref.first_visible_key(ctx, 1, 0, W), (ctx, W)
                        assert page == key // 32 == ref.first_visible_page(ctx, 1, W), (ctx, W)
                        # the visible pages [page, pages): never more than ceil((W + 31) / 32) of them
                        assert 1 <= _cdiv(ctx, 32) - page <= _cdiv(W + 31, 32), (ctx, W)


def test_prefill_form_plan_and_visible_range(lib):
    seqs = [(1, 1), (31, 31), (97, 97), (200, 200), (5, 150), (2, 2), (3, 70)]
    for H, Hkv in GEOMS:
        Gp, TQ, HC = _geom(H, Hkv)
        for W in (40, 64):
            for q in (2, 5, 97, 200):  # 2 and 5: the decode form of the causal launch
                fit = [s for s in seqs if s[0] <= q]
                got = query_window_plan(lib, 3, H, Hkv, 128, q, 1, W, fit)
                assert got is not None, lib.tgis_last_error()
                p = got["plan"]
                assert (p["form"], p["grid"], p["lds"], p["merge"]) == ("prefill", (_cdiv(q, TQ * 8), Hkv * HC, 3),
                                                                         2 * 2 * 32 * 128 * 2, "none"), (H, Hkv, W, q)
                for (ql, ctx), (page, key) in zip(fit, got["first"]):
                    assert key == ref.first_visible_key(ctx, ql, 0, W) and page == ref.first_visible_page(ctx, ql, W)
                    vis = ref.visible(ctx, ql, W)
                    assert int(vis[0].nonzero()[0]) == key and int(vis.sum(1).max()) <= W and bool(vis.any(1).all())


def test_refusals(lib):
    for args, msg in (((3, 8, 2, 128, 1, 1, 0), b"window 0 must be at least 1"),
                      ((3, 8, 2, 128, 1, 1, -7), b"window -7 must be at least 1"),
                      ((3, 8, 2, 128, 2, 2, 40), b"key splits are for one q token per sequence"),
                      ((3, 8, 2, 128, 200, 3, 40), b"key splits are for one q token per sequence"),
                      ((3, 8, 3, 128, 1, 1, 40), b"multiple of Hkv"), ((3, 8, 2, 80, 1, 1, 40), b"head_dim"),
                      ((0, 8, 2, 128, 1, 1, 40), b"tgis_debug_attn_plan_window")):
        assert query_window_plan(lib, *args) is None, args
        assert msg in lib.tgis_last_error(), (args, lib.tgis_last_error())
    assert query_window_plan(lib, 3, 8, 2, 128, 1, 1, 1 << 40, [(1, 5)])["first"] == [(0, 0)]


def test_causal_plan_is_what_it_was(lib):
    g = np.load(GOLDEN)
    points, info = g["points"], g["info"]
    want_points = list(grid_points()) + [p for p in grid_points(ds=(64, 96)) if p[0] in (1, 8, 128)]
    assert [tuple(int(v) for v in p[:6]) + (bool(p[6]),) for p in points] == want_points, "test_attn_plan_cpu's grid moved"
    for pt, was in zip(want_points, info.tolist()):
        got = ac.query_plan(lib, *pt)
        assert got == (None if was[0] < 0 else was), (pt, was, got)
