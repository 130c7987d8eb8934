"""CPU: the key-split rule for launches with more than one q token per sequence (tgis_attn_num_splits_q, csrc/attention.hip)
restated and compared with the library, the host-side gate in front of it (native.attn_q_splits), and the bound that lets
tgis_attn_workspace_bytes keep its signature: what it returns for B * max_q_len rows covers both record layouts of every
decode-form launch."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kv_layout_cpu import _cdiv, _library_or_skip, num_splits  # noqa: E402

BS = (1, 2, 3, 4, 8, 16, 32, 64, 128)
HEADS = ((1, 8), (8, 64), (32, 32), (4, 32), (1, 48), (1, 12), (2, 128), (1, 80), (2, 4), (1, 16), (1, 3), (1, 5))
CTXS = (1, 31, 512, 992, 1000, 1023, 1024, 1280, 2048, 4096, 8192, 16384, 32768, 100000)
QS = (1, 2, 4, 8, 16, 64)


def _geom(H, Hkv):
    G = H // Hkv
    Gp = 1 << (min(G, 16) - 1).bit_length()
    return G, Gp, 16 // Gp, _cdiv(G, 16)  # G, padded group, q tokens per tile, 16-head chunks


def prefill_form(H, Hkv, q):
    return q * _geom(H, Hkv)[1] > 64


def num_splits_q(B, Hkv, H, q, ctx):
    """tgis_attn_num_splits_q restated."""
    if q == 1:
        return num_splits(B, Hkv, H, 1, ctx)
    if B <= 0 or Hkv <= 0 or H <= 0 or H % Hkv or q < 1:
        return 1
    _, _, TQ, HC = _geom(H, Hkv)
    if prefill_form(H, Hkv, q) or ctx < 1024:
        return 1
    pages = _cdiv(ctx, 32)
    base = B * Hkv * HC * _cdiv(q, TQ)
    one = 256 // base                                   # one round of blocks on 256 CUs
    ns = min(one, pages // 16)
    ns = max(ns, min(one, pages // 4, 8))               # short contexts: up to 8 splits of >= 4 pages
    if 64 <= base < 256:
        ns = max(ns, min(512 // base, pages // 32))     # a second round of blocks from 32 pages per block on
    return max(1, min(ns, 32))


def _grid():
    for B in BS:
        for Hkv, H in HEADS:
            for ctx in CTXS:
                for q in QS:
                    yield B, Hkv, H, q, ctx


def test_restatement_matches_the_library():
    lib = _library_or_skip()
    for B, Hkv, H, q, ctx in _grid():
        assert lib.tgis_attn_num_splits_q(B, Hkv, H, q, ctx) == num_splits_q(B, Hkv, H, q, ctx), (B, Hkv, H, q, ctx)
    for bad in ((0, 8, 64, 4, 8192), (1, 0, 64, 4, 8192), (1, 8, 0, 4, 8192), (1, 3, 64, 4, 8192), (1, 8, 64, 0, 8192)):
        assert lib.tgis_attn_num_splits_q(*bad) == 1, bad


def test_one_q_token_is_the_old_entry_point():
    lib = _library_or_skip()
    for B, Hkv, H, _, ctx in _grid():
        assert lib.tgis_attn_num_splits_q(B, Hkv, H, 1, ctx) == lib.tgis_attn_num_splits(B, Hkv, H, 1, ctx)


def test_prefill_form_and_short_contexts_take_one_split():
    lib = _library_or_skip()
    seen_prefill = seen_short = 0
    for B, Hkv, H, q, ctx in _grid():
        if q == 1:
            continue
        got = lib.tgis_attn_num_splits_q(B, Hkv, H, q, ctx)
        if prefill_form(H, Hkv, q):
            assert got == 1, ("prefill form", B, Hkv, H, q, ctx)
            seen_prefill += 1
        if _cdiv(ctx, 32) < 32 or ctx < 1024:
            assert got == 1, ("below 32 pages / 1024 keys", B, Hkv, H, q, ctx)
            seen_short += 1
    assert seen_prefill and seen_short


def test_splits_where_the_issue_and_the_model_test_need_them():
    lib = _library_or_skip()
    assert lib.tgis_attn_num_splits_q(1, 32, 32, 4, 8192) > 1   # a 7B verify step, K 3, at ctx 8192
    assert lib.tgis_attn_num_splits_q(1, 2, 4, 4, 1280) > 1     # tests/test_spec_longctx_model_gpu.py: 40-page tables
    assert lib.tgis_attn_num_splits_q(3, 2, 4, 4, 1280) > 1
    assert lib.tgis_attn_num_splits_q(1, 2, 4, 8, 1280) > 1
    assert lib.tgis_attn_num_splits_q(1, 2, 4, 3, 1088) > 1     # a 3-token suffix behind a 1056-token header


def test_host_gate_asks_the_library_only_from_1024_keys_on(monkeypatch):
    from tgis_amd import native

    asked = []
    monkeypatch.setattr(native, "attn_num_splits", lambda *a: asked.append(("old", a)) or 5)
    monkeypatch.setattr(native, "attn_num_splits_q", lambda *a: asked.append(("q", a)) or 7)
    assert native.attn_q_splits(2, 8, 64, 1, 4096) == 5 and asked == [("old", (2, 8, 64, 1, 4096))]
    assert native.attn_q_splits(2, 8, 64, 1, 100) == 5 and len(asked) == 2  # q_len 1: always the old rule's answer
    del asked[:]
    assert native.attn_q_splits(2, 8, 64, 4, 1023) == 1 and asked == []
    assert native.attn_q_splits(2, 8, 64, 4, 1024) == 7 and asked == [("q", (2, 8, 64, 4, 1024))]


def test_workspace_bytes_cover_both_layouts_of_every_decode_form_launch():
    """Callers pass total_q = B * max_q_len.  The two-launch layout needs total_q * H * NS records of D + 2 floats; the
    in-launch merge needs B * q_tiles * Hkv * HC * 16 * NS records of D + 4 floats (one-chunk blocks at q_len > 1)."""
    lib = _library_or_skip()
    for B in (1, 2, 5, 8, 33):
        for Hkv, H in HEADS:
            _, _, TQ, HC = _geom(H, Hkv)
            for q in (2, 3, 4, 8, 17, 64):
                if prefill_form(H, Hkv, q):
                    continue
                for D in (64, 96, 128):
                    for ns in (2, 3, 9, 64):
                        got = lib.tgis_attn_workspace_bytes(B * q, H, Hkv, D, ns)
                        two_pass = B * q * H * ns * (D + 2) * 4
                        fused = B * _cdiv(q, TQ) * Hkv * HC * 16 * ns * (D + 4) * 4
                        assert got >= max(two_pass, fused), (B, Hkv, H, q, D, ns)
    # one q token: the sizes every caller has had
    assert lib.tgis_attn_workspace_bytes(4, 64, 8, 128, 8) == max(4 * 64 * 8 * 130 * 4, 4 * 8 * 16 * 8 * 132 * 4)
    assert lib.tgis_attn_workspace_bytes(4, 48, 1, 128, 8) == max(4 * 48 * 8 * 130 * 4, 4 * 1 * 3 * 16 * 8 * 132 * 4)
