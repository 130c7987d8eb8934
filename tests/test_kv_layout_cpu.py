"""CPU: the host-side page packer of the oracle (ops_ref.kv_page_pack) against its inverse and against the slot formulas of
csrc/kv_layout.h, and a restatement of the key-split rule (tgis_attn_num_splits) that pins the split counts the GPU cases of
tests/test_attention_edges_gpu.py are chosen for."""
import os

import pytest
import torch

from oracle import ops_ref


def _k_off(tok, d, D):  # kv_layout.h k_off
    return ((((tok >> 4) * (D >> 3) + (d >> 3)) * 16 + (tok & 15)) << 3) + (d & 7)


def _v_off(tok, d, D):  # kv_layout.h v_off
    i = tok & 15
    cp = (i >> 2) * 8 + (tok >> 4) * 4 + (i & 3)
    return (((cp >> 3) * D + d) << 3) + (cp & 7)


@pytest.mark.parametrize("D", [64, 96, 128])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32])
def test_pack_then_unpack_is_the_identity(D, n):
    g = torch.Generator().manual_seed(D * 100 + n)
    Hkv, pages, page = 3, 4, 2
    kp = torch.randn(pages, Hkv, 32 * D, generator=g).half()
    vp = torch.randn(pages, Hkv, 32 * D, generator=g).half()
    K = torch.randn(n, Hkv, D, generator=g).half()
    V = torch.randn(n, Hkv, D, generator=g).half()
    ops_ref.kv_page_pack(kp, vp, page, K, V)
    K2, V2 = ops_ref.kv_page_unpack(kp, vp, page, Hkv, D)
    assert torch.equal(K2[:n], K) and torch.equal(V2[:n], V)


@pytest.mark.parametrize("D", [64, 96, 128])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 31, 32])
def test_pack_touches_only_its_slots(D, n):
    """Every element the packer writes is the one kv_layout.h's k_off / v_off name for (token, d); nothing else of the pools
    changes (other pages, the page's unwritten tokens)."""
    g = torch.Generator().manual_seed(D + n)
    Hkv, pages, page = 2, 3, 1
    kp = -1.0 - torch.rand(pages, Hkv, 32 * D, generator=g)  # all < 0: the packed values (> 0) differ from every old one
    vp = -1.0 - torch.rand(pages, Hkv, 32 * D, generator=g)
    kp0, vp0 = kp.clone(), vp.clone()
    K = 1.0 + torch.rand(n, Hkv, D, generator=g)
    V = 1.0 + torch.rand(n, Hkv, D, generator=g)
    ops_ref.kv_page_pack(kp, vp, page, K, V)
    kwant, vwant = kp0.clone(), vp0.clone()
    for t in range(n):
        for d in range(D):
            kwant[page, :, _k_off(t, d, D)] = K[t, :, d]
            vwant[page, :, _v_off(t, d, D)] = V[t, :, d]
    assert torch.equal(kp, kwant) and torch.equal(vp, vwant)
    assert int((kp != kp0).sum()) == n * Hkv * D and int((vp != vp0).sum()) == n * Hkv * D


# ---- the key-split rule ------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def num_splits(B, Hkv, H, max_q_len, max_ctx):
    """tgis_attn_num_splits (csrc/attention.hip) restated: key splits of a decode launch."""
    if B <= 0 or Hkv <= 0 or H <= 0 or H % Hkv or max_q_len != 1:
        return 1
    G = H // Hkv
    HC = _cdiv(G, 16)
    TQ = 16 // (1 << (min(G, 16) - 1).bit_length())
    ch = min(HC, 3) if HC > 1 else 1  # chunks_per_block at max_q_len == 1
    base = B * Hkv * _cdiv(HC, ch) * _cdiv(max_q_len, TQ)
    pages = _cdiv(max(max_ctx, 1), 32)
    if ch == 1 and base < 256:  # wide_decode_blocks
        ns = min(_cdiv(256, base), pages // 16)
        if pages >= 32:
            ns = max(ns, min(256 // base, pages // 8, 8))
        if base >= 128:
            ns = 2 if base * 2 <= 256 and pages >= 64 else 1
    elif ch > 1:
        ns = min(_cdiv(256, base), pages // 16)
    else:
        ns = min(_cdiv(512, base), _cdiv(pages, 4))
    return max(1, min(ns, 64))


# (B, Hkv, H, ctx) -> splits that test_attention_edges_gpu.py's more-than-8-splits cases are chosen for.  A failure here means
# the rule changed: re-choose those cases so that they still reach the launch form they name.
EDGE_SPLITS = [
    ((1, 1, 8, 8192), 16),     # GQA 8:1, one kv head: fused in-launch merge over two batches of records
    ((1, 1, 8, 16384), 32),
    ((1, 1, 8, 32768), 64),
    ((1, 8, 64, 8192), 16),    # GQA 8:1 over 8 kv heads
    ((1, 1, 48, 8192), 16),    # MQA 48:1 (three 16-head chunks per block): combine launch, any split count
    ((2, 1, 48, 8192), 16),
    ((1, 1, 48, 16384), 32),
    ((2, 1, 48, 16384), 32),
]


@pytest.mark.parametrize("shape,want", EDGE_SPLITS)
def test_split_rule_gives_the_counts_the_gpu_cases_need(shape, want):
    B, Hkv, H, ctx = shape
    assert num_splits(B, Hkv, H, 1, ctx) == want


def _library_or_skip():
    from tgis_amd import native

    if not os.path.exists(native.LIB_PATH):
        pytest.skip("libtgis_hip.so is not built")
    return native.load_library()


def test_split_rule_restatement_matches_the_library():
    lib = _library_or_skip()
    for (B, Hkv, H, ctx), want in EDGE_SPLITS:
        assert lib.tgis_attn_num_splits(B, Hkv, H, 1, ctx) == want, (B, Hkv, H, ctx)
    for B in (1, 2, 3, 4, 8, 16, 32, 64, 128):
        for Hkv, H in ((1, 8), (8, 64), (32, 32), (4, 32), (1, 48), (1, 12), (2, 128), (1, 80)):
            for ctx in (1, 31, 512, 1000, 1024, 2048, 4096, 8192, 16384, 32768, 100000):
                for q in (1, 2):
                    got = lib.tgis_attn_num_splits(B, Hkv, H, q, ctx)
                    assert got == num_splits(B, Hkv, H, q, ctx), (B, Hkv, H, q, ctx)
