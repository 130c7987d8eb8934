"""The arithmetic of tests/far_pool.py, without a GPU: which pages sit on which side of 2^31 and 2^32 elements for the three
pool geometries of tests/test_far_pages_gpu.py and both element sizes, that a 32-bit-cut offset into any page the GPU file can
use lands inside the arena and on none of the case's data, and that every arena fits under the 9 GiB cap."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_pool as fp  # noqa: E402

GEOMS = [(8, 128), (8, 96), (1, 128)]
# more pages than any case of the GPU file maps (its q-split cases: three sequences of up to 35 pages, a spare, a NaN page),
# and enough to hand out every far page of the one-byte geometries
MOST_PAGES = 420


@pytest.mark.parametrize("esize", [1, 2], ids=["e4m3", "16bit"])
@pytest.mark.parametrize("Hkv,D", GEOMS, ids=[f"hkv{h}-d{d}" for h, d in GEOMS])
def test_threshold_pages(Hkv, D, esize):
    g = fp.Geometry(Hkv, D, esize)
    assert g.S == Hkv * 32 * D
    assert g.thresholds == ((1 << 31, 1 << 32) if esize == 1 else (1 << 31,))
    for T in g.thresholds:
        lb, fa = g.last_below(T), g.first_at(T)
        assert (lb + 1) * g.S <= T < (lb + 2) * g.S, "the last page wholly below T"
        assert fa * g.S <= T < (fa + 1) * g.S and fa == lb + 1, "the first page with an element at or above T"
        assert {lb, fa, fa + fp.BEYOND} <= set(g.required())
    assert sum(p < fp.VSHIFT for p in g.required()) == 2


def test_the_thresholds_are_where_the_issue_says():
    assert [fp.Geometry(8, 128, 1).first_at(T) for T in (1 << 31, 1 << 32)] == [65536, 131072]
    assert [fp.Geometry(1, 128, 1).first_at(T) for T in (1 << 31, 1 << 32)] == [524288, 1048576]
    g = fp.Geometry(8, 96, 1)
    assert g.S == 24576
    assert g.straddle(1 << 31) == (87381, 2, 2048) and g.straddle(1 << 32) == (174762, 5, 1024)
    assert fp.Geometry(8, 96, 2).straddle(1 << 31) == (87381, 2, 2048)
    assert fp.Geometry(8, 128, 2).straddle(1 << 31) is None
    # the straddle pages and the first page wholly above are among the pages every D 96 case uses
    assert {87380, 87381, 87382, 174761, 174762, 174763} <= set(g.required())


def test_wraps():
    assert fp.wrapped(5, 1) == [] and fp.wrapped(5, 2) == []
    assert fp.wrapped((1 << 31) + 5, 1) == [5 - (1 << 31)]                      # signed elements
    assert fp.wrapped((1 << 32) + 5, 1) == [5]                                  # unsigned and signed elements
    assert fp.wrapped((1 << 31) + 5, 2) == [5 - (1 << 31), 5]                   # signed elements; bytes mod 2^32
    assert fp.wrapped((1 << 30) + 5, 2) == [5 - (1 << 30)]                      # signed bytes
    assert fp.wrapped_ranges((1 << 31) - 3, 8, 1) == [(-(1 << 31), 5)]          # only the part past 2^31 wraps
    assert fp.fill_word(torch.float16) == 0x7E007E007E007E00 and fp.fill_word(torch.uint8) == 0x7F7F7F7F7F7F7F7F
    assert fp.fill_word(torch.bfloat16) == 0x7FC07FC07FC07FC0


@pytest.mark.parametrize("esize", [1, 2], ids=["e4m3", "16bit"])
@pytest.mark.parametrize("Hkv,D", GEOMS, ids=[f"hkv{h}-d{d}" for h, d in GEOMS])
def test_alias_rule_and_arena_size(Hkv, D, esize):
    g = fp.Geometry(Hkv, D, esize)
    pages = g.order(MOST_PAGES) + [g.spare_page()]
    assert len(set(pages)) == len(pages)
    assert set(g.far_pages()) <= set(pages), "every far page the GPU file can be given is checked"
    wrapping = [p for p in g.far_pages() if (p + 1) * g.S * esize > 1 << 31]  # a byte offset past 2^31 wraps one way at least
    assert len(wrapping) > len(g.far_pages()) // 2
    assert g.check_aliases(pages) >= 2 * len(wrapping), "the K and the V image of every such page were looked at"
    g.assert_mixed(pages)
    g.assert_mixed(g.order(len(g.required())))
    g.assert_crosses(g.order(3))  # three pages already have one on each side of every threshold
    assert g.arena_bytes() <= fp.ARENA_BYTES <= 9 * fp.GIB
    assert max(pages) < g.pool_pages()
    # every wrap of every pool element stays above the arena's start
    assert fp.BASE >= 1 << 31


def test_the_rule_notices_a_clash():
    g = fp.Geometry(8, 128, 1)
    assert g.check_aliases([65536 + 7, 7]) == 2  # one byte: 2^31 + 7 S only sign-wraps, to below the base
    with pytest.raises(AssertionError, match="meets blocks"):
        g.check_aliases([131072 + 7, 7])         # 2^32 + 7 S cut to 32 bits is page 7
    g2 = fp.Geometry(8, 128, 2)
    with pytest.raises(AssertionError, match="meets blocks"):
        g2.check_aliases([65536 + 7, 7])         # 16-bit: the byte offset 2^32 + 14 S cut to 32 bits is page 7
    with pytest.raises(AssertionError, match="no page at or above"):
        g.assert_crosses([65535, 128, 129])


def test_page_map_serves_the_longest_sequence_first_and_sends_the_spare_far():
    g = fp.Geometry(8, 128, 2)
    bt = torch.tensor([[4, 9, 9, 9], [0, 1, 2, 3], [5, 6, 9, 9]], dtype=torch.int32)
    m = fp.page_map(g, bt, [1, 4, 2], extra=[7])
    assert [m[p] for p in (0, 1, 2, 3)] == g.required()[:4]
    assert m[9] == g.spare_page() and m[7] in g.order(8)
    far = fp.remap(bt, m)
    assert far[1].tolist() == g.required()[:4] and far[0, 1:].tolist() == [g.spare_page()] * 3
    slots = torch.tensor([33, 2 * 32 + 31], dtype=torch.int32)
    assert fp.remap(slots, m, per=32).tolist() == [m[1] * 32 + 1, m[2] * 32 + 31]
    assert m[1] * 32 + 31 < 1 << 31


@pytest.mark.parametrize("esize", [1, 2], ids=["e4m3", "16bit"])
def test_commit_geometry(esize):
    c = fp.CommitGeometry(2, 64, esize)
    top = (1 << 32) if esize == 1 else (1 << 31)
    assert c.offset(c.L - 1, 1, 0) >= top > c.offset(c.L - 1, 0, 0), "only the last layer's V pool begins past the threshold"
    assert c.arena_bytes() <= fp.ARENA_BYTES
    assert c.check_aliases(c.pages()) > 0 and max(c.pages()) == c.P - 1 and len(set(c.pages())) == 9
