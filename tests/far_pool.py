"""Host helper of tests/test_far_pages_gpu.py: move a small paged-KV case to page ids whose element offsets
`(page * Hkv + hk) * 32 * D` lie on both sides of 2^31 and 2^32, inside ONE device arena that the test owns, so that an offset
computed in 32 bits lands in memory of the test's own that holds a NaN pattern: a wrong address shows as a wrong value.
Importing this file needs no GPU (tests/test_far_pool_cpu.py checks its arithmetic).

The arena is a flat integer tensor.  A pool's base sits BASE = 2^31 elements above the arena's start, so a signed 32-bit wrap
of an element offset (off - 2^32 >= -2^31) or of a byte offset stays inside; unsigned wraps land between the base and the
offset.  K and V share the arena: the V pool's base is VSHIFT page blocks above the K pool's, and the page ids in use come in
clusters narrower than VSHIFT (low pages, and around each threshold), so K page p = block p and V page p = block VSHIFT + p
never meet.  "Block" below always counts page-sized blocks from the K pool's base; block b covers elements [b S, (b + 1) S).
"""
import torch

GIB = 1 << 30
ARENA_BYTES = 35 * GIB // 4  # 8.75 GiB: the cap is 9 GiB of arena live at any time
BASE = 1 << 31               # elements between the arena's start and a pool's base
VSHIFT = 1024                # page blocks between the K pool's base and the V pool's
CLUSTER = 32                 # pages taken on either side of a threshold, and beyond it
BEYOND = 40                  # "a page 40 or more beyond T"
LOW0 = 128                   # the low pages start here: page T / S + k wraps onto page k, |k| < BEYOND + CLUSTER < LOW0
T31, T32 = 1 << 31, 1 << 32
FILL = {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0, torch.uint8: 0x7F}  # the dtype's NaN


def thresholds(esize):
    """The 16-bit pools cross 2^31 elements (2^32 bytes) under the cap, the one-byte pools 2^31 and 2^32."""
    return (T31,) if esize == 2 else (T31, T32)


def fill_word(dtype):
    """The NaN pattern of `dtype` repeated over one int64 (positive for all three patterns)."""
    p, n = FILL[dtype], 8 // (1 if dtype == torch.uint8 else 2)
    w = 0
    for _ in range(n):
        w = (w << (64 // n)) | p
    return w


def _s32(x):
    return ((x + T31) % T32) - T31


def wrapped(off, esize):
    """Where an element offset lands when it, or its byte offset, is cut to 32 bits (unsigned and signed): the element
    offsets that differ from `off`."""
    outs = {off % T32, _s32(off)}
    if esize == 2:
        outs |= {(off * 2 % T32) // 2, _s32(off * 2) // 2}  # (an even byte offset stays even)
    return sorted(outs - {off})


def wrapped_ranges(off, n, esize):
    """The wrapped images of the elements [off, off + n) as (start, length) runs.  A run is cut at every multiple of 2^30
    elements, where any of the wraps may change its shift; inside a piece every wrap is one shift."""
    out, lo = [], off
    while lo < off + n:
        hi = min(off + n, (lo // (1 << 30) + 1) << 30)
        out += [(w, hi - lo) for w in wrapped(lo, esize)]
        lo = hi
    return out


class Geometry:
    """One pool shape.  S = Hkv * 32 * D elements per page."""

    def __init__(self, Hkv, D, esize):
        self.Hkv, self.D, self.esize = Hkv, D, esize
        self.S = Hkv * 32 * D
        self.thresholds = thresholds(esize)

    # ---- page choice --------------------------------------------------------------------------------------------------------
    def last_below(self, T):
        """The last page wholly below T: (p + 1) S <= T."""
        return T // self.S - 1

    def first_at(self, T):
        """The first page with an element at or above T (it straddles T when S does not divide it)."""
        return T // self.S

    def straddle(self, T):
        """(page, kv head, offset inside the head) of the element at T, or None when T is a page edge."""
        if T % self.S == 0:
            return None
        r = T % self.S
        return T // self.S, r // (32 * self.D), r % (32 * self.D)

    def required(self):
        """The pages every relocated case uses first.  In this order the first three already have a page on each side of
        every threshold: the last page below 2^31, the first page at or above the top threshold, then per threshold the other
        side; then a page 40 beyond each threshold, the first page wholly above a straddled one, and two low pages."""
        ts = self.thresholds
        out = [self.last_below(ts[0]), self.first_at(ts[-1])]
        out += [p for T in ts for p in (self.first_at(T), self.last_below(T)) if p not in out]
        out += [self.first_at(T) + BEYOND for T in ts]
        out += [self.first_at(T) + 1 for T in ts if self.straddle(T)]
        return out + [LOW0, LOW0 + 1]

    def far_pages(self):
        """Every far page a case may be given, the required ones first."""
        rest = []
        for k in range(1, CLUSTER):
            for T in self.thresholds:
                rest += [self.last_below(T) - k, self.first_at(T) + BEYOND + k]
                if k + 1 < BEYOND:
                    rest.append(self.first_at(T) + 1 + k)
        req = self.required()
        return req[:-2] + [p for p in dict.fromkeys(rest) if p not in req]

    def order(self, n):
        """n distinct page ids: the required pages, then far pages and low pages in turn while far pages last."""
        far = self.far_pages()
        nreq = len(self.required()) - 2
        out, low = far[:nreq] + [LOW0, LOW0 + 1], LOW0 + 2
        far = far[nreq:]
        while len(out) < n:
            if far and len(out) % 2 == 0:
                out.append(far.pop(0))
            else:
                out.append(low)
                low += 1
        assert low < VSHIFT - BEYOND - CLUSTER, "the low cluster reaches the V pool's wrapped pages"
        return out[:n]

    def top_page(self):
        return max(self.far_pages())

    def spare_page(self):
        """The far page behind unused block-table entries: the highest page of the pool."""
        return self.top_page() + 1

    def pool_pages(self):
        return self.spare_page() + 1

    def arena_elems(self):
        """Elements from the arena's start to the end of the V pool."""
        return BASE + (VSHIFT + self.pool_pages()) * self.S

    def arena_bytes(self):
        return self.arena_elems() * self.esize

    # ---- the alias rule -----------------------------------------------------------------------------------------------------
    def alias_ranges(self, page, vpool):
        """The element ranges (from the K pool's base) that a 32-bit-cut offset into `page` of the K (or V) pool reaches."""
        shift = VSHIFT * self.S if vpool else 0
        return [(lo + shift, n) for lo, n in wrapped_ranges(page * self.S, self.S, self.esize)]

    def check_aliases(self, pages):
        """The alias rule for the K and V pages `pages`: every wrapped range lies inside the arena and meets none of the
        blocks that hold the case's data.  Returns the number of wrapped ranges looked at."""
        real = set(pages) | {p + VSHIFT for p in pages}
        count = 0
        for p in pages:
            for vpool in (False, True):
                for lo, n in self.alias_ranges(p, vpool):
                    count += 1
                    what = f"page {p} ({'v' if vpool else 'k'}): wrapped range [{lo}, {lo + n})"
                    assert -BASE <= lo and lo + n <= self.arena_elems() - BASE, f"{what} leaves the arena"
                    hit = set(range(lo // self.S, (lo + n - 1) // self.S + 1)) & real
                    assert not hit, f"{what} meets blocks {sorted(hit)} of the case's data"
        return count

    def assert_crosses(self, pages):
        """`pages` has a page wholly below and a page with elements at or above every threshold this geometry crosses."""
        for T in self.thresholds:
            assert any((p + 1) * self.S <= T for p in pages), f"no page below 2^{T.bit_length() - 1}"
            assert any((p + 1) * self.S > T for p in pages), f"no page at or above 2^{T.bit_length() - 1}"

    def assert_mixed(self, pages):
        """The whole page choice: next to both sides of every threshold, the pages right at it, one 40 or more beyond it,
        and two low pages."""
        self.assert_crosses(pages)
        for T in self.thresholds:
            assert {self.last_below(T), self.first_at(T)} <= set(pages), f"not the pages right at 2^{T.bit_length() - 1}"
            assert any(0 <= p - self.first_at(T) - BEYOND < CLUSTER for p in pages), f"no page 40 beyond 2^{T.bit_length() - 1}"
        assert sum(p < VSHIFT for p in pages) >= 2, "fewer than two low pages"

    def is_far(self, page):
        return page >= VSHIFT


def page_map(geom, bt, npages, first=(), extra=()):
    """near page id -> far page id for a block table `bt` [B, W] (host) whose row b uses its first npages[b] entries, plus
    the near pages `extra`.  The near pages `first` are served first, then the longest sequence, so the required pages mix
    inside its table; every other id in `bt` (the spare behind unused entries) maps to the far spare."""
    used = [int(p) for p in first]
    for b in sorted(range(bt.shape[0]), key=lambda b: -npages[b]):
        used += [int(bt[b, j]) for j in range(npages[b])]
    used = list(dict.fromkeys(used + [int(p) for p in extra]))
    far = geom.order(len(used))
    m = dict(zip(used, far))
    for p in set(bt.flatten().tolist()) - set(m):
        m[int(p)] = geom.spare_page()
    return m


def remap(t, m, per=1):
    """A tensor of page ids (per = 1) or slots (per = 32) moved through the page map."""
    flat = t.flatten().tolist()
    return torch.tensor([m[x // per] * per + x % per for x in flat], dtype=t.dtype).reshape(t.shape).to(t.device)


class CommitGeometry:
    """tgis_spec_tree_commit's pool [L, 2, P, Hkv, 32 D] as one view from BASE: the last layer's V pool begins at or past
    the top threshold (2^32 elements for one-byte pools, 2^31 for 16-bit ones) from layer 0's K pool."""

    def __init__(self, Hkv, D, esize, L=4):
        self.Hkv, self.D, self.esize, self.L = Hkv, D, esize, L
        self.S = Hkv * 32 * D
        self.T = thresholds(esize)[-1]
        self.P = -(-self.T // ((2 * L - 1) * self.S)) + 2

    def offset(self, layer, kv, page):
        return ((layer * 2 + kv) * self.P + page) * self.S

    def pages(self):
        """Nine pages for the tables of three requests: the pool's last pages, low ones and middle ones in turn."""
        P = self.P
        return [P - 1, 3, P - 2, P // 2, P - 3, 4, P // 2 + 1, P - 4, 5]

    def arena_bytes(self):
        return (BASE + 2 * self.L * self.P * self.S) * self.esize

    def check_aliases(self, pages):
        """Every wrapped range of every (layer, k / v, page) block in use lies inside the arena and meets no block in use."""
        real = sorted(self.offset(l, kv, p) for l in range(self.L) for kv in (0, 1) for p in pages)
        count = 0
        for off in real:
            for lo, n in wrapped_ranges(off, self.S, self.esize):
                count += 1
                assert -BASE <= lo and lo + n <= 2 * self.L * self.P * self.S, f"offset {off}: wrap {lo} leaves the arena"
                for r in real:
                    assert lo + n <= r or r + self.S <= lo, f"offset {off}: wrap {lo} meets the block at {r}"
        return count


class Arena:
    """The device arena of one test module: allocate once, `release()` at teardown."""

    def __init__(self, dev, nbytes=ARENA_BYTES):
        assert nbytes <= 9 * GIB and nbytes % 8 == 0
        self.words = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        self.nbytes = nbytes
        self.word = None

    def release(self):
        self.words = None
        torch.cuda.empty_cache()

    def fill(self, dtype):
        self.word = fill_word(dtype)
        self.dtype = dtype
        self.words.fill_(self.word)

    def typed(self, dtype=None):
        return self.words.view(dtype or self.dtype)

    def pools(self, geom, dtype):
        """NaN-fill the arena; (kpool, vpool) [pool_pages, Hkv, 32 D] views at BASE and VSHIFT blocks above it."""
        assert geom.arena_bytes() <= self.nbytes and geom.esize == torch.empty(0, dtype=dtype).element_size()
        self.fill(dtype)
        self.geom = geom
        flat, n = self.typed(), geom.pool_pages() * geom.S
        k = flat[BASE:BASE + n].view(geom.pool_pages(), geom.Hkv, 32 * geom.D)
        v0 = BASE + VSHIFT * geom.S
        v = flat[v0:v0 + n].view(geom.pool_pages(), geom.Hkv, 32 * geom.D)
        return k, v

    def block(self, off):
        """The page-sized run of elements at element offset `off` from BASE."""
        return self.typed()[BASE + off:BASE + off + self.geom.S]

    def scatter(self, near_k, near_v, m):
        """Copy the near pools' pages to their far ids, one plain slice copy per page."""
        S = self.geom.S
        for p, f in m.items():
            self.block(f * S).copy_(near_k[p].reshape(-1))
            self.block((f + VSHIFT) * S).copy_(near_v[p].reshape(-1))

    def gather(self, offsets):
        """[len(offsets), S] integer view copies of the blocks at the given element offsets."""
        return torch.stack([_bits(self.block(o)) for o in offsets])

    def restore(self, offsets):
        """Put the fill pattern back over the blocks a writer legitimately wrote."""
        pat = torch.tensor(FILL[self.dtype], dtype=torch.int64).to(_bits(self.typed()[:1]).dtype)
        for o in offsets:
            _bits(self.block(o)).fill_(int(pat))

    def untouched(self):
        """Whether every word of the arena holds the fill pattern: min and max over slices of 1 GiB, no temporaries."""
        step = GIB // 8
        mm = [torch.stack(torch.aminmax(self.words[i:i + step])) for i in range(0, self.words.numel(), step)]
        return bool((torch.stack(mm) == self.word).all())


def _bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int16)
