"""Which pages each wave of a windowed attention launch walks, and in which form, restated in plain arithmetic from the kernels
(csrc/attention.hip attn_paged_kernel<.., WINDOW> at one q token per sequence, csrc/attention_prefill.hip
attn_prefill_kernel<.., WINDOW> at more).  TEST INFRASTRUCTURE; imports nothing of the code under test.

It exists to CHOOSE and to GUARD test cases: tests/test_attn_window_wide_cpu.py asserts from it that the cases of
tests/test_attn_window_wide_gpu.py reach the loops they are there for (a wave that walks several pages, the `low` page with
mask-free pages behind it, splits of more than four pages, splits without a page, mask-free pages under a lower bound).  It is
not an oracle for values: those come from tests/attn_window_ref.py."""
from collections import namedtuple

PAGE = 32
NW = 4  # waves per block of the windowed decode form (attention_plan.h plan_attn: the restricted plan)


def first_key(ctx, q_len, t, W):
    """attention_plan.h attn_window_first_key."""
    p = ctx - q_len + t + 1
    return p - W if p > W else 0


# ---- decode form --------------------------------------------------------------------------------------------------------------
# masked / full: per wave the pages of the masked loop (in the order it takes them) and of the mask-free loop behind it
DecodeSplit = namedtuple("DecodeSplit", "pbeg pend masked full low")
DecodeWalk = namedtuple("DecodeWalk", "klo pfirst pages pps splits")


def decode_walk(ctx, W, ns=1):
    """One sequence of one q token under a window of W keys, its visible pages divided over ns key splits."""
    assert ctx >= 1 and W >= 1 and ns >= 1
    klo = first_key(ctx, 1, 0, W)
    pages = (ctx + PAGE - 1) // PAGE
    pfirst = klo // PAGE
    pps = (pages - pfirst + ns - 1) // ns
    kfull = ctx            # keys below it are visible to the q row; pages [.., nfullp) lie wholly below it
    nfullp = kfull // PAGE
    splits = []
    for s in range(ns):
        pbeg = pfirst + s * pps
        pend = min(pages, pbeg + pps)
        masked, full, lows = [], [], []
        for w in range(NW):
            p = pbeg + w
            pp_top = p + (max(nfullp - p, 0) + NW - 1) // NW * NW
            low = p == pfirst and klo % PAGE != 0 and p < min(pend, nfullp)
            pp = p if low else pp_top
            m = []
            while pp < pend:
                m.append(pp)
                pp = pp_top if pp < pp_top else pp + NW
            if low:
                p += NW
            f = []
            while p < pend and p * PAGE + PAGE <= kfull:
                f.append(p)
                p += NW
            masked.append(m)
            full.append(f)
            lows.append(low)
        splits.append(DecodeSplit(pbeg, pend, masked, full, lows))
    return DecodeWalk(klo, pfirst, pages, pps, splits)


def wave_pages(split, w):
    return split.masked[w] + split.full[w]


def low_exists(walk):
    """The page the window starts inside takes the masked body in front of the mask-free loop (wave 0 of split 0)."""
    return any(any(s.low) for s in walk.splits)


def full_after_low(walk):
    """How many mask-free pages wave 0 of split 0 walks behind the `low` page (0 without one)."""
    s = walk.splits[0]
    return len(s.full[0]) if s.low[0] else 0


def empty_splits(walk):
    return [i for i, s in enumerate(walk.splits) if s.pbeg >= s.pend]


def max_pages_per_wave(walk):
    return max(len(wave_pages(s, w)) for s in walk.splits for w in range(NW))


def visited(walk):
    """Every page some wave of some split visits, with repeats."""
    return sorted(p for s in walk.splits for w in range(NW) for p in wave_pages(s, w))


# ---- prefill form -------------------------------------------------------------------------------------------------------------
SKIP_LO, SKIP_HI, MASKED, FREE = "skip-lo", "skip-hi", "masked", "free"
PrefillWave = namedtuple("PrefillWave", "rows kmin kmax lo_any lo_full forms")  # rows: the q rows of the wave's valid columns
PrefillBlock = namedtuple("PrefillBlock", "t0 p0 pages waves")


def geom(H, Hkv):
    """(Gp, TQ) of attention_plan.h geom: a 16-column tile holds TQ q tokens x Gp columns of the (padded) group chunk."""
    Gc = min(H // Hkv, 16)
    Gp = 1 << (Gc - 1).bit_length()
    return Gp, 16 // Gp


def prefill_walk(q_len, ctx, W, Gp, TQ):
    """[PrefillBlock] of one sequence.  A block has TQ * 8 q tokens; wave w's 32 columns are TQ * 2 of them from t0 + w * TQ * 2
    on.  forms: {page: skip-lo | skip-hi | masked | free} over the block's page loop [p0, pages).  (The group's padding columns
    and the chunk's heads past G are invalid at EVERY q row alike, so the wave's bounds depend on its rows alone.)"""
    assert 1 <= q_len <= ctx and W >= 1 and Gp * TQ == 16
    TQB = TQ * 8
    blocks = []
    for t0 in range(0, q_len, TQB):
        kend = ctx - q_len + min(q_len, t0 + TQB)
        pages = (kend + PAGE - 1) // PAGE
        p0 = first_key(ctx, q_len, t0, W) // PAGE
        waves = []
        for w in range(4):
            rows = [t for t in range(t0 + w * 2 * TQ, t0 + (w + 1) * 2 * TQ) if t < q_len]
            kmaxs = [ctx - q_len + t + 1 for t in rows]
            kmax = max(kmaxs, default=0)
            kmin = min(kmaxs, default=0x7FFFFFFF)
            lo_full = max(kmax - W, 0)
            lo_any = 0 if not rows else max(kmin - W, 0)
            forms = {}
            for p in range(p0, pages):
                if not p * PAGE < kmax:
                    forms[p] = SKIP_HI
                elif not p * PAGE + PAGE > lo_any:
                    forms[p] = SKIP_LO
                elif (p + 1) * PAGE <= kmin and p * PAGE >= lo_full:
                    forms[p] = FREE
                else:
                    forms[p] = MASKED
            waves.append(PrefillWave(rows, kmin, kmax, lo_any, lo_full, forms))
        blocks.append(PrefillBlock(t0, p0, pages, waves))
    return blocks


def prefill_counts(blocks):
    """{form: how many (wave, page) pairs take it}, waves without a valid column left out."""
    n = {SKIP_LO: 0, SKIP_HI: 0, MASKED: 0, FREE: 0}
    for blk in blocks:
        for wv in blk.waves:
            if wv.rows:
                for f in wv.forms.values():
                    n[f] += 1
    return n
