"""The fused sampler's edge cases: tied 16-bit logits, rows of -inf, both zeros, every V at which a lane, the block or the
kernel changes, the context ids the kernel must skip.  Needs no GPU: tests/test_sampler_ties_cpu.py checks, on the CPU,
that the group-wise reference (tests/sampler_sets_ref.py) decides every row of every case with a margin the kernel's fp32
sums cannot cross; tests/test_sampler_edges_gpu.py runs the cases.

A case is (family of logits, V, set of per-row parameters) and a seed; every row of it is built from that seed alone.  A
case whose reference decision is a photo finish gets another seed in SEEDS — it is never skipped.

Logit families (what the rows hold before the chooser touches them; production logits are `scores.float()` of an f16 / bf16
lm_head output, utils/tokens.py):
  bf16        randn * 3 rounded through bf16: a few hundred distinct values at V = 32000, nearly every element tied
  f16         the same through f16
  head        a bf16 row with 5 values far above the rest
  zeros       both zeros in one row.  Rows with a top-k: the k-th largest value is +0.0 and -0.0 ranks below it (float
              comparison keeps it); rows with a top-p only: -0.0 and +0.0 are one group whose halves lie on either side
              of the cut; other rows: both zeros sprinkled over a bf16 row
  neginf      a bf16 row with 30 % of its entries -inf
  few_finite  fewer finite entries than the row's k (3 where it has no k)
  one_finite  a single finite entry
  const       a constant row: one tie group, which top-p and typical-p must keep whole
"""
import zlib

import numpy as np

from test_sampler_gpu import ROWSETS

F = np.float32
FAMILIES = ("bf16", "f16", "head", "zeros", "neginf", "few_finite", "one_finite", "const")
# lane edge (63 / 64 / 65), block edge (1023 / 1024 / 1025), two and three elements per thread, the last V of the register
# kernel and the first of the global-row kernel
VS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 32000, 32768, 32769)
V_GLOBAL = 128256  # a real 128k vocabulary: one case, 2 rows, on the global-row kernel
CONTEXT_L = (0, 1, 37, 1500)  # none, one id, the length the older tests use, longer than the 1024-thread block
LD_LOGITS_PAD, LD_SCORES_PAD, PAD_ROWS, LD_IDS_PAD = 7, 5, 2, 3


def cut_of(top_p):
    """1 - top_p as the host rounds it."""
    return float(F(1) - F(top_p))


def rowsets(V):
    """{name: [per-row parameters]}: ROWSETS of test_sampler_gpu and the edges they leave out."""
    out = {name: [dict(r) for r in rows] for name, rows in ROWSETS.items()}
    out["k_edges"] = [dict(top_k=1), dict(top_k=V - 1), dict(top_k=V), dict(top_k=V + 1)]
    out["p_edges"] = [dict(top_p_cut=float(F(0.001))), dict(top_p_cut=float(F(0.7))),
                      dict(top_p_cut=float(F(0.001)), temperature=5.0), dict(top_p_cut=float(F(0.7)), temperature=0.05)]
    out["typ_edges"] = [dict(typical_p=0.2), dict(typical_p=0.95), dict(typical_p=0.2, temperature=5.0),
                        dict(typical_p=0.95, temperature=0.05)]
    out["temp_edges"] = [dict(temperature=0.05), dict(temperature=5.0),
                         dict(temperature=5.0, top_k=40, top_p_cut=cut_of(0.7), rep_penalty=1.5),
                         dict(temperature=0.05, typical_p=0.5, eos=(2.0, 0.5))]
    # the EOS id inside the penalised context: the penalty lands on top of the EOS adjustment
    out["eos_ctx"] = [dict(eos=(1.0, 0.0), rep_penalty=1.5), dict(eos=(2.0, 0.5), rep_penalty=1.5),
                      dict(eos=(2.0, 3.0), rep_penalty=0.8, top_k=5), dict(eos=(1.0, 0.0), rep_penalty=1.2, typical_p=0.5)]
    if V == 1:  # EOS mode 1 would leave the only element -inf: a row of NaNs, which is not this table's subject
        for rows in out.values():
            for r in rows:
                if r.get("eos", (0.0, 0.0))[0] == 1.0:
                    r["eos"] = (2.0, 0.5)
    return out


ROWSET_NAMES = tuple(sorted(rowsets(64)))

# cases whose default seed (crc32 of the id) is a photo finish of the reference (tests/test_sampler_ties_cpu.py names them)
SEEDS = {
    "bf16-V32000-top_p": 911857132,
    "bf16-V32768-typ_edges": 498662733,
    "bf16-V32769-typ_edges": 3694535309,
    "f16-V32000-typ_edges": 4228483300,
    "f16-V32000-typical": 2391580275,
    "f16-V32768-typ_edges": 3565472289,
    "f16-V32769-p_edges": 2545364952,
    "f16-V32769-typ_edges": 352982498,
    "head-V1023-typ_edges": 3869204729,
    "f16-V32000-verify": 298943690,
}


def _case(family, V, name, index, rows=None):
    cid = f"{family}-V{V}-{name}"
    rows = rowsets(V)[name] if rows is None else rows
    return dict(id=cid, family=family, V=V, rowset=name, rows=rows, L=CONTEXT_L[index % 4],
                seed=SEEDS.get(cid, zlib.crc32(cid.encode())))


def _cases():
    out = []
    for family in FAMILIES:
        for V in VS:
            for name in ROWSET_NAMES:
                out.append(_case(family, V, name, len(out) + len(out) // 4))  # (every row set meets every L)
    return out


CASES = _cases()
GLOBAL_CASE = _case("bf16", V_GLOBAL, "wide", 2, rows=[
    dict(temperature=0.8, top_k=50, top_p_cut=cut_of(0.9), rep_penalty=1.2),
    dict(temperature=1.3, top_p_cut=float(F(0.001)), typical_p=0.9, rep_penalty=1.05, eos=(2.0, 0.25))])
GROUPS = sorted({(c["family"], c["V"]) for c in CASES}, key=lambda g: (FAMILIES.index(g[0]), g[1]))


def group(family, V):
    return [c for c in CASES if c["family"] == family and c["V"] == V]


# ---- building a case ----------------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> nearest bf16 (ties to even) -> float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def f16_round(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def eos_id_of(V):
    return 7 % V


def exclude_id_of(V):
    return 3 % V


def _not_eos(rs, V, n):
    """n distinct positions, none of them the EOS id where V allows it."""
    pool = np.array([i for i in range(min(V, 4096)) if i != eos_id_of(V)] or [0])
    if V > 4096:
        pool = np.concatenate([pool, rs.randint(4096, V, size=8)])
    return rs.permutation(np.unique(pool))[:n]


def _zeros_row(rs, V, r):
    k, cut = r.get("top_k", 0), r.get("top_p_cut", 0.0)
    T = F(r.get("temperature", 1.0))
    if 0 < k < V and V >= 4:
        # k - 2 positives, three +0.0 (ranks k - 1 .. k + 1: the k-th largest is +0.0), four -0.0, negatives below
        row = -np.abs(bf16_round(rs.randn(V) * 3)) - F(0.5)
        perm = rs.permutation(V)
        n_pos = max(k - 2, 0)
        row[perm[:n_pos]] = np.abs(bf16_round(rs.randn(n_pos) * 3)) + F(0.5)
        n_pz = min(3, V - n_pos - 1)
        row[perm[n_pos:n_pos + n_pz]] = F(0.0)
        row[perm[n_pos + n_pz:n_pos + n_pz + 4]] = F(-0.0)
        return row.astype(np.float32)
    if 0.0 < cut < 0.74 and V >= 3:
        # one value on top, the rest -0.0 and +0.0 alternating with a mass of 4/3 cut: the -0.0 half alone is below the cut
        row = np.where(np.arange(V) % 2 == 0, F(-0.0), F(0.0)).astype(np.float32)
        top = int(rs.randint(0, V))
        w = 4.0 * cut / 3.0
        row[top] = F(np.log((V - 1) * (1.0 - w) / w)) * T
        return row
    row = bf16_round(rs.randn(V) * 3)
    z = rs.rand(V)
    row[z < 0.15] = F(0.0)
    row[z > 0.85] = F(-0.0)
    return row


def build_row(family, V, r, rs):
    if family == "bf16":
        return bf16_round(rs.randn(V) * 3)
    if family == "f16":
        return f16_round(rs.randn(V) * 3)
    if family == "head":
        row = bf16_round(rs.randn(V) * 3)
        at = rs.permutation(V)[:5]
        row[at] = np.array([14.0, 14.5, 15.0, 15.5, 16.0], dtype=np.float32)[:at.shape[0]]
        return row
    if family == "zeros":
        return _zeros_row(rs, V, r)
    if family == "const":
        return np.full(V, bf16_round(np.array([rs.randn() * 3]))[0], dtype=np.float32)
    # Rows of -inf and the EOS adjustment: the length penalty (mode 2) of a -inf score is -inf + inf, a NaN, and the mask
    # (mode 1) of the only finite score leaves a row of NaNs; NaN rows are not this table's subject.  So the EOS score is
    # finite in a row whose EOS mode is 2, and everywhere else a finite score sits off the EOS id.
    row = bf16_round(rs.randn(V) * 3)
    eos_finite = r.get("eos", (0.0, 0.0))[0] == 2.0
    if family == "neginf":
        gone = rs.permutation(V)[:min(-(-3 * V // 10), V - 1)]
        gone = gone[gone != _not_eos(rs, V, 1)[0]]
        if eos_finite:
            gone = gone[gone != eos_id_of(V)]
        row[gone] = -np.inf
        return row
    k = r.get("top_k", 0)
    n = 1 if family == "one_finite" else max(1, min(k - 1 if k > 0 else 3, V - 1, 7))
    keep = _not_eos(rs, V, n)
    if eos_finite:
        keep[0] = eos_id_of(V)
    out = np.full(V, -np.inf, dtype=np.float32)
    out[keep] = row[keep]
    return out


def build_ids(V, B, L, rs):
    """[B, L + LD_IDS_PAD] context ids; the columns past L hold valid ids that must not be read."""
    ids = rs.randint(0, V, size=(B, L + LD_IDS_PAD)).astype(np.int64)
    special = [-1, V, V + 5, exclude_id_of(V), eos_id_of(V)]
    if L == 1:
        for b in range(B):
            ids[b, 0] = special[(b + 4) % 5]  # rows 0, 1, ...: the EOS id, -1, V, ...
    elif L >= 8:
        ids[:, :5] = special
        ids[:, 5] = ids[:, 6]  # a duplicate
        ids[:, L - 5:L] = exclude_id_of(V)  # padding-like repeats of the excluded id
    return ids


def build(case):
    """dict(logits [B, V] f32, ids [B, L + pad] i64, L, rows, eos_id, exclude_id, use_ids)."""
    V, rows = case["V"], case["rows"]
    B = len(rows)
    logits = np.stack([build_row(case["family"], V, r, np.random.RandomState((case["seed"] + 7919 * b) % 2 ** 32))
                       for b, r in enumerate(rows)])
    ids = build_ids(V, B, case["L"], np.random.RandomState((case["seed"] ^ 0x5bd1e995) % 2 ** 32))
    return dict(logits=logits, ids=ids, L=case["L"], rows=rows, eos_id=eos_id_of(V), exclude_id=exclude_id_of(V),
                use_ids=any("rep_penalty" in r for r in rows))


def ref_kwargs(d, b, req=None, extra_ids=()):
    """Keyword arguments of sampler_sets_ref.warp_row_sets / oracle.sampler_ref.warp_row for row b of a built case; a
    verify row takes the context of its request `req`, extended by the drafts in front of it."""
    r = d["rows"][b]
    mode, factor = r.get("eos", (0.0, 0.0))
    ids = None
    if d["use_ids"]:
        ids = [int(i) for i in d["ids"][b if req is None else req, :d["L"]]] + [int(i) for i in extra_ids]
    return dict(temperature=r.get("temperature", 1.0), top_k=r.get("top_k", 0), top_p_cut=r.get("top_p_cut", 0.0),
                typical_p=r.get("typical_p", 1.0), rep_penalty=r.get("rep_penalty", 1.0), input_ids=ids,
                exclude_id=d["exclude_id"], eos_id=d["eos_id"], eos_mode=int(mode), eos_factor=factor)


def reference(case):
    """[(warped scores, Margins)] per row, from the group-wise fp64 reference."""
    import sampler_sets_ref as ssr

    d = build(case)
    return d, [ssr.warp_row_sets(d["logits"][b], **ref_kwargs(d, b)) for b in range(len(d["rows"]))]


# ---- sampled rows ---------------------------------------------------------------------------------------------------------
# exact draws: V with more than one element per thread, two draws per stream; stream 2 starts at offset 2^32 - 1, so its
# second draw runs with a non-zero high counter word
DRAW_V = (1025, 2049)
DRAW_B = 8
DRAW_OFFSETS = [9, 0, 2 ** 32 - 1, 5, 123456789, 1, 2 ** 40 + 3, 77]
DRAW_SEEDS = [(1 << 40) * (b + 1) + 17 for b in range(DRAW_B)]
DRAW_SEEDS[5] = -3  # above 2^63 in two's complement


def draw_case(V):
    rows = [dict(temperature=0.8, top_k=(0 if b % 2 else 64), sample=1) for b in range(DRAW_B)]
    rows[3] = dict(temperature=1.0)  # a greedy row in the middle: no draw, stream untouched
    rows[6] = dict(temperature=1.1, top_p_cut=cut_of(0.9), typical_p=0.9, sample=1)
    c = _case("bf16" if V == 1025 else "f16", V, "draws", 0, rows=rows)
    return c


# distribution: 4096 streams over one tied bf16 row, top_k = 12; the seed is one at which exactly 12 elements survive (ties
# with the 12th would add more) and two of the 12 are tied with each other
CHI2_V, CHI2_B, CHI2_K, CHI2_SEED = 1500, 4096, 12, 0


def chi2_row():
    return bf16_round(np.random.RandomState(CHI2_SEED).randn(CHI2_V) * 3)


# verify form: K = 3 drafts per request, 2 requests, on the tied families
VERIFY_K = 3
VERIFY_CASES = [(family, V) for family in ("bf16", "f16", "head", "zeros", "const") for V in (1025, 32000)]


def verify_case(family, V):
    rows = [dict(temperature=0.8, top_k=50, top_p_cut=cut_of(0.9), rep_penalty=1.2, eos=(2.0, 0.5)),
            dict(temperature=1.3, top_p_cut=cut_of(0.7), typical_p=0.9, rep_penalty=1.5, eos=(1.0, 0.0), sample=1)]
    c = _case(family, V, "verify", 2, rows=rows)  # L = 37
    return c


def build_verify(case):
    """The verify problem of a 2-request case: logits [2 (K + 1), V], drafts [2, K], and per verify row the parameters of
    its request."""
    V, K1 = case["V"], VERIFY_K + 1
    rs = np.random.RandomState(case["seed"])
    expanded = dict(case, rows=[case["rows"][b] for b in range(2) for _ in range(K1)])
    d = build(expanded)
    ids = build_ids(V, 2, case["L"], np.random.RandomState((case["seed"] ^ 0x5bd1e995) % 2 ** 32))
    free = int(rs.randint(8, V))
    # a duplicate of a context id, the EOS id, an id of its own / an out-of-range id, an id of its own, the EOS id
    drafts = np.array([[ids[0, 8], eos_id_of(V), free], [V + 2, free, eos_id_of(V)]], dtype=np.int64)
    d.update(ids=ids, drafts=drafts, req_rows=case["rows"])
    return d


def verify_reference(case):
    """(built verify problem, [(warped scores, Margins)] per verify row): row (b, j) is the plain step of request b on its
    own logits with the context extended by drafts[b][:j]."""
    import sampler_sets_ref as ssr

    d = build_verify(case)
    K1 = VERIFY_K + 1
    return d, [ssr.warp_row_sets(d["logits"][r], **ref_kwargs(d, r, req=r // K1, extra_ids=d["drafts"][r // K1][:r % K1]))
               for r in range(2 * K1)]
