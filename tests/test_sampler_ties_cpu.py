"""CPU: the group-wise fp64 reference of the fused sampler (tests/sampler_sets_ref.py) and the case table it is used on
(tests/sampler_cases.py).

  - pinned to the existing oracle: on tie-free fp32 rows it equals oracle.sampler_ref.warp_row (same -inf pattern, surviving
    values bit-equal), on the inputs of test_sampling_cpu.py and on the reference's golden vectors;
  - the tie-group property: on 16-bit-rounded rows its top-p set differs from warp_row's only inside one group of equal
    values at the boundary (warp_row's stable sort splits that group by index), and the typical-p sets are equal;
  - the preconditions of every case of the table: every decision of the reference has a margin that the kernel's fp32 sums
    cannot cross (bounds and their derivation: sampler_sets_ref's docstring).  A case that misses one fails here and gets
    another seed in sampler_cases.SEEDS;
  - the sampled cases are decisive: at least 80 % of the compared draws have a race margin above 1e-3, and the chi-square
    row keeps exactly 12 elements, two of them tied."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
import sampler_sets_ref as ssr  # noqa: E402
from oracle import sampler_ref  # noqa: E402

F = np.float32


def _same_row(got, want, what):
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), what
    keep = ~np.isneginf(want)
    assert np.array_equal(got[keep].view(np.uint32), want[keep].view(np.uint32)), what


# ---- pinned to warp_row on tie-free rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_equals_warp_row_on_tie_free_rows(seed):
    """The inputs of test_sampling_cpu.test_oracle_warp_row_equals_hf_processors."""
    V = 500
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(1, V, generator=g) * 4)[0].numpy()
    ids = torch.randint(0, V, (1, 30), generator=g)[0].tolist()
    assert np.unique(logits).shape[0] == V
    cases = [dict(temperature=0.7), dict(top_k=12), dict(top_p_cut=float(F(1) - F(0.85))), dict(typical_p=0.6),
             dict(rep_penalty=1.3),
             dict(temperature=1.4, top_k=40, top_p_cut=float(F(1) - F(0.9)), typical_p=0.8, rep_penalty=1.15)]
    for c in cases:
        got, _ = ssr.warp_row_sets(logits, input_ids=ids, **c)
        _same_row(got, sampler_ref.warp_row(logits, input_ids=ids, **c), c)


def test_equals_warp_row_on_reference_golden():
    """tests/golden/chooser_reference.npz, with the arguments test_sampling_cpu.test_oracle_warp_row_equals_reference_golden
    derives from it."""
    from tgis_amd.pb import generate_pb2 as pb
    from tgis_amd.utils.tokens import HeterogeneousNextTokenChooser

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chooser_reference.npz"))
    rows = 0
    for name in sorted({k.split(".")[0] for k in z.files}):
        n = len([k for k in z.files if k.startswith(f"{name}.params.")])
        params = [pb.NextTokenChooserParameters.FromString(z[f"{name}.params.{i}"].tobytes()) for i in range(n)]
        ch = HeterogeneousNextTokenChooser.from_pb(params, 2, 2, [True] * n, torch.float32, "cpu")  # host bookkeeping only
        sampled = any(p.temperature != 0 for p in params)
        ids = z[f"{name}.ids"]
        for step in range(2):
            adj = ch._eos_adjustments()
            for b, p in enumerate(params):
                mode, factor = adj.get(b, (0.0, 0.0))
                kw = dict(
                    temperature=(p.temperature or 1.0) if sampled else 1.0, top_k=p.top_k if sampled else 0,
                    top_p_cut=float(F(1) - F(p.top_p)) if sampled and 0 < p.top_p < 1 else 0.0,
                    typical_p=p.typical_p if sampled and 0 < p.typical_p < 1 else 1.0,
                    rep_penalty=p.repetition_penalty if p.HasField("repetition_penalty") else 1.0, input_ids=ids[b],
                    exclude_id=2 if n != 1 else -1, eos_id=2, eos_mode=int(mode), eos_factor=factor)
                logits = z[f"{name}.{step}.logits"][b]
                got, _ = ssr.warp_row_sets(logits, **kw)
                _same_row(got, sampler_ref.warp_row(logits, **kw), (name, step, b))
                rows += 1
    assert rows > 0


# ---- the tie-group property -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1025, 32000])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_top_p_differs_from_warp_row_only_inside_the_boundary_group(kind, V):
    rnd = sc.bf16_round if kind == "bf16" else sc.f16_round
    split = 0
    for seed in range(20):
        row = rnd(np.random.RandomState(seed).randn(V) * 3)
        for cut in (0.1, 0.7, 0.001):
            cut = float(F(cut))
            got, _, lowest_kept = ssr.top_p_filter(row, cut)
            want = sampler_ref.warp_row(row, top_p_cut=cut)
            diff = np.isneginf(got) != np.isneginf(want)
            if not diff.any():
                continue
            split += 1
            vals = np.unique(row[diff])
            assert vals.shape[0] == 1, f"seed {seed} cut {cut}: the sets differ in {vals.shape[0]} value groups"
            # that group is the one at the boundary: the lowest group the reference keeps or the highest it removes
            below = row[row < lowest_kept]
            assert vals[0] == lowest_kept or (below.size and vals[0] == below.max()), (seed, cut)
            in_group = row == vals[0]
            assert np.isneginf(got[in_group]).all() or not np.isneginf(got[in_group]).any()
        for mass in (0.2, 0.5, 0.95):
            got, _, _, _ = ssr.typical_filter(row, float(F(mass)))
            want = sampler_ref.warp_row(row, typical_p=mass)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"seed {seed} typical_p {mass}"
    if kind == "bf16":
        assert split > 0  # warp_row does split tie groups on such rows: the reason this reference exists


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_table_covers_what_it_states():
    assert {(c["family"], c["V"]) for c in sc.CASES} == {(f, V) for f in sc.FAMILIES for V in sc.VS}
    for c in sc.CASES + [sc.GLOBAL_CASE]:
        assert len(c["rows"]) <= 8
    for name in sc.ROWSET_NAMES:
        if any("rep_penalty" in r for r in sc.rowsets(64)[name]):
            assert {c["L"] for c in sc.CASES if c["rowset"] == name} == set(sc.CONTEXT_L), name
    ks = {r.get("top_k") for r in sc.rowsets(1025)["k_edges"]}
    assert ks == {1, 1024, 1025, 1026}
    for L in (1, 37, 1500):
        ids = sc.build_ids(1025, 5, L, np.random.RandomState(0))[:, :L]
        assert {-1, 1025, 1030, sc.exclude_id_of(1025), sc.eos_id_of(1025)} <= set(ids.reshape(-1).tolist())
    assert np.unique(sc.build_ids(1025, 1, 37, np.random.RandomState(0))[0, :37]).shape[0] < 37  # duplicates


@pytest.mark.parametrize("V", [v for v in sc.VS if v >= 63])
def test_zeros_family_puts_both_zeros_on_the_boundaries(V):
    top_k = top_p = 0
    for c in sc.group("zeros", V):
        d = sc.build(c)
        for b, r in enumerate(c["rows"]):
            row, k = d["logits"][b], r.get("top_k", 0)
            neg0 = (row == 0) & np.signbit(row)
            pos0 = (row == 0) & ~np.signbit(row)
            assert neg0.any() and pos0.any(), (c["id"], b)
            if 0 < k < V:
                # ordered by (value, sign) the k-th largest is +0.0; by value alone the -0.0 entries tie with it
                assert (row > 0).sum() < k <= (row > 0).sum() + pos0.sum(), (c["id"], b)
                top_k += 1
            elif 0.0 < r.get("top_p_cut", 0.0) < 0.74:
                p = np.exp(row.astype(np.float64) / r.get("temperature", 1.0))
                p /= p.sum()
                cut = r["top_p_cut"]
                assert p[row < 0].sum() + p[neg0].sum() < cut < p[row < 0].sum() + p[neg0].sum() + p[pos0].sum()
                top_p += 1
    assert top_k > 0 and top_p > 0


def _check_margins(cid, V, refs):
    g = ssr.gamma(V)
    for b, (_, m) in enumerate(refs):
        for what, margin in (("top-p", m.top_p_mass), ("typical-p", m.typical_mass)):
            assert margin is None or margin > 4 * g, \
                f"{cid} row {b}: {what} mass margin {margin:.3g} <= 4 gamma = {4 * g:.3g}: give the case another seed"
        assert m.typical_gap is None or m.typical_gap > m.typical_gap_bar, \
            f"{cid} row {b}: typical-p dist gap {m.typical_gap:.3g} <= {m.typical_gap_bar:.3g}: give the case another seed"


def test_gamma():
    assert ssr.gamma(32768) == (2 * (32 + 21) + 6) * 2.0 ** -24 and 6.6e-6 < ssr.gamma(32768) < 6.8e-6
    assert ssr.gamma(1) == ssr.gamma(1024) == 50 * 2.0 ** -24 and ssr.gamma(1025) == 52 * 2.0 ** -24


@pytest.mark.parametrize("family,V", sc.GROUPS, ids=[f"{f}-V{V}" for f, V in sc.GROUPS])
def test_case_preconditions(family, V):
    for c in sc.group(family, V):
        _, refs = sc.reference(c)
        _check_margins(c["id"], V, refs)
        for s, _ in refs:
            assert np.isfinite(s).any() and not np.isnan(s).any(), f"{c['id']}: a row without a finite score, or a NaN"
        if family == "const":
            d = sc.build(c)
            for b, r in enumerate(c["rows"]):
                if set(r) <= {"temperature", "top_k", "top_p_cut", "typical_p"}:  # still constant when the filters run
                    assert np.isfinite(refs[b][0]).all(), f"{c['id']} row {b}: a constant row lost elements"
                    assert np.unique(d["logits"][b]).shape[0] == 1


def test_wide_and_verify_case_preconditions():
    _, refs = sc.reference(sc.GLOBAL_CASE)
    _check_margins(sc.GLOBAL_CASE["id"], sc.V_GLOBAL, refs)
    for family, V in sc.VERIFY_CASES:
        c = sc.verify_case(family, V)
        d, refs = sc.verify_reference(c)
        _check_margins(c["id"], V, refs)
        flat = d["drafts"].reshape(-1).tolist()
        assert sc.eos_id_of(V) in flat and any(i >= V for i in flat) and any(i in d["ids"][0, :d["L"]] for i in d["drafts"][0])


# ---- sampled rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", sc.DRAW_V)
def test_draw_seeds_are_decisive(V):
    """At least 80 % of the draws the GPU test compares are no photo finish (race margin > 1e-3)."""
    c = sc.draw_case(V)
    _, refs = sc.reference(c)
    decided = total = 0
    for b, r in enumerate(c["rows"]):
        if not r.get("sample"):
            continue
        for draw in range(2):
            _, margin = sampler_ref.race_choice(refs[b][0], sc.DRAW_SEEDS[b] & 0xFFFFFFFFFFFFFFFF, sc.DRAW_OFFSETS[b] + draw)
            total += 1
            decided += margin > 1e-3
    assert total == 14 and decided >= 0.8 * total, f"{decided} of {total}"
    assert sc.DRAW_OFFSETS[2] == 2 ** 32 - 1


def test_chi_square_row_keeps_twelve_with_a_tie_among_them():
    row = sc.chi2_row()
    s = ssr.top_k_filter(row, sc.CHI2_K)
    kept = s[np.isfinite(s)]
    assert kept.shape[0] == 12 and np.unique(kept).shape[0] < 12
    p = np.exp(kept.astype(np.float64) - kept.max())
    assert sc.CHI2_B * (p / p.sum()).min() >= 5  # every cell of the chi-square test expects at least 5 draws
