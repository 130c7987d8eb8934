"""CPU: the launch choice of every GEMM entry point, over a fixed grid of shapes (no GPU; the planners are host code).

Every kernel instance the default planners reach on the grid must be covered by a case of tests/gemm_cases.py, and every
case must still land on the instance it names.  Every grid point must also keep the planners' invariants: no empty split,
64-row passes only in two-k-part blocks, instantiated (TN, WK) pairs, unsplit SiLU / rotary epilogues, and workspace and
slab sizes that cover what the chosen plan writes."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

ROWS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 255, 256, 257, 1000, 3072, 3073)


def _projections():
    """(K, N, gate_up) of every projection of the served configs and their TP 2 / 4 / 8 shards, plus synthetic edges."""
    models = {  # hidden, intermediate, heads, kv heads, head size, vocab
        "tinyllama": (2048, 5632, 32, 4, 64, 32000),
        "llama7b": (4096, 11008, 32, 32, 128, 32000),
        "llama70b": (8192, 28672, 64, 8, 128, 32000),
        "starcoder15b": (6144, 24576, 48, 1, 128, 49152),
        "neox20b": (6144, 24576, 64, 64, 96, 50432),
        "pythia1.4b": (2048, 8192, 16, 16, 128, 50304),
        "pythia160m": (768, 3072, 12, 12, 64, 50304),
    }
    out = set()
    for h, inter, H, Hkv, D, vocab in models.values():
        for tp in (1, 2, 4, 8):
            if H % tp:
                continue
            kv = max(Hkv // tp, 1)
            out.add((h, (H // tp + 2 * kv) * D, False))  # qkv
            out.add((H // tp * D, h, False))  # o
            out.add((h, 2 * inter // tp, True))  # gate_up
            out.add((h, inter // tp, False))  # fc (NeoX / BigCode)
            out.add((inter // tp, h, False))  # down / proj
        out.add((h, vocab, False))  # lm_head
    # synthetic edges: K tails (K % 256, K % 64 == 32, K = 8 mod 64), ragged N, narrow and wide N
    for K in (224, 256, 264, 520, 1056, 1088, 4104):
        for N in (32, 64, 72, 100, 2048, 8192, 16384, 16424):
            out.add((K, N, N % 32 == 0))
    return sorted(out)


PROJ = _projections()


def _rope_shapes():
    """(K, N, H, Hkv, D) of the fused qkv projection of every served config with rotary heads and its TP shards, plus
    synthetic heads (K tails, D = 32 / 96, one kv head)."""
    models = {  # hidden, heads, kv heads, head size
        "tinyllama": (2048, 32, 4, 64), "llama7b": (4096, 32, 32, 128), "llama70b": (8192, 64, 8, 128),
        "neox20b": (6144, 64, 64, 96), "pythia1.4b": (2048, 16, 16, 128), "pythia160m": (768, 12, 12, 64),
    }
    out = set()
    for h, H, Hkv, D in models.values():
        for tp in (1, 2, 4, 8):
            if H % tp == 0:
                out.add((h, H // tp, max(Hkv // tp, 1), D))
    out |= {(1032, 32, 8, 128), (264, 64, 8, 96), (1024, 128, 1, 32), (4096, 40, 8, 128)}
    return sorted((K, (H + 2 * Hkv) * D, H, Hkv, D) for K, H, Hkv, D in out)


ROPE = _rope_shapes()
ROPE_HEADS = {(K, N): (H, Hkv, D) for K, N, H, Hkv, D in ROPE}


def _groups(K):
    gs = [1]
    for g in (32, 64, 96, 128):
        if K % g == 0 and K // g > 1:
            gs.append(K // g)
    return gs


def grid():
    """(entry, M, K, N, groups, act, act_order, frag_in, frag_out, dtype) of every legal call on the grid."""
    pts = []
    for K, N, gate_up in PROJ:
        for M in ROWS:
            # dense: K % 8 == 0
            if K % 8 == 0:
                for dt in ("f16", "bf16"):
                    for act in (0, 1, 4, 5) + ((2,) if gate_up else ()):
                        pts.append(("dense", M, K, N, 1, act, False, False, False, dt))
                    if M <= 256:
                        for act in (0, 1):
                            pts.append(("dense_partial", M, K, N, 1, act, False, False, False, dt))
            if K % 32 or N % 32:
                continue
            for groups in _groups(K):
                for ao in (False, True):
                    if ao and groups == 1:
                        continue
                    for act in (0, 1) + ((2,) if gate_up else ()):
                        pts.append(("gptq", M, K, N, groups, act, ao, False, False, "f16"))
                        if act != 2 and M <= 256:
                            pts.append(("gptq_partial", M, K, N, groups, act, ao, False, False, "f16"))
                    if ao or M > 64 or K % 64 or not _wide_groups(K, groups):
                        continue
                    for act in (0,) + ((2,) if gate_up else ()):
                        pts.append(("gptq", M, K, N, groups, act, False, True, False, "f16"))
                        if act == 2 and (N // 2) % 64 == 0:
                            pts.append(("gptq", M, K, N, groups, act, False, True, True, "f16"))
                    pts.append(("gptq_partial", M, K, N, groups, 0, False, True, False, "f16"))
    return pts + rope_grid()


def rope_grid():
    """The fused qkv + rotary + cache-write launches the model makes: M <= 64 rows where tgis_*_rope_ok holds; int4 with a
    row-major and (where the fragment-order kernel serves the shape) a fragment-order activation."""
    lib = _library()
    pts = []
    for K, N, H, Hkv, D in ROPE:
        for M in ROWS:
            if M > 64:
                continue
            if lib.tgis_dense_rope_ok(M, K, N, D):
                for dt in ("f16", "bf16"):
                    pts.append(("dense_rope", M, K, N, 1, 3, False, False, False, dt))
            for groups in _groups(K):
                if lib.tgis_gptq_rope_ok(M, K, N, groups, 0, D):
                    pts.append(("gptq_rope", M, K, N, groups, 3, False, False, False, "f16"))
                    if K % 64 == 0 and _wide_groups(K, groups):
                        pts.append(("gptq_rope", M, K, N, groups, 3, False, True, False, "f16"))
    return pts


def _library():
    from tgis_amd import native

    return native.load_library()


def _cost(pt):
    return pt[1] * pt[2] * pt[3]


def suggested_case(pt):
    """The case the table holds for a variant: its cheapest grid point (M K N), as a gemm_cases.CASES entry."""
    entry, M, K, N, groups, act, ao, fi, fo, dt = pt
    c = {"entry": entry, "M": M, "K": K, "N": N}
    if entry.startswith("gptq"):
        c["groups"] = groups
    if act:
        c["act"] = act
    if ao:
        c["act_order"] = True
    if fi:
        c["frag_in"] = True
    if fo:
        c["frag_out"] = True
    if entry.startswith("dense"):
        c["dtype"] = dt
    if entry.endswith("_rope"):
        c["H"], c["Hkv"], c["D"] = ROPE_HEADS[(K, N)]
    c["bias"] = True
    c["key"] = gc.variant_key(gc.query_plan(_library(), *pt))
    c["id"] = "-".join([entry, c["key"][0], f"M{M}-K{K}-N{N}"] + [f"{k}{v}" for k, v in c.items()
                                                                    if k in ("groups", "act", "act_order", "frag_in",
                                                                             "frag_out", "dtype")])
    return c


def _wide_groups(K, groups):
    gs = K // groups
    return groups == 1 or (gs % 64 == 0 and ((gs // 64) & (gs // 64 - 1)) == 0)


@pytest.fixture(scope="module")
def lib():
    from tgis_amd import native

    return native.load_library()


@pytest.fixture(scope="module")
def reached(lib):
    """variant key -> the cheapest grid point (M K N) reaching it, and the plan of every grid point."""
    keys, plans = {}, []
    for pt in grid():
        info = gc.query_plan(lib, *pt)
        assert info is not None, f"tgis_debug_gemm_plan refused {pt}"
        key = gc.variant_key(info)
        if key not in keys or _cost(pt) < _cost(keys[key]):
            keys[key] = pt
        plans.append((pt, gc.plan_fields(info)))
    return keys, plans


def test_cases_land_on_their_variant(lib):
    assert gc.CASES, "gemm_cases.CASES is empty"
    ids = [c["id"] for c in gc.CASES]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    wrong = []
    for c in gc.CASES:
        got = gc.variant_key(c, lib)
        if got != tuple(c["key"]):
            wrong.append(f"{c['id']}: names {gc.key_str(c['key'])} but lands on {gc.key_str(got)}")
    assert not wrong, "re-choose these cases:\n" + "\n".join(wrong)


def test_every_reachable_variant_has_a_case(reached):
    keys, _ = reached
    covered = {tuple(c["key"]) for c in gc.CASES}
    missing = [f"{gc.key_str(k)}\n    add: {suggested_case(pt)}" for k, pt in sorted(keys.items(), key=str)
               if k not in covered]
    assert not missing, "variants the planners reach without a case in gemm_cases.py:\n" + "\n".join(missing)


def test_cases_cover_the_edges(lib):
    """The shape edges every family must see, whatever variant they land on."""
    by_fam = {}
    for c in gc.CASES:
        by_fam.setdefault(c["key"][0], []).append(c)
    rows = {c["M"] for c in gc.CASES}
    for m in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257):
        assert m in rows, f"no case at M = {m}"
    assert any(33 <= c["M"] % 64 <= 63 and c["M"] > 64 for c in gc.CASES), "no 64-row pass with a partly filled second unit"
    assert any(1 <= c["M"] % 64 <= 31 and c["M"] > 64 for c in gc.CASES), "no 64-row pass with an empty second unit"
    assert any(c["key"][0] == "tall" and c["M"] % 128 for c in gc.CASES), "no tall case with M % 128 != 0"
    dense = by_fam["dense"]
    assert any(c["K"] % 256 and c["K"] % 64 == 8 for c in dense), "no dense case with K = 8 mod 64"
    assert any(c["K"] % 64 == 32 for c in by_fam["stream"]), "no int4 case with K % 64 == 32"
    for tn in {c["key"][1] for c in dense}:
        assert any(c["key"][1] == tn and c["N"] % (32 * tn) and c["N"] % 32 for c in dense), \
            f"dense TN={tn}: no case whose last tile and last column group are partly empty"
    acts = {(c["key"][0], c.get("act", 0)) for c in gc.CASES}
    for a in (0, 1, 2):
        assert ("stream", a) in acts, f"no streaming case with act {a}"
    for a in (0, 1, 2, 4, 5):
        assert ("dense", a) in acts, f"no dense case with act {a}"
    keys = {tuple(c["key"]) for c in gc.CASES}
    for fam in ("gptq_rope", "dense_rope"):
        assert any(k[0] == fam and k[6] == 3 for k in keys), f"no act 3 case of {fam}"
    assert any(k[0] == "wide" and k[6] == 3 for k in keys), "no act 3 case with a fragment-order activation"
    assert any(c["key"][0] == "dense_rope" and c["key"][1] == 1 for c in gc.CASES), "no one-tile dense rope case"
    assert any(c.get("out_f32") for c in dense), "no out_f32 case"
    consumers = {c.get("consumer") for c in gc.CASES}
    assert {"rms", "ln", "ln2"} <= consumers, consumers
    assert by_fam.get("split_silu"), "no split-SiLU case"
    for fam in ("stream", "dense", "tall", "wide"):
        splits = {gc.plan_fields(gc.case_plan(c, lib))["s"] > 1 for c in by_fam[fam] if not c["entry"].endswith("_partial")}
        assert splits == {False, True}, f"{fam}: cases need both S = 1 and S > 1"


def _short_last_split(plan, K):
    return plan["s"] > 1 and plan["s"] * plan["kr"] - K >= 256


def test_some_case_has_a_short_last_split(lib):
    for fam in ("stream", "dense"):
        assert any(_short_last_split(gc.plan_fields(gc.case_plan(c, lib)), c["K"]) for c in gc.CASES
                   if c["key"][0] == fam), f"{fam}: no case with S KR - K >= 256"


INSTANTIATED = {  # (TN, WK) pairs with a kernel
    "stream": {(2, 2), (2, 4), (3, 2), (3, 4), (4, 2), (4, 4)},
    "split_silu": {(2, 2), (2, 4), (3, 2), (3, 4), (4, 2), (4, 4)},
    "dense": {(2, 2), (2, 4), (3, 4), (4, 2), (4, 4)},
    "gptq_rope": {(2, 2), (2, 4), (3, 2), (3, 4), (4, 2), (4, 4)},
    "dense_rope": {(1, 4), (2, 2), (2, 4), (3, 4), (4, 2), (4, 4)},
}


def test_plan_invariants(reached, lib):
    _, plans = reached
    bad = []
    for pt, p in plans:
        entry, M, K, N, groups, act = pt[:6]
        fam = p["family"]
        if fam != "wide" and p["kr"]:
            if not ((p["s"] - 1) * p["kr"] < K <= p["s"] * p["kr"]):
                bad.append(f"{pt}: empty or short split (S={p['s']}, KR={p['kr']})")
        if fam in ("stream", "split_silu", "dense", "gptq_rope", "dense_rope") and p["mr"] == 2 and p["wk"] != 2:
            bad.append(f"{pt}: MR = 2 with WK = {p['wk']}")
        if fam in INSTANTIATED and (p["tn"], p["wk"]) not in INSTANTIATED[fam]:
            bad.append(f"{pt}: (TN, WK) = ({p['tn']}, {p['wk']}) has no kernel")
        if p["act"] in (2, 3) and p["s"] != 1:
            bad.append(f"{pt}: the act {p['act']} epilogue runs split (S={p['s']})")
        if fam == "split_silu" and not (act == 2 and p["s"] > 1 and p["reduce"] == 2):
            bad.append(f"{pt}: split-SiLU without a split")
    assert not bad, "\n".join(bad[:40])


def _slab_bytes(M, N, p):
    """Bytes of fp32 slabs the chosen plan writes: 32-row units x S x 32 rows x NT*32 columns."""
    np_ = -(-N // 32) * 32
    if p["family"] == "tall":
        units = -(-M // 32)
    else:
        units = -(-M // (32 * p["mr"])) * p["mr"]  # a pass writes all of its units
    return units * p["s"] * 32 * np_ * 4


def test_workspace_and_slab_sizes_cover_the_plan(reached, lib):
    _, plans = reached
    lib.tgis_gptq_gemm_workspace_bytes.restype = lib.tgis_dense_gemm_workspace_bytes.restype = __import__("ctypes").c_int64
    lib.tgis_gptq_gemm_partial_bytes.restype = lib.tgis_dense_gemm_partial_bytes.restype = __import__("ctypes").c_int64
    bad = []
    for pt, p in plans:
        entry, M, K, N = pt[:4]
        if entry.endswith("_rope"):
            continue  # unsplit, no workspace (checked above)
        writes = _slab_bytes(M, N, p)
        if entry in ("gptq", "dense"):
            if p["s"] == 1 and p["family"] != "split_silu":
                continue
            have = (lib.tgis_gptq_gemm_workspace_bytes if entry == "gptq" else lib.tgis_dense_gemm_workspace_bytes)(M, K, N)
            if have - 4096 < writes:
                bad.append(f"{pt}: workspace {have} < 4096 + {writes}")
        else:
            fn = lib.tgis_gptq_gemm_partial_bytes if entry == "gptq_partial" else lib.tgis_dense_gemm_partial_bytes
            # native.gptq_gemm_partial sizes its slabs once per row class (M <= 32 | passes of 64 | fragment order <= 32,
            # <= 64): the bytes asked for any M of the class must cover every M of it
            if entry == "gptq_partial":
                cls = [m for m in range(1, 65 if pt[7] else 257) if _row_class(m, pt[7]) == _row_class(M, pt[7])]
                have = min(fn(m, K, N) for m in cls)
            else:
                have = fn(M, K, N)
            if have < writes:
                bad.append(f"{pt}: slab buffer {have} < {writes}")
    assert not bad, "\n".join(bad[:40])


def _row_class(M, frag):
    if frag:
        return ("frag", M > 32)
    return (M + 63) // 64 if M > 32 else 0
