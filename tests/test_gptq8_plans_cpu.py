"""CPU: the launch choice of the 8-bit GPTQ GEMM over a fixed grid of shapes (no GPU; the planner is host code).

Every grid point must keep the planner's invariants, restated here without the header; every instance
gptq8_gemm_kernel<TN, WK, ACT, PERM, MR> the grid reaches, unsplit and split, must have a case in tests/gptq8_cases.py;
every case must land on the plan it names; and the table must hold every launch edge of gptq8_cases.EDGE_RULES."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gptq8_cases as g8  # noqa: E402

ROWS = (1, 16, 17, 31, 32, 33, 63, 64)
GROUP_SIZES = (16, 32, 48, 64, 128)  # and one group


def _projections():
    """(K, N, down) of the qkv / o / gate_up / down projections of the served Llama configs and their TP 2 / 4 / 8 shards,
    plus synthetic edges."""
    models = {  # hidden, intermediate, heads, kv heads, head size
        "tinyllama": (2048, 5632, 32, 4, 64),
        "llama7b": (4096, 11008, 32, 32, 128),
        "llama13b": (5120, 13824, 40, 40, 128),
        "llama70b": (8192, 28672, 64, 8, 128),
    }
    out = set()
    for h, inter, H, Hkv, D in models.values():
        for tp in (1, 2, 4, 8):
            kv = max(Hkv // tp, 1)
            out.add((h, (H // tp + 2 * kv) * D, False))  # qkv
            out.add((H // tp * D, h, False))  # o
            out.add((h, 2 * inter // tp, False))  # gate_up
            out.add((inter // tp, h, True))  # down: also with SiLU * up while staging
    for K in (96, 256, 288, 320, 1056, 1312, 1568):
        for N in (32, 64, 96, 8160, 8192, 8224, 8256, 8288):
            out.add((K, N, True))
    return sorted(out)


def _groups(K):
    return [1] + [K // gs for gs in GROUP_SIZES if K % gs == 0 and K // gs > 1]


def grid():
    """(M, K, N, groups, act, act_order) of every legal call on the grid."""
    pts = []
    for K, N, down in _projections():
        assert K % 32 == 0 and N % 32 == 0, (K, N)
        for groups in _groups(K):
            for ao in (False, True) if groups > 1 else (False,):
                for act in (0, 1) if down else (0,):
                    pts += [(M, K, N, groups, act, ao) for M in ROWS]
    return pts


def _cost(pt):
    return pt[0] * pt[1] * pt[2]


def suggested_case(pt, info):
    """A gptq8_cases entry for a grid point."""
    M, K, N, groups, act, ao = pt
    kw = f", G={groups}" + (', mode="act_order"' if ao else "") + (", act=1" if act else "")
    return f"_C8({M}, {K}, {N}, {tuple(info[:4])}, {info[4]}{kw})"


@pytest.fixture(scope="module")
def lib():
    from tgis_amd import native

    lib = native.load_library()
    lib.tgis_gptq8_gemm_workspace_bytes.restype = lib.tgis_gptq8_prepared_bytes.restype = ctypes.c_int64
    lib.tgis_gptq8_gemm_workspace_bytes.argtypes = lib.tgis_gptq8_prepared_bytes.argtypes = [ctypes.c_int64] * 3
    return lib


@pytest.fixture(scope="module")
def plans(lib):
    out = []
    for pt in grid():
        info = g8.query_plan(lib, *pt)
        assert info is not None, f"tgis_debug_gptq8_plan refused {pt}: {lib.tgis_last_error().decode()}"
        out.append((pt, info))
    return out


def _cdiv(a, b):
    return -(-a // b)


def test_plan_invariants(plans, lib):
    bad = []
    for pt, info in plans:
        M, K, N, groups, act, ao = pt
        TN, WK, KR, S, MR, reduce, perm, kact = info
        tiles = _cdiv(N, 32)
        if (TN, WK) not in g8.INSTANTIATED:
            bad.append(f"{pt}: (TN, WK) = ({TN}, {WK}) has no kernel")
        if (TN == 4) != (tiles >= 256):
            bad.append(f"{pt}: TN = {TN} at {tiles} column tiles")
        if KR <= 0 or KR % 256:
            bad.append(f"{pt}: KR = {KR} is no positive multiple of 256")
        if not ((S - 1) * KR < K <= S * KR):
            bad.append(f"{pt}: empty or short split (S={S}, KR={KR})")
        if MR != (2 if M > 32 else 1):
            bad.append(f"{pt}: MR = {MR}")
        if reduce != int(S > 1) or perm != int(ao) or kact != act:
            bad.append(f"{pt}: reports reduce {reduce}, PERM {perm}, ACT {kact}")
        ws = 4096 + (_cdiv(M, 32) * S * 32 * tiles * 32 * 4 if S > 1 else 0)
        if lib.tgis_gptq8_gemm_workspace_bytes(M, K, N) != ws:
            bad.append(f"{pt}: workspace {lib.tgis_gptq8_gemm_workspace_bytes(M, K, N)} != {ws}")
        prep = _cdiv(tiles * (_cdiv(K, 64) + 1) * 2048 + tiles * groups * 128, 256) * 256
        if lib.tgis_gptq8_prepared_bytes(K, N, groups) != prep:
            bad.append(f"{pt}: prepared image {lib.tgis_gptq8_prepared_bytes(K, N, groups)} != {prep}")
    assert not bad, "\n".join(bad[:40])


def test_the_grid_reaches_every_instance(plans):
    """The served Llama shapes and their shards run all 16 instances, each unsplit and split."""
    reached = {g8.instance_key(info) for _, info in plans}
    want = {(tn, a, p, mr, s) for tn in (2, 4) for a in (0, 1) for p in (0, 1) for mr in (1, 2) for s in (0, 1)}
    assert reached == want, sorted(want - reached)


def test_every_reachable_instance_has_a_case(plans):
    """Every (TN, ACT, PERM, MR) the grid reaches has a case, and so has each of them with S > 1."""
    keys = {}
    for pt, info in plans:
        key = g8.instance_key(info)
        if key not in keys or _cost(pt) < _cost(keys[key][0]):
            keys[key] = (pt, info)
    covered = {g8.instance_key(g8.named_plan(c)) for c in g8.CASES}
    missing = [f"{g8.key_str(k)}\n    add: {suggested_case(*v)}" for k, v in sorted(keys.items()) if k not in covered]
    assert not missing, "instances the planner reaches without a case in gptq8_cases.py:\n" + "\n".join(missing)


def test_cases_land_on_their_plan(lib):
    cases = g8.CASES + g8.SUBNORMAL
    ids = [c["id"] for c in cases]
    assert len(ids) == len(set(ids)), "duplicate case ids"
    wrong = []
    for c in cases:
        got = g8.case_plan(c, lib)
        if got != g8.named_plan(c):
            wrong.append(f"{c['id']}: names {g8.named_plan(c)} but lands on {got}")
    assert not wrong, "re-choose these cases:\n" + "\n".join(wrong)


def test_cases_cover_the_edges():
    lost = [what for what, holds in g8.EDGE_RULES if not any(holds(c) for c in g8.CASES)]
    assert not lost, "gptq8_cases.CASES has lost:\n" + "\n".join(lost)
    rows = {c["M"] for c in g8.CASES}
    for m in (1, 16, 17, 32, 33, 64):
        assert m in rows, f"no case at M = {m}"
    forms = {(c["plan"][0], c["mr"]) for c in g8.SUBNORMAL}
    assert forms == {(2, 1), (2, 2), (4, 1), (4, 2)}, f"subnormal cases run only {sorted(forms)} of (TN, MR)"


def test_every_new_case_is_needed():
    """Each case of INSTANCES is the only one of its (instance, split) or holds an edge alone: dropping it fails above."""
    spare = []
    for c in g8.INSTANCES:
        rest = [o for o in g8.CASES if o is not c]
        key = g8.instance_key(g8.named_plan(c))
        alone = key not in {g8.instance_key(g8.named_plan(o)) for o in rest}
        alone = alone or any(holds(c) and not any(holds(o) for o in rest) for _, holds in g8.EDGE_RULES)
        if not alone:
            spare.append(c["id"])
    assert not spare, f"cases that neither cover an instance nor hold an edge alone: {spare}"


@pytest.mark.parametrize("what,args", [
    ("no rows", (0, 256, 64, 2)),
    ("65 rows", (65, 256, 64, 2)),
    ("K % 32", (8, 272, 64, 1)),
    ("N % 32", (8, 256, 80, 2)),
    ("groups do not divide K", (8, 256, 64, 3)),
    ("group size 8", (8, 256, 64, 32)),
    ("K * gs >= 2^32", (8, 131072, 64, 2)),
])
def test_refusals(lib, what, args):
    lib.tgis_clear_error()
    assert g8.query_plan(lib, *args) is None, f"{what}: accepted"
    assert b"tgis_debug_gptq8_plan" in lib.tgis_last_error(), lib.tgis_last_error()
    lib.tgis_clear_error()
    assert g8.query_plan(lib, 8, 256, 64, 2) is not None  # the same call, legal
