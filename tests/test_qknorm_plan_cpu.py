"""CPU: the launch form of the q/k RMSNorm + rope + cache-write entry points, no GPU needed: the choosers are host code,
reported by tgis_debug_qknorm_plan, and the argument checks run before any launch.

Each case of tests/qknorm_cases.py must land on the form it states.  The launch rule is restated here in Python and checked
against the library over a grid, and every form the rule reaches on that grid must have a case: a threshold change fails here
first and names the cases to re-choose."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qknorm_cases as qc  # noqa: E402

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from tgis_amd import native

    return native.load_library()


def _cdiv(a, b):
    return -(-a // b)


# ---- the rules, restated --------------------------------------------------------------------------------------------------
def token_rule(T, H, Hkv, D):
    heads = H + 2 * Hkv
    gy = min(16, _cdiv(heads, 16)) if T <= 64 else 1
    return [gy, int(gy * 16 < heads), heads, 16 - D // 8]


def page_rule(max_len, D):
    return [_cdiv(max_len, 32), 2, _cdiv(32 * (D // 8), 256), 0]


# (H, Hkv) of Qwen3 0.6B .. 32B and their TP shards, q only, and the cases' own
GRID_HEADS = sorted({(H // tp, Hkv // tp) for H, Hkv in ((16, 8), (32, 8), (40, 8), (64, 8), (32, 0), (64, 0)) for tp in (1, 2, 4, 8)
                     if H % tp == 0 and Hkv % tp == 0} | {(c["H"], c["Hkv"]) for c in qc.TOKEN_CASES} | {(1, 0), (15, 0), (16, 0),
                                                                                                             (17, 0), (256, 0),
                                                                                                             (257, 0)})
GRID_T = (0, 1, 2, 32, 63, 64, 65, 128, 300, 4096)
GRID_D = (64, 96, 128)


def test_cases_land_on_their_forms(lib):
    bad = [f"{c['id']}: states {tuple(c['form'])}, lands on {qc.case_form(c, lib)}" for c in qc.TOKEN_CASES + qc.PAGE_CASES
           if qc.case_form(c, lib) != tuple(c["form"])]
    assert not bad, "re-choose these cases:\n" + "\n".join(bad)


def test_rules_restated(lib):
    for (H, Hkv), T, D in itertools.product(GRID_HEADS, GRID_T, GRID_D):
        assert qc.query(lib, 0, T, H, Hkv, D) == token_rule(T, H, Hkv, D), (T, H, Hkv, D)
    for max_len, D in itertools.product((0, 1, 31, 32, 33, 64, 65, 700, 4096, 32768), GRID_D):
        assert qc.query(lib, 1, max_len, D) == page_rule(max_len, D), (max_len, D)


def test_every_reachable_form_has_a_case(lib):
    reached = {qc.token_form(qc.query(lib, 0, T, H, Hkv, D)) for (H, Hkv), T, D in itertools.product(GRID_HEADS, GRID_T, GRID_D)}
    assert reached == {(k, i) for k in ("single", "looped", "spread", "strided") for i in (0, 4, 8)}
    covered = {tuple(c["form"]) for c in qc.TOKEN_CASES}
    assert reached <= covered, f"forms without a case: {sorted(reached - covered)}"
    # page-wise: the k store passes are a function of D alone; the pages per sequence of max_len alone, covered at 1, 2, 3 and
    # 22+ pages and once past every length
    assert {c["form"][1] for c in qc.PAGE_CASES} == {qc.page_form(qc.query(lib, 1, 64, D))[1] for D in GRID_D}
    assert {c["D"] for c in qc.PAGE_CASES} == set(GRID_D)
    assert any(c["max_len"] > max(c["lens"]) + 31 for c in qc.PAGE_CASES)
    # both forms: every D in both dtypes, a half rotary span, slabs, one-byte pools, reused pages
    for cases in (qc.TOKEN_CASES, qc.PAGE_CASES):
        assert {(c["D"], c["dtype"]) for c in cases} == set(itertools.product(GRID_D, ("f16", "bf16")))
        assert {c["D"] for c in cases if c["rot"] == c["D"] // 2} == set(GRID_D) and any(c["kv8"] for c in cases)
    assert {c["S"] for c in qc.TOKEN_CASES} == {0, 1, 3, 8, 9}
    assert {c["T"] for c in qc.TOKEN_CASES} == {1, 64, 65, 300}
    assert {(c["H"], c["Hkv"]) for c in qc.TOKEN_CASES} == {(4, 2), (5, 1), (32, 8), (16, 0), (128, 72)}
    assert any(c["past"] and len(set(c["past"])) == 3 for c in qc.PAGE_CASES)


# ---- argument checks: before any launch, so null pointers serve ---------------------------------------------------------
ONE = 1  # stands for a non-null pointer: a refused call dereferences nothing

TOKEN_OK = dict(qkv=ONE, ld=768, slabs=None, S=0, slab_ld=0, bias=None, qw=ONE, kw=ONE, eps=1e-6, cos=ONE, sin=ONE, pos=ONE,
                slots=ONE, kp=ONE, vp=ONE, T=4, H=4, Hkv=1, D=128, rot=128, dtype=0, kv=0, ks=1.0, vs=1.0)
PAGE_OK = dict(qkv=ONE, ld=768, qw=ONE, kw=ONE, eps=1e-6, cos=ONE, sin=ONE, pos=ONE, cu=ONE, past=None, bt=ONE, max_pages=4,
               kp=ONE, vp=ONE, B=2, T=40, max_len=33, H=4, Hkv=1, D=128, rot=128, dtype=0, kv=0, ks=1.0, vs=1.0)
REFUSED_BOTH = [dict(D=80), dict(D=32), dict(D=256), dict(rot=0), dict(rot=24), dict(rot=72), dict(rot=144), dict(qw=None),
                dict(kw=None), dict(cos=None), dict(sin=None), dict(pos=None), dict(eps=0.0), dict(eps=-1e-6), dict(qkv=None),
                dict(ld=760), dict(ld=767), dict(dtype=2), dict(kv=2), dict(kv=1, ks=0.0), dict(kv=1, vs=float("inf")), dict(H=0)]
REFUSED_TOKEN = [dict(slots=None), dict(slabs=ONE, S=0, slab_ld=768), dict(slabs=ONE, S=2, slab_ld=760),
                 dict(slabs=ONE, S=2, slab_ld=770), dict(bias=ONE), dict(Hkv=-1)]
REFUSED_PAGE = [dict(cu=None), dict(bt=None), dict(kp=None), dict(vp=None), dict(Hkv=0), dict(max_pages=0), dict(max_pages=1),
                dict(B=-1), dict(max_len=-1)]


def _token_call(lib, **kw):
    a = dict(TOKEN_OK, **kw)
    return lib.tgis_rope_kv_write_qknorm(a["qkv"], a["ld"], a["slabs"], a["S"], a["slab_ld"], a["bias"], a["qw"], a["kw"],
                                         a["eps"], a["cos"], a["sin"], a["pos"], a["slots"], a["kp"], a["vp"], a["T"], a["H"],
                                         a["Hkv"], a["D"], a["rot"], a["dtype"], a["kv"], a["ks"], a["vs"], None)


def _page_call(lib, **kw):
    a = dict(PAGE_OK, **kw)
    return lib.tgis_rope_kv_write_prefill_qknorm(a["qkv"], a["ld"], a["qw"], a["kw"], a["eps"], a["cos"], a["sin"], a["pos"],
                                                 a["cu"], a["past"], a["bt"], a["max_pages"], a["kp"], a["vp"], a["B"], a["T"],
                                                 a["max_len"], a["H"], a["Hkv"], a["D"], a["rot"], a["dtype"], a["kv"], a["ks"],
                                                 a["vs"], None)


@pytest.mark.parametrize("call,name,refused", [(_token_call, b"tgis_rope_kv_write_qknorm", REFUSED_BOTH + REFUSED_TOKEN),
                                               (_page_call, b"tgis_rope_kv_write_prefill_qknorm", REFUSED_BOTH + REFUSED_PAGE)],
                         ids=["per-token", "page-wise"])
def test_refused_arguments(lib, call, name, refused):
    for kw in refused:
        lib.tgis_clear_error()
        assert call(lib, **kw) == EINVAL, f"{name.decode()} accepted {kw}"
        assert name + b":" in lib.tgis_last_error(), (kw, lib.tgis_last_error())
    lib.tgis_clear_error()


def test_nothing_to_do_is_ok_and_touches_nothing(lib):
    """T == 0 and B == 0 return TGIS_OK without a launch: every pointer here is the address 1."""
    assert _token_call(lib, T=0) == 0
    assert _page_call(lib, T=0) == 0 and _page_call(lib, B=0) == 0
