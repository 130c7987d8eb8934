"""CPU: the launch form of every row-wise entry point (norms, rope + cache writes, argmax, sampler), no GPU needed: the
choosers are host code, reported by tgis_debug_rowwise_plan.

Each case of tests/rowwise_cases.py must land on the form it states.  Each launch rule is restated here in Python and
checked against the library over a grid, and every form the rules reach on that grid must have a case: a threshold change
fails here first and names the cases to re-choose."""
import itertools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowwise_cases as rc  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from tgis_amd import native

    return native.load_library()


def _cdiv(a, b):
    return -(-a // b)


# ---- the rules, restated --------------------------------------------------------------------------------------------------
def norm_rule(rows, hidden):
    nt = 512 if rows <= 64 and hidden >= 2048 else 256
    return (nt, _cdiv(hidden // 8, nt))


def rope_rule(T, H, Hkv, D, rot):
    items = (H + 2 * Hkv) * D // 8
    gy = min(16, _cdiv(items, 256)) if T <= 64 else 1
    return (gy, int(rot > 0 and rot % 16 != 0), int(gy * 256 < items))


def prefill_rule(max_len, rot):
    return (_cdiv(max_len, 32), int(rot > 0 and rot % 16 != 0))


def argmax_rule(B, V, scratch):
    nseg = min(16, 256 // max(B, 1))
    while nseg > 1 and _cdiv(V, nseg) < 1024:
        nseg -= 1
    return (nseg, int(scratch >= 0 and nseg > 1 and scratch >= rc.PART * B * nseg))


def sampler_rule(V):
    return (int(V <= 32768 and "TGIS_SAMPLER_GLOBAL_ROWS" not in os.environ),)


# ---- grids ------------------------------------------------------------------------------------------------------------------
NORM_ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 100, 200, 256, 1000)
NORM_HIDDEN = tuple(range(8, 16385, 8))
# (H, Hkv, D, rot) of the served configs and their TP shards (rotary, NeoX partial rotary, no rope, q only), plus ROPE_HEADS
ROPE_GRID_HEADS = sorted({(H // tp, max(Hkv // tp, 1) if Hkv else 0, D, rot)
                          for H, Hkv, D, rot in ((32, 32, 128, 128), (64, 8, 128, 128), (32, 4, 64, 64), (64, 64, 96, 24),
                                                 (16, 16, 128, 32), (12, 12, 64, 16), (48, 1, 128, 0), (16, 1, 128, 0),
                                                 (32, 0, 128, 128), (64, 0, 96, 24))
                          for tp in (1, 2, 4, 8) if H % tp == 0} | {h for h, _ in rc.ROPE_HEADS.values()})
ROPE_GRID_T = (1, 2, 16, 32, 63, 64, 65, 128, 300, 4096)
ARGMAX_B = tuple(range(1, 40)) + (63, 64, 65, 85, 86, 127, 128, 129, 200, 256, 257, 1024)
ARGMAX_V = (41, 1000, 1023, 1024, 1025, 2046, 2047, 2048, 4096, 16368, 16369, 32000, 32768, 49152, 50257, 152064)


def test_cases_land_on_their_forms(lib):
    bad = [f"{c['id']}: states {tuple(c['form'])}, lands on {rc.case_form(c, lib)}" for c in rc.CASES
           if rc.case_form(c, lib) != tuple(c["form"])]
    assert not bad, "re-choose these cases:\n" + "\n".join(bad)


def test_norm_rule_restated(lib):
    for rows, hidden in itertools.product(NORM_ROWS, NORM_HIDDEN):
        assert rc.form_of("norm", rc.query(lib, "norm", rows, hidden)) == norm_rule(rows, hidden), (rows, hidden)


def test_rope_rules_restated(lib):
    for (H, Hkv, D, rot), T in itertools.product(ROPE_GRID_HEADS, ROPE_GRID_T):
        got = rc.form_of("rope", rc.query(lib, "rope", T, H, Hkv, D, rot, int(rot > 0)))
        assert got == rope_rule(T, H, Hkv, D, rot), (T, H, Hkv, D, rot)
    for max_len, rot in itertools.product((1, 31, 32, 33, 64, 65, 700, 4096, 32768), (0, 10, 24, 32, 64, 128)):
        got = rc.form_of("rope_prefill", rc.query(lib, "rope_prefill", max_len, rot, int(rot > 0)))
        assert got == prefill_rule(max_len, rot), (max_len, rot)


def test_argmax_and_sampler_rules_restated(lib):
    for B, V in itertools.product(ARGMAX_B, ARGMAX_V):
        nseg = argmax_rule(B, V, -1)[0]
        need = rc.PART * B * max(nseg, 1)
        for scratch in (-1, 0, need - rc.PART * max(nseg, 1), need, need + 1):
            got = rc.form_of("argmax", rc.query(lib, "argmax", B, V, scratch))
            assert got == argmax_rule(B, V, scratch), (B, V, scratch)
            assert got[1] == 0 or rc.query(lib, "argmax", B, V, scratch)[2] == _cdiv(V, nseg)  # seg_len
    for V in (1, 41, 32000, 32767, 32768, 32769, 50257, 152064):
        assert rc.form_of("sampler", rc.query(lib, "sampler", V)) == sampler_rule(V), V


def test_every_reachable_form_has_a_case():
    missing = []
    # norms: every (kind, nt, iters), plain and partial alike (the 512-thread kernel reaches 1..4 chunks, the 256 one 1..8)
    forms = {norm_rule(r, h) for r, h in itertools.product(NORM_ROWS, NORM_HIDDEN)}
    have = {(c["op"], *c["form"]) for c in rc.NORM_CASES}
    missing += [f"norm {k} nt={nt} iters={it}" for k in rc.NORM_KINDS for nt, it in sorted(forms)
                if (k, nt, it) not in have]
    # rope per token: (gy > 1, gen, strided, rope) on plain and partial input; a q-only launch (Hkv = 0) of each input kind
    forms = {(f[0] > 1, f[1], f[2], rot > 0) for (H, Hkv, D, rot), T in itertools.product(ROPE_GRID_HEADS, ROPE_GRID_T)
             for f in [rope_rule(T, H, Hkv, D, rot)]}
    have = {(c["form"][0] > 1, c["form"][1], c["form"][2], c["rot"] > 0, c["S"] > 0) for c in rc.ROPE_CASES}
    missing += [f"rope multi-y={m} gen={g} strided={s} rope={r} partial={p}" for (m, g, s, r) in sorted(forms)
                for p in (False, True) if (m, g, s, r, p) not in have]
    missing += [f"rope q-only partial={p}" for p in (False, True)
                if not any(c["Hkv"] == 0 and (c["S"] > 0) == p for c in rc.ROPE_CASES)]
    # rope prefill: gen / not gen / no rope
    have = {(c["form"][1], c["rot"] > 0) for c in rc.PREFILL_CASES}
    missing += [f"prefill gen={g} rope={r}" for g, r in ((0, True), (1, True), (0, False)) if (g, r) not in have]
    # argmax: the one-block form, and the split form at every segment count it reaches
    forms = {argmax_rule(B, V, 1 << 40) for B, V in itertools.product(ARGMAX_B, ARGMAX_V)}
    have = {tuple(c["form"]) for c in rc.ARGMAX_CASES}
    missing += [f"argmax nseg={n} split" for n, s in sorted(forms) if s and (n, 1) not in have]
    missing += ["argmax one-block form"] if not any(f[1] == 0 for f in have) else []
    have = {c["form"] for c in rc.CASES if c["op"] == "sampler"}
    missing += [f"sampler reg={r}" for r in (0, 1) if (r,) not in have]
    assert not missing, "forms without a case:\n" + "\n".join(missing)


def test_cases_cover_the_edges():
    """What the issue of this table asks for besides the forms: thresholds from both sides and the input edges."""
    norm = rc.NORM_CASES
    assert {c["rows"] for c in norm} >= {1, 63, 64, 65, 200}
    assert {c["hidden"] for c in norm} >= {8, 72, 768, 2040, 2048, 2056, 4096, 5120, 6144, 8192, 16384}
    for kind in rc.NORM_KINDS:
        for dt in ("f16", "bf16"):
            assert any(c["op"] == kind and c["dtype"] == dt for c in norm), (kind, dt)
        assert any(c["op"] == kind and c["form"] in ((512, 4), (256, 8)) and c["hidden"] == 16384 for c in norm), kind
    for kind in ("rms_partial", "ln_partial"):
        pc = [c for c in norm if c["op"] == kind]
        for S in rc.SLABS:  # every slab bucket on a tail 32-row block past the 512-thread threshold
            assert any(c["S"] == S and c["rows"] > 64 and c["rows"] % 32 for c in pc), (kind, S)
        assert all(c["slab_pad"] > 0 for c in pc)
        assert {c["xbias"] for c in pc} == {False, True}
    assert any(not c["residual"] for c in norm if c["op"] in ("rms", "ln", "rms_partial", "ln_partial"))
    assert {c["bias"] for c in norm if c["op"] in ("ln", "ln_partial")} == {False, True}
    ln2 = [c for c in norm if c["op"] == "ln2"]
    for ad in rc.ADDENDS:
        assert any(c["A"] == ad for c in ln2) and any(c["B"] == ad for c in ln2), ad
    assert any(c["rows"] > 64 and c["hidden"] >= 2048 for c in ln2)
    assert {c["SA"] for c in ln2} >= set(rc.SLABS)

    rope = rc.ROPE_CASES
    assert {c["T"] for c in rope} >= {1, 64, 65, 300}
    items = {(c["H"] + 2 * c["Hkv"]) * c["D"] // 8 for c in rope}
    assert min(items) < 256 and 4096 in items and any(i > 4096 for i in items)
    assert any(c["form"][2] and c["T"] <= 64 for c in rope)  # grid-stride at decode-sized T
    heads = {(c["H"], c["Hkv"], c["D"], c["rot"]) for c in rope}
    assert heads >= {(32, 32, 128, 128), (64, 8, 128, 128), (8, 1, 128, 128), (16, 1, 128, 0)}
    assert any(D == 96 and rot == 24 for _, _, D, rot in heads) and any(D == 64 and rot == 10 for _, _, D, rot in heads)
    assert {c["S"] for c in rope} >= set(rc.SLABS) | {0}
    lens = {n for c in rc.PREFILL_CASES for n in c["lens"]}
    assert lens >= {1, 31, 32, 33, 64, 65, 700}
    assert any(c["max_len"] > sorted(c["lens"])[len(c["lens"]) // 2] for c in rc.PREFILL_CASES if len(c["lens"]) > 2)

    am = rc.ARGMAX_CASES
    assert {c["B"] for c in am} >= {16, 17, 32, 33, 128, 129, 256, 257}
    assert {c["V"] for c in am} >= {32000, 50257, 152064, 16368, 16369}
    assert {c["scratch"] for c in am} == {"none", "exact", "short"}
    assert {c["dtype"] for c in am if c["form"][1]} == {"f32", "f16", "bf16"}
    assert any(c["ld_pad"] and c["form"][1] for c in am) and any(c["ld_pad"] and not c["form"][1] for c in am)
    assert {c["V"] for c in rc.CASES if c["op"] == "sampler"} == {32768, 32769}


@pytest.mark.parametrize("hidden", [16392, 2052, 0, 16384 + 8 * 1024])
def test_norm_shapes_refused(lib, hidden):
    assert rc.query(lib, "norm", 1, hidden) is None
