"""CPU: the launch plan of paged attention (csrc/attention_plan.h plan_attn, reported by tgis_debug_attn_plan) against a
restatement of what attn_paged_impl and its launchers decided before the plan had a home of its own, over the grid of
test_attn_qsplit_rule_cpu.py; the plan's invariants at every grid point; the per-launch hooks; and that every variant the
default planner reaches on the grid is run by a case of the GPU files."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_cases as ac  # noqa: E402
from test_attn_qsplit_rule_cpu import BS, CTXS, HEADS, QS, _geom, num_splits_q, prefill_form  # noqa: E402
from test_kv_layout_cpu import _cdiv, _library_or_skip  # noqa: E402

# (tree, ch, nw, pipe) with an attn_paged_kernel instance
INSTANTIATED = ({(False, 1, nw, False) for nw in (1, 2, 3, 4, 8)} | {(False, 1, 2, True), (False, 1, 4, True)} |
                {(False, ch, nw, False) for ch in (2, 3) for nw in (1, 2, 4)} | {(False, 2, 4, True), (False, 3, 4, True)} |
                {(True, 1, 4, False)})


def restated_plan(B, H, Hkv, D, q, ns, tree, nw_env=None, ch_env=None, no_prefill_kernel=False):
    """The launch of tgis_attn_paged[_tree] restated from attn_paged_impl, launch_attn, launch_attn_one, launch_attn_pipe,
    launch_attn_tree and tgis_launch_attn_prefill; None where the call is refused.  Default PIPE / XCD / FUSED_COMBINE."""
    G, Gp, TQ, HC = _geom(H, Hkv)
    prefill = q * Gp > 64
    if prefill and (ns > 1 or tree):
        return None
    if prefill and not no_prefill_kernel:
        grid = (_cdiv(q, TQ * 8), Hkv * HC, B)
        if grid[1] > 65535 or grid[2] > 65535:
            return None
        return {"form": "prefill", "nw": 4, "ch": 1, "hcb": HC, "pipe": 0, "xcd_remap": 0, "grid": grid,
                "lds": 2 * 2 * 32 * D * 2, "merge": "none"}

    def chunks_per_block():
        most = ch_env if ch_env in (1, 2, 3) else 3
        return min(HC, most) if q == 1 and HC > 1 else 1

    ch = 1 if tree else chunks_per_block()
    HCB = _cdiv(HC, ch)
    q_tiles = _cdiv(q, TQ)
    grid = (q_tiles, Hkv * HCB, B * ns)
    if grid[1] > 65535 or grid[2] > 65535:
        return None
    if tree:
        nw, pipe, xcd = 4, 0, 0
    else:
        xcd = int(q == 1 and q_tiles == 1 and HCB > 1 and (B * ns * Hkv) % 8 == 0)
        nblocks = grid[0] * grid[1] * grid[2]
        nw = 2 if q == 1 and 1024 <= nblocks < 2048 else 4
        if q == 1 and ch == 1 and nblocks // ns < 256:  # wide_decode_blocks
            nw = 8
        if nw_env is not None:
            nw = nw_env if nw_env in (1, 2, 3, 8) else 4
            if ch > 1 and (nw > 4 or nw == 3):
                nw = 4
        pipe = int(ch > 1 and nw == 4)  # TGIS_ATTN_PIPE unset: multi-chunk blocks of 4 waves only
    lds = ch * (nw * D * 16 + nw * 2 * 16) * 4
    merge = "none"
    if ns > 1:
        ch_rec = chunks_per_block()  # fused_records: the causal launch's chunks per block, for the tree launch as well
        recs = B * q_tiles * Hkv * _cdiv(HC, ch_rec) * ch_rec * 16 * ns
        groups = B * q_tiles * Hkv * HCB
        fused = groups <= (1 << 20) and recs * D * 4 < (1 << 31) and ch == 1
        merge = "fused" if fused else "combine8" if ns <= 8 else "combine"
    return {"form": "tree" if tree else "decode", "nw": nw, "ch": ch, "hcb": HCB, "pipe": pipe, "xcd_remap": xcd,
            "grid": grid, "lds": lds, "merge": merge}


def grid_points(ds=(128,)):
    """(B, H, Hkv, D, q, ns, tree) over BS x HEADS x CTXS x QS: at the rule's split count and at 1, tree on and off."""
    seen = set()
    for B in BS:
        for Hkv, H in HEADS:
            for ctx in CTXS:
                for q in QS:
                    for ns in {num_splits_q(B, Hkv, H, q, ctx), 1}:
                        for D in ds:
                            for tree in (False, True):
                                pt = (B, H, Hkv, D, q, ns, tree)
                                if pt not in seen:
                                    seen.add(pt)
                                    yield pt


@pytest.fixture(scope="module")
def lib():
    return _library_or_skip()


def _compare(lib, pt, **hooks):
    B, H, Hkv, D, q, ns, tree = pt
    want = restated_plan(*pt, **hooks)
    info = ac.query_plan(lib, B, H, Hkv, D, q, ns, tree)
    if want is None:
        assert info is None, (pt, hooks, "should be refused")
        return None
    assert info is not None, (pt, hooks, lib.tgis_last_error())
    got = ac.plan_fields(info)
    assert {k: got[k] for k in want} == want, (pt, hooks)
    return got


def test_plan_matches_the_restatement_and_keeps_its_invariants(lib):
    import ctypes

    lib.tgis_attn_workspace_bytes.restype = ctypes.c_int64
    refused = 0
    for pt in grid_points():
        B, H, Hkv, D, q, ns, tree = pt
        p = _compare(lib, pt)
        if p is None:
            assert prefill_form(H, Hkv, q) and tree and ns == 1, pt  # the grid's only refusals: a tree in the prefill form
            refused += 1
            continue
        assert (p["gp"], p["tq"], p["hc"]) == _geom(H, Hkv)[1:], pt
        if p["form"] != "prefill":
            assert (p["form"] == "tree", p["ch"], p["nw"], bool(p["pipe"])) in INSTANTIATED, pt
        assert p["grid"][1] <= 65535 and p["grid"][2] <= 65535, pt
        if p["xcd_remap"]:
            assert p["grid"][0] == 1 and p["hcb"] > 1 and (B * ns * Hkv) % 8 == 0, pt
        if p["fused_ok"]:
            assert p["ch"] == 1 and ns > 1, pt
        if ns > 1:
            # both record layouts fit what callers allocate for B * q rows: ws_o then ws_ml
            have = lib.tgis_attn_workspace_bytes(B * q, H, Hkv, D, ns)
            records = p["grid"][0] * p["grid"][1] * B * p["ch"] * 16 * ns
            assert have >= B * q * H * ns * (D + 2) * 4, pt
            assert have >= records * (D + 4) * 4, pt
    assert refused


def test_lds_bytes_at_every_head_size(lib):
    for pt in grid_points(ds=(64, 96)):
        if pt[0] in (1, 8, 128):
            _compare(lib, pt)


def test_refusals(lib):
    for args, msg in (((1, 64, 3, 128, 1, 1, 0), b"multiple of Hkv"), ((1, 64, 0, 128, 1, 1, 0), b"multiple of Hkv"),
                      ((1, 32, 32, 80, 1, 1, 0), b"head_dim"), ((1, 32, 32, 128, 0, 1, 0), b"bad launch bounds"),
                      ((1, 32, 32, 128, 1, 0, 0), b"bad launch bounds"), ((1, 32, 32, 128, 65, 2, 0), b"prefill form takes none"),
                      ((1, 32, 32, 128, 65, 1, 1), b"only the decode form"), ((70000, 32, 32, 128, 1, 1, 0), b"grid too large"),
                      ((2000, 32, 32, 128, 1, 64, 0), b"grid too large"), ((0, 32, 32, 128, 1, 1, 0), b"tgis_debug_attn_plan")):
        assert ac.query_plan(lib, *args) is None, args
        assert msg in lib.tgis_last_error(), (args, lib.tgis_last_error())


# ---- the per-launch hooks (TGIS_ATTN_PIPE, _XCD and _FUSED_COMBINE are read once per process: the GPU files' children) ----
HOOK_POINTS = [pt for pt in grid_points() if pt[0] in (1, 8, 32, 128)]


@pytest.mark.parametrize("value", ["1", "2", "3", "4", "8", "0", "5", "x"])
def test_plan_follows_TGIS_ATTN_NW(lib, monkeypatch, value):
    monkeypatch.setenv("TGIS_ATTN_NW", value)
    nw = int(value) if value.isdigit() else 0
    seen = {_compare(lib, pt, nw_env=nw)["nw"] for pt in HOOK_POINTS if restated_plan(*pt) and not pt[6]
            and restated_plan(*pt)["form"] == "decode"}
    assert (nw if nw in (1, 2, 3, 8) else 4) in seen
    for pt in HOOK_POINTS:  # the tree launch and the prefill form do not follow it
        if restated_plan(*pt) and restated_plan(*pt)["form"] != "decode":
            _compare(lib, pt)


@pytest.mark.parametrize("value", ["1", "2", "3", "0", "4"])
def test_plan_and_sizes_follow_TGIS_ATTN_CH(lib, monkeypatch, value):
    import ctypes

    lib.tgis_attn_workspace_bytes.restype = ctypes.c_int64
    monkeypatch.setenv("TGIS_ATTN_CH", value)
    chs = set()
    for pt in HOOK_POINTS:
        p = _compare(lib, pt, ch_env=int(value))
        if p is not None:
            chs.add(p["ch"])
            B, H, Hkv, D, q, ns, tree = pt
            if ns > 1:
                records = p["grid"][0] * p["grid"][1] * B * p["ch"] * 16 * ns
                assert lib.tgis_attn_workspace_bytes(B * q, H, Hkv, D, ns) >= records * (D + 4) * 4, pt
    assert max(chs) == (int(value) if value in ("1", "2", "3") else 3)
    # the split rule counts the blocks of the chunks per block it is given.  MQA 48:1, B 32, ctx 4096 (128 pages): 96 one-chunk
    # blocks take the few-groups rule, max(min(cdiv(256, 96), 128 // 16), min(256 // 96, 128 // 8, 8)) = 3; 64 two-chunk blocks
    # min(cdiv(256, 64), 128 // 16) = 4; 32 three-chunk blocks min(cdiv(256, 32), 128 // 16) = 8
    assert lib.tgis_attn_num_splits(32, 1, 48, 1, 4096) == {"1": 3, "2": 4}.get(value, 8)


def test_plan_follows_TGIS_ATTN_NO_PREFILL_KERNEL(lib, monkeypatch):
    monkeypatch.setenv("TGIS_ATTN_NO_PREFILL_KERNEL", "1")
    forms = set()
    for pt in HOOK_POINTS:
        p = _compare(lib, pt, no_prefill_kernel=True)
        if p is not None:
            forms.add(p["form"])
            if prefill_form(pt[1], pt[2], pt[4]):
                assert p["form"] == "decode" and p["grid"][0] == _cdiv(pt[4], p["tq"]) and p["nw"] == 4 and p["ch"] == 1, pt
    assert forms == {"decode", "tree"}


# ---- coverage of the GPU files ------------------------------------------------------------------------------------------
def _gpu_case_keys(lib):
    """variant key -> a GPU case that runs it: every tgis_attn_paged call of the case tables (imported, not copied)."""
    import test_attention_edges_gpu as edges
    import test_attn_qsplit_gpu as qsplit
    import test_spec_tree_ops_gpu as tree

    keys = {}

    def add(what, H, Hkv, D, seqs, splits, is_tree=False):
        for ns in splits:
            keys.setdefault(ac.case_key(lib, H, Hkv, D, seqs, ns, is_tree), f"{what} at {ns} split(s)")

    for name, _, H, Hkv, D, lens in edges.DECODE:
        ns = lib.tgis_attn_num_splits(len(lens), Hkv, H, 1, max(lens))
        add(f"edges.DECODE {name}", H, Hkv, D, [(1, l) for l in lens], (ns,))
    for name, _, H, Hkv, D, lens, ns, _ in edges.SPLITS:
        add(f"edges.SPLITS {name}", H, Hkv, D, [(1, l) for l in lens], (ns, 1))
    for name, _, H, Hkv, D, seqs in edges.CONTRACT:
        add(f"edges.CONTRACT {name}", H, Hkv, D, seqs, (1,))
    for table in (edges.SHORT, edges.PREFILL):
        for name, _, H, Hkv, D, lens in table:
            add(f"edges {name}", H, Hkv, D, [(l, l) for l in lens], (1,))
    for name, _, H, Hkv, D, seqs, splits in qsplit.CASES:
        add(f"qsplit.CASES {name}", H, Hkv, D, seqs, (1,) + tuple(splits))
    for name, _, H, Hkv, D, seqs in tree.SHORT:
        add(f"tree.SHORT {name}", H, Hkv, D, seqs, (1,), True)
    for name, _, H, Hkv, D, seqs, splits in tree.SPLIT:
        add(f"tree.SPLIT {name}", H, Hkv, D, seqs, (1,) + tuple(splits), True)
    return keys


def _cost(pt):
    B, H, Hkv, D, q, ctx = pt
    return B * q * ctx * (H + Hkv)


def test_every_reachable_variant_has_a_gpu_case(lib):
    reached = {}
    for B in BS:
        for Hkv, H in HEADS:
            for ctx in CTXS:
                for q in QS:
                    if q > ctx:
                        continue
                    ns = lib.tgis_attn_num_splits_q(B, Hkv, H, q, ctx)
                    for is_tree in (False, True):
                        info = ac.query_plan(lib, B, H, Hkv, 128, q, ns, is_tree)
                        if info is None:
                            continue
                        key, pt = ac.variant_key(info), (B, H, Hkv, 128, q, ctx)
                        if key not in reached or _cost(pt) < _cost(reached[key][0]):
                            reached[key] = (pt, ns, is_tree)
    covered = _gpu_case_keys(lib)
    missing = [f"{ac.key_str(k)}\n    cheapest: B {pt[0]} H {pt[1]} Hkv {pt[2]} D {pt[3]} q_len {pt[4]} ctx {pt[5]}, {ns} split(s)"
               f"{', tree' if t else ''}" for k, (pt, ns, t) in sorted(reached.items(), key=str) if k not in covered]
    assert not missing, "variants the planner reaches without a GPU case (add one to test_attention_edges_gpu.DECODE):\n" + \
        "\n".join(missing)
    assert len(reached) >= 10, sorted(reached)


def test_added_gpu_cases_land_on_the_variant_they_name(lib):
    import test_attention_edges_gpu as edges

    for name, _, H, Hkv, D, lens in edges.DECODE:
        ns = lib.tgis_attn_num_splits(len(lens), Hkv, H, 1, max(lens))
        got = ac.key_str(ac.case_key(lib, H, Hkv, D, [(1, l) for l in lens], ns))
        assert got == edges.DECODE_VARIANTS[name], f"{name} lands on {got}: re-choose it"
