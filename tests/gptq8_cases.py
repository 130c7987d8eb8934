"""The 8-bit GPTQ GEMM cases: shape, weight form and epilogue of each, and the launch it is meant to land on.

tests/test_gptq8_plans_cpu.py checks, without a GPU, that every kernel instance gptq8_gemm_kernel<TN, WK, ACT, PERM, MR>
the planner reaches on a grid of served shapes has a case here (unsplit and split), that each case still lands on the plan
it names, and that the table holds every launch edge of EDGE_RULES: a planner change then names the cases to re-choose,
and an edit that drops a case names what it lost.  tests/test_gptq8_ops_gpu.py runs each case against fp64.

A case names (TN, WK, KR, S) in `plan`; MR follows from the rows (`mr` where the case states it), PERM from the weight
form and ACT from the epilogue, as tgis_debug_gptq8_plan reports them (a host-only export of the library):
  info[8] = {TN, WK, KR, S, MR, reduce launch (0 / 1), PERM, kernel ACT}
Fields: M, K, N, groups, plan, mode (plain | trivial | act_order | perm | subnormal: the weight forms of
test_gptq8_ops_gpu._weight), pads (perm: gather entries that are -1), act, bias, id."""
import ctypes

INSTANTIATED = {(4, 2), (2, 4)}  # (TN, WK) pairs with a kernel


def query_plan(lib, M, K, N, groups=1, act=0, act_order=False):
    """The raw info[8] of tgis_debug_gptq8_plan (see gptq8.hip), or None when the library refuses the arguments."""
    fn = lib.tgis_debug_gptq8_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_int)]
    info = (ctypes.c_int * 8)()
    rc = fn(M, K, N, groups, act, int(act_order), info)
    return tuple(info) if rc == 0 else None


def perm_form(c):
    return c.get("mode") in ("act_order", "perm")


def named_plan(c):
    """The info[8] a case names."""
    TN, WK, KR, S = c["plan"]
    return (TN, WK, KR, S, c.get("mr", 2 if c["M"] > 32 else 1), int(S > 1), int(perm_form(c)), c.get("act", 0))


def case_plan(c, lib):
    info = query_plan(lib, c["M"], c["K"], c["N"], c["groups"], c.get("act", 0), perm_form(c))
    assert info is not None, f"tgis_debug_gptq8_plan refused case {c['id']}"
    return info


def instance_key(info):
    """(TN, ACT, PERM, MR, S > 1) of an info[8]: the template instance (WK = 8 / TN) and whether the launch splits k."""
    return (info[0], info[7], info[6], info[4], int(info[3] > 1))


def key_str(key):
    return "TN={} ACT={} PERM={} MR={} {}".format(*key[:4], "S>1" if key[4] else "S=1")


def _C(M, K, N, plan, G=None, gs=128, **kw):
    G = G if G is not None else K // gs
    tag = "".join(f"-{k}{'' if v is True else v}" for k, v in kw.items())
    return dict(id=f"m{M}-k{K}-n{N}-g{G}{tag}", M=M, K=K, N=N, groups=G, plan=plan, entry="gptq8", **kw)


P_TINY_A = (2, 4, 256, 1)     # (TN, WK, KR, S) of 256 x 512
P_TINY_B = (2, 4, 512, 1)     # 512 x 256
P_O = (2, 4, 768, 6)          # 4096 x 4096: 64-column blocks, six splits, the last one chunk short of the others' three
P_QKV = (4, 2, 1024, 4)       # 4096 x 12288: 128-column blocks
P_DOWN = (2, 4, 2048, 6)      # 11008 x 4096: the last split holds 3 of 8 chunks
GRID = (
    # every instance (TN, WK, MR) and split form on M x {tiny model shapes, cfg3 layer shapes}
    [_C(M, 256, 512, P_TINY_A, gs=64) for M in (1, 16, 17, 32, 33, 64)]
    + [_C(M, 512, 256, P_TINY_B, gs=64) for M in (32, 33)]
    + [_C(M, 4096, 4096, P_O) for M in (1, 16, 17, 32, 33, 64)]
    + [_C(M, 4096, 12288, P_QKV) for M in (1, 32, 33, 64)]
    + [_C(M, 11008, 4096, P_DOWN) for M in (32, 33)]
)
EDGES = [
    _C(17, 96, 64, (2, 4, 256, 1), G=1),                                  # a k64 tail, a single group
    _C(33, 96, 64, (2, 4, 256, 1), G=2),                                  # groups of 48 rows: not a power of two
    _C(5, 128, 32, (2, 4, 256, 1), G=4, bias=True),                       # N = 32: one tile, group size 32
    _C(40, 256, 96, (2, 4, 256, 1), G=2),                                 # N = 96: the last block holds one tile
    _C(32, 1280, 64, (2, 4, 768, 2), G=10, bias=True),                    # a global split whose last part is short, + bias
    _C(64, 1280, 64, (2, 4, 768, 2), G=10, act=1),                        # SiLU * up while staging, split
    _C(17, 512, 64, (2, 4, 512, 1), G=8, act=1, bias=True),
    _C(33, 512, 96, (2, 4, 512, 1), G=8, mode="act_order"),
    _C(16, 1280, 64, (2, 4, 768, 2), G=20, mode="act_order", act=1),
    _C(9, 256, 64, (2, 4, 256, 1), G=8, mode="perm", pads=56),            # a padded row shard: -1 reads a zero
    _C(64, 1280, 32, (2, 4, 768, 2), G=40, mode="perm", pads=88, bias=True),
    _C(3, 4096, 8192, (4, 2, 768, 6), G=1),                               # 256 tiles: the first 128-column plan
]


def _C8(M, K, N, plan, mr, **kw):
    c = _C(M, K, N, plan, **kw)
    c["mr"] = mr
    return c


# Every kernel instance and launch edge the cases above leave out.  The (TN = 4) instances with ACT 1 or PERM need
# N >= 8192, which no tiny model has; served checkpoints run them (act-order qkv / gate_up from 7B up, Llama-70B down).
# One case per (instance, S = 1 | S > 1) the grid of test_gptq8_plans_cpu.py reaches and per edge of EDGE_RULES, each at
# the smallest K that has the property.
INSTANCES = [
    _C8(1, 256, 8192, (4, 2, 256, 1), 1, G=2),                            # one chunk under a ring of two: half of it clamped
    _C8(33, 96, 8224, (4, 2, 256, 1), 2, G=2),                            # k64 tail, gs 48; the last block holds 1 of 4 tiles
    _C8(17, 768, 8192, (4, 2, 768, 1), 1, G=24, act=1),                   # ACT 1 on TN 4; 3 chunks: odd against U = 2
    _C8(64, 1280, 8192, (4, 2, 768, 2), 2, G=10, act=1),                  # ACT 1, MR 2, a split with a shorter last part
    _C8(5, 512, 8256, (4, 2, 512, 1), 1, G=4, mode="act_order", bias=True),   # PERM on TN 4; the last block holds 2 tiles
    _C8(40, 1312, 8224, (4, 2, 512, 3), 2, G=82, mode="act_order"),       # PERM MR 2; last part 288 rows; gs 16; ragged, S > 1
    _C8(16, 1056, 8224, (4, 2, 768, 2), 1, G=33, mode="act_order", act=1),    # ACT 1 + PERM, split
    _C8(48, 512, 8192, (4, 2, 512, 1), 2, G=4, mode="act_order", act=1),  # ACT 1 + PERM + MR 2
    _C8(9, 320, 8192, (4, 2, 512, 1), 1, G=10, mode="perm", pads=40),     # -1 pads on TN 4; K % 256 = 64
    _C8(7, 512, 8288, (4, 2, 512, 1), 1, G=4, bias=True),                 # the last block holds 3 tiles
    _C8(48, 512, 64, (2, 4, 512, 1), 2, G=8, mode="act_order", act=1),    # the TN 2 instance no case launched
    _C8(7, 1568, 64, (2, 4, 768, 3), 1, G=98, bias=True),                 # gs 16; a last split of 32 rows
    _C8(3, 6144, 4096, (2, 4, 1024, 6), 1, G=48),                         # exactly U = 4 chunks per split
    _C8(33, 7680, 4096, (2, 4, 1280, 6), 2, G=60),                        # U + 1 chunks per split
    # the S = 1 | S > 1 halves of instances that the cases above run only the other way
    _C8(17, 1280, 8192, (4, 2, 768, 2), 1, G=10, act=1),
    _C8(5, 1056, 8224, (4, 2, 768, 2), 1, G=33, mode="act_order"),
    _C8(33, 512, 8192, (4, 2, 512, 1), 2, G=4, mode="act_order"),
    _C8(16, 512, 8192, (4, 2, 512, 1), 1, G=4, mode="act_order", act=1),
    _C8(48, 1056, 8192, (4, 2, 768, 2), 2, G=33, mode="act_order", act=1),
    _C8(33, 512, 8192, (4, 2, 512, 1), 2, G=4, act=1),
    _C8(17, 1280, 64, (2, 4, 768, 2), 1, G=10, act=1),
    _C8(33, 512, 64, (2, 4, 512, 1), 2, G=8, act=1),
    _C8(9, 1280, 64, (2, 4, 768, 2), 1, G=20, mode="act_order"),
    _C8(16, 512, 64, (2, 4, 512, 1), 1, G=8, mode="act_order", act=1),
    _C8(48, 1280, 64, (2, 4, 768, 2), 2, G=20, mode="act_order", act=1),
]
CASES = GRID + EDGES + INSTANCES

# Subnormal products (weight mode "subnormal": f16 column scales 2^-10 .. 2^-24, one column s = 0), both block forms.
SUBNORMAL = [
    _C8(M, 512, N, plan, mr, G=4, mode="subnormal")
    for N, plan in ((64, (2, 4, 512, 1)), (8192, (4, 2, 512, 1))) for M, mr in ((17, 1), (48, 2))
]


def _tiles(c):
    return -(-c["N"] // 32)


def _whole(c, n):
    """An unsplit launch over exactly n whole 256-row chunks."""
    return c["plan"][3] == 1 and c["K"] == c["plan"][2] == 256 * n


# (what the table must hold, predicate on a case: K, N, weight form and the plan it names)
EDGE_RULES = [
    (f"a TN = 4 case, S = 1, whose last column block holds {r} of its 4 tiles",
     lambda c, r=r: c["plan"][0] == 4 and c["plan"][3] == 1 and _tiles(c) % 4 == r) for r in (1, 2, 3)
] + [
    ("a TN = 4 case, S > 1, whose last column block is ragged", lambda c: c["plan"][0] == 4 and c["plan"][3] > 1 and _tiles(c) % 4),
] + [
    (f"a WK = 2 case of exactly {n} whole chunk(s), unsplit (ring of U = 2)", lambda c, n=n: c["plan"][1] == 2 and _whole(c, n))
    for n in (1, 2, 3)
] + [
    (f"a WK = 4 case with {n} chunks per split (ring of U = 4)", lambda c, n=n: c["plan"][1] == 4 and c["plan"][2] == 256 * n)
    for n in (1, 2, 3, 4, 5, 8)
] + [
    ("a case whose last split holds 32 rows", lambda c: c["plan"][3] > 1 and c["K"] - (c["plan"][3] - 1) * c["plan"][2] == 32),
    ("a case whose last split is a chunk or more short", lambda c: c["plan"][3] > 1 and c["plan"][3] * c["plan"][2] - c["K"] >= 256),
    ("a TN = 2 case of group size 16", lambda c: c["plan"][0] == 2 and c["K"] // c["groups"] == 16),
    ("a TN = 4 case of group size 16", lambda c: c["plan"][0] == 4 and c["K"] // c["groups"] == 16),
    ("a case of group size 48 (no power of two)", lambda c: c["K"] // c["groups"] == 48),
    ("a TN = 4 case with a k64 tail (K % 64 == 32)", lambda c: c["plan"][0] == 4 and c["K"] % 64 == 32),
    ("a TN = 2 case with a k64 tail (K % 64 == 32)", lambda c: c["plan"][0] == 2 and c["K"] % 64 == 32),
    ("a TN = 4 case with an explicit gather holding -1 pads",
     lambda c: c["plan"][0] == 4 and c.get("mode") == "perm" and c.get("pads", 0) > 0),
    ("a TN = 2 case with an explicit gather holding -1 pads",
     lambda c: c["plan"][0] == 2 and c.get("mode") == "perm" and c.get("pads", 0) > 0),
    ("a TN = 4 case with K % 256 == 64", lambda c: c["plan"][0] == 4 and c["K"] % 256 == 64),
]
