"""The row-wise edge cases: norms, rope + cache writes, argmax, the sampler and the small decode helpers, each with the launch
form it is meant to reach.

tests/test_rowwise_plans_cpu.py checks, without a GPU, that each case still lands on the form it states, restates every
launch rule in Python against the library, and checks that every form those rules reach has a case: a rule change then
names the cases to re-choose.  tests/test_rowwise_edges_gpu.py runs each case against a plain high-precision reference.

The form of a case is what tgis_debug_rowwise_plan reports for it (a host-only export of the library, kept out of
include/tgis_hip.h like tgis_debug_gemm_plan):
  norm          (nt, iters)        threads per row, 16-byte chunks per thread        (tgis_*norm_residual*, layernorm2)
  rope          (gy, gen, strided) workgroups per token, rot % 16 != 0 span, grid-stride loop   (tgis_rope_kv_write*)
  rope_prefill  (pps, gen)         32-token pages per sequence in the grid          (tgis_rope_kv_write_prefill)
  argmax        (nseg, split)      segments per row, two-launch split form          (tgis_argmax_logprob)
  sampler       (reg,)             register-row kernel, else the global-row kernel  (tgis_warp_sample)
The stated forms below are written out by hand (ITERS, the per-shape gy / nseg) rather than computed with the rule they
check.
"""
import ctypes

OPS = {"norm": 0, "rope": 1, "rope_prefill": 2, "argmax": 3, "sampler": 4}


def query(lib, op, *args):
    """The raw info[8] of tgis_debug_rowwise_plan (see elementwise.hip), or None when the library refuses the arguments."""
    fn = lib.tgis_debug_rowwise_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    a = (ctypes.c_int64 * 8)(*args)
    info = (ctypes.c_int64 * 8)()
    return list(info) if fn(OPS[op], a, info) == 0 else None


def plan_args(c):
    """(op, args) of the plan query a case's launch makes."""
    op = c["op"]
    if op in NORM_KINDS:
        return "norm", (c["rows"], c["hidden"])
    if op == "rope":
        return "rope", (c["T"], c["H"], c["Hkv"], c["D"], c["rot"], int(c["rot"] > 0))
    if op == "rope_prefill":
        return "rope_prefill", (c["max_len"], c["rot"], int(c["rot"] > 0))
    if op == "argmax":
        return "argmax", (c["B"], c["V"], scratch_bytes(c))
    if op == "sampler":
        return "sampler", (c["V"],)
    raise KeyError(op)


def form_of(op, info):
    if op == "norm":
        return (info[0], info[1])
    if op == "rope":
        return (info[0], info[1], info[2])
    if op == "rope_prefill":
        return (info[0], info[1])
    if op == "argmax":
        return (info[0], info[1])
    return (info[0],)


def case_form(c, lib):
    op, args = plan_args(c)
    info = query(lib, op, *args)
    assert info is not None, f"tgis_debug_rowwise_plan refused case {c['id']}"
    return form_of(op, info)


PART = 16  # bytes of one argmax segment record (ArgmaxPart)


def scratch_bytes(c):
    """-1 (no scratch), exactly the split form's need, or one row short of it."""
    if c["scratch"] == "none":
        return -1
    need = PART * c["B"] * max(c["nseg"], 1)
    return need if c["scratch"] == "exact" else need - PART * max(c["nseg"], 1)


# ---- norms ------------------------------------------------------------------------------------------------------------------
NORM_KINDS = ("rms", "ln", "rms_partial", "ln_partial", "ln2")
HIDDENS = (8, 72, 768, 2040, 2048, 2056, 4096, 5120, 6144, 8192, 10240, 12288, 14336, 16384)
# chunks per thread, hidden / 8 / NT rounded up: both kernels run their whole register array (MAXV) at hidden 16384
ITERS = {
    256: {8: 1, 72: 1, 768: 1, 2040: 1, 2048: 1, 2056: 2, 4096: 2, 5120: 3, 6144: 3, 8192: 4, 10240: 5, 12288: 6,
          14336: 7, 16384: 8},
    512: {2048: 1, 2056: 1, 4096: 1, 5120: 2, 6144: 2, 8192: 2, 10240: 3, 12288: 3, 14336: 4, 16384: 4},
}
SLABS = (1, 2, 3, 4, 5, 8, 9, 16)  # sum_slabs8 buckets 1, 2, 3-4, 5-8 and the tail loop past 8
# layernorm2 addends: (kind, with bias)
ADDENDS = (("tensor", False), ("tensor", True), ("slabs", False), ("slabs", True), ("bias", True), ("none", False))


def _norm_cases():
    out = []
    i = 0
    for kind in NORM_KINDS:
        for hi, hidden in enumerate(HIDDENS):
            for rows in (64, 65, (1, 63, 200)[(hi + NORM_KINDS.index(kind)) % 3]):
                nt = 512 if (rows <= 64 and hidden >= 2048) else 256
                c = dict(op=kind, rows=rows, hidden=hidden, dtype=("f16", "bf16")[i % 2], form=(nt, ITERS[nt][hidden]))
                if kind != "ln2":
                    c["residual"] = i % 5 != 0
                if kind in ("ln", "ln_partial"):
                    c["bias"] = i % 3 != 1
                if kind.endswith("_partial"):
                    c["S"] = SLABS[i % len(SLABS)]
                    c["slab_pad"] = (4, 12, 36)[i % 3]  # slab_ld = hidden + pad (a multiple of 4)
                    c["xbias"] = (i // 2) % 2 == 0
                if kind == "ln2":
                    j = len(out) - NORM_KINDS.index("ln2") * 3 * len(HIDDENS)  # every (A, B) pair over the ln2 cases
                    c["A"], c["B"] = ADDENDS[j % len(ADDENDS)], ADDENDS[j // len(ADDENDS) % len(ADDENDS)]
                    c["SA"], c["SB"] = SLABS[i % len(SLABS)], SLABS[(i + 3) % len(SLABS)]
                    c["slab_pad"] = (4, 12, 36)[i % 3]
                    c["y2"] = i % 3 != 2
                c["id"] = f"{kind}-r{rows}-h{hidden}-{c['dtype']}" + (f"-S{c['S']}" if "S" in c else "") + (
                    f"-{c['A'][0]}{'b' if c['A'][1] else ''}-{c['B'][0]}{'b' if c['B'][1] else ''}" if kind == "ln2" else "")
                out.append(c)
                i += 1
    return out


# ---- rope + cache write, per token ------------------------------------------------------------------------------------------
# (H, Hkv, D, rot; rot 0 = no rope) and the gy a decode-sized T (<= 64) takes: ceil((H + 2 Hkv) D / 8 / 256), at most 16
ROPE_HEADS = {
    "llama7b": ((32, 32, 128, 128), 6),
    "llama70b": ((64, 8, 128, 128), 5),
    "llama70b-tp8": ((8, 1, 128, 128), 1),
    "neox20b-tp8": ((8, 8, 96, 24), 2),
    "d64-rot10": ((4, 4, 64, 10), 1),
    "santacoder": ((16, 1, 128, 0), 2),
    "starcoder-tp8": ((6, 1, 128, 0), 1),
    "q-only": ((32, 0, 128, 128), 2),
    "items4096": ((128, 64, 128, 128), 16),  # gy = 16 exactly, one pass
    "items4352": ((128, 72, 128, 128), 16),  # past 16 * 256 items: the grid-stride loop
    "gen-items4224": ((192, 80, 96, 24), 16),
}
ROPE_T = (1, 64, 65, 300)


def _rope_cases():
    out = []
    i = 0
    for name, ((H, Hkv, D, rot), gy_small) in ROPE_HEADS.items():
        items = (H + 2 * Hkv) * D // 8
        for T in ROPE_T:
            if items > 4096 and T == 300:
                continue  # (the 65-token case already takes the one-workgroup grid-stride form)
            gy = gy_small if T <= 64 else 1
            for partial in (False, True):
                S = SLABS[i // 2 % len(SLABS)] if partial else 0
                c = dict(op="rope", T=T, H=H, Hkv=Hkv, D=D, rot=rot, dtype=("f16", "bf16")[(i + i // 2) % 2], S=S,
                         bias=partial and i % 3 != 0, slab_pad=(4, 20)[i % 2],
                         form=(gy, int(rot > 0 and rot % 16 != 0), int(gy * 256 < items)))
                c["id"] = f"rope-{name}-T{T}-{c['dtype']}" + (f"-S{S}" if partial else "")
                out.append(c)
                i += 1
    return out


# ---- rope + cache write, prefill (page-wise k / v, q through the per-token kernel) --------------------------------------------
PREFILL_HEADS = {"llama": (8, 8, 128, 128), "neox20b-tp8": (8, 8, 96, 24), "d64-rot10": (4, 4, 64, 10),
                 "santacoder": (16, 1, 128, 0)}
PREFILL_LENS = ([1], [31], [32], [33], [64], [65], [700], [5, 700, 33, 1], [33, 1])


def _prefill_cases():
    out = []
    i = 0
    for name, (H, Hkv, D, rot) in PREFILL_HEADS.items():
        for lens in PREFILL_LENS:
            if name != "llama" and len(lens) == 1 and lens[0] in (31, 64, 700):
                continue  # the single-length edges on one head shape; the others take the mixed batches
            max_len = 96 if lens == [33, 1] else max(lens)  # [33, 1]: a max_len past every length
            c = dict(op="rope_prefill", lens=lens, max_len=max_len, H=H, Hkv=Hkv, D=D, rot=rot,
                     dtype=("f16", "bf16")[i % 2], form=(-(-max_len // 32), int(rot > 0 and rot % 16 != 0)))
            c["id"] = f"prefill-{name}-{'_'.join(map(str, lens))}-m{max_len}-{c['dtype']}"
            out.append(c)
            i += 1
    return out


# ---- argmax + logprob ---------------------------------------------------------------------------------------------------------
def _argmax_cases():
    # (B, V, nseg): nseg = min(16, 256 // B), stepped down while ceil(V / nseg) < 1024
    pts = [(16, 32000, 16), (17, 32000, 15), (32, 32000, 8), (33, 32000, 7), (128, 32000, 2), (129, 32000, 1),
           (256, 32000, 1), (257, 32000, 0),
           (1, 16368, 15), (1, 16369, 16), (2, 2046, 1), (3, 2048, 2), (1, 50257, 16), (2, 152064, 16), (20, 1000, 1)]
    pts += [(1 + k % 3, 1024 * k, k) for k in range(3, 16)]  # every nseg of the split form: ceil(1024 k / k) = 1024
    out = []
    dts = ("f32", "f16", "bf16")
    for i, (B, V, nseg) in enumerate(pts):
        for scratch in (("none", "exact", "short") if nseg > 1 and i < 8 else (("exact",) if nseg > 1 else ("exact", "none"))):
            c = dict(op="argmax", B=B, V=V, nseg=nseg, scratch=scratch, dtype=dts[(i + len(out)) % 3],
                     ld_pad=64 if (i + len(out)) % 2 == 0 else 0)
            c["form"] = (nseg, int(scratch == "exact" and nseg > 1))
            c["id"] = f"argmax-B{B}-V{V}-{c['dtype']}-{scratch}" + ("-ld" if c["ld_pad"] else "")
            out.append(c)
    return out


SAMPLER_CASES = [dict(op="sampler", id="sampler-V32768", V=32768, form=(1,)),
                 dict(op="sampler", id="sampler-V32769", V=32769, form=(0,))]

CASES = _norm_cases() + _rope_cases() + _prefill_cases() + _argmax_cases() + SAMPLER_CASES
NORM_CASES = [c for c in CASES if c["op"] in NORM_KINDS]
ROPE_CASES = [c for c in CASES if c["op"] == "rope"]
PREFILL_CASES = [c for c in CASES if c["op"] == "rope_prefill"]
ARGMAX_CASES = [c for c in CASES if c["op"] == "argmax"]

# ---- launches without a chooser: flat grids with a tail ----------------------------------------------------------------------
ACT_MUL = [(1, 8), (3, 8), (5, 2056), (257, 8), (37, 768)]  # (T, I): T * I / 8 threads over 256-thread workgroups
GELU_N = [8, 2048, 2056, 65544]  # n / 8 threads
EMBED = [  # (E, with pos_table)
    (8, False), (8, True), (2056, False), (2056, True), (768, False)]
DECODE_SLOTS_B = [1, 64, 65, 130]

assert len({c["id"] for c in CASES}) == len(CASES), "duplicate case ids"
