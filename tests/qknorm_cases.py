"""Cases of the q/k RMSNorm + rope + cache-write launches (csrc/qk_norm_rope.hip), shared by tests/test_qknorm_plan_cpu.py
(each case lands on the launch form it states, no GPU) and tests/test_qknorm_ops_gpu.py (each case against the fp64
restatement of tests/qknorm_ref.py).  TEST INFRASTRUCTURE.

Per token, form = (kind, idle lanes): a head is the work of 16 lanes, of which 16 - D / 8 hold no chunk (D 64: 8, D 96: 4, D 128:
0), and a block takes 16 heads per pass, so kind is
  "single"   one block per token covers the H + 2 Hkv <= 16 heads in one pass;
  "looped"   T > 64, where the grid is never spread, and more than 16 heads: one block per token, several passes;
  "spread"   T <= 64 and 17 .. 256 heads: ceil(heads / 16) blocks per token, one pass each;
  "strided"  T <= 64 and more than 256 heads: 16 blocks per token that stride over the heads.
Page-wise, form = (pages per sequence in the grid, k store passes): 32 D / 8 (token, chunk) items over 256 threads, 1 pass at
D 64 and 2 at D 96 (the second half full) and D 128.

The shapes are the smallest at which each path can go wrong: a head count that does not fill the last wave ((5, 1): 7 heads),
q only ((16, 0), the launch the page-wise form makes for q), 272 heads ((128, 72): one past the widest grid), T on both sides of
64, slab counts on both sides of the 1 / 2 / 4 / 8 load buckets of sum_slabs8 and one past them (9)."""
import ctypes

EPS = 1e-6


def pt(id, T, H, Hkv, D, rot, dtype, form, S=0, slab_pad=4, bias=False, kv8=False, special=False):
    return dict(id=id, T=T, H=H, Hkv=Hkv, D=D, rot=rot, dtype=dtype, form=form, S=S, slab_pad=slab_pad, bias=bias, kv8=kv8,
                special=special)


# special: row 0's first q head is all zeros (finite output, rstd = eps^-1/2) and, in f16, row 1 has magnitude 3e4 (its squares
# exist only in fp32)
TOKEN_CASES = [
    pt("d128-4x2-T1", 1, 4, 2, 128, 128, "f16", ("single", 0)),
    pt("d128-32x8-T64-rot64-S3-bias", 64, 32, 8, 128, 64, "f16", ("spread", 0), S=3, bias=True),
    pt("d128-128x72-T1-bf16-S1", 1, 128, 72, 128, 128, "bf16", ("strided", 0), S=1, slab_pad=20),
    pt("d96-5x1-T65-special", 65, 5, 1, 96, 96, "f16", ("single", 4), special=True),
    pt("d96-32x8-T64-bf16-rot48-S8-bias", 64, 32, 8, 96, 48, "bf16", ("spread", 4), S=8, bias=True),
    pt("d96-128x72-T64-special", 64, 128, 72, 96, 96, "f16", ("strided", 4), special=True),
    pt("d64-16x0-T300", 300, 16, 0, 64, 64, "f16", ("single", 8)),
    pt("d64-32x8-T1-rot32-S9-bias", 1, 32, 8, 64, 32, "f16", ("spread", 8), S=9, slab_pad=20, bias=True),
    pt("d64-128x72-T1-bf16", 1, 128, 72, 64, 64, "bf16", ("strided", 8)),
    pt("d128-5x1-T300-bf16-rot64-special", 300, 5, 1, 128, 64, "bf16", ("single", 0), special=True),
    pt("d128-32x8-T65-S3", 65, 32, 8, 128, 128, "f16", ("looped", 0), S=3),
    pt("d96-32x8-T65-bf16", 65, 32, 8, 96, 96, "bf16", ("looped", 4)),
    pt("d64-32x8-T300-rot32", 300, 32, 8, 64, 32, "f16", ("looped", 8)),
    pt("d128-16x0-T64", 64, 16, 0, 128, 128, "f16", ("single", 0)),
    pt("d96-4x2-T1-rot48-S1-bias", 1, 4, 2, 96, 48, "f16", ("single", 4), S=1, bias=True),
    pt("d64-5x1-T64-bf16-S3", 64, 5, 1, 64, 64, "bf16", ("single", 8), S=3, slab_pad=20),
    pt("d128-4x2-T300-S9", 300, 4, 2, 128, 128, "f16", ("single", 0), S=9),
    pt("d64-4x2-T65-rot32-S8", 65, 4, 2, 64, 32, "f16", ("single", 8), S=8),
    pt("d128-32x8-T64-kv8", 64, 32, 8, 128, 128, "f16", ("spread", 0), kv8=True),
    pt("d96-5x1-T65-bf16-kv8-S3-bias", 65, 5, 1, 96, 48, "bf16", ("single", 4), S=3, bias=True, kv8=True),
    pt("d64-4x2-T1-kv8", 1, 4, 2, 64, 64, "f16", ("single", 8), kv8=True),
]
KV8_SCALES = (0.5, 2.0)


def pw(id, lens, max_len, H, Hkv, D, rot, dtype, past=None, kv8=False):
    form = (-(-max_len // 32), -(-32 * (D // 8) // 256))
    return dict(id=id, lens=lens, max_len=max_len, H=H, Hkv=Hkv, D=D, rot=rot, dtype=dtype, past=past, kv8=kv8, form=form)


# max_len is past every length once ("-long": blocks whose page lies behind the sequence's end return at once)
PAGE_CASES = [
    pw("d128-len1", [1], 1, 4, 2, 128, 128, "f16"),
    pw("d128-len31-bf16-rot64", [31], 31, 4, 2, 128, 64, "bf16"),
    pw("d96-len32", [32], 32, 5, 1, 96, 96, "f16"),
    pw("d96-len33-bf16-rot48", [33], 33, 5, 1, 96, 48, "bf16"),
    pw("d64-len65", [65], 65, 4, 2, 64, 64, "f16"),
    pw("d64-len33-rot32-long", [33], 100, 4, 2, 64, 32, "f16"),
    pw("d128-batch", [5, 700, 33, 1], 700, 4, 2, 128, 128, "f16"),
    pw("d128-batch-past-long", [5, 700, 33, 1], 740, 4, 2, 128, 128, "f16", past=[0, 32, 64, 32]),
    pw("d96-batch-past-bf16", [5, 70, 33, 1], 70, 5, 1, 96, 96, "bf16", past=[64, 0, 32, 0]),
    pw("d64-batch-past-bf16", [33, 1, 65], 65, 4, 2, 64, 64, "bf16", past=[32, 64, 0]),
    pw("d128-batch-kv8", [5, 70, 33, 1], 70, 4, 2, 128, 128, "f16", kv8=True),
    pw("d96-past-kv8-bf16-rot48", [33, 31], 33, 5, 1, 96, 48, "bf16", past=[32, 0], kv8=True),
]


def query(lib, op, *args):
    """tgis_debug_qknorm_plan (host-only, not in tgis_hip.h): the info words of op 0 (per token) or 1 (page-wise)."""
    fn = lib.tgis_debug_qknorm_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    a = (ctypes.c_int64 * 4)(*args)
    info = (ctypes.c_int64 * 4)()
    rc = fn(op, a, info)
    assert rc == 0, lib.tgis_last_error().decode()
    return list(info)


def token_form(info):
    gy, strided, _heads, idle = info
    kind = ("strided" if strided else "spread") if gy > 1 else ("looped" if strided else "single")
    return (kind, idle)


def page_form(info):
    return (info[0], info[2])


def case_form(c, lib):
    if "lens" in c:
        return page_form(query(lib, 1, c["max_len"], c["D"]))
    return token_form(query(lib, 0, c["T"], c["H"], c["Hkv"], c["D"]))
