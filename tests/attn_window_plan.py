"""Which launch a tgis_attn_paged_window call takes, asked from the library: tgis_debug_attn_plan_window (csrc/attention.hip, a
host-only export kept out of include/tgis_hip.h like tgis_debug_attn_plan; tests/attn_cases.py is its sibling's helper).
TEST INFRASTRUCTURE shared by tests/test_attn_window_plan_cpu.py and tests/test_attn_window_gpu.py."""
import ctypes

FORMS = ("prefill", "decode", "tree", "window")


def query_window_plan(lib, B, H, Hkv, D, max_q_len, num_splits, window, seqs=()):
    """{"plan": the fields of info[16], "first": [(first visible page, first visible key) per (q_len, ctx) of seqs]}, or None
    when the library refuses the arguments (lib.tgis_last_error() says why)."""
    fn = lib.tgis_debug_attn_plan_window
    fn.restype = ctypes.c_int
    i32p = ctypes.POINTER(ctypes.c_int32)
    fn.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                   ctypes.c_int64, i32p, i32p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    n = len(seqs)
    ctx = (ctypes.c_int32 * max(n, 1))(*[c for _, c in seqs])
    qls = (ctypes.c_int32 * max(n, 1))(*[q for q, _ in seqs])
    info = (ctypes.c_int * 16)()
    first = (ctypes.c_int * max(2 * n, 1))()
    if fn(B, H, Hkv, D, max_q_len, num_splits, window, n, ctx, qls, info, first) != 0:
        return None
    p = {"form": FORMS[info[0]], "nw": info[1], "ch": info[2], "pipe": info[3], "hcb": info[4], "xcd_remap": info[5],
         "grid": tuple(info[6:9]), "lds": info[9], "fused_ok": info[10], "maxs8": info[11], "gp": info[12], "tq": info[13],
         "hc": info[14], "ns": info[15]}
    p["merge"] = "none" if p["ns"] == 1 else "fused" if p["fused_ok"] else "combine8" if p["maxs8"] else "combine"
    return {"plan": p, "first": [(first[2 * i], first[2 * i + 1]) for i in range(n)]}
