"""Which launch a paged-attention call takes, asked from the library: tgis_debug_attn_plan (csrc/attention.hip, a host-only
export kept out of include/tgis_hip.h like tgis_debug_gemm_plan) reports the plan of csrc/attention_plan.h without a launch.

tests/test_attn_plan_cpu.py restates the plan and checks, without a GPU, that every variant the default planner reaches on a
fixed grid of shapes is run by a case of the GPU files; the GPU files ask here which form a case takes.

A variant key is the tuple VARIANT_FIELDS:
  form       prefill (attention_prefill.hip) | decode | tree (attn_paged_kernel, TREE = false | true)
  nw         waves per block
  ch         16-head chunks per block
  pipe       two pages of K / V loads in flight per wave
  xcd_remap  the chunk blocks of a (sequence, split, kv head) group run on one XCD
  merge      none (one split) | fused (the last block of a group merges in the launch) | combine8 | combine
             (attn_combine_kernel<MAXS = 8> up to 8 splits, <MAXS = 0> beyond)
i.e. the kernel template instance(s) a call runs and the launch-uniform branches that change which blocks do what.
"""
import ctypes

FORMS = ("prefill", "decode", "tree")
VARIANT_FIELDS = ("form", "nw", "ch", "pipe", "xcd_remap", "merge")


def query_plan(lib, B, H, Hkv, D, max_q_len, num_splits=1, tree=False):
    """The raw info[16] of tgis_debug_attn_plan (see attention.hip), or None when the library refuses the arguments."""
    fn = lib.tgis_debug_attn_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                   ctypes.POINTER(ctypes.c_int)]
    info = (ctypes.c_int * 16)()
    rc = fn(B, H, Hkv, D, max_q_len, num_splits, int(tree), info)
    return list(info) if rc == 0 else None


def plan_fields(info):
    """info[16] -> dict of the plan."""
    p = {"form": FORMS[info[0]], "nw": info[1], "ch": info[2], "pipe": info[3], "hcb": info[4], "xcd_remap": info[5],
         "grid": tuple(info[6:9]), "lds": info[9], "fused_ok": info[10], "maxs8": info[11], "gp": info[12], "tq": info[13],
         "hc": info[14], "ns": info[15]}
    p["merge"] = "none" if p["ns"] == 1 else "fused" if p["fused_ok"] else "combine8" if p["maxs8"] else "combine"
    return p


def variant_key(info):
    p = plan_fields(info)
    return tuple(p[f] for f in VARIANT_FIELDS)


def case_key(lib, H, Hkv, D, seqs, num_splits=1, tree=False):
    """The variant key of one call over sequences [(q_len, ctx, ...)], as the GPU files make it."""
    info = query_plan(lib, len(seqs), H, Hkv, D, max(s[0] for s in seqs), num_splits, tree)
    assert info is not None, f"tgis_debug_attn_plan refused {(H, Hkv, D, seqs, num_splits, tree)}: {lib.tgis_last_error().decode()}"
    return variant_key(info)


def key_str(key):
    return ",".join(f"{f}={v}" for f, v in zip(VARIANT_FIELDS, key))
