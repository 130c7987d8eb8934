"""ctypes binding of libtgis_hip.so (include/tgis_hip.h) for torch tensors on an MI355X.

This is the drop-in boundary #5 of SURVEY.md §8(b): where the reference imports CUDA extension modules
(`flash_attn_2_cuda`, `dropout_layer_norm`, `rotary_emb`, `exllamav2_kernels`; utils/flash_attn.py:23,
utils/layers.py:361,403-404, utils/gptq/exllamav2.py:7) this module loads one C-ABI shared library and
passes raw device pointers, sizes and the current HIP stream.  There is no CPU or eager-torch fallback:
if the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.getenv("TGIS_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libtgis_hip.so")

F16, BF16 = 0, 1
KV_PAGE_TOKENS = 32

OP_GPTQ_GEMM, OP_ATTN, OP_DENSE_GEMM, OP_NORM, OP_ROPE_KV, OP_ACT, OP_SAMPLE = range(7)

_c_i64 = ctypes.c_int64
_c_int = ctypes.c_int
_c_f = ctypes.c_float
_vp = ctypes.c_void_p
_KV8_ARGS = [_c_int, _c_f, _c_f]  # kv_dtype, k_scale, v_scale appended by the *_kv8 entry points


# name -> (restype, argtypes); must list every symbol declared in include/tgis_hip.h
SIGNATURES = {
    "tgis_version": (ctypes.c_char_p, []),
    "tgis_arch": (ctypes.c_char_p, []),
    "tgis_clear_error": (None, []),
    "tgis_last_error": (ctypes.c_char_p, []),
    "tgis_device_info": (_c_int, [_c_int, ctypes.POINTER(_c_int), ctypes.POINTER(_c_i64), ctypes.c_char_p, _c_int]),
    "tgis_timing_enable": (_c_int, [_c_int]),
    "tgis_timing_reset": (_c_int, []),
    "tgis_timing_read": (_c_int, [_c_int, ctypes.POINTER(_c_i64), ctypes.POINTER(ctypes.c_double)]),
    "tgis_gptq_prepared_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_gptq_prepare": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "tgis_gptq_gemm_fused_rows": (_c_i64, [_c_i64, _c_i64, _c_int, _c_int]),
    "tgis_gptq_gemm_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_gptq_gemm_f16": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                    _c_int, _vp, _c_i64, _vp]),
    "tgis_gptq_gemm_partial_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_gptq_gemm_f16_partial": (_c_int, [_vp, _c_i64, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp, _c_i64,
                                            ctypes.POINTER(_c_int), ctypes.POINTER(_c_i64), _vp]),
    "tgis_gptq_dequant_f16": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _c_int, _vp]),
    "tgis_gptq8_prepared_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_gptq8_prepare": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "tgis_gptq8_gemm_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_gptq8_gemm_f16": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64,
                                     _c_int, _vp, _c_i64, _vp]),
    "tgis_gptq8_dequant_f16": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp]),
    "tgis_dense_gemm_rope": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64, _c_i64,
                                      _c_i64, _c_i64, _c_i64, _c_int, _vp]),
    "tgis_dense_gemm_rope_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64,
                                          _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp] + _KV8_ARGS),
    "tgis_gptq_rope_ok": (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_i64]),
    "tgis_gptq_fragments_ok": (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int]),
    "tgis_dense_rope_ok": (_c_int, [_c_i64, _c_i64, _c_i64, _c_i64]),
    "tgis_gptq_gemm_rope_f16": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64,
                                         _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _vp]),
    "tgis_gptq_gemm_rope_f16_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64,
                                             _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _vp] + _KV8_ARGS),
    "tgis_dense_prepared_bytes": (_c_i64, [_c_i64, _c_i64]),
    "tgis_dense_prepare": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp]),
    "tgis_dense_gemm_workspace_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_dense_gemm": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int,
                                 _c_int, _vp, _c_i64, _vp]),
    "tgis_dense_gemm_partial_bytes": (_c_i64, [_c_i64, _c_i64, _c_i64]),
    "tgis_dense_gemm_partial": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _vp, _c_i64,
                                         ctypes.POINTER(_c_int), ctypes.POINTER(_c_i64), _vp]),
    "tgis_moe_route": (_c_int, [_vp, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tgis_moe_gemm_up": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int,
                                  _c_int, _vp]),
    "tgis_moe_gemm_down_bytes": (_c_i64, [_c_i64, _c_i64, _c_int, _c_int]),
    "tgis_moe_gemm_down": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                    _c_int, _vp, _c_i64, _vp, _c_i64, _vp]),
    "tgis_moe_gptq_gemm_up": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_i64, _c_int,
                                       _c_int, _c_int, _vp]),
    "tgis_moe_gptq_gemm_down": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _c_int,
                                         _c_int, _c_int, _vp, _c_i64, _vp, _c_i64, _vp]),
    "tgis_lora_a_bytes": (_c_i64, [_c_i64, _c_int, _c_int]),
    "tgis_lora_b_bytes": (_c_i64, [_c_i64, _c_int]),
    "tgis_lora_group": (_c_int, [_vp, _c_i64, _c_int, _vp, _vp, _vp, _vp]),
    "tgis_lora_shrink": (_c_int, [_vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int, _c_int,
                                  _c_int, _vp]),
    "tgis_lora_expand": (_c_int, [_vp, _vp, _c_i64, _vp, _vp, _vp, _vp, ctypes.POINTER(_c_i64), _vp, _c_i64, _c_i64, _c_i64,
                                  _c_int, _c_int, _c_int, _c_int, _vp]),
    "tgis_rmsnorm_residual":(_c_int, [_vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i64, _c_f, _c_int, _vp]),
    "tgis_rmsnorm_residual_partial": (_c_int, [_vp, _c_int, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_i64, _c_f,
                                               _c_int, _vp]),
    "tgis_layernorm_residual": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_f, _c_int, _vp]),
    "tgis_layernorm_residual_partial": (_c_int, [_vp, _c_int, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64,
                                                 _c_f, _c_int, _vp]),
    "tgis_layernorm2_residual": (_c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64,
                                          _c_f, _c_int, _vp]),
    "tgis_layernorm2_residual_partial": (_c_int, [_vp, _vp, _vp, _c_int, _c_i64, _vp, _vp, _vp, _c_int, _c_i64, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_f, _c_int, _vp]),
    "tgis_rope_kv_write": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int,
                                    _c_int, _c_int, _vp]),
    "tgis_rope_kv_write_partial": (_c_int, [_vp, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64,
                                            _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "tgis_rope_kv_write_prefill": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64, _c_i64,
                                            _c_int, _c_int, _c_int, _c_int, _c_int, _vp]),
    "tgis_rope_kv_write_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _c_int, _c_int, _c_int,
                                        _c_int, _c_int, _vp] + _KV8_ARGS),
    "tgis_rope_kv_write_partial_kv8": (_c_int, [_vp, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64,
                                                _c_int, _c_int, _c_int, _c_int, _c_int, _vp] + _KV8_ARGS),
    "tgis_rope_kv_write_prefill_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64,
                                                _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp] + _KV8_ARGS),
    "tgis_rope_kv_write_prefill_at": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64,
                                               _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp, _vp]),
    "tgis_rope_kv_write_prefill_at_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64,
                                                   _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int, _vp] + _KV8_ARGS + [_vp]),
    "tgis_rope_kv_write_qknorm": (_c_int, [_vp, _c_i64, _vp, _c_int, _c_i64, _vp, _vp, _vp, _c_f, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int] + _KV8_ARGS + [_vp]),
    "tgis_rope_kv_write_prefill_qknorm": (_c_int, [_vp, _c_i64, _vp, _vp, _c_f, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp,
                                                   _c_i64, _c_i64, _c_i64, _c_int, _c_int, _c_int, _c_int, _c_int]
                                          + _KV8_ARGS + [_vp]),
    "tgis_attn_num_splits": (_c_int, [_c_i64, _c_int, _c_int, _c_i64, _c_i64]),
    "tgis_attn_num_splits_q": (_c_int, [_c_i64, _c_int, _c_int, _c_i64, _c_i64]),
    "tgis_attn_workspace_bytes": (_c_i64, [_c_i64, _c_int, _c_int, _c_int, _c_int]),
    "tgis_attn_paged": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int,
                                 _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_int, _vp, _c_i64, _vp]),
    "tgis_attn_paged_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int,
                                     _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_int, _vp, _c_i64, _vp] + _KV8_ARGS),
    "tgis_attn_paged_tree": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int,
                                      _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_int, _vp, _c_i64, _vp, _vp]),
    "tgis_attn_paged_tree_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int,
                                          _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_int, _vp, _c_i64, _vp] + _KV8_ARGS + [_vp]),
    "tgis_attn_paged_window": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int,
                                        _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_int, _vp, _c_i64, _vp, _c_i64]),
    "tgis_attn_paged_window_kv8": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _c_int,
                                            _c_int, _c_i64, _c_i64, _c_f, _c_int, _c_int, _vp, _c_i64, _vp] + _KV8_ARGS
                                   + [_c_i64]),
    "tgis_kv_absmax": (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _c_int, _c_int, _c_int, _vp, _vp]),
    "tgis_act_mul": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_int, _c_int, _vp]),
    "tgis_gelu": (_c_int, [_vp, _vp, _c_i64, _c_int, _c_int, _vp]),
    "tgis_embedding": (_c_int, [_vp, _vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _c_int, _vp]),
    "tgis_decode_slots": (_c_int, [_vp, _vp, _c_i64, _vp, _vp, _c_i64, _vp]),
    "tgis_decode_advance": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_spec_stage": (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_spec_accept": (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_spec_accept_sampled": (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp,
                                          _c_i64, _vp]),
    "tgis_spec_propose": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_spec_tree_stage": (_c_int, [_vp, _vp, _vp, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_spec_tree_accept": (_c_int, [_vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp,
                                       _c_i64, _vp]),
    "tgis_spec_tree_commit": (_c_int, [_vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _c_i64,
                                       _c_int, _c_int, _c_int, _vp]),
    "tgis_spec_propose_multi": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_spec_mlp_input": (_c_int, [_vp, _vp, _c_i64, _vp, _vp, _c_i64, _c_i64, _c_int, _c_f, _c_int, _vp]),
    "tgis_spec_mlp_state": (_c_int, [_vp, _vp, _vp, _c_i64, _vp, _vp, _c_f, _c_f, _vp, _c_i64, _c_i64, _c_int, _vp]),
    "tgis_spec_mlp_drafts": (_c_int, [_vp, _c_i64, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_argmax_logprob": (_c_int, [_vp, _c_i64, _c_i64, _c_i64, _c_int, _c_int, _vp, _vp, _vp, _c_i64, _vp]),
    "tgis_argmax_scratch_bytes": (_c_i64, [_c_i64]),
    "tgis_warp_sample": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64,
                                  _c_i64, _c_i64, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tgis_warp_sample_verify": (_c_int, [_vp, _c_i64, _vp, _c_i64, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                         _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


class TgisHipError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> ctypes.CDLL:
    """dlopen the C-ABI library and bind every declared symbol.  Needs no GPU (no compute is run)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise TgisHipError(
            f"{p} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')"
        )
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        msg = load_library().tgis_last_error().decode()
        raise TgisHipError(f"{what} failed (code {rc}): {msg}")


# KV cache element codes of the *_kv8 entry points (TGIS_KV_* in tgis_hip.h)
KV_MODEL, KV_FP8_E4M3 = 0, 1
KV8_DTYPES = (torch.uint8, torch.float8_e4m3fn)  # a one-byte pool holds e4m3 codes; torch may see them as either


def kv_is8(pool: Optional[torch.Tensor]) -> bool:
    """Whether a KV pool holds one-byte (e4m3) codes: its writers and readers then take the *_kv8 entry points."""
    return pool is not None and pool.dtype in KV8_DTYPES


def _call_kv(name: str, args: tuple, k_pool, v_pool, kv_scales, tail: tuple = ()) -> None:
    """One launch of the entry point `name` that writes or reads the KV cache: `name` itself on 16-bit pools, its `_kv8`
    twin with (kv_dtype, k_scale, v_scale) appended on one-byte pools; `tail` follows either way."""
    if kv_is8(k_pool):
        assert kv_is8(v_pool) and k_pool.dtype == v_pool.dtype, "k and v pools must both hold e4m3 codes"
        k_scale, v_scale = (1.0, 1.0) if kv_scales is None else kv_scales
        name += "_kv8"
        args += (KV_FP8_E4M3, float(k_scale), float(v_scale))
    _check(getattr(load_library(), name)(*(args + tail)), name)


def _kv_args(k_pool, v_pool, kv_scales) -> tuple:
    """(kv_dtype, k_scale, v_scale) of an entry point that takes the cache element in its one signature."""
    if not kv_is8(k_pool):
        return (KV_MODEL, 1.0, 1.0)
    assert kv_is8(v_pool) and k_pool.dtype == v_pool.dtype, "k and v pools must both hold e4m3 codes"
    k_scale, v_scale = (1.0, 1.0) if kv_scales is None else kv_scales
    return (KV_FP8_E4M3, float(k_scale), float(v_scale))


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float16:
        return F16
    if dt == torch.bfloat16:
        return BF16
    raise TgisHipError(f"unsupported dtype {dt} (float16 / bfloat16 only)")


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise TgisHipError("tensor is not on the GPU: the HIP path has no CPU fallback")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream.  The raw getter skips the Stream object that
    torch.cuda.current_stream() builds (a third of the host time of an eager decode step went there)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def version() -> str:
    return load_library().tgis_version().decode()


def timing_enable(on: bool):
    _check(load_library().tgis_timing_enable(int(on)), "tgis_timing_enable")


def timing_reset():
    _check(load_library().tgis_timing_reset(), "tgis_timing_reset")


def timing_read(op: int):
    c = _c_i64()
    ms = ctypes.c_double()
    _check(load_library().tgis_timing_read(op, ctypes.byref(c), ctypes.byref(ms)), "tgis_timing_read")
    return c.value, ms.value


# ---- workspaces ---------------------------------------------------------------------------------
class Workspace:
    """Zero-initialised scratch for split-K slabs / arrival counters and attention splits.

    One per stream of work.  The first 4096 bytes hold the arrival counters that the GEMM kernels leave
    at zero after every call, so the buffer is zeroed exactly once, at allocation."""

    def __init__(self, nbytes: int, device):
        self.buf = torch.zeros(max(int(nbytes), 4096), dtype=torch.uint8, device=device)
        # Buffers replaced by larger ones stay allocated: HIP graphs captured while they were current hold their raw
        # pointers (slabs, arrival counters, attention splits).  Each buffer's counters are only ever touched by the
        # launches that captured it, so old graphs and new launches never share state.
        self.retired = []

    def ensure(self, nbytes: int):
        if self.buf.numel() < nbytes:
            self.retired.append(self.buf)
            self.buf = torch.zeros(max(int(nbytes), 2 * self.buf.numel()), dtype=torch.uint8, device=self.buf.device)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    @property
    def nbytes(self):
        return self.buf.numel()


# ---- activations in MFMA-fragment order (TGIS_LD_FRAGMENTS) ------------------------------------------------------------
LD_FRAGMENTS = -32


class FragAct:
    """A [M <= 64, K] f16 activation stored in fragment order (include/tgis_hip.h, TGIS_LD_FRAGMENTS): what the decode
    step's norm / attention / SiLU epilogue hand to the int4 GEMM behind them.  `buf` holds ceil(M / 32) * 32 * K elements."""

    def __init__(self, buf: torch.Tensor, M: int, K: int):
        assert 1 <= M <= 64 and K % 64 == 0 and buf.dtype == torch.float16 and buf.numel() == (M + 31) // 32 * 32 * K
        self.buf, self.M, self.K = buf, M, K
        self.dtype, self.device = buf.dtype, buf.device

    @property
    def shape(self):
        return (self.M, self.K)

    @staticmethod
    def empty(M: int, K: int, device) -> "FragAct":
        return FragAct(torch.empty((M + 31) // 32 * 32 * K, dtype=torch.float16, device=device), M, K)

    @staticmethod
    def from_rows(x: torch.Tensor) -> "FragAct":
        """Row-major [M, K] -> fragment order (torch ops; tests and cold paths only)."""
        M, K = x.shape
        rb = (M + 31) // 32
        full = torch.zeros((rb * 32, K), dtype=x.dtype, device=x.device)
        full[:M] = x
        # (row block, m, step, half, i, e) -> [row block][step][i][half][m][e]
        f = full.view(rb, 32, K // 64, 2, 4, 8).permute(0, 2, 4, 3, 1, 5).contiguous().view(-1)
        return FragAct(f, M, K)

    def to_rows(self) -> torch.Tensor:
        K, rb = self.K, (self.M + 31) // 32
        return self.buf.view(rb, K // 64, 4, 2, 32, 8).permute(0, 4, 1, 3, 2, 5).reshape(rb * 32, K)[:self.M].contiguous()


def _asked_once(w, key, ask):
    """A host-only answer of the library about the prepared weight `w`, asked on first use and kept on the weight: an eager
    decode step (tensor parallelism without graphs) would otherwise make these ctypes calls for every layer."""
    got = w.answers.get(key)
    if got is None:
        got = w.answers[key] = ask()
    return got


def gptq_fragments_ok(M: int, w: "GptqWeight", act: int = 0) -> bool:
    """Should an M-row activation reach this int4 GEMM in fragment order (tgis_gptq_fragments_ok)?  act 3 = the rope image."""
    return _asked_once(w, ("frag_ok", M, act), lambda: bool(
        load_library().tgis_gptq_fragments_ok(M, w.K, w.N, w.groups, int(w.perm is not None), act)))


# ---- GPTQ ------------------------------------------------------------------------------------------
class _GptqImage:
    """What the prepared 4- and 8-bit GPTQ matrices share: the repack launch, the activation permutation and its three
    sources.  g_idx is None, a [K] tensor (act-order when not trivial: the library then fills `perm`), or ("perm", gather
    index [K] with -1 = zero, activation columns) for rows that are already in image order (act-order row shards)."""

    def _prepare(self, bits: int, qweight, qzeros, scales, g_idx, flags: int):
        lib = load_library()
        entry = "tgis_gptq_" if bits == 4 else "tgis_gptq8_"
        self.K = qweight.shape[0] * (32 // bits)
        self.N = qweight.shape[1]
        self.groups = qzeros.shape[0]
        self.answers = {}  # see _asked_once
        dev = qweight.device
        self.image = torch.empty(getattr(lib, entry + "prepared_bytes")(self.K, self.N, self.groups), dtype=torch.uint8,
                                 device=dev)
        qweight = qweight.contiguous()
        qzeros = qzeros.contiguous()
        scales = scales.to(torch.float16).contiguous()
        self.perm = None
        self.in_features = self.K  # columns of the activation (differs from K only for padded act-order row shards)
        gi = perm_buf = explicit = None
        if isinstance(g_idx, tuple):
            _, explicit, self.in_features = g_idx
            assert explicit.numel() == self.K
        elif g_idx is not None:
            assert g_idx.numel() == self.K
            gi = g_idx.to("cpu", torch.int32).contiguous()
            perm_buf = torch.empty(self.K, dtype=torch.int32, device=dev)
        _check(
            getattr(lib, entry + "prepare")(
                _ptr(qweight), _ptr(qzeros), _ptr(scales), gi.data_ptr() if gi is not None else None, _ptr(perm_buf),
                self.K, self.N, self.groups, flags, _ptr(self.image), _stream()), entry + "prepare")
        if gi is not None:
            gs = self.K // self.groups
            if not bool((gi == (torch.arange(self.K, dtype=torch.int32) // gs)).all()):
                self.perm = perm_buf
        if explicit is not None:
            self.perm = explicit.to(dev, torch.int32).contiguous()
        torch.cuda.current_stream().synchronize()  # qweight/qzeros/scales may be freed by the caller


class GptqWeight(_GptqImage):
    """Prepared (repacked) GPTQ matrix; owner of the device image. Mirrors the q_handle of
    Ex4bitLinearV2.post_init (utils/gptq/exllamav2.py:124-137)."""

    def __init__(self, qweight, qzeros, scales, g_idx, bits: int, groupsize: int, gate_up: bool = False,
                 rope: Optional[tuple] = None):
        """rope = (D, rotated heads): the image of a fused qkv projection for gptq_gemm_rope (TGIS_GPTQ_ROPE_IMAGE)."""
        self.flags = 1 if gate_up else 0
        if rope is not None:
            assert not gate_up
            self.flags = 2 | (int(rope[0]) << 8) | (int(rope[1]) << 20)
        self.partial_plan = {}  # pass count -> (slab bytes, S, ld) of the deferred-reduce form, filled on first use
        if bits != 4:
            raise TgisHipError(f"GPTQ is supported at 4 and 8 bits, not {bits}; this is the 4-bit image (exllamav2.py:105), "
                               "8 bits take Gptq8Weight")
        if qweight.shape[0] * 8 % 32 or qweight.shape[1] % 32:
            raise TgisHipError("GPTQ height and width must be multiples of 32 (exllamav2.py:118-119)")
        self._prepare(4, qweight, qzeros, scales, g_idx, self.flags)

    def workspace_bytes(self, M: int) -> int:
        return load_library().tgis_gptq_gemm_workspace_bytes(M, self.K, self.N)

    def fused_rows(self, act: int = 0) -> int:
        """Largest M the fused kernels of tgis_gptq_gemm_f16 should be given (beyond: dequantise + library GEMM)."""
        return _asked_once(self, ("fused_rows", act), lambda: load_library().tgis_gptq_gemm_fused_rows(
            self.K, self.groups, int(self.perm is not None), act))


def gptq_gemm(x, w: GptqWeight, ws: Workspace, bias=None, act: int = 0, out=None, out_frag: bool = False):
    """act 0: out[M,N] = x @ dequant(W) (+bias); act 1: x is [M,2K], silu(x[:, :K]) * x[:, K:] is the operand;
    act 2 (weight prepared with gate_up=True): out[M,N/2] = silu(gate) * up.
    act 4 / 5 (M <= w.fused_rows(4) = 256, row-major x): out = gelu(x @ dequant(W) + bias), exact erf form / tanh
    approximation, applied where the GEMM finishes its output — the bits of act 0 followed by `gelu`.
    x may be a FragAct (decode, M <= 64); with act 2 the result may then leave as a FragAct too (out_frag)."""
    assert act != 2 or w.flags & 1, "act=2 needs a weight prepared with gate_up=True"
    if act in (4, 5):
        assert not isinstance(x, FragAct), "act 4 / 5 (GELU) take a row-major activation"
        if w.flags & 1:  # the library call does not carry the image's column order: refused here, in its name
            raise TgisHipError("tgis_gptq_gemm_f16: act 4 / 5 (GELU) on a gate|up image (its columns are interleaved for "
                               "act 2)")
    if isinstance(x, FragAct):
        assert x.K == w.K and act in (0, 2) and w.perm is None
        M, xp, ldx = x.M, _ptr(x.buf), LD_FRAGMENTS
    else:
        assert not out_frag, "a fragment-order output needs a fragment-order activation"
        assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
        M, xp, ldx = x.shape[0], _ptr(x), x.stride(0)
        assert x.shape[1] == (2 * w.in_features if act == 1 else w.in_features), (x.shape, w.in_features, act)
        assert act != 1 or w.in_features == w.K
    if out_frag:
        assert act == 2 and out is None
        res = FragAct.empty(M, w.N // 2, x.device)
        optr, ldo = _ptr(res.buf), LD_FRAGMENTS
    else:
        res = out if out is not None else torch.empty((M, w.N // 2 if act == 2 else w.N), dtype=torch.float16,
                                                      device=x.device)
        optr, ldo = _ptr(res), res.stride(0)
    ws.ensure(w.workspace_bytes(M))
    _check(
        load_library().tgis_gptq_gemm_f16(xp, ldx, _ptr(w.image), _ptr(bias), _ptr(w.perm), optr, ldo, M, w.K, w.N,
                                          w.groups, act, ws.ptr, ws.nbytes, _stream()), "tgis_gptq_gemm_f16")
    return res


class Partial:
    """fp32 split-K partial sums [ceil(M/32), S, 32, ld] of a GEMM whose reduce is deferred to the consumer kernel
    (rmsnorm_residual / rope_kv_write accept it in place of the f16 activation)."""

    def __init__(self, slabs: torch.Tensor, S: int, ld: int, M: int, N: int, bias):
        self.slabs, self.S, self.ld, self.M, self.N, self.bias = slabs, S, ld, M, N, bias
        self.dtype = torch.float16
        self.device = slabs.device

    @property
    def shape(self):
        return (self.M, self.N)


PARTIAL_MAX_M = 256  # rows up to which a GEMM may leave its split-K sum to the consumer kernel


def gptq_gemm_partial(x: torch.Tensor, w: GptqWeight, bias=None, act: int = 0) -> Partial:
    """Launch the GEMM but leave the split-K reduce (and bias) to the consumer.  Slabs are stored in 32-row units:
    [ceil(M/32)][S][32][ld]."""
    lib = load_library()
    if isinstance(x, FragAct):  # decode, <= 64 rows: the fragment-order kernel and ITS split plan
        assert x.K == w.K and act == 0 and w.perm is None
        # the split plan of the fragment-order kernel depends on the row class (plan_wide: <= 32 rows / 33 - 64 rows)
        M, key, xp, ldx = x.M, ("frag", x.M > 32), _ptr(x.buf), LD_FRAGMENTS
    else:
        assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] <= PARTIAL_MAX_M
        M = x.shape[0]
        key, xp, ldx = ((M + 63) // 64 if M > 32 else 0), _ptr(x), x.stride(0)  # plan depends on M through its pass count
    plan = w.partial_plan.get(key)  # (slab bytes, S, ld): asked from the library once per weight and pass count
    if plan is None:
        nbytes, S, ld = lib.tgis_gptq_gemm_partial_bytes(M, w.K, w.N), _c_int(), _c_i64()
        ask = (ctypes.byref(S), ctypes.byref(ld))
    else:
        nbytes, ask = plan[0], (None, None)
    slabs = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    _check(
        lib.tgis_gptq_gemm_f16_partial(xp, ldx, _ptr(w.image), _ptr(w.perm), M, w.K, w.N, w.groups, act, _ptr(slabs),
                                       nbytes, *ask, _stream()), "tgis_gptq_gemm_f16_partial")
    if plan is None:
        plan = w.partial_plan[key] = (nbytes, S.value, ld.value)
    return Partial(slabs, plan[1], plan[2], M, w.N, bias)


def gptq_rope_ok(M: int, w: GptqWeight, D: int) -> bool:
    return bool(load_library().tgis_gptq_rope_ok(M, w.K, w.N, w.groups, int(w.perm is not None), D))


def rope_gemm_ok(M: int, w, D: int) -> bool:
    """Whether the fused qkv + rotary + cache-write launch should serve M rows of this weight (int4 or dense image)."""
    if isinstance(w, GptqWeight):
        return _asked_once(w, ("rope_ok", M), lambda: gptq_rope_ok(M, w, D))
    return _asked_once(w, ("rope_ok", M), lambda: bool(load_library().tgis_dense_rope_ok(M, w.K, w.N, D)))


def gptq_gemm_rope(x: torch.Tensor, w: GptqWeight, bias, cos, sin, positions, slots, k_pool, v_pool, H: int, Hkv: int,
                   D: int, out=None, kv_scales=(1.0, 1.0)) -> torch.Tensor:
    """qkv projection + rotary embedding + cache write in one launch (decode, M <= 64; `w` is the rope image of the fused
    qkv weight).  Returns a [M, (H + 2 Hkv) D] tensor whose first H D columns hold the rotated q (the k / v columns are not
    written: they went straight into their cache pages).  One-byte pools (kv_is8) take tgis_gptq_gemm_rope_f16_kv8 with
    kv_scales = (k_scale, v_scale)."""
    if isinstance(x, FragAct):
        assert x.K == w.K
        M, xp, ldx = x.M, _ptr(x.buf), LD_FRAGMENTS
    else:
        assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1 and x.shape[1] == w.K
        M, xp, ldx = x.shape[0], _ptr(x), x.stride(0)
    assert w.flags & 2 and w.N == (H + 2 * Hkv) * D
    assert positions.dtype == torch.int32 and slots.dtype == torch.int32 and cos.dtype == torch.float16
    assert cos.shape[1] * 2 == D, "the fused epilogue covers the full rotary span only"
    if out is None:
        out = torch.empty((M, w.N), dtype=torch.float16, device=x.device)
    args = (xp, ldx, _ptr(w.image), _ptr(bias), _ptr(positions), _ptr(slots), _ptr(cos), _ptr(sin), _ptr(out),
            out.stride(0), _ptr(k_pool), _ptr(v_pool), M, w.K, w.N, w.groups, H, Hkv, D, _stream())
    _call_kv("tgis_gptq_gemm_rope_f16", args, k_pool, v_pool, kv_scales)
    return out


def gptq_dequant(w: GptqWeight, out=None) -> torch.Tensor:
    """Dense f16 [K,N] (rows in the prepared order: permuted by w.perm for act-order matrices)."""
    if out is None:
        out = torch.empty((w.K, w.N), dtype=torch.float16, device=w.image.device)
    assert out.shape == (w.K, w.N) and out.dtype == torch.float16 and out.is_contiguous()
    _check(load_library().tgis_gptq_dequant_f16(_ptr(w.image), _ptr(out), w.K, w.N, w.groups, w.flags, _stream()),
           "tgis_gptq_dequant_f16")
    return out


# ---- GPTQ, 8 bits --------------------------------------------------------------------------------------
GPTQ8_MAX_M = 64  # rows the fused 8-bit kernel serves (above: gptq8_dequant + a library GEMM)


class Gptq8Weight(_GptqImage):
    """Prepared 8-bit GPTQ matrix (csrc/gptq8_gemm_body.h); what QuantLinear holds for bits = 8
    (utils/gptq/quant_linear.py:259).  Takes the g_idx forms of GptqWeight."""

    def __init__(self, qweight, qzeros, scales, g_idx, bits: int, groupsize: int):
        if bits != 8:
            raise TgisHipError(f"Gptq8Weight is the 8-bit image, not {bits} bits")
        self._prepare(8, qweight, qzeros, scales, g_idx, 0)

    def workspace_bytes(self, M: int) -> int:
        return load_library().tgis_gptq8_gemm_workspace_bytes(M, self.K, self.N)


def gptq8_gemm(x, w: Gptq8Weight, ws: Workspace, bias=None, act: int = 0, out=None):
    """out[M <= 64, N] = x @ dequant(W) (+ bias); act 1: x is [M, 2K] and silu(x[:, :K]) * x[:, K:] is the operand."""
    assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
    M = x.shape[0]
    assert x.shape[1] == (2 * w.in_features if act == 1 else w.in_features), (x.shape, w.in_features, act)
    assert act != 1 or w.in_features == w.K
    if out is None:
        out = torch.empty((M, w.N), dtype=torch.float16, device=x.device)
    ws.ensure(w.workspace_bytes(M))
    _check(
        load_library().tgis_gptq8_gemm_f16(_ptr(x), x.stride(0), _ptr(w.image), _ptr(bias), _ptr(w.perm), _ptr(out),
                                           out.stride(0), M, w.K, w.N, w.groups, act, ws.ptr, ws.nbytes, _stream()),
        "tgis_gptq8_gemm_f16")
    return out


def gptq8_dequant(w: Gptq8Weight, out=None) -> torch.Tensor:
    """Dense f16 [K,N] (rows in the prepared order: permuted by w.perm for act-order matrices)."""
    if out is None:
        out = torch.empty((w.K, w.N), dtype=torch.float16, device=w.image.device)
    assert out.shape == (w.K, w.N) and out.dtype == torch.float16 and out.is_contiguous()
    _check(load_library().tgis_gptq8_dequant_f16(_ptr(w.image), _ptr(out), w.K, w.N, w.groups, _stream()),
           "tgis_gptq8_dequant_f16")
    return out


# ---- dense ------------------------------------------------------------------------------------------
class DenseWeight:
    """torch-Linear weight [N,K] repacked into MFMA tile order.  gate_up=True: the weight is the Llama MLP's
    [gate | up] and the image interleaves the pairs for the SiLU*up epilogue (dense_gemm(act=2))."""

    def __init__(self, weight: torch.Tensor, gate_up: bool = False, rope: Optional[tuple] = None):
        lib = load_library()
        assert weight.dim() == 2
        self.N, self.K = weight.shape
        self.dtype = weight.dtype
        self.answers = {}  # see _asked_once
        self.flags = 1 if gate_up else 0
        if rope is not None:  # (D, rotated heads): the image of a fused qkv projection for dense_gemm_rope
            assert not gate_up
            self.flags = 2 | (int(rope[0]) << 8) | (int(rope[1]) << 20)
        weight = weight.contiguous()
        self.image = torch.empty(lib.tgis_dense_prepared_bytes(self.N, self.K), dtype=torch.uint8,
                                 device=weight.device)
        _check(lib.tgis_dense_prepare(_ptr(weight), self.N, self.K, dtype_code(weight.dtype), self.flags,
                                      _ptr(self.image), _stream()), "tgis_dense_prepare")
        torch.cuda.current_stream().synchronize()

    def workspace_bytes(self, M: int) -> int:
        return load_library().tgis_dense_gemm_workspace_bytes(M, self.K, self.N)


def dense_gemm(x: torch.Tensor, w: DenseWeight, ws: Workspace, bias=None, out_f32: bool = False, act: int = 0,
               out=None) -> torch.Tensor:
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == w.dtype
    M = x.shape[0]
    assert x.shape[1] == (2 * w.K if act == 1 else w.K)
    assert (act == 2) == bool(w.flags & 1), "act 2 runs on (and only on) a gate|up image"
    if out is None:
        out = torch.empty((M, w.N // 2 if act == 2 else w.N), dtype=torch.float32 if out_f32 else w.dtype,
                          device=x.device)
    ws.ensure(w.workspace_bytes(M))
    _check(
        load_library().tgis_dense_gemm(_ptr(x), x.stride(0), _ptr(w.image), _ptr(bias), _ptr(out), out.stride(0), M,
                                       w.K, w.N, dtype_code(w.dtype), int(out_f32), act, ws.ptr, ws.nbytes,
                                       _stream()), "tgis_dense_gemm")
    return out


def dense_gemm_partial(x: torch.Tensor, w: DenseWeight, bias=None, act: int = 0) -> Partial:
    """Launch the dense GEMM but leave the split-K reduce (and bias) to the consumer kernel."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == w.dtype and x.shape[0] <= PARTIAL_MAX_M
    lib = load_library()
    nbytes = lib.tgis_dense_gemm_partial_bytes(x.shape[0], w.K, w.N)
    slabs = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
    S = _c_int()
    ld = _c_i64()
    _check(
        lib.tgis_dense_gemm_partial(_ptr(x), x.stride(0), _ptr(w.image), x.shape[0], w.K, w.N, dtype_code(w.dtype), act,
                                    _ptr(slabs), nbytes, ctypes.byref(S), ctypes.byref(ld), _stream()),
        "tgis_dense_gemm_partial")
    p = Partial(slabs, S.value, ld.value, x.shape[0], w.N, bias)
    p.dtype = w.dtype
    return p


def dense_gemm_rope(x: torch.Tensor, w: DenseWeight, bias, cos, sin, positions, slots, k_pool, v_pool, H: int, Hkv: int,
                    D: int, out=None, kv_scales=(1.0, 1.0)) -> torch.Tensor:
    """Dense qkv projection + rotary embedding + cache write in one launch (decode, M <= 64; `w` is the rope image of the
    fused qkv weight).  Returns [M, (H + 2 Hkv) D] whose first H D columns hold the rotated q.  One-byte pools: as
    gptq_gemm_rope."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == w.dtype and x.shape[1] == w.K
    assert w.flags & 2 and w.N == (H + 2 * Hkv) * D and cos.dtype == w.dtype and cos.shape[1] * 2 == D
    assert positions.dtype == torch.int32 and slots.dtype == torch.int32
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, w.N), dtype=w.dtype, device=x.device)
    args = (_ptr(x), x.stride(0), _ptr(w.image), _ptr(bias), _ptr(positions), _ptr(slots), _ptr(cos), _ptr(sin),
            _ptr(out), out.stride(0), _ptr(k_pool), _ptr(v_pool), M, w.K, w.N, H, Hkv, D, dtype_code(w.dtype), _stream())
    _call_kv("tgis_dense_gemm_rope", args, k_pool, v_pool, kv_scales)
    return out


# ---- routed expert MLP (Mixtral) ----------------------------------------------------------------------
class MoeWeights:
    """One projection of E experts: E images of tgis_dense_prepare in one buffer, `stride` bytes apart.  gate_up=True: each
    expert's weight is its [gate | up] (w1 | w3) and the image interleaves the pairs for the SiLU * up epilogue.
    `expert_weight(e)` returns expert e's [N, K] tensor on the GPU; it is dropped as soon as its image is made."""

    def __init__(self, expert_weight, E: int, gate_up: bool = False):
        lib = load_library()
        self.E, self.flags = E, (1 if gate_up else 0)
        self.image = None
        for e in range(E):
            w = expert_weight(e).contiguous()
            if self.image is None:
                assert w.dim() == 2
                self.N, self.K = w.shape
                self.dtype = w.dtype
                self.stride = lib.tgis_dense_prepared_bytes(self.N, self.K)
                self.image = torch.empty((E, self.stride), dtype=torch.uint8, device=w.device)
            assert tuple(w.shape) == (self.N, self.K) and w.dtype == self.dtype
            _check(lib.tgis_dense_prepare(_ptr(w), self.N, self.K, dtype_code(w.dtype), self.flags, _ptr(self.image[e]),
                                          _stream()), "tgis_dense_prepare")
            torch.cuda.current_stream().synchronize()  # (w goes out of scope here)

    def expert(self, e: int) -> DenseWeight:
        """Expert e's image as a DenseWeight (a view, nothing is copied): what dense_gemm takes on the loop path."""
        w = DenseWeight.__new__(DenseWeight)
        w.N, w.K, w.dtype, w.flags, w.answers, w.image = self.N, self.K, self.dtype, self.flags, {}, self.image[e]
        return w


class Routing:
    """What moe_route leaves on the device for T tokens: expert_ids int32 [T, top_k], expert_w f32 [T, top_k], counts int32
    [E], offsets int32 [E + 1], slot_rows int32 [T top_k] (slots t * top_k + k grouped by expert, ascending inside each)."""

    def __init__(self, T: int, E: int, top_k: int, device):
        self.T, self.E, self.top_k = T, E, top_k
        self.expert_ids = torch.empty((T, top_k), dtype=torch.int32, device=device)
        self.expert_w = torch.empty((T, top_k), dtype=torch.float32, device=device)
        # counts and offsets share one allocation: the loop path reads both back in one copy
        self.lists = torch.empty(2 * E + 1, dtype=torch.int32, device=device)
        self.counts, self.offsets = self.lists[:E], self.lists[E:]
        self.slot_rows = torch.empty(T * top_k, dtype=torch.int32, device=device)


def moe_route(logits: torch.Tensor, top_k: int) -> Routing:
    """Top-k routing of fp32 router logits [T, E] (softmax, top_k, renormalise: MixtralTopKRouter), all on the device."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and (logits.shape[0] == 0 or logits.stride(1) == 1)
    T, E = logits.shape
    r = Routing(T, E, top_k, logits.device)
    _check(load_library().tgis_moe_route(_ptr(logits), logits.stride(0), T, E, top_k, _ptr(r.expert_ids), _ptr(r.expert_w),
                                         _ptr(r.counts), _ptr(r.offsets), _ptr(r.slot_rows), _stream()), "tgis_moe_route")
    return r


def moe_gemm_up(x: torch.Tensor, w: MoeWeights, r: Routing, out=None) -> torch.Tensor:
    """h [T top_k, I]: SiLU(gate) * up of every slot's token under the slot's expert (act 2's rounding)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == w.dtype and x.shape == (r.T, w.K) and w.flags & 1 and w.E == r.E
    if out is None:
        out = torch.empty((r.T * r.top_k, w.N // 2), dtype=w.dtype, device=x.device)
    _check(load_library().tgis_moe_gemm_up(_ptr(x), x.stride(0), _ptr(w.image), w.stride, _ptr(r.offsets), _ptr(r.slot_rows),
                                           _ptr(out), out.stride(0), r.T, w.K, w.N, w.E, r.top_k, dtype_code(w.dtype),
                                           _stream()), "tgis_moe_gemm_up")
    return out


def moe_gemm_down(h: torch.Tensor, w: MoeWeights, r: Routing, partial: bool = False):
    """Every slot's row of h through its expert's down projection, scaled by its routing weight in fp32.  partial (T <=
    PARTIAL_MAX_M): a Partial with S = top_k whose slab k, row t holds token t's k-th expert — the next add + RMSNorm
    finishes the sum.  Otherwise the finished [T, hidden] tensor in the model dtype, summed over k in fixed order."""
    assert h.dim() == 2 and h.stride(1) == 1 and h.dtype == w.dtype and h.shape == (r.T * r.top_k, w.K)
    assert not (w.flags & 1) and w.E == r.E
    lib = load_library()
    form = 0 if partial else 1
    assert not partial or r.T <= PARTIAL_MAX_M
    nbytes = lib.tgis_moe_gemm_down_bytes(r.T, w.N, r.top_k, form)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=h.device)
    out = None if partial else torch.empty((r.T, w.N), dtype=w.dtype, device=h.device)
    _check(lib.tgis_moe_gemm_down(_ptr(h), h.stride(0), _ptr(w.image), w.stride, _ptr(r.offsets), _ptr(r.slot_rows),
                                  _ptr(r.expert_w), r.T, w.K, w.N, w.E, r.top_k, dtype_code(w.dtype), form, _ptr(scratch),
                                  nbytes, _ptr(out), w.N, _stream()), "tgis_moe_gemm_down")
    if not partial:
        return out
    p = Partial(scratch, r.top_k, (w.N + 31) // 32 * 32, r.T, w.N, None)
    p.dtype = w.dtype
    return p


# group sizes the int4 expert kernels have a form for (rows per group; a single group, written -1 or K, is served too)
MOE_GPTQ_GROUP_SIZES = tuple(64 << n for n in range(9))


def moe_gptq_group_ok(groupsize: int, K: Optional[int] = None) -> bool:
    """Whether tgis_moe_gptq_gemm_* serve this group size: one group (-1, or the whole K), or 64 * 2^n rows dividing K."""
    if groupsize == -1 or (K is not None and groupsize == K):
        return True
    return groupsize in MOE_GPTQ_GROUP_SIZES and (K is None or K % groupsize == 0)


class MoeGptqWeights:
    """The int4 twin of MoeWeights: E images of tgis_gptq_prepare in one [E, stride] buffer.  `expert_bundle(e)` returns expert
    e's (qweight, qzeros, scales, g_idx, bits, groupsize) on the GPU; the bundle is dropped as soon as its image is made.
    gate_up=True: the columns are [gate | up] (w1 | w3) and the image interleaves the pairs (flags bit 0)."""

    def __init__(self, expert_bundle, E: int, gate_up: bool = False):
        lib = load_library()
        self.E, self.flags = E, (1 if gate_up else 0)
        self.dtype = torch.float16
        self.image = None
        for e in range(E):
            qweight, qzeros, scales, g_idx, bits, groupsize = expert_bundle(e)[:6]
            if bits != 4:
                raise TgisHipError(f"Mixtral expert {e}: GPTQ experts are served at 4 bits, not {bits}")
            K, N, G = qweight.shape[0] * 8, qweight.shape[1], qzeros.shape[0]
            if K % 64 or N % 32:
                raise TgisHipError(f"Mixtral expert {e}: int4 expert matrices need K % 64 == 0 and N % 32 == 0, got K {K}, N {N}")
            if K % G or not moe_gptq_group_ok(K // G, K):
                raise TgisHipError(f"Mixtral expert {e}: the int4 expert kernels have no form for groups of "
                                   f"{K // G if K % G == 0 else groupsize} rows (one group, or 64 * 2^n rows)")
            if g_idx is not None:
                if isinstance(g_idx, tuple) or g_idx.numel() != K:
                    raise TgisHipError(f"Mixtral expert {e}: act-order (permuted) GPTQ experts are not served")
                gi = g_idx.to("cpu", torch.int64)
                if not (torch.equal(gi, torch.arange(K) // (K // G)) or (G == 1 and not bool(gi.any()))):
                    raise TgisHipError(f"Mixtral expert {e}: act-order GPTQ experts (a non-trivial g_idx) are not served")
            if self.image is None:
                self.K, self.N, self.groups = K, N, G
                self.stride = lib.tgis_gptq_prepared_bytes(K, N, G)
                self.image = torch.empty((E, self.stride), dtype=torch.uint8, device=qweight.device)
            assert (K, N, G) == (self.K, self.N, self.groups), "every expert of a layer has the same quantised shape"
            _check(lib.tgis_gptq_prepare(_ptr(qweight.contiguous()), _ptr(qzeros.contiguous()),
                                         _ptr(scales.to(torch.float16).contiguous()), None, None, K, N, G, self.flags,
                                         _ptr(self.image[e]), _stream()), "tgis_gptq_prepare")
            torch.cuda.current_stream().synchronize()  # (the bundle goes out of scope here)

    def expert(self, e: int) -> GptqWeight:
        """Expert e's image as a GptqWeight (a view, nothing is copied): what gptq_gemm takes on the loop path."""
        w = GptqWeight.__new__(GptqWeight)
        w.K, w.N, w.groups, w.flags, w.image = self.K, self.N, self.groups, self.flags, self.image[e]
        w.answers, w.partial_plan, w.perm, w.in_features = {}, {}, None, self.K
        return w


def moe_gptq_gemm_up(x: torch.Tensor, w: MoeGptqWeights, r: Routing, out=None) -> torch.Tensor:
    """moe_gemm_up over int4 expert images: h [T top_k, I] in f16."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.shape == (r.T, w.K) and w.flags & 1 and w.E == r.E
    if out is None:
        out = torch.empty((r.T * r.top_k, w.N // 2), dtype=x.dtype, device=x.device)
    _check(load_library().tgis_moe_gptq_gemm_up(_ptr(x), x.stride(0), _ptr(w.image), w.stride, _ptr(r.offsets),
                                                _ptr(r.slot_rows), _ptr(out), out.stride(0), r.T, w.K, w.N, w.groups, w.E,
                                                r.top_k, dtype_code(x.dtype), _stream()), "tgis_moe_gptq_gemm_up")
    return out


def moe_gptq_gemm_down(h: torch.Tensor, w: MoeGptqWeights, r: Routing, partial: bool = False):
    """moe_gemm_down over int4 expert images: a Partial with S = top_k (partial, T <= PARTIAL_MAX_M) or the finished f16
    [T, hidden] tensor."""
    assert h.dim() == 2 and h.stride(1) == 1 and h.shape == (r.T * r.top_k, w.K)
    assert not (w.flags & 1) and w.E == r.E
    lib = load_library()
    form = 0 if partial else 1
    assert not partial or r.T <= PARTIAL_MAX_M
    nbytes = lib.tgis_moe_gemm_down_bytes(r.T, w.N, r.top_k, form)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=h.device)
    out = None if partial else torch.empty((r.T, w.N), dtype=h.dtype, device=h.device)
    _check(lib.tgis_moe_gptq_gemm_down(_ptr(h), h.stride(0), _ptr(w.image), w.stride, _ptr(r.offsets), _ptr(r.slot_rows),
                                       _ptr(r.expert_w), r.T, w.K, w.N, w.groups, w.E, r.top_k, dtype_code(h.dtype), form,
                                       _ptr(scratch), nbytes, _ptr(out), w.N, _stream()), "tgis_moe_gptq_gemm_down")
    if not partial:
        return out
    return Partial(scratch, r.top_k, w.N, r.T, w.N, None)


# ---- per-request LoRA adapters (csrc/lora.hip) -----------------------------------------------------------
LORA_MAX_T, LORA_MAX_SLOTS, LORA_MAX_RANK = 64, 32, 64  # rows of the kernel path, slots, rank cap


class LoraImages:
    """The slot images of one linear (tgis_hip.h): A [S, P, max_rank, K] and B [S, max_rank / 16, N, 16] in the model dtype,
    ranks int32 [S] and scales f32 [S], allocated once, at fixed addresses.  `bounds`: the P + 1 column bounds of the P
    projections fused into the linear.  `host_ranks` / `host_scales` mirror the device arrays for the host loop of long
    prefills."""

    def __init__(self, K: int, bounds, S: int, max_rank: int, dtype, device):
        self.K, self.N, self.P, self.S, self.max_rank, self.dtype = K, bounds[-1], len(bounds) - 1, S, max_rank, dtype
        self.bounds = tuple(int(b) for b in bounds)
        self._bounds_c = (_c_i64 * 4)(*(self.bounds + (self.N,) * (4 - len(self.bounds))))
        self.A = torch.zeros((S, self.P, max_rank, K), dtype=dtype, device=device)
        self.B = torch.zeros((S, max_rank // 16, self.N, 16), dtype=dtype, device=device)
        self.ranks = torch.zeros(S, dtype=torch.int32, device=device)
        self.scales = torch.zeros(S, dtype=torch.float32, device=device)
        self.host_ranks, self.host_scales = [0] * S, [0.0] * S
        self.host_present = [(False,) * self.P for _ in range(S)]  # which of the P projections a slot's adapter targets
        self.a_stride = self.A.stride(0) * self.A.element_size()
        self.b_stride = self.B.stride(0) * self.B.element_size()

    @property
    def nbytes(self) -> int:
        return self.A.numel() * self.A.element_size() + self.B.numel() * self.B.element_size() + 8 * self.S

    @staticmethod
    def pack(As, Bs, bounds, K: int, dtype):
        """(rank, a [P, r16, K], b [r16 / 16, N, 16]) on the CPU from P pairs (A [r, K], B [n_p, r]), a pair None where the
        adapter leaves the projection out; zero from the rank up to the next multiple of 16.  rank 0: nothing to load."""
        rank = max((a.shape[0] for a in As if a is not None), default=0)
        if rank == 0:
            return 0, None, None
        r16, N = (rank + 15) // 16 * 16, bounds[-1]
        a = torch.zeros((len(As), r16, K), dtype=dtype)
        b = torch.zeros((N, r16), dtype=dtype)
        for p, (ap, bp) in enumerate(zip(As, Bs)):
            if ap is not None:
                a[p, :rank] = ap.to(dtype)
                b[bounds[p]:bounds[p + 1], :rank] = bp.to(dtype)
        return rank, a, b.view(N, r16 // 16, 16).permute(1, 0, 2).contiguous()

    def load(self, s: int, As, Bs, scale: float) -> None:
        """An adapter's share of this linear into slot s: copies on the current stream, so a captured graph sees it on its
        next replay.  What the slot held beyond the new rank (rounded up to 16) stays and is never read."""
        assert 0 <= s < self.S and len(As) == len(Bs) == self.P
        rank, a, b = self.pack(As, Bs, self.bounds, self.K, self.dtype)
        assert rank <= self.max_rank
        if rank:
            self.A[s, :, :a.shape[1]].copy_(a)
            self.B[s, :b.shape[0]].copy_(b)
        self.ranks[s:s + 1].copy_(torch.tensor([rank], dtype=torch.int32))
        self.scales[s:s + 1].copy_(torch.tensor([scale if rank else 0.0], dtype=torch.float32))
        self.host_ranks[s], self.host_scales[s] = rank, float(scale) if rank else 0.0
        self.host_present[s] = tuple(a is not None for a in As)


class LoraGroup:
    """What lora_group leaves on the device for T rows and S slots: counts int32 [S], offsets int32 [S + 1], rows int32 [T]."""

    def __init__(self, T: int, S: int, device):
        self.T, self.S = T, S
        self.lists = torch.empty(2 * S + 1, dtype=torch.int32, device=device)
        self.counts, self.offsets = self.lists[:S], self.lists[S:]
        self.rows = torch.empty(T, dtype=torch.int32, device=device)


def lora_group(slot: torch.Tensor, S: int) -> LoraGroup:
    """The rows of `slot` (int32 [T], -1 .. S-1) grouped by slot, all on the device."""
    assert slot.dim() == 1 and slot.dtype == torch.int32 and slot.is_contiguous()
    g = LoraGroup(slot.numel(), S, slot.device)
    _check(load_library().tgis_lora_group(_ptr(slot), g.T, S, _ptr(g.counts), _ptr(g.offsets), _ptr(g.rows), _stream()),
           "tgis_lora_group")
    return g


def lora_shrink(x: torch.Tensor, w: LoraImages, g: LoraGroup, v=None) -> torch.Tensor:
    """v fp32 [T, P, max_rank]: A_s[p] x[t] for the rows of the lists, up to each slot's rank rounded up to 16."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == w.dtype and x.shape == (g.T, w.K) and g.S == w.S
    if v is None:
        v = torch.empty((g.T, w.P, w.max_rank), dtype=torch.float32, device=x.device)
    _check(load_library().tgis_lora_shrink(_ptr(x), x.stride(0), _ptr(w.A), w.a_stride, _ptr(w.ranks), _ptr(g.offsets),
                                           _ptr(g.rows), _ptr(v), g.T, w.K, w.P, w.S, w.max_rank, dtype_code(w.dtype),
                                           _stream()), "tgis_lora_shrink")
    return v


def lora_expand(v: torch.Tensor, w: LoraImages, g: LoraGroup, y: torch.Tensor) -> torch.Tensor:
    """y[t] += scale_s B_s v[t] in place for the rows of the lists (one rounding to the model dtype); other rows untouched."""
    assert y.dim() == 2 and y.stride(1) == 1 and y.dtype == w.dtype and y.shape == (g.T, w.N) and g.S == w.S
    assert v.dtype == torch.float32 and v.is_contiguous() and v.shape == (g.T, w.P, w.max_rank)
    _check(load_library().tgis_lora_expand(_ptr(v), _ptr(w.B), w.b_stride, _ptr(w.ranks), _ptr(w.scales), _ptr(g.offsets),
                                           _ptr(g.rows), w._bounds_c, _ptr(y), y.stride(0), g.T, w.N, w.P, w.S, w.max_rank,
                                           dtype_code(w.dtype), _stream()), "tgis_lora_expand")
    return y


def clear_error() -> None:
    """Drop a stale HIP error (aborted graph capture) so that it is not blamed on the next launch."""
    load_library().tgis_clear_error()


# ---- norms --------------------------------------------------------------------------------------------
def rmsnorm_residual(x, residual, weight, eps: float, y=None, res_out=None, frag: bool = False):
    """(y, res) = fused add + RMSNorm; mirrors LlamaRMSNorm.forward (flash_llama_modeling.py:113-152).
    frag (rows <= 64, f16): y is returned as a FragAct, the layout the int4 GEMM behind the norm reads."""
    rows, hidden = x.shape
    yf = None
    if frag:
        assert y is None and rows <= 64 and hidden % 64 == 0 and x.dtype == torch.float16
        yf = FragAct.empty(rows, hidden, x.device)
        y, ldy = yf.buf, LD_FRAGMENTS
    else:
        ldy = hidden
    if isinstance(x, Partial):
        if y is None:
            y = torch.empty((rows, hidden), dtype=x.dtype, device=x.device)
        if res_out is None:
            res_out = torch.empty((rows, hidden), dtype=x.dtype, device=x.device)  # the reduced (+ residual) stream
        _check(
            load_library().tgis_rmsnorm_residual_partial(_ptr(x.slabs), x.S, x.ld, _ptr(x.bias), _ptr(residual),
                                                         _ptr(weight), _ptr(y), ldy, _ptr(res_out), rows, hidden,
                                                         float(eps), dtype_code(x.dtype), _stream()),
            "tgis_rmsnorm_residual_partial")
        return (yf if frag else y), res_out
    assert x.dim() == 2 and x.is_contiguous()
    if y is None:
        y = torch.empty_like(x)
    if res_out is None:
        res_out = torch.empty_like(x) if residual is not None else x
    _check(
        load_library().tgis_rmsnorm_residual(_ptr(x), _ptr(residual), _ptr(weight), _ptr(y), ldy,
                                             _ptr(res_out) if residual is not None else None, rows, hidden,
                                             float(eps), dtype_code(x.dtype), _stream()), "tgis_rmsnorm_residual")
    return (yf if frag else y), res_out


def layernorm_residual(x, residual, weight, bias, eps: float, y=None, res_out=None):
    """(y, res) = fused add + LayerNorm; mirrors FastLayerNorm.forward (utils/layers.py:363-396)."""
    if isinstance(x, Partial):
        rows, hidden = x.shape
        if y is None:
            y = torch.empty((rows, hidden), dtype=x.dtype, device=x.device)
        if res_out is None:
            res_out = torch.empty_like(y)  # always materialised: it is the reduced (+residual) stream
        _check(
            load_library().tgis_layernorm_residual_partial(_ptr(x.slabs), x.S, x.ld, _ptr(x.bias), _ptr(residual),
                                                           _ptr(weight), _ptr(bias), _ptr(y), _ptr(res_out), rows,
                                                           hidden, float(eps), dtype_code(x.dtype), _stream()),
            "tgis_layernorm_residual_partial")
        return y, res_out
    assert x.dim() == 2 and x.is_contiguous()
    rows, hidden = x.shape
    if y is None:
        y = torch.empty_like(x)
    if res_out is None:
        res_out = torch.empty_like(x) if residual is not None else x
    _check(
        load_library().tgis_layernorm_residual(_ptr(x), _ptr(residual), _ptr(weight), _ptr(bias), _ptr(y),
                                               _ptr(res_out) if residual is not None else None, rows, hidden,
                                               float(eps), dtype_code(x.dtype), _stream()),
        "tgis_layernorm_residual")
    return y, res_out


def layernorm2_residual(residual, a, b, w1, b1, eps: float, w2=None, b2=None, res_out=None, a_bias=None, b_bias=None):
    """GPT-NeoX parallel-residual boundary: h' = residual + a (+ a_bias) + b (+ b_bias) in fp32, rounded once, then
    y1 = LN(h'; w1, b1) and (w2 given) y2 = LN(h'; w2, b2).  `a` / `b` are tensors, `Partial`s or None.
    Returns (y1, y2 or None, h')."""
    assert residual.dim() == 2 and residual.is_contiguous()
    rows, hidden = residual.shape
    y1 = torch.empty_like(residual)
    y2 = torch.empty_like(residual) if w2 is not None else None
    if res_out is None:
        res_out = torch.empty_like(residual)

    def parts(x, bias):
        if isinstance(x, Partial):
            assert x.shape == (rows, hidden) and (bias is None or x.bias is None)
            return None, x.slabs, x.S, x.ld, x.bias if bias is None else bias
        if x is not None:
            assert x.shape == (rows, hidden) and x.is_contiguous() and x.dtype == residual.dtype
        return x, None, 0, 0, bias

    pa, pb = parts(a, a_bias), parts(b, b_bias)
    _check(
        load_library().tgis_layernorm2_residual_partial(
            _ptr(residual), _ptr(pa[0]), _ptr(pa[1]), pa[2], pa[3], _ptr(pa[4]), _ptr(pb[0]), _ptr(pb[1]), pb[2], pb[3],
            _ptr(pb[4]), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(y1), _ptr(y2), _ptr(res_out), rows, hidden,
            float(eps), dtype_code(residual.dtype), _stream()), "tgis_layernorm2_residual_partial")
    return y1, y2, res_out


# ---- rope + kv write, attention --------------------------------------------------------------------------
def _qk_norm_args(qk_norm, D: int, dtype) -> tuple:
    """(q_w, k_w, eps) of a `qk_norm` keyword as the arguments of the *_qknorm entry points."""
    q_w, k_w, eps = qk_norm
    for w in (q_w, k_w):
        assert w.dtype == dtype and w.is_contiguous() and w.numel() == D, "q / k norm weights are [head_dim] of the model dtype"
    return (_ptr(q_w), _ptr(k_w), float(eps))


def _rope_kv_write_qknorm(qkv, qk_norm, cos, sin, positions, slots, k_pool, v_pool, H, Hkv, D, rot_dim, kv_scales):
    if isinstance(qkv, Partial):
        out = torch.empty((qkv.M, qkv.N), dtype=qkv.dtype, device=qkv.device)
        src = (_ptr(qkv.slabs), qkv.S, qkv.ld, _ptr(qkv.bias))
    else:
        assert qkv.dim() == 2 and qkv.stride(1) == 1
        out, src = qkv, (None, 0, 0, None)
    _check(load_library().tgis_rope_kv_write_qknorm(
        _ptr(out), out.stride(0), *src, *_qk_norm_args(qk_norm, D, out.dtype), _ptr(cos), _ptr(sin), _ptr(positions),
        _ptr(slots), _ptr(k_pool), _ptr(v_pool), out.shape[0], H, Hkv, D, rot_dim, dtype_code(out.dtype),
        *_kv_args(k_pool, v_pool, kv_scales), _stream()), "tgis_rope_kv_write_qknorm")
    return out


def _rope_kv_write_prefill_qknorm(qkv, qk_norm, cos, sin, positions, cu_seqlens, past_lens, block_tables, k_pool, v_pool,
                                  max_len, H, Hkv, D, rot_dim, kv_scales):
    _check(load_library().tgis_rope_kv_write_prefill_qknorm(
        _ptr(qkv), qkv.stride(0), *_qk_norm_args(qk_norm, D, qkv.dtype), _ptr(cos), _ptr(sin), _ptr(positions),
        _ptr(cu_seqlens), _ptr(past_lens), _ptr(block_tables), block_tables.shape[1], _ptr(k_pool), _ptr(v_pool),
        block_tables.shape[0], qkv.shape[0], max_len, H, Hkv, D, rot_dim, dtype_code(qkv.dtype),
        *_kv_args(k_pool, v_pool, kv_scales), _stream()), "tgis_rope_kv_write_prefill_qknorm")
    return qkv


def rope_kv_write(qkv, cos, sin, positions, slots, k_pool, v_pool, H: int, Hkv: int, D: int, rot_dim: int,
                  kv_scales=(1.0, 1.0), qk_norm=None):
    """Rotates q,k in place and writes k,v to the cache.  `qkv` may be a Partial: the reduced, rotated activation is
    then materialised into a fresh [T, (H+2Hkv)D] tensor, which is returned (the plain form returns qkv itself).
    One-byte pools (kv_is8) receive e4m3 codes of k / k_scale and v / v_scale, kv_scales = (k_scale, v_scale).
    qk_norm = (q_w, k_w, eps): every q and k head is RMS-normalised over its D elements in front of the rotation
    (tgis_rope_kv_write_qknorm; Qwen3)."""
    if qk_norm is not None:
        return _rope_kv_write_qknorm(qkv, qk_norm, cos, sin, positions, slots, k_pool, v_pool, H, Hkv, D, rot_dim, kv_scales)
    if isinstance(qkv, Partial):
        T = qkv.M
        out = torch.empty((T, qkv.N), dtype=qkv.dtype, device=qkv.device)
        args = (_ptr(qkv.slabs), qkv.S, qkv.ld, _ptr(qkv.bias), _ptr(out), out.stride(0), _ptr(cos), _ptr(sin),
                _ptr(positions), _ptr(slots), _ptr(k_pool), _ptr(v_pool), T, H, Hkv, D, rot_dim, dtype_code(out.dtype),
                _stream())
        _call_kv("tgis_rope_kv_write_partial", args, k_pool, v_pool, kv_scales)
        return out
    assert qkv.dim() == 2 and qkv.stride(1) == 1
    T = qkv.shape[0]
    args = (_ptr(qkv), qkv.stride(0), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(slots), _ptr(k_pool), _ptr(v_pool), T,
            H, Hkv, D, rot_dim, dtype_code(qkv.dtype), _stream())
    _call_kv("tgis_rope_kv_write", args, k_pool, v_pool, kv_scales)
    return qkv


def rope_kv_write_prefill(qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, max_len: int, H: int,
                          Hkv: int, D: int, rot_dim: int, kv_scales=(1.0, 1.0), qk_norm=None):
    """rope_kv_write for a fresh prefill (token i of a sequence = cache position i): page-wise cache writes."""
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and block_tables.is_contiguous()
    if qk_norm is not None:
        return _rope_kv_write_prefill_qknorm(qkv, qk_norm, cos, sin, positions, cu_seqlens, None, block_tables, k_pool,
                                             v_pool, max_len, H, Hkv, D, rot_dim, kv_scales)
    B = block_tables.shape[0]
    args = (_ptr(qkv), qkv.stride(0), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(cu_seqlens), _ptr(block_tables),
            block_tables.shape[1], _ptr(k_pool), _ptr(v_pool), B, qkv.shape[0], max_len, H, Hkv, D, rot_dim,
            dtype_code(qkv.dtype), _stream())
    _call_kv("tgis_rope_kv_write_prefill", args, k_pool, v_pool, kv_scales)
    return qkv


def past_lens_tensor(past_lens, device) -> torch.Tensor:
    """[B] int32 on `device` from host ints: how many tokens of each sequence already sit in the cache in front of a
    prefill's.  Whole pages only, which is what rope_kv_write_prefill_at requires and cannot check on the device."""
    past = [int(n) for n in past_lens]
    assert all(n >= 0 and n % 32 == 0 for n in past), f"past_lens must be non-negative multiples of 32: {past}"
    return torch.tensor(past, dtype=torch.int32, device=device)


def rope_kv_write_prefill_at(qkv, cos, sin, positions, cu_seqlens, block_tables, k_pool, v_pool, max_len: int, H: int,
                             Hkv: int, D: int, rot_dim: int, past_lens, kv_scales=(1.0, 1.0), qk_norm=None):
    """rope_kv_write_prefill behind a cached prefix: token i of sequence b = cache position past_lens[b] + i.  `past_lens`
    is a list of host ints or the tensor `past_lens_tensor` made of one (a forward makes it once for all its layers);
    `cu_seqlens` and `max_len` describe the suffix tokens in `qkv`.  Pages in front of past_lens[b] / 32 are not written."""
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and block_tables.is_contiguous()
    if not isinstance(past_lens, torch.Tensor):
        past_lens = past_lens_tensor(past_lens, qkv.device)
    B = block_tables.shape[0]
    assert past_lens.dtype == torch.int32 and past_lens.is_contiguous() and past_lens.numel() == B
    if qk_norm is not None:
        return _rope_kv_write_prefill_qknorm(qkv, qk_norm, cos, sin, positions, cu_seqlens, past_lens, block_tables, k_pool,
                                             v_pool, max_len, H, Hkv, D, rot_dim, kv_scales)
    args = (_ptr(qkv), qkv.stride(0), _ptr(cos), _ptr(sin), _ptr(positions), _ptr(cu_seqlens), _ptr(block_tables),
            block_tables.shape[1], _ptr(k_pool), _ptr(v_pool), B, qkv.shape[0], max_len, H, Hkv, D, rot_dim,
            dtype_code(qkv.dtype), _stream())
    _call_kv("tgis_rope_kv_write_prefill_at", args, k_pool, v_pool, kv_scales, tail=(_ptr(past_lens),))
    return qkv


def attn_num_splits(B: int, Hkv: int, H: int, max_q_len: int, max_ctx: int) -> int:
    return load_library().tgis_attn_num_splits(B, Hkv, H, max_q_len, max_ctx)


def attn_num_splits_q(B: int, Hkv: int, H: int, max_q_len: int, max_ctx: int) -> int:
    """Key splits of a launch with up to max_q_len q tokens per sequence (a verify step, a suffix behind reused pages)."""
    return load_library().tgis_attn_num_splits_q(B, Hkv, H, max_q_len, max_ctx)


def attn_q_splits(B: int, Hkv: int, H: int, max_q_len: int, max_ctx: int) -> int:
    """What the model code asks: attn_num_splits at one q token, else attn_num_splits_q — whose answer below 1024 keys is 1
    by the rule's own definition (fewer than 32 pages), so the library is only asked from there on."""
    if max_q_len == 1:
        return attn_num_splits(B, Hkv, H, 1, max_ctx)
    return attn_num_splits_q(B, Hkv, H, max_q_len, max_ctx) if max_ctx >= 1024 else 1


def attn_workspace_bytes(total_q: int, H: int, Hkv: int, D: int, num_splits: int) -> int:
    return load_library().tgis_attn_workspace_bytes(total_q, H, Hkv, D, num_splits)


def attn_paged(q, ld_q: int, k_pool, v_pool, block_tables, ctx_lens, cu_seqlens_q, out, B: int, H: int, Hkv: int,
               D: int, max_q_len: int, max_ctx: int, scale: float, num_splits: int, ws: Optional[Workspace],
               kv_scales=(1.0, 1.0), q_mask=None, tree: Optional[bool] = None, window: Optional[int] = None):
    """q is a (view into a) [T, *] activation whose row stride is ld_q elements; out [T, H*D], or (decode, B <= 64) a
    FragAct of that shape for the o_proj GEMM.  One-byte pools (kv_is8) are read as k_scale * e4m3(k), v_scale * e4m3(v)
    (tgis_attn_paged_kv8), kv_scales = (k_scale, v_scale).
    q_mask (int64 [T], read as 64-bit words): tgis_attn_paged_tree — bit j of word i lets q row i of a sequence attend to that
    sequence's q row j, under the causal bound; the decode form only.  (tree=True with q_mask None asks the tree entry point
    with a null mask, which it refuses.)
    window (an int, not with q_mask / tree): tgis_attn_paged_window — a q row attends to the `window` cache positions up to
    its own; at max_q_len 1 the caller sizes num_splits for min(max_ctx, window + 31) keys, at any other it passes 1."""
    assert block_tables.dtype == torch.int32 and ctx_lens.dtype == torch.int32 and cu_seqlens_q.dtype == torch.int32
    if q_mask is not None:
        assert q_mask.dtype == torch.int64 and q_mask.is_contiguous() and q_mask.numel() >= q.shape[0]
    assert block_tables.is_contiguous()
    if isinstance(out, FragAct):
        assert max_q_len == 1 and out.K == H * D and out.M == B
        optr, ldo = _ptr(out.buf), LD_FRAGMENTS
    else:
        assert out.is_contiguous()
        optr, ldo = _ptr(out), H * D
    wptr, wbytes = (ws.ptr, ws.nbytes) if ws is not None else (None, 0)
    args = (_ptr(q), ld_q, _ptr(k_pool), _ptr(v_pool), _ptr(block_tables), block_tables.shape[1], _ptr(ctx_lens),
            _ptr(cu_seqlens_q), optr, ldo, B, H, Hkv, D, max_q_len, max_ctx, float(scale), dtype_code(q.dtype), num_splits,
            wptr, wbytes, _stream())
    if window is not None:
        assert q_mask is None and not tree, "a windowed launch takes no q_mask"
        _call_kv("tgis_attn_paged_window", args, k_pool, v_pool, kv_scales, tail=(int(window),))
    elif not (q_mask is not None if tree is None else tree):
        _call_kv("tgis_attn_paged", args, k_pool, v_pool, kv_scales)
    else:
        _call_kv("tgis_attn_paged_tree", args, k_pool, v_pool, kv_scales, tail=(_ptr(q_mask),))
    return out


def kv_absmax(k_pool, v_pool, block_tables, ctx_lens, Hkv: int, D: int, out):
    """Max-merges max |k| and max |v| per kv head over the cached tokens of block_tables / ctx_lens into out [2, Hkv] fp32
    (row 0 = k, row 1 = v; zeroed once by the caller, calls accumulate).  One layer's 16-bit pools only: the statistic is
    taken from a model running its ordinary cache."""
    assert block_tables.dtype == torch.int32 and ctx_lens.dtype == torch.int32 and block_tables.is_contiguous()
    assert k_pool.dtype == v_pool.dtype and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 2 * Hkv
    B = ctx_lens.numel()
    assert block_tables.dim() == 2 and block_tables.shape[0] == B
    _check(
        load_library().tgis_kv_absmax(_ptr(k_pool), _ptr(v_pool), _ptr(block_tables), block_tables.shape[1], _ptr(ctx_lens),
                                      B, Hkv, D, dtype_code(k_pool.dtype), _ptr(out), _stream()), "tgis_kv_absmax")
    return out


# ---- elementwise / sampling ---------------------------------------------------------------------------------
def act_mul(gate_up, I: int, out=None):
    T = gate_up.shape[0]
    assert gate_up.is_contiguous() and gate_up.shape[1] == 2 * I
    if out is None:
        out = torch.empty((T, I), dtype=gate_up.dtype, device=gate_up.device)
    _check(load_library().tgis_act_mul(_ptr(gate_up), _ptr(out), T, I, 1, dtype_code(gate_up.dtype), _stream()),
           "tgis_act_mul")
    return out


def gelu(x, tanh_approx: bool, out=None):
    assert x.is_contiguous()
    if out is None:
        out = torch.empty_like(x)
    _check(load_library().tgis_gelu(_ptr(x), _ptr(out), x.numel(), int(tanh_approx), dtype_code(x.dtype), _stream()),
           "tgis_gelu")
    return out


def embedding(ids, table, positions=None, pos_table=None, id_offset: int = 0, out=None):
    assert ids.dtype == torch.int64 and ids.is_contiguous() and table.is_contiguous()
    T = ids.numel()
    E = table.shape[1]
    if out is None:
        out = torch.empty((T, E), dtype=table.dtype, device=table.device)
    _check(
        load_library().tgis_embedding(_ptr(ids), _ptr(table), _ptr(positions), _ptr(pos_table), _ptr(out), T, E,
                                      table.shape[0], id_offset, dtype_code(table.dtype), _stream()),
        "tgis_embedding")
    return out


def decode_slots(positions, block_tables, slots, ctx_lens):
    B = positions.numel()
    _check(
        load_library().tgis_decode_slots(_ptr(positions), _ptr(block_tables), block_tables.shape[1], _ptr(slots),
                                         _ptr(ctx_lens), B, _stream()), "tgis_decode_slots")


def decode_advance(ids, position_ids, all_input_ids=None, cu_seqlens=None, cu_seqlens_q=None, stage_ids=None,
                   stage_positions=None):
    """After a decode step (flash_causal_lm.py:457,499,533-535 in one launch): position_ids += 1 in place, the new ids
    scattered into all_input_ids at the new positions, cu_seqlens += cu_seqlens_q in place; returns a private copy of
    `ids`.  stage_ids / stage_positions (a decode graph's static inputs) receive the next step's inputs as well."""
    B = ids.numel()
    assert ids.dtype == torch.int64 and position_ids.dtype == torch.int64 and position_ids.numel() == B
    assert ids.is_contiguous() and position_ids.is_contiguous()
    out = torch.empty_like(ids)
    ld = 0
    if all_input_ids is not None:
        assert all_input_ids.dtype == torch.int64 and all_input_ids.stride(1) == 1 and all_input_ids.shape[0] >= B
        ld = all_input_ids.stride(0)
    if cu_seqlens is not None:
        assert cu_seqlens.dtype == torch.int32 and cu_seqlens_q.dtype == torch.int32
        assert cu_seqlens.numel() == B + 1 and cu_seqlens_q.numel() == B + 1
    if stage_ids is not None:
        assert stage_ids.dtype == torch.int64 and stage_ids.numel() == B
    if stage_positions is not None:
        assert stage_positions.dtype == torch.int32 and stage_positions.numel() == B
    _check(
        load_library().tgis_decode_advance(_ptr(ids), _ptr(out), _ptr(position_ids), _ptr(all_input_ids), ld,
                                           _ptr(cu_seqlens), _ptr(cu_seqlens_q), _ptr(stage_ids), _ptr(stage_positions),
                                           B, _stream()), "tgis_decode_advance")
    return out


def _is(t, dtype, numel):
    return t.dtype == dtype and t.numel() == numel and t.is_contiguous()


def spec_stage(positions, latest_ids, drafts, block_tables, input_ids, positions_out, slots, ctx_lens):
    """The inputs of a verify forward (tgis_spec_stage): K + 1 rows per request, its latest token and its K drafts at the
    positions behind it, their cache slots from the block table, ctx_lens = position + K + 1."""
    B = positions.numel()
    K = drafts.shape[1] if drafts is not None else 0
    R = B * (K + 1)
    assert _is(positions, torch.int32, B) and _is(latest_ids, torch.int64, B) and _is(ctx_lens, torch.int32, B)
    assert drafts is None or (drafts.shape == (B, K) and _is(drafts, torch.int64, B * K))
    assert block_tables.dtype == torch.int32 and block_tables.shape[0] == B and block_tables.is_contiguous()
    assert _is(input_ids, torch.int64, R) and _is(positions_out, torch.int32, R) and _is(slots, torch.int32, R)
    _check(
        load_library().tgis_spec_stage(_ptr(positions), _ptr(latest_ids), _ptr(drafts), K, _ptr(block_tables),
                                       block_tables.shape[1], _ptr(input_ids), _ptr(positions_out), _ptr(slots),
                                       _ptr(ctx_lens), B, _stream()), "tgis_spec_stage")


def spec_accept(argmax_ids, argmax_logprobs, drafts, n_emit, position_ids, out_ids=None, out_logprobs=None,
                all_input_ids=None, cu_seqlens=None, stage_ids=None, stage_positions=None, _sampled=None):
    """After a verify step (tgis_spec_accept): request b emits the greedy ids behind its longest accepted draft prefix and
    the one that follows it; n_emit, the emitted ids / logprobs, position_ids += n_emit, the scatter into all_input_ids and
    the prefix sums onto cu_seqlens in one launch.  Returns the new latest ids.  drafts None (K = 0): decode_advance."""
    B = position_ids.numel()
    K = drafts.shape[1] if drafts is not None else 0
    R = B * (K + 1)
    assert _is(argmax_ids, torch.int64, R) and _is(position_ids, torch.int64, B) and _is(n_emit, torch.int32, B)
    assert drafts is None or (drafts.shape == (B, K) and _is(drafts, torch.int64, B * K))
    assert argmax_logprobs is None or _is(argmax_logprobs, torch.float32, R)
    assert out_ids is None or _is(out_ids, torch.int64, R)
    assert out_logprobs is None or (_is(out_logprobs, torch.float32, R) and argmax_logprobs is not None)
    ld = 0
    if all_input_ids is not None:
        assert all_input_ids.dtype == torch.int64 and all_input_ids.stride(1) == 1 and all_input_ids.shape[0] >= B
        ld = all_input_ids.stride(0)
    assert cu_seqlens is None or _is(cu_seqlens, torch.int32, B + 1)
    assert stage_ids is None or _is(stage_ids, torch.int64, B)
    assert stage_positions is None or _is(stage_positions, torch.int32, B)
    latest = torch.empty(B, dtype=torch.int64, device=position_ids.device)
    args = (_ptr(argmax_ids), _ptr(argmax_logprobs), _ptr(drafts), K, _ptr(n_emit), _ptr(out_ids), _ptr(out_logprobs),
            _ptr(latest), _ptr(position_ids), _ptr(all_input_ids), ld, _ptr(cu_seqlens), _ptr(stage_ids), _ptr(stage_positions))
    if _sampled is None:
        _check(load_library().tgis_spec_accept(*args, B, _stream()), "tgis_spec_accept")
    else:
        do_sample, rng = _sampled
        _check(load_library().tgis_spec_accept_sampled(*args, _ptr(do_sample), _ptr(rng), B, _stream()),
               "tgis_spec_accept_sampled")
    return latest


def spec_accept_sampled(chosen_ids, chosen_logprobs, drafts, n_emit, position_ids, do_sample=None, rng=None, **outputs):
    """tgis_spec_accept_sampled: spec_accept on the ids and logprobs warp_sample_verify chose, which also advances the
    offset of rng [B, 2] by n_emit for the requests with do_sample [B] != 0 (do_sample None: spec_accept bit for bit)."""
    B = position_ids.numel()
    assert do_sample is None or (_is(do_sample, torch.int32, B) and rng is not None)
    assert rng is None or (rng.dtype == torch.int64 and rng.shape == (B, 2) and rng.is_contiguous())
    return spec_accept(chosen_ids, chosen_logprobs, drafts, n_emit, position_ids, _sampled=(do_sample, rng), **outputs)


def spec_propose(all_input_ids, position_ids, ngram: int, drafts, hits, hits_copy=None):
    """Prompt lookup (tgis_spec_propose): drafts [B, K] = the tokens that followed the latest earlier occurrence of the
    longest suffix (<= ngram tokens) of each request's context all_input_ids[b, :position_ids[b] + 1]; hits [B] = the
    length that matched, 0 = none."""
    B, K = drafts.shape
    assert all_input_ids.dtype == torch.int64 and all_input_ids.stride(1) == 1 and all_input_ids.shape[0] >= B
    assert _is(position_ids, torch.int64, B) and _is(drafts, torch.int64, B * K) and _is(hits, torch.int32, B)
    assert hits_copy is None or _is(hits_copy, torch.int32, B)
    _check(
        load_library().tgis_spec_propose(_ptr(all_input_ids), all_input_ids.stride(0), _ptr(position_ids), K, ngram,
                                         _ptr(drafts), _ptr(hits), _ptr(hits_copy), B, _stream()), "tgis_spec_propose")


def spec_tree_stage(positions, latest_ids, drafts, block_tables, input_ids, positions_out, slots, ctx_lens):
    """The inputs of a tree verify forward (tgis_spec_tree_stage): drafts [B, C, K]; R = 1 + C K rows per request, the latest
    token, then candidate by candidate; positions_out by depth, slots by row, ctx_lens = position + R."""
    B = positions.numel()
    _, C, K = drafts.shape
    R = B * (1 + C * K)
    assert drafts.shape[0] == B and _is(drafts, torch.int64, B * C * K)
    assert _is(positions, torch.int32, B) and _is(latest_ids, torch.int64, B) and _is(ctx_lens, torch.int32, B)
    assert block_tables.dtype == torch.int32 and block_tables.shape[0] == B and block_tables.is_contiguous()
    assert _is(input_ids, torch.int64, R) and _is(positions_out, torch.int32, R) and _is(slots, torch.int32, R)
    _check(
        load_library().tgis_spec_tree_stage(_ptr(positions), _ptr(latest_ids), _ptr(drafts), C, K, _ptr(block_tables),
                                            block_tables.shape[1], _ptr(input_ids), _ptr(positions_out), _ptr(slots),
                                            _ptr(ctx_lens), B, _stream()), "tgis_spec_tree_stage")


def spec_tree_accept(argmax_ids, argmax_logprobs, drafts, n_emit, best, position_ids, out_ids=None, out_logprobs=None,
                     all_input_ids=None, cu_seqlens=None, stage_ids=None, stage_positions=None):
    """After a tree verify step (tgis_spec_tree_accept): drafts [B, C, K], argmax_ids / argmax_logprobs [B (1 + C K)];
    best [B] = the first candidate with the longest accepted prefix, and spec_accept's outputs (out_ids / out_logprobs
    [B (K + 1)]) along its path.  Returns the new latest ids."""
    B = position_ids.numel()
    _, C, K = drafts.shape
    R, E = B * (1 + C * K), B * (K + 1)
    assert drafts.shape[0] == B and _is(drafts, torch.int64, B * C * K)
    assert _is(argmax_ids, torch.int64, R) and _is(position_ids, torch.int64, B)
    assert _is(n_emit, torch.int32, B) and _is(best, torch.int32, B)
    assert argmax_logprobs is None or _is(argmax_logprobs, torch.float32, R)
    assert out_ids is None or _is(out_ids, torch.int64, E)
    assert out_logprobs is None or (_is(out_logprobs, torch.float32, E) and argmax_logprobs is not None)
    ld = 0
    if all_input_ids is not None:
        assert all_input_ids.dtype == torch.int64 and all_input_ids.stride(1) == 1 and all_input_ids.shape[0] >= B
        ld = all_input_ids.stride(0)
    assert cu_seqlens is None or _is(cu_seqlens, torch.int32, B + 1)
    assert stage_ids is None or _is(stage_ids, torch.int64, B)
    assert stage_positions is None or _is(stage_positions, torch.int32, B)
    latest = torch.empty(B, dtype=torch.int64, device=position_ids.device)
    _check(
        load_library().tgis_spec_tree_accept(_ptr(argmax_ids), _ptr(argmax_logprobs), _ptr(drafts), C, K, _ptr(n_emit),
                                             _ptr(best), _ptr(out_ids), _ptr(out_logprobs), _ptr(latest), _ptr(position_ids),
                                             _ptr(all_input_ids), ld, _ptr(cu_seqlens), _ptr(stage_ids),
                                             _ptr(stage_positions), B, _stream()), "tgis_spec_tree_accept")
    return latest


def spec_tree_commit(pool, block_tables, new_positions, best, n_emit, C: int, K: int):
    """Behind spec_tree_accept (tgis_spec_tree_commit): in every layer and kv head of pool [L, 2, pages, Hkv, 32 D] the keys
    and values of each request's accepted drafts move from the best candidate's rows to the first candidate's, where a chain
    would have written them.  new_positions [B] int32: what spec_tree_accept left in stage_positions."""
    B = new_positions.numel()
    L, two, pages, Hkv, PD = pool.shape
    assert two == 2 and pool.is_contiguous() and PD % 32 == 0 and pool.element_size() in (1, 2)
    assert _is(new_positions, torch.int32, B) and _is(best, torch.int32, B) and _is(n_emit, torch.int32, B)
    assert block_tables.dtype == torch.int32 and block_tables.shape[0] == B and block_tables.is_contiguous()
    _check(
        load_library().tgis_spec_tree_commit(_ptr(pool[0, 0]), _ptr(pool[0, 1]), pool.stride(0), L, pages, _ptr(block_tables),
                                             block_tables.shape[1], _ptr(new_positions), _ptr(best), _ptr(n_emit), C, K, B,
                                             Hkv, PD // 32, pool.element_size(), _stream()), "tgis_spec_tree_commit")


def spec_propose_multi(all_input_ids, position_ids, ngram: int, drafts, hits, hits_copy=None):
    """Prompt lookup for C candidates (tgis_spec_propose_multi): drafts [B, C, K]; sites from the longest suffix down and
    from the latest back, a site taken when its continuation starts with a token no taken candidate starts with; zeros for
    candidates not found.  hits [B] = the suffix length behind the first candidate, 0 = none."""
    B, C, K = drafts.shape
    assert all_input_ids.dtype == torch.int64 and all_input_ids.stride(1) == 1 and all_input_ids.shape[0] >= B
    assert _is(position_ids, torch.int64, B) and _is(drafts, torch.int64, B * C * K) and _is(hits, torch.int32, B)
    assert hits_copy is None or _is(hits_copy, torch.int32, B)
    _check(
        load_library().tgis_spec_propose_multi(_ptr(all_input_ids), all_input_ids.stride(0), _ptr(position_ids), C, K, ngram,
                                               _ptr(drafts), _ptr(hits), _ptr(hits_copy), B, _stream()),
        "tgis_spec_propose_multi")


def spec_mlp_input(hidden, n_emit, K1: int, out, out_copy=None, scale_input: bool = False, eps: float = 1e-6):
    """The MLP speculator's input (tgis_spec_mlp_input): out[b] (and out_copy[b]) = row b K1 + clamp(n_emit[b], 1, K1) - 1 of
    hidden [>= B K1, E] (n_emit None: row b K1), a bit-exact copy or, scale_input, its parameter-free RMS norm / sqrt(2)."""
    B, E = out.shape
    assert hidden.dim() == 2 and hidden.shape[1] == E and hidden.shape[0] >= B * K1 and hidden.is_contiguous()
    assert out.dtype == hidden.dtype and out.is_contiguous()
    assert n_emit is None or _is(n_emit, torch.int32, B)
    assert out_copy is None or (out_copy.shape == (B, E) and out_copy.dtype == hidden.dtype and out_copy.is_contiguous())
    _check(
        load_library().tgis_spec_mlp_input(_ptr(hidden), _ptr(n_emit), K1, _ptr(out), _ptr(out_copy), B, E, int(scale_input),
                                           float(eps), dtype_code(hidden.dtype), _stream()), "tgis_spec_mlp_input")
    return out


def spec_mlp_state(proj_out, tok, emb, ln_weight, ln_bias, alpha: float, x_out, eps: float = 1e-6):
    """Between the GEMMs of a speculator head (tgis_spec_mlp_state): x_out[b] = gelu(rmsln(proj_out[b] + alpha emb[tok[b]]))."""
    B, I = proj_out.shape
    dt = proj_out.dtype
    assert proj_out.is_contiguous() and _is(tok, torch.int64, B) and emb.dim() == 2 and emb.shape[1] == I
    assert emb.is_contiguous() and emb.dtype == dt and _is(ln_weight, dt, I) and _is(ln_bias, dt, I)
    assert x_out.shape == (B, I) and x_out.dtype == dt and x_out.is_contiguous()
    _check(
        load_library().tgis_spec_mlp_state(_ptr(proj_out), _ptr(tok), _ptr(emb), emb.shape[0], _ptr(ln_weight), _ptr(ln_bias),
                                           float(alpha), float(eps), _ptr(x_out), B, I, dtype_code(dt), _stream()),
        "tgis_spec_mlp_state")
    return x_out


def spec_mlp_drafts(toks, drafts, hits, hits_copy=None):
    """Behind the speculator's chain (tgis_spec_mlp_drafts): toks [K, B] -> drafts [B, K]; hits (and hits_copy) = 1."""
    B, K = drafts.shape
    assert toks.shape == (K, B) and _is(toks, torch.int64, K * B) and _is(drafts, torch.int64, B * K)
    assert _is(hits, torch.int32, B) and (hits_copy is None or _is(hits_copy, torch.int32, B))
    _check(load_library().tgis_spec_mlp_drafts(_ptr(toks), K, _ptr(drafts), _ptr(hits), _ptr(hits_copy), B, _stream()),
           "tgis_spec_mlp_drafts")


def argmax_scratch(B: int, device) -> torch.Tensor:
    """Scratch that lets argmax_logprob split the rows of a small batch over several workgroups each."""
    return torch.empty(max(16, load_library().tgis_argmax_scratch_bytes(B)), dtype=torch.uint8, device=device)


def argmax_logprob(logits, ids_out=None, logprob_out=None, scratch=None):
    assert logits.dim() == 2 and logits.stride(1) == 1
    B, V = logits.shape
    if ids_out is None:
        ids_out = torch.empty(B, dtype=torch.int64, device=logits.device)
    if logprob_out is None:
        logprob_out = torch.empty(B, dtype=torch.float32, device=logits.device)
    f32 = logits.dtype == torch.float32
    _check(
        load_library().tgis_argmax_logprob(_ptr(logits), logits.stride(0), B, V, int(f32),
                                           0 if f32 else dtype_code(logits.dtype), _ptr(ids_out),
                                           _ptr(logprob_out), _ptr(scratch), scratch.numel() if scratch is not None else 0,
                                           _stream()), "tgis_argmax_logprob")
    return ids_out, logprob_out


def warp_sample(logits, temperature=None, top_k=None, top_p_cut=None, typical_p=None, rep_penalty=None,
                input_ids=None, exclude_id: int = -1, eos_adjust=None, eos_id: int = -1, do_sample=None, rng=None):
    """The whole next-token chooser for a batch in one launch (tgis_warp_sample).  Returns (next_ids int64 [B],
    logprob f32 [B] of the chosen ids under the warped scores, lse f32 [B], warped scores f32 [B,V])."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    B, V = logits.shape
    dev = logits.device
    for t, dt in ((temperature, torch.float32), (top_k, torch.int32), (top_p_cut, torch.float32),
                  (typical_p, torch.float32), (rep_penalty, torch.float32), (do_sample, torch.int32)):
        assert t is None or (t.dtype == dt and t.numel() == B and t.is_contiguous() and t.device == dev)
    assert rng is None or (rng.dtype == torch.int64 and rng.shape == (B, 2) and rng.is_contiguous())
    assert eos_adjust is None or (eos_adjust.dtype == torch.float32 and eos_adjust.shape == (B, 2)
                                  and eos_adjust.is_contiguous())
    L = ld_ids = 0
    if input_ids is not None:
        assert input_ids.dtype == torch.int64 and input_ids.dim() == 2 and input_ids.shape[0] == B
        assert input_ids.stride(1) == 1
        L, ld_ids = input_ids.shape[1], input_ids.stride(0)
    scores = torch.empty((B, V), dtype=torch.float32, device=dev)
    ids = torch.empty(B, dtype=torch.int64, device=dev)
    lps = torch.empty(B, dtype=torch.float32, device=dev)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    _check(
        load_library().tgis_warp_sample(
            _ptr(logits), logits.stride(0), _ptr(scores), V, B, V, _ptr(temperature), _ptr(top_k), _ptr(top_p_cut),
            _ptr(typical_p), _ptr(rep_penalty), _ptr(input_ids), ld_ids, L, exclude_id, _ptr(eos_adjust), eos_id,
            _ptr(do_sample), _ptr(rng), _ptr(ids), _ptr(lps), _ptr(lse), _stream()), "tgis_warp_sample")
    return ids, lps, lse, scores


def warp_sample_verify(logits, drafts, K: int, temperature=None, top_k=None, top_p_cut=None, typical_p=None,
                       rep_penalty=None, input_ids=None, exclude_id: int = -1, eos_adjust=None, eos_id: int = -1,
                       do_sample=None, rng=None):
    """The chooser behind every row of a verify forward in one launch (tgis_warp_sample_verify): logits [B (K + 1), V], the
    parameter arrays [B] of warp_sample, drafts [B, K] (K = 0: None), eos_adjust [B, K + 1, 2]; rng [B, 2] is only read.
    Returns (next_ids int64 [B, K + 1], logprob f32 [B, K + 1], lse f32 [B, K + 1], warped scores f32 [B (K + 1), V])."""
    assert logits.dim() == 2 and logits.dtype == torch.float32 and logits.stride(1) == 1
    R, V = logits.shape
    K1 = K + 1
    assert 0 <= K <= 7 and R % K1 == 0
    B = R // K1
    dev = logits.device
    for t, dt in ((temperature, torch.float32), (top_k, torch.int32), (top_p_cut, torch.float32),
                  (typical_p, torch.float32), (rep_penalty, torch.float32), (do_sample, torch.int32)):
        assert t is None or (t.dtype == dt and t.numel() == B and t.is_contiguous() and t.device == dev)
    assert (drafts is None and K == 0) or (drafts.shape == (B, K) and _is(drafts, torch.int64, B * K))
    assert rng is None or (rng.dtype == torch.int64 and rng.shape == (B, 2) and rng.is_contiguous())
    assert eos_adjust is None or (eos_adjust.dtype == torch.float32 and eos_adjust.shape == (B, K1, 2)
                                  and eos_adjust.is_contiguous())
    L = ld_ids = 0
    if input_ids is not None:
        assert input_ids.dtype == torch.int64 and input_ids.dim() == 2 and input_ids.shape[0] == B
        assert input_ids.stride(1) == 1
        L, ld_ids = input_ids.shape[1], input_ids.stride(0)
    scores = torch.empty((R, V), dtype=torch.float32, device=dev)
    ids = torch.empty((B, K1), dtype=torch.int64, device=dev)
    lps = torch.empty((B, K1), dtype=torch.float32, device=dev)
    lse = torch.empty((B, K1), dtype=torch.float32, device=dev)
    _check(
        load_library().tgis_warp_sample_verify(
            _ptr(logits), logits.stride(0), _ptr(scores), V, B, K, V, _ptr(temperature), _ptr(top_k), _ptr(top_p_cut),
            _ptr(typical_p), _ptr(rep_penalty), _ptr(input_ids), ld_ids, L, exclude_id, _ptr(drafts), _ptr(eos_adjust),
            eos_id, _ptr(do_sample), _ptr(rng), _ptr(ids), _ptr(lps), _ptr(lse), _stream()), "tgis_warp_sample_verify")
    return ids, lps, lse, scores
