"""A tiny GPTQ GPT-BigCode checkpoint for the tests, built as tests/gptq8_ref.py builds the 8-bit Llama one: the four linears
of every layer of oracle.tiny_models.tiny_bigcode_tensors quantised min/max (oracle.tiny_models.quantize_gptq at 4 bits,
gptq8_ref.quantize8 at 8) at group size 64, optionally act-order, biases kept; plus the dense dict dequantised by the
reference formula (oracle.ops_ref.gptq_dequant / gptq8_ref.dequant8) on which oracle.santacoder_ref.SantacoderRef runs."""
import os
import sys
from typing import Dict

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gptq8_ref  # noqa: E402

from oracle import ops_ref  # noqa: E402
from oracle.tiny_models import quantize_gptq, tiny_bigcode_tensors  # noqa: E402

GS = 64
LINEARS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")


def tiny_bigcode_gptq_tensors(cfg, seed: int, groupsize: int = GS, act_order: bool = False, bits: int = 4
                              ) -> Dict[str, torch.Tensor]:
    """name -> tensor in HF GPTBigCode naming with qweight / qzeros / scales / g_idx (+ bias) for the four linears."""
    dense = tiny_bigcode_tensors(cfg, seed, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed + 1000)
    t: Dict[str, torch.Tensor] = {}
    for name, v in dense.items():
        if name.endswith(".weight") and any(f".{lin}." in name for lin in LINEARS):
            base = name[:-len(".weight")]
            w_kn = v.t().contiguous()
            perm = torch.randperm(w_kn.shape[0], generator=g).numpy() if act_order else None
            if bits == 4:
                qw, qz, sc, gi = quantize_gptq(w_kn, groupsize, perm)
            else:
                qw, qz, sc, gi = gptq8_ref.quantize8(w_kn, groupsize, perm)
            t[f"{base}.qweight"], t[f"{base}.qzeros"] = torch.from_numpy(qw), torch.from_numpy(qz)
            t[f"{base}.scales"], t[f"{base}.g_idx"] = torch.from_numpy(sc), torch.from_numpy(gi)
        else:
            t[name] = v.to(torch.float16)
    return t


def dense_tensors(tensors: Dict[str, torch.Tensor], groupsize: int = GS, bits: int = 4) -> Dict[str, torch.Tensor]:
    """The GPTQ dict -> the dense dict SantacoderRef runs (weights [N, K] fp32, dequantised by the reference formula)."""
    out = {}
    for name, v in tensors.items():
        if name.endswith(".qweight"):
            base = name[:-len(".qweight")]
            qz, sc, gi = tensors[f"{base}.qzeros"], tensors[f"{base}.scales"], tensors[f"{base}.g_idx"]
            if bits == 4:
                w = ops_ref.gptq_dequant(v.numpy(), qz.numpy(), sc, gi.numpy(), groupsize)
            else:
                w = gptq8_ref.dequant8(v, qz, sc, gi, groupsize)
            out[f"{base}.weight"] = w.t().contiguous()
        elif not name.endswith((".qzeros", ".scales", ".g_idx")):
            out[name] = v
    return out
