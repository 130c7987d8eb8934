"""The tiny Mixtral of tests/mixtral_tiny.py as a GPTQ checkpoint.  TEST INFRASTRUCTURE.

q/k/v/o and every expert's w1 / w3 / w2 are quantised min/max at 4 bits (oracle.tiny_models.quantize_gptq, group size 64, as
tests/bigcode_gptq_ref.py does for GPT-BigCode); the router, the norms, the embeddings and the head stay f16 — AutoGPTQ does not
quantise block_sparse_moe.gate.  `dense_tensors` is the same checkpoint with every quantised matrix replaced by
f16((q - z - 1) * s), the value the int4 kernels multiply by, under the published names: what the fixture generator
(tests/golden/make_mixtral_gptq_fixtures.py) runs transformers' fp32 MixtralForCausalLM on."""
from typing import Dict

import torch

from oracle import ops_ref
from oracle.tiny_models import quantize_gptq

try:
    from tests.mixtral_tiny import TinyMixtralConfig, tiny_mixtral_tensors  # noqa: F401
except ImportError:  # run from tests/golden with tests/ on the path
    from mixtral_tiny import TinyMixtralConfig, tiny_mixtral_tensors  # noqa: F401

GS = 64
QUANTISED = (".self_attn.q_proj.", ".self_attn.k_proj.", ".self_attn.v_proj.", ".self_attn.o_proj.", ".experts.")


def tiny_mixtral_gptq_tensors(cfg, seed: int, groupsize: int = GS) -> Dict[str, torch.Tensor]:
    """name -> tensor under the published Mixtral names with qweight / qzeros / scales / g_idx for the quantised linears."""
    t: Dict[str, torch.Tensor] = {}
    for name, v in tiny_mixtral_tensors(cfg, seed).items():
        if name.endswith(".weight") and any(q in name for q in QUANTISED):
            base = name[:-len(".weight")]
            qw, qz, sc, gi = quantize_gptq(v.float().t().contiguous(), groupsize)
            t[f"{base}.qweight"], t[f"{base}.qzeros"] = torch.from_numpy(qw), torch.from_numpy(qz)
            t[f"{base}.scales"], t[f"{base}.g_idx"] = torch.from_numpy(sc), torch.from_numpy(gi)
        else:
            t[name] = v
    return t


def dequantised(tensors: Dict[str, torch.Tensor], base: str, groupsize: int = GS) -> torch.Tensor:
    """W16 [K, N] of the quantised linear `base`: the reference formula, rounded once to f16."""
    return ops_ref.gptq_dequant(tensors[f"{base}.qweight"].numpy(), tensors[f"{base}.qzeros"].numpy(),
                                tensors[f"{base}.scales"], tensors[f"{base}.g_idx"].numpy(), groupsize).half()


def dense_tensors(tensors: Dict[str, torch.Tensor], groupsize: int = GS) -> Dict[str, torch.Tensor]:
    """The GPTQ dict -> the f16 dict of tests/mixtral_tiny.py's layout (weights [N, K]) holding the dequantised matrices."""
    out = {}
    for name, v in tensors.items():
        if name.endswith(".qweight"):
            base = name[:-len(".qweight")]
            out[f"{base}.weight"] = dequantised(tensors, base, groupsize).t().contiguous()
        elif not name.endswith((".qzeros", ".scales", ".g_idx")):
            out[name] = v
    return out
