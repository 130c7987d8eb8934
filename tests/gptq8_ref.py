"""The 8-bit GPTQ format restated for the tests (oracle/ops_ref.py is 4-bit only): the reference's packer
(QuantLinear.pack with bits = 8, utils/gptq/quant_linear.py:311-345), its dequantisation (:130-138,159-192; zeros + 1 is NOT
masked back to a byte), a min/max quantiser, and the dense tensor dict LlamaRef(..., quantize=None) runs."""
from typing import Dict, Optional

import numpy as np
import torch


def pack8(intweight: np.ndarray, zeros_true: np.ndarray):
    """Integer weights [K,N] (0..255) and true zero points [G,N] (1..256) -> (qweight int32 [K/4,N], qzeros int32 [G,N/4]):
    row r of qweight holds rows 4r..4r+3 in bytes 0..3; qzeros stores (zero - 1), byte t of word c = column 4c + t."""
    K, N = intweight.shape
    iw = intweight.astype(np.uint32)
    qweight = np.zeros((K // 4, N), dtype=np.uint32)
    for j in range(4):
        qweight |= iw[j::4] << (8 * j)
    z = (zeros_true.astype(np.int64) - 1).astype(np.uint32)
    assert z.max() <= 255
    qzeros = np.zeros((z.shape[0], N // 4), dtype=np.uint32)
    for j in range(4):
        qzeros |= z[:, j::4] << (8 * j)
    return qweight.astype(np.int32), qzeros.astype(np.int32)


def unpack8(qweight, qzeros):
    """(q int32 [K,N] in 0..255, stored zeros int32 [G,N] in 0..255) of packed tensors (numpy or torch, any device)."""
    qw = torch.as_tensor(np.asarray(qweight) if not torch.is_tensor(qweight) else qweight).to(torch.int32)
    qz = torch.as_tensor(np.asarray(qzeros) if not torch.is_tensor(qzeros) else qzeros).to(torch.int32)
    sh = torch.arange(4, dtype=torch.int32, device=qw.device) * 8
    q = ((qw.unsqueeze(1) >> sh.view(1, 4, 1)) & 255).reshape(qw.shape[0] * 4, qw.shape[1])
    z = ((qz.unsqueeze(2) >> sh.to(qz.device).view(1, 1, 4)) & 255).reshape(qz.shape[0], qz.shape[1] * 4)
    return q, z


def dequant8(qweight, qzeros, scales, g_idx, groupsize: int) -> torch.Tensor:
    """W[k,n] = (q[k,n] - (z[g(k),n] + 1)) * s[g(k),n] in fp32, [K,N]."""
    q, z = unpack8(qweight, qzeros)
    K = q.shape[0]
    if g_idx is None:
        gi = torch.arange(K, dtype=torch.int64) // groupsize
    else:
        gi = torch.as_tensor(np.asarray(g_idx) if not torch.is_tensor(g_idx) else g_idx).to(torch.int64)
    gi = gi.to(q.device)
    s = (scales if torch.is_tensor(scales) else torch.from_numpy(np.asarray(scales))).float().to(q.device)
    return (q - z[gi] - 1).float() * s[gi]


def quantize8(w_kn: torch.Tensor, groupsize: int, perm: Optional[np.ndarray] = None):
    """Asymmetric 8-bit min/max quantisation of W[K,N] per (group of rows, column) -> (qweight, qzeros, scales f16, g_idx)
    as numpy.  With `perm` the groups are formed in that row order (act-order): g_idx[perm[j]] = j // groupsize."""
    K, N = w_kn.shape
    G = K // groupsize
    src = w_kn if perm is None else w_kn[torch.from_numpy(perm)]
    w = src.float().view(G, groupsize, N)
    wmin = w.min(dim=1).values.clamp(max=0)
    wmax = w.max(dim=1).values.clamp(min=0)
    scale = ((wmax - wmin) / 255.0).clamp(min=1e-8).half().float()  # scales are stored in fp16
    zero = torch.round(-wmin / scale).clamp(1, 256)  # the stored (zero - 1) must fit a byte
    q = torch.clamp(torch.round(w / scale[:, None, :]) + zero[:, None, :], 0, 255).view(K, N).to(torch.uint8).numpy()
    g_idx = (np.arange(K) // groupsize).astype(np.int32)
    if perm is not None:
        qp = q
        q = np.empty_like(qp)
        q[perm] = qp
        g_idx = np.empty(K, dtype=np.int32)
        g_idx[perm] = (np.arange(K) // groupsize).astype(np.int32)
    qweight, qzeros = pack8(q, zero.to(torch.int32).numpy())
    return qweight, qzeros, scale.half().numpy(), g_idx


def tiny_llama8_tensors(cfg, seed: int, groupsize: int = 64, act_order: bool = False) -> Dict[str, torch.Tensor]:
    """oracle.tiny_models.tiny_llama_tensors with the seven projections of every layer quantised to 8 bits (same seeded
    dense weights; act-order: one row order per layer and input width, shared by the fused q/k/v and gate/up)."""
    from oracle.tiny_models import tiny_llama_tensors

    dense = tiny_llama_tensors(cfg, seed, quantize=None, dtype=torch.float32)
    g = torch.Generator().manual_seed(seed + 1000)
    t: Dict[str, torch.Tensor] = {}
    perms = {}
    for name, v in dense.items():
        if ".self_attn." in name or ".mlp." in name:
            base = name[:-len(".weight")]
            w_kn = v.t().contiguous()
            key = (name.split(".")[2], w_kn.shape[0])
            if act_order and key not in perms:
                perms[key] = torch.randperm(w_kn.shape[0], generator=g).numpy()
            qw, qz, sc, gi = quantize8(w_kn, groupsize, perms.get(key))
            t[f"{base}.qweight"], t[f"{base}.qzeros"] = torch.from_numpy(qw), torch.from_numpy(qz)
            t[f"{base}.scales"], t[f"{base}.g_idx"] = torch.from_numpy(sc), torch.from_numpy(gi)
        else:
            t[name] = v.to(torch.float16)
    return t


def dense_tensors(tensors: Dict[str, torch.Tensor], groupsize: int) -> Dict[str, torch.Tensor]:
    """A tiny 8-bit tensor dict -> the dense dict LlamaRef(..., quantize=None) runs (weights [N,K] fp32, dequantised)."""
    out = {}
    for name, v in tensors.items():
        if name.endswith(".qweight"):
            base = name[:-len(".qweight")]
            w = dequant8(v, tensors[f"{base}.qzeros"], tensors[f"{base}.scales"], tensors[f"{base}.g_idx"], groupsize)
            out[f"{base}.weight"] = w.t().contiguous()
        elif not name.endswith((".qzeros", ".scales", ".g_idx")):
            out[name] = v
    return out
