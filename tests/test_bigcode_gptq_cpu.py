"""CPU: the synthetic GPTQ GPT-BigCode tensors and the tensor-parallel slicing of a fused GPTQ `c_attn` (no GPU)."""
import hashlib

import numpy as np
import pytest
import torch

from tests import bigcode_gptq_ref as bref
from tests import gptq8_ref

from oracle import ops_ref

# sha256 over (name, dtype, shape, bytes) of every tensor in name order, of synthetic.bigcode_tensors as it was before it
# took `quantize`: (seed 3, bf16) and (seed 5, f16) at the small config below
DIGESTS = {(3, torch.bfloat16): "0c746354219236e24d3b3884c160eff65c67a22a9692118fadd9d7ef81a1a653",
           (5, torch.float16): "9926dea0a6a961ba27c7fee9b5d2c1bac2ccb33ae61042fe515bfd79fb813b6c"}


def _cfg():
    from tgis_amd.inference_engine.synthetic import BigCodeConfig

    return BigCodeConfig(vocab_size=128, hidden_size=128, n_inner=256, num_hidden_layers=2, num_attention_heads=4,
                         n_positions=64)


def _digest(t):
    h = hashlib.sha256()
    for name in sorted(t):
        v = t[name].contiguous()
        h.update(name.encode())
        h.update(str(v.dtype).encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(v.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def test_dense_output_is_what_it_was():
    from tgis_amd.inference_engine.synthetic import bigcode_tensors

    assert _digest(bigcode_tensors(_cfg(), 3)) == DIGESTS[(3, torch.bfloat16)]
    assert _digest(bigcode_tensors(_cfg(), 5, dtype=torch.float16)) == DIGESTS[(5, torch.float16)]
    assert _digest(bigcode_tensors(_cfg(), 5, dtype=torch.float16, quantize=None, groupsize=64, bits=8)) == \
        DIGESTS[(5, torch.float16)]


@pytest.mark.parametrize("bits", [4, 8])
def test_gptq_output_names_shapes_and_dtypes(bits):
    from tgis_amd.inference_engine.synthetic import bigcode_tensors

    cfg, gs = _cfg(), 64
    E, I, V, D, per = cfg.hidden_size, cfg.n_inner, cfg.vocab_size, cfg.hidden_size // cfg.num_attention_heads, 32 // bits
    t = bigcode_tensors(cfg, 9, dtype=torch.float16, quantize="gptq", groupsize=gs, bits=bits)
    want = {"transformer.wte.weight": ((V, E), torch.float16), "transformer.wpe.weight": ((cfg.n_positions, E), torch.float16)}
    for ln in ["transformer.ln_f"] + [f"transformer.h.{i}.{n}" for i in range(2) for n in ("ln_1", "ln_2")]:
        want[f"{ln}.weight"] = want[f"{ln}.bias"] = ((E,), torch.float16)
    for i in range(2):
        for name, n, k in (("attn.c_attn", E + 2 * D, E), ("attn.c_proj", E, E), ("mlp.c_fc", I, E), ("mlp.c_proj", E, I)):
            p = f"transformer.h.{i}.{name}"
            want[f"{p}.qweight"] = ((k // per, n), torch.int32)
            want[f"{p}.qzeros"] = ((k // gs, n // per), torch.int32)
            want[f"{p}.scales"] = ((k // gs, n), torch.float16)
            want[f"{p}.g_idx"] = ((k,), torch.int32)
            want[f"{p}.bias"] = ((n,), torch.float16)
    assert {k: (tuple(v.shape), v.dtype) for k, v in t.items()} == want
    # the recipe of llama_tensors: zero points centred on the mean code, groups of consecutive rows
    p = "transformer.h.1.mlp.c_fc"
    if bits == 4:
        z = (t[f"{p}.qzeros"].unsqueeze(2) >> (4 * torch.arange(8, dtype=torch.int32))) & 15
        assert int(z.min()) == 0 and int(z.max()) == 13
    else:
        _, z = gptq8_ref.unpack8(t[f"{p}.qweight"], t[f"{p}.qzeros"])
        assert int(z.min()) == 118 and int(z.max()) == 134
    assert torch.equal(t[f"{p}.g_idx"], torch.arange(E, dtype=torch.int32) // gs)


def _dequant(bits, qw, qz, sc, gi, gs):
    if bits == 4:
        return ops_ref.gptq_dequant(qw.numpy(), qz.numpy(), sc, np.asarray(gi), gs)
    return gptq8_ref.dequant8(qw, qz, sc, gi, gs)


@pytest.mark.parametrize("bits", [4, 8])
def test_c_attn_shards_hold_their_q_columns_and_the_whole_kv_head(bits):
    """World size 2: each rank's (qweight, qzeros, scales, bias) slices dequantise to its q columns of the full matrix
    followed by the k / v columns, which both ranks hold."""
    from oracle.tiny_models import TinyBigCodeConfig
    from tgis_amd.models.custom_modeling.flash_santacoder_modeling import _shard_q_keep_kv, shard_mqa_gptq

    cfg = TinyBigCodeConfig()
    E, D = cfg.hidden_size, cfg.hidden_size // cfg.num_attention_heads
    t = bref.tiny_bigcode_gptq_tensors(cfg, 13, bits=bits)
    p = "transformer.h.0.attn.c_attn"
    qw, qz, sc, gi, bias = (t[f"{p}.{n}"] for n in ("qweight", "qzeros", "scales", "g_idx", "bias"))
    full = _dequant(bits, qw, qz, sc, gi, bref.GS)
    assert full.shape == (E, E + 2 * D)
    world, parts, biases = 2, [], []
    for rank in range(world):
        sq, sz, ss = shard_mqa_gptq(qw, qz, sc, D, bits, rank, world)
        assert sq.shape[1] == ss.shape[1] == E // world + 2 * D and sz.shape[1] * (32 // bits) == sq.shape[1]
        parts.append(_dequant(bits, sq, sz, ss, gi, bref.GS))
        biases.append(_shard_q_keep_kv(bias, 0, D, rank, world))
    q = torch.cat([w[:, :E // world] for w in parts], dim=1)
    assert torch.equal(q, full[:, :E])
    assert torch.equal(torch.cat([b[:E // world] for b in biases]), bias[:E])
    for w, b in zip(parts, biases):
        assert torch.equal(w[:, E // world:], full[:, E:])
        assert torch.equal(b[E // world:], bias[E:])
