"""GPTQ Mixtral, the parts that need no GPU: what the loader hands out for every expert, whole and as a shard of two (the
column shards of w1 | w3, the row shards of w2, a group that straddles the rank boundary and is regrouped), and the refusals."""
import types

import numpy as np
import pytest
import torch

from oracle import ops_ref
from oracle.tiny_models import quantize_gptq
from tests import mixtral_gptq_tiny as mg
from tests.mixtral_tiny import TinyMixtralConfig, fused_names, tiny_mixtral_tensors

CPU = torch.device("cpu")


def _weights(tensors, rank, world, bits=4, groupsize=mg.GS):
    from tgis_amd.utils.dist import FakeGroup
    from tgis_amd.utils.weights import DictWeights

    w = DictWeights(tensors, CPU, torch.float16, FakeGroup(rank, world))
    w.gptq_bits, w.gptq_groupsize = bits, groupsize
    return w


def _dequant(bundle):
    qweight, qzeros, scales, g_idx, bits, groupsize = bundle
    assert bits == 4 and groupsize == qweight.shape[0] * 8 // qzeros.shape[0]
    gi = None if g_idx is None else g_idx.numpy()
    return ops_ref.gptq_dequant(qweight.numpy(), qzeros.numpy(), scales, gi, groupsize)


@pytest.fixture(scope="module")
def tiny():
    cfg = TinyMixtralConfig()
    return cfg, mg.tiny_mixtral_gptq_tensors(cfg, 3)


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_expert_bundles_dequantise_to_the_shards_of_the_whole_matrices(tiny, rank, world):
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors

    cfg, tensors = tiny
    I, Il = cfg.intermediate_size, cfg.intermediate_size // world
    lo = rank * Il
    for layer in range(cfg.num_hidden_layers):
        et = ExpertTensors(f"model.layers.{layer}", _weights(tensors, rank, world), I, "gptq")
        assert et.published and torch.equal(et.router(), tensors[f"model.layers.{layer}.block_sparse_moe.gate.weight"])
        for e in range(cfg.num_local_experts):
            p = f"model.layers.{layer}.block_sparse_moe.experts.{e}"
            w1, w3, w2 = (ops_ref.gptq_dequant(tensors[f"{p}.{n}.qweight"].numpy(), tensors[f"{p}.{n}.qzeros"].numpy(),
                                               tensors[f"{p}.{n}.scales"], None, mg.GS) for n in ("w1", "w3", "w2"))
            gu = _dequant(et.gate_up_gptq(e))
            assert gu.shape == (cfg.hidden_size, 2 * Il)
            assert torch.equal(gu[:, :Il], w1[:, lo:lo + Il]) and torch.equal(gu[:, Il:], w3[:, lo:lo + Il])
            dn = _dequant(et.down_gptq(e))
            assert dn.shape == (Il, cfg.hidden_size) and torch.equal(dn, w2[lo:lo + Il])


def _small_layer(hidden, I, gs, E=2, seed=0, act_order_expert=None):
    """One layer's router and GPTQ experts under the published names."""
    g = torch.Generator().manual_seed(seed)
    t, p = {}, "model.layers.0.block_sparse_moe"
    t[f"{p}.gate.weight"] = torch.randn(E, hidden, generator=g).half()
    for e in range(E):
        for name, n, k in (("w1", I, hidden), ("w3", I, hidden), ("w2", hidden, I)):
            w = (torch.randn(k, n, generator=g) * k ** -0.5)
            perm = np.random.default_rng(k).permutation(k) if e == act_order_expert else None
            qw, qz, sc, gi = quantize_gptq(w, gs, perm)
            for key, v in (("qweight", qw), ("qzeros", qz), ("scales", sc), ("g_idx", gi)):
                t[f"{p}.experts.{e}.{name}.{key}"] = torch.from_numpy(v)
    return t


@pytest.mark.parametrize("rank", (0, 1))
def test_a_group_that_straddles_the_rank_boundary_is_regrouped(rank):
    """I 384 at group size 128 over two ranks: 192 rows of w2 per rank are 1.5 groups, regrouped into sub-groups of 64 rows
    that carry their parent's scale and zero point — the same values, in a size the kernels serve."""
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors

    hidden, I, gs = 256, 384, 128
    tensors = _small_layer(hidden, I, gs)
    et = ExpertTensors("model.layers.0", _weights(tensors, rank, 2, groupsize=gs), I, "gptq")
    for e in range(2):
        p = f"model.layers.0.block_sparse_moe.experts.{e}.w2"
        whole = ops_ref.gptq_dequant(tensors[f"{p}.qweight"].numpy(), tensors[f"{p}.qzeros"].numpy(),
                                     tensors[f"{p}.scales"], None, gs)
        bundle = et.down_gptq(e)
        assert bundle[5] == 64 and bundle[1].shape[0] == 3
        assert torch.equal(_dequant(bundle), whole[rank * 192:(rank + 1) * 192])
        assert et.gate_up_gptq(e)[5] == gs  # the column shards keep the checkpoint's groups


def test_a_regrouped_size_outside_the_kernels_set_is_refused_by_name():
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors

    tensors = _small_layer(256, 192, 64)  # 96 rows per rank: sub-groups of gcd(64, 96) = 32 rows
    et = ExpertTensors("model.layers.0", _weights(tensors, 1, 2, groupsize=64), 192, "gptq")
    with pytest.raises(NotImplementedError, match=r"Mixtral.*GPTQ.*model\.layers\.0\.block_sparse_moe\.experts\.0\.w2"):
        et.down_gptq(0)


def _config(**over):
    ns = types.SimpleNamespace(model_type="mixtral", quantize="gptq", **TinyMixtralConfig().to_dict())
    for k, v in over.items():
        setattr(ns, k, v)
    return ns


def test_config_check_admits_what_has_a_kernel_and_refuses_the_rest():
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import (FlashMixtralForCausalLM, check_mixtral_config,
                                                                         gptq_params_of)

    for params in ((4, 128), (4, 64), (4, -1)):
        assert check_mixtral_config(_config(), "gptq", params) == (8, 2)
    for params in ((8, 128), (4, 32), (3, 128), None):
        with pytest.raises(NotImplementedError, match="Mixtral.*GPTQ"):
            check_mixtral_config(_config(), "gptq", params)
    # the parameters come from the weights object, tolerantly: one that does not know them is refused before any read
    assert gptq_params_of(object()) is None
    assert gptq_params_of(_weights({}, 0, 1, groupsize=128)) == (4, 128)
    unknown = _weights({}, 0, 1, bits=None, groupsize=None)
    assert gptq_params_of(unknown) is None
    for weights, _ in ((unknown, "unknown"), (_weights({}, 0, 1, bits=8), "8 bits"), (_weights({}, 0, 1, groupsize=32), "32")):
        with pytest.raises(NotImplementedError, match="Mixtral.*GPTQ"):
            FlashMixtralForCausalLM(_config(), weights)  # an empty dict: any read would raise another error


def test_an_act_order_expert_is_refused_by_name():
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors

    tensors = _small_layer(256, 128, 64, act_order_expert=1)
    et = ExpertTensors("model.layers.0", _weights(tensors, 0, 1), 128, "gptq")
    et.gate_up_gptq(0), et.down_gptq(0)  # expert 0 is in natural order
    with pytest.raises(NotImplementedError, match=r"Mixtral.*GPTQ.*experts\.1\.w1.*act-order"):
        et.gate_up_gptq(1)
    with pytest.raises(NotImplementedError, match=r"Mixtral.*GPTQ.*experts\.1\.w2.*act-order"):
        et.down_gptq(1)


def test_the_fused_naming_is_refused():
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import ExpertTensors

    cfg = TinyMixtralConfig()
    fused = fused_names(tiny_mixtral_tensors(cfg, 3), cfg)
    with pytest.raises(NotImplementedError, match="Mixtral.*GPTQ.*fused"):
        ExpertTensors("model.layers.0", _weights(fused, 0, 1), cfg.intermediate_size, "gptq")
    # the same names load as before without quantisation
    assert not ExpertTensors("model.layers.0", _weights(fused, 0, 1), cfg.intermediate_size).published
