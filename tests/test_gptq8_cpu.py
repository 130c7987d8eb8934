"""CPU: the 8-bit GPTQ format above the kernels — the packer and dequantiser of tests/gptq8_ref.py pinned bit for bit to
the reference's own (tests/golden/gptq8_pack_reference.npz, made by tests/golden/make_gptq8_fixture.py), get_linear's
dispatch on the width, and the tensor-parallel loader under gloo world size 2: every rank's column and row bundles
(plain and act-order, whose row shards are regrouped and padded) dequantise to the matching slices of the full matrix."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gptq8_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gptq8_pack_reference.npz")


def test_pack8_and_dequant8_match_the_reference_packer():
    f = np.load(GOLDEN)
    intw, zeros = f["intw"], f["zeros"]
    assert intw.min() == 0 and intw.max() == 255 and zeros.min() == 1 and zeros.max() == 256  # the extremes are in
    qweight, qzeros = gptq8_ref.pack8(intw, zeros)
    assert qweight.dtype == f["qweight"].dtype and np.array_equal(qweight, f["qweight"])
    assert qzeros.dtype == f["qzeros"].dtype and np.array_equal(qzeros, f["qzeros"])
    q, z = gptq8_ref.unpack8(f["qweight"], f["qzeros"])
    assert np.array_equal(q.numpy(), intw.astype(np.int32)) and np.array_equal(z.numpy() + 1, zeros)
    K = intw.shape[0]
    gs = K // zeros.shape[0]
    for g_idx in (None, (np.arange(K) // gs).astype(np.int32)):
        w = gptq8_ref.dequant8(f["qweight"], f["qzeros"], f["ref_scales"], g_idx, gs)
        assert w.dtype == torch.float32 and np.array_equal(w.numpy().view(np.uint32), f["dequant"].view(np.uint32))
    # a stored 255 is a zero point of 256: z + 1 is not masked back to a byte
    col = int(np.argwhere(zeros[1] == 256)[0, 0])
    assert float(w[K - 1, col]) == (float(intw[K - 1, col]) - 256.0) * float(f["ref_scales"][1, col])


def test_quantize8_round_trips_within_the_grid_error():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(128, 32, generator=g) * 0.05
    perm = torch.randperm(128, generator=g).numpy()
    for p in (None, perm):
        qw, qz, sc, gi = gptq8_ref.quantize8(w, 32, p)
        back = gptq8_ref.dequant8(qw, qz, sc, gi, 32)
        step = torch.from_numpy(sc).float()[torch.from_numpy(gi).long()]
        # half a step of rounding, half a step by which the rounded zero point shifts the grid (clamped at its ends), and
        # the f16 rounding of the scale over at most 255 steps: 255 * 2^-11 < 0.125 step
        assert ((back - w).abs() <= 1.125 * step + 1e-7).all()


@pytest.mark.parametrize("bits", [2, 3])
def test_get_linear_refuses_other_widths_at_construction(bits):
    from tgis_amd.utils.layers import get_linear

    K, N = 64, 32
    bundle = (torch.zeros((K * bits // 32, N), dtype=torch.int32), torch.zeros((1, N * bits // 32), dtype=torch.int32),
              torch.ones((1, N), dtype=torch.float16), None, bits, K, False)
    with pytest.raises(NotImplementedError, match="Only 4 and 8 bits are supported."):
        get_linear(bundle, None, "gptq")


def test_get_linear_dispatches_on_bits():
    from tgis_amd.utils.layers import Ex4bitLinearV2, Gptq8Linear, get_linear

    K, N = 64, 32
    for bits, cls in ((4, Ex4bitLinearV2), (8, Gptq8Linear)):
        bundle = (torch.zeros((K * bits // 32, N), dtype=torch.int32), torch.zeros((1, N * bits // 32), dtype=torch.int32),
                  torch.ones((1, N), dtype=torch.float16), None, bits, K, bits == 4)
        lin = get_linear(bundle, None, "gptq")
        assert type(lin) is cls and (lin.height, lin.width) == (K, N)


def _linear(kind, K=128, N=192):
    from tgis_amd.utils.layers import get_linear

    if kind == "dense":
        return get_linear(torch.zeros((N, K), dtype=torch.float16), None, None)
    bits = {"int4": 4, "int8": 8}[kind]
    bundle = (torch.zeros((K * bits // 32, N), dtype=torch.int32), torch.zeros((1, N * bits // 32), dtype=torch.int32),
              torch.ones((1, N), dtype=torch.float16), None, bits, K, bits == 4)
    return get_linear(bundle, None, "gptq")


def test_8bit_linears_offer_none_of_the_fused_forms(monkeypatch):
    """The models must take their generic paths for 8 bits: through the Linear protocol an 8-bit linear refuses every fused
    form.  The same questions to an int4 and a dense linear (kernels replaced by tests/cpu_backend.py, and a library that
    would serve fragments) are answered with yes, so the refusals are the 8-bit class's own."""
    from tests import cpu_backend
    from tgis_amd import native
    from tgis_amd.utils.layers import Linear

    cpu_backend.install(monkeypatch)
    monkeypatch.setattr(native, "gptq_fragments_ok", lambda M, w, act=0: True)
    cases = [(rows, act) for rows in (1, 32, 64) for act in (0, 2, 3)]

    lin8 = _linear("int8")
    assert isinstance(lin8, Linear) and callable(lin8.post_init)
    assert lin8.fuse_gate_up() is False
    lin8.declare_rope_heads(1, 1, 64)
    assert lin8.rope_handle is None and not any(lin8.rope_serves(rows) for rows in (1, 32, 64))
    assert all(lin8.wants_fragments(rows, act) is False for rows, act in cases)
    assert lin8.q_handle is None  # none of the questions needed the image

    lin4 = _linear("int4")
    assert lin4.fuse_gate_up() is True
    lin4.declare_rope_heads(1, 1, 64)
    lin4.post_init()
    lin4.post_init()  # idempotent: the checkpoint tensors are gone after the first
    assert lin4.rope_handle is not None and all(lin4.rope_serves(rows) for rows in (1, 32, 64))
    assert not lin4.rope_serves(65)
    assert all(lin4.wants_fragments(rows, act) is True for rows, act in cases) and not lin4.wants_fragments(65)

    dense = _linear("dense")
    assert dense.fuse_gate_up() is True and dense.prepared.flags == 1
    dense.declare_rope_heads(1, 1, 64)
    dense.post_init()
    assert dense.rope_handle is not None and dense.rope_serves(32) and not dense.rope_serves(65)
    assert all(dense.wants_fragments(rows, act) is False for rows, act in cases)  # fragment order is an int4 operand layout


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


K_, N_, GS_ = 256, 64, 64


def _tensors(act_order: bool):
    g = torch.Generator().manual_seed(11 + act_order)
    t = {}
    perm = torch.randperm(K_, generator=g).numpy() if act_order else None
    for name in ("a", "b"):
        qw, qz, sc, gi = gptq8_ref.quantize8(torch.randn(K_, N_, generator=g) * 0.05, GS_, perm)
        t.update({f"{name}.qweight": torch.from_numpy(qw), f"{name}.qzeros": torch.from_numpy(qz),
                  f"{name}.scales": torch.from_numpy(sc), f"{name}.g_idx": torch.from_numpy(gi)})
    return t


def _shard_dequant(bundle):
    """(W [rows of the rank's activation, N] fp32) of a loader bundle; the explicit-perm form is scattered back."""
    qw, qz, sc, gi, bits, gs, use = bundle
    assert bits == 8 and not use
    if isinstance(gi, tuple):  # ("perm", gather index with -1 pads, activation columns)
        _, perm, rows = gi
        w_img = gptq8_ref.dequant8(qw, qz, sc, None, gs)
        w = torch.zeros((rows, qw.shape[1]))
        keep = perm >= 0
        w[perm[keep].long()] = w_img[keep]
        assert int(keep.sum()) == rows
        return w
    return gptq8_ref.dequant8(qw, qz, sc, gi, gs if gs > 0 else qw.shape[0] * 4)


def _loader_worker(rank, world, port, act_order, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tgis_amd.utils.dist import initialize_torch_distributed
    from tgis_amd.utils.weights import DictWeights

    torch.set_num_threads(2)
    pg = initialize_torch_distributed(world, rank)
    assert pg.size() == world
    w = DictWeights(_tensors(act_order), torch.device("cpu"), torch.float16, pg)
    w.gptq_bits, w.gptq_groupsize = 8, GS_
    col = w.get_multi_weights_col(["a", "b"], "gptq", 0)
    row = w.get_multi_weights_row("a", "gptq")
    ret[rank] = (_shard_dequant(col), _shard_dequant(row), row[0].shape[0] * 4)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("act_order", [False, True])
def test_loader_world2_shards_dequantise_to_slices_of_the_full_matrix(act_order):
    mgr = mp.get_context("spawn").Manager()
    ret = mgr.dict()
    mp.spawn(_loader_worker, args=(2, _free_port(), act_order, ret), nprocs=2, join=True)
    t = _tensors(act_order)
    full = {n: gptq8_ref.dequant8(t[f"{n}.qweight"], t[f"{n}.qzeros"], t[f"{n}.scales"], t[f"{n}.g_idx"], GS_) for n in "ab"}
    half_n, half_k = N_ // 2, K_ // 2
    for rank in (0, 1):
        col, row, image_rows = ret[rank]
        want_col = torch.cat([full[n][:, rank * half_n:(rank + 1) * half_n] for n in "ab"], dim=1)
        assert torch.equal(col, want_col), f"rank {rank}: column shard"
        assert torch.equal(row, full["a"][rank * half_k:(rank + 1) * half_k]), f"rank {rank}: row shard"
        assert (image_rows > half_k) == act_order  # act-order row shards are padded per group
