"""CPU, two gloo ranks: what tensor-parallel ranks agree on when a model is built (utils/rank_group.py, and the two rendezvous
in utils/kv_cache.py that use it).  The invariant under test is that every rank issues the same sequence of collectives on
every path, error paths included: a rank that skipped or added one would leave its peer waiting, so a worker that is still
alive after its join (or that left with the collective timeout) fails the test."""
import os
import sys
import types

import pytest
import torch
import torch.multiprocessing as mp

from tests.test_tp_gloo import _free_port
from tgis_amd.utils.dist import FakeGroup
from tgis_amd.utils.kv_cache import KV_SCALES_FILE, kv_scales_stats, save_kv_scales
from tgis_amd.utils.rank_group import RankGroup


def _rank_main(rank, world, port, case, args, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_TIMEOUT_S="30")
    for var in ("TGIS_KV_CACHE_DTYPE", "TGIS_KV_SCALES"):
        os.environ.pop(var, None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tgis_amd.utils.dist import initialize_torch_distributed

    pg = initialize_torch_distributed(world, rank)
    group = RankGroup(types.SimpleNamespace(process_group=pg, world_size=world, rank=rank), torch.device("cpu"))
    assert group.real and group.device == torch.device("cpu")
    try:
        ret[rank] = globals()[case](group, *args)
    except (ValueError, OSError) as e:
        ret[rank] = ("raised", type(e).__name__, str(e))
    torch.distributed.destroy_process_group()


def _on_two_ranks(case, *args):
    """{rank: what `case(group, *args)` returned, or ("raised", type, message)} from two gloo ranks."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        port = _free_port()
        procs = [ctx.Process(target=_rank_main, args=(r, 2, port, case, args, ret)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(60)
        hung = [r for r, p in enumerate(procs) if p.is_alive()]
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(10)
        assert not hung, f"ranks {hung} were still waiting: the ranks' sequences of collectives differ"
        assert [p.exitcode for p in procs] == [0, 0]
        return dict(ret)


# ---- RankGroup ---------------------------------------------------------------------------------------------------------
def _primitives(group):
    r = group.rank
    return {
        "max_int": group.max_int(10 + r),
        "all_true": [group.all_true(True), group.all_true(r == 0), group.all_true(r == 1), group.all_true(False)],
        "values": group.broadcast_from_rank0([0.1, 2.5, -3.0] if r == 0 else None, 3),
        "none": group.broadcast_from_rank0(None if r == 0 else [9.0, 9.0, 9.0], 3),
        "pair": group.broadcast_int64_pair(*((0xFFFFFFFF, 7) if r == 0 else (1, 2))),
        "max_reduce": group.max_reduce(torch.tensor([[1.0, 5.0], [3.0, 0.5]]) if r == 0
                                       else torch.tensor([[2.0, 4.0], [-1.0, 0.75]])).tolist(),
    }


def test_rank_group_reduces_and_broadcasts_on_two_ranks():
    got = _on_two_ranks("_primitives")
    want = {"max_int": 11, "all_true": [True, False, False, False], "values": [0.1, 2.5, -3.0], "none": None,
            "pair": (0xFFFFFFFF, 7), "max_reduce": [[2.0, 5.0], [3.0, 0.75]]}
    assert got == {0: want, 1: want}


@pytest.mark.parametrize("engine", [types.SimpleNamespace(world_size=2, rank=0, process_group=FakeGroup(0, 2)),
                                    types.SimpleNamespace(world_size=1, rank=0, process_group=FakeGroup(0, 1)), object()],
                         ids=["fake-group-of-two", "world-of-one", "bare-engine"])
def test_rank_group_is_the_identity_without_a_real_group(engine):
    """One rank, and a FakeGroup standing in for a rank of several: every method hands the caller's value back."""
    group = RankGroup(engine, torch.device("cpu"))
    assert not group.real and not group.nccl and group.rank == 0
    assert group.world == getattr(engine, "world_size", 1) and group.process_group is getattr(engine, "process_group", None)
    assert group.min_int(5) == 5 and group.max_int(-7) == -7
    assert group.all_true(True) is True and group.all_true(False) is False
    values = [0.5, 2.0]
    assert group.broadcast_from_rank0(values, 2) is values and group.broadcast_from_rank0(None, 2) is None
    assert group.broadcast_int64_pair(3, 1 << 40) == (3, 1 << 40)
    t = torch.tensor([1.0, 2.0])
    assert group.max_reduce(t) is t
    assert group.fail_together(None, "peer") is None
    error = OSError("mine")
    with pytest.raises(OSError) as exc:
        group.fail_together(error, "peer")
    assert exc.value is error


# ---- the KV cache dtype --------------------------------------------------------------------------------------------------
def _dtype(group, values):
    from tgis_amd.utils.kv_cache import agree_kv_cache_dtype

    return agree_kv_cache_dtype(group, values[group.rank])


def test_ranks_agree_on_the_kv_cache_dtype():
    assert _on_two_ranks("_dtype", ("fp8_e4m3", "FP8_E4M3")) == {0: "fp8_e4m3", 1: "fp8_e4m3"}


def test_a_rank_with_an_unsupported_kv_cache_dtype_fails_both():
    got = _on_two_ranks("_dtype", ("fp8_e4m3", "fp9"))
    assert got[1] == ("raised", "ValueError", "KV cache dtype 'fp9' is not supported (one of auto, fp8_e4m3)")
    assert got[0] == ("raised", "ValueError",
                      "another tensor-parallel rank was given an unsupported KV cache dtype (TGIS_KV_CACHE_DTYPE)")


def test_ranks_that_disagree_on_the_kv_cache_dtype_fail_both():
    got = _on_two_ranks("_dtype", ("auto", "fp8_e4m3"))
    for rank, mine in enumerate(("auto", "fp8_e4m3")):
        kind, typ, message = got[rank]
        assert (kind, typ) == ("raised", "ValueError")
        assert message == (f"tensor-parallel ranks disagree on the KV cache dtype (this rank: {mine}; ranks use auto and "
                           f"fp8_e4m3): set TGIS_KV_CACHE_DTYPE alike on every rank")


# ---- the KV cache scales (two layers) ---------------------------------------------------------------------------------------
def _scales(group, kv_scales, kv_dtype, model_dirs):
    from tgis_amd.utils.kv_cache import agree_kv_scales

    return agree_kv_scales(group, kv_scales, kv_dtype, 2, model_dirs[group.rank])


def _model_dirs(tmp_path):
    dirs = [tmp_path / "rank0", tmp_path / "rank1"]
    for d in dirs:
        d.mkdir()
    return dirs, tuple(str(d) for d in dirs)


def test_every_rank_gets_the_scales_rank_0_found(tmp_path):
    dirs, names = _model_dirs(tmp_path)
    stats = [kv_scales_stats([k * 100.0, k * 3.0], [k, k * 0.01], tokens=1, model_dtype="float16") for k in (1.0, 64.0)]
    for d, st in zip(dirs, stats):  # rank 1 has a file of its own, with other scales: it is not the one that counts
        save_kv_scales(st, str(d / KV_SCALES_FILE))
    want = (stats[0]["k_scale"], stats[0]["v_scale"])
    assert want != (stats[1]["k_scale"], stats[1]["v_scale"])
    assert _on_two_ranks("_scales", None, "fp8_e4m3", names) == {0: want, 1: want}


def test_no_scale_file_means_none_on_every_rank(tmp_path):
    _, names = _model_dirs(tmp_path)
    assert _on_two_ranks("_scales", None, "fp8_e4m3", names) == {0: None, 1: None}


def test_a_scale_file_rank_0_cannot_read_fails_both(tmp_path):
    dirs, names = _model_dirs(tmp_path)
    (dirs[0] / KV_SCALES_FILE).write_text("{ not json")
    got = _on_two_ranks("_scales", None, "fp8_e4m3", names)
    assert got[0][:2] == ("raised", "ValueError") and "is not JSON" in got[0][2]
    assert got[1] == ("raised", "ValueError", "another tensor-parallel rank could not resolve the KV cache scales")


def test_explicit_scales_with_a_16_bit_cache_fail_every_rank(tmp_path):
    _, names = _model_dirs(tmp_path)
    stats = kv_scales_stats([100.0, 3.0], [1.0, 0.01], tokens=1, model_dtype="float16")
    got = _on_two_ranks("_scales", stats, "auto", names)
    for rank in (0, 1):
        assert got[rank][:2] == ("raised", "ValueError") and "16-bit" in got[rank][2]
