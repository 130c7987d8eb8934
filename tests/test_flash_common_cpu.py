"""The one place where the Llama, GPT-NeoX and Santacoder forwards reach the paged cache (flash_common.write_kv / attend):
which native entry point is called, in which order and with which arguments.  A recording stub stands in for tgis_amd.native,
so nothing here needs a GPU."""
import pytest
import torch

from tgis_amd import native
from tgis_amd.models.custom_modeling import flash_common
from tgis_amd.utils import layers
from tgis_amd.utils.kv_cache import PagedKVCache

H, HKV, D, ROT = 4, 2, 64, 32
LAYER = 1  # of 2: a helper that read layer 0's pools or scales would be caught
SCALE = D ** -0.5
WS_BYTES = 777_000_001  # what the stubbed attn_workspace_bytes answers: more than a Workspace holds to begin with


class Recorder:
    """Stands in for the native calls the helpers make; `calls` is [(name, args, kwargs)] in call order."""

    def __init__(self, monkeypatch):
        self.calls = []
        rec = self

        class Workspace:
            def __init__(self, nbytes, device):
                rec.calls.append(("Workspace", (nbytes, device), {}))

            def ensure(self, nbytes):
                rec.calls.append(("ensure", (nbytes,), {}))

        def record(name, result):
            def fn(*args, **kwargs):
                self.calls.append((name, args, kwargs))
                return result(args)
            monkeypatch.setattr(native, name, fn)

        record("rope_kv_write", lambda a: a[0] if isinstance(a[0], torch.Tensor) else
               torch.zeros(a[0].shape, dtype=torch.float16))
        record("rope_kv_write_prefill", lambda a: a[0])
        record("attn_paged", lambda a: a[7])
        record("attn_workspace_bytes", lambda a: WS_BYTES)
        monkeypatch.setattr(native, "Workspace", Workspace)
        monkeypatch.setattr(layers, "_WORKSPACES", {})

    def names(self):
        return [c[0] for c in self.calls]

    def only(self, name):
        (call,) = [c for c in self.calls if c[0] == name]
        return call[1], call[2]


@pytest.fixture
def rec(monkeypatch):
    return Recorder(monkeypatch)


def make(kv_dtype="auto", q=(3, 2), ctx=None, **kw):
    """Two sequences with `q` new tokens each, `ctx` tokens in the cache after this forward (default: the new ones only)."""
    cache = PagedKVCache(2, HKV, D, 4, torch.float16, "cpu", kv_dtype=kv_dtype)
    cache.k_scales[LAYER], cache.v_scales[LAYER] = 0.5, 2.0
    ctx = ctx or q
    T = sum(q)
    cu = torch.tensor([0, q[0], T], dtype=torch.int32)
    kv = flash_common.KVArgs(cache=cache, block_tables=torch.tensor([[0, 1], [2, 3]], dtype=torch.int32),
                             ctx_lens=torch.tensor(ctx, dtype=torch.int32), slots=torch.arange(T, dtype=torch.int32),
                             max_q_len=max(q), max_ctx=max(ctx), **kw)
    qkv = torch.zeros((T, (H + 2 * HKV) * D), dtype=torch.float16)
    cos, sin = torch.ones((64, ROT // 2), dtype=torch.float16), torch.zeros((64, ROT // 2), dtype=torch.float16)
    pos = torch.arange(T, dtype=torch.int32)
    return cache, kv, qkv, cos, sin, pos, cu


def same(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.dtype == b.dtype


def write(kv, qkv, cos, sin, pos, cu):
    return flash_common.write_kv(qkv, kv, LAYER, H, HKV, D, ROT, cos, sin, pos, cu)


def attend(kv, qkv, cu, **kw):
    return flash_common.attend(qkv, kv, LAYER, H, HKV, D, SCALE, cu, **kw)


def check_attn_args(args, cache, kv, qkv, cu, out, ws):
    assert args[0] is qkv and args[1] == qkv.stride(0)
    assert same(args[2], cache.k_pool(LAYER)) and same(args[3], cache.v_pool(LAYER))
    assert args[4] is kv.block_tables and args[5] is kv.ctx_lens and args[6] is cu and args[7] is out
    assert args[8:16] == (2, H, HKV, D, kv.max_q_len, kv.max_ctx, SCALE, kv.num_splits)
    assert args[16] is ws and len(args) == 17


def test_fresh_prefill_writes_page_wise_and_takes_no_workspace(rec):
    cache, kv, qkv, cos, sin, pos, cu = make(fresh_prefill=True)
    got = write(kv, qkv, cos, sin, pos, cu)
    out = attend(kv, got, cu)
    assert rec.names() == ["rope_kv_write_prefill", "attn_paged"]
    args, kwargs = rec.only("rope_kv_write_prefill")
    assert got is qkv and args[0] is qkv and args[1] is cos and args[2] is sin and args[3] is pos and args[4] is cu
    assert args[5] is kv.block_tables and same(args[6], cache.k_pool(LAYER)) and same(args[7], cache.v_pool(LAYER))
    assert args[8:] == (kv.max_q_len, H, HKV, D, ROT) and kwargs == {}
    args, kwargs = rec.only("attn_paged")
    assert isinstance(out, torch.Tensor) and out.shape == (5, H * D) and out.dtype == qkv.dtype
    check_attn_args(args, cache, kv, qkv, cu, out, None)
    assert kwargs == {}


def test_prefill_onto_an_existing_context_writes_per_token(rec):
    cache, kv, qkv, cos, sin, pos, cu = make(q=(3, 2), ctx=(40, 33))  # 3 and 2 new tokens behind 37 and 31 cached ones
    got = write(kv, qkv, cos, sin, pos, cu)
    assert rec.names() == ["rope_kv_write"]
    args, kwargs = rec.only("rope_kv_write")
    assert got is args[0] and args[1] is cos and args[2] is sin and args[4] is kv.slots
    assert same(args[5], cache.k_pool(LAYER)) and same(args[6], cache.v_pool(LAYER))
    assert args[7:] == (H, HKV, D, ROT) and kwargs == {}


@pytest.mark.parametrize("fresh", [False, True])
def test_a_partial_is_always_written_per_token(rec, fresh):
    """The per-token kernel is the one that finishes a split-K sum, whatever `fresh_prefill` says."""
    cache, kv, qkv, cos, sin, pos, cu = make(q=(9, 4) if fresh else (1, 1), ctx=(9, 4), fresh_prefill=fresh)
    T = qkv.shape[0]
    part = native.Partial(torch.zeros(8, dtype=torch.float32), 2, qkv.shape[1], T, qkv.shape[1], None)
    got = write(kv, part, cos, sin, pos, cu)
    assert rec.names() == ["rope_kv_write"]
    args, kwargs = rec.only("rope_kv_write")
    assert args[0] is part and args[3] is pos and args[4] is kv.slots and args[7:] == (H, HKV, D, ROT) and kwargs == {}
    assert isinstance(got, torch.Tensor) and got.shape == (T, qkv.shape[1])  # the materialised activation goes on


def test_no_rotary_passes_none_through(rec):
    """Santacoder: cos = sin = position_ids = None, one kv head, rot_dim = D."""
    cache, kv, qkv, _, _, _, cu = make(fresh_prefill=True)
    flash_common.write_kv(qkv, kv, LAYER, H, 1, D, D, None, None, None, cu)
    kv.fresh_prefill = False
    flash_common.write_kv(qkv, kv, LAYER, H, 1, D, D, None, None, None, cu)
    assert rec.names() == ["rope_kv_write_prefill", "rope_kv_write"]
    assert rec.calls[0][1][1:4] == (None, None, None) and rec.calls[0][1][9:] == (H, 1, D, D)
    assert rec.calls[1][1][1:4] == (None, None, None) and rec.calls[1][1][7:] == (H, 1, D, D)


def test_split_decode_ensures_the_workspace_before_attention(rec):
    cache, kv, qkv, cos, sin, pos, cu = make(q=(1, 1), ctx=(40, 33), num_splits=4)
    out = attend(kv, qkv, cu)
    assert rec.names() == ["Workspace", "attn_workspace_bytes", "ensure", "attn_paged"]
    assert rec.only("attn_workspace_bytes") == ((2, H, HKV, D, 4), {})
    assert rec.only("ensure") == ((WS_BYTES,), {})
    args, kwargs = rec.only("attn_paged")
    assert isinstance(args[16], native.Workspace) and args[16] is layers.workspace(qkv.device)
    check_attn_args(args, cache, kv, qkv, cu, out, args[16])
    assert kwargs == {}


def test_frag_out_hands_attention_a_fragment_order_output(rec):
    cache, kv, qkv, cos, sin, pos, cu = make(q=(1, 1), ctx=(40, 33))
    out = attend(kv, qkv, cu, frag_out=True)
    assert isinstance(out, native.FragAct) and out.shape == (2, H * D) and out.dtype == torch.float16
    assert rec.names() == ["attn_paged"]
    check_attn_args(rec.only("attn_paged")[0], cache, kv, qkv, cu, out, None)


@pytest.mark.parametrize("fresh", [False, True])
def test_fp8_cache_passes_the_layers_scales_to_writer_and_attention(rec, fresh):
    cache, kv, qkv, cos, sin, pos, cu = make("fp8_e4m3", fresh_prefill=fresh)
    assert cache.scales(LAYER) == (0.5, 2.0) != cache.scales(0)
    attend(kv, write(kv, qkv, cos, sin, pos, cu), cu)
    writer = "rope_kv_write_prefill" if fresh else "rope_kv_write"
    assert rec.names() == [writer, "attn_paged"]
    for name in (writer, "attn_paged"):
        args, kwargs = rec.only(name)
        assert kwargs == {"kv_scales": cache.scales(LAYER)}
        assert any(isinstance(a, torch.Tensor) and a.dtype == torch.uint8 and same(a, cache.k_pool(LAYER)) for a in args)


@pytest.mark.parametrize("fresh", [False, True])
def test_16_bit_cache_passes_no_kv_scales_keyword(rec, fresh):
    cache, kv, qkv, cos, sin, pos, cu = make("auto", fresh_prefill=fresh)
    attend(kv, write(kv, qkv, cos, sin, pos, cu), cu)
    assert len(rec.calls) == 2
    for _, _, kwargs in rec.calls:
        assert "kv_scales" not in kwargs and kwargs == {}
