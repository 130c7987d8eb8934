"""CPU: per-request LoRA adapters on the host (utils/lora.py, prompt_cache.py, FlashCausalLMBatch, the option parsers): every
refusal by its message, the id rules, slot reuse, pins and unpins through concatenate / prune / release, replacement order, the
decode graph's key, the exclusion from KV prefix reuse, the argument checks of the three entry points, and PrefixLookup.  Real
adapter directories are written into tmp_path with safetensors; no kernel runs."""
import asyncio
import json
import types
from collections import OrderedDict

import pytest
import torch

from tests import lora_tiny
from tests.fixture_utils import FixtureTokenizer, prompt_text
from tgis_amd.models import flash_causal_lm
from tgis_amd.models.flash_causal_lm import FlashCausalLM, FlashCausalLMBatch
from tgis_amd.pb import generate_pb2 as pb2
from tgis_amd.prompt_cache import PrefixCache
from tgis_amd.utils import lora
from tgis_amd.utils.kv_cache import PagedKVCache

CPU = torch.device("cpu")
CFG = lora_tiny.TinyLlamaConfig()
SEED = 3


def table(S=2, max_rank=64, uploads=None):
    up = (lambda s, a: uploads.append((s, a.prefix_id))) if uploads is not None else None
    return lora.LoraSlots(S, max_rank, lora.module_shapes(CFG), CFG.num_hidden_layers, torch.float16, upload=up)


def cache(tmp_path, slots=None):
    c = PrefixCache(CPU, torch.float16, 64, CFG.hidden_size, store=tmp_path)
    c.lora = slots
    return c


def store(tmp_path, *names, **kw):
    for n in names:
        lora_tiny.write_adapter(tmp_path / n, n, CFG, SEED, **kw)


# ---- options ----------------------------------------------------------------------------------------------------------------
def test_option_parsers(monkeypatch):
    monkeypatch.delenv("TGIS_LORA_SLOTS", raising=False)
    monkeypatch.delenv("TGIS_LORA_MAX_RANK", raising=False)
    assert lora.parse_lora_slots() == 0 and lora.parse_lora_max_rank() == 64
    assert lora.parse_lora_slots(32) == 32 and lora.parse_lora_slots("4") == 4 and lora.parse_lora_max_rank(16) == 16
    monkeypatch.setenv("TGIS_LORA_SLOTS", "8")
    monkeypatch.setenv("TGIS_LORA_MAX_RANK", "32")
    assert lora.parse_lora_slots() == 8 and lora.parse_lora_max_rank() == 32
    for bad in (33, -1, "many", 1.5, True):
        with pytest.raises(ValueError, match="lora_slots"):
            lora.parse_lora_slots(bad)
    for bad in (0, 8, 24 + 1, 80, 128):
        with pytest.raises(ValueError, match="lora_max_rank"):
            lora.parse_lora_max_rank(bad)
    with pytest.raises(ValueError, match="multiple of 16"):
        lora.parse_lora_max_rank(40)


def test_construction_time_refusals():
    """Checked where the other options are, before anything is loaded (and before a GPU is asked for)."""
    with pytest.raises(NotImplementedError, match="lora_slots=2 with spec_tokens=3"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=object(), lora_slots=2, spec_tokens=3)
    with pytest.raises(NotImplementedError, match="lora_slots=2 with 4 tensor-parallel ranks"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=types.SimpleNamespace(world_size=4), lora_slots=2)
    with pytest.raises(ValueError, match="lora_slots"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=object(), lora_slots=64)
    with pytest.raises(ValueError, match="lora_max_rank"):
        FlashCausalLM("x", None, "synthetic", torch.float16, None, engine=object(), lora_slots=2, lora_max_rank=48 + 1)
    with pytest.raises(NotImplementedError, match="does not serve LoRA adapters"):
        lora.check_lora_model(2, object())  # any model class but the Llama one
    lora.check_lora_model(0, object())
    from tgis_amd.models.custom_modeling.flash_llama_modeling import FlashLlamaForCausalLM
    from tgis_amd.models.custom_modeling.flash_mixtral_modeling import FlashMixtralForCausalLM

    assert hasattr(FlashLlamaForCausalLM, "enable_lora") and not hasattr(FlashMixtralForCausalLM, "enable_lora")


# ---- reading and refusing adapters -----------------------------------------------------------------------------------------
def test_a_real_adapter_directory_loads(tmp_path):
    store(tmp_path, "qv", "all")
    lora_tiny.write_adapter(tmp_path / "od", "od", CFG, SEED, fmt="bin")
    c = cache(tmp_path, table())
    for name in ("qv", "all", "od"):
        a = c.get(name)
        spec = lora_tiny.ADAPTERS[name]
        assert isinstance(a, lora.LoraAdapter) and a.r == spec["r"] and a.scale == spec["alpha"] / spec["r"]
        assert tuple(a.modules) == spec["modules"] and len(a.tensors) == CFG.num_hidden_layers * len(spec["modules"])
        want = lora_tiny.adapter_tensors(CFG, name, SEED)
        A, B = a.pair(1, spec["modules"][0])
        path = f"base_model.model.{lora_tiny.module_path(1, spec['modules'][0])}"
        assert torch.equal(A, want[f"{path}.lora_A.weight"]) and torch.equal(B, want[f"{path}.lora_B.weight"])
        assert a.pair(0, "k_proj" if name != "all" else "nothing") == (None, None)
    assert len(c) == 0  # adapters are not kept in the prompt LRU


@pytest.mark.parametrize("override, message", [
    (dict(use_rslora=True), "use_rslora is not supported"),
    (dict(use_dora=True), "use_dora is not supported"),
    (dict(bias="all"), "bias='all' is not supported"),
    (dict(modules_to_save=["lm_head"]), "a non-empty modules_to_save is not supported"),
    (dict(rank_pattern={"q_proj": 4}), "a non-empty rank_pattern is not supported"),
    (dict(alpha_pattern={"q_proj": 4}), "a non-empty alpha_pattern is not supported"),
    (dict(fan_in_fan_out=True), "fan_in_fan_out is not supported"),
    (dict(target_modules=["q_proj", "lm_head"]), r"target modules \['lm_head'\]"),
    (dict(r=128), "r=128 is above lora_max_rank"),
])
def test_config_refusals_by_name(tmp_path, override, message):
    store(tmp_path, "qv", **override)
    with pytest.raises(lora.LoraError, match=message):
        cache(tmp_path, table()).get("qv")


def test_rank_above_the_configured_cap(tmp_path):
    store(tmp_path, "all", r=32)
    with pytest.raises(lora.LoraError, match=r"r=32 is above lora_max_rank \(TGIS_LORA_MAX_RANK\) = 16"):
        cache(tmp_path, table(max_rank=16)).get("all")


def test_tensor_refusals(tmp_path):
    good = lora_tiny.adapter_tensors(CFG, "qv", SEED)
    key = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"

    def refused(tensors, message, name):
        lora_tiny.write_adapter(tmp_path / name, "qv", CFG, SEED, tensors=tensors)
        with pytest.raises(lora.LoraError, match=message):
            cache(tmp_path, table()).get(name)

    refused({**good, key: torch.zeros(8, 128).half()}, r"has shape \(8, 128\), the base model needs \(8, 256\)", "shape")
    bad = good[key].clone()
    bad[0, 0] = float("inf")
    refused({**good, key: bad}, "contains non-finite elements", "inf")
    refused({**good, key: good[key].float() * 1e6}, "non-finite elements after conversion", "overflow")
    refused({**good, "base_model.model.lm_head.lora_A.weight": torch.zeros(8, 256).half()},
            "outside the served target modules", "head")
    refused({**good, "base_model.model.model.layers.5.self_attn.q_proj.lora_A.weight": good[key].clone()}, "names layer 5", "layer")
    refused({k: v for k, v in good.items() if k != key}, "without its other half", "half")
    # a module under the wrong parent is refused, not mapped to its namesake
    refused({**good, "base_model.model.model.layers.0.mlp.q_proj.lora_A.weight": good[key].clone()},
            "outside the served target modules", "parent")
    refused({**good, "base_model.model.model.layers.0.self_attn.down_proj.lora_B.weight": torch.zeros(256, 8).half()},
            "outside the served target modules", "parent2")


def test_rank_16_fits_a_cap_of_16(tmp_path):
    store(tmp_path, "all")
    assert cache(tmp_path, table(max_rank=16)).get("all").r == 16


def test_id_rules_and_other_prefix_kinds(tmp_path):
    store(tmp_path, "qv")
    c = cache(tmp_path, table())
    from tgis_amd.prompt_cache import PrefixNotFound

    for bad in ("../qv", "qv/../../x", "a b", "", "qv/.."):
        with pytest.raises(ValueError, match="Invalid prefix id"):
            c.get(bad)
    # an id made of valid characters that still leaves the store: a LoRA directory outside it is not served
    lora_tiny.write_adapter(tmp_path.parent / (tmp_path.name + "_outside"), "qv", CFG, SEED)
    store(tmp_path / "inner", "qv")
    inner = cache(tmp_path / "inner", table())
    assert isinstance(inner.get("qv"), lora.LoraAdapter)
    with pytest.raises(ValueError, match="Invalid prefix id"):
        inner.get("/" + str(tmp_path.parent / (tmp_path.name + "_outside")).lstrip("/"))
    with pytest.raises(PrefixNotFound, match="Prefix id missing not found"):
        c.get("missing")
    # a prompt-tuning adapter and a plain decoder.pt keep today's behaviour
    (tmp_path / "pt").mkdir()
    with open(tmp_path / "pt" / "adapter_config.json", "w") as fh:
        json.dump({"peft_type": "PROMPT_TUNING"}, fh)
    from safetensors.torch import save_file

    save_file({"prompt_embeddings": torch.ones(3, CFG.hidden_size)}, str(tmp_path / "pt" / "adapter_model.safetensors"))
    (tmp_path / "plain").mkdir()
    torch.save(torch.ones(5, CFG.hidden_size), tmp_path / "plain" / "decoder.pt")
    assert c.get("pt").shape == (3, CFG.hidden_size) and c.get("plain").shape == (5, CFG.hidden_size) and len(c) == 2
    # a LoRA directory without its tensors
    (tmp_path / "empty").mkdir()
    with open(tmp_path / "empty" / "adapter_config.json", "w") as fh:
        json.dump(lora_tiny.adapter_config("qv"), fh)
    with pytest.raises(Exception, match="no adapter_model"):
        c.get("empty")


def test_a_lora_id_with_the_option_off_names_the_option(tmp_path):
    store(tmp_path, "qv")
    with pytest.raises(ValueError, match=r"lora_slots \(TGIS_LORA_SLOTS\)"):
        cache(tmp_path, None).get("qv")
    batch, errs = _from_pb(_pb([[5, 6, 7], [8, 9]], prefix_ids=["qv", None]), cache(tmp_path, None))
    assert [e.request_id for e in errs] == [0] and "TGIS_LORA_SLOTS" in errs[0].message
    assert [r.id for r in batch.requests] == [1] and batch.lora_slots is None  # the batch goes on


# ---- slots ------------------------------------------------------------------------------------------------------------------
def _adapter(name):
    return lora.LoraAdapter(name, 8, 2.0, {(0, "q_proj"): (torch.zeros(8, 256), torch.zeros(256, 8))})


def test_slot_reuse_pins_and_replacement_order():
    ups = []
    t = table(S=2, uploads=ups)
    a, b, c = _adapter("a"), _adapter("b"), _adapter("c")
    assert t.acquire(a) == 0 and t.acquire(b) == 1 and t.acquire(a) == 0
    assert ups == [(0, "a"), (1, "b")] and t.pins == [2, 1] and t.loads == 2  # a second request of a resident adapter: no load
    assert t.resident("a").tensors is None and t.resident("c") is None
    with pytest.raises(lora.LoraSlotsBusy, match=r"all 2 adapter slots \(lora_slots / TGIS_LORA_SLOTS\) are pinned"):
        t.acquire(c)
    assert t.pins == [2, 1] and t.ids == ["a", "b"]
    t.release(0)
    with pytest.raises(lora.LoraSlotsBusy):
        t.acquire(c)  # still pinned once
    t.release(0)
    t.release(1)
    # both unpinned: the least recently used goes first — b was acquired before a's second request
    assert t.acquire(c) == 1 and ups[-1] == (1, "c") and t.ids == ["a", "c"] and t.resident("b") is None
    t.release(1)
    assert t.acquire(a) == 0 and t.loads == 3  # still resident
    t.release(0)
    assert t.acquire(b) == 1 and t.ids == ["a", "b"]  # c was used before a: it goes
    t.release(-1)  # (a request without an adapter)
    with pytest.raises(AssertionError):
        t.release(0)  # not pinned


# ---- the batch --------------------------------------------------------------------------------------------------------------
def _pb(prompts, prefix_ids=None, max_new=4, first_id=0, batch_id=0):
    reqs = []
    for i, p in enumerate(prompts):
        r = pb2.Request(id=first_id + i, inputs=prompt_text(p), input_length=len(p), truncate=False, max_output_length=max_new)
        if prefix_ids and prefix_ids[i]:
            r.prefix_id = prefix_ids[i]
        reqs.append(r)
    return pb2.Batch(id=batch_id, requests=reqs)


def _from_pb(pb, prefix_cache):
    return FlashCausalLMBatch.from_pb(pb, FixtureTokenizer(4096), torch.float16, CPU, None, prefix_cache, True)


def _decoding(batch, pool):
    """The batch as its prefill leaves it, as far as concatenate and prune look."""
    batch.allocate_pages(pool)
    B = len(batch)
    batch.cu_seqlens_q = torch.arange(B + 1, dtype=torch.int32)
    batch.position_ids = torch.tensor(batch.input_lengths)
    batch.input_ids = torch.zeros(B, dtype=torch.int64)
    return batch


def test_pins_through_concatenate_prune_and_release(tmp_path):
    store(tmp_path, "qv", "all", "od")
    ups = []
    t = table(S=2, uploads=ups)
    c = cache(tmp_path, t)
    pool = PagedKVCache(1, 1, 64, 32, torch.float16, CPU)
    a, errs = _from_pb(_pb([[5] * 4, [6] * 3, [7] * 5], ["qv", None, "all"], batch_id=1), c)
    assert not errs and a.lora_slots == [0, -1, 1] and a.has_lora() and t.pins == [1, 1]
    assert a.input_lengths == [4, 3, 5] and a.inputs_embeds is None  # an adapter adds no tokens and no embeddings
    # every slot pinned: a third adapter's request gets the error, its batch goes on without it
    b, errs = _from_pb(_pb([[8] * 2, [9] * 2], ["od", "qv"], first_id=3, batch_id=2), c)
    assert [e.request_id for e in errs] == [3] and "pinned by live requests" in errs[0].message
    assert b.lora_slots == [0] and [r.id for r in b.requests] == [4] and t.pins == [2, 1]
    m = FlashCausalLMBatch.concatenate([_decoding(a, pool), _decoding(b, pool)])
    assert m.lora_slots == [0, -1, 1, 0] and a.lora_slots is None and b.lora_slots is None and m.lora_table is t
    del a, b  # (their __del__ must not unpin what changed hands)
    assert t.pins == [2, 1]
    m = FlashCausalLMBatch.prune(m, [2])  # the request on `all` completes
    assert m.lora_slots == [0, -1, 0] and t.pins == [2, 0]
    d, errs = _from_pb(_pb([[8] * 2], ["od"], first_id=5, batch_id=3), c)  # now it is served, over the unpinned slot
    assert not errs and d.lora_slots == [1] and t.ids == ["qv", "od"] and ups == [(0, "qv"), (1, "all"), (1, "od")]
    m = FlashCausalLMBatch.prune(m, [0, 4])
    assert m.lora_slots == [-1] and not m.has_lora() and t.pins == [0, 1]
    d.release()
    m.release()
    assert t.pins == [0, 0] and d.lora_slots is None
    d.release()  # twice is harmless
    assert t.pins == [0, 0]
    # a batch without adapters carries nothing
    e, _ = _from_pb(_pb([[5] * 4]), c)
    assert e.lora_slots is None and not e.has_lora()


def test_a_failed_from_pb_gives_its_pins_back(tmp_path):
    store(tmp_path, "qv")
    t = table()
    with pytest.raises(TypeError):  # no tokenizer: from_pb fails after the slot was pinned
        FlashCausalLMBatch.from_pb(_pb([[5] * 4], ["qv"]), None, torch.float16, CPU, None, cache(tmp_path, t), True)
    assert t.pins == [0, 0] and t.ids[0] == "qv"


def test_adapter_requests_neither_look_up_nor_register_pages(tmp_path):
    store(tmp_path, "qv")
    t = table()
    c = cache(tmp_path, t)
    pool = PagedKVCache(1, 1, 64, 32, torch.float16, CPU, prefix_reuse=True)
    prompt = list(range(10, 80))
    first, _ = _from_pb(_pb([prompt], batch_id=1), c)
    first.allocate_pages(pool)
    first.register_prompt_pages()
    assert pool.reuse_stats()["registered"] == 2
    mixed, _ = _from_pb(_pb([prompt, prompt, list(range(500, 570))], ["qv", None, "qv"], first_id=1, batch_id=2), c)
    mixed.allocate_pages(pool)
    assert mixed.reused_lengths == [0, 64, 0]  # the same prompt under an adapter has other keys
    mixed.register_prompt_pages()
    assert pool.reuse_stats()["registered"] == 2  # the third prompt is new, but it ran under the adapter
    for b in (first, mixed):
        b.release()
    assert pool.free_pages == pool.num_pages and t.pins == [0, 0]


# ---- the decode graph's key -------------------------------------------------------------------------------------------------
def test_graph_key_with_and_without_adapter_rows(tmp_path, monkeypatch):
    store(tmp_path, "qv")
    t = table()
    c = cache(tmp_path, t)
    pool = PagedKVCache(1, 1, 64, 32, torch.float16, CPU)
    made = []

    class FakeGraph:
        graph = None

        def __init__(self, lm, *key):
            self.key = key
            made.append((type(self).__name__, key))

        def run(self, *args):
            self.args = args
            return None, None, None

    for name in ("_DecodeGraph", "_LoraDecodeGraph"):
        monkeypatch.setattr(flash_causal_lm, name, type(name, (FakeGraph,), {}))
    lm = FlashCausalLM.__new__(FlashCausalLM)
    lm.spec_tokens, lm.lora_slots, lm._graphs, lm.max_graphs, lm.use_graphs = 0, 2, OrderedDict(), 4, False
    plain = _decoding(_from_pb(_pb([[5] * 4, [6] * 3]), c)[0], pool)
    adapted = _decoding(_from_pb(_pb([[5] * 4, [6] * 3], ["qv", None], first_id=2), c)[0], pool)
    lm._decode_forward(plain)
    lm._decode_forward(adapted)
    lm._decode_forward(adapted)
    assert made == [("_DecodeGraph", (2, 8)), ("_LoraDecodeGraph", (2, 8, "lora"))]
    assert list(lm._graphs) == [(2, 8), (2, 8, "lora")]
    slots = lm._graphs[(2, 8, "lora")].args[3]
    assert slots.dtype == torch.int32 and slots.tolist() == [0, -1] and slots is adapted.lora_slots_device()
    assert len(lm._graphs[(2, 8)].args) == 3
    # once the adapter's request is gone the batch is back on the plain key
    adapted = FlashCausalLMBatch.prune(adapted, [2])
    lm._decode_forward(adapted)
    assert len(made) == 3 and made[-1] == ("_DecodeGraph", (1, 8))
    # with the option off nothing looks at the slots
    lm.lora_slots = 0
    lm._decode_forward(plain)
    assert len(made) == 3
    plain.release()
    adapted.release()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_without_a_gpu():
    import ctypes

    from tgis_amd import native

    lib = native.load_library()
    assert lib.tgis_lora_a_bytes(320, 3, 64) == 3 * 64 * 320 * 2 and lib.tgis_lora_b_bytes(512, 64) == 64 * 512 * 2
    bounds = (ctypes.c_int64 * 4)(0, 256, 384, 512)
    p = 4096  # a non-null, 16-byte aligned address that is never read: every call below is refused first
    A, B = lib.tgis_lora_a_bytes(320, 3, 64), lib.tgis_lora_b_bytes(512, 64)

    def group(T=8, S=4):
        return lib.tgis_lora_group(p, T, S, p, p, p, None)

    def shrink(T=8, K=320, P=3, S=4, R=64, dtype=0, stride=A, ldx=320):
        return lib.tgis_lora_shrink(p, ldx, p, stride, p, p, p, p, T, K, P, S, R, dtype, None)

    def expand(T=8, N=512, P=3, S=4, R=64, dtype=0, stride=B, ldy=512, bnd=bounds):
        return lib.tgis_lora_expand(p, p, stride, p, p, p, p, bnd, p, ldy, T, N, P, S, R, dtype, None)

    def refused(rc, fn, words):
        msg = lib.tgis_last_error().decode()
        assert rc == -1 and fn in msg and words in msg, (rc, msg)

    refused(group(T=65), "tgis_lora_group", "0 <= T <= 64")
    refused(group(T=-1), "tgis_lora_group", "0 <= T <= 64")
    refused(group(S=33), "tgis_lora_group", "1 <= S <= 32")
    refused(group(S=0), "tgis_lora_group", "1 <= S <= 32")
    refused(shrink(T=65), "tgis_lora_shrink", "0 <= T <= 64")
    refused(shrink(K=324), "tgis_lora_shrink", "multiple of 8")
    refused(shrink(P=4), "tgis_lora_shrink", "1 <= P <= 3")
    refused(shrink(R=24), "tgis_lora_shrink", "multiple of 16")
    refused(shrink(R=80), "tgis_lora_shrink", "at most 64")
    refused(shrink(dtype=2), "tgis_lora_shrink", "bad dtype")
    refused(shrink(stride=A - 16), "tgis_lora_shrink", "must hold one A image")
    refused(shrink(ldx=312), "tgis_lora_shrink", "16-byte aligned")
    refused(expand(T=65), "tgis_lora_expand", "0 <= T <= 64")
    refused(expand(N=516), "tgis_lora_expand", "multiple of 8")
    refused(expand(S=40), "tgis_lora_expand", "1 <= S <= 32")
    refused(expand(stride=B - 16), "tgis_lora_expand", "must hold one B image")
    refused(expand(ldy=500), "tgis_lora_expand", "rows of y must hold N")
    refused(expand(bnd=(ctypes.c_int64 * 4)(0, 256, 384, 520)), "tgis_lora_expand", "from 0 to N")
    refused(expand(bnd=(ctypes.c_int64 * 4)(0, 260, 384, 512)), "tgis_lora_expand", "multiples of 8")
    refused(expand(bnd=(ctypes.c_int64 * 4)(0, 384, 256, 512)), "tgis_lora_expand", "must ascend")
    lib.tgis_clear_error()
    # the wrappers refuse tensors that are not on the GPU: no fall-back
    with pytest.raises(native.TgisHipError):
        native.lora_group(torch.zeros(4, dtype=torch.int32), 4)


def test_pack_lays_out_the_slot_images():
    from tgis_amd import native

    bounds, K = (0, 16, 24), 8
    A0, B0 = torch.arange(4 * K).view(4, K).half(), torch.arange(16 * 4).view(16, 4).half()
    rank, a, b = native.LoraImages.pack([A0, None], [B0, None], bounds, K, torch.float16)
    assert rank == 4 and a.shape == (2, 16, K) and b.shape == (1, 24, 16)
    assert torch.equal(a[0, :4], A0) and not a[0, 4:].any() and not a[1].any()
    assert torch.equal(b[0, :16, :4], B0) and not b[0, :, 4:].any() and not b[0, 16:].any()
    A1 = torch.ones(20, K).half()
    rank, a, b = native.LoraImages.pack([None, A1], [None, torch.ones(8, 20).half()], bounds, K, torch.float16)
    assert rank == 20 and a.shape == (2, 32, K) and b.shape == (2, 24, 16)
    assert b[1, 16:, :4].eq(1).all() and not b[1, 16:, 4:].any() and not b[:, :16].any()  # granule 1 holds columns 16 .. 31
    assert native.LoraImages.pack([None], [None], (0, 8), K, torch.float16) == (0, None, None)


# ---- PrefixLookup -----------------------------------------------------------------------------------------------------------
def test_prefix_lookup_answers_zero_for_an_adapter(tmp_path):
    from tgis_amd.server import TextGenerationService

    store(tmp_path, "qv")
    lora_tiny.write_adapter(tmp_path / "bad", "qv", CFG, SEED, use_dora=True)
    (tmp_path / "plain").mkdir()
    torch.save(torch.ones(5, CFG.hidden_size), tmp_path / "plain" / "decoder.pt")

    class Context:
        async def abort(self, code, message):
            raise RuntimeError(f"{code}: {message}")

    svc = TextGenerationService(types.SimpleNamespace(prefix_cache=cache(tmp_path, table())), None, [], None)
    look = lambda i: asyncio.run(svc.PrefixLookup(pb2.PrefixLookupRequest(prefix_id=i), Context())).prefix_length  # noqa: E731
    assert look("qv") == 0 and look("plain") == 5
    with pytest.raises(RuntimeError, match="NOT_FOUND"):
        look("bad")  # loaded and validated by the lookup
    off = TextGenerationService(types.SimpleNamespace(prefix_cache=cache(tmp_path, None)), None, [], None)
    with pytest.raises(RuntimeError, match="NOT_FOUND"):
        asyncio.run(off.PrefixLookup(pb2.PrefixLookupRequest(prefix_id="qv"), Context()))
