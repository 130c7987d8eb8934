"""-m gpu: calibrated scales of the one-byte KV cache end to end on the tiny dense f16 Llama of tests/test_kv_fp8_model_gpu.py.

(a) FlashCausalLM.calibrate_kv_scales on the 16-bit model: its absmax values equal a host recomputation from the pages the
    model wrote (exactly) and the oracle's K / V rounded to the model dtype (within the product's own rounding of k and v).
(b) A copy of the model with v_proj scaled by 2^-8 and o_proj by 2^8 — the same function in exact arithmetic, V of std
    0.004: the one-byte cache with unit scales loses V to e4m3's subnormals, with calibrated scales it does not.
(c) Scales from a file reach the pool, graph replay equals eager with them, and they cannot change under held pages.
(d) Two tensor-parallel ranks on one GPU take rank 0's scales and calibrate to the same dict."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8_ref as q8  # noqa: E402

from oracle import ops_ref  # noqa: E402
from oracle.llama_ref import LlamaRef  # noqa: E402
from oracle.tiny_models import TinyLlamaConfig, tiny_llama_tensors  # noqa: E402
from tgis_amd.utils.kv_cache import kv_scales_stats, save_kv_scales, scale_from_absmax  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPE = torch.float16
LENS = [5, 37, 16, 64]
# tests/test_kv_fp8_model_gpu.py's bar for f16 logits against the quantised-KV oracle (derived there)
LOGIT_TOL = 1.4
# Cached K / V against the oracle's: the bar of tests/test_fullwidth_gpu.py::_check_cache for f16, 0.02 * max(1, max |x|) —
# the oracle computes k and v in fp32 from fp32 activations, the product rounds the normed activation, the projection and
# the rotated k to f16.  |max |a| - max |b|| <= max |a - b|, so the bar on the elements carries over to their absmax.
CACHE_TOL = 0.02


def _tensors(rescale_v=False):
    tcfg = TinyLlamaConfig()
    tensors = tiny_llama_tensors(tcfg, seed=7, quantize=None, groupsize=64, dtype=DTYPE)
    if rescale_v:  # v = x W_v shrinks by 2^-8 and o = (P v) W_o grows back by 2^8
        for l in range(tcfg.num_hidden_layers):
            p = f"model.layers.{l}.self_attn"
            tensors[f"{p}.v_proj.weight"] = (tensors[f"{p}.v_proj.weight"].float() * 2.0 ** -8).to(DTYPE)
            tensors[f"{p}.o_proj.weight"] = (tensors[f"{p}.o_proj.weight"].float() * 2.0 ** 8).to(DTYPE)
    return tcfg, tensors


def _llama(tcfg, tensors, kv, use_graphs=True, pages=64, **kw):
    from tgis_amd.inference_engine.synthetic import InferenceEngine
    from tgis_amd.models.custom_modeling.flash_llama_modeling import LlamaConfig
    from tgis_amd.models.flash_causal_lm import FlashCausalLM
    from tgis_amd.testing import SyntheticTokenizer

    cfg = LlamaConfig(**tcfg.to_dict())
    tok = SyntheticTokenizer(cfg.vocab_size)
    eng = InferenceEngine({k: v.clone() for k, v in tensors.items()}, cfg, DTYPE, None, tokenizer=tok)
    lm = FlashCausalLM("synthetic", None, "synthetic", DTYPE, None, engine=eng, kv_cache_pages=pages, kv_cache_dtype=kv, **kw)
    lm.use_graphs = use_graphs
    return lm, tok


def _run(lm, tok, lens, steps):
    """Token ids per step, the prompts' ids, and the fp32 logits per step."""
    from tgis_amd.testing import make_batch_pb

    rows = []
    orig = lm._process_new_tokens

    def tapped(batch, out, *a, **kw):
        rows.append(out.detach().float().cpu().numpy().copy())
        return orig(batch, out, *a, **kw)

    lm._process_new_tokens = tapped
    pb = make_batch_pb(lens, max_new=steps + 1, logprobs=True)
    ids = []
    try:
        with lm.context_manager():
            batch, errs = lm.batch_type.from_pb(pb, tok, lm.dtype, lm.device, lm.word_embeddings, None, True)
            assert not errs
            prompts = [batch.all_input_ids_tensor[i, :l].tolist() for i, l in enumerate(lens)]
            ids.append([t.token_id for t in lm.generate_token(batch, first=True)[0]])
            for _ in range(steps):
                ids.append([t.token_id for t in lm.generate_token(batch)[0]])
        batch.release()
    finally:
        del lm._process_new_tokens
    return ids, prompts, rows


def _is_pow2(s):
    return s > 0 and math.frexp(s)[0] == 0.5


def _oracle_absmax(ref_state, layers):
    """[(max |k|, max |v|)] per layer over every sequence, of the oracle's K / V rounded to the model dtype."""
    out = []
    for l in range(layers):
        ks = [st[l][0].to(DTYPE).float().abs().max() for st in ref_state]
        vs = [st[l][1].to(DTYPE).float().abs().max() for st in ref_state]
        out.append((float(max(ks)), float(max(vs))))
    return out


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
def test_calibration_measures_the_cache(gpu_device):
    from tgis_amd.testing import make_batch_pb

    tcfg, tensors = _tensors()
    lm, tok = _llama(tcfg, tensors, "auto")
    L, Hkv, D = tcfg.num_hidden_layers, tcfg.num_key_value_heads, tcfg.hidden_size // tcfg.num_attention_heads
    free = lm.kv_cache.free_pages
    stats = lm.calibrate_kv_scales([make_batch_pb(LENS, max_new=4)])
    assert lm.kv_cache.free_pages == free == lm.kv_cache.num_pages
    assert stats["format"] == "tgis-kv-scales-1" and stats["num_layers"] == L and stats["tokens"] == sum(LENS)
    assert stats["headroom"] == 2.0 and stats["model_dtype"] == "float16" and stats["kv_cache_dtype"] == "fp8_e4m3"
    for name in ("k", "v"):
        for a, s in zip(stats[f"{name}_absmax"], stats[f"{name}_scale"]):
            assert a > 0 and _is_pow2(s) and s == scale_from_absmax(a) and 224.0 < 2.0 * a / s <= 448.0

    # exactly what the model wrote: the same prefill once more, its pages read back on the host
    pb = make_batch_pb(LENS, max_new=4)
    with lm.context_manager():
        batch, errs = lm.batch_type.from_pb(pb, tok, lm.dtype, lm.device, lm.word_embeddings, None, True)
        assert not errs
        prompts = [batch.all_input_ids_tensor[i, :n].tolist() for i, n in enumerate(LENS)]
        lm.generate_token(batch, first=True)
    for l in range(L):
        k_pool, v_pool = lm.kv_cache.k_pool(l).float().cpu(), lm.kv_cache.v_pool(l).float().cpu()
        km = vm = 0.0
        for pages, n in zip(batch.pages, LENS):
            K = torch.cat([ops_ref.kv_page_unpack(k_pool, v_pool, pg, Hkv, D)[0] for pg in pages])[:n]
            V = torch.cat([ops_ref.kv_page_unpack(k_pool, v_pool, pg, Hkv, D)[1] for pg in pages])[:n]
            km, vm = max(km, float(K.abs().max())), max(vm, float(V.abs().max()))
        assert stats["k_absmax"][l] == km and stats["v_absmax"][l] == vm, f"layer {l}"
    batch.release()

    # the oracle's K / V, rounded to the model dtype, within the product's own rounding (CACHE_TOL above)
    ref = LlamaRef(tcfg, tensors, quantize=None, groupsize=64)
    ref.generate_greedy(prompts, 1)
    for l, (km, vm) in enumerate(_oracle_absmax(ref.last_state, L)):
        assert abs(stats["k_absmax"][l] - km) <= CACHE_TOL * max(1.0, km), (l, stats["k_absmax"][l], km)
        assert abs(stats["v_absmax"][l] - vm) <= CACHE_TOL * max(1.0, vm), (l, stats["v_absmax"][l], vm)

    # decode steps add their tokens (the one chosen last is not cached yet) and can only raise a maximum
    more = lm.calibrate_kv_scales([make_batch_pb(LENS, max_new=4)], decode_steps=3)
    assert more["tokens"] == sum(LENS) + 3 * len(LENS) and lm.kv_cache.free_pages == free
    for name in ("k_absmax", "v_absmax"):
        assert all(b >= a for a, b in zip(stats[name], more[name]))
    # two batches accumulate
    both = lm.calibrate_kv_scales([make_batch_pb(LENS[:2], max_new=2), make_batch_pb(LENS[2:], max_new=2, first_request_id=2)])
    assert both["tokens"] == sum(LENS)
    for name in ("k_absmax", "v_absmax"):  # (another batch shape may take another GEMM plan: the product's own rounding)
        assert all(abs(a - b) <= CACHE_TOL * max(1.0, a) for a, b in zip(stats[name], both[name]))
    with pytest.raises(ValueError):
        lm.calibrate_kv_scales([make_batch_pb(LENS, max_new=2)], decode_steps=2)
    assert lm.kv_cache.free_pages == free


def test_calibration_needs_the_16_bit_cache(gpu_device):
    from tgis_amd.testing import make_batch_pb

    tcfg, tensors = _tensors()
    lm, _ = _llama(tcfg, tensors, "fp8_e4m3")
    with pytest.raises(ValueError, match="16-bit"):
        lm.calibrate_kv_scales([make_batch_pb([5], max_new=2)])


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = np.concatenate([x.ravel() for x in a]), np.concatenate([x.ravel() for x in b])
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_calibrated_scales_rescue_a_small_v(gpu_device, monkeypatch):
    """The error is the relative L2 error of the logits against the 16-bit cache's, over the steps whose fed tokens agree in
    all three runs.  The bar (3x) is the CPU figure of the reference quantiser; the fp32 oracle with that quantiser gives
    0.077 (unit scales) against 0.019 (calibrated) on this model, DESIGN.md §6.  Both figures are printed (-s)."""
    from tgis_amd.testing import make_batch_pb

    tcfg, tensors = _tensors(rescale_v=True)
    L = tcfg.num_hidden_layers
    lm16, tok = _llama(tcfg, tensors, "auto")
    stats = lm16.calibrate_kv_scales([make_batch_pb(LENS, max_new=2)])
    assert all(a < 2.0 ** -4 for a in stats["v_absmax"]), "the rescaled model's V is small"
    assert all(s < 2.0 ** -8 for s in stats["v_scale"]) and all(_is_pow2(s) for s in stats["k_scale"] + stats["v_scale"])

    steps = 4
    ids16, prompts, lg16 = _run(lm16, tok, LENS, steps)
    lm_unit, tok_u = _llama(tcfg, tensors, "fp8_e4m3")
    assert lm_unit.kv_cache.scales(0) == (1.0, 1.0)
    ids_unit, _, lg_unit = _run(lm_unit, tok_u, LENS, steps)
    lm_cal, tok_c = _llama(tcfg, tensors, "fp8_e4m3", kv_scales=stats)
    assert [lm_cal.kv_cache.scales(l) for l in range(L)] == list(zip(stats["k_scale"], stats["v_scale"]))
    ids_cal, _, lg_cal = _run(lm_cal, tok_c, LENS, steps)

    # the calibrated run against the oracle whose K / V pass through the quantiser with the calibrated scales of the layer
    orig_attn, orig_layer, layer = ops_ref.attention_varlen, LlamaRef._layer, [0]

    def attn(q, k, v, cu_q, cu_k, scale):
        ks, vs = stats["k_scale"][layer[0]], stats["v_scale"][layer[0]]
        k8 = q8.dequantize(q8.quantize(k.to(DTYPE), ks), ks)
        v8 = q8.dequantize(q8.quantize(v.to(DTYPE), vs), vs)
        return orig_attn(q, k8, v8, cu_q, cu_k, scale)

    def in_layer(self, l, *a, **kw):
        layer[0] = l
        return orig_layer(self, l, *a, **kw)

    monkeypatch.setattr(ops_ref, "attention_varlen", attn)
    monkeypatch.setattr(LlamaRef, "_layer", in_layer)
    want = LlamaRef(tcfg, tensors, quantize=None, groupsize=64).generate_greedy(prompts, len(ids_cal), forced=ids_cal)
    monkeypatch.undo()
    for i, (w, lg) in enumerate(zip(want, lg_cal)):
        err = float(np.abs(lg - w["logits"].numpy()).max())
        print(f"calibrated fp8 step {i}: max |logit - quantised-KV oracle| = {err:.4f}")
        assert err <= LOGIT_TOL, f"step {i}: max |logit - quantised-KV oracle| = {err:.4f} > {LOGIT_TOL}"

    # against the 16-bit cache: the steps that were fed the same tokens in all three runs (the prefill always is)
    n = 1
    while n < len(ids16) and ids16[n - 1] == ids_unit[n - 1] == ids_cal[n - 1]:
        n += 1
    err_unit, err_cal = _rel(lg_unit[:n], lg16[:n]), _rel(lg_cal[:n], lg16[:n])
    print(f"relative L2 error of the logits against the 16-bit cache over {n} step(s): unit scales {err_unit:.4f}, "
          f"calibrated {err_cal:.4f} (ratio {err_unit / err_cal:.2f})")
    assert err_unit >= 3.0 * err_cal, (err_unit, err_cal)


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def _scale_file(tmp_path, L, name="kv_cache_scales.json", k=0.25, v=2.0 ** -10):
    st = kv_scales_stats([k * 448.0 / 2.0 * (l + 1) for l in range(L)], [v * 448.0 / 2.0 * (l + 1) for l in range(L)], tokens=1,
                         model_dtype="float16")
    path = str(tmp_path / name)
    save_kv_scales(st, path)
    return path, st


def test_scales_from_a_file_and_graphs(gpu_device, tmp_path, monkeypatch):
    from tgis_amd.testing import make_batch_pb

    tcfg, tensors = _tensors(rescale_v=True)
    L = tcfg.num_hidden_layers
    path, st = _scale_file(tmp_path, L)
    assert st["k_scale"] == [0.25, 0.5] and st["v_scale"] == [2.0 ** -10, 2.0 ** -9]
    runs = []
    for graphs in (True, False):
        lm, tok = _llama(tcfg, tensors, "fp8_e4m3", use_graphs=graphs, kv_scales=path)
        assert [lm.kv_cache.scales(l) for l in range(L)] == list(zip(st["k_scale"], st["v_scale"]))
        runs.append(_run(lm, tok, LENS, 10))
        assert bool(lm._graphs) and all((g.graph is not None) == graphs for g in lm._graphs.values())
    assert runs[0][0] == runs[1][0], "graph replay and eager steps differ with calibrated scales"
    for a, b in zip(runs[0][2], runs[1][2]):
        assert np.array_equal(a, b), "graph and eager logits differ"

    # scales cannot change under written pages
    with lm.context_manager():
        batch, _ = lm.batch_type.from_pb(make_batch_pb([5], max_new=2), tok, lm.dtype, lm.device, lm.word_embeddings, None, True)
        lm.generate_token(batch, first=True)
    with pytest.raises(ValueError, match="handed out"):
        lm.kv_cache.set_scales([1.0] * L, [1.0] * L)
    batch.release()
    lm.kv_cache.set_scales([1.0] * L, [1.0] * L)

    # the environment names a file: used by a one-byte cache, ignored by a 16-bit one; an explicit argument is refused there
    other, st2 = _scale_file(tmp_path, L, "other.json", k=4.0, v=2.0 ** -6)
    monkeypatch.setenv("TGIS_KV_SCALES", other)
    lm, _ = _llama(tcfg, tensors, "fp8_e4m3")
    assert lm.kv_cache.scales(1) == (st2["k_scale"][1], st2["v_scale"][1]) != (1.0, 1.0)
    lm, _ = _llama(tcfg, tensors, "fp8_e4m3", kv_scales=st)
    assert lm.kv_cache.scales(1) == (st["k_scale"][1], st["v_scale"][1])
    lm, _ = _llama(tcfg, tensors, "auto")
    assert lm.kv_cache.scales(1) == (1.0, 1.0)
    with pytest.raises(ValueError, match="16-bit"):
        _llama(tcfg, tensors, "auto", kv_scales=path)
    monkeypatch.setenv("TGIS_KV_SCALES", str(tmp_path / "missing.json"))
    with pytest.raises(OSError):
        _llama(tcfg, tensors, "fp8_e4m3")


# ---- (d) tensor parallel: 2 ranks on one GPU, collectives through gloo (tests/test_tp_gpu.py) ------------------------------------
def _tp_worker(rank, world, port, files, ret):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      TGIS_DIST_BACKEND="gloo", TGIS_ALLOW_SHARED_GPU="1", TGIS_KV_SCALES=files[rank])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "text-generation-inference_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from tgis_amd.testing import make_batch_pb

    tcfg, tensors = _tensors()
    try:
        lm, _ = _llama(tcfg, tensors, "fp8_e4m3", pages=32)
        ret[f"scales{rank}"] = [lm.kv_cache.scales(l) for l in range(tcfg.num_hidden_layers)]
    except (ValueError, OSError) as e:
        ret[f"scales{rank}"] = f"{type(e).__name__}: {e}"
    else:
        lm16, _ = _llama(tcfg, tensors, "auto", pages=32)
        assert lm16.num_kv_heads == tcfg.num_key_value_heads // world
        ret[f"stats{rank}"] = lm16.calibrate_kv_scales([make_batch_pb(LENS, max_new=3)], decode_steps=1)
        ret[f"free{rank}"] = (lm16.kv_cache.free_pages, lm16.kv_cache.num_pages)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def _spawn_tp(files):
    import test_tp_gpu as tp

    mgr = mp.get_context("spawn").Manager()
    ret = mgr.dict()
    tp._spawn(_tp_worker, (2, tp._free_port(), files, ret), 2)
    return dict(ret)


def test_tp2_ranks_take_rank_0s_scales_and_calibrate_alike(gpu_device, tmp_path):
    tcfg, tensors = _tensors()
    L = tcfg.num_hidden_layers
    path0, st0 = _scale_file(tmp_path, L, "rank0.json")
    path1, _ = _scale_file(tmp_path, L, "rank1.json", k=8.0, v=2.0)
    ret = _spawn_tp([path0, path1])
    want = [(k, v) for k, v in zip(st0["k_scale"], st0["v_scale"])]
    assert ret["scales0"] == want and ret["scales1"] == want, ret
    assert ret["stats0"] == ret["stats1"]
    stats = ret["stats0"]
    assert stats["tokens"] == sum(LENS) + len(LENS) and stats["num_layers"] == L
    assert all(_is_pow2(s) for s in stats["k_scale"] + stats["v_scale"])
    assert ret["free0"][0] == ret["free0"][1] and ret["free1"][0] == ret["free1"][1]
    # both ranks' heads are in it: the unsharded oracle's absmax over prompt + the one fed token, within CACHE_TOL
    from tgis_amd.testing import SyntheticTokenizer, make_batch_pb

    tok = SyntheticTokenizer(tcfg.vocab_size)
    prompts = tok([r.inputs for r in make_batch_pb(LENS, max_new=3).requests])["input_ids"]
    ref = LlamaRef(tcfg, tensors, quantize=None, groupsize=64)
    ref.generate_greedy(prompts, 1)
    for l, (km, vm) in enumerate(_oracle_absmax(ref.last_state, L)):
        # (the decode step's token can only raise the product's maximum: a one-sided bar)
        assert stats["k_absmax"][l] >= km - CACHE_TOL * max(1.0, km), (l, stats["k_absmax"][l], km)
        assert stats["v_absmax"][l] >= vm - CACHE_TOL * max(1.0, vm), (l, stats["v_absmax"][l], vm)


def test_tp2_a_bad_file_on_rank_0_fails_every_rank(gpu_device, tmp_path):
    L = TinyLlamaConfig().num_hidden_layers
    good, _ = _scale_file(tmp_path, L, "good.json")
    bad, _ = _scale_file(tmp_path, L + 1, "bad.json")
    ret = _spawn_tp([bad, good])
    assert ret["scales0"].startswith("ValueError") and ret["scales1"].startswith("ValueError"), ret
