"""CPU: the calibrated scales of the one-byte KV cache (utils/kv_cache.py) — the rule absmax -> scale, what it buys on the
reference quantiser (tests/kv_fp8_ref.py), the scale file and its loader's refusals, PagedKVCache.set_scales, and the order
in which FlashCausalLM looks for scales (resolve_kv_scales, which needs no GPU)."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8_ref as q8  # noqa: E402

from tgis_amd.utils import kv_cache as kvc  # noqa: E402
from tgis_amd.utils.kv_cache import (PagedKVCache, check_kv_scales, kv_scales_stats, load_kv_scales, resolve_kv_scales,  # noqa: E402
                                     save_kv_scales, scale_from_absmax)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("headroom", [1.0, 2.0, 3.0])
def test_scale_is_the_smallest_power_of_two_that_fits(headroom):
    g = torch.Generator().manual_seed(3)
    values = (10.0 ** (torch.rand(200, generator=g, dtype=torch.float64) * 12 - 6)).tolist()
    # on and around the boundaries, where a rounded division would pick the wrong side
    values += [448.0 / headroom * 2.0 ** e for e in range(-20, 20)]
    values += [math.nextafter(448.0 / headroom * 2.0 ** e, math.inf) for e in range(-20, 20)]
    values += [65504.0, 2.0 ** -24, 6e-5, 3.3895e38]
    for a in values:
        s = scale_from_absmax(a, headroom)
        m, _ = math.frexp(s)
        assert m == 0.5, f"{s} is not a power of two"
        assert 224.0 < headroom * a / s <= 448.0, (a, s)
        assert float(torch.tensor(s, dtype=torch.float32)) == s  # survives the float the kernels take
        assert json.loads(json.dumps(s)) == s


def test_scale_of_zero_and_of_bad_input():
    assert scale_from_absmax(0.0) == 1.0
    assert scale_from_absmax(224.0) == 1.0 and scale_from_absmax(224.5) == 2.0 and scale_from_absmax(112.0) == 0.5
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
        with pytest.raises(ValueError):
            scale_from_absmax(bad)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            scale_from_absmax(1.0, headroom=bad)


# ---- what it buys: the e4m3 round trip of Gaussian data, relative L2 error ------------------------------------------------------
def _roundtrip_error(x, scale):
    y = q8.dequantize(q8.quantize(x, scale), scale)
    return float((y - x.float()).norm() / x.float().norm())


@pytest.mark.parametrize("std,unit_is_worse", [(1.0, False), (0.02, False), (0.005, True), (600.0, True)])
def test_calibrated_scale_on_the_reference_quantiser(std, unit_is_worse):
    """Calibrated: <= 0.03 in every case (0.0258 - 0.0267 measured with the reference quantiser: e4m3's own rounding, 3
    mantissa bits).  Unit scales lose std 0.005 to the subnormals below 2^-6 and std 600 to the clamp at 448: at least 3x the
    calibrated error (4.2x and 19x measured)."""
    g = torch.Generator().manual_seed(1234)
    x = (torch.randn(1 << 16, generator=g) * std).half()  # what a 16-bit pool would hold
    s = scale_from_absmax(float(x.float().abs().max()))
    calibrated, unit = _roundtrip_error(x, s), _roundtrip_error(x, 1.0)
    print(f"std {std}: scale {s}, relative L2 error calibrated {calibrated:.4f}, unit scale {unit:.4f}")
    assert calibrated <= 0.03
    if unit_is_worse:
        assert unit >= 3 * calibrated


# ---- the file --------------------------------------------------------------------------------------------------------------------
def _stats(L=3):
    return kv_scales_stats([300.0, 0.5, 17.0][:L], [0.004, 2.0, 0.0][:L], tokens=122, model_dtype="float16")


def test_stats_hold_the_rule_and_every_field():
    st = _stats()
    assert set(st) == {"format", "kv_cache_dtype", "num_layers", "k_absmax", "v_absmax", "k_scale", "v_scale", "headroom",
                       "tokens", "model_dtype"}
    assert st["format"] == "tgis-kv-scales-1" and st["kv_cache_dtype"] == "fp8_e4m3" and st["num_layers"] == 3
    assert st["k_scale"] == [2.0, 2.0 ** -8, 2.0 ** -3] and st["v_scale"] == [2.0 ** -15, 2.0 ** -6, 1.0]
    assert st["headroom"] == 2.0 and st["tokens"] == 122 and st["model_dtype"] == "float16"


def test_file_round_trip(tmp_path):
    st = _stats()
    path = str(tmp_path / "kv_cache_scales.json")
    save_kv_scales(st, path)
    assert load_kv_scales(path, 3) == st
    assert check_kv_scales(st, 3) == (st["k_scale"], st["v_scale"])


@pytest.mark.parametrize("edit,what", [
    (lambda s: s.update(format="tgis-kv-scales-2"), "format"),
    (lambda s: s.pop("format"), "format"),
    (lambda s: s.update(num_layers=4), "layers"),
    (lambda s: s.update(k_scale=s["k_scale"][:2]), "k_scale"),
    (lambda s: s.update(v_scale=s["v_scale"] + [1.0]), "v_scale"),
    (lambda s: s.pop("v_scale"), "v_scale"),
    (lambda s: s["k_scale"].__setitem__(1, 0.0), "k_scale"),
    (lambda s: s["k_scale"].__setitem__(1, -0.5), "k_scale"),
    (lambda s: s["v_scale"].__setitem__(0, float("nan")), "v_scale"),
    (lambda s: s["v_scale"].__setitem__(2, float("inf")), "v_scale"),
    (lambda s: s["v_scale"].__setitem__(2, "1.0"), "v_scale"),
], ids=["unknown-format", "no-format", "layer-count", "short-k", "long-v", "no-v", "zero", "negative", "nan", "inf", "string"])
def test_loader_refusals(tmp_path, edit, what):
    st = _stats()
    edit(st)
    path = str(tmp_path / "s.json")
    with open(path, "w") as f:
        json.dump(st, f)  # json writes NaN / Infinity as such, and reads them back
    with pytest.raises(ValueError, match=what):
        load_kv_scales(path, 3)


def test_loader_refuses_another_models_layer_count_and_non_json(tmp_path):
    path = str(tmp_path / "s.json")
    save_kv_scales(_stats(), path)
    with pytest.raises(ValueError, match="layers"):
        load_kv_scales(path, 2)
    with open(path, "w") as f:
        f.write("not json")
    with pytest.raises(ValueError):
        load_kv_scales(path, 3)
    with pytest.raises(ValueError):
        save_kv_scales({"format": "x"}, path)


# ---- the pool --------------------------------------------------------------------------------------------------------------------
def _pool(kv="fp8_e4m3", layers=2):
    return PagedKVCache(layers, 1, 64, 4, torch.float16, "cpu", kv_dtype=kv)


def test_set_scales():
    c = _pool()
    assert c.scales(0) == (1.0, 1.0)
    c.set_scales([0.5, 2.0], [0.25, 4])
    assert c.scales(0) == (0.5, 0.25) and c.scales(1) == (2.0, 4.0)
    for k, v in (([0.5], [0.25, 4.0]), ([0.5, 2.0, 1.0], [1.0, 1.0]), ([0.5, 0.0], [1.0, 1.0]), ([0.5, 1.0], [1.0, -1.0]),
                 ([0.5, float("nan")], [1.0, 1.0]), ([0.5, 1.0], [float("inf"), 1.0]), (None, [1.0, 1.0]),
                 ([0.5, "1"], [1.0, 1.0]), (0.5, 0.5), ([True, 1.0], [1.0, 1.0])):
        with pytest.raises(ValueError):
            c.set_scales(k, v)
    assert c.scales(0) == (0.5, 0.25) and c.scales(1) == (2.0, 4.0), "a refused call must leave the scales alone"


def test_set_scales_refuses_a_16_bit_pool_and_handed_out_pages():
    with pytest.raises(ValueError, match="one-byte"):
        _pool("auto").set_scales([1.0, 1.0], [1.0, 1.0])
    c = _pool()
    pages = c.alloc(1)
    with pytest.raises(ValueError, match="handed out"):
        c.set_scales([0.5, 0.5], [0.5, 0.5])
    c.free(pages)
    c.set_scales([0.5, 0.5], [0.5, 0.5])
    assert c.scales(1) == (0.5, 0.5)


# ---- where FlashCausalLM takes them from ---------------------------------------------------------------------------------------
def _write(path, k):
    st = kv_scales_stats([k * 100.0] * 2, [k] * 2, tokens=1, model_dtype="float16")
    save_kv_scales(st, str(path))
    return (st["k_scale"], st["v_scale"])


def test_resolution_order(tmp_path):
    explicit, env_file, model_dir = tmp_path / "explicit.json", tmp_path / "env.json", tmp_path / "model"
    model_dir.mkdir()
    want_explicit, want_env = _write(explicit, 1.0), _write(env_file, 8.0)
    want_found = _write(model_dir / kvc.KV_SCALES_FILE, 64.0)
    assert len({str(want_explicit), str(want_env), str(want_found)}) == 3
    env = {"TGIS_KV_SCALES": str(env_file)}
    fp8 = "fp8_e4m3"
    # an explicit path or dict wins over everything
    assert resolve_kv_scales(str(explicit), fp8, 2, str(model_dir), env) == want_explicit
    assert resolve_kv_scales(load_kv_scales(str(explicit), 2), fp8, 2, str(model_dir), env) == want_explicit
    # then the environment, then the file next to the weights, then nothing
    assert resolve_kv_scales(None, fp8, 2, str(model_dir), env) == want_env
    assert resolve_kv_scales(None, fp8, 2, str(model_dir), {}) == want_found
    assert resolve_kv_scales(None, fp8, 2, str(tmp_path), {}) is None
    assert resolve_kv_scales(None, fp8, 2, None, {}) is None
    # a 16-bit cache: explicit scales are an error, the environment and a discovered file are ignored
    for kv in ("auto", None):
        if kv is None and os.getenv("TGIS_KV_CACHE_DTYPE", "auto") != "auto":
            continue
        with pytest.raises(ValueError, match="16-bit"):
            resolve_kv_scales(str(explicit), kv, 2, str(model_dir), env)
        assert resolve_kv_scales(None, kv, 2, str(model_dir), env) is None
    # what is found must fit the model
    with pytest.raises(ValueError, match="layers"):
        resolve_kv_scales(None, fp8, 3, str(model_dir), {})
    with pytest.raises(ValueError):
        resolve_kv_scales(3.5, fp8, 2, None, {})
    with pytest.raises(OSError):
        resolve_kv_scales(str(tmp_path / "missing.json"), fp8, 2, None, {})


def test_resolution_reads_the_process_environment(tmp_path, monkeypatch):
    want = _write(tmp_path / "env.json", 8.0)
    monkeypatch.setenv("TGIS_KV_SCALES", str(tmp_path / "env.json"))
    assert resolve_kv_scales(None, "fp8_e4m3", 2) == want
    monkeypatch.delenv("TGIS_KV_SCALES")
    assert resolve_kv_scales(None, "fp8_e4m3", 2) is None


def test_flash_causal_lm_takes_kv_scales():
    """The keyword exists on the model class (its use is exercised on the GPU: tests/test_kv_scales_model_gpu.py)."""
    import inspect

    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    sig = inspect.signature(FlashCausalLM.__init__)
    assert sig.parameters["kv_scales"].default is None
    assert callable(FlashCausalLM.calibrate_kv_scales)


def test_kv_absmax_validates_its_arguments_without_a_gpu():
    """tgis_kv_absmax refuses bad arguments before it touches the device (the pointers are never dereferenced here)."""
    from tgis_amd import native

    lib = native.load_library()

    def call(k=1, v=1, bt=1, w=4, ctx=1, B=1, Hkv=2, D=64, dtype=native.F16, out=1):
        lib.tgis_clear_error()
        rc = lib.tgis_kv_absmax(k or None, v or None, bt or None, w, ctx or None, B, Hkv, D, dtype, out or None, None)
        return rc, lib.tgis_last_error()

    for kw in (dict(k=0), dict(v=0), dict(bt=0), dict(ctx=0), dict(out=0), dict(D=80), dict(dtype=2), dict(B=-1), dict(w=0),
               dict(Hkv=0), dict(Hkv=65536)):
        rc, msg = call(**kw)
        assert rc == -1 and b"tgis_kv_absmax" in msg, (kw, rc, msg)
    assert call(B=0) == (0, b"") and call(B=0, bt=0, ctx=0) == (0, b"")
    with pytest.raises(native.TgisHipError):  # no CPU fallback
        native.kv_absmax(torch.zeros(1, 1, 2048, dtype=torch.float16), torch.zeros(1, 1, 2048, dtype=torch.float16),
                         torch.zeros(1, 1, dtype=torch.int32), torch.ones(1, dtype=torch.int32), 1, 64, torch.zeros(2, 1))
