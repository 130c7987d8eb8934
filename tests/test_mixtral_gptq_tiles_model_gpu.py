"""-m gpu: the GPTQ Mixtral fixture of tests/test_mixtral_gptq_model_gpu.py on the int4 tile path (csrc/moe_gptq_tiles.h):
forced on every eager forward with TGIS_MOE_PATH=tiles against the golden fixture, and taken by the rule alone for a prompt
longer than MOE_GPTQ_FUSED_MAX_TOKENS, against the forced loop path on the same prompt."""
import numpy as np
import pytest

from tests.test_mixtral_gptq_model_gpu import _build, _fixture
from tests.test_mixtral_model_gpu import LOGIT_TOL, _check, _run

pytestmark = pytest.mark.gpu


def _counted(monkeypatch, lm, names):
    """Calls of native.<name>, counted; of gptq_gemm, those on an expert's view (the loop path's): the attention linears
    are int4 too."""
    from tgis_amd import native

    views = {id(w) for layer in lm.model.model.layers for w in layer.moe.experts.gate_up_experts + layer.moe.experts.down_experts}
    calls = dict.fromkeys(names, 0)

    def counting(name, real):
        def call(*a, **kw):
            if name != "gptq_gemm" or id(a[1]) in views:
                calls[name] += 1
            return real(*a, **kw)
        return call

    for name in names:
        monkeypatch.setattr(native, name, counting(name, getattr(native, name)))
    return calls


def test_the_tile_path_matches_the_fixture(gpu_device, monkeypatch):
    """TGIS_MOE_PATH=tiles, eager: the prefill (58 tokens) and every decode step (3) run route_tiles and the int4 tile GEMMs;
    ids are the fixture's, logits within LOGIT_TOL; the expert blocks launch neither a per-expert int4 GEMM nor a slab kernel."""
    meta, ids, logits, _ = _fixture()
    monkeypatch.setenv("TGIS_MOE_PATH", "tiles")
    lm, tok = _build(meta, use_graphs=False)
    calls = _counted(monkeypatch, lm, ("moe_gptq_tile_gemm_up", "moe_gptq_tile_gemm_down", "moe_route_tiles", "moe_route",
                                   "moe_gptq_gemm_up", "gptq_gemm"))
    steps = ids.shape[1]
    _check(_run(lm, tok, meta, steps), ids, logits, "gptq tiles")
    layers = len(lm.model.model.layers)
    assert calls["moe_gptq_tile_gemm_up"] == calls["moe_gptq_tile_gemm_down"] == calls["moe_route_tiles"] == layers * steps
    assert calls["moe_gptq_gemm_up"] == 0 and calls["moe_route"] == 0
    assert calls["gptq_gemm"] == 0, "a per-expert int4 GEMM ran behind the tile path"


def test_the_tile_path_refuses_dense_experts(gpu_device, monkeypatch):
    from tests.test_mixtral_model_gpu import _build as build_dense, _fixture as dense_fixture

    meta = dense_fixture()[0]
    monkeypatch.setenv("TGIS_MOE_PATH", "tiles")
    lm, tok = build_dense(meta, use_graphs=False)
    with pytest.raises(ValueError, match="16-bit"):
        _run(lm, tok, meta, 1)


def test_the_rule_takes_the_tiles_above_the_switch_point(gpu_device, monkeypatch):
    """One prompt of MOE_GPTQ_FUSED_MAX_TOKENS + 22 tokens, no override: the prefill takes the tile path.  Its first-token
    logits and the forced loop path's are each an f16 run of the same model, within LOGIT_TOL of the truth, so within twice
    that of each other; the argmax is equal when the loop run's top-2 margin exceeds that."""
    from tgis_amd.models.custom_modeling import flash_mixtral_modeling as fm

    meta = dict(_fixture()[0])
    T = fm.MOE_GPTQ_FUSED_MAX_TOKENS + 22
    meta["prompts"] = [np.random.default_rng(5).integers(3, 250, size=T).tolist()]
    first = {}
    for path in ("auto", "loop"):
        monkeypatch.setenv("TGIS_MOE_PATH", path)
        lm, tok = _build(meta, use_graphs=False)
        calls = _counted(monkeypatch, lm, ("moe_gptq_tile_gemm_up", "moe_gptq_gemm_up", "moe_route", "gptq_gemm"))
        from tests.test_neox_model_gpu import _from_pb, _LogitTap, _pb, _step

        tap = _LogitTap(lm)
        toks, rows = _step(lm, _from_pb(lm, tok, _pb(meta["prompts"], 2)), tap, first=True)
        first[path] = rows[0]
        layers = len(lm.model.model.layers)
        assert calls["moe_gptq_gemm_up"] == 0 and (calls["gptq_gemm"] == 0) == (path == "auto")
        assert (calls["moe_gptq_tile_gemm_up"], calls["moe_route"]) == ((layers, 0) if path == "auto" else (0, layers)), path
        monkeypatch.undo()
    err = float(np.abs(first["auto"] - first["loop"]).max())
    print(f"T {T}: max |tile logits - loop logits| = {err:.4f}")
    assert err <= 2 * LOGIT_TOL
    top = np.sort(first["loop"])[::-1]
    if top[0] - top[1] > 2 * LOGIT_TOL:
        assert int(first["auto"].argmax()) == int(first["loop"].argmax())
