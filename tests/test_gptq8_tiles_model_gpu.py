"""-m gpu: the tiny 8-bit GPTQ Llama of tests/test_gptq8_model_gpu.py with a 112-token prefill on either path above 64 rows,
at that file's bars against LlamaRef on the dequantised tensors.  TGIS_GPTQ8_PATH=tiles: every prefill projection is one
launch of the tile GEMM and nothing is dequantised; TGIS_GPTQ8_PATH=dequant: the converse.  Decode steps (3 rows) take neither."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gptq8_model_gpu import _generate_and_check  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path,act_order", [("tiles", False), ("dequant", False), ("tiles", True)])
def test_long_prefill_on_either_path(gpu_device, monkeypatch, path, act_order):
    from tgis_amd import native

    calls = {"gptq8_tile_gemm": 0, "gptq8_dequant": 0}

    def counted(name):
        fn = getattr(native, name)

        def wrapper(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)

        return wrapper

    for name in calls:
        monkeypatch.setattr(native, name, counted(name))
    monkeypatch.setenv("TGIS_GPTQ8_PATH", path)
    lm = _generate_and_check([70, 9, 33], 11 if act_order else 7, f"long, {path}", act_order=act_order)
    assert (lm.model.model.layers[0].mlp.down_proj.linear.q_handle.perm is not None) == act_order
    other = "gptq8_dequant" if path == "tiles" else "gptq8_tile_gemm"
    used = "gptq8_tile_gemm" if path == "tiles" else "gptq8_dequant"
    assert calls[used] > 0 and calls[other] == 0, calls
