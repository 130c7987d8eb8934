"""CPU: the fused_input_logprobs option and the argument checks of tgis_head_logprobs, which need no device."""
import ctypes
import inspect

import pytest


def test_option_keyword_parser_and_tensor_parallel_refusal(monkeypatch):
    from tgis_amd.utils.input_logprobs import check_fused_input_world, parse_fused_input_logprobs

    monkeypatch.delenv("TGIS_FUSED_INPUT_LOGPROBS", raising=False)
    assert parse_fused_input_logprobs() is False
    assert parse_fused_input_logprobs(True) is True and parse_fused_input_logprobs(" False ") is False
    monkeypatch.setenv("TGIS_FUSED_INPUT_LOGPROBS", "true")
    assert parse_fused_input_logprobs() is True and parse_fused_input_logprobs(False) is False
    with pytest.raises(ValueError, match="TGIS_FUSED_INPUT_LOGPROBS"):
        parse_fused_input_logprobs("yes")
    check_fused_input_world(True, 1)
    check_fused_input_world(False, 8)
    with pytest.raises(NotImplementedError, match="tensor-parallel"):
        check_fused_input_world(True, 2)
    from tgis_amd.models.flash_causal_lm import FlashCausalLM

    assert inspect.signature(FlashCausalLM.__init__).parameters["fused_input_logprobs"].default is None


def test_bad_arguments_are_refused_without_a_device():
    from tgis_amd import native

    lib = native.load_library()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf) // 16 * 16 + 16
    good = dict(x=p, ldx=32, w=p, targets=p, T=4, V=10, K=32, dtype=0, lp=p, rank=p, lse=p, ws=p, ws_bytes=4096, stream=None)
    for change in (dict(x=None), dict(w=None), dict(targets=None), dict(lp=None), dict(ws=None), dict(K=24), dict(T=-1),
                   dict(V=0), dict(ldx=16), dict(ws_bytes=16)):
        lib.tgis_clear_error()
        rc = lib.tgis_head_logprobs(*{**good, **change}.values())
        assert rc == -1 and b"tgis_head_logprobs" in lib.tgis_last_error(), change
    lib.tgis_clear_error()


def test_workspace_grows_with_rows_and_splits():
    from tgis_amd import native

    lib = native.load_library()
    s = ctypes.c_int()

    def query(T, V):
        return lib.tgis_head_logprobs_bytes(T, V, ctypes.byref(s)), s.value

    assert query(128, 128 * 4) == (128 * (4 + 16 * 4), 4) and query(256, 128 * 4) == (256 * (4 + 16 * 4), 4)
    assert query(128, 128 * 64) == (128 * (4 + 16 * 64), 64)
    # one launch fills the CUs: the fewer row tiles, the more splits; never more splits than column tiles
    assert query(8192, 128256)[1] < query(512, 128256)[1] <= 128 and query(8192, 100)[1] == 1
