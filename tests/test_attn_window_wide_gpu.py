"""-m gpu: tgis_attn_paged_window at windows wider than four pages (129, 300, 1000, 1024, 4096 keys: what a Mistral checkpoint
carries), where a wave of the windowed decode form walks several pages and the windowed prefill form takes most pages
mask-free.  tests/test_attn_window_gpu.py stops at 95 keys: there every wave sees at most one page.

Built on that file: its _WCase (the fp64 restatement tests/attn_window_ref.py as `want`, a NaN page behind every table entry
below a sequence's window, +-65504 in every stale slot, NaN guards on `out` and the workspace) and its `check`; once more than
1024 keys are visible the bound is test_attention_edges_gpu.py's for long contexts (max abs 4e-3 f16 / 2.5e-2 bf16).  The
cases live in tests/attn_window_wide_cases.py, and tests/test_attn_window_wide_cpu.py asserts from the page walk
(tests/attn_window_walk.py) that they reach the loops they are there for."""
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":  # the combine-launch child (test_combine_launch_in_a_child)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "text-generation-inference_amd")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_window_wide_cases as wc  # noqa: E402
from test_attention_edges_gpu import BF16, F16, _nat  # noqa: E402
from test_attn_window_gpu import _form, _fp8, _WCase, fp8_scales  # noqa: E402, F401

pytestmark = pytest.mark.gpu

DT = {"f16": F16, "bf16": BF16}


def _long(W, ctxs):
    """More than 1024 visible keys in some sequence: the long-context bound."""
    return max(min(c, W) for c in ctxs) > 1024


def _checked(c, what, long, **kw):
    got = c.run(**kw)
    assert torch.isfinite(got).all(), f"{what}: non-finite output: a page below the window (or an unwritten slot) was read"
    c.check(got, c.want_once(), what, long=long)
    return got


class _Wide(_WCase):
    def want_once(self):
        """The restatement, computed once per case (the inputs do not change between launches)."""
        if not hasattr(self, "_want"):
            self._want = self.want()
        return self._want


def _decode_case(dev, dtype, H, Hkv, D, ctxs, W, seed, **kw):
    c = _Wide(dev, dtype, H, Hkv, D, [(1, n) for n in ctxs], W, seed, **kw)
    assert c.max_ctx > W and _form(c)["form"] == "window"
    return c


# ---- decode form ------------------------------------------------------------------------------------------------------------
DECODE = [(W, H, Hkv, dt) for W in wc.WINDOWS for H, Hkv, dt in wc.decode_geoms(W)]


@pytest.mark.parametrize("W,H,Hkv,dt", DECODE, ids=[f"w{W}-h{h}kv{k}-{dt}" for W, h, k, dt in DECODE])
def test_wide_window_decode(gpu_device, W, H, Hkv, dt):
    hidden = 0
    for i, ctxs in enumerate(wc.decode_batches(W)):
        c = _decode_case(gpu_device, DT[dt], H, Hkv, 128, ctxs, W, seed=W * 31 + H + i)
        _checked(c, f"W {W} ctx {ctxs}", _long(W, ctxs))
        hidden += c.hidden_pages
    assert hidden >= 4 * (W // 32)  # the NaN pages were there: the longest sequence of each batch hides W + 5 keys


@pytest.mark.parametrize("D,dt,H,Hkv", wc.OTHER_HEAD_SIZES, ids=[f"d{c[0]}-{c[1]}" for c in wc.OTHER_HEAD_SIZES])
def test_wide_window_decode_other_head_sizes(gpu_device, D, dt, H, Hkv):
    for W in wc.OTHER_HEAD_SIZE_WINDOWS:
        for ctxs in wc.decode_batches(W):
            _checked(_decode_case(gpu_device, DT[dt], H, Hkv, D, ctxs, W, seed=W + D), f"D {D} W {W} ctx {ctxs}", _long(W, ctxs))


def test_wide_window_decode_in_fragment_order(gpu_device):
    W = wc.FRAGMENT_ORDER_WINDOW
    for ctxs in wc.decode_batches(W):
        c = _decode_case(gpu_device, F16, 8, 2, 128, ctxs, W, seed=11)
        rows = _checked(c, f"row-major, ctx {ctxs}", _long(W, ctxs))
        assert torch.equal(c.run(frag=True), rows), ctxs


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_wide_window_decode_over_e4m3_pools(gpu_device, fp8_scales, dt):
    """Against the restatement on the dequantised K / V, unwritten slots +-448 (tests/test_kv_fp8_ops_gpu.py)."""
    for W in wc.FP8_WINDOWS:
        for ctxs in wc.decode_batches(W):
            c = _decode_case(gpu_device, DT[dt], 8, 2, 128, ctxs, W, seed=5 + W, to_fp8=_fp8)
            assert c.kpool.element_size() == 1 and c.hidden_pages
            _checked(c, f"e4m3 pools W {W} ctx {ctxs}", _long(W, ctxs))


@pytest.mark.parametrize("W", wc.WINDOWS)
def test_causal_launch_reads_the_pages_below_a_wide_window(gpu_device, W):
    """What the feature is for: tgis_attn_paged on the same inputs reads the NaN pages."""
    ctxs = wc.decode_batches(W)[-1]
    c = _decode_case(gpu_device, F16, 8, 2, 128, ctxs, W, seed=13)
    assert c.hidden_pages
    assert not torch.isfinite(c.run(window=None)).all()
    _checked(c, f"windowed, W {W} ctx {ctxs}", _long(W, ctxs))


# ---- key splits -------------------------------------------------------------------------------------------------------------
SPLIT_CASES = wc.split_cases()


def _split_case(dev, W, name, dt, H, Hkv, D, ctxs, splits, fused):
    nat = _nat()
    c = _decode_case(dev, DT[dt], H, Hkv, D, ctxs, W, seed=H + D + W)
    long = _long(W, ctxs)
    one = _checked(c, f"{name} W {W}: one split", long)
    assert torch.equal(one, c.run()), f"{name} W {W}: one split, the second launch differs from the first"
    for ns in splits:
        if ns == wc.BY_RULE:  # what _DecodeGraph takes for a window
            ns = nat.attn_num_splits(len(ctxs), Hkv, H, 1, min(max(ctxs), W + 31))
            assert ns > 1, "the split rule changed: windowed decode graphs of this shape are no longer split"
        merge = _form(c, ns)["merge"]
        assert merge == ("fused" if fused else "combine8" if ns <= 8 else "combine"), (ns, merge)
        what = f"{name} W {W}: {ns} splits ({merge})"
        got = _checked(c, what, long, ns=ns)
        c.check(got, one, f"{what} against one", long=long)
        assert torch.equal(got, c.run(ns=ns)), f"{what}: the second launch differs from the first"


@pytest.mark.parametrize("W,name,dt,H,Hkv,D,ctxs,splits", SPLIT_CASES, ids=[f"w{c[0]}-{c[1]}" for c in SPLIT_CASES])
def test_wide_window_key_splits_merged_in_the_launch(gpu_device, W, name, dt, H, Hkv, D, ctxs, splits):
    _split_case(gpu_device, W, name, dt, H, Hkv, D, ctxs, splits, fused=True)


def test_combine_launch_in_a_child():
    """TGIS_ATTN_FUSED_COMBINE is read once per process: the split cases again in one fresh child with it set to 0, through
    attn_combine_kernel<MAXS = 8> up to 8 splits and <MAXS = 0> above."""
    env = {**os.environ, "TGIS_ATTN_FUSED_COMBINE": "0"}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    assert f"{len(SPLIT_CASES)} passed" in p.stdout, p.stdout[-4000:]


# ---- prefill form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pools", ["16bit", "e4m3"])
@pytest.mark.parametrize("name,dt,H,Hkv,D", wc.PREFILL, ids=[c[0] for c in wc.PREFILL])
def test_wide_window_prefill(gpu_device, request, name, dt, H, Hkv, D, pools):
    if pools == "e4m3":
        request.getfixturevalue("fp8_scales")
    for W in wc.PREFILL_WINDOWS:
        for seqs in wc.PREFILL_BATCHES:
            c = _Wide(gpu_device, DT[dt], H, Hkv, D, seqs, W, seed=W + H + len(seqs), to_fp8=_fp8 if pools == "e4m3" else None)
            assert c.kpool.element_size() == (1 if pools == "e4m3" else 2)
            assert c.max_ctx > W and _form(c)["form"] == "prefill"
            if any(ql < ctx for ql, ctx in seqs):
                assert c.hidden_pages > 0  # the suffixes: pages of cached tokens below the first row's window
            _checked(c, f"{name} {pools} W {W} {seqs}", long=False)


if __name__ == "__main__":
    assert os.environ.get("TGIS_ATTN_FUSED_COMBINE") == "0"
    dev = torch.device("cuda:0")
    passed = 0
    for case in SPLIT_CASES:
        try:
            _split_case(dev, *case, fused=False)
        except AssertionError as e:
            print(f"FAILED w{case[0]}-{case[1]} (combine launch): {e}", flush=True)
            sys.exit(1)
        print(f"ok w{case[0]}-{case[1]} (combine launch)", flush=True)
        passed += 1
    print(f"{passed} passed", flush=True)
