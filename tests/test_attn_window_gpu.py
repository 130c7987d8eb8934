"""-m gpu: tgis_attn_paged_window (sliding-window attention, csrc/attention.hip and attention_prefill.hip) against the fp64
restatement tests/attn_window_ref.py, at the edges of the window: W and ctx on both sides of a page edge, the window starting
and ending inside one page, windows that leave key splits without pages.

Built on test_attention_edges_gpu.py: its _Case (every pool slot +-65504 under the packed tokens, q inside a NaN activation,
NaN `out` and workspace with NaN guards behind them) and its tolerances (`check`: f16 2e-3 / bf16 1.6e-2 relative plus
absolute).  On top of it every block-table entry of a page wholly below a sequence's window names a page filled with NaN: a
finite output proves that the page was not read.  Through tgis_attn_paged the same inputs give NaN (test_causal_launch_*)."""
import functools
import os
import subprocess
import sys
import types

import pytest
import torch

if __name__ == "__main__":  # the combine-launch child (test_combine_launch_in_a_child)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "text-generation-inference_amd")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_window_ref as ref  # noqa: E402
from attn_window_plan import query_window_plan  # noqa: E402
from test_attention_edges_gpu import BF16, F16, GUARD_FLOATS, GUARD_ROWS, _Case, _nat  # noqa: E402

pytestmark = pytest.mark.gpu

WINDOWS = (1, 32, 40, 64, 95)
GEOMS = ((4, 4), (8, 2), (8, 1), (20, 1))  # (H, Hkv): MHA, GQA 4 and 8, and a padded group of two 16-head chunks


def window_ctxs(W):
    return sorted({c for c in (1, W - 1, W, W + 1, W + 31, W + 32, 3 * W + 5) if c >= 1})


def decode_batches(W):
    """The ctx grid of one W as ragged batches of 3 sequences, each with the longest ctx in it: the launch is then a windowed
    one (max_ctx > W) and the sequences the window does not reach run through the window variant beside it."""
    ctxs = window_ctxs(W)
    top, rest = ctxs[-1], ctxs[:-1]
    assert top > W
    if len(rest) % 2:
        rest.append(rest[0])
    return [[rest[i], top, rest[i + 1]] for i in range(0, len(rest), 2)]


class _WCase(_Case):
    """_Case under a window of W keys: `want` is the fp64 restatement and `run` calls the windowed entry point."""

    def __init__(self, dev, dtype, H, Hkv, D, seqs, W, seed, to_fp8=None):
        super().__init__(dev, dtype, H, Hkv, D, seqs, seed)
        if to_fp8 is not None:
            to_fp8(self)
        self.W = W
        # a page no sequence owns, filled with NaN, behind every table entry below a sequence's window
        spare = sorted(set(range(self.kpool.shape[0])) - set(self.bt.flatten().tolist()))
        assert spare
        self.nan_page = spare[0]
        one_byte = self.kpool.element_size() == 1
        for pool in (self.kpool, self.vpool):
            if one_byte:
                pool[self.nan_page] = 0x7F  # e4m3 NaN
            else:
                pool[self.nan_page] = float("nan")
        self.hidden_pages = 0
        for b, (ql, ctx) in enumerate(seqs):
            first = ref.first_visible_page(ctx, ql, W)
            self.bt[b, :first] = self.nan_page
            self.hidden_pages += first

    def want(self):
        return torch.cat([ref.window_attention(q, K, V, self.W, self.D ** -0.5)
                          for q, K, V in zip(self.q, self.K, self.V)]).float()

    def run(self, ns=1, window="own", frag=False):
        """One launch: tgis_attn_paged_window with this case's W (or `window`; None: tgis_attn_paged).  Checks the guards,
        returns out [T, H, D] on the host (not checked for finiteness: the causal launch is expected to fail that)."""
        nat = _nat()
        H, Hkv, D = self.H, self.Hkv, self.D
        window = self.W if window == "own" else window
        rows = len(self.seqs) * self.max_q
        outbuf = torch.full((rows + GUARD_ROWS, H * D), float("nan"), dtype=self.dtype, device=self.dev)
        out = outbuf[:self.T]
        if frag:
            fa = nat.FragAct(torch.full(((self.T + 31) // 32 * 32 * H * D,), float("nan"), dtype=self.dtype, device=self.dev),
                             self.T, H * D)
        ws = None
        if ns > 1:
            need = nat.attn_workspace_bytes(rows, H, Hkv, D, ns)
            assert need % 4 == 0
            buf = torch.full((need // 4 + GUARD_FLOATS,), float("nan"), dtype=torch.float32, device=self.dev)
            ws = types.SimpleNamespace(buf=buf, ptr=buf.data_ptr(), nbytes=need)
        kw = {} if window is None else {"window": window}
        nat.attn_paged(self.qa, self.qa.stride(0), self.kpool, self.vpool, self.bt, self.ctx, self.cu, fa if frag else out,
                       len(self.seqs), H, Hkv, D, self.max_q, self.max_ctx, D ** -0.5, ns, ws, **kw)
        torch.cuda.synchronize()
        if frag:
            return fa.to_rows().view(self.T, H, D).float().cpu()
        assert torch.isnan(outbuf[self.T:].float()).all(), "rows past cu_seqlens_q[B] were written"
        if ws is not None:
            assert torch.isnan(ws.buf[need // 4:]).all(), "the workspace was written past attn_workspace_bytes"
        return out.view(self.T, H, D).float().cpu()

    def run_checked(self, what, **kw):
        got = self.run(**kw)
        assert torch.isfinite(got).all(), f"{what}: non-finite output: a page below the window (or an unwritten slot) was read"
        self.check(got, self.want(), what)
        return got


def _form(c, ns=1):
    info = query_window_plan(_nat().load_library(), len(c.seqs), c.H, c.Hkv, c.D, c.max_q, ns, c.W)
    assert info is not None
    return info["plan"]


# ---- decode form ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("H,Hkv", GEOMS, ids=[f"h{h}kv{k}" for h, k in GEOMS])
def test_window_decode(gpu_device, H, Hkv, dtype):
    hidden = 0
    for W in WINDOWS:
        for i, ctxs in enumerate(decode_batches(W)):
            c = _WCase(gpu_device, dtype, H, Hkv, 128, [(1, n) for n in ctxs], W, seed=W * 31 + H + i)
            assert _form(c)["form"] == "window"
            c.run_checked(f"W {W} ctx {ctxs}")
            hidden += c.hidden_pages
    assert hidden > 20  # the NaN pages were there


@pytest.mark.parametrize("D,dtype,H,Hkv", [(64, F16, 8, 2), (96, BF16, 4, 4)], ids=["d64-f16", "d96-bf16"])
def test_window_decode_other_head_sizes(gpu_device, D, dtype, H, Hkv):
    for W in (40, 95):
        for ctxs in decode_batches(W):
            _WCase(gpu_device, dtype, H, Hkv, D, [(1, n) for n in ctxs], W, seed=W + D).run_checked(f"D {D} W {W} ctx {ctxs}")


FP8_SCALES = (0.5, 2.0)


def _fp8(c):
    import test_kv_fp8_ops_gpu as fp8ops

    return fp8ops._to_fp8(c, *FP8_SCALES)


@pytest.fixture
def fp8_scales(monkeypatch):
    nat = _nat()
    monkeypatch.setattr(nat, "attn_paged", functools.partial(nat.attn_paged, kv_scales=FP8_SCALES))


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_window_decode_over_e4m3_pools(gpu_device, fp8_scales, dtype):
    """Against the restatement on the dequantised K / V, unwritten slots +-448, as test_kv_fp8_ops_gpu.py."""
    for ns in (1, 2):
        c = _WCase(gpu_device, dtype, 8, 2, 128, [(1, 41), (1, 300), (1, 136)], 95, seed=5, to_fp8=_fp8)
        assert c.kpool.element_size() == 1 and c.hidden_pages
        c.run_checked(f"e4m3 pools, {ns} split(s)", ns=ns)


# W 95, ctx up to 300: (ctx, visible pages) = (300, 6..9), (96, 0..2), (290, 6..9), (1, 0), (127, 1..3), (200, 3..6)
SPLIT_CASES = [
    ("g4-d128-f16", F16, 8, 2, 128, [300, 96, 290]),
    ("mha-d64-bf16", BF16, 4, 4, 64, [1, 300, 127]),
    ("g20pad-d128-bf16", BF16, 20, 1, 128, [200, 94, 300]),
    ("g8-d96-f16", F16, 8, 1, 96, [289, 300, 95]),
]
SPLITS = (1, 2, 5)


def _split_case(dev, name, dtype, H, Hkv, D, ctxs, fused):
    c = _WCase(dev, dtype, H, Hkv, D, [(1, n) for n in ctxs], 95, seed=H + D)
    # at 5 splits the window leaves at least one split of every sequence without pages
    for n in ctxs:
        first = ref.first_visible_page(n, 1, 95)
        visible = (n + 31) // 32 - first
        assert -(-visible // 5) * 4 >= visible, (n, visible)
    one = c.run_checked(f"{name}: one split")
    for ns in SPLITS[1:]:
        plan = _form(c, ns)
        assert plan["merge"] == ("fused" if fused else "combine8"), plan
        got = c.run_checked(f"{name}: {ns} splits", ns=ns)
        c.check(got, one, f"{name}: {ns} splits against one")
        assert torch.equal(got, c.run(ns=ns)), f"{name}: {ns} splits, the second launch differs from the first"
    assert torch.equal(one, c.run()), f"{name}: one split, the second launch differs from the first"


@pytest.mark.parametrize("name,dtype,H,Hkv,D,ctxs", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_window_decode_key_splits_merged_in_the_launch(gpu_device, name, dtype, H, Hkv, D, ctxs):
    _split_case(gpu_device, name, dtype, H, Hkv, D, ctxs, fused=True)


def test_combine_launch_in_a_child():
    """TGIS_ATTN_FUSED_COMBINE is read once per process: the split cases again in one fresh child with it set to 0, through
    attn_combine_kernel."""
    env = {**os.environ, "TGIS_ATTN_FUSED_COMBINE": "0"}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    assert f"{len(SPLIT_CASES)} passed" in p.stdout, p.stdout[-4000:]


def test_window_decode_in_fragment_order(gpu_device):
    c = _WCase(gpu_device, F16, 8, 2, 128, [(1, 300), (1, 64), (1, 97)], 64, seed=11)
    rows = c.run_checked("row-major")
    assert torch.equal(c.run(frag=True), rows)


def test_causal_launch_reads_the_pages_below_the_window(gpu_device):
    """What the feature is for: tgis_attn_paged on the same inputs reads the NaN pages."""
    c = _WCase(gpu_device, F16, 8, 2, 128, [(1, 300), (1, 64), (1, 97)], 64, seed=11)
    assert c.hidden_pages
    assert not torch.isfinite(c.run(window=None)).all()
    c.run_checked("windowed")


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_window_no_row_reaches_is_the_causal_launch(gpu_device, dtype):
    for seqs in ([(1, 95), (1, 1), (1, 64)], [(95, 95), (3, 40)], [(2, 95), (1, 33)]):
        c = _WCase(gpu_device, dtype, 8, 2, 128, seqs, 95, seed=len(seqs))
        assert c.hidden_pages == 0
        causal = c.run(window=None)
        assert torch.isfinite(causal).all()
        for W in (95, 96, 1 << 40):
            assert torch.equal(c.run(window=W), causal), (seqs, W)


# ---- prefill form -----------------------------------------------------------------------------------------------------------
PREFILL = [
    ("mha-d128-f16", F16, 4, 4, 128),
    ("g4-d128-bf16", BF16, 8, 2, 128),
    ("g8-d64-f16", F16, 8, 1, 64),
    ("g20pad-d96-bf16", BF16, 20, 1, 96),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D", PREFILL, ids=[c[0] for c in PREFILL])
def test_window_prefill(gpu_device, name, dtype, H, Hkv, D):
    for W in (40, 64):
        # q_len = ctx in {1, 31, 97, 200} as two ragged batches of 3, and a suffix of 5 rows over 150 cached tokens
        for seqs in ([(97, 97), (1, 1), (200, 200)], [(31, 31), (200, 200), (5, 150)], [(5, 150), (2, 2), (3, 70)]):
            c = _WCase(gpu_device, dtype, H, Hkv, D, seqs, W, seed=W + H + len(seqs))
            assert c.max_ctx > W and _form(c)["form"] == "prefill"
            c.run_checked(f"{name} W {W} {seqs}")
    assert c.hidden_pages  # (the suffix case: pages 0 - 2 of the 150-token sequence)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_device):
    nat = _nat()
    c = _WCase(gpu_device, F16, 8, 2, 64, [(1, 300), (1, 100)], 95, seed=3)
    for W in (0, -4):
        with pytest.raises(nat.TgisHipError, match=r"tgis_attn_paged_window failed \(code -1\).*window -?\d+ must be at least 1"):
            c.run(window=W)
    q = _WCase(gpu_device, F16, 8, 2, 64, [(2, 300), (1, 100)], 95, seed=3)
    with pytest.raises(nat.TgisHipError, match=r"code -1\).*key splits are for one q token per sequence.*prefill form"):
        q.run(ns=2)
    need = nat.attn_workspace_bytes(2, 8, 2, 64, 4)
    buf = torch.zeros(need // 4, dtype=torch.float32, device=gpu_device)
    out = torch.full((c.T, 8 * 64), float("nan"), dtype=F16, device=gpu_device)

    def call(ws):
        nat.attn_paged(c.qa, c.qa.stride(0), c.kpool, c.vpool, c.bt, c.ctx, c.cu, out, 2, 8, 2, 64, 1, c.max_ctx, 64 ** -0.5,
                       4, ws, window=95)
        torch.cuda.synchronize()

    for ws in (types.SimpleNamespace(ptr=buf.data_ptr(), nbytes=need - 1), None):
        with pytest.raises(nat.TgisHipError, match=r"code -1\).*workspace too small"):
            call(ws)
    assert torch.isnan(out.float()).all()  # refused before any launch
    call(types.SimpleNamespace(ptr=buf.data_ptr(), nbytes=need))
    assert torch.isfinite(out.float()).all()


if __name__ == "__main__":
    assert os.environ.get("TGIS_ATTN_FUSED_COMBINE") == "0"
    dev = torch.device("cuda:0")
    passed = 0
    for case in SPLIT_CASES:
        try:
            _split_case(dev, *case, fused=False)
        except AssertionError as e:
            print(f"FAILED {case[0]} (combine launch): {e}", flush=True)
            sys.exit(1)
        print(f"ok {case[0]} (combine launch)", flush=True)
        passed += 1
    print(f"{passed} passed", flush=True)
