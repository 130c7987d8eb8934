"""-m gpu: key splits of tgis_attn_paged with more than one q token per sequence (the verify step of speculative decoding,
a short suffix behind reused prefix pages): the decode form at num_splits > 1 and max_q_len > 1, through both merges.

Built on test_attention_edges_gpu.py: its _Case (poisoned pools, q inside a NaN activation, NaN `out` and workspace with
guards), its bounds (`check`, the max-abs bound of its split cases) against the fp32 oracle and against the same inputs at
one split, and its _merge_probe.  What differs from _Case.run is only the sizes: the launcher counts B * max_q_len rows
(ragged cu_seqlens_q hold fewer), so the workspace is sized for those and the NaN rows behind `out` reach that far — rows
past cu_seqlens_q[B] must stay NaN in both merges.

A case names its sequences [(q_len, ctx)] and its split counts.  The contexts sit at 1000 - 2200 keys (33 - 69 pages) with
tails ctx mod 32 in {0, 1, 2, q_len - 1, 31}: the q rows then straddle the last page boundary and, where a split holds only
the last page(s), some columns of a tile see no key of that split (records m = NEG_BIG, l = 0, O = 0)."""
import functools
import math
import os
import subprocess
import sys
import types

import pytest
import torch

if __name__ == "__main__":  # the two-launch combine child (test_two_launch_combine_at_several_q_tokens)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "text-generation-inference_amd")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_attention_edges_gpu import BF16, F16, GUARD_FLOATS, GUARD_ROWS, _Case, _form, _merge_probe, _nat  # noqa: E402

pytestmark = pytest.mark.gpu


class _QCase(_Case):
    def run(self, ns, probe=None):
        """_Case.run with the launcher's row count: B * max_q_len rows of workspace, NaN rows behind `out` up to there."""
        nat = _nat()
        H, Hkv, D = self.H, self.Hkv, self.D
        rows = len(self.seqs) * self.max_q
        outbuf = torch.full((rows + GUARD_ROWS, H * D), float("nan"), dtype=self.dtype, device=self.dev)
        out = outbuf[:self.T]
        ws = None
        if ns > 1:
            need = nat.attn_workspace_bytes(rows, H, Hkv, D, ns)
            assert need % 4 == 0
            buf = torch.full((need // 4 + GUARD_FLOATS,), float("nan"), dtype=torch.float32, device=self.dev)
            ws = types.SimpleNamespace(buf=buf, ptr=buf.data_ptr(), nbytes=need)
        nat.attn_paged(self.qa, self.qa.stride(0), self.kpool, self.vpool, self.bt, self.ctx, self.cu, out, len(self.seqs),
                       H, Hkv, D, self.max_q, self.max_ctx, D ** -0.5, ns, ws)
        torch.cuda.synchronize()
        assert torch.isnan(outbuf[self.T:].float()).all(), "rows past cu_seqlens_q[B] were written"
        if ws is not None:
            assert torch.isnan(ws.buf[need // 4:]).all(), "the workspace was written past attn_workspace_bytes"
            if probe is not None:
                probe(ws.buf)
        assert torch.isfinite(out.float()).all(), "non-finite output: an unwritten slot or record reached the result"
        return out.view(self.T, H, D).float().cpu()


def _probe_at(idx, fused):
    """A workspace float that the two-launch layout writes (a record's O) and the in-launch layout never does."""
    def probe(buf):
        v = float(buf[idx])
        assert math.isnan(v) if fused else math.isfinite(v), \
            f"expected the {'in-launch merge' if fused else 'combine launch'} (workspace float {idx} = {v})"
    return probe


def _probe(case, ns, fused):
    """H 8 / Hkv 1 (two q tokens per tile).  One sequence of 3 tokens: edges._merge_probe's float, {m, l} of (token 0, head 0,
    split 0) in the two-launch layout, is the in-launch record of column 8 of tile 1 — token 3, which does not exist.  The
    ragged batch: float 8 NS D is O of (token 1, head 0, split 0) there and here the record of column 8 of sequence 0's tile
    0 — its token 1, and the sequence has one."""
    if (case.H, case.Hkv) != (8, 1):
        return None
    if case.seqs[0][0] == 3 and len(case.seqs) == 1:
        return _merge_probe(case.T, ns, case.D, fused)
    if case.seqs[0][0] == 1 and len(case.seqs) > 1:
        return _probe_at(8 * ns * case.D, fused)
    return None


# (name, dtype, H, Hkv, D, [(q_len, ctx)], split counts)
CASES = [
    # MHA, 16 q tokens per tile
    ("mha-d128-f16-q4-tail0", F16, 32, 32, 128, [(4, 2048)], (2, 8)),
    # 33 pages: at 40 splits every split is one page (7 unreached), the last one visible to the last q row alone
    ("mha-d96-bf16-q8-tail1-more-splits-than-pages", BF16, 32, 32, 96, [(8, 1025)], (3, 40)),
    ("mha-d64-f16-q17-q64-several-tiles", F16, 8, 8, 64, [(17, 1200), (64, 1055)], (2, 9)),
    ("mha-d128-bf16-q64-tail31", BF16, 8, 8, 128, [(64, 1087), (2, 1025)], (16,)),
    # GQA
    ("g2-d64-f16-tails-0-2-1", F16, 4, 2, 64, [(4, 1280), (8, 1282), (2, 1057)], (2, 16)),
    ("g4-d128-bf16-tail-q-1-31", BF16, 8, 2, 128, [(4, 1027), (2, 1055)], (3, 8)),
    ("g4-d96-f16-q8-tail7", F16, 8, 2, 96, [(8, 1031), (8, 1024)], (9,)),
    ("g8-d128-f16-q3-probe", F16, 8, 1, 128, [(3, 1100)], (2, 9, 16)),
    ("g8-d64-bf16-q3-probe", BF16, 8, 1, 64, [(3, 1089)], (3, 8)),
    # ragged: max_q_len 8 gives four q tiles per sequence, most of them empty
    ("g8-d128-f16-ragged-1-3-8-2", F16, 8, 1, 128, [(1, 1500), (3, 1090), (8, 2200), (2, 1031)], (3, 8)),
    ("g8-d96-bf16-ragged-1-3-8-2", BF16, 8, 1, 96, [(1, 1025), (3, 1058), (8, 1095), (2, 1033)], (2, 9)),
    # padded groups
    ("g3pad-d96-f16", F16, 3, 1, 96, [(8, 1100), (2, 1058)], (2, 9)),
    ("g5pad-d64-bf16", BF16, 5, 1, 64, [(4, 1091), (8, 1061)], (3, 16)),
    # one q token per tile
    ("g16-d128-bf16-q4", BF16, 16, 1, 128, [(4, 1091), (2, 1056)], (2, 8)),
    ("g16-d64-f16-q2", F16, 16, 1, 64, [(2, 1025)], (9,)),
    # MQA 48:1: three one-chunk blocks per kv head
    ("mqa48-d128-f16-q4", F16, 48, 1, 128, [(4, 1091), (3, 1025)], (2, 9)),
    ("mqa48-d64-bf16-q2", BF16, 48, 1, 64, [(2, 1150)], (16,)),
    # ctx == q_len: one or two pages, every split but the first (two) unreached
    ("mha-d64-f16-ctx-equals-q64", F16, 8, 8, 64, [(64, 64)], (2, 3)),
    ("g2-d128-bf16-ctx-equals-q8", BF16, 4, 2, 128, [(8, 8), (2, 2)], (2,)),
    # short sequences beside a long one: most of their splits are unreached
    ("g4-d64-f16-short-beside-long", F16, 8, 2, 64, [(2, 5), (4, 33), (4, 2100)], (8, 16)),
    ("mha-d128-bf16-short-beside-long", BF16, 8, 8, 128, [(4, 5), (8, 33), (2, 2100), (1, 1), (8, 1024)], (9,)),
]


def _one_case(dev, name, dtype, H, Hkv, D, seqs, splits, fused, to_fp8=None):
    c = _QCase(dev, dtype, H, Hkv, D, seqs, seed=H * 7 + D + len(seqs) + seqs[0][1])
    if to_fp8 is not None:
        c = to_fp8(c)
    assert _form(H, Hkv, c.max_q, 2, fused) == "decode q>1"
    assert c.max_q > 1 and c.max_q * (1 << (min(H // Hkv, 16) - 1).bit_length()) <= 64
    want, one = c.want(), c.run(1)
    c.check(one, want, f"{name}: one split against the oracle", long=True)
    for ns in splits:
        got = c.run(ns, probe=_probe(c, ns, fused))
        c.check(got, want, f"{name}: {ns} splits against the oracle", long=True)
        c.check(got, one, f"{name}: {ns} splits against one", long=True)
        # the same launch again: bit-equal, so the first one left its arrival counters at zero
        assert torch.equal(got, c.run(ns)), f"{name}: {ns} splits, second launch differs from the first"


@pytest.mark.parametrize("name,dtype,H,Hkv,D,seqs,splits", CASES, ids=[c[0] for c in CASES])
def test_split_verify_rows(gpu_device, name, dtype, H, Hkv, D, seqs, splits):
    _one_case(gpu_device, name, dtype, H, Hkv, D, seqs, splits, fused=True)


def test_probed_cases_reach_the_probe():
    """(CPU arithmetic) the cases whose workspace is probed are there, so both merges are told apart."""
    probed = [c for c in CASES if (c[2], c[3]) == (8, 1) and ((c[5][0][0] == 3 and len(c[5]) == 1) or
                                                               (c[5][0][0] == 1 and len(c[5]) > 1))]
    assert len(probed) == 4


# ---- the one-byte cache ---------------------------------------------------------------------------------------------------
FP8_CASE = ("fp8-g4-d128-f16", F16, 8, 2, 128, [(4, 1027), (8, 1090), (2, 1056)], (3, 9))
FP8_SCALES = (0.5, 2.0)


def _fp8_case(dev, fused):
    import test_kv_fp8_ops_gpu as fp8ops

    nat = _nat()
    orig = nat.attn_paged
    nat.attn_paged = functools.partial(orig, kv_scales=FP8_SCALES)
    try:
        _one_case(dev, *FP8_CASE, fused=fused, to_fp8=lambda c: fp8ops._to_fp8(c, *FP8_SCALES))
    finally:
        nat.attn_paged = orig


def test_split_verify_rows_over_e4m3_pools(gpu_device):
    """Against the oracle on the dequantised K / V (tests/kv_fp8_ref.py), unwritten slots +-448, as test_kv_fp8_ops_gpu.py."""
    _fp8_case(gpu_device, fused=True)


# ---- the two-launch combine -----------------------------------------------------------------------------------------------
def test_two_launch_combine_at_several_q_tokens():
    """TGIS_ATTN_FUSED_COMBINE is read once per process: every case above, and the e4m3 one, again in ONE fresh child with
    it set to 0.  The combine launch runs over B * max_q_len rows and must stop at cu_seqlens_q[B]."""
    env = {**os.environ, "TGIS_ATTN_FUSED_COMBINE": "0"}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    assert f"{len(CASES) + 1} passed" in p.stdout, p.stdout[-4000:]


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_prefill_form_splits_are_refused(gpu_device):
    nat = _nat()
    for H, Hkv, q in ((32, 32, 65), (8, 1, 9), (48, 1, 5)):
        c = _QCase(gpu_device, F16, H, Hkv, 64, [(q, 1100)], seed=q)
        assert _form(H, Hkv, q, 1) == "prefill"
        with pytest.raises(nat.TgisHipError, match=r"code -1\).*decode form.*prefill form takes none"):
            c.run(2)


def test_workspace_one_byte_short_is_refused(gpu_device):
    nat = _nat()
    c = _QCase(gpu_device, F16, 8, 2, 64, [(4, 1100), (2, 1030)], seed=3)
    need = nat.attn_workspace_bytes(len(c.seqs) * c.max_q, 8, 2, 64, 4)
    buf = torch.zeros(need // 4, dtype=torch.float32, device=gpu_device)
    out = torch.full((c.T, 8 * 64), float("nan"), dtype=F16, device=gpu_device)

    def call(nbytes):
        ws = types.SimpleNamespace(ptr=buf.data_ptr(), nbytes=nbytes)
        nat.attn_paged(c.qa, c.qa.stride(0), c.kpool, c.vpool, c.bt, c.ctx, c.cu, out, len(c.seqs), 8, 2, 64, c.max_q,
                       c.max_ctx, 64 ** -0.5, 4, ws)
        torch.cuda.synchronize()

    with pytest.raises(nat.TgisHipError, match=r"code -1\).*workspace too small"):
        call(need - 1)
    assert torch.isnan(out.float()).all()  # refused before any launch
    call(need)
    assert torch.isfinite(out.float()).all()


if __name__ == "__main__":
    assert os.environ.get("TGIS_ATTN_FUSED_COMBINE") == "0"
    dev = torch.device("cuda:0")
    passed = 0
    for case in CASES + [None]:
        label = case[0] if case else FP8_CASE[0]
        try:
            if case:
                _one_case(dev, *case, fused=False)
            else:
                _fp8_case(dev, fused=False)
        except AssertionError as e:
            print(f"FAILED {label} (two-launch combine): {e}", flush=True)
            sys.exit(1)
        print(f"ok {label} (two-launch combine)", flush=True)
        passed += 1
    print(f"{passed} passed", flush=True)
