"""-m gpu: the library side of speculative decoding over several candidates per request — tgis_attn_paged_tree[_kv8] against
the fp32 masked oracle, tgis_spec_tree_stage / tgis_spec_tree_accept / tgis_spec_propose_multi against their numpy restatements
bit for bit (and, at C = 1, against the existing entry points on the same inputs), tgis_spec_tree_commit against the whole pool.

Tree attention is built on test_attention_edges_gpu.py: its _Case (poisoned pools, q inside a NaN activation), its bounds
(`check`) and, for the row count of a q_len > 1 launch, the guards of test_attn_qsplit_gpu.py's run.  A case names its sequences
[(q_len, ctx, mask)]; a mask is ("layout", C, K), the mask of the (C, K) verify step (q_len = 1 + C K), or "drawn": a general
tree, the parent of row r drawn from [0, r), with junk bits above the row's own index that the kernel must ignore; or
("words", [...]), the words themselves (rows that see no key at all)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

if __name__ == "__main__":  # the two-launch combine child (test_tree_two_launch_combine)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "text-generation-inference_amd")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ops_ref  # noqa: E402
from test_attention_edges_gpu import BF16, F16, GUARD_FLOATS, GUARD_ROWS, POISON, _Case, _merge_probe, _nat  # noqa: E402

import spec_ref  # noqa: E402
import spec_tree_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -7777


def _words(mask, ql, rng):
    if mask == "drawn":
        par = [-1] + [int(rng.integers(0, r)) for r in range(1, ql)]
        words = ref.mask_from_parents(par)
        # bits above the row's own index are ignored by the kernel and by the oracle
        return [w | ((int(rng.integers(0, 2 ** 62)) << (i + 1)) & (2 ** 64 - 1)) for i, w in enumerate(words)]
    if mask[0] == "words":
        assert len(mask[1]) == ql
        return list(mask[1])
    _, C, K = mask
    assert ref.rows(C, K) == ql, (mask, ql)
    return ref.q_mask(C, K)


class _TreeCase(_Case):
    def __init__(self, dev, dtype, H, Hkv, D, seqs, seed):
        super().__init__(dev, dtype, H, Hkv, D, [(ql, ctx) for ql, ctx, _ in seqs], seed)
        rng = np.random.default_rng(seed)
        self.words = [_words(m, ql, rng) for ql, _, m in seqs]
        self.qmask = ref.as_int64([w for ws in self.words for w in ws]).to(dev)
        self.kv_scales = (1.0, 1.0)
        self.out = None

    def want(self):
        return [ref.attention_masked(q, K, V, w, self.D ** -0.5) for q, K, V, w in zip(self.q, self.K, self.V, self.words)]

    def repack(self, b):
        """Sequence b's pages again from self.K / self.V (a test changed them)."""
        kp, vp, bt = self.kpool.cpu(), self.vpool.cpu(), self.bt.cpu()
        for j in range((self.seqs[b][1] + 31) // 32):
            ops_ref.kv_page_pack(kp, vp, int(bt[b, j]), self.K[b][32 * j:32 * j + 32], self.V[b][32 * j:32 * j + 32])
        self.kpool, self.vpool = kp.to(self.dev), vp.to(self.dev)

    def run(self, ns, probe=None, finite=True, **kw):
        """One tgis_attn_paged_tree call over B * max_q_len rows of workspace; NaN rows behind `out` and NaN floats behind
        the workspace must survive; returns out [T, H, D] on the host."""
        nat = _nat()
        H, Hkv, D = self.H, self.Hkv, self.D
        rows = len(self.seqs) * self.max_q
        outbuf = torch.full((rows + GUARD_ROWS, H * D), float("nan"), dtype=self.dtype, device=self.dev)
        self.out = out = outbuf[:self.T]
        ws = None
        if ns > 1:
            need = nat.attn_workspace_bytes(rows, H, Hkv, D, ns)
            assert need % 4 == 0
            buf = torch.full((need // 4 + GUARD_FLOATS,), float("nan"), dtype=torch.float32, device=self.dev)
            ws = types.SimpleNamespace(buf=buf, ptr=buf.data_ptr(), nbytes=need)
        args = dict(q_mask=self.qmask, kv_scales=self.kv_scales)
        args.update(kw)
        nat.attn_paged(self.qa, self.qa.stride(0), self.kpool, self.vpool, self.bt, self.ctx, self.cu, out, len(self.seqs),
                       H, Hkv, D, self.max_q, self.max_ctx, D ** -0.5, ns, ws, **args)
        torch.cuda.synchronize()
        assert torch.isnan(outbuf[self.T:].float()).all(), "rows past cu_seqlens_q[B] were written"
        if ws is not None:
            assert torch.isnan(ws.buf[need // 4:]).all(), "the workspace was written past attn_workspace_bytes"
            if probe is not None:
                probe(ws.buf)
        if finite:
            assert torch.isfinite(out.float()).all(), "non-finite output: an unwritten slot or record reached the result"
        return out.view(self.T, H, D).float().cpu()


L23, L33, L43, L31 = ("layout", 2, 3), ("layout", 3, 3), ("layout", 4, 3), ("layout", 3, 1)
# (name, dtype, H, Hkv, D, [(q_len, ctx, mask)])
SHORT = [
    # tails: (ctx - q_len) mod 32 in {0, 1, 20, 31}; q_len 7 straddles one page boundary at 31, q_len 40 two
    ("mha-d128-f16-q7-tails", F16, 4, 4, 128, [(7, 71, L23), (7, 72, L23), (7, 91, "drawn"), (7, 102, L23)]),
    ("mha-d96-bf16-q40-tails", BF16, 2, 2, 96, [(40, 72, ("layout", 13, 3)), (40, 73, "drawn"), (40, 92, "drawn"),
                                               (40, 103, ("layout", 3, 13))]),
    # no context at all
    ("mha-d64-f16-ctx-equals-q", F16, 4, 4, 64, [(7, 7, L23), (1, 1, "drawn"), (64, 64, ("layout", 9, 7)), (33, 33, "drawn")]),
    # q_len 64 at MHA: the tail is two full pages, or three started ones
    ("mha-d64-bf16-q64", BF16, 2, 2, 64, [(64, 128, ("layout", 7, 9)), (64, 101, "drawn")]),
    # GQA 8:1, q_len 7: TQ = 2, four q tiles
    ("g8-d128-bf16-q7-four-tiles", BF16, 16, 2, 128, [(7, 90, L23), (7, 39, "drawn")]),
    # padded groups: G = 3 in Gp = 4, TQ = 4
    ("g3pad-d96-f16-q13", F16, 6, 2, 96, [(13, 80, L43), (10, 42, L33), (16, 47, "drawn")]),
    # one q token per tile
    ("g16-d128-f16-q4", F16, 16, 1, 128, [(4, 66, L31), (4, 35, "drawn")]),
    ("g16-d64-bf16-q4", BF16, 16, 1, 64, [(4, 4, L31), (3, 95, "drawn")]),
    # ragged q lengths in one launch
    ("g2-d64-f16-ragged", F16, 4, 2, 64, [(7, 100, L23), (4, 37, L31), (1, 70, "drawn"), (10, 10, L33), (32, 65, "drawn")]),
    ("g4-d96-bf16-ragged", BF16, 8, 2, 96, [(1, 33, "drawn"), (13, 64, L43), (5, 36, "drawn")]),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,seqs", SHORT, ids=[c[0] for c in SHORT])
def test_tree_attention(gpu_device, name, dtype, H, Hkv, D, seqs):
    c = _TreeCase(gpu_device, dtype, H, Hkv, D, seqs, seed=H * D + len(seqs))
    got = c.run(1)
    c.check(got, c.want(), name)
    assert torch.equal(got, c.run(1)), f"{name}: a second launch differs"


def test_tree_mask_of_a_chain_is_the_causal_kernel(gpu_device):
    """All-ones masks: the tree entry point then computes what tgis_attn_paged computes (the same terms; the pages of the
    tail are added in another order), and both meet the causal oracle."""
    c = _TreeCase(gpu_device, F16, 8, 2, 128, [(7, 90, L23), (4, 33, L31), (8, 8, "drawn")], seed=5)
    c.qmask = torch.full_like(c.qmask, -1)
    tree = c.run(1)
    plain = c.run(1, tree=False, q_mask=None)
    want = [ops_ref.attention_varlen(q, K, V, [0, q.shape[0]], [0, K.shape[0]], c.D ** -0.5) for q, K, V in zip(c.q, c.K, c.V)]
    c.check(tree, want, "all-ones mask against the causal oracle")
    c.check(plain, want, "tgis_attn_paged against the causal oracle")


def test_a_row_that_sees_no_key_gives_zeros(gpu_device):
    """ctx == q_len, so nothing is visible but what the mask allows.  Row 3 of the first sequence has the word 0 and row 2
    of the second only bits above its own index (ignored): no key at all, m stays NEG_BIG, l = 0, and the output is exactly
    zero — at one split and through both records of the split merges (the two-launch combine: the child below)."""
    words_a = ref.q_mask(2, 3)
    words_a[3] = 0
    words_b = [1, 3, 0b11111000, 0b1001, 0b10001]
    seqs = [(7, 7, ("words", words_a)), (5, 5, ("words", words_b)), (7, 40, ("layout", 2, 3))]
    c = _TreeCase(gpu_device, F16, 8, 2, 64, seqs, seed=23)
    want = torch.cat(c.want())
    assert not want[3].any() and not want[7 + 2].any() and want[0].any(), "the oracle's rows without a key are zero"
    for ns in (1, 2, 3):
        got = c.run(ns)
        c.check(got, want, f"a row without keys, {ns} splits")
        assert not got[3].any() and not got[7 + 2].any(), f"{ns} splits: a row that sees no key is not exactly zero"


# ---- key splits -----------------------------------------------------------------------------------------------------------
# (name, dtype, H, Hkv, D, [(q_len, ctx, mask)], split counts); contexts of 1025 - 2200 keys
SPLIT = [
    # 65 pages at 9 splits: 8 pages per split, split 8 holds page 64 alone — a tail page (the rows start on page 63)
    ("mha-d128-f16-q40-last-split-all-tail", F16, 2, 2, 128, [(40, 2060, "drawn"), (7, 1025, L23)], (2, 9)),
    ("g8-d128-f16-q3-probe", F16, 8, 1, 128, [(3, 1100, ("layout", 2, 1))], (2, 9)),
    ("g4-d96-bf16-q7", BF16, 8, 2, 96, [(7, 1031, L23), (7, 2200, "drawn"), (4, 1056, L31)], (2, 9)),
    ("g16-d64-bf16-q4", BF16, 16, 1, 64, [(4, 1091, L31), (2, 1057, "drawn")], (9,)),
    ("g3pad-d64-f16-q13-short-beside-long", F16, 3, 1, 64, [(13, 1500, L43), (10, 10, L33), (4, 33, L31)], (2, 9)),
    # a row that sees no key at all (word 0 at ctx == q_len) beside a long sequence: its records are m = NEG_BIG, l = 0
    ("g4-d64-f16-row-without-keys", F16, 8, 2, 64, [(7, 7, ("words", [1, 3, 7, 0, 17, 49, 113])), (7, 1100, L23)], (2, 9)),
]


def _split_case(dev, name, dtype, H, Hkv, D, seqs, splits, fused):
    c = _TreeCase(dev, dtype, H, Hkv, D, seqs, seed=H * 7 + D + len(seqs) + seqs[0][1])
    want, one = c.want(), c.run(1)
    c.check(one, want, f"{name}: one split against the oracle", long=True)
    for ns in splits:
        probe = _merge_probe(c.T, ns, D, fused) if (H, Hkv) == (8, 1) and len(seqs) == 1 and seqs[0][0] == 3 else None
        got = c.run(ns, probe=probe)
        c.check(got, want, f"{name}: {ns} splits against the oracle", long=True)
        c.check(got, one, f"{name}: {ns} splits against one", long=True)
        assert torch.equal(got, c.run(ns)), f"{name}: {ns} splits, second launch differs from the first"


@pytest.mark.parametrize("name,dtype,H,Hkv,D,seqs,splits", SPLIT, ids=[c[0] for c in SPLIT])
def test_tree_attention_key_splits(gpu_device, name, dtype, H, Hkv, D, seqs, splits):
    _split_case(gpu_device, name, dtype, H, Hkv, D, seqs, splits, fused=True)


def test_tree_two_launch_combine():
    """TGIS_ATTN_FUSED_COMBINE is read once per process: the split cases again in ONE fresh child with it set to 0, through
    the combine launch (which must stop at cu_seqlens_q[B])."""
    env = {**os.environ, "TGIS_ATTN_FUSED_COMBINE": "0"}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    assert f"{len(SPLIT)} passed" in p.stdout, p.stdout[-4000:]


# ---- exact zeros, the one-byte cache, refusals --------------------------------------------------------------------------------
def test_rows_outside_a_candidate_get_exactly_nothing_of_it(gpu_device):
    """The V rows of candidate 1 are +-65504: a P that is small instead of exactly 0 would show in every other row."""
    C, K = 3, 3
    c = _TreeCase(gpu_device, F16, 4, 2, 64, [(10, 75, ("layout", C, K)), (10, 10, ("layout", C, K))], seed=11)
    g = torch.Generator().manual_seed(3)
    for b, (ql, ctx) in enumerate(c.seqs):
        rows = slice(ctx - ql + 1 + K, ctx - ql + 1 + 2 * K)
        sign = torch.randint(0, 2, c.V[b][rows].shape, generator=g) * 2 - 1
        c.V[b][rows] = (sign.float() * POISON).to(c.dtype)
        c.repack(b)
    got, want = c.run(1, finite=False), torch.cat(c.want())
    keep = torch.ones(c.T, dtype=torch.bool)
    keep[1 + K:1 + 2 * K] = keep[10 + 1 + K:10 + 1 + 2 * K] = False
    assert torch.isfinite(got[keep]).all()
    c.check(got[keep], want[keep], "rows outside the poisoned candidate")


def test_tree_attention_over_e4m3_pools(gpu_device):
    """Against the oracle on the dequantised K / V, unwritten slots +-448, scales (0.5, 2.0), one and several splits."""
    import test_kv_fp8_ops_gpu as fp8ops

    c = _TreeCase(gpu_device, F16, 8, 2, 128, [(7, 1027, L23), (13, 1090, "drawn"), (4, 36, L31)], seed=17)
    c = fp8ops._to_fp8(c, 0.5, 2.0)
    c.kv_scales = (0.5, 2.0)
    want, one = c.want(), c.run(1)
    c.check(one, want, "e4m3, one split", long=True)
    got = c.run(9)
    c.check(got, want, "e4m3, 9 splits", long=True)
    assert torch.equal(got, c.run(9))


def test_tree_refusals_leave_out_untouched(gpu_device):
    nat = _nat()
    # the prefill form (9 * 8 > 64, and 65 * 1 > 64: one word per row holds 64 rows)
    for H, Hkv, ql in ((8, 1, 9), (4, 4, 65)):
        c = _TreeCase(gpu_device, F16, H, Hkv, 64, [(ql, 100, "drawn")], seed=ql)
        with pytest.raises(nat.TgisHipError, match=r"code -1\).*tgis_attn_paged_tree: only the decode form"):
            c.run(1)
        assert torch.isnan(c.out.float()).all()
    c = _TreeCase(gpu_device, F16, 4, 2, 64, [(7, 100, L23)], seed=1)
    with pytest.raises(nat.TgisHipError, match=r"code -1\).*null q_mask"):
        c.run(1, q_mask=None, tree=True)
    assert torch.isnan(c.out.float()).all()
    assert torch.isfinite(c.run(1)).all()  # (the same case is served with its mask)


# ---- stage --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat(gpu_device):
    return _nat()


def _guarded(n, dtype, dev, shape=None):
    whole = torch.full((n + 16,), SENT, dtype=dtype, device=dev)
    view = whole[:n]
    return (view.view(shape) if shape else view), whole


def _tail_intact(whole, n):
    return bool((whole[n:] == SENT).all())


CKS = [(1, 3), (2, 3), (3, 1), (4, 3), (4, 7), (2, 7)]


@pytest.mark.parametrize("C,K", CKS)
@pytest.mark.parametrize("B", [1, 5, 16])
def test_stage_equals_the_restatement(nat, gpu_device, B, C, K):
    rng = np.random.default_rng(31 * B + 7 * C + K)
    R, width = ref.rows(C, K), 4
    # positions whose rows cross one page boundary, none, or run to the last slot of the table; one past it (clamped)
    pos = rng.integers(0, width * 32 - R, size=B).astype(np.int32)
    pos[0] = 31
    if B > 1:
        pos[1] = width * 32 - R
        pos[B - 1] = width * 32 - 2
    latest = rng.integers(3, 250, size=B).astype(np.int64)
    drafts = rng.integers(3, 250, size=(B, C, K)).astype(np.int64)
    bt = rng.permutation(B * width + 3)[:B * width].reshape(B, width).astype(np.int32)
    w_ids, w_pos, w_slots, w_ctx = ref.stage(pos, latest, drafts, bt)
    ids, ids_w = _guarded(B * R, torch.int64, gpu_device)
    po, po_w = _guarded(B * R, torch.int32, gpu_device)
    sl, sl_w = _guarded(B * R, torch.int32, gpu_device)
    ctx, ctx_w = _guarded(B, torch.int32, gpu_device)
    dev = [torch.from_numpy(x).to(gpu_device) for x in (pos, latest, drafts, bt)]
    nat.spec_tree_stage(dev[0], dev[1], dev[2], dev[3], ids, po, sl, ctx)
    torch.cuda.synchronize()
    assert ids.cpu().tolist() == w_ids.tolist() and po.cpu().tolist() == w_pos.tolist()
    assert sl.cpu().tolist() == w_slots.tolist() and ctx.cpu().tolist() == w_ctx.tolist()
    assert all(_tail_intact(w, n) for w, n in ((ids_w, B * R), (po_w, B * R), (sl_w, B * R), (ctx_w, B)))
    if C == 1:  # the existing entry point on the same inputs
        o = [torch.full_like(t, SENT) for t in (ids, po, sl, ctx)]
        nat.spec_stage(dev[0], dev[1], dev[2][:, 0].contiguous(), dev[3], *o)
        assert all(torch.equal(a, b) for a, b in zip(o, (ids, po, sl, ctx)))


# ---- accept -------------------------------------------------------------------------------------------------------------------
def _accept_case(B, C, K, rng):
    """Request b: the choices along candidate (b % (C + 1)) - 1's path equal its drafts up to a drawn depth (candidate -1:
    nobody is right); every candidate in front of it is right up to a drawn, usually shorter depth — ties included."""
    R, L = ref.rows(C, K), 80
    am = rng.integers(3, 250, size=(B, R)).astype(np.int64)
    lps = -rng.random((B, R)).astype(np.float32)
    drafts = rng.integers(300, 900, size=(B, C, K)).astype(np.int64)  # disjoint from the choices: wrong unless set below
    for b in range(B):
        right = b % (C + 1) - 1
        depth = int(rng.integers(1, K + 1))
        for c in range(C):
            d = depth if c == right else (int(rng.integers(0, depth + 1)) if right >= 0 and c < right else 0)
            if b % 7 == 6:
                d = min(depth, K)  # every candidate ties
            for j in range(d):
                drafts[b, c, j] = am[b, 0 if j == 0 else 1 + c * K + j - 1]
    pos = rng.integers(0, L - K - 2, size=B).astype(np.int64)
    all_ids = rng.integers(3, 250, size=(B + 2, L)).astype(np.int64)
    cu = (np.cumsum(rng.integers(1, 40, size=B + 1)) - 1).astype(np.int32)
    return am, lps, drafts, pos, all_ids, cu


def _run_accept(nat, dev, am, lps, drafts, pos, all_ids, cu, nullable=True):
    B, C, K = drafts.shape
    R, K1 = ref.rows(C, K), K + 1
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    n_emit, ne_w = _guarded(B, torch.int32, dev)
    best, be_w = _guarded(B, torch.int32, dev)
    dpos, dall, dcu = d(pos), d(all_ids), d(cu)
    out = dict(out_ids=_guarded(B * K1, torch.int64, dev)[0], out_logprobs=_guarded(B * K1, torch.float32, dev)[0],
               all_input_ids=dall, cu_seqlens=dcu, stage_ids=torch.full((B,), SENT, dtype=torch.int64, device=dev),
               stage_positions=torch.full((B,), SENT, dtype=torch.int32, device=dev)) if nullable else {}
    latest = nat.spec_tree_accept(d(am.reshape(-1)), d(lps.reshape(-1)), d(drafts), n_emit, best, dpos, **out)
    torch.cuda.synchronize()
    assert _tail_intact(ne_w, B) and _tail_intact(be_w, B)
    return n_emit, best, latest, dpos, out


@pytest.mark.parametrize("C,K", CKS)
@pytest.mark.parametrize("B", [1, 6, 16, 300])
def test_accept_equals_the_restatement(nat, gpu_device, B, C, K):
    rng = np.random.default_rng(77 * B + 5 * C + K)
    am, lps, drafts, pos, all_ids, cu = _accept_case(B, C, K, rng)
    want = ref.accept(am, lps, drafts, pos, all_ids[:B], cu)
    if B == 300 and C > 1:
        assert set(want["best"].tolist()) == set(range(C)), "the first, a middle and the last candidate all win somewhere"
        assert {1, K + 1} <= set(want["n_emit"].tolist())
    n_emit, best, latest, dpos, out = _run_accept(nat, gpu_device, am, lps, drafts, pos, all_ids, cu)
    assert n_emit.cpu().tolist() == want["n_emit"].tolist() and best.cpu().tolist() == want["best"].tolist()
    assert out["out_ids"].cpu().tolist() == want["out_ids"].reshape(-1).tolist()
    assert torch.equal(out["out_logprobs"].cpu(), torch.from_numpy(want["out_lps"].reshape(-1)))
    assert latest.cpu().tolist() == want["latest"].tolist() and dpos.cpu().tolist() == want["positions"].tolist()
    assert out["all_input_ids"][:B].cpu().tolist() == want["all_ids"].tolist()
    assert out["all_input_ids"][B:].cpu().tolist() == all_ids[B:].tolist(), "rows behind the batch are untouched"
    assert out["cu_seqlens"].cpu().tolist() == want["cu_seqlens"].tolist()
    assert out["stage_ids"].cpu().tolist() == want["latest"].tolist()
    assert out["stage_positions"].cpu().tolist() == want["positions"].tolist()
    if C == 1:  # tgis_spec_accept on the same inputs
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(gpu_device)  # noqa: E731
        K1 = K + 1
        ne, p2, a2, c2 = torch.empty_like(n_emit), d(pos), d(all_ids), d(cu)
        oi, ol = torch.empty(B * K1, dtype=torch.int64, device=gpu_device), torch.empty(B * K1, device=gpu_device)
        l2 = nat.spec_accept(d(am.reshape(-1)), d(lps.reshape(-1)), d(drafts[:, 0]), ne, p2, out_ids=oi, out_logprobs=ol,
                             all_input_ids=a2, cu_seqlens=c2)
        assert torch.equal(ne, n_emit) and torch.equal(l2, latest) and torch.equal(p2, dpos) and torch.equal(c2, out["cu_seqlens"])
        assert torch.equal(oi, out["out_ids"]) and torch.equal(ol, out["out_logprobs"]) and torch.equal(a2, out["all_input_ids"])
        assert (best == 0).all()


def test_accept_with_all_ids_cut_short_and_without_the_nullable_outputs(nat, gpu_device):
    rng = np.random.default_rng(5)
    B, C, K = 6, 3, 3
    am, lps, drafts, pos, all_ids, cu = _accept_case(B, C, K, rng)
    # ld_all = 24: emitted tokens that fall behind the row's end are not written (they would land in the next row's start)
    pos[:] = [20, 21, 22, 23, 19, 30]
    all_ids = np.ascontiguousarray(all_ids[:, :24])
    want = ref.accept(am, lps, drafts, pos, all_ids[:B], cu)
    assert (want["positions"] >= 24).any()
    n_emit, best, latest, dpos, out = _run_accept(nat, gpu_device, am, lps, drafts, pos, all_ids, cu)
    assert out["all_input_ids"][:B].cpu().tolist() == want["all_ids"].tolist()
    assert out["all_input_ids"][B:].cpu().tolist() == all_ids[B:].tolist()
    assert n_emit.cpu().tolist() == want["n_emit"].tolist() and dpos.cpu().tolist() == want["positions"].tolist()
    n2, b2, l2, p2, _ = _run_accept(nat, gpu_device, am, lps, drafts, pos, all_ids, cu, nullable=False)
    assert torch.equal(n2, n_emit) and torch.equal(b2, best) and torch.equal(l2, latest) and torch.equal(p2, dpos)


# ---- propose ------------------------------------------------------------------------------------------------------------------
def _contexts(B, rng):
    cases = [
        [7],                                                          # no site at all
        [21, 22, 30, 21, 22, 31, 50, 21, 22, 32, 60, 21, 22],         # three sites at n = 2, three first tokens: 32, 31, 30
        [21, 22, 30, 9, 21, 22, 30, 8, 22, 40, 5, 21, 22],            # n = 2 gives 30 twice (one taken); n = 1 adds 40
        [1, 2, 3, 70, 71, 3, 72, 73, 9, 1, 2, 3],                     # n = 3 at j = 0 first, then n = 1 sites
        [5, 6, 7, 5, 6],                                              # the continuation runs into the context's end
        list(range(100, 120)),                                        # no match
    ]
    return [cases[i] if i < len(cases) else rng.integers(0, 4, size=int(rng.integers(1, 90))).tolist() for i in range(B)]


@pytest.mark.parametrize("N", [1, 3, 4])
@pytest.mark.parametrize("C,K", CKS)
def test_propose_multi_equals_the_restatement(nat, gpu_device, C, K, N):
    B, L = 16, 96
    rng = np.random.default_rng(100 * C + 10 * K + N)
    ctxs = _contexts(B, rng)
    all_ids = np.full((B + 2, L), 3, dtype=np.int64)
    for b, c in enumerate(ctxs):
        all_ids[b, :len(c)] = c
        all_ids[b, len(c):] = rng.integers(0, 4, size=L - len(c))  # what follows the context must not be looked at
    pos = np.array([len(c) - 1 for c in ctxs], dtype=np.int64)
    want_d, want_h = ref.propose_multi(all_ids[:B], pos, C, K, N)
    if N >= 2 and C >= 3:
        assert want_d[1, :, 0].tolist()[:3] == [32, 31, 30] and want_d[2, :2, 0].tolist() == [30, 40]
    drafts, d_whole = _guarded(B * C * K, torch.int64, gpu_device, (B, C, K))
    hits, h_whole = _guarded(B, torch.int32, gpu_device)
    copy, c_whole = _guarded(B, torch.int32, gpu_device)
    dev_all, dev_pos = torch.from_numpy(all_ids).to(gpu_device), torch.from_numpy(pos).to(gpu_device)
    nat.spec_propose_multi(dev_all[:B], dev_pos, N, drafts, hits, copy)
    torch.cuda.synchronize()
    assert drafts.cpu().tolist() == want_d.tolist(), (ctxs, want_h.tolist())
    assert hits.cpu().tolist() == want_h.tolist() and torch.equal(copy, hits)
    assert _tail_intact(d_whole, B * C * K) and _tail_intact(h_whole, B) and _tail_intact(c_whole, B)
    assert torch.equal(dev_all.cpu(), torch.from_numpy(all_ids)), "the contexts are read only"
    for b in range(B):  # candidates part at depth 1
        firsts = [int(want_d[b, c, 0]) for c in range(C) if want_d[b, c].any()]
        assert len(set(firsts)) == len(firsts)
    if C == 1:  # tgis_spec_propose on the same inputs, and its restatement
        d1, h1 = torch.full((B, K), SENT, dtype=torch.int64, device=gpu_device), torch.full_like(hits, SENT)
        nat.spec_propose(dev_all[:B], dev_pos, N, d1, h1)
        assert torch.equal(d1, drafts[:, 0]) and torch.equal(h1, hits)
        sd, sh = spec_ref.propose(all_ids[:B], pos, K, N)
        assert sd.tolist() == want_d[:, 0].tolist() and sh.tolist() == want_h.tolist()


# ---- commit -------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.uint8)


@pytest.mark.parametrize("Hkv,D", [(1, 64), (2, 128)])
@pytest.mark.parametrize("pool_dtype", [F16, BF16, torch.uint8], ids=["f16", "bf16", "e4m3"])
def test_commit_moves_the_winning_chain_and_nothing_else(nat, gpu_device, pool_dtype, Hkv, D):
    L, C, K, H, width = 2, 3, 3, 2 * Hkv, 3
    R = ref.rows(C, K)
    dtype = F16 if pool_dtype == torch.uint8 else pool_dtype
    # (pos, best, n_emit): rows crossing a page boundary in source, destination or both; best = 0 and n_emit = 1 change nothing
    reqs = [(5, 1, 3), (28, 2, 4), (23, 1, 2), (30, 2, 3), (40, 0, 4), (50, 2, 1), (60, 1, 4), (31, 1, 4)]
    B = len(reqs)
    g = torch.Generator().manual_seed(Hkv * D)
    pages = B * width + 2
    perm = torch.randperm(pages, generator=g)
    bt = perm[:B * width].reshape(B, width).int()
    if pool_dtype == torch.uint8:
        pool = torch.randint(0, 256, (L, 2, pages + 1, Hkv, 32 * D), generator=g, dtype=torch.uint8)
    else:
        pool = torch.randn((L, 2, pages + 1, Hkv, 32 * D), generator=g).to(pool_dtype)
    pool = pool.to(gpu_device)
    pos = torch.tensor([r[0] for r in reqs], dtype=torch.int32)
    best = torch.tensor([r[1] for r in reqs], dtype=torch.int32)
    n_emit = torch.tensor([r[2] for r in reqs], dtype=torch.int32)
    ids = torch.empty(B * R, dtype=torch.int64, device=gpu_device)
    rpos, slots = (torch.empty(B * R, dtype=torch.int32, device=gpu_device) for _ in range(2))
    ctx = torch.empty(B, dtype=torch.int32, device=gpu_device)
    nat.spec_tree_stage(pos.to(gpu_device), torch.zeros(B, dtype=torch.int64, device=gpu_device),
                        torch.zeros((B, C, K), dtype=torch.int64, device=gpu_device), bt.to(gpu_device), ids, rpos, slots, ctx)
    cos, sin = ops_ref.rope_tables(D, 10000.0, 128, dtype)
    for layer in range(L):  # the tree step's cache write, per layer as the model does it
        qkv = torch.randn(B * R, (H + 2 * Hkv) * D, generator=g).to(dtype).to(gpu_device)
        nat.rope_kv_write(qkv, cos.to(gpu_device), sin.to(gpu_device), rpos, slots, pool[layer, 0], pool[layer, 1], H, Hkv, D,
                          D, kv_scales=(0.5, 2.0))
    torch.cuda.synchronize()
    before = pool.cpu().clone()
    new_pos = (pos + n_emit).to(gpu_device)
    nat.spec_tree_commit(pool, bt.to(gpu_device), new_pos, best.to(gpu_device), n_emit.to(gpu_device), C, K)
    torch.cuda.synchronize()
    after = pool.cpu()
    want = before.clone()
    moved = 0
    for layer in range(L):
        for b, (p, bc, n) in enumerate(reqs):
            for src, dst in ref.commit_moves(p, C, K, bc, n):
                Ks, Vs = ops_ref.kv_page_unpack(before[layer, 0], before[layer, 1], int(bt[b, src // 32]), Hkv, D)
                pg = int(bt[b, dst // 32])
                Kd, Vd = ops_ref.kv_page_unpack(want[layer, 0], want[layer, 1], pg, Hkv, D)
                Kd, Vd = Kd.clone(), Vd.clone()
                Kd[dst % 32], Vd[dst % 32] = Ks[src % 32], Vs[src % 32]
                ops_ref.kv_page_pack(want[layer, 0], want[layer, 1], pg, Kd, Vd)
                # read back: the destination holds the winning chain's keys and values bit for bit
                Ka, Va = ops_ref.kv_page_unpack(after[layer, 0], after[layer, 1], pg, Hkv, D)
                assert torch.equal(_bits(Ka[dst % 32]), _bits(Ks[src % 32])) and torch.equal(_bits(Va[dst % 32]), _bits(Vs[src % 32]))
                moved += 1
    assert moved == L * sum(n - 1 for _, bc, n in reqs if bc > 0)
    assert not torch.equal(_bits(want), _bits(before))
    assert torch.equal(_bits(after), _bits(want)), "a byte outside the moved positions changed"


def test_commit_clamps_what_the_host_got_wrong(nat, gpu_device):
    """best and n_emit outside their ranges and a position behind the table are clamped: the call stays inside the request's
    table and the pool (every page of it belongs to this test), and pages of other requests keep their bytes."""
    L, C, K, Hkv, D, width = 2, 2, 3, 1, 64, 2
    B = 3
    pool = torch.randn((L, 2, B * width + 1, Hkv, 32 * D), generator=torch.Generator().manual_seed(1)).half().to(gpu_device)
    bt = torch.arange(B * width, dtype=torch.int32).reshape(B, width)
    bt[2, 1] = 10 ** 6  # a page id far outside the pool: clamped to the last page
    before = pool.cpu().clone()
    new_pos = torch.tensor([10, 10 ** 6, 40], dtype=torch.int32, device=gpu_device)
    best = torch.tensor([99, 1, -5], dtype=torch.int32, device=gpu_device)  # -> 1, 1, 0
    n_emit = torch.tensor([99, 3, 4], dtype=torch.int32, device=gpu_device)  # -> 4, 3, 4
    nat.spec_tree_commit(pool, bt.to(gpu_device), new_pos, best, n_emit, C, K)
    torch.cuda.synchronize()
    after = pool.cpu()
    assert torch.equal(after[:, :, 4:6], before[:, :, 4:6]), "request 2 (best clamped to 0) changed"
    assert not torch.equal(after[:, :, 0], before[:, :, 0]), "request 0 (best 99 -> 1, n_emit 99 -> 4) moved nothing"
    assert torch.equal(after[:, :, 6], before[:, :, 6])


if __name__ == "__main__":
    assert os.environ.get("TGIS_ATTN_FUSED_COMBINE") == "0"
    dev = torch.device("cuda:0")
    passed = 0
    for case in SPLIT:
        try:
            _split_case(dev, *case, fused=False)
        except AssertionError as e:
            print(f"FAILED {case[0]} (two-launch combine): {e}", flush=True)
            sys.exit(1)
        print(f"ok {case[0]} (two-launch combine)", flush=True)
        passed += 1
    print(f"{passed} passed", flush=True)
