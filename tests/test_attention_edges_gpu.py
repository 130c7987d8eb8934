"""-m gpu: tgis_attn_paged at the edges of each of its launch forms (csrc/attention.hip attn_paged_impl), against the fp32
oracle ops_ref.attention_varlen, one sequence at a time.

Forms (G = H / Hkv, Gp = next_pow2(min(G, 16))) and the tests here that reach them:
  prefill      num_splits 1, max_q_len * Gp > 64: attention_prefill.hip, 8 * 16 / Gp q tokens per block
               -> test_multi_tile_prefill_kernel, test_short_prefill_at_the_kernel_boundary,
                  test_new_tokens_over_a_longer_context
  decode q>1   2 <= max_q_len, max_q_len * Gp <= 64: attn_paged_kernel with several q tokens per 16-column tile
               -> test_short_prefill_on_the_decode_kernel, test_short_prefill_at_the_kernel_boundary,
                  test_new_tokens_over_a_longer_context
  fused merge  decode, NS > 1, single-chunk groups: the last block of a group merges the NS records in the launch (NS > 8:
               in batches of MB records) -> test_split_decode[*fused*]
  combine      decode, NS > 1, multi-chunk (MQA) groups or no arrival counters: attn_combine_kernel in a second launch
               (MAXS = 8 up to 8 splits, MAXS = 0 beyond) -> test_split_decode[*combine*],
               test_two_launch_combine_for_single_chunk_groups
Splits a sequence does not reach (records m = NEG_BIG, l = 0): test_split_decode[unreached-*] and the 33-split cases.

Every case is built to notice small errors: q is scaled so that the softmax is peaked, V has a non-zero mean, every pool
slot holds +-65504 (a reused page's stale tail) before the real tokens are packed on the host (ops_ref.kv_page_pack), q sits
in a wider activation whose other columns are NaN, `out` and the split workspace start as NaN and carry NaN guards past
their ends that must survive the call."""
import math
import os
import subprocess
import sys
import types

import pytest
import torch

if __name__ == "__main__":  # the two-launch combine child (test_two_launch_combine_for_single_chunk_groups)
    _ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "text-generation-inference_amd")]
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases  # noqa: E402
from oracle import ops_ref  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
POISON = 65504.0  # the largest finite f16 (bf16 holds it as 65536): what the stale tail of a reused page can hold
GUARD_ROWS = 3
GUARD_FLOATS = 1024


def _nat():
    from tgis_amd import native

    native.load_library()
    return native


def _form(H, Hkv, max_q_len, ns, fused=True):
    """The launch attn_paged_impl picks, asked from the library's plan (tests/attn_cases.py).  `fused`: whether this process
    lets split launches merge in the launch (the children run with TGIS_ATTN_FUSED_COMBINE=0, and the plan follows it)."""
    info = attn_cases.query_plan(_nat().load_library(), 1, H, Hkv, 64, max_q_len, ns)
    assert info is not None, "the library refuses this shape"
    p = attn_cases.plan_fields(info)
    if p["form"] == "prefill":
        return "prefill"
    if max_q_len > 1:
        return "decode q>1"
    if ns == 1:
        return "decode"
    assert fused or p["merge"] != "fused"
    return "fused merge" if p["merge"] == "fused" else "combine"


class _Case:
    """Sequences [(q_len, ctx)] of one shape: q rows are the last q_len of ctx positions.  Pages are shuffled over a pool
    of +-65504 with two spare pages; unused block-table entries name a spare page."""

    def __init__(self, dev, dtype, H, Hkv, D, seqs, seed):
        g = torch.Generator().manual_seed(seed)
        self.dev, self.dtype, self.H, self.Hkv, self.D, self.seqs = dev, dtype, H, Hkv, D, seqs
        npages = [(ctx + 31) // 32 for _, ctx in seqs]
        total = sum(npages) + 2
        perm = torch.randperm(total, generator=g)
        bt = torch.full((len(seqs), max(npages)), int(perm[-1]), dtype=torch.int32)

        def poisoned():
            sign = torch.randint(0, 2, (total, Hkv, 32 * D), generator=g, dtype=torch.int8) * 2 - 1
            return (sign.to(torch.float32) * POISON).to(dtype)

        kpool, vpool = poisoned(), poisoned()
        self.q, self.K, self.V = [], [], []
        o = 0
        for b, (ql, ctx) in enumerate(seqs):
            assert 1 <= ql <= ctx
            K = torch.randn(ctx, Hkv, D, generator=g).to(dtype)
            V = (torch.randn(ctx, Hkv, D, generator=g) + 1.0).to(dtype)
            self.q.append((torch.randn(ql, H, D, generator=g) * 2.0).to(dtype))
            self.K.append(K)
            self.V.append(V)
            pages = perm[o:o + npages[b]]
            o += npages[b]
            bt[b, :npages[b]] = pages.int()
            for j, pg in enumerate(pages.tolist()):
                ops_ref.kv_page_pack(kpool, vpool, pg, K[32 * j:32 * j + 32], V[32 * j:32 * j + 32])
        self.T = sum(ql for ql, _ in seqs)
        self.max_q = max(ql for ql, _ in seqs)
        self.max_ctx = max(ctx for _, ctx in seqs)
        # q as a view into a wider activation (the product passes the qkv GEMM's output): the other columns are NaN
        W = (H + 2 * Hkv) * D
        qa = torch.full((self.T, W), float("nan"), dtype=dtype)
        qa[:, :H * D] = torch.cat(self.q).reshape(self.T, H * D)
        self.qa = qa.to(dev)
        self.kpool, self.vpool = kpool.to(dev), vpool.to(dev)
        self.bt = bt.to(dev)
        self.ctx = torch.tensor([c for _, c in seqs], dtype=torch.int32, device=dev)
        cu = [0]
        for ql, _ in seqs:
            cu.append(cu[-1] + ql)
        self.cu = torch.tensor(cu, dtype=torch.int32, device=dev)

    def want(self):
        return [ops_ref.attention_varlen(q, K, V, [0, q.shape[0]], [0, K.shape[0]], self.D ** -0.5)
                for q, K, V in zip(self.q, self.K, self.V)]

    def run(self, ns, probe=None):
        """One tgis_attn_paged call; checks the guards and that every output is finite, returns out [T, H, D] on the host.
        `probe(workspace)` may look at the workspace afterwards."""
        nat = _nat()
        H, Hkv, D = self.H, self.Hkv, self.D
        outbuf = torch.full((self.T + GUARD_ROWS, H * D), float("nan"), dtype=self.dtype, device=self.dev)
        out = outbuf[:self.T]
        ws = None
        if ns > 1:
            need = nat.attn_workspace_bytes(self.T, H, Hkv, D, ns)
            assert need % 4 == 0
            # the library is told `need` bytes; the NaN tail behind them must stay untouched
            buf = torch.full((need // 4 + GUARD_FLOATS,), float("nan"), dtype=torch.float32, device=self.dev)
            ws = types.SimpleNamespace(buf=buf, ptr=buf.data_ptr(), nbytes=need)
        nat.attn_paged(self.qa, self.qa.stride(0), self.kpool, self.vpool, self.bt, self.ctx, self.cu, out, len(self.seqs),
                       H, Hkv, D, self.max_q, self.max_ctx, D ** -0.5, ns, ws)
        torch.cuda.synchronize()
        assert torch.isnan(outbuf[self.T:].float()).all(), "rows past the last token were written"
        if ws is not None:
            assert torch.isnan(ws.buf[need // 4:]).all(), "the workspace was written past attn_workspace_bytes"
            if probe is not None:
                probe(ws.buf)
        assert torch.isfinite(out.float()).all(), "non-finite output: an unwritten slot or record reached the result"
        return out.view(self.T, H, D).float().cpu()

    def check(self, got, want, what, long=False):
        """f16 2e-3 / bf16 1.6e-2 relative + absolute; over long contexts the max-abs bound 4e-3 / 2.5e-2."""
        f16 = self.dtype == F16
        if isinstance(want, list):
            want = torch.cat(want)
        err = (got - want).abs()
        if long:
            tol = 4e-3 if f16 else 2.5e-2
            assert float(err.max()) <= tol, f"{what}: max err {float(err.max()):.5f} > {tol}"
        else:
            tol = 2e-3 if f16 else 1.6e-2
            bad = err > tol + tol * want.abs()
            assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err "
                                   f"{float(err.max()):.4g} (want max {float(want.abs().max()):.4g})")


# ---- a. short prefill on the decode kernel ------------------------------------------------------------------------------
# q lengths include 1, 2, TQ = 16 / Gp, TQ + 1 and the largest 64 / Gp: one to four q tiles, pages partly visible to some
# columns of a tile.  Padded groups (Gc < Gp): G = 3, 5, 12; G = 48 is three one-chunk blocks per kv head.
SHORT = [
    ("g1-d128-f16", F16, 32, 32, 128, [1, 2, 16, 17, 64, 40]),
    ("g1-d96-bf16", BF16, 32, 32, 96, [64, 1, 2, 16, 17, 33]),
    ("g2-d64-bf16", BF16, 8, 4, 64, [1, 2, 8, 9, 32, 20]),
    ("g3pad-d96-f16", F16, 12, 4, 96, [1, 2, 4, 5, 16, 11]),
    ("g5pad-d128-bf16", BF16, 20, 4, 128, [1, 2, 3, 8, 5]),
    ("g8-d96-bf16", BF16, 32, 4, 96, [1, 2, 3, 8, 7]),
    ("g8-d128-f16", F16, 64, 8, 128, [8, 3, 2, 1]),
    ("g12pad-d64-f16", F16, 12, 1, 64, [1, 2, 3, 4]),
    ("g16-d128-f16", F16, 16, 1, 128, [1, 2, 3, 4]),
    ("g48-3chunks-d128-bf16", BF16, 48, 1, 128, [1, 2, 3, 4]),
    ("g48-3chunks-d64-f16", F16, 48, 1, 64, [4, 1, 3, 2]),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens", SHORT, ids=[c[0] for c in SHORT])
def test_short_prefill_on_the_decode_kernel(gpu_device, name, dtype, H, Hkv, D, lens):
    c = _Case(gpu_device, dtype, H, Hkv, D, [(l, l) for l in lens], seed=H * D + len(lens))
    assert _form(H, Hkv, c.max_q, 1) == "decode q>1"
    c.check(c.run(1), c.want(), name)


# the same shape on both sides of max_q_len * Gp == 64
BOUNDARY = [
    ("g1-d128-f16", F16, 32, 32, 128, [33, 1], 64),
    ("g1-d128-bf16", BF16, 32, 32, 128, [33, 1], 64),
    ("g3pad-d64-f16", F16, 12, 4, 64, [5, 1], 16),
    ("g8-d128-bf16", BF16, 32, 4, 128, [3, 1], 8),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens,qmax", BOUNDARY, ids=[c[0] for c in BOUNDARY])
def test_short_prefill_at_the_kernel_boundary(gpu_device, name, dtype, H, Hkv, D, lens, qmax):
    for ql, form in ((qmax, "decode q>1"), (qmax + 1, "prefill")):
        c = _Case(gpu_device, dtype, H, Hkv, D, [(l, l) for l in [ql] + lens], seed=ql * H + D)
        assert _form(H, Hkv, c.max_q, 1) == form
        c.check(c.run(1), c.want(), f"{name} max_q_len {ql} ({form})")


# ---- b. multi-tile prefill kernel ---------------------------------------------------------------------------------------
TILE_EDGES = [1, 127, 128, 129, 255, 256, 257, 700]  # MHA: 128-token tiles
PREFILL = [
    ("mha-d128-f16", F16, 16, 16, 128, TILE_EDGES),
    ("mha-d128-bf16", BF16, 16, 16, 128, TILE_EDGES),
    ("mha-d96-bf16", BF16, 16, 16, 96, TILE_EDGES),
    ("mha-d64-f16", F16, 16, 16, 64, TILE_EDGES),
    ("gqa4-32tok-tiles-d128-bf16", BF16, 32, 8, 128, [31, 32, 33, 63, 64, 65, 97, 250]),
    ("gqa8-16tok-tiles-d64-f16", F16, 32, 4, 64, [17, 40, 100, 16, 9]),  # tiles start half-way through a page
    ("g3pad-d96-f16", F16, 12, 4, 96, [100, 33, 5]),
    ("g5pad-d128-bf16", BF16, 20, 4, 128, [77, 9, 40]),
    ("mqa48-d128-f16", F16, 48, 1, 128, [300, 77]),
    ("mqa48-d128-bf16", BF16, 48, 1, 128, [129, 250]),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens", PREFILL, ids=[c[0] for c in PREFILL])
def test_multi_tile_prefill_kernel(gpu_device, name, dtype, H, Hkv, D, lens):
    c = _Case(gpu_device, dtype, H, Hkv, D, [(l, l) for l in lens], seed=H + Hkv + D)
    assert _form(H, Hkv, c.max_q, 1) == "prefill"
    c.check(c.run(1), c.want(), name)


# ---- c / d. decode at more than 8 key splits, and splits a sequence does not reach ----------------------------------------
def _merge_probe(total_q, ns, D, fused):
    """H 8 / Hkv 1 decode: where the two-launch layout keeps the {m, l} of (token 0, head 0, split 0) — float total_q * H * NS
    * D of the workspace — the fused layout has the record of column 8 (token 1 of the tile: never written at q_len 1).  So
    that float is still NaN after an in-launch merge and finite after a combine launch."""
    idx = total_q * 8 * ns * D

    def probe(buf):
        v = float(buf[idx])
        assert math.isnan(v) if fused else math.isfinite(v), \
            f"expected the {'in-launch merge' if fused else 'combine launch'} (workspace float {idx} = {v})"
    return probe


# (name, dtype, H, Hkv, D, ctx lens, splits, whether `splits` is what attn_num_splits returns for the shape)
SPLITS = [
    ("g8-fused-ctx8192-ns16", F16, 8, 1, 128, [8192], 16, True),
    ("g8-fused-ctx32768-ns64", F16, 8, 1, 128, [32768], 64, True),
    ("g8x8kv-fused-ctx8192-ns16", F16, 64, 8, 128, [8192], 16, True),
    ("g8-fused-explicit-ns9", F16, 8, 1, 128, [8192], 9, False),
    ("g8-fused-explicit-ns13", BF16, 8, 1, 64, [8192], 13, False),
    ("g8-fused-explicit-ns33", F16, 8, 1, 96, [8192], 33, False),  # 8 pages per split: split 32 is empty
    ("mqa48-combine-b1-ctx8192-ns16", BF16, 48, 1, 128, [8192], 16, True),
    ("mqa48-combine-b2-ctx8192-ns16", F16, 48, 1, 128, [8192, 8170], 16, True),
    ("mqa48-combine-b1-ctx16384-ns32", F16, 48, 1, 128, [16384], 32, True),
    ("mqa48-combine-b2-ctx16384-ns32", BF16, 48, 1, 128, [16384, 16001], 32, True),
    ("mqa48-combine-explicit-ns9", F16, 48, 1, 128, [8192], 9, False),
    ("mqa48-combine-explicit-ns13", BF16, 48, 1, 64, [8192], 13, False),
    ("mqa48-combine-explicit-ns33", F16, 48, 1, 96, [8192], 33, False),
    # d. one batch with sequences that end before most splits begin (their records: m = NEG_BIG, l = 0)
    ("unreached-g8-fused-ns8", F16, 8, 1, 128, [1, 31, 33, 4000, 8191], 8, False),
    ("unreached-g8-fused-ns16", BF16, 8, 1, 128, [1, 31, 33, 4000, 8191], 16, False),
    ("unreached-mqa48-combine-ns8", BF16, 48, 1, 128, [1, 31, 33, 4000, 8191], 8, False),
    ("unreached-mqa48-combine-ns16", F16, 48, 1, 128, [1, 31, 33, 4000, 8191], 16, False),
]
SINGLE_CHUNK_SPLITS = [s for s in SPLITS if s[2] // s[3] <= 16]


def _split_case(dev, name, dtype, H, Hkv, D, lens, ns, by_rule, fused):
    nat = _nat()
    if by_rule:
        assert nat.attn_num_splits(len(lens), Hkv, H, 1, max(lens)) == ns, "the split rule changed: re-choose this case"
    assert _form(H, Hkv, 1, ns, fused) == ("fused merge" if "fused" in name and fused else "combine")
    c = _Case(dev, dtype, H, Hkv, D, [(1, l) for l in lens], seed=H + D + ns + len(lens))
    got = c.run(ns, probe=_merge_probe(c.T, ns, D, fused) if (H, Hkv) == (8, 1) else None)
    c.check(got, c.want(), f"{name}: {ns} splits against the oracle", long=True)
    c.check(got, c.run(1), f"{name}: {ns} splits against one", long=True)


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens,ns,by_rule", SPLITS, ids=[s[0] for s in SPLITS])
def test_split_decode(gpu_device, name, dtype, H, Hkv, D, lens, ns, by_rule):
    _split_case(gpu_device, name, dtype, H, Hkv, D, lens, ns, by_rule, fused=True)


# ---- c2. one-token launches on the variants no case above reaches -------------------------------------------------------
# One case per variant key (tests/attn_cases.py) that tests/test_attn_plan_cpu.py found without a GPU case, at the smallest
# shape that reaches it, at the split count the rule gives it.  (name, dtype, H, Hkv, D, ctx lens) and the key it must land on.
DECODE = [
    # 32 sequences x 32 kv heads = 1024 blocks: 2-wave blocks, 1 - 3 pages dealt over two waves (one wave idle at one page)
    ("mha-1024-blocks-2waves-d64-f16", F16, 32, 32, 64, [1, 31, 32, 33, 63, 64, 65, 70] + [33 + (5 * i) % 38 for i in range(24)]),
    # G = 64 as two blocks of 3 + 1 chunks per kv head, 8 (sequence, kv head) groups: the chunk blocks of a group share an XCD
    ("mqa64-xcd-unsplit-d128-bf16", BF16, 128, 2, 128, [1, 33, 100, 257]),
    ("mqa64-xcd-combine8-ns2-d96-f16", F16, 128, 2, 96, [1000, 700]),
    # G = 80: 3 + 2 chunks, the second block's third chunk is past the group
    ("mqa80-xcd-combine-ns16-d64-bf16", BF16, 80, 1, 64, [8192]),
]
DECODE_VARIANTS = {
    "mha-1024-blocks-2waves-d64-f16": "form=decode,nw=2,ch=1,pipe=0,xcd_remap=0,merge=none",
    "mqa64-xcd-unsplit-d128-bf16": "form=decode,nw=4,ch=3,pipe=1,xcd_remap=1,merge=none",
    "mqa64-xcd-combine8-ns2-d96-f16": "form=decode,nw=4,ch=3,pipe=1,xcd_remap=1,merge=combine8",
    "mqa80-xcd-combine-ns16-d64-bf16": "form=decode,nw=4,ch=3,pipe=1,xcd_remap=1,merge=combine",
}


@pytest.mark.parametrize("name,dtype,H,Hkv,D,lens", DECODE, ids=[c[0] for c in DECODE])
def test_decode_variant(gpu_device, name, dtype, H, Hkv, D, lens):
    nat = _nat()
    ns = nat.attn_num_splits(len(lens), Hkv, H, 1, max(lens))
    key = attn_cases.key_str(attn_cases.case_key(nat.load_library(), H, Hkv, D, [(1, l) for l in lens], ns))
    assert key == DECODE_VARIANTS[name], f"the plan changed ({key}): re-choose this case"
    c = _Case(gpu_device, dtype, H, Hkv, D, [(1, l) for l in lens], seed=H + D + len(lens))
    got = c.run(ns)
    c.check(got, c.want(), f"{name}: {ns} split(s) against the oracle", long=ns > 1)
    if ns > 1:
        c.check(got, c.run(1), f"{name}: {ns} splits against one", long=True)


# ---- e. the two-launch combine for single-chunk groups ----------------------------------------------------------------
def test_two_launch_combine_for_single_chunk_groups():
    """TGIS_ATTN_FUSED_COMBINE is read once per process: the single-chunk cases above run again in one fresh child with it
    set to 0 — the production fallback when no arrival counters are free (a fifth concurrent stream, a capture before any
    eager call) — through attn_combine_kernel<MAXS = 8> (NS <= 8) and <MAXS = 0> (NS > 8)."""
    env = {**os.environ, "TGIS_ATTN_FUSED_COMBINE": "0"}
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)  # (inside pytest's 300 s)
    assert p.returncode == 0, f"child exit {p.returncode}\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
    assert f"{len(SINGLE_CHUNK_SPLITS)} passed" in p.stdout, p.stdout[-4000:]


# ---- f. q rows are the last q_len of ctx positions ------------------------------------------------------------------------
CONTRACT = [
    ("decode-kernel-mha", F16, 32, 32, 128, [(5, 100), (17, 300), (1, 1), (64, 64)]),
    ("prefill-kernel-mha", BF16, 16, 16, 128, [(200, 1000), (1, 50), (129, 129)]),
    ("prefill-kernel-gqa8", F16, 32, 4, 128, [(200, 1000), (200, 1013), (3, 40)]),
]


@pytest.mark.parametrize("name,dtype,H,Hkv,D,seqs", CONTRACT, ids=[c[0] for c in CONTRACT])
def test_new_tokens_over_a_longer_context(gpu_device, name, dtype, H, Hkv, D, seqs):
    c = _Case(gpu_device, dtype, H, Hkv, D, seqs, seed=7 * H + D)
    assert _form(H, Hkv, c.max_q, 1) == ("decode q>1" if name.startswith("decode") else "prefill")
    c.check(c.run(1), c.want(), name)


if __name__ == "__main__":
    assert os.environ.get("TGIS_ATTN_FUSED_COMBINE") == "0"
    dev = torch.device("cuda:0")
    passed = 0
    for case in SINGLE_CHUNK_SPLITS:
        try:
            _split_case(dev, *case, fused=False)
        except AssertionError as e:
            print(f"FAILED {case[0]} (two-launch combine): {e}", flush=True)
            sys.exit(1)
        print(f"ok {case[0]} (two-launch combine)", flush=True)
        passed += 1
    print(f"{passed} passed", flush=True)
