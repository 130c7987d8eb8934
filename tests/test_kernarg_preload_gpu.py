"""-m gpu: the decode kernels whose leading arguments are preloaded into SGPRs at wave launch (csrc/gptq_wide_body.h
wide_args, csrc/attention.hip attn_paged_kernel) and the launches between them in a decode step (add + RMSNorm, lm_head,
greedy), each against oracle/ops_ref.py with the bars the op tests use (tests/test_ops_gpu.py, tests/test_fragments_gpu.py),
at the smallest shapes that reach its branches.

A preloaded argument that the kernel and its launcher disagree about (order, width, a field that the block behind it still
overrules) shows as a wrong address or a wrong count: every case below reads each preloaded field in a way that changes the
result — tiles past the matrix (NT), fewer k-steps than waves (K), split and unsplit plans (S), both row classes (M), one
and several groups (G, spg_shift), key splits and GQA (NS, Hkv, HCB, max_pages).
The fragment-order GEMM's plan (CT, S) is the library's own, and — through its tuning hook TGIS_GPTQ_WIDE_PLAN — every plan
a shape admits that puts a tile past the matrix or splits k."""
import numpy as np
import pytest
import torch

from oracle import ops_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat(gpu_device):
    from tgis_amd import native

    native.load_library()
    return native


def _close(got, want, rtol, atol, what=""):
    got = got.float().cpu()
    want = want.float().cpu()
    err = (got - want).abs()
    bad = err > atol + rtol * want.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {err.max():.4g} " \
                          f"(want max {want.abs().max():.4g})"


def _weight(nat, dev, K, N, gs, seed, **kw):
    """The oracle's tensors and a factory of prepared weights: every plan under test gets a fresh GptqWeight, whose cached
    split plan and workspace size are then that plan's."""
    qw, qz, sc, gi = ops_ref.make_gptq_tensors(K, N, gs, seed=seed)
    t = [torch.from_numpy(a).to(dev) for a in (qw, qz, sc)]
    return (qw, qz, sc, gi), lambda: nat.GptqWeight(t[0], t[1], t[2], None, 4, gs, **kw)


def _set_plan(monkeypatch, plan):
    if plan is None:
        monkeypatch.delenv("TGIS_GPTQ_WIDE_PLAN", raising=False)
    else:
        monkeypatch.setenv("TGIS_GPTQ_WIDE_PLAN", plan)


def _frag(nat, x, M):
    """x in fragment order; the rows past M of the last row block are NaN: they must not matter."""
    xf = nat.FragAct.from_rows(x)
    if M % 32:
        xf.buf.view((M + 31) // 32, -1, 2, 32, 8)[-1][:, :, M % 32:].fill_(float("nan"))
    return xf


ROWS = (1, 32, 33, 64)
# K 64: one k64-step, seven of a block's eight waves have none; one group.  K 512: eight steps, one per wave; gs 128: four
# groups of two steps (spg_shift 1), gs 512: one group.
K_GS = ((64, 64), (512, 128), (512, 512))


def _plans(K, split):
    """TGIS_GPTQ_WIDE_PLAN values: the library's own plan, tiles past the matrix at every CT, and (act 0) two k splits where
    a split still holds a k64-step per wave-share (K 512: four steps per split)."""
    plans = [None, "2,1", "3,1", "4,1"]
    if split and K >= 512:
        plans += ["2,2", "1,2"]
    return plans


@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("K,gs", K_GS)
def test_fragment_gemm_plain(nat, gpu_device, monkeypatch, K, gs, N):
    """act 0: the f16 result (unsplit, or split + reduce launch) and the deferred form (fp32 slabs) against the oracle."""
    (qw, qz, sc, gi), make = _weight(nat, gpu_device, K, N, gs, seed=K + N + gs)
    for M in ROWS:
        g = torch.Generator().manual_seed(M * 11 + K)
        x = (torch.randn(M, K, generator=g) * 0.5).half()
        bias = (torch.randn(N, generator=g) * 0.1).half()
        want = ops_ref.gptq_linear(x, qw, qz, sc, gi, gs, bias)
        tol = dict(rtol=2e-3, atol=2e-3 * float(want.abs().mean()) + 1e-4)
        for plan in _plans(K, split=True):
            _set_plan(monkeypatch, plan)
            w = make()
            ws = nat.Workspace(w.workspace_bytes(M), gpu_device)
            xf = _frag(nat, x.to(gpu_device), M)
            got = nat.gptq_gemm(xf, w, ws, bias=bias.to(gpu_device))
            _close(got, want, what=f"M {M} plan {plan}", **tol)
            p = nat.gptq_gemm_partial(xf, w, bias=bias.to(gpu_device))
            if plan is not None:
                assert p.S == int(plan.split(",")[1]), "the hooked plan did not reach the launch"
            rb = (M + 31) // 32
            sl = p.slabs[:rb * p.S * 32 * p.ld].view(rb, p.S, 32, p.ld).sum(1).reshape(rb * 32, p.ld)[:M, :N]
            _close((sl + bias.to(gpu_device).float()).half(), want, what=f"slabs, M {M} plan {plan}", **tol)


@pytest.mark.parametrize("N", [32, 96, 128])
@pytest.mark.parametrize("K,gs", K_GS)
def test_fragment_gemm_silu_epilogue(nat, gpu_device, monkeypatch, K, gs, N):
    """act 2 on the interleaved gate / up image, row-major output and (N / 2 a multiple of 64) fragment-order output."""
    I = N // 2
    (qw, qz, sc, gi), make = _weight(nat, gpu_device, K, N, gs, seed=K + N + 2, gate_up=True)
    for M in ROWS:
        g = torch.Generator().manual_seed(M * 13 + K)
        x = (torch.randn(M, K, generator=g) * 0.5).half()
        lin = ops_ref.gptq_linear(x, qw, qz, sc, gi, gs, None)
        want = ops_ref.silu_mul(lin.half().view(M, N), I)
        scale = float(want.abs().max())
        for plan in _plans(K, split=False):
            _set_plan(monkeypatch, plan)
            w = make()
            ws = nat.Workspace(w.workspace_bytes(M), gpu_device)
            xf = _frag(nat, x.to(gpu_device), M)
            a_row = nat.gptq_gemm(xf, w, ws, act=2)
            assert float((a_row.float().cpu() - want.float()).abs().max()) <= 6e-3 * scale, f"M {M} plan {plan}"
            if I % 64 == 0:
                a_frag = nat.gptq_gemm(xf, w, ws, act=2, out_frag=True)
                assert torch.equal(a_frag.to_rows(), a_row), f"fragment-order output, M {M} plan {plan}"


@pytest.mark.parametrize("K,gs", K_GS)
def test_fragment_gemm_rope_epilogue(nat, gpu_device, monkeypatch, K, gs):
    """act 3 at N = 96: one q, one k and one v head of 32 (one tile each); q and the cache pages against the oracle's rotary
    embedding of the oracle's linear."""
    H, Hkv, D = 1, 1, 32
    N = (H + 2 * Hkv) * D
    (qw, qz, sc, gi), make = _weight(nat, gpu_device, K, N, gs, seed=K + 3, rope=(D, H + Hkv))
    cos, sin = ops_ref.rope_tables(D, 10000.0, 80, torch.float16)
    for M in ROWS:
        g = torch.Generator().manual_seed(M * 17 + K)
        x = (torch.randn(M, K, generator=g) * 0.5).half()
        bv = (torch.randn(N, generator=g) * 0.1).half()
        pos = torch.randint(0, 80, (M,), generator=g).int()
        slots = torch.randperm(8 * 32, generator=g)[:M].int()
        lin = ops_ref.gptq_linear(x, qw, qz, sc, gi, gs, bv)
        scale = float(lin.abs().max())
        eps = 2.0 ** -11
        qkv_ref = lin.half()
        want_q = ops_ref.apply_rope(qkv_ref[:, :H * D].view(M, H, D), cos[pos.long()], sin[pos.long()])
        want_k = ops_ref.apply_rope(qkv_ref[:, H * D:(H + Hkv) * D].view(M, Hkv, D), cos[pos.long()], sin[pos.long()])
        for plan in _plans(K, split=False):
            _set_plan(monkeypatch, plan)
            wr = make()
            kp = torch.zeros((8, Hkv, 32 * D), dtype=torch.float16, device=gpu_device)
            vp = torch.zeros_like(kp)
            q1 = nat.gptq_gemm_rope(_frag(nat, x.to(gpu_device), M), wr, bv.to(gpu_device), cos.to(gpu_device),
                                    sin.to(gpu_device), pos.to(gpu_device), slots.to(gpu_device), kp, vp, H, Hkv, D)
            what = f"M {M} plan {plan}"
            _close(q1[:, :H * D].view(M, H, D), want_q, rtol=4e-3, atol=6 * eps * scale, what="rope q, " + what)
            kc, vc = kp.cpu(), vp.cpu()
            used = torch.zeros(8 * 32, dtype=torch.bool)
            for b in range(M):
                s_ = int(slots[b])
                used[s_] = True
                Kp, Vp = ops_ref.kv_page_unpack(kc, vc, s_ >> 5, Hkv, D)
                _close(Kp[s_ & 31], want_k[b], rtol=4e-3, atol=6 * eps * scale, what="rope k page, " + what)
                _close(Vp[s_ & 31], qkv_ref[b, (H + Hkv) * D:].view(Hkv, D), rtol=4e-3, atol=6 * eps * scale,
                       what="v page, " + what)
            for page in range(8):  # slots no row owns stay zero
                Kp, Vp = ops_ref.kv_page_unpack(kc, vc, page, Hkv, D)
                free = ~used[page * 32:(page + 1) * 32]
                assert not Kp[free].any() and not Vp[free].any(), "a cache slot no row owns was written, " + what


@pytest.mark.parametrize("S", [0, 1, 4])
@pytest.mark.parametrize("hidden", [64, 4096])
@pytest.mark.parametrize("rows", [1, 33])
def test_add_rmsnorm(nat, gpu_device, rows, hidden, S):
    """S = 0: x is a tensor; S >= 1: x arrives as S fp32 slabs (+ the bias of the GEMM before).  Row-major and fragment-order
    y hold the same bits; y against the oracle, the residual stream bit-exact.  (Slab values are multiples of 2^-6 below 1:
    their fp32 sum is exact in any order, so the oracle's x is the kernel's x.)"""
    g = torch.Generator().manual_seed(rows + hidden + S)
    res = torch.randn(rows, hidden, generator=g).half()
    wn = (1 + 0.1 * torch.randn(hidden, generator=g)).half()
    if S:
        ld = hidden + 32  # a row stride past the row: slab_ld is not hidden
        slabs = torch.randint(-63, 64, ((rows + 31) // 32, S, 32, ld), generator=g).float() / 64
        xb = (torch.randint(-8, 9, (hidden,), generator=g).float() / 64).half()
        x = (slabs.sum(1).reshape(-1, ld)[:rows, :hidden] + xb.float()).half()
        sd = slabs.to(gpu_device).reshape(-1)
        src = lambda: nat.Partial(sd, S, ld, rows, hidden, xb.to(gpu_device))  # noqa: E731
    else:
        x = torch.randn(rows, hidden, generator=g).half()
        xd = x.to(gpu_device)
        src = lambda: xd  # noqa: E731
    wy, wres = ops_ref.rmsnorm_residual(x, res, wn, 1e-5)
    y0, r0 = nat.rmsnorm_residual(src(), res.to(gpu_device), wn.to(gpu_device), 1e-5)
    y1, r1 = nat.rmsnorm_residual(src(), res.to(gpu_device), wn.to(gpu_device), 1e-5, frag=True)
    _close(y0, wy, rtol=1e-3, atol=1e-3, what="rmsnorm y")
    assert torch.equal(r0.cpu(), wres.half()), "residual stream must be the rounded fp32 sum, bit-exact"
    assert isinstance(y1, nat.FragAct) and torch.equal(y1.to_rows(), y0) and torch.equal(r0, r1)


@pytest.mark.parametrize("ns", [1, 2, 3])
@pytest.mark.parametrize("ctx", [1, 31, 33, 65])
@pytest.mark.parametrize("B", [1, 3])
def test_decode_attention_gqa(nat, gpu_device, B, ctx, ns):
    """GQA 4:1 decode over a shuffled block table: one and several key splits (a split past a short sequence's pages has
    nothing to do), sequences that end in, at and just behind a page; row-major and fragment-order output."""
    H, Hkv, D = 8, 2, 128
    lens = [ctx, 1 + (ctx * 7) % 65, 65 - (ctx % 2)][:B]
    g = torch.Generator().manual_seed(B * 100 + ctx)
    pages_per = [(l + 31) // 32 for l in lens]
    total_pages = sum(pages_per) + 3
    bt = torch.zeros((B, max(pages_per) + 1), dtype=torch.int32)  # a table wider than any sequence: max_pages is its stride
    perm = torch.randperm(total_pages, generator=g)
    kpool = torch.zeros((total_pages, Hkv, 32 * D), dtype=torch.float16)
    vpool = torch.zeros_like(kpool)
    ks, vs, o = [], [], 0
    for b, l in enumerate(lens):
        bt[b, :pages_per[b]] = perm[o:o + pages_per[b]].int()
        o += pages_per[b]
        k = torch.randn(l, Hkv, D, generator=g).half()
        v = torch.randn(l, Hkv, D, generator=g).half()
        for p in range(pages_per[b]):
            ops_ref.kv_page_pack(kpool, vpool, int(bt[b, p]), k[p * 32:(p + 1) * 32], v[p * 32:(p + 1) * 32])
        ks.append(k)
        vs.append(v)
    q = torch.randn(B, H * D, generator=g).half()
    cuk = [0] + list(np.cumsum(lens))
    want = ops_ref.attention_varlen(q.view(B, H, D), torch.cat(ks), torch.cat(vs), torch.arange(B + 1), cuk, D ** -0.5)
    ws = nat.Workspace(nat.attn_workspace_bytes(B, H, Hkv, D, ns), gpu_device) if ns > 1 else None
    args = (kpool.to(gpu_device), vpool.to(gpu_device), bt.to(gpu_device),
            torch.tensor(lens, dtype=torch.int32, device=gpu_device), torch.arange(B + 1, dtype=torch.int32, device=gpu_device))
    out = torch.empty((B, H * D), dtype=torch.float16, device=gpu_device)
    nat.attn_paged(q.to(gpu_device), H * D, *args, out, B, H, Hkv, D, 1, max(lens), D ** -0.5, ns, ws)
    _close(out.view(B, H, D), want, rtol=2e-3, atol=2e-3, what=f"decode attention, lens {lens}, {ns} splits")
    of = nat.FragAct.empty(B, H * D, gpu_device)
    nat.attn_paged(q.to(gpu_device), H * D, *args, of, B, H, Hkv, D, 1, max(lens), D ** -0.5, ns, ws)
    assert torch.equal(of.to_rows(), out), "fragment-order output"


@pytest.mark.parametrize("M", [1, 32])
def test_lm_head_and_greedy_at_a_small_vocabulary(nat, gpu_device, M):
    """The last launches of a decode step at V = 512: hidden -> fp32 logits (dense GEMM), then ids + logprobs in one launch
    and split over workgroups (two launches)."""
    K, V = 256, 512
    g = torch.Generator().manual_seed(M + V)
    x = (torch.randn(M, K, generator=g) * 0.5).half()
    w = (torch.randn(V, K, generator=g) * 0.05).half()
    want = x.float() @ w.float().t()
    dw = nat.DenseWeight(w.to(gpu_device))
    ws = nat.Workspace(dw.workspace_bytes(M), gpu_device)
    logits = nat.dense_gemm(x.to(gpu_device), dw, ws, out_f32=True)
    eps = 1e-5
    _close(logits, want, rtol=2 * eps, atol=2 * eps * float(want.abs().mean()) + 1e-5, what="lm_head logits")
    lg = logits.clone()
    r = M // 2
    lg[r, V - 1] = lg[r, 3] = lg[r].max() + 1  # a tie between the first and the last segment: the lowest index wins
    ids0, lp0 = nat.argmax_logprob(lg)
    ids1, lp1 = nat.argmax_logprob(lg, scratch=nat.argmax_scratch(M, gpu_device))
    wi, wl = ops_ref.greedy(lg.cpu())
    assert torch.equal(ids0.cpu(), wi) and torch.equal(ids1, ids0) and int(ids0[r]) == 3
    _close(lp0, wl, rtol=1e-5, atol=1e-5, what="logprob")
    _close(lp1, wl, rtol=1e-5, atol=1e-5, what="logprob (split rows)")
